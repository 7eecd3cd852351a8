// rt_query_walk.h -- the per-ray walk of a LEAN program (BOX / SPHERE / END records, flat_scene.h) for the ray queries of
// include/rtiow_gpu_query.h: the closest walk with the shrinking `best` (hit_top, rt_trace.h) and the any-hit walk with the
// fixed t_max and an early exit (occluded, rt_light.h), one record per step.  The arithmetic is theirs exactly: 1 / d formed
// once per ray by a correctly rounded divide, aabb.rs's order in the box test, Sphere::hit in the one-division form of
// rt_sphere_hit.h (the reference's bits, proved there) with a = dot(d, d) formed once per ray.
// No HIP in here: the header compiles for the device (rt_query.h: the records are the workgroup's LDS copy) and for the host
// (tests/test_query_walk_host.py builds a g++ program that compares both walks with the oracle's hit_top).  V is any struct
// with float members x, y, z; R any struct with uint32_t members x, y, z, w (uint4 on the device).
// Compile with -ffp-contract=off, like everything that restates the reference's arithmetic.
#pragma once
#include <stdint.h>

#include "flat_scene.h"
#include "rt_sphere_hit.h"

namespace rtg {

constexpr float QUERY_F32_MAX = 3.402823466e+38f;
constexpr uint32_t QUERY_NO_HIT = 0xffffffffu;

RT_HD float query_u2f(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, sizeof f);
  return f;
}

// What a walk keeps of its ray: origin, direction, 1 / direction (aabb.rs:17), a = dot(d, d), the range start.
template <class V>
struct QueryRay {
  V o, d, inv;
  float a, t_min;
  bool t_min_pos;  // t_min > 0: the same for every ray of a call (rt_sphere_hit.h: claim 1 needs it)
};

template <class V>
RT_HD QueryRay<V> query_ray(float ox, float oy, float oz, float dx, float dy, float dz, float t_min) {
  QueryRay<V> r;
  r.o.x = ox, r.o.y = oy, r.o.z = oz;
  r.d.x = dx, r.d.y = dy, r.d.z = dz;
  r.inv.x = 1.f / dx, r.inv.y = 1.f / dy, r.inv.z = 1.f / dz;
  r.a = sphere_dot(r.d, r.d);
  r.t_min = t_min, r.t_min_pos = t_min > 0.f;
  return r;
}

// One record.  `end`: the far end of the range -- the closest hit so far (ANY = false: a hit shrinks it) or the ray's t_max
// (ANY = true: never written).  `hit_pc`: the record of the accepted hit.  Returns the record the walk goes on at: always > pc
// (a skip pointer that does not point forward is stepped over), and `n` -- the walk is over -- at END, at any record that is
// neither BOX nor SPHERE, and at the first accepted hit of an any-hit walk.
template <bool ANY, class V, class R>
RT_HD uint32_t query_step(const R& l, const R& h, uint32_t pc, uint32_t n, const QueryRay<V>& r, float& end, uint32_t& hit_pc) {
  const uint32_t op = h.w & 0xffu;
  if (op == OP_BOX) {  // Aabb::hit, aabb.rs:16-27: lo = (min.x, max.x, min.y, max.y), hi = (min.z, max.z, skip, flags)
    const float t0x = (query_u2f(l.x) - r.o.x) * r.inv.x, t1x = (query_u2f(l.y) - r.o.x) * r.inv.x;
    const float t0y = (query_u2f(l.z) - r.o.y) * r.inv.y, t1y = (query_u2f(l.w) - r.o.y) * r.inv.y;
    const float t0z = (query_u2f(h.x) - r.o.z) * r.inv.z, t1z = (query_u2f(h.y) - r.o.z) * r.inv.z;
    const float ax = r.inv.x < 0.f ? t1x : t0x, bx = r.inv.x < 0.f ? t0x : t1x;
    const float ay = r.inv.y < 0.f ? t1y : t0y, by = r.inv.y < 0.f ? t0y : t1y;
    const float az = r.inv.z < 0.f ? t1z : t0z, bz = r.inv.z < 0.f ? t0z : t1z;
    const float start = __builtin_fmaxf(r.t_min, __builtin_fmaxf(__builtin_fmaxf(ax, ay), az));
    const float stop = __builtin_fminf(end, __builtin_fminf(__builtin_fminf(bx, by), bz));
    if (stop > start) return pc + 1u;
    return h.z > pc ? h.z : pc + 1u;
  }
  if (op == OP_SPHERE) {  // Sphere::hit behind an optional Translate (object.rs:275-278): lo = (offset.xyz, radius)
    V q = r.o;
    if (h.w & F_TRANSLATE) q.x = r.o.x - query_u2f(l.x), q.y = r.o.y - query_u2f(l.y), q.z = r.o.z - query_u2f(l.z);
    float t;
    if (sphere_hit_t_a_1div(q, r.d, r.a, query_u2f(l.w), r.t_min, end, r.t_min_pos, t)) {
      hit_pc = pc;
      if (ANY) return n;
      end = t;
    }
    return pc + 1u;
  }
  return n;  // END
}

// The hit record of a closest walk from the record it ended on, as hit_top forms it at the hit (rt_trace.h): p = o' + t d,
// n = p / radius in the sphere's frame, then the Translate back and the flipped normal.  out8: (1, t, p.xyz, n.xyz).
template <class V, class R>
RT_HD uint32_t query_hit_record(const R& l, const R& h, const QueryRay<V>& r, float t, float* out8) {
  const bool tr = (h.w & F_TRANSLATE) != 0u;
  const float cx = query_u2f(l.x), cy = query_u2f(l.y), cz = query_u2f(l.z), radius = query_u2f(l.w);
  const float qx = tr ? r.o.x - cx : r.o.x, qy = tr ? r.o.y - cy : r.o.y, qz = tr ? r.o.z - cz : r.o.z;
  float px = qx + t * r.d.x, py = qy + t * r.d.y, pz = qz + t * r.d.z;  // ray.rs:15
  float nx = px / radius, ny = py / radius, nz = pz / radius;           // object.rs:104
  if (tr) px = px + cx, py = py + cy, pz = pz + cz;                     // object.rs:279-282
  if (h.w & F_FLIP) nx = -nx, ny = -ny, nz = -nz;                       // object.rs:249-252
  out8[0] = 1.f, out8[1] = t, out8[2] = px, out8[3] = py, out8[4] = pz, out8[5] = nx, out8[6] = ny, out8[7] = nz;
  return h.z;
}

// The two walks whole, one ray each (the host program; the device kernel runs query_step in a loop of its own, rt_query.h).
// Every step moves pc forward, so a walk takes at most n steps.
template <class V, class R>
RT_HD bool query_closest_walk(const R* lo, const R* hi, uint32_t n, const QueryRay<V>& r, float* out8, uint32_t* material) {
  float best = QUERY_F32_MAX;
  uint32_t hit_pc = QUERY_NO_HIT;
  for (uint32_t pc = 0; pc < n;) pc = query_step<false>(lo[pc], hi[pc], pc, n, r, best, hit_pc);
  if (hit_pc == QUERY_NO_HIT) {
    for (int k = 0; k < 8; k++) out8[k] = 0.f;
    *material = QUERY_NO_HIT;
    return false;
  }
  *material = query_hit_record(lo[hit_pc], hi[hit_pc], r, best, out8);
  return true;
}

template <class V, class R>
RT_HD bool query_occluded_walk(const R* lo, const R* hi, uint32_t n, const QueryRay<V>& r, float t_max) {
  if (!(t_max > r.t_min)) return false;
  uint32_t hit_pc = QUERY_NO_HIT;
  for (uint32_t pc = 0; pc < n;) pc = query_step<true>(lo[pc], hi[pc], pc, n, r, t_max, hit_pc);
  return hit_pc != QUERY_NO_HIT;
}

}  // namespace rtg
