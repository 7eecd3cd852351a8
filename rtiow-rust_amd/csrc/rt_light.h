// rt_light.h -- scene option light_sampling (include/rtiow_gpu.h, at rtg_scene_set_option): direct light sampling of the
// scene's rect lights at diffuse hits.  NOT the reference's estimator -- same expectation, other samples, other bits.
//   occluded()   the shadow ray's walk: bounded by t_max, returns at the first accepted hit
//   color_ls()   color() (rt_trace.h) with the light sample between emission and scatter
//   the one-lane-per-pixel kernels over color_ls (pixel mapping and ordered folds of rtg_kernels.inc)
// The light table is a kernel argument of these kernels alone: DevScene, a kernarg of every tuned kernel, stays as it is.
#pragma once
#include "rt_trace.h"

namespace rtg {

struct LightTable {
  const LightRect* lights;  // n records (flat_scene.h), world order
  const uint8_t* sampled;   // per material: 1 = every surface that emits with it is in `lights`
  uint32_t n;               // 1 .. RT_MAX_LIGHTS (a scene with an empty table renders on the plain kernels: rtg_launch.inc)
};

// Is anything hit in [t_near, t_max) along o + t d?  hit_top's predicates and visiting order without the hit record and without
// a shrinking range: the first accepted hit ends the walk.  A ConstantMedium takes part with its own free-path draw from `rng`
// (object.rs:562) -- the ray is blocked with probability 1 - transmittance, an unbiased estimate of the transmittance.
template <uint32_t FEAT, bool COUNT>
RT_DEV bool occluded(const DevScene& sc, V3 o, V3 d, float time, float t_near, float t_max, SampleRng& rng, Counts& cnt) {
  if (COUNT) cnt.rays++;
  if (FEAT & FEAT_DEEP) {  // graph shapes only the general walk handles
    float t;
    constexpr int XD = (FEAT & FEAT_DEEP_FEW_WRAPPERS) ? DEEP_FEW_WRAPPERS : MAX_DEEP_XFORM_DEPTH;
    constexpr int ML = (FEAT & FEAT_DEEP_ONE_LEVEL) ? 1 : MAX_MEDIUM_NESTING;
    return walk_deep<0, COUNT, XD, ML, true, (FEAT & FEAT_TRI) != 0u, (FEAT & FEAT_SURFACE) != 0u>(sc, 0u, sc.n_prog, o, d, time, t_near, t_max, rng, nullptr, t, cnt);
  }
  V3 inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
  int depth = 0;
  V3 so[MAX_XFORM_DEPTH], sd[MAX_XFORM_DEPTH];
  uint32_t pc = 0;
  for (;;) {
    const uint4 hi = sc.hi[pc];
    const uint32_t op = hi.w & 0xffu;
    if (op == OP_END) break;
    const uint4 lo = sc.lo[pc];
    if (op == OP_BOX) {  // Aabb::hit, aabb.rs:16-27
      if (COUNT) cnt.aabb++;
      float t0x = (u2f(lo.x) - o.x) * inv.x, t1x = (u2f(lo.y) - o.x) * inv.x;
      float t0y = (u2f(lo.z) - o.y) * inv.y, t1y = (u2f(lo.w) - o.y) * inv.y;
      float t0z = (u2f(hi.x) - o.z) * inv.z, t1z = (u2f(hi.y) - o.z) * inv.z;
      float ax = inv.x < 0.f ? t1x : t0x, bx = inv.x < 0.f ? t0x : t1x;
      float ay = inv.y < 0.f ? t1y : t0y, by = inv.y < 0.f ? t0y : t1y;
      float az = inv.z < 0.f ? t1z : t0z, bz = inv.z < 0.f ? t0z : t1z;
      float start = rs_max(t_near, rs_max(rs_max(ax, ay), az));
      float end = rs_min(t_max, rs_min(rs_min(bx, by), bz));
      pc = (end > start) ? pc + 1 : hi.z;
      continue;
    }
    if (op == OP_SPHERE) {
      if (COUNT) cnt.prim++;
      V3 lo_o = o;
      if (hi.w & F_TRANSLATE) lo_o = vsub(o, mk(u2f(lo.x), u2f(lo.y), u2f(lo.z)));
      if ((FEAT & FEAT_XFORM) && (hi.w & F_MOVE)) {  // fused LinearMove (flat_scene.h)
        const uint4 mv = sc.lo[++pc];
        lo_o = vsub(lo_o, smul(time, mk(u2f(mv.x), u2f(mv.y), u2f(mv.z))));
      }
      float t;
      if (sphere_hit_t(lo_o, d, u2f(lo.w), t_near, t_max, t)) return true;
      pc++;
      continue;
    }
    if ((FEAT & FEAT_RECT) && op == OP_RECT) {
      if (COUNT) cnt.prim++;
      float t;
      if (rect_hit_t(o, d, (hi.w >> F_AXIS_SHIFT) & 3u, u2f(lo.x), u2f(lo.y), u2f(lo.z), u2f(lo.w), u2f(hi.x), t_near, t_max, t)) return true;
      pc++;
      continue;
    }
    if ((FEAT & FEAT_RECT) && op == OP_PRISM) {
      if (COUNT) cnt.prim += 6;
      float t;
      uint32_t face = 0;
      if (prism_hit_t(lo, hi, o, d, t_near, t_max, t, face)) return true;
      pc++;
      continue;
    }
    if ((FEAT & FEAT_TRI) && op == OP_TRI) {
      if (COUNT) cnt.prim++;
      float t;
      if (tri_rec_hit_t(lo, hi, sc.lo[pc + 1], o, d, t_near, t_max, t)) return true;
      pc += (FEAT & FEAT_SURFACE) ? tri_rec_step(hi) : 2u;  // (its data record; an attribute triangle's three)
      continue;
    }
    if ((FEAT & FEAT_XFORM) && op == OP_PUSH) {
      uint32_t kind = (hi.w >> F_KIND_SHIFT) & 7u;
      so[depth] = o, sd[depth] = d;
      depth++;
      V3 a = mk(u2f(lo.x), u2f(lo.y), u2f(lo.z));
      if (hi.w & F_PRE_TRANSLATE) o = vsub(o, mk(u2f(lo.w), u2f(hi.x), u2f(hi.y)));
      if (kind == XF_TRANSLATE) {
        o = vsub(o, a);
      } else if (kind == XF_ROTATE_Y) {
        o = rot_y(o, -a.x, a.y), d = rot_y(d, -a.x, a.y);
        inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
      } else if (kind == XF_SCALE) {
        o = vdiv(o, a), d = vdiv(d, a);
        inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
      } else if (kind == XF_MOVE) {
        o = vsub(o, smul(time, a));
      }
      pc++;
      continue;
    }
    if ((FEAT & FEAT_XFORM) && op == OP_POP) {
      uint32_t kind = (hi.w >> F_KIND_SHIFT) & 7u;
      depth--;
      o = so[depth], d = sd[depth];
      if (kind == XF_ROTATE_Y || kind == XF_SCALE) inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
      pc++;
      continue;
    }
    if ((FEAT & FEAT_MEDIUM) && op == OP_MEDIUM) {  // ConstantMedium::hit, object.rs:545-575, over [t_near, t_max)
      float t1, t2;
      bool h1, h2 = false;
      if (hi.w & F_GENERAL_BOUNDARY) {
        const BoundaryHit b1 = boundary_hit_t<(FEAT & FEAT_TRI) != 0u, (FEAT & FEAT_SURFACE) != 0u>(sc.lo, sc.hi, pc + 1, hi.x, o, d, time, -F32_MAX, F32_MAX);
        h1 = b1.any != 0u, t1 = b1.t;
        if (COUNT) cnt.aabb += b1.n_aabb, cnt.prim += b1.n_prim;
        if (h1) {
          const BoundaryHit b2 = boundary_hit_t<(FEAT & FEAT_TRI) != 0u, (FEAT & FEAT_SURFACE) != 0u>(sc.lo, sc.hi, pc + 1, hi.x, o, d, time, t1 + 0.0001f, F32_MAX);
          h2 = b2.any != 0u, t2 = b2.t;
          if (COUNT) cnt.aabb += b2.n_aabb, cnt.prim += b2.n_prim;
        }
      } else {
        uint32_t n_tests;
        h1 = h2 = boundary_pair_t(sc.lo[pc + 1], sc.hi[pc + 1], o, d, t1, t2, n_tests);
        if (COUNT) cnt.prim += n_tests;
      }
      if (h1 && h2) {
        t1 = rs_max(t1, t_near);
        t2 = rs_min(t2, t_max);
        if (!(t1 >= t2)) {
          float distance_inside = (t2 - t1) * vlen(d);
          float hit_distance = -(1.f / u2f(lo.x)) * rt_logf(rng.gen_f32());
          if (hit_distance < distance_inside) return true;
        }
      }
      pc = hi.x;  // first record after the boundary's stream
      continue;
    }
    pc++;  // OP_SEG: stepped over, its primitives executed (flat_scene.h)
  }
  return false;
}

// color() (rt_trace.h; lib.rs:60-101) with direct light sampling.  At a hit (p, n, material), `bounces` the running count:
//   1. emission, as color() -- except at a SAMPLED light reached by the ray scattered at a hit that took a light sample: that
//      light was counted there.  Camera rays and rays leaving Metal, Dielectric or the capped hit collect it as always.
//   2. at a Lambertian or Isotropic hit with bounces < max_bounces (the hit at which the cap ends the path scatters no ray a
//      light could be found with, so it samples none): three gen_f32 draws -- the light i = min(N - 1, floor(u0 N)), the point
//      q of its rect from (u1, u2) -- then w = q - p, r2 = w.w, cos_l = |w[axis]| / sqrt(r2) (DiffuseLight emits from both
//      faces) and the density `lobe` of the material's scattered direction along w:
//        Lambertian scatters towards p + n + in_unit_sphere(), a point of the unit BALL around p + n (material.rs:57-65): with
//        b = n.w / sqrt(r2) and disc = b^2 - (n.n - 1) the ray along w is inside that ball for r in (max(b - sqrt(disc), 0),
//        b + sqrt(disc)), and the density is the ball's share of it, (r_hi^3 - r_lo^3) / (4 pi) -- 2 cos^3 / pi for |n| = 1, not
//        the cos / pi of a cosine lobe; valid for any |n| (Scale leaves normals unnormalised).  Isotropic: 1 / (4 pi).
//      When lobe, r2 and cos_l are positive a shadow ray runs from p along w, unnormalised: the light sits at t = 1 and the ray
//      is occluded by anything in [t_near, 1 - 1e-3) (the last 1e-3 of the segment is not tested: the accepted bias, the light
//      itself and whatever touches it).  Unoccluded: accum += strength * albedo(p) * Le(q) * lobe * N * area_i * cos_l / r2.
//   3. scatter, as color().
// A miss returns accum (+ the background): without the option accum is always +0 there, so lib.rs:100 drops nothing.
template <uint32_t FEAT, bool COUNT>
RT_DEV V3 color_ls(const DevScene& sc, const LightTable& lt, V3 o, V3 d, float time, const DevParams& P, SampleRng& rng, Counts& cnt,
                   uint32_t& bounces_out) {
  V3 accum = mk(0.f, 0.f, 0.f);
  V3 strength = splat(1.f);
  uint32_t bounces = 0;
  bool sampled_before = false;  // step 2 ran at the previous hit
  HitRecOf<FEAT> hit;
  rng.set_event(1);
  while (hit_top<FEAT, COUNT>(sc, o, d, time, P.t_near, rng, hit, cnt)) {
    if (COUNT) cnt.shaded++;
    const uint4 mlo = sc.mat[2 * hit.mat], mhi = sc.mat[2 * hit.mat + 1];
    const uint32_t kind = mhi.w & 0xffu;
    const float param = u2f(mlo.w);
    if (kind == MAT_DIFFUSE_LIGHT) {  // material.rs:108, :120-128
      if (!(sampled_before && lt.sampled[hit.mat])) accum = vadd(accum, vmul(strength, smul(param, material_texture<FEAT>(sc, mlo, mhi, texture_point(hit, mhi)))));
      bounces_out = bounces;
      return accum;
    }
    accum = vadd(accum, vmul(strength, mk(0.f, 0.f, 0.f)));  // lib.rs:76 for a material that emits nothing
    V3 nd, att;
    bool scattered = true;
    sampled_before = false;
    if (kind == MAT_LAMBERTIAN || kind == MAT_ISOTROPIC) {
      att = material_texture<FEAT>(sc, mlo, mhi, texture_point(hit, mhi));
      if (bounces < P.max_bounces) {
        sampled_before = true;
        const float u0 = rng.gen_f32(), u1 = rng.gen_f32(), u2 = rng.gen_f32();
        const float fn = (float)lt.n;
        uint32_t i = (uint32_t)(u0 * fn);
        if (i > lt.n - 1u) i = lt.n - 1u;
        const LightRect L = lt.lights[i];
        const float a = L.r0s + u1 * (L.r0e - L.r0s), b2 = L.r1s + u2 * (L.r1e - L.r1s);
        const V3 q = L.axis == 0u ? mk(L.k, a, b2) : (L.axis == 1u ? mk(a, L.k, b2) : mk(a, b2, L.k));  // object.rs:157-181
        const V3 w = vsub(q, hit.p);
        const float r2 = vdot(w, w), dist = __builtin_sqrtf(r2);
        const float cos_l = __builtin_fabsf(vget(w, L.axis)) / dist;
        float lobe = 1.f / (4.f * 3.14159265358979323846f);
        if (kind == MAT_LAMBERTIAN) {
          const float b = vdot(hit.n, w) / dist, disc = b * b - (vdot(hit.n, hit.n) - 1.f);
          lobe = 0.f;
          if (disc > 0.f) {
            const float sq = __builtin_sqrtf(disc), r_hi = b + sq, r_lo = rs_max(b - sq, 0.f);
            if (r_hi > 0.f) lobe = ((r_hi * r_hi) * r_hi - (r_lo * r_lo) * r_lo) / (4.f * 3.14159265358979323846f);
          }
        }
        if (lobe > 0.f && r2 > 0.f && cos_l > 0.f && !occluded<FEAT, COUNT>(sc, hit.p, w, time, P.t_near, 1.f - 1e-3f, rng, cnt)) {
          const uint4 llo = sc.mat[2 * L.mat], lhi = sc.mat[2 * L.mat + 1];
          const V3 le = smul(u2f(llo.w), material_texture<FEAT>(sc, llo, lhi, q));
          const float g = (((lobe * fn) * L.area) * cos_l) / r2;
          accum = vadd(accum, vmul(vmul(strength, att), smul(g, le)));
        }
      }
      if (kind == MAT_LAMBERTIAN) nd = vsub(vadd(vadd(hit.p, hit.n), in_unit_sphere(rng)), hit.p);  // material.rs:57-65
      else nd = in_unit_sphere(rng);                                                                  // material.rs:109-116
    } else if (kind == MAT_METAL) {  // material.rs:66-80
      V3 refl = reflect(vunit(d), hit.n);
      nd = vadd(refl, smul(param, in_unit_sphere(rng)));
      att = mk(u2f(mlo.x), u2f(mlo.y), u2f(mlo.z));
      scattered = vdot(nd, hit.n) > 0.f;
    } else {  // Dielectric, material.rs:81-107
      V3 outward;
      float ni_over_nt, cosine;
      float dn = vdot(d, hit.n);
      if (dn > 0.f) {
        outward = vneg(hit.n);
        ni_over_nt = param;
        cosine = param * dn / vlen(d);
      } else {
        outward = hit.n;
        ni_over_nt = 1.0f / param;
        cosine = -dn / vlen(d);
      }
      V3 uv = vunit(d);  // refract, vec3.rs:321-330
      float dt = vdot(uv, outward);
      float disc = 1.0f - ni_over_nt * ni_over_nt * (1.f - dt * dt);
      bool refracted = disc > 0.f;
      if (refracted) {
        nd = vsub(smul(ni_over_nt, vsub(uv, smul(dt, outward))), smul(__builtin_sqrtf(disc), outward));
        refracted = rng.gen_f32() >= schlick(cosine, param);  // material.rs:97: draw only if Some
      }
      if (!refracted) nd = reflect(d, hit.n);
      att = splat(1.f);
    }
    if (!scattered) {  // lib.rs:88-91
      bounces_out = bounces;
      return accum;
    }
    o = hit.p, d = nd;
    strength = vmul(strength, att);
    if (bounces == P.max_bounces) {  // lib.rs:93-95
      bounces_out = bounces;
      return accum;
    }
    bounces += 1;
    rng.set_event(bounces + 1);
  }
  bounces_out = bounces;
  if (P.bg.mode != BG_NONE) return miss_colour_scene<FEAT>(sc, P.bg, accum, strength, d);  // (the environment too: at full weight, never sampled)
  return accum;
}

// One sample of par_cast's closure (rt_trace.h sample_color) over color_ls
template <uint32_t FEAT, bool COUNT>
RT_DEV V3 sample_color_ls(const DevScene& sc, const LightTable& lt, const DevCamera& cam, const DevParams& P, uint32_t x, uint32_t y, uint32_t s,
                          Counts& cnt, uint32_t& bounces, uint32_t& draws) {
  SampleRng rng;
  rng.init(((uint64_t)P.seed_hi << 32) | P.seed_lo, y * P.nx + x, s);
  float u = ((float)x + rng.gen_f32()) / (float)P.nx;
  float v = ((float)y + rng.gen_f32()) / (float)P.ny;
  V3 o, d;
  float time;
  get_ray(cam, u, v, rng, o, d, time);
  V3 c = color_ls<FEAT, COUNT>(sc, lt, o, d, time, P, rng, cnt, bounces);
  draws = rng.draws;
  return c;
}

}  // namespace rtg
