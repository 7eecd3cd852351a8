// rt_box_plan.h -- host only: which interior BOX records of a lean program the production image of the lean pool kernel
// leaves out (option box_prune).  No device code, no HIP header: a plain C++ program can include it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "flat_scene.h"

namespace rtg {

// Record layout as in rt_pool.h box_chain_followers: lo = (min.x, max.x, min.y, max.y), hi = (min.z, max.z, skip, flags) for
// a BOX, lo = (offset.xyz, radius), hi = (-, -, material, flags) for a SPHERE.
constexpr uint8_t BOX_KEPT = 0, BOX_FOLLOWER = 1, BOX_PRUNED = 2;
// Probe rays per scene, and which plan.  The plan may not cost more than creating the scene does without it (book-1:
// rtg_scene_create 0.20 ms on the measuring host), and a probe costs ~0.34 us there: 256 probes.  That many find the boxes
// that EVERY ray passes (the sure-pass subset: book-1's root and dome path), which is the plan that ships.  The cost plan
// over all pass counts (RT_BOX_PLAN_FULL = 1, the tree DP below) needs 8192 probes or more before it beats the subset by
// more than run-to-run spread (HISTORY.md "Box pruning"); it is a build-time switch for measurements until probes are cheaper.
#ifndef RT_BOX_PLAN_PROBES
#define RT_BOX_PLAN_PROBES 256
#endif
#ifndef RT_BOX_PLAN_FULL
#define RT_BOX_PLAN_FULL 0
#endif
constexpr uint32_t BOX_PLAN_PROBES = RT_BOX_PLAN_PROBES;
constexpr bool BOX_PLAN_FULL = RT_BOX_PLAN_FULL != 0;
// Which plan: the sure-pass subset, the tree DP on the probes' pass counts, or the same DP on a pass probability that needs no
// ray -- a box's surface area over the area of the box around everything that is not a sky dome (at `box_plan`, "Choice").
// BOX_PLAN_COUNTS: the DP on pass counts handed in from outside -- the camera plan, whose probe paths the GPU walks for the camera
// a launch renders with (rt_camera_probe.h; option box_camera).
enum BoxPlanKind : int { BOX_PLAN_SURE = 0, BOX_PLAN_PROBE_DP = 1, BOX_PLAN_AREA = 2, BOX_PLAN_COUNTS = 3 };
constexpr BoxPlanKind BOX_PLAN_DEFAULT = BOX_PLAN_FULL ? BOX_PLAN_PROBE_DP : BOX_PLAN_SURE;
// The plan of the rebuilt program (box_tree_rebuild below; option box_tree) and its probes.  The area model ships: no probe
// walk at all.  0 / 1 keep the other two plans buildable for measurements (HISTORY.md "Box tree").
#ifndef RT_BOX_TREE_PLAN
#define RT_BOX_TREE_PLAN 2
#endif
constexpr BoxPlanKind BOX_TREE_PLAN = (BoxPlanKind)(RT_BOX_TREE_PLAN);

struct BoxPlan {
  uint32_t n_pruned = 0;  // records with mask BOX_PRUNED
  uint32_t n_sure = 0;    // ... of which every probe ray passed (the sure-pass subset)
  uint32_t n_rays = 0;    // probe walks made
};

namespace box_plan_detail {
inline float as_f(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// Aabb::hit (aabb.rs:18-29), the reference's order: (plane - o) * (1 / d), swap on 1/d < 0, f32::max / f32::min (fmaxf / fminf
// ignore a NaN operand as they do), end > start
inline bool aabb_hit(const uint32_t* lo, const uint32_t* hi, const float* o, const float* inv, float t_near, float best) {
  const float mn[3] = {as_f(lo[0]), as_f(lo[2]), as_f(hi[0])}, mx[3] = {as_f(lo[1]), as_f(lo[3]), as_f(hi[1])};
  float t0[3], t1[3];
  for (int a = 0; a < 3; a++) {
    const float u = (mn[a] - o[a]) * inv[a], v = (mx[a] - o[a]) * inv[a];
    t0[a] = inv[a] < 0.f ? v : u, t1[a] = inv[a] < 0.f ? u : v;
  }
  const float start = fmaxf(t_near, fmaxf(fmaxf(t0[0], t0[1]), t0[2]));
  const float end = fminf(best, fminf(fminf(t1[0], t1[1]), t1[2]));
  return end > start;
}
// Sphere::hit (object.rs:84-111) behind an optional Translate (object.rs:275)
inline bool sphere_hit(const uint32_t* lo, uint32_t flags, const float* o, const float* d, float dd, float t_near, float best, float* t_out) {
  float p[3] = {o[0], o[1], o[2]};
  if (flags & F_TRANSLATE)
    for (int a = 0; a < 3; a++) p[a] = o[a] - as_f(lo[a]);
  const float r = as_f(lo[3]);
  const float b = p[0] * d[0] + p[1] * d[1] + p[2] * d[2];
  const float c = p[0] * p[0] + p[1] * p[1] + p[2] * p[2] - r * r;
  const float disc = b * b - dd * c;
  if (disc > 0.f) {
    const float sq = sqrtf(disc);
    float t = (-b - sq) / dd;
    if (t < best && t >= t_near) return *t_out = t, true;
    t = (-b + sq) / dd;
    if (t < best && t >= t_near) return *t_out = t, true;
  }
  return false;
}
struct Rng {  // splitmix64: seeded and fixed, so a scene always gets the same plan
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  float unit() { return (float)(next() >> 40) * (1.f / 16777216.f); }  // [0, 1)
  void in_unit_sphere(float* v) {
    do {
      for (int a = 0; a < 3; a++) v[a] = 2.f * unit() - 1.f;
    } while (v[0] * v[0] + v[1] * v[1] + v[2] * v[2] >= 1.f);
  }
};
inline bool finite6(const uint32_t* lo, const uint32_t* hi) {
  return std::isfinite(as_f(lo[0])) && std::isfinite(as_f(lo[1])) && std::isfinite(as_f(lo[2])) && std::isfinite(as_f(lo[3])) &&
         std::isfinite(as_f(hi[0])) && std::isfinite(as_f(hi[1]));
}
// surface area of a BOX record's planes, in float64
inline double box_area(const uint32_t* lo, const uint32_t* hi) {
  const double dx = (double)as_f(lo[1]) - (double)as_f(lo[0]), dy = (double)as_f(lo[3]) - (double)as_f(lo[2]),
               dz = (double)as_f(hi[1]) - (double)as_f(hi[0]);
  return 2.0 * (dx * dy + dy * dz + dz * dx);
}
// The shape of a lean program: the BOX around every record and its depth (false: a skip pointer does not nest or point
// forward), and which records meet conditions (a)-(c) of the statement below.
struct Shape {
  std::vector<int32_t> parent;
  std::vector<uint32_t> depth;
  std::vector<uint8_t> prunable;
  uint32_t n_prunable = 0;
};
inline bool leaf_box_at(const uint32_t (*hi)[4], size_t n, size_t j) {
  return (hi[j][3] & 0xffu) == OP_BOX && j + 2 < n && (hi[j + 1][3] & 0xffu) == OP_SPHERE && hi[j][2] == j + 2;
}
inline bool program_shape(const uint32_t (*lo)[4], const uint32_t (*hi)[4], size_t n, Shape* sh) {
  auto op = [&](size_t j) { return hi[j][3] & 0xffu; };
  auto skip = [&](size_t j) { return (size_t)hi[j][2]; };
  sh->parent.assign(n, -1), sh->depth.assign(n, 0), sh->prunable.assign(n, 0), sh->n_prunable = 0;
  if (n < 4 || n > 0x7fffffffu) return false;
  std::vector<uint32_t> open;
  for (size_t j = 0; j < n; j++) {
    while (!open.empty() && skip(open.back()) <= j) open.pop_back();
    if (!open.empty()) sh->parent[j] = (int32_t)open.back(), sh->depth[j] = (uint32_t)open.size();
    if (op(j) != OP_BOX) continue;
    if (skip(j) <= j || skip(j) >= n || (!open.empty() && skip(j) > skip(open.back()))) return false;
    open.push_back((uint32_t)j);
  }
  auto contains = [&](size_t j, size_t c) {
    return as_f(lo[j][0]) <= as_f(lo[c][0]) && as_f(lo[j][1]) >= as_f(lo[c][1]) && as_f(lo[j][2]) <= as_f(lo[c][2]) &&
           as_f(lo[j][3]) >= as_f(lo[c][3]) && as_f(hi[j][0]) <= as_f(hi[c][0]) && as_f(hi[j][1]) >= as_f(hi[c][1]);
  };
  for (size_t j = n; j-- > 0;) {  // bottom-up: the children of a node come behind it
    if (op(j) != OP_BOX || j + 1 >= n || op(j + 1) != OP_BOX) continue;
    const size_t L = j + 1, R = skip(L);
    if (!(L < R && R < skip(j)) || op(R) != OP_BOX || skip(R) != skip(j)) continue;
    if (!finite6(lo[j], hi[j]) || !finite6(lo[L], hi[L]) || !finite6(lo[R], hi[R]) || !contains(j, L) || !contains(j, R)) continue;
    if (!(leaf_box_at(hi, n, L) || sh->prunable[L]) || !(leaf_box_at(hi, n, R) || sh->prunable[R])) continue;
    sh->prunable[j] = 1, sh->n_prunable++;
  }
  return true;
}
// A SPHERE record's centre, and the spheres that hold the box around all centres (a sky dome): no probe starts or bounces
// there.  `starts` (optional): the other spheres with finite geometry, where the host probes begin.
inline void sphere_centre(const uint32_t (*lo)[4], const uint32_t (*hi)[4], uint32_t j, float* c) {
  for (int a = 0; a < 3; a++) c[a] = (hi[j][3] & F_TRANSLATE) ? as_f(lo[j][a]) : 0.f;
}
inline void enclosing_spheres(const uint32_t (*lo)[4], const uint32_t (*hi)[4], size_t n, std::vector<uint8_t>* enclosing,
                              std::vector<uint32_t>* starts = nullptr) {
  std::vector<uint32_t> spheres;
  for (size_t j = 0; j < n; j++)
    if ((hi[j][3] & 0xffu) == OP_SPHERE) spheres.push_back((uint32_t)j);
  float cmin[3] = {INFINITY, INFINITY, INFINITY}, cmax[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t j : spheres) {
    float c[3];
    sphere_centre(lo, hi, j, c);
    for (int a = 0; a < 3; a++) cmin[a] = fminf(cmin[a], c[a]), cmax[a] = fmaxf(cmax[a], c[a]);
  }
  enclosing->assign(n, 0);
  for (uint32_t j : spheres) {
    float cj[3];
    sphere_centre(lo, hi, j, cj);
    const float r = as_f(lo[j][3]);
    float far2 = 0.f;  // squared distance to the farthest corner of that box
    for (int a = 0; a < 3; a++) {
      const float d = fmaxf(cmax[a] - cj[a], cj[a] - cmin[a]);
      far2 += d * d;
    }
    const bool all = spheres.size() > 1 && far2 < r * r;
    (*enclosing)[j] = all;
    if (starts && !all && std::isfinite(r) && std::isfinite(cj[0]) && std::isfinite(cj[1]) && std::isfinite(cj[2])) starts->push_back(j);
  }
}
}  // namespace box_plan_detail

// Box pruning.  Statement: in the production walk an interior BOX j may be left out (its test taken as passed) without
// changing which spheres are tested, in which order, against which t range -- so (best, best_pc) stay bit for bit -- when
// j is PRUNABLE:
//   (a) j is a BOX, L = j + 1 is a BOX, R = skip[L] is a BOX with L < R < skip[j] and skip[R] == skip[j]: a binary Bvh node
//       (bvh.rs:66-81), not a leaf box and not a box around anything else;
//   (b) every plane of j, L and R is finite, and min_j <= min_L, min_R and max_j >= max_L, max_R on all three axes;
//   (c) L and R are each a leaf box (BOX, SPHERE, skip = the record behind the sphere) or prunable themselves;
//   (d) the run of box-chain followers right behind j, if any, does not end in a leaf box (below, at `choosable`).
// Proof.  Fix a ray (o, d) and t_near.  Per axis Aabb::hit forms u(p) = fl(fl(p - o) * inv) for both planes.  fl(p - o) is
// monotone in p, the product with the fixed inv keeps the order (inv >= 0) or reverses it (inv < 0), and the swap on inv < 0
// reverses it again, for parent and child alike: near(parent) <= near(child) and far(parent) >= far(child) wherever both are
// numbers.  A NaN term is ignored by f32::max / f32::min, i.e. acts as -inf in `start` and +inf in `end`.  With finite planes
// the child's term is NaN only when o or inv is NaN (then the parent's is NaN too), when fl(p - o) is infinite (o is, and the
// parent's difference is the same infinity) or when it is 0 * inf; in the last case the parent's difference has the sign that
// makes its term NaN or -inf in `start`, NaN or +inf in `end`.  So start(parent) <= start(child), and for equal t_range.end
// end(parent) >= end(child).  An ancestor is tested before its descendants, when `best` (t_range.end) is no smaller.  Hence
// by (b) along the whole path, which (c) grants: whenever a leaf box below j passes at the moment the left-to-right walk
// reaches it, every box on the path up to j passed when it was tested.  Conversely, with j left out, a leaf box that the
// reference would not have reached fails on its own test, or an interior box that is still there fails above it.  A leaf
// is reached, and its Sphere::hit evaluated, exactly when the reference does so, with the same `best`.  (Leaf boxes stay: a
// sphere can accept a hit that its own box rejects by rounding.)  The image gives a pruned record 0 bytes like a follower:
// its offset is its left child's, and a skip pointer that targeted it lands on that child (rt_pool.h, the staging loop).
//
// Choice.  The plan that ships leaves out the allowed boxes that every probe ray passed: such a box costs a test and never
// saves one.  BOX_PLAN_PROBE_DP (the reference program's plan in a build with RT_BOX_PLAN_FULL): n_pass(B), the number of walks in which B passes, does not depend on which prunable boxes are left out (above).
// The box tests a plan executes are the sum over kept boxes of n_pass of their nearest kept ancestor (the ray count when
// there is none): f(B, A) = min(n_pass(A) + sum f(child, B), sum f(child, A)), the second term for prunable B only, taken
// on <= -- a box that every probe passes is always pruned.  A box-chain follower costs nothing (it is left out anyway).
// n_pass comes from `n_probes` seeded rays walked here through the full program: each chain starts at a random point of a
// random sphere that does not enclose the others, leaves along normal + in_unit_sphere, and bounces on like that one to three
// times while it hits such a sphere.  BOX_PLAN_AREA is the same DP without a ray: n_pass(B) / rays is replaced by
// min(1, SA(B) / SA_ref), the chance that a line through the scene's box also meets B (below, where n_pass is filled).
// BOX_PLAN_COUNTS is the same DP once more, on n_pass handed in from outside: counts[j] walks out of count_rays passed BOX j
// (the camera plan: paths from the camera a launch renders with, walked on the GPU -- rt_camera_probe.h).  The proof above
// never asks where n_pass comes from: every subset of the choosable records is a sound plan, and the counts only decide which
// subset is taken to be the cheapest.  So any counts are accepted -- zeros, counts above the ray count (clamped to it), counts
// that rise from a parent to its child, which no walk produces -- and the mask is sound for all of them.
//
// mask[j] = BOX_FOLLOWER where follower[j] (the box-chains rule wins), BOX_PRUNED for the plan's records, else BOX_KEPT.
// sure[j] (optional) = 1 for the pruned records that every probe passed.  A malformed program (a skip pointer that does
// not nest) gets no pruned record.
inline BoxPlan box_plan(const uint32_t (*lo)[4], const uint32_t (*hi)[4], size_t n, const uint8_t* follower, uint8_t* mask,
                        uint8_t* sure = nullptr, uint32_t n_probes = BOX_PLAN_PROBES, BoxPlanKind kind = BOX_PLAN_DEFAULT,
                        const uint32_t* counts = nullptr, uint64_t count_rays = 0) {
  using namespace box_plan_detail;
  BoxPlan out;
  for (size_t j = 0; j < n; j++) {
    mask[j] = follower && follower[j] ? BOX_FOLLOWER : BOX_KEPT;
    if (sure) sure[j] = 0;
  }
  auto op = [&](size_t j) { return hi[j][3] & 0xffu; };
  auto skip = [&](size_t j) { return (size_t)hi[j][2]; };
  Shape shape;
  if (!program_shape(lo, hi, n, &shape) || !shape.n_prunable) return out;
  const std::vector<int32_t>& parent = shape.parent;
  const std::vector<uint32_t>& depth = shape.depth;
  const std::vector<uint8_t>& prunable = shape.prunable;
  auto leaf_box = [&](size_t j) { return leaf_box_at(hi, n, j); };
  // (d) a follower LEAF box is left out because the box right before its run of followers, bitwise the same, has just passed:
  // that head must stay in the walk, or nothing tests the leaf's box any more.  (Interior followers behind a prunable head are
  // prunable themselves by (c).)  The head costs what the leaf box would: one test per ray that gets there.
  std::vector<uint8_t> choosable(prunable);
  for (size_t j = 0; j + 1 < n; j++) {
    if (!prunable[j] || !follower) continue;
    size_t k = j + 1;
    while (k + 1 < n && follower[k] && !leaf_box(k)) k++;
    if (follower[k] && leaf_box(k)) choosable[j] = 0;
  }

  // ---- probe walks: n_pass ----
  std::vector<uint64_t> n_pass(n, 0);
  std::vector<uint32_t> starts;
  std::vector<uint8_t> enclosing;
  enclosing_spheres(lo, hi, n, &enclosing, &starts);
  auto centre = [&](uint32_t j, float* c) { sphere_centre(lo, hi, j, c); };
  uint64_t n_rays = 0;
  if (kind == BOX_PLAN_COUNTS) {
    if (!counts) return out;
    for (size_t j = 0; j < n; j++)
      if (op(j) == OP_BOX) n_pass[j] = counts[j] < count_rays ? counts[j] : count_rays;
    n_rays = count_rays;
  } else if (!starts.empty() && kind != BOX_PLAN_AREA) {
    Rng rng{0x626f78706c616e31ull ^ (uint64_t)n};
    const float t_near = 0.001f;
    while (n_rays < n_probes) {
      const uint32_t s0 = starts[rng.next() % starts.size()];
      float c[3], nrm[3], o[3], d[3], v[3];
      centre(s0, c);
      do rng.in_unit_sphere(nrm);
      while (nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2] < 1e-4f);
      const float len = sqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]), r0 = as_f(lo[s0][3]);
      for (int a = 0; a < 3; a++) nrm[a] /= len, o[a] = c[a] + r0 * nrm[a];
      const uint32_t bounces = 1u + (uint32_t)(rng.next() % 3u);
      for (uint32_t k = 0; k <= bounces && n_rays < n_probes; k++) {
        rng.in_unit_sphere(v);
        for (int a = 0; a < 3; a++) d[a] = nrm[a] + v[a];
        const float inv[3] = {1.f / d[0], 1.f / d[1], 1.f / d[2]};
        const float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        float best = 3.402823466e+38f;
        int64_t best_pc = -1;
        n_rays++;
        for (size_t pc = 0; pc < n;) {  // hit_top of a lean program: BOX / SPHERE / END
          const uint32_t o_ = op(pc);
          if (o_ == OP_BOX) {
            if (aabb_hit(lo[pc], hi[pc], o, inv, t_near, best)) n_pass[pc]++, pc++;
            else pc = skip(pc);
          } else if (o_ == OP_SPHERE) {
            float t;
            if (sphere_hit(lo[pc], hi[pc][3], o, d, dd, t_near, best, &t)) best = t, best_pc = (int64_t)pc;
            pc++;
          } else break;
        }
        if (best_pc < 0 || enclosing[best_pc]) break;
        centre((uint32_t)best_pc, c);
        const float r = as_f(lo[best_pc][3]);
        for (int a = 0; a < 3; a++) o[a] = o[a] + best * d[a], nrm[a] = (o[a] - c[a]) / r;
        if (!(std::isfinite(nrm[0]) && std::isfinite(nrm[1]) && std::isfinite(nrm[2]))) break;
      }
    }
  }
  out.n_rays = (uint32_t)n_rays;
  if (kind == BOX_PLAN_AREA) {
    // no ray: "B passes" with probability min(1, SA(B) / SA_ref) in units of 2^-30, SA_ref the area of the box around the leaf
    // boxes of all spheres that are no sky dome -- a box that holds the dome gets 1 and, where allowed, is always left out
    constexpr uint64_t ONE = 1ull << 30;
    float rmin[3] = {INFINITY, INFINITY, INFINITY}, rmax[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t j = 0; j + 1 < n; j++) {
      if (!leaf_box(j) || enclosing[j + 1] || !finite6(lo[j], hi[j])) continue;
      const float mn[3] = {as_f(lo[j][0]), as_f(lo[j][2]), as_f(hi[j][0])}, mx[3] = {as_f(lo[j][1]), as_f(lo[j][3]), as_f(hi[j][1])};
      for (int a = 0; a < 3; a++) rmin[a] = fminf(rmin[a], mn[a]), rmax[a] = fmaxf(rmax[a], mx[a]);
    }
    const double dx = (double)rmax[0] - rmin[0], dy = (double)rmax[1] - rmin[1], dz = (double)rmax[2] - rmin[2];
    const double sa_ref = 2.0 * (dx * dy + dy * dz + dz * dx);
    if (!(sa_ref > 0.0) || !std::isfinite(sa_ref)) return out;  // (no such leaf: no model, followers only)
    for (size_t j = 0; j < n; j++) {
      if (op(j) != OP_BOX) continue;
      const double r = finite6(lo[j], hi[j]) ? box_area(lo[j], hi[j]) / sa_ref : 1.0;
      n_pass[j] = r >= 1.0 ? ONE : (r > 0.0 ? (uint64_t)(r * (double)ONE) : 0u);
    }
    n_rays = ONE;
  }

  // ---- the tree DP ----  f[j][k]: tests executed below and at j when its nearest kept ancestor is the k-th box of its path
  // (k = 0: none, the ray count).  States = sum of (depth + 1): a degenerate tree of very many records keeps only the sure subset,
  // as BOX_PLAN_SURE always does.
  uint64_t states = 0;
  for (size_t j = 0; kind != BOX_PLAN_SURE && j < n; j++)
    if (op(j) == OP_BOX) states += depth[j] + 2u;
  const bool dp = kind != BOX_PLAN_SURE && states <= (1ull << 26);
  std::vector<uint32_t> kidx(n, 0);
  std::vector<uint8_t> pruned(n, 0);
  if (dp) {
    // (one arena each: record j's entries start at at[j])
    std::vector<uint64_t> at(n + 1, 0);
    for (size_t j = 0; j < n; j++) at[j + 1] = at[j] + (op(j) == OP_BOX ? depth[j] + 2u : 0u);
    std::vector<uint64_t> acc(at[n], 0);    // sum of the children's f, per k of the child (depth + 2 entries)
    std::vector<uint8_t> choice(at[n], 0);  // per k: 1 = leave j out (depth + 1 entries)
    std::vector<uint64_t> path_pass, f;
    for (size_t j = n; j-- > 0;) {
      if (op(j) != OP_BOX) continue;
      const uint32_t dj = depth[j];
      uint64_t* acc_j = &acc[at[j]];
      uint8_t* choice_j = &choice[at[j]];
      path_pass.assign(dj + 1u, n_rays);
      for (int32_t a = parent[j], k = (int32_t)dj; a >= 0; a = parent[a], k--) path_pass[k] = n_pass[a];
      f.assign(dj + 1u, 0);
      for (uint32_t k = 0; k <= dj; k++) {
        const uint64_t own = follower && follower[j] ? 0u : path_pass[k];
        const uint64_t keep = own + acc_j[dj + 1u], leave = acc_j[k];
        if (choosable[j] && leave <= keep) f[k] = leave, choice_j[k] = 1;
        else f[k] = keep;
      }
      if (parent[j] >= 0) {
        uint64_t* up = &acc[at[parent[j]]];  // (the parent's depth + 2 = dj + 1 entries)
        for (uint32_t k = 0; k <= dj; k++) up[k] += f[k];
      }
    }
    for (size_t j = 0; j < n; j++) {  // top-down
      if (op(j) != OP_BOX) continue;
      const int32_t p = parent[j];
      kidx[j] = p < 0 ? 0u : (pruned[p] ? kidx[p] : depth[j]);
      pruned[j] = choice[at[j] + kidx[j]];
    }
  } else {
    for (size_t j = 0; j < n; j++) pruned[j] = choosable[j] && n_rays && n_pass[j] == n_rays && op(j) == OP_BOX;
  }
  for (size_t j = 0; j < n; j++) {
    if (!pruned[j] || mask[j] == BOX_FOLLOWER) continue;
    mask[j] = BOX_PRUNED, out.n_pruned++;
    if (n_pass[j] == n_rays) {
      out.n_sure++;
      if (sure) sure[j] = 1;
    }
  }
  return out;
}

// Box tree (option box_tree).  The proof above never uses the SHAPE of the tree below a prunable record: it needs
// that every interior box contains its children's boxes (finite planes), and that the leaves -- a leaf BOX and its SPHERE --
// are met in the reference's left-to-right order.  Then a leaf's Sphere::hit runs exactly when that leaf's own box passes
// against the `best` the earlier leaves left, whatever interior boxes stand above it.  So every binary tree over the same leaf
// sequence makes the same Sphere::hit calls, in the same order, against the same t range: (best, winning sphere) stay bit for
// bit, and only the number of box tests changes.  Bvh::new (bvh.rs:22-81) splits at the median of a random axis, a poor tree
// for its own leaf order.  This builds a better one:
//   region   a maximal part of the program under conditions (a)-(c): the records [j, skip[j]) of a prunable j whose enclosing
//            BOX is not prunable (or does not exist);
//   leaves   its leaf pairs in program order, copied unchanged (planes, sphere, material, flags);
//   tree     top-down over the sequence: the node over leaves [a, b) splits at the k that minimises
//            SA(a..k) * (k - a) + SA(k..b) * (b - k), areas in float64 from prefix and suffix merges, ties at the lowest k;
//   boxes    a node's planes are the min / max over its leaves' planes (the first of equal values is kept, so any association
//            gives the same bits; this is Aabb::merge, exact on finite floats), its flag word the region root's (F_BVH_ROOT
//            only at the root), its skip pointer the record behind its subtree, as the flattener forms it.
// A region has as many interior records as before (a binary tree over m leaves has m - 1), so it fills the same range of the
// program and nothing outside it moves.  A region with a non-finite leaf plane is left as it is, and so is one whose build
// would take more than 64 * m * (1 + log2 m) merges (a degenerate sequence: the budget keeps the work far below m^2); a
// program whose skip pointers do not nest is copied.  out_lo / out_hi: n records.  origin[j]: the record of the given program
// that record j copies, BOX_TREE_NEW for a new interior box.  Returns the number of regions rebuilt.
constexpr uint32_t BOX_TREE_NEW = 0xffffffffu;
inline uint32_t box_tree_rebuild(const uint32_t (*lo)[4], const uint32_t (*hi)[4], size_t n, uint32_t (*out_lo)[4],
                                 uint32_t (*out_hi)[4], uint32_t* origin) {
  using namespace box_plan_detail;
  for (size_t j = 0; j < n; j++) {
    std::memcpy(out_lo[j], lo[j], 16), std::memcpy(out_hi[j], hi[j], 16);
    origin[j] = (uint32_t)j;
  }
  Shape shape;
  if (!program_shape(lo, hi, n, &shape) || !shape.n_prunable) return 0;
  struct Box { float mn[3], mx[3]; };
  auto merge = [](const Box& a, const Box& b) {
    Box m;
    for (int x = 0; x < 3; x++) m.mn[x] = b.mn[x] < a.mn[x] ? b.mn[x] : a.mn[x], m.mx[x] = b.mx[x] > a.mx[x] ? b.mx[x] : a.mx[x];
    return m;
  };
  auto area = [](const Box& b) {
    const double dx = (double)b.mx[0] - b.mn[0], dy = (double)b.mx[1] - b.mn[1], dz = (double)b.mx[2] - b.mn[2];
    return 2.0 * (dx * dy + dy * dz + dz * dx);
  };
  std::vector<uint32_t> leaf;    // the region's leaf BOX records
  std::vector<Box> box;
  std::vector<double> suffix;
  struct Job { uint32_t a, b, at; };  // leaves [a, b) go to the records from `at` on
  std::vector<Job> jobs;
  std::vector<uint32_t> rec_lo, rec_hi, rec_origin;  // the region's new records (8 words each) until the build is known to finish
  uint32_t regions = 0;
  for (size_t j = 0; j < n; j++) {
    if (!shape.prunable[j]) continue;
    const size_t end = hi[j][2];
    if (shape.parent[j] >= 0 && shape.prunable[shape.parent[j]]) continue;
    leaf.clear(), box.clear();
    bool ok = true;
    for (size_t i = j; i < end; i++) {
      if (!leaf_box_at(hi, n, i)) continue;
      ok = ok && finite6(lo[i], hi[i]);
      leaf.push_back((uint32_t)i);
      box.push_back(Box{{as_f(lo[i][0]), as_f(lo[i][2]), as_f(hi[i][0])}, {as_f(lo[i][1]), as_f(lo[i][3]), as_f(hi[i][1])}});
    }
    const size_t m = leaf.size();
    if (!ok || m < 2 || 3 * m - 1 != end - j) { j = end - 1; continue; }  // ((a)-(c) make it m - 1 nodes + m leaf pairs)
    uint64_t budget = 64ull * m, work = 0;
    for (size_t v = m; v > 1; v >>= 1) budget += 64ull * m;
    const size_t len = end - j;
    rec_lo.assign(4 * len, 0), rec_hi.assign(4 * len, 0), rec_origin.assign(len, BOX_TREE_NEW);
    suffix.resize(m);
    jobs.clear();
    jobs.push_back(Job{0u, (uint32_t)m, 0u});
    while (!jobs.empty() && ok) {
      const Job t = jobs.back();
      jobs.pop_back();
      uint32_t* rl = &rec_lo[4 * t.at];
      uint32_t* rh = &rec_hi[4 * t.at];
      if (t.b - t.a == 1) {  // the leaf pair, unchanged but for where its skip pointer lands
        const uint32_t src = leaf[t.a];
        std::memcpy(rl, lo[src], 16), std::memcpy(rh, hi[src], 16), std::memcpy(rl + 4, lo[src + 1], 16), std::memcpy(rh + 4, hi[src + 1], 16);
        rh[2] = (uint32_t)j + t.at + 2u;
        rec_origin[t.at] = src, rec_origin[t.at + 1] = src + 1u;
        continue;
      }
      work += 2ull * (t.b - t.a);
      if (work > budget) { ok = false; break; }
      Box run = box[t.b - 1];
      for (uint32_t k = t.b - 1; k > t.a; k--) run = k == t.b - 1 ? run : merge(box[k], run), suffix[k] = area(run);
      run = box[t.a];
      uint32_t best_k = t.a + 1;
      double best_cost = INFINITY;
      for (uint32_t k = t.a + 1; k < t.b; k++) {  // left = [a, k), right = [k, b)
        if (k > t.a + 1) run = merge(run, box[k - 1]);
        const double cost = area(run) * (double)(k - t.a) + suffix[k] * (double)(t.b - k);
        if (cost < best_cost) best_cost = cost, best_k = k;
      }
      const Box all = merge(run, box[t.b - 1]);  // (run: the leaves [a, b - 1), merged left to right)
      const float f[6] = {all.mn[0], all.mx[0], all.mn[1], all.mx[1], all.mn[2], all.mx[2]};
      std::memcpy(rl, f, 16), std::memcpy(rh, f + 4, 8);
      rh[2] = (uint32_t)j + t.at + 3u * (t.b - t.a) - 1u;
      rh[3] = t.at == 0u ? hi[j][3] : (hi[j][3] & ~F_BVH_ROOT);
      jobs.push_back(Job{best_k, t.b, t.at + 1u + 3u * (best_k - t.a) - 1u});
      jobs.push_back(Job{t.a, best_k, t.at + 1u});
    }
    if (ok) {
      for (size_t i = 0; i < len; i++) {
        std::memcpy(out_lo[j + i], &rec_lo[4 * i], 16), std::memcpy(out_hi[j + i], &rec_hi[4 * i], 16);
        origin[j + i] = rec_origin[i];
      }
      regions++;
    }
    j = end - 1;
  }
  return regions;
}

}  // namespace rtg
