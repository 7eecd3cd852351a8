// rt_camera_probe.h -- the probe walk of the camera plan (option box_camera, DESIGN.md 3 "Camera plan"): seeded paths from the
// camera a launch renders with, walked through the UNPRUNED lean program, counting for every BOX record in how many walks it
// passed.  The counts feed the tree DP of rt_box_plan.h (BOX_PLAN_COUNTS), which decides which interior boxes the
// image of that (scene, camera) pair leaves out.  Nothing here has to be exact: every plan the DP can pick is sound, the counts
// only decide its cost.  Integer adds commute, so a fixed seed gives the same counts on every run.
#pragma once
#include <cmath>
#include <vector>

#include "rt_box_plan.h"
#include "rt_trace.h"

namespace rtg {

// Paths per camera and bounces per path.  Swept once on book-1 with the benchmark camera (profiles/r24_camera_plan/sweep.txt,
// 128 .. 65 536 paths x 0 .. 5 bounces): the smallest setting whose plan stays within 0.5 % of the box tests of the largest one
// -- 1024 x 2: 0.8854 of the scene's plan against 0.8831; 512 x 3 gives 0.8896, 1024 x 1 0.8896, 2048 x 3 0.8843.  The kernel's time
// does not depend on the number of paths (they run side by side) but on the records its slowest path visits, so the cap on those
// (CAMERA_PROBE_TRIPS below) is halved and the paths are 4096: 0.8859 (sweep_trips.txt), still within 0.5 %.
#ifndef RT_CAMERA_PROBE_PATHS
#define RT_CAMERA_PROBE_PATHS 4096
#endif
#ifndef RT_CAMERA_PROBE_BOUNCES
#define RT_CAMERA_PROBE_BOUNCES 2
#endif
constexpr uint32_t CAMERA_PROBE_PATHS = RT_CAMERA_PROBE_PATHS, CAMERA_PROBE_BOUNCES = RT_CAMERA_PROBE_BOUNCES;
constexpr uint32_t CAMERA_PROBE_MAX_RECORDS = 4550;  // the program and the counts must fit a CU's 160 KB of LDS (36 B per record); larger programs keep the scene's plan
// The walk lasts as long as its slowest path (a path of three long rays visits 300 records of book-1; the mean path visits 94).  A
// path stops at this many records: the counts of the few long paths lose their tails, which only steers the DP (profiles/
// r24_camera_plan/sweep_trips.txt: the plan's box tests at other caps and without one).
#ifndef RT_CAMERA_PROBE_TRIPS
#define RT_CAMERA_PROBE_TRIPS 64
#endif
constexpr uint32_t CAMERA_PROBE_TRIPS = RT_CAMERA_PROBE_TRIPS;
constexpr uint32_t CAMERA_PROBE_STOP = 0x80000000u;  // in the flag word of a SPHERE record of the workgroup's copy: ends a path
// One wave per workgroup: all 64 lanes copy the program, 16 walk a path each.  The lanes of a wave sit at different records, so the
// fewer of them walk, the fewer trips run more than one arm of the loop: 256 paths in one workgroup took 89 .. 118 us, 16 per wave 73 us.
constexpr uint32_t CAMERA_PROBE_BLOCK = 64, CAMERA_PROBE_WALKERS = 16;

struct CameraProbe {
  const uint4* lo;       // the unpruned program, n records
  const uint4* hi;
  const uint8_t* stop;   // per record: a SPHERE that ends a path (camera_probe_stops)
  uint32_t* n_pass;      // n + 1 words, zeroed by the launcher: [j] walks in which BOX j passed, [n] rays walked
  uint32_t n;
  uint32_t grid_w, grid_h;  // the paths: one per cell of this grid over the image
  uint32_t bounces;
  uint32_t max_trips;    // records a path may visit over all its rays (CAMERA_PROBE_TRIPS): what bounds the kernel's time
  float t_near;
};

// The strata of `paths` probe paths over an image of the camera's aspect ratio: grid_w x grid_h >= paths cells, one path each.
inline void camera_probe_grid(const DevCamera& cam, uint32_t paths, uint32_t* grid_w, uint32_t* grid_h) {
  const double h = std::sqrt((double)cam.horizontal.x * cam.horizontal.x + (double)cam.horizontal.y * cam.horizontal.y + (double)cam.horizontal.z * cam.horizontal.z);
  const double v = std::sqrt((double)cam.vertical.x * cam.vertical.x + (double)cam.vertical.y * cam.vertical.y + (double)cam.vertical.z * cam.vertical.z);
  double aspect = h / v;
  if (!(aspect > 1.0 / 64.0) || !(aspect < 64.0)) aspect = 1.0;
  paths = paths < 1u ? 1u : (paths > (1u << 20) ? (1u << 20) : paths);
  uint32_t w = (uint32_t)std::ceil(std::sqrt((double)paths * aspect));
  w = w < 1u ? 1u : w;
  *grid_w = w, *grid_h = (paths + w - 1u) / w;
}

// Which SPHERE records end a probe path: a sphere that encloses all the others (a sky dome; rt_box_plan.h enclosing_spheres, the
// rule of the host probes) and an emitter (the MatKind copy in the record's flag word).
inline void camera_probe_stops(const uint32_t (*lo)[4], const uint32_t (*hi)[4], size_t n, std::vector<uint8_t>* stop) {
  box_plan_detail::enclosing_spheres(lo, hi, n, stop);
  for (size_t j = 0; j < n; j++)
    if ((hi[j][3] & 0xffu) == OP_SPHERE && ((hi[j][3] >> F_MATKIND_SHIFT) & 7u) == MAT_DIFFUSE_LIGHT) (*stop)[j] = 1;
}

// The walk is bounded by construction: the host launches it only for programs that program_shape (rt_box_plan.h) accepts, whose
// skip pointers all point forward and stay inside the program -- and the loop below still never moves a ray backwards: every trip
// either moves the lane's record number forward or starts the path's next ray, of which there are bounces + 1 at the most, so a
// path takes fewer than (bounces + 1) (n + 1) trips, and the trip count is capped at that and at `max_trips`; no other loop;
// every write is indexed by a record number < n, or by n itself (the ray count).
// `lo` / `hi`: the workgroup's copy of the program.
// The lanes of a wave sit at different records, so a wave runs the box arm AND the sphere arm in nearly every trip, as many trips
// as its slowest lane needs, 4 cycles per instruction.  Hence (a) ONE loop per path -- a lane that ends a ray starts its next one
// in the same trip instead of waiting for the wave at the end of a bounce; (b) no rejection loops; (c) short arithmetic: v_rcp_f32 and v_sqrt_f32 (1 ulp)
// where the render kernels divide and take correctly rounded roots (30 instructions each).  The counts only steer the DP; no plan
// is unsound.
RT_DEV void camera_probe_path(const CameraProbe& p, const uint4* lo, const uint4* hi, const DevCamera& cam, uint32_t i, uint32_t* s_pass) {
  uint32_t state = i * 0x9e3779b9u + 0x7f4a7c15u;
  auto unit = [&]() {  // PCG output on an LCG state: [0, 1)
    state = state * 747796405u + 2891336453u;
    uint32_t w = ((state >> ((state >> 28) + 4u)) ^ state) * 277803737u;
    w = (w >> 22) ^ w;
    return (float)(w >> 8) * (1.0f / 16777216.0f);
  };
  const uint32_t cx = i % p.grid_w, cy = i / p.grid_w;
  const float s = ((float)cx + unit()) * __builtin_amdgcn_rcpf((float)p.grid_w), t = ((float)cy + unit()) * __builtin_amdgcn_rcpf((float)p.grid_h);
  float lx = 2.f * unit() - 1.f, ly = 2.f * unit() - 1.f;  // a point of the lens disc: of the square, halved when outside the disc
  if (lx * lx + ly * ly >= 1.f) lx *= 0.5f, ly *= 0.5f;
  const V3 offset = vadd(smul(cam.lens_radius * lx, cam.u), smul(cam.lens_radius * ly, cam.v));
  V3 o = vadd(cam.origin, offset);
  V3 d = vsub(vsub(vadd(vadd(cam.llc, smul(s, cam.horizontal)), smul(t, cam.vertical)), cam.origin), offset);
  V3 inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
  float dd = vdot(d, d), inv_dd = __builtin_amdgcn_rcpf(dd);
  float best = F32_MAX, best_r = 1.f;
  uint32_t best_pc = 0xffffffffu, pc = 0, bounce = 0;
  V3 best_c = mk(0.f, 0.f, 0.f);
  bool best_stop = false;
  atomicAdd(&s_pass[p.n], 1u);
  const uint32_t bound = (p.bounces + 1u) * (p.n + 1u), max_trips = bound < p.max_trips ? bound : p.max_trips;
  for (uint32_t trip = 0; trip < max_trips; trip++) {
    if (pc < p.n) {
      const uint4 l = lo[pc], h = hi[pc];
      const uint32_t op = h.w & 0xffu;
      if (op == OP_BOX) {  // Aabb::hit, lo = (min.x, max.x, min.y, max.y), hi = (min.z, max.z, skip, flags)
        const float ax = (__uint_as_float(l.x) - o.x) * inv.x, bx = (__uint_as_float(l.y) - o.x) * inv.x;
        const float ay = (__uint_as_float(l.z) - o.y) * inv.y, by = (__uint_as_float(l.w) - o.y) * inv.y;
        const float az = (__uint_as_float(h.x) - o.z) * inv.z, bz = (__uint_as_float(h.y) - o.z) * inv.z;
        const float start = rs_max(p.t_near, rs_max(rs_max(inv.x < 0.f ? bx : ax, inv.y < 0.f ? by : ay), inv.z < 0.f ? bz : az));
        const float end = rs_min(best, rs_min(rs_min(inv.x < 0.f ? ax : bx, inv.y < 0.f ? ay : by), inv.z < 0.f ? az : bz));
        if (end > start) {
          atomicAdd(&s_pass[pc], 1u);
          pc++;
        } else {
          pc = h.z > pc ? h.z : pc + 1u;
        }
      } else if (op == OP_SPHERE) {  // Sphere::hit behind an optional Translate; lo = (offset.xyz, radius)
        const bool tr = (h.w & F_TRANSLATE) != 0u;
        const V3 c = tr ? mk(__uint_as_float(l.x), __uint_as_float(l.y), __uint_as_float(l.z)) : mk(0.f, 0.f, 0.f);
        const float r = __uint_as_float(l.w);
        const V3 q = vsub(o, c);
        const float b = vdot(q, d), cc = vdot(q, q) - r * r, disc = b * b - dd * cc;
        if (disc > 0.f) {
          const float sq = __builtin_amdgcn_sqrtf(disc);
          float th = (-b - sq) * inv_dd;
          if (!(th < best && th >= p.t_near)) th = (-b + sq) * inv_dd;
          if (th < best && th >= p.t_near) best = th, best_pc = pc, best_c = c, best_r = r, best_stop = (h.w & CAMERA_PROBE_STOP) != 0u;
        }
        pc++;
      } else {
        pc = p.n;  // END
      }
    }
    if (pc >= p.n) {  // the ray is walked: the path ends on a miss, the dome, an emitter or its last bounce, else its next ray starts
      if (best_pc >= p.n || best_stop || bounce >= p.bounces) break;
      o = vadd(o, smul(best, d));
      const V3 nrm = smul(__builtin_amdgcn_rcpf(best_r), vsub(o, best_c));
      // a point of the unit ball without a rejection loop (the arm runs for the whole wave whenever one lane is here): a point of
      // the cube, halved when it lies outside the ball
      const float wx = 2.f * unit() - 1.f, wy = 2.f * unit() - 1.f, wz = 2.f * unit() - 1.f;
      const float ws = wx * wx + wy * wy + wz * wz < 1.f ? 1.f : 0.5f;
      const V3 v = mk(ws * wx, ws * wy, ws * wz);
      d = vadd(nrm, v);
      dd = vdot(d, d);
      if (!(dd < F32_MAX)) break;  // (a NaN or infinite normal: a degenerate sphere)
      inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z)), inv_dd = __builtin_amdgcn_rcpf(dd);
      best = F32_MAX, best_pc = 0xffffffffu, best_stop = false, pc = 0, bounce++;
      atomicAdd(&s_pass[p.n], 1u);
    }
  }
}

// A walk is a chain of dependent record reads, about 50 per ray.  From global memory the kernel took 126 us (profiles/
// r24_camera_plan/README.txt): every workgroup first copies the program to LDS -- plain global loads, 47 KB for book-1 -- and walks
// that copy, and it keeps the counts in LDS too (every ray passes the boxes at the top of the tree), adding them to the global ones
// once at the end: 256 adds per record instead of thousands on one word.  Dynamic LDS: camera_probe_lds_bytes(n).
inline size_t camera_probe_lds_bytes(size_t n) { return n * 32u + (n + 1u) * sizeof(uint32_t); }
__global__ __launch_bounds__(CAMERA_PROBE_BLOCK) void camera_probe_kernel(CameraProbe p, DevCamera cam) {
  extern __shared__ uint4 s_probe[];
  uint4* s_lo = s_probe;
  uint4* s_hi = s_probe + p.n;
  uint32_t* s_pass = reinterpret_cast<uint32_t*>(s_probe + 2u * p.n);
  // (eight records per lane in flight)
  for (uint32_t j0 = threadIdx.x; j0 < p.n; j0 += 8u * CAMERA_PROBE_BLOCK) {
    uint4 l[8], h[8];
    uint32_t st[8];
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) {
      const uint32_t j = j0 + k * CAMERA_PROBE_BLOCK;
      if (j < p.n) l[k] = p.lo[j], h[k] = p.hi[j], st[k] = p.stop[j];
    }
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) {
      const uint32_t j = j0 + k * CAMERA_PROBE_BLOCK;
      if (j < p.n) {
        if (st[k]) h[k].w |= CAMERA_PROBE_STOP;
        s_lo[j] = l[k], s_hi[j] = h[k];
      }
    }
  }
  for (uint32_t j = threadIdx.x; j <= p.n; j += blockDim.x) s_pass[j] = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * CAMERA_PROBE_WALKERS + threadIdx.x;
  if (threadIdx.x < CAMERA_PROBE_WALKERS && i < p.grid_w * p.grid_h) camera_probe_path(p, s_lo, s_hi, cam, i, s_pass);
  __syncthreads();
  for (uint32_t j = threadIdx.x; j <= p.n; j += blockDim.x)
    if (s_pass[j]) atomicAdd(&p.n_pass[j], s_pass[j]);
}

}  // namespace rtg
