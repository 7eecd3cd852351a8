// rt_query.h -- the kernels of the ray queries (include/rtiow_gpu_query.h): closest hit and occlusion for the caller's rays.
//   query_closest_kernel / query_occluded_kernel   the general kernels: one lane per ray over hit_top / occluded (rt_trace.h,
//                                                  rt_light.h), the program in global memory; every program the library flattens
//   query_lean_kernel<ANY>                         lean programs (BOX / SPHERE / END) that fit a CU's LDS: every workgroup copies
//                                                  the program to LDS once and walks that copy (rt_query_walk.h)
// Both write the same bits: the lean walk is hit_top's arithmetic, and a lean program holds no medium, so nothing draws.
#pragma once
#include "rt_light.h"
#include "rt_query_walk.h"
#include "rt_trace.h"

namespace rtg {

// ---- the general kernels ------------------------------------------------------------------------------------------------------
// Ray i has the stream rtg_debug_hit_top gives it: (seed, first + i, sample 0), event 1.
constexpr uint32_t QUERY_GENERAL_BLOCK = 64;

template <uint32_t FEAT>
__global__ __launch_bounds__(QUERY_GENERAL_BLOCK) void query_closest_kernel(DevScene sc, uint64_t n, const float* rays, uint32_t seed_lo, uint32_t seed_hi,
                                                                             uint32_t first, float t_min, float* out, uint32_t* out_mat) {
  const uint64_t i = (uint64_t)blockIdx.x * QUERY_GENERAL_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 7ull * i;
  SampleRng rng;
  rng.init(((uint64_t)seed_hi << 32) | seed_lo, first + (uint32_t)i, 0);
  rng.set_event(1);
  HitRecOf<FEAT> h;
  Counts cnt = {0, 0, 0, 0};
  const bool hit = hit_top<FEAT, false>(sc, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], t_min, rng, h, cnt);
  float* o = out + 8ull * i;
  o[0] = hit ? 1.f : 0.f;
  o[1] = hit ? h.t : 0.f;
  o[2] = hit ? h.p.x : 0.f, o[3] = hit ? h.p.y : 0.f, o[4] = hit ? h.p.z : 0.f;
  o[5] = hit ? h.n.x : 0.f, o[6] = hit ? h.n.y : 0.f, o[7] = hit ? h.n.z : 0.f;
  out_mat[i] = hit ? h.mat : 0xffffffffu;
}

template <uint32_t FEAT>
__global__ __launch_bounds__(QUERY_GENERAL_BLOCK) void query_occluded_kernel(DevScene sc, uint64_t n, const float* rays, uint32_t seed_lo, uint32_t seed_hi,
                                                                              uint32_t first, float t_min, uint8_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * QUERY_GENERAL_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 8ull * i;
  const float t_max = r[7];
  bool hit = false;
  if (t_max > t_min) {  // (false for a NaN t_max)
    SampleRng rng;
    rng.init(((uint64_t)seed_hi << 32) | seed_lo, first + (uint32_t)i, 0);
    rng.set_event(1);
    Counts cnt = {0, 0, 0, 0};
    hit = occluded<FEAT, false>(sc, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], t_min, t_max, rng, cnt);
  }
  out[i] = hit ? 1u : 0u;
}

// ---- the lean kernel ----------------------------------------------------------------------------------------------------------
// A walk is a chain of dependent record reads, about 50 per ray of book-1: from an LDS copy of the program each costs a fraction
// of what it costs through the caches (rt_camera_probe.h measured 41 us against 126 us for its walk).  Workgroup b owns the rays
// [b * rays_per_wg, (b + 1) * rays_per_wg) -- a static range, so the kernel has no global work counter, needs nothing zeroed
// between calls and may run twice at once -- and hands them to its lanes one at a time through a counter in LDS: a lane that
// finishes a ray takes its next one inside its ONE loop instead of waiting for the slowest ray of its wave.
//
// The refill arm -- the result's stores, the hand-out, the ray's loads, three divides -- runs for the whole wave whenever one
// lane is in it, and with 64 walkers whose rays end in different trips that is nearly every trip: it then costs a wave more than
// the walk itself.  So a finished lane takes its next ray in the same trip only when `refill_min` lanes of its wave are finished
// (or none is walking); until then it sits out the trips of the others.  refill_min = 1 is the every-trip shape.
//
// Sizing.  8 waves per workgroup; book-1's program is 47 KB, so three workgroups share a CU's 160 KB: 6 waves per SIMD, which
// the kernel's registers allow (make resource-usage: DESIGN.md "Ray queries").  QUERY_LEAN_MIN_RAYS rays per workgroup at the
// least -- two per lane -- so that the copy-in, 32 bytes per record, stays small beside the walks' own reads (about 50 records per
// ray); above that the rays are spread over as many workgroups as the chip holds at once (rtg_query.inc query_lean_geometry).
constexpr uint32_t QUERY_LEAN_BLOCK = 512;
constexpr uint32_t QUERY_LEAN_MIN_RAYS = 2u * QUERY_LEAN_BLOCK;
constexpr uint32_t QUERY_LEAN_MAX_RAYS = 65536u;  // rays_per_wg * (n_prog + 1) is the trip cap below: it must fit 32 bits (n_prog <= 5119)
constexpr uint32_t QUERY_LEAN_MAX_RECORDS = (160u * 1024u - 16u) / 32u;

struct QueryLean {
  const uint4* lo;        // the reference program, n_prog records
  const uint4* hi;
  uint32_t n_prog;
  uint32_t rays_per_wg;   // QUERY_LEAN_MIN_RAYS .. QUERY_LEAN_MAX_RAYS
  uint64_t n;             // rays
  const float* rays;      // n x 7 (closest) or n x 8 (any-hit: the eighth is t_max)
  float* out;             // closest: n x 8
  uint32_t* out_mat;      // closest: n
  uint8_t* out_occ;       // any-hit: n
  float t_min;
  uint32_t refill_min;    // finished lanes of a wave that start the refill arm (1 .. 64)
};
inline size_t query_lean_lds_bytes(size_t n_prog) { return n_prog * 32u + 16u; }

// Termination.  The only loop is the trip loop.  query_step returns a record number greater than the one it was given (a skip
// pointer that does not point forward is stepped over) or n_prog, so a ray is walked in at most n_prog trips; a trip that does
// in which no lane of the wave steps a ray finds every lane finished, so the refill arm runs and each lane fetches a ray or
// leaves the loop; the LDS counter hands out each of the range's `count` rays once.  So the steps and fetches of a wave number
// at most count * (n_prog + 1) + 64, every trip holds at least one of them, and the loop is capped at that.  Every LDS read
// is at a record number < n_prog; every global access is indexed by a ray number < q.n.
template <bool ANY>
__global__ __launch_bounds__(QUERY_LEAN_BLOCK) void query_lean_kernel(QueryLean q) {
  extern __shared__ uint4 s_query[];
  uint4* s_lo = s_query;
  uint4* s_hi = s_query + q.n_prog;
  uint32_t* s_next = reinterpret_cast<uint32_t*>(s_query + 2u * q.n_prog);
  // (four records per lane in flight: every load is issued, from a clamped record number, so that the copies stay in registers;
  // only records < n_prog are stored)
  for (uint32_t j0 = threadIdx.x; j0 < q.n_prog; j0 += 4u * QUERY_LEAN_BLOCK) {
    uint4 l[4], h[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
      const uint32_t j = j0 + k * QUERY_LEAN_BLOCK < q.n_prog ? j0 + k * QUERY_LEAN_BLOCK : q.n_prog - 1u;
      l[k] = q.lo[j], h[k] = q.hi[j];
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
      const uint32_t j = j0 + k * QUERY_LEAN_BLOCK;
      if (j < q.n_prog) s_lo[j] = l[k], s_hi[j] = h[k];
    }
  }
  if (threadIdx.x == 0) *s_next = 0u;
  __syncthreads();
  const uint64_t begin = (uint64_t)blockIdx.x * q.rays_per_wg;
  const uint32_t count = (uint32_t)(q.n - begin < (uint64_t)q.rays_per_wg ? q.n - begin : (uint64_t)q.rays_per_wg);
  const uint32_t stride = ANY ? 8u : 7u;
  const uint32_t max_trips = count * (q.n_prog + 1u) + 64u;
  QueryRay<V3> r = query_ray<V3>(0.f, 0.f, 0.f, 0.f, 0.f, 0.f, q.t_min);
  uint64_t ray = 0;
  bool have = false;
  uint32_t pc = q.n_prog, hit_pc = QUERY_NO_HIT;
  float end = QUERY_F32_MAX;
  for (uint32_t trip = 0; trip < max_trips; trip++) {
    if (pc < q.n_prog) pc = query_step<ANY>(s_lo[pc], s_hi[pc], pc, q.n_prog, r, end, hit_pc);
    const bool done = pc >= q.n_prog;  // the ray is walked (or the lane has none yet)
    const unsigned long long done_mask = __ballot(done), in_loop = __ballot(true);
    if (done && ((uint32_t)__popcll(done_mask) >= q.refill_min || done_mask == in_loop)) {  // its result out, the next ray in
      if (have) {
        if (ANY) {
          q.out_occ[ray] = hit_pc != QUERY_NO_HIT ? 1u : 0u;
        } else {
          float* o = q.out + 8ull * ray;
          uint32_t mat = QUERY_NO_HIT;
          if (hit_pc != QUERY_NO_HIT) {
            mat = query_hit_record(s_lo[hit_pc], s_hi[hit_pc], r, end, o);
          } else {
#pragma unroll
            for (int k = 0; k < 8; k++) o[k] = 0.f;
          }
          q.out_mat[ray] = mat;
        }
      }
      const uint32_t k = atomicAdd(s_next, 1u);
      if (k >= count) break;
      ray = begin + k, have = true;
      const float* in = q.rays + (uint64_t)stride * ray;
      r = query_ray<V3>(in[0], in[1], in[2], in[3], in[4], in[5], q.t_min);
      end = ANY ? in[7] : QUERY_F32_MAX;
      hit_pc = QUERY_NO_HIT;
      pc = (!ANY || end > q.t_min) ? 0u : q.n_prog;  // !(t_max > t_min), a NaN included: 0 without a walk (written in the next trip)
    }
  }
}

}  // namespace rtg
