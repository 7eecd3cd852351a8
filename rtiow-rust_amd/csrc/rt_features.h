// rt_features.h -- the feature pass of RTG_FLAG_FEATURES (include/rtiow_gpu.h): first-hit albedo, normal and depth planes from
// g x g primary rays per pixel, sent from the lens centre at the middle of the exposure -- deterministic, independent of the
// frame's samples.  Two kernels:
//   features -- one lane per pixel, a wave an 8 x 8 pixel block of ONE tile (as render_pixel, rtg_kernels.inc): the rays of
//               rtiow-rust_amd/features.py subpixel_rays in its order, one hit_top each with the RNG stream rtg_debug_hit_top gives
//               ray index y * nx + x, the left fold of the seven values from +0, one division per value; counts traced / missed per block;
//   finish   -- one workgroup sums the block counts into the caller's rtg_features block.
// Every float operation is a single rounded f32 operation (the build has -ffp-contract=off and the correctly rounded divide).
// All stores are plain stores.
#pragma once
#include "rt_trace.h"

namespace rtg {

constexpr uint32_t FT_MAX_GRID = 4;  // RTG_FEATURES_MAX_GRID

struct FeatureBufs {
  float* albedo;      // nx ny 3
  float* normal;      // nx ny 3
  float* depth;       // nx ny
  uint32_t* block;    // the caller's rtg_features, as 16 words
  uint32_t* blk_u32;  // per block of the feature kernel: traced, missed
};

// what a material returns as its colour at the hit: the attenuation of scatter(), emitted() for a light (material.rs:55-128);
// a surface-mapped texture (MAT_SURFACE) is read at the hit's (tu, tv, 0) as color() reads it
template <uint32_t FEAT>
RT_DEV V3 feature_albedo(const DevScene& sc, const HitRecOf<FEAT>& h) {
  const uint4 mlo = sc.mat[2 * h.mat], mhi = sc.mat[2 * h.mat + 1];
  const uint32_t kind = mhi.w & 0xffu;
  if (kind == MAT_METAL) return mk(u2f(mlo.x), u2f(mlo.y), u2f(mlo.z));
  if (kind == MAT_DIELECTRIC) return splat(1.f);
  const V3 t = material_texture<FEAT>(sc, mlo, mhi, texture_point(h, mhi));
  return kind == MAT_DIFFUSE_LIGHT ? smul(u2f(mlo.w), t) : t;
}

template <uint32_t FEAT>
__global__ __launch_bounds__(256) void features_kernel(DevScene sc, DevCamera cam, DevParams P, uint32_t g, FeatureBufs b) {
  __shared__ uint32_t s_t[4], s_m[4];
  const uint32_t nbx = (P.nx + 15u) / 16u;
  const uint32_t bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const uint32_t tiles_x = (P.nx + P.tile_w - 1u) / P.tile_w;
  const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63u;
  const uint32_t x0 = bx * 16u + (w & 1u) * 8u, row0 = by * 16u + (w >> 1) * 8u;  // this wave's 8x8 block: inside ONE tile
  const uint32_t tile = (row0 / P.tile_h) * tiles_x + x0 / P.tile_w;
  const uint32_t x = x0 + (l & 7u), row = row0 + (l >> 3);
  const bool mine = tile % P.nranks == P.rank && x < P.nx && row < P.ny;
  bool miss = false;
  if (mine) {
    const uint32_t y = P.ny - 1u - row;  // lib.rs:328: row 0 is y = ny-1
    const float gf = (float)g;
    const float time = cam.e0 + 0.5f * (cam.e1 - cam.e0);
    V3 a = mk(0.f, 0.f, 0.f), n = mk(0.f, 0.f, 0.f);
    float z = 0.f;
    bool any = false;
#pragma unroll 1
    for (uint32_t j = 0; j < g; j++) {
#pragma unroll 1
      for (uint32_t i = 0; i < g; i++) {
        const float su = ((float)i + 0.5f) / gf, sv = ((float)j + 0.5f) / gf;
        const float u = ((float)x + su) / (float)P.nx, v = ((float)y + sv) / (float)P.ny;
        const V3 d = vsub(vadd(vadd(cam.llc, smul(u, cam.horizontal)), smul(v, cam.vertical)), cam.origin);  // camera.rs:52-63, no lens offset
        SampleRng rng;
        rng.init(((uint64_t)P.seed_hi << 32) | P.seed_lo, y * P.nx + x, 0);
        rng.set_event(1);
        HitRecOf<FEAT> h;
        Counts cnt = {0, 0, 0, 0};
        V3 ha = mk(0.f, 0.f, 0.f), hn = mk(0.f, 0.f, 0.f);
        float hz = 0.f;
        if (hit_top<FEAT, false>(sc, cam.origin, d, time, P.t_near, rng, h, cnt)) {
          ha = feature_albedo<FEAT>(sc, h), hn = h.n, hz = h.t;
          any = true;
        }
        a = vadd(a, ha), n = vadd(n, hn), z = z + hz;
      }
    }
    const float gg = (float)(g * g);
    a = sdiv(a, gg), n = sdiv(n, gg), z = z / gg;
    const size_t p = (size_t)row * P.nx + x;
    float* oa = b.albedo + 3ull * p;
    float* on = b.normal + 3ull * p;
    oa[0] = a.x, oa[1] = a.y, oa[2] = a.z;
    on[0] = n.x, on[1] = n.y, on[2] = n.z;
    b.depth[p] = z;
    miss = !any;
  }
  const uint32_t n_t = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(mine));
  const uint32_t n_m = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(miss));
  if (l == 0u) s_t[w] = n_t, s_m[w] = n_m;
  __syncthreads();
  if (threadIdx.x == 0u) {
    b.blk_u32[2u * blockIdx.x] = s_t[0] + s_t[1] + s_t[2] + s_t[3];
    b.blk_u32[2u * blockIdx.x + 1u] = s_m[0] + s_m[1] + s_m[2] + s_m[3];
  }
}

// One workgroup of 256: thread t sums blocks t, t + 256, ..., then a tree over the threads.  Writes the out-fields of the
// rtg_features block (words 6 .. 15: traced, missed, reserved).  n_blk = 0 (compute = 0, or a rank without a tile): zeros.
__global__ __launch_bounds__(256) void features_finish_kernel(uint32_t n_blk, FeatureBufs b) {
  __shared__ uint32_t s_u[2][256];
  const uint32_t t = threadIdx.x;
  uint32_t tr = 0, ms = 0;
  for (uint32_t i = t; i < n_blk; i += 256u) tr += b.blk_u32[2u * i], ms += b.blk_u32[2u * i + 1u];
  s_u[0][t] = tr, s_u[1][t] = ms;
  __syncthreads();
  for (uint32_t h = 128u; h > 0u; h >>= 1) {
    if (t < h) s_u[0][t] += s_u[0][t + h], s_u[1][t] += s_u[1][t + h];
    __syncthreads();
  }
  if (t < 10u) b.block[6u + t] = t == 0u ? s_u[0][0] : (t == 1u ? s_u[1][0] : 0u);
}

}  // namespace rtg
