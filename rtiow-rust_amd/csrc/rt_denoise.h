// rt_denoise.h -- the filter step of RTG_FLAG_DENOISE (include/rtiow_gpu.h): a variance-driven non-local-means filter over the
// frame's undivided running sums, bit for bit rtiow-rust_amd/denoise.py nlm.  Three kernels:
//   prepare -- per pixel (m, v, valid) from (S, Q, e_p) into a 32-byte record (two float4: means + valid word, variances);
//              writes the pass-through pixels (e_p > 0, not valid) of the output plane and counts filtered / passed per block;
//   filter  -- a workgroup owns a 32 x 16 tile of output pixels.  It stages the records of the tile plus a halo of R + F pixels
//              into LDS once (two float4 planes: consecutive lanes read consecutive 16-byte slots), then, per displacement in
//              raster order: pd for the tile plus F halo (once per pair, three divisions), barrier, the row folds, barrier, the
//              column folds, the weight and the accumulation in registers;
//   finish  -- one workgroup sums the block counts into the caller's rtg_denoise block.
// Every float operation is a single rounded f32 operation (the build has -ffp-contract=off and the correctly rounded divide),
// in the order denoise.py states; zero-weight neighbours are skipped (every accumulator starts at +0 and never becomes -0, so
// adding their +-0 products changes nothing).  All stores are plain stores.
// With RTG_FLAG_FEATURES the filter is GUIDED (denoise.py nlm_guided): a fourth kernel, guide, packs the frame's albedo, normal
// and depth planes into a second 32-byte record per pixel, and the filter's guided instantiations cap every colour weight by
// the feature weight of the pair -- reading the neighbour's record through the caches (GUIDED = 1) or from an LDS copy of the
// tile plus a halo of R (GUIDED = 2).  A pair whose colour weight is +0 skips the feature weight: min(wf, +0) is +0 for every wf.
// With RTG_FLAG_DENOISE_ERROR the prepare and filter kernels are their ERR instantiations (denoise.py nlm_error / nlm_guided_error):
// the filter also folds (w * w) * v_q per pair -- one more recB read, inside the staged halo -- and stores ev = (acc2 / wsum) / wsum
// into the frame's error plane; prepare writes the +inf of the pass-through pixels there.  ERR = false compiles to the code
// without the flag.
#pragma once
#include "rt_pool.h"

namespace rtg {

constexpr uint32_t DN_TW = 32, DN_TH = 16, DN_THREADS = 256;
constexpr uint32_t DN_MAX_RADIUS = 8, DN_MAX_PATCH = 3;  // RTG_DENOISE_MAX_RADIUS / RTG_DENOISE_MAX_PATCH
// iterations of the strided loops at the largest patch: pd over (32 + 6) x (16 + 6) pixels, row folds over 32 x (16 + 6)
constexpr uint32_t DN_PD_ITER = ((DN_TW + 2 * DN_MAX_PATCH) * (DN_TH + 2 * DN_MAX_PATCH) + DN_THREADS - 1) / DN_THREADS;
constexpr uint32_t DN_ROW_ITER = (DN_TW * (DN_TH + 2 * DN_MAX_PATCH) + DN_THREADS - 1) / DN_THREADS;

// The block's in-fields (validated by the launcher) and the call's ns
struct DenoiseArgs {
  float k;
  uint32_t radius, patch;
  uint32_t ns;  // e_p = min(n_p, ns) with a count plane, else ns
};

struct DenoiseBufs {
  const float* planes;     // plane 0 (running sums); plane 1 (running sums of squares) at + 3 nx ny
  const uint32_t* counts;  // the count plane, or nullptr
  float4* rec;             // per pixel (m0, m1, m2, valid ? word 1 : 0) (v0, v1, v2, 0); all zero when not valid
  float* outp;             // the output plane
  uint32_t* block;         // the caller's rtg_denoise, as 16 words
  uint32_t* blk_u32;       // per prepare block: filtered, passed
  float* errp;             // RTG_FLAG_DENOISE_ERROR: the error plane (the ERR instantiations alone read this field)
};

// The guided filter's own arguments: the feature records ((a0, a1, a2, z) (n0, n1, n2, all seven finite ? word 1 : 0) per pixel)
// and the three sigmas of the rtg_features block
struct DenoiseGuide {
  const float4* frec;
  float sigma_normal, sigma_albedo, sigma_depth;
};

// bytes of dynamic LDS the filter kernel needs; guide_lds: the guided filter's LDS copy of the feature records (GUIDED = 2)
static inline size_t denoise_lds_bytes(uint32_t radius, uint32_t patch, bool guide_lds = false) {
  const size_t h = radius + patch;
  const size_t guide = guide_lds ? (DN_TW + 2 * radius) * (DN_TH + 2 * radius) * 32u : 0u;
  return (DN_TW + 2 * h) * (DN_TH + 2 * h) * 32u + (DN_TW + 2 * patch) * (DN_TH + 2 * patch) * 8u + DN_TW * (DN_TH + 2 * patch) * 8u + guide;
}

RT_DEV bool dn_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

template <bool ERR>
__global__ __launch_bounds__(256) void denoise_prepare_kernel(uint32_t n_pix, DenoiseArgs a, DenoiseBufs b) {
  __shared__ uint32_t s_f[4], s_p[4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
  bool valid = false, pass = false;
  if (p < n_pix) {
    uint32_t e = a.ns;
    if (b.counts) {
      const uint32_t n = b.counts[p];
      e = n < a.ns ? n : a.ns;
    }
    const float* s = b.planes + 3ull * p;
    const float* q = s + 3ull * n_pix;
    const float ef = (float)(e > 1u ? e : 1u);
    const float ee = ef * (ef - 1.f);
    float m[3], v[3];
    bool fin = true;
    for (int c = 0; c < 3; c++) {
      m[c] = s[c] / ef;
      float d = q[c] - s[c] * m[c];
      d = d > 0.f ? d : 0.f;
      v[c] = d / ee;
      fin = fin && dn_finite(m[c]) && dn_finite(v[c]);
    }
    valid = e >= 2u && fin;
    pass = !valid && e > 0u;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    b.rec[2ull * p] = valid ? make_float4(m[0], m[1], m[2], __uint_as_float(1u)) : zero;
    b.rec[2ull * p + 1u] = valid ? make_float4(v[0], v[1], v[2], 0.f) : zero;
    if (pass) {
      float* o = b.outp + 3ull * p;
      o[0] = m[0], o[1] = m[1], o[2] = m[2];
      if (ERR) {  // a pass-through pixel: its error is unknown
        float* ev = b.errp + 3ull * p;
        ev[0] = ev[1] = ev[2] = __uint_as_float(0x7f800000u);
      }
    }
  }
  const uint32_t n_f = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(valid));
  const uint32_t n_p = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(pass));
  if (lane == 0u) s_f[wave] = n_f, s_p[wave] = n_p;
  __syncthreads();
  if (threadIdx.x == 0u) {
    b.blk_u32[2u * blockIdx.x] = s_f[0] + s_f[1] + s_f[2] + s_f[3];
    b.blk_u32[2u * blockIdx.x + 1u] = s_p[0] + s_p[1] + s_p[2] + s_p[3];
  }
}

// RTG_FLAG_DENOISE | RTG_FLAG_FEATURES: the feature records of the guided filter from the frame's three feature planes
__global__ __launch_bounds__(256) void denoise_guide_kernel(uint32_t n_pix, const float* albedo, const float* normal, const float* depth, float4* frec) {
  const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (p >= n_pix) return;
  const float* al = albedo + 3ull * p;
  const float* nn = normal + 3ull * p;
  const float z = depth[p];
  const bool fin = dn_finite(al[0]) && dn_finite(al[1]) && dn_finite(al[2]) && dn_finite(nn[0]) && dn_finite(nn[1]) && dn_finite(nn[2]) && dn_finite(z);
  frec[2ull * p] = make_float4(al[0], al[1], al[2], z);
  frec[2ull * p + 1u] = make_float4(nn[0], nn[1], nn[2], __uint_as_float(fin ? 1u : 0u));
}

// the feature weight of a pair (denoise.py nlm_guided): pA / pB and qA / qB are the two pixels' feature records
RT_DEV float dn_feature_weight(float4 pA, float4 pB, float4 qA, float4 qB, float sn2, float sa2, float sz2) {
  if (__float_as_uint(pB.w) == 0u || __float_as_uint(qB.w) == 0u) return 1.f;
  const float dn0 = pB.x - qB.x, dn1 = pB.y - qB.y, dn2 = pB.z - qB.z;
  const float da0 = pA.x - qA.x, da1 = pA.y - qA.y, da2 = pA.z - qA.z;
  const float xn = ((dn0 * dn0 + dn1 * dn1) + dn2 * dn2) / sn2;
  const float xa = ((da0 * da0 + da1 * da1) + da2 * da2) / sa2;
  const float dz = pA.w - qA.w, s = pA.w + qA.w;
  const float xz = ((dz * dz) / (s * s + 1e-20f)) / sz2;
  float x = xn;
  x = xa > x ? xa : x;
  x = xz > x ? xz : x;
  float u = 1.f - x * 0.25f;
  u = u > 0.f ? u : 0.f;
  return (u * u) * (u * u);
}

// GUIDED: 0 = the colour-only filter; 1 / 2 = the guided filter, the neighbours' feature records read through the caches / from LDS
// ERR: also the variance of the output into the error plane
template <int GUIDED, bool ERR>
__global__ __launch_bounds__(256) void denoise_filter_kernel(uint32_t nx, uint32_t ny, DenoiseArgs a, DenoiseBufs b, DenoiseGuide gd) {
  extern __shared__ float4 dn_lds[];
  const int R = (int)a.radius, F = (int)a.patch, H = R + F;
  const int WR = (int)DN_TW + 2 * H, HR = (int)DN_TH + 2 * H;  // the staged records: tile + halo of R + F
  const int WA = (int)DN_TW + 2 * F, HA = (int)DN_TH + 2 * F;  // where pd is needed: tile + halo of F
  float4* recA = dn_lds;                                       // (m0, m1, m2, valid)
  float4* recB = recA + WR * HR;                               // (v0, v1, v2, 0)
  float2* pd = reinterpret_cast<float2*>(recB + WR * HR);      // (pd, counted ? 1 : 0) of the current displacement
  float2* rr = pd + WA * HA;                                   // its row folds (r, rc): rows of the tile + F halo, columns of the tile
  const int tid = (int)threadIdx.x;
  const uint32_t tiles_x = (nx + DN_TW - 1u) / DN_TW;
  const long long tx0 = (long long)(blockIdx.x % tiles_x) * DN_TW, ty0 = (long long)(blockIdx.x / tiles_x) * DN_TH;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = tid; i < WR * HR; i += (int)DN_THREADS) {
    const long long gx = tx0 + (i % WR) - H, gy = ty0 + (i / WR) - H;
    float4 A = zero, B = zero;
    if (gx >= 0 && gx < (long long)nx && gy >= 0 && gy < (long long)ny) {
      const size_t p = (size_t)gy * nx + (size_t)gx;
      A = b.rec[2ull * p], B = b.rec[2ull * p + 1u];
    }
    recA[i] = A, recB[i] = B;
  }
  // GUIDED = 2: the feature records of the tile plus a halo of R, behind the row folds
  const int WG = (int)DN_TW + 2 * R, HG = (int)DN_TH + 2 * R;
  float4* fA = reinterpret_cast<float4*>(rr + (int)DN_TW * HA);
  float4* fB = fA + WG * HG;
  if (GUIDED == 2) {
    for (int i = tid; i < WG * HG; i += (int)DN_THREADS) {
      const long long gx = tx0 + (i % WG) - R, gy = ty0 + (i / WG) - R;
      float4 A = zero, B = zero;
      if (gx >= 0 && gx < (long long)nx && gy >= 0 && gy < (long long)ny) {
        const size_t p = (size_t)gy * nx + (size_t)gx;
        A = gd.frec[2ull * p], B = gd.frec[2ull * p + 1u];
      }
      fA[i] = A, fB[i] = B;
    }
  }
  // this thread's pd elements (index into the records, -1: none) and row folds
  int pd_at[DN_PD_ITER];
  for (uint32_t j = 0; j < DN_PD_ITER; j++) {
    const int i = tid + (int)(j * DN_THREADS);
    pd_at[j] = i < WA * HA ? (i / WA + R) * WR + (i % WA) + R : -1;
  }
  // ... and its two output pixels: (x, y0) and (x, y0 + 8) of the tile
  const int x = tid & 31, y0 = tid >> 5;
  __syncthreads();
  int at[2];
  bool ok[2];
  float acc[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, wsum[2] = {0.f, 0.f};
  float acc2[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};  // (ERR)
  for (int j = 0; j < 2; j++) {
    at[j] = (y0 + 8 * j + H) * WR + x + H;
    ok[j] = __float_as_uint(recA[at[j]].w) != 0u;  // valid (pixels outside the image are not)
  }
  // guided: this thread's two feature records, where the neighbours' are (GUIDED = 1: in the frame; 2: in LDS), the sigmas squared
  long long gat[2] = {0, 0};
  float4 pfA[2] = {zero, zero}, pfB[2] = {zero, zero};
  const float sn2 = gd.sigma_normal * gd.sigma_normal, sa2 = gd.sigma_albedo * gd.sigma_albedo, sz2 = gd.sigma_depth * gd.sigma_depth;
  if (GUIDED != 0) {
    for (int j = 0; j < 2; j++) {
      if (!ok[j]) continue;  // (valid: inside the image)
      if (GUIDED == 1) {
        gat[j] = (ty0 + y0 + 8 * j) * (long long)nx + (tx0 + x);
        pfA[j] = gd.frec[2ull * (size_t)gat[j]], pfB[j] = gd.frec[2ull * (size_t)gat[j] + 1u];
      } else {
        gat[j] = (y0 + 8 * j + R) * WG + x + R;
        pfA[j] = fA[gat[j]], pfB[j] = fB[gat[j]];
      }
    }
  }
  const float k2 = a.k * a.k, eps = 1e-10f;
  for (int dy = -R; dy <= R; dy++)
    for (int dx = -R; dx <= R; dx++) {
      const int delta = dy * WR + dx;
#pragma unroll
      for (uint32_t j = 0; j < DN_PD_ITER; j++) {
        const int ia = pd_at[j];
        if (ia < 0) continue;
        const float4 aA = recA[ia], bA = recA[ia + delta];
        float2 o = make_float2(0.f, 0.f);
        if (__float_as_uint(aA.w) != 0u && __float_as_uint(bA.w) != 0u) {
          const float4 aB = recB[ia], bB = recB[ia + delta];
          const float ma[3] = {aA.x, aA.y, aA.z}, mb[3] = {bA.x, bA.y, bA.z};
          const float va[3] = {aB.x, aB.y, aB.z}, vb[3] = {bB.x, bB.y, bB.z};
          float d2[3];
          for (int c = 0; c < 3; c++) {
            const float diff = ma[c] - mb[c];
            const float num = diff * diff - (va[c] + (vb[c] < va[c] ? vb[c] : va[c]));
            const float den = eps + k2 * (va[c] + vb[c]);
            d2[c] = num / den;
          }
          o = make_float2((d2[0] + d2[1]) + d2[2], 1.f);
        }
        pd[tid + (int)(j * DN_THREADS)] = o;
      }
      __syncthreads();
#pragma unroll
      for (uint32_t j = 0; j < DN_ROW_ITER; j++) {
        const int i = tid + (int)(j * DN_THREADS);
        if (i >= (int)DN_TW * HA) continue;
        const float2* src = pd + (i >> 5) * WA + (i & 31);
        float r = 0.f, rc = 0.f;
        for (int ox = 0; ox <= 2 * F; ox++) {
          const float2 t = src[ox];
          r = r + t.x, rc = rc + t.y;
        }
        rr[i] = make_float2(r, rc);
      }
      __syncthreads();
      for (int j = 0; j < 2; j++) {
        if (!ok[j]) continue;
        const float4 qA = recA[at[j] + delta];
        if (__float_as_uint(qA.w) == 0u) continue;  // w = 0
        const float2* src = rr + (y0 + 8 * j) * (int)DN_TW + x;
        float D = 0.f, cnt = 0.f;
        for (int oy = 0; oy <= 2 * F; oy++) {
          const float2 t = src[oy * (int)DN_TW];
          D = D + t.x, cnt = cnt + t.y;
        }
        float xx = D / (3.f * cnt);
        xx = xx > 0.f ? xx : 0.f;
        float u = 1.f - xx * 0.25f;
        u = u > 0.f ? u : 0.f;
        const float u2 = u * u;
        float w = u2 * u2;
        if (GUIDED != 0 && w > 0.f) {  // (q is valid: inside the image)
          float4 qfA, qfB;
          if (GUIDED == 1) {
            const size_t q = (size_t)(gat[j] + (long long)dy * (long long)nx + dx);
            qfA = gd.frec[2ull * q], qfB = gd.frec[2ull * q + 1u];
          } else {
            qfA = fA[gat[j] + dy * WG + dx], qfB = fB[gat[j] + dy * WG + dx];
          }
          const float wf = dn_feature_weight(pfA[j], pfB[j], qfA, qfB, sn2, sa2, sz2);
          w = wf < w ? wf : w;
        }
        acc[j][0] = acc[j][0] + w * qA.x;
        acc[j][1] = acc[j][1] + w * qA.y;
        acc[j][2] = acc[j][2] + w * qA.z;
        wsum[j] = wsum[j] + w;
        if (ERR && w > 0.f) {  // (w = +0 adds three +0 products)
          const float4 qB = recB[at[j] + delta];
          const float w2 = w * w;
          acc2[j][0] = acc2[j][0] + w2 * qB.x;
          acc2[j][1] = acc2[j][1] + w2 * qB.y;
          acc2[j][2] = acc2[j][2] + w2 * qB.z;
        }
      }
      // (the next displacement's pd stores follow this one's row folds by the second barrier; its row folds follow these reads
      // by its first barrier)
    }
  for (int j = 0; j < 2; j++) {
    if (!ok[j]) continue;  // (valid: inside the image)
    const size_t p = (size_t)(ty0 + y0 + 8 * j) * nx + (size_t)(tx0 + x);
    float* o = b.outp + 3ull * p;
    o[0] = acc[j][0] / wsum[j], o[1] = acc[j][1] / wsum[j], o[2] = acc[j][2] / wsum[j];
    if (ERR) {
      float* ev = b.errp + 3ull * p;
      ev[0] = (acc2[j][0] / wsum[j]) / wsum[j], ev[1] = (acc2[j][1] / wsum[j]) / wsum[j], ev[2] = (acc2[j][2] / wsum[j]) / wsum[j];
    }
  }
}

// One workgroup of 256: thread t sums blocks t, t + 256, ..., then a tree over the threads.  Writes the out-fields of the
// rtg_denoise block (words 4 .. 15: filtered, passed, reserved).
__global__ __launch_bounds__(256) void denoise_finish_kernel(uint32_t n_blk, DenoiseBufs b) {
  __shared__ uint32_t s_u[2][256];
  const uint32_t t = threadIdx.x;
  uint32_t f = 0, p = 0;
  for (uint32_t i = t; i < n_blk; i += 256u) f += b.blk_u32[2u * i], p += b.blk_u32[2u * i + 1u];
  s_u[0][t] = f, s_u[1][t] = p;
  __syncthreads();
  for (uint32_t h = 128u; h > 0u; h >>= 1) {
    if (t < h) s_u[0][t] += s_u[0][t + h], s_u[1][t] += s_u[1][t + h];
    __syncthreads();
  }
  if (t < 12u) b.block[4u + t] = t == 0u ? s_u[0][0] : (t == 1u ? s_u[1][0] : 0u);
}

}  // namespace rtg
