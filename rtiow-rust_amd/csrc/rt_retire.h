// rt_retire.h -- the retire step of adaptive sampling (include/rtiow_gpu.h RTG_FLAG_RETIRE): at the end of a counts call, before
// its division, every owned pixel whose (2 radius + 1)^2 window has converged gets n_p := k (= ns of the call) in the count plane.
// Three kernels, in the shape of the compaction of rt_pool.h (blocks of 256 work items in work_to_pixel order):
//   mark   -- per pixel q: its OK bit (e_q >= 2 and three standard errors <= target; pixels with n_q == 0 do not veto) into a
//             bit plane, and per block the pixels with a finite estimate, their sum of se^2 and the samples held;
//   apply  -- per candidate pixel p (n_p > k, k >= min_samples): the AND of the OK bits over its window, clipped to the image;
//             writes n_p := k, and counts per block the pixels still active and those retired;
//   finish -- one workgroup sums the block partials in a fixed order into the caller's rtg_retire block.
// Every reduction has a fixed order (wave butterflies, then the 4 waves of a block in order, then the blocks by a fixed
// stride-and-tree), so sum_se2 has the same bits however the kernels are scheduled.  All stores are plain stores.
// With RTG_FLAG_DENOISE_ERROR the mark kernel is retire_mark_error_kernel: the same bit plane and partials from the frame's error
// plane (rt_denoise.h: the variance ev of every filtered pixel) instead of (S, Q); apply and finish are shared.
#pragma once
#include "rt_pool.h"

namespace rtg {

// The block's in-fields (validated by the launcher) and the call's k
struct RetireArgs {
  double target_se;
  uint32_t k;            // ns of the call: e_q = min(n_q, k)
  uint32_t min_samples;
  uint32_t radius;       // <= RTG_RETIRE_MAX_RADIUS (8): a window row spans at most 17 bits, two words of the bit plane
};

struct RetireBufs {
  const float* planes;   // plane 0 (running sums); plane 1 (running sums of squares) at + 3 nx ny
  uint32_t* counts;      // the count plane (n_p, row-major)
  uint32_t* block;       // the caller's rtg_retire, as 16 words: written word by word (the frame need only be 4-byte aligned)
  uint32_t* okbits;      // one bit per pixel (bit x & 31 of word x >> 5 of its row): q is OK, or n_q == 0
  uint32_t pitch;        // words per row of okbits: nx / 32 rounded up, plus one (a window's second word stays in its row)
  uint32_t* blk_u32;     // per block: estimated, active, retired
  unsigned long long* blk_held;  // per block: the samples held (sum of e_p)
  double* blk_se2;       // per block: the sum of se^2 over its estimated pixels
  const float* errp;     // RTG_FLAG_DENOISE_ERROR: the error plane (retire_mark_error_kernel alone reads this field)
};

// noise.standard_error_counts of one channel with e >= 2 samples, in its operation order (the build has -ffp-contract=off: no
// fused multiply-add): m = S / e, v = (Q - (e m) m) / (e - 1), np.maximum(0, v) (NaN stays NaN), sqrt(v / e).
RT_DEV double retire_se(float sum, float sq, uint32_t e) {
  const double n = (double)e;
  const double m = (double)sum / n;
  double v = ((double)sq - (n * m) * m) / (n - 1.0);
  v = (0.0 >= v) ? 0.0 : v;
  return sqrt(v / n);
}

__global__ __launch_bounds__(256) void retire_mark_kernel(DevParams P, PixMap pm, RetireArgs a, RetireBufs b) {
  __shared__ uint32_t s_est[4];
  __shared__ unsigned long long s_held[4];
  __shared__ double s_se2[4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  uint32_t x = 0, row = 0;
  const bool in = work_to_pixel(P, pm, blockIdx.x * 256u + threadIdx.x, x, row);
  bool ok = true, est = false;  // (outside the image: no veto -- the window is clipped anyway)
  unsigned long long held = 0;
  double se2 = 0.0;
  if (in) {
    const size_t p = (size_t)row * P.nx + x;
    const uint32_t n = b.counts[p], e = n < a.k ? n : a.k;
    held = e;
    if (n != 0u) {
      ok = false;
      if (e >= 2u) {
        const float* s = b.planes + 3ull * p;
        const float* q = s + 3ull * ((size_t)P.nx * P.ny);
        const double se_0 = retire_se(s[0], q[0], e), se_1 = retire_se(s[1], q[1], e), se_2 = retire_se(s[2], q[2], e);
        ok = se_0 <= a.target_se && se_1 <= a.target_se && se_2 <= a.target_se;
        est = isfinite(se_0) && isfinite(se_1) && isfinite(se_2);
        if (est) se2 = (se_0 * se_0 + se_1 * se_1) + se_2 * se_2;
      }
    }
  }
  // A wave is one 8x8 block of a tile (work_to_pixel: tiles are multiples of 8, so lane = index in the block): byte j of the
  // ballot holds the OK bits of the block's row j, pixels x0 .. x0 + 7 with x0 a multiple of 8 -- byte x0 / 8 of that row.
  const uint64_t m = __builtin_amdgcn_ballot_w64(ok);
  if (in && (lane & 7u) == 0u) reinterpret_cast<uint8_t*>(b.okbits + (size_t)row * b.pitch)[x >> 3] = (uint8_t)(m >> (lane & 56u));
  const uint32_t n_est = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(est));
  for (int off = 32; off > 0; off >>= 1) {
    held += __shfl_xor(held, off, 64);
    se2 += __shfl_xor(se2, off, 64);
  }
  if (lane == 0u) s_est[wave] = n_est, s_held[wave] = held, s_se2[wave] = se2;
  __syncthreads();
  if (threadIdx.x == 0u) {
    b.blk_u32[3u * blockIdx.x] = s_est[0] + s_est[1] + s_est[2] + s_est[3];
    b.blk_held[blockIdx.x] = s_held[0] + s_held[1] + s_held[2] + s_held[3];
    b.blk_se2[blockIdx.x] = ((s_se2[0] + s_se2[1]) + s_se2[2]) + s_se2[3];
  }
}

// RTG_FLAG_DENOISE_ERROR (noise.py retire_filtered): q is OK when its three ev are finite and (double)ev <= target2, the float64
// product target_se * target_se the launcher computed once; estimated = the pixels with n > 0 and three finite ev, their
// partial ((double)ev_0 + ev_1) + ev_2.  The filter of the same call wrote the plane of every pixel with n > 0.
__global__ __launch_bounds__(256) void retire_mark_error_kernel(DevParams P, PixMap pm, RetireArgs a, RetireBufs b, double target2) {
  __shared__ uint32_t s_est[4];
  __shared__ unsigned long long s_held[4];
  __shared__ double s_se2[4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  uint32_t x = 0, row = 0;
  const bool in = work_to_pixel(P, pm, blockIdx.x * 256u + threadIdx.x, x, row);
  bool ok = true, est = false;  // (outside the image: no veto -- the window is clipped anyway)
  unsigned long long held = 0;
  double se2 = 0.0;
  if (in) {
    const size_t p = (size_t)row * P.nx + x;
    const uint32_t n = b.counts[p];
    held = n < a.k ? n : a.k;
    if (n != 0u) {
      const float* ev = b.errp + 3ull * p;
      const float e0 = ev[0], e1 = ev[1], e2 = ev[2];
      est = (__float_as_uint(e0) & 0x7f800000u) != 0x7f800000u && (__float_as_uint(e1) & 0x7f800000u) != 0x7f800000u &&
            (__float_as_uint(e2) & 0x7f800000u) != 0x7f800000u;
      ok = est && (double)e0 <= target2 && (double)e1 <= target2 && (double)e2 <= target2;
      if (est) se2 = ((double)e0 + (double)e1) + (double)e2;
    }
  }
  // (the bit plane and the partials as retire_mark_kernel writes them)
  const uint64_t m = __builtin_amdgcn_ballot_w64(ok);
  if (in && (lane & 7u) == 0u) reinterpret_cast<uint8_t*>(b.okbits + (size_t)row * b.pitch)[x >> 3] = (uint8_t)(m >> (lane & 56u));
  const uint32_t n_est = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(est));
  for (int off = 32; off > 0; off >>= 1) {
    held += __shfl_xor(held, off, 64);
    se2 += __shfl_xor(se2, off, 64);
  }
  if (lane == 0u) s_est[wave] = n_est, s_held[wave] = held, s_se2[wave] = se2;
  __syncthreads();
  if (threadIdx.x == 0u) {
    b.blk_u32[3u * blockIdx.x] = s_est[0] + s_est[1] + s_est[2] + s_est[3];
    b.blk_held[blockIdx.x] = s_held[0] + s_held[1] + s_held[2] + s_held[3];
    b.blk_se2[blockIdx.x] = ((s_se2[0] + s_se2[1]) + s_se2[2]) + s_se2[3];
  }
}

__global__ __launch_bounds__(256) void retire_apply_kernel(DevParams P, PixMap pm, RetireArgs a, RetireBufs b) {
  __shared__ uint32_t s_act[4], s_ret[4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  uint32_t x = 0, row = 0;
  const bool in = work_to_pixel(P, pm, blockIdx.x * 256u + threadIdx.x, x, row);
  bool cand = false, ret = false;
  if (in) {
    const size_t p = (size_t)row * P.nx + x;
    cand = b.counts[p] > a.k;
    if (cand && a.k >= a.min_samples) {
      const uint32_t r = a.radius;
      const uint32_t x0 = x > r ? x - r : 0u, x1 = x + r < P.nx ? x + r : P.nx - 1u;
      const uint32_t y0 = row > r ? row - r : 0u, y1 = row + r < P.ny ? row + r : P.ny - 1u;
      const uint32_t sh = x0 & 31u;
      const uint64_t want = (1ull << (x1 - x0 + 1u)) - 1ull;  // (x1 - x0 + 1 <= 17)
      const uint32_t* col = b.okbits + (x0 >> 5);
      ret = true;
      for (uint32_t y = y0; y <= y1 && ret; y++) {
        const uint32_t* w2 = col + (size_t)y * b.pitch;
        ret = (((((uint64_t)w2[1] << 32) | w2[0]) >> sh) & want) == want;
      }
      if (ret) b.counts[p] = a.k;
    }
  }
  const uint32_t n_act = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cand && !ret));
  const uint32_t n_ret = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ret));
  if (lane == 0u) s_act[wave] = n_act, s_ret[wave] = n_ret;
  __syncthreads();
  if (threadIdx.x == 0u) {
    b.blk_u32[3u * blockIdx.x + 1u] = s_act[0] + s_act[1] + s_act[2] + s_act[3];
    b.blk_u32[3u * blockIdx.x + 2u] = s_ret[0] + s_ret[1] + s_ret[2] + s_ret[3];
  }
}

// One workgroup of 256: thread t sums blocks t, t + 256, ... in index order, then a fixed tree over the threads.  Writes the
// out-fields of the rtg_retire block (words 4 .. 11: active, retired, estimated, reserved, sum_se2, samples_held); n_blk = 0
// (a rank that owns no tile) writes zeros.
__global__ __launch_bounds__(256) void retire_finish_kernel(uint32_t n_blk, RetireBufs b) {
  __shared__ uint32_t s_u[3][256];
  __shared__ unsigned long long s_held[256];
  __shared__ double s_se2[256];
  const uint32_t t = threadIdx.x;
  uint32_t est = 0, act = 0, ret = 0;
  unsigned long long held = 0;
  double se2 = 0.0;
  for (uint32_t i = t; i < n_blk; i += 256u) {
    est += b.blk_u32[3u * i], act += b.blk_u32[3u * i + 1u], ret += b.blk_u32[3u * i + 2u];
    held += b.blk_held[i];
    se2 += b.blk_se2[i];
  }
  s_u[0][t] = est, s_u[1][t] = act, s_u[2][t] = ret, s_held[t] = held, s_se2[t] = se2;
  __syncthreads();
  for (uint32_t h = 128u; h > 0u; h >>= 1) {
    if (t < h) {
      s_u[0][t] += s_u[0][t + h], s_u[1][t] += s_u[1][t + h], s_u[2][t] += s_u[2][t + h];
      s_held[t] += s_held[t + h];
      s_se2[t] += s_se2[t + h];
    }
    __syncthreads();
  }
  if (t == 0u) {
    const unsigned long long se2_bits = (unsigned long long)__double_as_longlong(s_se2[0]), h = s_held[0];
    uint32_t* o = b.block;
    o[4] = s_u[1][0], o[5] = s_u[2][0], o[6] = s_u[0][0], o[7] = 0u;
    o[8] = (uint32_t)se2_bits, o[9] = (uint32_t)(se2_bits >> 32);
    o[10] = (uint32_t)h, o[11] = (uint32_t)(h >> 32);
  }
}

}  // namespace rtg
