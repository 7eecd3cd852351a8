// rt_multi_planes.h -- the frame layout of the flagged framebuffers (include/rtiow_gpu.h RTG_FLAG_SUM_SQUARES .. RTG_FLAG_FEATURES)
// and the packed collective of rtg_par_cast_multi that carries every plane of such a frame (scene option multi_planes).
//
// Host part (plain C++, no HIP type: a host compiler builds it alone): where the parts of a frame stand (FrameLayout), which byte
// ranges of it rtg_par_cast uploads and copies back (Extents), which word ranges travel from a rank to the first device
// (PlaneSet), and where a word lies in the packed buffer.  Device part (hipcc only):
// pack_planes_kernel / unpack_planes_kernel, ONE launch per handle for all its planes.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/rtiow_gpu.h"

namespace rtg {

// ---- frame layout, in 32-bit words (64-bit arithmetic throughout) ------------------------------------------------------------
// Where every part of a framebuffer starts: the one rule of include/rtiow_gpu.h, field for field what capi.FrameLayout (the
// binding) computes.  Built once per call from (nx, ny, flags); it belongs to the FRAME, whichever slice of it a launch renders.
// The float planes (one, or two with squares) start at word 0; behind them, each only with its flag: the count plane, the retire
// block, the denoise block and its output plane (3n), the features block and the albedo (3n), normal (3n) and depth (n) planes
// and the error plane (3n) and, at the very end, the background block of RTG_FLAG_BACKGROUND (in-only: it never travels back).
// A block is BLOCK_WORDS long; blocks and the error plane start on an even word (8-byte aligned).  RTG_FLAG_RETIRE implies the count plane and the squares, RTG_FLAG_DENOISE the squares (check_params refuses
// a call without them).  A part the frame does not have is ABSENT.
struct FrameLayout {
  static constexpr uint64_t ABSENT = ~0ull;
  static constexpr uint64_t BLOCK_WORDS = 16;
  uint64_t n = 0;           // pixels
  bool squares = false;     // two float planes
  uint64_t counts = ABSENT, retire = ABSENT, denoise = ABSENT, denoised = ABSENT;
  uint64_t features = ABSENT, albedo = ABSENT, normal = ABSENT, depth = ABSENT;
  uint64_t error = ABSENT;
  uint64_t background = ABSENT;
  uint64_t words = 0;       // the whole frame

  FrameLayout(uint32_t nx, uint32_t ny, uint32_t flags)
      : n((uint64_t)nx * ny), squares((flags & (RTG_FLAG_SUM_SQUARES | RTG_FLAG_RETIRE | RTG_FLAG_DENOISE)) != 0u) {
    auto even = [](uint64_t w) { return (w + 1u) & ~1ull; };
    uint64_t w = planes();
    if (flags & (RTG_FLAG_SAMPLE_COUNTS | RTG_FLAG_RETIRE)) counts = w, w += n;
    if (flags & RTG_FLAG_RETIRE) retire = even(w), w = retire + BLOCK_WORDS;
    if (flags & RTG_FLAG_DENOISE) denoise = even(w), denoised = denoise + BLOCK_WORDS, w = denoised + 3u * n;
    if (flags & RTG_FLAG_FEATURES) {
      features = even(w), albedo = features + BLOCK_WORDS;
      normal = albedo + 3u * n, depth = albedo + 6u * n, w = depth + n;
    }
    if (flags & RTG_FLAG_DENOISE_ERROR) error = even(w), w = error + 3u * n;
    if (flags & RTG_FLAG_BACKGROUND) background = even(w), w = background + BLOCK_WORDS;
    words = w;
  }
  static bool has(uint64_t part) { return part != ABSENT; }
  uint64_t planes() const { return (squares ? 6u : 3u) * n; }  // the float planes' words
  uint64_t plane() const { return 3u * n; }                     // one float plane: the output and the error plane's words too
  uint64_t feature_planes() const { return 7u * n; }            // albedo, normal and depth together
  // the end of everything in front of the features block
  uint64_t in_end() const { return has(denoise) ? denoised + plane() : has(retire) ? retire + BLOCK_WORDS : has(counts) ? counts + n : planes(); }
  // `part` of the frame at `base` (nullptr: the frame has no such part)
  template <typename T>
  T* at(T* base, uint64_t part) const {
    static_assert(sizeof(T) == 4, "a frame is 32-bit words");
    return has(part) ? base + part : nullptr;
  }
};

// ---- what rtg_par_cast moves around rtg_par_cast_device (and rtg_par_cast_multi's flagged frames around their ranks) ---------
// Byte ranges [lo, hi) of a frame, ascending and disjoint, at most seven
struct Extents {
  struct { uint64_t lo, hi; } e[7];
  int n = 0;
  void add(uint64_t lo_word, uint64_t hi_word, uint64_t lo_byte = 0, uint64_t hi_byte = 0) {
    const uint64_t lo = 4u * lo_word + lo_byte, hi = 4u * hi_word + hi_byte;
    if (hi > lo) e[n].lo = lo, e[n].hi = hi, n++;
  }
};
// What travels to the device before the call.  `other_ranks` (nranks > 1): pixels of other ranks must come back as the caller
// left them.  A single rank overwrites every pixel -- unless it resumes a progressive frame (`begin` > 0), whose running sums are
// in the frame, or renders per-pixel counts (pixels with n_p = 0 stay as they are).  Under RTG_FLAG_SAMPLE_COUNTS the count plane
// travels with the float planes, under RTG_FLAG_RETIRE / RTG_FLAG_DENOISE their blocks (and the output plane: pixels with
// e_p = 0 keep what it held); the error plane of RTG_FLAG_DENOISE_ERROR whenever the output plane travels; the background
// block of RTG_FLAG_BACKGROUND always.
inline Extents upload_extents(const FrameLayout& L, bool other_ranks, uint32_t begin, uint32_t features_compute) {
  Extents x;
  const bool keeps = other_ranks || begin != 0u || L.has(L.counts);
  if (keeps) x.add(0, L.in_end());
  else if (L.has(L.denoise)) x.add(L.denoise, L.denoised);  // (the block alone: a whole frame without counts writes every pixel of every plane)
  // the features block; the planes too when the call does not trace them and the guided filter reads them -- and whenever other
  // ranks' pixels must come back as the caller left them
  if (L.has(L.features)) x.add(L.features, L.albedo + (other_ranks || (features_compute == 0u && L.has(L.denoise)) ? L.feature_planes() : 0u));
  if (L.has(L.error) && keeps) x.add(L.error, L.error + L.plane());
  if (L.has(L.background)) x.add(L.background, L.words);  // (rtg_par_cast_device reads the in-fields from the device frame)
  return x;
}
// ... and back afterwards: the float planes; under RTG_FLAG_RETIRE the count plane and the block's out-fields (active ..
// samples_held); under RTG_FLAG_DENOISE the out-fields (filtered .. reserved) and the output plane behind them; under
// RTG_FLAG_FEATURES the out-fields (traced .. reserved) and, when this call traced them, the planes behind them; under
// RTG_FLAG_DENOISE_ERROR the error plane
inline Extents copy_back_extents(const FrameLayout& L, uint32_t features_compute) {
  Extents x;
  x.add(0, L.has(L.retire) ? L.counts + L.n : L.planes());
  if (L.has(L.retire)) x.add(L.retire, L.retire, offsetof(rtg_retire, active), offsetof(rtg_retire, reserved2));
  if (L.has(L.denoise)) x.add(L.denoise, L.in_end(), offsetof(rtg_denoise, filtered));
  if (L.has(L.features)) x.add(L.features, L.albedo + (features_compute ? L.feature_planes() : 0u), offsetof(rtg_features, traced));
  if (L.has(L.error)) x.add(L.error, L.error + L.plane());
  return x;
}

// ---- what travels between the devices ----------------------------------------------------------------------------------------
// The planes a rank of a multi_planes call writes, as groups (first word of the plane in the frame, words per pixel): the sum
// (3), under RTG_FLAG_SUM_SQUARES the squares (3), under RTG_FLAG_FEATURES with compute = 1 the albedo (3), the normal (3) and
// the depth (1).  The count plane, the blocks and the denoise output plane never travel: the count plane is the caller's input,
// the rest is written on the first device.  words_per_pixel = the sum of the groups' widths, 3 .. 13.
constexpr uint32_t PLANE_GROUPS = 5;
struct PlaneGroup {
  uint64_t first;  // word offset of the plane in the frame
  uint32_t wpp;    // its words per pixel: 3 or 1
  uint32_t k0;     // the packed word index of its first word (the widths of the groups before it)
};
struct PlaneSet {
  PlaneGroup g[PLANE_GROUPS];
  uint32_t n_groups;
  uint32_t words_per_pixel;
};

inline PlaneSet make_plane_set(const FrameLayout& L, bool features_compute) {
  PlaneSet ps{};
  auto add = [&](uint64_t first, uint32_t wpp) {
    ps.g[ps.n_groups++] = PlaneGroup{first, wpp, ps.words_per_pixel};
    ps.words_per_pixel += wpp;
  };
  add(0u, 3u);
  if (L.squares) add(L.plane(), 3u);
  if (L.has(L.features) && features_compute) add(L.albedo, 3u), add(L.normal, 3u), add(L.depth, 1u);
  return ps;
}

// The packed buffer is PLANE-MAJOR: word k (0 .. words_per_pixel - 1) of work item w (0 .. pix_work - 1) lies at k * pix_work + w,
// so the lanes of a wave -- consecutive work items -- read and write consecutive dwords of it, whatever the planes' widths.
inline
#ifdef __HIPCC__
    __host__ __device__
#endif
    uint64_t
    packed_word(uint32_t k, uint32_t w, uint32_t pix_work) {
  return (uint64_t)k * pix_work + w;
}
// ... and where that word lies in the frame, for the pixel with raster index `pix`
inline
#ifdef __HIPCC__
    __host__ __device__
#endif
    uint64_t
    frame_word(const PlaneGroup& g, uint32_t c, uint64_t pix) {
  return g.first + (uint64_t)g.wpp * pix + c;
}

}  // namespace rtg

#ifdef __HIPCC__
#include "rt_pool.h"

namespace rtg {

// Work item w of the rank P.rank -> its pixel (rt_pool.h work_to_pixel; items beyond the image are padding): every word of every travelling
// plane of that pixel, frame -> packed.  On the frame side the lanes of a wave follow the 8-pixel row segments of an 8x8 block
// (96 contiguous bytes per segment of a 3-word plane); on the packed side they are consecutive dwords.  Padding items (beyond the
// image) pack +0.  The loops are fully unrolled over the at most 5 x 3 words, so the PlaneSet stays in the kernel arguments.
__global__ __launch_bounds__(256) void pack_planes_kernel(DevParams P, PixMap pm, uint32_t pix_work, PlaneSet ps, const uint32_t* __restrict__ frame,
                                                          uint32_t* __restrict__ packed) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= pix_work) return;
  uint32_t x, row;
  const bool in = work_to_pixel(P, pm, w, x, row);
  const uint64_t pix = (uint64_t)row * P.nx + x;
#pragma unroll
  for (uint32_t g = 0; g < PLANE_GROUPS; g++) {
    if (g < ps.n_groups) {
#pragma unroll
      for (uint32_t c = 0; c < 3u; c++)
        if (c < ps.g[g].wpp) packed[packed_word(ps.g[g].k0 + c, w, pix_work)] = in ? frame[frame_word(ps.g[g], c, pix)] : 0u;
    }
  }
}

// ... and packed -> frame on the first device; padding items are skipped
__global__ __launch_bounds__(256) void unpack_planes_kernel(DevParams P, PixMap pm, uint32_t pix_work, PlaneSet ps, uint32_t* __restrict__ frame,
                                                            const uint32_t* __restrict__ packed) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w >= pix_work) return;
  uint32_t x, row;
  if (!work_to_pixel(P, pm, w, x, row)) return;
  const uint64_t pix = (uint64_t)row * P.nx + x;
#pragma unroll
  for (uint32_t g = 0; g < PLANE_GROUPS; g++) {
    if (g < ps.n_groups) {
#pragma unroll
      for (uint32_t c = 0; c < 3u; c++)
        if (c < ps.g[g].wpp) frame[frame_word(ps.g[g], c, pix)] = packed[packed_word(ps.g[g].k0 + c, w, pix_work)];
    }
  }
}

}  // namespace rtg
#endif  // __HIPCC__
