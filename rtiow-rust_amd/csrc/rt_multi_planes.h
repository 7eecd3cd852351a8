// rt_multi_planes.h -- the frame layout of the flagged framebuffers (include/rtiow_gpu.h RTG_FLAG_SUM_SQUARES .. RTG_FLAG_FEATURES)
// and the packed collective of rtg_par_cast_multi that carries every plane of such a frame (scene option multi_planes).
//
// Host part (plain C++, no HIP type: a host compiler builds it alone): where the blocks stand in a frame, which word ranges of
// it travel from a rank to the first device (PlaneSet), and where a word lies in the packed buffer.  Device part (hipcc only):
// pack_planes_kernel / unpack_planes_kernel, ONE launch per handle for all its planes.
#pragma once
#include <cstdint>

namespace rtg {

// ---- frame layout, in 32-bit words (64-bit arithmetic throughout) ------------------------------------------------------------
// A `Slice` is anything with the bool members squares / counts / retire / denoise / features (rtg_api.hip SampleSlice).

// RTG_FLAG_RETIRE: the retire block's word offset in the framebuffer (7 nx ny words of planes and counts, rounded up to an even
// word: 8-byte aligned)
inline uint64_t retire_block_word(uint32_t nx, uint32_t ny) { return ((uint64_t)7 * nx * ny + 1u) & ~1ull; }

// RTG_FLAG_DENOISE: the denoise block's word offset in the framebuffer -- the first even word behind the planes (6 nx ny words),
// the count plane (7 nx ny) or the retire block (its word + 16) -- the output plane 16 words behind it
inline uint64_t denoise_block_word(uint32_t nx, uint32_t ny, bool counts, bool retire) {
  if (retire) return retire_block_word(nx, ny) + 16u;
  return ((uint64_t)(counts ? 7 : 6) * nx * ny + 1u) & ~1ull;
}

// RTG_FLAG_FEATURES: the features block's word offset in the framebuffer -- the first even word behind everything the other
// flags put there: the float planes, the count plane, the retire block or the denoise output plane -- the albedo plane 16 words
// behind it, then the normal and the depth plane
template <typename Slice>
inline uint64_t features_block_word(uint32_t nx, uint32_t ny, const Slice& sl) {
  const uint64_t n = (uint64_t)nx * ny;
  uint64_t end = (sl.squares ? 6u : 3u) * n + (sl.counts ? n : 0u);
  if (sl.retire) end = retire_block_word(nx, ny) + 16u;
  if (sl.denoise) end = denoise_block_word(nx, ny, sl.counts, sl.retire) + 16u + 3u * n;
  return (end + 1u) & ~1ull;
}

// RTG_FLAG_DENOISE_ERROR (needs RTG_FLAG_DENOISE): the error plane's word offset in the framebuffer -- the first even word behind
// the denoise output plane or, with RTG_FLAG_FEATURES, behind the depth plane: the frame's old end
template <typename Slice>
inline uint64_t error_plane_word(uint32_t nx, uint32_t ny, const Slice& sl) {
  const uint64_t n = (uint64_t)nx * ny;
  uint64_t end = denoise_block_word(nx, ny, sl.counts, sl.retire) + 16u + 3u * n;
  if (sl.features) end = features_block_word(nx, ny, sl) + 16u + 7u * n;
  return (end + 1u) & ~1ull;
}

// ---- what travels ------------------------------------------------------------------------------------------------------------
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

template <typename Slice>
inline PlaneSet make_plane_set(uint32_t nx, uint32_t ny, const Slice& sl, bool features_compute) {
  PlaneSet ps{};
  const uint64_t n = (uint64_t)nx * ny;
  auto add = [&](uint64_t first, uint32_t wpp) {
    ps.g[ps.n_groups++] = PlaneGroup{first, wpp, ps.words_per_pixel};
    ps.words_per_pixel += wpp;
  };
  add(0u, 3u);
  if (sl.squares) add(3u * n, 3u);
  if (sl.features && features_compute) {
    const uint64_t albedo = features_block_word(nx, ny, sl) + 16u;
    add(albedo, 3u), add(albedo + 3u * n, 3u), add(albedo + 6u * n, 1u);
  }
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

// Work item w of the rank P.rank -> its pixel (rt_pool.h work_to_pixel, as pack_tiles_kernel): every word of every travelling
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
