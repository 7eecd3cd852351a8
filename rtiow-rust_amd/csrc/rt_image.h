// rt_image.h -- the image texture's sampler (include/rtiow_gpu_image.h), ONE host-and-device function: texture_eval (rt_trace.h)
// calls it on the GPU, rtg_debug_texture_host calls the very same source on the host, and rtiow-rust_amd/image.py sample() is the
// same arithmetic in numpy, bit for bit.  Compile with -ffp-contract=off: every operation is rounded on its own.
//
// Texels are plain global memory: float4 packets (r, g, b, -), row-major, row 0 at the top, one 16-byte load per texel.  No HIP
// texture objects: CDNA has no filtering hardware to lean on, and the bits must be the definition's.
#pragma once
#include <stdint.h>

#include "rt_libm.h"

namespace rtg {

// flag word of an image record (flat_scene.h TEX_IMAGE)
constexpr uint32_t IMG_SPHERICAL = 1u;  // mapping 1
constexpr uint32_t IMG_BILINEAR = 2u;   // filter 1
constexpr uint32_t IMG_CLAMP_U = 4u;    // wrap_u 1
constexpr uint32_t IMG_CLAMP_V = 8u;    // wrap_v 1
constexpr uint32_t IMG_MAX_SIDE = 16384u, IMG_MAX_TEXELS = 1u << 24;

struct alignas(16) ImgTexel {
  float r, g, b, pad;
};
struct ImgRgb {
  float r, g, b;
};

// Rust `as i32` (saturating, NaN -> 0): rt_trace.h f32_as_i32, for the host too
RT_LIBM_HD inline int32_t img_as_i32(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.0f) return 2147483647;
  if (f <= -2147483648.0f) return (int32_t)0x80000000;
  return (int32_t)f;
}

// wrap(i, n) and wrap(i + 1, n) of the definition, which computes both in 64 bits.  n <= 16384, so 32 bits give the same values:
// the Euclidean remainder of an int32 needs no wider type, the remainder of i + 1 is the remainder of i stepped once, and the
// clamp of i + 1 can only overflow where i >= n - 1 already decides it.
RT_LIBM_HD inline void img_wrap_pair(int32_t i, int32_t n, bool clamp, int32_t& w0, int32_t& w1) {
  if (clamp) {
    w0 = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    w1 = i >= n - 1 ? n - 1 : (i + 1 < 0 ? 0 : i + 1);
  } else {
    int32_t r = i % n;
    if (r < 0) r += n;
    w0 = r;
    w1 = r + 1 == n ? 0 : r + 1;
  }
}

RT_LIBM_HD inline ImgRgb image_sample(const ImgTexel* texels, uint32_t w, uint32_t h, uint32_t flags, const float m[8], float px, float py,
                                 float pz) {
  float u, v;
  if (flags & IMG_SPHERICAL) {  // the book's get_sphere_uv about the centre (m0, m1, m2)
    const float dx = px - m[0], dy = py - m[1], dz = pz - m[2];
    const float phi = rt_atan2f(dz, dx);
    const float rho = __builtin_sqrtf(dx * dx + dz * dz);
    const float theta = rt_atan2f(dy, rho);
    u = 0.5f - phi * 0x1.45f306p-3f;    // INV_2PI: the float32 nearest to 1 / (2 pi)
    v = 0.5f + theta * 0x1.45f306p-2f;  // INV_PI: the float32 nearest to 1 / pi
  } else {
    u = ((px * m[0] + py * m[1]) + pz * m[2]) + m[3];
    v = ((px * m[4] + py * m[5]) + pz * m[6]) + m[7];
  }
  float x = u * (float)w;
  float y = (1.0f - v) * (float)h;
  int32_t i0, i1, j0, j1;
  if (!(flags & IMG_BILINEAR)) {
    img_wrap_pair(img_as_i32(__builtin_floorf(x)), (int32_t)w, (flags & IMG_CLAMP_U) != 0u, i0, i1);
    img_wrap_pair(img_as_i32(__builtin_floorf(y)), (int32_t)h, (flags & IMG_CLAMP_V) != 0u, j0, j1);
    const ImgTexel t = texels[(uint32_t)j0 * w + (uint32_t)i0];
    return ImgRgb{t.r, t.g, t.b};
  }
  x = x - 0.5f, y = y - 0.5f;
  const float fx = __builtin_floorf(x), fy = __builtin_floorf(y);
  const float tx = x - fx, ty = y - fy;
  img_wrap_pair(img_as_i32(fx), (int32_t)w, (flags & IMG_CLAMP_U) != 0u, i0, i1);
  img_wrap_pair(img_as_i32(fy), (int32_t)h, (flags & IMG_CLAMP_V) != 0u, j0, j1);
  const ImgTexel t00 = texels[(uint32_t)j0 * w + (uint32_t)i0], t01 = texels[(uint32_t)j0 * w + (uint32_t)i1];
  const ImgTexel t10 = texels[(uint32_t)j1 * w + (uint32_t)i0], t11 = texels[(uint32_t)j1 * w + (uint32_t)i1];
  // a + t * (b - a), not (1 - t) * a + t * b: a constant image comes back exactly
  const float ar = t00.r + tx * (t01.r - t00.r), br = t10.r + tx * (t11.r - t10.r);
  const float ag = t00.g + tx * (t01.g - t00.g), bg = t10.g + tx * (t11.g - t10.g);
  const float ab = t00.b + tx * (t01.b - t00.b), bb = t10.b + tx * (t11.b - t10.b);
  return ImgRgb{ar + ty * (br - ar), ag + ty * (bg - ag), ab + ty * (bb - ab)};
}

}  // namespace rtg
