/* rtiow_gpu_image.h -- image textures of librtiow_gpu.so: a sampled image as a fourth texture kind beside constant, checker and
 * perlin of rtiow_gpu.h.  The reference's Texture is a closure of the hit point (texture.rs:6); the three kinds restate the
 * closures the reference itself makes.  A sampled image is the escape hatch for everything else: ordinary image assets (the
 * book's earth globe, a painted wall, a patterned light), and any closure of p baked to the caller's resolution.  Like the ray
 * queries (rtiow_gpu_query.h) and the ray frames (rtiow_gpu_rays.h) these entry points have no counterpart in a CPU
 * restatement of the renderer and are not part of the ABI of rtiow_gpu.h: bindings that mirror that header need not follow.
 *
 * The image.  w x h texels of three floats, row-major, ROW 0 AT THE TOP: the layout of the frames the library writes, so a
 * rendered frame is a texture as it stands.  Texel values are used as given, like a constant texture's colour.
 * 1 <= w, h <= 16384 and w * h <= 2^24.  The builder copies the texels.  (A scene whose images together hold 2^32 texels or more
 * is refused by rtg_scene_create with RTG_ERR_RANGE.)
 *
 * The value at a point p.  Everything is float32; every operation is rounded on its own (no contraction).
 *
 *   mapping 0 (planar):     u = ((p.x*m0 + p.y*m1) + p.z*m2) + m3
 *                           v = ((p.x*m4 + p.y*m5) + p.z*m6) + m7
 *   mapping 1 (spherical, the book's get_sphere_uv about a centre; m3 .. m7 must be 0):
 *                           d = p - (m0, m1, m2)
 *                           phi = rt_atan2f(d.z, d.x);  rho = sqrt(d.x*d.x + d.z*d.z);  theta = rt_atan2f(d.y, rho)
 *                           u = 0.5f - phi * INV_2PI;   v = 0.5f + theta * INV_PI
 *                           (INV_2PI, INV_PI: the float32 nearest to 1 / (2 pi) and 1 / pi)
 *   texel coordinates:      x = u * (float)w;  y = (1.0f - v) * (float)h
 *   filter 0 (nearest):     i = wrap(as_i32(floorf(x)), w);  j = wrap(as_i32(floorf(y)), h);  the value is texel[j][i]
 *   filter 1 (bilinear):    x = x - 0.5f;  y = y - 0.5f
 *                           fx = floorf(x);  tx = x - fx;  i0 = as_i32(fx);  i1 = i0 + 1 (in 64 bits);  likewise fy, ty, j0, j1
 *                           all four indices wrapped; per channel
 *                           a = t[j0][i0] + tx * (t[j0][i1] - t[j0][i0]);  b = the same on row j1;  out = a + ty * (b - a)
 *                           (this form, not (1 - t) * a + t * b: a constant image comes back exactly)
 *   as_i32:                 Rust's `as i32`: saturating, NaN -> 0
 *   wrap(i, n), in 64 bits: wrap 0 (repeat) = the Euclidean remainder of i by n;  wrap 1 (clamp) = min(max(i, 0), n - 1)
 *   rt_atan2f:              float64 inside (one divide, a polynomial, no libm call), rounded to float32 once; within 1 ulp of the
 *                           correctly rounded atan2; (+-0, +-0), the infinities and NaN as C's atan2f (csrc/rt_libm.h)
 *
 * NaN and infinities in p give whatever this arithmetic gives.  rtiow-rust_amd/image.py sample() and atan2f() are this
 * definition in numpy and the authority: the library equals them bit for bit, on the host and on the device.
 *
 * rtg_texture_image returns an ordinary texture id: it goes into rtg_material_lambertian, _isotropic and _diffuse_light, and
 * into rtg_texture_checker as either child.  (It takes two consecutive ids; the one behind the returned id names the record that
 * holds m and is refused wherever a texture id is expected.)  RTG_INVALID_ID, with the builder unchanged, for: a NULL argument;
 * a wrong struct_size; an unknown mapping, filter or wrap; reserved_in != 0; w or h outside the limits; mapping 1 with a
 * non-zero m3 .. m7.
 *
 * A scene with an image is a textured scene: it renders on the kernels that render checker and Perlin textures, with the same
 * bits on every one of them, and every frame kind, feature plane (the albedo plane shows the image), query and ray frame works
 * on it as on those.  rtg_scene_info's n_textures counts records, not texels; hbm_bytes includes the texels (16 bytes each).
 *
 * The probes.  rtg_debug_texture_host needs no GPU: image and constant textures, any other kind RTG_ERR_UNSUPPORTED.
 * rtg_debug_texture evaluates on the scene's device, one lane per point, through the function every kernel calls: every
 * texture kind.  rtg_debug_atan2f_host is rt_atan2f(y[i], x[i]) on the host; on the device it is rtg_debug_math op 6. */
#ifndef RTIOW_GPU_IMAGE_H
#define RTIOW_GPU_IMAGE_H
#include "rtiow_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtg_image_params {
  uint32_t struct_size;    /* = sizeof(rtg_image_params) */
  uint32_t mapping;        /* 0 = planar, 1 = spherical */
  uint32_t filter;         /* 0 = nearest, 1 = bilinear */
  uint32_t wrap_u, wrap_v; /* 0 = repeat, 1 = clamp */
  uint32_t reserved_in;    /* must be 0 */
  float m[8];
} rtg_image_params;

rtg_id rtg_texture_image(rtg_builder* b, const rtg_image_params* params, uint32_t w, uint32_t h, const float* rgb /* w*h*3 */);
/* host only, no GPU needed: the texture's value at n points (p: n x 3, out: n x 3) */
int rtg_debug_texture_host(rtg_builder* b, rtg_id texture, size_t n, const float* p, float* out);
/* on the scene's device, one lane per point */
int rtg_debug_texture(rtg_scene* s, rtg_id texture, size_t n, const float* p, float* out);
/* host only: rt_atan2f on n pairs */
int rtg_debug_atan2f_host(size_t n, const float* y, const float* x, float* out);

#ifdef __cplusplus
}
#endif
#endif /* RTIOW_GPU_IMAGE_H */
