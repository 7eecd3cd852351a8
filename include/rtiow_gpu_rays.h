/* rtiow_gpu_rays.h -- ray frames of librtiow_gpu.so: path-trace the CALLER's rays against a scene made with rtiow_gpu.h.  The
 * ray queries (rtiow_gpu_query.h) answer "what does this ray hit?"; a ray frame answers "what radiance arrives along it?" --
 * color() (lib.rs:60-101) on a ray the caller supplies, folded into a frame like rtg_par_cast's.  That is what a fisheye,
 * equirectangular, orthographic or stereo camera, an irradiance probe, a baked lightmap or a second bounce continued from the
 * caller's own first hit needs.  Like the queries these entry points have no counterpart in a CPU restatement of the renderer
 * and are not part of the ABI of rtiow_gpu.h: bindings that mirror that header need not follow this one.
 *
 * Rays and pixels.  rays7 has the layout of rtg_query_closest: 7 floats per ray (origin.xyz, direction.xyz, time); directions
 * need not be normalised.  Pixel p = row * nx + x, row 0 = top: the layout of out.  Every ray offset is computed in 64 bits.
 *
 * A sample.  Sample s of pixel (x, row), with y = ny - 1 - row, is color() on the pixel's ray with the counter RNG's stream
 * SampleRng::init(seed, y * nx + x, s).  No event-0 draw is made (those are the camera's); color()'s first draw is the first
 * word of event 1, exactly as for a camera ray.  t_near, max_bounces and seed come from rtg_params.  The pixel is the
 * reference's fold (lib.rs:365-374): left to right from +0 over s = 0 .. ns - 1, then divided by (float)ns.
 *
 * Parity.  With rays equal to the camera's own (RTG_RAYS_PER_SAMPLE) every word of out equals what rtg_par_cast writes for
 * that camera and those params, bit for bit, on every scene.
 *
 * Flags honoured, with the meaning and the frame layout rtiow_gpu.h gives them: RTG_FLAG_PARTIAL; RTG_FLAG_RESUME with
 * sample_begin (only rays of samples [sample_begin, ns) are read; a per-sample array still covers [0, ns));
 * RTG_FLAG_SUM_SQUARES (plane 1); RTG_FLAG_BACKGROUND (the block at the frame's end).  tile_w, tile_h, rank and nranks as in
 * rtg_par_cast: pixels of other ranks stay untouched, so a ray frame can be sharded over devices.
 *
 * Refused with RTG_ERR_UNSUPPORTED, nothing written or enqueued: RTG_FLAG_COUNTERS, TRACE_KERNEL, SAMPLE_COUNTS, RETIRE,
 * DENOISE, FEATURES, DENOISE_ERROR (and any flag bit this header does not name); a handle with scene option light_sampling = 1.
 * Refused with RTG_ERR_INVALID, nothing written or enqueued: ray_mode > 1; a NULL scene, params, rays or out; a wrong
 * struct_size (params, stats); nx, ny or ns = 0; sample_begin > ns; what the honoured flags and the tile / rank fields refuse
 * in rtg_par_cast.  Without a HIP device: RTG_ERR_DEVICE (there is no CPU fallback).
 *
 * NaN, infinite and zero rays are not screened: they walk as a scattered ray with those values would, and the path loop is
 * bounded by max_bounces.
 *
 * Stats: kernel_ms (the fold kernel included where one runs) and samples = owned pixels x (ns - sample_begin); the counters
 * stay 0.
 *
 * rtg_par_cast_rays_device reads and writes device memory of the scene's device and enqueues on hip_stream.  It allocates
 * nothing per call beyond what rtg_par_cast_device does, is asynchronous unless stats are requested, and synchronises only
 * where rtg_par_cast_device does: the read-back of the background block.  rtg_par_cast_rays takes host pointers: the rays in
 * a temporary device buffer, the frame staged under rtg_par_cast's upload rules (untouched pixels survive under RESUME and
 * nranks > 1), the device variant on the default stream.
 *
 * Which kernel renders is the scene option "ray_pool" (rtg_scene_set_option): 1 (default) = lean programs (BOX / SPHERE / END
 * records: book-1 and its kin) on the lean pool kernel, whose END pass loads the caller's ray where a camera frame draws its
 * own; 0 = always the general kernel (one lane per pixel; every program the library can flatten).  Every other program takes
 * the general kernel whatever the option says: the three full-feature schedules (the full-feature pool kernel, the pool-2
 * kernel, the lock-step kernel) do not render ray frames yet, so Cornell- and book-2-like scenes pay the gap between those
 * kernels and the one-lane-per-pixel walk (DESIGN.md "Ray frames" has the measured figures).  The result does not depend on the
 * choice: the same bits.  Option "verbose" names the kernel a ray frame took. */
#ifndef RTIOW_GPU_RAYS_H
#define RTIOW_GPU_RAYS_H
#include "rtiow_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RTG_RAYS_PER_PIXEL 0u  /* rays7 holds nx*ny rays: ray p starts every sample of pixel p */
#define RTG_RAYS_PER_SAMPLE 1u /* rays7 holds ns*nx*ny rays, sample-major: sample s of pixel p at s*nx*ny+p */

int rtg_par_cast_rays(rtg_scene* s, const float* rays7, uint32_t ray_mode, const rtg_params* params, float* out_rgb,
                      rtg_stats* stats_or_null);
int rtg_par_cast_rays_device(rtg_scene* s, const float* d_rays7, uint32_t ray_mode, const rtg_params* params, float* d_out_rgb,
                             void* hip_stream, rtg_stats* stats_or_null);

#ifdef __cplusplus
}
#endif
#endif /* RTIOW_GPU_RAYS_H */
