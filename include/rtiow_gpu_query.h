/* rtiow_gpu_query.h -- ray queries of librtiow_gpu.so: closest hit and occlusion for the CALLER's rays, against a scene made
 * with rtiow_gpu.h.  These entry points have no counterpart in a CPU restatement of the renderer (the reference has no ray
 * queries) and are not part of the ABI of rtiow_gpu.h: bindings that mirror that header need not follow this one.
 *
 * Both queries are the renderer's own walks over the scene's flat program, so what they answer is what a frame would see:
 *   closest   one World::hit_top over [t_min, f32::MAX)
 *   occluded  is anything hit in [t_min, t_max)?  hit_top's predicates and visiting order, ended at the first accepted hit
 * A ConstantMedium takes part in both with a free-path draw from the ray's own stream of the counter RNG: stream
 * (seed, first_index + i, sample 0), event 1 -- the stream rtg_debug_hit_top gives ray i.  Nothing else draws. */
#ifndef RTIOW_GPU_QUERY_H
#define RTIOW_GPU_QUERY_H
#include "rtiow_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtg_query_params {
  uint32_t struct_size;  /* = sizeof(rtg_query_params) */
  uint32_t reserved;     /* must be 0 */
  uint64_t seed;         /* media draw from the counter RNG keyed (seed, first_index + i, sample 0), event 1 */
  uint64_t first_index;  /* RNG index of ray 0: a batch split into calls gives the bits of one call */
  float t_min;           /* range start of every ray (the reference's NEAR = 0.001) */
  uint32_t reserved2;    /* must be 0 */
} rtg_query_params;

/* Closest hit.  rays7: n x 7 floats (origin.xyz, direction.xyz, time), rtg_debug_hit_top's layout; the direction need not be
 * normalised, t is in units of it.  out8: n x 8 floats (hit ? 1 : 0, t, p.xyz, normal.xyz), zeros on a miss; out_material: n
 * material handles, 0xffffffff on a miss.  With first_index = 0 every output word is the one rtg_debug_hit_top(seed, t_near =
 * t_min) writes for the same rays, bit for bit, on every scene.
 *
 * Occlusion.  rays8: n x 8 floats, the eighth the ray's own t_max.  out[i] = 1 when anything is hit in [t_min, t_max), else 0.
 * A ConstantMedium blocks with probability 1 - transmittance (its own draw: an unbiased estimate of the transmittance).  A
 * ray with !(t_max > t_min) (a NaN t_max included) gives 0 without a walk.
 *
 * The _device variants read and write device memory of the scene's device, enqueue on hip_stream, allocate nothing, keep no
 * per-call state in the scene handle and do not synchronise: two calls on two streams may overlap.  A non-NULL stats makes the
 * call synchronous (as for rtg_par_cast_device) and fills kernel_ms and rays = n; the other counters stay 0.
 * The host variants take host pointers: temporary device buffers, the device variant on the default stream, one synchronise,
 * the copies back.
 *
 * Refused with RTG_ERR_INVALID, nothing written and nothing enqueued: a NULL scene or params; a NULL rays / output pointer with
 * n > 0; a wrong struct_size (params, stats); a non-zero reserved field; first_index + n > 2^32 (the RNG index is 32 bits); a
 * NaN t_min.  n = 0 is RTG_OK and enqueues nothing.  Without a HIP device: RTG_ERR_DEVICE (there is no CPU fallback).
 *
 * Which kernel answers is the scene option "query_lds" (rtg_scene_set_option): 0 = always the general kernel (one lane per
 * ray, the program read from global memory; every program the library can flatten); 2 = the lean kernel whenever the program
 * is lean (BOX / SPHERE / END records: book-1) and fits a CU's LDS -- every workgroup walks its own LDS copy of the program;
 * 1 (default) = automatic, the kernel measured to be the faster one: at present always the general kernel (the lean one is
 * ahead only on large batches of incoherent rays, about 20 % at a million; DESIGN.md "Ray queries").  The answer does not
 * depend on the choice: the same bits. */
int rtg_query_closest(rtg_scene* s, size_t n, const float* rays7, const rtg_query_params* params, float* out8,
                      uint32_t* out_material, rtg_stats* stats_or_null);
int rtg_query_closest_device(rtg_scene* s, size_t n, const float* d_rays7, const rtg_query_params* params, float* d_out8,
                             uint32_t* d_out_material, void* hip_stream, rtg_stats* stats_or_null);
int rtg_query_occluded(rtg_scene* s, size_t n, const float* rays8, const rtg_query_params* params, uint8_t* out,
                       rtg_stats* stats_or_null);
int rtg_query_occluded_device(rtg_scene* s, size_t n, const float* d_rays8, const rtg_query_params* params, uint8_t* d_out,
                              void* hip_stream, rtg_stats* stats_or_null);

#ifdef __cplusplus
}
#endif
#endif /* RTIOW_GPU_QUERY_H */
