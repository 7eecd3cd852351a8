/* rtiow_gpu_debug.h -- host-only inspection entry points of librtiow_gpu.so that have no counterpart in a CPU restatement of
 * the renderer and are not part of the ABI of rtiow_gpu.h (bindings that mirror that header need not follow this one). */
#ifndef RTIOW_GPU_DEBUG_H
#define RTIOW_GPU_DEBUG_H
#include "rtiow_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The box plan of a lean program (BOX / SPHERE / END records; csrc/rt_box_plan.h), from the function rtg_scene_create calls
 * for the production image of the lean pool kernel: mask_out[i] = 0 record i is kept, 1 it is a box-chain follower (the rule
 * rtg_scene_info's n_box_followers counts), 2 it is an interior BOX the plan leaves out (scene option "box_prune").  Every
 * other program gets zeros.  (rtg_scene_create itself makes no plan for a program whose image cannot fit a CU's LDS even
 * without its interior boxes -- such a program is never staged; this entry point plans every lean program.)
 * The program is `world` flattened by `b`, as rtg_debug_flatten does -- or, when `words` is not NULL, the n_records x 8 words
 * given (the layout rtg_debug_flatten writes; b and world are then ignored).
 * Writes min(record count, capacity) bytes; returns the record count, or a negative rtg_status.  Works without a GPU. */
int rtg_debug_box_plan(rtg_builder* b, const rtg_id* world, size_t n, const uint32_t* words, size_t n_records,
                       uint8_t* mask_out, size_t capacity);

/* The production program of a lean program (csrc/rt_box_plan.h box_tree_rebuild; scene option "box_tree"): the program that
 * production launches of the lean pool kernel stage -- every maximal Bvh region rebuilt over the same leaf order, everything
 * else copied.  The program is given as for rtg_debug_box_plan.  words_out: record count x 8 words in rtg_debug_flatten's
 * layout; origin_out[i]: the record of the given program that record i copies, 0xffffffff for a new interior BOX; mask_out:
 * the plan over the production program (0 / 1 / 2 as above).  Another kind of program comes back unchanged, with
 * origin_out[i] = i and zeros.  Each array may be NULL; min(record count, capacity) records are written.  Returns the record
 * count, or a negative rtg_status.  Works without a GPU. */
int rtg_debug_production_program(rtg_builder* b, const rtg_id* world, size_t n, const uint32_t* words, size_t n_records,
                                 uint32_t* words_out, uint32_t* origin_out, uint8_t* mask_out, size_t capacity);

/* The camera plan of a lean program (scene option "box_camera"; csrc/rt_box_plan.h BOX_PLAN_COUNTS): the plan the launcher makes
 * from the pass counts of its probe kernel, here from counts handed in.  The program is given as for rtg_debug_box_plan and
 * planned as it stands (hand in rtg_debug_production_program's words to plan what production launches stage).  counts: one
 * word per record, the number of probe walks out of n_rays in which that BOX passed (ignored for other records); any values are
 * accepted, and every mask that comes back is a sound plan.  mask_out as for rtg_debug_box_plan.  Writes min(record count,
 * capacity) bytes; returns the record count, or a negative rtg_status.  Works without a GPU. */
int rtg_debug_camera_plan(rtg_builder* b, const rtg_id* world, size_t n, const uint32_t* words, size_t n_records,
                          const uint32_t* counts, uint64_t n_rays, uint8_t* mask_out, size_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* RTIOW_GPU_DEBUG_H */
