/* rtiow_gpu_mesh.h -- triangles and triangle meshes of librtiow_gpu.so: a third primitive beside the Sphere and the Rect of
 * rtiow_gpu.h.  The reference's geometry is spheres, axis-aligned rects and what `And` and the wrappers make of them; a triangle
 * is the escape hatch for everything else, as the sampled image of rtiow_gpu_image.h is on the texture side.  Like the ray
 * queries, the ray frames and the image textures these entry points have no counterpart in a CPU restatement of the renderer and
 * are not part of the ABI of rtiow_gpu.h: bindings that mirror that header need not follow.
 *
 * The definition.  Everything is float32; every operation is rounded on its own (no contraction).
 *
 *   cross(a, b) = (a.y*b.z - a.z*b.y,  a.z*b.x - a.x*b.z,  a.x*b.y - a.y*b.x)      each product rounded before the subtraction
 *   dot(a, b)   = (a.x*b.x + a.y*b.y) + a.z*b.z
 *
 *   the record of (v0, v1, v2):   e1 = v1 - v0;  e2 = v2 - v0;  c = cross(e1, e2);  len = sqrt((c.x*c.x + c.y*c.y) + c.z*c.z)
 *                                 N = c / len  (three divides).  A counter-clockwise winding gives the front face.
 *   the hit of ray (o, d) over [t_min, t_max)  (Moeller-Trumbore, in this order):
 *                                 pv = cross(d, e2);  det = dot(e1, pv);  inv = 1.0f / det;  tv = o - v0
 *                                 u = dot(tv, pv) * inv;  qv = cross(tv, e1);  v = dot(d, qv) * inv;  t = dot(e2, qv) * inv
 *                                 accepted if and only if  u >= 0 && v >= 0 && u + v <= 1 && t >= t_min && t < t_max
 *                                 (positive predicates: a zero or NaN det misses; both edges inclusive: a shared edge is covered
 *                                 twice rather than cracked; no watertightness is claimed)
 *   the hit record:               p = o + t * d;  normal = N, or -N under an odd number of FlipNormals.  Two-sided like Rect: the
 *                                 normal never turns towards the ray.
 *   the bounding box:             per axis min(v0, v1, v2) - 0.0001f and max(v0, v1, v2) + 0.0001f: Rect's pad on every axis.
 *
 * rtiow-rust_amd/triangle.py is this definition in numpy and the authority: the library equals it bit for bit, on the host
 * (rtg_debug_triangle_host) and on the device (rtg_debug_hit_top and the ray queries answer hits for any scene).
 *
 * rtg_object_triangle returns an ordinary object id: it goes into every wrapper, `And`, rtg_object_bvh / _bvh_sah,
 * rtg_object_constant_medium (as part of a boundary graph: a closed mesh bounds a medium) and a world list.  RTG_INVALID_ID, with
 * the builder unchanged, for: a NULL argument; a bad material; a vertex coordinate that is not finite; a normal whose len is 0
 * or not finite (scale such a mesh with rtg_object_scale instead).
 *
 * rtg_object_mesh makes the n_triangles triangle objects (triangle t has the vertices indices[3t], [3t + 1], [3t + 2] of the
 * n_vertices x 3 floats), then one Bvh object over them: sah = 0 Bvh::new's median split (rtg_object_bvh), sah = 1 the SAH builder
 * (rtg_object_bvh_sah), exposure (0, 0) because nothing inside moves -- exactly what the caller would get from those calls.  It
 * refuses as a whole, with the builder unchanged: a NULL argument, an index >= n_vertices, any triangle rtg_object_triangle would
 * refuse, n_triangles == 0 (RTG_ERR_EMPTY_BVH's message) or sah > 1.
 *
 * Per-vertex normals and UVs are not part of this header: textures are functions of p and work on a mesh as they stand;
 * rtiow_gpu_surface.h adds them (rtg_object_triangle_attr, rtg_object_mesh_attr) and textures that follow the surface.  A
 * DiffuseLight on a triangle emits, and is found by scattered rays at full weight; scene option light_sampling never samples it.
 *
 * Which kernels.  A scene that holds a triangle is a full-feature scene: camera frames render on the full-feature ray-pool
 * kernel or the lock-step kernel, with the same bits as on the one-lane kernel (scene option kernel = 1); it has no second
 * program (the pool-2 kernel never takes it), a frame with RTG_FLAG_SAMPLE_COUNTS renders on the one-lane kernel, and queries,
 * ray frames and the feature pass run one lane per ray as for every full-feature scene.  rtg_stats.prim_tests counts one per
 * triangle test.
 *
 * rtg_debug_triangle_host needs no GPU: for n (triangle, ray) pairs -- tri9: v0, v1, v2; rays8: o, d, time (unused), t_max --
 * it writes (hit, t, p.xyz, n.xyz) through the function the kernels call, zeros on a miss.  A triangle rtg_object_triangle would
 * refuse is evaluated as it stands (its N is whatever c / len gives). */
#ifndef RTIOW_GPU_MESH_H
#define RTIOW_GPU_MESH_H
#include "rtiow_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif

rtg_id rtg_object_triangle(rtg_builder* b, const float v0[3], const float v1[3], const float v2[3], rtg_id material);
rtg_id rtg_object_mesh(rtg_builder* b, const float* vertices, size_t n_vertices, const uint32_t* indices, size_t n_triangles, rtg_id material, uint32_t sah);
int rtg_debug_triangle_host(size_t n, const float* tri9, const float* rays8, float t_min, float* out8);

#ifdef __cplusplus
}
#endif
#endif /* RTIOW_GPU_MESH_H */
