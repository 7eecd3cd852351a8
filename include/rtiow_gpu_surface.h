/* rtiow_gpu_surface.h -- surface attributes of librtiow_gpu.so: per-vertex normals and UVs on the triangles of rtiow_gpu_mesh.h,
 * and textures evaluated at a hit's surface coordinates instead of its world point.  A mesh with vertex normals shades smooth
 * (a 320-triangle icosphere looks like the sphere it approximates), and an image follows the surface it is mapped on, whatever
 * wrappers move the mesh.  Like rtiow_gpu_mesh.h these entry points have no counterpart in a CPU restatement of the renderer and
 * are not part of the ABI of rtiow_gpu.h: bindings that mirror that header need not follow.
 *
 * The definition.  Everything is float32; every operation is rounded on its own (no contraction).  u, v are the very floats
 * Moeller-Trumbore's accept test used (rtiow_gpu_mesh.h), N the face normal of the record, n0 n1 n2 the vertex normals and
 * (u0, v0) (u1, v1) (u2, v2) the vertex UVs of v0 v1 v2:
 *
 *   w   = (1.0f - u) - v
 *   s   = (w*n0 + u*n1) + v*n2                 per component, each product rounded, left to right
 *   len = sqrt((s.x*s.x + s.y*s.y) + s.z*s.z)
 *   n   = s / len  (three divides)             if len > 0 && len <= f32::MAX   (positive form: NaN falls through)
 *       = N                                    otherwise
 *   normal = n, or -n under an odd number of FlipNormals
 *   tu  = (w*u0 + u*u1) + v*u2;  tv likewise   the surface coordinates of the hit
 *
 * rtiow-rust_amd/triangle.py (shade, closest_attr) is this definition in numpy and the authority: the library equals it bit for
 * bit, on the host (rtg_debug_triangle_attr_host) and on the device (rtg_debug_hit_surface answers for any scene).
 *
 * Normals.  Vertex normals are used as given: not normalised at build time, not turned towards either side of the face.  The hit
 * normal is the SHADING normal everywhere a hit normal is used: scatter, light sampling, the feature planes, rtg_query_closest.
 * Wrappers treat it as they treat any hit normal: RotateY rotates it, Scale divides it without renormalising.  By design, and as
 * every renderer with interpolated normals has it: a Lambertian target p + n + sphere can point below the face, and dot(d, n) of
 * the dielectric reads the shading side, not the geometric one.  No geometric-side check of scattered directions is made.
 *
 * Where attributes do not apply.  Wrappers do not touch (tu, tv).  A boundary query of a ConstantMedium ignores attributes: only
 * t matters.  A triangle without UVs has the surface coordinates (0, 0), and so has every other primitive.  A triangle without
 * normals shades with N.
 *
 * rtg_object_triangle_attr: rtg_object_triangle with normals9 (n0, n1, n2) and / or uvs6 (u0, v0, u1, v1, u2, v2), either may be
 * NULL.  With both NULL it IS rtg_object_triangle: the same id, the same records.  It refuses what that call refuses, a normal or
 * UV component that is not finite, and a surface material (below) on a triangle without UVs.  A zero vertex normal is accepted:
 * the len fallback covers it.
 *
 * rtg_object_mesh_attr: rtg_object_mesh with normals (n_vertices x 3) and / or uvs (n_vertices x 2), either may be NULL: what
 * the caller would get from the triangle calls above plus rtg_object_bvh (sah = 0) or rtg_object_bvh_sah (sah = 1).  A refusal
 * covers the whole mesh and leaves the builder unchanged.
 *
 * rtg_texture_surface(child): a texture whose value at a hit is `child` evaluated at the point (tu, tv, 0.0f) instead of p.
 * `child` may be any texture id rtg_material_lambertian takes, except a surface texture.  An image child with the planar mapping
 * m = (1,0,0,0, 0,1,0,0) is ordinary UV mapping -- v up, row 0 of the image at the top (rtiow_gpu_image.h: y = (1 - v) * h); other
 * m scale, shift and rotate the UVs for free.  A checker or Perlin child is a pattern in UV space.  The id is accepted as the
 * texture of rtg_material_lambertian and rtg_material_diffuse_light only: rtg_texture_checker refuses it as a child,
 * rtg_texture_surface as its own child, rtg_material_isotropic as an albedo (a medium has no surface); and a material built on
 * it goes on triangles with UVs alone: every object constructor but the two above refuses it.  rtg_debug_texture_host and
 * rtg_debug_texture answer for it with the child's value at (p.x, p.y, 0).
 *
 * Which kernels.  As for every scene with a triangle (rtiow_gpu_mesh.h): the full-feature ray-pool kernel or the lock-step kernel,
 * with the same bits as the one-lane kernel; queries, ray frames, the feature pass and flagged frames one lane per ray.  The
 * flattened program has feature bit 2048 (FEAT_SURFACE) when it holds a triangle with an attribute, and only then.
 *
 * rtg_debug_triangle_attr_host needs no GPU: for n (triangle, ray) pairs -- tri9: v0, v1, v2; attr15: n0, n1, n2, uv0, uv1, uv2;
 * has: bit 0 = use the normals, bit 1 = use the UVs; rays8: o, d, time (unused), t_max -- it writes (hit, t, p.xyz, n.xyz, tu, tv)
 * through the functions the kernels call, zeros on a miss.
 *
 * rtg_debug_hit_surface is rtg_debug_hit_top (rtiow_gpu_debug.h) with (tu, tv) behind the normal: one lane per ray through
 * hit_top, for any scene; rays7: o, d, time; out10 per ray, zeros on a miss; mat: the material id, 0xffffffff on a miss. */
#ifndef RTIOW_GPU_SURFACE_H
#define RTIOW_GPU_SURFACE_H
#include "rtiow_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif

rtg_id rtg_object_triangle_attr(rtg_builder* b, const float v0[3], const float v1[3], const float v2[3], const float* normals9, const float* uvs6, rtg_id material);
rtg_id rtg_object_mesh_attr(rtg_builder* b, const float* vertices, size_t n_vertices, const uint32_t* indices, size_t n_triangles, const float* normals, const float* uvs, rtg_id material, uint32_t sah);
rtg_id rtg_texture_surface(rtg_builder* b, rtg_id child);
int rtg_debug_triangle_attr_host(size_t n, const float* tri9, const float* attr15, uint32_t has, const float* rays8, float t_min, float* out10);
int rtg_debug_hit_surface(rtg_scene* s, size_t n, const float* rays7, uint64_t seed, float t_near, float* out10, uint32_t* mat);

#ifdef __cplusplus
}
#endif
#endif /* RTIOW_GPU_SURFACE_H */
