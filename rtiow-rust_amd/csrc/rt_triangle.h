// rt_triangle.h -- the triangle primitive (include/rtiow_gpu_mesh.h), ONE host-and-device function: every walk that executes an
// OP_TRI record (rt_trace.h hit_top / boundary_hit_t / walk_deep, rt_light.h occluded, rt_full_ops.inc exec_op) calls tri_hit_t on the GPU,
// rtg_debug_triangle_host and the builder call the very same source on the host, and rtiow-rust_amd/triangle.py is the same
// arithmetic in numpy, bit for bit.  Compile with -ffp-contract=off: every operation is rounded on its own.
// Plain C++ (no HIP types), so that a host program can include it on its own.
// Surface attributes (include/rtiow_gpu_surface.h) stand below the hit test: tri_uv / tri_hit_uv and tri_shade, for the FEAT_SURFACE /
// SURF instantiations of the same walks, rtg_debug_triangle_attr_host and triangle.py shade -- the same arithmetic, bit for bit.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RT_TRI_HD __host__ __device__ __forceinline__
#else
#define RT_TRI_HD inline
#endif

namespace rtg {

struct Tri3 {
  float x, y, z;
};

// cross(a, b).x = a.y*b.z - a.z*b.y, cyclic for y and z; each product rounded before the subtraction
RT_TRI_HD Tri3 tri_cross(Tri3 a, Tri3 b) { return Tri3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
RT_TRI_HD float tri_dot(Tri3 a, Tri3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RT_TRI_HD Tri3 tri_sub(Tri3 a, Tri3 b) { return Tri3{a.x - b.x, a.y - b.y, a.z - b.z}; }

// The record of (v0, v1, v2): e1 = v1 - v0, e2 = v2 - v0, N = cross(e1, e2) / len.  Returns len: the caller refuses a triangle
// whose len is 0 or not finite.  A counter-clockwise winding gives the front face.
RT_TRI_HD float tri_record(Tri3 v0, Tri3 v1, Tri3 v2, Tri3& e1, Tri3& e2, Tri3& n) {
  e1 = tri_sub(v1, v0), e2 = tri_sub(v2, v0);
  const Tri3 c = tri_cross(e1, e2);
  const float len = __builtin_sqrtf((c.x * c.x + c.y * c.y) + c.z * c.z);
  n = Tri3{c.x / len, c.y / len, c.z / len};
  return len;
}

// Moeller-Trumbore over [t_min, t_max).  Every predicate is in positive form: a zero or NaN determinant misses without a test of
// its own.  Both barycentric edges are inclusive: a shared edge is covered twice rather than cracked.  The range predicate is
// Sphere::hit's (object.rs:99).
RT_TRI_HD bool tri_hit_t(Tri3 v0, Tri3 e1, Tri3 e2, Tri3 o, Tri3 d, float t_min, float t_max, float& t_out) {
  const Tri3 pv = tri_cross(d, e2);
  const float det = tri_dot(e1, pv);
  const float inv = 1.0f / det;
  const Tri3 tv = tri_sub(o, v0);
  const float u = tri_dot(tv, pv) * inv;
  const Tri3 qv = tri_cross(tv, e1);
  const float v = tri_dot(d, qv) * inv;
  const float t = tri_dot(e2, qv) * inv;
  if (u >= 0.f && v >= 0.f && u + v <= 1.0f && t >= t_min && t < t_max) {
    t_out = t;
    return true;
  }
  return false;
}

// ---- surface attributes (include/rtiow_gpu_surface.h) ---------------------------------------------------------------------------
// tri_hit_uv: tri_hit_t that also hands out the barycentric u, v its accept test used.  tri_uv: u, v alone, recomputed with the
// same operations in the same order -- the same bits -- for a walk that kept only t (rt_pool_full.h rebuild_hit).
RT_TRI_HD void tri_uv(Tri3 v0, Tri3 e1, Tri3 e2, Tri3 o, Tri3 d, float& u_out, float& v_out) {
  const Tri3 pv = tri_cross(d, e2);
  const float det = tri_dot(e1, pv);
  const float inv = 1.0f / det;
  const Tri3 tv = tri_sub(o, v0);
  u_out = tri_dot(tv, pv) * inv;
  const Tri3 qv = tri_cross(tv, e1);
  v_out = tri_dot(d, qv) * inv;
}
RT_TRI_HD bool tri_hit_uv(Tri3 v0, Tri3 e1, Tri3 e2, Tri3 o, Tri3 d, float t_min, float t_max, float& t_out, float& u_out, float& v_out) {
  const Tri3 pv = tri_cross(d, e2);
  const float det = tri_dot(e1, pv);
  const float inv = 1.0f / det;
  const Tri3 tv = tri_sub(o, v0);
  const float u = tri_dot(tv, pv) * inv;
  const Tri3 qv = tri_cross(tv, e1);
  const float v = tri_dot(d, qv) * inv;
  const float t = tri_dot(e2, qv) * inv;
  if (u >= 0.f && v >= 0.f && u + v <= 1.0f && t >= t_min && t < t_max) {
    t_out = t, u_out = u, v_out = v;
    return true;
  }
  return false;
}

// The vertex attributes of one triangle: normals as given (not normalised, not turned), UVs as given.
struct TriAttr {
  Tri3 n0, n1, n2;
  float u0, v0, u1, v1, u2, v2;
};

// The shading normal and the surface coordinates at (u, v):  w = (1 - u) - v;  s = (w n0 + u n1) + v n2 per component, every
// product rounded, left to right;  n = s / len when len = sqrt((s.x s.x + s.y s.y) + s.z s.z) is > 0 and <= f32::MAX (positive
// form: NaN falls through), else the face normal N;  (tu, tv) = (w u0 + u u1) + v u2, likewise.  A triangle without normals
// shades with N, one without UVs has (tu, tv) = (0, 0).  FlipNormals is the caller's.
RT_TRI_HD Tri3 tri_shade(float u, float v, const TriAttr& a, Tri3 face_n, bool has_normals, bool has_uvs, float& tu, float& tv) {
  const float w = (1.0f - u) - v;
  tu = 0.f, tv = 0.f;
  if (has_uvs) {
    tu = (w * a.u0 + u * a.u1) + v * a.u2;
    tv = (w * a.v0 + u * a.v1) + v * a.v2;
  }
  if (!has_normals) return face_n;
  const Tri3 s{(w * a.n0.x + u * a.n1.x) + v * a.n2.x, (w * a.n0.y + u * a.n1.y) + v * a.n2.y, (w * a.n0.z + u * a.n1.z) + v * a.n2.z};
  const float len = __builtin_sqrtf((s.x * s.x + s.y * s.y) + s.z * s.z);
  if (len > 0.f && len <= 3.40282347e+38f) return Tri3{s.x / len, s.y / len, s.z / len};
  return face_n;
}

}  // namespace rtg
