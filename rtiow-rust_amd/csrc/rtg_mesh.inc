// rtg_mesh.inc -- included by rtg_api.hip: triangles and meshes (include/rtiow_gpu_mesh.h) -- the two builder calls and the host
// probe.  The hit test is rt_triangle.h (one source for host and device), the record layout flat_scene.h OP_TRI, the builder's
// part scene_builder.cpp add_triangle / add_mesh / emit, the kernels' part rt_trace.h and rt_light.h (the FEAT_TRI instantiations),
// rt_full_ops.inc exec_op and rt_pool_full.h rebuild_hit (the TRI instantiations of the full-feature pool and lock-step kernels).

extern "C" {

rtg_id rtg_object_triangle(rtg_builder* b, const float v0[3], const float v1[3], const float v2[3], rtg_id material) {
  if (!b || !v0 || !v1 || !v2) return bad("null argument");
  const float v[9] = {v0[0], v0[1], v0[2], v1[0], v1[1], v1[2], v2[0], v2[1], v2[2]};
  try {
    return b->sb.add_triangle(v, material);
  } catch (const BuildError& e) {
    fail(e.code, e.msg);
    return RTG_INVALID_ID;
  }
}

rtg_id rtg_object_mesh(rtg_builder* b, const float* vertices, size_t n_vertices, const uint32_t* indices, size_t n_triangles, rtg_id material,
                       uint32_t sah) {
  if (!b || (n_triangles && (!vertices || !indices))) return bad("null argument");
  if (sah > 1u) return bad("mesh: sah > 1");
  try {
    return b->sb.add_mesh(vertices, n_vertices, indices, n_triangles, material, sah != 0u);
  } catch (const BuildError& e) {
    fail(e.code, e.msg);
    return RTG_INVALID_ID;
  } catch (const std::bad_alloc&) {
    return bad("mesh: out of memory");
  }
}

int rtg_debug_triangle_host(size_t n, const float* tri9, const float* rays8, float t_min, float* out8) {
  if (n && (!tri9 || !rays8 || !out8)) return fail(RTG_ERR_INVALID, "null argument");
  for (size_t i = 0; i < n; i++) {
    const float *v = tri9 + 9 * i, *r = rays8 + 8 * i;
    float* o = out8 + 8 * i;
    Tri3 e1, e2, nn;
    const Tri3 v0{v[0], v[1], v[2]}, ro{r[0], r[1], r[2]}, rd{r[3], r[4], r[5]};
    (void)tri_record(v0, Tri3{v[3], v[4], v[5]}, Tri3{v[6], v[7], v[8]}, e1, e2, nn);
    float t = 0.f;
    if (tri_hit_t(v0, e1, e2, ro, rd, t_min, r[7], t)) {
      o[0] = 1.f, o[1] = t;
      o[2] = ro.x + t * rd.x, o[3] = ro.y + t * rd.y, o[4] = ro.z + t * rd.z;
      o[5] = nn.x, o[6] = nn.y, o[7] = nn.z;
    } else {
      for (int k = 0; k < 8; k++) o[k] = 0.f;
    }
  }
  return RTG_OK;
}

}  // extern "C"
