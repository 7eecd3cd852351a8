// rtg_surface.inc -- included by rtg_api.hip: surface attributes (include/rtiow_gpu_surface.h) -- the three builder calls and the
// two probes.  The interpolation is rt_triangle.h tri_uv / tri_shade (one source for host and device), the record layout
// flat_scene.h OP_TRI (F_TRI_NORMALS / F_TRI_UVS) and MAT_SURFACE, the builder's part scene_builder.cpp add_triangle / add_mesh /
// emit / finish_materials, the kernels' part the FEAT_SURFACE instantiations of rt_trace.h, rt_light.h and rt_features.h and the
// SURF instantiations of the full-feature pool and lock-step kernels (rt_full_ops.inc exec_op, rt_pool_full.h rebuild_hit).

extern "C" {

rtg_id rtg_object_triangle_attr(rtg_builder* b, const float v0[3], const float v1[3], const float v2[3], const float* normals9, const float* uvs6,
                                rtg_id material) {
  if (!b || !v0 || !v1 || !v2) return bad("null argument");
  const float v[9] = {v0[0], v0[1], v0[2], v1[0], v1[1], v1[2], v2[0], v2[1], v2[2]};
  try {
    return b->sb.add_triangle(v, material, normals9, uvs6);
  } catch (const BuildError& e) {
    fail(e.code, e.msg);
    return RTG_INVALID_ID;
  }
}

rtg_id rtg_object_mesh_attr(rtg_builder* b, const float* vertices, size_t n_vertices, const uint32_t* indices, size_t n_triangles, const float* normals,
                            const float* uvs, rtg_id material, uint32_t sah) {
  if (!b || (n_triangles && (!vertices || !indices))) return bad("null argument");
  if (sah > 1u) return bad("mesh: sah > 1");
  try {
    return b->sb.add_mesh(vertices, n_vertices, indices, n_triangles, material, sah != 0u, normals, uvs);
  } catch (const BuildError& e) {
    fail(e.code, e.msg);
    return RTG_INVALID_ID;
  } catch (const std::bad_alloc&) {
    return bad("mesh: out of memory");
  }
}

rtg_id rtg_texture_surface(rtg_builder* b, rtg_id child) {
  if (!b) return bad("null argument");
  if (child >= b->sb.textures.size() || b->sb.textures[child].kind == TEX_EXT) return bad("surface: bad texture handle");
  if (b->sb.textures[child].kind == TEX_SURFACE) return bad("surface: the child is a surface texture itself");
  HostTexture t;
  t.kind = TEX_SURFACE;
  t.t0 = child;
  b->sb.textures.push_back(t);
  return (rtg_id)b->sb.textures.size() - 1;
}

int rtg_debug_triangle_attr_host(size_t n, const float* tri9, const float* attr15, uint32_t has, const float* rays8, float t_min, float* out10) {
  if (n && (!tri9 || !attr15 || !rays8 || !out10)) return fail(RTG_ERR_INVALID, "null argument");
  if (has > 3u) return fail(RTG_ERR_INVALID, "rtg_debug_triangle_attr_host: has > 3");
  for (size_t i = 0; i < n; i++) {
    const float *v = tri9 + 9 * i, *a = attr15 + 15 * i, *r = rays8 + 8 * i;
    float* o = out10 + 10 * i;
    Tri3 e1, e2, nn;
    const Tri3 v0{v[0], v[1], v[2]}, ro{r[0], r[1], r[2]}, rd{r[3], r[4], r[5]};
    (void)tri_record(v0, Tri3{v[3], v[4], v[5]}, Tri3{v[6], v[7], v[8]}, e1, e2, nn);
    float t = 0.f;
    if (tri_hit_t(v0, e1, e2, ro, rd, t_min, r[7], t)) {
      float bu, bv, tu, tv;
      tri_uv(v0, e1, e2, ro, rd, bu, bv);  // (as rebuild_hit has them: the same operations as the accept test's)
      const TriAttr at{Tri3{a[0], a[1], a[2]}, Tri3{a[3], a[4], a[5]}, Tri3{a[6], a[7], a[8]}, a[9], a[10], a[11], a[12], a[13], a[14]};
      const Tri3 sn = tri_shade(bu, bv, at, nn, (has & 1u) != 0u, (has & 2u) != 0u, tu, tv);
      o[0] = 1.f, o[1] = t;
      o[2] = ro.x + t * rd.x, o[3] = ro.y + t * rd.y, o[4] = ro.z + t * rd.z;
      o[5] = sn.x, o[6] = sn.y, o[7] = sn.z;
      o[8] = tu, o[9] = tv;
    } else {
      for (int k = 0; k < 10; k++) o[k] = 0.f;
    }
  }
  return RTG_OK;
}

int rtg_debug_hit_surface(rtg_scene* s, size_t n, const float* rays7, uint64_t seed, float t_near, float* out10, uint32_t* mat) {
  if (!s || (n && (!rays7 || !out10 || !mat))) return fail(RTG_ERR_INVALID, "null argument");
  if (n > 0xffffffffull) return fail(RTG_ERR_RANGE, "rtg_debug_hit_surface: too many rays");
  if (n == 0) return RTG_OK;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<float> d_rays, d_out;
  DevBuf<uint32_t> d_mat;
  HIP_TRY(d_rays.alloc(7 * n));
  HIP_TRY(d_out.alloc(10 * n));
  HIP_TRY(d_mat.alloc(n));
  HIP_TRY(hipMemcpy(d_rays.p, rays7, 7 * n * sizeof(float), hipMemcpyHostToDevice));
  dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  with_feat<false>(s, [&](auto feat) {
    hipLaunchKernelGGL((debug_hit_surface_kernel<decltype(feat)::value>), grid, block, 0, 0, s->dev, (uint32_t)n, d_rays.p, (uint32_t)seed, (uint32_t)(seed >> 32),
                       t_near, d_out.p, d_mat.p);
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out10, d_out.p, 10 * n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(mat, d_mat.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTG_OK;
}

}  // extern "C"
