// rtg_image.inc -- included by rtg_api.hip: image textures (include/rtiow_gpu_image.h) -- the builder call and the probes.  The
// sampler is rt_image.h (one source for host and device), the record layout flat_scene.h TEX_IMAGE, the flattener's part
// scene_builder.cpp finish_materials, the kernels' part rt_trace.h texture_eval / image_eval.

// One lane per point through texture_eval, the function every kernel evaluates a non-constant texture with
__global__ void debug_texture_kernel(DevScene sc, uint32_t idx, size_t n, const float* __restrict__ p, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 c = texture_eval(sc, idx, mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]));
  out[3 * i] = c.x, out[3 * i + 1] = c.y, out[3 * i + 2] = c.z;
}

extern "C" {

rtg_id rtg_texture_image(rtg_builder* b, const rtg_image_params* params, uint32_t w, uint32_t h, const float* rgb) {
  if (!b || !params || !rgb) return bad("null argument");
  if (params->struct_size != sizeof(rtg_image_params)) return bad("image: wrong struct_size");
  if (params->mapping > 1u || params->filter > 1u || params->wrap_u > 1u || params->wrap_v > 1u) return bad("image: unknown mapping, filter or wrap");
  if (params->reserved_in != 0u) return bad("image: reserved_in != 0");
  if (w < 1u || h < 1u || w > IMG_MAX_SIDE || h > IMG_MAX_SIDE || (uint64_t)w * h > IMG_MAX_TEXELS) return bad("image: w or h outside 1 .. 16384, or w * h > 2^24");
  if (params->mapping == 1u)
    for (int i = 3; i < 8; i++)
      if (params->m[i] != 0.f) return bad("image: the spherical mapping takes a centre (m0, m1, m2); m3 .. m7 must be 0");
  HostTexture t, ext;
  t.kind = TEX_IMAGE;
  t.w = w, t.h = h;
  t.flags = (params->mapping ? IMG_SPHERICAL : 0u) | (params->filter ? IMG_BILINEAR : 0u) | (params->wrap_u ? IMG_CLAMP_U : 0u) | (params->wrap_v ? IMG_CLAMP_V : 0u);
  const size_t texels = (size_t)w * h;
  try {
    t.texels.resize(4 * texels);
  } catch (const std::bad_alloc&) {
    return bad("image: out of memory");
  }
  for (size_t k = 0; k < texels; k++) t.texels[4 * k] = rgb[3 * k], t.texels[4 * k + 1] = rgb[3 * k + 1], t.texels[4 * k + 2] = rgb[3 * k + 2], t.texels[4 * k + 3] = 0.f;
  ext.kind = TEX_EXT;
  for (int i = 0; i < 8; i++) ext.m[i] = params->m[i];
  b->sb.textures.push_back(std::move(t));
  b->sb.textures.push_back(ext);
  return (rtg_id)b->sb.textures.size() - 2;
}

int rtg_debug_texture_host(rtg_builder* b, rtg_id texture, size_t n, const float* p, float* out) {
  if (!b || (n && (!p || !out))) return fail(RTG_ERR_INVALID, "null argument");
  if (texture >= b->sb.textures.size() || b->sb.textures[texture].kind == TEX_EXT) return fail(RTG_ERR_INVALID, "rtg_debug_texture_host: bad texture handle");
  if (b->sb.textures[texture].kind == TEX_SURFACE) {  // include/rtiow_gpu_surface.h: the child's value at (p.x, p.y, 0)
    std::vector<float> q(p, p + 3 * n);
    for (size_t i = 0; i < n; i++) q[3 * i + 2] = 0.f;
    return rtg_debug_texture_host(b, b->sb.textures[texture].t0, n, q.data(), out);
  }
  const HostTexture& t = b->sb.textures[texture];
  if (t.kind == TEX_CONSTANT) {
    for (size_t i = 0; i < n; i++) out[3 * i] = t.rgb[0], out[3 * i + 1] = t.rgb[1], out[3 * i + 2] = t.rgb[2];
    return RTG_OK;
  }
  if (t.kind != TEX_IMAGE) return fail(RTG_ERR_UNSUPPORTED, "rtg_debug_texture_host evaluates image and constant textures; rtg_debug_texture evaluates every kind");
  const float* m = b->sb.textures[texture + 1].m;
  const ImgTexel* texels = reinterpret_cast<const ImgTexel*>(t.texels.data());
  for (size_t i = 0; i < n; i++) {
    const ImgRgb c = image_sample(texels, t.w, t.h, t.flags, m, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
    out[3 * i] = c.r, out[3 * i + 1] = c.g, out[3 * i + 2] = c.b;
  }
  return RTG_OK;
}

int rtg_debug_texture(rtg_scene* s, rtg_id texture, size_t n, const float* p, float* out) {
  if (!s || (n && (!p || !out))) return fail(RTG_ERR_INVALID, "null argument");
  if (texture >= s->tex_kind.size() || s->tex_kind[texture] == TEX_EXT) return fail(RTG_ERR_INVALID, "rtg_debug_texture: bad texture handle");
  if (n > 0xffffffffull * 256ull) return fail(RTG_ERR_RANGE, "rtg_debug_texture: too many points");
  if (n == 0) return RTG_OK;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<float> d_p, d_out;
  HIP_TRY(d_p.alloc(3 * n));
  HIP_TRY(d_out.alloc(3 * n));
  if (s->tex_kind[texture] == TEX_SURFACE) {  // include/rtiow_gpu_surface.h: the child's value at (p.x, p.y, 0)
    std::vector<float> q(p, p + 3 * n);
    for (size_t i = 0; i < n; i++) q[3 * i + 2] = 0.f;
    HIP_TRY(hipMemcpy(d_p.p, q.data(), 3 * n * sizeof(float), hipMemcpyHostToDevice));
    texture = s->tex_child[texture];
  } else {
    HIP_TRY(hipMemcpy(d_p.p, p, 3 * n * sizeof(float), hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(debug_texture_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, s->dev, (uint32_t)texture, n, d_p.p, d_out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_out.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
  return RTG_OK;
}

int rtg_debug_atan2f_host(size_t n, const float* y, const float* x, float* out) {
  if (n && (!y || !x || !out)) return fail(RTG_ERR_INVALID, "null argument");
  for (size_t i = 0; i < n; i++) out[i] = rt_atan2f(y[i], x[i]);
  return RTG_OK;
}

}  // extern "C"
