// rtg_environment.inc -- included by rtg_api.hip: the scene's environment (include/rtiow_gpu_environment.h) -- the builder calls
// and the probes.  The direction mapping is rt_environment.h (one source for host and device), the kernels' part rt_trace.h
// environment_colour / miss_colour_scene, the flattener's part scene_builder.cpp flatten (FEAT_ENVIRONMENT), and the frame
// parameters' part rtg_api.hip check_params (rtg_scene::env_bg).

// One lane per direction through environment_colour, the function every textured kernel's miss branch calls
__global__ void debug_environment_kernel(DevScene sc, Background bg, size_t n, const float* __restrict__ d, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 c = environment_colour(sc, bg, mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]));
  out[3 * i] = c.x, out[3 * i + 1] = c.y, out[3 * i + 2] = c.z;
}

extern "C" {

int rtg_builder_set_environment(rtg_builder* b, const rtg_environment_params* p) {
  if (!b || !p) return fail(RTG_ERR_INVALID, "null argument");
  if (p->struct_size != sizeof(rtg_environment_params)) return fail(RTG_ERR_INVALID, "environment: wrong struct_size");
  if (p->reserved_in[0] != 0u || p->reserved_in[1] != 0u) return fail(RTG_ERR_INVALID, "environment: reserved_in != 0");
  if (p->texture == RTG_INVALID_ID) {
    b->sb.environment = SceneBuilder::Environment{};
    return RTG_OK;
  }
  if (p->texture >= b->sb.textures.size() || b->sb.textures[p->texture].kind == TEX_EXT) return fail(RTG_ERR_INVALID, "environment: bad texture handle");
  if (b->sb.textures[p->texture].kind == TEX_SURFACE) return fail(RTG_ERR_INVALID, "environment: a miss has no surface coordinates for a surface texture");
  if (!std::isfinite(p->rotate_y_degrees)) return fail(RTG_ERR_INVALID, "environment: rotate_y_degrees is not finite");
  SceneBuilder::Environment ev;
  ev.texture = p->texture;
  for (int c = 0; c < 3; c++) ev.scale[c] = p->scale[c];
  ev.degrees = p->rotate_y_degrees;
  rotate_y_pair(ev.degrees, &ev.s, &ev.c);
  b->sb.environment = ev;
  return RTG_OK;
}

int rtg_builder_get_environment(const rtg_builder* b, rtg_environment_params* out, float sin_cos[2]) {
  if (!b || !out) return fail(RTG_ERR_INVALID, "null argument");
  const SceneBuilder::Environment& ev = b->sb.environment;
  *out = rtg_environment_params{};
  out->struct_size = sizeof(rtg_environment_params);
  out->texture = ev.texture;  // (0xffffffff = RTG_INVALID_ID: none)
  for (int c = 0; c < 3; c++) out->scale[c] = ev.scale[c];
  out->rotate_y_degrees = ev.degrees;
  if (sin_cos) sin_cos[0] = ev.s, sin_cos[1] = ev.c;
  return RTG_OK;
}

int rtg_debug_environment_host(rtg_builder* b, size_t n, const float* d, float* out) {
  if (!b || (n && (!d || !out))) return fail(RTG_ERR_INVALID, "null argument");
  const SceneBuilder::Environment& ev = b->sb.environment;
  if (ev.texture >= b->sb.textures.size()) return fail(RTG_ERR_INVALID, "rtg_debug_environment_host: the builder has no environment");
  std::vector<float> q(3 * n);
  for (size_t i = 0; i < n; i++) environment_direction(d[3 * i], d[3 * i + 1], d[3 * i + 2], ev.s, ev.c, &q[3 * i]);
  if (int rc = rtg_debug_texture_host(b, ev.texture, n, q.data(), out)) return rc;  // (image and constant textures, else RTG_ERR_UNSUPPORTED)
  for (size_t i = 0; i < n; i++)
    for (int c = 0; c < 3; c++) out[3 * i + c] = ev.scale[c] * out[3 * i + c];
  return RTG_OK;
}

int rtg_debug_environment(rtg_scene* s, size_t n, const float* d, float* out) {
  if (!s || (n && (!d || !out))) return fail(RTG_ERR_INVALID, "null argument");
  if (s->env_bg.mode != BG_TEXTURE) return fail(RTG_ERR_INVALID, "rtg_debug_environment: the scene has no environment");
  if (n > 0xffffffffull * 256ull) return fail(RTG_ERR_RANGE, "rtg_debug_environment: too many directions");
  if (n == 0) return RTG_OK;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<float> d_d, d_out;
  HIP_TRY(d_d.alloc(3 * n));
  HIP_TRY(d_out.alloc(3 * n));
  HIP_TRY(hipMemcpy(d_d.p, d, 3 * n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(debug_environment_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, s->dev, s->env_bg, n, d_d.p, d_out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_out.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
  return RTG_OK;
}

}  // extern "C"
