// rtg_rays.inc -- included by rtg_api.hip: ray frames (include/rtiow_gpu_rays.h) -- a frame whose paths start on the CALLER's
// rays instead of a camera's.  The general kernel, which renders every program; the choice between it and the RAYS
// instantiations of the lean pool kernel (rt_pool.h; rtg_launch.inc launch_pool); the two entry points.
//
// A sample is color() (rt_trace.h) on the caller's ray with the stream SampleRng::init(seed, y * nx + x, s): color() restarts
// the stream at event 1, so the camera's event-0 draws never reached a path -- with the camera's own rays the frame is
// rtg_par_cast's, bit for bit.  The frame machinery (slices, squares plane, background, tiles and ranks) is the camera frames'.

// The general kernel: one lane per pixel over color<FEAT, false>, render_pixel's 16x16 block, 8x8 wave mapping and tile / rank
// test (rtg_kernels.inc); one body in the style of render_light_kernel: s_begin and divide are run-time values (a whole frame
// is s_begin = 0, divide = 1), SQ as render_squares_kernel.  `per_sample`: RTG_RAYS_PER_SAMPLE.  Every ray offset in 64 bits.
template <uint32_t FEAT, bool SQ>
__global__ __launch_bounds__(256) void render_rays_kernel(DevScene sc, const float* __restrict__ rays, uint32_t per_sample, DevParams P, float* out,
                                                          uint32_t s_begin, uint32_t divide) {
  const uint32_t nbx = (P.nx + 15u) / 16u;
  const uint32_t bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const uint32_t tiles_x = (P.nx + P.tile_w - 1u) / P.tile_w;
  const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63u;
  const uint32_t x0 = bx * 16u + (w & 1u) * 8u, row0 = by * 16u + (w >> 1) * 8u;
  const uint32_t tile = (row0 / P.tile_h) * tiles_x + x0 / P.tile_w;
  if (tile % P.nranks != P.rank) return;
  const uint32_t x = x0 + (l & 7u);
  const uint32_t row = row0 + (l >> 3);
  if (x >= P.nx || row >= P.ny) return;
  const uint32_t y = P.ny - 1u - row;
  const uint64_t pixel = (uint64_t)row * P.nx + x, n_pix = (uint64_t)P.nx * P.ny;
  float* o = out + 3ull * pixel;
  float* q = o + 3ull * n_pix;
  V3 col = mk(0.f, 0.f, 0.f), sq = mk(0.f, 0.f, 0.f);
  if (s_begin != 0u) {
    col = mk(o[0], o[1], o[2]);
    if (SQ) sq = mk(q[0], q[1], q[2]);
  }
  Counts cnt = {0, 0, 0, 0};
  for (uint32_t s = s_begin; s < P.ns; s++) {
    const float* r = rays + 7ull * (per_sample ? (uint64_t)s * n_pix + pixel : pixel);
    SampleRng rng;
    rng.init(((uint64_t)P.seed_hi << 32) | P.seed_lo, y * P.nx + x, s);
    uint32_t bounces;
    V3 c = color<FEAT, false>(sc, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], P, rng, cnt, bounces);
    col = vadd(col, c);
    if (SQ) sq = vadd(sq, vmul(c, c));
  }
  if (divide) col = sdiv(col, (float)P.ns);  // lib.rs:374
  o[0] = col.x, o[1] = col.y, o[2] = col.z;
  if (SQ) q[0] = sq.x, q[1] = sq.y, q[2] = sq.z;
}

namespace {

constexpr uint32_t RAY_FRAME_FLAGS = RTG_FLAG_PARTIAL | RTG_FLAG_RESUME | RTG_FLAG_SUM_SQUARES | RTG_FLAG_BACKGROUND;

// The rays a frame's array holds
uint64_t ray_count(const rtg_params* p, uint32_t ray_mode) {
  return (uint64_t)p->nx * p->ny * (ray_mode == RTG_RAYS_PER_SAMPLE ? (uint64_t)p->ns : 1ull);
}

// The checks both entry points make before anything is written or enqueued
int rays_check(const rtg_scene* s, const float* rays, uint32_t ray_mode, const rtg_params* p, const float* out, const rtg_stats* stats, DevParams* d) {
  if (!s || !p || !rays || !out) return fail(RTG_ERR_INVALID, "null argument");
  if (p->struct_size != sizeof(rtg_params)) return fail(RTG_ERR_INVALID, "rtg_params.struct_size mismatch");
  if (stats && stats->struct_size != sizeof(rtg_stats)) return fail(RTG_ERR_INVALID, "rtg_stats.struct_size mismatch");
  if (ray_mode > RTG_RAYS_PER_SAMPLE) return fail(RTG_ERR_INVALID, "rtg_par_cast_rays: ray_mode > RTG_RAYS_PER_SAMPLE");
  if (p->flags & ~RAY_FRAME_FLAGS)
    return fail(RTG_ERR_UNSUPPORTED, "rtg_par_cast_rays: flags other than RTG_FLAG_PARTIAL | RESUME | SUM_SQUARES | BACKGROUND are not supported on ray frames");
  if (s->light_sampling) return fail(RTG_ERR_UNSUPPORTED, "rtg_par_cast_rays: scene option light_sampling = 1 is not supported on ray frames");
  rtg_camera none{};  // (check_params wants a camera with a valid exposure: the ray's time is the caller's)
  none.exposure_end = 1.f;
  if (int rc = check_params(s, &none, p, d)) return rc;
  if (ray_count(p, ray_mode) > (~0ull >> 1) / (7u * sizeof(float))) return fail(RTG_ERR_INVALID, "rtg_par_cast_rays: the ray array does not fit the address space");
  return RTG_OK;
}

// Does the lean pool kernel render a ray frame of this scene (option ray_pool)?  launch_slice's conditions for a camera frame.
bool rays_take_pool(const rtg_scene* s, const DevParams& d) {
  if (!s->ray_pool || (s->features & (FEAT_NOT_LEAN | FEAT_DEEP)) != 0u) return false;
  const bool accum_zero = !(s->features & FEAT_WIDE_ALBEDO) && (!(s->features & FEAT_BRIGHT_ALBEDO) || d.max_bounces <= 63u);
  return accum_zero && s->kernel_version >= 3 && d.nx <= 0xffffu && d.ny <= 0xffffu;
}

// The render of the samples [sl.begin, d.ns) of a ray frame
hipError_t launch_rays(rtg_scene* s, const float* d_rays, uint32_t ray_mode, const DevParams& d, float* d_out, hipStream_t stream, const SampleSlice& sl) {
  if (sl.begin == d.ns) return sl.divide ? launch_resolve(d, d_out, stream) : hipSuccess;  // the resolve step of a progressive frame
  const char* layout = ray_mode == RTG_RAYS_PER_SAMPLE ? "sample" : "pixel";
  if (rays_take_pool(s, d)) {
    s->cx->last_kernel = KernelKind::lean_pool;
    if (s->verbose) fprintf(stderr, "[rtg] ray frame: lean pool kernel, one ray per %s\n", layout);
    return launch_pool<false>(s, DevCamera{}, d, d_out, stream, sl, d_rays, ray_mode);
  }
  s->cx->last_kernel = KernelKind::baseline;
  const dim3 grid(((d.nx + 15) / 16) * ((d.ny + 15) / 16)), block(256);
  if (s->verbose) fprintf(stderr, "[rtg] ray frame: general kernel, one ray per %s, %u workgroups x 256 threads\n", layout, grid.x);
  with_feat<false>(s, [&](auto feat) {
    constexpr uint32_t F = decltype(feat)::value;
    void (*k)(DevScene, const float*, uint32_t, DevParams, float*, uint32_t, uint32_t) = sl.squares ? render_rays_kernel<F, true> : render_rays_kernel<F, false>;
    hipLaunchKernelGGL(k, grid, block, 0, stream, s->dev, d_rays, ray_mode, d, d_out, sl.begin, sl.divide ? 1u : 0u);
  });
  return hipGetLastError();
}

}  // namespace

extern "C" {

int rtg_par_cast_rays_device(rtg_scene* s, const float* d_rays7, uint32_t ray_mode, const rtg_params* params, float* d_out, void* hip_stream,
                             rtg_stats* stats) {
  DevParams d;
  if (int rc = rays_check(s, d_rays7, ray_mode, params, d_out, stats, &d)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t stream = (hipStream_t)hip_stream;
  if (int rc = ctx_acquire(s)) return rc;
  const SampleSlice sl = slice_of(params);
  const FrameLayout L(d.nx, d.ny, params->flags);
  if (sl.background) {  // the block's in-fields come back now, in one copy-and-wait, before anything is enqueued (as rtg_par_cast_device)
    FrameBlocks fb;
    HIP_TRY(read_blocks(L, sl, d_out, stream, &fb));
    HIP_TRY(hipStreamSynchronize(stream));
    if (const char* why = blocks_refusal(sl, fb, d.nranks)) return fail(RTG_ERR_INVALID, why);
    d.bg = dev_background(fb.background);
  }
  // (from here on work of this frame may sit on `stream`: a failure drains it before the context is handed out again)
  hipError_t e = stats ? hipEventRecord(s->cx->ev0, stream) : hipSuccess;
  if (e == hipSuccess) e = launch_rays(s, d_rays7, ray_mode, d, d_out, stream, sl);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(stream);
    return hip_fail(e, "rtg_par_cast_rays: launch");
  }
  if (int rc = ctx_release(s, stream)) {
    (void)hipStreamSynchronize(stream);
    return rc;
  }
  if (stats) {
    HIP_TRY(hipEventRecord(s->cx->ev1, stream));
    HIP_TRY(hipEventSynchronize(s->cx->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->cx->ev0, s->cx->ev1));
    const uint32_t size = stats->struct_size;
    *stats = rtg_stats{};
    stats->struct_size = size, stats->kernel_ms = ms, stats->samples = owned_pixels(d) * (d.ns - sl.begin);
  }
  return RTG_OK;
}

int rtg_par_cast_rays(rtg_scene* s, const float* rays7, uint32_t ray_mode, const rtg_params* params, float* out_rgb, rtg_stats* stats) {
  {
    DevParams d;  // (refused before anything is uploaded)
    if (int rc = rays_check(s, rays7, ray_mode, params, out_rgb, stats, &d)) return rc;
  }
  const SampleSlice sl = slice_of(params);
  const FrameLayout L(params->nx, params->ny, params->flags);
  FrameBlocks fb;
  if (int rc = check_blocks(L, sl, out_rgb, params->nranks ? params->nranks : 1u, &fb)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  // the rays in a temporary buffer: all of a per-pixel array, the samples [sample_begin, ns) of a per-sample one
  const uint64_t n_pix = (uint64_t)params->nx * params->ny, n_rays = ray_count(params, ray_mode);
  const uint64_t first = ray_mode == RTG_RAYS_PER_SAMPLE ? (uint64_t)sl.begin * n_pix : 0ull;
  DevBuf<float> d_rays;
  HIP_TRY(d_rays.alloc(7u * n_rays));
  if (n_rays > first) HIP_TRY(hipMemcpy(d_rays.p + 7u * first, rays7 + 7u * first, 7u * (n_rays - first) * sizeof(float), hipMemcpyHostToDevice));
  // the frame as rtg_par_cast stages it: the scene's staging frame, the same upload rules
  hipError_t e = s->frame.grow(L.words ? L.words * sizeof(float) : 16);
  if (e != hipSuccess) return hip_fail(e, "hipMalloc(framebuffer)");
  float* d_out = s->frame.as<float>();
  char* dev = reinterpret_cast<char*>(d_out);
  char* host = reinterpret_cast<char*>(out_rgb);
  const Extents up = upload_extents(L, params->nranks > 1, sl.begin, 0u);
  for (int i = 0; i < up.n && e == hipSuccess; i++) e = hipMemcpy(dev + up.e[i].lo, host + up.e[i].lo, up.e[i].hi - up.e[i].lo, hipMemcpyHostToDevice);
  int rc = (e == hipSuccess) ? rtg_par_cast_rays_device(s, d_rays.p, ray_mode, params, d_out, nullptr, stats) : hip_fail(e, "hipMemcpy");
  if (rc == RTG_OK) {
    e = hipDeviceSynchronize();
    const Extents back = copy_back_extents(L, 0u);
    for (int i = 0; i < back.n && e == hipSuccess; i++) e = hipMemcpy(host + back.e[i].lo, dev + back.e[i].lo, back.e[i].hi - back.e[i].lo, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = hip_fail(e, "render / copy back");
  } else {
    (void)hipDeviceSynchronize();  // (the temporary ray buffer is freed on return)
  }
  return rc;
}

}  // extern "C"
