// rtg_probes.inc -- included by rtg_api.hip inside its extern "C" block: the debug / probe entry points and the output stage.
// ---- probes --------------------------------------------------------------------------------------
int rtg_debug_hit_top(rtg_scene* s, size_t n, const float* rays, uint64_t seed, float t_near, float* out,
                      uint32_t* out_material) {
  if (!s || !rays || !out || !out_material) return fail(RTG_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<float> d_rays, d_out;
  DevBuf<uint32_t> d_mat;
  HIP_TRY(d_rays.alloc(7 * n));
  HIP_TRY(d_out.alloc(8 * n));
  HIP_TRY(d_mat.alloc(n));
  HIP_TRY(hipMemcpy(d_rays.p, rays, 7 * n * sizeof(float), hipMemcpyHostToDevice));
  dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  if (n)
    with_feat<false>(s, [&](auto feat) {
      hipLaunchKernelGGL((debug_hit_top_kernel<decltype(feat)::value>), grid, block, 0, 0, s->dev, (uint32_t)n, d_rays.p, (uint32_t)seed, (uint32_t)(seed >> 32),
                         t_near, d_out.p, d_mat.p);
    });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_out.p, 8 * n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_material, d_mat.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTG_OK;
}

int rtg_debug_samples(rtg_scene* s, const rtg_camera* camera, const rtg_params* params, size_t n, const uint32_t* xs,
                      const uint32_t* ys, const uint32_t* samples, float* out_rgb, uint32_t* out_info) {
  DevParams d;
  int rc = check_params(s, camera, params, &d);
  if (rc) return rc;
  if (!xs || !ys || !samples || !out_rgb || !out_info) return fail(RTG_ERR_INVALID, "null argument");
  if (params->flags & (RTG_FLAG_PARTIAL | RTG_FLAG_RESUME)) return fail(RTG_ERR_INVALID, "rtg_debug_samples renders whole frames: RTG_FLAG_PARTIAL / RTG_FLAG_RESUME are not accepted");
  if (params->flags & RTG_FLAG_SUM_SQUARES) return fail(RTG_ERR_INVALID, "rtg_debug_samples: RTG_FLAG_SUM_SQUARES is not accepted");
  if (params->flags & RTG_FLAG_SAMPLE_COUNTS) return fail(RTG_ERR_INVALID, "rtg_debug_samples: RTG_FLAG_SAMPLE_COUNTS is not accepted");
  if (params->flags & RTG_FLAG_RETIRE) return fail(RTG_ERR_INVALID, "rtg_debug_samples: RTG_FLAG_RETIRE is not accepted");
  if (params->flags & RTG_FLAG_DENOISE) return fail(RTG_ERR_INVALID, "rtg_debug_samples: RTG_FLAG_DENOISE is not accepted");
  if (params->flags & RTG_FLAG_FEATURES) return fail(RTG_ERR_INVALID, "rtg_debug_samples: RTG_FLAG_FEATURES is not accepted");
  if (params->flags & RTG_FLAG_DENOISE_ERROR) return fail(RTG_ERR_INVALID, "rtg_debug_samples: RTG_FLAG_DENOISE_ERROR is not accepted");
  if (params->flags & RTG_FLAG_BACKGROUND) return fail(RTG_ERR_INVALID, "rtg_debug_samples: RTG_FLAG_BACKGROUND is not accepted");
  HIP_TRY(hipSetDevice(s->device));
  if (params->flags & RTG_FLAG_TRACE_KERNEL) {
    // Trace the PRODUCTION kernel: render the whole frame with the instrumented variant of whatever kernel par_cast
    // uses for this scene, with its per-sample trace table switched on, then pick the requested keys out of the table
    // (colour: the per-sample scratch the ordered fold reads).
    const uint32_t tiles_x = (d.nx + d.tile_w - 1) / d.tile_w;
    const uint64_t pix_work = rank_pix_work(d);
    // per-slot accumulators, indexed by (workgroup * waves + wave): a CU holds at most 32 waves of these kernels, and the
    // `wg_per_cu` option may ask for more (queued) workgroups of up to 16 waves each
    const size_t trace_waves = (size_t)s->num_cus * std::max(32, s->wg_per_cu > 0 ? s->wg_per_cu * 16 : 0);
    const size_t table = (size_t)4 * d.ns * pix_work, slots = trace_waves * std::max(std::max(FPOOL, POOL), P2POOL) * 3;
    DevBuf<uint32_t> d_trace;
    HIP_TRY(d_trace.alloc(table + slots));
    HIP_TRY(hipMemset(d_trace.p, 0, (table + slots) * sizeof(uint32_t)));
    if ((rc = ctx_acquire(s))) return rc;
    HIP_TRY(s->frame.grow((size_t)d.nx * d.ny * 3 * sizeof(float)));
    HIP_TRY(hipMemset(s->cx->d_counters, 0, 32 * sizeof(unsigned long long)));
    const unsigned long long ptrs[2] = {(unsigned long long)(uintptr_t)d_trace.p, (unsigned long long)(uintptr_t)(d_trace.p + table)};
    HIP_TRY(hipMemcpy(s->cx->d_counters + 30, ptrs, sizeof(ptrs), hipMemcpyHostToDevice));
    const DevCamera cam = to_dev(camera);
    s->whole_scratch = true;  // the trace reads every sample colour back: one sample pass
    hipError_t e = launch_render<true>(s, cam, d, s->frame.as<float>(), nullptr, SampleSlice{}, FrameLayout(d.nx, d.ny, 0u), FrameBlocks{});
    s->whole_scratch = false;
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipMemset(s->cx->d_counters + 30, 0, 2 * sizeof(unsigned long long));
    if (e != hipSuccess) return hip_fail(e, "trace launch");
    if (s->cx->last_kernel == KernelKind::baseline || s->cx->last_pix_work == 0)
      return fail(RTG_ERR_UNSUPPORTED, "this scene / frame runs on the baseline kernel (or without the per-sample scratch): nothing to trace");
    std::vector<uint32_t> h_trace(table);
    std::vector<float> h_col((size_t)3 * d.ns * pix_work);
    HIP_TRY(hipMemcpy(h_trace.data(), d_trace.p, table * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_col.data(), s->cx->scratch.p, h_col.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
      const uint32_t x = xs[i], row = d.ny - 1u - ys[i], sm = samples[i];
      const uint32_t tx = x / d.tile_w, ty = row / d.tile_h, tile = ty * tiles_x + tx;
      if (x >= d.nx || ys[i] >= d.ny || sm >= d.ns || tile % d.nranks != d.rank) return fail(RTG_ERR_INVALID, "trace key outside this rank's frame");
      const uint32_t k = tile / d.nranks, lx = x - tx * d.tile_w, ly = row - ty * d.tile_h;  // = pixel_to_work (rt_pool.h)
      const uint32_t b = (ly >> 3) * (d.tile_w >> 3) + (lx >> 3);
      const size_t w = (size_t)k * d.tile_w * d.tile_h + b * 64u + (ly & 7u) * 8u + (lx & 7u);
      const size_t at = (size_t)sm * pix_work + w;
      for (int c = 0; c < 3; c++) out_rgb[3 * i + c] = h_col[3 * at + c];
      for (int c = 0; c < 4; c++) out_info[4 * i + c] = h_trace[4 * at + c];
    }
    return RTG_OK;
  }
  DevBuf<uint32_t> dx, dy, ds, dinfo;
  DevBuf<float> drgb;
  HIP_TRY(dx.alloc(n));
  HIP_TRY(dy.alloc(n));
  HIP_TRY(ds.alloc(n));
  HIP_TRY(dinfo.alloc(4 * n));
  HIP_TRY(drgb.alloc(3 * n));
  HIP_TRY(hipMemcpy(dx.p, xs, n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dy.p, ys, n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(ds.p, samples, n * 4, hipMemcpyHostToDevice));
  DevCamera cam = to_dev(camera);
  dim3 grid((uint32_t)((n + 63) / 64)), block(64);
  if (n && s->light_sampling && s->lights.n != 0u)  // scene option light_sampling: the sample of color_ls (rt_light.h)
    with_feat<false>(s, [&](auto feat) {
      constexpr uint32_t F = decltype(feat)::value;
      if constexpr (F != 0u)
        hipLaunchKernelGGL((debug_samples_light_kernel<F>), grid, block, 0, 0, s->dev, s->lights, cam, d, (uint32_t)n, dx.p, dy.p, ds.p, drgb.p, dinfo.p);
    });
  else if (n)
    with_feat<false>(s, [&](auto feat) {
      hipLaunchKernelGGL((debug_samples_kernel<decltype(feat)::value>), grid, block, 0, 0, s->dev, cam, d, (uint32_t)n, dx.p, dy.p, ds.p, drgb.p, dinfo.p);
    });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out_rgb, drgb.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_info, dinfo.p, 4 * n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTG_OK;
}

int rtg_tonemap_device(int device, size_t n, const float* d_rgb, uint8_t* d_out, void* hip_stream) {
  if (!d_rgb || !d_out) return fail(RTG_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(device));
  if (n) hipLaunchKernelGGL(tonemap_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, n, d_rgb, d_out);
  HIP_TRY(hipGetLastError());
  return RTG_OK;
}

int rtg_tonemap(int device, size_t n, const float* rgb, uint8_t* out) {
  if (!rgb || !out) return fail(RTG_ERR_INVALID, "null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(RTG_ERR_DEVICE, "no HIP device");
  HIP_TRY(hipSetDevice(device));
  DevBuf<float> di;
  DevBuf<uint8_t> dout;
  HIP_TRY(di.alloc(n));
  HIP_TRY(dout.alloc(n));
  HIP_TRY(hipMemcpy(di.p, rgb, n * sizeof(float), hipMemcpyHostToDevice));
  int rc = rtg_tonemap_device(device, n, di.p, dout.p, nullptr);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, dout.p, n, hipMemcpyDeviceToHost));
  return RTG_OK;
}

int rtg_debug_flatten(rtg_builder* b, const rtg_id* world, size_t n, uint32_t* n_instructions, uint32_t* features,
                      uint32_t* words_out, size_t capacity) {
  if (!b || (!world && n)) return fail(RTG_ERR_INVALID, "null argument");
  FlatScene fs;
  try {
    b->sb.flatten(world, n, &fs);
  } catch (const BuildError& e) {
    return fail(e.code, e.msg);
  }
  if (n_instructions) *n_instructions = (uint32_t)fs.lo.size();
  if (features) *features = fs.features;
  if (words_out) {
    size_t m = fs.lo.size() < capacity ? fs.lo.size() : capacity;
    for (size_t i = 0; i < m; i++) {
      std::memcpy(words_out + 8 * i, fs.lo[i].w, 16);
      std::memcpy(words_out + 8 * i + 4, fs.hi[i].w, 16);
    }
  }
  return RTG_OK;
}

int rtg_debug_flatten_pool2(rtg_builder* b, const rtg_id* world, size_t n, uint32_t* n_instructions, uint32_t* table_out,
                            uint32_t* words_out, size_t capacity) {
  if (!b || (!world && n)) return fail(RTG_ERR_INVALID, "null argument");
  FlatScene fs;
  try {
    b->sb.flatten(world, n, &fs);
  } catch (const BuildError& e) {
    return fail(e.code, e.msg);
  }
  if (n_instructions) *n_instructions = (uint32_t)fs.lo2.size();
  static_assert(sizeof(P2Table) == 24 * sizeof(uint32_t), "rtg_debug_flatten_pool2: table_out holds 24 words");
  if (table_out) std::memcpy(table_out, &fs.p2, sizeof(P2Table));
  if (words_out) {
    size_t m = fs.lo2.size() < capacity ? fs.lo2.size() : capacity;
    for (size_t i = 0; i < m; i++) {
      std::memcpy(words_out + 8 * i, fs.lo2[i].w, 16);
      std::memcpy(words_out + 8 * i + 4, fs.hi2[i].w, 16);
    }
  }
  return RTG_OK;
}

// The program the two entry points below inspect: `world` flattened by `b`, or the n_records x 8 `words` given.
static int debug_lean_program(const char* who, rtg_builder* b, const rtg_id* world, size_t n, const uint32_t* words, size_t n_records,
                              std::vector<Packet>* lo, std::vector<Packet>* hi, bool* lean) {
  *lean = true;
  if (words) {
    lo->resize(n_records), hi->resize(n_records);
    for (size_t i = 0; i < n_records; i++) {
      std::memcpy((*lo)[i].w, words + 8 * i, 16), std::memcpy((*hi)[i].w, words + 8 * i + 4, 16);
      const uint32_t op = (*hi)[i].w[3] & 0xffu;
      *lean = *lean && (op == OP_BOX || op == OP_SPHERE || op == OP_END) && !((*hi)[i].w[3] & F_MOVE);
      if (op == OP_BOX && (*hi)[i].w[2] >= n_records) return fail(RTG_ERR_INVALID, std::string(who) + ": a skip pointer leaves the program");
    }
  } else {
    if (!b || (!world && n)) return fail(RTG_ERR_INVALID, "null argument");
    FlatScene fs;
    try {
      b->sb.flatten(world, n, &fs);
    } catch (const BuildError& e) {
      return fail(e.code, e.msg);
    }
    *lean = (fs.features & FEAT_NOT_LEAN) == 0;
    lo->swap(fs.lo), hi->swap(fs.hi);
  }
  if (hi->size() > 0x7fffffffu) return fail(RTG_ERR_INVALID, std::string(who) + ": program too large");
  return RTG_OK;
}

// Host-only (include/rtiow_gpu_debug.h): the box plan of a lean program -- per record 0 kept, 1 box-chain follower, 2 pruned
// (rt_box_plan.h) -- by the function rtg_scene_create calls (which skips it for programs too large to be staged; this does not).  `words` (8 per record, as rtg_debug_flatten writes them) replaces the
// flattened world when given.  Returns the record count, or a negative error code.
int rtg_debug_box_plan(rtg_builder* b, const rtg_id* world, size_t n, const uint32_t* words, size_t n_records, uint8_t* mask_out,
                       size_t capacity) {
  std::vector<Packet> lo, hi;
  bool lean = true;
  int rc = debug_lean_program("rtg_debug_box_plan", b, world, n, words, n_records, &lo, &hi, &lean);
  if (rc) return rc;
  std::vector<uint8_t> follower(hi.size(), 0), mask(hi.size(), 0);
  if (lean && !hi.empty()) {
    box_chain_followers(reinterpret_cast<const uint32_t (*)[4]>(lo.data()), reinterpret_cast<const uint32_t (*)[4]>(hi.data()), hi.size(), follower.data());
    box_plan(reinterpret_cast<const uint32_t (*)[4]>(lo.data()), reinterpret_cast<const uint32_t (*)[4]>(hi.data()), hi.size(), follower.data(), mask.data());
  }
  if (mask_out) std::memcpy(mask_out, mask.data(), std::min(mask.size(), capacity));
  return (int)hi.size();
}

// Host-only (include/rtiow_gpu_debug.h): the production program of a lean program (rt_box_plan.h box_tree_rebuild), which record
// of the given program every record copies, and the plan over it -- by the functions rtg_scene_create calls.  Another program
// comes back unchanged with origin[i] = i and a mask of zeros.  Returns the record count, or a negative error code.
int rtg_debug_production_program(rtg_builder* b, const rtg_id* world, size_t n, const uint32_t* words, size_t n_records,
                                 uint32_t* words_out, uint32_t* origin_out, uint8_t* mask_out, size_t capacity) {
  std::vector<Packet> lo, hi;
  bool lean = true;
  int rc = debug_lean_program("rtg_debug_production_program", b, world, n, words, n_records, &lo, &hi, &lean);
  if (rc) return rc;
  const size_t m = hi.size();
  std::vector<Packet> plo(lo), phi(hi);
  std::vector<uint32_t> origin(m);
  std::vector<uint8_t> follower(m, 0), mask(m, 0);
  for (size_t i = 0; i < m; i++) origin[i] = (uint32_t)i;
  if (lean && m) {
    box_tree_rebuild(reinterpret_cast<const uint32_t (*)[4]>(lo.data()), reinterpret_cast<const uint32_t (*)[4]>(hi.data()), m,
                     reinterpret_cast<uint32_t (*)[4]>(plo.data()), reinterpret_cast<uint32_t (*)[4]>(phi.data()), origin.data());
    box_chain_followers(reinterpret_cast<const uint32_t (*)[4]>(plo.data()), reinterpret_cast<const uint32_t (*)[4]>(phi.data()), m, follower.data());
    box_plan(reinterpret_cast<const uint32_t (*)[4]>(plo.data()), reinterpret_cast<const uint32_t (*)[4]>(phi.data()), m, follower.data(), mask.data(), nullptr, BOX_PLAN_PROBES, BOX_TREE_PLAN);
  }
  const size_t k = std::min(m, capacity);
  for (size_t i = 0; words_out && i < k; i++) std::memcpy(words_out + 8 * i, plo[i].w, 16), std::memcpy(words_out + 8 * i + 4, phi[i].w, 16);
  if (origin_out) std::memcpy(origin_out, origin.data(), k * sizeof(uint32_t));
  if (mask_out) std::memcpy(mask_out, mask.data(), k);
  return (int)m;
}

// Host-only (include/rtiow_gpu_debug.h): the camera plan of a lean program from pass counts handed in -- the tree DP the launcher
// runs on the counts of the probe kernel (rt_box_plan.h BOX_PLAN_COUNTS), over the program as given (no rebuild: hand in the
// production program to plan what launches stage).  counts[i]: walks out of n_rays in which BOX i passed; any values are accepted.
// Returns the record count, or a negative error code.
int rtg_debug_camera_plan(rtg_builder* b, const rtg_id* world, size_t n, const uint32_t* words, size_t n_records, const uint32_t* counts,
                          uint64_t n_rays, uint8_t* mask_out, size_t capacity) {
  if (!counts) return fail(RTG_ERR_INVALID, "null argument");
  std::vector<Packet> lo, hi;
  bool lean = true;
  int rc = debug_lean_program("rtg_debug_camera_plan", b, world, n, words, n_records, &lo, &hi, &lean);
  if (rc) return rc;
  std::vector<uint8_t> follower(hi.size(), 0), mask(hi.size(), 0);
  if (lean && !hi.empty()) {
    box_chain_followers(reinterpret_cast<const uint32_t (*)[4]>(lo.data()), reinterpret_cast<const uint32_t (*)[4]>(hi.data()), hi.size(), follower.data());
    box_plan(reinterpret_cast<const uint32_t (*)[4]>(lo.data()), reinterpret_cast<const uint32_t (*)[4]>(hi.data()), hi.size(), follower.data(), mask.data(), nullptr, 0u,
             BOX_PLAN_COUNTS, counts, n_rays);
  }
  if (mask_out) std::memcpy(mask_out, mask.data(), std::min(mask.size(), capacity));
  return (int)hi.size();
}

int rtg_debug_math(int device, int op, size_t n, const float* in, const float* in2, float* out) {
  if (!in || !out || op < 0 || op > 6 || (op >= 5 && !in2)) return fail(RTG_ERR_INVALID, "bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(RTG_ERR_DEVICE, "no HIP device");
  HIP_TRY(hipSetDevice(device));
  DevBuf<float> di, di2, dout;
  HIP_TRY(di.alloc(n));
  HIP_TRY(di2.alloc(n));
  HIP_TRY(dout.alloc(n));
  HIP_TRY(hipMemcpy(di.p, in, n * sizeof(float), hipMemcpyHostToDevice));
  if (in2) HIP_TRY(hipMemcpy(di2.p, in2, n * sizeof(float), hipMemcpyHostToDevice));
  if (n) hipLaunchKernelGGL(debug_math_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, op, n, di.p, di2.p, dout.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, dout.p, n * sizeof(float), hipMemcpyDeviceToHost));
  return RTG_OK;
}

