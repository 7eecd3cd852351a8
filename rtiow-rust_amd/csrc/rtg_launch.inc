// rtg_launch.inc -- included by rtg_api.hip (after struct rtg_scene): which kernel renders a frame, with what launch geometry, scratch
// budget (sample passes), LDS image and cost-ordered queue.  Host code only.
// The per-sample colour scratches of a handle may take up to half of the free HBM (288 GB per MI355X) TOGETHER: every launch
// context of the ring (frames in flight) budgets its share, so four contexts cannot starve later allocations.
static uint64_t scratch_cap(int n_ctx) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return (16ull << 30) / (uint64_t)std::max(1, n_ctx);
  return (uint64_t)free_b / 2 / (uint64_t)std::max(1, n_ctx);
}

// Sample passes.  The pool kernels park every sample colour in a [sample][pixel work index] scratch (12 B each) that the
// ordered fold consumes; a frame whose scratch would exceed the budget (option scratch_mb, default half of the free HBM)
// or whose work items would overflow the 32-bit queue counter is rendered in several passes over consecutive sample
// ranges, the fold kernel carrying the running per-pixel sum from pass to pass (rt_pool.h ChunkMode::s_begin) -- the
// same left fold, bit for bit, with O(budget) instead of O(spp) memory.  Returns the samples per pass (>= 1).
static uint32_t samples_per_pass(const rtg_scene* s, uint64_t pix_work, uint32_t ns) {
  const uint64_t per_sample = pix_work * 3 * sizeof(float);
  uint64_t budget = s->scratch_limit ? s->scratch_limit : std::max<uint64_t>(scratch_cap(s->n_ctx), s->cx->scratch.bytes);
  if (s->whole_scratch) budget = ~0ull;
  uint64_t k = std::max<uint64_t>(1, budget / std::max<uint64_t>(per_sample, 1));
  k = std::min<uint64_t>(k, 0xfffffffeull / std::max<uint64_t>(pix_work, 1));  // work items of a pass: one 32-bit counter
  k = std::max<uint64_t>(1, std::min<uint64_t>(k, ns));
  const uint64_t n_pass = (ns + k - 1) / k;
  return (uint32_t)((ns + n_pass - 1) / n_pass);  // balanced passes
}

// Tile ownership (part of the ABI; rt_pool.h work_to_pixel is its device side): the tiles are numbered row-major and tile t
// belongs to rank t % nranks.  A rank's work items are its tiles x the tile area, rounded up to whole 256-item reservations
// (tiles smaller than 16 x 16 need not add up to one; the padding items lie beyond the rank's last tile, i.e. outside the
// image, and are skipped like the padding of ragged image sizes).
static uint64_t rank_pix_work(const DevParams& d) {
  const uint32_t tiles_x = (d.nx + d.tile_w - 1) / d.tile_w, tiles_y = (d.ny + d.tile_h - 1) / d.tile_h, tiles = tiles_x * tiles_y;
  const uint32_t owned = tiles > d.rank ? (tiles - d.rank + d.nranks - 1) / d.nranks : 0;
  return ((uint64_t)owned * d.tile_w * d.tile_h + 255u) & ~255ull;
}
// ... and the pixels of those tiles that lie inside the image, exactly (rtg_stats.samples)
static uint64_t owned_pixels(const DevParams& d) {
  uint64_t px = 0;
  uint32_t tiles_x = (d.nx + d.tile_w - 1) / d.tile_w, tiles_y = (d.ny + d.tile_h - 1) / d.tile_h;
  for (uint32_t ty = 0; ty < tiles_y; ty++)
    for (uint32_t tx = 0; tx < tiles_x; tx++) {
      if ((ty * tiles_x + tx) % d.nranks != d.rank) continue;
      uint32_t w = std::min(d.tile_w, d.nx - tx * d.tile_w), h = std::min(d.tile_h, d.ny - ty * d.tile_h);
      px += (uint64_t)w * h;
    }
  return px;
}

// ---- one pick per kernel family ------------------------------------------------------------------------------------------------
// The baseline walk's FEAT template argument for a scene (rt_trace.h), handed to `f` as a std::integral_constant: FEAT_DEEP graphs
// take the general walk, lean programs the lean one, every other scene the full one.  SIZED (render_kernel alone): the general
// walk instantiated for the graph's real depths (flat_scene.h FEAT_DEEP_FEW_WRAPPERS / FEAT_DEEP_ONE_LEVEL, option deep_sized);
// every other kernel keeps its largest instantiation: the same arithmetic.
template <bool SIZED, typename F>
static void with_feat(const rtg_scene* s, F&& f) {
  constexpr uint32_t D = FEAT_ALL | FEAT_DEEP;
  if ((s->features & FEAT_DEEP) && (s->features & FEAT_SURFACE)) return f(std::integral_constant<uint32_t, D | FEAT_TRI | FEAT_SURFACE>{});
  if ((s->features & FEAT_DEEP) && (s->features & FEAT_TRI)) return f(std::integral_constant<uint32_t, D | FEAT_TRI>{});  // (one size: the largest)
  if (s->features & FEAT_DEEP) {
    if constexpr (SIZED) {
      const bool few = s->deep_sized && (s->features & FEAT_DEEP_FEW_WRAPPERS) != 0, one = s->deep_sized && (s->features & FEAT_DEEP_ONE_LEVEL) != 0;
      if (few && one) return f(std::integral_constant<uint32_t, D | FEAT_DEEP_FEW_WRAPPERS | FEAT_DEEP_ONE_LEVEL>{});
      if (few) return f(std::integral_constant<uint32_t, D | FEAT_DEEP_FEW_WRAPPERS>{});
      if (one) return f(std::integral_constant<uint32_t, D | FEAT_DEEP_ONE_LEVEL>{});
    }
    return f(std::integral_constant<uint32_t, D>{});
  }
  if ((s->features & FEAT_NOT_LEAN) == 0) return f(std::integral_constant<uint32_t, 0u>{});
  if (s->features & FEAT_SURFACE) return f(std::integral_constant<uint32_t, FEAT_ALL | FEAT_TRI | FEAT_SURFACE>{});  // (attribute triangles: include/rtiow_gpu_surface.h)
  if (s->features & FEAT_TRI) return f(std::integral_constant<uint32_t, FEAT_ALL | FEAT_TRI>{});  // (the only walks with a TRI case)
  return f(std::integral_constant<uint32_t, FEAT_ALL>{});
}
// Runtime bools as template arguments: f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...).  For kernel families of which
// every combination is instantiated.
template <typename F>
static void with_bools(F&& f) {
  f();
}
template <typename F, typename... Rest>
static void with_bools(F&& f, bool b, Rest... rest) {
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

static hipError_t setup_lpt(rtg_scene* s, ChunkMode& cm, uint64_t capacity);
static void launch_pass_setup(rtg_scene* s, const LaunchConsts& c, uint32_t* queue, hipStream_t stream);

// hipFuncSetAttribute(max dynamic LDS) + the occupancy query of a (kernel, block, LDS) triple: the two runtime calls cost a
// small frame more than its kernels (tools/latency_probe.py), so they are made once per process.  The attribute belongs to
// the FUNCTION (per device), not to a scene handle, and the last call wins: it is raised once to all of a CU's LDS, so that
// handles (or frame sizes of one handle) that ask the same kernel for different amounts never lower it under each other.
// `per_cu`: the workgroups per CU a launch counts on -- option wg_per_cu when set, else the occupancy figure, at least one.
static hipError_t kernel_setup(rtg_scene* s, const void* kernel, int bt, size_t lds, int* per_cu) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> raised;                                // (device, kernel) -> the dynamic-LDS limit the function has now
  static std::map<std::tuple<int, const void*, int, size_t>, int> occupancy;                  // (device, kernel, block, LDS)
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = raised[std::make_pair(s->device, kernel)];
  if (have < lds) {
    // all of a CU's LDS -- as much of it as THIS device lets one workgroup have (160 KB on gfx950; a part with less must still
    // launch the scenes that fit it).  Should the device report less than this launch needs (or the raise fail), ask for exactly
    // what the launch needs; a later launch that needs more raises again (the limit is remembered, not a flag).
    static std::map<int, int> device_cap;
    int& cap = device_cap[s->device];
    if (cap == 0 && (hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, s->device) != hipSuccess || cap <= 0)) cap = 64 * 1024;
    const int want = std::min(160 * 1024, std::max(cap, (int)std::min<size_t>(lds, 160 * 1024)));
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, want);
    if (e == hipSuccess) {
      have = (size_t)want;
    } else {
      (void)hipGetLastError();
      e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      have = lds;
    }
  }
  const auto key = std::make_tuple(s->device, kernel, bt, lds);
  auto it = occupancy.find(key);
  if (it == occupancy.end()) {
    int n = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, bt, lds);
    if (e != hipSuccess) return e;
    it = occupancy.emplace(key, n).first;
  }
  *per_cu = s->wg_per_cu > 0 ? s->wg_per_cu : std::max(1, it->second);
  return hipSuccess;
}

// Launch geometry of a pool kernel.  A frame with fewer work items than the chip has lanes (total_work < 64 x 16 waves x CUs) is
// a LATENCY problem: with one 1024-thread workgroup per CU and 256-item reservations the 1 024 items of the reference's own
// benchmark frame (benches/scene.rs: 10 x 10 pixels x 4 samples, one 16 x 16 tile) were 4 waves of ONE CU running four generations
// of paths one after another.  Such a frame gets one work item per lane: reservations of 64, workgroups of as few waves as
// spread the items over all CUs (a small workgroup also stages the program into LDS per workgroup -- from L2 -- which is why large
// frames keep ONE 16-wave workgroup per CU).  In between (every lane busy, but fewer than four 256-item reservations per
// wave) the lean kernel's reservations shrink so that the waves finish within one generation of each other (`shrink_mid`;
// book-1 300x300x10: 1.15 -> 1.02 ms; on the full-feature kernel the 8x8-pixel reservations cost the Criterion scene 5 %).  The cost-ordered queue keeps
// 256 (its blocks are the reservations).  `bt_max`: the kernel variant's workgroup limit; `forced`: option `block`.
struct PoolGeometry { int bt; uint32_t grid, work_block; };
static PoolGeometry pool_geometry(const rtg_scene* s, uint64_t total_work, int bt_max, int forced_bt, uint32_t pool, bool shrink_mid) {
  PoolGeometry g;
  g.bt = forced_bt > 0 && forced_bt <= bt_max ? forced_bt : bt_max;
  g.work_block = WORK_BLOCK;
  const uint64_t lanes_worth = (total_work + 63) / 64;
  const uint64_t cus = (uint64_t)std::max(1, s->num_cus);
  if (s->small_frames && lanes_worth < cus * (uint64_t)(bt_max / 64)) {
    if (forced_bt <= 0) g.bt = 64 * (int)std::min<uint64_t>((uint64_t)(bt_max / 64), (lanes_worth + cus - 1) / cus);
    g.work_block = 64;
    g.grid = (uint32_t)std::max<uint64_t>(1, (lanes_worth + (uint64_t)(g.bt / 64) - 1) / (uint64_t)(g.bt / 64));
    return g;
  }
  const uint64_t waves = (uint64_t)(g.bt / 64);
  uint64_t want = (total_work + waves * pool - 1) / (waves * pool);  // a wave keeps `pool` paths in flight: no more waves than there is work for
  g.grid = (uint32_t)std::min<uint64_t>(want ? want : 1, 0xffffffffull);  // (the caller caps it at what the chip holds at once)
  if (s->small_frames && shrink_mid && total_work < std::min<uint64_t>(g.grid, cus) * waves * WORK_BLOCK * 4) g.work_block = 64;
  return g;
}

// A pool-kernel launch, decided before its first sample pass: the kernel, its block, dynamic LDS, geometry and workgroups per
// CU (kernel_setup), and the paths a wave keeps in flight as the cost-ordered queue counts them.
struct PoolLaunch {
  KernelKind kind;
  int bt, per_cu;
  size_t lds;
  PoolGeometry geo;
  uint32_t pool;
};

// The sample passes of a pool-kernel frame, ONE unless the scratch budget is smaller than the call's sample colours.
// `chunks(s0, end)`: the work items of the pass over samples [s0, end) (rt_pool.h ChunkMode, without the reservations and the
// cost-ordered queue); `issue(s0, dp, cm, grid, total_work)`: make room for the launch, write its constants, launch the kernel.
template <typename Chunks, typename Issue>
static hipError_t sample_passes(rtg_scene* s, const DevParams& d, float* d_out, hipStream_t stream, const SampleSlice& sl,
                                const PoolLaunch& L, uint32_t per_pass, Chunks chunks, Issue issue) {
  for (uint32_t s0 = sl.begin; s0 < d.ns; s0 += per_pass) {
    DevParams dp = d;
    dp.ns = std::min(d.ns, s0 + per_pass);  // the pass renders samples [s0, dp.ns)
    ChunkMode cm = chunks(s0, dp.ns);
    cm.work_block = L.geo.work_block;
    const uint64_t total_work = (uint64_t)cm.pix_work * cm.n_chunks;
    if (total_work > 0xfffffffeull) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(L.geo.grid, (uint64_t)s->num_cus * L.per_cu);
    hipError_t e = setup_lpt(s, cm, (uint64_t)grid * (uint32_t)(L.bt / 64) * L.pool);
    if (e != hipSuccess) return e;
    if (cm.lpt) cm.work_block = WORK_BLOCK;  // (its blocks are the reservations)
    e = issue(s0, dp, cm, grid, (uint32_t)total_work);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (cm.scratch && sl.counts) {  // RTG_FLAG_SAMPLE_COUNTS: the list's fold, per pixel up to e_p, never dividing (launch_counts resolves)
      void (*fold)(DevParams, ChunkMode, PixMap, float*, ListConsts) = sl.squares ? fold_samples_list_kernel<true> : fold_samples_list_kernel<false>;
      hipLaunchKernelGGL(fold, dim3((uint32_t)(((uint64_t)cm.pix_work + 255) / 256)), dim3(256), 0, stream, dp, cm, make_pixmap(dp), d_out, sl.list);
      e = hipGetLastError();
      if (e != hipSuccess) return e;
    } else if (cm.scratch) {  // (ns_frame 0 = never divide: RTG_FLAG_PARTIAL; RTG_FLAG_SUM_SQUARES: the fold that also sums the squares)
      void (*fold)(DevParams, ChunkMode, PixMap, float*, uint32_t) = sl.squares ? fold_samples_sq_kernel : fold_samples_kernel;
      hipLaunchKernelGGL(fold, dim3((uint32_t)(((uint64_t)cm.pix_work + 255) / 256)), dim3(256), 0, stream, dp, cm, make_pixmap(dp), d_out,
                         sl.divide ? d.ns : 0u);
      e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

// ---- camera plan (option box_camera; rt_camera_probe.h, rt_box_plan.h BOX_PLAN_COUNTS) ----------------------------------------
// The scene's plan (lean_plan) is made from box areas and knows nothing about where the rays go.  The pair (scene, camera)
// stays the same from call to call -- the slices of a progressive frame, the sample passes of a large one, repeated frames -- so
// the launcher keeps a plan per camera: the first launch that sees a camera enqueues the probe kernel in front of itself, with
// an asynchronous copy of the counts to pinned memory and an event behind it, and stages the scene's image; the next launch
// with that camera (the next sample pass of the same call included) waits for the event, runs the tree DP on the counts,
// uploads the offsets table on its stream and stages the camera's image, as does every launch after it.
//
// A launch probes when the probe costs it at most 1 %.  CAMERA_PLAN_MIN_SAMPLES = probe time / 1 % / time per sample:
//   probe kernel, book-1's rebuilt program (1 455 records), 4 108 paths x 2 bounces, at most 64 records per path, one MI355X
//     (rocprofv3 --kernel-trace --stats over tools/camera_plan_cost.py, 5 launches): 41 us, rounded up to 42 below (profiles/
//     r24_camera_plan/probe_kernel_stats.csv; the earlier versions of the kernel, 73 .. 126 us: README.txt there)
//   time per sample of the launches that gain, book-1 1200x800x50 on the parent commit: 6.01 ms / 48 M samples = 0.1252 ns
//   42 us / 1 % / 0.1252 ns = 33.5 M samples (book-1 1200x800x50 is 48 M)
constexpr uint64_t CAMERA_PLAN_MIN_SAMPLES = 33500000ull;

static hipError_t camera_plan_make(rtg_scene* s, const LeanImages& im, CameraPlan* e, bool chains, hipStream_t stream) {
  hipError_t err = hipEventSynchronize(e->ev);  // (recorded in front of the launch that probed: long past)
  if (err != hipSuccess) return err;
  const size_t n = im.h_hi->size();
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> mask(n), drop(n);
  e->n_rays = e->h_words[n];
  e->n_pruned = box_plan(reinterpret_cast<const uint32_t (*)[4]>(im.h_lo->data()), reinterpret_cast<const uint32_t (*)[4]>(im.h_hi->data()), n, im.follower.data(),
                         mask.data(), nullptr, 0u, BOX_PLAN_COUNTS, e->h_words, e->n_rays).n_pruned;
  for (size_t i = 0; i < n; i++) drop[i] = mask[i] == BOX_PRUNED || (chains && mask[i] == BOX_FOLLOWER);
  uint32_t* off = e->h_words + n + 1u;
  e->bytes = lds_image_offsets(im.plan_ops.data(), n, off, drop.data());
  e->plan_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if ((err = hipMemcpyAsync(e->d_off, off, n * sizeof(uint32_t), hipMemcpyHostToDevice, stream)) != hipSuccess) return err;
  if ((err = hipEventRecord(e->ev, stream)) != hipSuccess) return err;
  e->up_stream = stream, e->state = CameraPlan::PLANNED;
  if (s->verbose)
    fprintf(stderr, "[rtg] camera plan: %u rays probed, %u interior record(s) left out (the scene's plan: %u), image %u B, DP + table %.3f ms\n", e->n_rays, e->n_pruned,
            im.n_pruned, e->bytes, e->plan_ms);
  return hipSuccess;
}

// The camera's plan for a launch of `samples` samples that would stage the pruned image of `im` (`tree`: the rebuilt program):
// *out = the entry whose table the launch stages, nullptr = the scene's own.
static hipError_t camera_plan(rtg_scene* s, LeanImages& im, bool tree, const DevCamera& cam, hipStream_t stream, uint64_t samples, const CameraPlan** out) {
  *out = nullptr;
  if (!s->box_camera || !im.h_lo || !im.h_hi) return hipSuccess;
  const size_t n = im.h_hi->size();
  if (im.probe_ok < 0) {  // skip pointers point forward and nest: the probe's walk is bounded (rt_camera_probe.h)
    box_plan_detail::Shape shape;
    im.probe_ok = n == s->n_prog && n <= CAMERA_PROBE_MAX_RECORDS && box_plan_detail::program_shape(reinterpret_cast<const uint32_t (*)[4]>(im.h_lo->data()), reinterpret_cast<const uint32_t (*)[4]>(im.h_hi->data()), n, &shape) &&
                  shape.n_prunable != 0u;
  }
  if (!im.probe_ok) return hipSuccess;
  const bool chains = s->box_chains != 0;
  unsigned char key[CAMERA_KEY_BYTES];
  memcpy(key, &cam, sizeof(DevCamera));
  key[sizeof(DevCamera)] = tree ? 1 : 0, key[sizeof(DevCamera) + 1] = chains ? 1 : 0;
  CameraPlan* e = nullptr;
  for (CameraPlan& c : s->cam_plans)
    if (c.state != CameraPlan::FREE && !memcmp(c.key, key, CAMERA_KEY_BYTES)) e = &c;
  hipError_t err;
  if (!e) {
    if (s->box_camera == 1 && samples < CAMERA_PLAN_MIN_SAMPLES) return hipSuccess;
    for (CameraPlan& c : s->cam_plans)  // a free entry, else the least recently used
      if (c.state == CameraPlan::FREE && (!e || e->state != CameraPlan::FREE)) e = &c;
      else if (!e || (e->state != CameraPlan::FREE && c.stamp < e->stamp)) e = &c;
    if (e->state != CameraPlan::FREE) {  // evicted: kernels in flight, on whichever stream, may still read its table -- a fifth camera on a
                                         // handle waits for the whole device once (DESIGN.md "Camera plan", costs)
      if ((err = hipDeviceSynchronize()) != hipSuccess) return err;
      e->state = CameraPlan::FREE;
    }
    if (!e->ev && (err = hipEventCreateWithFlags(&e->ev, hipEventDisableTiming)) != hipSuccess) return err;
    if (!e->d_counts && (err = hipMalloc((void**)&e->d_counts, (n + 1u) * sizeof(uint32_t))) != hipSuccess) return err;
    if (!e->d_off) {
      if ((err = hipMalloc((void**)&e->d_off, n * sizeof(uint32_t))) != hipSuccess) return err;
      s->bytes += (2u * n + 1u) * sizeof(uint32_t);
    }
    if (!e->h_words && (err = hipHostMalloc((void**)&e->h_words, (2u * n + 1u) * sizeof(uint32_t))) != hipSuccess) return err;
    if (!im.d_stop) {
      std::vector<uint8_t> stop;
      camera_probe_stops(reinterpret_cast<const uint32_t (*)[4]>(im.h_lo->data()), reinterpret_cast<const uint32_t (*)[4]>(im.h_hi->data()), n, &stop);
      if ((err = hipMalloc((void**)&im.d_stop, n)) != hipSuccess) return err;
      if ((err = hipMemcpy(im.d_stop, stop.data(), n, hipMemcpyHostToDevice)) != hipSuccess) return err;
      s->bytes += n;
    }
    CameraProbe p{im.lo, im.hi, im.d_stop, e->d_counts, (uint32_t)n, 0u, 0u, (uint32_t)s->cam_bounces, (uint32_t)s->cam_trips, 0.001f};
    camera_probe_grid(cam, (uint32_t)s->cam_paths, &p.grid_w, &p.grid_h);
    if ((err = hipMemsetAsync(e->d_counts, 0, (n + 1u) * sizeof(uint32_t), stream)) != hipSuccess) return err;
    int probe_per_cu = 0;  // (raises the kernel's dynamic-LDS limit when the program needs more than the default 64 KB)
    if ((err = kernel_setup(s, (const void*)camera_probe_kernel, (int)CAMERA_PROBE_BLOCK, camera_probe_lds_bytes(n), &probe_per_cu)) != hipSuccess) return err;
    hipLaunchKernelGGL(camera_probe_kernel, dim3((p.grid_w * p.grid_h + CAMERA_PROBE_WALKERS - 1u) / CAMERA_PROBE_WALKERS), dim3(CAMERA_PROBE_BLOCK), camera_probe_lds_bytes(n), stream, p, cam);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if ((err = hipMemcpyAsync(e->h_words, e->d_counts, (n + 1u) * sizeof(uint32_t), hipMemcpyDeviceToHost, stream)) != hipSuccess) return err;
    if ((err = hipEventRecord(e->ev, stream)) != hipSuccess) return err;
    memcpy(e->key, key, CAMERA_KEY_BYTES);
    e->state = CameraPlan::PROBING, e->stamp = ++s->cam_clock;
    if (s->box_camera != 2) return hipSuccess;  // this launch stages the scene's image; the next one makes the plan
  }
  e->stamp = ++s->cam_clock;
  if (e->state == CameraPlan::PROBING && (err = camera_plan_make(s, im, e, chains, stream)) != hipSuccess) return err;
  if (e->up_stream != stream && (err = hipStreamWaitEvent(stream, e->ev, 0)) != hipSuccess) return err;
  *out = e;
  return hipSuccess;
}

// Lean scenes, ray-pool kernel (rt_pool.h): one persistent 1024-thread workgroup per CU.
// `sl`: the samples [sl.begin, d.ns) of a progressive frame's slice -- pass sizing, chunking and launch geometry follow this
// call's samples, not the frame's.  A counts call (sl.counts) runs over its list of active pixels: `pix_work` is the list's
// length, and the kernel the list variant (LIST; the 4-wide walk of option bvh4 is not instantiated for it: such a call takes
// the binary walk and reports its counters).
// `d_rays` (ray frames, rtg_rays.inc; nullptr: a camera frame): the launch has no camera -- `cam` is not read, the camera plan
// is skipped (the scene's own pruned image is staged: a plan changes cost, never bits) and the kernel is the RAYS instantiation,
// which exists for production launches of the binary walk only.  Everything else is a production launch's.
template <bool COUNT>
static hipError_t launch_pool(rtg_scene* s, const DevCamera& cam, const DevParams& d, float* d_out,
                              hipStream_t stream, const SampleSlice& sl, const float* d_rays = nullptr, uint32_t ray_mode = 0u) {
  if (d_rays && (COUNT || sl.counts)) return hipErrorNotSupported;
  const uint64_t pix_work = sl.counts ? sl.list_work : rank_pix_work(d);
  if (pix_work == 0) return hipSuccess;  // this rank owns no tile
  if (pix_work > 0xfffffffeull) return hipErrorInvalidValue;
  // Sample-chunk mode (see rt_pool.h).  Default: one sample per work item.  Work items are then ~100x more numerous than
  // path slots, so the end-of-frame tail (slots finishing their last item while the queue is empty) is negligible;
  // measured on C2: 40.6 ms with one pixel (50 samples) per item, 23.5 ms with one sample per item.
  const uint32_t ns_call = d.ns - sl.begin;  // samples of this call
  uint64_t n_chunks = ns_call;
  if (s->force_chunks > 0) n_chunks = (uint64_t)s->force_chunks;
  if (n_chunks > ns_call) n_chunks = ns_call;
  // else (ns = 1, or option chunks = 1): a slot folds its pixel's samples itself -- from +0, dividing at the end; a slice of a
  // progressive frame takes the chunk mode instead, whose fold kernel continues the running sum and divides only when asked,
  // and so does a call that sums the squares (the fold kernel squares every sample colour: one sample per work item), or
  // renders per-pixel counts (the fold stops at each pixel's own count)
  const bool use_scratch = n_chunks > 1 || sl.sliced() || sl.squares || sl.counts;
  uint32_t per_pass = d.ns, chunk = d.ns;
  if (use_scratch) {
    per_pass = samples_per_pass(s, pix_work, ns_call);
    chunk = (uint32_t)((ns_call + n_chunks - 1) / n_chunks);
    // several passes: one sample per work item; the same when the slice does not begin on a chunk boundary (the kernel ends a
    // work item where s % chunk == 0)
    if (per_pass < ns_call || sl.begin % chunk != 0u || sl.squares || sl.counts) chunk = 1u;
    hipError_t ea = s->cx->scratch.grow(pix_work * per_pass * 3 * sizeof(float));
    if (ea != hipSuccess) return ea;
  }
  s->cx->last_pix_work = use_scratch && per_pass == d.ns ? (uint32_t)pix_work : 0u;
  uint32_t* queue = (uint32_t*)(s->cx->d_counters + 7);
  // (geometry from the first pass's work: passes are balanced, so every pass of the frame gets the same one)
  const uint64_t work0 = pix_work * (use_scratch ? (std::min(ns_call, per_pass) + chunk - 1) / chunk : 1u);
  const PoolGeometry geo = pool_geometry(s, work0, RT_POOL_MAX_THREADS, s->pool_threads, POOL, true);
  const int bt = geo.bt;
  const uint32_t waves = (uint32_t)bt / 64;
  const size_t lds_limit = 160 * 1024;
  const bool wide = s->bvh4 && s->wide_bytes != 0 && !sl.counts && !d_rays;
  // production launches stage the image without box-chain followers (rt_pool.h box_chain_followers) and without the interior
  // boxes of the pruning plan (rt_box_plan.h); counting launches keep the full image, so that their counters and traces report
  // every test of the reference's walk (option box_prune = 2: they stage the pruned image too, and report the production walk's)
  // Option box_tree: those launches walk the program whose Bvh regions are rebuilt over the same leaf order (rt_box_plan.h
  // box_tree_rebuild) -- the same Sphere::hit calls in the same order, fewer box tests -- when the scene has one and its image
  // can be staged; its images are chosen by the same two options.
  const bool production = !COUNT || s->box_prune == 2;
  DevScene dev = s->dev;
  bool chains = false, prune = false;
  auto choose = [&](const LeanImages& im) {
    chains = !COUNT && !wide && s->box_chains && im.d_chain_off != nullptr;
    prune = !wide && s->box_prune && production && im.d_prune_off[s->box_chains ? 1 : 0] != nullptr;
    dev.lo = im.lo, dev.hi = im.hi, dev.lds_off = im.d_off, dev.lds_image_bytes = im.bytes;
    if (chains) dev.lds_off = im.d_chain_off, dev.lds_image_bytes = im.chain_bytes;
    if (prune) dev.lds_off = im.d_prune_off[s->box_chains ? 1 : 0], dev.lds_image_bytes = im.prune_bytes[s->box_chains ? 1 : 0];
  };
  bool tree = s->box_tree && s->tree.lo != nullptr && production && !wide && s->ref.lo != nullptr;
  if (tree) {
    choose(s->tree);
    if (pool_lds_bytes(dev.lds_image_bytes, s->n_mat, waves, true, false) > lds_limit) tree = false;  // (the global-memory walk keeps the reference program)
  }
  if (!tree && s->ref.lo != nullptr) choose(s->ref);
  LeanImages& im = tree ? s->tree : s->ref;
  // Option box_camera: a launch that stages the pruned image takes the table planned for the camera it renders with, once there
  // is one (camera_plan above).  The camera's image may be LARGER than the scene's: the area model leaves out a box that covers
  // half of its parent, the counts keep it when few of the probe's rays pass it (tests/test_camera_plan.py has such a program).
  // So the table is taken only where that is safe.  Before the launch is sized: when the image is no larger than the scene's, or
  // picks the same kernel (program staged, hot slot fields in LDS) -- a plan never moves a scene to a slower kernel.  In a later
  // pass of the call, whose dynamic LDS was sized below from the image of its first pass and which lays LDS out from the image
  // size it is given: only when the camera's image is no larger than that one; else the call keeps its table, and the next call
  // is sized for the camera's.
  const bool camera_ok = prune && !d_rays && pool_lds_bytes(dev.lds_image_bytes, s->n_mat, waves, true, false) <= lds_limit;
  const CameraPlan* cplan = nullptr;
  uint32_t sized_for = 0;  // the image the launch was sized for, 0 = not sized yet
  auto kernel_for = [&](uint32_t bytes) {  // bit 0: the program is staged, bit 1: the hot slot fields live in LDS
    const bool u = bytes != 0 && pool_lds_bytes(bytes, s->n_mat, waves, true, false) <= lds_limit;
    const bool r = s->ray_lds && pool_lds_bytes(bytes, s->n_mat, waves, u, true) <= lds_limit && (!u || bytes < (1u << 17));
    return (u ? 1u : 0u) | (r ? 2u : 0u);
  };
  auto camera_image = [&]() {
    if (!camera_ok || cplan) return hipSuccess;
    const CameraPlan* cp = nullptr;
    hipError_t ec = camera_plan(s, im, tree, cam, stream, pix_work * ns_call, &cp);
    if (ec != hipSuccess || !cp) return ec;
    const bool take = sized_for ? cp->bytes <= sized_for : (cp->bytes <= dev.lds_image_bytes || kernel_for(cp->bytes) == kernel_for(dev.lds_image_bytes));
    if (take) cplan = cp, dev.lds_off = cp->d_off, dev.lds_image_bytes = cp->bytes;
    else if (s->verbose) fprintf(stderr, "[rtg] camera plan: image %u B against %u B: not staged by this %s\n", cp->bytes, sized_for ? sized_for : dev.lds_image_bytes, sized_for ? "call" : "launch");
    return hipSuccess;
  };
  if (hipError_t ec = camera_image(); ec != hipSuccess) return ec;
  if (wide) dev.lds_off = s->d_wide, dev.lds_image_bytes = s->wide_bytes;  // the WIDE kernel's reading of these two
  const uint32_t image = dev.lds_image_bytes;
  sized_for = image;
  bool use_lds = image != 0 && pool_lds_bytes(image, s->n_mat, waves, true, false) <= lds_limit;
  if (wide && !use_lds) return hipErrorNotSupported;  // (rtg_scene_set_option refuses bvh4 for images that do not fit)
  // (hot slot fields in LDS keep best_pc as 16 bits = 14 bits of image offset / 8 + 2 bits of scatter tries: images < 128 KB)
  bool ray_lds = s->ray_lds && pool_lds_bytes(image, s->n_mat, waves, use_lds, true) <= lds_limit && (!use_lds || image < (1u << 17));
  size_t lds = pool_lds_bytes(image, s->n_mat, waves, use_lds, ray_lds);
  if (s->verbose && s->ray_lds && !ray_lds && use_lds && image >= (1u << 17) && pool_lds_bytes(image, s->n_mat, waves, use_lds, true) <= lds_limit)
    fprintf(stderr, "[rtg] pool: the LDS image is %u B (>= 128 KB): the slots' hot fields stay in global memory although they would fit LDS (their 16-bit best_pc holds image offsets / 8 < 2^14)\n", image);
  // A table, not with_bools: only 10 of the 16 (STAGED, RAY_LDS, WIDE, LIST) combinations exist -- the 4-wide walk has neither a
  // LIST nor an unstaged variant.
  void (*kernel)(DevScene, const LaunchConsts*, float*, uint32_t, uint32_t*, unsigned long long*, PoolTuning, uint32_t*);
  if (sl.counts) {
    if (ray_lds) kernel = use_lds ? render_lean_pool<true, COUNT, true, false, true> : render_lean_pool<false, COUNT, true, false, true>;
    else kernel = use_lds ? render_lean_pool<true, COUNT, false, false, true> : render_lean_pool<false, COUNT, false, false, true>;
  } else if (wide) kernel = ray_lds ? render_lean_pool<true, COUNT, true, true> : render_lean_pool<true, COUNT, false, true>;
  else if (ray_lds) kernel = use_lds ? render_lean_pool<true, COUNT, true> : render_lean_pool<false, COUNT, true>;
  else kernel = use_lds ? render_lean_pool<true, COUNT, false> : render_lean_pool<false, COUNT, false>;
  if constexpr (!COUNT) {
    if (d_rays) {
      if (ray_lds) kernel = use_lds ? render_lean_pool<true, false, true, false, false, true> : render_lean_pool<false, false, true, false, false, true>;
      else kernel = use_lds ? render_lean_pool<true, false, false, false, false, true> : render_lean_pool<false, false, false, false, false, true>;
    }
  }
  if (s->verbose && (chains || prune) && use_lds)
    fprintf(stderr, "[rtg] pool: %s program (%u region(s) rebuilt in %.2f ms), box chains: %u follower record(s)%s, box pruning: %u interior record(s)%s (%s plan %.2f ms): LDS image %u B, %u records of %u; without followers %u B, full image %u B\n",
            tree ? "rebuilt" : "reference", s->n_regions, s->tree_ms, im.n_followers, chains || (prune && s->box_chains) ? " dropped" : " kept", cplan ? cplan->n_pruned : im.n_pruned, prune ? " dropped" : " kept",
            cplan ? "the camera's" : "the scene's", cplan ? cplan->plan_ms : im.plan_ms, image,
            s->n_prog - (chains || (prune && s->box_chains) ? im.n_followers : 0u) - (prune ? (cplan ? cplan->n_pruned : im.n_pruned) : 0u), s->n_prog, im.chain_bytes ? im.chain_bytes : im.bytes, im.bytes);
  PoolLaunch L{KernelKind::lean_pool, bt, 0, lds, geo, POOL};
  hipError_t e = kernel_setup(s, (const void*)kernel, bt, lds, &L.per_cu);
  if (e != hipSuccess) return e;
  auto chunks = [&](uint32_t s0, uint32_t end) {
    ChunkMode cm{};
    cm.scratch = nullptr, cm.chunk = d.ns, cm.n_chunks = 1, cm.pix_work = (uint32_t)pix_work, cm.s_begin = s0;
    if (use_scratch) {
      cm.chunk = chunk;
      cm.n_chunks = (end - s0 + chunk - 1) / chunk;
      cm.scratch = s->cx->scratch.as<float>() - 3ull * s0 * pix_work;  // biased: sample s of work index w at scratch[3 * (s * pix_work + w)]
    }
    return cm;
  };
  auto issue = [&](uint32_t s0, const DevParams& dp, const ChunkMode& cm, uint32_t grid, uint32_t total_work) {
    if (s->verbose)
      fprintf(stderr, "[rtg] pool: samples [%u, %u) of %u: grid %u x %d threads, %d WG/CU, lds %zu B (program staged: %d, hot slot fields in LDS: %d), %u chunk(s) of %u samples, cost-ordered queue after %u chunk(s)\n",
              s0, dp.ns, d.ns, grid, bt, L.per_cu, lds, (int)use_lds, (int)ray_lds, cm.n_chunks, cm.chunk, (cm.lpt_samples - (cm.lpt_samples ? s0 : 0u)) / (cm.chunk ? cm.chunk : 1u));
    hipError_t eg = s->cx->slots.grow((size_t)grid * waves * POOL * POOL_FIELDS * sizeof(uint32_t));
    if (eg != hipSuccess) return eg;
    if (s0 != sl.begin && (eg = camera_image()) != hipSuccess) return eg;  // (a later pass: the plan its first pass probed for)
    LaunchConsts c{cam, dp, cm, make_pixmap(dp)};
    c.rays = d_rays, c.ray_mode = ray_mode;
    launch_pass_setup(s, c, queue, stream);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(bt), lds, stream, dev, (const LaunchConsts*)s->cx->d_consts, d_out, total_work, queue,
                       s->cx->d_counters, s->pool_tune, s->cx->slots.as<uint32_t>());
    return hipSuccess;
  };
  return sample_passes(s, d, d_out, stream, sl, L, per_pass, chunks, issue);
}

// The 4-wide image of a lean program that is ONE Bvh over spheres (rt_pool.h WIDE; option `bvh4`): every node record holds
// the boxes of up to four GRANDCHILDREN of a node of the reference's tree (bvh.rs:22-81), in the reference's left-to-right
// order, so that a traversal step tests four boxes at once and the leaves are still met in the reference's order.  Returns
// false when the program has another shape (list-level objects, bare leaves, more than 8 levels).
static bool build_wide_image(const Packet* lo, const Packet* hi, size_t n, std::vector<uint32_t>& out) {
  struct T { uint32_t box; int left, right; uint32_t sphere; };  // left < 0: a leaf (box + sphere)
  std::vector<T> nodes;
  auto op_of = [&](size_t i) { return hi[i].w[3] & 0xffu; };
  if (n < 4 || op_of(n - 1) != OP_END || op_of(0) != OP_BOX || hi[0].w[2] != n - 1) return false;
  bool ok = true;
  std::function<int(size_t, size_t&)> parse = [&](size_t i, size_t& end) -> int {
    if (i >= n || op_of(i) != OP_BOX) { ok = false; end = i + 1; return -1; }
    end = hi[i].w[2];
    const int id = (int)nodes.size();
    nodes.push_back(T{(uint32_t)i, -1, -1, 0});
    if (op_of(i + 1) == OP_SPHERE) {
      if (end != i + 2) ok = false;
      nodes[id].sphere = (uint32_t)(i + 1);
      return id;
    }
    size_t e1 = 0, e2 = 0;
    const int l = parse(i + 1, e1);
    if (!ok || e1 >= end) { ok = false; return id; }
    const int r = parse(e1, e2);
    if (e2 != end) ok = false;
    nodes[id].left = l, nodes[id].right = r;
    return id;
  };
  size_t end0 = 0;
  const int root = parse(0, end0);
  if (!ok || root < 0 || nodes[root].left < 0) return false;
  out.clear();
  auto alloc = [&](uint32_t bytes) { const uint32_t at = (uint32_t)out.size() * 4u; out.resize(out.size() + bytes / 4u, 0u); return at; };
  std::function<uint32_t(int, uint32_t, uint32_t)> emit = [&](int t, uint32_t parent, uint32_t level) -> uint32_t {
    if (level > 7u) { ok = false; return 0; }
    const uint32_t at = alloc(WIDE_NODE_BYTES);
    int entry[4];
    uint32_t n_ch = 0;
    for (int x : {nodes[t].left, nodes[t].right}) {
      if (nodes[x].left < 0) entry[n_ch++] = x;
      else entry[n_ch++] = nodes[x].left, entry[n_ch++] = nodes[x].right;
    }
    uint32_t child[4] = {0, 0, 0, 0}, leafmask = 0;
    for (uint32_t k = 0; k < n_ch; k++) {
      const T e = nodes[entry[k]];
      const Packet bl = lo[e.box], bh = hi[e.box];  // (min.x, max.x, min.y, max.y) (min.z, max.z, ..)
      uint32_t* b = out.data() + at / 4u + 4u + 12u * k;  // (min, max) pairs, then (max, min) pairs: rt_pool.h
      b[0] = bl.w[0], b[1] = bl.w[1], b[2] = bl.w[2], b[3] = bl.w[3], b[4] = bh.w[0], b[5] = bh.w[1];
      b[6] = bl.w[1], b[7] = bl.w[0], b[8] = bl.w[3], b[9] = bl.w[2], b[10] = bh.w[1], b[11] = bh.w[0];
      if (e.left < 0) {
        const uint32_t sp = alloc(WIDE_SPHERE_BYTES);
        uint32_t* r = out.data() + sp / 4u;
        r[0] = hi[e.sphere].w[2], r[1] = hi[e.sphere].w[3];
        r[2] = lo[e.sphere].w[0], r[3] = lo[e.sphere].w[1], r[4] = lo[e.sphere].w[2], r[5] = lo[e.sphere].w[3];
        r[6] = at, r[7] = 0u;
        child[k] = sp, leafmask |= 1u << k;
      } else {
        child[k] = emit(entry[k], at, level + 1u);
      }
    }
    uint32_t* h = out.data() + at / 4u;
    h[0] = parent, h[1] = LDS_BOX_BIT | OP_BOX | (level << 8) | (n_ch << 12) | (leafmask << 16);
    h[2] = (child[0] >> 3) | ((child[1] >> 3) << 16), h[3] = (child[2] >> 3) | ((child[3] >> 3) << 16);
    return at;
  };
  emit(root, WIDE_NO_PARENT, 0u);
  return ok && out.size() * 4u < 512u * 1024u;
}

// Cost-ordered work queue (rt_pool.h, ChunkMode): enabled when the frame has enough chunks for a measuring
// phase and enough blocks to order.  This decides and sizes; the descriptor and the zeroed counters reach the device with the
// pass's constants (launch_pass_setup), every pass.
static hipError_t setup_lpt(rtg_scene* s, ChunkMode& cm, uint64_t capacity) {
  cm.lpt = nullptr, cm.lpt_samples = 0, cm.lpt_deep = 0;
  const uint32_t n_blocks = cm.pix_work / LPT_BLOCK;
  if (!s->lpt || !cm.scratch || cm.n_chunks < 6 || n_blocks < 64 || n_blocks > 65536 || cm.pix_work % LPT_BLOCK) return hipSuccess;
  // Phase 1 must outlast the first fill of the pools (`capacity` paths in flight) by enough for the
  // counts to mean something when the blocks are filed; it may take up to a third of the frame.
  uint32_t phase1 = std::max<uint32_t>(std::min(8u, std::max(2u, cm.n_chunks / 8u)), (uint32_t)((2 * capacity + cm.pix_work - 1) / cm.pix_work));
  if (s->lpt_phase1 > 0) phase1 = (uint32_t)s->lpt_phase1;
  if (phase1 < 1 || phase1 > cm.n_chunks / 3) return hipSuccess;
  // layout: [descriptor, 64 B] [cost n] [ctl LPT_CTL] [list LPT_CLASSES x n]
  const size_t words = 16 + (size_t)n_blocks * (1 + LPT_CLASSES) + LPT_CTL;
  hipError_t e = s->cx->lpt.grow(words * sizeof(uint32_t));
  if (e != hipSuccess) return e;
  LptQueue q;
  memset(&q, 0, sizeof(q));
  static_assert(sizeof(LptQueue) <= 64, "descriptor slot");
  q.cost = s->cx->lpt.as<uint32_t>() + 16, q.ctl = q.cost + n_blocks, q.list = q.ctl + LPT_CTL;
  q.n_blocks = n_blocks, q.phase1 = phase1;
  q.phase2_base = phase1 * cm.pix_work;
  q.span = LPT_BLOCK * (cm.n_chunks - phase1);
  q.mode = (uint32_t)s->lpt, q.shift = (uint32_t)s->lpt_shift;
  s->cx->lpt_desc = q;
  cm.lpt = reinterpret_cast<const LptQueue*>(s->cx->lpt.as<uint32_t>());
  cm.lpt_samples = cm.s_begin + phase1 * cm.chunk;  // samples [s_begin, lpt_samples) of every pixel: phase 1 of this pass
  cm.lpt_deep = (uint32_t)s->lpt_deep;
  return hipSuccess;
}

// The one stream operation in front of a pass's render kernel (rt_pool.h write_pass_setup): constants, queue head and, when
// setup_lpt switched the cost-ordered queue on for this pass (c.cm.lpt), its descriptor and zeroed counters -- on the launch
// stream, so ordered with the render kernels before and after.
static void launch_pass_setup(rtg_scene* s, const LaunchConsts& c, uint32_t* queue, hipStream_t stream) {
  const bool lpt = c.cm.lpt != nullptr;
  const LptQueue q = lpt ? s->cx->lpt_desc : LptQueue{};
  hipLaunchKernelGGL(write_pass_setup, dim3(1), dim3(256), 0, stream, s->cx->d_consts, c, (unsigned long long*)queue,
                     lpt ? reinterpret_cast<LptQueue*>(s->cx->lpt.as<uint32_t>()) : (LptQueue*)nullptr, q, lpt ? q.n_blocks + LPT_CTL : 0u);
}

// Full-feature scenes, ray-pool kernel (rt_pool_full.h) or, for list worlds without a Bvh, the lock-step kernel
// (rt_sync_full.h): always one sample per work item + ordered fold, in as many sample passes as the scratch budget asks for.
// (`sl`: as in launch_pool; a counts call takes the LIST variant of whichever kernel its list's work picks)
template <bool COUNT>
static hipError_t launch_full_pool(rtg_scene* s, const DevCamera& cam, const DevParams& d, float* d_out,
                                   hipStream_t stream, const SampleSlice& sl) {
  const uint64_t pix_work = sl.counts ? sl.list_work : rank_pix_work(d);
  if (pix_work == 0) return hipSuccess;
  if (pix_work > 0xfffffffeull) return hipErrorInvalidValue;
  const uint32_t ns_call = d.ns - sl.begin;  // samples of this call
  const uint32_t per_pass = samples_per_pass(s, pix_work, ns_call);
  const bool tex = (s->features & FEAT_TEXTURE) != 0;
  // ONE 16-wave workgroup per CU shares one LDS copy of the program (128 VGPRs per lane).
  const int bt_max = tex ? RT_FULL_TEX_THREADS : 1024;
  const PoolGeometry geo = pool_geometry(s, pix_work * std::min(ns_call, per_pass), bt_max, s->full_threads, FPOOL, false);
  const int bt = geo.bt;
  const uint32_t waves = (uint32_t)bt / 64;
  hipError_t e = s->cx->scratch.grow(pix_work * per_pass * 3 * sizeof(float));
  if (e != hipSuccess) return e;
  s->cx->last_pix_work = per_pass == d.ns ? (uint32_t)pix_work : 0u;
  uint32_t* queue = (uint32_t*)(s->cx->d_counters + 7);
  // Program placement: the whole program in LDS when it fits, else a leading window
  // (depth-first order: the window holds whole leading subtrees) and global memory for the rest.
  const size_t list_bytes = full_pool_lds_bytes(0, waves);
  const size_t budget = 160 * 1024;  // all of a CU's LDS: one workgroup per CU
  uint32_t window = s->n_prog;
  int prog = 1;
  if ((size_t)window * 32 + list_bytes > budget) window = (uint32_t)((budget - list_bytes) / 32), prog = 2;
  if (s->window >= 0) {
    window = std::min<uint32_t>(s->n_prog, (uint32_t)s->window);
    prog = window == 0 ? 0 : (window == s->n_prog ? 1 : 2);
  }
  // the material records ride behind the program when LDS has the room (a few hundred bytes for the reference's scenes)
  const size_t mat_bytes = (size_t)s->n_mat * 32;
  const bool mats_in_lds = s->mat_lds > 0 && prog == 1 && full_pool_lds_bytes(window, waves) + mat_bytes <= budget;
  const size_t lds = full_pool_lds_bytes(window, waves) + (mats_in_lds ? mat_bytes : 0);
  void (*kernel)(DevScene, const LaunchConsts*, float*, uint32_t, uint32_t*, unsigned long long*, PoolTuning, uint32_t*, float*,
                 uint32_t) = nullptr;
  const bool genb = (s->features & FEAT_BOUNDARY) != 0;  // a medium bounded by an object graph: the nested-walk variant
  void (*sync_kernel)(DevScene, const LaunchConsts*, float*, uint32_t, uint32_t*, unsigned long long*, PoolTuning, float*, uint32_t) = nullptr;
  void (*pool2_kernel)(DevScene, const LaunchConsts*, float*, uint32_t, uint32_t*, unsigned long long*, Pool2Tuning, uint32_t*, const P2Table*) = nullptr;
  // a program with FEAT_TRI: the instantiations that execute OP_TRI records (rt_pool_full.h TRI) -- no LIST ones (launch_slice sends a
  // counts call of such a scene to the baseline kernel) and never the pool-2 kernel (such a scene has no second program)
  // ... with FEAT_SURFACE (attribute triangles, include/rtiow_gpu_surface.h): their SURF siblings, chosen the same way
  const bool tri = (s->features & FEAT_TRI) != 0, surf = (s->features & FEAT_SURFACE) != 0;
  // ... with FEAT_ENVIRONMENT (include/rtiow_gpu_environment.h): the PROG_ENV instantiations (rt_pool_full.h), which exist with TEX and
  // without GENB and LIST alone (launch_slice sends the other frames of such a scene to the baseline kernel); no pool-2 kernel
  const bool env = (s->features & FEAT_ENVIRONMENT) != 0;
  with_bools([&](auto tex_c, auto genb_c, auto list_c, auto tri_c, auto surf_c, auto env_c) {  // (a counts call: the LIST variants; the pool-2 kernel has no GENB one)
    constexpr bool T = decltype(tex_c)::value, G = decltype(genb_c)::value, LI = decltype(list_c)::value, TR = decltype(tri_c)::value, SU = decltype(surf_c)::value;
    if constexpr (decltype(env_c)::value) {
      if constexpr (T && !G && !LI && (TR || !SU)) {
        constexpr int E = PROG_ENV;
        kernel = prog == 0 ? render_full_pool<0 + E, true, COUNT, false, false, TR, SU> : (prog == 1 ? render_full_pool<1 + E, true, COUNT, false, false, TR, SU> : render_full_pool<2 + E, true, COUNT, false, false, TR, SU>);
        sync_kernel = render_full_sync<1 + E, true, COUNT, false, false, TR, SU>;
      }
    } else if constexpr (TR) {
      if constexpr (!LI) {
        kernel = prog == 0 ? render_full_pool<0, T, COUNT, G, false, true, SU> : (prog == 1 ? render_full_pool<1, T, COUNT, G, false, true, SU> : render_full_pool<2, T, COUNT, G, false, true, SU>);
        sync_kernel = render_full_sync<1, T, COUNT, G, false, true, SU>;
      }
    } else if constexpr (!SU) {
      kernel = prog == 0 ? render_full_pool<0, T, COUNT, G, LI> : (prog == 1 ? render_full_pool<1, T, COUNT, G, LI> : render_full_pool<2, T, COUNT, G, LI>);
      sync_kernel = render_full_sync<1, T, COUNT, G, LI>;
      pool2_kernel = render_full_pool2<T, COUNT, LI>;
    }
  }, tex, genb, sl.counts, tri, surf, env);
  if (!kernel) return hipErrorInvalidValue;  // (a counts call on a FEAT_TRI program, a counts call or a FEAT_BOUNDARY program under an environment: not routed here)
  // The lock-step kernel (rt_sync_full.h: one path per lane, no stacks, no pools) renders list worlds without a Bvh -- and, by
  // default (option sync = -1), programs whose Bvhs are tiny (<= 32 BOX records: the Criterion scene of benches/scene.rs has 15,
  // volume_test under bvh::from_scene 5; a box loop has nothing to batch there) and frames with fewer work items than the chip has
  // waves' worth of lanes per CU (latency-bound launches: the pool kernel's services and stack traffic are a cost per generation
  // that only pays at width).  Measured, pool -> lock-step (profiles/r05_experiments/r05f_lockstep_rule.txt): scene/par/10x10x4
  // 469 -> 344 us, 100x100x4 641 -> 485 us, 300x300x10 1.19 -> 0.94 ms, volume_bvh 600x600x50 13.1 -> 11.0 ms, book-2 32x32x8
  // 2.2 -> 1.8 ms; book-2 100x100x10 and larger stay on the pool kernel (2.5 vs 3.0 ms).
  const bool tiny_bvh = s->n_box <= 32u;
  const bool tiny_frame = pix_work * std::min(ns_call, per_pass) <= (uint64_t)std::max(1, s->num_cus) * 64u;
  const bool lock_step = (s->sync_full > 0 || (s->sync_full < 0 && (s->n_box == 0 || tiny_bvh || tiny_frame))) && prog == 1;
  // The pool-2 kernel (rt_pool2.h) for programs that have a second program (flat_scene.h "the list level, hoisted"), when that
  // program and the waves' lists fit LDS whole; option pool2 = 0 keeps the first kernel (A/B).
  // (pool2 = 1: frames of >= 32 M samples -- the pool-2 kernel's slope is 11 % lower, its fixed cost per launch 1.7 ms higher:
  // profiles/r06_experiments/r06c_pool2_tail_probe.txt; pool2 = 2: every frame)
  const bool p2_size_ok = s->pool2 > 1 || pix_work * (uint64_t)ns_call >= (32ull << 20);
  const bool mats3 = s->mat_lds > 0 && pool2_lds_bytes(s->n_prog2, s->n_mat, waves) <= budget;
  const size_t lds3 = pool2_lds_bytes(s->n_prog2, mats3 ? s->n_mat : 0u, waves);
  const bool pool2 = s->pool2 > 0 && p2_size_ok && s->n_prog2 != 0 && !lock_step && !genb && lds3 <= budget;
  // The launch of the kernel that takes the frame.  The first kernel is set up whichever wins, and before the winner: the LDS
  // raise and the occupancy query are cached per function.
  PoolLaunch L{KernelKind::full_pool, bt, 0, lds, geo, FPOOL};  // (FPOOL for all three: the queue's phase 1 as the first kernel sizes it)
  LaunchConsts consts{};  // the launch constants particular to the kernel (parent, mat_lds, seg_first / seg_end, p2_lists)
  consts.parent = s->d_parent;
  e = kernel_setup(s, (const void*)kernel, bt, lds, &L.per_cu);
  if (e != hipSuccess) return e;
  if (lock_step) {
    L.kind = KernelKind::lock_step;
    L.lds = (size_t)window * 32;
    // the lock-step kernel keeps ONE path per lane (64 per wave, not the pool kernel's FPOOL): its grid comes from that, and
    // the cap from ITS occupancy -- with the pool kernel's figures a frame of 0.3 .. 0.9 M work items left CUs idle
    L.geo = pool_geometry(s, pix_work * std::min(ns_call, per_pass), bt_max, s->full_threads, 64u, false);
    if (L.geo.bt != bt) L.geo = geo;  // (one block size serves both: the stack and slot buffers below are sized by `waves`)
    e = kernel_setup(s, (const void*)sync_kernel, bt, L.lds, &L.per_cu);
  } else if (pool2) {
    L.kind = KernelKind::pool2;
    L.lds = lds3;
    const uint32_t tab = s->n_prog2 * 32u + DC_WORDS * 4u;
    consts.mat_lds = mats3 ? tab + P2_TABLE_BYTES : 0u;
    consts.p2_lists = tab + P2_TABLE_BYTES + (mats3 ? s->n_mat * 32u : 0u);
    e = kernel_setup(s, (const void*)pool2_kernel, bt, L.lds, &L.per_cu);
  } else {
    // (pool kernel only: book-2 -1 %, book2_bvh -0.7 %; the lock-step kernel measured 2 % slower on Cornell with its materials in LDS)
    if (mats_in_lds) consts.mat_lds = (uint32_t)full_pool_lds_bytes(window, waves);
    if (s->hoist > 0 && s->seg_end > s->seg_first) consts.seg_first = s->seg_first * RSZ, consts.seg_end = s->seg_end * RSZ;
  }
  if (e != hipSuccess) return e;
  s->cx->last_kernel = L.kind;
  auto chunks = [&](uint32_t s0, uint32_t end) {
    ChunkMode cm{};
    cm.scratch = s->cx->scratch.as<float>() - 3ull * s0 * pix_work, cm.chunk = 1u, cm.n_chunks = end - s0, cm.pix_work = (uint32_t)pix_work, cm.s_begin = s0;
    cm.drain_share = (uint32_t)std::max(0, s->drain_share);
    return cm;
  };
  auto issue = [&](uint32_t s0, const DevParams& dp, const ChunkMode& cm, uint32_t grid, uint32_t total_work) {
    hipError_t eg = s->cx->slots.grow((size_t)grid * std::max(full_pool_wg_words(waves), pool2_slot_words(waves)) * sizeof(uint32_t));
    if (eg != hipSuccess) return eg;
    eg = s->cx->stack.grow((size_t)grid * waves * (genb ? 2 : 1) * MAX_XFORM_DEPTH * 6 * 64 * sizeof(float));
    if (eg != hipSuccess) return eg;
    // (the lock-step kernel reports as the first kernel, with that kernel's LDS figure)
    const bool p2 = L.kind == KernelKind::pool2;
    if (s->verbose)
      fprintf(stderr, "[rtg] full pool%s: samples [%u, %u) of %u: grid %u x %d threads, %d WG/CU, lds %zu B (program window: %u of %u records), cost-ordered queue after %u chunk(s)\n",
              p2 ? " 2 (second program)" : "", s0, dp.ns, d.ns, grid, bt, L.per_cu, p2 ? lds3 : lds, p2 ? s->n_prog2 : window, p2 ? s->n_prog2 : s->n_prog,
              cm.lpt_samples - (cm.lpt_samples ? s0 : 0u));
    LaunchConsts c = consts;
    c.cam = cam, c.P = dp, c.cm = cm, c.pm = make_pixmap(dp);
    launch_pass_setup(s, c, queue, stream);
    if (L.kind == KernelKind::lock_step)
      hipLaunchKernelGGL(sync_kernel, dim3(grid), dim3(bt), L.lds, stream, s->dev, (const LaunchConsts*)s->cx->d_consts, d_out, total_work, queue,
                         s->cx->d_counters, s->sync_tune, s->cx->stack.as<float>(), window);
    else if (p2)
      hipLaunchKernelGGL(pool2_kernel, dim3(grid), dim3(bt), L.lds, stream, s->dev2, (const LaunchConsts*)s->cx->d_consts, d_out, total_work, queue,
                         s->cx->d_counters, s->pool2_tune, s->cx->slots.as<uint32_t>(), s->d_p2);
    else
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(bt), L.lds, stream, s->dev, (const LaunchConsts*)s->cx->d_consts, d_out, total_work, queue,
                         s->cx->d_counters, s->full_tune, s->cx->slots.as<uint32_t>(), s->cx->stack.as<float>(), window);
    return hipSuccess;
  };
  return sample_passes(s, d, d_out, stream, sl, L, per_pass, chunks, issue);
}

// The resolve step of a progressive frame (a call with sample_begin = ns and no RTG_FLAG_PARTIAL): divide the running sum of
// every owned pixel by ns.  Work items as in the pool kernels (work_to_pixel), so it follows the tiles whichever kernel
// rendered the samples.
static hipError_t launch_resolve(const DevParams& d, float* d_out, hipStream_t stream) {
  const uint64_t pix_work = rank_pix_work(d);
  if (pix_work == 0) return hipSuccess;
  if (pix_work > 0xfffffffeull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(resolve_sum_kernel, dim3((uint32_t)((pix_work + 255) / 256)), dim3(256), 0, stream, d, make_pixmap(d), (uint32_t)pix_work, d_out);
  return hipGetLastError();
}

// ... and of a counts frame: every owned pixel with e_p > 0 divided by e_p = min(n_p, ns)
static hipError_t launch_resolve_counts(const DevParams& d, float* d_out, hipStream_t stream, const FrameLayout& L) {
  const uint64_t pix_work = rank_pix_work(d);
  if (pix_work == 0) return hipSuccess;
  if (pix_work > 0xfffffffeull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(resolve_counts_kernel, dim3((uint32_t)(pix_work / 256u)), dim3(256), 0, stream, d, make_pixmap(d), (uint32_t)pix_work, d_out,
                     L.at(reinterpret_cast<const uint32_t*>(d_out), L.counts));
  return hipGetLastError();
}

// RTG_FLAG_RETIRE (include/rtiow_gpu.h): the retire step of a counts call over this rank's work items (rt_retire.h) -- mark the
// OK bits and the estimate's partials, retire the candidates whose window is OK, sum the partials into the caller's block.
// `r`: the block's in-fields, already validated.  A rank without work items (pix_work = 0) only writes the block's zeros.
// A frame with an error plane (RTG_FLAG_DENOISE_ERROR): the rule reads that plane, which the filter of this call has written,
// instead of (S, Q) -- launch_post_steps orders the two.
static hipError_t launch_retire(rtg_scene* s, const DevParams& d, float* d_out, hipStream_t stream, const FrameLayout& L, uint64_t pix_work,
                                const rtg_retire& r) {
  const uint32_t n_blk = (uint32_t)(pix_work / 256u);
  const float* errp = L.at(d_out, L.error);
  RetireBufs b;
  b.pitch = (d.nx + 31u) / 32u + 1u;
  // [blk_se2: f64 x n_blk] [blk_held: u64 x n_blk] [blk_u32: 3 x n_blk] [okbits: ny x pitch words]
  hipError_t e = s->cx->retire.grow((size_t)n_blk * 28u + (size_t)d.ny * b.pitch * 4u);
  if (e != hipSuccess) return e;
  b.blk_se2 = s->cx->retire.as<double>();
  b.blk_held = reinterpret_cast<unsigned long long*>(b.blk_se2 + n_blk);
  b.blk_u32 = reinterpret_cast<uint32_t*>(b.blk_held + n_blk);
  b.okbits = b.blk_u32 + 3ull * n_blk;
  b.planes = d_out;
  b.counts = reinterpret_cast<uint32_t*>(d_out) + L.counts;
  b.block = reinterpret_cast<uint32_t*>(d_out) + L.retire;
  b.errp = errp;
  const RetireArgs a{r.target_se, d.ns, r.min_samples, r.radius};
  if (n_blk != 0u) {
    const PixMap pm = make_pixmap(d);
    if (errp) hipLaunchKernelGGL(retire_mark_error_kernel, dim3(n_blk), dim3(256), 0, stream, d, pm, a, b, r.target_se * r.target_se);
    else hipLaunchKernelGGL(retire_mark_kernel, dim3(n_blk), dim3(256), 0, stream, d, pm, a, b);
    hipLaunchKernelGGL(retire_apply_kernel, dim3(n_blk), dim3(256), 0, stream, d, pm, a, b);
  }
  hipLaunchKernelGGL(retire_finish_kernel, dim3(1), dim3(256), 0, stream, n_blk, b);
  return hipGetLastError();
}

// RTG_FLAG_DENOISE (include/rtiow_gpu.h): the filter step over the whole frame (rt_denoise.h; nranks = 1) -- the per-pixel
// records and the pass-through pixels, the filter into the output plane, the block's out-fields.  It reads the UNDIVIDED
// running sums: the callers run it after the slice (and the retire step) and before the division.  `in`: the block's
// in-fields, already validated.
// `guide` (RTG_FLAG_FEATURES in the same call, else nullptr): the features block's in-fields -- the filter is the guided one, over
// the feature planes the frame holds now (the callers run the feature pass first).
// A frame with an error plane (RTG_FLAG_DENOISE_ERROR): the ERR instantiations, which also write it.
static hipError_t launch_denoise(rtg_scene* s, const DevParams& d, float* d_out, hipStream_t stream, const FrameLayout& L, const rtg_denoise& in,
                                 const rtg_features* guide = nullptr) {
  const uint64_t n_pix = L.n;
  const bool error = L.has(L.error);
  const uint32_t n_blk = (uint32_t)((n_pix + 255u) / 256u);
  // [records: 32 B x n_pix] [blk_u32: 2 x n_blk, padded to 16 B] [guided: feature records: 32 B x n_pix]
  const size_t frec_at = (size_t)n_pix * 32u + (((size_t)n_blk * 8u + 15u) & ~(size_t)15u);
  hipError_t e = s->cx->denoise.grow(frec_at + (guide ? (size_t)n_pix * 32u : 0u));
  if (e != hipSuccess) return e;
  uint32_t* words = reinterpret_cast<uint32_t*>(d_out);
  DenoiseBufs b;
  b.planes = d_out;
  b.counts = L.at(words, L.counts);
  b.rec = s->cx->denoise.as<float4>();
  b.blk_u32 = reinterpret_cast<uint32_t*>(b.rec + 2ull * n_pix);
  b.block = words + L.denoise;
  b.outp = d_out + L.denoised;
  b.errp = L.at(d_out, L.error);
  const DenoiseArgs a{in.k, in.radius, in.patch, d.ns};
  // the guided filter reads its neighbours' feature records through the caches, or (option guide_lds) from an LDS copy
  const int guided = !guide ? 0 : (s->guide_lds > 0 ? 2 : 1);
  void (*filter)(uint32_t, uint32_t, DenoiseArgs, DenoiseBufs, DenoiseGuide) =
      error ? (guided == 0 ? denoise_filter_kernel<0, true> : (guided == 1 ? denoise_filter_kernel<1, true> : denoise_filter_kernel<2, true>))
               : (guided == 0 ? denoise_filter_kernel<0, false> : (guided == 1 ? denoise_filter_kernel<1, false> : denoise_filter_kernel<2, false>));
  const size_t lds = denoise_lds_bytes(in.radius, in.patch, guided == 2);
  int per_cu = 0;
  e = kernel_setup(s, (const void*)filter, (int)DN_THREADS, lds, &per_cu);  // (the raise of the dynamic-LDS limit)
  if (e != hipSuccess) return e;
  const uint64_t tiles = (uint64_t)((d.nx + DN_TW - 1u) / DN_TW) * ((d.ny + DN_TH - 1u) / DN_TH);
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  DenoiseGuide gd{nullptr, 1.f, 1.f, 1.f};
  if (guide) {
    float4* frec = reinterpret_cast<float4*>(s->cx->denoise.as<char>() + frec_at);
    gd = DenoiseGuide{frec, guide->sigma_normal, guide->sigma_albedo, guide->sigma_depth};
    hipLaunchKernelGGL(denoise_guide_kernel, dim3(n_blk), dim3(256), 0, stream, (uint32_t)n_pix, (const float*)d_out + L.albedo, (const float*)d_out + L.normal,
                       (const float*)d_out + L.depth, frec);
  }
  hipLaunchKernelGGL(error ? denoise_prepare_kernel<true> : denoise_prepare_kernel<false>, dim3(n_blk), dim3(256), 0, stream, (uint32_t)n_pix, a, b);
  hipLaunchKernelGGL(filter, dim3((uint32_t)tiles), dim3(DN_THREADS), lds, stream, d.nx, d.ny, a, b, gd);
  hipLaunchKernelGGL(denoise_finish_kernel, dim3(1), dim3(256), 0, stream, n_blk, b);
  return hipGetLastError();
}

// RTG_FLAG_FEATURES (include/rtiow_gpu.h): the feature pass over this rank's pixels (rt_features.h) -- the three planes behind the
// features block and the block's out-fields.  `in`: the block's in-fields, already validated; compute = 0 writes the
// out-fields alone.  The kernel is instantiated per scene-feature set as the probes' (rtg_probes.inc): deep graphs take the
// general walk.
static hipError_t launch_features(rtg_scene* s, const DevCamera& cam, const DevParams& d, float* d_out, hipStream_t stream, const FrameLayout& L,
                                  const rtg_features& in) {
  const uint64_t blocks = (uint64_t)((d.nx + 15u) / 16u) * ((d.ny + 15u) / 16u);
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const uint32_t n_blk = in.compute ? (uint32_t)blocks : 0u;
  hipError_t e = s->cx->features.grow((size_t)std::max<uint64_t>(blocks, 1) * 8u);
  if (e != hipSuccess) return e;
  FeatureBufs b;
  b.block = reinterpret_cast<uint32_t*>(d_out) + L.features;
  b.albedo = d_out + L.albedo, b.normal = d_out + L.normal, b.depth = d_out + L.depth;
  b.blk_u32 = s->cx->features.as<uint32_t>();
  if (n_blk != 0u)
    with_feat<false>(s, [&](auto feat) { hipLaunchKernelGGL((features_kernel<decltype(feat)::value>), dim3(n_blk), dim3(256), 0, stream, s->dev, cam, d, in.grid, b); });
  hipLaunchKernelGGL(features_finish_kernel, dim3(1), dim3(256), 0, stream, n_blk, b);
  return hipGetLastError();
}

// What follows the render of a slice, in the one order of include/rtiow_gpu.h: the retire step (a frame without an error plane),
// the filter (guided when the slice has feature planes), the retire step on the error plane the filter wrote, then the division
// when the slice divides.  `fb`: the blocks' in-fields, already validated.  Called by launch_counts, launch_render and, on the
// first device over the gathered frame, by rtg_par_cast_multi's flagged frames.
static hipError_t launch_post_steps(rtg_scene* s, const DevParams& d, float* d_out, hipStream_t stream, const SampleSlice& sl, const FrameLayout& L,
                                    const FrameBlocks& fb) {
  const uint64_t pix_work = rank_pix_work(d);
  hipError_t e = hipSuccess;
  if (sl.retire && !sl.error) e = launch_retire(s, d, d_out, stream, L, pix_work, fb.retire);
  if (e == hipSuccess && sl.denoise) e = launch_denoise(s, d, d_out, stream, L, fb.denoise, sl.features ? &fb.features : nullptr);
  if (e == hipSuccess && sl.retire && sl.error) e = launch_retire(s, d, d_out, stream, L, pix_work, fb.retire);
  if (e != hipSuccess || !sl.divide) return e;
  return sl.counts ? launch_resolve_counts(d, d_out, stream, L) : launch_resolve(d, d_out, stream);
}

// The render of the samples [sl.begin, d.ns), by the kernel the scene's features pick.  A counts call (sl.counts) runs the pool
// kernels over its list; the baseline kernel walks every pixel and skips the inactive ones itself.
template <bool COUNT>
static hipError_t launch_slice(rtg_scene* s, const DevCamera& cam, const DevParams& d, float* d_out, hipStream_t stream, const SampleSlice& sl) {
  // geometry / texture features pick the kernel; the albedo-range bits only say whether the pool kernels' "accum
  // is +0" argument holds (rt_pool.h PoolField)
  const uint32_t geom = s->features & FEAT_NOT_LEAN;
  const bool accum_zero = !(s->features & FEAT_WIDE_ALBEDO) && (!(s->features & FEAT_BRIGHT_ALBEDO) || d.max_bounces <= 63u);
  // FEAT_DEEP: graph shapes only the general walk of the baseline kernel handles (flat_scene.h)
  // scene option light_sampling: the one-lane-per-pixel family in every case, whatever options kernel, bvh4 and the pool thresholds say
  // FEAT_TRI: the full-feature pool kernel and the lock-step kernel have instantiations that execute the record (rt_pool_full.h TRI);
  // their LIST variants do not exist, so a counts call of such a scene renders on the baseline kernel
  // FEAT_ENVIRONMENT: the pool kernels' environment instantiations (rt_pool_full.h PROG_ENV) exist without LIST and GENB: a counts
  // call of such a scene, and every frame of one with FEAT_BOUNDARY, renders on the baseline kernel
  const bool pool_ok = accum_zero && s->kernel_version >= 3 && d.nx <= 0xffffu && d.ny <= 0xffffu && !(s->features & FEAT_DEEP) && !s->light_sampling &&
                       !((s->features & FEAT_TRI) && sl.counts) &&
                       !((s->features & FEAT_ENVIRONMENT) && (sl.counts || (s->features & FEAT_BOUNDARY)));
  if (pool_ok) {  // (launch_full_pool names the kernel it picks)
    s->cx->last_kernel = geom != 0 ? KernelKind::full_pool : KernelKind::lean_pool;
    return geom != 0 ? launch_full_pool<COUNT>(s, cam, d, d_out, stream, sl) : launch_pool<COUNT>(s, cam, d, d_out, stream, sl);
  }
  // the baseline kernels: counts, squares and slices of a progressive frame have instantiations of their own
  const dim3 grid(((d.nx + 15) / 16) * ((d.ny + 15) / 16)), block(256);
  const uint32_t divide = sl.divide ? 1u : 0u;
  if (s->light_sampling && s->verbose) fprintf(stderr, "[rtg] light sampling: light table of %u rect(s)%s\n", s->n_lights, s->lights.n ? "" : ": the plain kernels");
  if (s->light_sampling && s->lights.n != 0u) {  // ... over color_ls (rt_light.h); with an empty table color_ls is color(): the kernels below
    with_feat<false>(s, [&](auto feat) {
      constexpr uint32_t F = decltype(feat)::value;
      if constexpr (F != 0u)  // (a table that is not empty holds a Rect: never a lean program)
        with_bools([&](auto sq, auto cn) {
          hipLaunchKernelGGL((render_light_kernel<F, COUNT, decltype(sq)::value, decltype(cn)::value>), grid, block, 0, stream, s->dev, s->lights, cam, d, d_out,
                             s->cx->d_counters, sl.begin, divide, sl.list.counts);
        }, sl.squares, sl.counts);
    });
    return hipGetLastError();
  }
  if (sl.counts)
    with_feat<false>(s, [&](auto feat) {
      constexpr uint32_t F = decltype(feat)::value;
      void (*k)(DevScene, DevCamera, DevParams, float*, unsigned long long*, uint32_t, const uint32_t*) =
          sl.squares ? render_counts_kernel<F, COUNT, true> : render_counts_kernel<F, COUNT, false>;
      hipLaunchKernelGGL(k, grid, block, 0, stream, s->dev, cam, d, d_out, s->cx->d_counters, sl.begin, sl.list.counts);
    });
  else if (sl.squares)
    with_feat<false>(s, [&](auto feat) {
      hipLaunchKernelGGL((render_squares_kernel<decltype(feat)::value, COUNT>), grid, block, 0, stream, s->dev, cam, d, d_out, s->cx->d_counters, sl.begin, divide);
    });
  else if (sl.sliced())
    with_feat<false>(s, [&](auto feat) {
      hipLaunchKernelGGL((render_slice_kernel<decltype(feat)::value, COUNT>), grid, block, 0, stream, s->dev, cam, d, d_out, s->cx->d_counters, sl.begin, divide);
    });
  else
    with_feat<true>(s, [&](auto feat) { hipLaunchKernelGGL((render_kernel<decltype(feat)::value, COUNT>), grid, block, 0, stream, s->dev, cam, d, d_out, s->cx->d_counters); });
  return hipGetLastError();
}

// RTG_FLAG_SAMPLE_COUNTS (include/rtiow_gpu.h): compact this rank's active pixels (e_p > sl.begin) into the list the pool
// kernels run over (rt_pool.h compact_*), read back its length and the call's sample count -- the one synchronisation of the
// stream a counts call makes -- render the list (launch_slice), then the post-steps (launch_post_steps): without
// RTG_FLAG_PARTIAL every owned pixel with e_p > 0 ends divided by e_p.
// The in-fields of the slice's blocks (RTG_FLAG_RETIRE / DENOISE / FEATURES) come back with that read-back (on their own when the
// call renders nothing; a call that renders nothing and has no block does not synchronise); refused ones end the call before it
// renders (s->cx->refusal).  The feature pass runs first, before the render.  The background of RTG_FLAG_BACKGROUND rides with
// them and goes into the frame parameters of the render.
template <bool COUNT>
static hipError_t launch_counts(rtg_scene* s, const DevCamera& cam, const DevParams& d, float* d_out, hipStream_t stream,
                                const SampleSlice& sl, const FrameLayout& L) {
  s->cx->counts_samples = 0;
  const uint64_t pix_work = rank_pix_work(d);
  if (pix_work == 0 && !sl.retire && !sl.features) return hipSuccess;  // this rank owns no tile
  if (pix_work > 0xfffffffeull) return hipErrorInvalidValue;
  FrameBlocks fb;
  SampleSlice ls = sl;
  ls.list.counts = L.at(reinterpret_cast<const uint32_t*>(d_out), L.counts);
  const bool renders = sl.begin < d.ns && pix_work != 0;
  CompactResult h{};
  hipError_t e = hipSuccess;
  if (renders) {
    const PixMap pm = make_pixmap(d);
    const uint32_t n_blk = (uint32_t)(pix_work / 256u);
    e = s->cx->list.grow(2 * pix_work * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    // [blk_samples: u64 x n_blk] [CompactResult] [blk_active: n_blk] [blk_offset: n_blk]
    e = s->cx->compact.grow((size_t)n_blk * 16u + sizeof(CompactResult));
    if (e != hipSuccess) return e;
    unsigned long long* blk_samples = s->cx->compact.as<unsigned long long>();
    CompactResult* res = reinterpret_cast<CompactResult*>(blk_samples + n_blk);
    uint32_t* blk_active = reinterpret_cast<uint32_t*>(res + 1);
    uint32_t* blk_offset = blk_active + n_blk;
    uint32_t* list = s->cx->list.as<uint32_t>();
    uint32_t* inv = list + pix_work;
    ls.list.list = list, ls.list.inv = inv;
    hipLaunchKernelGGL(compact_count_kernel, dim3(n_blk), dim3(256), 0, stream, d, pm, (uint32_t)pix_work, ls.list.counts, sl.begin, blk_active, blk_samples);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, stream, n_blk, blk_active, blk_samples, blk_offset, list, res);
    hipLaunchKernelGGL(compact_write_kernel, dim3(n_blk), dim3(256), 0, stream, d, pm, (uint32_t)pix_work, ls.list.counts, sl.begin, blk_offset, list, inv);
    hipLaunchKernelGGL(write_list_consts, dim3(1), dim3(1), 0, stream, reinterpret_cast<ListConsts*>(s->cx->d_consts + 1), ls.list);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(&h, res, sizeof(h), hipMemcpyDeviceToHost, stream);
  }
  DevParams dr = d;  // the render's parameters: d with the background the frame's block names
  if (renders || sl.retire || sl.denoise || sl.features || sl.background) {  // the blocks ride with the compaction result: ONE synchronisation
    if (e == hipSuccess) e = read_blocks(L, sl, d_out, stream, &fb);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    if ((s->cx->refusal = blocks_refusal(sl, fb, d.nranks))) return hipSuccess;
    if (sl.background) dr.bg = dev_background(fb.background);
  }
  if (sl.features && (e = launch_features(s, cam, d, d_out, stream, L, fb.features)) != hipSuccess) return e;
  if (renders) {
    s->cx->counts_samples = h.samples;
    ls.list_work = h.padded;
    if (s->verbose)
      fprintf(stderr, "[rtg] sample counts: samples [%u, %u): %u of %llu owned pixels active (list of %u work items), %llu samples\n",
              sl.begin, d.ns, h.active, (unsigned long long)owned_pixels(d), h.padded, h.samples);
    if (h.active != 0u && (e = launch_slice<COUNT>(s, cam, dr, d_out, stream, ls)) != hipSuccess) return e;
  }
  return launch_post_steps(s, d, d_out, stream, sl, L, fb);
}

// One call's frame: the feature pass, the render, the post-steps.  `sl` (rtg_api.hip SampleSlice): the samples of a progressive
// frame this call renders and what it does at the end; `L`: the frame's layout; `fb`: the in-fields of the slice's blocks, read
// and validated by the caller (a counts call reads them itself, with its compaction result: launch_counts).
// The kernel that renders also divides -- unless a post-step follows: then it renders an undivided slice and launch_post_steps
// divides last.  A call with nothing to render (sample_begin = ns) and no post-step is the resolve step alone.
template <bool COUNT>
static hipError_t launch_render(rtg_scene* s, const DevCamera& cam, const DevParams& d, float* d_out, hipStream_t stream, const SampleSlice& sl,
                                const FrameLayout& L, const FrameBlocks& fb) {
  s->cx->last_kernel = KernelKind::baseline;
  if (sl.counts) return launch_counts<COUNT>(s, cam, d, d_out, stream, sl, L);
  hipError_t e = sl.features ? launch_features(s, cam, d, d_out, stream, L, fb.features) : hipSuccess;
  if (e != hipSuccess) return e;
  const bool post = sl.denoise;  // (the retire step needs a count plane)
  if (sl.begin != d.ns) {
    SampleSlice render = sl;
    if (post) render.divide = false;
    e = launch_slice<COUNT>(s, cam, d, d_out, stream, render);
  } else if (!post) {
    return sl.divide ? launch_resolve(d, d_out, stream) : hipSuccess;
  }
  if (e != hipSuccess || !post) return e;
  return launch_post_steps(s, d, d_out, stream, sl, L, fb);
}
