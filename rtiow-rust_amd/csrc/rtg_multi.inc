// rtg_multi.inc -- included by rtg_api.hip inside its extern "C" block: rtg_par_cast_multi / rtg_multi_reset and the RCCL loader.
// ---- single-process multi-GPU par_cast (SURVEY.md 8b) ---------------------------------------------------
// RCCL is dlopen()ed on first use (more than one distinct device, or the `force_rccl` option), so librtiow_gpu.so carries
// no link-time dependency on it and one-GPU hosts never load it.
namespace {
struct Rccl {
  void* lib = nullptr;
  std::string path;  // rtg_multi_reset: the library to load instead of the default search ("" = default)
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;  // (packed collective; may be absent in an old librccl)
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::map<std::vector<int>, std::vector<ncclComm_t>> comms;  // one clique per device list, created once, destroyed by rtg_multi_reset
  uint64_t n_reduces = 0;                                      // ncclReduce calls issued (rtg_multi_reset reports and clears it)
  std::mutex mu;
};
Rccl g_rccl;

// (g_rccl.mu held)
int rccl_load() {
  if (g_rccl.lib) return RTG_OK;
  void* h = nullptr;
  std::string tried;
  auto attempt = [&](const char* n, int flags) {
    if (h) return;
    (void)dlerror();
    h = dlopen(n, flags);
    if (!h && !(flags & RTLD_NOLOAD)) {
      const char* e = dlerror();  // ONE call: dlerror() clears the message it returns
      tried += std::string(tried.empty() ? "" : "; ") + (e ? e : n);
    }
  };
  if (!g_rccl.path.empty()) {
    attempt(g_rccl.path.c_str(), RTLD_NOW | RTLD_LOCAL);
  } else {
    // an already-loaded librccl (e.g. the one a host framework ships) first, then the ROCm installation's
    for (const char* n : {"librccl.so", "librccl.so.1"}) attempt(n, RTLD_NOW | RTLD_NOLOAD);
    for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) attempt(n, RTLD_NOW | RTLD_LOCAL);
  }
  if (!h) return fail(RTG_ERR_DEVICE, "librccl not loadable: " + (tried.empty() ? std::string("?") : tried));
  auto sym = [&](const char* n) { return dlsym(h, n); };
  g_rccl.CommInitAll = (decltype(g_rccl.CommInitAll))sym("ncclCommInitAll");
  g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))sym("ncclCommDestroy");
  g_rccl.GroupStart = (decltype(g_rccl.GroupStart))sym("ncclGroupStart");
  g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))sym("ncclGroupEnd");
  g_rccl.Reduce = (decltype(g_rccl.Reduce))sym("ncclReduce");
  g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))sym("ncclGetErrorString");
  g_rccl.Send = (decltype(g_rccl.Send))sym("ncclSend");
  g_rccl.Recv = (decltype(g_rccl.Recv))sym("ncclRecv");
  if (!g_rccl.CommInitAll || !g_rccl.CommDestroy || !g_rccl.GroupStart || !g_rccl.GroupEnd || !g_rccl.Reduce || !g_rccl.GetErrorString) {
    dlclose(h);
    return fail(RTG_ERR_DEVICE, "librccl lacks ncclCommInitAll / ncclCommDestroy / ncclGroupStart / ncclGroupEnd / ncclReduce / ncclGetErrorString");
  }
  g_rccl.lib = h;
  return RTG_OK;
}

// (g_rccl.mu held) destroy the cached cliques
void rccl_drop_comms() {
  if (g_rccl.CommDestroy)
    for (auto& kv : g_rccl.comms)
      for (ncclComm_t c : kv.second)
        if (c) (void)g_rccl.CommDestroy(c);
  g_rccl.comms.clear();
}

// (g_rccl.mu held) ONE grouped collective over the clique of this device list (created on first use): `body(comms, err)` issues
// its calls, stopping at the first failure, which it reports in `err`.  The group is always closed (a group left open would
// swallow every later RCCL call of the process); after any failure the clique's communicators are dropped (their state is
// unknown).  The caller synchronizes the streams.
int rccl_group(const std::vector<int>& devs, const std::function<void(const std::vector<ncclComm_t>&, std::string&)>& body) {
  auto it = g_rccl.comms.find(devs);
  if (it == g_rccl.comms.end()) {
    std::vector<ncclComm_t> c(devs.size(), nullptr);
    ncclResult_t r = g_rccl.CommInitAll(c.data(), (int)devs.size(), devs.data());
    if (r != ncclSuccess) return fail(RTG_ERR_DEVICE, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r));
    it = g_rccl.comms.emplace(devs, std::move(c)).first;
  }
  std::string err;
  ncclResult_t r = g_rccl.GroupStart();
  if (r != ncclSuccess) {
    err = std::string("ncclGroupStart: ") + g_rccl.GetErrorString(r);
  } else {
    body(it->second, err);
    const ncclResult_t r2 = g_rccl.GroupEnd();
    if (r2 != ncclSuccess && err.empty()) err = std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(r2);
  }
  if (err.empty()) return RTG_OK;
  for (ncclComm_t c : it->second)
    if (c) (void)g_rccl.CommDestroy(c);
  g_rccl.comms.erase(it);
  return fail(RTG_ERR_DEVICE, err);
}

// ONE collective over the distinct devices: reduce(sum) of the float3 framebuffers heads[k]->frame (device devs[k],
// stream heads[k]->own_stream) to heads[0]'s.
int rccl_reduce_frames(const std::vector<int>& devs, const std::vector<rtg_scene*>& heads, size_t n_floats) {
  std::lock_guard<std::mutex> lock(g_rccl.mu);
  if (int rc = rccl_load()) return rc;
  return rccl_group(devs, [&](const std::vector<ncclComm_t>& comms, std::string& err) {
    for (size_t k = 0; k < devs.size() && err.empty(); k++) {
      hipError_t he = hipSetDevice(devs[k]);
      if (he != hipSuccess) {
        err = std::string("hipSetDevice: ") + hipGetErrorString(he);
        break;
      }
      ncclResult_t r = g_rccl.Reduce(heads[k]->frame.p, heads[k]->frame.p, n_floats, ncclFloat, ncclSum, 0, comms[k], heads[k]->own_stream);
      if (r != ncclSuccess) err = std::string("ncclReduce: ") + g_rccl.GetErrorString(r);
      else g_rccl.n_reduces++;
    }
  });
}

// The PACKED collective (plain frames under scene option multi_gather, and every flagged frame): a scene ships only the pixels it
// owns -- the planes of its tiles in work-item order (rt_multi_planes.h: pix_work x words_per_pixel, 1 / n_scenes of the frame) --
// to the first device, which scatters them into the frame.  Grouped ncclSend / ncclRecv: scene i's packed planes (moves[k]:
// buffer, words, clique rank of its device) arrive in moves[k].dst on device 0, on `head_stream`.  Copies only: bit-identical
// by construction.
struct PackedMove { const float* src; float* dst; size_t n_floats; int from; hipStream_t src_stream; };
int rccl_gather_tiles(const std::vector<int>& devs, hipStream_t head_stream, const std::vector<PackedMove>& moves) {
  std::lock_guard<std::mutex> lock(g_rccl.mu);
  if (int rc = rccl_load()) return rc;
  if (!g_rccl.Send || !g_rccl.Recv) return fail(RTG_ERR_DEVICE, "librccl lacks ncclSend / ncclRecv (the packed collective needs them)");
  // every move is checked before the group opens: an argument error must not leave a half-issued group behind
  if (devs.empty() || !head_stream) return fail(RTG_ERR_INVALID, "packed collective: no first device");
  for (const PackedMove& m : moves) {
    if (!m.src || !m.dst) return fail(RTG_ERR_INVALID, "packed collective: a move without a buffer");
    if (m.n_floats == 0) return fail(RTG_ERR_INVALID, "packed collective: an empty move");
    if (m.from < 0 || (size_t)m.from >= devs.size()) return fail(RTG_ERR_INVALID, "packed collective: a move from a device outside the clique");
    if (!m.src_stream) return fail(RTG_ERR_INVALID, "packed collective: a move without a stream");
  }
  return rccl_group(devs, [&](const std::vector<ncclComm_t>& comms, std::string& err) {
    for (size_t k = 0; k < moves.size() && err.empty(); k++) {
      const PackedMove& m = moves[k];
      hipError_t he = hipSetDevice(devs[m.from]);
      if (he == hipSuccess) {
        ncclResult_t r = g_rccl.Send(m.src, m.n_floats, ncclFloat, 0, comms[m.from], m.src_stream);
        if (r != ncclSuccess) err = std::string("ncclSend: ") + g_rccl.GetErrorString(r);
        he = hipSetDevice(devs[0]);
      }
      if (he != hipSuccess) {
        err = std::string("hipSetDevice: ") + hipGetErrorString(he);
        break;
      }
      if (err.empty()) {
        ncclResult_t r = g_rccl.Recv(m.dst, m.n_floats, ncclFloat, m.from, comms[0], head_stream);
        if (r != ncclSuccess) err = std::string("ncclRecv: ") + g_rccl.GetErrorString(r);
        else g_rccl.n_reduces++;
      }
    }
  });
}

// RTG_FLAG_RESUME: scene i's full frame starts as the caller's running sums on the pixels it owns and +0 on every other pixel, so
// that the reduce (x + 0 is exact; a sum starts at +0, so it is never -0) and the packed gather assemble the frame unchanged
__global__ void keep_owned_kernel(DevParams P, float* __restrict__ fb) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)P.nx * P.ny) return;
  const uint32_t row = (uint32_t)(i / P.nx), x = (uint32_t)(i - (size_t)row * P.nx);
  const uint32_t tiles_x = (P.nx + P.tile_w - 1u) / P.tile_w;
  if (((row / P.tile_h) * tiles_x + x / P.tile_w) % P.nranks == P.rank) return;
  fb[3 * i] = 0.f, fb[3 * i + 1] = 0.f, fb[3 * i + 2] = 0.f;
}

__global__ void add_frames_kernel(size_t n, float* __restrict__ dst, const float* __restrict__ src) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = dst[i] + src[i];  // every pixel has ONE non-zero contributor: x + 0 is exact
}

// Tile size when the caller leaves it to the library (tile_w / tile_h = 0): 16x16 up to 7 devices, 8x8 from 8 on -- with an eighth
// of the tiles per device the slowest shard of the 16x16 interleave lies 5-6 % above the mean, with 8x8 tiles 2-4 %
// (profiles/r04_experiments/r04x_shard_tiles.txt; the same rule as rtiow-rust_amd/parallel.py shard_tile, which bench.py uses).
// Scene i's checked DevParams: the caller's params as rank i of n_scenes, with those tiles.
static int rank_params(const rtg_scene* s, const rtg_camera* camera, const rtg_params* params, int i, int n_scenes, DevParams* d) {
  rtg_params p = *params;
  p.rank = (uint32_t)i, p.nranks = (uint32_t)n_scenes;
  const uint32_t t = n_scenes >= 8 ? 8u : 16u;
  if (p.tile_w == 0) p.tile_w = t;
  if (p.tile_h == 0) p.tile_h = t;
  return check_params(s, camera, &p, d);
}

// The scenes' distinct devices in order of first appearance, the first scene on each (`heads`: it holds that device's frame)
// and, per scene, the index of its device in both
struct DeviceGroups {
  std::vector<int> devs;
  std::vector<rtg_scene*> heads;
  std::vector<int> of;
};
static DeviceGroups group_by_device(rtg_scene* const* scenes, int n_scenes) {
  DeviceGroups g;
  for (int i = 0; i < n_scenes; i++) {
    size_t k = 0;
    while (k < g.devs.size() && g.devs[k] != scenes[i]->device) k++;
    if (k == g.devs.size()) g.devs.push_back(scenes[i]->device), g.heads.push_back(scenes[i]);
    g.of.push_back((int)k);
  }
  return g;
}

// rtg_stats of a call whose streams are drained: the slowest shard's kernel time, `samples`, the counters summed over the ranks
static int multi_stats(rtg_scene* const* scenes, int n_scenes, uint64_t samples, rtg_stats* stats, bool count) {
  if (stats) {
    rtg_stats total{};
    total.struct_size = sizeof(rtg_stats);
    total.samples = samples;
    for (int i = 0; i < n_scenes; i++) {
      rtg_scene* s = scenes[i];
      HIP_TRY(hipSetDevice(s->device));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, s->cx->ev0, s->cx->ev1));
      total.kernel_ms = std::max(total.kernel_ms, ms);
      if (count) {
        unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIP_TRY(hipMemcpy(h, s->cx->d_counters, sizeof(h), hipMemcpyDeviceToHost));
        total.aabb_tests += h[0], total.prim_tests += h[1], total.shaded_hits += h[2], total.rays += h[3], total.draws += h[4];
      }
    }
    *stats = total;
  }
  return RTG_OK;
}

// (1) The rank stage of both kinds of call: every scene renders ITS tiles (tile % n_scenes == i) of the frame L into its own device
// frame, on its own stream.  `rp`: the caller's params with the flags the ranks render with -- never RTG_FLAG_BACKGROUND: a rank
// gets the block in its parameters, from the checked host copy in `fb`.  `packed`: the packed collective will carry the ranks'
// pixels (its kernels index a rank's work items with 32 bits, as launch_resolve and launch_counts do).  `fill(i, s, d)` enqueues
// on s->own_stream what rank i's frame holds before it renders.  `features`: the feature pass follows the render (the planes do
// not depend on each other): a counts call's compaction wait, a rank's one host wait, then covers no feature kernel, and the next
// rank is launched while this one traces.  Every rank's parameters are checked before anything is enqueued; they come back in
// `dps` with the samples of the call.
using RankFill = std::function<int(int, rtg_scene*, const DevParams&)>;
static int enqueue_ranks(rtg_scene* const* scenes, int n_scenes, const rtg_camera* camera, const rtg_params& rp, const FrameLayout& L, const FrameBlocks& fb,
                         bool packed, bool features, bool count, const RankFill& fill, std::vector<DevParams>* dps, uint64_t* samples) {
  const SampleSlice rsl = slice_of(&rp);
  const DevCamera cam = to_dev(camera);
  dps->resize(n_scenes);
  for (int i = 0; i < n_scenes; i++) {
    DevParams& d = (*dps)[i];
    if (int rc = rank_params(scenes[i], camera, &rp, i, n_scenes, &d)) return rc;
    if (L.has(L.background)) d.bg = dev_background(fb.background);
    if (packed && rank_pix_work(d) > 0xfffffffeull) return fail(RTG_ERR_RANGE, "rtg_par_cast_multi: a rank's work items overflow the 32-bit work index");
  }
  *samples = 0;
  for (int i = 0; i < n_scenes; i++) {
    rtg_scene* s = scenes[i];
    const DevParams& d = (*dps)[i];
    HIP_TRY(hipSetDevice(s->device));
    if (!s->own_stream) HIP_TRY(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
    hipError_t e = s->frame.grow(L.words ? L.words * sizeof(float) : 16);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(framebuffer)");
    if (int rc = fill(i, s, d)) return rc;
    if (int rc = ctx_acquire(s)) return rc;
    if (count) HIP_TRY(clear_counters(s->cx, s->own_stream));
    HIP_TRY(hipEventRecord(s->cx->ev0, s->own_stream));
    float* frame = s->frame.as<float>();
    HIP_TRY(count ? launch_render<true>(s, cam, d, frame, s->own_stream, rsl, L, fb) : launch_render<false>(s, cam, d, frame, s->own_stream, rsl, L, fb));
    if (features) HIP_TRY(launch_features(s, cam, d, frame, s->own_stream, L, fb.features));
    HIP_TRY(hipEventRecord(s->cx->ev1, s->own_stream));
    *samples += rsl.counts ? s->cx->counts_samples : owned_pixels(d) * (d.ns - rsl.begin);
    if (int rc = ctx_release(s, s->own_stream)) return rc;
  }
  return RTG_OK;
}

// (2) The packed gather of both kinds of call, over the planes `ps` the ranks wrote (rt_multi_planes.h PlaneSet: one pack kernel,
// one ncclSend / ncclRecv pair and one unpack kernel per handle that travels).  A handle without a work item is skipped; the first
// handle's own pixels already stand in the frame unless it travels (a clique of one under force_rccl: its planes take the send /
// recv path too, to itself); another handle on the first device is unpacked from its own pack buffer once its stream is drained.
// The unpack kernels are left on the first handle's stream: the caller waits.  `verbose`: events around the pack kernels and in
// front of the unpack kernels (s->pack0 / pack1, head->unpack0).  at_head[i]: where scene i's packed planes stand on the first
// device (nullptr: nothing was packed); `through_rccl`: how many travelled.
static int gather_planes(rtg_scene* const* scenes, int n_scenes, const DeviceGroups& g, const std::vector<DevParams>& dps, const PlaneSet& ps, bool force_rccl,
                         bool verbose, std::vector<const uint32_t*>* at_head, size_t* through_rccl) {
  rtg_scene* head = g.heads[0];  // (= scenes[0])
  std::vector<PackedMove> moves;
  at_head->assign(n_scenes, nullptr);
  for (int i = 0; i < n_scenes; i++) {
    rtg_scene* s = scenes[i];
    const uint32_t pw = (uint32_t)rank_pix_work(dps[i]);
    const bool travels = g.of[i] != 0 || (force_rccl && g.devs.size() == 1 && i == 0);
    if (pw == 0 || (s == head && !travels)) continue;
    const size_t words = (size_t)pw * ps.words_per_pixel;
    HIP_TRY(hipSetDevice(s->device));
    hipError_t e = s->pack.grow(words * sizeof(uint32_t));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(packed planes)");
    if (verbose) {
      if (!s->pack0) HIP_TRY(hipEventCreate(&s->pack0));
      if (!s->pack1) HIP_TRY(hipEventCreate(&s->pack1));
      HIP_TRY(hipEventRecord(s->pack0, s->own_stream));
    }
    hipLaunchKernelGGL(pack_planes_kernel, dim3((pw + 255) / 256), dim3(256), 0, s->own_stream, dps[i], make_pixmap(dps[i]), pw, ps, s->frame.as<const uint32_t>(),
                       s->pack.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    if (verbose) HIP_TRY(hipEventRecord(s->pack1, s->own_stream));
    if (travels) {
      HIP_TRY(hipSetDevice(g.devs[0]));
      e = s->recv.grow(words * sizeof(uint32_t));
      if (e != hipSuccess) return hip_fail(e, "hipMalloc(received planes)");
      moves.push_back(PackedMove{s->pack.as<float>(), s->recv.as<float>(), words, g.of[i], s->own_stream});
      (*at_head)[i] = s->recv.as<uint32_t>();
    } else {
      (*at_head)[i] = s->pack.as<uint32_t>();
      HIP_TRY(hipStreamSynchronize(s->own_stream));  // (another handle on the first device: its own stream)
    }
  }
  *through_rccl = moves.size();
  if (!moves.empty()) {
    int rc = rccl_gather_tiles(g.devs, head->own_stream, moves);
    if (rc) return rc;
  }
  HIP_TRY(hipSetDevice(head->device));
  if (verbose) {
    if (!head->unpack0) HIP_TRY(hipEventCreate(&head->unpack0));
    HIP_TRY(hipEventRecord(head->unpack0, head->own_stream));
  }
  for (int i = 0; i < n_scenes; i++) {
    if (!(*at_head)[i]) continue;
    const uint32_t pw = (uint32_t)rank_pix_work(dps[i]);
    hipLaunchKernelGGL(unpack_planes_kernel, dim3((pw + 255) / 256), dim3(256), 0, head->own_stream, dps[i], make_pixmap(dps[i]), pw, ps, head->frame.as<uint32_t>(),
                       (*at_head)[i]);
    HIP_TRY(hipGetLastError());
  }
  return RTG_OK;
}

// ... and the wait behind either route: every handle's stream; the first device is current afterwards
static int drain_streams(rtg_scene* const* scenes, int n_scenes) {
  for (int i = n_scenes - 1; i >= 0; i--) {
    HIP_TRY(hipSetDevice(scenes[i]->device));
    HIP_TRY(hipStreamSynchronize(scenes[i]->own_stream));
  }
  return RTG_OK;
}

// The flags of a flagged frame, which needs scene option multi_planes on a handle (include/rtiow_gpu.h, at rtg_par_cast_multi)
const struct { uint32_t flag; const char* name; } PLANE_FLAGS[5] = {{RTG_FLAG_SUM_SQUARES, "RTG_FLAG_SUM_SQUARES"}, {RTG_FLAG_SAMPLE_COUNTS, "RTG_FLAG_SAMPLE_COUNTS"}, {RTG_FLAG_RETIRE, "RTG_FLAG_RETIRE"},
                                                                   {RTG_FLAG_DENOISE, "RTG_FLAG_DENOISE"}, {RTG_FLAG_FEATURES, "RTG_FLAG_FEATURES"}};

// The plain frame: float3 sums, assembled on the first device by the full-frame reduce or, under scene option multi_gather, by
// the packed gather of the one plane.
int par_cast_multi_body(rtg_scene* const* scenes, int n_scenes, const rtg_camera* camera, const rtg_params* params, float* out_rgb,
                        rtg_stats* stats) {
  const size_t n_floats = (size_t)params->nx * params->ny * 3;
  const size_t bytes = n_floats * sizeof(float);
  const bool count = stats && (params->flags & RTG_FLAG_COUNTERS);
  const SampleSlice sl = slice_of(params);
  const FrameLayout L(params->nx, params->ny, params->flags);  // (the plain frame and, under RTG_FLAG_BACKGROUND, the block behind it)
  FrameBlocks fb;
  if (int rc = check_blocks(L, sl, out_rgb, 1u, &fb)) return rc;
  rtg_params rp = *params;
  rp.flags &= ~RTG_FLAG_BACKGROUND;
  bool gather = false, force_rccl = false;
  for (int i = 0; i < n_scenes; i++) {
    gather = gather || scenes[i]->multi_gather != 0;
    force_rccl = force_rccl || scenes[i]->force_rccl != 0;
  }
  // (1) into a zero-filled full frame (resuming a progressive frame: its tiles hold the caller's running sums)
  const RankFill fill = [&](int, rtg_scene* s, const DevParams& d) -> int {
    if (sl.begin == 0u) {
      HIP_TRY(hipMemsetAsync(s->frame.p, 0, bytes, s->own_stream));
      return RTG_OK;
    }
    HIP_TRY(hipMemcpyAsync(s->frame.p, out_rgb, bytes, hipMemcpyHostToDevice, s->own_stream));
    hipLaunchKernelGGL(keep_owned_kernel, dim3((uint32_t)(((size_t)d.nx * d.ny + 255) / 256)), dim3(256), 0, s->own_stream, d, s->frame.as<float>());
    HIP_TRY(hipGetLastError());
    return RTG_OK;
  };
  std::vector<DevParams> dps;
  uint64_t samples = 0;
  if (int rc = enqueue_ranks(scenes, n_scenes, camera, rp, L, fb, gather, false, count, fill, &dps, &samples)) return rc;
  const DeviceGroups g = group_by_device(scenes, n_scenes);
  const std::vector<rtg_scene*>& heads = g.heads;
  if (gather) {  // (2') the packed gather
    std::vector<const uint32_t*> at_head;
    size_t through_rccl = 0;
    if (int rc = gather_planes(scenes, n_scenes, g, dps, make_plane_set(L, false), force_rccl, false, &at_head, &through_rccl)) return rc;
  } else {
    // (2) scenes that share a device with an earlier one are summed there; one frame per DISTINCT device remains
    for (int i = 0; i < n_scenes; i++) {
      rtg_scene *s = scenes[i], *h = heads[g.of[i]];
      if (s == h) continue;
      HIP_TRY(hipSetDevice(s->device));
      HIP_TRY(hipStreamSynchronize(s->own_stream));
      hipLaunchKernelGGL(add_frames_kernel, dim3((uint32_t)((n_floats + 255) / 256)), dim3(256), 0, h->own_stream, n_floats, h->frame.as<float>(), s->frame.as<const float>());
      HIP_TRY(hipGetLastError());
    }
    // (3) ONE collective over the distinct devices: reduce(sum) of the float3 framebuffer to the first device (xGMI).
    // `force_rccl`: also with ONE distinct device (a clique of one) -- the same dlopen / ncclCommInitAll / grouped in-place
    // ncclReduce code as on a node, which one-GPU test boxes could otherwise never execute.
    if (g.devs.size() > 1 || force_rccl) {
      int rc = rccl_reduce_frames(g.devs, heads, n_floats);
      if (rc) return rc;
    }
  }
  // (4) wait, copy the assembled frame out, gather stats (kernel time = the slowest shard)
  if (int rc = drain_streams(scenes, n_scenes)) return rc;
  HIP_TRY(hipMemcpy(out_rgb, heads[0]->frame.p, bytes, hipMemcpyDeviceToHost));
  return multi_stats(scenes, n_scenes, samples, stats, count);
}

// The flagged frames (scene option multi_planes; include/rtiow_gpu.h at rtg_par_cast_multi): RTG_FLAG_SUM_SQUARES, SAMPLE_COUNTS,
// RETIRE, DENOISE and FEATURES over several handles.
// (0) the refusals of rtg_par_cast with nranks = 1, on the host copy of the blocks;
// (1) every scene renders ITS tiles as a PARTIAL slice (squares / counts as given) into its own frame of the full layout, and
//     traces the feature pass for the pixels it owns -- no retire rule, no filter, no division.  A rank's launch holds at most
//     one host wait (a counts call's compaction), so launching the ranks in turn keeps the devices busy;
// (2) the packed gather over EVERY plane the ranks wrote assembles the frame on the first device.  Copies only;
// (3) the first device runs what a one-handle call with sample_begin == ns runs on that frame: launch_post_steps (the retire
//     step with any radius: the window sees the whole frame; the filter guided over the gathered feature planes; the division);
// (4) copy back what rtg_par_cast copies back; traced / missed of the features block are the sums over the ranks.
int par_cast_multi_planes_body(rtg_scene* const* scenes, int n_scenes, const rtg_camera* camera, const rtg_params* params, float* out_rgb,
                               rtg_stats* stats) {
  const SampleSlice sl = slice_of(params);
  DevParams d1;  // the one-handle call's parameters (nranks = 1, the caller's tiles): the first device's step runs over them
  if (int rc = check_params(scenes[0], camera, params, &d1)) return rc;
  const FrameLayout L(params->nx, params->ny, params->flags);
  FrameBlocks fb;
  if (int rc = check_blocks(L, sl, out_rgb, 1u, &fb)) return rc;
  if (rank_pix_work(d1) > 0xfffffffeull) return fail(RTG_ERR_RANGE, "rtg_par_cast_multi: the frame's work items overflow the 32-bit work index");
  const uint32_t compute = sl.features ? fb.features.compute : 0u;
  const PlaneSet ps = make_plane_set(L, compute != 0u);
  rtg_params rp = *params;  // what the ranks render into that frame: the slice, never retired, filtered or resolved
  rp.flags = (rp.flags & ~(RTG_FLAG_RETIRE | RTG_FLAG_DENOISE | RTG_FLAG_DENOISE_ERROR | RTG_FLAG_FEATURES | RTG_FLAG_BACKGROUND)) | RTG_FLAG_PARTIAL;
  const bool count = stats && (params->flags & RTG_FLAG_COUNTERS);
  char* host = reinterpret_cast<char*>(out_rgb);
  // (1) the first scene's frame is the call's frame: uploaded as rtg_par_cast uploads it (untouched pixels and an untouched
  // output plane survive); the others get what their slice reads -- the float planes when it resumes or renders counts (pixels
  // with n_p = 0 must travel back as they came), and the count plane.  The feature pass takes its in-fields from the host copy.
  Extents rank_up;
  if (sl.begin != 0u || sl.counts) rank_up.add(0, sl.counts ? L.counts + L.n : L.planes());
  const RankFill fill = [&](int i, rtg_scene* s, const DevParams&) -> int {
    const Extents up = i == 0 ? upload_extents(L, false, sl.begin, compute) : rank_up;
    for (int k = 0; k < up.n; k++) HIP_TRY(hipMemcpyAsync(s->frame.as<char>() + up.e[k].lo, host + up.e[k].lo, up.e[k].hi - up.e[k].lo, hipMemcpyHostToDevice, s->own_stream));
    return RTG_OK;
  };
  std::vector<DevParams> dps;
  uint64_t samples = 0;
  if (int rc = enqueue_ranks(scenes, n_scenes, camera, rp, L, fb, true, sl.features, count, fill, &dps, &samples)) return rc;
  bool force_rccl = false, verbose = false;
  for (int i = 0; i < n_scenes; i++) force_rccl = force_rccl || scenes[i]->force_rccl != 0, verbose = verbose || scenes[i]->verbose != 0;
  const DeviceGroups g = group_by_device(scenes, n_scenes);
  rtg_scene* head = g.heads[0];  // (= scenes[0])
  const hipStream_t hs = head->own_stream;
  // (2) pack, travel, unpack
  std::vector<const uint32_t*> at_head;
  size_t through_rccl = 0;
  if (int rc = gather_planes(scenes, n_scenes, g, dps, ps, force_rccl, verbose, &at_head, &through_rccl)) return rc;
  // (3) the first device's step over the assembled frame, through the launch functions of the one-handle call
  if (!head->post0) HIP_TRY(hipEventCreate(&head->post0));
  if (!head->post1) HIP_TRY(hipEventCreate(&head->post1));
  HIP_TRY(hipEventRecord(head->post0, hs));
  HIP_TRY(launch_post_steps(head, d1, head->frame.as<float>(), hs, sl, L, fb));
  HIP_TRY(hipEventRecord(head->post1, hs));
  // (4) wait, copy out
  HIP_TRY(hipStreamSynchronize(hs));
  if (int rc = drain_streams(scenes, n_scenes)) return rc;
  if (sl.features) {  // traced / missed: the sums over the ranks' blocks, into the first scene's before it is copied out
    uint32_t sum[2] = {0u, 0u};
    const size_t at = L.features * sizeof(uint32_t) + offsetof(rtg_features, traced);
    for (int i = 0; i < n_scenes; i++) {
      uint32_t tm[2] = {0u, 0u};
      HIP_TRY(hipSetDevice(scenes[i]->device));
      HIP_TRY(hipMemcpy(tm, scenes[i]->frame.as<const char>() + at, sizeof(tm), hipMemcpyDeviceToHost));
      sum[0] += tm[0], sum[1] += tm[1];
    }
    HIP_TRY(hipSetDevice(head->device));
    HIP_TRY(hipMemcpy(head->frame.as<char>() + at, sum, sizeof(sum), hipMemcpyHostToDevice));
  }
  const Extents back = copy_back_extents(L, compute);
  for (int k = 0; k < back.n; k++) HIP_TRY(hipMemcpy(host + back.e[k].lo, head->frame.as<const char>() + back.e[k].lo, back.e[k].hi - back.e[k].lo, hipMemcpyDeviceToHost));
  if (verbose) {  // the pack kernels (summed over the handles) and the first device's unpack kernels, by their events
    float pack_ms = 0.f, unpack_ms = 0.f;
    uint64_t items = 0;
    for (int i = 0; i < n_scenes; i++) {
      if (!at_head[i]) continue;
      float ms = 0.f;
      HIP_TRY(hipSetDevice(scenes[i]->device));
      HIP_TRY(hipEventElapsedTime(&ms, scenes[i]->pack0, scenes[i]->pack1));
      pack_ms += ms, items += rank_pix_work(dps[i]);
    }
    HIP_TRY(hipSetDevice(head->device));
    HIP_TRY(hipEventElapsedTime(&unpack_ms, head->unpack0, head->post0));
    // (tools/multi_planes_cost.py parses this line -- VERBOSE_LINE there: change both together)
    fprintf(stderr, "[rtg] multi planes: %d handle(s) on %zu device(s), %u words per pixel, %llu work items packed (%llu bytes), %zu through RCCL; pack %.4f ms, unpack %.4f ms\n",
            n_scenes, g.devs.size(), ps.words_per_pixel, (unsigned long long)items, (unsigned long long)(items * ps.words_per_pixel * 4u), through_rccl, pack_ms, unpack_ms);
  }
  if (int rc = multi_stats(scenes, n_scenes, samples, stats, count)) return rc;
  if (stats) {  // the slowest shard's render span + the first device's span for retire / filter / division
    float ms = 0.f;
    HIP_TRY(hipSetDevice(head->device));
    HIP_TRY(hipEventElapsedTime(&ms, head->post0, head->post1));
    stats->kernel_ms += ms;
  }
  return RTG_OK;
}
}  // namespace

int rtg_par_cast_multi(rtg_scene* const* scenes, int n_scenes, const rtg_camera* camera, const rtg_params* params,
                       float* out_rgb, rtg_stats* stats) {
  if (!scenes || n_scenes <= 0 || !camera || !params || !out_rgb) return fail(RTG_ERR_INVALID, "null argument");
  if (params->struct_size != sizeof(rtg_params)) return fail(RTG_ERR_INVALID, "rtg_params.struct_size mismatch");
  if (params->nranks > 1u) return fail(RTG_ERR_INVALID, "rtg_par_cast_multi shards by itself: params.rank / nranks must be 0 / 0|1");
  if (stats && stats->struct_size != sizeof(rtg_stats)) return fail(RTG_ERR_INVALID, "rtg_stats.struct_size mismatch");
  if ((params->flags & RTG_FLAG_DENOISE_ERROR) && !(params->flags & RTG_FLAG_DENOISE)) return fail(RTG_ERR_INVALID, "RTG_FLAG_DENOISE_ERROR needs RTG_FLAG_DENOISE");
  if ((params->flags & RTG_FLAG_RESUME) && params->sample_begin > params->ns) return fail(RTG_ERR_INVALID, "RTG_FLAG_RESUME: sample_begin > ns");
  // the flagged frames need scene option multi_planes on a handle (include/rtiow_gpu.h, at rtg_par_cast_multi)
  bool planes = false;
  for (int i = 0; i < n_scenes; i++) planes = planes || (scenes[i] && scenes[i]->multi_planes != 0);
  uint32_t plane_flags = 0;
  for (const auto& f : PLANE_FLAGS) {
    if (!planes && (params->flags & f.flag)) return fail(RTG_ERR_UNSUPPORTED, std::string("rtg_par_cast_multi: ") + f.name + " is not supported without scene option multi_planes");
    plane_flags |= f.flag;
  }
  for (int i = 0; i < n_scenes; i++) {
    if (!scenes[i]) return fail(RTG_ERR_INVALID, "null scene handle");
    // one handle = one frame, one work queue, one stream: the same handle twice would wipe its own tiles
    for (int k = 0; k < i; k++)
      if (scenes[k] == scenes[i]) return fail(RTG_ERR_INVALID, "rtg_par_cast_multi: the same scene handle appears twice (one handle per shard)");
    // ... and one estimator: tiles with light sampling beside tiles without it are no frame
    if (scenes[i]->light_sampling != scenes[0]->light_sampling) return fail(RTG_ERR_INVALID, "rtg_par_cast_multi: the handles disagree on scene option light_sampling");
  }
  // a call without any of the five flags is the plain frame whatever the option says
  const int rc = (params->flags & plane_flags) ? par_cast_multi_planes_body(scenes, n_scenes, camera, params, out_rgb, stats)
                                               : par_cast_multi_body(scenes, n_scenes, camera, params, out_rgb, stats);
  if (rc != RTG_OK) {
    // whatever was queued before the failure must not outlive the call (the caller may free out_rgb, destroy the handles
    // or call again): drain every stream that may hold work, keeping the first error message
    const std::string first = g_err;
    for (int i = 0; i < n_scenes; i++) {
      if (!scenes[i]->own_stream) continue;
      if (hipSetDevice(scenes[i]->device) == hipSuccess) (void)hipStreamSynchronize(scenes[i]->own_stream);
    }
    g_err = first;
  }
  return rc;
}

int rtg_multi_reset(const char* rccl_library_or_null, uint64_t* n_reduces_or_null) {
  std::lock_guard<std::mutex> lock(g_rccl.mu);
  if (n_reduces_or_null) *n_reduces_or_null = g_rccl.n_reduces;
  g_rccl.n_reduces = 0;
  rccl_drop_comms();
  if (g_rccl.lib) dlclose(g_rccl.lib);
  g_rccl.lib = nullptr;
  g_rccl.CommInitAll = nullptr, g_rccl.CommDestroy = nullptr, g_rccl.GroupStart = nullptr, g_rccl.GroupEnd = nullptr;
  g_rccl.Reduce = nullptr, g_rccl.GetErrorString = nullptr;
  g_rccl.path = rccl_library_or_null ? rccl_library_or_null : "";
  return RTG_OK;
}

