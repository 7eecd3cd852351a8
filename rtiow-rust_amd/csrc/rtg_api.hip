// rtg_api.hip -- kernels + the C ABI of include/rtiow_gpu.h (librtiow_gpu.so).
//
// There is no CPU fallback anywhere in this file: without a HIP device every compute entry point
// returns RTG_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enums only: librccl is dlopen()ed by rtg_par_cast_multi, never linked

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <functional>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/rtiow_gpu.h"
#include "../../include/rtiow_gpu_debug.h"
#include "../../include/rtiow_gpu_query.h"
#include "../../include/rtiow_gpu_rays.h"
#include "../../include/rtiow_gpu_image.h"
#include "../../include/rtiow_gpu_mesh.h"
#include "../../include/rtiow_gpu_surface.h"
#include "../../include/rtiow_gpu_environment.h"
#include "rt_pool.h"
#include "rt_box_plan.h"
#include "rt_camera_probe.h"
#include "rt_retire.h"
#include "rt_denoise.h"
#include "rt_features.h"
#include "rt_multi_planes.h"
#include "rt_pool_full.h"
#include "rt_sync_full.h"
#include "rt_pool2.h"
#include "rt_trace.h"
#include "rt_light.h"
#include "rt_query.h"
#include "scene_builder.h"

using namespace rtg;

#include "rtg_kernels.inc"

// ===================================================================================================
// Host side
// ===================================================================================================
namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int hip_fail(hipError_t e, const char* what) {
  return fail(RTG_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);   \
  } while (0)
}  // namespace

struct rtg_builder {
  SceneBuilder sb;
};

// Everything ONE frame in flight owns: work-queue head and statistics, launch constants, cost-ordered queue, per-sample scratch,
// path slots / stacks, timing events.  A scene handle keeps a ring of these (option frames_in_flight, default 1); a call takes
// the next one and first waits for the frame that used it last (`done`), so asynchronous calls on one handle are always safe
// and, with more than one context, overlap.
constexpr int RTG_MAX_FRAMES = 4;
// The kernel that rendered a frame (rtg_launch.inc launch_render)
enum class KernelKind { baseline, lean_pool, full_pool, lock_step, pool2 };
// A device allocation that a handle owns and grows on demand: it never shrinks; when it is too small it is freed and allocated
// anew (nothing is held when that fails).  The device it lives on is current when grow / release are called.
struct DevMem {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t grow(size_t need) {
    if (need <= bytes) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p, need);
    if (e == hipSuccess) bytes = need;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr, bytes = 0;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

struct LaunchCtx {
  unsigned long long* d_counters = nullptr;  // [0..4] N/P/H/rays/draws, [7] = work-queue head (persistent kernel), [8..] schedule statistics
  hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr;
  bool busy = false;            // `done` was recorded and not waited for yet
  DevMem stack;                 // float: full-feature pool kernel: per-wave transform stacks
  DevMem slots;                 // uint32_t: ray-pool path slots when they live in global memory
  DevMem scratch;               // float: per-sample colours (sample passes: rtg_launch.inc)
  LaunchConsts* d_consts = nullptr;  // camera / frame parameters / chunk description of the launch (rt_pool.h), written on the launch stream
  DevMem lpt;                   // uint32_t: cost-ordered work queue (rt_pool.h LptQueue)
  LptQueue lpt_desc{};          // descriptor of the last launch (RTG_VERBOSE histogram)
  KernelKind last_kernel = KernelKind::baseline;  // what launch_render chose last
  uint32_t last_pix_work = 0;   // pixel work items of that launch (tiles x tile area), 0 when it kept no per-sample scratch
  DevMem list;                  // uint32_t: RTG_FLAG_SAMPLE_COUNTS: the active-pixel list and its inverse (rt_pool.h ListConsts), 2 x the rank's work items
  DevMem compact;               // ... the compaction's per-block counts, offsets and samples, and its CompactResult
  unsigned long long counts_samples = 0;  // ... rtg_stats.samples of the last counts call
  DevMem retire;                // RTG_FLAG_RETIRE: the OK bit plane and the retire kernels' per-block partials (rt_retire.h)
  const char* refusal = nullptr;  // ... set by launch_counts when a block's in-fields are refused (RTG_ERR_INVALID, nothing written)
  DevMem denoise;               // RTG_FLAG_DENOISE: the per-pixel (m, v, valid) records and the prepare kernel's per-block counts (rt_denoise.h)
  DevMem features;              // uint32_t: RTG_FLAG_FEATURES: the feature kernel's per-block counts (rt_features.h)
};

// The camera plan of ONE (program, camera) pair (rt_camera_probe.h, rtg_launch.inc camera_plan): the probe's counts on their way
// to the host, then the record offsets of the image that leaves out what the tree DP picks from those counts.  A scene keeps
// CAMERA_PLANS of them, least recently used evicted; the buffers stay with the entry (every program of a scene has n_prog records).
constexpr int CAMERA_PLANS = 4;
constexpr size_t CAMERA_KEY_BYTES = sizeof(DevCamera) + 2;
struct CameraPlan {
  enum State { FREE, PROBING, PLANNED } state = FREE;
  unsigned char key[CAMERA_KEY_BYTES] = {};  // the DevCamera bytes, then which program is staged: box_tree, box_chains
  uint64_t stamp = 0;            // last use (rtg_scene::cam_clock)
  hipEvent_t ev = nullptr;       // behind the copy of the counts, then behind the upload of the table
  hipStream_t up_stream = nullptr;  // ... the stream that upload went to (a launch on another stream waits for ev)
  uint32_t* d_counts = nullptr;  // n + 1 words: the probe's n_pass and its ray count
  uint32_t* h_words = nullptr;   // pinned, 2 n + 1 words: the counts, then the offsets on their way up
  uint32_t* d_off = nullptr;     // n words: the record offsets of the camera's image
  uint32_t bytes = 0;            // ... and its size
  uint32_t n_pruned = 0, n_rays = 0;
  float plan_ms = 0.f;           // host time of the DP and the table (option verbose, tools/camera_plan_cost.py)
};

// The LDS images of ONE lean program (rt_pool.h): the full one, the one without box-chain followers and the ones without the
// records of the pruning plan.  A scene has two: the reference program's and the rebuilt one's (rt_box_plan.h box_tree_rebuild).
struct LeanImages {
  const uint4* lo = nullptr;   // the program on the device; nullptr = the scene has no such program
  const uint4* hi = nullptr;
  const uint32_t* d_off = nullptr;  // record offsets of the full image, and its size
  uint32_t bytes = 0;
  uint32_t n_followers = 0;    // records the production image drops (0: it is the full image, and no table is allocated)
  const uint32_t* d_chain_off = nullptr;  // the record offsets of that image
  uint32_t chain_bytes = 0;    // ... and its size
  bool planned = false;        // the pruning plan is made (at creation for the program that production launches stage, else on demand)
  uint32_t n_pruned = 0;       // records the plan leaves out beyond the followers
  float plan_ms = 0.f;         // host time of the plan (option verbose)
  // record offsets of the pruned image, [1] without the followers too (the default), [0] with them
  // (option box_chains = 0: a measurement switch, so that table is made when the option is first set -- prune_table below)
  const uint32_t* d_prune_off[2] = {nullptr, nullptr};
  uint32_t prune_bytes[2] = {0, 0};
  std::vector<uint32_t> plan_ops;  // ... from these: every record's flag word and its mask (BOX_KEPT / BOX_FOLLOWER / BOX_PRUNED)
  std::vector<uint8_t> plan_mask;
  std::vector<uint8_t> follower;
  // camera plan: the host copy of the program, whether program_shape accepts it (-1: not asked yet; 0: no probe, no camera plan)
  // and which of its spheres end a probe path (rt_camera_probe.h camera_probe_stops), on the device from the first probe on
  const std::vector<Packet>* h_lo = nullptr;
  const std::vector<Packet>* h_hi = nullptr;
  int probe_ok = -1;
  uint8_t* d_stop = nullptr;
};

struct rtg_scene {
  int device = 0;
  DevScene dev{};
  uint32_t features = 0;
  uint32_t n_prog = 0, n_mat = 0, n_tex = 0;
  std::vector<uint8_t> tex_kind;  // kind of every texture record (flat_scene.h TexKind, TEX_EXT): which ids rtg_debug_texture evaluates
  std::vector<uint32_t> tex_child;  // ... and the child of every TEX_SURFACE id (include/rtiow_gpu_surface.h), the id itself otherwise
  // The environment the builder carried when the scene was made (include/rtiow_gpu_environment.h), as the kernels read it from the
  // frame parameters of a call without an RTG_FLAG_BACKGROUND block (rt_device.h BG_TEXTURE); mode BG_NONE: the scene has none
  Background env_bg{BG_NONE, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  uint64_t bytes = 0;
  std::vector<void*> owned;    // what `upload` allocated: freed when the scene is destroyed
  const uint32_t* d_parent = nullptr;  // the wrapper around every program record (rt_pool_full.h rebuild_hit)
  hipStream_t own_stream = nullptr;  // rtg_par_cast_multi: this scene's launch stream (created on first use)
  int num_cus = 0;
  DevMem frame;                // rtg_par_cast: device staging frame for host framebuffers
  int force_chunks = 0;        // RTG_CHUNKS: 0 = automatic
  uint64_t scratch_limit = 0;  // option scratch_mb: budget of the per-sample colour scratch in bytes, 0 = half of the free HBM
  bool whole_scratch = false;  // the kernel trace reads every sample colour back: one pass regardless of the budget
  int verbose = 0;
  int window = -1;             // full-feature kernel: records of the program staged in LDS (-1 = as many as fit)
  int ray_lds = 1;             // 0: all slot fields in global memory
  int force_rccl = 0;          // rtg_par_cast_multi: run the RCCL reduce even over ONE distinct device (a clique of one)
  int multi_gather = 0;        // rtg_par_cast_multi: 1 = the packed collective (every scene ships its own tiles only; rtg_multi.inc) instead of the full-frame reduce
  DevMem pack;                 // ... this scene's planes, packed in work-item order (on its device)
  DevMem recv;                 // ... and where they arrive on the first device
  int multi_planes = 0;        // rtg_par_cast_multi: 1 = accept the flagged frames (SUM_SQUARES .. FEATURES): every plane gathered on the first device, which retires, filters and divides (rtg_multi.inc)
  hipEvent_t post0 = nullptr, post1 = nullptr;  // ... the first device's span for that step (rtg_stats.kernel_ms), created on first use
  hipEvent_t pack0 = nullptr, pack1 = nullptr, unpack0 = nullptr;  // ... option verbose: this scene's pack kernel, and where the first device's unpack kernels begin (they end at post0)
  int bvh4 = 0;                // 1: traverse the 4-wide collapse of the Bvh (same image, other counters; needs wide_bytes)
  const uint32_t* d_wide = nullptr;  // the 4-wide image
  uint32_t wide_bytes = 0;     // ... and its size, 0 = the scene has none
  int box_chains = 1;          // production launches of the lean pool kernel stage the image without box-chain followers (rt_pool.h); 0 = off
  // box pruning (rt_box_plan.h): 1 = production launches stage the image without the plan's interior boxes, 2 = counting launches
  // too (their aabb_tests then report what the production walk executes), 0 = off
  int box_prune = 1;
  // box tree (rt_box_plan.h box_tree_rebuild): 1 = production launches of the staged lean pool kernel (and, with box_prune = 2,
  // its counting launches) walk the program whose Bvh regions are rebuilt over the same leaf order; 0 = the reference program
  int box_tree = 1;
  // camera plan (rtg_launch.inc camera_plan): 1 = launches that stage a pruned image probe the camera they render with once, when
  // they are large enough, and every later launch with that camera stages the image planned from the probe's counts; 2 = every
  // such launch, planned before it runs (tests and measurements); 0 = off
  int box_camera = 1;
  int cam_paths = (int)CAMERA_PROBE_PATHS, cam_bounces = (int)CAMERA_PROBE_BOUNCES, cam_trips = (int)CAMERA_PROBE_TRIPS;  // options box_camera_paths / _bounces / _trips (the sweeps of profiles/r24_camera_plan/)
  CameraPlan cam_plans[CAMERA_PLANS];
  uint64_t cam_clock = 0;
  std::vector<Packet> t_lo, t_hi;  // host copy of the rebuilt program (the reference program's: h_lo / h_hi below)
  LeanImages ref;              // the reference program (dev.lo / dev.hi)
  LeanImages tree;             // the rebuilt one; tree.lo = nullptr: no region was rebuilt
  bool tree_tried = false;     // ... and whether the rebuild has run
  float tree_ms = 0.f;         // host time of the rebuild (option verbose)
  uint32_t n_regions = 0;      // regions rebuilt
  bool plannable = false;      // a lean program whose image may fit a CU's LDS without its interior boxes: it gets plans
  std::vector<Packet> h_lo, h_hi;  // ... and keeps the host copy that plans made on demand read
  int sync_full = -1;          // full-feature scenes on the pool-free lock-step kernel (rt_sync_full.h): -1 = when the program holds no BOX record, 0 / 1 = never / always
  uint32_t n_box = 0;          // BOX records of the flat program
  int lpt = 2;                 // RTG_LPT=0: natural order throughout; 1 / 2 = LptQueue::mode
  int lpt_deep = 4;            // RTG_LPT_DEEP: scatter events at bounce >= this make up a block's cost
  int lpt_shift = 0;           // RTG_LPT_SHIFT: merge cost classes in groups of 1 << shift
  int lpt_phase1 = 0;          // RTG_LPT_PHASE1: chunks in natural order, 0 = n_chunks / 8 clamped to [2, 8]
  // 3 = ray-pool kernels (rt_pool.h / rt_pool_full.h), 1 = one-lane-per-pixel baseline (rt_trace.h) for every scene
  int kernel_version = 3;
  PoolTuning pool_tune{40, 16, 24, 16, 16, 40};  // lean ray-pool kernel (refill_min, sphere_min, box_leave: profiles/r02_e_final/lean_knob_sweep.txt, middle of round 2)
  PoolTuning full_tune{20, 24, 32, 16, 24, 40};  // full-feature pool kernel (a service there also has hit records to move)
  PoolTuning sync_tune{20, 16, 32, 16, 16, 40};  // lock-step kernel (only run_ahead / run_ahead_min / gather_min matter there)
  int wg_per_cu = 0;                       // 0 = ask the occupancy API
  int full_threads = 0;                    // full-feature pool kernel: 0 = the variant's maximum (RTG_BLOCK overrides)
  int pool_threads = 0;                    // lean ray-pool kernel: 0 = ONE 16-wave workgroup per CU shares one LDS copy of the program (RTG_BLOCK overrides)
  int mat_lds = 1;                          // full-feature kernels: material records staged in LDS when they fit (0 = always from global memory)
  int deep_sized = 1;                       // FEAT_DEEP graphs: the general walk instantiated for the graph's real depths (0 = always 32 wrappers x 3 media levels)
  int hoist = 1;                            // full-feature pool kernel: evaluate the hoisted segment when a ray is created (flat_scene.h OP_SEG); 0 = the walk executes its records
  uint32_t seg_first = 0, seg_end = 0;      // ... its records, as record indices (0, 0: the program has none)
  int drain_share = 1;                      // pool kernels, drain-phase work sharing (rt_pool_full.h RT_DRAIN_SHARE): 0 = off
  // The second program and its kernel (rt_pool2.h; flat_scene.h "the list level, hoisted"): n_prog2 = 0 when the world has another shape
  int pool2 = 1;                            // 1 (default): programs with a second program run on the pool-2 kernel; 0: on the first full-feature kernel
  uint32_t n_prog2 = 0, n_box2 = 0;
  DevScene dev2{};                          // lo / hi = the second program; materials, textures, Perlin tables shared
  const P2Table* d_p2 = nullptr;            // ... and its table
  Pool2Tuning pool2_tune{24, 48, 40, 4, 8, 24, 2};  // refill_min, box_leave, park_max, t_sphere, t_prism, t_list, t_push
  int guide_lds = 0;                       // guided filter (rt_denoise.h GUIDED): 1 = the neighbours' feature records from an LDS copy, 0 = through the caches
  int small_frames = 1;                    // rtg_launch.inc pool_geometry: frames smaller than the chip get small workgroups and reservations
  // Scene option light_sampling (rt_light.h): 1 = every frame on the one-lane-per-pixel kernels over color_ls.  The table is made
  // when the scene is created (scene_builder.cpp light_table), on the host; it goes to buffers of its own when the option is first
  // set to 1 (unless it is empty or too long), so a handle that never sets the option holds and reports the bytes it always did.
  int light_sampling = 0;
  uint32_t n_lights = 0;                   // the table's length, whatever it is
  std::vector<LightRect> h_lights;         // the table and the per-material sampled bytes
  std::vector<uint8_t> h_sampled;
  LightTable lights{nullptr, nullptr, 0};  // on the device: .n = 0 until uploaded, and when there is nothing to sample
  // Scene option query_lds (include/rtiow_gpu_query.h): which kernel answers ray queries -- 0 = always the general one, 2 = the
  // lean kernel whenever the program is lean and fits LDS, 1 = that kernel from QUERY_LDS_MIN_RAYS rays upward (rtg_query.inc)
  int query_lds = 1;
  int query_refill = 16;  // ... and the finished lanes of a wave at which the lean kernel runs its refill arm (rt_query.h; measurement switch)
  // Scene option ray_pool (include/rtiow_gpu_rays.h): which kernel renders ray frames -- 1 = lean programs on the RAYS instantiations
  // of the lean pool kernel, 0 = always the general kernel (rtg_rays.inc).  The same bits either way.
  int ray_pool = 1;
  LaunchCtx ctx[RTG_MAX_FRAMES];           // frames in flight
  int n_ctx = 1, next_ctx = 0;
  LaunchCtx* cx = &ctx[0];                 // the context of the call being made (ctx_acquire)
};

// A context that leaves the ring (frames_in_flight lowered) or whose scene is destroyed: wait for its frame, free what it
// holds (the sample scratch alone may be a large part of the HBM).  The events and the small buffers stay for reuse.
static void ctx_free_buffers(LaunchCtx* c) {
  if (c->busy) (void)hipEventSynchronize(c->done);
  c->busy = false;
  for (DevMem* m : {&c->scratch, &c->slots, &c->stack, &c->lpt, &c->list, &c->compact, &c->retire, &c->denoise, &c->features}) m->release();
}

// Take the next launch context of the ring: create its small buffers on first use, wait for the frame that used it last.
static int ctx_acquire(rtg_scene* s) {
  LaunchCtx* c = &s->ctx[s->next_ctx];
  s->next_ctx = (s->next_ctx + 1) % s->n_ctx;
  if (!c->d_counters) {
    if (hipMalloc((void**)&c->d_counters, 64 * sizeof(unsigned long long)) != hipSuccess || hipMemset(c->d_counters, 0, 64 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc((void**)&c->d_consts, sizeof(LaunchConsts) + sizeof(ListConsts)) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreate(&c->ev1) != hipSuccess || hipEventCreateWithFlags(&c->done, hipEventDisableTiming) != hipSuccess)
      return fail(RTG_ERR_DEVICE, "scene: launch-context allocation failed");
  }
  if (c->busy) {
    hipError_t e = hipEventSynchronize(c->done);
    c->busy = false;
    if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize(previous frame of this launch context)");
  }
  s->cx = c;
  return RTG_OK;
}
// A counting launch starts from cleared counters and schedule statistics ([7], the work-queue head, is the kernels' own)
static hipError_t clear_counters(LaunchCtx* c, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(c->d_counters, 0, 7 * sizeof(unsigned long long), stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->d_counters + 8, 0, 24 * sizeof(unsigned long long), stream);
  return e;
}
// ... and mark it in flight on `stream` once its work is enqueued
static int ctx_release(rtg_scene* s, hipStream_t stream) {
  hipError_t e = hipEventRecord(s->cx->done, stream);
  if (e != hipSuccess) return hip_fail(e, "hipEventRecord(done)");
  s->cx->busy = true;
  return RTG_OK;
}

// Progressive rendering (include/rtiow_gpu.h RTG_FLAG_PARTIAL / RTG_FLAG_RESUME): the samples one call renders and what it does
// at the end.  The default is the whole frame: samples [0, ns), divided by ns.
struct SampleSlice {
  uint32_t begin = 0;   // first sample this call renders; the framebuffer holds the running sum of [0, begin) when it is > 0
  bool divide = true;   // false under RTG_FLAG_PARTIAL: the running sum stays in the framebuffer
  bool squares = false; // RTG_FLAG_SUM_SQUARES: the framebuffer has a second plane, the running sum of the squared colours
  bool counts = false;  // RTG_FLAG_SAMPLE_COUNTS: the framebuffer ends with the count plane; the pool kernels run over a list
  uint32_t list_work = 0;  // ... set by the launcher (launch_counts): the list's length, a multiple of 256
  ListConsts list{};       // ... and where the list, its inverse and the count plane are
  bool retire = false;  // RTG_FLAG_RETIRE: the framebuffer ends with an rtg_retire block; the retire step runs before the division
  bool denoise = false; // RTG_FLAG_DENOISE: the framebuffer ends with an rtg_denoise block and the output plane; the filter runs before the division
  bool features = false; // RTG_FLAG_FEATURES: the framebuffer ends with an rtg_features block and the albedo / normal / depth planes
  bool error = false;   // RTG_FLAG_DENOISE_ERROR: the framebuffer ends with the error plane; the filter runs before the retire step, which reads it
  // RTG_FLAG_BACKGROUND: the framebuffer ends with an rtg_background block whose in-fields the call reads from the frame and puts
  // into its frame parameters (DevParams::bg).  The ranks of rtg_par_cast_multi get them from the host block instead: not set there
  bool background = false;
  bool sliced() const { return begin != 0u || !divide; }
};
static SampleSlice slice_of(const rtg_params* p) {
  SampleSlice sl;
  if (p->flags & RTG_FLAG_RESUME) sl.begin = p->sample_begin;
  if (p->flags & RTG_FLAG_PARTIAL) sl.divide = false;
  if (p->flags & RTG_FLAG_SUM_SQUARES) sl.squares = true;
  if (p->flags & RTG_FLAG_SAMPLE_COUNTS) sl.counts = true;
  if (p->flags & RTG_FLAG_RETIRE) sl.retire = true;
  if (p->flags & RTG_FLAG_DENOISE) sl.denoise = true;
  if (p->flags & RTG_FLAG_FEATURES) sl.features = true;
  if (p->flags & RTG_FLAG_DENOISE_ERROR) sl.error = true;
  if (p->flags & RTG_FLAG_BACKGROUND) sl.background = true;
  return sl;
}

// The frame layout (FrameLayout) is rt_multi_planes.h's host part.
// RTG_FLAG_RETIRE: why the block's in-fields are refused (nullptr: accepted)
static const char* retire_refusal(const rtg_retire& r, uint32_t nranks) {
  if (r.radius > RTG_RETIRE_MAX_RADIUS) return "RTG_FLAG_RETIRE: radius > RTG_RETIRE_MAX_RADIUS";
  if (!(r.target_se >= 0.0)) return "RTG_FLAG_RETIRE: target_se is NaN or negative";
  if (r.radius > 0u && nranks > 1u) return "RTG_FLAG_RETIRE: radius > 0 needs nranks = 1 (the neighbours live on other ranks)";
  return nullptr;
}

// RTG_FLAG_DENOISE: why the block's in-fields are refused (nullptr: accepted)
static const char* denoise_refusal(const rtg_denoise& r, uint32_t nranks) {
  if (r.radius > RTG_DENOISE_MAX_RADIUS) return "RTG_FLAG_DENOISE: radius > RTG_DENOISE_MAX_RADIUS";
  if (r.patch > RTG_DENOISE_MAX_PATCH) return "RTG_FLAG_DENOISE: patch > RTG_DENOISE_MAX_PATCH";
  if (!(r.k > 0.f) || !std::isfinite(r.k)) return "RTG_FLAG_DENOISE: k is NaN, infinite or <= 0";
  if (r.reserved_in != 0u) return "RTG_FLAG_DENOISE: reserved_in != 0";
  if (nranks > 1u) return "RTG_FLAG_DENOISE needs nranks = 1 (the neighbours live on other ranks)";
  return nullptr;
}

// RTG_FLAG_FEATURES: why the block's in-fields are refused (nullptr: accepted)
static const char* features_refusal(const rtg_features& r, bool denoise) {
  if (r.grid == 0u || r.grid > RTG_FEATURES_MAX_GRID) return "RTG_FLAG_FEATURES: grid is 0 or > RTG_FEATURES_MAX_GRID";
  if (r.compute > 1u) return "RTG_FLAG_FEATURES: compute > 1";
  if (r.reserved_in != 0u) return "RTG_FLAG_FEATURES: reserved_in != 0";
  for (float sg : {r.sigma_normal, r.sigma_albedo, r.sigma_depth})
    if (denoise && (!(sg > 0.f) || !std::isfinite(sg))) return "RTG_FLAG_FEATURES with RTG_FLAG_DENOISE: a sigma is NaN, infinite or <= 0";
  return nullptr;
}

// RTG_FLAG_BACKGROUND: why the block's in-fields are refused (nullptr: accepted)
static const char* background_refusal(const rtg_background& r) {
  if (r.mode > 1u) return "RTG_FLAG_BACKGROUND: mode > 1";
  if (r.reserved_in != 0u) return "RTG_FLAG_BACKGROUND: reserved_in != 0";
  return nullptr;
}
// ... and the accepted block as the kernels read it (rt_device.h Background)
static Background dev_background(const rtg_background& r) {
  Background b;
  b.mode = r.mode == 0u ? BG_CONSTANT : BG_GRADIENT;
  for (int c = 0; c < 3; c++) b.bottom[c] = r.bottom[c], b.top[c] = r.top[c];
  return b;
}

// The in-fields of a flagged frame's blocks, in ONE place: read (from the host frame by check_blocks, from the device frame by
// read_blocks), checked by blocks_refusal, then handed to the launchers as an argument.
struct FrameBlocks {
  rtg_retire retire{};
  rtg_denoise denoise{};
  rtg_features features{};
  rtg_background background{};
};
// Enqueue on `stream` the read-backs of the in-fields of the blocks the slice's flags name; the caller synchronises
static hipError_t read_blocks(const FrameLayout& L, const SampleSlice& sl, const float* d_out, hipStream_t stream, FrameBlocks* fb) {
  hipError_t e = hipSuccess;
  if (sl.retire) e = hipMemcpyAsync(&fb->retire, d_out + L.retire, offsetof(rtg_retire, active), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && sl.denoise) e = hipMemcpyAsync(&fb->denoise, d_out + L.denoise, offsetof(rtg_denoise, filtered), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && sl.features) e = hipMemcpyAsync(&fb->features, d_out + L.features, offsetof(rtg_features, traced), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && sl.background) e = hipMemcpyAsync(&fb->background, d_out + L.background, offsetof(rtg_background, reserved), hipMemcpyDeviceToHost, stream);
  return e;
}
// Why a call of `nranks` ranks refuses those in-fields (nullptr: accepted)
static const char* blocks_refusal(const SampleSlice& sl, const FrameBlocks& fb, uint32_t nranks) {
  const char* why = nullptr;
  if (sl.retire && (why = retire_refusal(fb.retire, nranks))) return why;
  if (sl.denoise && (why = denoise_refusal(fb.denoise, nranks))) return why;
  if (sl.features && (why = features_refusal(fb.features, sl.denoise))) return why;
  if (sl.background && (why = background_refusal(fb.background))) return why;
  return nullptr;
}

#include "rtg_launch.inc"

template <typename T>
struct DevBuf {
  T* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t n) { return hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)); }
};

// `bytes` of `src` in a device allocation of their own, which the scene owns until it is destroyed and counts in rtg_scene::bytes
// (an empty upload still takes 16 bytes); *dst = the typed pointer
template <typename T>
static int upload(rtg_scene* s, const T** dst, const void* src, size_t bytes) {
  const size_t alloc = bytes ? bytes : 16;
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, alloc));
  s->owned.push_back(p);
  if (bytes) HIP_TRY(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
  s->bytes += alloc;
  *dst = static_cast<const T*>(p);
  return RTG_OK;
}

extern "C" {

const char* rtg_version(void) { return "rtiow-rust_amd 0.2 (gfx950 HIP; flat-program ray-pool kernels; flat-program encoding 3: OP_SEG = 9, OP_SAVE / OP_MERGE / OP_EXT = 10 / 11 / 12, OP_LIST = 13, MEDIUM lo.y = 1 / density)"; }
const char* rtg_last_error(void) { return g_err.c_str(); }

int rtg_device_count(int* n) {
  if (!n) return fail(RTG_ERR_INVALID, "null argument");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    return hip_fail(e, "hipGetDeviceCount");
  }
  *n = c;
  return RTG_OK;
}

int rtg_builder_create(rtg_builder** out) {
  if (!out) return fail(RTG_ERR_INVALID, "null argument");
  *out = new rtg_builder();
  return RTG_OK;
}
void rtg_builder_destroy(rtg_builder* b) { delete b; }

// ---- textures ------------------------------------------------------------------------------------
static rtg_id bad(const char* msg) {
  fail(RTG_ERR_INVALID, msg);
  return RTG_INVALID_ID;
}

rtg_id rtg_texture_constant(rtg_builder* b, const float rgb[3]) {
  if (!b || !rgb) return bad("null argument");
  HostTexture t;
  t.kind = TEX_CONSTANT;
  t.rgb[0] = rgb[0], t.rgb[1] = rgb[1], t.rgb[2] = rgb[2];
  b->sb.textures.push_back(t);
  return (rtg_id)b->sb.textures.size() - 1;
}
rtg_id rtg_texture_checker(rtg_builder* b, rtg_id t0, rtg_id t1) {
  if (!b) return bad("null argument");
  if (t0 >= b->sb.textures.size() || t1 >= b->sb.textures.size()) return bad("checker: bad texture handle");
  if (b->sb.textures[t0].kind == TEX_EXT || b->sb.textures[t1].kind == TEX_EXT) return bad("checker: bad texture handle");
  if (b->sb.textures[t0].kind == TEX_SURFACE || b->sb.textures[t1].kind == TEX_SURFACE) return bad("checker: a surface texture is no checker child");
  HostTexture t;
  t.kind = TEX_CHECKER;
  t.t0 = t0, t.t1 = t1;
  b->sb.textures.push_back(t);
  return (rtg_id)b->sb.textures.size() - 1;
}
rtg_id rtg_texture_perlin(rtg_builder* b, float scale) {
  if (!b) return bad("null argument");
  if (!b->sb.has_perlin) return bad("perlin: call rtg_builder_set_perlin_tables first");
  HostTexture t;
  t.kind = TEX_PERLIN;
  t.scale = scale;
  b->sb.textures.push_back(t);
  return (rtg_id)b->sb.textures.size() - 1;
}
int rtg_builder_set_perlin_tables(rtg_builder* b, const float vecs[768], const uint8_t px[256],
                                  const uint8_t py[256], const uint8_t pz[256]) {
  if (!b || !vecs || !px || !py || !pz) return fail(RTG_ERR_INVALID, "null argument");
  for (int i = 0; i < 256; i++) {
    b->sb.perlin_vecs[4 * i] = vecs[3 * i], b->sb.perlin_vecs[4 * i + 1] = vecs[3 * i + 1];
    b->sb.perlin_vecs[4 * i + 2] = vecs[3 * i + 2], b->sb.perlin_vecs[4 * i + 3] = 0.f;
    b->sb.perlin_perm[i] = px[i], b->sb.perlin_perm[256 + i] = py[i], b->sb.perlin_perm[512 + i] = pz[i];
  }
  b->sb.has_perlin = true;
  return RTG_OK;
}

// ---- materials -----------------------------------------------------------------------------------
static rtg_id push_material(rtg_builder* b, uint32_t kind, rtg_id tex, const float* albedo, float param) {
  if (!b) return bad("null argument");
  HostMaterial m;
  m.kind = kind;
  if (tex != RTG_INVALID_ID) {
    if (tex >= b->sb.textures.size() || b->sb.textures[tex].kind == TEX_EXT) return bad("material: bad texture handle");
    if (kind == MAT_ISOTROPIC && b->sb.textures[tex].kind == TEX_SURFACE) return bad("isotropic: a medium has no surface for a surface texture");
    m.tex = tex;
  }
  if (albedo) m.albedo[0] = albedo[0], m.albedo[1] = albedo[1], m.albedo[2] = albedo[2];
  m.param = param;
  b->sb.materials.push_back(m);
  return (rtg_id)b->sb.materials.size() - 1;
}
rtg_id rtg_material_lambertian(rtg_builder* b, rtg_id albedo) {
  if (albedo == RTG_INVALID_ID) return bad("material: bad texture handle");
  return push_material(b, MAT_LAMBERTIAN, albedo, nullptr, 0.f);
}
rtg_id rtg_material_metal(rtg_builder* b, const float albedo[3], float fuzz) {
  if (!albedo) return bad("null argument");
  return push_material(b, MAT_METAL, RTG_INVALID_ID, albedo, fuzz);
}
rtg_id rtg_material_dielectric(rtg_builder* b, float ref_idx) {
  return push_material(b, MAT_DIELECTRIC, RTG_INVALID_ID, nullptr, ref_idx);
}
rtg_id rtg_material_diffuse_light(rtg_builder* b, rtg_id emission, float brightness) {
  if (emission == RTG_INVALID_ID) return bad("material: bad texture handle");
  return push_material(b, MAT_DIFFUSE_LIGHT, emission, nullptr, brightness);
}
rtg_id rtg_material_isotropic(rtg_builder* b, rtg_id albedo) {
  if (albedo == RTG_INVALID_ID) return bad("material: bad texture handle");
  return push_material(b, MAT_ISOTROPIC, albedo, nullptr, 0.f);
}

// ---- objects -------------------------------------------------------------------------------------
static rtg_id push_object(rtg_builder* b, const HostObject& o) {
  if (!b) return bad("null argument");
  try {
    return b->sb.add_object(o);
  } catch (const BuildError& e) {
    fail(e.code, e.msg);
    return RTG_INVALID_ID;
  }
}
rtg_id rtg_object_sphere(rtg_builder* b, float radius, rtg_id material) {
  HostObject o;
  o.kind = HostObject::SPHERE;
  o.f[0] = radius;
  o.mat = material;
  return push_object(b, o);
}
rtg_id rtg_object_rect(rtg_builder* b, int axis, float r0s, float r0e, float r1s, float r1e, float k, rtg_id material) {
  HostObject o;
  o.kind = HostObject::RECT;
  o.axis = axis;
  o.f[0] = k, o.f[1] = r0s, o.f[2] = r0e, o.f[3] = r1s, o.f[4] = r1e;
  o.mat = material;
  return push_object(b, o);
}
static rtg_id wrapper(rtg_builder* b, HostObject::Kind kind, const float* v, rtg_id child) {
  HostObject o;
  o.kind = kind;
  if (v) o.f[0] = v[0], o.f[1] = v[1], o.f[2] = v[2];
  o.a = child;
  return push_object(b, o);
}
rtg_id rtg_object_flip_normals(rtg_builder* b, rtg_id object) { return wrapper(b, HostObject::FLIP, nullptr, object); }
rtg_id rtg_object_translate(rtg_builder* b, const float offset[3], rtg_id object) {
  if (!offset) return bad("null argument");
  return wrapper(b, HostObject::TRANSLATE, offset, object);
}
rtg_id rtg_object_scale(rtg_builder* b, const float factor[3], rtg_id object) {
  if (!factor) return bad("null argument");
  return wrapper(b, HostObject::SCALE, factor, object);
}
// object.rs:477-484: radians = degrees * PI / 180; sin/cos via the platform libm (host-side setup).  The one place the pair is
// made: rtg_object_rotate_y and rtg_builder_set_environment (rtg_environment.inc)
static void rotate_y_pair(float degrees, float* s, float* c) {
  float radians = degrees * 3.14159265358979323846f / 180.f;
  *s = sinf(radians), *c = cosf(radians);
}
rtg_id rtg_object_rotate_y(rtg_builder* b, float degrees, rtg_id object) {
  float sc[3] = {0.f, 0.f, 0.f};
  rotate_y_pair(degrees, &sc[0], &sc[1]);
  return wrapper(b, HostObject::ROTATE_Y, sc, object);
}
rtg_id rtg_object_and(rtg_builder* b, rtg_id o0, rtg_id o1) {
  HostObject o;
  o.kind = HostObject::AND;
  o.a = o0, o.b = o1;
  return push_object(b, o);
}
rtg_id rtg_object_rect_prism(rtg_builder* b, const float p0[3], const float p1[3], rtg_id m) {
  // object.rs:420-473: And(And(+Z, And(+Y, +X)), And(Flip(-Z), And(Flip(-Y), Flip(-X))))
  if (!b || !p0 || !p1) return bad("null argument");
  rtg_id zp = rtg_object_rect(b, 2, p0[0], p1[0], p0[1], p1[1], p1[2], m);
  rtg_id yp = rtg_object_rect(b, 1, p0[0], p1[0], p0[2], p1[2], p1[1], m);
  rtg_id xp = rtg_object_rect(b, 0, p0[1], p1[1], p0[2], p1[2], p1[0], m);
  if (zp == RTG_INVALID_ID || yp == RTG_INVALID_ID || xp == RTG_INVALID_ID) return RTG_INVALID_ID;
  rtg_id zn = rtg_object_flip_normals(b, rtg_object_rect(b, 2, p0[0], p1[0], p0[1], p1[1], p0[2], m));
  rtg_id yn = rtg_object_flip_normals(b, rtg_object_rect(b, 1, p0[0], p1[0], p0[2], p1[2], p0[1], m));
  rtg_id xn = rtg_object_flip_normals(b, rtg_object_rect(b, 0, p0[1], p1[1], p0[2], p1[2], p0[0], m));
  return rtg_object_and(b, rtg_object_and(b, zp, rtg_object_and(b, yp, xp)),
                        rtg_object_and(b, zn, rtg_object_and(b, yn, xn)));
}
rtg_id rtg_object_linear_move(rtg_builder* b, rtg_id object, const float motion[3]) {
  if (!motion) return bad("null argument");
  return wrapper(b, HostObject::MOVE, motion, object);
}
rtg_id rtg_object_constant_medium(rtg_builder* b, rtg_id boundary, float density, rtg_id material) {
  HostObject o;
  o.kind = HostObject::MEDIUM;
  o.f[0] = density;
  o.a = boundary;
  o.mat = material;
  return push_object(b, o);
}
rtg_id rtg_object_bvh(rtg_builder* b, const rtg_id* objects, size_t n, float e0, float e1) {
  if (!b || (!objects && n)) return bad("null argument");
  try {
    return b->sb.add_bvh(objects, n, e0, e1);
  } catch (const BuildError& e) {
    fail(e.code, e.msg);
    return RTG_INVALID_ID;
  }
}

rtg_id rtg_object_bvh_sah(rtg_builder* b, const rtg_id* objects, size_t n, float e0, float e1) {
  if (!b || (!objects && n)) return bad("null argument");
  try {
    return b->sb.add_bvh(objects, n, e0, e1, true);
  } catch (const BuildError& e) {
    fail(e.code, e.msg);
    return RTG_INVALID_ID;
  }
}

// ---- camera (camera.rs:18-50; host-side setup, tan from the platform libm) ---------------------
int rtg_camera_look(const float from[3], const float at[3], const float up[3], float fov, float aspect,
                    float aperture, float focus_dist, float e0, float e1, rtg_camera* out) {
  if (!from || !at || !up || !out) return fail(RTG_ERR_INVALID, "null argument");
  auto dot3 = [](const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
  auto unit = [&](float* v) {
    float len = sqrtf(dot3(v, v));
    v[0] = v[0] / len, v[1] = v[1] / len, v[2] = v[2] / len;
  };
  auto cross3 = [](const float* a, const float* b, float* r) {
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = -(a[0] * b[2] - a[2] * b[0]);
    r[2] = a[0] * b[1] - a[1] * b[0];
  };
  float lens_radius = aperture / 2.f;
  float theta = fov * 3.14159265358979323846f / 180.f;
  float half_height = tanf(theta / 2.f);
  float half_width = aspect * half_height;
  float w[3] = {from[0] - at[0], from[1] - at[1], from[2] - at[2]};
  unit(w);
  float u[3], v[3];
  cross3(up, w, u);
  unit(u);
  cross3(w, u, v);
  float hw_fd = half_width * focus_dist, hh_fd = half_height * focus_dist;
  float h2 = (2.f * half_width) * focus_dist, v2 = (2.f * half_height) * focus_dist;
  for (int i = 0; i < 3; i++) {
    out->origin[i] = from[i];
    out->lower_left_corner[i] = ((from[i] - hw_fd * u[i]) - hh_fd * v[i]) - focus_dist * w[i];
    out->horizontal[i] = h2 * u[i];
    out->vertical[i] = v2 * v[i];
    out->u[i] = u[i];
    out->v[i] = v[i];
  }
  out->lens_radius = lens_radius;
  out->exposure_start = e0;
  out->exposure_end = e1;
  return RTG_OK;
}

// ---- scene ---------------------------------------------------------------------------------------
// The record offsets of the pruned image of a lean program (rt_box_plan.h): the plan's records 0 bytes, and the box-chain
// followers too (chains = 1) or not; made once per scene, program and kind.
static int prune_table(rtg_scene* s, LeanImages* im, int chains) {
  if (im->d_prune_off[chains] || !im->n_pruned) return RTG_OK;
  const size_t n = im->plan_mask.size();
  std::vector<uint8_t> drop(n);
  std::vector<uint32_t> off(n);
  for (size_t i = 0; i < n; i++) drop[i] = im->plan_mask[i] == BOX_PRUNED || (chains && im->plan_mask[i] == BOX_FOLLOWER);
  im->prune_bytes[chains] = lds_image_offsets(im->plan_ops.data(), n, off.data(), drop.data());
  return upload(s, &im->d_prune_off[chains], off.data(), n * sizeof(uint32_t));
}

// The full image's offsets, the followers and the image without them of the program (lo, hi), which is on the device already.
static int lean_images(rtg_scene* s, LeanImages* im, const std::vector<Packet>& lo, const std::vector<Packet>& hi) {
  std::vector<uint32_t> off(hi.size());
  im->plan_ops.resize(hi.size());
  for (size_t i = 0; i < hi.size(); i++) im->plan_ops[i] = hi[i].w[3];
  im->bytes = lds_image_offsets(im->plan_ops.data(), hi.size(), off.data());
  int rc = upload(s, &im->d_off, off.data(), off.size() * sizeof(uint32_t));
  if (rc) return rc;
  im->follower.resize(hi.size());
  im->n_followers = box_chain_followers(reinterpret_cast<const uint32_t (*)[4]>(lo.data()), reinterpret_cast<const uint32_t (*)[4]>(hi.data()), hi.size(), im->follower.data());
  if (im->n_followers) {  // the production image: every follower 0 bytes (the counting launches keep the full one)
    im->chain_bytes = lds_image_offsets(im->plan_ops.data(), hi.size(), off.data(), im->follower.data());
    if ((rc = upload(s, &im->d_chain_off, off.data(), off.size() * sizeof(uint32_t)))) return rc;
  }
  return RTG_OK;
}

// The pruning plan of one program and its default table, once.  (Only staged images have pruned records: no plan for a
// program that cannot fit a CU's LDS even without its interior boxes -- rtg_scene::plannable.)
static int lean_plan(rtg_scene* s, LeanImages* im, const std::vector<Packet>& lo, const std::vector<Packet>& hi, BoxPlanKind kind) {
  if (im->planned || !s->plannable) return RTG_OK;
  im->planned = true;
  im->plan_mask.resize(hi.size());
  const auto t0 = std::chrono::steady_clock::now();
  im->n_pruned = box_plan(reinterpret_cast<const uint32_t (*)[4]>(lo.data()), reinterpret_cast<const uint32_t (*)[4]>(hi.data()), hi.size(), im->follower.data(), im->plan_mask.data(), nullptr, BOX_PLAN_PROBES, kind).n_pruned;
  im->plan_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return prune_table(s, im, 1);
}
static int ref_plan(rtg_scene* s) { return lean_plan(s, &s->ref, s->h_lo, s->h_hi, BOX_PLAN_DEFAULT); }

// The rebuilt program (rt_box_plan.h box_tree_rebuild), its images and its plan, once; s->tree.lo stays nullptr when the
// program has no region to rebuild (production launches then stage the reference program whatever option box_tree says).
static int tree_program(rtg_scene* s) {
  if (s->tree_tried || !s->plannable) return RTG_OK;
  s->tree_tried = true;
  const size_t n = s->h_hi.size();
  std::vector<Packet> lo(n), hi(n);
  std::vector<uint32_t> origin(n);
  const auto t0 = std::chrono::steady_clock::now();
  s->n_regions = box_tree_rebuild(reinterpret_cast<const uint32_t (*)[4]>(s->h_lo.data()), reinterpret_cast<const uint32_t (*)[4]>(s->h_hi.data()), n,
                                  reinterpret_cast<uint32_t (*)[4]>(lo.data()), reinterpret_cast<uint32_t (*)[4]>(hi.data()), origin.data());
  s->tree_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (!s->n_regions) return RTG_OK;
  int rc;
  const uint4 *d_lo = nullptr, *d_hi = nullptr;
  if ((rc = upload(s, &d_lo, lo.data(), n * 16)) || (rc = upload(s, &d_hi, hi.data(), n * 16))) return rc;
  if ((rc = lean_images(s, &s->tree, lo, hi)) || (rc = lean_plan(s, &s->tree, lo, hi, BOX_TREE_PLAN))) return rc;
  if (!s->box_chains && (rc = prune_table(s, &s->tree, 0))) return rc;
  s->tree.lo = d_lo, s->tree.hi = d_hi;
  s->t_lo.swap(lo), s->t_hi.swap(hi);
  s->tree.h_lo = &s->t_lo, s->tree.h_hi = &s->t_hi;
  return RTG_OK;
}

void rtg_scene_destroy(rtg_scene* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  for (void* p : s->owned) (void)hipFree(p);
  for (LaunchCtx& c : s->ctx) {
    ctx_free_buffers(&c);
    if (c.d_counters) (void)hipFree(c.d_counters);
    if (c.d_consts) (void)hipFree(c.d_consts);
    if (c.ev0) (void)hipEventDestroy(c.ev0);
    if (c.ev1) (void)hipEventDestroy(c.ev1);
    if (c.done) (void)hipEventDestroy(c.done);
  }
  for (CameraPlan& c : s->cam_plans) {
    if (c.ev) (void)hipEventDestroy(c.ev);
    if (c.d_counts) (void)hipFree(c.d_counts);
    if (c.d_off) (void)hipFree(c.d_off);
    if (c.h_words) (void)hipHostFree(c.h_words);
  }
  for (LeanImages* im : {&s->ref, &s->tree})
    if (im->d_stop) (void)hipFree(im->d_stop);
  for (DevMem* m : {&s->frame, &s->pack, &s->recv}) m->release();
  if (s->post0) (void)hipEventDestroy(s->post0);
  if (s->post1) (void)hipEventDestroy(s->post1);
  for (hipEvent_t ev : {s->pack0, s->pack1, s->unpack0})
    if (ev) (void)hipEventDestroy(ev);
  if (s->own_stream) (void)hipStreamDestroy(s->own_stream);
  delete s;
}

int rtg_scene_create(rtg_builder* b, const rtg_id* world, size_t n, int device, rtg_scene** out) {
  if (!b || !out || (!world && n)) return fail(RTG_ERR_INVALID, "null argument");
  FlatScene fs;
  try {
    b->sb.flatten(world, n, &fs);
  } catch (const BuildError& e) {
    return fail(e.code, e.msg);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(RTG_ERR_DEVICE, "no HIP device: the rtiow hot path has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(RTG_ERR_INVALID, "bad device index");
  HIP_TRY(hipSetDevice(device));
  rtg_scene* s = new rtg_scene();
  s->device = device;
  s->features = fs.features;
  s->n_prog = (uint32_t)fs.lo.size();
  s->n_mat = (uint32_t)fs.mat.size() / 2;
  s->n_tex = fs.n_tex;  // records, not the texels behind them
  for (const HostTexture& t : b->sb.textures) s->tex_kind.push_back((uint8_t)t.kind);
  for (size_t i = 0; i < b->sb.textures.size(); i++) s->tex_child.push_back(b->sb.textures[i].kind == TEX_SURFACE ? b->sb.textures[i].t0 : (uint32_t)i);
  if (fs.features & FEAT_ENVIRONMENT) {  // include/rtiow_gpu_environment.h: the builder's environment at this moment
    const SceneBuilder::Environment& ev = b->sb.environment;
    s->env_bg.mode = BG_TEXTURE;
    for (int c = 0; c < 3; c++) s->env_bg.bottom[c] = ev.scale[c];
    std::memcpy(&s->env_bg.top[0], &ev.texture, sizeof(uint32_t));
    s->env_bg.top[1] = ev.s, s->env_bg.top[2] = ev.c;
  }
  int rc;
  if ((rc = upload(s, &s->dev.lo, fs.lo.data(), fs.lo.size() * 16)) ||
      (rc = upload(s, &s->dev.hi, fs.hi.data(), fs.hi.size() * 16)) ||
      (rc = upload(s, &s->dev.mat, fs.mat.data(), fs.mat.size() * 16)) ||
      (rc = upload(s, &s->dev.tex, fs.tex.data(), fs.tex.size() * 16)) ||
      (rc = upload(s, &s->dev.perlin_vecs, fs.perlin_vecs.data(), sizeof(float) * 1024)) ||
      (rc = upload(s, &s->dev.perlin_perm, fs.perlin_perm.data(), 768))) {
    rtg_scene_destroy(s);
    return rc;
  }
  s->dev.n_prog = s->n_prog;
  s->dev.n_mat = s->n_mat;
  for (const Packet& h : fs.hi) s->n_box += (h.w[3] & 0xffu) == OP_BOX ? 1u : 0u;
  {  // the wrapper around every record (rt_pool_full.h rebuild_hit): PUSH / POP pairs nest in program order, boundary streams included
    std::vector<uint32_t> parent(fs.hi.size(), 0xffffffffu), open;
    for (size_t i = 0; i < fs.hi.size(); i++) {
      const uint32_t op = fs.hi[i].w[3] & 0xffu;
      if (op == OP_POP && !open.empty()) open.pop_back();
      parent[i] = open.empty() ? 0xffffffffu : open.back();
      if (op == OP_PUSH) open.push_back((uint32_t)i);
    }
    if ((rc = upload(s, &s->d_parent, parent.data(), parent.size() * sizeof(uint32_t)))) {
      rtg_scene_destroy(s);
      return rc;
    }
  }
  for (size_t i = 0; i < fs.hi.size(); i++)
    if ((fs.hi[i].w[3] & 0xffu) == OP_SEG) s->seg_first = (uint32_t)i + 1u, s->seg_end = fs.hi[i].w[2];
  if (!fs.hi2.empty()) {  // the second program (pool-2 kernel)
    s->dev2 = s->dev;
    if ((rc = upload(s, &s->dev2.lo, fs.lo2.data(), fs.lo2.size() * 16)) ||
        (rc = upload(s, &s->dev2.hi, fs.hi2.data(), fs.hi2.size() * 16)) ||
        (rc = upload(s, &s->d_p2, &fs.p2, sizeof(P2Table)))) {
      rtg_scene_destroy(s);
      return rc;
    }
    s->dev2.n_prog = s->n_prog2 = (uint32_t)fs.hi2.size();
    s->dev2.lds_off = nullptr, s->dev2.lds_image_bytes = 0;
    for (const Packet& h : fs.hi2) s->n_box2 += (h.w[3] & 0xffu) == OP_BOX ? 1u : 0u;
  }
  if ((fs.features & FEAT_NOT_LEAN) == 0) {  // lean program (BOX / SPHERE / END): layout of its LDS image (rt_pool.h)
    s->ref.lo = s->dev.lo, s->ref.hi = s->dev.hi;
    if ((rc = lean_images(s, &s->ref, fs.lo, fs.hi))) {
      rtg_scene_destroy(s);
      return rc;
    }
    s->dev.lds_off = s->ref.d_off, s->dev.lds_image_bytes = s->ref.bytes;
    // plans and the rebuilt program: for the program production launches stage now; the other one's when option box_tree asks
    s->plannable = s->dev.lds_image_bytes - LDS_BOX_BYTES * (s->n_box / 2u) <= 160u * 1024u;
    if (s->plannable) {
      s->h_lo = fs.lo, s->h_hi = fs.hi;
      s->ref.h_lo = &s->h_lo, s->ref.h_hi = &s->h_hi;
      if ((s->box_tree && (rc = tree_program(s))) || (!s->tree.lo && (rc = ref_plan(s)))) {
        rtg_scene_destroy(s);
        return rc;
      }
    }
    std::vector<uint32_t> wide;
    if (build_wide_image(fs.lo.data(), fs.hi.data(), fs.hi.size(), wide)) {
      if ((rc = upload(s, &s->d_wide, wide.data(), wide.size() * sizeof(uint32_t)))) {
        rtg_scene_destroy(s);
        return rc;
      }
      s->wide_bytes = (uint32_t)(wide.size() * sizeof(uint32_t));
    }
  }
  b->sb.light_table(world, n, &s->h_lights, &s->h_sampled);  // (scene option light_sampling uploads it)
  s->n_lights = (uint32_t)s->h_lights.size();
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) s->num_cus = prop.multiProcessorCount;
  if (s->num_cus <= 0) s->num_cus = 256;
  if ((rc = ctx_acquire(s))) {  // the first launch context now: a scene that cannot allocate it is no scene
    rtg_scene_destroy(s);
    return rc;
  }
  s->next_ctx = 0;
  *out = s;
  return RTG_OK;
}


// Scheduling / measurement switches of ONE scene handle (none of them changes a bit of the result; every setting is
// covered by test_every_kernel_variant_and_schedule_gives_the_same_bits) -- and light_sampling, the one option that changes the
// estimator (include/rtiow_gpu.h).  The library itself reads no environment variable for these: sweep tools and the test-suite
// set them through this call (capi.py forwards RTG_* variables).
int rtg_scene_set_option(rtg_scene* s, const char* name, int value) {
  if (!s || !name) return fail(RTG_ERR_INVALID, "null argument");
  const std::string k(name);
  const uint32_t u = (uint32_t)value;
  if (k == "kernel") s->kernel_version = value;                 // 3 = ray pools (default), 1 = one lane per pixel
  else if (k == "chunks") s->force_chunks = value;              // lean pool kernel: sample chunks per pixel, 0 = one sample per work item
  else if (k == "scratch_mb") s->scratch_limit = value > 0 ? (uint64_t)value << 20 : 0;  // budget of the per-sample colour scratch (0 = half of the free HBM): larger frames render in sample passes
  else if (k == "lpt") s->lpt = value;                          // cost-ordered queue: 0 off, 1 block-major, 2 class-major (default)
  else if (k == "lpt_phase1") s->lpt_phase1 = value;
  else if (k == "lpt_deep") s->lpt_deep = value;
  else if (k == "lpt_shift") s->lpt_shift = std::min(6, std::max(0, value));
  else if (k == "ray_lds") s->ray_lds = value;
  else if (k == "box_chains") {                                 // 0: production launches stage the image with its box-chain followers (A/B switch)
    if (!value) {  // ... and, with box_prune on, without the pruned records only: that table is made now
      HIP_TRY(hipSetDevice(s->device));
      int rc = prune_table(s, &s->ref, 0);
      if (!rc) rc = prune_table(s, &s->tree, 0);
      if (rc) return rc;
    }
    s->box_chains = value;
  }
  else if (k == "box_tree") {                                   // 0: production launches stage the reference program (A/B switch); what the other value needs is made now
    if (value < 0 || value > 1) return fail(RTG_ERR_INVALID, "box_tree: 0 or 1");
    HIP_TRY(hipSetDevice(s->device));
    int rc = value ? tree_program(s) : ref_plan(s);
    if (!rc && !s->box_chains) rc = prune_table(s, value ? &s->tree : &s->ref, 0);
    if (rc) return rc;
    s->box_tree = value;
  }
  else if (k == "box_prune") {                                  // 0: no interior box pruned; 1: production launches; 2: counting launches too (rtg_scene above)
    if (value < 0 || value > 2) return fail(RTG_ERR_INVALID, "box_prune: 0 .. 2");
    s->box_prune = value;
  }
  else if (k == "box_camera") {                                 // camera plan: 0 off, 1 launches that are large enough (default), 2 every launch, planned before it runs
    if (value < 0 || value > 2) return fail(RTG_ERR_INVALID, "box_camera: 0 .. 2");
    s->box_camera = value;
  }
  else if (k == "box_camera_paths" || k == "box_camera_bounces" || k == "box_camera_trips") {
    // measurement switches of the probe (profiles/r24_camera_plan/ sweep.txt, sweep_trips.txt): paths per camera, bounces per path,
    // records a path may visit.  They are not part of a plan's key, so the handle's plans are dropped and made again with the new values.
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());  // (kernels in flight may read a plan's table)
    for (CameraPlan& c : s->cam_plans) c.state = CameraPlan::FREE;
    if (k == "box_camera_paths") s->cam_paths = std::min(1 << 20, std::max(1, value));
    else if (k == "box_camera_bounces") s->cam_bounces = std::min(16, std::max(0, value));
    else s->cam_trips = std::max(1, value);
  }
  else if (k == "bvh4") {
    if (value && !s->wide_bytes) return fail(RTG_ERR_INVALID, "bvh4: the scene is not one Bvh of spheres (no 4-wide image)");
    if (value && pool_lds_bytes(s->wide_bytes, s->n_mat, (uint32_t)(s->pool_threads > 0 ? s->pool_threads : RT_POOL_MAX_THREADS) / 64u, true, false) > 160 * 1024)
      return fail(RTG_ERR_INVALID, "bvh4: the 4-wide image does not fit a CU's 160 KB of LDS (the 4-wide walk only exists LDS-staged)");
    s->bvh4 = value;
  }
  else if (k == "frames_in_flight") {  // launch contexts of this handle: asynchronous rtg_par_cast_device calls overlap up to this many frames
    if (value < 1 || value > RTG_MAX_FRAMES) return fail(RTG_ERR_INVALID, "frames_in_flight: 1 .. 4");
    HIP_TRY(hipSetDevice(s->device));
    for (int i = value; i < RTG_MAX_FRAMES; i++) ctx_free_buffers(&s->ctx[i]);  // contexts that leave the ring: wait for their frame, give the HBM back
    s->n_ctx = value, s->next_ctx = 0;
  }
  else if (k == "force_rccl") s->force_rccl = value;
  else if (k == "multi_gather") s->multi_gather = value;        // rtg_par_cast_multi: the packed collective (1 / n of the bytes per scene) instead of the reduce
  else if (k == "multi_planes") s->multi_planes = value;        // rtg_par_cast_multi: accept the flagged frames (include/rtiow_gpu.h, at rtg_par_cast_multi)
  else if (k == "sync") s->sync_full = value;
  else if (k == "block") {
    if (value < 64 || value > 1024 || value % 64) return fail(RTG_ERR_INVALID, "block: a multiple of 64 in [64, 1024]");
    s->pool_threads = s->full_threads = value;
  }
  else if (k == "wg_per_cu") s->wg_per_cu = value;
  else if (k == "drain_share") s->drain_share = value;
  else if (k == "hoist") s->hoist = value;
  else if (k == "pool2") s->pool2 = value;                      // 0: the first full-feature pool kernel also for programs the pool-2 kernel walks (A/B switch)
  else if (k == "deep_sized") s->deep_sized = value;
  else if (k == "mat_lds") s->mat_lds = value;
  else if (k == "guide_lds") s->guide_lds = value;
  else if (k == "light_sampling") {                             // 1: direct light sampling of the scene's rect lights (rt_light.h): other samples, the same expectation
    if (value < 0 || value > 1) return fail(RTG_ERR_INVALID, "light_sampling: 0 or 1");
    if (value && s->n_lights > RT_MAX_LIGHTS) return fail(RTG_ERR_INVALID, "light_sampling: the scene's light table has " + std::to_string(s->n_lights) + " rects, more than RT_MAX_LIGHTS (64)");
    if (value && s->n_lights != 0u && !s->lights.n) {  // the first time: the table to the device
      HIP_TRY(hipSetDevice(s->device));
      int rc = upload(s, &s->lights.lights, s->h_lights.data(), s->h_lights.size() * sizeof(LightRect));
      if (!rc) rc = upload(s, &s->lights.sampled, s->h_sampled.data(), s->h_sampled.size());
      if (rc) return rc;
      s->lights.n = s->n_lights;
    }
    if (s->verbose) {
      fprintf(stderr, "[rtg] light sampling %s: light table of %u rect(s)\n", value ? "on" : "off", s->n_lights);
      for (const LightRect& l : s->h_lights)
        fprintf(stderr, "[rtg]   light: axis %u k %.9g r0 %.9g %.9g r1 %.9g %.9g area %.9g material %u\n", l.axis, l.k, l.r0s, l.r0e, l.r1s, l.r1e, l.area, l.mat);
      std::string ids;
      for (size_t m = 0; m < s->h_sampled.size(); m++)
        if (s->h_sampled[m]) ids += " " + std::to_string(m);
      fprintf(stderr, "[rtg]   sampled materials:%s\n", ids.c_str());
    }
    s->light_sampling = value;
  }
  else if (k == "query_lds") {                                  // ray queries: 0 the general kernel, 1 automatic (default), 2 the lean kernel whenever the program fits
    if (value < 0 || value > 2) return fail(RTG_ERR_INVALID, "query_lds: 0 .. 2");
    s->query_lds = value;
  }
  else if (k == "query_refill") s->query_refill = std::min(64, std::max(1, value));
  else if (k == "ray_pool") {                                   // ray frames: 1 lean programs on the lean pool kernel (default), 0 always the general kernel
    if (value < 0 || value > 1) return fail(RTG_ERR_INVALID, "ray_pool: 0 or 1");
    s->ray_pool = value;
  }
  else if (k == "small_frames") s->small_frames = value;        // 0: one geometry for every frame size (measurement switch)
  else if (k == "verbose") {                                    // print launch geometry / schedule statistics to stderr
    s->verbose = value;
    if (value && s->env_bg.mode == BG_TEXTURE) {
      uint32_t id;
      std::memcpy(&id, &s->env_bg.top[0], sizeof(id));
      fprintf(stderr, "[rtg] environment: texture %u, scale (%g, %g, %g), (s, c) = (%.9g, %.9g)\n", id, s->env_bg.bottom[0], s->env_bg.bottom[1], s->env_bg.bottom[2],
              s->env_bg.top[1], s->env_bg.top[2]);
    }
  }
  else if (k == "window") s->window = value;                    // full-feature kernel: records staged in LDS, -1 = automatic
  else if (k == "box_leave") s->pool_tune.box_leave = s->full_tune.box_leave = s->sync_tune.box_leave = u;
  else if (k == "refill_min") s->pool_tune.refill_min = s->full_tune.refill_min = s->sync_tune.refill_min = u;
  else if (k == "gather_min") s->pool_tune.gather_min = s->full_tune.gather_min = s->sync_tune.gather_min = u;
  else if (k == "run_ahead") s->pool_tune.run_ahead = s->full_tune.run_ahead = s->sync_tune.run_ahead = u;
  else if (k == "run_ahead_min") s->pool_tune.run_ahead_min = s->full_tune.run_ahead_min = s->sync_tune.run_ahead_min = u;
  else if (k == "sphere_min") s->pool_tune.sphere_min = s->full_tune.sphere_min = s->sync_tune.sphere_min = std::max(1u, u);  // (0 would let no arm run while lanes sit at a BOX; 0 and 1 choose alike otherwise)
  else if (k == "p2_refill") s->pool2_tune.refill_min = u;      // pool-2 kernel's schedule thresholds (rt_pool2.h Pool2Tuning)
  else if (k == "p2_box_leave") s->pool2_tune.box_leave = u;
  else if (k == "p2_park") s->pool2_tune.park_max = u;
  else if (k == "p2_sphere") s->pool2_tune.t_sphere = std::max(1u, u);
  else if (k == "p2_prism") s->pool2_tune.t_prism = std::max(1u, u);
  else if (k == "p2_list") s->pool2_tune.t_list = std::max(1u, u);
  else if (k == "p2_push") s->pool2_tune.t_push = std::max(1u, u);
  else return fail(RTG_ERR_INVALID, "rtg_scene_set_option: unknown option '" + k + "'");
  return RTG_OK;
}

int rtg_scene_info(const rtg_scene* s, uint32_t* n_instructions, uint32_t* n_materials, uint32_t* n_textures,
                   uint64_t* hbm_bytes, uint32_t* n_box_followers) {
  if (!s) return fail(RTG_ERR_INVALID, "null argument");
  if (n_instructions) *n_instructions = s->n_prog;
  if (n_materials) *n_materials = s->n_mat;
  if (n_textures) *n_textures = s->n_tex;
  if (hbm_bytes) *hbm_bytes = s->bytes;
  if (n_box_followers) *n_box_followers = s->ref.n_followers;
  return RTG_OK;
}

// ---- render --------------------------------------------------------------------------------------
static DevCamera to_dev(const rtg_camera* c) {
  DevCamera d;
  auto v = [](const float* p) { return V3{p[0], p[1], p[2]}; };
  d.origin = v(c->origin), d.llc = v(c->lower_left_corner), d.horizontal = v(c->horizontal);
  d.vertical = v(c->vertical), d.u = v(c->u), d.v = v(c->v);
  d.lens_radius = c->lens_radius, d.e0 = c->exposure_start, d.e1 = c->exposure_end;
  return d;
}

static int check_params(const rtg_scene* s, const rtg_camera* camera, const rtg_params* p, DevParams* out) {
  if (!s || !camera || !p) return fail(RTG_ERR_INVALID, "null argument");
  if (p->struct_size != sizeof(rtg_params)) return fail(RTG_ERR_INVALID, "rtg_params.struct_size mismatch");
  if (p->nx == 0 || p->ny == 0 || p->ns == 0) return fail(RTG_ERR_INVALID, "nx, ny, ns must be > 0");
  if ((uint64_t)p->nx * p->ny > 0xffffffffull) return fail(RTG_ERR_INVALID, "image too large for 32-bit pixel index");
  if (!(camera->exposure_start < camera->exposure_end))  // camera.rs:55 / rand assert
    return fail(RTG_ERR_RANGE, "Uniform::sample_single called with low >= high");
  // rand 0.6.5's sample_single panics on non-finite bounds once its scale is not finite ("non-finite boundaries");
  // with scale = inf the retry loop of SampleRng::gen_range would never accept a value (a hung GPU)
  if (!std::isfinite(camera->exposure_start) || !std::isfinite(camera->exposure_end))
    return fail(RTG_ERR_RANGE, "Uniform::sample_single called with non-finite boundaries");
  if (!std::isfinite(camera->exposure_end - camera->exposure_start))  // rand would shrink the scale here; not restated
    return fail(RTG_ERR_RANGE, "exposure range wider than f32::MAX is not supported");
  DevParams d;
  d.nx = p->nx, d.ny = p->ny, d.ns = p->ns, d.max_bounces = p->max_bounces;
  d.t_near = p->t_near;
  d.seed_lo = (uint32_t)p->seed, d.seed_hi = (uint32_t)(p->seed >> 32);
  d.tile_w = p->tile_w ? p->tile_w : 16u;
  d.tile_h = p->tile_h ? p->tile_h : 16u;
  if (d.tile_w % 8u || d.tile_h % 8u) return fail(RTG_ERR_INVALID, "tile_w / tile_h must be multiples of 8");
  d.nranks = p->nranks ? p->nranks : 1u;
  d.rank = p->rank;
  d.bg = s->env_bg;  // the scene's environment, BG_NONE without one (RTG_FLAG_BACKGROUND: the entry points put the block in its place once they have read it)
  if (d.rank >= d.nranks) return fail(RTG_ERR_INVALID, "rank >= nranks");
  if ((p->flags & RTG_FLAG_RESUME) && p->sample_begin > p->ns) return fail(RTG_ERR_INVALID, "RTG_FLAG_RESUME: sample_begin > ns");
  if ((p->flags & RTG_FLAG_RETIRE) && (~p->flags & (RTG_FLAG_SAMPLE_COUNTS | RTG_FLAG_SUM_SQUARES)))
    return fail(RTG_ERR_INVALID, "RTG_FLAG_RETIRE needs RTG_FLAG_SAMPLE_COUNTS | RTG_FLAG_SUM_SQUARES");
  if ((p->flags & RTG_FLAG_DENOISE) && !(p->flags & RTG_FLAG_SUM_SQUARES)) return fail(RTG_ERR_INVALID, "RTG_FLAG_DENOISE needs RTG_FLAG_SUM_SQUARES");
  if ((p->flags & RTG_FLAG_DENOISE_ERROR) && !(p->flags & RTG_FLAG_DENOISE)) return fail(RTG_ERR_INVALID, "RTG_FLAG_DENOISE_ERROR needs RTG_FLAG_DENOISE");
  if ((p->flags & RTG_FLAG_DENOISE) && d.nranks > 1u) return fail(RTG_ERR_INVALID, "RTG_FLAG_DENOISE needs nranks = 1 (the neighbours live on other ranks)");
  *out = d;
  return RTG_OK;
}

// Option verbose, counting builds: the schedule statistics of the frame just rendered (`ms`: its kernel time)
static int print_schedule_stats(rtg_scene* s, float ms) {
  if (s->cx->lpt_desc.n_blocks && s->cx->lpt.p) {  // cost classes of the last frame (class 0 = deepest)
    std::vector<uint32_t> ctl(LPT_CTL);
    HIP_TRY(hipMemcpy(ctl.data(), s->cx->lpt_desc.ctl, LPT_CTL * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::string line;
    for (uint32_t c = 0; c < LPT_CLASSES; c++)
      if (ctl[c]) line += " " + std::to_string(c) + ":" + std::to_string(ctl[c]);
    fprintf(stderr, "[rtg] cost-ordered queue: %u of %u blocks filed, class:blocks%s\n", ctl[LPT_CLASSES], s->cx->lpt_desc.n_blocks, line.c_str());
  }
  unsigned long long q[24];
  HIP_TRY(hipMemcpy(q, s->cx->d_counters + 8, sizeof(q), hipMemcpyDeviceToHost));
  if (q[18]) {  // lean pool kernel: per-wave timeline, scaled so that the longest wave = the measured kernel time
    const double us = (double)ms * 1000. / (double)q[16], n = (double)q[18];
    fprintf(stderr, "[rtg] wave timeline (us from its start): sees the work queue empty at min %.0f / mean %.0f / max %.0f; done at mean %.0f / max %.0f\n",
            (double)((1ull << 62) - q[19]) * us, (double)q[20] / n * us, (double)q[21] * us, (double)q[17] / n * us, (double)q[16] * us);
  }
  double tt = (double)(q[8] + q[9] + q[10] + q[11]);  // (q[9] = service minus shade)
  fprintf(stderr, "[rtg] wave-time shares (s_memtime, instrumented variant): shade %.1f%% gen+pull|service %.1f%% box %.1f%% sphere %.1f%%; "
          "per pass: shade %.0f, gen|service %.0f, box %.0f, sphere %.0f ticks\n", 100 * q[8] / tt, 100 * q[9] / tt, 100 * q[10] / tt,
          100 * q[11] / tt, q[4] ? (double)q[8] / q[4] : 0., q[4] ? (double)q[9] / q[4] : 0., q[0] ? (double)q[10] / q[0] : 0.,
          q[2] ? (double)q[11] / q[2] : 0.);
  if (q[15]) {  // full-feature pool kernel: the steps of a service
    unsigned long long f[2];
    HIP_TRY(hipMemcpy(f, s->cx->d_counters + 5, sizeof(f), hipMemcpyDeviceToHost));
    fprintf(stderr, "[rtg] services %llu: finish step %.1f%% of wave time (%.0f ticks each), refill step %.1f%% (%.0f ticks per refill)\n", f[0],
            100 * f[1] / tt, f[0] ? (double)f[1] / f[0] : 0., 100 * q[15] / tt, q[6] ? (double)q[15] / q[6] : 0.);
  }
#ifdef RT_CENSUS
  {
    unsigned long long c[32];
    HIP_TRY(hipMemcpy(c, s->cx->d_counters + 32, sizeof(c), hipMemcpyDeviceToHost));
    static const char* nm[13] = {"BOX", "END", "no-ray", "held", "?", "?", "SPHERE", "RECT", "PUSH", "POP", "MEDIUM", "PRISM", "BEND"};
    for (int k = 0; k < 2; k++) {
      std::string line;
      char buf[64];
      for (int j = 0; j < 13; j++)
        if (c[16 * k + j]) snprintf(buf, sizeof buf, " %s %.1f", nm[j], (double)c[16 * k + j] / (double)c[16 * k + 15]), line += buf;
      fprintf(stderr, "[rtg] lane census at %s (%llu):%s\n", k ? "slow-pass iterations" : "box steps", c[16 * k + 15], line.c_str());
    }
  }
#endif
  fprintf(stderr, "[rtg] pool schedule: box steps %llu (avg %.1f lanes), sphere passes %llu (avg %.1f lanes), shade passes %llu "
            "(avg %.1f lanes), end / camera-ray passes %llu (avg %.1f lanes), refills %llu (avg %.1f lanes)\n", q[0], q[0] ? (double)q[1] / q[0] : 0.0, q[2],
            q[2] ? (double)q[3] / q[2] : 0.0, q[4], q[4] ? (double)q[5] / q[4] : 0.0, q[12], q[12] ? (double)q[13] / q[12] : 0.0, q[6],
            q[6] && q[7] ? (double)q[7] / q[6] : 0.0);
  return RTG_OK;
}

int rtg_par_cast_device(rtg_scene* s, const rtg_camera* camera, const rtg_params* params, float* d_out,
                        void* hip_stream, rtg_stats* stats) {
  DevParams d;
  int rc = check_params(s, camera, params, &d);
  if (rc) return rc;
  if (!d_out) return fail(RTG_ERR_INVALID, "null output");
  if (stats && stats->struct_size != sizeof(rtg_stats)) return fail(RTG_ERR_INVALID, "rtg_stats.struct_size mismatch");
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t stream = (hipStream_t)hip_stream;
  if ((rc = ctx_acquire(s))) return rc;
  DevCamera cam = to_dev(camera);
  bool count = stats && (params->flags & RTG_FLAG_COUNTERS);
  const SampleSlice sl = slice_of(params);
  const FrameLayout L(d.nx, d.ny, params->flags);
  FrameBlocks fb;
  // From here on work of this frame may sit on `stream`: a failure must not hand the context out again while kernels of the
  // partly enqueued frame still run (they read d_consts / d_lpt / the scratch the next call would rewrite) -- drain first.
#define HIP_TRY_CTX(expr)                               \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) {                             \
      (void)hipStreamSynchronize(stream);               \
      return hip_fail(e_, #expr);                       \
    }                                                   \
  } while (0)
  if ((sl.denoise || sl.features || sl.background) && !sl.counts) {
    // RTG_FLAG_DENOISE / RTG_FLAG_FEATURES / RTG_FLAG_BACKGROUND without a count plane: the blocks' in-fields come back now, in one copy-and-wait, before
    // anything of the frame is enqueued and outside the timed span (a counts call reads them with its compaction result: launch_counts)
    HIP_TRY(read_blocks(L, sl, d_out, stream, &fb));
    HIP_TRY(hipStreamSynchronize(stream));
    if (const char* why = blocks_refusal(sl, fb, d.nranks)) return fail(RTG_ERR_INVALID, why);
    if (sl.background) d.bg = dev_background(fb.background);
  }
  if (count) {
    HIP_TRY_CTX(clear_counters(s->cx, stream));
    HIP_TRY_CTX(hipMemsetAsync(s->cx->d_counters + 32, 0, 32 * sizeof(unsigned long long), stream));  // (RT_CENSUS builds)
  }
#ifdef RT_TIMELINE  // diagnostic build (rt_pool.h RT_TL_*): one 16-dword drain record per wave, dumped to $RTG_TIMELINE_OUT
  static uint32_t* d_tl = nullptr;
  const size_t tl_bytes = (size_t)1024 * 16 * 16 * sizeof(uint32_t);  // <= 1024 workgroups x 16 waves
  if (!count) {
    if (!d_tl) HIP_TRY_CTX(hipMalloc((void**)&d_tl, tl_bytes));
    HIP_TRY_CTX(hipMemsetAsync(d_tl, 0, tl_bytes, stream));
    static unsigned long long tl_ptr;
    tl_ptr = (unsigned long long)(uintptr_t)d_tl;
    HIP_TRY_CTX(hipMemcpyAsync(s->cx->d_counters + 31, &tl_ptr, sizeof(tl_ptr), hipMemcpyHostToDevice, stream));
  }
#endif
  if (stats) HIP_TRY_CTX(hipEventRecord(s->cx->ev0, stream));
  s->cx->refusal = nullptr;
  HIP_TRY_CTX(count ? launch_render<true>(s, cam, d, d_out, stream, sl, L, fb) : launch_render<false>(s, cam, d, d_out, stream, sl, L, fb));
  if ((rc = ctx_release(s, stream))) {
    (void)hipStreamSynchronize(stream);
    return rc;
  }
#undef HIP_TRY_CTX
  if (s->cx->refusal) return fail(RTG_ERR_INVALID, s->cx->refusal);  // (read back on the stream: nothing of the frame was enqueued)
  if (stats) {
    HIP_TRY(hipEventRecord(s->cx->ev1, stream));
    HIP_TRY(hipEventSynchronize(s->cx->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->cx->ev0, s->cx->ev1));
#ifdef RT_TIMELINE
    if (!count && getenv("RTG_TIMELINE_OUT")) {
      std::vector<uint32_t> h_tl(tl_bytes / sizeof(uint32_t));
      HIP_TRY(hipMemcpy(h_tl.data(), d_tl, tl_bytes, hipMemcpyDeviceToHost));
      if (FILE* f = fopen(getenv("RTG_TIMELINE_OUT"), "wb")) {
        fwrite(&ms, sizeof(ms), 1, f);
        fwrite(h_tl.data(), 1, tl_bytes, f);
        fclose(f);
      }
    }
#endif
    stats->kernel_ms = ms;
    stats->samples = sl.counts ? s->cx->counts_samples : owned_pixels(d) * (d.ns - sl.begin);
    unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (count) HIP_TRY(hipMemcpy(h, s->cx->d_counters, sizeof(h), hipMemcpyDeviceToHost));
    stats->aabb_tests = h[0], stats->prim_tests = h[1], stats->shaded_hits = h[2], stats->rays = h[3], stats->draws = h[4];
    if (count && s->verbose && (rc = print_schedule_stats(s, ms))) return rc;
  }
  return RTG_OK;
}

// ---- what rtg_par_cast does around rtg_par_cast_device, shared with rtg_par_cast_multi's flagged frames (rtg_multi.inc) ------
// The host copies of a flagged frame's blocks, checked: the refusals of include/rtiow_gpu.h for a call of `nranks` ranks, made
// before anything is uploaded or enqueued.  (The upload and copy-back extents are rt_multi_planes.h's host part.)
static int check_blocks(const FrameLayout& L, const SampleSlice& sl, const float* out_rgb, uint32_t nranks, FrameBlocks* fb) {
  if (sl.retire) memcpy(&fb->retire, out_rgb + L.retire, sizeof(rtg_retire));
  if (sl.denoise) memcpy(&fb->denoise, out_rgb + L.denoise, sizeof(rtg_denoise));
  if (sl.features) memcpy(&fb->features, out_rgb + L.features, sizeof(rtg_features));
  if (sl.background) memcpy(&fb->background, out_rgb + L.background, sizeof(rtg_background));
  if (const char* why = blocks_refusal(sl, *fb, nranks)) return fail(RTG_ERR_INVALID, why);
  return RTG_OK;
}

int rtg_par_cast(rtg_scene* s, const rtg_camera* camera, const rtg_params* params, float* out_rgb, rtg_stats* stats) {
  if (!s || !params || !out_rgb) return fail(RTG_ERR_INVALID, "null argument");
  {
    DevParams d;  // (refused before anything is uploaded)
    const int rc0 = check_params(s, camera, params, &d);
    if (rc0) return rc0;
  }
  const SampleSlice sl = slice_of(params);
  const FrameLayout L(params->nx, params->ny, params->flags);
  // the blocks' in-fields are checked here, before anything is uploaded
  FrameBlocks fb;
  if (int rc0 = check_blocks(L, sl, out_rgb, params->nranks ? params->nranks : 1u, &fb)) return rc0;
  HIP_TRY(hipSetDevice(s->device));
  // the staging frame lives with the scene handle (no hipMalloc / hipFree per call)
  hipError_t e = s->frame.grow(L.words ? L.words * sizeof(float) : 16);
  if (e != hipSuccess) return hip_fail(e, "hipMalloc(framebuffer)");
  float* d_out = s->frame.as<float>();
  char* dev = reinterpret_cast<char*>(d_out);
  char* host = reinterpret_cast<char*>(out_rgb);
  const Extents up = upload_extents(L, params->nranks > 1, sl.begin, fb.features.compute);
  for (int i = 0; i < up.n && e == hipSuccess; i++) e = hipMemcpy(dev + up.e[i].lo, host + up.e[i].lo, up.e[i].hi - up.e[i].lo, hipMemcpyHostToDevice);
  int rc = (e == hipSuccess) ? rtg_par_cast_device(s, camera, params, d_out, nullptr, stats) : hip_fail(e, "hipMemcpy");
  if (rc == RTG_OK) {
    e = hipDeviceSynchronize();
    const Extents back = copy_back_extents(L, fb.features.compute);
    for (int i = 0; i < back.n && e == hipSuccess; i++) e = hipMemcpy(host + back.e[i].lo, dev + back.e[i].lo, back.e[i].hi - back.e[i].lo, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = hip_fail(e, "render / copy back");
  }
  return rc;
}

#include "rtg_multi.inc"

#include "rtg_probes.inc"

}  // extern "C"

#include "rtg_query.inc"

#include "rtg_rays.inc"

#include "rtg_image.inc"

#include "rtg_mesh.inc"

#include "rtg_surface.inc"

#include "rtg_environment.inc"
