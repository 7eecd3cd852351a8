// rtg_query.inc -- included by rtg_api.hip: the host side of the ray queries (include/rtiow_gpu_query.h; kernels: rt_query.h).
namespace {

// From how many rays scene option query_lds = 1 sends a lean program that fits LDS to the lean kernel: never, as measured.
// Book-1, closest hit, kernel time between device events on one MI355X (tools/query_cost.py; profiles/r25_ray_queries/
// query_cost.txt; the kernel trace of the 960 000-ray sets agrees: kernel_times.txt), general kernel -> lean kernel:
//   1 024 primary rays 0.057 -> 0.067 ms, 16 384: 0.059 -> 0.131, 262 144: 0.059 -> 0.125, 960 000 (1200 x 800): 0.084 -> 0.120
//   (the parent's debug_hit_top_kernel on that set: 0.087 ms, max - min 0.0025);
//   secondary-like rays: 1 024: 0.077 -> 0.103, 65 536: 0.093 -> 0.127, 262 144: 0.121 -> 0.132, 960 000: 0.244 -> 0.201.
// The 47 KB program stays in the caches, neighbouring primary rays walk the same records, and the general kernel's 64-ray
// workgroups balance themselves; a workgroup of the lean kernel first copies the program (36 MB over the grid, more than the
// rays themselves).  There is no crossover on primary rays, so the automatic choice stays on the general kernel; the lean
// kernel is ahead only on large incoherent batches (-17 % at 960 000 secondary rays), which a caller selects with query_lds = 2.
constexpr uint64_t QUERY_LDS_MIN_RAYS = ~0ull;

// Why the params of a query of n rays are refused (nullptr: accepted)
const char* query_refusal(const rtg_query_params* p, size_t n, const rtg_stats* stats) {
  if (p->struct_size != sizeof(rtg_query_params)) return "rtg_query_params.struct_size mismatch";
  if (p->reserved != 0u || p->reserved2 != 0u) return "rtg_query_params: a reserved field is not 0";
  if (p->first_index > (1ull << 32) || (uint64_t)n > (1ull << 32) - p->first_index) return "rtg_query: first_index + n > 2^32 (the RNG index of a ray is 32 bits)";
  if (p->t_min != p->t_min) return "rtg_query_params.t_min is NaN";
  if (stats && stats->struct_size != sizeof(rtg_stats)) return "rtg_stats.struct_size mismatch";
  return nullptr;
}

// Does the lean kernel answer a query of n rays on this scene (option query_lds)?
bool query_takes_lean(const rtg_scene* s, uint64_t n) {
  if (s->query_lds == 0) return false;
  if ((s->features & (FEAT_NOT_LEAN | FEAT_DEEP)) != 0u) return false;  // BOX / SPHERE / END records only
  if (s->n_prog == 0u || s->n_prog > QUERY_LEAN_MAX_RECORDS) return false;          // the reference program + the hand-out counter in 160 KB
  return s->query_lds >= 2 || n >= QUERY_LDS_MIN_RAYS;
}

// Rays per workgroup and grid of the lean kernel: the rays spread over the workgroups the chip holds at once (`per_cu` per CU:
// what the LDS copies and the registers allow, kernel_setup), QUERY_LEAN_MIN_RAYS each at the least.
void query_lean_geometry(const rtg_scene* s, uint64_t n, int per_cu, uint32_t* rays_per_wg, uint32_t* grid) {
  const uint64_t slots = (uint64_t)s->num_cus * (uint64_t)std::max(1, per_cu);
  uint64_t rpw = (n + slots - 1) / slots;
  rpw = std::min<uint64_t>(QUERY_LEAN_MAX_RAYS, std::max<uint64_t>(QUERY_LEAN_MIN_RAYS, rpw));
  *rays_per_wg = (uint32_t)rpw;
  *grid = (uint32_t)((n + rpw - 1) / rpw);
}

// Enqueue one query on `stream`.  ANY = false: closest (d_out8, d_mat); true: any-hit (d_occ).
template <bool ANY>
int query_enqueue(rtg_scene* s, size_t n, const float* d_rays, const rtg_query_params* p, float* d_out8, uint32_t* d_mat, uint8_t* d_occ,
                  hipStream_t stream, rtg_stats* stats) {
  HIP_TRY(hipSetDevice(s->device));
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // (a synchronous call's own pair: the scene handle keeps nothing of a query)
  if (stats) {
    HIP_TRY(hipEventCreate(&ev0));
    hipError_t e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, stream);
    if (e != hipSuccess) {
      (void)hipEventDestroy(ev0);
      if (ev1) (void)hipEventDestroy(ev1);
      return hip_fail(e, "hipEventCreate / hipEventRecord(query)");
    }
  }
  hipError_t e = hipSuccess;
  const uint32_t seed_lo = (uint32_t)p->seed, seed_hi = (uint32_t)(p->seed >> 32), first = (uint32_t)p->first_index;
  if (query_takes_lean(s, n)) {
    const size_t lds = query_lean_lds_bytes(s->n_prog);
    int per_cu = 0;
    e = kernel_setup(s, (const void*)query_lean_kernel<ANY>, (int)QUERY_LEAN_BLOCK, lds, &per_cu);
    if (e == hipSuccess) {
      QueryLean q{s->dev.lo, s->dev.hi, s->n_prog, 0u, (uint64_t)n, d_rays, d_out8, d_mat, d_occ, p->t_min, (uint32_t)s->query_refill};
      uint32_t grid = 0;
      query_lean_geometry(s, n, per_cu, &q.rays_per_wg, &grid);
      if (s->verbose)
        fprintf(stderr, "[rtg] query %s: lean kernel, %u workgroups x %u threads, %u rays each, %zu B of LDS (%u records), %d workgroups per CU, refill at %d lanes\n",
                ANY ? "occluded" : "closest", grid, QUERY_LEAN_BLOCK, q.rays_per_wg, lds, s->n_prog, per_cu, s->query_refill);
      hipLaunchKernelGGL((query_lean_kernel<ANY>), dim3(grid), dim3(QUERY_LEAN_BLOCK), lds, stream, q);
      e = hipGetLastError();
    }
  } else {
    const dim3 grid((uint32_t)(((uint64_t)n + QUERY_GENERAL_BLOCK - 1) / QUERY_GENERAL_BLOCK)), block(QUERY_GENERAL_BLOCK);
    if (s->verbose) fprintf(stderr, "[rtg] query %s: general kernel, %u workgroups x %u threads\n", ANY ? "occluded" : "closest", grid.x, QUERY_GENERAL_BLOCK);
    with_feat<false>(s, [&](auto feat) {
      constexpr uint32_t F = decltype(feat)::value;
      if constexpr (ANY)
        hipLaunchKernelGGL((query_occluded_kernel<F>), grid, block, 0, stream, s->dev, (uint64_t)n, d_rays, seed_lo, seed_hi, first, p->t_min, d_occ);
      else
        hipLaunchKernelGGL((query_closest_kernel<F>), grid, block, 0, stream, s->dev, (uint64_t)n, d_rays, seed_lo, seed_hi, first, p->t_min, d_out8, d_mat);
    });
    e = hipGetLastError();
  }
  if (stats) {
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventRecord(ev1, stream);
    if (e == hipSuccess) e = hipEventSynchronize(ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    if (e == hipSuccess) {
      const uint32_t size = stats->struct_size;
      *stats = rtg_stats{};
      stats->struct_size = size, stats->kernel_ms = ms, stats->rays = n;
    }
  }
  if (e != hipSuccess) return hip_fail(e, "rtg_query: launch");
  return RTG_OK;
}

// The checks every entry point makes before anything is written or enqueued
int query_check(const rtg_scene* s, size_t n, const void* rays, const rtg_query_params* p, const void* out_a, const void* out_b, const rtg_stats* stats) {
  if (!s || !p) return fail(RTG_ERR_INVALID, "null argument");
  if (n && (!rays || !out_a || !out_b)) return fail(RTG_ERR_INVALID, "null argument");
  if (const char* why = query_refusal(p, n, stats)) return fail(RTG_ERR_INVALID, why);
  return RTG_OK;
}

}  // namespace

extern "C" {

int rtg_query_closest_device(rtg_scene* s, size_t n, const float* d_rays7, const rtg_query_params* params, float* d_out8,
                             uint32_t* d_out_material, void* hip_stream, rtg_stats* stats) {
  if (int rc = query_check(s, n, d_rays7, params, d_out8, d_out_material, stats)) return rc;
  if (!n) return RTG_OK;
  return query_enqueue<false>(s, n, d_rays7, params, d_out8, d_out_material, nullptr, (hipStream_t)hip_stream, stats);
}

int rtg_query_occluded_device(rtg_scene* s, size_t n, const float* d_rays8, const rtg_query_params* params, uint8_t* d_out,
                              void* hip_stream, rtg_stats* stats) {
  if (int rc = query_check(s, n, d_rays8, params, d_out, d_out, stats)) return rc;
  if (!n) return RTG_OK;
  return query_enqueue<true>(s, n, d_rays8, params, nullptr, nullptr, d_out, (hipStream_t)hip_stream, stats);
}

int rtg_query_closest(rtg_scene* s, size_t n, const float* rays7, const rtg_query_params* params, float* out8, uint32_t* out_material,
                      rtg_stats* stats) {
  if (int rc = query_check(s, n, rays7, params, out8, out_material, stats)) return rc;
  if (!n) return RTG_OK;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<float> d_rays, d_out;
  DevBuf<uint32_t> d_mat;
  HIP_TRY(d_rays.alloc(7 * n));
  HIP_TRY(d_out.alloc(8 * n));
  HIP_TRY(d_mat.alloc(n));
  HIP_TRY(hipMemcpy(d_rays.p, rays7, 7 * n * sizeof(float), hipMemcpyHostToDevice));
  if (int rc = query_enqueue<false>(s, n, d_rays.p, params, d_out.p, d_mat.p, nullptr, nullptr, stats)) return rc;
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(out8, d_out.p, 8 * n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_material, d_mat.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTG_OK;
}

int rtg_query_occluded(rtg_scene* s, size_t n, const float* rays8, const rtg_query_params* params, uint8_t* out, rtg_stats* stats) {
  if (int rc = query_check(s, n, rays8, params, out, out, stats)) return rc;
  if (!n) return RTG_OK;
  HIP_TRY(hipSetDevice(s->device));
  DevBuf<float> d_rays;
  DevBuf<uint8_t> d_out;
  HIP_TRY(d_rays.alloc(8 * n));
  HIP_TRY(d_out.alloc(n));
  HIP_TRY(hipMemcpy(d_rays.p, rays8, 8 * n * sizeof(float), hipMemcpyHostToDevice));
  if (int rc = query_enqueue<true>(s, n, d_rays.p, params, nullptr, nullptr, d_out.p, nullptr, stats)) return rc;
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(out, d_out.p, n, hipMemcpyDeviceToHost));
  return RTG_OK;
}

}  // extern "C"
