// rtg_kernels.inc -- included by rtg_api.hip: the baseline kernel (one lane per pixel) and the small kernels of the probes / output stage.
// ===================================================================================================
// Kernels
// ===================================================================================================
constexpr uint32_t FEAT_ALL = FEAT_XFORM | FEAT_MEDIUM | FEAT_RECT | FEAT_TEXTURE;
// a program with none of these bits is lean (BOX / SPHERE / END records only)
constexpr uint32_t FEAT_NOT_LEAN = FEAT_ALL | FEAT_BOUNDARY | FEAT_TRI;  // (FEAT_SURFACE never comes without FEAT_TRI)

__device__ __forceinline__ void flush_counts(const Counts& c, uint32_t draws, unsigned long long* g) {
  // one atomic per counter per wave would be nicer; the instrumented variant is not the timed one
  atomicAdd(&g[0], (unsigned long long)c.aabb);
  atomicAdd(&g[1], (unsigned long long)c.prim);
  atomicAdd(&g[2], (unsigned long long)c.shaded);
  atomicAdd(&g[3], (unsigned long long)c.rays);
  atomicAdd(&g[4], (unsigned long long)draws);
}

// par_cast (lib.rs:363-376): one lane owns one pixel and folds its ns samples IN ORDER
// (iter::Sum is a left fold from (0,0,0), vec3.rs:195-203), then divides by ns.
// Block = 16x16 pixels, each wave an 8x8 sub-tile (primary rays of a wave stay coherent).
// SLICE (render_slice_kernel only, include/rtiow_gpu.h progressive rendering): the fold starts at sample s_begin from the
// running sum `out` holds (+0 when s_begin = 0) and divides only when `divide` -- the plain instantiations do not see it.
// SQ (render_squares_kernel only, RTG_FLAG_SUM_SQUARES): a second fold of the squared colours into plane 1 (out + 3 nx ny),
// continued like the first and never divided.
template <uint32_t FEAT, bool COUNT, bool SLICE, bool SQ = false>
__device__ __forceinline__ void render_pixel(const DevScene& sc, const DevCamera& cam, const DevParams& P, float* out,
                                             unsigned long long* counters, uint32_t s_begin, bool divide) {
  const uint32_t nbx = (P.nx + 15u) / 16u;
  const uint32_t bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const uint32_t tiles_x = (P.nx + P.tile_w - 1u) / P.tile_w;
  const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63u;
  const uint32_t x0 = bx * 16u + (w & 1u) * 8u, row0 = by * 16u + (w >> 1) * 8u;  // this wave's 8x8 block: inside ONE tile (tile sizes are multiples of 8)
  const uint32_t tile = (row0 / P.tile_h) * tiles_x + x0 / P.tile_w;
  if (tile % P.nranks != P.rank) return;
  const uint32_t x = x0 + (l & 7u);
  const uint32_t row = row0 + (l >> 3);
  if (x >= P.nx || row >= P.ny) return;
  const uint32_t y = P.ny - 1u - row;  // lib.rs:328: row 0 is y = ny-1
  Counts cnt = {0, 0, 0, 0};
  uint32_t total_draws = 0;
  V3 col = mk(0.f, 0.f, 0.f), sq = mk(0.f, 0.f, 0.f);
  uint32_t s0 = 0;
  if (SLICE && s_begin != 0u) {
    const float* i = out + 3ull * ((size_t)row * P.nx + x);
    col = mk(i[0], i[1], i[2]), s0 = s_begin;
    if (SQ) i += 3ull * ((size_t)P.nx * P.ny), sq = mk(i[0], i[1], i[2]);
  }
  for (uint32_t s = s0; s < P.ns; s++) {
    uint32_t bounces, draws;
    V3 c = sample_color<FEAT, COUNT>(sc, cam, P, x, y, s, cnt, bounces, draws);
    col = vadd(col, c);
    if (SQ) sq = vadd(sq, vmul(c, c));
    if (COUNT) total_draws += draws;
  }
  if (!SLICE || divide) col = sdiv(col, (float)P.ns);  // lib.rs:374
  float* o = out + 3ull * ((size_t)row * P.nx + x);
  o[0] = col.x, o[1] = col.y, o[2] = col.z;
  if (SQ) o += 3ull * ((size_t)P.nx * P.ny), o[0] = sq.x, o[1] = sq.y, o[2] = sq.z;
  if (COUNT) flush_counts(cnt, total_draws, counters);
}

template <uint32_t FEAT, bool COUNT>
__global__ __launch_bounds__(256) void render_kernel(DevScene sc, DevCamera cam, DevParams P, float* out,
                                                     unsigned long long* counters) {
  render_pixel<FEAT, COUNT, false>(sc, cam, P, out, counters, 0u, true);
}

// the same for a slice of a progressive frame: samples [s_begin, P.ns), `divide` = 0 under RTG_FLAG_PARTIAL
template <uint32_t FEAT, bool COUNT>
__global__ __launch_bounds__(256) void render_slice_kernel(DevScene sc, DevCamera cam, DevParams P, float* out,
                                                           unsigned long long* counters, uint32_t s_begin, uint32_t divide) {
  render_pixel<FEAT, COUNT, true>(sc, cam, P, out, counters, s_begin, divide != 0u);
}

// RTG_FLAG_SUM_SQUARES: whole frames and slices alike (s_begin = 0, divide = 1: a whole frame), plane 1 beside the sum
template <uint32_t FEAT, bool COUNT>
__global__ __launch_bounds__(256) void render_squares_kernel(DevScene sc, DevCamera cam, DevParams P, float* out,
                                                             unsigned long long* counters, uint32_t s_begin, uint32_t divide) {
  render_pixel<FEAT, COUNT, true, true>(sc, cam, P, out, counters, s_begin, divide != 0u);
}

// RTG_FLAG_SAMPLE_COUNTS (with or without RTG_FLAG_SUM_SQUARES: SQ): the pixel's samples [s_begin, e_p), e_p = min(n_p, ns)
// with n_p from the count plane, continuing the running sums and never dividing (the launcher's resolve divides by e_p); a
// pixel with e_p <= s_begin is left alone.  Pixel mapping, fold and counters as render_pixel.
template <uint32_t FEAT, bool COUNT, bool SQ>
__global__ __launch_bounds__(256) void render_counts_kernel(DevScene sc, DevCamera cam, DevParams P, float* out,
                                                            unsigned long long* counters, uint32_t s_begin, const uint32_t* counts) {
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
  const uint32_t n = counts[(size_t)row * P.nx + x], s_end = n < P.ns ? n : P.ns;
  if (s_end <= s_begin) return;
  Counts cnt = {0, 0, 0, 0};
  uint32_t total_draws = 0;
  float* o = out + 3ull * ((size_t)row * P.nx + x);
  float* q = o + 3ull * ((size_t)P.nx * P.ny);
  V3 col = mk(0.f, 0.f, 0.f), sq = mk(0.f, 0.f, 0.f);
  if (s_begin != 0u) {
    col = mk(o[0], o[1], o[2]);
    if (SQ) sq = mk(q[0], q[1], q[2]);
  }
  for (uint32_t s = s_begin; s < s_end; s++) {
    uint32_t bounces, draws;
    V3 c = sample_color<FEAT, COUNT>(sc, cam, P, x, y, s, cnt, bounces, draws);
    col = vadd(col, c);
    if (SQ) sq = vadd(sq, vmul(c, c));
    if (COUNT) total_draws += draws;
  }
  o[0] = col.x, o[1] = col.y, o[2] = col.z;
  if (SQ) q[0] = sq.x, q[1] = sq.y, q[2] = sq.z;
  if (COUNT) flush_counts(cnt, total_draws, counters);
}

// Scene option light_sampling (rt_light.h): the kernels above over color_ls, for scenes whose light table is not empty -- the
// same pixel mapping, the same ordered folds.  One body: a whole frame is s_begin = 0, divide = 1; SQ as render_squares_kernel;
// CNT as render_counts_kernel (the pixel's samples [s_begin, min(n_p, ns)), never divided).
template <uint32_t FEAT, bool COUNT, bool SQ, bool CNT>
__global__ __launch_bounds__(256) void render_light_kernel(DevScene sc, LightTable lt, DevCamera cam, DevParams P, float* out,
                                                           unsigned long long* counters, uint32_t s_begin, uint32_t divide, const uint32_t* counts) {
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
  uint32_t s_end = P.ns;
  if (CNT) {
    const uint32_t n = counts[(size_t)row * P.nx + x];
    s_end = n < P.ns ? n : P.ns;
    if (s_end <= s_begin) return;
  }
  Counts cnt = {0, 0, 0, 0};
  uint32_t total_draws = 0;
  float* o = out + 3ull * ((size_t)row * P.nx + x);
  float* q = o + 3ull * ((size_t)P.nx * P.ny);
  V3 col = mk(0.f, 0.f, 0.f), sq = mk(0.f, 0.f, 0.f);
  if (s_begin != 0u) {
    col = mk(o[0], o[1], o[2]);
    if (SQ) sq = mk(q[0], q[1], q[2]);
  }
  for (uint32_t s = s_begin; s < s_end; s++) {
    uint32_t bounces, draws;
    V3 c = sample_color_ls<FEAT, COUNT>(sc, lt, cam, P, x, y, s, cnt, bounces, draws);
    col = vadd(col, c);
    if (SQ) sq = vadd(sq, vmul(c, c));
    if (COUNT) total_draws += draws;
  }
  if (!CNT && divide) col = sdiv(col, (float)P.ns);  // lib.rs:374
  o[0] = col.x, o[1] = col.y, o[2] = col.z;
  if (SQ) q[0] = sq.x, q[1] = sq.y, q[2] = sq.z;
  if (COUNT) flush_counts(cnt, total_draws, counters);
}

template <uint32_t FEAT>
__global__ void debug_samples_light_kernel(DevScene sc, LightTable lt, DevCamera cam, DevParams P, uint32_t n, const uint32_t* xs,
                                           const uint32_t* ys, const uint32_t* ss, float* out_rgb, uint32_t* out_info) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Counts cnt = {0, 0, 0, 0};
  uint32_t bounces = 0, draws = 0;
  V3 c = sample_color_ls<FEAT, true>(sc, lt, cam, P, xs[i], ys[i], ss[i], cnt, bounces, draws);
  out_rgb[3 * i] = c.x, out_rgb[3 * i + 1] = c.y, out_rgb[3 * i + 2] = c.z;
  out_info[4 * i] = bounces, out_info[4 * i + 1] = draws, out_info[4 * i + 2] = cnt.aabb, out_info[4 * i + 3] = cnt.prim;
}

template <uint32_t FEAT>
__global__ void debug_hit_top_kernel(DevScene sc, uint32_t n, const float* rays, uint32_t seed_lo, uint32_t seed_hi,
                                     float t_near, float* out, uint32_t* out_mat) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 7ull * i;
  SampleRng rng;
  rng.init(((uint64_t)seed_hi << 32) | seed_lo, i, 0);
  rng.set_event(1);
  HitRecOf<FEAT> h;
  Counts cnt = {0, 0, 0, 0};
  bool hit = hit_top<FEAT, false>(sc, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], t_near, rng, h, cnt);
  float* o = out + 8ull * i;
  o[0] = hit ? 1.f : 0.f;
  o[1] = hit ? h.t : 0.f;
  o[2] = hit ? h.p.x : 0.f, o[3] = hit ? h.p.y : 0.f, o[4] = hit ? h.p.z : 0.f;
  o[5] = hit ? h.n.x : 0.f, o[6] = hit ? h.n.y : 0.f, o[7] = hit ? h.n.z : 0.f;
  out_mat[i] = hit ? h.mat : 0xffffffffu;
}

// rtg_debug_hit_surface (include/rtiow_gpu_surface.h): the same with (tu, tv) behind the normal.  Only the FEAT_SURFACE
// instantiations carry them; every other program answers (0, 0), as the definition says of a world without attribute triangles.
template <uint32_t FEAT>
__global__ void debug_hit_surface_kernel(DevScene sc, uint32_t n, const float* rays, uint32_t seed_lo, uint32_t seed_hi, float t_near, float* out,
                                         uint32_t* out_mat) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 7ull * i;
  SampleRng rng;
  rng.init(((uint64_t)seed_hi << 32) | seed_lo, i, 0);
  rng.set_event(1);
  HitRecS h;
  h.tu = 0.f, h.tv = 0.f;
  Counts cnt = {0, 0, 0, 0};
  bool hit = hit_top<FEAT, false>(sc, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), r[6], t_near, rng, h, cnt);
  float* o = out + 10ull * i;
  o[0] = hit ? 1.f : 0.f;
  o[1] = hit ? h.t : 0.f;
  o[2] = hit ? h.p.x : 0.f, o[3] = hit ? h.p.y : 0.f, o[4] = hit ? h.p.z : 0.f;
  o[5] = hit ? h.n.x : 0.f, o[6] = hit ? h.n.y : 0.f, o[7] = hit ? h.n.z : 0.f;
  o[8] = hit ? h.tu : 0.f, o[9] = hit ? h.tv : 0.f;
  out_mat[i] = hit ? h.mat : 0xffffffffu;
}

template <uint32_t FEAT>
__global__ void debug_samples_kernel(DevScene sc, DevCamera cam, DevParams P, uint32_t n, const uint32_t* xs,
                                     const uint32_t* ys, const uint32_t* ss, float* out_rgb, uint32_t* out_info) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Counts cnt = {0, 0, 0, 0};
  uint32_t bounces = 0, draws = 0;
  V3 c = sample_color<FEAT, true>(sc, cam, P, xs[i], ys[i], ss[i], cnt, bounces, draws);
  out_rgb[3 * i] = c.x, out_rgb[3 * i + 1] = c.y, out_rgb[3 * i + 2] = c.z;
  out_info[4 * i] = bounces, out_info[4 * i + 1] = draws, out_info[4 * i + 2] = cnt.aabb, out_info[4 * i + 3] = cnt.prim;
}

// print_ppm's to_u8 (lib.rs:348-352): sqrt, * 255.99, `as i32` (saturating, NaN -> 0), clamp 0..=255
__global__ void tonemap_kernel(size_t n, const float* __restrict__ rgb, uint8_t* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = 255.99f * __builtin_sqrtf(rgb[i]);
  int32_t q = f32_as_i32(v);
  out[i] = (uint8_t)(q < 0 ? 0 : (q > 255 ? 255 : q));
}

__global__ void debug_math_kernel(int op, size_t n, const float* in, const float* in2, float* out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x = in[i];
  float r;
  switch (op) {
    case 0: r = rt_logf(x); break;
    case 1: r = rt_pow5f(x); break;
    case 2: r = rt_sinf(x); break;
    case 3: r = __builtin_sqrtf(x); break;
    case 4: r = 1.f / x; break;
    case 6: r = rt_atan2f(x, in2[i]); break;
    default: r = x / in2[i]; break;
  }
  out[i] = r;
}

