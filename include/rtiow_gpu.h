/*
 * rtiow_gpu.h -- C ABI of the MI355X-native path-tracing hot path (librtiow_gpu.so).
 *
 * Drop-in boundary for cbiffle/rtiow-rust's `par_cast(nx, ny, ns, &camera, world)` seam
 * (reference src/lib.rs:363) and everything below it: World::hit_top (lib.rs:23-55), color()
 * (lib.rs:60-101), Bvh/Aabb traversal (bvh.rs:84-120, aabb.rs:16-27), Object::hit for
 * Sphere/Rect/FlipNormals/Translate/Scale/RotateY/And/LinearMove/ConstantMedium (object.rs),
 * Material::{scatter,emitted} (material.rs:55-128), Texture (texture.rs), Perlin (perlin.rs),
 * Camera::get_ray (camera.rs:52-63).
 *
 * The reference has no FFI (`#![forbid(unsafe_code)]`, lib.rs:1).  A Rust `-sys` binding would walk
 * its own object graph and mirror each constructor through the builder calls below (one call per
 * reference constructor -- see INTEGRATION.md), then call rtg_par_cast where it called par_cast.
 *
 * Conventions: plain pointers and sizes only; return 0 = ok, negative = error (never throws or
 * aborts across the boundary); rtg_last_error() gives the message for the calling thread.  Handles
 * (rtg_id) are indices local to one builder.  A scene is bound to one device and may be used from
 * one thread at a time; different scenes are independent.
 */
#ifndef RTIOW_GPU_H
#define RTIOW_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTG_OK 0
#define RTG_ERR_INVALID (-1)     /* bad argument / handle (reference: type error at compile time)   */
#define RTG_ERR_EMPTY_BVH (-2)   /* bvh.rs:60 panic "Can't create a BVH from zero objects."          */
#define RTG_ERR_NAN (-3)         /* bvh.rs:45,56 partial_cmp().unwrap() panic on NaN extents          */
#define RTG_ERR_RANGE (-4)       /* camera.rs:55 gen_range(lo,hi) asserts lo < hi                     */
#define RTG_ERR_UNSUPPORTED (-5) /* nesting beyond the general walk's stacks (32 wrappers, 3 media levels) */
#define RTG_ERR_DEVICE (-6)      /* HIP runtime error / no GPU                                         */

typedef uint32_t rtg_id;
#define RTG_INVALID_ID 0xffffffffu

typedef struct rtg_builder rtg_builder; /* a scene under construction (host only)              */
typedef struct rtg_scene rtg_scene;     /* a flattened scene resident in one GPU's HBM         */

/* camera.rs:6-15 `struct Camera` -- 21 floats, plain data. */
typedef struct rtg_camera {
  float origin[3];
  float lower_left_corner[3];
  float horizontal[3];
  float vertical[3];
  float u[3];
  float v[3];
  float lens_radius;
  float exposure_start, exposure_end;
} rtg_camera;

/* Arguments of par_cast (lib.rs:363) plus the constants the reference bakes in. */
typedef struct rtg_params {
  uint32_t struct_size; /* = sizeof(rtg_params)                                               */
  uint32_t nx, ny, ns;  /* lib.rs:363                                                         */
  uint32_t max_bounces; /* literal 50 at lib.rs:93                                            */
  float t_near;         /* NEAR = 0.001 at lib.rs:35,53                                       */
  uint64_t seed;        /* key of the per-(pixel,sample) counter RNG (DESIGN.md determinism)  */
  /* Pixel sharding for multi-GPU (one process per GPU): the image is cut into tile_w x tile_h
   * tiles numbered row-major from the top-left; this call renders tiles with
   * tile_index % nranks == rank and leaves every other pixel of `out` untouched. */
  uint32_t tile_w, tile_h; /* multiples of 8; 0 -> 16                                         */
  uint32_t rank, nranks;   /* nranks 0 -> 1                                                   */
  uint32_t flags;          /* RTG_FLAG_*                                                      */
  uint32_t sample_begin;   /* RTG_FLAG_RESUME: first sample this call renders (ignored without)  */
} rtg_params;

#define RTG_FLAG_COUNTERS 1u /* fill rtg_stats counters (instrumented kernel variant, slower) */
#define RTG_FLAG_TRACE_KERNEL 2u /* rtg_debug_samples: trace the production ray-pool kernel instead of the one-lane probe */
#define RTG_FLAG_PARTIAL 4u /* leave the UNNORMALISED running sum of the samples in out (skip lib.rs:374's division)  */
#define RTG_FLAG_RESUME 8u  /* out holds the running sum of samples [0, sample_begin): render [sample_begin, ns) only */

/* Progressive rendering (a frame in sample slices).  The RNG is keyed by (seed, pixel, sample index), so the first n
 * samples of an ns-spp frame are exactly the samples of an n-spp frame, and the per-pixel sum is the reference's left fold
 * (lib.rs:365-374).  RTG_FLAG_PARTIAL ends a call without dividing: `out` keeps the f32 running sum of the samples rendered
 * so far.  RTG_FLAG_RESUME continues that fold: `out` holds the running sum of samples [0, sample_begin) of every pixel the
 * call renders (as a PARTIAL call left it), and the call adds samples [sample_begin, ns) to it in order.
 *   - RESUME without PARTIAL divides by ns at the end: the frame is finished, bit-identical to one call with that ns.
 *   - sample_begin == ns renders nothing; without PARTIAL the call only divides (the resolve step: run it on a copy of
 *     the running sum for a preview that is bit-identical to par_cast(ns = sample_begin)).
 *   - sample_begin > ns: RTG_ERR_INVALID, nothing written or enqueued.  sample_begin == 0: as if RESUME were not set.
 *   - Pixels of other ranks / tiles stay untouched, as without the flags.  rtg_stats.samples counts owned pixels x
 *     (ns - sample_begin); every counter summed over the slices of a frame equals the one-call counter.
 * The slices of one frame must agree on camera, nx / ny, seed, max_bounces, t_near and the tiling (tile_w / tile_h, rank /
 * nranks); the library cannot check this.  rtg_par_cast, rtg_par_cast_device and rtg_par_cast_multi honour both flags;
 * rtg_debug_samples rejects them (RTG_ERR_INVALID). */

#define RTG_FLAG_SUM_SQUARES 16u /* out holds a second plane: the running sum of the squared sample colours (below) */

/* Per-pixel noise estimates.  With RTG_FLAG_SUM_SQUARES `out` holds two planes of nx * ny * 3 floats each (2 * nx * ny * 3 in
 * all).  Plane 0 is exactly what the call writes without the flag.  Plane 1 starts at out + 3 * nx * ny, has the same pixel
 * layout, and holds per pixel and channel the f32 left fold q = q + (c * c) over the samples c in order, from +0: the product
 * is rounded before the add (no fused multiply-add).  (sum, sum of squares, n) give each pixel's sample variance and the
 * standard error of its mean (rtiow-rust_amd/noise.py).
 *   - Plane 1 is never divided, with or without RTG_FLAG_PARTIAL.
 *   - RTG_FLAG_RESUME: plane 1 holds the sum over samples [0, sample_begin) and the call continues it.  The resolve call
 *     (sample_begin == ns, no PARTIAL) divides plane 0 and leaves plane 1 bit for bit as it was.
 *   - Pixels of other ranks / tiles stay untouched in both planes.
 *   - rtg_par_cast and rtg_par_cast_device honour the flag; rtg_par_cast_multi returns RTG_ERR_UNSUPPORTED and writes and
 *     enqueues nothing; rtg_debug_samples returns RTG_ERR_INVALID.
 *   - The lean ray-pool kernel then always parks every sample colour in its scratch for the fold, one sample per work item:
 *     scene option "chunks" is overridden for the call.  rtg_stats and its counters are those of the call without the flag. */

#define RTG_FLAG_SAMPLE_COUNTS 32u /* out ends with a count plane: every pixel's own sample count n_p (below) */

/* Per-pixel sample counts (adaptive sampling).  With RTG_FLAG_SAMPLE_COUNTS `out` ends with a count plane of nx * ny uint32_t
 * words in pixel order (row 0 = top): it starts right after the float planes, at word 3 * nx * ny without
 * RTG_FLAG_SUM_SQUARES and at word 6 * nx * ny with it.  Its value n_p is pixel p's target count; let e_p = min(n_p, ns).  The
 * library only reads the count plane, never writes it (RTG_FLAG_RETIRE, below, is the one exception).
 *   - Precondition: the running sum of p holds samples [0, min(e_p, sample_begin)) (sample_begin = 0 without RTG_FLAG_RESUME).
 *   - The call renders samples [sample_begin, e_p) of p and continues the left fold in order (both planes under
 *     RTG_FLAG_SUM_SQUARES).  Pixels with e_p <= sample_begin get no samples.
 *   - Without RTG_FLAG_PARTIAL the call finishes the frame: every owned pixel with e_p > 0 ends as its sum divided by e_p,
 *     including pixels this call rendered nothing for.  The resolve-only call (sample_begin == ns) divides every pixel by its
 *     own e_p.  Plane 1 is never divided.
 *   - Pixels with n_p == 0, and pixels of other ranks / tiles, are left untouched in every plane.
 *   - Parity: a pixel whose sum holds e_p samples resolves bit for bit to par_cast(ns = e_p) at that pixel, and its plane 1 is
 *     bit for bit the RTG_FLAG_SUM_SQUARES call's.  With n_p == ns everywhere the call is bit-identical to the same call
 *     without the flag, in both planes.
 *   - rtg_stats.samples is the number of (pixel, sample) pairs rendered: the sum over owned pixels of max(0, e_p -
 *     sample_begin); every counter is the sum over exactly those pairs, and kernel_ms covers the call's kernels.  (Scene
 *     option bvh4 is not honoured by a counts call: it takes the binary walk, whose counters differ from the 4-wide walk's.)
 *   - rtg_par_cast and rtg_par_cast_device honour the flag.  rtg_par_cast_device synchronises `hip_stream` once during the
 *     call, to read back how many pixels are active (the ray-pool kernels run over a compacted list of them).
 *     rtg_par_cast_multi returns RTG_ERR_UNSUPPORTED and writes and enqueues nothing; rtg_debug_samples returns
 *     RTG_ERR_INVALID. */

#define RTG_FLAG_RETIRE 64u /* after the slice, retire converged pixels: n_p := ns in the count plane (below) */
#define RTG_RETIRE_MAX_RADIUS 8u

/* Adaptive sampling in the library.  RTG_FLAG_RETIRE needs RTG_FLAG_SAMPLE_COUNTS | RTG_FLAG_SUM_SQUARES (else RTG_ERR_INVALID,
 * nothing written or enqueued).  `out` then ends with a 64-byte retire block (rtg_retire) behind the count plane, at word
 * 7 * nx * ny rounded up to an even word (8-byte aligned; compute the offset in 64 bits).  Let k = ns of the call and, for a
 * pixel q, e_q = min(n_q, k).  Its standard errors se_q,c (c = the 3 channels) are computed in float64 from the running sums
 * (S, Q) and e_q, in this order and without contraction:  m = S / e;  v = (Q - (e * m) * m) / (e - 1);  v = 0 where v <= 0 (NaN
 * stays NaN);  se = sqrt(v / e);  se = +inf when e_q < 2 -- rtiow-rust_amd/noise.py standard_error_counts, bit for bit.  q is
 * OK when e_q >= 2 and all three se_q,c <= target_se (NaN is never OK).  Pixel p RETIRES when it is owned, n_p > k,
 * k >= min_samples, and every pixel q with n_q > 0 of the (2 radius + 1)^2 window around p (clipped to the image) is OK --
 * pixels with n_q == 0 are not part of the frame and are ignored.  A retiring pixel gets n_p := k: the only write the library
 * ever makes to the count plane.  radius = 0 is noise.retire's rule.
 *   - Order: the call renders its slice, applies the rule to the undivided running sums, then divides (without
 *     RTG_FLAG_PARTIAL; the division uses e_p, which retiring does not change).  sample_begin == ns with RTG_FLAG_PARTIAL
 *     renders nothing and only applies the rule (re-deciding with another target, say).
 *   - RTG_ERR_INVALID, nothing written: radius > RTG_RETIRE_MAX_RADIUS, a NaN or negative target_se, radius > 0 with
 *     nranks > 1 (the neighbours live on other ranks).  With radius = 0 each rank decides for its own pixels.
 *   - Every accepted call writes every out-field of the block, a rank that owns no tile included (zeros); it never writes the
 *     in-fields or reserved2.  The integer fields are exact; sum_se2 is summed in a fixed order (the same inputs give the same
 *     bits, whichever entry point and however the kernels are scheduled).
 *   - rtg_par_cast uploads the block with the planes and copies back the planes, the count plane and the block's out-fields.
 *     rtg_par_cast_device reads the in-fields back on `hip_stream` together with the compaction's result -- still one
 *     synchronisation of the stream per call (the render-less call syncs for the in-fields alone).
 *   - rtg_stats as without the flag; kernel_ms also covers the retire kernels.  rtg_par_cast_multi returns
 *     RTG_ERR_UNSUPPORTED and rtg_debug_samples RTG_ERR_INVALID. */
typedef struct rtg_retire {
  double target_se;      /* in:  the largest standard error of a converged pixel's channel                       */
  uint32_t min_samples;  /* in:  no pixel retires before k >= min_samples                                         */
  uint32_t radius;       /* in:  0 .. RTG_RETIRE_MAX_RADIUS: the window every pixel of which must be OK          */
  uint32_t active;       /* out: owned pixels with n_p > k after the call                                         */
  uint32_t retired;      /* out: owned pixels whose n_p this call set to k                                        */
  uint32_t estimated;    /* out: owned pixels with e_p >= 2 and three finite standard errors                      */
  uint32_t reserved;     /* out: 0                                                                                */
  double sum_se2;        /* out: sum of se^2 over those pixels' 3 channels (estimated RMSE: sqrt(sum_se2 / (3 estimated))) */
  uint64_t samples_held; /* out: sum of e_p over the owned pixels                                                 */
  uint64_t reserved2[2];
} rtg_retire;

#define RTG_FLAG_DENOISE 128u /* after the slice, filter the frame into an output plane at the end of out (below) */
#define RTG_DENOISE_MAX_RADIUS 8u
#define RTG_DENOISE_MAX_PATCH 3u

/* Denoising from the noise estimates.  RTG_FLAG_DENOISE needs RTG_FLAG_SUM_SQUARES (else RTG_ERR_INVALID, nothing written or
 * enqueued) and combines freely with PARTIAL, RESUME, SAMPLE_COUNTS, RETIRE and COUNTERS.  `out` then grows at its end by a
 * 64-byte denoise block (rtg_denoise) and an output plane of nx * ny * 3 floats (the pixel layout of plane 0).  The block
 * starts at the first even word (8-byte aligned) behind everything the call's other flags put in the frame: word 6 * nx * ny;
 * with RTG_FLAG_SAMPLE_COUNTS word 7 * nx * ny rounded up to even; with RTG_FLAG_RETIRE the retire block's word + 16.  The
 * output plane starts 16 words behind the block.  Compute the offsets in 64 bits.
 * The filter is a variance-driven non-local-means filter (Rousselle, Knaus, Zwicker 2012) over the pixel means and the
 * variances of those means.  Let e_p = min(n_p, ns) with RTG_FLAG_SAMPLE_COUNTS, else ns (the samples the running sums hold
 * when the call's slice is done).  Everything is float32, every operation rounded on its own, no contraction:
 *   per pixel and channel  m = S / e;  d = Q - S * m, negative or NaN d becomes 0;  v = d / (e * (e - 1)).
 *   A pixel is VALID when e >= 2 and its three m and three v are finite; all others take no part.
 *   For a displacement delta (raster order, dy outer, dx inner, each -radius .. radius) and pixels a, b = a + delta, per channel
 *   d2 = ((m_a - m_b)^2 - (v_a + min(v_b, v_a))) / (1e-10 + k^2 * (v_a + v_b));  pd(a) = (d2_0 + d2_1) + d2_2, and +0, not
 *   counted, when a or b is outside the image or not valid.  The patch distance of p is a sum of row sums:
 *   r(a) = fold over ox = -patch .. patch of pd(a + (0, ox)),  D(p) = fold over oy = -patch .. patch of r(p + (oy, 0)), both
 *   left to right from +0; cnt = the counted elements.  x = D / (3 * cnt);  x = x > 0 ? x : 0;  u = 1 - x * 0.25;
 *   u = u > 0 ? u : 0;  w = (u * u) * (u * u), and w = 0 unless p and p + delta are both valid.  acc_c = acc_c + w * m_{p+delta,c}
 *   and wsum = wsum + w over the displacements in raster order; out_c = acc_c / wsum.
 * rtiow-rust_amd/denoise.py (mean_var, nlm) is this definition in numpy; the output plane equals it bit for bit.
 *   - The output plane gets the filter's result for every valid pixel and S / e_p for every other pixel with e_p > 0 (bit-equal
 *     to the resolved plane 0); pixels with e_p == 0 keep whatever the plane held.
 *   - Order: the call renders its slice, applies RTG_FLAG_RETIRE if set (it changes no e_p), filters the UNDIVIDED running sums,
 *     then divides plane 0 (without RTG_FLAG_PARTIAL).  The planes, the count plane and the retire block end bit for bit as in
 *     the same call without RTG_FLAG_DENOISE.  sample_begin == ns with RTG_FLAG_PARTIAL renders nothing and only filters
 *     (another k, or sums the caller brought).
 *   - RTG_ERR_INVALID, nothing written to any plane: radius > RTG_DENOISE_MAX_RADIUS, patch > RTG_DENOISE_MAX_PATCH, k NaN,
 *     infinite or <= 0, reserved_in != 0, nranks > 1 (the neighbours live on other ranks).
 *   - Every accepted call writes every out-field of the block and never its in-fields.
 *   - rtg_par_cast uploads the block with the frame and copies back the planes, the output plane and the block's out-fields.
 *     rtg_par_cast_device reads the in-fields back on `hip_stream`: one synchronisation of the stream per call.  A counts /
 *     retire call already makes one and the in-fields travel in the same copy-and-wait; a call without a count plane gains
 *     a synchronisation it did not have, made before the call's first kernel (outside rtg_stats.kernel_ms).
 *   - rtg_stats as without the flag; kernel_ms also covers the filter's kernels.  rtg_par_cast_multi returns
 *     RTG_ERR_UNSUPPORTED and rtg_debug_samples RTG_ERR_INVALID, both writing nothing. */
typedef struct rtg_denoise {
  float k;               /* in:  strength: finite and > 0 (0.7 is a good start; larger = smoother)              */
  uint32_t radius;       /* in:  R, 0 .. RTG_DENOISE_MAX_RADIUS: the (2R+1)^2 search window                      */
  uint32_t patch;        /* in:  F, 0 .. RTG_DENOISE_MAX_PATCH: the (2F+1)^2 patches that are compared           */
  uint32_t reserved_in;  /* in:  must be 0                                                                        */
  uint32_t filtered;     /* out: pixels that took part (valid, above) and were filtered                           */
  uint32_t passed;       /* out: pixels with e_p > 0 that are not valid: their plain mean was copied              */
  uint32_t reserved[10]; /* out: 0                                                                                 */
} rtg_denoise;

#define RTG_FLAG_FEATURES 256u /* out ends with first-hit feature planes: albedo, normal, depth (below) */
#define RTG_FEATURES_MAX_GRID 4u

/* Feature planes (what a denoiser or compositor wants beside the colour).  RTG_FLAG_FEATURES needs no other flag and combines
 * freely with PARTIAL, RESUME, SUM_SQUARES, SAMPLE_COUNTS, RETIRE, DENOISE and COUNTERS.  `out` then grows at its end by a
 * 64-byte features block (rtg_features) and three float planes in the pixel layout of plane 0: albedo (nx * ny * 3 floats),
 * normal (nx * ny * 3) and depth (nx * ny).  The block starts at the first even word (8-byte aligned) behind everything the
 * call's other flags put in the frame: behind the float planes (word 3 * nx * ny, or 6 * nx * ny with RTG_FLAG_SUM_SQUARES), the
 * count plane, the retire block (its word + 16) or, with RTG_FLAG_DENOISE, that flag's output plane (the denoise block's word
 * + 16 + 3 * nx * ny).  The albedo plane starts 16 words behind the block, the normal plane 3 * nx * ny words behind that, the
 * depth plane another 3 * nx * ny words on.  Compute the offsets in 64 bits.
 * The planes are deterministic and do not depend on the frame's samples: with grid = g every pixel sends g * g primary rays
 * through the centres of a g x g grid of its area, from the lens centre, at the middle of the exposure.  For pixel (x, row),
 * y = ny - 1 - row, and the rays j = 0 .. g - 1 (outer), i = 0 .. g - 1 (inner), everything float32, every operation rounded on
 * its own, no contraction:  su = (i + 0.5) / g;  sv = (j + 0.5) / g;  u = (x + su) / nx;  v = (y + sv) / ny;  origin =
 * camera.origin;  direction = ((lower_left_corner + u * horizontal) + v * vertical) - origin (Camera::get_ray, camera.rs:52-63,
 * with a zero lens offset);  time = exposure_start + 0.5 * (exposure_end - exposure_start).  Each ray is one hit_top (lib.rs:33)
 * from params.t_near, its RNG keyed (params.seed, pixel = y * nx + x, sample 0) at event 1 -- rtg_debug_hit_top's stream for
 * ray index y * nx + x, so media draw the same numbers.  A hit gives seven values: the albedo (Lambertian and Isotropic: the
 * texture at the hit point; Metal: its albedo; Dielectric: (1, 1, 1); DiffuseLight: brightness * texture, what emitted()
 * returns), the normal of the hit record and its t; a miss gives seven +0.  A plane holds per pixel the left fold of its values
 * over the rays, from +0, divided by (float)(g * g).  rtiow-rust_amd/features.py subpixel_rays is the rays in numpy.
 *   - Everything in front of the features block ends bit for bit as in the same call without the flag, with one exception:
 *     under RTG_FLAG_DENOISE the output plane is the GUIDED filter's.  That filter is the one above with one more factor: for
 *     a displacement, pixels p and q = p + delta, the feature values (a, n, z) of both, and the block's three sigmas,
 *     xn = ((dn0^2 + dn1^2) + dn2^2) / (sigma_normal^2) with dn = n_p - n_q;  xa likewise from the albedo and sigma_albedo;
 *     dz = z_p - z_q;  s = z_p + z_q;  xz = ((dz * dz) / (s * s + 1e-20)) / (sigma_depth^2);  x = xn;  x = xa > x ? xa : x;
 *     x = xz > x ? xz : x;  u = 1 - x * 0.25;  u = u > 0 ? u : 0;  wf = (u * u) * (u * u);  wf = 1 when any of the fourteen
 *     values is not finite;  w = wf < w ? wf : w.  rtiow-rust_amd/denoise.py nlm_guided is this in numpy; the output plane
 *     equals it bit for bit on the feature planes the frame holds when the filter runs.
 *   - compute = 1 traces the planes in this call, for every pixel the call owns (rank / tiles), whatever a count plane says;
 *     pixels of other ranks stay untouched.  compute = 0 leaves the planes alone: they hold what an earlier call traced (a
 *     progressive or adaptive loop computes them on its first slice only) or what the caller put there.  nranks > 1 is fine
 *     without RTG_FLAG_DENOISE.
 *   - RTG_ERR_INVALID, nothing written or enqueued: grid 0 or > RTG_FEATURES_MAX_GRID, compute > 1, reserved_in != 0 and, under
 *     RTG_FLAG_DENOISE, a sigma that is NaN, infinite or <= 0 (without that flag the sigmas are not read).
 *   - Every accepted call writes every out-field of the block and never its in-fields.
 *   - rtg_par_cast uploads the block (and, with compute = 0 under RTG_FLAG_DENOISE, the feature planes), copies back the feature
 *     planes when compute = 1, and always the block's out-fields.  rtg_par_cast_device reads the in-fields back on
 *     `hip_stream` in the copy-and-wait of the denoise / retire / counts read-backs; a call that has none of those gains one
 *     synchronisation, made before its first kernel.
 *   - rtg_stats: the counters are those of the call without the flag (feature rays are not counted); kernel_ms also covers the
 *     feature kernel.  rtg_par_cast_multi returns RTG_ERR_UNSUPPORTED and rtg_debug_samples RTG_ERR_INVALID, both writing
 *     nothing. */
typedef struct rtg_features {
  uint32_t grid;        /* in:  g, 1 .. RTG_FEATURES_MAX_GRID: g * g feature rays per pixel                            */
  uint32_t compute;     /* in:  1 = trace the planes in this call; 0 = the planes already hold them: left alone        */
  float sigma_normal;   /* in:  read only with RTG_FLAG_DENOISE: finite and > 0 (large = that feature is off)          */
  float sigma_albedo;   /* in:  likewise                                                                                */
  float sigma_depth;    /* in:  likewise                                                                                */
  uint32_t reserved_in; /* in:  must be 0                                                                               */
  uint32_t traced;      /* out: owned pixels whose features this call wrote (0 when compute = 0)                        */
  uint32_t missed;      /* out: of those, pixels none of whose rays hit anything                                        */
  uint32_t reserved[8]; /* out: 0                                                                                       */
} rtg_features;

#define RTG_FLAG_DENOISE_ERROR 512u /* out ends with an error plane: the variance of every filtered pixel (below) */

/* The error of the filtered frame.  RTG_FLAG_DENOISE_ERROR needs RTG_FLAG_DENOISE (else RTG_ERR_INVALID, nothing written or
 * enqueued) and combines with everything that flag combines with.  It adds no block: `out` grows at its very end by an error
 * plane of nx * ny * 3 floats (the pixel layout of plane 0), at the first even word (8-byte aligned) behind everything the
 * call's other flags put in the frame -- behind the denoise output plane (the denoise block's word + 16 + 3 * nx * ny) or, with
 * RTG_FLAG_FEATURES, behind the depth plane (the features block's word + 16 + 7 * nx * ny).  No other offset moves.  Compute it
 * in 64 bits.
 * For out_c = sum_q w_q m_q,c / sum_q w_q the variance of the output is ev_c = sum_q w_q^2 v_q,c / (sum_q w_q)^2 (the weights
 * taken as given: the filter's bias is not in it, so the estimate runs low).  In the filter's loop above, for every valid pixel
 * p and every displacement in raster order, once the pair's final weight w is known (the guided cap and the mask of valid pairs
 * included):  acc2_c = acc2_c + (w * w) * v_{p+delta,c}, from +0;  after the loop  ev_c = (acc2_c / wsum) / wsum.  Float32,
 * every operation rounded on its own, no contraction, denormals kept.  rtiow-rust_amd/denoise.py nlm_error / nlm_guided_error
 * are this in numpy; the error plane equals their second result bit for bit.
 *   - The error plane gets ev for every valid pixel, +inf (0x7f800000) in all three channels for every other pixel with e_p > 0
 *     (a pass-through pixel: its error is unknown), and nothing for pixels with e_p == 0, which keep what the plane held.
 *   - Everything in front of the error plane ends bit for bit as in the same call without the flag.
 *   - With RTG_FLAG_RETIRE the call's order becomes render, filter, retire, divide (retiring changes no e_p, so the filter's
 *     output is that of the other order), and the retire rule reads the error plane instead of (S, Q): q is OK when its three
 *     ev_q,c are finite and (double)ev_q,c <= target_se * target_se (the float64 product, computed once; no square root, so ties
 *     are exact).  The window, min_samples, pixels with n_q == 0 being ignored, n_p := k and the block's active / retired /
 *     samples_held stay as above.  Two fields change meaning: estimated counts the owned pixels with n_p > 0 and three finite
 *     ev; sum_se2 is the sum of ((double)ev_0 + ev_1) + ev_2 over them, in the same fixed order -- sqrt(sum_se2 / (3 estimated))
 *     is the estimated RMSE of the FILTERED frame.  rtiow-rust_amd/noise.py retire_filtered is the rule in numpy.
 *   - Without RTG_FLAG_RETIRE the flag only produces the plane.  Without the flag every call is as above, its order included.
 *   - The refusals are those of the call's other flags.  rtg_par_cast and rtg_par_cast_multi (scene option "multi_planes": the
 *     first device writes the plane, it never travels between ranks) treat the error plane as they treat the denoise output
 *     plane: uploaded when that one is, so untouched pixels survive, and copied back.  rtg_debug_samples returns
 *     RTG_ERR_INVALID. */

#define RTG_FLAG_BACKGROUND 1024u /* out ends with a background block: what a ray that leaves the scene sees (below) */

/* A background.  Without the flag a path whose ray misses everything is black (lib.rs:100), so an open scene is lit only by
 * wrapping it in an emitting dome (FlipNormals(Sphere{10000, DiffuseLight})), which costs every ray a sphere test and makes
 * every Bvh root box as wide as the dome.  RTG_FLAG_BACKGROUND needs no other flag and combines freely with PARTIAL, RESUME,
 * SUM_SQUARES, SAMPLE_COUNTS, RETIRE, DENOISE, FEATURES, DENOISE_ERROR and COUNTERS (all of which act on sums the render
 * produced).  `out` then grows at its very end by a 64-byte background block (rtg_background): it starts at the first even word
 * (8-byte aligned) behind everything the call's other flags put in the frame, behind the error plane when there is one; without
 * other flags at word 3 * nx * ny rounded up to even.  No other offset moves.  Compute it in 64 bits.
 * When hit_top (lib.rs:33) returns None for the ray (o, d) of a path with running `accum` and `strength`, the sample's colour is
 *   accum + strength * B(d)
 * -- what lib.rs:76 followed by scatter() == None gives for a light of emission B -- instead of lib.rs:100's black.  strength
 * is (1, 1, 1) for the camera ray.  Float32, every operation rounded on its own, no contraction:
 *   mode 0:  B = bottom;
 *   mode 1:  len = sqrt((dx * dx + dy * dy) + dz * dz);  uy = dy / len;  t = 0.5f * (uy + 1.0f);
 *            B_c = (1.0f - t) * bottom_c + t * top_c     (the book's sky: bottom (1, 1, 1), top (0.5, 0.7, 1.0)).
 * rtiow-rust_amd/background.py sky() is this definition in numpy.  The colours are used as given, like a DiffuseLight's: NaN
 * and infinity propagate.  No RNG draw is made, and the bounce cap is unchanged: a miss ends the path.
 *   - A constant background equals the dome: the frame of a world under mode 0 is bit for bit the frame of that world with
 *     FlipNormals(Sphere{10000, DiffuseLight(bottom, 1.0)}) appended (for rays that end inside that sphere).
 *   - Every render kernel honours the flag, the pool-2 kernel included (its "a miss is booked first" pass reads the missed ray
 *     and the strength back from the path's slot).
 *   - rtg_stats and its counters are those of the same scene without the flag: the walk is identical, only the booked colour
 *     differs.  Feature planes are unchanged: a miss still gives seven +0.
 *   - The block is in-only: the library never writes it.
 *   - RTG_ERR_INVALID, nothing written or enqueued: mode > 1, reserved_in != 0.
 *   - rtg_par_cast reads the block from the host frame.  rtg_par_cast_device reads the in-fields back on `hip_stream` in the
 *     copy-and-wait of the other blocks' read-backs; a call that has none of those gains one synchronisation, made before its
 *     first kernel.  rtg_par_cast_multi accepts the flag with and without scene option "multi_planes": every rank gets the
 *     same host block, and the collective still moves only the planes.  rtg_debug_samples returns RTG_ERR_INVALID.
 *   - Without the flag every call is bit for bit what it is without this section. */
typedef struct rtg_background {
  uint32_t mode;         /* in: 0 = constant (bottom), 1 = gradient along world +y */
  uint32_t reserved_in;  /* in: must be 0 */
  float bottom[3];       /* in */
  float top[3];          /* in: read only in mode 1 */
  uint32_t reserved[8];  /* never written */
} rtg_background;

typedef struct rtg_stats {
  uint32_t struct_size; /* = sizeof(rtg_stats)                                                */
  float kernel_ms;      /* HIP-event time of the render kernel on its stream                  */
  uint64_t samples;     /* pixels rendered by this call x its samples (ns - sample_begin);
                           RTG_FLAG_SAMPLE_COUNTS: the (pixel, sample) pairs it rendered       */
  uint64_t aabb_tests;  /* Aabb::hit calls        (aabb.rs:16)                                 */
  uint64_t prim_tests;  /* Sphere/Rect::hit calls (object.rs:84,185)                           */
  uint64_t shaded_hits; /* hit_top() == Some      (lib.rs:73)                                  */
  uint64_t rays;        /* hit_top() calls                                                     */
  uint64_t draws;       /* RNG u32 draws                                                       */
} rtg_stats;

/* ---- library ---------------------------------------------------------------------------- */
const char* rtg_version(void);
const char* rtg_last_error(void);
int rtg_device_count(int* n);

/* ---- builder: one call per reference constructor ----------------------------------------- */
int rtg_builder_create(rtg_builder** out);
void rtg_builder_destroy(rtg_builder* b);

/* texture.rs:8 constant, :12 checker, :23 perlin.  Return RTG_INVALID_ID on error. */
rtg_id rtg_texture_constant(rtg_builder* b, const float rgb[3]);
rtg_id rtg_texture_checker(rtg_builder* b, rtg_id t0, rtg_id t1);
rtg_id rtg_texture_perlin(rtg_builder* b, float scale);
/* perlin.rs:24-29 VECS / PERM_X / PERM_Y / PERM_Z (thread_rng-seeded globals in the reference):
 * 256 xyz gradient vectors and three 256-entry permutations, supplied by the caller. */
int rtg_builder_set_perlin_tables(rtg_builder* b, const float vecs[768], const uint8_t perm_x[256],
                                  const uint8_t perm_y[256], const uint8_t perm_z[256]);

/* material.rs:10-39 enum Material */
rtg_id rtg_material_lambertian(rtg_builder* b, rtg_id albedo_texture);
rtg_id rtg_material_metal(rtg_builder* b, const float albedo[3], float fuzz);
rtg_id rtg_material_dielectric(rtg_builder* b, float ref_idx);
rtg_id rtg_material_diffuse_light(rtg_builder* b, rtg_id emission_texture, float brightness);
rtg_id rtg_material_isotropic(rtg_builder* b, rtg_id albedo_texture);

/* object.rs: Sphere :75, Rect<A> :131 (axis 0/1/2 = StaticX/Y/Z), FlipNormals :239, Translate :262,
 * Scale :296, rotate_y :477, And :394, rect_prism :420, LinearMove :489, ConstantMedium :533;
 * bvh.rs:128 from_scene (a Bvh is itself an Object, bvh.rs:84). */
rtg_id rtg_object_sphere(rtg_builder* b, float radius, rtg_id material);
rtg_id rtg_object_rect(rtg_builder* b, int orthogonal_to, float range0_start, float range0_end,
                       float range1_start, float range1_end, float k, rtg_id material);
rtg_id rtg_object_flip_normals(rtg_builder* b, rtg_id object);
rtg_id rtg_object_translate(rtg_builder* b, const float offset[3], rtg_id object);
rtg_id rtg_object_scale(rtg_builder* b, const float factor[3], rtg_id object);
rtg_id rtg_object_rotate_y(rtg_builder* b, float degrees, rtg_id object);
rtg_id rtg_object_and(rtg_builder* b, rtg_id object0, rtg_id object1);
rtg_id rtg_object_rect_prism(rtg_builder* b, const float p0[3], const float p1[3], rtg_id material);
rtg_id rtg_object_linear_move(rtg_builder* b, rtg_id object, const float motion[3]);
rtg_id rtg_object_constant_medium(rtg_builder* b, rtg_id boundary, float density, rtg_id material);
rtg_id rtg_object_bvh(rtg_builder* b, const rtg_id* objects, size_t n, float exposure_start,
                      float exposure_end);

/* NOT in the reference (non-parity option): the same Bvh object built with a surface-area
 * heuristic instead of Bvh::new's widest-axis median split.  Closest-hit results are tree-invariant except
 * at exact-t ties; fewer Aabb tests per ray (book-1: 26.0 instead of 40.8). */
rtg_id rtg_object_bvh_sah(rtg_builder* b, const rtg_id* objects, size_t n, float exposure_start,
                          float exposure_end);

/* camera.rs:18 Camera::look */
int rtg_camera_look(const float look_from[3], const float look_at[3], const float up[3], float fov,
                    float aspect, float aperture, float focus_dist, float exposure_start,
                    float exposure_end, rtg_camera* out);

/* ---- scene: flatten the world once into HBM ---------------------------------------------- */
/* `world` is the `[Box<dyn Object>]` list world of lib.rs:33; a `Bvh` world (lib.rs:51) is the
 * one-element list holding the rtg_object_bvh handle (identical arithmetic). */
int rtg_scene_create(rtg_builder* b, const rtg_id* world, size_t n, int device, rtg_scene** out);
void rtg_scene_destroy(rtg_scene* s);
/* Scheduling / measurement switches of one scene handle -- kernel generation, cost-ordered work queue, pool
 * thresholds, workgroup size (names: DESIGN.md section 4 "Knobs").  None of them changes a bit of the result, with one
 * exception: "light_sampling" (below) is another estimator of the same image.  The
 * library reads no environment variable for these.  "box_chains" = 0 stages the full LDS image of a lean
 * program (default 1: the image without box-chain followers; the same framebuffer and counters).  "box_prune" (default 1)
 * leaves out of that image the interior BOX records of the pruning plan too (rtiow_gpu_debug.h rtg_debug_box_plan): the
 * same framebuffer and counters; 0 = off; 2 = counting launches (rtg_stats) stage that image as well, so aabb_tests reports
 * what the production walk executes (fewer than the reference's; every other counter unchanged; a measurement switch).
 * "bvh4" = 1 (scenes
 * that are ONE Bvh of spheres; RTG_ERR_INVALID otherwise) traverses the reference's tree (bvh.rs:22-120) as 4-wide
 * nodes: the same framebuffer, other rtg_stats.aabb_tests / prim_tests than the reference's walk.
 *
 * "light_sampling" = 1 (default 0): direct light sampling (next-event estimation) of the scene's rect lights.  An explicit
 * non-parity mode, like rtg_object_bvh_sah: the same expectation for every max_bounces, other samples, other bits.
 * What it costs (measured): every frame on the one-lane-per-pixel kernels, 25 .. 100 x the kernel time of
 * the ray-pool kernels; and one light sample per hit without multiple importance sampling is heavy-tailed where a surface comes
 * close to a light -- the Cornell box's light hangs one unit under its ceiling: at 256 x 256 x 64 the variance is TEN TIMES the
 * plain estimator's, single pixels spike, and a frame of few samples reads 1-2 % dark; the book-2 final scene's variance is
 * 1.34 x lower.  More plain samples win on both scenes at equal time.  It adds no flag, no struct field and no frame offset: every flag of
 * rtg_params works unchanged on its sums.
 *   Which lights: a DiffuseLight material is SAMPLED when every primitive of the world's graph that uses it is a Rect at the
 *   world's list level, bare or under any number of FlipNormals (not under Translate, Scale, RotateY, LinearMove, And, a
 *   medium boundary or a Bvh).  The rects of the sampled materials, in world order, are the light table, N entries (rects
 *   with an empty range are left out); more than RT_MAX_LIGHTS = 64 entries: setting the option to 1 returns RTG_ERR_INVALID;
 *   none: accepted, the frames are those without the option, bit for bit.  Every other emitter is found by scattered rays
 *   as without the option, at full weight.  Scene option "verbose" prints N.
 *   At a hit (p, n, material) of color()'s loop (lib.rs:60-101), `bounces` the running count:
 *   1. Emission is added as always -- except when the material is sampled and step 2 ran at the previous hit.  Camera rays and
 *      rays leaving Metal, Dielectric or the hit at which the bounce cap ends the path still collect it.
 *   2. When the material is Lambertian or Isotropic, N > 0 and bounces < max_bounces: three gen_f32 draws from the path's
 *      stream -- light i = min(N - 1, floor(u0 N)), then the point q of its rect from (u1, u2), uniform.  w = q - p,
 *      r2 = w.w, cos_l = |w[axis]| / sqrt(r2) (DiffuseLight emits from both faces).  `lobe` is the density of the material's
 *      scattered direction along w.  The reference's Lambertian scatters towards p + n + in_unit_sphere(), a point of the unit
 *      BALL (material.rs:57-65), so its lobe is not cos / pi: with b = n.w / sqrt(r2), disc = b^2 - (n.n - 1),
 *      r_hi = b + sqrt(disc), r_lo = max(b - sqrt(disc), 0): lobe = (r_hi^3 - r_lo^3) / (4 pi), 0 when disc <= 0 or r_hi <= 0
 *      -- 2 cos^3 / pi for |n| = 1, and valid for the unnormalised normals Scale leaves.  Isotropic: lobe = 1 / (4 pi).
 *      When lobe, r2 and cos_l are > 0 a shadow ray runs from p along w (unnormalised: the light sits at t = 1) at the path's
 *      time; it is occluded when anything is hit in [t_near, 1 - 1e-3).  A ConstantMedium takes part with its own free-path
 *      draw, an unbiased estimate of its transmittance.  Unoccluded:
 *        accum += strength * albedo(p) * Le(q) * (lobe * N * area_i * cos_l / r2),  Le(q) = brightness * texture(q).
 *      The last 1e-3 of the segment is not tested (the light itself lies there); that bias is accepted.
 *   3. Scatter as always.  A miss returns accum, plus the background under RTG_FLAG_BACKGROUND (without the option accum is
 *      always +0 at a miss).  max_bounces = 0 makes no new draw.
 *   Every frame of the handle renders on the one-lane-per-pixel kernels (rtg_stats / the debug interface report the baseline
 *   kernel; options "kernel", "bvh4" and the pool thresholds are ignored meanwhile); rtg_debug_samples without
 *   RTG_FLAG_TRACE_KERNEL returns the option's samples, with it RTG_ERR_UNSUPPORTED as for every baseline frame.
 *   rtg_par_cast_multi returns RTG_ERR_INVALID when its handles disagree on the option.  rtg_stats counts what runs: `rays`
 *   includes the shadow rays, `draws` the three light draws and the media draws of shadow rays; `samples` is unchanged. */
int rtg_scene_set_option(rtg_scene* s, const char* name, int value);
/* size of the flattened program (for DESIGN.md's byte accounting / tests); n_box_followers: BOX records of a lean program
 * that repeat the BOX before them bit for bit and are no skip target ("box chains") -- the records production
 * launches leave out of the LDS image.  Every pointer may be NULL. */
int rtg_scene_info(const rtg_scene* s, uint32_t* n_instructions, uint32_t* n_materials,
                   uint32_t* n_textures, uint64_t* hbm_bytes, uint32_t* n_box_followers);

/* ---- the hot path ------------------------------------------------------------------------- */
/* par_cast (lib.rs:363): out_rgb is caller-owned HOST memory, nx*ny*3 floats, row 0 = top
 * (y = ny-1, lib.rs:328), linear radiance (no gamma).  Synchronous. */
int rtg_par_cast(rtg_scene* s, const rtg_camera* camera, const rtg_params* params, float* out_rgb,
                 rtg_stats* stats_or_null);
/* Same, but out_rgb is DEVICE memory on the scene's device and the kernel is enqueued on
 * `hip_stream` (a hipStream_t, NULL = default stream).  Asynchronous unless stats are requested
 * (stats need the kernel to finish).  Frames in flight: a handle owns a ring of launch contexts (work-queue counter,
 * launch constants, cost-ordered queue, scratch, path slots; scene option "frames_in_flight" = 1..4, default 1).  A call
 * takes the next context and first WAITS (on the host) for the frame that used it last, so back-to-back asynchronous calls
 * on one handle are always safe -- with one context they serialise, with n they overlap up to n frames (on different
 * streams).  Each context keeps its own scratch (12 B per pixel and sample up to the budget). */
int rtg_par_cast_device(rtg_scene* s, const rtg_camera* camera, const rtg_params* params,
                        float* d_out_rgb, void* hip_stream, rtg_stats* stats_or_null);

/* Single-process multi-GPU par_cast (SURVEY.md 8b `rtg_render_multi`; reference seam lib.rs:363-376): `scenes[i]` is
 * the SAME world flattened onto device i's HBM (rtg_scene_create with that device index; the scene is small and
 * read-only, so it is replicated).  Scene i renders the pixel tiles (params->tile_w x tile_h; 0 = 16x16, 8x8 from 8 scenes on) with tile_index % n_scenes == i into a
 * zero-filled full frame on its device -- pixels, not samples, are sharded, so every pixel keeps the reference's
 * ordered sample fold -- then ONE collective, ncclReduce(sum) of the float3 framebuffer to the first device over
 * RCCL / xGMI (librccl is dlopen()ed on first use with > 1 distinct device), assembles the frame: x + 0 is exact, the
 * result is bit-identical to rtg_par_cast on one GPU.  Scenes that share a device are summed on that device first.
 * params->rank / nranks must be 0 / 0-or-1 (the call shards by itself).  out_rgb: caller-owned HOST memory.
 * stats: kernel_ms = the slowest shard, counters summed over the shards.  Synchronous.
 * Scene option "multi_gather" = 1 (on any handle) selects the PACKED collective instead: every scene packs the pixels it owns
 * (1 / n_scenes of the frame), grouped ncclSend / ncclRecv bring the packed tiles of the other devices to the first one, which
 * scatters them into its frame -- copies only, bit-identical by construction, 1 / n_scenes of the bytes per device. */
/* Flagged frames over several handles: scene option "multi_planes" (default 0; it counts when set on ANY handle of the call,
 * like "multi_gather" and "force_rccl").  Off, nothing changes: a call with RTG_FLAG_SUM_SQUARES, SAMPLE_COUNTS, RETIRE, DENOISE
 * or FEATURES returns RTG_ERR_UNSUPPORTED and writes nothing.  On, rtg_par_cast_multi accepts these five flags in every
 * combination rtg_par_cast accepts; PARTIAL, RESUME and COUNTERS combine with them as on one handle.
 *   - `out` is HOST memory with exactly the layout rtg_par_cast defines for the same flags, blocks included.  Every word of it
 *     that rtg_par_cast on ONE handle (nranks 0 / 1, same camera, params and blocks) would write ends bit-identical to that
 *     call's; every word that call leaves alone stays as the caller left it (pixels with n_p == 0, the blocks' in-fields,
 *     reserved2, the feature planes under compute = 0, the count plane except under RTG_FLAG_RETIRE) -- for any number of
 *     handles, any tile size, any device placement and either RCCL route.
 *   - Order: every scene renders its tiles as a PARTIAL slice, with SUM_SQUARES / SAMPLE_COUNTS as given, and traces the
 *     feature pass for the pixels it owns when compute = 1; the ranks apply no retire rule, no filter and no division.  The
 *     owned pixels of every plane the ranks wrote (the sum, the squares, the three feature planes when compute = 1) are then
 *     gathered onto the first device's frame, and on that frame the first device runs what a one-handle call with
 *     sample_begin == ns runs: RTG_FLAG_RETIRE with any radius up to RTG_RETIRE_MAX_RADIUS, then RTG_FLAG_DENOISE (guided
 *     when RTG_FLAG_FEATURES is set, over the feature planes the frame now holds), then the division unless RTG_FLAG_PARTIAL --
 *     the same kernels as on one handle.
 *   - Refusals: those of rtg_par_cast with nranks = 1 (the window and the filter see the whole frame, so the "nranks > 1"
 *     clauses above do not apply), checked on the host copy of the blocks before anything is uploaded or enqueued; nothing is
 *     written.  params->rank / nranks must stay 0 / 0-or-1.
 *   - Blocks: the out-fields of every block equal the one-handle call's.  rtg_features.traced / missed are the sums over the
 *     ranks; rtg_retire.sum_se2 comes from the first device's run over the whole frame (tiles of the caller's params, 0 =
 *     16x16), so its bits are the one-handle call's.
 *   - Collective: a call with any of the five flags always takes the packed route (copies only: bit-identical by
 *     construction).  ONE ncclSend / ncclRecv pair per handle that travels carries all its planes, plane-major (word k of work
 *     item w at k * pix_work + w; 3 .. 13 words per pixel), so rtg_multi_reset counts the same transfers as for a plain packed
 *     frame; handles on the first device are unpacked from their own buffer.  The count plane is the caller's input and never
 *     travels back.  A call WITHOUT any of the five flags is unchanged whatever the option says.
 *   - rtg_stats: samples and the counters are the sums over the ranks, equal to the one-handle call's; kernel_ms is the slowest
 *     shard's render span plus the first device's span for retire / filter / division.
 *   - Uploads: the first device's frame is uploaded as rtg_par_cast uploads it (untouched pixels and an untouched output plane
 *     survive); every other rank gets the float planes when the call resumes or has a count plane, and the count plane. */
int rtg_par_cast_multi(rtg_scene* const* scenes, int n_scenes, const rtg_camera* camera,
                       const rtg_params* params, float* out_rgb, rtg_stats* stats_or_null);

/* Forget the multi-GPU state of the library: destroy the cached RCCL communicators (ncclCommDestroy), unload librccl,
 * and choose the library the NEXT rtg_par_cast_multi loads: a path / soname, or NULL for the default search (an already
 * loaded librccl first, then librccl.so.1 / librccl.so / /opt/rocm/lib/librccl.so.1).  A library that cannot be loaded makes
 * rtg_par_cast_multi return RTG_ERR_DEVICE with dlopen's reason.  *n_reduces (may be NULL) receives the number of
 * ncclReduce calls issued since the last reset.  Scene option "force_rccl" = 1 sends rtg_par_cast_multi through the RCCL
 * collective even when all handles sit on ONE device (a clique of one), so that one-GPU hosts exercise the same code. */
int rtg_multi_reset(const char* rccl_library_or_null, uint64_t* n_reduces_or_null);

/* ---- output stage -------------------------------------------------------------------------- */
/* print_ppm's per-channel quantisation (lib.rs:348-356): sqrt gamma, `(255.99 * x) as i32` (saturating,
 * NaN -> 0), clamped to 0..=255.  n floats in, n bytes out; both HOST pointers, computed on `device`.
 * The ASCII P3 writer itself stays on the host (rtiow-rust_amd/ppm.py, host/rtiow.hpp). */
int rtg_tonemap(int device, size_t n, const float* rgb, uint8_t* out_u8);
/* Same on DEVICE pointers, enqueued on `hip_stream`. */
int rtg_tonemap_device(int device, size_t n, const float* d_rgb, uint8_t* d_out_u8, void* hip_stream);

/* ---- probes used by the parity tests (not part of the reference surface) ------------------ */
/* One hit_top() (lib.rs:33-49) per ray. rays: n x 7 floats (origin, direction, time).
 * out: n x 8 floats (hit?1:0, t, p.xyz, normal.xyz); out_material: n material handles.
 * Media inside the scene draw from the counter RNG keyed (seed, pixel=i, sample=0). */
int rtg_debug_hit_top(rtg_scene* s, size_t n, const float* rays, uint64_t seed, float t_near,
                      float* out, uint32_t* out_material);
/* One sample of par_cast's closure (lib.rs:366-372) per (x, y, sample) triple, y counted from the
 * bottom as in the reference. out_rgb: n x 3; out_info: n x 4 (bounces, draws, aabb_tests, prim_tests).
 * Default: a one-lane-per-key probe kernel built from the same device functions as the baseline kernel.  With
 * params->flags & RTG_FLAG_TRACE_KERNEL the WHOLE frame (nx, ny, ns, rank / nranks of `params`) is rendered by the
 * instrumented variant of the production kernel par_cast uses for this scene, with a per-sample trace table switched
 * on, and the keys are read out of it -- so a broken schedule can be localised to a (pixel, sample).
 * RTG_ERR_UNSUPPORTED when that kernel is the baseline one (nothing pooled to trace). */
int rtg_debug_samples(rtg_scene* s, const rtg_camera* camera, const rtg_params* params, size_t n,
                      const uint32_t* xs, const uint32_t* ys, const uint32_t* samples,
                      float* out_rgb, uint32_t* out_info);
/* Evaluate the shared libm restatements on the GPU: op 0 = rt_logf, 1 = rt_pow5f, 2 = rt_sinf,
 * 3 = sqrtf, 4 = 1/x, 5 = x/y with y = in2[i], 6 = rt_atan2f(in[i], in2[i]) (rtiow_gpu_image.h); in2 may be NULL for unary
 * ops. */
int rtg_debug_math(int device, int op, size_t n, const float* in, const float* in2, float* out);

/* Host-only: flatten `world` and copy the flat program out (8 words per instruction: the lo packet
 * then the hi packet, see csrc/flat_scene.h).  Works without a GPU; used by the CPU-side tests. */
int rtg_debug_flatten(rtg_builder* b, const rtg_id* world, size_t n, uint32_t* n_instructions,
                      uint32_t* features, uint32_t* words_out, size_t capacity_instructions);

/* Host-only: the SECOND flat program of `world` -- the one the pool-2 kernel walks (csrc/flat_scene.h "the list level,
 * hoisted": Bvh streams and OP_LIST records, then the records of the list-level items) -- and its item table: 4 words
 * (kind, a, b, c) per item, P2_MAX_ITEMS = 5 items, then (n_items, n_media, n_wrapped, 0): 24 words in `table_out`.
 * *n_instructions = 0 when the world has another shape (such worlds render on the first program only). */
int rtg_debug_flatten_pool2(rtg_builder* b, const rtg_id* world, size_t n, uint32_t* n_instructions, uint32_t* table_out,
                            uint32_t* words_out, size_t capacity_instructions);

#ifdef __cplusplus
}
#endif
#endif /* RTIOW_GPU_H */
