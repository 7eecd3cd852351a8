"""What the error plane of the filtered frame costs and what adaptive sampling on it buys (include/rtiow_gpu.h
RTG_FLAG_DENOISE_ERROR).

Part 1, the filter's cost: a frame's running sums at 8 samples, then the render-less call (sample_begin == ns, PARTIAL: the
filter's kernels alone) without and with the flag, alternating call by call after one warm-up call of each, colour-only and
guided (feature planes traced once, compute = 0 afterwards); medians of rtg_stats.kernel_ms over --reps calls and a word-for-word
check of everything in front of the error plane.  --other-lib PATH: the flagless call also through another build of the library
(the parent commit's), alternating with this one's.

Part 2, three routes to a filtered frame, per target and radius: Scene.adaptive with the filtered rule (filtered_error=True);
Scene.adaptive with the raw rule and one filter call on its final sums; one uniform call with the filter at the sample count
whose filtered frame first reaches the first route's estimated RMSE (found slice by slice).  For each: mean samples per pixel,
kernel ms (rtg_stats.kernel_ms summed over the route's calls), the estimated RMSE of the filtered frame (its error plane) and
its true RMSE against a --ref-spp render with ANOTHER seed (a sample's stream is keyed by its index: the routes' own seed would put
their very samples into the reference), whose own estimated RMSE is printed first -- a "true" RMSE near it is the reference's noise.

  python tools/filtered_error_cost.py                      # C2 (book-1 1200x800, ns <= 50) and C4 (book-2 800x800, ns <= 1000)
  python tools/filtered_error_cost.py --frames C2 --part 1
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

FRAMES = {
    "C2": (lambda pkg, b, nx, ny: pkg.scenes.random_scene(b, nx, ny), 1200, 800, 50),
    "C4": (lambda pkg, b, nx, ny: pkg.scenes.book_final_scene(b, nx, ny, pkg.small_rng.SmallRng(0xDEADBEEF)), 800, 800, 1000),
}
TARGETS = (0.03, 0.05, 0.08)
STEPS = {"C2": 5, "C4": 32}
DENOISE = {"k": 0.7, "radius": 5, "patch": 2}
REF_SEED = 12345


def raw_call(capi, scene, cam, buf, nx, ny, ns, **kw):
    """One rtg_par_cast on a frame's buffer, with an rtg_stats and without RTG_FLAG_COUNTERS: kernel_ms."""
    p = capi.make_params(nx, ny, ns, **kw)
    st = capi.Stats.new()
    scene.be.check(scene.be._par_cast(scene.h, C.byref(cam), C.byref(p), buf.ctypes.data_as(capi.c_f32p), C.byref(st)))
    return st.kernel_ms


def scene_of(pkg, be, name):
    fn, nx, ny, ns = FRAMES[name]
    b = be.builder()
    world, cam, _ = fn(pkg, b, nx, ny)
    return b.scene(world), cam, nx, ny, ns


def filter_cost(pkg, gpu, other, name, reps):
    capi = pkg.capi
    scene, cam, nx, ny, _ = scene_of(pkg, gpu, name)
    other_scene = scene_of(pkg, other, name)[0] if other is not None else None
    ns = 8
    for guided in (False, True):
        feat = {"grid": 1} if guided else None
        make = (lambda error: capi.features_frame(nx, ny, True, False, False, DENOISE, feat, error)) if guided else (
            lambda error: capi.denoise_frame(nx, ny, denoise=DENOISE, error=error))
        frames = {False: make(False), True: make(True)}
        on = {"squares": True, "denoise": True, "features": guided}
        for error, f in frames.items():   # the sums (and the feature planes), then compute = 0
            raw_call(capi, scene, cam, f.buf, nx, ny, ns, partial=True, error=error, **on)
            if guided:
                f.features.compute = 0
        only = dict(on, sample_begin=ns, resume=True, partial=True)
        runs = [("plain", scene, frames[False], False), ("error", scene, frames[True], True)]
        if other_scene is not None:
            runs.append(("plain_other_lib", other_scene, frames[False], False))
        t = {k: [] for k, _, _, _ in runs}
        for i in range(reps + 1):   # (the first round warms up)
            for k, sc, f, error in runs:
                ms = raw_call(capi, sc, cam, f.buf, nx, ny, ns, error=error, **only)
                if i:
                    t[k].append(ms)
        w = frames[False].layout.words
        same = bool((frames[True].buf.view(np.uint32)[:w] == frames[False].buf.view(np.uint32)).all())
        ev = frames[True].error
        out = {"part": 1, "frame": "%s %dx%d sums of %d samples" % (name, nx, ny, ns), "filter": dict(DENOISE, guided=guided),
               "reps": reps, "front_words_equal": same, "finite_ev_pct": round(100 * float(np.isfinite(ev).all(axis=-1).mean()), 2)}
        for k in t:
            out[k] = {"kernel_ms": round(float(np.median(t[k])), 4), "range": [round(min(t[k]), 4), round(max(t[k]), 4)]}
        out["error_cost_pct"] = round(100 * (out["error"]["kernel_ms"] / out["plain"]["kernel_ms"] - 1), 2)
        if other_scene is not None:
            out["plain_vs_other_lib_pct"] = round(100 * (out["plain"]["kernel_ms"] / out["plain_other_lib"]["kernel_ms"] - 1), 2)
        print(json.dumps(out), flush=True)
        if not same:
            raise SystemExit("the flag changed a word in front of the error plane")


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def est_rmse(pkg, ev, counts):
    n, s2 = pkg.noise.filtered_estimate(ev, counts)
    return float(np.sqrt(s2 / (3 * n))) if n else float("inf")


def routes(pkg, gpu, name, ref_spp, radii):
    capi = pkg.capi
    scene, cam, nx, ny, ns = scene_of(pkg, gpu, name)
    step = STEPS[name]
    sums = scene.par_cast(cam, nx, ny, ref_spp, seed=REF_SEED, squares=True, partial=True)
    ref = (sums[0].astype(np.float64) / ref_spp).astype(np.float32)
    frame = "%s %dx%d ns<=%d step %d" % (name, nx, ny, ns, step)
    print(json.dumps({"part": 2, "frame": frame, "reference_spp": ref_spp, "reference_seed": REF_SEED,
                      "reference_est_rmse": round(pkg.noise.estimated_rmse(sums[0], sums[1], ref_spp), 5)}), flush=True)
    for target in TARGETS:
        for radius in radii:
            out = {"part": 2, "frame": frame, "target_se": target, "radius": radius}
            # (a) the filtered rule
            stats, f = [], capi.denoise_frame(nx, ny, True, denoise=DENOISE, error=True)
            for item in scene.adaptive(cam, nx, ny, ns, step, target, out=f, stats=stats, radius=radius, denoise=DENOISE,
                                       filtered_error=True):
                pass
            samples = int(sum(s["samples"] for s in stats))
            est_a = est_rmse(pkg, f.error, f.counts)
            out["adaptive_filtered_rule"] = {"spp_mean": round(samples / (nx * ny), 2), "kernel_ms": round(sum(s["kernel_ms"] for s in stats), 2),
                                             "slices": len(stats), "est_rmse": round(est_a, 5), "true_rmse": round(rmse(f.denoised, ref), 5),
                                             "retired_px_pct": round(100 * float((f.counts < ns).mean()), 1)}
            # (b) the raw rule, then one filter call on the final sums
            stats, c = [], capi.counts_frame(nx, ny, squares=True)
            for item in scene.adaptive(cam, nx, ny, ns, step, target, out=c, stats=stats, radius=radius):
                pass
            g = capi.denoise_frame(nx, ny, True, denoise=DENOISE, error=True)
            g.planes[...], g.counts[...] = c.planes, c.counts
            ms = raw_call(capi, scene, cam, g.buf, nx, ny, ns, squares=True, counts=True, denoise=True, error=True, sample_begin=ns,
                          resume=True, partial=True)
            samples = int(sum(s["samples"] for s in stats))
            out["adaptive_raw_rule_then_filter"] = {"spp_mean": round(samples / (nx * ny), 2),
                                                    "kernel_ms": round(sum(s["kernel_ms"] for s in stats) + ms, 2), "slices": len(stats),
                                                    "est_rmse": round(est_rmse(pkg, g.error, g.counts), 5),
                                                    "true_rmse": round(rmse(g.denoised, ref), 5),
                                                    "retired_px_pct": round(100 * float((c.counts < ns).mean()), 1)}
            # (c) uniform: the first slice end whose filtered frame reaches (a)'s estimated RMSE, then ONE call at that count
            u = capi.denoise_frame(nx, ny, denoise=DENOISE, error=True)
            n_u, done = ns, 0
            everywhere = np.ones((ny, nx), np.uint32)
            while done < ns:
                end = min(ns, done + step)
                raw_call(capi, scene, cam, u.buf, nx, ny, end, squares=True, denoise=True, error=True, sample_begin=done, resume=True,
                         partial=True)
                done = end
                if est_rmse(pkg, u.error, everywhere) <= est_a:
                    n_u = end
                    break
            u = capi.denoise_frame(nx, ny, denoise=DENOISE, error=True)
            raw_call(capi, scene, cam, u.buf, nx, ny, n_u, squares=True, denoise=True, error=True)   # (warm-up of this sample count)
            ms = raw_call(capi, scene, cam, u.buf, nx, ny, n_u, squares=True, denoise=True, error=True)
            out["uniform_then_filter"] = {"spp": n_u, "kernel_ms": round(ms, 2), "est_rmse": round(est_rmse(pkg, u.error, everywhere), 5),
                                          "true_rmse": round(rmse(u.denoised, ref), 5)}
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="C2,C4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--part", default="1,2")
    ap.add_argument("--radii", default="0,1")
    ap.add_argument("--ref-spp", type=int, default=0, help="reference render (default: 4 x ns)")
    ap.add_argument("--other-lib", default=None, help="part 1: another build of librtiow_gpu.so to time the flagless call against")
    a = ap.parse_args()
    pkg = graft.load_package()
    gpu = pkg.load()
    other = pkg.capi.Backend(a.other_lib, "rtg_") if a.other_lib else None
    for name in a.frames.split(","):
        if "1" in a.part:
            filter_cost(pkg, gpu, other, name, a.reps)
        if "2" in a.part:
            routes(pkg, gpu, name, a.ref_spp or 4 * FRAMES[name][3], [int(r) for r in a.radii.split(",")])


if __name__ == "__main__":
    main()
