"""What the feature pass of RTG_FLAG_FEATURES and the guided filter cost, and what guiding buys (include/rtiow_gpu.h; run on
an MI355X).  The method is tools/denoise_cost.py's: alternating calls after one warm-up call of each, medians and ranges of
rtg_stats.kernel_ms over --reps calls.

Step pass: the same whole-frame call through rtg_par_cast without the flag and with it at grid 1, 2 and 4; the difference is
the feature pass.  Plane 0 is checked bit for bit.

Step guided: on one rendered RTG_FLAG_SUM_SQUARES frame, the render-less filter call (sample_begin = ns, PARTIAL: the call's
kernels are the filter's alone) colour-only, guided with the neighbours' feature records read through the caches, and guided
with them in LDS (scene option guide_lds), at (radius, patch) = (5, 2) and (8, 3).

Step buys: at a few sample counts, the true RMSE -- against a render with 4 x the samples and another seed -- of the plain
frame, of the colour-only filter and of the guided filter over k and sigma (all three sigmas equal).

Every step runs in a child process of its own under a time limit; the first step that fails or runs out of time ends the run.

  python tools/features_cost.py                    # C2 (book-1 1200x800) and C4's frame (book-2 800x800)
  python tools/features_cost.py --frames C2 --steps pass,guided
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

FRAMES = {
    # name: (scene, nx, ny, ns of the cost steps, sample counts of step buys)
    "C2": (lambda pkg, b, nx, ny: pkg.scenes.random_scene(b, nx, ny), 1200, 800, 50, (8, 50)),
    "C4": (lambda pkg, b, nx, ny: pkg.scenes.book_final_scene(b, nx, ny, pkg.small_rng.SmallRng(0xDEADBEEF)), 800, 800, 100, (32, 100)),
}
KS = (0.7, 1.0, 1.5, 2.5)
SIGMAS = (0.1, 0.25, 0.5, 1.0)
STEP_TIMEOUT_S = 420


def call(scene, cam, p, frame):
    """One rtg_par_cast into `frame` with an rtg_stats, without RTG_FLAG_COUNTERS: kernel_ms."""
    capi = sys.modules["rtiow_rust_amd"].capi
    st = capi.Stats()
    st.struct_size = C.sizeof(capi.Stats)
    scene.be.check(scene.be._par_cast(scene.h, C.byref(cam), C.byref(p), frame.buf.ctypes.data_as(capi.c_f32p), C.byref(st)))
    return st.kernel_ms


def spread(ts):
    return {"median": round(float(np.median(ts)), 3), "range": [round(min(ts), 3), round(max(ts), 3)]}


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def step_pass(pkg, scene, cam, name, nx, ny, ns, reps):
    capi = pkg.capi
    grids = (0, 1, 2, 4)   # 0: the call without the flag
    frames = {g: capi.features_frame(nx, ny, features={"grid": g}) if g else capi.features_frame(nx, ny) for g in grids}
    params = {g: capi.make_params(nx, ny, ns, features=g != 0) for g in grids}
    t = {g: [] for g in grids}
    for rep in range(reps + 1):
        for g in grids:
            ms = call(scene, cam, params[g], frames[g])
            if rep:   # (the first round is the warm-up)
                t[g].append(ms)
    same = all(np.array_equal(frames[g].planes.view(np.uint32), frames[0].planes.view(np.uint32)) for g in grids)
    base = float(np.median(t[0]))
    print(json.dumps({"step": "pass", "frame": "%s %dx%dx%d" % (name, nx, ny, ns), "reps": reps, "kernel_ms": spread(t[0]),
                      "with_features": {"grid %d" % g: dict(spread(t[g]), pass_ms=round(float(np.median(t[g])) - base, 3),
                                                            missed=frames[g].features.missed) for g in grids[1:]},
                      "plane_0_bit_equal": bool(same)}), flush=True)
    if not same:
        raise SystemExit("plane 0 differs from the call without the flag")


def rendered(pkg, scene, cam, nx, ny, ns):
    """A FeaturesFrame with two planes of running sums at ns samples, its 2 x 2 feature planes and a denoise block."""
    f = pkg.capi.features_frame(nx, ny, squares=True, denoise=True, features={"grid": 2})
    scene.par_cast(cam, nx, ny, ns, out=f, features=True, denoise=True, squares=True, partial=True)
    f.features.compute = 0
    return f


def filter_call(pkg, scene, cam, f, ns, k, radius, patch, sigma=None, plain=None):
    """The render-less filter call on f's sums: guided by f's feature planes with the three sigmas = sigma, or (sigma None)
    colour-only through the DenoiseFrame `plain`, which holds the same sums.  -> (kernel_ms, filtered frame)."""
    capi = pkg.capi
    frame = f if sigma is not None else plain
    frame.denoise.k, frame.denoise.radius, frame.denoise.patch = k, radius, patch
    if sigma is not None:
        f.features.sigma_normal = f.features.sigma_albedo = f.features.sigma_depth = sigma
    p = capi.make_params(f.nx, f.ny, ns, squares=True, denoise=True, features=sigma is not None, partial=True, resume=True, sample_begin=ns)
    return call(scene, cam, p, frame), frame.denoised


def step_guided(pkg, scene, cam, name, nx, ny, ns, reps):
    f = rendered(pkg, scene, cam, nx, ny, ns)
    plain = pkg.capi.denoise_frame(nx, ny)
    plain.planes[...] = f.planes
    for R, F in ((5, 2), (8, 3)):
        t = {"colour_only": [], "guided_through_caches": [], "guided_lds": []}
        for rep in range(reps + 1):
            for kind in t:
                scene.set_option("guide_lds", 1 if kind == "guided_lds" else 0)
                ms, _ = filter_call(pkg, scene, cam, f, ns, 1.0, R, F, None if kind == "colour_only" else 0.5, plain)
                if rep:
                    t[kind].append(ms)
        scene.set_option("guide_lds", 0)
        print(json.dumps(dict({"step": "guided", "frame": "%s %dx%dx%d" % (name, nx, ny, ns), "radius": R, "patch": F, "reps": reps},
                              **{kind: spread(ts) for kind, ts in t.items()})), flush=True)


def step_buys(pkg, scene, cam, name, nx, ny, spps):
    for ns in spps:
        ref = scene.par_cast(cam, nx, ny, 4 * ns, seed=12345)
        f = rendered(pkg, scene, cam, nx, ny, ns)
        plain = pkg.capi.denoise_frame(nx, ny)
        plain.planes[...] = f.planes
        row = {"step": "buys", "frame": "%s %dx%d" % (name, nx, ny), "spp": ns, "reference_spp": 4 * ns,
               "rmse_plain": round(rmse(f.planes[0] / np.float32(ns), ref), 5), "colour_only": {}, "guided": {}}
        for k in KS:
            row["colour_only"]["k %.1f" % k] = round(rmse(filter_call(pkg, scene, cam, f, ns, k, 5, 2, None, plain)[1], ref), 5)
            row["guided"]["k %.1f" % k] = {"sigma %.2f" % s: round(rmse(filter_call(pkg, scene, cam, f, ns, k, 5, 2, s)[1], ref), 5)
                                           for s in SIGMAS}
        print(json.dumps(row), flush=True)


def run_step(a):
    pkg = graft.load_package()
    gpu = pkg.load()
    fn, nx, ny, ns, spps = FRAMES[a.frame]
    b = gpu.builder()
    world, cam, _ = fn(pkg, b, nx, ny)
    scene = b.scene(world)
    if a.step == "pass":
        step_pass(pkg, scene, cam, a.frame, nx, ny, ns, a.reps)
    elif a.step == "guided":
        step_guided(pkg, scene, cam, a.frame, nx, ny, ns, a.reps)
    else:
        step_buys(pkg, scene, cam, a.frame, nx, ny, spps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="C2,C4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", default="pass,guided,buys")
    ap.add_argument("--step", choices=("pass", "guided", "buys"), help="(internal) run one step in this process")
    ap.add_argument("--frame", help="(internal) the step's frame")
    a = ap.parse_args()
    if a.step:
        return run_step(a)
    for name in a.frames.split(","):
        for step in a.steps.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--frame", name, "--reps", str(a.reps)]
            try:
                rc = subprocess.run(cmd, timeout=STEP_TIMEOUT_S).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit("step %s %s ran past %d s: stopping" % (step, name, STEP_TIMEOUT_S))
            if rc != 0:
                raise SystemExit("step %s %s ended with status %d: stopping" % (step, name, rc))


if __name__ == "__main__":
    main()
