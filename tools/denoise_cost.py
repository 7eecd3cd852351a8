"""What the filter of RTG_FLAG_DENOISE costs and what it buys (include/rtiow_gpu.h; run on an MI355X).

Part 1, the step's cost: the same RTG_FLAG_SUM_SQUARES frame through rtg_par_cast with and without RTG_FLAG_DENOISE, alternating
call by call after one warm-up call of each; medians of rtg_stats.kernel_ms (HIP events around the call's kernels; the read-back
of the block's in-fields happens before the first event) over --reps calls, at (radius, patch) = (5, 2) and (8, 3), and a bit-for-bit check of planes 0 and 1.

Part 2, what it buys: at a few sample counts, the true RMSE -- against a render with 4 x the samples and another seed -- of
the plain frame, of the filtered frame (defaults: 5, 2, k 0.7), and of the plain frame at the sample count whose kernel time
equals render + filter (n_eq = ceil(ns x flagged / plain kernel time), rendered and timed): the equal-time comparison.

Every step runs in a child process of its own under a time limit; the first step that fails or runs out of time ends the run.

  python tools/denoise_cost.py                    # C2 (book-1 1200x800) and C4's frame (book-2 800x800)
  python tools/denoise_cost.py --frames C2 --part 1
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

FRAMES = {
    # name: (scene, nx, ny, ns of part 1, sample counts of part 2)
    "C2": (lambda pkg, b, nx, ny: pkg.scenes.random_scene(b, nx, ny), 1200, 800, 50, (8, 16, 50)),
    "C4": (lambda pkg, b, nx, ny: pkg.scenes.book_final_scene(b, nx, ny, pkg.small_rng.SmallRng(0xDEADBEEF)), 800, 800, 100, (32, 100)),
}
STEP_TIMEOUT_S = 420


def timed(capi, scene, cam, nx, ny, ns, denoise=None, seed=0xDEADBEEF):
    """One whole-frame RTG_FLAG_SUM_SQUARES call with an rtg_stats, without RTG_FLAG_COUNTERS: (frame, kernel_ms)."""
    f = capi.denoise_frame(nx, ny, denoise=denoise)
    p = capi.make_params(nx, ny, ns, seed=seed, squares=True, denoise=denoise is not None)
    st = capi.Stats()
    st.struct_size = C.sizeof(capi.Stats)
    scene.be.check(scene.be._par_cast(scene.h, C.byref(cam), C.byref(p), f.buf.ctypes.data_as(capi.c_f32p), C.byref(st)))
    return f, st.kernel_ms


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def step_cost(pkg, scene, cam, name, nx, ny, ns, reps):
    for R, F in ((5, 2), (8, 3)):
        dn = {"k": 0.7, "radius": R, "patch": F}
        ref, _ = timed(pkg.capi, scene, cam, nx, ny, ns)
        got, _ = timed(pkg.capi, scene, cam, nx, ny, ns, dn)
        same = bool(np.array_equal(got.planes.view(np.uint32), ref.planes.view(np.uint32)))
        t = {False: [], True: []}
        for _ in range(reps):
            for flag in (False, True):
                t[flag].append(timed(pkg.capi, scene, cam, nx, ny, ns, dn if flag else None)[1])
        m0, m1 = float(np.median(t[False])), float(np.median(t[True]))
        print(json.dumps({"part": 1, "frame": "%s %dx%dx%d" % (name, nx, ny, ns), "radius": R, "patch": F, "reps": reps,
                          "kernel_ms": round(m0, 3), "kernel_ms_denoise": round(m1, 3), "filter_ms": round(m1 - m0, 3),
                          "kernel_ms_range": [round(min(t[False]), 3), round(max(t[False]), 3)],
                          "kernel_ms_denoise_range": [round(min(t[True]), 3), round(max(t[True]), 3)],
                          "filtered": got.denoise.filtered, "passed": got.denoise.passed, "planes_bit_equal": same}), flush=True)
        if not same:
            raise SystemExit("planes 0 / 1 differ from the call without the flag")


def step_buys(pkg, scene, cam, name, nx, ny, spps):
    for ns in spps:
        ref = scene.par_cast(cam, nx, ny, 4 * ns, seed=12345)
        timed(pkg.capi, scene, cam, nx, ny, ns), timed(pkg.capi, scene, cam, nx, ny, ns, True)   # warm-up
        t0 = float(np.median([timed(pkg.capi, scene, cam, nx, ny, ns)[1] for _ in range(3)]))
        runs = [timed(pkg.capi, scene, cam, nx, ny, ns, True) for _ in range(3)]
        t1 = float(np.median([r[1] for r in runs]))
        f = runs[-1][0]
        n_eq = max(ns, int(math.ceil(ns * t1 / t0)))
        eq, t_eq = timed(pkg.capi, scene, cam, nx, ny, n_eq)
        print(json.dumps({"part": 2, "frame": "%s %dx%d" % (name, nx, ny), "spp": ns, "reference_spp": 4 * ns,
                          "kernel_ms_plain": round(t0, 3), "kernel_ms_filtered": round(t1, 3),
                          "rmse_plain": round(rmse(f.planes[0], ref), 5), "rmse_filtered": round(rmse(f.denoised, ref), 5),
                          "equal_time": {"spp": n_eq, "kernel_ms": round(t_eq, 3), "rmse_plain": round(rmse(eq.planes[0], ref), 5)}}),
              flush=True)


def run_step(a):
    pkg = graft.load_package()
    gpu = pkg.load()
    fn, nx, ny, ns, spps = FRAMES[a.frame]
    b = gpu.builder()
    world, cam, _ = fn(pkg, b, nx, ny)
    scene = b.scene(world)
    if a.step == "cost":
        step_cost(pkg, scene, cam, a.frame, nx, ny, ns, a.reps)
    else:
        step_buys(pkg, scene, cam, a.frame, nx, ny, spps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="C2,C4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--part", default="1,2")
    ap.add_argument("--step", choices=("cost", "buys"), help="(internal) run one step in this process")
    ap.add_argument("--frame", help="(internal) the step's frame")
    a = ap.parse_args()
    if a.step:
        return run_step(a)
    for name in a.frames.split(","):
        for part, step in (("1", "cost"), ("2", "buys")):
            if part not in a.part:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--frame", name, "--reps", str(a.reps)]
            try:
                rc = subprocess.run(cmd, timeout=STEP_TIMEOUT_S).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit("step %s %s ran past %d s: stopping" % (step, name, STEP_TIMEOUT_S))
            if rc != 0:
                raise SystemExit("step %s %s ended with status %d: stopping" % (step, name, rc))


if __name__ == "__main__":
    main()
