"""What RTG_FLAG_SUM_SQUARES costs (include/rtiow_gpu.h): the same frame through rtg_par_cast with and without the flag,
alternating call by call after one warm-up call of each, timed two ways -- rtg_stats.kernel_ms (HIP events around the frame's
kernels on the library's stream) and a host clock around the whole synchronous call (uploads, kernels, copy back: the flag
doubles the copy back).  Prints the medians of --reps calls of each and checks plane 0 against the flagless frame, bit for bit.

  python tools/squares_cost.py                 # C2 (book-1 1200x800x50) and C4 (book-2 800x800x1000)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

FRAMES = {
    "C2": (lambda pkg, b, nx, ny: pkg.scenes.random_scene(b, nx, ny), 1200, 800, 50),
    "C4": (lambda pkg, b, nx, ny: pkg.scenes.book_final_scene(b, nx, ny, pkg.small_rng.SmallRng(0xDEADBEEF)), 800, 800, 1000),
}


def timed(capi, scene, cam, nx, ny, ns, squares):
    """One rtg_par_cast with an rtg_stats but without RTG_FLAG_COUNTERS (Scene.par_cast(stats=True) would run the instrumented
    kernels): (frame, kernel_ms, host ms)."""
    img = np.zeros((2, ny, nx, 3) if squares else (ny, nx, 3), dtype=np.float32)
    p = capi.make_params(nx, ny, ns, squares=squares)
    st = capi.Stats()
    st.struct_size = C.sizeof(capi.Stats)
    t0 = time.perf_counter()
    scene.be.check(scene.be._par_cast(scene.h, C.byref(cam), C.byref(p), img.ctypes.data_as(capi.c_f32p), C.byref(st)))
    return img, st.kernel_ms, (time.perf_counter() - t0) * 1e3   # (rtg_par_cast returns after the copy back)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="C2,C4")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    pkg = graft.load_package()
    gpu = pkg.load()
    for name in a.frames.split(","):
        fn, nx, ny, ns = FRAMES[name]
        b = gpu.builder()
        world, cam, _ = fn(pkg, b, nx, ny)
        scene = b.scene(world)
        ref, _, _ = timed(pkg.capi, scene, cam, nx, ny, ns, False)   # warm-up (allocations, occupancy queries), both variants
        planes, _, _ = timed(pkg.capi, scene, cam, nx, ny, ns, True)
        same = bool(np.array_equal(planes[0].view(np.uint32), ref.view(np.uint32)))
        t = {False: ([], []), True: ([], [])}
        for _ in range(a.reps):
            for squares in (False, True):
                _, k, h = timed(pkg.capi, scene, cam, nx, ny, ns, squares)
                t[squares][0].append(k)
                t[squares][1].append(h)
        med = {sq: (float(np.median(t[sq][0])), float(np.median(t[sq][1]))) for sq in t}
        print(json.dumps({"frame": "%s %dx%dx%d" % (name, nx, ny, ns), "reps": a.reps,
                          "kernel_ms": round(med[False][0], 2), "kernel_ms_squares": round(med[True][0], 2),
                          "kernel_cost_pct": round(100 * (med[True][0] / med[False][0] - 1), 2),
                          "kernel_ms_range": [round(min(t[False][0]), 2), round(max(t[False][0]), 2)],
                          "kernel_ms_squares_range": [round(min(t[True][0]), 2), round(max(t[True][0]), 2)],
                          "host_ms": round(med[False][1], 2), "host_ms_squares": round(med[True][1], 2),
                          "host_cost_pct": round(100 * (med[True][1] / med[False][1] - 1), 2),
                          "plane0_bit_equal": same}), flush=True)
        if not same:
            raise SystemExit("plane 0 differs from the flagless frame")


if __name__ == "__main__":
    main()
