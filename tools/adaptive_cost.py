"""What per-pixel sample counts cost and what adaptive sampling saves (include/rtiow_gpu.h RTG_FLAG_SAMPLE_COUNTS).

Part 1, the flag's cost: the same frame through rtg_par_cast without the flag and with n_p = ns everywhere, alternating call by
call after one warm-up call of each; medians of rtg_stats.kernel_ms (HIP events around the call's kernels, compaction included)
over --reps calls, and a bit-for-bit check of the two frames.

Part 2, adaptive against uniform: Scene.adaptive at a few target_se values (samples and kernel time summed over its slices),
its estimated RMSE (noise.standard_error_counts of the final sums), the uniform progressive frame that first reaches the same
estimated RMSE (Scene.progressive(target_rmse=): samples, and the kernel time of one par_cast at that count), and the true RMSE
of both against a --ref-spp render.

Part 3, the retire rule in the library (include/rtiow_gpu.h RTG_FLAG_RETIRE): (a) wall time per slice of Scene.adaptive's host
loop (numpy rule, whole frames up and down every slice) against its device loop (one RETIRE call, a device-to-device preview
copy, the resolve call, one read-back of the retire block) at target_se 0.05 -- a host clock around each slice, every slice
ending in a synchronisation, one warm-up run of each loop, then host / device alternating --reps-wall times; (b) the device loop
with radius 0 / 1 / 2 against uniform sampling at equal estimated RMSE, as in part 2 (est. RMSE = the retire block's).

  python tools/adaptive_cost.py                          # C2 (book-1 1200x800x50) and C4 (book-2 800x800x1000)
  python tools/adaptive_cost.py --frames C2 --part 1
  python tools/adaptive_cost.py --part 3
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
TARGETS = {"C2": (0.08, 0.05, 0.03), "C4": (0.08, 0.05, 0.03)}
STEPS = {"C2": 5, "C4": 32}


def timed(capi, scene, cam, nx, ny, ns, counts):
    """One rtg_par_cast with an rtg_stats, without RTG_FLAG_COUNTERS: (frame, kernel_ms)."""
    if counts:
        f = capi.counts_frame(nx, ny)
        f.counts[...] = ns
        img, buf = f.planes, f.buf
    else:
        img = buf = np.zeros((ny, nx, 3), dtype=np.float32)
    p = capi.make_params(nx, ny, ns, counts=counts)
    st = capi.Stats()
    st.struct_size = C.sizeof(capi.Stats)
    scene.be.check(scene.be._par_cast(scene.h, C.byref(cam), C.byref(p), buf.ctypes.data_as(capi.c_f32p), C.byref(st)))
    return img, st.kernel_ms


def flag_cost(pkg, scene, cam, name, nx, ny, ns, reps):
    ref, _ = timed(pkg.capi, scene, cam, nx, ny, ns, False)
    got, _ = timed(pkg.capi, scene, cam, nx, ny, ns, True)
    same = bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
    t = {False: [], True: []}
    for _ in range(reps):
        for counts in (False, True):
            t[counts].append(timed(pkg.capi, scene, cam, nx, ny, ns, counts)[1])
    m0, m1 = float(np.median(t[False])), float(np.median(t[True]))
    print(json.dumps({"part": 1, "frame": "%s %dx%dx%d" % (name, nx, ny, ns), "reps": reps, "kernel_ms": round(m0, 2),
                      "kernel_ms_counts": round(m1, 2), "cost_pct": round(100 * (m1 / m0 - 1), 2),
                      "kernel_ms_range": [round(min(t[False]), 2), round(max(t[False]), 2)],
                      "kernel_ms_counts_range": [round(min(t[True]), 2), round(max(t[True]), 2)], "bit_equal": same}), flush=True)
    if not same:
        raise SystemExit("n_p = ns differs from the flagless frame")


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def adaptive_vs_uniform(pkg, scene, cam, name, nx, ny, ns, ref_spp):
    t0 = time.perf_counter()
    ref = scene.par_cast(cam, nx, ny, ref_spp)
    print(json.dumps({"part": 2, "frame": name, "reference_spp": ref_spp, "reference_s": round(time.perf_counter() - t0, 2)}), flush=True)
    step = STEPS[name]
    for target in TARGETS[name]:
        stats = []
        f = pkg.capi.counts_frame(nx, ny, squares=True)
        last = None
        for counts, preview, se in scene.adaptive(cam, nx, ny, ns, step, target, out=f, stats=stats):
            last = (counts, preview, se)
        counts, preview, se = last
        est = float(np.sqrt(np.mean(se[np.isfinite(se)] ** 2)))
        a_samples = int(sum(s["samples"] for s in stats))
        a_ms = float(sum(s["kernel_ms"] for s in stats))
        n_u, img_u = None, None
        for n, img, _ in scene.progressive(cam, nx, ny, ns, step, target_rmse=est):
            n_u, img_u = n, img
        _, u_ms = timed(pkg.capi, scene, cam, nx, ny, n_u, False)
        print(json.dumps({"part": 2, "frame": "%s %dx%d ns<=%d step %d" % (name, nx, ny, ns, step), "target_se": target,
                          "adaptive": {"samples": a_samples, "spp_mean": round(a_samples / (nx * ny), 1),
                                       "kernel_ms": round(a_ms, 1), "slices": len(stats), "est_rmse": round(est, 5),
                                       "true_rmse": round(rmse(preview, ref), 5), "retired_px_pct": round(100 * float((counts < ns).mean()), 1)},
                          "uniform": {"spp": n_u, "samples": n_u * nx * ny, "kernel_ms_one_call": round(u_ms, 1),
                                      "true_rmse": round(rmse(img_u, ref), 5)}}), flush=True)


class DeviceFrames:
    """A retire frame and a preview buffer in device memory (hipMalloc), and a stream."""
    def __init__(self, capi, nx, ny):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.hip.hipStreamDestroy.argtypes = [C.c_void_p]
        self.nx, self.ny = nx, ny
        self.out, self.preview, self.stream = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.out), capi.retire_frame_bytes(nx, ny)) == 0
        assert self.hip.hipMalloc(C.byref(self.preview), 4 * nx * ny * 4) == 0
        assert self.hip.hipStreamCreate(C.byref(self.stream)) == 0

    def read(self, what):
        n = self.nx * self.ny
        if what == "preview":
            a = np.empty((self.ny, self.nx, 3), np.float32)
            assert self.hip.hipMemcpy(a.ctypes.data, self.preview, a.nbytes, 2) == 0
        else:
            a = np.empty((self.ny, self.nx), np.uint32)
            assert self.hip.hipMemcpy(a.ctypes.data, self.out.value + 24 * n, a.nbytes, 2) == 0
        return a

    def close(self):
        self.hip.hipFree(self.out), self.hip.hipFree(self.preview), self.hip.hipStreamDestroy(self.stream)


def run_loop(scene, cam, nx, ny, ns, step, target, dev=None, radius=0, stats=None):
    """One Scene.adaptive run: wall ms of every slice (host clock around each, every slice ends in a synchronisation) and the
    last item."""
    if dev is None:
        gen = scene.adaptive(cam, nx, ny, ns, step, target, radius=radius, stats=stats)
    else:
        gen = scene.adaptive(cam, nx, ny, ns, step, target, radius=radius, stats=stats, out=dev.out.value,
                             preview=dev.preview.value, stream=dev.stream.value)
    walls, last = [], None
    while True:
        t0 = time.perf_counter()
        try:
            last = next(gen)
        except StopIteration:
            return walls, last
        walls.append(1e3 * (time.perf_counter() - t0))


def loop_wall(pkg, scene, cam, name, nx, ny, ns, reps):
    step, target = STEPS[name], 0.05
    dev = DeviceFrames(pkg.capi, nx, ny)
    try:
        run_loop(scene, cam, nx, ny, ns, step, target)
        run_loop(scene, cam, nx, ny, ns, step, target, dev)
        w = {"host": [], "device": []}
        k_ms = {"host": [], "device": []}
        for _ in range(reps):
            for kind in ("host", "device"):
                stats = []
                walls, last = run_loop(scene, cam, nx, ny, ns, step, target, dev if kind == "device" else None, stats=stats)
                w[kind].append(walls)
                k_ms[kind].append([s["kernel_ms"] for s in stats])
                if kind == "host":
                    held = last[0]
                else:
                    same = bool((np.minimum(dev.read("counts"), last[0]) == held).all())
        out = {"part": 3, "what": "wall per slice", "frame": "%s %dx%d ns<=%d step %d" % (name, nx, ny, ns, step),
               "target_se": target, "reps": reps, "same_counts": same}
        for kind in ("host", "device"):
            flat = [x for r in w[kind] for x in r]
            kf = [x for r in k_ms[kind] for x in r]
            out[kind] = {"slices": len(w[kind][0]), "wall_ms_per_slice_median": round(float(np.median(flat)), 2),
                         "wall_ms_per_slice_range": [round(min(flat), 2), round(max(flat), 2)],
                         "kernel_ms_per_slice_median": round(float(np.median(kf)), 2),
                         "wall_ms_total_median": round(float(np.median([sum(r) for r in w[kind]])), 1)}
        print(json.dumps(out), flush=True)
    finally:
        dev.close()


def radius_vs_uniform(pkg, scene, cam, name, nx, ny, ns, ref_spp):
    ref = scene.par_cast(cam, nx, ny, ref_spp)
    step = STEPS[name]
    dev = DeviceFrames(pkg.capi, nx, ny)
    try:
        for target in TARGETS[name]:
            n_u, img_u = None, None
            for radius in (0, 1, 2):
                stats = []
                _, (k, _, info) = run_loop(scene, cam, nx, ny, ns, step, target, dev, radius=radius, stats=stats)
                held = np.minimum(dev.read("counts"), k)
                preview = dev.read("preview")
                est = info["est_rmse"]
                for n, img, _ in scene.progressive(cam, nx, ny, ns, step, target_rmse=est):
                    n_u, img_u = n, img
                _, u_ms = timed(pkg.capi, scene, cam, nx, ny, n_u, False)
                a_samples = int(sum(s["samples"] for s in stats))
                print(json.dumps({"part": 3, "frame": "%s %dx%d ns<=%d step %d" % (name, nx, ny, ns, step), "target_se": target,
                                  "radius": radius, "reference_spp": ref_spp,
                                  "adaptive": {"samples": a_samples, "spp_mean": round(a_samples / (nx * ny), 1),
                                               "kernel_ms": round(float(sum(s["kernel_ms"] for s in stats)), 1), "slices": len(stats),
                                               "est_rmse": round(est, 5), "true_rmse": round(rmse(preview, ref), 5),
                                               "retired_px_pct": round(100 * float((held < ns).mean()), 1)},
                                  "uniform": {"spp": n_u, "samples": n_u * nx * ny, "kernel_ms_one_call": round(u_ms, 1),
                                              "true_rmse": round(rmse(img_u, ref), 5)}}), flush=True)
    finally:
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="C2,C4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--part", default="1,2")
    ap.add_argument("--ref-spp", type=int, default=0, help="reference render (default: 4 x ns)")
    ap.add_argument("--reps-wall", type=int, default=3, help="part 3 (a): measured runs of each loop")
    a = ap.parse_args()
    pkg = graft.load_package()
    gpu = pkg.load()
    for name in a.frames.split(","):
        fn, nx, ny, ns = FRAMES[name]
        b = gpu.builder()
        world, cam, _ = fn(pkg, b, nx, ny)
        scene = b.scene(world)
        if "1" in a.part:
            flag_cost(pkg, scene, cam, name, nx, ny, ns, a.reps)
        if "2" in a.part:
            adaptive_vs_uniform(pkg, scene, cam, name, nx, ny, ns, a.ref_spp or 4 * ns)
        if "3" in a.part:
            loop_wall(pkg, scene, cam, name, nx, ny, ns, a.reps_wall)
            radius_vs_uniform(pkg, scene, cam, name, nx, ny, ns, a.ref_spp or 4 * ns)


if __name__ == "__main__":
    main()
