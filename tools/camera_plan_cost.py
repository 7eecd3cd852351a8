#!/usr/bin/env python3
"""One-off cost of the camera plan (scene option box_camera; GPU box): for book-1 at 1200x800x50 and at 300x300x100, the wall time
of the first, second and third call of a fresh handle (rtg_par_cast_device + stream sync) at box_camera 0 and at the default, and
the GPU-side time of each (stats->kernel_ms).  At the default the first call of a large enough frame carries the probe kernel, the
second the wait for its counts, the tree DP and the table's upload (the library prints that host time with option verbose: the
"[rtg] camera plan:" line), the third neither.  Frames below CAMERA_PLAN_MIN_SAMPLES never probe.
Run it under `rocprofv3 --kernel-trace --stats` for the duration of camera_probe_kernel itself.
usage: camera_plan_cost.py [nx ny ns]..."""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def main():
    import torch
    pkg = graft.load_package()
    gpu = pkg.load()
    args = sys.argv[1:]
    frames = [(1200, 800, 50), (300, 300, 100)]
    if args:
        frames = [(int(args[i]), int(args[i + 1]), int(args[i + 2])) for i in range(0, len(args), 3)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for nx, ny, ns in frames:
        fb = torch.zeros((ny, nx, 3), dtype=torch.float32, device="cuda:0")
        ptr = ctypes.c_void_p(fb.data_ptr())
        p = pkg.make_params(nx, ny, ns)
        for mode in (0, 1):
            calls = [[], [], []]
            for rep in range(5):
                b = gpu.builder()
                world, cam, _ = pkg.scenes.random_scene(b, nx, ny)
                sc = b.scene(world)
                sc.set_option("box_camera", mode)
                sc.set_option("verbose", 1 if rep == 0 and mode else 0)
                warm = gpu.camera_look(pkg.scenes.v(-13, 2, -3), pkg.scenes.v(0, 0, 0), pkg.scenes.v(0, 1, 0), 20.0, nx / ny, 0.1, 10.0)
                sc.par_cast_device(warm, pkg.make_params(nx, ny, 1), ptr, stream)   # (buffers, kernel set-up: not the camera's cost)
                torch.cuda.synchronize()
                for k in range(3):
                    t0 = time.perf_counter()
                    st = sc.par_cast_device(cam, p, ptr, stream, want_stats=True)
                    torch.cuda.synchronize()
                    calls[k].append(((time.perf_counter() - t0) * 1e3, st["kernel_ms"]))
                sc.close()
            print("book1 %dx%dx%d box_camera %d (median of 5 fresh handles): " % (nx, ny, ns, mode) + "; ".join(
                "call %d wall %.3f ms, GPU-side %.3f ms" % (k + 1, statistics.median(w for w, _ in c), statistics.median(g for _, g in c))
                for k, c in enumerate(calls)))


if __name__ == "__main__":
    main()
