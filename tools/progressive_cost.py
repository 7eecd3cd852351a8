"""What slicing a frame costs (include/rtiow_gpu.h RTG_FLAG_PARTIAL / RTG_FLAG_RESUME): the same frame rendered in one
rtg_par_cast_device call and in n equal slices, back to back on one stream into one device buffer (no previews, no host
copies), timed with HIP events around the whole sequence; median of --reps after one warm-up.  Every sliced frame is
checked bit for bit against the one-call frame.

  python tools/progressive_cost.py                 # C2 (book-1 1200x800x50): 1, 5 and 50 slices; C4 (book-2 800x800x1000): 1 and 10
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
    "C2": (lambda pkg, b, nx, ny: pkg.scenes.random_scene(b, nx, ny), 1200, 800, 50, (1, 5, 50)),
    "C4": (lambda pkg, b, nx, ny: pkg.scenes.book_final_scene(b, nx, ny, pkg.small_rng.SmallRng(0xDEADBEEF)), 800, 800, 1000, (1, 10)),
}


def hip_runtime():
    """The HIP runtime librtiow_gpu.so links: device buffers, a stream and events without a second runtime in the process."""
    hip = C.CDLL("libamdhip64.so")
    for name, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipMemcpy", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
                       ("hipFree", [C.c_void_p]), ("hipStreamCreate", [C.POINTER(C.c_void_p)]), ("hipEventCreate", [C.POINTER(C.c_void_p)]),
                       ("hipEventRecord", [C.c_void_p, C.c_void_p]), ("hipEventSynchronize", [C.c_void_p]),
                       ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p])):
        getattr(hip, name).argtypes = args
    return hip


def ok(rc, what):
    if rc != 0:
        raise SystemExit("%s failed: %d" % (what, rc))


def render(scene, capi, cam, nx, ny, ns, n_slices, out, stream):
    step = ns // n_slices
    begin = 0
    for i in range(n_slices):
        end = ns if i == n_slices - 1 else begin + step
        p = capi.make_params(nx, ny, end, sample_begin=begin, resume=True, partial=end != ns)
        scene.par_cast_device(cam, p, out, stream)
        begin = end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="C2,C4")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pkg = graft.load_package()
    gpu = pkg.load()
    hip = hip_runtime()
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipStreamCreate(C.byref(stream)) or hip.hipEventCreate(C.byref(e0)) or hip.hipEventCreate(C.byref(e1)), "stream / events")
    for name in a.frames.split(","):
        fn, nx, ny, ns, slicings = FRAMES[name]
        b = gpu.builder()
        world, cam, _ = fn(pkg, b, nx, ny)
        scene = b.scene(world)
        out = C.c_void_p()
        ok(hip.hipMalloc(C.byref(out), nx * ny * 3 * 4), "hipMalloc")
        ref = None
        for n in slicings:
            render(scene, pkg.capi, cam, nx, ny, ns, n, out, stream)   # warm-up (allocations, occupancy queries)
            times = []
            for _ in range(a.reps):
                ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
                render(scene, pkg.capi, cam, nx, ny, ns, n, out, stream)
                ok(hip.hipEventRecord(e1, stream) or hip.hipEventSynchronize(e1), "hipEventRecord / Synchronize")
                ms = C.c_float()
                ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
                times.append(ms.value)
            img = np.empty((ny, nx, 3), dtype=np.float32)
            ok(hip.hipMemcpy(img.ctypes.data, out, img.nbytes, 2), "hipMemcpy")
            if ref is None:
                ref = img.copy()
            same = bool(np.array_equal(img.view(np.uint32), ref.view(np.uint32)))
            ms = float(np.median(times))
            print(json.dumps({"frame": "%s %dx%dx%d" % (name, nx, ny, ns), "slices": n, "ms": round(ms, 2),
                              "ms_min": round(min(times), 2), "ms_max": round(max(times), 2),
                              "bit_equal_to_one_call": same}), flush=True)
            if not same:
                raise SystemExit("sliced frame differs from the one-call frame")
        hip.hipFree(out)


if __name__ == "__main__":
    main()
