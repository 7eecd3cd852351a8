"""What a background costs, and what dropping the dome buys (include/rtiow_gpu.h RTG_FLAG_BACKGROUND; run on an MI355X).  The
method is tools/features_cost.py's: alternating calls after one warm-up call of each, medians and ranges of rtg_stats.kernel_ms
over --reps calls, in a child process under a time limit.

On C2's frame (book-1 1200x800x50) three cases through rtg_par_cast:
  dome      the scene as bench.py renders it: the world wrapped in FlipNormals(Sphere{10000, DiffuseLight}), no flag
  constant  the world without the dome and a constant background of the dome's emission -- the same image: checked bit for bit
            against the dome BEHIND the Bvh (the list world [Bvh(objects), dome], rendered once, not timed), which it equals by
            construction.  With the dome INSIDE the Bvh the tree is another one, and closest hits are tree-invariant only up to
            rounding in the box tests: the pixels that differ from that frame are counted and reported
  gradient  the world without the dome and the book's gradient sky
and, with RTG_FLAG_COUNTERS in calls of their own (the instrumented variant, not timed), each case's counters: the dome is one
more record in every walk and ends every escaping path with a sphere test.

  python tools/background_cost.py
  python tools/background_cost.py --nx 300 --ny 200 --ns 10 --reps 3
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

STEP_TIMEOUT_S = 420
BOOK_SKY = {"bottom": (1.0, 1.0, 1.0), "top": (0.5, 0.7, 1.0)}


def call(scene, cam, p, frame):
    """One rtg_par_cast into `frame` with an rtg_stats: (kernel_ms, the stats as a dict)."""
    capi = sys.modules["rtiow_rust_amd"].capi
    st = capi.Stats.new()
    scene.be.check(scene.be._par_cast(scene.h, C.byref(cam), C.byref(p), frame.buf.ctypes.data_as(capi.c_f32p), C.byref(st)))
    return st.kernel_ms, st.as_dict()


def spread(ts):
    return {"median": round(float(np.median(ts)), 3), "range": [round(min(ts), 3), round(max(ts), 3)]}


def measure(nx, ny, ns, reps):
    pkg = graft.load_package()
    gpu = pkg.load()
    capi, S = pkg.capi, pkg.scenes
    b = gpu.builder()
    world, cam, _ = S.random_scene(b, nx, ny)
    with_dome = b.scene(world)
    b2 = gpu.builder()
    world2, _, _, sky = S.random_scene(b2, nx, ny, sky="background")
    without = b2.scene(world2)
    b3 = gpu.builder()
    objs = S.random_scene_objects(b3, pkg.small_rng.SmallRng(0xDEADBEEF), dome=False)
    dome = b3.flip_normals(b3.sphere(10000.0, b3.diffuse_light(b3.constant(S.v(*S.DOME_COLOUR)), 1.0)))
    behind, behind_frame = b3.scene([b3.bvh(objs, (0.0, 1.0)), dome]), capi.Frame(nx, ny)
    call(behind, cam, capi.make_params(nx, ny, ns), behind_frame)
    cases = {
        "dome": (with_dome, capi.Frame(nx, ny), {}),
        "constant": (without, capi.Frame(nx, ny, background=sky), {"background": True}),
        "gradient": (without, capi.Frame(nx, ny, background=BOOK_SKY), {"background": True}),
    }
    t = {name: [] for name in cases}
    for rep in range(reps + 1):
        for name, (scene, frame, flags) in cases.items():
            ms, _ = call(scene, cam, capi.make_params(nx, ny, ns, **flags), frame)
            if rep:   # (the first round is the warm-up)
                t[name].append(ms)
    counters = {}
    for name, (scene, frame, flags) in cases.items():
        _, st = call(scene, cam, capi.make_params(nx, ny, ns, flags=capi.FLAG_COUNTERS, **flags), frame)
        counters[name] = {k: st[k] for k in ("aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")}
    const_bits = cases["constant"][1].planes.view(np.uint32)
    same = bool(np.array_equal(const_bits, behind_frame.planes.view(np.uint32)))
    differ = int((const_bits != cases["dome"][1].planes.view(np.uint32)).any(axis=-1).sum())
    base = float(np.median(t["dome"]))
    out = {"frame": "book-1 %dx%dx%d" % (nx, ny, ns), "reps": reps,
           "kernel_ms": {name: dict(spread(ts), vs_dome_percent=round(100.0 * (float(np.median(ts)) - base) / base, 2)) for name, ts in t.items()},
           "counters": counters, "records": {"dome": with_dome.info()["instructions"], "without": without.info()["instructions"]},
           "constant_equals_dome_behind_the_bvh_bit_for_bit": same, "pixels_differing_from_dome_inside_the_bvh": differ}
    print(json.dumps(out), flush=True)
    if not same:
        raise SystemExit("the constant background's frame differs from the frame of the dome behind the Bvh")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nx", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=800)
    ap.add_argument("--ns", type=int, default=50)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        measure(args.nx, args.ny, args.ns, args.reps)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--nx", str(args.nx), "--ny", str(args.ny), "--ns", str(args.ns),
           "--reps", str(args.reps)]
    try:
        rc = subprocess.run(cmd, timeout=STEP_TIMEOUT_S).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit("background_cost: the measurement ran past %d s" % STEP_TIMEOUT_S)
    if rc != 0:
        raise SystemExit("background_cost: the measurement failed (exit status %d)" % rc)


if __name__ == "__main__":
    main()
