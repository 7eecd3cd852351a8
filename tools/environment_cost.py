"""What an environment costs (include/rtiow_gpu_environment.h; run on an MI355X).  The method is tools/mesh_cost.py's: alternating
calls after one warm-up call of each, medians and ranges of rtg_stats.kernel_ms (HIP events) over --reps calls, in a child
process under a time limit.

  book-1 at --nx x --ny x --ns (1200 x 800 x 50): what leaving the lean pool costs
    as shipped, with the dome, on the lean pool kernel
    without the dome under RTG_FLAG_BACKGROUND (the book's gradient), on the lean pool kernel
    without the dome under a constant environment, a 1 x 1 image, and a 2048 x 1024 sun_sky image with the nearest and the
      bilinear filter: all on the full-feature pool kernel
  the mesh scene of tools/mesh_cost.py (the 320-triangle smooth icosphere alone) at 256 x 256 x 16 under the gradient flag
    against the same sun_sky image environment: the same kernel family, so the price of the lookup alone
  the probe: rtg_debug_environment per direction, wall time of the call (copies included), 4 M coherent and 4 M random directions

  python tools/environment_cost.py
  python tools/environment_cost.py --nx 300 --ny 200 --ns 10 --reps 2 --sky 256 128 --probe 65536
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

STEP_TIMEOUT_S = 540
RADIUS, CENTRE = 90.0, (212.5, 90.0, 147.5)
SKY = {"bottom": (1.0, 1.0, 1.0), "top": (0.5, 0.7, 1.0)}


def spread(ts):
    return {"median": round(float(np.median(ts)), 3), "range": [round(min(ts), 3), round(max(ts), 3)]}


def alternate(cases, nx, ny, ns, reps):
    """cases: name -> (scene, camera, render keywords).  One warm-up call of each, then reps rounds over all of them."""
    t = {name: [] for name in cases}
    for rep in range(reps + 1):
        for name, (sc, cam, kw) in cases.items():
            _, st = sc.par_cast(cam, nx, ny, ns, stats=True, counters=False, **kw)
            if rep:
                t[name].append(st["kernel_ms"])
    return {name: {"kernel_ms": spread(ts), "records": cases[name][0].info()["instructions"]} for name, ts in t.items()}


def measure(nx, ny, ns, reps, sky_w, sky_h, probe_n):
    pkg = graft.load_package()
    gpu = pkg.load()
    S, T, I, E = pkg.scenes, pkg.triangle, pkg.image, pkg.environment
    sky = E.sun_sky(sky_w, sky_h)
    out = {"frame": "%dx%dx%d" % (nx, ny, ns), "reps": reps, "sky": "%dx%d" % (sky_w, sky_h)}

    def book1(env):
        b = gpu.builder()
        if env == "dome":
            world, cam, _ = S.random_scene(b, nx, ny)
            return b.scene(world), cam, {}
        world, cam, _, _ = S.random_scene(b, nx, ny, sky="background")
        if env == "flag":
            return b.scene(world), cam, {"background": SKY}
        if env == "constant":
            b.environment(b.constant(S.DOME_COLOUR))
        elif env == "image1x1":
            b.environment(b.image(np.array(S.DOME_COLOUR, np.float32).reshape(1, 1, 3), E.lat_long_params()))
        else:
            b.environment(b.image(sky, E.lat_long_params(filter=I.NEAREST if env == "sky_nearest" else I.BILINEAR)))
        return b.scene(world), cam, {}

    cases = {"dome (lean pool)": book1("dome"), "gradient flag (lean pool)": book1("flag"), "constant environment": book1("constant"),
             "1x1 image environment": book1("image1x1"), "sun_sky nearest": book1("sky_nearest"), "sun_sky bilinear": book1("sky_bilinear")}
    out["book1"] = alternate(cases, nx, ny, ns, reps)
    del cases

    def mesh(env):
        b = gpu.builder()
        cam, _ = S._cornell_camera(gpu, 256, 256)
        v, f, nn, _ = T.icosphere_attr(2, RADIUS, CENTRE)
        world = [b.mesh(v, f, b.lambertian(b.constant(S.vfrom(0.73))), normals=nn)]
        if env:
            b.environment(b.image(sky, E.lat_long_params()))
        return b.scene(world), cam, ({} if env else {"background": SKY})

    out["mesh 256x256x16"] = alternate({"gradient flag": mesh(False), "sun_sky bilinear": mesh(True)}, 256, 256, 16, reps)

    # the probe: coherent = the camera-like sweep of a lat-long grid, random = shuffled
    b = gpu.builder()
    b.environment(b.image(sky, E.lat_long_params()))
    sc = b.scene([b.sphere(1.0, b.lambertian(b.constant((0.5, 0.5, 0.5))))])
    side = int(np.sqrt(probe_n))
    d = E.texel_directions(side, side).reshape(-1, 3).astype(np.float32)
    rows = {}
    for name, dirs in (("coherent", d), ("random", d[np.random.RandomState(1).permutation(len(d))])):
        sc.debug_environment(dirs[:1024])
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            sc.debug_environment(dirs)
            ts.append((time.perf_counter() - t0) * 1e3)
        rows[name] = {"directions": len(dirs), "call_ms": spread(ts), "ns_per_direction": round(float(np.median(ts)) * 1e6 / len(dirs), 3)}
    out["probe (wall time of the call, copies included)"] = rows
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nx", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=800)
    ap.add_argument("--ns", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sky", type=int, nargs=2, default=[2048, 1024], metavar=("W", "H"))
    ap.add_argument("--probe", type=int, default=1 << 22, help="directions per probe call")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        measure(args.nx, args.ny, args.ns, args.reps, args.sky[0], args.sky[1], args.probe)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--nx", str(args.nx), "--ny", str(args.ny), "--ns", str(args.ns),
           "--reps", str(args.reps), "--sky", str(args.sky[0]), str(args.sky[1]), "--probe", str(args.probe)]
    try:
        rc = subprocess.run(cmd, timeout=STEP_TIMEOUT_S).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit("environment_cost: the measurement ran past %d s" % STEP_TIMEOUT_S)
    if rc != 0:
        raise SystemExit("environment_cost: the measurement failed (exit status %d)" % rc)


if __name__ == "__main__":
    main()
