"""What a triangle mesh costs (include/rtiow_gpu_mesh.h; run on an MI355X).  The method is tools/image_texture_cost.py's:
alternating calls after one warm-up call of each, medians and ranges of rtg_stats.kernel_ms over --reps calls, in a child process
under a time limit.

  an icosphere of 320 / 5 120 / 81 920 triangles (2, 4 and 6 subdivisions), radius 90, at --nx x --ny x --ns (256 x 256 x 16)
    in the Cornell box, where the short box stood           (a list world of rects with the mesh's Bvh inside)
    alone under the book's gradient sky (RTG_FLAG_BACKGROUND)
  per mesh: the median-split Bvh against the SAH Bvh; scene option kernel = 1 (one lane per pixel) against 3 (the production
    choice: the full-feature pool kernel, or the lock-step kernel where launch_full_pool picks it); the analytic sphere of the
    same radius in the mesh's place as a yardstick; the host time of rtg_object_mesh; aabb_tests and prim_tests per ray from one instrumented call.

  --surface: the part for include/rtiow_gpu_surface.h instead -- in both worlds the 320-triangle icosphere flat against smooth (per-vertex
    normals) with the 81 920-triangle flat icosphere beside them, a planar image against the surface-mapped image on the same
    mesh, and the host time of rtg_object_mesh_attr.

  python tools/mesh_cost.py
  python tools/mesh_cost.py --surface
  python tools/mesh_cost.py --nx 64 --ny 64 --ns 4 --reps 2 --subdivisions 2 4
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


def measure(nx, ny, ns, reps, subdivisions, sah_max):
    pkg = graft.load_package()
    gpu = pkg.load()
    S, T = pkg.scenes, pkg.triangle

    def build(where, what, sub=0, sah=False):
        """(scene, camera, host seconds of the mesh call)"""
        b = gpu.builder()
        cam, _ = S._cornell_camera(gpu, nx, ny)
        world = S.cornell_box(b) if where == "cornell" else []
        white = b.lambertian(b.constant(S.vfrom(0.73)))
        took = 0.0
        if what == "mesh":
            v, f = T.icosphere(sub, RADIUS, CENTRE)
            t0 = time.perf_counter()
            world.append(b.mesh(v, f, white, sah=sah))
            took = time.perf_counter() - t0
        else:
            world.append(b.translate(S.v(*CENTRE), b.sphere(RADIUS, white)))
        return b.scene(world), cam, took

    out = {"frame": "%dx%dx%d" % (nx, ny, ns), "reps": reps, "worlds": {}}
    for where in ("cornell", "sky"):
        kw = {"background": SKY} if where == "sky" else {}
        cases = {"sphere": build(where, "sphere")}
        for sub in subdivisions:
            for sah in ((False, True) if 20 * 4 ** sub <= sah_max else (False,)):
                cases["ico%d_%s" % (20 * 4 ** sub, "sah" if sah else "median")] = build(where, "mesh", sub, sah)
        t = {(name, k): [] for name in cases for k in (1, 3)}
        for rep in range(reps + 1):
            for name, (sc, cam, _) in cases.items():
                for k in (1, 3):
                    sc.set_option("kernel", k)
                    _, st = sc.par_cast(cam, nx, ny, ns, stats=True, counters=False, **kw)
                    if rep:
                        t[(name, k)].append(st["kernel_ms"])
        rows = {}
        for name, (sc, cam, took) in cases.items():
            sc.set_option("kernel", 1)
            _, st = sc.par_cast(cam, nx, ny, ns, stats=True, **kw)
            rows[name] = {"kernel1_ms": spread(t[(name, 1)]), "kernel3_ms": spread(t[(name, 3)]), "host_build_s": round(took, 3),
                          "aabb_tests_per_ray": round(st["aabb_tests"] / max(1, st["rays"]), 2),
                          "prim_tests_per_ray": round(st["prim_tests"] / max(1, st["rays"]), 2), "records": sc.info()["instructions"]}
        out["worlds"][where] = rows
    print(json.dumps(out), flush=True)


def measure_surface(nx, ny, ns, reps):
    """The part for surface attributes: production kernels only (scene option kernel = 3)."""
    pkg = graft.load_package()
    gpu = pkg.load()
    S, T, I = pkg.scenes, pkg.triangle, pkg.image
    img = np.random.RandomState(3).rand(64, 64, 3).astype(np.float32)

    def build(where, sub, normals, texture):
        b = gpu.builder()
        cam, _ = S._cornell_camera(gpu, nx, ny)
        world = S.cornell_box(b) if where == "cornell" else []
        v, f, nn, uv = T.icosphere_attr(sub, RADIUS, CENTRE)
        if texture == "planar":
            mat = b.lambertian(b.image(img, I.planar((1.0 / 180.0, 0, 0), 0.0, (0, 1.0 / 180.0, 0), 0.0)))
        elif texture == "surface":
            mat = b.lambertian(b.surface(b.image(img, I.planar((1, 0, 0), 0.0, (0, 1, 0), 0.0))))
        else:
            mat = b.lambertian(b.constant(S.vfrom(0.73)))
        t0 = time.perf_counter()
        world.append(b.mesh(v, f, mat, normals=nn if normals else None, uvs=uv if texture == "surface" else None))
        took = time.perf_counter() - t0
        return b.scene(world), cam, took

    out = {"frame": "%dx%dx%d" % (nx, ny, ns), "reps": reps, "worlds": {}}
    for where in ("cornell", "sky"):
        kw = {"background": SKY} if where == "sky" else {}
        cases = {"ico320_flat": build(where, 2, False, None), "ico320_smooth": build(where, 2, True, None),
                 "ico81920_flat": build(where, 6, False, None), "ico320_planar_image": build(where, 2, False, "planar"),
                 "ico320_surface_image": build(where, 2, False, "surface"), "ico81920_smooth_surface_image": build(where, 6, True, "surface")}
        t = {name: [] for name in cases}
        for rep_ in range(reps + 1):
            for name, (sc, cam, _) in cases.items():
                sc.set_option("kernel", 3)
                _, st = sc.par_cast(cam, nx, ny, ns, stats=True, counters=False, **kw)
                if rep_:
                    t[name].append(st["kernel_ms"])
        out["worlds"][where] = {name: {"kernel3_ms": spread(t[name]), "host_build_s": round(took, 3), "records": sc.info()["instructions"]}
                                for name, (sc, cam, took) in cases.items()}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nx", type=int, default=256)
    ap.add_argument("--ny", type=int, default=256)
    ap.add_argument("--ns", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--subdivisions", type=int, nargs="+", default=[2, 4, 6])
    ap.add_argument("--sah-max", type=int, default=81920, help="largest mesh that also gets a SAH Bvh")
    ap.add_argument("--surface", action="store_true", help="the part for include/rtiow_gpu_surface.h")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child and args.surface:
        measure_surface(args.nx, args.ny, args.ns, args.reps)
        return
    if args.child:
        measure(args.nx, args.ny, args.ns, args.reps, args.subdivisions, args.sah_max)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--nx", str(args.nx), "--ny", str(args.ny), "--ns", str(args.ns),
           "--reps", str(args.reps), "--sah-max", str(args.sah_max), "--subdivisions"] + [str(s) for s in args.subdivisions] + (["--surface"] if args.surface else [])
    try:
        rc = subprocess.run(cmd, timeout=STEP_TIMEOUT_S).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit("mesh_cost: the measurement ran past %d s" % STEP_TIMEOUT_S)
    if rc != 0:
        raise SystemExit("mesh_cost: the measurement failed (exit status %d)" % rc)


if __name__ == "__main__":
    main()
