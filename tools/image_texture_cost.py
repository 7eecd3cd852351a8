"""What an image texture costs (include/rtiow_gpu_image.h; run on an MI355X).  The method is tools/background_cost.py's:
alternating calls after one warm-up call of each, medians and ranges of rtg_stats.kernel_ms over --reps calls, in a child process
under a time limit.

  book-1 at the benchmark frame (1200x800x50), the ground sphere's albedo as
    constant          the scene as bench.py renders it: a lean program on the lean pool kernel
    checker           a checker of the constant with itself: the same image on the full-feature pool kernel, which every
                      non-constant texture moves the scene to -- the fair baseline for the image rows
    image 1x1         nearest and bilinear: the sampler's arithmetic, every fetch the same texel
    image 2048x2048   nearest and bilinear: 64 MB of texels under a spherical mapping (the book's earth globe, as a ground)
  (every image is filled with the constant, so all six frames are the same image: checked bit for bit)
  the Cornell box (300x300x100) with its floor as a constant and as a 512x512 bilinear image
  rtg_debug_texture: wall time per point of the whole call (two copies and one kernel) for --points points, coherent (a
    raster over the image) and random, against the same call on a constant texture (the copies alone)

  python tools/image_texture_cost.py
  python tools/image_texture_cost.py --nx 300 --ny 200 --ns 10 --reps 3 --points 100000
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

STEP_TIMEOUT_S = 420
GROUND = (0.5, 0.5, 0.5)


class Swap:
    """A Builder whose constant(colour) makes something else where the colour is `match`."""

    def __init__(self, builder, match, make):
        self._b, self.match, self.make = builder, np.asarray(match, np.float32), make

    def __getattr__(self, name):
        return getattr(self._b, name)

    def constant(self, color):
        c = np.array([color[0], color[1], color[2]], np.float32)
        return self.make(self._b, c) if (c == self.match).all() else self._b.constant(color)


def call(scene, cam, p, frame):
    capi = sys.modules["rtiow_rust_amd"].capi
    st = capi.Stats.new()
    scene.be.check(scene.be._par_cast(scene.h, C.byref(cam), C.byref(p), frame.buf.ctypes.data_as(capi.c_f32p), C.byref(st)))
    return st.kernel_ms


def spread(ts):
    return {"median": round(float(np.median(ts)), 3), "range": [round(min(ts), 3), round(max(ts), 3)]}


def timed(cases, cam, p, reps):
    """cases: {name: (scene, frame)} -> {name: [kernel_ms]}, alternating, the first round a warm-up."""
    t = {name: [] for name in cases}
    for rep in range(reps + 1):
        for name, (scene, frame) in cases.items():
            ms = call(scene, cam, p, frame)
            if rep:
                t[name].append(ms)
    return t


def measure(nx, ny, ns, reps, points):
    pkg = graft.load_package()
    gpu = pkg.load()
    capi, S, I = pkg.capi, pkg.scenes, pkg.image

    def flat(w, h):
        return lambda c: np.broadcast_to(c, (h, w, 3)).copy()
    globe = I.spherical((0.0, -1000.0, 0.0))
    makers = {
        "constant": lambda b, c: b.constant(c),
        "checker": lambda b, c: b.checker(b.constant(c), b.constant(c)),
        "image_1x1_nearest": lambda b, c: b.image(flat(1, 1)(c), dict(globe, filter=I.NEAREST)),
        "image_1x1_bilinear": lambda b, c: b.image(flat(1, 1)(c), dict(globe, filter=I.BILINEAR)),
        "image_2048_nearest": lambda b, c: b.image(flat(2048, 2048)(c), dict(globe, filter=I.NEAREST)),
        "image_2048_bilinear": lambda b, c: b.image(flat(2048, 2048)(c), dict(globe, filter=I.BILINEAR)),
    }
    cases, cam = {}, None
    for name, make in makers.items():
        sb = Swap(gpu.builder(), GROUND, make)
        world, cam, _ = S.random_scene(sb, nx, ny)
        cases[name] = (sb.scene(world), capi.Frame(nx, ny))
    t = timed(cases, cam, capi.make_params(nx, ny, ns), reps)
    first = cases["constant"][1].planes.view(np.uint32)
    same = {name: bool(np.array_equal(first, f.planes.view(np.uint32))) for name, (_, f) in cases.items()}
    base, fair = float(np.median(t["constant"])), float(np.median(t["checker"]))
    book1 = {name: dict(spread(ts), vs_constant_percent=round(100.0 * (float(np.median(ts)) - base) / base, 2),
                        vs_checker_percent=round(100.0 * (float(np.median(ts)) - fair) / fair, 2),
                        hbm_bytes=cases[name][0].info()["hbm_bytes"]) for name, ts in t.items()}

    # the Cornell box, 300 x 300 x 100, its floor a material of its own
    cnx = cny = 300
    cns = 100
    cornell = {}
    rs = np.random.RandomState(1)
    tex = {"constant": lambda b: b.constant((0.5, 0.5, 0.5)),
           "image_512_bilinear": lambda b: b.image(rs.rand(512, 512, 3).astype(np.float32),
                                                   I.planar((1.0 / 555.0, 0, 0), 0.0, (0, 0, 1.0 / 555.0), 0.0, filter=I.BILINEAR))}
    ccam = None
    for name, make in tex.items():
        b = gpu.builder()
        world, ccam, _ = S.cornell_box_scene(b, cnx, cny)
        world[1] = b.rect(S.Y, (0.0, 555.0), (0.0, 555.0), 0.0, b.lambertian(make(b)))
        cornell[name] = (b.scene(world), capi.Frame(cnx, cny))
    tc = timed(cornell, ccam, capi.make_params(cnx, cny, cns), max(3, reps // 2))
    cbase = float(np.median(tc["constant"]))
    cornell_out = {name: dict(spread(ts), vs_constant_percent=round(100.0 * (float(np.median(ts)) - cbase) / cbase, 2)) for name, ts in tc.items()}

    # rtg_debug_texture per point
    b = gpu.builder()
    img = rs.rand(2048, 2048, 3).astype(np.float32)
    prm = I.planar((1, 0, 0), 0.0, (0, 1, 0), 0.0, filter=I.BILINEAR)
    t_img, t_con = b.image(img, prm), b.constant((0.1, 0.2, 0.3))
    sc = b.scene([b.sphere(1.0, b.lambertian(t_img))])
    side = int(np.sqrt(points))
    n = side * side
    yy, xx = np.meshgrid(np.arange(side, dtype=np.float32), np.arange(side, dtype=np.float32), indexing="ij")
    coherent = np.stack([(xx.ravel() + 0.5) / side, (yy.ravel() + 0.5) / side, np.zeros(n, np.float32)], axis=1).astype(np.float32)
    random = np.concatenate([rs.rand(n, 2), np.zeros((n, 1))], axis=1).astype(np.float32)
    probe = {}
    for name, tx, pts in (("image_coherent", t_img, coherent), ("image_random", t_img, random), ("constant_coherent", t_con, coherent)):
        sc.debug_texture(tx, pts[:1024])
        ts = []
        for _ in range(max(3, reps // 2)):
            t0 = time.perf_counter()
            sc.debug_texture(tx, pts)
            ts.append((time.perf_counter() - t0) * 1e9 / n)
        probe[name] = {"ns_per_point": spread(ts), "points": n}

    out = {"book1": {"frame": "book-1 %dx%dx%d" % (nx, ny, ns), "reps": reps, "kernel_ms": book1, "same_frame_as_constant": same},
           "cornell": {"frame": "Cornell %dx%dx%d" % (cnx, cny, cns), "kernel_ms": cornell_out},
           "debug_texture": probe}
    print(json.dumps(out), flush=True)
    if not all(same.values()):
        raise SystemExit("a frame with a constant-filled image differs from the constant's frame")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nx", type=int, default=1200)
    ap.add_argument("--ny", type=int, default=800)
    ap.add_argument("--ns", type=int, default=50)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--points", type=int, default=1 << 22)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        measure(args.nx, args.ny, args.ns, args.reps, args.points)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--nx", str(args.nx), "--ny", str(args.ny), "--ns", str(args.ns),
           "--reps", str(args.reps), "--points", str(args.points)]
    try:
        rc = subprocess.run(cmd, timeout=STEP_TIMEOUT_S).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit("image_texture_cost: the measurement ran past %d s" % STEP_TIMEOUT_S)
    if rc != 0:
        raise SystemExit("image_texture_cost: the measurement failed (exit status %d)" % rc)


if __name__ == "__main__":
    main()
