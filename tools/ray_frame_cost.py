#!/usr/bin/env python3
"""Cost of ray frames (include/rtiow_gpu_rays.h; GPU box) against camera frames, on one handle per scene and in one process.
Kernel time between the library's device events (stats: rtg_stats.kernel_ms, the fold kernel included), the variants
alternating, the median of --repeats launches each after one warm-up round.

  --part book1    book-1 at 1200 x 800 x 50:
                    (a) rtg_par_cast_device, the yardstick
                    (b) a ray frame of per-pixel pinhole rays through the pixel centres on the lean pool kernel (ray_pool 1)
                    (c) the same rays on the general kernel (ray_pool 0)
                  and at 8 spp, (b8) the rays of (b) against (d8) the same rays repeated to per-sample layout: what reading a ray
                  per sample costs.  Reports (b)/(a), (c)/(b), (d8)/(b8), and whether (b) and (c) gave the same bits.
  --part cornell  Cornell box at 300 x 300 x 100: rtg_par_cast_device against the general-kernel ray frame
  --part book2    book-2 at 300 x 300 x 100: the same -- the gap a ray frame on the full-feature schedules would close
Every part is one GPU step: run each under a time limit of its own."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

SEED = 0xDEADBEEF


def pinhole_rays(cam, nx, ny):
    """One ray per pixel from the camera's origin through the pixel's centre: float32 [nx * ny, 7], row 0 = top."""
    o, llc = np.array(list(cam.origin), np.float64), np.array(list(cam.lower_left_corner), np.float64)
    hor, ver = np.array(list(cam.horizontal), np.float64), np.array(list(cam.vertical), np.float64)
    row, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    u, v = ((x + 0.5) / nx).reshape(-1, 1), ((ny - 1 - row + 0.5) / ny).reshape(-1, 1)
    rays = np.zeros((nx * ny, 7), np.float32)
    rays[:, 0:3] = o
    rays[:, 3:6] = llc + u * hor + v * ver - o
    return rays


def spread(xs):
    return "median %.4f ms (min %.4f, max %.4f, max - min %.4f, %d launches)" % (statistics.median(xs), min(xs), max(xs), max(xs) - min(xs), len(xs))


def measure(plan, repeats):
    """plan: [(label, fn() -> kernel ms)], alternated; the first round is the warm-up."""
    ms = {label: [] for label, _ in plan}
    for rep in range(repeats + 1):
        for label, fn in plan:
            t = fn()
            if rep:
                ms[label].append(t)
    for label, _ in plan:
        print("%-44s %s" % (label, spread(ms[label])), flush=True)
    return {label: statistics.median(v) for label, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("book1", "cornell", "book2"), required=True)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    if args.repeats < 10:
        raise SystemExit("--repeats: at least 10 launches per variant")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ray_frame_cost.py measures on the GPU: no device")
    pkg = graft.load_package()
    gpu = pkg.load()
    capi = pkg.capi
    nx, ny, ns = (1200, 800, 50) if args.part == "book1" else (300, 300, 100)
    b = gpu.builder()
    if args.part == "book1":
        world, cam, _ = pkg.scenes.random_scene(b, nx, ny)
    elif args.part == "cornell":
        world, cam, _ = pkg.scenes.cornell_box_scene(b, nx, ny)
    else:
        world, cam, _ = pkg.scenes.book_final_scene(b, nx, ny, pkg.small_rng.SmallRng(0xDEADBEEF))
    sc = b.scene(world)
    rays = pinhole_rays(cam, nx, ny)
    d_rays = torch.from_numpy(rays).cuda()
    d_cam, d_ray = (torch.zeros((ny, nx, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    print("library %s; %s %d x %d x %d; %d repeats" % (gpu.path, args.part, nx, ny, ns, args.repeats), flush=True)

    def camera_frame(n):
        p = capi.make_params(nx, ny, n, seed=SEED)
        return lambda: sc.par_cast_device(cam, p, d_cam.data_ptr(), want_stats=True)["kernel_ms"]

    def ray_frame(route, n, d, per_sample=False):
        def fn():
            sc.set_option("ray_pool", route)
            return sc.cast_rays(d, nx, ny, n, per_sample=per_sample, seed=SEED, out=d_ray, stats=True)[1]["kernel_ms"]
        return fn

    if args.part != "book1":
        m = measure([("(a) rtg_par_cast_device", camera_frame(ns)), ("(c) ray frame, general kernel", ray_frame(0, ns, d_rays))], args.repeats)
        print("%s: general-kernel ray frame / camera frame = %.2f" % (args.part, m["(c) ray frame, general kernel"] / m["(a) rtg_par_cast_device"]))
        return
    m = measure([("(a) rtg_par_cast_device", camera_frame(ns)), ("(b) ray frame per pixel, lean pool kernel", ray_frame(1, ns, d_rays)),
                 ("(c) ray frame per pixel, general kernel", ray_frame(0, ns, d_rays))], args.repeats)
    a, bb, c = m["(a) rtg_par_cast_device"], m["(b) ray frame per pixel, lean pool kernel"], m["(c) ray frame per pixel, general kernel"]
    print("book1: (b)/(a) = %.3f, (c)/(b) = %.2f" % (bb / a, c / bb))
    frames = {}
    for route in (1, 0):   # the same bits from both kernels, at the size timed
        sc.set_option("ray_pool", route)
        frames[route] = sc.cast_rays(d_rays, nx, ny, ns, seed=SEED).cpu().numpy()
    print("book1: lean pool kernel == general kernel, bit for bit: %s; mean radiance %.4f" % (frames[0].tobytes() == frames[1].tobytes(), frames[1].mean()))
    n8 = 8
    d_tiled = d_rays.repeat(n8, 1).contiguous()
    torch.cuda.synchronize()
    m = measure([("(b8) per-pixel rays, 8 spp, lean pool kernel", ray_frame(1, n8, d_rays)),
                 ("(d8) per-sample rays, 8 spp, lean pool kernel", ray_frame(1, n8, d_tiled, True))], args.repeats)
    print("book1: (d8)/(b8) = %.3f" % (m["(d8) per-sample rays, 8 spp, lean pool kernel"] / m["(b8) per-pixel rays, 8 spp, lean pool kernel"]))
    sc.set_option("ray_pool", 1)
    same = sc.cast_rays(d_tiled, nx, ny, n8, per_sample=True, seed=SEED).cpu().numpy().tobytes() == sc.cast_rays(d_rays, nx, ny, n8, seed=SEED).cpu().numpy().tobytes()
    print("book1: per-sample == per-pixel rays at 8 spp, bit for bit: %s" % same)


if __name__ == "__main__":
    main()
