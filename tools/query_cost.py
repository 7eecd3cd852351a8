#!/usr/bin/env python3
"""Cost of the ray queries (include/rtiow_gpu_query.h; GPU box) on book-1, on two ray sets of 960 000 rays each:
  primary    the 1200 x 800 primary rays of the benchmark camera (features.subpixel_rays, grid 1)
  secondary  secondary-like rays between random points of the scene's volume, as tests/probe_rays.py builds them
Closest hit asks both as they are; any-hit asks the primary rays with t_max = f32::MAX and the secondary rays with t_max = 1
(is the segment's far end visible from its near end?).

  query_cost.py [--repeats R]            wall time of Scene.closest_hit / Scene.occluded on torch tensors (enqueue + one stream
                                         synchronise) at query_lds 2 and 0, of Scene.debug_hit_top on the same rays (host arrays:
                                         three allocations, the copies and a device-wide synchronise per call), the kernels' own
                                         time from device events (stats=True), and the crossover sweep: lean against general
                                         kernel from 1 024 rays upward
  query_cost.py --profile [--repeats R]  the launches alone, in a fixed order, for a run under
                                         `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/query_cost.py --profile`
  query_cost.py --parse DIR              per kernel and ray set, min / median / max of the durations in DIR's kernel trace
With RTIOW_GPU_LIB pointing at a build without the query entry points (the parent's), only debug_hit_top is run: that is how the
parent's debug_hit_top_kernel is measured on the same rays.  The secondary set is generated from a fixed seed."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

NX, NY = 1200, 800
F32_MAX = np.float32(3.402823466e+38)
SEED = 77
KERNELS = ("query_lean_kernel<false>", "query_lean_kernel<true>", "query_closest_kernel", "query_occluded_kernel", "debug_hit_top_kernel")


def ray_sets(pkg, cam):
    primary = np.ascontiguousarray(pkg.features.subpixel_rays(cam, NX, NY, 1).reshape(-1, 7))
    n = len(primary)
    rs = np.random.RandomState(99)
    lo, hi = np.array([-12, 0, -12.0]), np.array([12, 3, 12.0])
    a, b = lo + rs.rand(n, 3) * (hi - lo), lo + rs.rand(n, 3) * (hi - lo)
    secondary = np.concatenate([a, (b - a) * rs.rand(n, 1) * 2, rs.rand(n, 1)], axis=1).astype(np.float32)
    t_max = {"primary": np.full((n, 1), F32_MAX, np.float32), "secondary": np.ones((n, 1), np.float32)}
    return {"primary": primary, "secondary": secondary}, t_max


def spread(xs):
    return "min %.4f median %.4f max %.4f (max - min %.4f, %d runs)" % (min(xs), statistics.median(xs), max(xs), max(xs) - min(xs), len(xs))


def parse(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    if not rows:
        raise SystemExit("no kernel trace under " + d)
    for k in KERNELS:
        ms = [(e - s) * 1e-6 for s, e, name in rows if k.replace(" ", "") in name.replace(" ", "")]
        if not ms:
            continue
        # the launches of one kernel: the primary set's (1 warm-up + R), then the secondary set's
        half = len(ms) // 2
        for label, part in (("primary", ms[1:half]), ("secondary", ms[half + 1:])):
            print("%-28s %-9s kernel ms: %s" % (k, label, spread(part)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--parse")
    args = ap.parse_args()
    if args.parse:
        return parse(args.parse)
    import torch
    pkg = graft.load_package()
    gpu = pkg.load()
    has_query = hasattr(gpu.lib, "rtg_query_closest")
    b = gpu.builder()
    world, cam, _ = pkg.scenes.random_scene(b, NX, NY)
    sc = b.scene(world)
    sets, t_max = ray_sets(pkg, cam)
    R = args.repeats
    print("library %s; %d rays per set; %d repeats" % (gpu.path, len(sets["primary"]), R))

    def sync():
        torch.cuda.synchronize()

    def wall(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    for label in ("primary", "secondary"):
        rays = sets[label]
        if has_query:
            d7 = torch.from_numpy(rays).cuda()
            d8 = torch.from_numpy(np.concatenate([rays, t_max[label]], axis=1)).cuda()
            plan = [("closest query_lds 2", 2, lambda st=False: sc.closest_hit(d7, seed=SEED, stats=st)),
                    ("closest query_lds 0", 0, lambda st=False: sc.closest_hit(d7, seed=SEED, stats=st)),
                    ("occluded query_lds 2", 2, lambda st=False: sc.occluded(d8, seed=SEED, stats=st)),
                    ("occluded query_lds 0", 0, lambda st=False: sc.occluded(d8, seed=SEED, stats=st))]
        else:
            plan = []
        plan.append(("debug_hit_top (host arrays)", None, lambda st=False: sc.debug_hit_top(rays, seed=SEED)))
        if args.profile:   # one warm-up + R launches of each, back to back
            for name, lds, fn in plan:
                if lds is not None:
                    sc.set_option("query_lds", lds)
                for _ in range(R + 1):
                    fn()
                sync()
            continue
        walls, kern = {name: [] for name, _, _ in plan}, {name: [] for name, _, _ in plan}
        for rep in range(R + 1):   # alternating; the first round is the warm-up
            for name, lds, fn in plan:
                if lds is not None:
                    sc.set_option("query_lds", lds)
                w = wall(fn)
                k = fn(True)[1]["kernel_ms"] if lds is not None else None
                if rep:
                    walls[name].append(w)
                    if k is not None:
                        kern[name].append(k)
        for name, _, _ in plan:
            print("%-9s %-28s wall ms: %s" % (label, name, spread(walls[name])))
            if kern[name]:
                print("%-9s %-28s kernel ms (device events): %s" % (label, name, spread(kern[name])))
        if has_query:   # the same bits from both kernels, at the size timed
            res = {}
            for lds in (0, 2):
                sc.set_option("query_lds", lds)
                out, mat = sc.closest_hit(d7, seed=SEED)
                res[lds] = (out.cpu().numpy().tobytes(), mat.cpu().numpy().tobytes(), sc.occluded(d8, seed=SEED).cpu().numpy().tobytes())
            own = sc.debug_hit_top(rays, seed=SEED)
            print("%-9s outputs: lean == general %s; closest == debug_hit_top %s; hits %d, occluded %d" % (
                label, res[0] == res[2], res[2][0] == own[0].tobytes() and res[2][1] == own[1].tobytes(),
                int((own[0][:, 0] != 0).sum()), int(np.frombuffer(res[2][2], np.uint8).sum())))
    if has_query and not args.profile:   # the lean kernel's refill threshold (option query_refill; 1 = a finished lane refills in the same trip)
        default = 16
        for label in ("primary", "secondary"):
            d7 = torch.from_numpy(sets[label]).cuda()
            d8 = torch.from_numpy(np.concatenate([sets[label], t_max[label]], axis=1)).cuda()
            sc.set_option("query_lds", 2)
            for refill in (1, 4, 8, 16, 24, 32, 48, 64):
                sc.set_option("query_refill", refill)
                c = [sc.closest_hit(d7, seed=SEED, stats=True)[1]["kernel_ms"] for _ in range(R + 1)][1:]
                o = [sc.occluded(d8, seed=SEED, stats=True)[1]["kernel_ms"] for _ in range(R + 1)][1:]
                print("refill %-9s query_refill %2d: closest %.4f ms (%.4f .. %.4f), occluded %.4f ms (%.4f .. %.4f)" % (
                    label, refill, statistics.median(c), min(c), max(c), statistics.median(o), min(o), max(o)))
            sc.set_option("query_refill", default)
    if has_query and not args.profile:   # crossover: from how many rays is the lean kernel the faster one?
        for label in ("primary", "secondary"):
            rays = sets[label]
            n = 1024
            while n <= len(rays):
                sub = torch.from_numpy(np.ascontiguousarray(rays[::len(rays) // n][:n])).cuda()
                ms = {}
                for lds in (0, 2):
                    sc.set_option("query_lds", lds)
                    t = [sc.closest_hit(sub, seed=SEED, stats=True)[1]["kernel_ms"] for _ in range(R + 1)][1:]
                    ms[lds] = (statistics.median(t), min(t), max(t))
                print("crossover %-9s %7d rays: general %.4f ms (%.4f .. %.4f), lean %.4f ms (%.4f .. %.4f)" % ((label, n) + ms[0] + ms[2]))
                n *= 2 if n < 65536 else 4
    sc.close()


if __name__ == "__main__":
    main()
