"""What scene option light_sampling costs and what it buys (include/rtiow_gpu.h, at rtg_scene_set_option), on an MI355X.

For the Cornell box and the book-2 final scene, the frame with the option off (the production ray-pool kernels) and on (the
one-lane-per-pixel kernels over color_ls), at the same sample count ns:
  kernel ms (median of --reps calls after a warm-up call, rtg_stats.kernel_ms) and Msamples/s;
  the summed variance of the pixel means (RTG_FLAG_SUM_SQUARES), over every pixel and channel;
  RMSE against a plain frame of --ref-spp samples (another seed), and the relative difference of the frame means;
  and at equal kernel time: the plain frame at ns x (ms on / ms off) samples, its kernel ms and RMSE.
The option's estimator has a heavy tail where a surface comes close to a light (no multiple importance sampling): the frame
mean at low ns reads low and single pixels spike, so the RMSE is given with and without the pixels whose reference is >= 1
(those that look into the light).

  python tools/light_sampling_cost.py                       # both scenes, 256 x 256 x 64, reference 8192 / 4096 spp
  python tools/light_sampling_cost.py --out profiles/NAME   # where light_sampling_cost.{json,txt} go
  python tools/light_sampling_cost.py --tail                # the tail probe instead: Cornell and volume_test, 64 x 64, the option at
                                                            # 64 (three seeds) / 1 024 (two) / 16 384 spp against 16 384 plain spp -- frame z per
                                                            # channel, relative difference of the frame mean, worst 8 x 8 block, brightest
                                                            # pixel mean; and the plain estimator at 64 / 1 024 spp for scale -> tail_probe.txt
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

SCENES = {
    "cornell": (lambda pkg, b, nx, ny: pkg.scenes.cornell_box_scene(b, nx, ny), 8192),
    "book2": (lambda pkg, b, nx, ny: pkg.scenes.book_final_scene(b, nx, ny, pkg.small_rng.SmallRng(0xDEADBEEF)), 4096),
}


def render(scene, cam, nx, ny, ns, seed, reps):
    """(planes [2, ny, nx, 3], median kernel ms) of `reps` timed calls after one warm-up call."""
    ms = []
    for i in range(reps + 1):
        planes, st = scene.par_cast(cam, nx, ny, ns, seed=seed, squares=True, stats=True, counters=False)
        if i:
            ms.append(st["kernel_ms"])
    return planes, float(np.median(ms))


def summed_variance(planes, ns):
    mean, q = planes[0].astype(np.float64), planes[1].astype(np.float64)
    return float((np.maximum(q - ns * mean * mean, 0.0) / (ns * (ns - 1.0))).sum())


def errors(img, ref):
    d = img.astype(np.float64) - ref
    dark = ref.max(axis=-1) < 1.0
    return {"rmse": float(np.sqrt((d * d).mean())), "rmse_without_light_pixels": float(np.sqrt((d[dark] ** 2).mean())),
            "mean_rel_diff": float((img.mean() - ref.mean()) / ref.mean())}


def block_z(a, ns_a, b, ns_b, block=8):
    """z scores between two divided two-plane frames over block x block pixel blocks and channels, and of the frame means."""
    def stats(p, ns):
        mean, q = p[0].astype(np.float64), p[1].astype(np.float64)
        return mean, np.maximum(q - ns * mean * mean, 0.0) / (ns * (ns - 1.0))
    (ma, va), (mb, vb) = stats(a, ns_a), stats(b, ns_b)
    ny, nx, _ = ma.shape

    def blocks(x):
        return x.reshape(ny // block, block, nx // block, block, 3).sum(axis=(1, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        zb = np.nan_to_num((blocks(ma) - blocks(mb)) / np.sqrt(blocks(va) + blocks(vb)))
    zf = (ma.sum((0, 1)) - mb.sum((0, 1))) / np.sqrt(va.sum((0, 1)) + vb.sum((0, 1)))
    return zb, zf, ma, mb


def tail_probe(pkg, gpu, out):
    nx = ny = 64
    big = 16384
    lines = []
    for name, fn in (("cornell", pkg.scenes.cornell_box_scene), ("volume", pkg.scenes.volume_test)):
        b = gpu.builder()
        world, cam, _ = fn(b, nx, ny)
        off, on = b.scene(world), b.scene(world)
        on.set_option("light_sampling", 1)
        a = off.par_cast(cam, nx, ny, big, seed=1, squares=True)
        lines.append("%s %d x %d against %d plain spp (seed 1)" % (name, nx, ny, big))
        for scene, tag, runs in ((on, "option", ((64, 2), (64, 3), (64, 4), (1024, 5), (1024, 6), (big, 7))), (off, "plain ", ((64, 2), (1024, 5)))):
            for ns, seed in runs:
                zb, zf, ma, mb = block_z(a, big, scene.par_cast(cam, nx, ny, ns, seed=seed, squares=True), ns)
                lines.append("  %s ns %5d seed %d: frame z %s, rel diff %s, block |z| max %.2f, max pixel mean %.1f" % (
                    tag, ns, seed, np.round(zf, 2), np.round((mb.mean((0, 1)) - ma.mean((0, 1))) / ma.mean((0, 1)), 4), np.abs(zb).max(), mb.max()))
        print("\n".join(lines[-9:]), flush=True)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "tail_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tail", action="store_true", help="the tail probe instead of the cost table")
    ap.add_argument("--scenes", default="cornell,book2")
    ap.add_argument("--nx", type=int, default=256)
    ap.add_argument("--ny", type=int, default=256)
    ap.add_argument("--ns", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=0, help="0: the scene's default")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_sampling"))
    a = ap.parse_args()
    pkg = graft.load_package()
    gpu = pkg.load()
    if a.tail:
        return tail_probe(pkg, gpu, a.out)
    nx, ny, ns = a.nx, a.ny, a.ns
    rows, lines = {}, []
    for name in a.scenes.split(","):
        fn, ref_spp = SCENES[name]
        ref_spp = a.ref_spp or ref_spp
        b = gpu.builder()
        world, cam, _ = fn(pkg, b, nx, ny)
        off, on = b.scene(world), b.scene(world)
        on.set_option("light_sampling", 1)
        ref = off.par_cast(cam, nx, ny, ref_spp, seed=1).astype(np.float64)
        p_off, ms_off = render(off, cam, nx, ny, ns, 2, a.reps)
        p_on, ms_on = render(on, cam, nx, ny, ns, 2, a.reps)
        ns_eq = max(2, int(round(ns * ms_on / ms_off)))
        p_eq, ms_eq = render(off, cam, nx, ny, ns_eq, 2, a.reps)
        r = rows[name] = {
            "nx": nx, "ny": ny, "ns": ns, "ref_spp": ref_spp,
            "off": {"kernel_ms": ms_off, "msamples_per_s": nx * ny * ns / ms_off / 1e3, "summed_variance": summed_variance(p_off, ns), **errors(p_off[0], ref)},
            "on": {"kernel_ms": ms_on, "msamples_per_s": nx * ny * ns / ms_on / 1e3, "summed_variance": summed_variance(p_on, ns), **errors(p_on[0], ref)},
            "off_equal_time": {"ns": ns_eq, "kernel_ms": ms_eq, "summed_variance": summed_variance(p_eq, ns_eq), **errors(p_eq[0], ref)},
        }
        lines.append("%s %d x %d, reference %d spp" % (name, nx, ny, ref_spp))
        for k in ("off", "on", "off_equal_time"):
            v = r[k]
            lines.append("  %-15s ns %6d  %9.2f ms  %8.1f Msamples/s  summed variance %10.4g  RMSE %.4f (without light pixels %.4f)  frame mean %+.2f %%" % (
                k, v.get("ns", ns), v["kernel_ms"], nx * ny * v.get("ns", ns) / v["kernel_ms"] / 1e3, v["summed_variance"], v["rmse"],
                v["rmse_without_light_pixels"], 100 * v["mean_rel_diff"]))
        lines.append("  variance off / on at equal ns: %.2f; kernel time on / off: %.1f" % (
            r["off"]["summed_variance"] / r["on"]["summed_variance"], ms_on / ms_off))
        print("\n".join(lines[-5:]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "light_sampling_cost.json"), "w") as f:
        json.dump(rows, f, indent=1)
    with open(os.path.join(a.out, "light_sampling_cost.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
