"""What a flagged frame costs through rtg_par_cast_multi (scene option multi_planes; include/rtiow_gpu.h at rtg_par_cast_multi; run
on an MI355X).  The book-1 frame at 1200 x 800, 50 samples in slices of 10, with RTG_FLAG_SUM_SQUARES + SAMPLE_COUNTS + RETIRE
(radius 1) + DENOISE (5, 2) + FEATURES (grid 2, traced in the first slice only): once through rtg_par_cast on one handle, then
through rtg_par_cast_multi with 1, 2, 4 and 8 handles spread over the devices the host has (with one device they share it, and
the output says so).

Per configuration, averaged over the slices of one frame after one warm-up frame: the host wall time around the synchronous
call, rtg_stats.kernel_ms, and the pack + unpack kernels' event time (the library reports it under scene option verbose) with
the bytes they move -- words_per_pixel x work items x 4, read and written once by each of the two -- as GB/s.  Every slice's
frame must be word-equal to the one-handle call's.

Every configuration runs in a child process of its own under a time limit; the first that fails ends the run.

  python tools/multi_planes_cost.py --out profiles/r14_multi_planes/multi_planes_cost.txt
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

NX, NY, NS, STEP = 1200, 800, 50, 10
RETIRE = {"target_se": 0.02, "min_samples": 10, "radius": 1}
DENOISE = {"k": 0.7, "radius": 5, "patch": 2}
STEP_TIMEOUT_S = 300
VERBOSE_LINE = re.compile(r"\[rtg\] multi planes: .* (\d+) words per pixel, (\d+) work items packed \((\d+) bytes\), (\d+) through RCCL; "
                          r"pack ([0-9.]+) ms, unpack ([0-9.]+) ms")


def frame_of(pkg):
    capi = pkg.capi
    f = capi.features_frame(NX, NY, squares=True, counts=True, retire=True, denoise=DENOISE, features={"grid": 2})
    f.retire.target_se, f.retire.min_samples, f.retire.radius = RETIRE["target_se"], RETIRE["min_samples"], RETIRE["radius"]
    f.counts[...] = NS
    return f


def run_config(n):
    """One configuration in this process: n = 0 is rtg_par_cast on one handle, n > 0 rtg_par_cast_multi with n handles."""
    pkg = graft.load_package()
    gpu = pkg.load()
    n_dev = gpu.device_count()
    scenes = []
    for i in range(max(n, 1)):
        b = gpu.builder()
        world, cam, _ = pkg.scenes.random_scene(b, NX, NY)
        scenes.append(b.scene(world, device=i % n_dev if n else 0))
    if n:
        scenes[0].set_option("multi_planes", 1)
    rows = []
    for rep in range(3):   # (the first frame is the warm-up, the second is timed, the third reports the pack / unpack events)
        if n:
            scenes[0].set_option("verbose", 1 if rep == 2 else 0)
        f = frame_of(pkg)
        for begin in range(0, NS, STEP):
            end = begin + STEP
            f.features.compute = 1 if begin == 0 else 0
            kw = dict(sample_begin=begin, resume=begin > 0, partial=end < NS, stats=True, counters=False)
            t0 = time.perf_counter()
            if n:
                _, st = gpu.par_cast_multi(scenes, cam, NX, NY, end, out=f, **kw)
            else:
                _, st = scenes[0].par_cast(cam, NX, NY, end, out=f, features=True, denoise=True, squares=True, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            if rep == 1:
                rows.append({"end": end, "wall_ms": wall, "kernel_ms": st["kernel_ms"], "samples": st["samples"],
                             "retired": f.retire.retired, "sha256": hashlib.sha256(f.buf.tobytes()).hexdigest()})
    print(json.dumps({"handles": n, "devices": n_dev, "slices": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--handles", default="1,2,4,8")
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--config", type=int, help="(internal) run one configuration in this process")
    a = ap.parse_args()
    if a.config is not None:
        return run_config(a.config)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("book-1 %d x %d, %d samples in slices of %d: SUM_SQUARES + SAMPLE_COUNTS + RETIRE (radius %d) + DENOISE (%d, %d) + FEATURES (grid 2, first slice)"
        % (NX, NY, NS, STEP, RETIRE["radius"], DENOISE["radius"], DENOISE["patch"]))
    ref = None
    for n in [0] + [int(v) for v in a.handles.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--config", str(n)]
        try:
            r = subprocess.run(cmd, timeout=STEP_TIMEOUT_S, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit("configuration %d ran past %d s: stopping" % (n, STEP_TIMEOUT_S))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit("configuration %d ended with status %d: stopping" % (n, r.returncode))
        res = json.loads(r.stdout.strip().splitlines()[-1])
        rows = res["slices"]
        if ref is None:
            ref = [row["sha256"] for row in rows]
            say("devices found: %d%s" % (res["devices"], " (the handles of every multi configuration share it)" if res["devices"] == 1 else ""))
        equal = [row["sha256"] for row in rows] == ref
        mean = lambda k: sum(row[k] for row in rows) / len(rows)   # noqa: E731
        what = "rtg_par_cast, one handle" if n == 0 else "rtg_par_cast_multi, %d handle(s) on %d device(s)" % (n, min(n, res["devices"]))
        say("%-52s wall %8.3f ms  kernel_ms %8.3f  per slice (mean of %d); frames word-equal to one handle: %s"
            % (what, mean("wall_ms"), mean("kernel_ms"), len(rows), "yes" if equal else "NO"))
        packs = [VERBOSE_LINE.search(ln) for ln in r.stderr.splitlines()]
        packs = [m for m in packs if m]
        if packs:
            ms = sum(float(m.group(5)) + float(m.group(6)) for m in packs) / len(packs)
            moved = sum(int(m.group(3)) for m in packs) / len(packs) * 4   # pack: read + write; unpack: read + write
            say("%-52s pack + unpack %.4f ms per slice, %.1f MB read + written, %.1f GB/s; words per pixel by slice: %s; RCCL transfers per slice: %s"
                % ("", ms, moved / 1e6, moved / 1e6 / ms if ms > 0 else 0.0, " ".join(m.group(1) for m in packs), " ".join(m.group(4) for m in packs)))
        elif n:
            say("%-52s nothing packed: the one handle's pixels already stand in the first device's frame" % "")
        if not equal:
            raise SystemExit("configuration %d: a frame differs from the one-handle call's" % n)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
