"""Camera plan (DESIGN.md 3 "Camera plan", csrc/rt_box_plan.h BOX_PLAN_COUNTS; scene option box_camera): the launcher plans the
interior boxes a (scene, camera) pair leaves out from pass counts that a probe kernel gathers for that camera.  The tree DP does
not care where its counts come from, and every subset of the choosable records is a sound plan -- so these CPU tests hand the DP
(rtg_debug_camera_plan) hostile counts as well as real ones and ask of every mask what test_box_tree asks of the scene's own:
the structure conditions, and the float32 model walk of test_box_prune returning the reference program's (best, winning record,
Sphere::hit sequence).  The DP's optimality is checked against brute force under the header's cost formula on the small worlds,
and on book-1 by what it is for: fewer modelled box tests than the scene's plan on camera paths it was not planned on.  A
stand-alone g++ program runs box_plan on book-1's words under -fsanitize=address,undefined."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_box_chains import followers
from test_box_prune import (F_TRANSLATE, FOLLOWER, KEPT, OP_BOX, OP_SPHERE, PRUNED, T_NEAR, WORLD_NAMES, leaf_run_heads, model_rays,
                            planes, program, prunable_records, walk)
from test_box_tree import assert_same_walk, check_mask, mapped, production

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtiow-rust_amd", "csrc")
KINDS = ("zero", "all", "above", "random", "rising")
MAT_DIFFUSE_LIGHT, F_MATKIND_SHIFT = 3, 16


def hostile_counts(prod, kind, seed):
    """(counts, n_rays): no count at all; every box passed by every ray; counts above the ray count; random ones; counts that
    rise from every parent to its children, which no walk produces (a child is only tested when its parent passed)."""
    n = len(prod)
    rs = np.random.RandomState(seed)
    if kind == "zero":
        return np.zeros(n, dtype=np.uint32), 0
    if kind == "all":
        return np.full(n, 4096, dtype=np.uint32), 4096
    if kind == "above":
        return rs.randint(0, 1 << 31, n).astype(np.uint32), 1000
    if kind == "random":
        return rs.randint(0, 5001, n).astype(np.uint32), 5000
    return (np.arange(n, dtype=np.uint32) * 3 + 1), 3 * n + 1        # records come in depth-first order: a child behind its parent


def camera_mask(pkg, prod, counts, n_rays):
    return pkg.load().builder().camera_plan(prod, counts, n_rays)


@pytest.mark.parametrize("name", WORLD_NAMES)
def test_every_mask_is_sound_whatever_the_counts(pkg, name):
    words, _ = program(pkg, name)
    prod, origin, today = production(pkg, name)
    o, d, best0 = model_rays(words, 23 + len(words), n_rays=1500)
    ref = walk(words, o, d, best0, np.zeros(len(words), dtype=bool))
    assert len(ref[2]) > 0
    seen = set()
    for k, kind in enumerate(KINDS):
        counts, n_rays = hostile_counts(prod, kind, 100 * len(prod) + k)
        mask = camera_mask(pkg, prod, counts, n_rays)
        check_mask(prod, mask)           # pruned records are prunable ones, leaf boxes stay, rule (d) heads stay, followers win
        assert np.array_equal(mask == FOLLOWER, today == FOLLOWER), (name, kind)
        if mask.tobytes() in seen:       # (the same mask again: its walk is the one already compared)
            continue
        seen.add(mask.tobytes())
        assert_same_walk(mapped(walk(prod, o, d, best0, mask != KEPT), origin), ref, (name, kind))


def test_other_programs_get_no_camera_plan(pkg):
    b = pkg.load().builder()
    world, _, _ = pkg.scenes.cornell_box_scene(b, 32, 32)
    words = b.flatten(world)[0]
    assert not b.camera_plan(words, np.full(len(words), 7, dtype=np.uint32), 7).any()
    with pytest.raises(ValueError):
        b.camera_plan(words, np.zeros(3, dtype=np.uint32), 7)


# ---- the DP against brute force ---------------------------------------------------------------------------------------

def choosable_records(prod):
    """the prunable records without the rule (d) heads"""
    ok = prunable_records(prod)
    ok[list(leaf_run_heads(prod))] = False
    return ok


def plan_cost(prod, left_out, counts, n_rays):
    """The cost formula of csrc/rt_box_plan.h: every BOX that is not left out and is no follower executes one test per walk in
    which its nearest ancestor that is not left out passed (the ray count when there is none)."""
    ops = prod[:, 7] & 0xff
    fol = set(followers(prod))
    n_pass = np.minimum(counts.astype(np.int64), n_rays)
    cost, open_ = 0, []
    for j in range(len(prod)):
        while open_ and prod[open_[-1], 6] <= j:
            open_.pop()
        if ops[j] != OP_BOX:
            continue
        if not left_out[j] and j not in fol:
            up = [a for a in open_ if not left_out[a]]
            cost += int(n_pass[up[-1]]) if up else n_rays
        open_.append(j)
    return cost


# the hand-built and dome worlds whose subsets can be listed: at most 13 choosable records (dome_2 .. dome_5 have 22 to 49)
SMALL_WORLDS = [n for n in WORLD_NAMES if n.startswith("hand_")] + ["dome_0", "dome_1"]


@pytest.mark.parametrize("name", SMALL_WORLDS)
def test_the_dp_is_optimal_on_small_worlds(pkg, name):
    prod, _, _ = production(pkg, name)
    cand = np.nonzero(choosable_records(prod))[0]
    assert len(cand) <= 13, len(cand)
    fol = set(followers(prod))
    free = [int(j) for j in cand if j in fol]      # a choosable follower costs nothing either way, but decides whose count its children pay
    for k, kind in enumerate(("random", "rising", "above", "all", "zero")):
        counts, n_rays = hostile_counts(prod, kind, 7 * len(prod) + k)
        best = None
        for r in range(len(cand) + 1):
            for sub in itertools.combinations(cand.tolist(), r):
                left = np.zeros(len(prod), dtype=bool)
                left[list(sub)] = True
                c = plan_cost(prod, left, counts, n_rays)
                best = c if best is None else min(best, c)
        mask = camera_mask(pkg, prod, counts, n_rays)
        got = None
        for r in range(len(free) + 1):
            for sub in itertools.combinations(free, r):
                left = mask == PRUNED
                left[list(sub)] = True
                c = plan_cost(prod, left, counts, n_rays)
                got = c if got is None else min(got, c)
        assert got == best, (name, kind, got, best)


# ---- book-1: counts of camera paths --------------------------------------------------------------------------------

def walk_counts(words, o, d, drop):
    """test_box_prune.walk with the number of passes of every BOX record: (best, winning record, n_pass, box tests)"""
    n = len(words)
    ops = (words[:, 7] & 0xff).astype(np.int64)
    skip = words[:, 6].astype(np.int64)
    mn, mx = planes(words)
    sph = words[:, :4].copy().view(np.float32)
    tr = (words[:, 7] & F_TRANSLATE) != 0
    N = len(o)
    n_pass = np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        inv = (np.float32(1.0) / d).astype(np.float32)
        dd = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        pc = np.zeros(N, dtype=np.int64)
        best = np.full(N, np.finfo(np.float32).max, dtype=np.float32)
        win = np.full(N, -1, dtype=np.int64)
        box_tests = 0
        for _ in range(4 * n + 4):
            op = ops[pc]
            dr = (op == OP_BOX) & drop[pc]
            bx = np.nonzero((op == OP_BOX) & ~dr)[0]
            sp = np.nonzero(op == OP_SPHERE)[0]
            if not len(bx) and not len(sp) and not dr.any():
                break
            if len(bx):
                p = pc[bx]
                t0 = (mn[p] - o[bx]) * inv[bx]
                t1 = (mx[p] - o[bx]) * inv[bx]
                neg = inv[bx] < 0
                near, far = np.where(neg, t1, t0), np.where(neg, t0, t1)
                start = np.fmax(T_NEAR, np.fmax(np.fmax(near[:, 0], near[:, 1]), near[:, 2]))
                end = np.fmin(best[bx], np.fmin(np.fmin(far[:, 0], far[:, 1]), far[:, 2]))
                ok = end > start
                np.add.at(n_pass, p[ok], 1)
                pc[bx] = np.where(ok, p + 1, skip[p])
                box_tests += len(bx)
            if len(sp):
                p = pc[sp]
                lo_o = np.where(tr[p][:, None], o[sp] - sph[p, :3], o[sp])
                r, di, a = sph[p, 3], d[sp], dd[sp]
                b_ = lo_o[:, 0] * di[:, 0] + lo_o[:, 1] * di[:, 1] + lo_o[:, 2] * di[:, 2]
                c = lo_o[:, 0] * lo_o[:, 0] + lo_o[:, 1] * lo_o[:, 1] + lo_o[:, 2] * lo_o[:, 2] - r * r
                disc = b_ * b_ - a * c
                pos = disc > 0
                sq = np.sqrt(np.where(pos, disc, np.float32(0))).astype(np.float32)
                ta, tb = (-b_ - sq) / a, (-b_ + sq) / a
                ha = pos & (ta < best[sp]) & (ta >= T_NEAR)
                hb = pos & ~ha & (tb < best[sp]) & (tb >= T_NEAR)
                hit = ha | hb
                best[sp] = np.where(hit, np.where(ha, ta, tb), best[sp])
                win[sp] = np.where(hit, p, win[sp])
                pc[sp] = p + 1
            pc[dr] += 1
        else:
            raise AssertionError("the walk does not end")
    return best, win, n_pass, box_tests


def camera_paths(words, cam, n_paths, bounces, seed):
    """The rays of n_paths camera paths as the probe kernel walks them: one camera ray per stratum of the image, then up to
    `bounces` bounces along normal + in_unit_sphere, every material diffuse; a miss, the dome or an emitter ends a path.
    Returns (origins, directions) of all rays."""
    rs = np.random.RandomState(seed)
    f = lambda a: np.array(list(a), dtype=np.float32)
    origin, llc, hor, ver = f(cam.origin), f(cam.lower_left_corner), f(cam.horizontal), f(cam.vertical)
    gw = int(np.ceil(np.sqrt(n_paths * np.linalg.norm(hor) / np.linalg.norm(ver))))
    gh = (n_paths + gw - 1) // gw
    ix, iy = np.meshgrid(np.arange(gw), np.arange(gh))
    s = ((ix.ravel() + rs.rand(gw * gh)) / gw).astype(np.float32)
    t = ((iy.ravel() + rs.rand(gw * gh)) / gh).astype(np.float32)
    disc = rs.uniform(-1, 1, (gw * gh, 2))
    disc[(disc ** 2).sum(axis=1) >= 1] = 0
    off = (cam.lens_radius * (disc[:, :1] * f(cam.u) + disc[:, 1:] * f(cam.v))).astype(np.float32)
    o = (origin + off).astype(np.float32)
    d = (llc + s[:, None] * hor + t[:, None] * ver - origin - off).astype(np.float32)
    sph = words[:, :4].copy().view(np.float32)
    tr = (words[:, 7] & F_TRANSLATE) != 0
    emitter = ((words[:, 7] >> F_MATKIND_SHIFT) & 7) == MAT_DIFFUSE_LIGHT
    none = np.zeros(len(words), dtype=bool)
    all_o, all_d = [o], [d]
    for _ in range(bounces):
        best, win, _, _ = walk_counts(words, o, d, none)
        w = np.maximum(win, 0)
        go = (win >= 0) & (sph[w, 3] < 2000.0) & ~emitter[w]
        if not go.any():
            break
        o, d, best, w = o[go], d[go], best[go], w[go]
        p = (o + best[:, None] * d).astype(np.float32)
        nrm = (p - np.where(tr[w][:, None], sph[w, :3], 0.0)) / sph[w, 3:4]
        v = rs.uniform(-1, 1, (len(p), 3))
        while True:
            bad = (v ** 2).sum(axis=1) >= 1
            if not bad.any():
                break
            v[bad] = rs.uniform(-1, 1, (int(bad.sum()), 3))
        o, d = p, (nrm + v).astype(np.float32)
        all_o.append(o), all_d.append(d)
    return np.concatenate(all_o), np.concatenate(all_d)


_book1 = {}


def book1_camera_counts(pkg):
    """book-1's production program, today's mask, the benchmark camera's pass counts of 2048 paths and the camera mask"""
    if not _book1:
        prod, origin, today = production(pkg, "book1_1200")
        cam = pkg.scenes.random_scene(pkg.load().builder(), 1200, 800)[1]
        o, d = camera_paths(prod, cam, 2048, 3, 1)
        n_pass = walk_counts(prod, o, d, np.zeros(len(prod), dtype=bool))[2]
        _book1.update(prod=prod, origin=origin, today=today, cam=cam, counts=n_pass.astype(np.uint32), n_rays=len(o))
        _book1["mask"] = camera_mask(pkg, prod, _book1["counts"], len(o))
    return _book1


def test_book1_camera_plan_beats_todays_on_other_camera_paths(pkg):
    k = book1_camera_counts(pkg)
    prod, today, mask = k["prod"], k["today"], k["mask"]
    check_mask(prod, mask)
    o, d = camera_paths(prod, k["cam"], 2048, 3, 2)           # a second, disjoint ray set: other jitter, other bounce directions
    a = walk_counts(prod, o, d, today != KEPT)
    b = walk_counts(prod, o, d, mask != KEPT)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
    print("book-1, benchmark camera, %d rays of 2048 paths: %d records left out (today %d); modelled box tests per ray %.2f, today %.2f: ratio %.4f"
          % (len(o), int((mask == PRUNED).sum()), int((today == PRUNED).sum()), b[3] / len(o), a[3] / len(o), b[3] / a[3]))
    assert b[3] < a[3]
    # ... and on the planning set it is the optimum of the cost formula, so no worse than today's there either
    assert plan_cost(prod, mask == PRUNED, k["counts"], k["n_rays"]) <= plan_cost(prod, today == PRUNED, k["counts"], k["n_rays"])


# ---- box_plan on book-1's words under the sanitizers -------------------------------------------------------------------

PROGRAM = r"""
#include "rt_box_plan.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace rtg;

int main(int argc, char** argv) {
  if (argc < 2) return 3;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  uint32_t head[2];
  if (fread(head, 4, 2, f) != 2) return 3;
  const size_t n = head[0];
  const uint64_t n_rays = head[1];
  std::vector<uint32_t> words(8 * n), fol32(n), counts(n);
  if (fread(words.data(), 4, 8 * n, f) != 8 * n || fread(fol32.data(), 4, n, f) != n || fread(counts.data(), 4, n, f) != n) return 3;
  fclose(f);
  std::vector<uint32_t> lo(4 * n), hi(4 * n);
  std::vector<uint8_t> follower(n), mask(n), sure(n);
  for (size_t i = 0; i < n; i++) {
    for (int k = 0; k < 4; k++) lo[4 * i + k] = words[8 * i + k], hi[4 * i + k] = words[8 * i + 4 + k];
    follower[i] = (uint8_t)fol32[i];
  }
  auto L = reinterpret_cast<const uint32_t (*)[4]>(lo.data());
  auto H = reinterpret_cast<const uint32_t (*)[4]>(hi.data());
  uint64_t state = 12345;
  for (int kind = 0; kind < 6; kind++) {
    std::vector<uint32_t> c(counts);
    uint64_t rays = n_rays;
    for (size_t i = 0; i < n && kind > 0; i++) {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      c[i] = kind == 1 ? 0u : kind == 2 ? 777u : kind == 3 ? (uint32_t)(state >> 33) : kind == 4 ? (uint32_t)(3 * i + 1) : 0xffffffffu;
    }
    if (kind == 1) rays = 0;
    if (kind == 2) rays = 777;
    if (kind == 4) rays = 3 * n + 1;
    const BoxPlan p = box_plan(L, H, n, kind == 5 ? nullptr : follower.data(), mask.data(), sure.data(), 0u, BOX_PLAN_COUNTS, c.data(), rays);
    printf("kind %d: %u pruned, %u sure\n", kind, p.n_pruned, p.n_sure);
    if (kind == 0) {
      printf("MASK ");
      for (size_t i = 0; i < n; i++) putchar('0' + mask[i]);
      putchar('\n');
    }
  }
  box_plan(L, H, n, follower.data(), mask.data(), nullptr, 0u, BOX_PLAN_COUNTS, nullptr, 5);   // no counts: no pruned record
  for (size_t i = 0; i < n; i++)
    if (mask[i] == BOX_PRUNED) return 2;
  box_plan(L, H, 3, follower.data(), mask.data(), nullptr, 0u, BOX_PLAN_COUNTS, counts.data(), 5);   // too short to hold a node
  printf("OK\n");
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_box_plan_on_counts_under_the_sanitizers(pkg, tmp_path):
    k = book1_camera_counts(pkg)
    prod = k["prod"]
    fol = np.isin(np.arange(len(prod)), followers(prod)).astype(np.uint32)
    with open(tmp_path / "book1.bin", "wb") as f:
        np.array([len(prod), k["n_rays"]], dtype=np.uint32).tofile(f)
        np.ascontiguousarray(prod, dtype=np.uint32).tofile(f)
        fol.tofile(f)
        k["counts"].tofile(f)
    src = tmp_path / "camera_plan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "camera_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe), str(tmp_path / "book1.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout[-600:])
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout[-2000:]
    line = next(l for l in out.stdout.splitlines() if l.startswith("MASK "))
    assert line[5:] == "".join(str(int(v)) for v in k["mask"])       # the library's plan, from the same header


# ---- a counts plan may keep what the area plan leaves out ----------------------------------------------------------------

def row_of_four_words():
    """Four spheres of radius 0.5 in a row along x under a root box and two half boxes, as the flattener writes a Bvh."""
    OP_END, F_BVH_ROOT = 0, 1 << 13
    cx = [0.0, 1.2, 2.4, 3.6]
    w = np.zeros((12, 8), dtype=np.uint32)
    f = w.view(np.float32)

    def box(j, x0, x1, skip, flags=0):
        f[j, :6] = (x0, x1, -0.5, 0.5, -0.5, 0.5)
        w[j, 6], w[j, 7] = skip, OP_BOX | flags

    def sphere(j, x):
        f[j, :4] = (x, 0.0, 0.0, 0.5)
        w[j, 6], w[j, 7] = 0, OP_SPHERE | F_TRANSLATE
    box(0, cx[0] - 0.5, cx[3] + 0.5, 11, F_BVH_ROOT)
    box(1, cx[0] - 0.5, cx[1] + 0.5, 6)
    box(6, cx[2] - 0.5, cx[3] + 0.5, 11)
    for k, j in enumerate((2, 4, 7, 9)):
        box(j, cx[k] - 0.5, cx[k] + 0.5, j + 2)
        sphere(j + 1, cx[k])
    w[11, 7] = OP_END
    return w


def test_a_counts_plan_can_leave_out_fewer_records_than_the_scenes(pkg):
    """The area model leaves out a box that covers half of its parent; counts of rays that mostly fail the half boxes keep them.
    The camera's image of such a scene is LARGER than the scene's, which is why the launcher compares the two sizes before it
    stages a camera's table (csrc/rtg_launch.inc launch_pool)."""
    b = pkg.load().builder()
    prod, origin, today = b.production_program(words=row_of_four_words())
    ops = prod[:, 7] & 0xff
    interior = (ops == OP_BOX) & (np.roll(ops, -1) == OP_BOX)
    assert int(interior.sum()) == 3 and int((today == PRUNED).sum()) == 3          # root and both halves
    counts = np.where(interior, 470, 200).astype(np.uint32)
    counts[0] = 1000
    mask = b.camera_plan(prod, counts, 2000)
    check_mask(prod, mask)
    assert 0 < int((mask == PRUNED).sum()) < int((today == PRUNED).sum()), (mask, today)
    o, d, best0 = model_rays(prod, 3, n_rays=800)
    ref = walk(prod, o, d, best0, np.zeros(len(prod), dtype=bool))
    assert_same_walk(mapped(walk(prod, o, d, best0, mask != KEPT), np.arange(len(prod))), ref, "row of four")
