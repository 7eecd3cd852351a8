"""Box tree (csrc/rt_box_plan.h box_tree_rebuild): production launches of the lean pool kernel stage a program
whose Bvh regions are rebuilt over the reference's leaf order -- the same leaf boxes and spheres in the same order, other
interior boxes above them -- because the proof of box pruning never uses the shape of the tree.  CPU tests: the structure
of the production program (rtg_debug_production_program) recomputed here, and the float32 model walk of test_box_prune, which
must return the same (best, winning sphere) and, mapped through `origin`, the same Sphere::hit sequence as the reference
program, hostile rays included.  GPU tests: option box_tree 0 / 1 give the same bits and the oracle's frame and counters;
with box_prune 2 (counting launches walk the production image) aabb_tests alone changes.

aabb_tests at box_prune 2: strictly below box_tree 0 on book-1 and on book1_sah, where the CPU model predicts a cut; equal
to the oracle's on big_lean, whose image does not fit LDS (the global-memory walk gets no production program).  The hand-built
and dome worlds have 2 to 51 leaves: there the greedy tree may be the reference's own (nested_pair: two leaves), so the two
values are printed and the five counters that may not move are asserted."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from scene_cases import CASES, build_case
from test_box_chains import HAND_BUILT, camera, followers, random_dome_world
from test_box_prune import (COUNTERS, FOLLOWER, KEPT, OP_BOX, OP_SPHERE, PRUNED, WORLD_NAMES, _worlds, leaf_run_heads,
                            model_rays, planes, program, prunable_records, walk)

NEW = 0xffffffff
FIVE = ("samples", "prim_tests", "shaded_hits", "rays", "draws")
_cache = {}


def production(pkg, name):
    """(production words, origin, mask over them) of a world, made once per session"""
    if name not in _cache:
        b = pkg.load().builder()
        _cache[name] = b.production_program(_worlds(pkg)[name](pkg, b))
    return _cache[name]


# ---- structure -----------------------------------------------------------------------------------------------------

def check_structure(words, prod, origin):
    """Every property a production program must have against its reference program `words`; raises AssertionError."""
    n = len(words)
    assert prod.shape == words.shape and origin.shape == (n,)
    ops = prod[:, 7] & 0xff
    skip = prod[:, 6].astype(np.int64)
    assert np.array_equal(np.bincount(ops, minlength=3), np.bincount(words[:, 7] & 0xff, minlength=3))   # (m - 1 nodes over m leaf pairs, as before)
    open_ = []                                              # skip pointers nest and point forward
    for j in range(n):
        while open_ and open_[-1] <= j:
            open_.pop()
        if ops[j] == OP_BOX:
            assert j < skip[j] < n and (not open_ or skip[j] <= open_[-1]), j
            open_.append(int(skip[j]))
    # the spheres in the reference's order, each behind its unchanged leaf box
    sph = np.nonzero(ops == OP_SPHERE)[0]
    assert np.array_equal(origin[sph].astype(np.int64), np.nonzero((words[:, 7] & 0xff) == OP_SPHERE)[0])
    assert (np.diff(origin[sph].astype(np.int64)) > 0).all()
    for j in sph:
        assert np.array_equal(prod[j], words[origin[j]]), j
        ref_leaf = origin[j] > 0 and (words[origin[j] - 1, 7] & 0xff) == OP_BOX and words[origin[j] - 1, 6] == origin[j] + 1
        if ref_leaf:
            assert origin[j - 1] == origin[j] - 1 and skip[j - 1] == j + 1, j
            assert np.array_equal(prod[j - 1, [0, 1, 2, 3, 4, 5, 7]], words[origin[j] - 1, [0, 1, 2, 3, 4, 5, 7]]), j
    # new interior boxes: finite, binary, bitwise the min / max of their two children (the first of equal values)
    mn, mx = planes(prod)
    new = np.nonzero(origin == NEW)[0]
    inside = np.zeros(n, dtype=bool)
    for j in new:
        assert ops[j] == OP_BOX and np.isfinite(mn[j]).all() and np.isfinite(mx[j]).all(), j
        L = j + 1
        R = int(skip[L])
        assert ops[L] == OP_BOX and ops[R] == OP_BOX and L < R < skip[j] and skip[R] == skip[j], j
        lo = np.where(mn[R] < mn[L], mn[R], mn[L])
        hi = np.where(mx[R] > mx[L], mx[R], mx[L])
        assert np.array_equal(lo.view(np.uint32), mn[j].view(np.uint32)) and np.array_equal(hi.view(np.uint32), mx[j].view(np.uint32)), j
        inside[j:skip[j]] = True
    # everything else is a copy; outside the rebuilt regions nothing moved
    old = np.nonzero(origin != NEW)[0]
    assert (origin[~inside] == np.nonzero(~inside)[0]).all()
    assert np.array_equal(prod[~inside], words[~inside])
    assert len(np.unique(origin[old])) == len(old)
    return inside


def check_mask(prod, mask):
    ops = prod[:, 7] & 0xff
    assert sorted(np.nonzero(mask == FOLLOWER)[0].tolist()) == followers(prod)
    ok = prunable_records(prod)
    assert ok[mask == PRUNED].all()
    assert (ops[mask != KEPT] == OP_BOX).all()
    assert not (mask[(ops == OP_BOX) & (np.roll(ops, -1) == OP_SPHERE)] == PRUNED).any()    # leaf boxes stay
    for h in leaf_run_heads(prod):
        assert mask[h] == KEPT, h                                                            # rule (d)


@pytest.mark.parametrize("name", WORLD_NAMES)
def test_structure_of_the_production_program(pkg, name):
    words, _ = program(pkg, name)
    prod, origin, mask = production(pkg, name)
    inside = check_structure(words, prod, origin)
    check_mask(prod, mask)
    if name == "book1_1200":
        assert inside.sum() == len(words) - 1 and (origin == NEW).sum() == 484        # one region: all but END


def test_two_builders_give_the_same_program(pkg):
    for name in ("book1_1200", "dome_3", "fuzz_2"):
        b = pkg.load().builder()
        got = b.production_program(_worlds(pkg)[name](pkg, b))
        for a, e in zip(got, production(pkg, name)):
            assert np.array_equal(a, e), name
    words, _ = program(pkg, "book1_1200")
    for a, e in zip(pkg.load().builder().production_program(words=words), production(pkg, "book1_1200")):
        assert np.array_equal(a, e)                                                   # ... and so do the words alone


def test_other_programs_get_no_production_program(pkg):
    for make in (lambda b: pkg.scenes.cornell_box_scene(b, 32, 32)[0], lambda b: CASES["book2_bvh"][0](pkg, b, 32, 32)[0]):
        b = pkg.load().builder()
        world = make(b)
        words = b.flatten(world)[0]
        prod, origin, mask = b.production_program(world)
        assert np.array_equal(prod, words) and np.array_equal(origin, np.arange(len(words))) and not mask.any()


# ---- the model walk -------------------------------------------------------------------------------------------------

def mapped(res, origin):
    """(best bits, winning record, Sphere::hit rows) of a walk of the production program in the reference's record numbers"""
    best, win, seq, boxes = res
    o = origin.astype(np.int64)
    return best.view(np.uint32), np.where(win >= 0, o[np.maximum(win, 0)], -1), np.stack([seq[:, 0], o[seq[:, 1]]], axis=1), boxes


def assert_same_walk(got, ref, what):
    assert np.array_equal(got[0], ref[0].view(np.uint32)), what
    assert np.array_equal(got[1], ref[1]), what
    assert np.array_equal(got[2], ref[2]), what              # the same Sphere::hit calls, in the same order


@pytest.mark.parametrize("name", WORLD_NAMES)
def test_model_walk_of_the_production_program(pkg, name):
    words, today = program(pkg, name)
    prod, origin, mask = production(pkg, name)
    o, d, best0 = model_rays(words, 11 + len(words))
    none = np.zeros(len(words), dtype=bool)
    ref = walk(words, o, d, best0, none)
    assert len(ref[2]) > 0
    for what, drop in (("tree", none), ("followers", mask == FOLLOWER), ("pruned", mask == PRUNED), ("both", mask != KEPT)):
        got = mapped(walk(prod, o, d, best0, drop), origin)
        assert_same_walk(got, ref, (name, what))
    if name == "book1_1200":
        before = walk(words, o, d, best0, today != KEPT)[3]
        print("book-1 model walk: box tests reference %d, today's image %d, production image %d" % (ref[3], before, got[3]))
        assert got[3] < before < ref[3]


def test_the_checks_notice_swapped_leaves_and_a_shrunk_box(pkg):
    """The checks are able to fail: a production program whose sibling leaves are swapped is caught by the structure check and
    by the model walk, one whose interior box lies one ulp below a child by the structure check."""
    words, _ = program(pkg, "book1_1200")
    prod, origin, mask = production(pkg, "book1_1200")
    ops = prod[:, 7] & 0xff
    bad, bad_origin = prod.copy(), origin.copy()
    swaps = 0
    for j in np.nonzero(origin == NEW)[0]:
        if ops[j + 2] == OP_SPHERE and ops[j + 3] == OP_BOX and ops[j + 4] == OP_SPHERE and prod[j, 6] == j + 5:   # two leaf children
            cols = [0, 1, 2, 3, 4, 5, 7]                  # (a leaf box keeps its place's skip pointer)
            bad[np.ix_([j + 1, j + 3], cols)] = bad[np.ix_([j + 3, j + 1], cols)]
            bad[[j + 2, j + 4]] = bad[[j + 4, j + 2]]
            bad_origin[[j + 1, j + 3]] = bad_origin[[j + 3, j + 1]]
            bad_origin[[j + 2, j + 4]] = bad_origin[[j + 4, j + 2]]
            swaps += 1
    assert swaps > 10
    with pytest.raises(AssertionError):
        check_structure(words, bad, bad_origin)
    o, d, best0 = model_rays(words, 5)
    none = np.zeros(len(words), dtype=bool)
    ref = walk(words, o, d, best0, none)
    got = mapped(walk(bad, o, d, best0, none), bad_origin)
    assert not np.array_equal(got[2], ref[2])
    # an interior box one ulp short of its left child's max.x
    j = int(np.nonzero(origin == NEW)[0][40])
    bad = prod.copy()
    f = bad.view(np.float32)
    f[j, 1] = np.nextafter(f[j + 1, 1], np.float32(-np.inf))
    with pytest.raises(AssertionError):
        check_structure(words, bad, origin)


@pytest.mark.parametrize("damage", ["nan_min", "nan_max", "child_sticks_out", "inf_plane"])
def test_a_damaged_region_is_not_rebuilt(pkg, damage):
    """Edited reference programs: a NaN or infinite plane, or a child that sticks out of its box, ends the region there: that
    record and every box above it stay as they are, and what is rebuilt below still passes every check."""
    words, _ = program(pkg, "book1_1200")
    ops = words[:, 7] & 0xff
    interior = [j for j in range(len(words)) if ops[j] == OP_BOX and ops[j + 1] == OP_BOX]
    j = next(j for j in interior if 3 <= int((words[:j, 6] > j).sum()) <= 6 and words[j, 6] - j > 20)
    w = words.copy()
    f = w.view(np.float32)
    if damage == "nan_min":
        f[j, 0] = np.nan
    elif damage == "nan_max":
        f[j + 1, 3] = np.nan        # a plane of the left child
    elif damage == "inf_plane":
        f[j, 5] = np.inf
    else:
        f[j, 1] = np.nextafter(f[j + 1, 1], np.float32(-np.inf))
    prod, origin, mask = pkg.load().builder().production_program(words=w)
    up = [i for i in range(j) if ops[i] == OP_BOX and w[i, 6] > j]
    keep = up + [j]
    assert np.array_equal(prod[keep], w[keep]) and np.array_equal(origin[keep], keep)
    assert (origin == NEW).any()                       # (the regions below are still rebuilt)
    inside = check_structure(w, prod, origin)
    assert not inside[keep].any()
    if damage != "inf_plane":                          # (the library also asks for finite planes: stricter than prunable_records)
        check_mask(prod, mask)
    o, d, best0 = model_rays(w, 17)
    ref = walk(w, o, d, best0, np.zeros(len(w), dtype=bool))
    assert_same_walk(mapped(walk(prod, o, d, best0, mask != KEPT), origin), ref, damage)


# ---- GPU: the same bits, the oracle's counters ------------------------------------------------------------------------

def _render_0_1(scene, cam, nx, ny, ns):
    scene.set_option("box_tree", 0)
    off = scene.par_cast(cam, nx, ny, ns)
    scene.set_option("box_tree", 1)
    return off, scene.par_cast(cam, nx, ny, ns)


def _counting_walks(scene, cam, nx, ny, ns, ref, st_ref, what):
    """box_prune 2: counting launches walk the production image -- the frame and five counters are the oracle's; returns
    aabb_tests at box_tree (0, 1)"""
    scene.set_option("box_prune", 2)
    aabb = []
    for tree in (0, 1):
        scene.set_option("box_tree", tree)
        img, st = scene.par_cast(cam, nx, ny, ns, stats=True)
        assert_bit_equal(img, ref, "%s (counting launch, box_prune 2, box_tree %d)" % (what, tree))
        for k in FIVE:
            assert st[k] == st_ref[k], (what, tree, k, st[k], st_ref[k])
        aabb.append(st["aabb_tests"])
    scene.set_option("box_prune", 1)
    print("%s %dx%dx%d aabb_tests: oracle %d, box_prune 2 with box_tree 0 %d, with box_tree 1 %d" % (what, nx, ny, ns, st_ref["aabb_tests"], aabb[0], aabb[1]))
    return aabb


@pytest.mark.gpu
def test_book1_same_bits_counters_and_slices(pkg, gpu, oracle):
    nx, ny, ns = 64, 48, 6
    b = gpu.builder()
    world, cam, _ = pkg.scenes.random_scene(b, nx, ny)
    sc = b.scene(world)
    assert (b.production_program(world)[1] == NEW).sum() > 0
    bo = oracle.builder()
    world_o, cam_o, _ = pkg.scenes.random_scene(bo, nx, ny)
    ref, st_ref = bo.scene(world_o).par_cast(cam_o, nx, ny, ns, stats=True)
    for chains in (0, 1):
        for prune in (0, 1):
            sc.set_option("box_chains", chains)
            sc.set_option("box_prune", prune)
            off, on = _render_0_1(sc, cam, nx, ny, ns)
            assert_bit_equal(on, off, "book1 box_tree 1 vs 0 (box_chains %d, box_prune %d)" % (chains, prune))
            assert_bit_equal(on, ref, "book1 box_tree 1 vs oracle (box_chains %d, box_prune %d)" % (chains, prune))
    acc = np.zeros((ny, nx, 3), dtype=np.float32)      # slices of 3 + 3 against one call
    sc.par_cast(cam, nx, ny, 3, out=acc, sample_begin=0, resume=True, partial=True)
    sc.par_cast(cam, nx, ny, ns, out=acc, sample_begin=3, resume=True)
    assert_bit_equal(acc, ref, "book1 slices 3 + 3")
    img, st = sc.par_cast(cam, nx, ny, ns, stats=True)  # box_tree 1, box_prune 1: counting launches walk the full reference image
    assert_bit_equal(img, ref, "book1 counting launch")
    for k in COUNTERS:
        assert st[k] == st_ref[k], (k, st[k], st_ref[k])
    aabb = _counting_walks(sc, cam, nx, ny, ns, ref, st_ref, "book1")
    assert aabb[1] < aabb[0] < st_ref["aabb_tests"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_hand_built_scenes_same_bits(pkg, gpu, oracle, name):
    nx, ny, ns = 32, 24, 8
    b = gpu.builder()
    sc = b.scene(HAND_BUILT[name][0](pkg, b))
    cam = camera(pkg, gpu, nx, ny)
    off, on = _render_0_1(sc, cam, nx, ny, ns)
    bo = oracle.builder()
    ref, st_ref = bo.scene(HAND_BUILT[name][0](pkg, bo)).par_cast(camera(pkg, oracle, nx, ny), nx, ny, ns, stats=True)
    assert_bit_equal(on, off, name)
    assert_bit_equal(on, ref, name + " (oracle)")
    _counting_walks(sc, cam, nx, ny, ns, ref, st_ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_random_dome_worlds_same_bits_and_counters(pkg, gpu, oracle, seed):
    nx, ny, ns = 32, 24, 6
    n = 5 + 9 * seed
    b = gpu.builder()
    sc = b.scene(random_dome_world(pkg, b, 1000 + seed, n))
    cam = camera(pkg, gpu, nx, ny)
    off, on = _render_0_1(sc, cam, nx, ny, ns)
    bo = oracle.builder()
    ref, st_ref = bo.scene(random_dome_world(pkg, bo, 1000 + seed, n)).par_cast(camera(pkg, oracle, nx, ny), nx, ny, ns, stats=True)
    assert_bit_equal(on, off, "seed %d" % seed)
    assert_bit_equal(on, ref, "seed %d (oracle)" % seed)
    _counting_walks(sc, cam, nx, ny, ns, ref, st_ref, "dome seed %d" % seed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["big_lean", "book1_sah"])
def test_scene_cases_same_bits(pkg, gpu, oracle, name):
    sg, cam, nx, ny, ns = build_case(pkg, gpu, name)
    off, on = _render_0_1(sg, cam, nx, ny, ns)
    so, cam_o, _, _, _ = build_case(pkg, oracle, name)
    ref, st_ref = so.par_cast(cam_o, nx, ny, ns, stats=True)
    assert_bit_equal(on, off, name)
    assert_bit_equal(on, ref, name + " (oracle)")
    _, st = sg.par_cast(cam, nx, ny, ns, stats=True)
    for k in COUNTERS:
        assert st[k] == st_ref[k], (name, k, st[k], st_ref[k])
    aabb = _counting_walks(sg, cam, nx, ny, ns, ref, st_ref, name)
    if name == "big_lean":      # 3000 spheres: the image cannot fit LDS, the global-memory walk keeps the reference program
        assert aabb[0] == aabb[1] == st_ref["aabb_tests"]
    else:
        assert aabb[1] < aabb[0]


@pytest.mark.gpu
def test_one_handle_switches_between_the_two_programs(pkg, gpu):
    nx, ny, ns = 64, 48, 4
    b = gpu.builder()
    world, cam, _ = pkg.scenes.random_scene(b, nx, ny)
    sc = b.scene(world)
    frames = []
    for tree in (1, 0, 1):
        sc.set_option("box_tree", tree)
        frames.append(sc.par_cast(cam, nx, ny, ns))
    assert_bit_equal(frames[1], frames[0], "box_tree 1 -> 0")
    assert_bit_equal(frames[2], frames[0], "box_tree 1 -> 0 -> 1")
