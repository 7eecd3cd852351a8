"""Box pruning (csrc/rt_box_plan.h): production launches of the lean pool kernel leave out of the LDS image the
interior BOX records of a plan -- boxes of binary Bvh nodes that contain both children's boxes, all the way down -- because a
leaf box that passes implies that every box above it passed.  CPU tests: the library's mask (rtg_debug_box_plan) against the
follower rule and the soundness conditions recomputed here, and a float32 numpy model of the walk (aabb.rs:18-29,
object.rs:84-111) that must test the same spheres in the same order and return the same (best, winning record) with and
without the pruned records, hostile rays included.  GPU tests: option box_prune 0 / 1 give the same bits and the oracle's
image and counters; box_prune 2 (counting launches walk the pruned image) changes aabb_tests alone."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from scene_cases import CASES, build_case
from test_box_chains import HAND_BUILT, camera, followers, random_dome_world

OP_END, OP_BOX, OP_SPHERE = 0, 1, 2
F_TRANSLATE = 1 << 8
KEPT, FOLLOWER, PRUNED = 0, 1, 2
LEAN_CASES = ("big_lean", "book1", "book1_list", "book1_sah")   # the scene cases whose program is BOX / SPHERE / END
T_NEAR = np.float32(0.001)


# ---- worlds ---------------------------------------------------------------------------------------------------------

def book1_world(pkg, b):
    return pkg.scenes.random_scene(b, 1200, 800)[0]


def lean_fuzz_world(pkg, b, seed):
    """Spheres of very different radii (bare, translated, flipped), some at list level, the rest under a Bvh (built the
    reference's way or by SAH) that may hold a nested Bvh and an enclosing sphere."""
    S = pkg.scenes
    rs = np.random.RandomState(seed)
    mats = [b.lambertian(b.constant(S.v(0.7, 0.3, 0.2))), b.metal(S.v(0.8, 0.8, 0.9), 0.1), b.dielectric(1.5)]

    def sphere(i):
        r = float(np.float32(10.0 ** rs.uniform(-1.5, 0.7)))
        o = b.sphere(r, mats[i % 3])
        if rs.rand() < 0.85:
            c = rs.uniform(-6, 6, 3).astype(np.float32)
            o = b.translate(S.v(float(c[0]), float(c[1]), float(c[2])), o)
        return b.flip_normals(o) if rs.rand() < 0.1 else o
    n = int(rs.randint(3, 40))
    objs = [sphere(i) for i in range(n)]
    if rs.rand() < 0.5:
        objs.append(b.bvh([sphere(i) for i in range(int(rs.randint(1, 9)))], (0.0, 1.0)))
    if rs.rand() < 0.6:
        objs.append(b.flip_normals(b.sphere(10000.0, b.diffuse_light(b.constant(S.v(0.7, 0.8, 1.0)), 1.0))))
    top = [sphere(i) for i in range(int(rs.randint(0, 3)))]
    tree = b.bvh_sah(objs, (0.0, 1.0)) if rs.rand() < 0.3 else b.bvh(objs, (0.0, 1.0))
    return top + [tree]


def _worlds(pkg):
    """name -> world builder (pkg, b): every scene the CPU tests walk"""
    w = {"book1_1200": book1_world}
    for name in sorted(HAND_BUILT):
        w["hand_" + name] = HAND_BUILT[name][0]
    for seed in range(6):
        w["dome_%d" % seed] = lambda pkg, b, seed=seed: random_dome_world(pkg, b, 1000 + seed, 5 + 9 * seed)
    for name in LEAN_CASES:
        w["case_" + name] = lambda pkg, b, name=name: CASES[name][0](pkg, b, CASES[name][1], CASES[name][2])[0]
    for seed in range(8):
        w["fuzz_%d" % seed] = lambda pkg, b, seed=seed: lean_fuzz_world(pkg, b, 7000 + seed)
    return w


WORLD_NAMES = sorted(_worlds(None))
_cache = {}


def program(pkg, name):
    """(words, mask) of a world, flattened and planned once per session"""
    if name not in _cache:
        b = pkg.load().builder()
        world = _worlds(pkg)[name](pkg, b)
        words, feat = b.flatten(world)
        assert feat == 0, name
        _cache[name] = (words, b.box_plan(world))
    return _cache[name]


# ---- the soundness conditions, recomputed --------------------------------------------------------------------------

def planes(words):
    """(min [n, 3], max [n, 3]) of every record read as a BOX: lo = (min.x, max.x, min.y, max.y), hi = (min.z, max.z, ..)"""
    f = words[:, :6].copy().view(np.float32)
    return f[:, 0::2], f[:, 1::2]


def prunable_records(words):
    """Records that MAY be pruned: a BOX j with L = j + 1 a BOX, R = skip[L] a BOX, L < R < skip[j], skip[R] == skip[j]; no
    plane of j, L, R NaN; j's box contains L's and R's; L and R each a leaf box (BOX, SPHERE, skip behind it) or prunable."""
    n = len(words)
    ops = words[:, 7] & 0xff
    skip = words[:, 6].astype(np.int64)
    mn, mx = planes(words)
    ok = np.zeros(n, dtype=bool)

    def leaf(j):
        return ops[j] == OP_BOX and j + 2 < n and ops[j + 1] == OP_SPHERE and skip[j] == j + 2
    for j in range(n - 2, -1, -1):
        if ops[j] != OP_BOX or ops[j + 1] != OP_BOX:
            continue
        L = j + 1
        R = int(skip[L])
        if not (L < R < skip[j]) or ops[R] != OP_BOX or skip[R] != skip[j]:
            continue
        if np.isnan(mn[[j, L, R]]).any() or np.isnan(mx[[j, L, R]]).any():
            continue
        if not ((mn[j] <= mn[L]).all() and (mn[j] <= mn[R]).all() and (mx[j] >= mx[L]).all() and (mx[j] >= mx[R]).all()):
            continue
        ok[j] = (leaf(L) or ok[L]) and (leaf(R) or ok[R])
    return ok


def ancestors(words, j):
    """the BOX records whose [i + 1, skip) range holds record j"""
    ops = words[:, 7] & 0xff
    return [i for i in range(j) if ops[i] == OP_BOX and words[i, 6] > j]


@pytest.mark.parametrize("name", WORLD_NAMES)
def test_mask_is_followers_plus_sound_records(pkg, name):
    words, mask = program(pkg, name)
    ops = words[:, 7] & 0xff
    assert len(mask) == len(words) and set(np.unique(mask)) <= {KEPT, FOLLOWER, PRUNED}
    assert sorted(np.nonzero(mask == FOLLOWER)[0].tolist()) == followers(words)      # value 1: today's rule, unchanged
    ok = prunable_records(words)
    assert ok[mask == PRUNED].all(), np.nonzero((mask == PRUNED) & ~ok)[0]
    leaf_box = (ops == OP_BOX) & (np.roll(ops, -1) == OP_SPHERE)
    assert not (mask[leaf_box] == PRUNED).any()                                      # leaf boxes stay
    assert (ops[mask != KEPT] == OP_BOX).all()


def leaf_run_heads(words):
    """Records right in front of a run of followers that ends in a LEAF box.  Such a follower is left out because the record
    in front of its run, bitwise the same box, has just passed -- so that record must stay in the walk (rule (d))."""
    ops = words[:, 7] & 0xff
    fol = set(followers(words))
    heads = set()
    for j in fol:
        if ops[j + 1] == OP_SPHERE:
            h = j - 1
            while h in fol:
                h -= 1
            heads.add(h)
    return heads


@pytest.mark.parametrize("name", WORLD_NAMES)
def test_the_box_in_front_of_a_follower_leaf_stays(pkg, name):
    words, mask = program(pkg, name)
    for h in leaf_run_heads(words):
        assert mask[h] == KEPT, (name, h)


def test_book1_counts_and_the_dome_path(pkg):
    """Every record that carries the root's planes is a follower or pruned -- except a leaf box that is no follower, and
    except the one record in front of the dome's own (follower) leaf box: leaving out both would leave the dome's box
    untested, and the model walk below then tests the dome's sphere for rays its box rejects."""
    words, mask = program(pkg, "book1_1200")
    ops = words[:, 7] & 0xff
    assert int((mask == FOLLOWER).sum()) == 8
    root_planes = [i for i in range(len(words)) if ops[i] == OP_BOX and np.array_equal(words[i, :6], words[0, :6])]
    assert len(root_planes) == 10
    heads = leaf_run_heads(words)
    assert [i for i in root_planes if i in heads] == [root_planes[7]]
    for i in root_planes:
        if (ops[i + 1] == OP_SPHERE and mask[i] != FOLLOWER) or i in heads:
            continue
        assert mask[i] in (FOLLOWER, PRUNED), i
    assert mask[0] == PRUNED and mask[root_planes[1]] == PRUNED    # the root (production walks enter at its left child), R1
    assert int((mask == PRUNED).sum()) >= 2


def test_scene_case_follower_counts_are_unchanged(pkg):
    counts = {name: int((program(pkg, "case_" + name)[1] == FOLLOWER).sum()) for name in LEAN_CASES}
    assert counts == {"big_lean": 4, "book1": 8, "book1_list": 0, "book1_sah": 1}


def test_two_builders_give_the_same_mask(pkg):
    for name in ("book1_1200", "dome_3", "fuzz_2"):
        b = pkg.load().builder()
        assert np.array_equal(b.box_plan(_worlds(pkg)[name](pkg, b)), program(pkg, name)[1]), name
    words, mask = program(pkg, "book1_1200")
    assert np.array_equal(pkg.load().builder().box_plan(words=words), mask)          # ... and so do the words alone


def test_other_programs_get_no_plan(pkg):
    b = pkg.load().builder()
    world, _, _ = pkg.scenes.cornell_box_scene(b, 32, 32)
    assert not b.box_plan(world).any()
    b = pkg.load().builder()
    world, _, _ = CASES["book2_bvh"][0](pkg, b, 32, 32)
    mask = b.box_plan(world)
    assert len(mask) == len(b.flatten(world)[0]) and not mask.any()


@pytest.mark.parametrize("damage", ["nan_min", "nan_max", "child_sticks_out", "inf_plane"])
def test_a_damaged_box_keeps_itself_and_everything_above_it(pkg, damage):
    """Edited programs: a NaN (or infinite) plane, or a box that does not contain a child, keeps that record, its parent and
    every box above them; the rest of the mask still meets the conditions."""
    words, mask = program(pkg, "book1_1200")
    ops = words[:, 7] & 0xff
    deep = [j for j in np.nonzero(mask == PRUNED)[0] if len(ancestors(words, j)) >= 1 and (mask[ancestors(words, j)] == PRUNED).any()]
    assert deep
    j = int(deep[len(deep) // 2])
    w = words.copy()
    f = w.view(np.float32)
    if damage == "nan_min":
        f[j, 0] = np.nan
    elif damage == "nan_max":
        f[j + 1, 3] = np.nan        # a plane of the left child
    elif damage == "inf_plane":
        f[j, 5] = np.inf
    else:
        f[j, 1] = np.nextafter(f[j + 1, 1], np.float32(-np.inf))   # max.x just below the left child's
    got = pkg.load().builder().box_plan(words=w)
    up = ancestors(w, j)
    assert got[j] != PRUNED and not (got[up] == PRUNED).any()
    assert (mask[up] == PRUNED).any()                  # (some of them were pruned before the damage)
    if damage != "inf_plane":                          # (the library also asks for finite planes: stricter than the conditions here)
        assert prunable_records(w)[got == PRUNED].all()
        assert not prunable_records(w)[[j] + up].any()
    assert np.array_equal(got == FOLLOWER, np.isin(np.arange(len(w)), followers(w)))
    assert (got[ops != OP_BOX] == KEPT).all()


# ---- a float32 model of the walk -------------------------------------------------------------------------------------

def walk(words, o, d, best0, drop):
    """hit_top of a lean program for N rays at once, float32 throughout: Aabb::hit (aabb.rs:18-29), Sphere::hit
    (object.rs:84-111) behind Translate (object.rs:275).  Records in `drop` are stepped over as if they had passed.
    Returns (best, winning record, [ray, sphere record] rows of every Sphere::hit in each ray's own order, box tests)."""
    n = len(words)
    ops = (words[:, 7] & 0xff).astype(np.int64)
    skip = words[:, 6].astype(np.int64)
    mn, mx = planes(words)
    sph = words[:, :4].copy().view(np.float32)
    tr = (words[:, 7] & F_TRANSLATE) != 0
    N = len(o)
    with np.errstate(all="ignore"):
        inv = (np.float32(1.0) / d).astype(np.float32)
        dd = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        pc = np.zeros(N, dtype=np.int64)
        best = best0.copy()
        win = np.full(N, -1, dtype=np.int64)
        tested_ray, tested_pc, box_tests = [], [], 0
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
                pc[bx] = np.where(end > start, p + 1, skip[p])
                box_tests += len(bx)
            if len(sp):
                p = pc[sp]
                tested_ray.append(sp), tested_pc.append(p)
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
    rays = np.concatenate(tested_ray) if tested_ray else np.zeros(0, dtype=np.int64)
    recs = np.concatenate(tested_pc) if tested_pc else np.zeros(0, dtype=np.int64)
    order = np.argsort(rays, kind="stable")
    return best, win, np.stack([rays[order], recs[order]], axis=1), box_tests


def model_rays(words, seed, n_rays=3000):
    """Ordinary rays (from sphere surfaces and from outside the scene) and hostile ones: origins exactly on box planes,
    direction components +0, -0 and denormal, origins outside the root box, best preset to t_near."""
    rs = np.random.RandomState(seed)
    ops = words[:, 7] & 0xff
    mn, mx = planes(words)
    boxes = np.nonzero(ops == OP_BOX)[0]
    spheres = np.nonzero(ops == OP_SPHERE)[0]
    small = spheres[words[spheres, :4].view(np.float32)[:, 3] < 2000.0]
    if not len(small):
        small = spheres
    sphf = words[:, :4].view(np.float32)
    tr = (words[:, 7] & F_TRANSLATE) != 0
    pick = small[rs.randint(0, len(small), n_rays)]
    nrm = rs.standard_normal((n_rays, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cen = np.where(tr[pick][:, None], sphf[pick, :3], 0.0)
    o = (cen + sphf[pick, 3:4] * nrm).astype(np.float32)
    d = (nrm + rs.uniform(-0.6, 0.6, (n_rays, 3))).astype(np.float32)
    best = np.full(n_rays, np.finfo(np.float32).max, dtype=np.float32)
    k = np.arange(n_rays)
    if len(boxes):
        on_plane = k % 4 == 1          # an origin coordinate (or all three) exactly on a plane of some box
        bxs = boxes[rs.randint(0, len(boxes), n_rays)]
        corner = np.where(rs.rand(n_rays, 3) < 0.5, mn[bxs], mx[bxs])
        axes = rs.rand(n_rays, 3) < 0.6
        o = np.where(on_plane[:, None] & axes & np.isfinite(corner), corner, o).astype(np.float32)
        outside = k % 8 == 2           # outside the root box, aimed at the scene or past it
        root = boxes[0]
        span = np.where(np.isfinite(mx[root] - mn[root]), mx[root] - mn[root], 1.0).astype(np.float32)
        far = (mx[root] + span * rs.uniform(0.1, 2.0, (n_rays, 3))).astype(np.float32)
        o = np.where(outside[:, None], far * np.where(rs.rand(n_rays, 3) < 0.5, 1, -1), o).astype(np.float32)
        d = np.where(outside[:, None], (cen - o) + rs.uniform(-1, 1, (n_rays, 3)), d).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, 1.0, -1.0], dtype=np.float32)
    odd = k % 3 == 0                   # direction components +0, -0, denormal
    comp = special[rs.randint(0, len(special), (n_rays, 3))]
    d = np.where(odd[:, None] & (rs.rand(n_rays, 3) < 0.5), comp, d).astype(np.float32)
    best[k % 16 == 5] = T_NEAR         # t_range = t_near .. t_near: nothing can pass
    best[k % 16 == 6] = np.float32(0.5)
    return o, d, best


@pytest.mark.parametrize("name", WORLD_NAMES)
def test_model_walk_is_the_same_with_and_without_the_pruned_records(pkg, name):
    words, mask = program(pkg, name)
    o, d, best0 = model_rays(words, 11 + len(words))
    none = np.zeros(len(words), dtype=bool)
    ref = walk(words, o, d, best0, none)
    assert len(ref[2]) > 0             # (the rays do test spheres)
    for what, drop in (("followers", mask == FOLLOWER), ("pruned", mask == PRUNED), ("both", mask != KEPT)):
        got = walk(words, o, d, best0, drop)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), (name, what)
        assert np.array_equal(got[1], ref[1]), (name, what)
        assert np.array_equal(got[2], ref[2]), (name, what)          # the same Sphere::hit calls, in the same order
        if name == "book1_1200" or what == "followers":   # (a plan is a bet on where rays go: on another ray set it may lose)
            assert got[3] <= ref[3] and (got[3] < ref[3] or not drop.any() or name != "book1_1200"), (name, what)


def test_model_walk_notices_an_unsound_drop(pkg):
    """The model is able to fail: leaving out LEAF boxes (never in a plan) tests more spheres, and so does leaving out the
    record in front of the dome's follower leaf box together with the followers (rule (d))."""
    words, mask = program(pkg, "book1_1200")
    ops = words[:, 7] & 0xff
    o, d, best0 = model_rays(words, 5)
    ref = walk(words, o, d, best0, np.zeros(len(words), dtype=bool))
    got = walk(words, o, d, best0, (ops == OP_BOX) & (np.roll(ops, -1) == OP_SPHERE))
    assert len(got[2]) > len(ref[2])
    drop = mask != KEPT
    drop[list(leaf_run_heads(words))] = True
    got = walk(words, o, d, best0, drop)
    assert len(got[2]) > len(ref[2])


# ---- GPU: the same bits, the oracle's counters ------------------------------------------------------------------------

COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")


def _render_0_1(scene, cam, nx, ny, ns):
    scene.set_option("box_prune", 0)
    off = scene.par_cast(cam, nx, ny, ns)
    scene.set_option("box_prune", 1)
    return off, scene.par_cast(cam, nx, ny, ns)


@pytest.mark.gpu
def test_book1_same_bits_counters_and_slices(pkg, gpu, oracle):
    nx, ny, ns = 64, 48, 6
    b = gpu.builder()
    world, cam, _ = pkg.scenes.random_scene(b, nx, ny)
    sc = b.scene(world)
    assert int((b.box_plan(world) == PRUNED).sum()) > 0
    bo = oracle.builder()
    world_o, cam_o, _ = pkg.scenes.random_scene(bo, nx, ny)
    ref, st_ref = bo.scene(world_o).par_cast(cam_o, nx, ny, ns, stats=True)
    off, on = _render_0_1(sc, cam, nx, ny, ns)
    assert_bit_equal(on, off, "book1 box_prune 1 vs 0")
    assert_bit_equal(on, ref, "book1 box_prune 1 vs oracle")
    sc.set_option("box_chains", 0)                     # only the pruned records left out
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns), ref, "book1 box_prune 1, box_chains 0")
    sc.set_option("box_chains", 1)
    acc = np.zeros((ny, nx, 3), dtype=np.float32)      # slices of 3 + 3 against one call
    sc.par_cast(cam, nx, ny, 3, out=acc, sample_begin=0, resume=True, partial=True)
    sc.par_cast(cam, nx, ny, ns, out=acc, sample_begin=3, resume=True)
    assert_bit_equal(acc, ref, "book1 slices 3 + 3")
    img, st = sc.par_cast(cam, nx, ny, ns, stats=True)  # box_prune 1: counting launches walk the full image
    assert_bit_equal(img, ref, "book1 counting launch")
    for k in COUNTERS:
        assert st[k] == st_ref[k], (k, st[k], st_ref[k])
    sc.set_option("box_prune", 2)                      # ... 2: the pruned one -- the theorem on the device
    img2, st2 = sc.par_cast(cam, nx, ny, ns, stats=True)
    assert_bit_equal(img2, ref, "book1 counting launch, box_prune 2")
    for k in ("samples", "prim_tests", "shaded_hits", "rays", "draws"):
        assert st2[k] == st_ref[k], (k, st2[k], st_ref[k])
    print("book1 %dx%dx%d aabb_tests: reference %d, pruned image %d" % (nx, ny, ns, st_ref["aabb_tests"], st2["aabb_tests"]))
    assert st2["aabb_tests"] < st_ref["aabb_tests"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_hand_built_scenes_same_bits(pkg, gpu, oracle, name):
    nx, ny, ns = 32, 24, 8
    b = gpu.builder()
    sc = b.scene(HAND_BUILT[name][0](pkg, b))
    off, on = _render_0_1(sc, camera(pkg, gpu, nx, ny), nx, ny, ns)
    bo = oracle.builder()
    ref = bo.scene(HAND_BUILT[name][0](pkg, bo)).par_cast(camera(pkg, oracle, nx, ny), nx, ny, ns)
    assert_bit_equal(on, off, name)
    assert_bit_equal(on, ref, name + " (oracle)")


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
    sc.set_option("box_prune", 2)
    img, st = sc.par_cast(cam, nx, ny, ns, stats=True)
    assert_bit_equal(img, ref, "seed %d (counting launch, box_prune 2)" % seed)
    for k in ("samples", "prim_tests", "shaded_hits", "rays", "draws"):
        assert st[k] == st_ref[k], (seed, k, st[k], st_ref[k])
    assert st["aabb_tests"] <= st_ref["aabb_tests"]


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
