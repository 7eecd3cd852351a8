"""Box chains: production launches of the lean pool kernel leave out of the LDS image every BOX record that
repeats the BOX right before it bit for bit and is no skip target -- its test is known to pass.  CPU tests: the rule,
recomputed here from the flat program, on book-1 and hand-built scenes.  GPU tests: the library finds the same records, and
option box_chains 0 / 1 give the same bits, the oracle's image and the oracle's counters."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from scene_cases import CASES, build_case

OP_END, OP_BOX, OP_SPHERE = 0, 1, 2


def followers(words):
    """Records j with: j a BOX, j - 1 a BOX with bitwise the same (min, max) on all three axes, no BOX's skip pointing at j.
    Flat program rows: lo = (min.x, max.x, min.y, max.y), hi = (min.z, max.z, skip, flags)."""
    ops = words[:, 7] & 0xff
    targets = {int(words[i, 6]) for i in range(len(words)) if ops[i] == OP_BOX}
    return [j for j in range(1, len(words))
            if ops[j] == OP_BOX and ops[j - 1] == OP_BOX and j not in targets and np.array_equal(words[j, :6], words[j - 1, :6])]


def enclosing_sphere_world(pkg, b, centres):
    """A Bvh of small spheres at `centres` and a sky-dome-like sphere (FlipNormals{Sphere(10000)}) at the origin."""
    S = pkg.scenes
    mat = b.lambertian(b.constant(S.vfrom(0.5)))
    objs = [b.translate(S.v(*c), b.sphere(0.5, mat)) for c in centres]
    objs.append(b.flip_normals(b.sphere(10000.0, b.diffuse_light(b.constant(S.v(0.7, 0.8, 1.0)), 1.0))))
    return [b.bvh(objs, (0.0, 1.0))]


def nested_pair_world(pkg, b):
    """Two spheres, the left one (smaller centroid on every axis) enclosing the right one: the left leaf's box is its parent's."""
    S = pkg.scenes
    mat = b.lambertian(b.constant(S.vfrom(0.5)))
    return [b.bvh([b.sphere(10.0, mat), b.translate(S.v(5.0, 5.0, 5.0), b.sphere(1.0, b.metal(S.v(0.8, 0.8, 0.9), 0.1)))], (0.0, 1.0))]


def disjoint_world(pkg, b):
    S = pkg.scenes
    mat = b.lambertian(b.constant(S.vfrom(0.5)))
    return [b.bvh([b.translate(S.v(3.0 * i, i, -i), b.sphere(0.5, mat)) for i in range(1, 12)], (0.0, 1.0))]


# hand-built scenes: (world builder, expected number of followers)
HAND_BUILT = {
    # dome first in centroid order: root, left half [dome, s1, s2, s3], its left [dome, s1], the dome's leaf -- three repeats
    "dome_first": (lambda pkg, b: enclosing_sphere_world(pkg, b, [(i, i, i) for i in range(1, 8)]), 3),
    # dome fourth of eight: the left half repeats the root; [s-1, dome] is a right child (a skip target), and so is the dome's leaf
    "dome_middle": (lambda pkg, b: enclosing_sphere_world(pkg, b, [(i, i, i) for i in (-3, -2, -1, 1, 2, 3, 4)]), 1),
    "nested_pair": (nested_pair_world, 1),
    # disjoint small spheres: no box repeats another
    "no_repeats": (lambda pkg, b: disjoint_world(pkg, b), 0),
}


def camera(pkg, be, nx, ny):
    S = pkg.scenes
    return be.camera_look(S.v(13, 2, 3), S.v(0, 0, 0), S.v(0.0, 1.0, 0.0), 40.0, float(S.f32(nx) / S.f32(ny)), 0.0, 10.0)


def random_dome_world(pkg, b, seed, n):
    """n random spheres (random radii, some overlapping) and the enclosing dome, under one Bvh."""
    S = pkg.scenes
    rng = pkg.small_rng.SmallRng(seed)
    mats = [b.lambertian(b.constant(S.v(0.7, 0.3, 0.2))), b.metal(S.v(0.8, 0.8, 0.9), 0.1), b.dielectric(1.5)]
    objs = []
    for i in range(n):
        c = S.f32(8.0) * rng.gen_vec3() - S.f32(4.0)
        objs.append(b.translate(S.v(c[0], c[1], c[2]), b.sphere(float(S.f32(0.05) + S.f32(1.5) * rng.gen_f32()), mats[i % 3])))
    objs.append(b.flip_normals(b.sphere(10000.0, b.diffuse_light(b.constant(S.v(0.7, 0.8, 1.0)), 1.0))))
    return [b.bvh(objs, (0.0, 1.0))]


# ---- CPU: the rule on flat programs -------------------------------------------------------------------------------

def test_book1_followers_are_the_dome_path_repeats(pkg):
    """book-1 (bvh::from_scene with the sky dome): the ten records that carry the dome's box are the root, two right children
    (skip targets) and seven followers; every follower has a skip pointer past it, none is a skip target."""
    be = pkg.load()
    b = be.builder()
    world, _, _ = pkg.scenes.random_scene(b, 1200, 800)
    words, feat = b.flatten(world)
    assert feat == 0
    ops = words[:, 7] & 0xff
    fol = followers(words)
    dome_box = [i for i in range(len(words)) if ops[i] == OP_BOX and np.array_equal(words[i, :6], words[0, :6])]
    assert len(dome_box) == 10
    targets = {int(words[i, 6]) for i in range(len(words)) if ops[i] == OP_BOX}
    assert [i for i in dome_box if i in targets] == [dome_box[1], dome_box[7]]  # R1, R7
    assert [i for i in dome_box if i in fol] == dome_box[2:7] + dome_box[8:10]
    assert ops[dome_box[9] + 1] == OP_SPHERE  # the last follower is the dome's leaf box
    assert not set(fol) & targets
    for j in fol:
        assert ops[j] == OP_BOX and np.array_equal(words[j, :6], words[j - 1, :6])
    assert len(fol) == 8  # (one repeat off the dome path too)


@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_hand_built_follower_counts(pkg, name):
    build, expect = HAND_BUILT[name]
    be = pkg.load()
    b = be.builder()
    words, feat = b.flatten(build(pkg, b))
    assert feat == 0
    assert len(followers(words)) == expect, followers(words)


def test_no_followers_without_repeats(pkg):
    """book-1 without the Bvh (a list world: no BOX record) and a Bvh of disjoint spheres have none."""
    be = pkg.load()
    b = be.builder()
    world, _, _ = pkg.scenes.random_scene(b, 120, 80, use_bvh=False)
    assert followers(b.flatten(world)[0]) == []
    b = be.builder()
    words, _ = b.flatten(HAND_BUILT["no_repeats"][0](pkg, b))
    assert (words[:, 7] & 0xff == OP_BOX).sum() == 21 and followers(words) == []


def _lean_cases(pkg):
    out = []
    for name in sorted(CASES):
        be = pkg.load()
        b = be.builder()
        world, _, _ = CASES[name][0](pkg, b, CASES[name][1], CASES[name][2])
        if b.flatten(world)[1] == 0:
            out.append(name)
    return out


def test_lean_scene_cases(pkg):
    """The scene cases the GPU test below renders with and without box chains (their programs have an LDS image), and their
    followers: the SAH tree and the 3000-sphere Bvh repeat boxes too, a list world has no BOX record."""
    counts = {}
    for name in _lean_cases(pkg):
        b = pkg.load().builder()
        world, _, _ = CASES[name][0](pkg, b, CASES[name][1], CASES[name][2])
        counts[name] = len(followers(b.flatten(world)[0]))
    assert counts == {"big_lean": 4, "book1": 8, "book1_list": 0, "book1_sah": 1}


# ---- GPU: the library's records, and the same bits with and without them ------------------------------------------

def _render_both(scene, cam, nx, ny, ns):
    scene.set_option("box_chains", 0)
    off = scene.par_cast(cam, nx, ny, ns)
    scene.set_option("box_chains", 1)
    on = scene.par_cast(cam, nx, ny, ns)
    return off, on


@pytest.mark.gpu
def test_scene_cases_same_bits_with_and_without_box_chains(pkg, gpu, oracle):
    for name in _lean_cases(pkg):
        sg, cam, nx, ny, ns = build_case(pkg, gpu, name)
        b = gpu.builder()
        world, _, _ = CASES[name][0](pkg, b, nx, ny)
        assert sg.info()["box_followers"] == len(followers(b.flatten(world)[0])), name
        off, on = _render_both(sg, cam, nx, ny, ns)
        assert_bit_equal(on, off, name)
        so, cam_o, _, _, _ = build_case(pkg, oracle, name)
        assert_bit_equal(on, so.par_cast(cam_o, nx, ny, ns), name + " (oracle)")


@pytest.mark.gpu
def test_book1_library_finds_the_followers_and_counts_stay_the_oracles(pkg, gpu, oracle):
    nx, ny, ns = 64, 48, 6
    imgs, stats = [], []
    for be in (gpu, oracle):
        b = be.builder()
        world, cam, _ = pkg.scenes.random_scene(b, nx, ny)
        sc = b.scene(world)
        if be is gpu:
            assert sc.info()["box_followers"] == len(followers(b.flatten(world)[0])) == 8
            off, on = _render_both(sc, cam, nx, ny, ns)
            assert_bit_equal(on, off, "book1")
        img, st = sc.par_cast(cam, nx, ny, ns, stats=True)
        imgs.append(img), stats.append(st)
    assert_bit_equal(imgs[0], imgs[1], "book1 (counting launch)")
    assert_bit_equal(on, imgs[1], "book1 (production launch)")
    for k in ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws"):
        assert stats[0][k] == stats[1][k], (k, stats[0][k], stats[1][k])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_hand_built_scenes_same_bits(pkg, gpu, oracle, name):
    build, expect = HAND_BUILT[name]
    nx, ny, ns = 32, 24, 8
    imgs = []
    for be in (gpu, oracle):
        b = be.builder()
        sc = b.scene(build(pkg, b))
        cam = camera(pkg, be, nx, ny)
        if be is gpu:
            assert sc.info()["box_followers"] == expect
            off, on = _render_both(sc, cam, nx, ny, ns)
            assert_bit_equal(on, off, name)
            imgs.append(on)
        else:
            imgs.append(sc.par_cast(cam, nx, ny, ns))
    assert_bit_equal(imgs[0], imgs[1], name + " (oracle)")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_random_dome_bvhs_same_bits(pkg, gpu, oracle, seed):
    nx, ny, ns = 32, 24, 6
    n = 5 + 9 * seed
    imgs = []
    for be in (gpu, oracle):
        b = be.builder()
        world = random_dome_world(pkg, b, 1000 + seed, n)
        sc = b.scene(world)
        cam = camera(pkg, be, nx, ny)
        if be is gpu:
            assert sc.info()["box_followers"] == len(followers(b.flatten(world)[0]))
            off, on = _render_both(sc, cam, nx, ny, ns)
            assert_bit_equal(on, off, "seed %d" % seed)
            imgs.append(on)
        else:
            imgs.append(sc.par_cast(cam, nx, ny, ns))
    assert_bit_equal(imgs[0], imgs[1], "seed %d (oracle)" % seed)
