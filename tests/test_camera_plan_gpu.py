"""Camera plan on the GPU (DESIGN.md 3 "Camera plan"; scene option box_camera): launches that stage a pruned image probe the
camera they render with (csrc/rt_camera_probe.h) and stage the image planned from the probe's counts.  Every plan leaves the
walk's Sphere::hit calls alone, so at box_camera 2 (every launch, planned before it runs) frames must be bit-equal to box_camera 0
and to the live oracle, the five counters other than aabb_tests must be the oracle's in counting launches, and at box_prune 2
(counting launches walk the production image) aabb_tests must drop on book-1.  The default, box_camera 1, probes only launches
of CAMERA_PLAN_MIN_SAMPLES or more and makes the plan in the launch after the one that probed: the benchmark's own frame, twice."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from scene_cases import build_case
from test_box_chains import HAND_BUILT, camera, random_dome_world
from test_pass_blocks_gpu import _grazing_inside_glass

pytestmark = pytest.mark.gpu

FIVE = ("samples", "prim_tests", "shaded_hits", "rays", "draws")
NX, NY, NS = 96, 64, 8
_ref = {}


def book1(pkg, be, nx=NX, ny=NY):
    b = be.builder()
    world, cam, _ = pkg.scenes.random_scene(b, nx, ny)
    return b.scene(world), cam


def book1_oracle(pkg, oracle):
    """book-1 96x64x8 by the oracle, once per session, never written to"""
    if not _ref:
        so, cam_o = book1(pkg, oracle)
        img, st = so.par_cast(cam_o, NX, NY, NS, stats=True)
        img.setflags(write=False)
        _ref.update(img=img, st=st)
    return _ref["img"], _ref["st"]


def both_settings(sc, cam, nx, ny, ns, ref, st_ref, what, strictly_below=False):
    """Frames at box_camera 0 and 2 against `ref`; counting launches at box_prune 1 (the full reference image: all six counters)
    and at box_prune 2 (the production image: the five, and aabb_tests at box_camera 0 and 2, which are returned)."""
    aabb = {}
    for mode in (0, 2):
        sc.set_option("box_camera", mode)
        sc.set_option("box_prune", 1)
        assert_bit_equal(sc.par_cast(cam, nx, ny, ns), ref, "%s, box_camera %d" % (what, mode))
        img, st = sc.par_cast(cam, nx, ny, ns, stats=True)
        assert_bit_equal(img, ref, "%s, box_camera %d (counting launch)" % (what, mode))
        for k in FIVE + ("aabb_tests",):
            assert st[k] == st_ref[k], (what, mode, k, st[k], st_ref[k])
        sc.set_option("box_prune", 2)
        img, st = sc.par_cast(cam, nx, ny, ns, stats=True)
        assert_bit_equal(img, ref, "%s, box_camera %d (counting launch, box_prune 2)" % (what, mode))
        for k in FIVE:
            assert st[k] == st_ref[k], (what, mode, k, st[k], st_ref[k])
        aabb[mode] = st["aabb_tests"]
    sc.set_option("box_prune", 1)
    print("%s %dx%dx%d aabb_tests: oracle %d, production walk at box_camera 0 %d, at box_camera 2 %d (%.4f)"
          % (what, nx, ny, ns, st_ref["aabb_tests"], aabb[0], aabb[2], aabb[2] / max(1, aabb[0])))
    if strictly_below:
        assert aabb[2] < aabb[0], (what, aabb)
    return aabb


@pytest.mark.parametrize("options", [{}, {"box_chains": 0}, {"box_tree": 0}])
def test_book1_frames_counters_and_fewer_box_tests(pkg, gpu, oracle, options):
    ref, st_ref = book1_oracle(pkg, oracle)
    sc, cam = book1(pkg, gpu)
    for k, v in options.items():
        sc.set_option(k, v)
    both_settings(sc, cam, NX, NY, NS, ref, st_ref, "book1 %r" % (options,), strictly_below=True)


def test_book1_camera_turned_away(pkg, gpu, oracle):
    """Every primary ray ends on the dome: the probe's paths have no bounce, and every box but the dome's path fails."""
    S = pkg.scenes
    look = lambda be: be.camera_look(S.v(13.0, 2.0, 3.0), S.v(26.0, 6.0, 6.0), S.v(0.0, 1.0, 0.0), 20.0, 1.5, 0.1, 10.0)
    sc, _ = book1(pkg, gpu)
    so, _ = book1(pkg, oracle)
    ref, st_ref = so.par_cast(look(oracle), 48, 32, 4, stats=True)
    assert st_ref["rays"] == st_ref["samples"]                  # no path bounces
    both_settings(sc, look(gpu), 48, 32, 4, ref, st_ref, "book1, camera turned away")


def test_camera_inside_the_glass_sphere(pkg, gpu, oracle):
    sg, cam_g = _grazing_inside_glass(pkg, gpu)
    so, cam_o = _grazing_inside_glass(pkg, oracle)
    ref, st_ref = so.par_cast(cam_o, 16, 16, 8, stats=True)
    both_settings(sg, cam_g, 16, 16, 8, ref, st_ref, "camera inside glass")


@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_hand_built_scenes(pkg, gpu, oracle, name):
    nx, ny, ns = 32, 24, 6
    b, bo = gpu.builder(), oracle.builder()
    sc = b.scene(HAND_BUILT[name][0](pkg, b))
    ref, st_ref = bo.scene(HAND_BUILT[name][0](pkg, bo)).par_cast(camera(pkg, oracle, nx, ny), nx, ny, ns, stats=True)
    both_settings(sc, camera(pkg, gpu, nx, ny), nx, ny, ns, ref, st_ref, name)


@pytest.mark.parametrize("seed", range(6))
def test_random_dome_worlds(pkg, gpu, oracle, seed):
    nx, ny, ns = 32, 24, 6
    b, bo = gpu.builder(), oracle.builder()
    sc = b.scene(random_dome_world(pkg, b, 1000 + seed, 5 + 9 * seed))
    ref, st_ref = bo.scene(random_dome_world(pkg, bo, 1000 + seed, 5 + 9 * seed)).par_cast(camera(pkg, oracle, nx, ny), nx, ny, ns, stats=True)
    both_settings(sc, camera(pkg, gpu, nx, ny), nx, ny, ns, ref, st_ref, "dome seed %d" % seed)


def test_book1_sah(pkg, gpu, oracle):
    nx, ny, ns = 32, 24, 6
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1_sah", nx, ny)
    so, cam_o, _, _, _ = build_case(pkg, oracle, "book1_sah", nx, ny)
    ref, st_ref = so.par_cast(cam_o, nx, ny, ns, stats=True)
    both_settings(sg, cam, nx, ny, ns, ref, st_ref, "book1_sah")


def test_big_lean_gets_no_plan(pkg, gpu, oracle):
    """3000 spheres: the program is walked from global memory, nothing is staged, probed or planned."""
    sg, cam, nx, ny, ns = build_case(pkg, gpu, "big_lean")
    so, cam_o, _, _, _ = build_case(pkg, oracle, "big_lean")
    ref, st_ref = so.par_cast(cam_o, nx, ny, ns, stats=True)
    aabb = both_settings(sg, cam, nx, ny, ns, ref, st_ref, "big_lean")
    assert aabb[0] == aabb[2] == st_ref["aabb_tests"]


def test_six_cameras_on_one_handle(pkg, gpu):
    """A, B, A, B, then four more cameras: the cache of four evicts, and every frame is the one a fresh handle renders."""
    S = pkg.scenes
    nx, ny, ns = 48, 32, 4
    spots = [(13.0, 2.0, 3.0), (-9.0, 3.0, 8.0), (4.0, 9.0, -11.0), (0.5, 1.0, 14.0), (-12.0, 1.5, -4.0), (7.0, 0.8, 0.5)]
    cams = [gpu.camera_look(S.v(*p), S.v(0, 0.5, 0), S.v(0.0, 1.0, 0.0), 25.0 + 3 * i, 1.5, 0.05, 10.0) for i, p in enumerate(spots)]
    fresh = []
    for c in cams:
        sc, _ = book1(pkg, gpu, nx, ny)
        sc.set_option("box_camera", 2)
        fresh.append(sc.par_cast(c, nx, ny, ns))
    plain, _ = book1(pkg, gpu, nx, ny)
    plain.set_option("box_camera", 0)
    for i, c in enumerate(cams):
        assert_bit_equal(fresh[i], plain.par_cast(c, nx, ny, ns), "camera %d, box_camera 2 vs 0" % i)
    one, _ = book1(pkg, gpu, nx, ny)
    one.set_option("box_camera", 2)
    for i in (0, 1, 0, 1, 2, 3, 4, 5, 0, 1, 5):
        assert_bit_equal(one.par_cast(cams[i], nx, ny, ns), fresh[i], "one handle, camera %d" % i)


def test_default_setting_slices_and_ranks(pkg, gpu, oracle):
    """box_camera 1, the default: a frame in slices 3 + 5 and a frame from two ranks equal the one-call frame."""
    ref, _ = book1_oracle(pkg, oracle)
    sc, cam = book1(pkg, gpu)
    assert_bit_equal(sc.par_cast(cam, NX, NY, NS), ref, "one call")
    acc = np.zeros((NY, NX, 3), dtype=np.float32)
    sc.par_cast(cam, NX, NY, 3, out=acc, sample_begin=0, resume=True, partial=True)
    sc.par_cast(cam, NX, NY, NS, out=acc, sample_begin=3, resume=True)
    assert_bit_equal(acc, ref, "slices 3 + 5")
    canvas = np.zeros((NY, NX, 3), dtype=np.float32)
    for r in range(2):
        sc.par_cast(cam, NX, NY, NS, out=canvas, tile_w=16, tile_h=16, rank=r, nranks=2)
    assert_bit_equal(canvas, ref, "rank 0 of 2 + rank 1 of 2")
    sc.set_option("box_camera", 2)       # ... and with a plan made in the first slice and used by the second
    acc = np.zeros((NY, NX, 3), dtype=np.float32)
    sc.par_cast(cam, NX, NY, 3, out=acc, sample_begin=0, resume=True, partial=True)
    sc.par_cast(cam, NX, NY, NS, out=acc, sample_begin=3, resume=True)
    assert_bit_equal(acc, ref, "slices 3 + 5, box_camera 2")


def test_default_setting_plans_behind_the_launch_that_probed(pkg, gpu, oracle):
    """The benchmark's frame (book-1 1200x800x50) at the default: the first call probes and stages the scene's image, the second
    makes the plan and stages the camera's; a third in two sample passes.  All equal the box_camera 0 frame.  The camera of a
    96x64 frame has the same bytes, so a small counting launch at box_prune 2 then walks the plan the large calls left behind."""
    nx, ny, ns = 1200, 800, 50
    sc, cam = book1(pkg, gpu, nx, ny)
    sc.set_option("box_camera", 0)
    want = sc.par_cast(cam, nx, ny, ns)
    sc.set_option("box_prune", 2)
    _, st0 = sc.par_cast(cam, NX, NY, NS, stats=True)
    sc.set_option("box_camera", 1)
    _, st1 = sc.par_cast(cam, NX, NY, NS, stats=True)           # too small to probe: no plan yet
    sc.set_option("box_prune", 1)
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns), want, "first call (probes)")
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns), want, "second call (plans)")
    sc.set_option("scratch_mb", 320)                            # 11.5 MB per sample: two passes of 25
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns), want, "third call, two passes")
    small_cam = pkg.scenes.random_scene(gpu.builder(), NX, NY)[1]
    assert bytes(small_cam) == bytes(cam)
    sc.set_option("box_prune", 2)
    img, st2 = sc.par_cast(small_cam, NX, NY, NS, stats=True)
    assert_bit_equal(img, book1_oracle(pkg, oracle)[0], "small counting launch on the large calls' plan")
    print("book1 %dx%dx%d aabb_tests of the production walk: box_camera 0 %d, the plan of the 1200x800x50 calls %d" % (NX, NY, NS, st0["aabb_tests"], st2["aabb_tests"]))
    assert st1["aabb_tests"] == st0["aabb_tests"]
    assert st2["aabb_tests"] < st0["aabb_tests"]
    # a fresh handle whose FIRST call takes two passes: the first pass probes, the second plans
    sc2, _ = book1(pkg, gpu, nx, ny)
    sc2.set_option("scratch_mb", 320)
    assert_bit_equal(sc2.par_cast(cam, nx, ny, ns), want, "fresh handle, two passes")


def _row_of_four(pkg, be):
    """Four spheres in a row along x, seen head-on: nearly every ray that meets the row ends on the first sphere, so the probe's
    counts keep the box around the far pair, which the area model leaves out -- the camera's image is LARGER than the scene's."""
    S = pkg.scenes
    b = be.builder()
    mats = [b.diffuse_light(b.constant(S.v(0.9, 0.8, 0.6)), 2.0), b.lambertian(b.constant(S.v(0.7, 0.3, 0.2))),
            b.metal(S.v(0.8, 0.8, 0.9), 0.1), b.lambertian(b.constant(S.v(0.2, 0.6, 0.3)))]
    objs = [b.translate(S.v(1.2 * k, 0.0, 0.0), b.sphere(0.5, mats[k])) for k in range(4)]
    cam = be.camera_look(S.v(-8.0, 0.05, 0.02), S.v(4.0, 0.0, 0.0), S.v(0.0, 1.0, 0.0), 20.0, 1.5, 0.0, 10.0)
    return b.scene([b.bvh(objs, (0.0, 1.0))]), cam


def test_a_camera_image_larger_than_the_scenes(pkg, gpu, capfd):
    """box_camera 1, a first call of 34.6 M samples in two passes: pass 1 probes, pass 2 makes the plan, finds its image larger
    than the one the call's LDS was sized for and keeps the scene's table; the next call is sized for the camera's image and
    stages it.  Every frame equals the box_camera 0 frame."""
    import re
    nx, ny, ns = 1200, 800, 36
    sc, cam = _row_of_four(pkg, gpu)
    sc.set_option("box_camera", 0)
    want = sc.par_cast(cam, nx, ny, ns)
    assert (want != 0).any() and np.isfinite(want).all()
    sc.set_option("box_camera", 1)
    sc.set_option("scratch_mb", 256)                              # 11.5 MB per sample: two passes of 18
    sc.set_option("verbose", 1)
    capfd.readouterr()
    first = sc.par_cast(cam, nx, ny, ns)
    err = capfd.readouterr().err
    m = re.search(r"camera plan: (\d+) rays probed, (\d+) interior record\(s\) left out \(the scene's plan: (\d+)\), image (\d+) B", err)
    assert m and err.count(") of %d:" % ns) == 2, err[-1500:]
    left_out, scenes, cam_bytes = int(m.group(2)), int(m.group(3)), int(m.group(4))
    print("row of four: the camera's plan leaves out %d record(s), the scene's %d; camera image %d B" % (left_out, scenes, cam_bytes))
    assert left_out < scenes, err[-1500:]
    assert "not staged by this call" in err, err[-1500:]
    assert_bit_equal(first, want, "first call: probe in pass 1, plan in pass 2, the scene's table kept")
    second = sc.par_cast(cam, nx, ny, ns)
    err = capfd.readouterr().err
    assert "LDS image %d B" % cam_bytes in err and "the camera's plan" in err, err[-1500:]
    sc.set_option("verbose", 0)
    assert_bit_equal(second, want, "second call: sized for the camera's image")
    sc.set_option("box_prune", 2)
    img, st = sc.par_cast(cam, 96, 64, 4, stats=True)            # (the same camera bytes: aspect 1.5)
    sc.set_option("box_camera", 0)
    img0, st0 = sc.par_cast(cam, 96, 64, 4, stats=True)
    assert_bit_equal(img, img0, "counting launch on the camera's plan")
    for k in FIVE:
        assert st[k] == st0[k], (k, st[k], st0[k])
