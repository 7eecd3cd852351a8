"""The lean pool kernel's traverse loop (rt_pool.h): the box run and the sphere pass are two `if`s on one wave-uniform flag
(`do_box`), a run is entered on scalar instructions alone (floor_lanes in signed scalar arithmetic, the first step's entry
mask = the ballot that chose the arm).  Frames and the N / P / H / rays / draws counters against the live oracle, bit for bit,
on the production kernel and on the counting variant, at the shapes where the choice of the arm can go wrong.  The lock-step
kernel (rt_sync_full.h) attaches its slow pass the same way (`if (!do_box)`): Cornell, a program without a BOX, and book-2 on
a small frame, where both arms run."""
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")


def _book1(pkg, be, nx, ny):
    b = be.builder()
    world, cam, _ = pkg.scenes.random_scene(b, nx, ny)
    return b.scene(world), cam


def _three_spheres_off_axis(pkg, be):
    """One Bvh of three spheres at the right edge of the view: most camera rays fail the root box and stand at END after one
    step, so the loop meets iterations in which no lane is at a BOX or at a SPHERE."""
    S = pkg.scenes
    b = be.builder()
    objs = [b.translate(S.v(-0.6, 0.0, -3.0), b.sphere(0.25, b.lambertian(b.constant(S.v(0.8, 0.3, 0.3))))),
            b.translate(S.v(0.0, 0.0, -3.0), b.sphere(0.25, b.metal(S.v(0.8, 0.8, 0.8), 0.1))),
            b.translate(S.v(0.6, 0.0, -3.0), b.sphere(0.25, b.diffuse_light(b.constant(S.v(1.0, 0.9, 0.7)), 4.0)))]
    cam = be.camera_look(S.v(0, 0, 0), S.v(1.6, 0.0, -3.0), S.v(0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    return b.scene([b.bvh(objs, (0.0, 1.0))]), cam


def _sphere_then_bvh_then_sphere(pkg, be):
    """SPHERE, BOX, SPHERE, END: the first iteration of every walk has no lane at a BOX, and every box run is one step."""
    S = pkg.scenes
    b = be.builder()
    light = b.translate(S.v(-0.5, 0.0, -2.0), b.sphere(0.4, b.diffuse_light(b.constant(S.v(0.7, 0.8, 1.0)), 2.0)))
    ball = b.translate(S.v(0.5, 0.0, -2.0), b.sphere(0.4, b.lambertian(b.constant(S.v(0.6, 0.6, 0.2)))))
    cam = be.camera_look(S.v(0, 0, 0), S.v(0, 0, -2.0), S.v(0, 1, 0), 50.0, 1.0, 0.0, 1.0)
    return b.scene([light, b.bvh([ball], (0.0, 1.0))]), cam


def _against_the_oracle(sg, cam_g, img_o, st_o, nx, ny, ns, what):
    img_g, st_g = sg.par_cast(cam_g, nx, ny, ns, stats=True)   # the counting variant
    assert_bit_equal(img_g, img_o, what + " (counting variant)")
    for k in COUNTERS:
        assert st_g[k] == st_o[k], (what, k, st_g[k], st_o[k])
    assert_bit_equal(sg.par_cast(cam_g, nx, ny, ns), img_o, what + " (production kernel)")


@pytest.fixture(scope="module")
def book1_oracle(pkg, oracle):
    """book-1 48x32x4 on the oracle, once for every case below (never modified)."""
    so, cam_o = _book1(pkg, oracle, 48, 32)
    img, st = so.par_cast(cam_o, 48, 32, 4, stats=True)
    img.setflags(write=False)
    return bytes(cam_o), img, st


@pytest.mark.parametrize("option,value", [(None, None), ("sphere_min", 1), ("sphere_min", 64), ("box_leave", 0), ("box_leave", 64),
                                          ("refill_min", 1), ("refill_min", 64), ("ray_lds", 0)])
def test_book1_every_path_of_the_selection(pkg, gpu, book1_oracle, option, value):
    """book-1 random_scene 48x32x4, one scene option at a time: sphere_min 1 (the sphere arm wins whenever one lane is parked) and
    64 (a box run starts with up to 63 lanes parked), box_leave 0 (one-iteration runs) and 64 (runs to exhaustion: floor_lanes
    saturates at 0), refill_min 1 and 64 (the loop is left after every arm / only when nothing is busy), ray_lds 0 (the slots'
    hot fields in global memory).  The schedule never changes a result: every frame equals the oracle's -- and so the default's."""
    cam_bytes, img_o, st_o = book1_oracle
    sg, cam_g = _book1(pkg, gpu, 48, 32)
    assert bytes(cam_g) == cam_bytes
    if option is not None:
        sg.set_option(option, value)
    _against_the_oracle(sg, cam_g, img_o, st_o, 48, 32, 4, "book-1 48x32x4, %s = %s" % (option, value))


def test_program_that_starts_with_a_sphere(pkg, gpu, oracle):
    """SPHERE, BOX, SPHERE, END at 32x32x2."""
    sg, cam_g = _sphere_then_bvh_then_sphere(pkg, gpu)
    so, cam_o = _sphere_then_bvh_then_sphere(pkg, oracle)
    assert bytes(cam_g) == bytes(cam_o)
    img_o, st_o = so.par_cast(cam_o, 32, 32, 2, stats=True)
    _against_the_oracle(sg, cam_g, img_o, st_o, 32, 32, 2, "sphere, Bvh of one sphere")
    assert st_o["aabb_tests"] == st_o["rays"]      # one box, tested once per ray: runs of one step
    assert st_o["prim_tests"] > st_o["rays"]       # the list-level sphere is tested by every ray, the leaf by some
    assert (img_o != 0).any()


@pytest.mark.parametrize("bvh4", [0, 1])
def test_iterations_in_which_neither_arm_has_work(pkg, gpu, oracle, bvh4):
    """Three spheres under one Bvh at the edge of the view, 32x32x2; bvh4 = 1 is the 4-wide walk (the WIDE instantiation)."""
    sg, cam_g = _three_spheres_off_axis(pkg, gpu)
    so, cam_o = _three_spheres_off_axis(pkg, oracle)
    assert bytes(cam_g) == bytes(cam_o)
    img_o, st_o = so.par_cast(cam_o, 32, 32, 2, stats=True)
    assert st_o["aabb_tests"] < 2 * st_o["rays"], st_o     # most rays fail the root: one Aabb test, then END
    assert st_o["prim_tests"] > 0 and (img_o != 0).any()
    if bvh4:
        sg.set_option("bvh4", 1)
        # the 4-wide walk tests other boxes and, against a looser best, more spheres (rt_pool.h): the frame is the oracle's, the
        # N / P counters are its own
        assert_bit_equal(sg.par_cast(cam_g, 32, 32, 2), img_o, "three spheres off axis, bvh4 (production kernel)")
        img_g, st_g = sg.par_cast(cam_g, 32, 32, 2, stats=True)
        assert_bit_equal(img_g, img_o, "three spheres off axis, bvh4 (counting variant)")
        for k in ("samples", "shaded_hits", "rays", "draws"):
            assert st_g[k] == st_o[k], (k, st_g[k], st_o[k])
        assert st_g["prim_tests"] >= st_o["prim_tests"]    # a superset of the reference's leaves
        return
    _against_the_oracle(sg, cam_g, img_o, st_o, 32, 32, 2, "three spheres off axis")


@pytest.mark.parametrize("name", ["cornell", "book2"])
def test_lock_step_kernel(pkg, gpu, oracle, name):
    """32x32x4 on the lock-step kernel: the Cornell box (no BOX record: the box arm never runs) and book_final_scene (a frame
    this small is the lock-step kernel's by the launcher's rule; its Bvhs give box runs and slow passes in turn)."""
    S = pkg.scenes

    def scene(be):
        b = be.builder()
        if name == "cornell":
            world, cam, _ = S.cornell_box_scene(b, 32, 32)
        else:
            world, cam, _ = S.book_final_scene(b, 32, 32, pkg.small_rng.SmallRng(0xDEADBEEF))
        return b.scene(world), cam
    sg, cam_g = scene(gpu)
    so, cam_o = scene(oracle)
    assert bytes(cam_g) == bytes(cam_o)
    img_o, st_o = so.par_cast(cam_o, 32, 32, 4, stats=True)
    assert (st_o["aabb_tests"] == 0) == (name == "cornell")
    _against_the_oracle(sg, cam_g, img_o, st_o, 32, 32, 4, name + " 32x32x4, lock-step kernel")
