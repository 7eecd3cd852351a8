"""The lean pool kernel's box run and sphere pass (rt_pool.h: one "at a BOX" compare per step that is the step's entry mask,
the loop-end ballot and the next iteration's entry; scalar exit test; dot(d, d) formed once per ray) and the one setup kernel
in front of every sample pass (write_pass_setup): frames and the N / P / H / rays / draws counters against the live oracle,
on the production kernel and on the counting variant, at the shapes where the loop's bookkeeping can go wrong."""
import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")


def _book1(pkg, be, nx, ny):
    b = be.builder()
    world, cam, _ = pkg.scenes.random_scene(b, nx, ny)
    return b.scene(world), cam


def _three_spheres_off_axis(pkg, be):
    """One Bvh of three spheres at the right edge of the view: most camera rays fail the root box, so a box run's first step
    empties the run, and waves reach the traverse loop with no lane at a BOX."""
    S = pkg.scenes
    b = be.builder()
    objs = [b.translate(S.v(-0.6, 0.0, -3.0), b.sphere(0.25, b.lambertian(b.constant(S.v(0.8, 0.3, 0.3))))),
            b.translate(S.v(0.0, 0.0, -3.0), b.sphere(0.25, b.metal(S.v(0.8, 0.8, 0.8), 0.1))),
            b.translate(S.v(0.6, 0.0, -3.0), b.sphere(0.25, b.diffuse_light(b.constant(S.v(1.0, 0.9, 0.7)), 4.0)))]
    cam = be.camera_look(S.v(0, 0, 0), S.v(1.6, 0.0, -3.0), S.v(0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    return b.scene([b.bvh(objs, (0.0, 1.0))]), cam


def _sphere_then_bvh(pkg, be):
    """A list-level sphere in front of a Bvh of one sphere: the program is SPHERE, BOX, SPHERE, END -- it does not start with a
    BOX, and every box run is one step long."""
    S = pkg.scenes
    b = be.builder()
    light = b.translate(S.v(-0.5, 0.0, -2.0), b.sphere(0.4, b.diffuse_light(b.constant(S.v(0.7, 0.8, 1.0)), 2.0)))
    ball = b.translate(S.v(0.5, 0.0, -2.0), b.sphere(0.4, b.lambertian(b.constant(S.v(0.6, 0.6, 0.2)))))
    cam = be.camera_look(S.v(0, 0, 0), S.v(0, 0, -2.0), S.v(0, 1, 0), 50.0, 1.0, 0.0, 1.0)
    return b.scene([light, b.bvh([ball], (0.0, 1.0))]), cam


def _against_the_oracle(sg, cam_g, so, cam_o, nx, ny, ns, what):
    assert bytes(cam_g) == bytes(cam_o)
    img_o, st_o = so.par_cast(cam_o, nx, ny, ns, stats=True)
    img_g, st_g = sg.par_cast(cam_g, nx, ny, ns, stats=True)   # the counting variant
    assert_bit_equal(img_g, img_o, what + " (counting variant)")
    for k in COUNTERS:
        assert st_g[k] == st_o[k], (what, k, st_g[k], st_o[k])
    assert_bit_equal(sg.par_cast(cam_g, nx, ny, ns), img_o, what + " (production kernel)")
    return img_o, st_o


def test_book1_small_frame(pkg, gpu, oracle):
    """(a) book-1 random_scene 48x32x4."""
    sg, cam_g = _book1(pkg, gpu, 48, 32)
    so, cam_o = _book1(pkg, oracle, 48, 32)
    _against_the_oracle(sg, cam_g, so, cam_o, 48, 32, 4, "book-1 48x32x4")


def test_runs_that_end_at_their_first_step(pkg, gpu, oracle):
    """(b) three spheres under a Bvh, camera turned away, 32x32x2."""
    sg, cam_g = _three_spheres_off_axis(pkg, gpu)
    so, cam_o = _three_spheres_off_axis(pkg, oracle)
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 32, 32, 2, "three spheres off axis")
    # the scene is what it claims to be: a ray that fails the root box costs ONE Aabb test, one that passes at least three
    assert st["aabb_tests"] < 2 * st["rays"], st
    assert st["prim_tests"] > 0 and (img != 0).any()


def test_program_that_does_not_start_with_a_box(pkg, gpu, oracle):
    """(c) a list-level sphere beside a Bvh of one sphere, 16x16x2."""
    sg, cam_g = _sphere_then_bvh(pkg, gpu)
    so, cam_o = _sphere_then_bvh(pkg, oracle)
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 16, 16, 2, "sphere, then a Bvh of one sphere")
    assert st["aabb_tests"] == st["rays"]          # one box, tested once per ray: runs of length 1
    assert (img != 0).any()


def test_slices_and_queue_modes_share_one_setup_kernel(pkg, gpu, capfd):
    """(d) GPU against GPU (the oracle knows neither slices nor the queue): book-1 48x32 as slices of 2 + 2 samples and as one
    call; then calls with the cost-ordered queue off and on, one after the other on one handle -- at 64x64x8, where the queue
    stays off either way (16 cost blocks; it needs 64), and at 128x128x8 (64 blocks), where the second call does run it."""
    sg, cam = _book1(pkg, gpu, 48, 32)
    one = sg.par_cast(cam, 48, 32, 4)
    acc = np.zeros((32, 48, 3), dtype=np.float32)
    sg.par_cast(cam, 48, 32, 2, out=acc, sample_begin=0, resume=True, partial=True)
    sg.par_cast(cam, 48, 32, 4, out=acc, sample_begin=2, resume=True)
    assert_bit_equal(acc, one, "slices of 2 + 2 samples vs one call")
    for n, engages in ((64, False), (128, True)):
        sg, cam = _book1(pkg, gpu, n, n)
        sg.set_option("lpt_phase1", 2)
        sg.set_option("verbose", 1)
        frames = []
        for lpt in (0, 2, 0):
            sg.set_option("lpt", lpt)
            capfd.readouterr()
            frames.append(sg.par_cast(cam, n, n, 8))
            err = capfd.readouterr().err
            line = [l for l in err.splitlines() if "pool: samples [" in l]
            assert len(line) == 1, err[-400:]
            on = "cost-ordered queue after 0 chunk(s)" not in line[0]
            assert on == (engages and lpt != 0), (n, lpt, line[0])
        sg.set_option("verbose", 0)
        assert_bit_equal(frames[1], frames[0], "%dx%dx8: queue off, then on" % (n, n))
        assert_bit_equal(frames[2], frames[0], "%dx%dx8: queue on, then off" % (n, n))
