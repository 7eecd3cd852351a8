"""The lean pool kernel's sphere pass with one division per Sphere::hit and an unconditional Translate subtraction
(csrc/rt_sphere_hit.h, rt_pool.h): frames and the six counters against the live oracle, on the production kernel and on the
counting variant, on small scenes built for the pass -- first roots close to 0 (rays refracted into glass), hits that are second
roots (the camera inside a sphere), first roots at or beyond the walk's best (overlapping spheres), SPHERE records without a
Translate, and a launch with t_near = 0, which must not use the claim that needs t_near > 0."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from test_lean_loop_gpu import _against_the_oracle

pytestmark = pytest.mark.gpu

OP_SPHERE, F_TRANSLATE = 2, 1 << 8


def _dome(pkg, b, radius=60.0):
    S = pkg.scenes
    return b.flip_normals(b.sphere(radius, b.diffuse_light(b.constant(S.v(0.7, 0.8, 1.0)), 1.0)))


def _glass_grid(pkg, be):
    """(a) One Bvh of 24 spheres in a 6 x 4 grid, every other one glass, and the emitter dome: a ray refracted into a glass
    sphere starts on its surface and points inward -- its first root lies within a few ulps of 0."""
    S = pkg.scenes
    b = be.builder()
    rs = np.random.RandomState(7)
    objs = []
    for i in range(6):
        for j in range(4):
            c = S.v(-2.5 + i + 0.2 * rs.rand(), -1.5 + j + 0.2 * rs.rand(), -6.0 + 1.5 * rs.rand())
            k = i * 4 + j
            if k % 2 == 0:
                mat = b.dielectric(1.5)
            elif k % 4 == 1:
                mat = b.lambertian(b.constant(S.v(*(0.2 + 0.7 * rs.rand(3)))))
            else:
                mat = b.metal(S.v(*(0.5 + 0.5 * rs.rand(3))), 0.05)
            objs.append(b.translate(c, b.sphere(0.42, mat)))
    assert len(objs) == 24
    objs.append(_dome(pkg, b))
    cam = be.camera_look(S.v(0, 0, 2.0), S.v(0, 0, -6.0), S.v(0, 1, 0), 42.0, 1.0, 0.0, 1.0)
    return b.scene([b.bvh(objs, (0.0, 1.0))]), cam


def _camera_inside_glass(pkg, be):
    """(b) The camera sits inside a glass sphere: the first root of every camera ray against it is negative, the hit is the
    second root."""
    S = pkg.scenes
    b = be.builder()
    objs = [b.translate(S.v(0.0, 0.0, 0.0), b.sphere(1.0, b.dielectric(1.5))),
            b.translate(S.v(-1.2, 0.3, -4.0), b.sphere(0.8, b.lambertian(b.constant(S.v(0.8, 0.3, 0.2))))),
            b.translate(S.v(1.2, -0.3, -4.0), b.sphere(0.8, b.metal(S.v(0.8, 0.8, 0.6), 0.0))),
            _dome(pkg, b)]
    cam = be.camera_look(S.v(0.0, 0.0, 0.3), S.v(0, 0, -4.0), S.v(0, 1, 0), 60.0, 1.0, 0.0, 1.0)
    return b.scene([b.bvh(objs, (0.0, 1.0))]), cam


def _overlapping(pkg, be):
    """(c) Ten spheres that overlap their neighbours along and across the view: whichever is tested later has a first root at or
    beyond the best of the one in front of it, and rays leaving a surface start inside the neighbour."""
    S = pkg.scenes
    b = be.builder()
    objs = []
    for k in range(10):
        c = S.v(-0.9 + 0.2 * k, 0.15 * ((k % 3) - 1), -3.0 - 0.25 * (k % 4))
        mat = b.metal(S.v(0.9, 0.8, 0.7), 0.0) if k % 3 == 0 else b.lambertian(b.constant(S.v(0.3 + 0.07 * k, 0.5, 0.9 - 0.07 * k)))
        objs.append(b.translate(c, b.sphere(0.5, mat)))
    # two concentric ones of equal radius: the same roots twice, the second a first root AT best
    objs.append(b.translate(S.v(0.0, 1.2, -3.0), b.sphere(0.4, b.lambertian(b.constant(S.v(0.9, 0.2, 0.2))))))
    objs.append(b.translate(S.v(0.0, 1.2, -3.0), b.sphere(0.4, b.lambertian(b.constant(S.v(0.2, 0.9, 0.2))))))
    objs.append(_dome(pkg, b))
    cam = be.camera_look(S.v(0, 0.3, 0), S.v(0, 0.3, -3.0), S.v(0, 1, 0), 50.0, 1.0, 0.0, 1.0)
    return b.scene([b.bvh(objs, (0.0, 1.0))]), cam


def _no_translate(pkg, be, words=None):
    """(d) SPHERE records without a Translate, at list level and under a Bvh, beside translated ones: their records in the
    staged image carry the offset +0."""
    S = pkg.scenes
    b = be.builder()
    world = [b.sphere(0.6, b.lambertian(b.constant(S.v(0.7, 0.6, 0.3)))),
             b.bvh([b.sphere(0.9, b.dielectric(1.5)),
                    b.translate(S.v(1.3, 0.0, 0.2), b.sphere(0.5, b.metal(S.v(0.8, 0.8, 0.8), 0.1))),
                    b.translate(S.v(-1.3, 0.0, -0.2), b.sphere(0.5, b.lambertian(b.constant(S.v(0.2, 0.4, 0.8))))),
                    _dome(pkg, b)], (0.0, 1.0))]
    if words is not None:
        words.append(b.flatten(world)[0])
    cam = be.camera_look(S.v(0.5, 0.8, 4.0), S.v(0, 0, 0), S.v(0, 1, 0), 45.0, 1.0, 0.0, 1.0)
    return b.scene(world), cam


def _is_what_it_claims(img, st):
    assert st["prim_tests"] > 0 and st["shaded_hits"] > 0 and (img != 0).any() and np.isfinite(img).all(), st


def test_glass_grid_under_a_dome(pkg, gpu, oracle):
    sg, cam_g = _glass_grid(pkg, gpu)
    so, cam_o = _glass_grid(pkg, oracle)
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 32, 32, 8, "24 spheres, half glass")
    _is_what_it_claims(img, st)
    assert st["rays"] > st["samples"]      # paths go on through the glass
    # the same frame from the other instantiations that share the pass: hot slot fields in global memory, and the 4-wide walk
    # (its image keeps the Translate select)
    sg.set_option("ray_lds", 0)
    assert_bit_equal(sg.par_cast(cam_g, 32, 32, 8), img, "ray_lds = 0")
    sg.set_option("ray_lds", 1)
    sg.set_option("bvh4", 1)
    assert_bit_equal(sg.par_cast(cam_g, 32, 32, 8), img, "bvh4 = 1")


def test_camera_inside_a_glass_sphere(pkg, gpu, oracle):
    sg, cam_g = _camera_inside_glass(pkg, gpu)
    so, cam_o = _camera_inside_glass(pkg, oracle)
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 16, 16, 8, "camera inside glass")
    _is_what_it_claims(img, st)
    assert st["shaded_hits"] >= st["samples"]   # every path hits the enclosing glass first: a second root


def test_overlapping_spheres(pkg, gpu, oracle):
    sg, cam_g = _overlapping(pkg, gpu)
    so, cam_o = _overlapping(pkg, oracle)
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 24, 24, 8, "overlapping spheres")
    _is_what_it_claims(img, st)


def test_sphere_records_without_a_translate(pkg, gpu, oracle):
    words = []
    sg, cam_g = _no_translate(pkg, gpu, words)
    so, cam_o = _no_translate(pkg, oracle)
    w = words[0]
    sph = w[(w[:, 7] & 0xff) == OP_SPHERE]
    bare = sph[(sph[:, 7] & F_TRANSLATE) == 0]
    assert len(sph) == 5 and len(bare) == 3 and set((w[:, 7] & 0xff).tolist()) <= {0, 1, 2}   # a lean program: END, BOX, SPHERE
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 24, 24, 8, "spheres without a Translate")
    _is_what_it_claims(img, st)


def test_t_near_zero_takes_the_reference_order(pkg, gpu, oracle):
    """(e) t_near = 0 through the binding: the pass's `t_near > 0` flag is false and every lane divides the first numerator
    first.  (Rays then re-hit the surface they leave; the frame is the oracle's all the same.)"""
    sg, cam_g = _glass_grid(pkg, gpu)
    so, cam_o = _glass_grid(pkg, oracle)
    for near in (0.0, -0.5):
        img_o, st_o = so.par_cast(cam_o, 16, 16, 4, stats=True, t_near=near, max_bounces=12)
        img_g, st_g = sg.par_cast(cam_g, 16, 16, 4, stats=True, t_near=near, max_bounces=12)
        assert_bit_equal(img_g, img_o, "t_near = %g (counting variant)" % near)
        for k in ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws"):
            assert st_g[k] == st_o[k], (near, k, st_g[k], st_o[k])
        assert_bit_equal(sg.par_cast(cam_g, 16, 16, 4, t_near=near, max_bounces=12), img_o, "t_near = %g (production kernel)" % near)
        _is_what_it_claims(img_o, st_o)
