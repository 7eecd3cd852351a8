"""The lean pool kernel's SCATTER pass generates the first Philox block of every lane's stream position at ONE place (csrc/
rt_device.h in_unit_sphere_tries_shared, rt_pool.h): the block serves the first attempts of the lanes that draw a direction and
the one draw of the Dielectric lanes.  Frames and the six counters against the live oracle, on the production kernel and on the
counting variant, on small scenes built for the change: passes of Dielectric lanes alone, passes without any, passes in which
deferred lanes (`tries` >= 1, stream position 12 x tries) and Dielectric lanes (position 0) share the generation point, and
total internal reflection, where the block is generated and no word of it may be taken.  `draws` only counts the words taken,
so its equality with the oracle's is the check that no draw moved.  The camera cases cover the END pass (the `chunk` test in
front of the camera ray, and the time draw behind lens-disc attempts of different lengths)."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from test_lean_loop_gpu import _against_the_oracle
from test_sphere_pass_gpu import _dome, _glass_grid

pytestmark = pytest.mark.gpu


def _grid(pkg, be, material_of, camera=None):
    """A 4 x 3 grid of spheres under the emitter dome; material_of(b, k, rs) gives sphere k its material."""
    S = pkg.scenes
    b = be.builder()
    rs = np.random.RandomState(11)
    objs = []
    for i in range(4):
        for j in range(3):
            c = S.v(-1.5 + i + 0.2 * rs.rand(), -1.0 + j + 0.2 * rs.rand(), -5.0 + 1.5 * rs.rand())
            objs.append(b.translate(c, b.sphere(0.45, material_of(b, i * 3 + j, rs))))
    objs.append(_dome(pkg, b))
    cam = camera(be) if camera else be.camera_look(S.v(0, 0, 2.0), S.v(0, 0, -5.0), S.v(0, 1, 0), 40.0, 1.0, 0.0, 1.0)
    return b.scene([b.bvh(objs, (0.0, 1.0))]), cam


def _glass(b, k, rs):
    return b.dielectric(1.3 + 0.1 * (k % 4))


def _no_glass(pkg):
    def material_of(b, k, rs):
        if k % 2 == 0:
            return b.lambertian(b.constant(pkg.scenes.v(*(0.2 + 0.7 * rs.rand(3)))))
        return b.metal(pkg.scenes.v(*(0.5 + 0.5 * rs.rand(3))), 0.3)
    return material_of


def _grazing_inside_glass(pkg, be):
    """The camera sits inside a glass sphere of radius 1, 0.9 from its centre, and looks ACROSS the radius through it: a ray at
    the angle phi to that radius meets the surface at sin(theta) = 0.9 sin(phi), and beyond sin(theta) = 1 / 1.5 the reflection
    is total -- at every later bounce too, a chord of a sphere keeps its angle.  Such a path draws nothing after its camera ray.
    The field of view is wide enough for the rays at the frame's left and right edges (phi near 30 and 150 degrees) to refract."""
    S = pkg.scenes
    b = be.builder()
    objs = [b.translate(S.v(0.0, 0.0, 0.0), b.sphere(1.0, b.dielectric(1.5))),
            b.translate(S.v(3.0, 0.4, 0.9), b.sphere(0.8, b.lambertian(b.constant(S.v(0.8, 0.3, 0.2))))),
            _dome(pkg, b)]
    cam = be.camera_look(S.v(0.0, 0.0, 0.9), S.v(5.0, 0.0, 0.9), S.v(0, 1, 0), 120.0, 1.0, 0.0, 1.0)
    return b.scene([b.bvh(objs, (0.0, 1.0))]), cam


def _is_a_picture(img, st):
    assert st["shaded_hits"] > 0 and (img != 0).any() and np.isfinite(img).all(), st


def test_every_sphere_glass(pkg, gpu, oracle):
    """1. No lane of a SCATTER pass enters the attempts: the shared block is consumed by the Dielectric draw alone."""
    sg, cam_g = _grid(pkg, gpu, _glass)
    so, cam_o = _grid(pkg, oracle, _glass)
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 32, 32, 8, "every sphere glass")
    _is_a_picture(img, st)
    assert st["rays"] > st["samples"]
    # a camera ray draws five times (u, v, one disc attempt, the time) and twice per further disc attempt (0.27 expected per
    # sample); a scatter event here draws once at the most, where a drawn direction would take three or more
    events = st["rays"] - st["samples"]
    assert events > st["samples"] // 2 and st["draws"] < 5 * st["samples"] + 3 * events, st


def test_no_glass_at_all(pkg, gpu, oracle):
    """2. Every lane of a SCATTER pass draws a direction: nobody takes a word past the attempts."""
    sg, cam_g = _grid(pkg, gpu, _no_glass(pkg))
    so, cam_o = _grid(pkg, oracle, _no_glass(pkg))
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 32, 32, 8, "no glass")
    _is_a_picture(img, st)
    # every continued path drew a direction: three draws or more per scatter event behind the camera ray's five
    assert st["rays"] > st["samples"] and st["draws"] >= 5 * st["samples"] + 3 * (st["rays"] - st["samples"]), st


def test_glass_metal_and_lambertian_share_passes(pkg, gpu, oracle):
    """3. Deferred lanes and Dielectric lanes in the same passes, on every instantiation that holds the pass."""
    sg, cam_g = _glass_grid(pkg, gpu)
    so, cam_o = _glass_grid(pkg, oracle)
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 32, 32, 8, "24 spheres, half glass")
    _is_a_picture(img, st)
    print("draws %d, shaded_hits %d: %.2f draws per shaded hit" % (st["draws"], st["shaded_hits"], st["draws"] / st["shaded_hits"]))
    # well above three draws per shaded hit although half the spheres and the dome draw one or none: the diffuse and metal hits
    # take their rejected attempts (5.7 draws expected, 5 % of them more than twelve -- a deferral)
    assert st["draws"] > 3 * st["shaded_hits"], st
    for name, value in (("ray_lds", 0), ("bvh4", 1)):   # hot slot fields in global memory; the 4-wide walk
        sg.set_option(name, value)
        assert_bit_equal(sg.par_cast(cam_g, 32, 32, 8), img, "%s = %d" % (name, value))
        sg.set_option(name, 1 - value)


@pytest.mark.parametrize("chunks", [1, 3, 4])
def test_samples_in_chunks(pkg, gpu, oracle, chunks):
    """The END pass ends a work item where s % chunk == 0: chunk = ns (no scratch), 3 (the last item is short) and 2; the default
    launch has chunk = 1 and skips the division."""
    sg, cam_g = _glass_grid(pkg, gpu)
    so, cam_o = _glass_grid(pkg, oracle)
    img_o, st_o = so.par_cast(cam_o, 16, 16, 8, stats=True)
    sg.set_option("chunks", chunks)
    img_g, st_g = sg.par_cast(cam_g, 16, 16, 8, stats=True)
    assert_bit_equal(img_g, img_o, "chunks = %d (counting variant)" % chunks)
    for k in ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws"):
        assert st_g[k] == st_o[k], (chunks, k, st_g[k], st_o[k])
    assert_bit_equal(sg.par_cast(cam_g, 16, 16, 8), img_o, "chunks = %d (production kernel)" % chunks)


def test_total_internal_reflection_draws_nothing(pkg, gpu, oracle):
    """4. `refracted` is false: the block is there and no word of it may be taken."""
    sg, cam_g = _grazing_inside_glass(pkg, gpu)
    so, cam_o = _grazing_inside_glass(pkg, oracle)
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 16, 16, 8, "grazing rays inside glass")
    assert st["shaded_hits"] > 0 and np.isfinite(img).all(), st
    # a totally reflected path hits the sphere from inside until the bounce cap (51 hits) on its camera ray's draws alone
    # (5.55 expected), where a path that refracts draws at each of its hits: with the middle of the frame totally reflected, the
    # frame's hits outnumber its draws, and some paths end before the cap
    assert st["shaded_hits"] > st["draws"] and st["rays"] < 51 * st["samples"], st


@pytest.mark.parametrize("aperture,exposure", [(0.0, (0.0, 1.0)), (0.4, (0.0, 1.0)), (0.4, (0.25, 0.75)), (2.0, (0.5, 0.625))])
def test_camera_draws(pkg, gpu, oracle, aperture, exposure):
    """5. The camera ray: u, v, lens-disc attempts of different lengths, then the time draw, which stands at a block boundary
    behind an even number of attempts and inside a block behind an odd one."""
    S = pkg.scenes

    def camera(be):
        return be.camera_look(S.v(0, 0, 2.0), S.v(0, 0, -5.0), S.v(0, 1, 0), 40.0, 1.0, aperture, 7.0, exposure)
    mat = lambda b, k, rs: _glass(b, k, rs) if k % 3 == 0 else _no_glass(pkg)(b, k, rs)
    sg, cam_g = _grid(pkg, gpu, mat, camera)
    so, cam_o = _grid(pkg, oracle, mat, camera)
    img, st = _against_the_oracle(sg, cam_g, so, cam_o, 16, 16, 8, "aperture %g, shutter %r" % (aperture, exposure))
    _is_a_picture(img, st)
