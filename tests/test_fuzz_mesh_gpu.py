"""Random worlds with triangles, meshes and image textures on the GPU (fuzz_scenes.random_world with meshes / images; the seed
sets and tolerances of fuzz_mesh_cases.py).  The CPU oracle has neither primitive, so the worlds are compared

A. across the kernels: the one-lane kernel, the full-feature pool kernel and the lock-step kernel (their TRI instantiations,
   with and without counters) render the same bits and count the same work, frame by frame and sample by sample;
B. FEAT_DEEP worlds (the general walk): the frame is the fold of its samples and the ray frame of the camera's own rays;
C. first hits against the float64 closest hit of physics_ref (spheres, rects, prisms and triangles under their chains);
D. the image sampler on the device against the float64 sampler of image_ref;
E. the albedo, normal and depth planes against the float64 feature reference, images included.

Frames are 40 x 24 x 5 (feature frames 24 x 16), ray sets 2048."""
import re

import numpy as np
import pytest

import fuzz_mesh_cases as C
import image_cases as IC
import image_ref as IR
import physics_ref as PR
from conftest import assert_bit_equal
from test_fuzz_mesh import SAMPLER_SIZES, check_sampler, sampler_points
from test_image_texture_gpu import COUNTERS, _fold, _render_named

pytestmark = pytest.mark.gpu
f32 = np.float32
F = np.float64
SEED = 0xDEADBEEF
NX, NY, NS = 40, 24, 5
F32_MAX = np.finfo(f32).max
taken = set()   # (sync, schedule) pairs that verbose showed over the scheduled worlds


def _schedule(err):
    """Which full-feature schedule a verbose launch line names.  The lock-step kernel reports on the pool kernel's line
    (rtg_launch.inc launch_full_pool: "[rtg] full pool: ... (program window: W of N records)"); it takes the frame when option
    sync is 1 and the program sits in LDS whole (W = N), the pool kernel takes it whenever sync is 0."""
    m = re.search(r"\[rtg\] full pool: .*program window: (\d+) of (\d+) records", err)
    assert m and " 2 (second program)" not in err, err
    return int(m.group(1)) == int(m.group(2))


def _keys(seed, nx, ny, ns, n=64):
    rs = np.random.RandomState(seed)
    return rs.randint(0, nx, n), rs.randint(0, ny, n), rs.randint(0, ns, n)


def _same_bits_on_every_kernel(sc, cam, seed, capfd, what):
    """one lane per pixel against the production kernels under sync = 0 and 1, with counters and without; 64 samples of the
    kernels' own trace against the one-lane probe"""
    sc.set_option("sync", 0)
    base, c_base, took = _render_named(sc, cam, NX, NY, NS, 1, capfd)
    assert took == "one-lane", (what, took)
    assert np.isfinite(base).all() and base.max() > 0, what
    assert_bit_equal(sc.par_cast(cam, NX, NY, NS, seed=SEED), base, what + ": one lane per pixel, production variant")
    xs, ys, ss = _keys(seed, NX, NY, NS)
    one, i_one = sc.debug_samples(cam, NX, NY, NS, xs, ys, ss, seed=SEED)
    for sync in (0, 1):
        sc.set_option("sync", sync)
        sc.set_option("verbose", 1)
        capfd.readouterr()
        try:
            sc.set_option("kernel", 3)
            prod, st = sc.par_cast(cam, NX, NY, NS, seed=SEED, stats=True)
        finally:
            sc.set_option("verbose", 0)
        whole = _schedule(capfd.readouterr().err)
        taken.add((sync, "lock-step" if sync == 1 and whole else "pool"))
        assert_bit_equal(prod, base, "%s sync=%d: production kernel against one lane per pixel" % (what, sync))
        assert {k: st[k] for k in COUNTERS} == c_base, (what, sync, st, c_base)
        assert_bit_equal(sc.par_cast(cam, NX, NY, NS, seed=SEED), base, "%s sync=%d: production variant" % (what, sync))
        traced, i_traced = sc.debug_samples(cam, NX, NY, NS, xs, ys, ss, seed=SEED, trace_kernel=True)
        assert_bit_equal(traced, one, "%s sync=%d: RTG_FLAG_TRACE_KERNEL against the one-lane probe" % (what, sync))
        assert np.array_equal(i_traced, i_one), (what, sync)
    return c_base


# ---- A. every kernel, the same bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", C.SCHEDULED)
def test_mesh_worlds_render_the_same_bits_on_every_kernel(pkg, gpu, capfd, seed):
    b, world, cam, marks = C.build(pkg, gpu, seed, NX, NY)
    feat = b.flatten(world)[1]
    assert feat & C.FEAT_TRI and not feat & C.FEAT_DEEP
    sc = b.scene(world)
    counters = _same_bits_on_every_kernel(sc, cam, seed, capfd, "mesh world %d" % seed)
    assert counters["prim_tests"] > 0 and counters["rays"] > 0
    if marks["rect_light"]:
        # light sampling renders on the one-lane family whatever option `kernel` says (rtg_launch.inc launch_slice): the light
        # table is not empty, the frame and the samples do not depend on the options, and they differ from the plain ones
        plain = sc.par_cast(cam, NX, NY, NS, seed=SEED)
        sc.set_option("light_sampling", 1)
        sc.set_option("verbose", 1)
        capfd.readouterr()
        try:
            lit, _, _ = _render_named(sc, cam, NX, NY, NS, 1, capfd)
            sc.set_option("verbose", 1)
            sc.set_option("kernel", 3)
            again = sc.par_cast(cam, NX, NY, NS, seed=SEED)
        finally:
            sc.set_option("verbose", 0)
        m = re.search(r"light table of (\d+) rect", capfd.readouterr().err)
        assert m and int(m.group(1)) >= 1
        assert_bit_equal(again, lit, "mesh world %d, light sampling: kernel 3 against kernel 1" % seed)
        assert np.isfinite(lit).all() and not np.array_equal(lit, plain)
        # (RTG_FLAG_TRACE_KERNEL has nothing to trace on that family: the samples are the one-lane probe's, and the frame under
        # either value of sync is their fold)
        s_i, row_i, x_i = np.meshgrid(np.arange(NS), np.arange(NY), np.arange(NX), indexing="ij")
        rgb, _ = sc.debug_samples(cam, NX, NY, NS, x_i.ravel(), (NY - 1 - row_i).ravel(), s_i.ravel(), seed=SEED)
        fold = _fold(rgb.reshape(NS, NY, NX, 3), NS)
        for sync in (0, 1):
            sc.set_option("sync", sync)
            assert_bit_equal(sc.par_cast(cam, NX, NY, NS, seed=SEED), fold, "mesh world %d, light sampling, sync=%d: the fold of the samples" % (seed, sync))


def test_both_schedules_were_taken(pkg, gpu, capfd):
    """Over the seed set the lock-step kernel and the pool kernel each took frames, not merely the option.  (Run alone, this test
    renders the first four worlds itself.)"""
    if not taken:
        for seed in C.SCHEDULED[:4]:
            b, world, cam, _ = C.build(pkg, gpu, seed, NX, NY)
            _same_bits_on_every_kernel(b.scene(world), cam, seed, capfd, "mesh world %d" % seed)
    assert (1, "lock-step") in taken and (0, "pool") in taken, taken


# ---- B. deep worlds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", C.DEEP)
def test_deep_mesh_worlds_on_the_general_walk(pkg, gpu, seed):
    b, world, cam, _ = C.build(pkg, gpu, seed, NX, NY)
    feat = b.flatten(world)[1]
    assert feat & C.FEAT_TRI and feat & C.FEAT_DEEP
    sc = b.scene(world)
    img, st = sc.par_cast(cam, NX, NY, NS, seed=SEED, stats=True)
    assert np.isfinite(img).all() and img.max() > 0
    assert all(st[k] > 0 for k in COUNTERS), st
    assert_bit_equal(sc.par_cast(cam, NX, NY, NS, seed=SEED), img, "deep mesh world %d: production variant" % seed)
    s_i, row_i, x_i = np.meshgrid(np.arange(NS), np.arange(NY), np.arange(NX), indexing="ij")
    rgb, _ = sc.debug_samples(cam, NX, NY, NS, x_i.ravel(), (NY - 1 - row_i).ravel(), s_i.ravel(), seed=SEED)
    assert_bit_equal(_fold(rgb.reshape(NS, NY, NX, 3), NS), img, "deep mesh world %d: the fold of rtg_debug_samples" % seed)
    rays = pkg.rays.camera_rays(cam, NX, NY, NS, SEED)
    assert_bit_equal(sc.cast_rays(rays, NX, NY, NS, per_sample=True, seed=SEED), img, "deep mesh world %d: ray frame" % seed)


# ---- C. first hits against float64 ------------------------------------------------------------------------------------------------
def _rays8(rays7, t_max):
    return np.concatenate([np.asarray(rays7, f32), np.broadcast_to(np.asarray(t_max, f32), (len(rays7),))[:, None]], axis=1).astype(f32)


def _hits_against_float64(pkg, gpu, seed, fault=None):
    rec, world, prims, rays, ref = C.hit_reference(pkg, gpu, seed, fault=fault)
    sc = rec.scene(world)
    out, mat = sc.debug_hit_top(rays, seed=5, t_near=PR.T_NEAR)
    C.assert_by_kind(C.compare_by_kind(prims, ref, out, mat), "mesh world %d" % seed)
    return sc, rays, out, mat


@pytest.mark.parametrize("seed", C.FREE + C.FREE_DEEP)
def test_first_hits_against_the_float64_reference(pkg, gpu, seed):
    sc, rays, out, mat = _hits_against_float64(pkg, gpu, seed)
    q_out, q_mat = sc.closest_hit(rays, seed=5, t_min=PR.T_NEAR)
    assert_bit_equal(q_out, out, "mesh world %d: rtg_query_closest against rtg_debug_hit_top" % seed)
    assert np.array_equal(q_mat, mat)
    hit = out[:, 0] != 0
    far = sc.occluded(_rays8(rays, F32_MAX), seed=5, t_min=PR.T_NEAR)
    assert np.array_equal(far != 0, hit)
    near = sc.occluded(_rays8(rays, np.where(hit, out[:, 1] * f32(0.5), f32(1.0))), seed=5, t_min=PR.T_NEAR)
    assert not near[hit].any()


def _failure(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError as e:
        return str(e) or "failed"
    raise AssertionError("%s%r did not notice the planted fault %r" % (fn.__name__, a[2:], kw))


def test_the_checks_notice_planted_faults(pkg, gpu):
    """A reference that turns RotateY the other way, or multiplies the normal by the Scale, fails C against the (unchanged)
    kernels, in at least four worlds each; a reference that samples images by a wrong convention fails D and E."""
    for fault in ("rotate_neg", "scale_normal"):
        noticed = 0
        for seed in C.FREE + C.FREE_DEEP:
            try:
                _hits_against_float64(pkg, gpu, seed, fault=fault)
            except AssertionError:
                noticed += 1
        assert noticed >= 4, (fault, noticed)
    for fault in IR.FAULTS:
        _failure(_device_sampler, pkg, gpu, (5, 4), fault=fault)
    _failure(_feature_planes, pkg, gpu, IMAGE_WORLD, 1, image_fault="v_unflipped")


# ---- D. the image sampler on the device -------------------------------------------------------------------------------------------
def _device_sampler(pkg, gpu, size, fault=None):
    I = pkg.image
    b = gpu.builder()
    img = IC.image(size)
    cases = [(prm, b.image(img, prm)) for prm in IC.settings(I, size)]
    sc = b.scene([b.sphere(1.0, b.lambertian(cases[0][1]))])
    for k, (prm, t) in enumerate(cases):
        p = sampler_points(size, k)
        check_sampler(size, prm, sc.debug_texture(t, p), p, fault=fault)


@pytest.mark.parametrize("size", SAMPLER_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_device_sampler_against_the_float64_sampler(pkg, gpu, size):
    _device_sampler(pkg, gpu, size)


# ---- E. feature planes ------------------------------------------------------------------------------------------------------------
FNX, FNY = 24, 16
IMAGE_WORLD = C.FREE[0]      # a world that shows an image on a mesh in at least 2 % of its pixels (asserted below)
_shares = {}


def _feature_planes(pkg, gpu, seed, grid, image_fault=None):
    # (the world of C with its enclosing emitter: from the generator's cameras the objects alone fill 6 .. 77 % of a frame, and
    # compare_planes wants a quarter of the pixels hit)
    rec, world, cam, _ = C.build(pkg, gpu, seed, FNX, FNY, record=True, sky=True)
    ref, usable, allow, on_tri = PR.feature_reference(rec, world, cam, FNX, FNY, grid, allowance=True, image_fault=image_fault)
    fr = rec.scene(world).par_cast(cam, FNX, FNY, 1, seed=SEED, features={"grid": grid})
    _shares[(seed, grid)] = float(on_tri.mean())
    PR.compare_planes(ref, usable, fr.albedo, fr.normal, fr.depth, "mesh world %d grid %d" % (seed, grid), allow=allow)


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("seed", C.FREE)
def test_feature_planes_against_the_float64_reference(pkg, gpu, seed, grid):
    _feature_planes(pkg, gpu, seed, grid)
    if seed == IMAGE_WORLD:
        assert _shares[(seed, grid)] >= 0.02, _shares
