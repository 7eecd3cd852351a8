"""Scene option light_sampling (include/rtiow_gpu.h, at rtg_scene_set_option) on the GPU: the light table the library makes,
the frames that must not change, the routes that must agree bit for bit, and the estimator against a quadrature and against
the plain estimator -- every expectation from light_ref.py or from the plain frames, none from the option's own output.
Run with -s to see the z scores and variances the statistical tests assert on."""
import ctypes as C
import re

import numpy as np
import pytest

import light_ref as L
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu


def _scene(pkg, gpu, name, on=True):
    b, world, cam, n = L.build(pkg, gpu, name)
    sc = b.scene(world)
    if on:
        sc.set_option("light_sampling", 1)
    return sc, cam, b, world


@pytest.mark.parametrize("name", sorted(L.WORLDS))
def test_the_library_makes_the_table_of_the_rule(pkg, gpu, name, capfd):
    b, world, cam, n = L.build(pkg, gpu, name)
    want = len(L.light_table(b, world))
    assert want == n
    sc = b.scene(world)
    sc.set_option("verbose", 1)
    capfd.readouterr()
    if want > L.MAX_LIGHTS:
        with pytest.raises(pkg.RtError) as ei:
            sc.set_option("light_sampling", 1)
        assert ei.value.code == pkg.capi.ERR_INVALID
        sc.set_option("light_sampling", 0)
    else:
        sc.set_option("light_sampling", 1)
        err = capfd.readouterr().err
        got = re.findall(r"light table of (\d+) rect", err)
        assert got and int(got[-1]) == want, (name, got, want)
        # ... and every entry, in world order: axis, k, the two ranges, the float32 area, the material; and the sampled materials
        f32 = np.float32
        table = L.light_table(b, world)
        lines = re.findall(r"light: axis (\d+) k (\S+) r0 (\S+) (\S+) r1 (\S+) (\S+) area (\S+) material (\d+)", err)
        assert len(lines) == want
        for (axis, r0, r1, k, m), ln in zip(table, lines):
            area = (f32(r0[1]) - f32(r0[0])) * (f32(r1[1]) - f32(r1[0]))
            assert (int(ln[0]), [float(x) for x in ln[1:7]], int(ln[7])) == (axis, [k, r0[0], r0[1], r1[0], r1[1], float(area)], m), (name, ln)
        ids = re.findall(r"sampled materials:([ \d]*)", err)[-1].split()
        assert sorted(int(i) for i in ids) == sorted({e[4] for e in table}), (name, ids)
    sc.set_option("verbose", 0)
    with pytest.raises(pkg.RtError):
        sc.set_option("light_sampling", 2)


@pytest.mark.parametrize("name,nx,ny,kw", [("book1", 48, 32, {}), ("shared", 48, 48, {}), ("cornell", 48, 48, {"max_bounces": 0})])
def test_nothing_to_sample_changes_no_bit(pkg, gpu, name, nx, ny, kw):
    """No table (book 1, the light material a sphere shares), or a cap that lets no hit take a light sample."""
    ns = 4
    on, cam, _, _ = _scene(pkg, gpu, name)
    off, _, _, _ = _scene(pkg, gpu, name, on=False)
    a, st_a = on.par_cast(cam, nx, ny, ns, stats=True, **kw)
    b, st_b = off.par_cast(cam, nx, ny, ns, stats=True, **kw)
    assert_bit_equal(a, b, name)
    for k in ("samples", "rays", "draws", "shaded_hits"):
        assert st_a[k] == st_b[k], (name, k)
    assert a.max() > 0


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def test_every_route_gives_the_same_bits(pkg, gpu):
    nx, ny, ns = 48, 48, 16
    sc, cam, _, _ = _scene(pkg, gpu, "cornell")
    plain_sc, _, _, _ = _scene(pkg, gpu, "cornell", on=False)
    ref, st = sc.par_cast(cam, nx, ny, ns, stats=True)
    plain, st_plain = plain_sc.par_cast(cam, nx, ny, ns, stats=True)
    assert (ref != plain).any(), "the option changed nothing"
    # rtg_stats counts what runs: the shadow rays, the three light draws of every sampling hit; samples unchanged
    assert st["samples"] == st_plain["samples"] == nx * ny * ns
    assert st["rays"] > st_plain["rays"] and st["draws"] > st_plain["draws"]
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns), ref, "timed vs instrumented")
    # PARTIAL / RESUME slices of 4
    acc = np.zeros((ny, nx, 3), np.float32)
    for begin in range(0, ns, 4):
        sc.par_cast(cam, nx, ny, begin + 4, out=acc, sample_begin=begin, resume=True, partial=begin + 4 != ns)
    assert_bit_equal(acc, ref, "slices of 4")
    # plane 0 of a SUM_SQUARES call; its plane 1 against the fold of the probe's colours below
    planes = sc.par_cast(cam, nx, ny, ns, squares=True)
    assert_bit_equal(planes[0], ref, "plane 0 of the squares call")
    # a counts call with n_p = ns
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns, counts=np.full((ny, nx), ns, np.uint32)), ref, "counts call")
    # rtg_par_cast_device
    hip = _hip()
    buf = C.c_void_p()
    nbytes = nx * ny * 3 * 4
    assert hip.hipMalloc(C.byref(buf), nbytes) == 0
    try:
        assert hip.hipMemset(buf, 0xFF, nbytes) == 0
        sc.par_cast_device(cam, pkg.capi.make_params(nx, ny, ns), buf.value, None)
        got = np.empty((ny, nx, 3), np.float32)
        assert hip.hipMemcpy(got.ctypes.data, buf, nbytes, 2) == 0
    finally:
        hip.hipFree(buf)
    assert_bit_equal(got, ref, "device entry point")
    # rtg_par_cast_multi over two handles; mixed handles are refused
    sc2, _, _, _ = _scene(pkg, gpu, "cornell")
    assert_bit_equal(gpu.par_cast_multi([sc, sc2], cam, nx, ny, ns), ref, "two handles")
    with pytest.raises(pkg.RtError) as ei:
        gpu.par_cast_multi([sc, plain_sc], cam, nx, ny, ns)
    assert ei.value.code == pkg.capi.ERR_INVALID
    with pytest.raises(pkg.RtError) as ei:
        gpu.par_cast_multi([plain_sc, sc], cam, nx, ny, ns)
    assert ei.value.code == pkg.capi.ERR_INVALID
    # the ordered float32 fold of the default probe over every key; the kernel trace has nothing to read on baseline frames
    rows, xs = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    rgb, _ = sc.debug_samples(cam, nx, ny, ns, np.tile(xs.ravel(), ns), np.tile((ny - 1 - rows).ravel(), ns), np.repeat(np.arange(ns), nx * ny))
    c = rgb.reshape(ns, ny, nx, 3)
    s, q = np.zeros((ny, nx, 3), np.float32), np.zeros((ny, nx, 3), np.float32)
    for k in range(ns):
        s, q = s + c[k], q + c[k] * c[k]
    assert_bit_equal(s / np.float32(ns), ref, "fold of debug_samples")
    assert_bit_equal(q, planes[1], "fold of the squares of debug_samples")
    with pytest.raises(pkg.RtError) as ei:
        sc.debug_samples(cam, nx, ny, ns, [1], [1], [0], trace_kernel=True)
    assert ei.value.code == pkg.capi.ERR_UNSUPPORTED
    # options kernel and bvh4 are ignored meanwhile; switching the option off gives the plain frame back
    sc.set_option("kernel", 1)
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns), ref, "option kernel = 1")
    sc.set_option("kernel", 3)
    sc.set_option("light_sampling", 0)
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns), plain, "option off again")


def _floor_points(cam, nx, ny):
    """Where the ray through every pixel centre meets the plane y = 0 (row 0 = top), float64."""
    o, llc, h, v = (np.array(list(a), np.float64) for a in (cam.origin, cam.lower_left_corner, cam.horizontal, cam.vertical))
    rows, xs = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    d = llc + ((xs + 0.5) / nx)[..., None] * h + ((ny - 1 - rows + 0.5) / ny)[..., None] * v - o
    t = -o[1] / d[..., 1]
    assert (t > 0).all()
    return o + t[..., None] * d


def test_against_quadrature(pkg, gpu):
    """One bounce under one rect light: every pixel is 0.5 * Le * integral of lobe * cos_l / r2 over the light, at the floor
    point of the pixel's centre.  The frame mean within 4 standard errors, every pixel-channel within 5, and the frame mean
    more than 5 away from the quadrature of each planted variant (cos / pi lobe, no cos_l, no area factor).
    Measured: frame z -1.0 per channel at a relative standard error of 0.14 %, worst pixel-channel |z| 3.3; planted cosine
    292, no_cos_l -61, no_area 357.  (The pixel-centre rule is 0.06 % above the average over the pixels' footprints, float64.)"""
    import physics_ref
    nx = ny = 16
    ns = 256
    b = physics_ref.Recorder(gpu.builder())
    world, cam = L.quadrature_world(pkg, b)
    (axis, r0, r1, k, m), = L.light_table(b, world)
    le = np.array([4.0, 2.0, 1.0]) * b.materials[m][2]
    sc = b.scene(world)
    sc.set_option("light_sampling", 1)
    planes = sc.par_cast(cam, nx, ny, ns, squares=True, max_bounces=1)
    mean, var = L.mean_and_variance(planes, ns)
    pts = _floor_points(cam, nx, ny)
    assert (np.abs(pts[..., 0]) < 4).all() and (np.abs(pts[..., 2]) < 4).all()
    n = np.array([0.0, 1.0, 0.0])

    g = [[L.direct_all(pts[r, c], n, axis, r0, r1, k) for c in range(nx)] for r in range(ny)]

    def want(variant=None):
        return 0.5 * np.array([[cell[variant] for cell in row] for row in g])[..., None] * le
    w = want()
    z_pix = (mean - w) / np.sqrt(var)
    se_frame = np.sqrt(var.sum((0, 1))) / (nx * ny)
    z_frame = (mean.mean((0, 1)) - w.mean((0, 1))) / se_frame
    print("quadrature: frame z %s, worst pixel-channel |z| %.2f, relative standard error of the frame mean %s" % (
        np.round(z_frame, 2), np.abs(z_pix).max(), np.round(se_frame / w.mean((0, 1)), 5)))
    planted = {}
    for variant in L.VARIANTS:
        planted[variant] = (mean.mean((0, 1)) - want(variant).mean((0, 1))) / se_frame
        print("  planted %-8s: frame z %s" % (variant, np.round(planted[variant], 1)))
    assert (var > 0).all()
    assert (np.abs(z_frame) <= 4).all(), z_frame
    assert np.abs(z_pix).max() <= 5, np.abs(z_pix).max()
    for variant, z in planted.items():
        assert (np.abs(z) > 5).all(), (variant, z)


@pytest.mark.parametrize("name", ["cornell", "volume"])
def test_against_the_plain_estimator(pkg, gpu, name):
    """A: the option off, 1024 samples, seed 1.  B: the option on, 64 samples, seed 2.  No 8 x 8 block-channel further apart
    than 5 standard errors, no channel of the frame mean further than 4 -- and at 64 samples of one seed the option's summed
    variance of the pixel means is below the plain frame's.
    Measured: cornell block |z| max 2.7, frame z 2.4 / 2.3 / 2.1, variance 191 -> 99; volume 2.6, 2.1 / 2.0 / 2.2, 146 -> 100.
    The frame z are positive on every seed tried (1.8 .. 3.3 against 16 384 plain samples): the estimator is unbiased but
    heavy-tailed -- Cornell's light hangs one unit under the ceiling and emits upwards too, so ceiling points beside it draw,
    rarely, samples 10^3 times their mean, and a 64-sample frame that misses them reads 1-2 % low (at 16 384 samples the
    difference is +0.7 %, z -1.0; HISTORY.md "Light sampling").  The conditions are the ones set for the feature; with
    fixed seeds the frames, and so the verdict, are the same on every run."""
    nx = ny = 64
    on, cam, _, _ = _scene(pkg, gpu, name)
    off, _, _, _ = _scene(pkg, gpu, name, on=False)
    a = off.par_cast(cam, nx, ny, 1024, seed=1, squares=True)
    b = on.par_cast(cam, nx, ny, 64, seed=2, squares=True)
    c = off.par_cast(cam, nx, ny, 64, seed=2, squares=True)
    zb, zf = L.block_z(a, 1024, b, 64)
    var_on, var_off = L.mean_and_variance(b, 64)[1].sum(), L.mean_and_variance(c, 64)[1].sum()
    print("%s: block |z| max %.2f, frame z %s, summed variance at 64 samples: option %.4g, plain %.4g (x %.1f)" % (
        name, np.abs(zb).max(), np.round(zf, 2), var_on, var_off, var_off / var_on))
    assert np.abs(zb).max() <= 5, np.abs(zb).max()
    assert (np.abs(zf) <= 4).all(), zf
    assert var_on < var_off


def test_the_general_walk_gives_the_flat_interpreter_s_bits(pkg, gpu, capfd):
    """The same world as a flat program and, its occluder under five Translates by zero, as a graph only the general walk
    renders (light_ref.WORLDS "shallow" / "deep"): hit_top and the shadow ray take walk_deep, the latter returning at its
    first accepted hit, the fog drawing inside it.  Frames, squares, counters and single samples agree bit for bit, through
    every instantiation of the light kernels; so do the plain frames, the control."""
    nx, ny, ns = 40, 40, 8
    frames = {}
    for name in ("shallow", "deep"):
        on, cam, _, _ = _scene(pkg, gpu, name)
        off, _, _, _ = _scene(pkg, gpu, name, on=False)
        # which walk: without the option the flat program renders on a pool kernel, the deep graph on the baseline kernel
        off.set_option("verbose", 1)
        capfd.readouterr()
        off.par_cast(cam, nx, ny, ns)
        assert ("[rtg] full pool" in capfd.readouterr().err) == (name == "shallow")
        off.set_option("verbose", 0)
        counted, st = on.par_cast(cam, nx, ny, ns, stats=True)
        rows, xs = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        rgb, info = on.debug_samples(cam, nx, ny, ns, np.tile(xs.ravel(), ns), np.tile((ny - 1 - rows).ravel(), ns), np.repeat(np.arange(ns), nx * ny))
        half = np.full((ny, nx), ns // 2, np.uint32)
        half[::3] = ns
        frames[name] = {
            "timed": on.par_cast(cam, nx, ny, ns), "counted": counted,
            "counters": np.array([st[k] for k in ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")], np.float64),
            "squares": on.par_cast(cam, nx, ny, ns, squares=True), "squares counted": on.par_cast(cam, nx, ny, ns, squares=True, stats=True)[0],
            "counts": on.par_cast(cam, nx, ny, ns, counts=half), "counts counted": on.par_cast(cam, nx, ny, ns, counts=half, stats=True)[0],
            "counts squares": on.par_cast(cam, nx, ny, ns, counts=half, squares=True),
            "counts squares counted": on.par_cast(cam, nx, ny, ns, counts=half, squares=True, stats=True)[0],
            "samples": rgb, "sample info": info[:, :2].astype(np.float64), "plain": off.par_cast(cam, nx, ny, ns),
        }
    a, b = frames["shallow"], frames["deep"]
    assert (a["timed"] != a["plain"]).any() and a["timed"].max() > 0
    assert_bit_equal(a["timed"], a["counted"], "shallow: timed vs instrumented")
    for k in a:
        assert_bit_equal(a[k], b[k], "shallow vs deep: " + k)
    assert a["counters"][4] > 2 * a["counters"][0]   # camera rays, scattered rays and shadow rays


def test_two_lights_against_the_plain_estimator(pkg, gpu):
    """Two sampled materials (two axes, two areas, two colours, one rect flipped) against the plain estimator, under the
    thresholds of test_against_the_plain_estimator: a table in the wrong order, or an entry with another entry's area,
    axis or material, moves the frame by tens of per cent."""
    nx = ny = 64
    on, cam, _, _ = _scene(pkg, gpu, "two_lights")
    off, _, _, _ = _scene(pkg, gpu, "two_lights", on=False)
    a = off.par_cast(cam, nx, ny, 1024, seed=1, squares=True)
    b = on.par_cast(cam, nx, ny, 64, seed=2, squares=True)
    c = off.par_cast(cam, nx, ny, 64, seed=2, squares=True)
    zb, zf = L.block_z(a, 1024, b, 64)
    var_on, var_off = L.mean_and_variance(b, 64)[1].sum(), L.mean_and_variance(c, 64)[1].sum()
    print("two_lights: block |z| max %.2f, frame z %s, summed variance at 64 samples: option %.4g, plain %.4g" % (
        np.abs(zb).max(), np.round(zf, 2), var_on, var_off))
    assert np.abs(zb).max() <= 5, np.abs(zb).max()
    assert (np.abs(zf) <= 4).all(), zf
