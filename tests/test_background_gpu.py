"""A background on the device (include/rtiow_gpu.h RTG_FLAG_BACKGROUND).

1. A constant background equals the dome, against the oracle: the frame is the oracle's frame of the same world with
   FlipNormals(Sphere 10000, DiffuseLight(c, 1.0)) appended; the counters are the oracle's for the world WITHOUT the dome.
2. The gradient, exact: a scene every ray of which misses; the frame equals the fold of background.sky over rays built in numpy.
3. The gradient on every scheduled kernel equals the baseline kernel's frame.
4. Flag off: the same handle with and without the flag, alternately; the unflagged frames are the oracle's (black misses).
5. Refusals write nothing.
6. rtg_par_cast_device and rtg_par_cast_multi equal rtg_par_cast.
7. The reference's picture (img/demo-scene.jpg has a gradient sky): the gradient render correlates with it at least as well as
   the dome render of the same call."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import assert_bit_equal
from fuzz_scenes import random_camera, random_world
from test_retire_gpu import _DeviceBuf, _hip

pytestmark = pytest.mark.gpu

COUNTERS = ("aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")   # rtg_stats: all five
NAN_BITS = 0x7FC0DEAD
SKY = (0.7, 0.8, 1.0)
BOOK = {"bottom": (1.0, 1.0, 1.0), "top": (0.5, 0.7, 1.0)}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dome(pkg, b, colour=SKY):
    return b.flip_normals(b.sphere(10000.0, b.diffuse_light(b.constant(pkg.scenes.v(*colour)), 1.0)))


def _book1(pkg, be, nx, ny, dome):
    """book-1 as one Bvh, with the dome inside it (the world of random_scene) or without a dome."""
    b = be.builder()
    if dome:
        world, cam, _ = pkg.scenes.random_scene(b, nx, ny)
    else:
        world, cam, _, bg = pkg.scenes.random_scene(b, nx, ny, sky="background")
        assert bg == {"bottom": SKY}
    return b.scene(world), cam


LIST_WORLDS = {
    "volume": lambda pkg, b, nx, ny: pkg.scenes.volume_test(b, nx, ny),
    "cornell": lambda pkg, b, nx, ny: pkg.scenes.cornell_box_scene(b, nx, ny),
    "book2": lambda pkg, b, nx, ny: pkg.scenes.book_final_scene(b, nx, ny, pkg.small_rng.SmallRng(0xDEADBEEF)),
}


def _list_world(pkg, be, name, nx, ny, dome):
    b = be.builder()
    world, cam, _ = LIST_WORLDS[name](pkg, b, nx, ny)
    return b.scene(world + ([_dome(pkg, b)] if dome else [])), cam


@pytest.fixture(scope="module")
def book1_ref(pkg, oracle):
    """(the oracle's frame of book-1 WITH the dome, its stats for book-1 WITHOUT the dome and its black-miss frame), 48x32x4"""
    nx, ny, ns = 48, 32, 4
    so, cam = _book1(pkg, oracle, nx, ny, True)
    img = so.par_cast(cam, nx, ny, ns)
    so2, cam2 = _book1(pkg, oracle, nx, ny, False)
    black, st = so2.par_cast(cam2, nx, ny, ns, stats=True)
    return img, st, black


def _check_stats(st_g, st_o, what):
    for k in COUNTERS:
        assert st_g[k] == st_o[k], (what, k, st_g[k], st_o[k])


# ---- 1. constant background = the dome ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "chunks1", "chunks2", "ray_lds0", "squares", "slices", "counts"])
def test_constant_equals_dome_book1(pkg, gpu, book1_ref, variant):
    nx, ny, ns = 48, 32, 4
    img_o, st_o, _ = book1_ref
    sg, cam = _book1(pkg, gpu, nx, ny, False)
    if variant.startswith("chunks"):
        sg.set_option("chunks", int(variant[-1]))
    if variant == "ray_lds0":
        sg.set_option("ray_lds", 0)
    if variant == "squares":   # the scratch path: one sample per work item, the fold kernel sums
        (planes, st) = sg.par_cast(cam, nx, ny, ns, squares=True, background=SKY, stats=True)
        assert_bit_equal(planes[0], img_o, "squares: plane 0")
        _check_stats(st, st_o, variant)
        return
    if variant == "slices":    # 2 + 2: a PARTIAL slice, then the RESUME slice that finishes the frame
        acc, st1 = sg.par_cast(cam, nx, ny, 2, partial=True, background=SKY, stats=True)
        out, st2 = sg.par_cast(cam, nx, ny, ns, out=acc, sample_begin=2, resume=True, background=SKY, stats=True)
        assert_bit_equal(out, img_o, "2 + 2 slices")
        for k in COUNTERS:
            assert st1[k] + st2[k] == st_o[k], (k, st1[k], st2[k], st_o[k])
        return
    if variant == "counts":    # a count plane: the block is read with the compaction result
        out, st = sg.par_cast(cam, nx, ny, ns, counts=np.full((ny, nx), ns, np.uint32), background=SKY, stats=True)
        assert_bit_equal(out, img_o, "counts = ns everywhere")
        _check_stats(st, st_o, variant)
        return
    out, st = sg.par_cast(cam, nx, ny, ns, background=SKY, stats=True)
    assert_bit_equal(out, img_o, variant + ", counting variant")
    _check_stats(st, st_o, variant)
    assert_bit_equal(sg.par_cast(cam, nx, ny, ns, background=SKY), img_o, variant + ", production variant")


@pytest.mark.parametrize("name", sorted(LIST_WORLDS))
def test_constant_equals_dome_list_worlds(pkg, gpu, oracle, name):
    nx, ny, ns = 32, 32, 8
    so, cam_o = _list_world(pkg, oracle, name, nx, ny, True)
    img_o = so.par_cast(cam_o, nx, ny, ns)
    so2, _ = _list_world(pkg, oracle, name, nx, ny, False)
    _, st_o = so2.par_cast(cam_o, nx, ny, ns, stats=True)
    sg, cam = _list_world(pkg, gpu, name, nx, ny, False)
    assert bytes(cam) == bytes(cam_o)
    # render_full_pool, the lock-step kernel, the pool-2 kernel (worlds that have a second program; the others stay on the first
    # kernel), the baseline kernel
    for opts in ({"sync": 0, "pool2": 0}, {"sync": 1, "pool2": 0}, {"sync": 0, "pool2": 2}, {"kernel": 1}):
        for o, v in opts.items():
            sg.set_option(o, v)
        out, st = sg.par_cast(cam, nx, ny, ns, background=SKY, stats=True)
        assert_bit_equal(out, img_o, "%s %s, counting variant" % (name, opts))
        _check_stats(st, st_o, (name, opts))
        assert_bit_equal(sg.par_cast(cam, nx, ny, ns, background=SKY), img_o, "%s %s, production variant" % (name, opts))


def _fuzz(pkg, be, seed, nx, ny, dome, **kw):
    rs = np.random.RandomState(seed)
    b = be.builder()
    world = random_world(pkg, b, rs, **kw)
    cam = random_camera(pkg, be, rs, nx, ny)
    return b, world + ([_dome(pkg, b)] if dome else []), cam


@pytest.mark.parametrize("seed", range(16))
def test_constant_equals_dome_fuzz_graphs(pkg, gpu, oracle, seed):
    nx, ny, ns = 24, 16, 4
    bo, wo, cam_o = _fuzz(pkg, oracle, 1000 + seed, nx, ny, True)
    img_o = bo.scene(wo).par_cast(cam_o, nx, ny, ns)
    bo2, wo2, _ = _fuzz(pkg, oracle, 1000 + seed, nx, ny, False)
    _, st_o = bo2.scene(wo2).par_cast(cam_o, nx, ny, ns, stats=True)
    bg_, wg, cam = _fuzz(pkg, gpu, 1000 + seed, nx, ny, False)
    sg = bg_.scene(wg)
    for sync, pool2 in ((0, 0), (0, 2), (1, 0)):
        sg.set_option("sync", sync)
        sg.set_option("pool2", pool2)
        out, st = sg.par_cast(cam, nx, ny, ns, background=SKY, stats=True)
        assert_bit_equal(out, img_o, "fuzz scene %d sync=%d pool2=%d" % (seed, sync, pool2))
        _check_stats(st, st_o, (seed, sync, pool2))


def test_constant_equals_dome_deep_graph(pkg, gpu, oracle):
    """A FEAT_DEEP graph: the general walk of the baseline kernel (rt_trace.h walk_deep)."""
    nx, ny, ns = 24, 16, 4
    kw = {"general_boundaries": True, "deep_shapes": True}
    for seed in range(9000, 9024):
        b, world, _ = _fuzz(pkg, gpu, seed, nx, ny, False, **kw)
        if b.flatten(world)[1] & 128:   # FEAT_DEEP (flat_scene.h)
            break
    else:
        pytest.fail("no FEAT_DEEP graph among the seeds")
    bo, wo, cam_o = _fuzz(pkg, oracle, seed, nx, ny, True, **kw)
    img_o = bo.scene(wo).par_cast(cam_o, nx, ny, ns)
    bo2, wo2, _ = _fuzz(pkg, oracle, seed, nx, ny, False, **kw)
    _, st_o = bo2.scene(wo2).par_cast(cam_o, nx, ny, ns, stats=True)
    bg_, wg, cam = _fuzz(pkg, gpu, seed, nx, ny, False, **kw)
    sg = bg_.scene(wg)
    for sized in (1, 0):
        sg.set_option("deep_sized", sized)
        out, st = sg.par_cast(cam, nx, ny, ns, background=SKY, stats=True)
        assert_bit_equal(out, img_o, "deep graph %d, deep_sized %d" % (seed, sized))
        _check_stats(st, st_o, (seed, sized))
        assert_bit_equal(sg.par_cast(cam, nx, ny, ns, background=SKY), img_o, "deep graph %d, production variant" % seed)


# ---- 2. the gradient, exact ------------------------------------------------------------------------------------------------
def _philox(oracle, key, ctr):
    out = (C.c_uint32 * 4)()
    oracle.lib.rto_debug_philox(C.c_uint32(key[0]), C.c_uint32(key[1]), *[C.c_uint32(c) for c in ctr], out)
    return [int(x) for x in out]


def _empty_sky_fold(pkg, oracle, cam, nx, ny, ns, seed, bg):
    """Every sample's camera ray in numpy (the stream layout of tests/test_rng.py: block 0 of event 0 of (seed, pixel, sample)
    holds r1, r2; Camera::get_ray, camera.rs:52-63, with a zero lens offset), background.sky of its direction, the left fold of
    the samples from +0: the undivided sums [ny, nx, 3]."""
    f = np.float32
    llc, hor, ver, org = (np.array(getattr(cam, k), dtype=f) for k in ("lower_left_corner", "horizontal", "vertical", "origin"))
    total = np.zeros((ny, nx, 3), dtype=f)
    for s in range(ns):
        d = np.zeros((ny, nx, 3), dtype=f)
        for row in range(ny):
            y = ny - 1 - row
            for x in range(nx):
                w = _philox(oracle, (seed & 0xffffffff, seed >> 32), (0, s, y * nx + x, 0))
                r1, r2 = f(w[0] >> 8) * f(1.0 / 16777216.0), f(w[1] >> 8) * f(1.0 / 16777216.0)
                u, v = (f(x) + r1) / f(nx), (f(y) + r2) / f(ny)
                d[row, x] = ((llc + u * hor) + v * ver) - org
        colour = pkg.background.miss_colour(d, bg["bottom"], bg["top"], 1)   # 0 + 1 * B(d)
        total = total + colour
    return total


def test_gradient_exact(pkg, gpu, oracle):
    S = pkg.scenes
    nx, ny, ns, seed = 40, 24, 3, 0x1234567887654321
    bg = {"bottom": (0.9, 0.25, 0.125), "top": (0.05, 0.6, 1.5)}
    b = gpu.builder()
    world = [b.translate(S.v(0.0, 0.0, 5.0), b.sphere(0.01, b.lambertian(b.constant(S.vfrom(0.5)))))]   # behind the camera
    cam = gpu.camera_look(S.v(0.0, 0.0, 0.0), S.v(0.0, 0.3, -1.0), S.v(0.0, 1.0, 0.0), 70.0, float(S.f32(nx) / S.f32(ny)), 0.0, 1.0)
    sg = b.scene(world)
    total = _empty_sky_fold(pkg, oracle, cam, nx, ny, ns, seed, bg)
    assert np.ptp(total[..., 0]) > 0.5   # (the frame is a gradient, not a constant)
    out, st = sg.par_cast(cam, nx, ny, ns, seed=seed, background=bg, stats=True)
    assert_bit_equal(out, total / np.float32(ns), "gradient frame vs the numpy fold")
    assert st["rays"] == nx * ny * ns and st["shaded_hits"] == 0
    assert_bit_equal(sg.par_cast(cam, nx, ny, ns, seed=seed, background=bg, partial=True), total, "PARTIAL: the undivided fold")
    sg.set_option("kernel", 1)
    assert_bit_equal(sg.par_cast(cam, nx, ny, ns, seed=seed, background=bg), total / np.float32(ns), "baseline kernel")


# ---- 3. the gradient across kernels ------------------------------------------------------------------------------------------
def test_gradient_across_kernels_book1(pkg, gpu):
    nx, ny, ns = 48, 32, 4
    ref_sg, cam = _book1(pkg, gpu, nx, ny, False)
    ref_sg.set_option("kernel", 1)
    ref = ref_sg.par_cast(cam, nx, ny, ns, background=BOOK)
    dome_sg, _ = _book1(pkg, gpu, nx, ny, True)
    assert not np.array_equal(ref, dome_sg.par_cast(cam, nx, ny, ns))   # (the gradient is another picture than the dome's)
    for opts in ({}, {"ray_lds": 0}, {"chunks": 1}, {"chunks": 2}, {"bvh4": 1}, {"box_tree": 0}, {"box_prune": 0, "box_chains": 0}):
        sg, _ = _book1(pkg, gpu, nx, ny, False)
        for o, v in opts.items():
            sg.set_option(o, v)
        assert_bit_equal(sg.par_cast(cam, nx, ny, ns, background=BOOK), ref, "lean pool kernel %s" % opts)
        out, _ = sg.par_cast(cam, nx, ny, ns, background=BOOK, stats=True)
        assert_bit_equal(out, ref, "lean pool kernel %s, counting variant" % opts)


def test_gradient_across_kernels_book2(pkg, gpu):
    nx, ny, ns = 32, 32, 8
    sg, cam = _list_world(pkg, gpu, "book2", nx, ny, False)
    sg.set_option("kernel", 1)
    ref = sg.par_cast(cam, nx, ny, ns, background=BOOK)
    sg.set_option("kernel", 3)
    assert not np.array_equal(ref, sg.par_cast(cam, nx, ny, ns))
    for opts in ({"sync": 0, "pool2": 0}, {"sync": 1, "pool2": 0}, {"sync": 0, "pool2": 2}, {"sync": 0, "pool2": 2, "mat_lds": 0}):
        for o, v in opts.items():
            sg.set_option(o, v)
        assert_bit_equal(sg.par_cast(cam, nx, ny, ns, background=BOOK), ref, "book-2 %s" % opts)
        out, _ = sg.par_cast(cam, nx, ny, ns, background=BOOK, stats=True)
        assert_bit_equal(out, ref, "book-2 %s, counting variant" % opts)


# ---- 4. flag off -----------------------------------------------------------------------------------------------------------
def test_flag_off_is_unchanged(pkg, gpu, oracle, book1_ref):
    nx, ny, ns = 48, 32, 4
    img_dome, _, black = book1_ref
    sg, cam = _book1(pkg, gpu, nx, ny, False)
    for _ in range(2):
        assert_bit_equal(sg.par_cast(cam, nx, ny, ns), black, "book-1 without the dome, no flag: black misses")
        assert_bit_equal(sg.par_cast(cam, nx, ny, ns, background=SKY), img_dome, "the same handle, with the flag")
    name, nx, ny, ns = "book2", 32, 32, 8
    so, cam_o = _list_world(pkg, oracle, name, nx, ny, False)
    black2 = so.par_cast(cam_o, nx, ny, ns)
    sg, cam = _list_world(pkg, gpu, name, nx, ny, False)
    for pool2 in (0, 2):
        sg.set_option("pool2", pool2)
        with_bg = sg.par_cast(cam, nx, ny, ns, background=BOOK)
        assert_bit_equal(sg.par_cast(cam, nx, ny, ns), black2, "book-2, no flag, pool2 = %d" % pool2)
        assert not np.array_equal(with_bg, black2)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [("mode", 2), ("reserved_in", 1)])
def test_refusals_write_nothing(pkg, gpu, field, value):
    capi = pkg.capi
    nx, ny, ns = 24, 16, 2
    sg, cam = _book1(pkg, gpu, nx, ny, False)
    hip = _hip()
    for kw in ({}, {"squares": True, "counts": True}, {"squares": True, "denoise": True, "features": True}):
        f = capi.Frame(nx, ny, **kw, background=SKY)
        f.buf.view(np.uint32)[...] = NAN_BITS
        if f.counts is not None:
            f.counts[...] = ns
        for block in (capi.make_denoise(True), capi.make_features(True)):
            if getattr(f, type(block).__name__.lower()) is not None:
                f.set_in(block)
        block = capi.make_background(SKY)
        setattr(block, field, value)
        f.set_in(block)
        keep = f.buf.view(np.uint32).copy()
        p = capi.make_params(nx, ny, ns, **f.flags())
        with pytest.raises(capi.RtError) as ei:
            sg.be.check(sg.be._par_cast(sg.h, C.byref(cam), C.byref(p), f.buf.ctypes.data_as(capi.c_f32p), None))
        assert ei.value.code == capi.ERR_INVALID and "RTG_FLAG_BACKGROUND" in str(ei.value)
        assert (f.buf.view(np.uint32) == keep).all(), "rtg_par_cast wrote to a refused frame (%s)" % kw
        dev = _DeviceBuf(hip, keep.nbytes)
        try:
            dev.put(keep)
            with pytest.raises(capi.RtError) as ei:
                sg.par_cast_device(cam, p, dev.p.value)
            assert ei.value.code == capi.ERR_INVALID
            assert (dev.get() == keep).all(), "rtg_par_cast_device wrote to a refused frame (%s)" % kw
        finally:
            dev.free()
        if not kw:   # rtg_par_cast_multi, both bodies read the host block
            for planes in (0, 1):
                sg.set_option("multi_planes", planes)
                with pytest.raises(capi.RtError) as ei:
                    gpu._par_cast_multi_call([sg], cam, p, f.buf)
                assert ei.value.code == capi.ERR_INVALID and (f.buf.view(np.uint32) == keep).all()


def test_debug_samples_refuses_the_flag(pkg, gpu):
    capi = pkg.capi
    nx, ny, ns = 24, 16, 2
    sg, cam = _book1(pkg, gpu, nx, ny, False)
    p = capi.make_params(nx, ny, ns, background=True)
    xs = np.zeros(4, np.uint32)
    rgb = np.full((4, 3), NAN_BITS, np.uint32)
    info = np.full((4, 4), NAN_BITS, np.uint32)
    rc = gpu._debug_samples(sg.h, C.byref(cam), C.byref(p), 4, xs.ctypes.data_as(capi.c_u32p), xs.ctypes.data_as(capi.c_u32p),
                            xs.ctypes.data_as(capi.c_u32p), rgb.ctypes.data_as(capi.c_f32p), info.ctypes.data_as(capi.c_u32p))
    assert rc == capi.ERR_INVALID and "RTG_FLAG_BACKGROUND" in gpu.last_error()
    assert (rgb == NAN_BITS).all() and (info == NAN_BITS).all()


# ---- 6. entry points -------------------------------------------------------------------------------------------------------
def test_par_cast_device_equals_par_cast(pkg, gpu):
    capi = pkg.capi
    nx, ny, ns = 48, 32, 4
    sg, cam = _book1(pkg, gpu, nx, ny, False)
    hip = _hip()
    for kw in ({}, {"squares": True, "counts": True}, {"squares": True, "denoise": True}):
        f = capi.Frame(nx, ny, **{k: (True if k != "denoise" else {"k": 0.7, "radius": 2, "patch": 1}) for k in kw}, background=BOOK)
        if f.counts is not None:
            f.counts[...] = ns
        start = f.buf.view(np.uint32).copy()
        p = capi.make_params(nx, ny, ns, **f.flags())
        dev = _DeviceBuf(hip, start.nbytes)
        try:
            dev.put(start)
            sg.par_cast_device(cam, p, dev.p.value)
            assert hip.hipDeviceSynchronize() == 0
            got = dev.get()
        finally:
            dev.free()
        sg.be.check(sg.be._par_cast(sg.h, C.byref(cam), C.byref(p), f.buf.ctypes.data_as(capi.c_f32p), None))
        want = f.buf.view(np.uint32)
        assert (got == want).all(), "device frame differs from the host call's (%s)" % kw
        at = f.layout.background
        assert (want[at:] == start[at:]).all()   # the block is in-only
        # ... and the binding's background= beside a device frame writes the block itself
        dev = _DeviceBuf(hip, start.nbytes)
        try:
            blank = start.copy()
            blank[at:] = 0
            dev.put(blank)
            sg.par_cast_device(cam, capi.make_params(nx, ny, ns, **{k: v for k, v in f.flags().items() if k != "background"}), dev.p.value,
                               background=BOOK)
            assert hip.hipDeviceSynchronize() == 0
            assert (dev.get() == want).all(), "par_cast_device(background=) (%s)" % kw
        finally:
            dev.free()


@pytest.mark.parametrize("n", [2, 3])
def test_par_cast_multi_equals_par_cast(pkg, gpu, n):
    nx, ny, ns = 48, 32, 4
    one, cam = _book1(pkg, gpu, nx, ny, False)
    want = one.par_cast(cam, nx, ny, ns, background=BOOK)
    assert not np.array_equal(want, one.par_cast(cam, nx, ny, ns))
    for gather in (0, 1):   # the reduce and the packed collective, both through RCCL on one device
        scenes = [_book1(pkg, gpu, nx, ny, False)[0] for _ in range(n)]
        scenes[-1].set_option("force_rccl", 1)
        scenes[-1].set_option("multi_gather", gather)
        got, st = gpu.par_cast_multi(scenes, cam, nx, ny, ns, background=BOOK, stats=True)
        assert_bit_equal(got, want, "%d handles, multi_gather %d" % (n, gather))
        _, st1 = one.par_cast(cam, nx, ny, ns, background=BOOK, stats=True)
        _check_stats(st, st1, (n, gather))
        acc = gpu.par_cast_multi(scenes, cam, nx, ny, 2, background=BOOK, partial=True)
        assert_bit_equal(gpu.par_cast_multi(scenes, cam, nx, ny, ns, out=acc, background=BOOK, sample_begin=2, resume=True), want,
                         "%d handles, 2 + 2 slices" % n)


def test_par_cast_multi_planes_equals_par_cast(pkg, gpu):
    """DENOISE | FEATURES | SAMPLE_COUNTS under multi_planes, against the one-handle call: every word of the frame."""
    capi = pkg.capi
    nx, ny, ns = 48, 32, 6
    parts = {"squares": True, "counts": True, "denoise": {"k": 0.7, "radius": 3, "patch": 1}, "features": {"grid": 2}}
    rs = np.random.RandomState(3)
    counts = rs.randint(0, ns + 3, (ny, nx)).astype(np.uint32)

    def frame():
        f = capi.FeaturesFrame(nx, ny, True, True, False, parts["denoise"], parts["features"], background=BOOK)
        keep_in = {name: bytes(getattr(f, name)) for name in ("denoise", "features", "background")}
        f.buf.view(np.uint32)[...] = NAN_BITS
        for name, raw in keep_in.items():
            C.memmove(C.addressof(getattr(f, name)), raw, type(getattr(f, name)).OUT_OFFSET)
        f.counts[...] = counts
        return f
    one, cam = _book1(pkg, gpu, nx, ny, False)
    f1 = frame()
    one.par_cast(cam, nx, ny, ns, out=f1, squares=True, denoise=True, features=True, background=True)
    for n in (2, 3):
        scenes = [_book1(pkg, gpu, nx, ny, False)[0] for _ in range(n)]
        scenes[-1].set_option("multi_planes", 1)
        scenes[-1].set_option("force_rccl", 1)
        fm = frame()
        gpu.par_cast_multi(scenes, cam, nx, ny, ns, out=fm, background=True)
        a, b = fm.buf.view(np.uint32), f1.buf.view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, "%d handles: %d words differ, first at word %d" % (n, bad.size, bad[0])
    # (the background changed the frame: the same call without it is another picture)
    f0 = capi.FeaturesFrame(nx, ny, True, True, False, parts["denoise"], parts["features"])
    f0.counts[...] = counts
    one.par_cast(cam, nx, ny, ns, out=f0, squares=True, denoise=True, features=True)
    assert not np.array_equal(f0.planes[0], f1.planes[0])
    assert_bit_equal(f0.albedo, f1.albedo, "feature planes do not see the background")
    assert_bit_equal(f0.depth, f1.depth, "feature planes do not see the background")


def test_loops_take_a_background(pkg, gpu):
    """progressive / adaptive with background=: the last preview is the one-call frame."""
    nx, ny, ns = 48, 32, 4
    sg, cam = _book1(pkg, gpu, nx, ny, False)
    want = sg.par_cast(cam, nx, ny, ns, background=BOOK)
    last = None
    for last in sg.progressive(cam, nx, ny, ns, 2, background=BOOK):
        pass
    assert last[0] == ns
    assert_bit_equal(last[1], want, "progressive(background=)")
    for last in sg.adaptive(cam, nx, ny, ns, 2, target_se=0.0, background=BOOK):
        pass
    assert (last[0] == ns).all()
    assert_bit_equal(last[1], want, "adaptive(background=)")


# ---- 7. the reference's picture ------------------------------------------------------------------------------------------------
def test_gradient_render_matches_the_reference_demo_image(pkg, gpu):
    """img/demo-scene.jpg was rendered with the book's gradient sky.  The dome render of the same call is the yardstick: the
    gradient render must correlate with the reference's picture at least as well, overall and on the ground."""
    nx, ny, ns = 300, 200, 200
    ref = np.load(os.path.join(GOLD, "ref_demo_scene_300x200.npz"))["rgb"].astype(np.float32)
    ground = slice(ny * 55 // 100, ny)

    def corr(a, b):
        return float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    sd, cam = _book1(pkg, gpu, nx, ny, True)
    dome = pkg.ppm.to_u8(sd.par_cast(cam, nx, ny, ns)).astype(np.float32)
    sb, _ = _book1(pkg, gpu, nx, ny, False)
    sky = pkg.ppm.to_u8(sb.par_cast(cam, nx, ny, ns, background=BOOK)).astype(np.float32)
    c_dome, c_sky = (corr(dome, ref), corr(dome[ground], ref[ground])), (corr(sky, ref), corr(sky[ground], ref[ground]))
    print("correlation with the reference's demo image (overall, ground): dome %.4f %.4f, gradient %.4f %.4f" % (c_dome + c_sky))
    assert c_sky[0] >= c_dome[0] and c_sky[1] >= c_dome[1]
