"""Flagged frames over several handles (include/rtiow_gpu.h at rtg_par_cast_multi, scene option multi_planes): with the option
on a handle, rtg_par_cast_multi takes RTG_FLAG_SUM_SQUARES, SAMPLE_COUNTS, RETIRE, DENOISE and FEATURES, and every 32-bit word of
the frame ends as the one-handle rtg_par_cast leaves it -- for 1, 2, 3, 5 and 8 handles, 8x8 and default tiles, whole frames and
PARTIAL / RESUME slices, through the same-device route and through RCCL.  The references are the one-handle call and the numpy
definitions (noise.py, denoise.py, feature_ref.py); without the option the library answers as before."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from feature_ref import reference_planes
from scene_cases import CASES, build_case

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")
NAN_BITS = 0x7FC0DEAD
TILES = ({"tile_w": 8, "tile_h": 8}, {})
ALL_FIVE = {"retire": {"target_se": 0.05, "min_samples": 4, "radius": 1}, "denoise": {"k": 0.7, "radius": 3, "patch": 1},
            "features": {"grid": 2}}


def _words(f):
    return (f.buf if hasattr(f, "buf") else f).view(np.uint32).reshape(-1)


def _frame(pkg, nx, ny, squares=False, counts=None, retire=None, denoise=None, features=None):
    """The frame of the flags' layout, every word a NaN canary, then the count plane and the blocks' in-fields.  counts: an
    array or a number; retire / denoise / features: dicts of the in-fields."""
    capi = pkg.capi
    if features is not None:
        f = capi.features_frame(nx, ny, squares, counts is not None, retire is not None, denoise, features)
    elif denoise is not None:
        f = capi.denoise_frame(nx, ny, counts is not None, retire is not None, denoise)
    elif counts is not None:
        f = capi.counts_frame(nx, ny, squares, retire is not None)
    else:
        return np.full(((2,) if squares else ()) + (ny, nx, 3), NAN_BITS, np.uint32).view(np.float32)
    _words(f)[...] = NAN_BITS
    if counts is not None:
        f.counts[...] = counts
    if retire is not None:
        block = capi.Retire()
        block.target_se, block.min_samples, block.radius = retire["target_se"], retire["min_samples"], retire["radius"]
        C.memmove(C.addressof(f.retire), C.addressof(block), capi.Retire.active.offset)
    if denoise is not None:
        block = capi.make_denoise(denoise)   # (a name keeps the block alive while memmove reads it)
        C.memmove(C.addressof(f.denoise), C.addressof(block), capi.Denoise.OUT_OFFSET)
    if features is not None:
        block = capi.make_features(features)
        C.memmove(C.addressof(f.features), C.addressof(block), capi.Features.OUT_OFFSET)
    return f


def _one(pkg, sg, cam, f, nx, ny, ns, **kw):
    """The one-handle rtg_par_cast into the frame, in place."""
    capi = pkg.capi
    if isinstance(f, capi.FeaturesFrame):
        return sg.par_cast(cam, nx, ny, ns, out=f, features=True, denoise=True if f.denoise is not None else None,
                           squares=f.squares, **kw)
    if isinstance(f, capi.DenoiseFrame):
        return sg.par_cast(cam, nx, ny, ns, out=f, denoise=True, squares=True, **kw)
    if isinstance(f, capi.CountsFrame):
        return sg.par_cast(cam, nx, ny, ns, out=f.planes, counts=f.counts, retire=f.retire, squares=f.planes.ndim == 4, **kw)
    return sg.par_cast(cam, nx, ny, ns, out=f, squares=f.ndim == 4, **kw)


def _many(gpu, scenes, cam, f, nx, ny, ns, **kw):
    """rtg_par_cast_multi into the frame, in place."""
    if isinstance(f, np.ndarray):
        return gpu.par_cast_multi(scenes, cam, nx, ny, ns, out=f, squares=f.ndim == 4, **kw)
    return gpu.par_cast_multi(scenes, cam, nx, ny, ns, out=f, **kw)


def _handles(pkg, gpu, name, nx, ny, n, last=("multi_planes",), every=()):
    """n fresh handles of a scene case, spread over (at most two of) the devices; options `last` on the last handle only."""
    n_dev = gpu.device_count()
    scenes, cam = [], None
    for i in range(n):
        b = gpu.builder()
        world, cam, _ = CASES[name][0](pkg, b, nx, ny)
        sg = b.scene(world, device=i % min(n_dev, 2))
        for o in every:
            sg.set_option(o, 1)
        scenes.append(sg)
    for o in last:
        scenes[-1].set_option(o, 1)
    return scenes, cam


def _same(got, want, what):
    a, b = _words(got), _words(want)
    assert a.shape == b.shape, what
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "%s: %d of %d words differ, first at word %d: %#x vs %#x" % (what, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]])


def _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, frames, calls, what, stats=False):
    """The same calls on the one-handle frame and the multi frame, each from its own output; every word equal after each."""
    f1, fm = frames
    for ns, kw in calls:
        r1 = _one(pkg, sg, cam, f1, nx, ny, ns, stats=stats, **kw)
        rm = _many(gpu, scenes, cam, fm, nx, ny, ns, stats=stats, **kw)
        _same(fm, f1, "%s, ns %d %s" % (what, ns, kw))
        if stats:
            for c in COUNTERS:
                assert rm[1][c] == r1[1][c], (what, ns, c, rm[1][c], r1[1][c])
            assert rm[1]["kernel_ms"] > 0


WHOLE = lambda ns: [(ns, {})]                                                                    # noqa: E731
SLICES = lambda a, b: [(a, {"partial": True}), (b, {"sample_begin": a, "resume": True})]         # noqa: E731


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_noise_planes(pkg, gpu, n):
    nx, ny, ns = 44, 28, 6
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    scenes, cam_m = _handles(pkg, gpu, "book1", nx, ny, n)
    for tiles in TILES:
        for calls in (WHOLE(ns), SLICES(2, ns)):
            calls = [(k, dict(kw, **tiles)) for k, kw in calls]
            frames = (_frame(pkg, nx, ny, squares=True), _frame(pkg, nx, ny, squares=True))
            _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, frames, calls, "squares, %d handles" % n, stats=True)


def _count_plane(nx, ny, top, seed=5):
    rs = np.random.RandomState(seed)
    n = rs.randint(1, top + 1, size=(ny, nx)).astype(np.uint32)
    n[rs.rand(ny, nx) < 0.2] = 0
    return n


@pytest.mark.parametrize("squares", [False, True])
def test_counts(pkg, gpu, squares):
    nx, ny, ns = 24, 24, 8
    counts = _count_plane(nx, ny, 12)
    assert (counts == 0).any() and (counts > ns).any() and counts.max() <= 12
    sg, cam, _, _, _ = build_case(pkg, gpu, "cornell", nx, ny)
    for n in (2, 3):
        scenes, _ = _handles(pkg, gpu, "cornell", nx, ny, n)
        for tiles in TILES:
            f1, fm = (_frame(pkg, nx, ny, squares=squares, counts=counts) for _ in range(2))
            _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, (f1, fm), [(ns, tiles)], "counts, %d handles" % n, stats=True)
            assert (fm.planes.view(np.uint32)[..., counts == 0, :] == NAN_BITS).all(), "pixels with n_p == 0 were written"
            assert (fm.counts == counts).all()


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_retire_across_ranks(pkg, gpu, radius):
    nx, ny, top = 44, 28, 12
    noise = pkg.noise
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    tiles = {"tile_w": 8, "tile_h": 8}
    # the target: the median over the pixels of the largest channel's standard error after the first slice, one handle
    plain = _frame(pkg, nx, ny, squares=True, counts=top)
    _one(pkg, sg, cam, plain, nx, ny, 4, partial=True, **tiles)
    se = noise.standard_error_counts(plain.planes[0], plain.planes[1], np.minimum(plain.counts, 4))
    target = float(np.median(se.max(axis=-1)))
    block = {"target_se": target, "min_samples": 2, "radius": radius}
    f1, fm = (_frame(pkg, nx, ny, squares=True, counts=top, retire=block) for _ in range(2))
    scenes, _ = _handles(pkg, gpu, "book1", nx, ny, 3)
    begin = 0
    for k in (4, 8):
        kw = dict(tiles, partial=True, sample_begin=begin, resume=begin > 0)
        before = fm.counts.copy()
        _one(pkg, sg, cam, f1, nx, ny, k, **kw)
        if k == 4:   # (the case cannot pass vacuously)
            assert 0 < f1.retire.retired and f1.retire.active > 0, (radius, f1.retire.as_dict())
        _many(gpu, scenes, cam, fm, nx, ny, k, **kw)
        _same(fm, f1, "retire radius %d at k = %d" % (radius, k))
        se_m = noise.standard_error_counts(fm.planes[0], fm.planes[1], np.minimum(before, k))
        want = noise.retire(before > k, k, se_m, 2, target, radius=radius, present=before > 0)
        assert fm.retire.retired == int(want.sum()) and ((fm.counts != before) == want).all(), (radius, k)
        begin = k


@pytest.mark.parametrize("name,nx,ny", [("book1", 44, 28), ("cornell", 24, 24)])
def test_filter_across_ranks(pkg, gpu, name, nx, ny):
    ns, dn = 8, {"k": 0.7, "radius": 3, "patch": 1}
    e = np.full((ny, nx), ns, np.uint32)
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    for n in (2, 3):
        scenes, _ = _handles(pkg, gpu, name, nx, ny, n)
        for tiles in TILES:
            for partial in (True, False):
                f1, fm = (_frame(pkg, nx, ny, squares=True, denoise=dn) for _ in range(2))
                _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, (f1, fm), [(ns, dict(tiles, partial=partial))], "%s filter, %d handles" % (name, n))
                if partial:   # (the running sums are still in the frame)
                    assert_bit_equal(fm.denoised, pkg.denoise.nlm(fm.planes[0], fm.planes[1], e, 3, 1, 0.7), "denoise.nlm of the multi call's own sums")
        # guided: the planes traced in the first of two slices, left alone in the second
        ft = {"grid": 2, "sigma_normal": 0.3, "sigma_albedo": 0.2, "sigma_depth": 0.1}
        f1, fm = (_frame(pkg, nx, ny, squares=True, denoise=dn, features=ft) for _ in range(2))
        _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, (f1, fm), [(4, {"partial": True})], "%s guided, slice 1" % name)
        f1.features.compute = fm.features.compute = 0
        _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, (f1, fm), [(ns, {"partial": True, "sample_begin": 4, "resume": True})], "%s guided, slice 2" % name)
        want = pkg.denoise.nlm_guided(fm.planes[0], fm.planes[1], e, fm.albedo, fm.normal, fm.depth, 3, 1, 0.7, 0.3, 0.2, 0.1)
        assert_bit_equal(fm.denoised, want, "denoise.nlm_guided of the multi call's own sums and planes")
        assert (fm.features.traced, fm.features.missed) == (0, 0)


def test_feature_planes_alone(pkg, gpu, oracle):
    nx, ny, ns = 40, 32, 2
    ref = reference_planes(pkg, oracle, "book2", nx, ny, 2)
    sg, cam, _, _, _ = build_case(pkg, gpu, "book2", nx, ny)
    scenes, _ = _handles(pkg, gpu, "book2", nx, ny, 3)
    for tiles in TILES:
        f1, fm = (_frame(pkg, nx, ny, features={"grid": 2}) for _ in range(2))
        _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, (f1, fm), [(ns, tiles)], "features alone")
        for got, want, plane in zip((fm.albedo, fm.normal, fm.depth), ref[:3], ("albedo", "normal", "depth")):
            assert_bit_equal(got, want, plane + " plane against the reference planes")
        assert (fm.features.traced, fm.features.missed) == (nx * ny, ref[3])


def test_everything_fed_forward(pkg, gpu):
    nx, ny = 40, 32
    counts = _count_plane(nx, ny, 14, seed=9)
    sg, cam, _, _, _ = build_case(pkg, gpu, "book2", nx, ny)
    scenes, _ = _handles(pkg, gpu, "book2", nx, ny, 3)
    f1, fm = (_frame(pkg, nx, ny, squares=True, counts=counts, **ALL_FIVE) for _ in range(2))
    begin = 0
    for k in (4, 8, 12):
        kw = {"partial": k != 12, "sample_begin": begin, "resume": begin > 0, "tile_w": 8, "tile_h": 8}
        _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, (f1, fm), [(k, kw)], "all five flags, slice ending at %d" % k, stats=True)
        f1.features.compute = fm.features.compute = 0
        begin = k


@pytest.mark.parametrize("parts", [{}, ALL_FIVE], ids=["squares_counts", "all_five"])
def test_more_handles_than_tiles(pkg, gpu, parts):
    """Two of the three ranks own no tile: they change nothing -- nor do their (zero) traced / missed counts in the sum."""
    nx, ny, ns = 16, 8, 4
    counts = _count_plane(nx, ny, 6)
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    scenes, _ = _handles(pkg, gpu, "book1", nx, ny, 3)
    f1, fm = (_frame(pkg, nx, ny, squares=True, counts=counts, **parts) for _ in range(2))
    _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, (f1, fm), [(ns, {"tile_w": 16, "tile_h": 16})], "one tile, three handles", stats=True)
    if parts:
        assert fm.features.traced == nx * ny


def test_through_rccl(pkg, gpu):
    nx, ny = 44, 28
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    gpu.multi_reset()
    calls = 0
    for n in (1, 3):
        scenes, _ = _handles(pkg, gpu, "book1", nx, ny, n, every=("force_rccl",))
        f1, fm = (_frame(pkg, nx, ny, squares=True, counts=10, **ALL_FIVE) for _ in range(2))
        _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, (f1, fm), [(4, {"partial": True})], "force_rccl, %d handles, slice 1" % n)
        f1.features.compute = fm.features.compute = 0   # (fewer planes travel: the transfers stay one per handle)
        _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, (f1, fm), [(8, {"sample_begin": 4, "resume": True})], "force_rccl, %d handles, slice 2" % n)
        calls += 2
    # one transfer per travelling handle and call: the first handle to itself on one GPU, the handle on the second device on two
    assert gpu.multi_reset() == calls


def test_refusals(pkg, gpu, oracle):
    capi = pkg.capi
    nx, ny, ns = 24, 16, 2
    so, cam_o, _, _, _ = build_case(pkg, oracle, "book1", nx, ny)
    ref = so.par_cast(cam_o, nx, ny, ns)
    # option off: as before
    scenes, cam = _handles(pkg, gpu, "book1", nx, ny, 2, last=())
    for flag in ("squares", "counts", "retire", "denoise", "features"):
        buf = np.full((2, ny, nx, 3) if flag == "squares" else (ny, nx, 3), NAN_BITS, np.uint32).view(np.float32)
        with pytest.raises(capi.RtError) as ei:
            gpu.par_cast_multi(scenes, cam, nx, ny, ns, out=buf, **{flag: True})
        assert ei.value.code == capi.ERR_UNSUPPORTED and "multi_planes" in str(ei.value), flag
        assert (buf.view(np.uint32) == NAN_BITS).all(), flag
    # option on: the refusals of the one-handle call, nothing written
    scenes[-1].set_option("multi_planes", 1)
    good = {"target_se": 0.1, "min_samples": 2, "radius": 1}
    cases = [
        ("radius 9", dict(counts=4, retire=dict(good, radius=9)), {}),
        ("target_se NaN", dict(counts=4, retire=dict(good, target_se=float("nan"))), {}),
        ("k NaN", dict(denoise={"k": float("nan"), "radius": 2, "patch": 1}), {}),
        ("patch 4", dict(denoise={"k": 0.7, "radius": 2, "patch": 4}), {}),
        ("grid 0", dict(features={"grid": 0}), {}),
        ("rank 1 of 2", dict(counts=4), {"rank": 1, "nranks": 2}),
    ]
    for what, parts, kw in cases:
        f = _frame(pkg, nx, ny, squares=True, **parts)
        before = _words(f).copy()
        with pytest.raises(capi.RtError) as ei:
            _many(gpu, scenes, cam, f, nx, ny, ns, **kw)
        assert ei.value.code == capi.ERR_INVALID, (what, str(ei.value))
        assert (_words(f) == before).all(), what + ": the refused call wrote"
    buf = np.full((8, ny, nx, 3), NAN_BITS, np.uint32).view(np.float32)   # (room for every plane, should the call write)
    with pytest.raises(capi.RtError) as ei:
        gpu._par_cast_multi_call(scenes, cam, capi.make_params(nx, ny, ns, squares=True, retire=True), buf)
    assert ei.value.code == capi.ERR_INVALID and (buf.view(np.uint32) == NAN_BITS).all(), "RETIRE without SAMPLE_COUNTS"
    assert_bit_equal(gpu.par_cast_multi(scenes, cam, nx, ny, ns), ref, "the handles after the refusals")


def test_plain_frame_with_the_option_on(pkg, gpu, oracle):
    nx, ny, ns = 96, 64, 6
    so, cam_o, _, _, _ = build_case(pkg, oracle, "book1", nx, ny)
    ref = so.par_cast(cam_o, nx, ny, ns)
    n_dev = gpu.device_count()
    for n in (1, 2, 3):
        scenes, cam = _handles(pkg, gpu, "book1", nx, ny, n)
        assert_bit_equal(gpu.par_cast_multi(scenes, cam, nx, ny, ns), ref, "plain frame, option on, %d handles" % n)
    gpu.multi_reset()
    for n in (1, 3):   # the reduce: one ncclReduce per distinct device and frame
        scenes, cam = _handles(pkg, gpu, "book1", nx, ny, n, every=("force_rccl",))
        assert_bit_equal(gpu.par_cast_multi(scenes, cam, nx, ny, ns), ref, "reduce, option on, %d handles" % n)
    assert gpu.multi_reset() == (2 if n_dev < 2 else 1 + 2)
    for n in (1, 3):   # the packed collective: one transfer per handle that travels
        scenes, cam = _handles(pkg, gpu, "book1", nx, ny, n, every=("force_rccl", "multi_gather"))
        assert_bit_equal(gpu.par_cast_multi(scenes, cam, nx, ny, ns), ref, "packed, option on, %d handles" % n)
    assert gpu.multi_reset() == 2


@pytest.mark.timeout(300)
def test_full_size(pkg, gpu):
    nx, ny, ns = 1200, 800, 4
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    scenes, _ = _handles(pkg, gpu, "book1", nx, ny, 8)
    parts = dict(ALL_FIVE, denoise={"k": 0.7, "radius": 5, "patch": 2})
    f1, fm = (_frame(pkg, nx, ny, squares=True, counts=8, **parts) for _ in range(2))
    _lock_step(pkg, gpu, sg, scenes, cam, nx, ny, (f1, fm), [(ns, {})], "1200 x 800, 8 handles, all five flags")
    assert fm.retire.estimated == nx * ny and fm.features.traced == nx * ny


@pytest.mark.parametrize("parts", [{}, {"radius": 1, "denoise": {"k": 0.7, "radius": 2, "patch": 1}, "features": {"grid": 2}}])
def test_adaptive_loop_over_several_handles(pkg, gpu, parts):
    """Backend.adaptive_multi yields what Scene.adaptive's host-frame loop yields, slice by slice."""
    nx, ny, ns, step = 24, 24, 12, 4
    sg, cam, _, _, _ = build_case(pkg, gpu, "cornell", nx, ny)
    scenes, _ = _handles(pkg, gpu, "cornell", nx, ny, 3)
    one = list(sg.adaptive(cam, nx, ny, ns, step, 0.05, min_samples=4, tile_w=8, tile_h=8, **parts))
    many = list(gpu.adaptive_multi(scenes, cam, nx, ny, ns, step, 0.05, min_samples=4, tile_w=8, tile_h=8, **parts))
    assert len(one) == len(many) >= 1
    for k, (a, b) in enumerate(zip(one, many)):
        assert len(a) == len(b) == 3 + (1 if "denoise" in parts else 0) + (1 if "features" in parts else 0)
        assert (a[0] == b[0]).all(), "counts after slice %d" % k
        assert_bit_equal(b[1], a[1], "preview after slice %d" % k)
        assert (a[2].view(np.uint64) == b[2].view(np.uint64)).all(), "standard errors after slice %d" % k
        if "denoise" in parts:
            assert_bit_equal(b[3], a[3], "filtered frame after slice %d" % k)
    if "features" in parts:   # (the loop yields its frame: the last state)
        _same(many[-1][-1], one[-1][-1], "the loops' frames")
