"""Feature planes on the device (include/rtiow_gpu.h RTG_FLAG_FEATURES): the albedo, normal and depth planes equal the reference
planes (features.subpixel_rays, the oracle's hit_top, a numpy albedo evaluator, the fold) bit for bit on every scene case and
grid, on ragged frames and across ranks; compute = 0 leaves them alone; with RTG_FLAG_DENOISE the output plane equals
denoise.nlm_guided of the frame's own running sums and feature planes -- on planted data, slice by slice, with count planes and
the retire step, from both entry points and at full size; everything else in the frame ends as without the flag; refused
calls write nothing."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal, bits
from feature_ref import reference_planes
from scene_cases import CASES, build_case
from test_denoise_abi import random_sums
from test_denoise_gpu import _plain_slices
from test_features_abi import random_features
from test_retire_gpu import _DeviceBuf, _hip

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")
NAN_BITS = 0x7FC0DEAD
RF = [(0, 0), (1, 0), (5, 2), (8, 3)]
SIGMAS = [(0.3, 0.2, 0.1), (1e18, 0.05, 2.0)]


def _words(f):
    return f.buf.view(np.uint32)


def _canary_frame(pkg, nx, ny, squares=False, counts=False, retire=False, denoise=None, features=None):
    """A FeaturesFrame filled with a NaN canary, its blocks' in-fields set."""
    capi = pkg.capi
    f = capi.features_frame(nx, ny, squares, counts, retire, denoise)
    _words(f)[...] = NAN_BITS
    if f.denoise is not None:
        block = capi.make_denoise(None if denoise is True else denoise)
        C.memmove(C.addressof(f.denoise), C.addressof(block), capi.Denoise.OUT_OFFSET)
    block = capi.make_features(features)
    C.memmove(C.addressof(f.features), C.addressof(block), capi.Features.OUT_OFFSET)
    return f


def _check_planes(f, ref, what, owned=None):
    """The frame's three planes against the reference planes (on `owned` pixels; the others keep the canary)."""
    for got, want, name in zip((f.albedo, f.normal, f.depth), ref[:3], ("albedo", "normal", "depth")):
        if owned is None:
            assert_bit_equal(got, want, "%s: %s plane" % (what, name))
        else:
            assert_bit_equal(got[owned], want[owned], "%s: %s plane, owned pixels" % (what, name))
            assert (bits(got)[~owned] == NAN_BITS).all(), "%s: %s plane written outside the rank's tiles" % (what, name)
    assert all(w == 0 for w in f.features.reserved) and f.features.reserved_in == 0, what


def _check_guided(pkg, f, S, Q, e, what):
    """The output plane against denoise.nlm_guided of (S, Q, e) and the frame's own feature planes; the denoise block's fields."""
    d, ft = f.denoise, f.features
    want = pkg.denoise.nlm_guided(S, Q, e, f.albedo, f.normal, f.depth, d.radius, d.patch, d.k, ft.sigma_normal, ft.sigma_albedo,
                                  ft.sigma_depth)
    held = e > 0
    assert_bit_equal(f.denoised[held], want[held], what + ": output plane")
    assert (bits(f.denoised)[~held] == NAN_BITS).all(), what + ": pixels without samples were written"
    valid = pkg.denoise.mean_var(S, Q, e)[2]
    assert d.filtered == int(valid.sum()) and d.filtered + d.passed == int(held.sum()), (what, d.filtered, d.passed)
    assert all(w == 0 for w in d.reserved) and d.reserved_in == 0, what


@pytest.mark.parametrize("name", sorted(CASES))
def test_planes_of_every_scene_case(pkg, gpu, oracle, name):
    sg, cam, nx, ny, ns = build_case(pkg, gpu, name)
    plain, st_plain = sg.par_cast(cam, nx, ny, ns, stats=True)
    for grid in (1, 2, 3):
        what = "%s grid %d" % (name, grid)
        ref = reference_planes(pkg, oracle, name, nx, ny, grid)
        f = _canary_frame(pkg, nx, ny, features={"grid": grid})
        got, st = sg.par_cast(cam, nx, ny, ns, out=f, features=True, stats=True)
        assert got is f
        _check_planes(f, ref, what)
        assert (f.features.traced, f.features.missed) == (nx * ny, ref[3]), (what, f.features.as_dict(), ref[3])
        assert (f.features.grid, f.features.compute) == (grid, 1)
        assert_bit_equal(f.planes, plain, what + ": plane 0 with the flag")
        for c in COUNTERS:   # feature rays are not counted
            assert st[c] == st_plain[c], (what, c, st[c], st_plain[c])
    # arrays of the caller's: a new frame carries them
    out = np.zeros((ny, nx, 3), np.float32)
    g = sg.par_cast(cam, nx, ny, ns, out=out, features={"grid": 3})
    assert_bit_equal(out, plain, name + ": out= array")
    _check_planes(g, ref, name + ": staged frame")


@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (200, 3), (29, 37)])
def test_ragged_frames(pkg, gpu, oracle, shape):
    ny, nx = shape
    sg, cam, _, _, _ = build_case(pkg, gpu, "book2", nx, ny)
    ref = reference_planes(pkg, oracle, "book2", nx, ny, 2)
    f = _canary_frame(pkg, nx, ny, features={"grid": 2})
    sg.par_cast(cam, nx, ny, 2, out=f, features=True)
    _check_planes(f, ref, "book2 %s" % (shape,))
    assert (f.features.traced, f.features.missed) == (nx * ny, ref[3])


def test_ranks_write_their_own_pixels(pkg, gpu, oracle):
    ny, nx = 29, 37
    sg, cam, _, _, _ = build_case(pkg, gpu, "book2", nx, ny)
    ref = reference_planes(pkg, oracle, "book2", nx, ny, 2)
    rows, xs = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    tile = (rows // 8) * ((nx + 7) // 8) + xs // 8
    whole = _canary_frame(pkg, nx, ny, features={"grid": 2})
    traced = missed = 0
    for rank in (0, 1):
        owned = tile % 2 == rank
        f = _canary_frame(pkg, nx, ny, features={"grid": 2})
        sg.par_cast(cam, nx, ny, 2, out=f, features=True, tile_w=8, tile_h=8, rank=rank, nranks=2)
        _check_planes(f, ref, "rank %d" % rank, owned)
        assert f.features.traced == int(owned.sum())
        assert f.features.missed == int((owned & (ref[2] == 0) & (ref[0] == 0).all(axis=-1)).sum())
        traced, missed = traced + f.features.traced, missed + f.features.missed
        sg.par_cast(cam, nx, ny, 2, out=whole, features=True, tile_w=8, tile_h=8, rank=rank, nranks=2)   # (the other rank's pixels stay)
    _check_planes(whole, ref, "the two ranks together")
    assert (traced, missed) == (nx * ny, ref[3])


def test_compute_0_leaves_the_planes_alone(pkg, gpu):
    nx, ny, ns = 37, 29, 3
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    plain = sg.par_cast(cam, nx, ny, ns)
    f = _canary_frame(pkg, nx, ny, features={"grid": 2, "compute": 0})
    f.features.traced = f.features.missed = 77
    sg.par_cast(cam, nx, ny, ns, out=f, features=True)
    for plane in (f.albedo, f.normal, f.depth):
        assert (bits(plane) == NAN_BITS).all()
    assert f.features.as_dict() == {"traced": 0, "missed": 0} and all(w == 0 for w in f.features.reserved)
    assert_bit_equal(f.planes, plain, "plane 0")
    hip = _hip()
    dev = _DeviceBuf(hip, f.buf.nbytes)
    try:
        keep = f.buf.copy()
        dev.put(keep)
        sg.par_cast_device(cam, pkg.capi.make_params(nx, ny, ns, features=True), dev.p.value)
        assert (dev.get() == keep.view(np.uint32)).all()   # (the out-fields were 0 already)
    finally:
        dev.free()


@pytest.mark.parametrize("shape", [(9, 13), (1, 1), (3, 200), (48, 64), (29, 37)])
def test_guided_filter_on_planted_data(pkg, gpu, shape):
    ny, nx = shape
    ns = 8
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    S, Q, n = random_sums(ny, nx, 7 * ny + nx)
    a, nn, z = random_features(ny, nx, 3 * ny + nx)
    try:
        for counts in (False, True):
            e = np.minimum(n, ns).astype(np.uint32) if counts else np.full((ny, nx), ns, np.uint32)
            for (R, F), sig in zip(RF + RF, [SIGMAS[0]] * 4 + [SIGMAS[1]] * 4):
                want = None
                for lds in (0, 1):   # the neighbours' feature records through the caches / from LDS
                    sg.set_option("guide_lds", lds)
                    what = "%s counts=%s R %d F %d sigmas %s lds %d" % (shape, counts, R, F, sig, lds)
                    f = _canary_frame(pkg, nx, ny, True, counts, denoise={"k": 1.5, "radius": R, "patch": F},
                                      features={"compute": 0, "sigma_normal": sig[0], "sigma_albedo": sig[1], "sigma_depth": sig[2]})
                    f.planes[0], f.planes[1] = S, Q
                    f.albedo[...], f.normal[...], f.depth[...] = a, nn, z
                    if counts:
                        f.counts[...] = n
                    before = f.buf.copy().view(np.uint32)
                    sg.par_cast(cam, nx, ny, ns, out=f, denoise=True, features=True, sample_begin=ns, resume=True, partial=True,
                                squares=True)
                    d_off, f_off = capi.denoise_block_offset(nx, ny, counts) // 4, capi.features_block_offset(nx, ny, True, counts, False, True) // 4
                    assert (_words(f)[:d_off + 4] == before[:d_off + 4]).all(), what + ": planes / counts / in-fields written"
                    assert (_words(f)[f_off:f_off + 6] == before[f_off:f_off + 6]).all(), what + ": features in-fields written"
                    assert (_words(f)[f_off + 16:] == before[f_off + 16:]).all(), what + ": feature planes written"
                    assert f.features.as_dict() == {"traced": 0, "missed": 0}
                    if want is None:
                        _check_guided(pkg, f, S, Q, e, what)
                        want = f.denoised.copy()
                    else:
                        assert (bits(f.denoised) == bits(want)).all(), what + ": the two variants differ"
    finally:
        sg.set_option("guide_lds", 0)


@pytest.mark.parametrize("name", ["book1", "cornell", "book2"])
def test_slices(pkg, gpu, oracle, name):
    nx, ny, ns, cuts = 48, 32, 9, (2, 5, 9)
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    ref = sg.par_cast(cam, nx, ny, ns, squares=True)
    sums = _plain_slices(pkg, sg, cam, nx, ny, cuts)
    planes = reference_planes(pkg, oracle, name, nx, ny, 2)
    f = _canary_frame(pkg, nx, ny, True, denoise={"k": 1.0, "radius": 3, "patch": 1}, features={"grid": 2})
    begin = 0
    for end, s in zip(cuts, sums):
        sg.par_cast(cam, nx, ny, end, out=f, denoise=True, features=True, sample_begin=begin, resume=True, partial=end != ns, squares=True)
        what = "%s slice to %d" % (name, end)
        _check_planes(f, planes, what)
        assert f.features.traced == (nx * ny if begin == 0 else 0), what
        f.features.compute = 0   # traced on the first slice only
        _check_guided(pkg, f, s[0], s[1], np.full((ny, nx), end, np.uint32), what)
        if end != ns:
            assert_bit_equal(f.planes, s, "%s: running sums at %d" % (name, end))
        begin = end
    assert_bit_equal(f.planes, ref, name + ": the last slice divides plane 0")
    # the loops of the binding: features traced by the first slice, the planes of every item the reference's
    last = None
    for t in sg.progressive(cam, nx, ny, ns, 4, features={"grid": 2}, denoise={"k": 1.0, "radius": 3, "patch": 1}):
        assert len(t) == 5
        done, _, _, den, fr = t
        _check_planes(fr, planes, "%s progressive at %d" % (name, done))
        assert fr.features.compute == 0 and fr.features.traced == (nx * ny if done == 4 else 0)
        last = den
    assert_bit_equal(last, f.denoised, name + ": progressive, the last filtered frame")
    plain_loop = [t[1] for t in sg.progressive(cam, nx, ny, ns, 4)]
    feat_loop = list(sg.progressive(cam, nx, ny, ns, 4, features=True))
    assert all(len(t) == 3 for t in feat_loop)
    for a, t in zip(plain_loop, feat_loop):
        assert_bit_equal(t[1], a, name + ": preview with features=")


@pytest.mark.parametrize("name,target", [("book1", 0.15), ("cornell", 2.0)])
def test_counts_and_retire_in_the_same_call(pkg, gpu, oracle, name, target):
    nx, ny, ns, half = 40, 24, 12, 6
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    planes = reference_planes(pkg, oracle, name, nx, ny, 1)
    rs = np.random.RandomState(11)
    n = rs.randint(0, ns + 4, size=(ny, nx)).astype(np.uint32)
    n[rs.rand(ny, nx) < 0.5] = ns + 2
    plain = capi.counts_frame(nx, ny, squares=True, retire=True)
    f = _canary_frame(pkg, nx, ny, True, True, True, features={"grid": 1})
    g = _canary_frame(pkg, nx, ny, True, True, True, denoise={"k": 0.7, "radius": 2, "patch": 1}, features={"grid": 1})
    for fr in (plain, f, g):
        fr.planes[...] = 0
        fr.counts[...] = n
        C.memset(C.addressof(fr.retire), 0, 64)
        fr.retire.target_se, fr.retire.min_samples, fr.retire.radius = target, 2, 1
    n_plain = 7 * nx * ny
    begin = 0
    for end in (half, ns):
        sg.par_cast(cam, nx, ny, end, out=plain.planes, counts=plain.counts, retire=plain.retire, sample_begin=begin, resume=True,
                    partial=True, squares=True)
        before = g.counts.copy()
        for fr, dn in ((f, None), (g, True)):
            sg.par_cast(cam, nx, ny, end, out=fr, features=True, denoise=dn, sample_begin=begin, resume=True, partial=True, squares=True)
            what = "%s retire + features%s to %d" % (name, " + denoise" if dn else "", end)
            assert (_words(fr)[:n_plain] == plain.buf.view(np.uint32)[:n_plain]).all(), what + ": planes / count plane"
            assert bytes(fr.retire) == bytes(plain.retire), what + ": retire block"
            _check_planes(fr, planes, what)   # every owned pixel, whatever the count plane says
            assert fr.features.traced == (nx * ny if begin == 0 else 0)
            fr.features.compute = 0
        if end == half:
            assert plain.retire.retired > 0, "the case retires nothing"
        _check_guided(pkg, g, plain.planes[0], plain.planes[1], np.minimum(before, end).astype(np.uint32), what)
        begin = end


def test_device_entry_point_matches_host(pkg, gpu):
    nx, ny, ns = 37, 29, 6
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, "book2", nx, ny)
    hip = _hip()
    rs = np.random.RandomState(3)
    n = rs.randint(0, ns + 3, size=(ny, nx)).astype(np.uint32)
    for squares, counts, retire, denoise in ((False, False, False, False), (False, True, False, False), (True, False, False, True),
                                             (True, True, True, True)):
        f = _canary_frame(pkg, nx, ny, squares, counts, retire, {"k": 0.5, "radius": 6, "patch": 3} if denoise else None,
                          {"grid": 2, "sigma_normal": 0.2})
        f.planes[...] = 0
        if counts:
            f.counts[...] = n
        if retire:
            C.memset(C.addressof(f.retire), 0, 64)
            f.retire.target_se, f.retire.min_samples, f.retire.radius = 0.2, 2, 1
        start = f.buf.copy()
        dev = _DeviceBuf(hip, f.buf.nbytes)
        try:
            begin = 0
            for end, partial in ((3, True), (ns, False)):
                sg.par_cast(cam, nx, ny, end, out=f, features=True, denoise=True if denoise else None, sample_begin=begin, resume=True,
                            partial=partial, squares=squares)
                if begin == 0:
                    dev.put(start)
                block = capi.make_features(f.features)
                block.traced = block.missed = 77
                sg.par_cast_device(cam, capi.make_params(nx, ny, end, sample_begin=begin, resume=True, partial=partial, squares=squares,
                                                         counts=counts, retire=retire, denoise=denoise), dev.p.value, None, features=block)
                what = "squares=%s counts=%s retire=%s denoise=%s to %d" % (squares, counts, retire, denoise, end)
                assert (dev.get() == _words(f)).all(), what + ": device frame differs from the host call's"
                assert block.as_dict() == f.features.as_dict() and block.traced == (nx * ny if begin == 0 else 0), what
                f.features.compute = 0
                begin = end
        finally:
            dev.free()


def test_rejections(pkg, gpu):
    nx, ny, ns = 32, 32, 4
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    ref = sg.par_cast(cam, nx, ny, ns)
    hip = _hip()
    bad = [dict(grid=0), dict(grid=5), dict(grid=0xFFFFFFFF), dict(compute=2), dict(reserved_in=1)]
    bad_sigma = [{name: v} for name in ("sigma_normal", "sigma_albedo", "sigma_depth") for v in (float("nan"), float("inf"), 0.0, -1.0)]
    for squares, counts, denoise in ((False, False, False), (False, True, False), (True, False, True), (True, True, True)):
        dev = _DeviceBuf(hip, capi.features_frame_bytes(nx, ny, squares, counts, False, denoise))
        try:
            for fields in bad + (bad_sigma if denoise else []):
                f = _canary_frame(pkg, nx, ny, squares, counts, denoise=True if denoise else None)
                if counts:
                    f.counts[...] = ns + 1
                for name, v in fields.items():
                    setattr(f.features, name, v)
                keep = f.buf.copy()
                with pytest.raises(capi.RtError) as ei:
                    sg.par_cast(cam, nx, ny, ns, out=f, features=True, denoise=True if denoise else None, squares=squares, partial=True)
                assert ei.value.code == capi.ERR_INVALID and "FEATURES" in str(ei.value)
                assert (_words(f) == keep.view(np.uint32)).all(), (counts, denoise, fields)
                dev.put(keep)
                for begin in (0, ns, None):   # with a render in front, the render-less call's own read-back, a call without RESUME
                    with pytest.raises(capi.RtError) as ei:
                        sg.par_cast_device(cam, capi.make_params(nx, ny, ns, squares=squares, counts=counts, denoise=denoise, features=True,
                                                                 partial=True, resume=begin is not None, sample_begin=begin or 0),
                                           dev.p.value)
                    assert ei.value.code == capi.ERR_INVALID
                    assert (dev.get() == keep.view(np.uint32)).all(), (counts, denoise, fields, begin)
            if not denoise:   # without the filter the sigmas are not read
                f = _canary_frame(pkg, nx, ny, squares, counts)
                if counts:
                    f.counts[...] = ns + 1
                f.features.sigma_normal, f.features.sigma_albedo, f.features.sigma_depth = float("nan"), 0.0, -1.0
                sg.par_cast(cam, nx, ny, ns, out=f, features=True, squares=squares)
                assert f.features.traced == nx * ny
        finally:
            dev.free()
    buf = np.full((ny, nx, 3), NAN_BITS, dtype=np.uint32).view(np.float32)
    with pytest.raises(capi.RtError) as ei:
        gpu.par_cast_multi([sg], cam, nx, ny, ns, out=buf, features=True)
    assert ei.value.code == capi.ERR_UNSUPPORTED
    assert (bits(buf) == NAN_BITS).all()
    with pytest.raises(capi.RtError) as ei:
        sg.debug_samples(cam, nx, ny, ns, [1], [1], [0], features=True)
    assert ei.value.code == capi.ERR_INVALID
    assert_bit_equal(sg.par_cast(cam, nx, ny, ns), ref, "the handle after the refusals")


def test_full_size_frame(pkg, gpu):
    """The benchmark's book-1 frame, 1200 x 800 at 8 samples: a 2 x 2 grid of feature rays and the guided filter at (5, 2)."""
    nx, ny, ns = 1200, 800, 8
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    f = _canary_frame(pkg, nx, ny, True, denoise=True, features={"grid": 2})
    _, st = sg.par_cast(cam, nx, ny, ns, out=f, denoise=True, features=True, squares=True, partial=True, stats=True, counters=False)
    print("1200x800x8 with 2 x 2 feature rays and the guided filter at (5, 2): kernel_ms %.3f" % st["kernel_ms"])
    assert (f.features.traced, f.features.missed) == (nx * ny, 0)   # (the sky dome catches every ray)
    assert np.isfinite(f.albedo).all() and np.isfinite(f.normal).all() and (f.depth > 0).all()
    _check_guided(pkg, f, f.planes[0], f.planes[1], np.full((ny, nx), ns, np.uint32), "1200x800x8")
    assert f.denoise.filtered + f.denoise.passed == nx * ny
