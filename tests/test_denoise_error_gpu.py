"""The error plane of the filtered frame on the device (include/rtiow_gpu.h RTG_FLAG_DENOISE_ERROR): it equals the second result
of denoise.nlm_error / nlm_guided_error bit for bit on planted sums, +inf on pass-through pixels and untouched where a pixel
holds no sample; everything in front of it ends as in the same call without the flag; the retire rule under the flag is
noise.retire_filtered, ties exact, with the same bits from both entry points; the device adaptive loop matches the host loop
slice by slice; several handles give the one-handle frame; refused calls write nothing."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal, bits
from scene_cases import CASES, build_case
from test_denoise_abi import random_sums
from test_features_abi import random_features
from test_retire_gpu import _DeviceBuf, _hip, _planted

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0DEAD
INF_BITS = 0x7F800000
RF = [(0, 0), (1, 0), (5, 2), (8, 3)]
KS = [0.3, 2.0]


def _words(f):
    return f.buf.view(np.uint32)


def _canary(pkg, nx, ny, counts=False, retire=False, denoise=None, features=None, error=True):
    """A frame of the flags' layout, every word a NaN canary, the blocks' in-fields set (retire: a dict of its in-fields)."""
    capi = pkg.capi
    if features is not None:
        f = capi.features_frame(nx, ny, True, counts, retire is not False, denoise, features, error)
    else:
        f = capi.denoise_frame(nx, ny, counts, retire is not False, denoise, error)
    _words(f)[...] = NAN_BITS
    block = capi.make_denoise(denoise)   # (a name keeps the block alive while memmove reads it)
    C.memmove(C.addressof(f.denoise), C.addressof(block), capi.Denoise.OUT_OFFSET)
    if features is not None:
        fblock = capi.make_features(features)
        C.memmove(C.addressof(f.features), C.addressof(fblock), capi.Features.OUT_OFFSET)
    if retire is not False:
        rblock = capi.Retire()
        rblock.target_se, rblock.min_samples, rblock.radius = retire["target_se"], retire["min_samples"], retire["radius"]
        C.memmove(C.addressof(f.retire), C.addressof(rblock), capi.Retire.active.offset)
    return f


def _filter_only(sg, cam, f, nx, ny, ns, **kw):
    """The render-less call: sample_begin == ns, PARTIAL -- the filter (and the retire rule) alone, in place."""
    on = {"features": True} if f.features is not None else {}
    if f.error is not None:
        on["error"] = True
    return sg.par_cast(cam, nx, ny, ns, out=f, denoise=True, squares=True, sample_begin=ns, resume=True, partial=True, **on, **kw)


def _check_error_plane(f, want_ev, e, what):
    held = e > 0
    assert_bit_equal(f.error[held], want_ev[held], what + ": error plane")   # (+inf where a held pixel is not valid)
    assert (bits(f.error)[~held] == NAN_BITS).all(), what + ": pixels without samples were written"


def _check_front(f, g, what):
    """Every word in front of the error plane equals the frame `g` of the same call without the flag; the padding word, if any,
    keeps its canary."""
    w = g.layout.words
    assert f.layout.error in (w, w + 1)
    bad = np.flatnonzero(_words(f)[:w] != _words(g))
    assert bad.size == 0, "%s: %d words in front of the error plane differ, first at %d" % (what, bad.size, bad[0])
    assert (_words(f)[w:f.layout.error] == NAN_BITS).all(), what + ": padding word written"


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (13, 9), (37, 29), (64, 48), (200, 3)])
def test_planted_sums(pkg, gpu, shape):
    ny, nx = shape
    ns = 8
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    S, Q, n = random_sums(ny, nx, 7 * ny + nx)
    for counts in (False, True):
        e = np.minimum(n, ns).astype(np.uint32) if counts else np.full((ny, nx), ns, np.uint32)
        valid = pkg.denoise.mean_var(S, Q, e)[2]
        for R, F in RF:
            for k in KS:
                what = "%s counts=%s R %d F %d k %g" % (shape, counts, R, F, k)
                frames = []
                for error in (True, False):
                    f = _canary(pkg, nx, ny, counts, denoise={"k": k, "radius": R, "patch": F}, error=error)
                    f.planes[0], f.planes[1] = S, Q
                    if counts:
                        f.counts[...] = n
                    _filter_only(sg, cam, f, nx, ny, ns)
                    frames.append(f)
                f, g = frames
                want_out, want_ev = pkg.denoise.nlm_error(S, Q, e, R, F, k)
                _check_error_plane(f, want_ev, e, what)
                assert (bits(f.error)[(e > 0) & ~valid] == INF_BITS).all(), what + ": pass-through pixels"
                assert_bit_equal(f.denoised[e > 0], want_out[e > 0], what + ": output plane")
                _check_front(f, g, what)
                assert f.denoise.filtered == int(valid.sum()) and f.denoise.filtered + f.denoise.passed == int((e > 0).sum()), what


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (13, 9), (37, 29), (64, 48), (200, 3)])
def test_planted_sums_guided(pkg, gpu, shape):
    """test_planted_sums with planted feature planes (compute = 0), sigmas 0.5 / 1.0, through both guided instantiations: the
    neighbours' feature records through the caches (scene option guide_lds = 0) and from LDS (1)."""
    ny, nx = shape
    ns = 8
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    S, Q, n = random_sums(ny, nx, 7 * ny + nx)
    a, nn, z = random_features(ny, nx, 3 * ny + nx)
    differs = False
    for counts in (False, True):
        e = np.minimum(n, ns).astype(np.uint32) if counts else np.full((ny, nx), ns, np.uint32)
        for i, (R, F) in enumerate(RF):
            for k in KS:
                sig = ((0.5, 1.0, 0.5), (1.0, 0.5, 1.0))[(i + int(counts)) % 2]
                feat = {"grid": 1, "compute": 0, "sigma_normal": sig[0], "sigma_albedo": sig[1], "sigma_depth": sig[2]}
                want_out, want_ev = pkg.denoise.nlm_guided_error(S, Q, e, a, nn, z, R, F, k, *sig)
                differs = differs or bool((bits(pkg.denoise.nlm_error(S, Q, e, R, F, k)[1]) != bits(want_ev)).any())
                for guide_lds in (0, 1):
                    sg.set_option("guide_lds", guide_lds)
                    what = "%s guide_lds %d counts=%s R %d F %d k %g" % (shape, guide_lds, counts, R, F, k)
                    frames = []
                    for error in (True, False):
                        f = _canary(pkg, nx, ny, counts, denoise={"k": k, "radius": R, "patch": F}, features=feat, error=error)
                        f.planes[0], f.planes[1] = S, Q
                        f.albedo[...], f.normal[...], f.depth[...] = a, nn, z
                        if counts:
                            f.counts[...] = n
                        _filter_only(sg, cam, f, nx, ny, ns)
                        frames.append(f)
                    f, g = frames
                    _check_error_plane(f, want_ev, e, what)
                    assert_bit_equal(f.denoised[e > 0], want_out[e > 0], what + ": output plane")
                    _check_front(f, g, what)
    sg.set_option("guide_lds", 0)
    assert differs or nx * ny == 1, "%s: the features change nothing" % (shape,)


def test_ties_are_exact(pkg, gpu):
    """R = 0, so ev == v.  e = 2, S = b, Q = b * b with b = 2^-3 give v = 2^-8 exactly: target 2^-4 retires the pixel, the next
    float64 below does not, and b one ulp larger does not."""
    nx, ny, ns = 8, 8, 2
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    b = np.float32(2.0 ** -3)
    b_up = np.nextafter(b, np.float32(1))

    def run(target, odd=None):
        f = _canary(pkg, nx, ny, True, {"target_se": target, "min_samples": 0, "radius": 0}, {"k": 0.7, "radius": 0, "patch": 0})
        f.planes[0], f.planes[1] = b, b * b
        if odd is not None:
            f.planes[0][odd], f.planes[1][odd] = b_up, b_up * b_up
        f.counts[...] = 5
        _filter_only(sg, cam, f, nx, ny, ns)
        return f
    f = run(2.0 ** -4)
    assert (bits(f.error) == bits(np.float32(2.0 ** -8))).all()
    assert (f.counts == ns).all() and f.retire.retired == nx * ny and f.retire.active == 0 and f.retire.estimated == nx * ny
    assert f.retire.sum_se2 == 3 * nx * ny * 2.0 ** -8
    f = run(float(np.nextafter(2.0 ** -4, 0.0)))
    assert (f.counts == 5).all() and f.retire.retired == 0 and f.retire.active == nx * ny
    f = run(2.0 ** -4, odd=(3, 5))
    assert (f.error[3, 5] > np.float32(2.0 ** -8)).all()
    want = np.full((ny, nx), ns, np.uint32)
    want[3, 5] = 5
    assert (f.counts == want).all() and f.retire.retired == nx * ny - 1 and f.retire.active == 1


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("nx,ny", [(37, 29), (24, 16)])
def test_retire_on_planted_sums(pkg, gpu, nx, ny, radius):
    ns = 8
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    hip = _hip()
    lay = capi.FrameLayout(nx, ny, True, True, True, True, False, True)
    dev = _DeviceBuf(hip, 4 * lay.words)
    some = 0
    try:
        for seed, min_samples, target, (R, F) in ((1, 4, 0.05, (2, 1)), (2, 12, 0.05, (2, 1)), (3, 2, 2.0, (0, 0)), (4, 8, 0.02, (3, 0))):
            src = _planted(pkg, nx, ny, ns, seed + 10 * radius)
            f = _canary(pkg, nx, ny, True, {"target_se": target, "min_samples": min_samples, "radius": radius},
                        {"k": 0.7, "radius": R, "patch": F})
            f.planes[...], f.counts[...] = src.planes, src.counts
            # (the lower half without the planted special values, so that whole windows can be OK there)
            low = f.planes[:, ny // 2:]
            low[~np.isfinite(low) | (np.abs(low) > 1e20)] = 1.0
            before = f.buf.copy()
            n = f.counts.copy()
            e = np.minimum(n, ns).astype(np.uint32)
            want_out, ev = pkg.denoise.nlm_error(f.planes[0], f.planes[1], e, R, F, 0.7)
            ret = pkg.noise.retire_filtered(n > ns, ns, ev, n, min_samples, target, radius=radius)
            want = np.where(ret, np.uint32(ns), n)
            est = (n > 0) & np.isfinite(ev).all(axis=-1)
            ev64 = ev.astype(np.float64)
            se2 = float(((ev64[..., 0] + ev64[..., 1]) + ev64[..., 2])[est].sum())
            fields = {"active": int((want > ns).sum()), "retired": int(ret.sum()), "estimated": int(est.sum()), "reserved": 0,
                      "samples_held": int(e.astype(np.uint64).sum())}
            what = "%dx%d radius %d seed %d min_samples %d" % (nx, ny, radius, seed, min_samples)
            _filter_only(sg, cam, f, nx, ny, ns)
            _check_error_plane(f, ev, e, what)
            assert_bit_equal(f.denoised[e > 0], want_out[e > 0], what + ": output plane")
            assert (f.counts == want).all(), (what, np.argwhere(f.counts != want)[:5])
            got = {k: getattr(f.retire, k) for k in fields}
            assert got == fields, (what, got, fields)
            assert pkg.noise.filtered_estimate(ev, n)[0] == fields["estimated"]
            assert abs(f.retire.sum_se2 - se2) <= 1e-12 * abs(se2), (what, f.retire.sum_se2, se2)
            assert (bits(f.planes) == before.view(np.uint32)[:6 * nx * ny].reshape(f.planes.shape)).all(), what + ": planes written"
            if min_samples > ns:
                assert fields["retired"] == 0
            some += fields["retired"]
            # the device entry point: the same words, sum_se2 included
            dev.put(before)
            sg.par_cast_device(cam, capi.make_params(nx, ny, ns, sample_begin=ns, resume=True, partial=True, squares=True, counts=True,
                                                     retire=True, denoise=True, error=True), dev.p.value, None)
            assert (dev.get() == _words(f)).all(), what + ": device frame differs from the host call's"
        assert some > 0, "no planted pixel retired: the targets test nothing"
    finally:
        dev.free()


@pytest.mark.parametrize("name,target,radius", [("book1", 0.08, 1), ("cornell", 0.3, 0)])
def test_adaptive_device_loop_matches_host_loop(pkg, gpu, name, target, radius):
    nx, ny, ns, step = 48, 32, 40, 4
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    dn = {"k": 0.7, "radius": 3, "patch": 1}
    host = capi.denoise_frame(nx, ny, True, error=True)
    hip = _hip()
    lay = capi.FrameLayout(nx, ny, True, True, True, True, False, True)
    n = nx * ny
    d_out, d_pv, d_dn = _DeviceBuf(hip, 4 * lay.words), _DeviceBuf(hip, 16 * n), _DeviceBuf(hip, 12 * n)
    try:
        d_out.put(np.zeros(lay.words, np.float32))
        loop_h = sg.adaptive(cam, nx, ny, ns, step, target, min_samples=8, out=host, radius=radius, denoise=dn, filtered_error=True)
        loop_d = sg.adaptive(cam, nx, ny, ns, step, target, min_samples=8, out=d_out.p.value, preview=d_pv.p.value,
                             denoised=d_dn.p.value, radius=radius, denoise=dn, filtered_error=True)
        slices = 0
        for (held, preview, ev, filtered), (k, _, info, _) in zip(loop_h, loop_d):
            slices += 1
            what = "%s after %d samples" % (name, k)
            w = d_out.get()
            assert (w[:6 * n] == _words(host)[:6 * n]).all(), what + ": running sums"
            assert (w[lay.counts:lay.counts + n].reshape(ny, nx) == host.counts).all(), what + ": count plane"
            assert (np.minimum(host.counts, k) == held).all()
            assert (w[lay.denoised:lay.denoised + 3 * n] == bits(host.denoised).ravel()).all(), what + ": output plane"
            assert (bits(filtered).ravel() == bits(host.denoised).ravel()).all()
            assert (w[lay.error:lay.error + 3 * n] == bits(host.error).ravel()).all(), what + ": error plane"
            assert (bits(ev) == bits(host.error)).all()
            assert (d_pv.get(12 * n) == bits(preview).ravel()).all(), what + ": preview"
            est, se2 = pkg.noise.filtered_estimate(host.error, host.counts)
            assert info["estimated"] == est and abs(info["sum_se2"] - se2) <= 1e-12 * abs(se2), what
            assert info["active"] == int((host.counts > k).sum()), what
        assert slices >= 2 and (host.counts < ns).any(), "no pixel retired before ns: the target tests nothing"
        # planes 0 / 1 of a pixel that holds e samples are those of par_cast(ns = e)
        held = np.minimum(host.counts, ns)
        for e in np.unique(held):
            ref = sg.par_cast(cam, nx, ny, int(e), squares=True)
            at = held == e
            assert_bit_equal(preview[at], ref[0][at], "%s: pixels holding %d samples, plane 0" % (name, e))
            assert_bit_equal(host.planes[1][at], ref[1][at], "%s: pixels holding %d samples, plane 1" % (name, e))
    finally:
        for d in (d_out, d_pv, d_dn):
            d.free()


@pytest.mark.parametrize("force_rccl", [0, 1])
@pytest.mark.parametrize("n_handles", [2, 3])
def test_several_handles_on_one_device(pkg, gpu, n_handles, force_rccl):
    nx, ny = 72, 40
    scenes, cam = [], None
    for i in range(n_handles + 1):   # (the first one makes the one-handle calls)
        b = gpu.builder()
        world, cam, _ = CASES["book1"][0](pkg, b, nx, ny)
        sg = b.scene(world, device=0)
        if i > 0 and force_rccl:
            sg.set_option("force_rccl", 1)
        scenes.append(sg)
    scenes[-1].set_option("multi_planes", 1)
    rs = np.random.RandomState(9)
    counts = rs.choice(np.array([0, 1, 3, 8, 12], np.uint32), size=(ny, nx)).astype(np.uint32)
    parts = dict(counts=True, retire={"target_se": 0.1, "min_samples": 2, "radius": 2}, denoise={"k": 0.7, "radius": 3, "patch": 1},
                 features={"grid": 1})
    f1, fm = _canary(pkg, nx, ny, **parts), _canary(pkg, nx, ny, **parts)
    for f in (f1, fm):
        f.planes[...] = 0
        f.counts[...] = counts
    tiles = {"tile_w": 8, "tile_h": 8}
    for ns, kw in ((4, {"partial": True}), (8, {"sample_begin": 4, "resume": True})):
        scenes[0].par_cast(cam, nx, ny, ns, out=f1, denoise=True, features=True, error=True, squares=True, **tiles, **kw)
        gpu.par_cast_multi(scenes[1:], cam, nx, ny, ns, out=fm, **tiles, **kw)
        bad = np.flatnonzero(_words(fm) != _words(f1))
        assert bad.size == 0, "%d handles, force_rccl %d, ns %d: %d words differ, first at %d" % (n_handles, force_rccl, ns, bad.size, bad[0])
        for f in (f1, fm):
            f.features.compute = 0
    assert f1.retire.retired + f1.retire.active > 0 and np.isfinite(f1.error[counts >= 2]).any()
    assert (bits(f1.error)[counts == 0] == NAN_BITS).all()


def _raw(pkg, sg, cam, p, buf):
    st = pkg.capi.Stats.new()
    return sg.be._par_cast(sg.h, C.byref(cam), C.byref(p), buf.ctypes.data_as(pkg.capi.c_f32p), C.byref(st))


def test_refusals_write_nothing(pkg, gpu):
    nx, ny, ns = 21, 13, 4
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    S, Q, n = random_sums(ny, nx, 3)

    def frame(retire=False, **dn):
        f = _canary(pkg, nx, ny, retire is not False, retire, dict({"k": 0.7, "radius": 2, "patch": 1}, **dn))
        f.planes[0], f.planes[1] = S, Q
        if f.counts is not None:
            f.counts[...] = n + 3
        return f

    hip = _hip()
    dev = _DeviceBuf(hip, 4 * capi.FrameLayout(nx, ny, True, True, True, True, False, True).words)   # (the largest frame below)

    def refused(f, what, **kw):
        """Both entry points; with a render in front (begin 0), the render-less call, and a call without RESUME."""
        before = f.buf.copy()
        on = dict(squares=True, denoise=True, error=True, counts=f.counts is not None, retire=f.retire is not None)
        on.update(kw)
        for begin in (0, ns, None):
            p = capi.make_params(nx, ny, ns, sample_begin=begin or 0, resume=begin is not None, partial=True, **on)
            assert _raw(pkg, sg, cam, p, f.buf) == capi.ERR_INVALID, (what, begin)
            assert (_words(f) == before.view(np.uint32)).all(), "%s, begin %s: the frame was written" % (what, begin)
            dev.put(before)
            assert sg.be._par_cast_device(sg.h, C.byref(cam), C.byref(p), dev.p.value, C.c_void_p(None), None) == capi.ERR_INVALID, (what, begin)
            assert (dev.get(before.nbytes) == before.view(np.uint32)).all(), "%s, begin %s: the device frame was written" % (what, begin)
    try:
        # the flag without RTG_FLAG_DENOISE, and with it but without the plane that flag needs
        refused(frame(), "no DENOISE", denoise=False)
        refused(frame(), "no DENOISE, no SUM_SQUARES", denoise=False, squares=False)
        refused(frame(), "DENOISE without SUM_SQUARES", squares=False)
        refused(frame(retire={"target_se": 0.1, "min_samples": 0, "radius": 0}), "DENOISE, counts, no SUM_SQUARES", squares=False, retire=False)
        # every denoise refusal under the flag, without and with a count plane and the retire block
        ok_retire = {"target_se": 0.1, "min_samples": 0, "radius": 0}
        for retire in (False, ok_retire):
            for dn in ({"radius": 9}, {"patch": 4}, {"radius": 0xFFFFFFFF}, {"k": float("nan")}, {"k": float("inf")}, {"k": 0.0}, {"k": -1.0}):
                refused(frame(retire=retire, **dn), "denoise %s retire %s" % (dn, retire is not False))
            f = frame(retire=retire)
            f.denoise.reserved_in = 1
            refused(f, "reserved_in")
            refused(frame(retire=retire), "nranks 2", nranks=2, rank=1, tile_w=8, tile_h=8)
        # ... and every retire refusal
        for rt in ({"radius": 9}, {"target_se": float("nan")}, {"target_se": -1.0}, {"radius": 0xFFFFFFFF}):
            refused(frame(retire=dict(ok_retire, **rt)), "retire %s" % rt)
        refused(frame(), "RETIRE without SAMPLE_COUNTS", retire=True)
    finally:
        dev.free()
    with pytest.raises(capi.RtError) as ei:
        sg.debug_samples(cam, nx, ny, ns, [0], [0], [0], error=True)
    assert ei.value.code == capi.ERR_INVALID
    with pytest.raises(capi.RtError) as ei:
        sg.debug_samples(cam, nx, ny, ns, [0], [0], [0], squares=True, denoise=True, error=True)
    assert ei.value.code == capi.ERR_INVALID
    # a call without the flag on a buffer sized for it leaves the tail alone
    for retire in (False, {"target_se": 0.1, "min_samples": 0, "radius": 1}):
        f = frame(retire=retire)
        p = capi.make_params(nx, ny, ns, sample_begin=ns, resume=True, partial=True, squares=True, denoise=True,
                             counts=f.counts is not None, retire=f.retire is not None)
        assert _raw(pkg, sg, cam, p, f.buf) == 0
        tail = f.layout.denoised + 3 * nx * ny
        assert (_words(f)[tail:] == NAN_BITS).all(), "the tail behind the output plane was written"
        assert not (bits(f.denoised) == NAN_BITS).all()
