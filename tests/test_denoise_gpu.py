"""Denoising on the device (include/rtiow_gpu.h RTG_FLAG_DENOISE): the output plane equals denoise.nlm of the frame's own
undivided running sums bit for bit -- on every scene case, on planted sums (ragged tiles, halos wider than the image, invalid
pixels, every radius / patch), slice by slice, with count planes and the retire step in the same call, from both entry points
and at full size; everything else in the frame ends as without the flag; refused calls write nothing."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal, bits
from scene_cases import CASES, build_case
from test_denoise_abi import random_sums
from test_retire_gpu import _DeviceBuf, _hip

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")
NAN_BITS = 0x7FC0DEAD
RF = [(0, 0), (1, 0), (5, 2), (8, 3), (8, 0), (3, 3)]
KS = [0.3, 0.7, 2.0]


def _words(f):
    return f.buf.view(np.uint32)


def _canary_frame(pkg, nx, ny, counts=False, retire=False, denoise=None):
    """A DenoiseFrame filled with a NaN canary, its block's in-fields set."""
    f = pkg.capi.denoise_frame(nx, ny, counts, retire)
    _words(f)[...] = NAN_BITS
    block = pkg.capi.make_denoise(denoise)
    C.memmove(C.addressof(f.denoise), C.addressof(block), pkg.capi.Denoise.OUT_OFFSET)
    return f


def _check_output(pkg, f, S, Q, e, what):
    """The output plane against denoise.nlm of (S, Q, e); pixels with e = 0 keep the canary; the block's fields."""
    d = f.denoise
    want = pkg.denoise.nlm(S, Q, e, d.radius, d.patch, d.k)
    held = e > 0
    assert_bit_equal(f.denoised[held], want[held], what + ": output plane")
    assert (bits(f.denoised)[~held] == NAN_BITS).all(), what + ": pixels without samples were written"
    valid = pkg.denoise.mean_var(S, Q, e)[2]
    assert d.filtered == int(valid.sum()) and d.filtered + d.passed == int(held.sum()), (what, d.filtered, d.passed)
    assert all(w == 0 for w in d.reserved) and d.reserved_in == 0, what


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_scene_case(pkg, gpu, name):
    sg, cam, nx, ny, ns = build_case(pkg, gpu, name)
    ref, st_ref = sg.par_cast(cam, nx, ny, ns, squares=True, stats=True)
    sums = sg.par_cast(cam, nx, ny, ns, squares=True, partial=True)
    f = _canary_frame(pkg, nx, ny)
    got, st = sg.par_cast(cam, nx, ny, ns, out=f, denoise=True, squares=True, stats=True)
    assert got is f
    assert_bit_equal(f.planes, ref, name + ": planes 0 and 1 with the flag")
    for c in COUNTERS:
        assert st[c] == st_ref[c], (name, c, st[c], st_ref[c])
    _check_output(pkg, f, sums[0], sums[1], np.full((ny, nx), ns, np.uint32), name)
    assert (f.denoise.k, f.denoise.radius, f.denoise.patch) == (np.float32(0.7), 5, 2)
    # a Denoise of the caller's and arrays of the caller's: a new frame carries them
    out = np.zeros((2, ny, nx, 3), np.float32)
    g = sg.par_cast(cam, nx, ny, ns, out=out, denoise={"k": 0.7, "radius": 5, "patch": 2}, squares=True)
    assert_bit_equal(out, ref, name + ": out= array")
    assert_bit_equal(g.denoised, f.denoised, name + ": staged frame")


FRAMES = [(9, 13), (7, 5), (1, 6), (12, 10), (48, 64), (29, 37), (1, 1), (3, 200), (200, 3)]


@pytest.mark.parametrize("shape", FRAMES)
def test_planted_sums(pkg, gpu, shape):
    ny, nx = shape
    ns = 8
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    S, Q, n = random_sums(ny, nx, 7 * ny + nx)
    for counts in (False, True):
        e = np.minimum(n, ns).astype(np.uint32) if counts else np.full((ny, nx), ns, np.uint32)
        for R, F in RF:
            for k in KS:
                what = "%s counts=%s R %d F %d k %g" % (shape, counts, R, F, k)
                f = _canary_frame(pkg, nx, ny, counts, denoise={"k": k, "radius": R, "patch": F})
                f.planes[0], f.planes[1] = S, Q
                if counts:
                    f.counts[...] = n
                before = f.buf.copy()
                off = pkg.capi.denoise_block_offset(nx, ny, counts) // 4
                sg.par_cast(cam, nx, ny, ns, out=f, denoise=True, sample_begin=ns, resume=True, partial=True, squares=True)
                assert (_words(f)[:off + 4] == before.view(np.uint32)[:off + 4]).all(), what + ": planes / counts / in-fields written"
                _check_output(pkg, f, S, Q, e, what)


def _plain_slices(pkg, sg, cam, nx, ny, cuts, n=None):
    """The undivided running sums after every slice of a progressive frame without the flag ([2, ny, nx, 3] each); n: the
    count plane of a counts frame."""
    fr = pkg.capi.counts_frame(nx, ny, squares=True)
    sums, begin = [], 0
    for end in cuts:
        if n is None:
            sg.par_cast(cam, nx, ny, end, out=fr.planes, sample_begin=begin, resume=True, partial=True, squares=True)
        else:
            fr.counts[...] = n
            sg.par_cast(cam, nx, ny, end, out=fr.planes, counts=fr.counts, sample_begin=begin, resume=True, partial=True,
                        squares=True)
        sums.append(fr.planes.copy())
        begin = end
    return sums


@pytest.mark.parametrize("name", ["book1", "book2", "cornell"])
def test_slices(pkg, gpu, name):
    nx, ny, ns, cuts = 48, 32, 9, (2, 5, 9)
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    ref = sg.par_cast(cam, nx, ny, ns, squares=True)
    sums = _plain_slices(pkg, sg, cam, nx, ny, cuts)
    f = _canary_frame(pkg, nx, ny, denoise={"k": 0.7, "radius": 3, "patch": 1})
    begin = 0
    for end, s in zip(cuts, sums):
        sg.par_cast(cam, nx, ny, end, out=f, denoise=True, sample_begin=begin, resume=True, partial=end != ns, squares=True)
        _check_output(pkg, f, s[0], s[1], np.full((ny, nx), end, np.uint32), "%s slice to %d" % (name, end))
        if end != ns:
            assert_bit_equal(f.planes, s, "%s: running sums at %d" % (name, end))
        begin = end
    assert_bit_equal(f.planes, ref, name + ": the last slice divides plane 0")
    # per-pixel counts: 0, 1, 2, ns / 2, ns and beyond
    rs = np.random.RandomState(5)
    n = rs.choice(np.array([0, 1, 2, ns // 2, ns, ns + 3], np.uint32), size=(ny, nx)).astype(np.uint32)
    sums = _plain_slices(pkg, sg, cam, nx, ny, cuts, n=n)
    want = pkg.capi.counts_frame(nx, ny, squares=True)
    want.counts[...] = n
    sg.par_cast(cam, nx, ny, ns, out=want.planes, counts=want.counts, squares=True)
    f = _canary_frame(pkg, nx, ny, counts=True, denoise={"k": 1.0, "radius": 4, "patch": 2})
    f.planes[...] = 0
    f.counts[...] = n
    begin = 0
    for end, s in zip(cuts, sums):
        sg.par_cast(cam, nx, ny, end, out=f, denoise=True, sample_begin=begin, resume=True, partial=end != ns, squares=True)
        _check_output(pkg, f, s[0], s[1], np.minimum(n, end).astype(np.uint32), "%s counts slice to %d" % (name, end))
        assert (f.counts == n).all()
        begin = end
    held = n > 0
    assert_bit_equal(f.planes[:, held], want.planes[:, held], name + ": the last counts slice resolves per pixel")


@pytest.mark.parametrize("name,target", [("book1", 0.15), ("cornell", 2.0)])
def test_retire_in_the_same_call(pkg, gpu, name, target):
    nx, ny, ns, half = 40, 24, 12, 6
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    rs = np.random.RandomState(11)
    n = rs.randint(0, ns + 4, size=(ny, nx)).astype(np.uint32)
    n[rs.rand(ny, nx) < 0.5] = ns + 2
    plain = pkg.capi.counts_frame(nx, ny, squares=True, retire=True)
    f = _canary_frame(pkg, nx, ny, counts=True, retire=True, denoise={"k": 0.7, "radius": 2, "patch": 1})
    f.planes[...] = 0
    for fr in (plain, f):
        fr.counts[...] = n
        fr.retire.target_se, fr.retire.min_samples, fr.retire.radius = target, 2, 1
        fr.retire.active = fr.retire.retired = fr.retire.estimated = fr.retire.reserved = 0
        fr.retire.sum_se2, fr.retire.samples_held = 0.0, 0
        fr.retire.reserved2[0] = fr.retire.reserved2[1] = 0
    n_plain = 7 * nx * ny
    begin = 0
    for end in (half, ns):
        sg.par_cast(cam, nx, ny, end, out=plain.planes, counts=plain.counts, retire=plain.retire, sample_begin=begin, resume=True,
                    partial=True, squares=True)
        before = f.counts.copy()
        sg.par_cast(cam, nx, ny, end, out=f, denoise=True, sample_begin=begin, resume=True, partial=True, squares=True)
        what = "%s retire + denoise to %d" % (name, end)
        assert (_words(f)[:n_plain] == plain.buf.view(np.uint32)[:n_plain]).all(), what + ": planes / count plane"
        assert bytes(f.retire) == bytes(plain.retire), what + ": retire block"
        if end == half:
            assert plain.retire.retired > 0, "the case retires nothing"
        e = np.minimum(before, end).astype(np.uint32)
        assert (e == np.minimum(f.counts, end)).all()
        _check_output(pkg, f, plain.planes[0], plain.planes[1], e, what)
        begin = end


def test_device_entry_point_matches_host(pkg, gpu):
    nx, ny, ns = 37, 29, 6
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    hip = _hip()
    rs = np.random.RandomState(3)
    n = rs.randint(0, ns + 3, size=(ny, nx)).astype(np.uint32)
    for counts, retire in ((False, False), (True, False), (True, True)):
        f = _canary_frame(pkg, nx, ny, counts, retire, denoise={"k": 0.5, "radius": 6, "patch": 3})
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
                sg.par_cast(cam, nx, ny, end, out=f, denoise=True, sample_begin=begin, resume=True, partial=partial, squares=True)
                if begin == 0:
                    dev.put(start)
                block = capi.make_denoise(f.denoise)
                block.filtered = block.passed = 77
                sg.par_cast_device(cam, capi.make_params(nx, ny, end, sample_begin=begin, resume=True, partial=partial,
                                                         squares=True, counts=counts, retire=retire), dev.p.value, None,
                                   denoise=block)
                what = "counts=%s retire=%s to %d" % (counts, retire, end)
                assert (dev.get() == _words(f)).all(), what + ": device frame differs from the host call's"
                assert block.as_dict() == f.denoise.as_dict() and block.filtered > 0, what
                begin = end
        finally:
            dev.free()


def test_progressive_and_adaptive_loops(pkg, gpu):
    nx, ny, ns, step = 48, 32, 12, 4
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    dn = {"k": 0.7, "radius": 3, "patch": 1}
    plain = list(sg.progressive(cam, nx, ny, ns, step))
    plain_sq = list(sg.progressive(cam, nx, ny, ns, step, squares=True))
    assert all(len(t) == 2 for t in plain) and all(len(t) == 3 for t in plain_sq)
    acc = np.zeros((2, ny, nx, 3), np.float32)
    host = []
    for t in sg.progressive(cam, nx, ny, ns, step, out=acc, denoise=dn):
        assert len(t) == 4
        done, pv, se, den = t
        assert_bit_equal(den, pkg.denoise.nlm(acc[0], acc[1], np.full((ny, nx), done, np.uint32), 3, 1, 0.7), "progressive at %d" % done)
        host.append((done, pv.copy(), den.copy()))
    assert [h[0] for h in host] == [4, 8, 12]
    for (done, pv, _), (d0, p0, _) in zip(host, plain_sq):
        assert done == d0
        assert_bit_equal(pv, p0, "preview with denoise= at %d" % done)
    hip = _hip()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    d_acc = _DeviceBuf(hip, capi.denoise_frame_bytes(nx, ny))
    d_pv, d_dn = _DeviceBuf(hip, 3 * nx * ny * 4), _DeviceBuf(hip, 3 * nx * ny * 4)
    d_ad = _DeviceBuf(hip, capi.denoise_frame_bytes(nx, ny, True, True))
    d_apv = _DeviceBuf(hip, 4 * nx * ny * 4)
    try:
        d_acc.put(np.zeros(d_acc.nbytes // 4, np.float32))
        i = 0
        for t in sg.progressive(cam, nx, ny, ns, step, out=d_acc.p.value, preview=d_pv.p.value, stream=stream.value, denoise=dn,
                                denoised=d_dn.p.value):
            assert len(t) == 4 and t[3] == d_dn.p.value
            assert hip.hipStreamSynchronize(stream) == 0
            assert_bit_equal(d_pv.get().view(np.float32).reshape(ny, nx, 3), host[i][1], "device preview %d" % i)
            assert_bit_equal(d_dn.get().view(np.float32).reshape(ny, nx, 3), host[i][2], "device denoised %d" % i)
            i += 1
        assert i == len(host)
        # adaptive: host loop against device loop, and today's tuples without denoise=
        assert all(len(t) == 3 for t in sg.adaptive(cam, nx, ny, ns, step, 0.05, min_samples=4))
        ahost = [(h.copy(), p.copy(), d.copy()) for h, p, _, d in sg.adaptive(cam, nx, ny, ns, step, 0.05, min_samples=4, denoise=dn)]
        assert len(ahost) >= 2
        i = 0
        for t in sg.adaptive(cam, nx, ny, ns, step, 0.05, min_samples=4, out=d_ad.p.value, preview=d_apv.p.value,
                             stream=stream.value, denoise=dn, denoised=d_dn.p.value):
            assert len(t) == 4 and t[3] == d_dn.p.value
            assert_bit_equal(d_apv.get(3 * nx * ny * 4).view(np.float32).reshape(ny, nx, 3), ahost[i][1], "adaptive preview %d" % i)
            assert_bit_equal(d_dn.get().view(np.float32).reshape(ny, nx, 3), ahost[i][2], "adaptive denoised %d" % i)
            i += 1
        assert i == len(ahost)
        n3 = sum(1 for t in sg.adaptive(cam, nx, ny, ns, step, 0.05, min_samples=4, out=d_ad.p.value, preview=d_apv.p.value,
                                        stream=stream.value) if len(t) == 3)
        assert n3 == len(ahost)
    finally:
        for b in (d_acc, d_pv, d_dn, d_ad, d_apv):
            b.free()
        hip.hipStreamDestroy(stream)


def test_rejections(pkg, gpu):
    nx, ny, ns = 32, 32, 4
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    ref = sg.par_cast(cam, nx, ny, ns)
    # the flag without the plane it needs: refused before anything is uploaded
    for flags in (capi.FLAG_DENOISE, capi.FLAG_DENOISE | capi.FLAG_SAMPLE_COUNTS, capi.FLAG_DENOISE | capi.FLAG_PARTIAL):
        f = _canary_frame(pkg, nx, ny, counts=True)
        keep = f.buf.copy()
        p = capi.make_params(nx, ny, ns, flags=flags)
        assert sg.be._par_cast(sg.h, C.byref(cam), C.byref(p), f.buf.ctypes.data_as(capi.c_f32p), None) == capi.ERR_INVALID
        assert (_words(f) == keep.view(np.uint32)).all(), flags
    hip = _hip()
    bad = [dict(radius=9), dict(patch=4), dict(radius=0xFFFFFFFF), dict(k=float("nan")), dict(k=float("inf")), dict(k=0.0),
           dict(k=-1.0), dict(reserved_in=1)]
    for counts in (False, True):
        dev = _DeviceBuf(hip, capi.denoise_frame_bytes(nx, ny, counts))
        try:
            for fields in bad:
                f = _canary_frame(pkg, nx, ny, counts)
                if counts:
                    f.counts[...] = ns + 1
                for name, v in fields.items():
                    setattr(f.denoise, name, v)
                keep = f.buf.copy()
                with pytest.raises(capi.RtError) as ei:
                    sg.par_cast(cam, nx, ny, ns, out=f, denoise=True, squares=True, partial=True)
                assert ei.value.code == capi.ERR_INVALID and "DENOISE" in str(ei.value)
                assert (_words(f) == keep.view(np.uint32)).all(), (counts, fields)
                dev.put(keep)
                for begin in (0, ns, None):   # with a render in front, the render-less call's own read-back, a call without RESUME
                    with pytest.raises(capi.RtError) as ei:
                        sg.par_cast_device(cam, capi.make_params(nx, ny, ns, squares=True, counts=counts, denoise=True, partial=True,
                                                                 resume=begin is not None, sample_begin=begin or 0), dev.p.value)
                    assert ei.value.code == capi.ERR_INVALID
                    assert (dev.get() == keep.view(np.uint32)).all(), (counts, fields, begin)
            # across ranks
            f = _canary_frame(pkg, nx, ny, counts)
            keep = f.buf.copy()
            with pytest.raises(capi.RtError) as ei:
                sg.par_cast(cam, nx, ny, ns, out=f, denoise=True, squares=True, partial=True, tile_w=8, tile_h=8, rank=1, nranks=2)
            assert ei.value.code == capi.ERR_INVALID
            assert (_words(f) == keep.view(np.uint32)).all()
        finally:
            dev.free()
    buf = np.full((ny, nx, 3), NAN_BITS, dtype=np.uint32).view(np.float32)
    with pytest.raises(capi.RtError) as ei:
        gpu.par_cast_multi([sg], cam, nx, ny, ns, out=buf, denoise=True)
    assert ei.value.code == capi.ERR_UNSUPPORTED
    assert (bits(buf) == NAN_BITS).all()
    with pytest.raises(capi.RtError) as ei:
        sg.debug_samples(cam, nx, ny, ns, [1], [1], [0], denoise=True)
    assert ei.value.code == capi.ERR_INVALID
    with pytest.raises(capi.RtError) as ei:
        sg.debug_samples(cam, nx, ny, ns, [1], [1], [0], denoise=True, squares=True)
    assert ei.value.code == capi.ERR_INVALID
    assert_bit_equal(sg.par_cast(cam, nx, ny, ns), ref, "the handle after the refusals")


def test_full_size_frame(pkg, gpu):
    """The benchmark's book-1 frame, 1200 x 800 at 8 samples, default parameters."""
    nx, ny, ns = 1200, 800, 8
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    f = _canary_frame(pkg, nx, ny)
    _, st = sg.par_cast(cam, nx, ny, ns, out=f, denoise=True, squares=True, partial=True, stats=True, counters=False)
    print("1200x800x8 with the filter at (5, 2): kernel_ms %.3f" % st["kernel_ms"])
    _check_output(pkg, f, f.planes[0], f.planes[1], np.full((ny, nx), ns, np.uint32), "1200x800x8")
    assert f.denoise.filtered + f.denoise.passed == nx * ny
