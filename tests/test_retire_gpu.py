"""Adaptive sampling's retire rule on the device (include/rtiow_gpu.h RTG_FLAG_RETIRE): planted running sums retire exactly the
pixels noise.retire names (radius 0 .. 8, ties included), with exact block fields and the same bits from both entry points; the
render part of a RETIRE call is bit for bit the call without the flag on every kernel; the device adaptive loop matches the host
loop slice by slice; sharded frames decide per rank; refused calls write nothing."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal, bits
from fuzz_scenes import random_camera, random_world
from scene_cases import build_case
from test_counts_gpu import FORCED

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0DEAD


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    return hip


class _DeviceBuf:
    """hipMalloc'ed bytes with host copies in and out (the tests' device frames)."""
    def __init__(self, hip, nbytes):
        self.hip, self.nbytes, self.p = hip, nbytes, C.c_void_p()
        assert hip.hipMalloc(C.byref(self.p), nbytes) == 0

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes and self.hip.hipMemcpy(self.p, a.ctypes.data, a.nbytes, 1) == 0

    def get(self, nbytes=None, offset=0):
        out = np.empty((nbytes or self.nbytes) // 4, np.uint32)
        assert self.hip.hipMemcpy(out.ctypes.data, self.p.value + offset, out.nbytes, 2) == 0
        return out

    def free(self):
        self.hip.hipFree(self.p)


def _rule(pkg, f, ns, target, min_samples, radius, owned=None):
    """The numpy restatement: (expected count plane, expected block fields) for the frame `f` before a RETIRE call at k = ns."""
    noise = pkg.noise
    n = f.counts.copy()
    e = np.minimum(n, ns)
    with np.errstate(all="ignore"):
        se = noise.standard_error_counts(f.planes[0], f.planes[1], e)
        ret = noise.retire(n > ns, ns, se, min_samples, target, radius=radius, present=n > 0)
    own = np.ones(n.shape, bool) if owned is None else owned
    ret &= own
    want = np.where(ret, np.uint32(ns), n)
    est = own & (e >= 2) & np.isfinite(se).all(axis=-1)
    se2 = (se[..., 0] * se[..., 0] + se[..., 1] * se[..., 1]) + se[..., 2] * se[..., 2]
    fields = {"active": int((own & (want > ns)).sum()), "retired": int(ret.sum()), "estimated": int(est.sum()), "reserved": 0,
              "samples_held": int(e[own].astype(np.uint64).sum())}
    return want, fields, float(se2[est].sum()), se


def _planted(pkg, nx, ny, ns, seed):
    """A retire frame with random running sums around a few noise levels, special values sprinkled in, counts 0 .. ns + 3."""
    rs = np.random.RandomState(seed)
    f = pkg.capi.counts_frame(nx, ny, squares=True, retire=True)
    n = rs.randint(0, ns + 4, size=(ny, nx)).astype(np.uint32)
    n[rs.rand(ny, nx) < 0.4] = ns + 3   # plenty of candidates
    n[0, 0], n[0, 1], n[0, 2], n[-1, -1] = 0, 1, 2, ns + 1
    e = np.maximum(np.minimum(n, ns), 1).astype(np.float64)[..., None]
    mean = rs.gamma(1.0, 0.5, size=(ny, nx, 3))
    sigma = rs.choice([0.005, 0.05, 0.2, 1.0], size=(ny, nx, 1)) * rs.uniform(0.5, 1.5, size=(ny, nx, 3))
    f.planes[0] = (mean * e).astype(np.float32)
    f.planes[1] = ((mean * mean + sigma * sigma) * e).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30], np.float32)
    for plane in (0, 1):
        m = rs.rand(ny, nx, 3) < 0.03
        f.planes[plane][m] = rs.choice(special, size=int(m.sum()))
    f.counts[...] = n
    return f


def _block(f):
    return {k: getattr(f.retire, k) for k in ("active", "retired", "estimated", "reserved", "samples_held")}


def _retire_call(sg, cam, f, nx, ny, ns, target, min_samples, radius, **kw):
    f.retire.target_se, f.retire.min_samples, f.retire.radius = target, min_samples, radius
    sg.par_cast(cam, nx, ny, ns, out=f.planes, counts=f.counts, retire=f.retire, sample_begin=ns, resume=True, partial=True,
                squares=True, **kw)


@pytest.mark.parametrize("radius", [0, 1, 2, 8])
def test_planted_sums(pkg, gpu, radius):
    nx, ny, ns = 37, 29, 8   # nx * ny odd: the block sits behind a padding word
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    hip = _hip()
    dev = _DeviceBuf(hip, pkg.capi.retire_frame_bytes(nx, ny))
    try:
        for seed, min_samples, target in ((1, 4, 0.05), (2, 12, 0.05), (3, 2, 0.2), (4, 8, 0.01)):
            f = _planted(pkg, nx, ny, ns, seed + 10 * radius)
            before = f.buf.copy()
            want, fields, se2, _ = _rule(pkg, f, ns, target, min_samples, radius)
            _retire_call(sg, cam, f, nx, ny, ns, target, min_samples, radius)
            what = "radius %d seed %d min_samples %d" % (radius, seed, min_samples)
            assert (f.counts == want).all(), (what, np.argwhere(f.counts != want)[:5])
            assert (bits(f.planes) == bits(before[:6 * nx * ny].reshape(f.planes.shape))).all(), what + ": planes written"
            assert _block(f) == fields, (what, _block(f), fields)
            assert abs(f.retire.sum_se2 - se2) <= 1e-12 * abs(se2), (what, f.retire.sum_se2, se2)
            if min_samples > ns:
                assert fields["retired"] == 0
            # the device entry point: the same count plane and block bits, on the caller's stream
            dev.put(before)
            r = pkg.capi.Retire()
            r.target_se, r.min_samples, r.radius = target, min_samples, radius
            sg.par_cast_device(cam, pkg.capi.make_params(nx, ny, ns, sample_begin=ns, resume=True, partial=True, squares=True,
                                                         counts=True), dev.p.value, None, retire=r)
            got = dev.get()
            assert (got == f.buf.view(np.uint32)).all(), what + ": device frame differs from the host call's"
    finally:
        dev.free()


def test_ties_retire(pkg, gpu):
    """target_se equal to a pixel's largest standard error (numpy's float64 bits): that pixel is OK and retires."""
    nx, ny, ns = 24, 16, 8
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    f = _planted(pkg, nx, ny, ns, 77)
    base = f.buf.copy()
    n = f.counts.copy()
    _, _, _, se = _rule(pkg, f, ns, 0.0, 0, 0)
    worst = se.max(axis=-1)
    cand = np.argwhere((n > ns) & np.isfinite(worst) & (worst > 0))
    assert len(cand) >= 32
    for y, x in cand[:48]:
        f.buf[...] = base
        t = float(worst[y, x])
        want, fields, _, _ = _rule(pkg, f, ns, t, 0, 0)
        _retire_call(sg, cam, f, nx, ny, ns, t, 0, 0)
        assert f.counts[y, x] == ns, ("tie at", y, x, repr(t))
        assert (f.counts == want).all() and _block(f) == fields
        # one ulp below: the pixel stays
        f.buf[...] = base
        _retire_call(sg, cam, f, nx, ny, ns, float(np.nextafter(t, 0.0)), 0, 0)
        assert f.counts[y, x] == n[y, x]


def _random_counts(nx, ny, ns, seed):
    rs = np.random.RandomState(seed)
    n = rs.randint(0, ns + 4, size=(ny, nx)).astype(np.uint32)
    n[rs.rand(ny, nx) < 0.5] = ns + 2
    return n


def _render_unchanged(pkg, sg, cam, nx, ny, ns, what):
    """A RETIRE call's planes equal the flagless counts call's, bit for bit -- one PARTIAL slice, then the resolving slice --
    and its count plane follows the rule on the sums it rendered."""
    n = _random_counts(nx, ny, ns, 6)
    half = ns // 2
    plain = pkg.capi.counts_frame(nx, ny, squares=True)
    plain.counts[...] = n
    f = pkg.capi.counts_frame(nx, ny, squares=True, retire=True)
    f.counts[...] = n
    f.retire.target_se, f.retire.min_samples, f.retire.radius = 0.08, 2, 1
    sg.par_cast(cam, nx, ny, half, out=plain.planes, counts=plain.counts, partial=True, squares=True)
    sg.par_cast(cam, nx, ny, half, out=f.planes, counts=f.counts, partial=True, squares=True, retire=f.retire)
    assert_bit_equal(f.planes, plain.planes, what + ": PARTIAL slice")
    probe = pkg.capi.counts_frame(nx, ny, squares=True)
    probe.planes[...] = plain.planes
    probe.counts[...] = n
    want, fields, _, _ = _rule(pkg, probe, half, 0.08, 2, 1)
    assert (f.counts == want).all() and _block(f) == fields, what
    # the second slice: the retired pixels are held at `half` on both sides; the resolve divides by the same e_p
    plain.counts[...] = f.counts
    sg.par_cast(cam, nx, ny, ns, out=plain.planes, counts=plain.counts, sample_begin=half, resume=True, squares=True)
    sg.par_cast(cam, nx, ny, ns, out=f.planes, counts=f.counts, sample_begin=half, resume=True, squares=True, retire=f.retire)
    assert_bit_equal(f.planes, plain.planes, what + ": resolving slice")


@pytest.mark.parametrize("name,options,verbose_tag", FORCED)
def test_render_part_unchanged(pkg, gpu, name, options, verbose_tag):
    nx, ny, ns = 64, 48, 8
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    for o, v in options.items():
        sg.set_option(o, v)
    _render_unchanged(pkg, sg, cam, nx, ny, ns, "%s %s" % (name, options))


def test_render_part_unchanged_deep_graph(pkg, gpu):
    nx, ny, ns = 40, 24, 6
    for seed in range(9000, 9064):
        rs = np.random.RandomState(seed)
        bg = gpu.builder()
        wg = random_world(pkg, bg, rs, general_boundaries=True, deep_shapes=True)
        if bg.flatten(wg)[1] & 128:
            break
    else:
        pytest.fail("no FEAT_DEEP graph among the fuzz seeds")
    cam = random_camera(pkg, gpu, rs, nx, ny)
    _render_unchanged(pkg, bg.scene(wg), cam, nx, ny, ns, "deep %d" % seed)


@pytest.mark.parametrize("name,target", [("book1", 0.04), ("book2", 0.06), ("cornell", 0.06)])
@pytest.mark.parametrize("radius", [0, 1])
def test_device_loop_matches_host_loop(pkg, gpu, name, target, radius):
    nx, ny, ns, step, mins = 48, 32, 40, 4, 8
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    host = []
    hf = pkg.capi.counts_frame(nx, ny, squares=True)
    for held, preview, _ in sg.adaptive(cam, nx, ny, ns, step, target, min_samples=mins, radius=radius, out=hf):
        host.append((held.copy(), preview.copy(), int((hf.counts > len(host) * step + step).sum())))
    hip = _hip()
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    out = _DeviceBuf(hip, pkg.capi.retire_frame_bytes(nx, ny))
    pv = _DeviceBuf(hip, 4 * nx * ny * 4)
    try:
        dev = []
        stats = []
        for k, p, info in sg.adaptive(cam, nx, ny, ns, step, target, min_samples=mins, radius=radius, out=out.p.value,
                                      preview=pv.p.value, stream=stream.value, stats=stats):
            assert p == pv.p.value
            counts = out.get(nx * ny * 4, 6 * nx * ny * 4).reshape(ny, nx)
            dev.append((k, np.minimum(counts, k), pv.get(3 * nx * ny * 4).view(np.float32).reshape(ny, nx, 3), info))
        assert len(dev) == len(host), (name, radius, len(dev), len(host))
        retired = 0
        for i, ((held, preview, active), (k, dheld, dpreview, info)) in enumerate(zip(host, dev)):
            assert k == min(ns, (i + 1) * step)
            assert (dheld == held).all(), (name, radius, k, np.argwhere(dheld != held)[:5])
            assert_bit_equal(dpreview, preview, "%s radius %d: preview at %d" % (name, radius, k))
            assert info["active"] == active, (name, radius, k, info["active"], active)
            assert info["samples_held"] == int(held.astype(np.uint64).sum())
            retired += info["retired"]
            assert np.isfinite(info["est_rmse"]) and info["estimated"] > 0
        assert retired == int((host[-1][0] < ns).sum())
        assert len(stats) == len(dev) and sum(s["samples"] for s in stats) == int(host[-1][0].astype(np.uint64).sum())
    finally:
        out.free(), pv.free(), hip.hipStreamDestroy(stream)


def test_sharded_frames(pkg, gpu):
    nx, ny, ns = 72, 40, 8   # ragged: tiles past the edge
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    tile = (np.arange(ny) // 8)[:, None] * ((nx + 7) // 8) + (np.arange(nx) // 8)[None, :]
    whole = _planted(pkg, nx, ny, ns, 21)
    base = whole.buf.copy()
    _retire_call(sg, cam, whole, nx, ny, ns, 0.05, 4, 0)
    canvas = _planted(pkg, nx, ny, ns, 21)
    total = dict.fromkeys(_block(whole), 0)
    for r in range(3):
        own = tile % 3 == r
        want, fields, se2, _ = _rule(pkg, canvas, ns, 0.05, 4, 0, owned=own)
        before = canvas.counts.copy()
        _retire_call(sg, cam, canvas, nx, ny, ns, 0.05, 4, 0, tile_w=8, tile_h=8, rank=r, nranks=3)
        assert (canvas.counts == want).all() and (canvas.counts[~own] == before[~own]).all(), r
        assert _block(canvas) == fields, (r, _block(canvas), fields)
        assert abs(canvas.retire.sum_se2 - se2) <= 1e-12 * abs(se2)
        for k, v in _block(canvas).items():
            total[k] += v
    assert (canvas.counts == whole.counts).all()
    assert (bits(canvas.planes) == bits(base[:6 * nx * ny].reshape(canvas.planes.shape))).all()
    assert total == _block(whole)
    # radius 1 across ranks: refused, the NaN canvas untouched
    nan = pkg.capi.counts_frame(nx, ny, squares=True, retire=True)
    nan.buf.view(np.uint32)[...] = NAN_BITS
    nan.counts[...] = ns + 1
    nan.retire.target_se, nan.retire.min_samples, nan.retire.radius = 1.0, 0, 1
    keep = nan.buf.copy()
    with pytest.raises(pkg.capi.RtError) as ei:
        sg.par_cast(cam, nx, ny, ns, out=nan.planes, counts=nan.counts, retire=nan.retire, squares=True, partial=True,
                    tile_w=8, tile_h=8, rank=1, nranks=3)
    assert ei.value.code == pkg.capi.ERR_INVALID
    assert (nan.buf.view(np.uint32) == keep.view(np.uint32)).all()


def test_rank_without_tiles_writes_zeros(pkg, gpu):
    nx, ny, ns = 16, 16, 4   # one 16x16 tile: rank 1 of 2 owns nothing
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    f = _planted(pkg, nx, ny, ns, 5)
    f.retire.active = f.retire.retired = f.retire.estimated = f.retire.reserved = 7
    f.retire.sum_se2, f.retire.samples_held = 1.5, 9
    counts = f.counts.copy()
    _retire_call(sg, cam, f, nx, ny, ns, 1.0, 0, 0, rank=1, nranks=2)
    assert _block(f) == dict.fromkeys(_block(f), 0) and f.retire.sum_se2 == 0.0
    assert (f.counts == counts).all()


def test_rejections(pkg, gpu):
    nx, ny, ns = 32, 32, 4
    capi = pkg.capi
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    ref = sg.par_cast(cam, nx, ny, ns)
    nbytes = capi.retire_frame_bytes(nx, ny)

    def nan_frame():
        f = capi.counts_frame(nx, ny, squares=True, retire=True)
        f.buf.view(np.uint32)[...] = NAN_BITS
        f.counts[...] = ns + 1
        return f
    # the flag without the planes it needs: refused before anything is uploaded
    for flags in (capi.FLAG_RETIRE | capi.FLAG_SAMPLE_COUNTS, capi.FLAG_RETIRE | capi.FLAG_SUM_SQUARES, capi.FLAG_RETIRE):
        f = nan_frame()
        keep = f.buf.copy()
        p = capi.make_params(nx, ny, ns, flags=flags | capi.FLAG_PARTIAL)
        assert sg.be._par_cast(sg.h, C.byref(cam), C.byref(p), f.buf.ctypes.data_as(capi.c_f32p), None) == capi.ERR_INVALID
        assert (f.buf.view(np.uint32) == keep.view(np.uint32)).all(), flags
    # bad in-fields, through both entry points
    hip = _hip()
    dev = _DeviceBuf(hip, nbytes)
    try:
        for target, radius in ((0.1, 9), (float("nan"), 0), (-1.0, 0), (0.1, 0xFFFFFFFF)):
            f = nan_frame()
            f.retire.target_se, f.retire.min_samples, f.retire.radius = target, 0, radius
            keep = f.buf.copy()
            with pytest.raises(capi.RtError) as ei:
                sg.par_cast(cam, nx, ny, ns, out=f.planes, counts=f.counts, retire=f.retire, squares=True, partial=True)
            assert ei.value.code == capi.ERR_INVALID and "RETIRE" in str(ei.value)
            assert (f.buf.view(np.uint32) == keep.view(np.uint32)).all(), (target, radius)
            dev.put(keep)
            for begin in (0, ns):   # with the compaction's read-back, and the render-less call's own
                with pytest.raises(capi.RtError) as ei:
                    sg.par_cast_device(cam, capi.make_params(nx, ny, ns, squares=True, counts=True, retire=True, partial=True,
                                                             resume=True, sample_begin=begin), dev.p.value)
                assert ei.value.code == capi.ERR_INVALID
                assert (dev.get() == keep.view(np.uint32)).all(), (target, radius, begin)
    finally:
        dev.free()
    buf = np.full((ny, nx, 3), NAN_BITS, dtype=np.uint32).view(np.float32)
    with pytest.raises(capi.RtError) as ei:
        gpu.par_cast_multi([sg], cam, nx, ny, ns, out=buf, retire=True)
    assert ei.value.code == capi.ERR_UNSUPPORTED
    assert (bits(buf) == NAN_BITS).all()
    with pytest.raises(capi.RtError) as ei:
        sg.debug_samples(cam, nx, ny, ns, [1], [1], [0], retire=True)
    assert ei.value.code == capi.ERR_INVALID
    assert_bit_equal(sg.par_cast(cam, nx, ny, ns), ref, "the handle after the refusals")
