"""Per-pixel noise estimates (include/rtiow_gpu.h RTG_FLAG_SUM_SQUARES): plane 0 is bit for bit the call without the flag, and
plane 1 is the f32 left fold of c * c over the samples -- checked against the oracle's per-sample colours, on every scene case
and every kernel, in slices, on tiles, through the device entry point -- and the progressive stop rule built on it."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal, bits
from scene_cases import CASES, build_case

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")
NAN_BITS = 0x7FC0DEAD


def _oracle_squares(so, cam, nx, ny, ns, **kw):
    """Plane 1 as numpy computes it from the oracle's colour of every sample of every pixel: q = q + c * c in float32, in
    sample order, from +0."""
    rows, xs = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    n = nx * ny
    rgb, _ = so.debug_samples(cam, nx, ny, ns, np.tile(xs.ravel(), ns), np.tile((ny - 1 - rows).ravel(), ns),
                              np.repeat(np.arange(ns), n), **kw)
    c = rgb.reshape(ns, ny, nx, 3)
    q = np.zeros((ny, nx, 3), dtype=np.float32)
    for s in range(ns):
        q = q + c[s] * c[s]
    return q


def _sliced_squares(scene, cam, nx, ny, ns, cuts, out=None, stats=False, **kw):
    """Samples [0, ns) in slices ending at `cuts`, with the flag, into the two-plane running sums `out`; returns (final planes,
    counters summed over the slices).  Every preview resolve must leave plane 1 alone."""
    acc = np.zeros((2, ny, nx, 3), dtype=np.float32) if out is None else out
    total = {}
    begin = 0
    for end in list(cuts) + [ns]:
        last = end == ns
        r = scene.par_cast(cam, nx, ny, end, out=acc, sample_begin=begin, resume=True, partial=not last, squares=True,
                           stats=stats, **kw)
        if stats:
            for k in COUNTERS:
                total[k] = total.get(k, 0) + r[1][k]
        if not last:
            frame = acc.copy()   # the resolve call with the flag: divides plane 0, leaves plane 1 bit for bit
            scene.par_cast(cam, nx, ny, end, out=frame, sample_begin=end, resume=True, squares=True, **kw)
            assert (bits(frame[1]) == bits(acc[1])).all(), "the resolve call changed plane 1"
            plain = acc[0].copy()
            scene.par_cast(cam, nx, ny, end, out=plain, sample_begin=end, resume=True, **kw)
            assert_bit_equal(frame[0], plain, "resolve at %d vs the flagless resolve" % end)
        begin = end
    return acc, total


def _check(sg, cam_g, so, cam_o, nx, ny, ns, what, **kw):
    """One flagged call and three flagged slices against the flagless call, the oracle and the oracle's squares; the counters
    of the flagged call (and of the slices, summed) against the flagless call's."""
    plain, st_plain = sg.par_cast(cam_g, nx, ny, ns, stats=True, **kw)
    ref = so.par_cast(cam_o, nx, ny, ns, **kw)
    q_ref = _oracle_squares(so, cam_o, nx, ny, ns, **kw)
    assert_bit_equal(plain, ref, what + ": flagless GPU vs oracle")
    for stats in (False, True):
        tag = "%s (%s)" % (what, "instrumented" if stats else "timed")
        r = sg.par_cast(cam_g, nx, ny, ns, squares=True, stats=stats, **kw)
        planes = r[0] if stats else r
        assert planes.shape == (2, ny, nx, 3)
        assert_bit_equal(planes[0], plain, tag + ": plane 0 vs the flagless call")
        assert_bit_equal(planes[1], q_ref, tag + ": plane 1 vs the oracle's squares")
        if stats:
            for c in COUNTERS:
                assert r[1][c] == st_plain[c], (tag, c, r[1][c], st_plain[c])
        k = max(2, ns // 2)
        sliced, total = _sliced_squares(sg, cam_g, nx, ny, ns, [1, k], stats=stats, **kw)
        assert_bit_equal(sliced, planes, tag + ": 3 flagged slices vs one flagged call")
        if stats:
            for c in COUNTERS:
                assert total[c] == st_plain[c], (tag, "slices", c, total[c], st_plain[c])
    return planes


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(pkg, gpu, oracle, name):
    sg, cam_g, nx, ny, ns = build_case(pkg, gpu, name)
    so, cam_o, _, _, _ = build_case(pkg, oracle, name)
    _check(sg, cam_g, so, cam_o, nx, ny, ns, name)


@pytest.mark.parametrize("name,options,verbose_tag", [
    ("book2", {"pool2": 2, "sync": 0}, "full pool 2 (second program): samples [0, 8) of 8"),
    ("book2", {"pool2": 0, "sync": 0}, "full pool: samples [0, 8) of 8"),
    ("cornell", {"sync": 1}, None),                        # the lock-step kernel
    ("book1", {"chunks": 1}, "8 chunk(s) of 1 samples"),   # the in-slot fold mode is overridden: scratch and fold
    ("book1", {"chunks": 2}, "8 chunk(s) of 1 samples"),   # so are chunks of several samples
    ("book1", {}, "pool: samples [0, 8) of 8"),            # the lean pool kernel
    ("book1", {"bvh4": 1}, None),
    ("book1", {"kernel": 1}, None),                        # the baseline kernel
    ("cornell", {"kernel": 1}, None),
])
def test_each_kernel_forced(pkg, gpu, oracle, name, options, verbose_tag, capfd):
    nx, ny, ns = 64, 48, 8
    sg, cam_g, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    so, cam_o, _, _, _ = build_case(pkg, oracle, name, nx, ny)
    for o, v in options.items():
        sg.set_option(o, v)
    if verbose_tag:
        sg.set_option("verbose", 1)
        capfd.readouterr()
        sg.par_cast(cam_g, nx, ny, ns, squares=True)
        err = capfd.readouterr().err
        assert verbose_tag in err, (verbose_tag, err[-800:])
        sg.set_option("verbose", 0)
    _check(sg, cam_g, so, cam_o, nx, ny, ns, "%s %s" % (name, options))


@pytest.mark.parametrize("name,nx,ny,ns", [("book1", 128, 96, 20), ("book2", 128, 128, 12)])
def test_sample_passes(pkg, gpu, oracle, name, nx, ny, ns, capfd):
    """A scratch budget smaller than the frame's sample colours: several fold passes carry both planes."""
    sg, cam_g, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    one_pass = sg.par_cast(cam_g, nx, ny, ns, squares=True)
    sg.set_option("scratch_mb", 1)
    sg.set_option("verbose", 1)
    capfd.readouterr()
    planes = sg.par_cast(cam_g, nx, ny, ns, squares=True)
    err = capfd.readouterr().err
    assert err.count(") of %d:" % ns) >= 2, err[-800:]
    sg.set_option("verbose", 0)
    assert_bit_equal(planes, one_pass, name + ": several passes vs one pass")
    sliced, _ = _sliced_squares(sg, cam_g, nx, ny, ns, [1, 4])
    assert_bit_equal(sliced, one_pass, name + ": slices in passes vs one pass")
    so, cam_o, _, _, _ = build_case(pkg, oracle, name, nx, ny)
    assert_bit_equal(planes[0], so.par_cast(cam_o, nx, ny, ns), name + ": plane 0 vs oracle")


@pytest.mark.parametrize("name,options", [("book1", {}), ("book2", {}), ("book2", {"pool2": 2}), ("cornell", {}),
                                          ("book1", {"kernel": 1})])
def test_tiles_leave_other_pixels_alone(pkg, gpu, name, options):
    nx, ny, ns = 72, 40, 7   # ragged: tiles past the edge
    sg, cam_g, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    for o, v in options.items():
        sg.set_option(o, v)
    ref = sg.par_cast(cam_g, nx, ny, ns, squares=True)
    tx, ty = np.arange(nx) // 8, np.arange(ny) // 8
    tile = ty[:, None] * ((nx + 7) // 8) + tx[None, :]
    for sliced in (False, True):
        canvas = np.full((2, ny, nx, 3), NAN_BITS, dtype=np.uint32).view(np.float32)
        owned = np.zeros((ny, nx), dtype=bool)
        for r in range(3):
            kw = dict(tile_w=8, tile_h=8, rank=r, nranks=3)
            if sliced:
                _sliced_squares(sg, cam_g, nx, ny, ns, [1, 3], out=canvas, **kw)
            else:
                sg.par_cast(cam_g, nx, ny, ns, out=canvas, squares=True, **kw)
            owned |= tile % 3 == r
            for plane in (0, 1):
                assert (bits(canvas[plane])[~owned] == NAN_BITS).all(), (name, r, plane)   # bitwise untouched
                assert_bit_equal(canvas[plane][owned], ref[plane][owned], "%s rank %d plane %d" % (name, r, plane))
        assert_bit_equal(canvas, ref, "%s 3 ranks (sliced: %s)" % (name, sliced))


def _hip():
    """Device buffers and streams straight from the HIP runtime the library itself uses (as test_progressive_gpu does)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    return hip


class _Tensor:
    """A device buffer behind the duck types Scene.progressive takes for torch objects: data_ptr() ..."""
    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


class _Stream:
    """... and .cuda_stream"""
    def __init__(self, handle):
        self.cuda_stream = handle


def _download(hip, d, shape):
    h = np.empty(shape, dtype=np.float32)
    assert hip.hipMemcpy(h.ctypes.data, d, h.nbytes, 2) == 0   # device to host
    return h


def test_device_entry_point(pkg, gpu):
    """rtg_par_cast_device with the flag into a device buffer on a stream of its own -- whole frames, slices and the device
    progressive loop -- against the host call."""
    hip = _hip()
    for name, nx, ny, ns in (("book1", 96, 64, 10), ("book2", 64, 64, 10), ("cornell", 48, 32, 10)):
        sg, cam_g, _, _, _ = build_case(pkg, gpu, name, nx, ny)
        ref = sg.par_cast(cam_g, nx, ny, ns, squares=True)
        stream = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(stream)) == 0
        nbytes = 2 * nx * ny * 3 * 4
        buf, acc, prev = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(buf), nbytes) == 0 and hip.hipMalloc(C.byref(acc), nbytes) == 0
        assert hip.hipMalloc(C.byref(prev), nbytes // 2) == 0
        try:
            assert hip.hipMemset(buf, 0xFF, nbytes) == 0   # NaN everywhere: the call must write both planes
            sg.par_cast_device(cam_g, pkg.capi.make_params(nx, ny, ns), buf.value, stream.value, squares=True)
            assert hip.hipStreamSynchronize(stream) == 0
            assert_bit_equal(_download(hip, buf, (2, ny, nx, 3)), ref, name + " device call")
            assert hip.hipMemset(buf, 0xFF, nbytes) == 0
            for b, e in ((0, 1), (1, 6), (6, ns)):
                p = pkg.capi.make_params(nx, ny, e, sample_begin=b, resume=True, partial=e != ns, squares=True)
                sg.par_cast_device(cam_g, p, buf.value, stream.value)
            assert hip.hipStreamSynchronize(stream) == 0
            assert_bit_equal(_download(hip, buf, (2, ny, nx, 3)), ref, name + " device slices")
            # the device progressive loop: the third item is the two-plane running sum itself
            assert hip.hipMemset(acc, 0, nbytes) == 0
            out, preview, st = _Tensor(acc.value), _Tensor(prev.value), _Stream(stream.value)
            got = []
            for n, p, sums in sg.progressive(cam_g, nx, ny, ns, 4, out=out, preview=preview, stream=st, squares=True):
                assert p is preview and sums is out
                assert hip.hipStreamSynchronize(stream) == 0
                got.append((n, _download(hip, prev, (ny, nx, 3)), _download(hip, acc, (2, ny, nx, 3))))
            assert [n for n, _, _ in got] == [4, 8, 10]
            for n, img, planes in got:
                assert_bit_equal(img, sg.par_cast(cam_g, nx, ny, n), "%s device preview at %d" % (name, n))
                assert_bit_equal(planes, sg.par_cast(cam_g, nx, ny, n, squares=True, partial=True), "%s device sums at %d" % (name, n))
            with pytest.raises(ValueError):
                next(sg.progressive(cam_g, nx, ny, ns, 4, out=out, preview=preview, stream=st, target_rmse=0.1))
        finally:
            hip.hipFree(buf), hip.hipFree(acc), hip.hipFree(prev), hip.hipStreamDestroy(stream)


def test_rejections(pkg, gpu):
    nx, ny, ns = 32, 32, 4
    sg, cam_g, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    buf = np.full((2, ny, nx, 3), NAN_BITS, dtype=np.uint32).view(np.float32)
    for kw in ({}, {"partial": True}, {"resume": True, "sample_begin": 2}):
        with pytest.raises(pkg.RtError) as ei:
            gpu.par_cast_multi([sg], cam_g, nx, ny, ns, out=buf, squares=True, **kw)
        assert ei.value.code == pkg.capi.ERR_UNSUPPORTED, kw
    assert (bits(buf) == NAN_BITS).all()
    with pytest.raises(pkg.RtError) as ei:
        sg.debug_samples(cam_g, nx, ny, ns, [1], [1], [0], squares=True)
    assert ei.value.code == pkg.capi.ERR_INVALID
    # the handle still renders, with and without the flag
    assert_bit_equal(sg.par_cast(cam_g, nx, ny, ns, squares=True)[0], sg.par_cast(cam_g, nx, ny, ns), "after the rejections")


def test_stop_rule(pkg, gpu):
    noise = pkg.noise
    nx, ny, ns, step = 48, 32, 40, 4
    sg, cam_g, _, _, _ = build_case(pkg, gpu, "cornell", nx, ny)
    # every slice's estimate, recomputed from the two planes the loop leaves in `out`
    out = np.zeros((2, ny, nx, 3), dtype=np.float32)
    est = []
    for n, frame, se in sg.progressive(cam_g, nx, ny, ns, step, out=out, squares=True):
        assert_bit_equal(frame, sg.par_cast(cam_g, nx, ny, n), "preview at %d" % n)
        assert np.array_equal(se, noise.standard_error(out[0], out[1], n))
        est.append((n, noise.estimated_rmse(out[0], out[1], n)))
    assert [n for n, _ in est] == list(range(step, ns + 1, step))
    assert est[0][1] > est[-1][1] > 0
    for target in (est[2][1], 0.5 * (est[3][1] + est[4][1]), est[0][1] * 10):
        stop = next(n for n, e in est if e <= target)
        got = list(sg.progressive(cam_g, nx, ny, ns, step, target_rmse=target))
        assert [g[0] for g in got] == list(range(step, stop + 1, step)), (target, stop)
        n, frame, se = got[-1]
        assert float(np.sqrt(np.mean(se * se))) <= target
        if len(got) > 1:
            n1, _, se1 = got[-2]
            assert float(np.sqrt(np.mean(se1 * se1))) > target
    got = list(sg.progressive(cam_g, nx, ny, ns, step, target_rmse=1e-30))   # unreachable: runs to ns
    assert got[-1][0] == ns and len(got) == ns // step
    # with a budget already spent: whichever comes first
    got = list(sg.progressive(cam_g, nx, ny, ns, step, target_rmse=1e-30, budget_s=0.0))
    assert [g[0] for g in got] == [step]


def test_the_estimate_matches_the_spread_of_seeds(pkg, gpu):
    """The standard error estimated from one frame's planes predicts how far the pixel means of frames rendered with other
    seeds scatter: mean per-pixel standard error within [0.7, 1.4] x the empirical standard deviation of K frames' means.
    Fixed seeds: deterministic."""
    noise = pkg.noise
    nx, ny, ns, K = 32, 32, 64, 12
    sg, cam_g, _, _, _ = build_case(pkg, gpu, "cornell", nx, ny)
    ses, means = [], []
    for k in range(K):
        planes = sg.par_cast(cam_g, nx, ny, ns, seed=0x5EED0000 + k, squares=True, partial=True)
        ses.append(noise.standard_error(planes[0], planes[1], ns))
        means.append(planes[0].astype(np.float64) / ns)
    spread = np.std(np.array(means), axis=0, ddof=1)
    ratio = float(np.mean(ses) / np.mean(spread))
    assert 0.7 <= ratio <= 1.4, ratio
