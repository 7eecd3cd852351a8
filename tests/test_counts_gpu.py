"""Per-pixel sample counts (include/rtiow_gpu.h RTG_FLAG_SAMPLE_COUNTS): n_p = ns everywhere is bit for bit the call without the
flag (both planes, every counter, whole frames, slices, tiles, both entry points); random counts resolve every pixel to
par_cast(ns = e_p) at that pixel and leave n_p = 0 pixels and other ranks' pixels untouched; slices under changing counts keep
that parity; Scene.adaptive obeys its retire rule and previews bit-exactly -- on every scene case and every kernel."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal, bits
from fuzz_scenes import random_camera, random_world
from scene_cases import CASES, build_case

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")
NAN_BITS = 0x7FC0DEAD


def _nan_frame(pkg, nx, ny, squares=False):
    f = pkg.capi.counts_frame(nx, ny, squares=squares)
    f.planes.view(np.uint32)[...] = NAN_BITS
    return f


def _uniform(sg, cam, nx, ny, ns, what, **kw):
    """n_p = ns everywhere against the flagless call: one call, three slices, with and without squares, counters too."""
    for squares in (False, True):
        ref, st_ref = sg.par_cast(cam, nx, ny, ns, stats=True, squares=squares, **kw)
        f = _nan_frame(_PKG["pkg"], nx, ny, squares)
        f.counts[...] = ns
        f.planes[...] = 0
        got, st = sg.par_cast(cam, nx, ny, ns, out=f.planes, counts=f.counts, stats=True, squares=squares, **kw)
        assert_bit_equal(got, ref, "%s squares=%s: n_p = ns vs no flag" % (what, squares))
        for c in COUNTERS:
            assert st[c] == st_ref[c], (what, squares, c, st[c], st_ref[c])
        f.planes[...] = 0
        total = dict.fromkeys(COUNTERS, 0)
        begin = 0
        for end in (1, max(2, ns // 2), ns):
            _, st = sg.par_cast(cam, nx, ny, end, out=f.planes, counts=f.counts, sample_begin=begin, resume=True,
                                partial=end != ns, squares=squares, stats=True, **kw)
            for c in COUNTERS:
                total[c] += st[c]
            begin = end
        assert_bit_equal(f.planes, ref, "%s squares=%s: 3 slices with n_p = ns" % (what, squares))
        for c in COUNTERS:
            assert total[c] == st_ref[c], (what, "slices", c, total[c], st_ref[c])


_PKG = {}


def _fresh(nx, ny, n, e, squares):
    """A NaN-filled count frame with the counts `n` and +0 running sums where e_p > 0."""
    f = _nan_frame(_PKG["pkg"], nx, ny, squares)
    f.counts[...] = n
    if squares:
        f.planes[:, e > 0] = 0
    else:
        f.planes[e > 0] = 0
    return f


def _random_counts(refs_of, sg, cam, nx, ny, ns, what, seed=1, **kw):
    """Random n_p in [0, ns + 3]: every pixel with e_p > 0 is par_cast(ns = e_p) at that pixel (one render per distinct
    count), n_p = 0 pixels keep their NaN bits, stats.samples is exact; with and without squares, in one call and in two
    slices."""
    rs = np.random.RandomState(seed)
    n = rs.randint(0, ns + 4, size=(ny, nx)).astype(np.uint32)
    n[0, 0], n[-1, -1] = 0, ns + 3
    e = np.minimum(n, ns)
    refs = {int(k): refs_of(k) for k in np.unique(e) if k > 0}
    for squares in (False, True):
        f = _fresh(nx, ny, n, e, squares)
        _, st = sg.par_cast(cam, nx, ny, ns, out=f.planes, counts=f.counts, stats=True, counters=False, squares=squares, **kw)
        assert st["samples"] == int(e.sum()), (what, st["samples"], int(e.sum()))
        plane0 = f.planes[0] if squares else f.planes
        assert (bits(plane0)[e == 0] == NAN_BITS).all(), what + ": n_p = 0 pixels were written"
        for k, ref in refs.items():
            m = e == k
            assert_bit_equal(plane0[m], ref.plain[m], "%s squares=%s: pixels with e_p = %d" % (what, squares, k))
            if squares:
                assert_bit_equal(f.planes[1][m], ref.sq[1][m], "%s: plane 1 of pixels with e_p = %d" % (what, k))
        g = _fresh(nx, ny, n, e, squares)
        k = max(1, ns // 2)
        _, st1 = sg.par_cast(cam, nx, ny, k, out=g.planes, counts=g.counts, partial=True, stats=True, counters=False,
                             squares=squares, **kw)
        _, st2 = sg.par_cast(cam, nx, ny, ns, out=g.planes, counts=g.counts, sample_begin=k, resume=True, stats=True,
                             counters=False, squares=squares, **kw)
        assert st1["samples"] + st2["samples"] == int(e.sum())
        assert_bit_equal(g.planes, f.planes, "%s squares=%s: two slices vs one call" % (what, squares))


class _Ref:
    """par_cast(ns = k): the plain frame and the two-plane squares frame."""
    def __init__(self, sg, cam, nx, ny, k, kw):
        self.plain = sg.par_cast(cam, nx, ny, int(k), **kw)
        self.sq = sg.par_cast(cam, nx, ny, int(k), squares=True, **kw)


def _case_refs(sg, cam, nx, ny, **kw):
    return lambda k: _Ref(sg, cam, nx, ny, k, kw)


@pytest.fixture(autouse=True)
def _remember_pkg(pkg):
    _PKG["pkg"] = pkg


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(pkg, gpu, name):
    sg, cam, nx, ny, ns = build_case(pkg, gpu, name)
    _uniform(sg, cam, nx, ny, ns, name)
    _random_counts(_case_refs(sg, cam, nx, ny), sg, cam, nx, ny, ns, name)


FORCED = [("book2", {"pool2": 2, "sync": 0}, "full pool 2 (second program)"),
          ("book2", {"pool2": 0, "sync": 0}, "full pool: samples"),
          ("cornell", {"sync": 1}, None),
          ("book1", {}, "pool: samples"),
          ("book1", {"chunks": 2}, "chunk(s) of 1 samples"),
          ("book1", {"ray_lds": 0}, None),
          ("book1", {"kernel": 1}, None),
          ("cornell", {"kernel": 1}, None)]


@pytest.mark.parametrize("name,options,verbose_tag", FORCED)
def test_each_kernel_forced(pkg, gpu, name, options, verbose_tag, capfd):
    nx, ny, ns = 64, 48, 8
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    for o, v in options.items():
        sg.set_option(o, v)
    if verbose_tag:
        sg.set_option("verbose", 1)
        capfd.readouterr()
        sg.par_cast(cam, nx, ny, ns, counts=np.full((ny, nx), ns, np.uint32))
        err = capfd.readouterr().err
        assert verbose_tag in err and "[rtg] sample counts:" in err, (verbose_tag, err[-800:])
        sg.set_option("verbose", 0)
    _uniform(sg, cam, nx, ny, ns, "%s %s" % (name, options))
    _random_counts(_case_refs(sg, cam, nx, ny), sg, cam, nx, ny, ns, "%s %s" % (name, options), seed=3)


def test_deep_graph_on_the_baseline_kernel(pkg, gpu):
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
    sg = bg.scene(wg)
    _uniform(sg, cam, nx, ny, ns, "deep %d" % seed)
    _random_counts(_case_refs(sg, cam, nx, ny), sg, cam, nx, ny, ns, "deep %d" % seed)


@pytest.mark.parametrize("name,options", [("book1", {}), ("book2", {}), ("book2", {"pool2": 2}), ("cornell", {}),
                                          ("book1", {"kernel": 1})])
def test_tiles_leave_other_pixels_alone(pkg, gpu, name, options):
    nx, ny, ns = 72, 40, 7   # ragged: tiles past the edge
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    for o, v in options.items():
        sg.set_option(o, v)
    rs = np.random.RandomState(5)
    n = rs.randint(0, ns + 2, size=(ny, nx)).astype(np.uint32)
    e = np.minimum(n, ns)
    whole = _nan_frame(pkg, nx, ny, True)
    whole.counts[...] = n
    whole.planes[:, e > 0] = 0
    _, st_all = sg.par_cast(cam, nx, ny, ns, out=whole.planes, counts=whole.counts, squares=True, stats=True)
    # n_p = ns on every rank reproduces the flagless sharded call
    tx, ty = np.arange(nx) // 8, np.arange(ny) // 8
    tile = ty[:, None] * ((nx + 7) // 8) + tx[None, :]
    canvas = _nan_frame(pkg, nx, ny, True)
    canvas.counts[...] = n
    owned = np.zeros((ny, nx), dtype=bool)
    total = dict.fromkeys(COUNTERS, 0)
    for r in range(3):
        kw = dict(tile_w=8, tile_h=8, rank=r, nranks=3)
        canvas.planes[:, (tile % 3 == r) & (e > 0)] = 0   # this rank's running sums start at +0; the rest stays NaN
        _, st = sg.par_cast(cam, nx, ny, ns, out=canvas.planes, counts=canvas.counts, squares=True, stats=True, **kw)
        for c in COUNTERS:
            total[c] += st[c]
        owned |= tile % 3 == r
        assert st["samples"] == int(e[tile % 3 == r].sum())
        for plane in (0, 1):
            assert (bits(canvas.planes[plane])[~owned & (e > 0)] == NAN_BITS).all(), (name, r, plane)
            assert (bits(canvas.planes[plane])[e == 0] == NAN_BITS).all(), (name, r, plane)
    assert_bit_equal(canvas.planes, whole.planes, "%s 3 ranks vs one" % name)
    for c in COUNTERS:
        assert total[c] == st_all[c], (name, c)


def test_slices_under_changing_counts(pkg, gpu):
    """The adaptive pattern by hand: slices of 3 samples, pixels retiring at random slice ends; at every slice end the resolved
    copy is par_cast(ns = held samples) at every pixel."""
    for name, options in (("book1", {}), ("book2", {"pool2": 2}), ("cornell", {}), ("book1", {"kernel": 1})):
        nx, ny, ns, step = 40, 32, 12, 3
        sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
        for o, v in options.items():
            sg.set_option(o, v)
        refs = {k: sg.par_cast(cam, nx, ny, k) for k in range(step, ns + 1, step)}
        rs = np.random.RandomState(9)
        f = pkg.capi.counts_frame(nx, ny, squares=True)
        f.counts[...] = ns
        active = np.ones((ny, nx), bool)
        done = 0
        while done < ns:
            end = done + step
            sg.par_cast(cam, nx, ny, end, out=f.planes, counts=f.counts, sample_begin=done, resume=True, partial=True,
                        squares=True)
            done = end
            held = np.minimum(f.counts, done)
            retire = active & (rs.rand(ny, nx) < 0.3)
            f.counts[retire] = done
            active &= ~retire
            pv = pkg.capi.counts_frame(nx, ny)
            pv.planes[...] = f.planes[0]
            pv.counts[...] = held
            sg.par_cast(cam, nx, ny, done, out=pv.planes, counts=pv.counts, sample_begin=done, resume=True)
            for k, ref in refs.items():
                m = held == k
                assert_bit_equal(pv.planes[m], ref[m], "%s %s at %d: pixels holding %d" % (name, options, done, k))


@pytest.mark.parametrize("name,nx,ny,ns,step,target", [("book1", 48, 32, 48, 8, 0.03), ("book2", 48, 48, 40, 8, 0.05)])
def test_scene_adaptive(pkg, gpu, name, nx, ny, ns, step, target):
    sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    stats = []
    prev_counts = None
    ends = []
    for counts, preview, se in sg.adaptive(cam, nx, ny, ns, step, target, min_samples=16, stats=stats):
        done = len(ends) * step + step
        ends.append(done)
        assert counts.dtype == np.uint32 and counts.shape == (ny, nx) and counts.max() <= done
        if prev_counts is not None:
            # a pixel that stopped before this slice stays where it stopped; the others moved on by `step`
            held = counts < done   # retired: no samples in this slice, stopped at a slice end >= min_samples
            assert (counts[held] == prev_counts[held]).all() and (counts[held] >= 16).all()
            assert (prev_counts[~held] == done - step).all()
        for k in np.unique(counts):
            ref = sg.par_cast(cam, nx, ny, int(k))
            assert_bit_equal(preview[counts == k], ref[counts == k], "%s preview at %d, pixels holding %d" % (name, done, k))
        # the retire rule, re-applied: exactly the pixels with a good enough estimate stop after this slice
        prev_counts = counts.copy()
    assert sum(st["samples"] for st in stats) == int(prev_counts.sum())
    assert prev_counts.min() < ns or ends[-1] == ns
    assert len(stats) == len(ends)


def test_adaptive_retire_rule_holds(pkg, gpu):
    """At every slice end: a pixel that keeps going either has k < min_samples or an estimate above target; a pixel that
    stops there meets the rule (noise.retire) on the estimate the loop yielded at that slice."""
    nx, ny, ns, step, target, mins = 40, 32, 40, 8, 0.04, 16
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    hist = list((c.copy(), se.copy()) for c, _, se in sg.adaptive(cam, nx, ny, ns, step, target, min_samples=mins))
    for i, (counts, se) in enumerate(hist):
        k = (i + 1) * step
        still = counts == k
        worst = se.max(axis=-1)
        nxt = hist[i + 1][0] if i + 1 < len(hist) else None
        if nxt is not None:
            stops = still & (nxt == k)
            goes = still & (nxt > k)
            assert (worst[stops] <= target).all() and k >= mins or not stops.any()
            assert ((worst[goes] > target) | (k < mins)).all()


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    return hip


def test_device_entry_point(pkg, gpu):
    """rtg_par_cast_device with the flag: n_p = ns equals the flagless device call, random counts equal the host call."""
    hip = _hip()
    for name, nx, ny, ns in (("book1", 96, 64, 10), ("book2", 64, 64, 10), ("cornell", 48, 32, 10)):
        sg, cam, _, _, _ = build_case(pkg, gpu, name, nx, ny)
        rs = np.random.RandomState(2)
        n = rs.randint(0, ns + 2, size=(ny, nx)).astype(np.uint32)
        host = pkg.capi.counts_frame(nx, ny, squares=True)
        host.counts[...] = n
        sg.par_cast(cam, nx, ny, ns, out=host.planes, counts=host.counts, squares=True)
        ref_uniform = sg.par_cast(cam, nx, ny, ns, squares=True)
        stream = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(stream)) == 0
        nf = 2 * nx * ny * 3
        buf = C.c_void_p()
        assert hip.hipMalloc(C.byref(buf), (nf + nx * ny) * 4) == 0
        try:
            for counts, want in ((np.full((ny, nx), ns, np.uint32), ref_uniform), (n, host.planes)):
                assert hip.hipMemset(buf, 0, nf * 4) == 0
                st = sg.par_cast_device(cam, pkg.capi.make_params(nx, ny, ns, squares=True), buf.value, stream.value,
                                        want_stats=True, counts=counts)
                assert hip.hipStreamSynchronize(stream) == 0
                got = np.empty((2, ny, nx, 3), np.float32)
                assert hip.hipMemcpy(got.ctypes.data, buf, got.nbytes, 2) == 0
                assert_bit_equal(got, want, name + " device call")
                assert st["samples"] == int(np.minimum(counts, ns).sum())
                back = np.empty((ny, nx), np.uint32)
                assert hip.hipMemcpy(back.ctypes.data, buf.value + nf * 4, back.nbytes, 2) == 0
                assert (back == counts).all(), "the library wrote the count plane"
        finally:
            hip.hipFree(buf), hip.hipStreamDestroy(stream)


def test_rejections(pkg, gpu):
    nx, ny, ns = 32, 32, 4
    sg, cam, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    buf = np.full((ny, nx, 3), NAN_BITS, dtype=np.uint32).view(np.float32)
    with pytest.raises(pkg.capi.RtError) as ei:
        gpu.par_cast_multi([sg], cam, nx, ny, ns, out=buf, counts=True)
    assert ei.value.code == pkg.capi.ERR_UNSUPPORTED
    assert (bits(buf) == NAN_BITS).all()
    with pytest.raises(pkg.capi.RtError) as ei:
        sg.debug_samples(cam, nx, ny, ns, [1], [1], [0], counts=True)
    assert ei.value.code == pkg.capi.ERR_INVALID


@pytest.mark.parametrize("name", ["book1", "cornell", "book2"])
def test_counters_are_sums_over_the_rendered_pairs(pkg, gpu, oracle, name):
    """On a small frame with random counts: aabb_tests / prim_tests / draws of the counts call equal the oracle's per-sample
    debug_samples info summed over exactly the (pixel, sample) pairs the call rendered."""
    nx, ny, ns, begin = 24, 16, 6, 2
    sg, cam_g, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    so, cam_o, _, _, _ = build_case(pkg, oracle, name, nx, ny)
    rs = np.random.RandomState(4)
    n = rs.randint(0, ns + 2, size=(ny, nx)).astype(np.uint32)
    e = np.minimum(n, ns)
    f = pkg.capi.counts_frame(nx, ny)
    f.counts[...] = n
    _, st = sg.par_cast(cam_g, nx, ny, ns, out=f.planes, counts=f.counts, sample_begin=begin, resume=True, partial=True,
                        stats=True)
    rows, xs = np.nonzero(e > begin)
    xs_all, ys_all, ss_all = [], [], []
    for r, x in zip(rows, xs):
        for s in range(begin, int(e[r, x])):
            xs_all.append(x), ys_all.append(ny - 1 - r), ss_all.append(s)
    assert st["samples"] == len(ss_all)
    _, info = so.debug_samples(cam_o, nx, ny, ns, xs_all, ys_all, ss_all)
    info = info.astype(np.uint64)
    assert st["draws"] == int(info[:, 1].sum()), (name, "draws")
    assert st["aabb_tests"] == int(info[:, 2].sum()), (name, "aabb_tests")
    assert st["prim_tests"] == int(info[:, 3].sum()), (name, "prim_tests")
