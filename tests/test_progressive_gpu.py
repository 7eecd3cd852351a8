"""Progressive rendering (include/rtiow_gpu.h RTG_FLAG_PARTIAL / RTG_FLAG_RESUME): a frame rendered in sample slices is
bit-identical to one par_cast(ns), and the resolve of the running sum after k samples is bit-identical to par_cast(ns = k)
-- against the oracle, which knows nothing of slices, and against one-shot GPU calls, on every kernel."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal, bits
from fuzz_scenes import random_camera, random_world
from scene_cases import CASES, build_case

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")
NAN_BITS = 0x7FC0DEAD


def _sliced(scene, cam, nx, ny, ns, cuts, out=None, stats=False, **kw):
    """Render samples [0, ns) in slices ending at `cuts` (the last slice ends at ns) into the running sum `out`; returns
    (final frame, {k: resolve at k for every cut k}, counters summed over the slices)."""
    acc = np.zeros((ny, nx, 3), dtype=np.float32) if out is None else out
    previews, total = {}, {}
    begin = 0
    for end in list(cuts) + [ns]:
        last = end == ns
        r = scene.par_cast(cam, nx, ny, end, out=acc, sample_begin=begin, resume=True, partial=not last, stats=stats, **kw)
        if stats:
            for k in COUNTERS:
                total[k] = total.get(k, 0) + r[1][k]
        if not last:
            preview = acc.copy()
            scene.par_cast(cam, nx, ny, end, out=preview, sample_begin=end, resume=True, **kw)
            previews[end] = preview
        begin = end
    return acc, previews, total


def _check_three_slices(scene, cam, nx, ny, ns, ref_full, ref_k=None, what="", **kw):
    """Slices [0, 1), [1, k), [k, ns) on the timed and on the instrumented kernels; returns (resolve at k, one-shot k-spp
    frame, counters summed over the slices)."""
    k = max(2, ns // 2)
    one, st_one = scene.par_cast(cam, nx, ny, ns, stats=True, **kw)
    one_k = scene.par_cast(cam, nx, ny, k, **kw)
    for stats in (False, True):
        img, previews, st = _sliced(scene, cam, nx, ny, ns, [1, k], stats=stats, **kw)
        tag = "%s (%s)" % (what, "instrumented" if stats else "timed")
        assert_bit_equal(img, ref_full, tag + ": 3 slices vs oracle par_cast(ns)")
        assert_bit_equal(img, one, tag + ": 3 slices vs one GPU call")
        assert_bit_equal(previews[k], one_k, tag + ": resolve at k vs GPU par_cast(k)")
        if ref_k is not None:
            assert_bit_equal(previews[k], ref_k, tag + ": resolve at k vs oracle par_cast(k)")
        assert_bit_equal(previews[1], scene.par_cast(cam, nx, ny, 1, **kw), tag + ": resolve at 1")
    for c in COUNTERS:
        assert st[c] == st_one[c], (what, c, st[c], st_one[c])
    return previews[k], one_k, st


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_in_three_slices(pkg, gpu, oracle, name):
    sg, cam_g, nx, ny, ns = build_case(pkg, gpu, name)
    so, cam_o, _, _, _ = build_case(pkg, oracle, name)
    k = max(2, ns // 2)
    ref, st_o = so.par_cast(cam_o, nx, ny, ns, stats=True)
    preview, one_k, st = _check_three_slices(sg, cam_g, nx, ny, ns, ref, so.par_cast(cam_o, nx, ny, k), name)
    assert np.array_equal(gpu.tonemap(preview), gpu.tonemap(one_k)), name
    for c in COUNTERS:
        assert st[c] == st_o[c], (name, c, st[c], st_o[c])


@pytest.mark.parametrize("name,options,verbose_tag", [
    ("book2", {"pool2": 2, "sync": 0}, "full pool 2 (second program): samples ["),
    ("book2", {"pool2": 0, "sync": 0}, "full pool: samples ["),
    ("cornell", {"sync": 1}, None),
    ("book1", {"chunks": 1}, None),        # the lean kernel's in-slot fold mode (slice [4, 8): one chunk of 4 samples)
    ("book1", {"chunks": 2}, None),        # chunks of several samples
    ("book1", {}, "pool: samples ["),      # the lean pool kernel, 1-sample slice included
    ("book1", {"bvh4": 1}, None),
    ("book1", {"kernel": 1}, None),        # the baseline kernel
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
    _check_three_slices(sg, cam_g, nx, ny, ns, so.par_cast(cam_o, nx, ny, ns), so.par_cast(cam_o, nx, ny, max(2, ns // 2)),
                        "%s %s" % (name, options))
    if verbose_tag:
        err = capfd.readouterr().err
        # the slices ran on that kernel too: [0, 1) of 1, [1, 4) of 4, [4, 8) of 8 (twice: timed and instrumented)
        for sl in ("[0, 1) of 1", "[1, 4) of 4", "[4, 8) of 8"):
            assert err.count(verbose_tag[:-1] + sl) >= 2, (sl, err[-800:])


def test_deep_graph_on_the_baseline_kernel(pkg, gpu, oracle):
    """A FEAT_DEEP fuzz graph: only the general walk of the baseline kernel renders it."""
    nx, ny, ns = 40, 24, 6
    for seed in range(9000, 9064):
        rs = np.random.RandomState(seed)
        bg = gpu.builder()
        wg = random_world(pkg, bg, rs, general_boundaries=True, deep_shapes=True)
        if bg.flatten(wg)[1] & 128:
            break
    else:
        pytest.fail("no FEAT_DEEP graph among the fuzz seeds")
    cam_g = random_camera(pkg, gpu, rs, nx, ny)
    rs = np.random.RandomState(seed)
    bo = oracle.builder()
    wo = random_world(pkg, bo, rs, general_boundaries=True, deep_shapes=True)
    cam_o = random_camera(pkg, oracle, rs, nx, ny)
    sg, so = bg.scene(wg), bo.scene(wo)
    _check_three_slices(sg, cam_g, nx, ny, ns, so.par_cast(cam_o, nx, ny, ns), so.par_cast(cam_o, nx, ny, 3), "deep %d" % seed)


@pytest.mark.parametrize("name,nx,ny,ns", [("book1", 128, 96, 20), ("book2", 128, 128, 12)])
def test_passes_inside_a_slice(pkg, gpu, oracle, name, nx, ny, ns, capfd):
    """A scratch budget smaller than a slice's sample colours: the slice itself runs in several sample passes."""
    sg, cam_g, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    so, cam_o, _, _, _ = build_case(pkg, oracle, name, nx, ny)
    sg.set_option("scratch_mb", 1)
    sg.set_option("verbose", 1)
    capfd.readouterr()
    img, previews, _ = _sliced(sg, cam_g, nx, ny, ns, [1, 4])
    err = capfd.readouterr().err
    assert err.count(") of %d:" % ns) >= 2 and "samples [4, " in err, err[-800:]   # the last slice: several passes
    sg.set_option("verbose", 0)
    assert_bit_equal(img, so.par_cast(cam_o, nx, ny, ns), name + " slices in passes")
    assert_bit_equal(previews[4], so.par_cast(cam_o, nx, ny, 4), name + " resolve at 4")


@pytest.mark.parametrize("name,options", [("book1", {}), ("book2", {}), ("book2", {"pool2": 2}), ("cornell", {}),
                                          ("book1", {"kernel": 1})])
def test_sharded_slices_leave_other_pixels_alone(pkg, gpu, name, options):
    nx, ny, ns = 72, 40, 7   # ragged: tiles past the edge
    sg, cam_g, _, _, _ = build_case(pkg, gpu, name, nx, ny)
    for o, v in options.items():
        sg.set_option(o, v)
    ref = sg.par_cast(cam_g, nx, ny, ns)
    ref3 = sg.par_cast(cam_g, nx, ny, 3)
    canvas = np.full((ny, nx, 3), NAN_BITS, dtype=np.uint32).view(np.float32)
    tx, ty = np.arange(nx) // 8, np.arange(ny) // 8
    tile = ty[:, None] * ((nx + 7) // 8) + tx[None, :]
    owned_so_far = np.zeros((ny, nx), dtype=bool)
    for r in range(3):
        _, previews, _ = _sliced(sg, cam_g, nx, ny, ns, [1, 3], out=canvas, tile_w=8, tile_h=8, rank=r, nranks=3)
        owned_so_far |= tile % 3 == r
        assert (bits(canvas)[~owned_so_far] == NAN_BITS).all(), (name, r)   # bitwise untouched
        assert_bit_equal(canvas[owned_so_far], ref[owned_so_far], "%s rank %d" % (name, r))
        mine = tile % 3 == r
        assert_bit_equal(previews[3][mine], ref3[mine], "%s rank %d resolve at 3" % (name, r))
        assert (bits(previews[3])[~owned_so_far] == NAN_BITS).all(), (name, r)
    assert_bit_equal(canvas, ref, name + " 3 ranks")


def _hip():
    """Device buffers and streams straight from the HIP runtime the library itself uses (as test_parity_gpu does)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    return hip


def _download(hip, d, shape):
    h = np.empty(shape, dtype=np.float32)
    assert hip.hipMemcpy(h.ctypes.data, d, h.nbytes, 2) == 0   # device to host
    return h


def test_device_path_on_one_stream(pkg, gpu):
    """par_cast_device into device buffers, every slice, copy and resolve on one stream, two frames in flight on the handle."""
    hip = _hip()
    for name, nx, ny, ns in (("book1", 96, 64, 10), ("book2", 64, 64, 10)):
        sg, cam_g, _, _, _ = build_case(pkg, gpu, name, nx, ny)
        sg.set_option("frames_in_flight", 2)
        stream = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(stream)) == 0
        nbytes = nx * ny * 3 * 4
        acc, prev = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(acc), nbytes) == 0 and hip.hipMalloc(C.byref(prev), nbytes) == 0
        try:
            got = []
            for n, p in sg.progressive(cam_g, nx, ny, ns, 3, out=acc.value, preview=prev.value, stream=stream.value):
                assert p == prev.value
                assert hip.hipStreamSynchronize(stream) == 0
                got.append((n, _download(hip, prev, (ny, nx, 3))))
            assert [n for n, _ in got] == [3, 6, 9, 10]
            for n, img in got:
                assert_bit_equal(img, sg.par_cast(cam_g, nx, ny, n), "%s device preview at %d" % (name, n))
            # the same frame in two slices by hand, with stats
            total = {}
            for b, e in ((0, 4), (4, ns)):
                p = pkg.capi.make_params(nx, ny, e, sample_begin=b, resume=True, partial=e != ns, flags=pkg.capi.FLAG_COUNTERS)
                st = sg.par_cast_device(cam_g, p, acc, stream, want_stats=True)
                for k in COUNTERS:
                    total[k] = total.get(k, 0) + st[k]
            assert hip.hipStreamSynchronize(stream) == 0
            one, st_one = sg.par_cast(cam_g, nx, ny, ns, stats=True)
            assert_bit_equal(_download(hip, acc, (ny, nx, 3)), one, name + " device slices")
            assert total == {k: st_one[k] for k in COUNTERS}, (total, st_one)
            # a refused slice (sample_begin > ns) enqueues nothing: the buffer keeps its bits
            p = pkg.capi.make_params(nx, ny, ns, sample_begin=ns + 1, resume=True)
            with pytest.raises(pkg.RtError) as ei:
                sg.par_cast_device(cam_g, p, acc, stream)
            assert ei.value.code == pkg.capi.ERR_INVALID
            assert hip.hipStreamSynchronize(stream) == 0
            assert_bit_equal(_download(hip, acc, (ny, nx, 3)), one, name + " after a refused slice")
        finally:
            hip.hipFree(acc), hip.hipFree(prev), hip.hipStreamDestroy(stream)


@pytest.mark.parametrize("gather", [0, 1])
def test_multi_gpu_slices(pkg, gpu, gather):
    """rtg_par_cast_multi with a clique of one (force_rccl) and with two handles on one device."""
    nx, ny, ns = 80, 48, 8
    ref_scene, cam_g, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    ref, st_ref = ref_scene.par_cast(cam_g, nx, ny, ns, stats=True)
    ref4 = ref_scene.par_cast(cam_g, nx, ny, 4)
    for n in (1, 2):
        scenes = []
        for _ in range(n):
            sg, _, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
            sg.set_option("force_rccl", 1)
            sg.set_option("multi_gather", gather)
            scenes.append(sg)
        acc = np.full((ny, nx, 3), NAN_BITS, dtype=np.uint32).view(np.float32)   # every pixel is owned: overwritten
        total = {}
        for b, e in ((0, 1), (1, 4), (4, ns)):
            _, st = gpu.par_cast_multi(scenes, cam_g, nx, ny, e, out=acc, sample_begin=b, resume=True, partial=e != ns, stats=True)
            for k in COUNTERS:
                total[k] = total.get(k, 0) + st[k]
            if e == 4:
                preview = acc.copy()
                gpu.par_cast_multi(scenes, cam_g, nx, ny, 4, out=preview, sample_begin=4, resume=True)
                assert_bit_equal(preview, ref4, "multi n=%d gather=%d resolve at 4" % (n, gather))
        assert_bit_equal(acc, ref, "multi n=%d gather=%d" % (n, gather))
        assert total == {k: st_ref[k] for k in COUNTERS}, (n, gather, total)
    # 20 x 12 in 8x8 tiles over 3 handles (two tiles per rank, pixels beyond the image inside them), as a PARTIAL then RESUME
    # pair: the resumed ranks start from the caller's sums on their own tiles and +0 elsewhere
    nx, ny, ns = 20, 12, 6
    ref_scene, cam_g, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    ref, st_ref = ref_scene.par_cast(cam_g, nx, ny, ns, stats=True)
    scenes = []
    for _ in range(3):
        sg, _, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
        sg.set_option("multi_gather", gather)
        scenes.append(sg)
    acc = np.full((ny, nx, 3), NAN_BITS, dtype=np.uint32).view(np.float32)
    total = {}
    for b, e in ((0, 2), (2, ns)):
        _, st = gpu.par_cast_multi(scenes, cam_g, nx, ny, e, out=acc, sample_begin=b, resume=b != 0, partial=e != ns, stats=True, tile_w=8, tile_h=8)
        for k in COUNTERS:
            total[k] = total.get(k, 0) + st[k]
    assert_bit_equal(acc, ref, "multi 20 x 12, 3 handles, gather=%d, 2 + 4 samples" % gather)
    assert total == {k: st_ref[k] for k in COUNTERS}, (gather, total)
    gpu.multi_reset()


def test_scene_progressive(pkg, gpu, oracle):
    nx, ny, ns = 64, 48, 10
    sg, cam_g, _, _, _ = build_case(pkg, gpu, "book2", nx, ny)
    so, cam_o, _, _, _ = build_case(pkg, oracle, "book2", nx, ny)
    got = list(sg.progressive(cam_g, nx, ny, ns, 4))
    assert [n for n, _ in got] == [4, 8, 10]
    for n, p in got:
        assert_bit_equal(p, so.par_cast(cam_o, nx, ny, n), "progressive preview at %d" % n)
    # a budget already spent after the first slice: one preview, then stop
    got = list(sg.progressive(cam_g, nx, ny, ns, 3, budget_s=0.0))
    assert [n for n, _ in got] == [3]
    assert_bit_equal(got[0][1], sg.par_cast(cam_g, nx, ny, 3), "budgeted preview")


def test_errors_leave_the_buffer_alone(pkg, gpu):
    nx, ny, ns = 32, 32, 4
    sg, cam_g, _, _, _ = build_case(pkg, gpu, "book1", nx, ny)
    buf = np.full((ny, nx, 3), NAN_BITS, dtype=np.uint32).view(np.float32)
    for partial in (False, True):
        with pytest.raises(pkg.RtError) as ei:
            sg.par_cast(cam_g, nx, ny, ns, out=buf, sample_begin=ns + 1, resume=True, partial=partial)
        assert ei.value.code == pkg.capi.ERR_INVALID and "sample_begin" in str(ei.value)
        with pytest.raises(pkg.RtError) as ei:
            gpu.par_cast_multi([sg], cam_g, nx, ny, ns, out=buf, sample_begin=ns + 1, resume=True, partial=partial)
        assert ei.value.code == pkg.capi.ERR_INVALID
    assert (bits(buf) == NAN_BITS).all()
    for kw in ({"partial": True}, {"resume": True, "sample_begin": 1}, {"resume": True}):
        with pytest.raises(pkg.RtError) as ei:
            sg.debug_samples(cam_g, nx, ny, ns, [1], [1], [0], **kw)
        assert ei.value.code == pkg.capi.ERR_INVALID, kw
    # sample_begin without RTG_FLAG_RESUME is ignored, as `reserved` was
    assert_bit_equal(sg.par_cast(cam_g, nx, ny, ns, sample_begin=3), sg.par_cast(cam_g, nx, ny, ns), "sample_begin ignored")
    # sample_begin == 0 with RESUME: as without it
    assert_bit_equal(sg.par_cast(cam_g, nx, ny, ns, out=buf.copy(), resume=True), sg.par_cast(cam_g, nx, ny, ns), "resume at 0")
