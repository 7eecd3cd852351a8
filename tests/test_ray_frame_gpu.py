"""Ray frames on the GPU (include/rtiow_gpu_rays.h; Scene.cast_rays): a frame of the camera's own rays, restated on the host
(rays.camera_rays), is the rtg_par_cast frame bit for bit -- on the lean pool kernel and on the general kernel, on lean, Cornell,
media, motion and FEAT_DEEP programs; the frame machinery (slices, squares plane, background, ranks, host against device);
per-pixel against per-sample rays; exact answers the oracle did not supply; refusals."""
import ctypes as C

import numpy as np
import pytest

import ray_frame_ref as R
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEF
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
LEAN_LINE, GENERAL_LINE = "[rtg] ray frame: lean pool kernel", "[rtg] ray frame: general kernel"

_scenes, _refs = {}, {}


def scene_of(pkg, gpu, name, nx, ny):
    """One handle per (scene, frame size) for the whole module; every test sets the options it needs."""
    key = (name, nx, ny)
    if key not in _scenes:
        _scenes[key] = R.build(pkg, gpu, name, nx, ny)
    return _scenes[key]


def reference(pkg, gpu, name, nx, ny, ns):
    """(scene, camera, the camera's rays restated on the host, rtg_par_cast's frame), computed once and left unchanged."""
    key = (name, nx, ny, ns)
    if key not in _refs:
        sc, cam = scene_of(pkg, gpu, name, nx, ny)
        rays = pkg.rays.camera_rays(cam, nx, ny, ns, SEED)
        frame = sc.par_cast(cam, nx, ny, ns, seed=SEED)
        rays.setflags(write=False), frame.setflags(write=False)
        _refs[key] = (sc, cam, rays, frame)
    return _refs[key]


def cast(sc, route, capfd, rays, nx, ny, ns, **kw):
    """Scene.cast_rays on the route `route` (option ray_pool), with the proof from option verbose that the kernel was taken."""
    sc.set_option("ray_pool", route)
    sc.set_option("verbose", 1)
    capfd.readouterr()
    try:
        out = sc.cast_rays(rays, nx, ny, ns, seed=SEED, **kw)
    finally:
        sc.set_option("verbose", 0)
    err = capfd.readouterr().err
    if kw.get("sample_begin", 0) < ns:
        want, other = (LEAN_LINE, GENERAL_LINE) if route else (GENERAL_LINE, LEAN_LINE)
        assert want in err and other not in err, err[-800:]
        if route:
            assert "[rtg] pool: samples [" in err and "full pool" not in err, err[-800:]
    return out


# ---- 1. camera-ray parity ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,nx,ny,ns,route", [("book1", 48, 32, 4, 1), ("book1", 48, 32, 4, 0), ("book1", 10, 10, 4, 1), ("book1", 10, 10, 4, 0),
                                                 ("cornell", 24, 24, 4, 0), ("volume", 24, 24, 4, 0), ("motion", 24, 24, 4, 0), ("deep", 16, 16, 2, 0)])
def test_the_camera_s_own_rays_give_the_par_cast_frame(pkg, gpu, oracle, capfd, name, nx, ny, ns, route):
    sc, cam, rays, frame = reference(pkg, gpu, name, nx, ny, ns)
    so, cam_o = R.build(pkg, oracle, name, nx, ny)
    assert_bit_equal(frame, so.par_cast(cam_o, nx, ny, ns, seed=SEED), "par_cast against the oracle: " + name)
    got = cast(sc, route, capfd, rays, nx, ny, ns, per_sample=True)
    assert got.shape == (ny, nx, 3) and got.dtype == np.float32
    assert_bit_equal(got, frame, "ray frame of the camera's rays: %s, ray_pool %d" % (name, route))
    assert np.isfinite(frame).all() and frame.max() > 0


def test_a_lean_program_takes_the_general_kernel_only_when_told(pkg, gpu, capfd):
    """The default of option ray_pool on a lean program, and every other program whatever the option says."""
    sc, cam, rays, frame = reference(pkg, gpu, "cornell", 24, 24, 4)
    sc.set_option("ray_pool", 1)
    sc.set_option("verbose", 1)
    capfd.readouterr()
    got = sc.cast_rays(rays, 24, 24, 4, per_sample=True, seed=SEED)
    sc.set_option("verbose", 0)
    assert GENERAL_LINE in capfd.readouterr().err
    assert_bit_equal(got, frame, "cornell with ray_pool = 1")


# ---- 2. frame machinery -----------------------------------------------------------------------------------------------------

MACHINERY = [("book1", 48, 32, 4, 1), ("book1", 48, 32, 4, 0), ("cornell", 24, 24, 4, 0)]
IDS = ["book1-pool", "book1-general", "cornell"]


@pytest.mark.parametrize("name,nx,ny,ns,route", MACHINERY, ids=IDS)
def test_two_slices_equal_the_one_call(pkg, gpu, capfd, name, nx, ny, ns, route):
    capi = pkg.capi
    sc, cam, rays, frame = reference(pkg, gpu, name, nx, ny, ns)
    acc = cast(sc, route, capfd, rays[:2 * nx * ny], nx, ny, 2, per_sample=True, flags=capi.FLAG_PARTIAL)
    half = sc.par_cast(cam, nx, ny, 2, seed=SEED, partial=True)
    assert_bit_equal(acc, half, "the running sum of samples [0, 2)")
    # only the rays of samples [2, 4) are read: the first half of the array is poison
    poisoned = np.array(rays)
    poisoned[:2 * nx * ny] = np.nan
    got = cast(sc, route, capfd, poisoned, nx, ny, ns, per_sample=True, flags=capi.FLAG_RESUME, sample_begin=2, out=acc)
    assert got is acc
    assert_bit_equal(got, frame, "slices [0, 2) PARTIAL + [2, 4) RESUME")
    # ... and the resolve step alone: a sum of all four samples, then sample_begin = ns
    total = cast(sc, route, capfd, rays, nx, ny, ns, per_sample=True, flags=capi.FLAG_PARTIAL)
    assert_bit_equal(cast(sc, route, capfd, poisoned * np.float32(np.nan), nx, ny, ns, per_sample=True, flags=capi.FLAG_RESUME, sample_begin=ns, out=total),
                     frame, "resolve step")


@pytest.mark.parametrize("name,nx,ny,ns,route", MACHINERY, ids=IDS)
def test_sum_of_squares(pkg, gpu, capfd, name, nx, ny, ns, route):
    sc, cam, rays, frame = reference(pkg, gpu, name, nx, ny, ns)
    want = sc.par_cast(cam, nx, ny, ns, seed=SEED, squares=True)
    got = cast(sc, route, capfd, rays, nx, ny, ns, per_sample=True, flags=pkg.capi.FLAG_SUM_SQUARES)
    assert got.shape == (2, ny, nx, 3)
    assert_bit_equal(got[0], want[0], "plane 0")
    assert_bit_equal(got[1], want[1], "plane 1")
    assert_bit_equal(got[0], frame, "plane 0 is the frame without the flag")
    assert got[1].max() > 0


@pytest.mark.parametrize("name,nx,ny,ns,route", MACHINERY, ids=IDS)
def test_gradient_background(pkg, gpu, capfd, name, nx, ny, ns, route):
    sc, cam, rays, frame = reference(pkg, gpu, name, nx, ny, ns)
    sky = {"bottom": (1.0, 1.0, 1.0), "top": (0.5, 0.7, 1.0)}
    want = sc.par_cast(cam, nx, ny, ns, seed=SEED, background=sky)
    got = cast(sc, route, capfd, rays, nx, ny, ns, per_sample=True, background=sky)
    assert_bit_equal(got, want, "RTG_FLAG_BACKGROUND mode 1")
    if name == "cornell":   # (book-1's dome hides the sky)
        assert not np.array_equal(want, frame)


@pytest.mark.parametrize("name,nx,ny,ns,route", MACHINERY, ids=IDS)
def test_two_ranks_are_disjoint_and_their_union_is_the_frame(pkg, gpu, capfd, name, nx, ny, ns, route):
    sc, cam, rays, frame = reference(pkg, gpu, name, nx, ny, ns)
    parts, stats = [], []
    for rank in (0, 1):
        out = np.full((ny, nx, 3), -7.0, np.float32)
        got, st = cast(sc, route, capfd, rays, nx, ny, ns, per_sample=True, out=out, rank=rank, nranks=2, tile_w=8, tile_h=8, stats=True)
        parts.append(np.array(got))
        stats.append(st)
    own = [(p != -7.0).any(axis=-1) for p in parts]
    tile = (np.arange(ny)[:, None] // 8) * ((nx + 7) // 8) + np.arange(nx)[None, :] // 8
    for rank in (0, 1):
        assert np.array_equal(own[rank], tile % 2 == rank), "rank %d wrote other pixels than its tiles'" % rank
        assert stats[rank]["samples"] == int(own[rank].sum()) * ns and stats[rank]["kernel_ms"] > 0
        assert all(stats[rank][k] == 0 for k in ("aabb_tests", "prim_tests", "shaded_hits", "rays", "draws"))
    assert_bit_equal(np.where(own[0][..., None], parts[0], parts[1]), frame, "the union of the two ranks")


class Hip:
    """The HIP runtime the library links, through ctypes: device arrays of the test's own."""

    def __init__(self):
        h = self.lib = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipFree.argtypes = [C.c_void_p]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.held = []

    def array(self, host):
        host = np.ascontiguousarray(host)
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), max(host.nbytes, 16)) == 0
        assert self.lib.hipMemcpy(p, host.ctypes.data, host.nbytes, 1) == 0
        self.held.append(p)
        return p.value

    def read(self, ptr, like):
        out = np.empty_like(like)
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
        return out

    def close(self):
        assert self.lib.hipDeviceSynchronize() == 0
        for p in self.held:
            self.lib.hipFree(p)
        self.held = []


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.mark.parametrize("name,nx,ny,ns,route", MACHINERY, ids=IDS)
def test_the_device_variant_gives_the_host_variant_s_frame(pkg, gpu, hip, name, nx, ny, ns, route):
    """rtg_par_cast_rays_device on device arrays of the test's own, without stats (asynchronous) and with them."""
    capi = pkg.capi
    sc, cam, rays, frame = reference(pkg, gpu, name, nx, ny, ns)
    sc.set_option("ray_pool", route)
    d_rays = hip.array(rays)
    for stats in (False, True):
        d_out = hip.array(np.full((ny, nx, 3), -7.0, np.float32))
        p, st = capi.make_params(nx, ny, ns, seed=SEED), capi.Stats.new()
        gpu.check(gpu._par_cast_rays_device(sc.h, d_rays, capi.RAYS_PER_SAMPLE, C.byref(p), d_out, None, C.byref(st) if stats else None))
        assert_bit_equal(hip.read(d_out, frame), frame, "device variant, stats %s" % stats)
        if stats:
            assert st.samples == nx * ny * ns and st.kernel_ms > 0 and st.rays == 0 and st.draws == 0


# ---- 3. per-pixel mode ------------------------------------------------------------------------------------------------------

def test_one_ray_per_pixel_equals_the_same_rays_per_sample(pkg, gpu, capfd):
    """130 x 1 rays: no multiple of 8 or 64, one row."""
    nx, ny, ns = 130, 1, 4
    sc, cam = scene_of(pkg, gpu, "book1", 48, 32)
    rays = R.pinhole_rays(cam, nx, ny)
    tiled = np.ascontiguousarray(np.tile(rays, (ns, 1)))
    frames = []
    for route in (1, 0):
        per_pixel = cast(sc, route, capfd, rays, nx, ny, ns)
        per_sample = cast(sc, route, capfd, tiled, nx, ny, ns, per_sample=True)
        assert_bit_equal(per_pixel, per_sample, "per-pixel against per-sample rays, ray_pool %d" % route)
        frames.append(per_pixel)
    assert_bit_equal(frames[0], frames[1], "lean pool kernel against general kernel")
    assert frames[0].shape == (1, 130, 3) and np.isfinite(frames[0]).all() and (frames[0].max(axis=-1) > 0).all()
    # a ray array of the wrong length is refused by the binding
    with pytest.raises(ValueError):
        sc.cast_rays(tiled, nx, ny, ns)


# ---- 4. exact answers the oracle did not supply -----------------------------------------------------------------------------

NX4, NY4, NS4 = 9, 5, 4
BOTTOM = (0.25, 0.5, 0.75)


def _lone_sphere(gpu, material):
    b = gpu.builder()
    return b.scene([b.sphere(1.0, material(b))])


@pytest.mark.parametrize("route", [1, 0])
def test_rays_at_a_lone_light_see_its_emission_exactly(pkg, gpu, capfd, route):
    sc = _lone_sphere(gpu, lambda b: b.diffuse_light(b.constant(pkg.scenes.v(1.0, 0.5, 0.25)), 3.0))
    got = cast(sc, route, capfd, R.aimed_rays((0.0, 0.0, 0.0), NX4, NY4), NX4, NY4, NS4)
    assert (got == np.array([3.0, 1.5, 0.75], np.float32)).all(), got.reshape(-1, 3)[:4]


@pytest.mark.parametrize("route", [1, 0])
def test_rays_that_miss_see_the_constant_background_exactly(pkg, gpu, capfd, route):
    sc = _lone_sphere(gpu, lambda b: b.lambertian(b.constant(pkg.scenes.vfrom(0.5))))
    away = R.aimed_rays((0.0, 0.0, 0.0), NX4, NY4)
    away[:, 3:6] = -away[:, 3:6]
    got = cast(sc, route, capfd, away, NX4, NY4, NS4, background=BOTTOM)
    assert (got == np.array(BOTTOM, np.float32)).all(), got.reshape(-1, 3)[:4]
    # without a background a miss is black (lib.rs:100)
    assert (cast(sc, route, capfd, away, NX4, NY4, NS4) == 0).all()


@pytest.mark.parametrize("route", [1, 0])
def test_the_bounce_cap_ends_a_path_at_its_first_hit(pkg, gpu, capfd, route):
    sc = _lone_sphere(gpu, lambda b: b.lambertian(b.constant(pkg.scenes.vfrom(0.5))))
    at = R.aimed_rays((0.0, 0.0, 0.0), NX4, NY4)
    got = cast(sc, route, capfd, at, NX4, NY4, NS4, background=BOTTOM, max_bounces=0)
    assert (got == 0).all(), got.reshape(-1, 3)[:4]
    # one bounce more and the scattered ray leaves for the background: 0.5 x bottom, exactly
    got = cast(sc, route, capfd, at, NX4, NY4, NS4, background=BOTTOM, max_bounces=1)
    assert (got == np.float32(0.5) * np.array(BOTTOM, np.float32)).all(), got.reshape(-1, 3)[:4]


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_frame_untouched(pkg, gpu, hip):
    capi = pkg.capi
    nx, ny, ns = 16, 8, 2
    sc, cam = scene_of(pkg, gpu, "book1", 48, 32)
    rays = np.ascontiguousarray(np.tile(R.pinhole_rays(cam, nx, ny), (ns, 1)))
    words = capi.FrameLayout(nx, ny, squares=True, background=True).words + 8 * nx * ny   # room for every flag's planes
    canary = np.full(words, 7.0, np.float32)
    d_rays, d_out = hip.array(rays), hip.array(canary)

    def params(**kw):
        fields = {k: kw.pop(k) for k in ("struct_size",) if k in kw}
        p = capi.make_params(kw.pop("nx", nx), kw.pop("ny", ny), kw.pop("ns", ns), seed=SEED, **kw)
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    def both(code, word, p, mode=1, rays_ptr=True, out_ptr=True, stats=None, null_params=False):
        out = np.array(canary)
        pp = None if null_params else C.byref(p)
        st = C.byref(stats) if stats is not None else None
        assert gpu._par_cast_rays(sc.h, rays.ctypes.data if rays_ptr else None, mode, pp, out.ctypes.data if out_ptr else None, st) == code, word
        assert word in gpu.last_error(), (word, gpu.last_error())
        assert gpu._par_cast_rays_device(sc.h, d_rays if rays_ptr else None, mode, pp, d_out if out_ptr else None, None, st) == code, word
        assert word in gpu.last_error(), (word, gpu.last_error())
        assert (out == 7.0).all() and (hip.read(d_out, canary) == 7.0).all(), word

    for flag in (capi.FLAG_COUNTERS, capi.FLAG_TRACE_KERNEL, capi.FLAG_SAMPLE_COUNTS, capi.FLAG_RETIRE | capi.FLAG_SAMPLE_COUNTS | capi.FLAG_SUM_SQUARES,
                 capi.FLAG_DENOISE | capi.FLAG_SUM_SQUARES, capi.FLAG_FEATURES, capi.FLAG_DENOISE_ERROR | capi.FLAG_DENOISE | capi.FLAG_SUM_SQUARES,
                 capi.FLAG_RETIRE, capi.FLAG_DENOISE, capi.FLAG_DENOISE_ERROR):
        both(ERR_UNSUPPORTED, "not supported on ray frames", params(flags=flag))
    sc.set_option("light_sampling", 1)
    try:
        both(ERR_UNSUPPORTED, "light_sampling", params())
    finally:
        sc.set_option("light_sampling", 0)
    both(ERR_INVALID, "ray_mode", params(), mode=2)
    both(ERR_INVALID, "ray_mode", params(), mode=0xffffffff)
    both(ERR_INVALID, "null", params(), null_params=True)
    both(ERR_INVALID, "null", params(), rays_ptr=False)
    both(ERR_INVALID, "null", params(), out_ptr=False)
    both(ERR_INVALID, "rtg_params.struct_size", params(struct_size=52))
    both(ERR_INVALID, "rtg_params.struct_size", params(struct_size=0))
    bad_stats = capi.Stats.new()
    bad_stats.struct_size = 48
    both(ERR_INVALID, "rtg_stats.struct_size", params(), stats=bad_stats)
    for zero in ("nx", "ny", "ns"):
        both(ERR_INVALID, "must be > 0", params(**{zero: 0}))
    both(ERR_INVALID, "sample_begin > ns", params(flags=capi.FLAG_RESUME, sample_begin=ns + 1))
    # the refusals the honoured flags and the tile / rank fields define
    both(ERR_INVALID, "multiples of 8", params(tile_w=12))
    both(ERR_INVALID, "rank >= nranks", params(rank=2, nranks=2))
    # a background block with mode 2: the block sits at the end of the one-plane frame
    lay = capi.FrameLayout(nx, ny, background=True)
    block = capi.make_background({"bottom": (0.5, 0.5, 0.5), "mode": 0})
    block.mode = 2
    raw = np.frombuffer(bytes(block), np.float32)
    host = np.array(canary)
    host[lay.background:lay.background + 16] = raw
    p = params(flags=capi.FLAG_BACKGROUND)
    assert gpu._par_cast_rays(sc.h, rays.ctypes.data, 1, C.byref(p), host.ctypes.data, None) == ERR_INVALID and "mode > 1" in gpu.last_error()
    assert (host[:lay.background] == 7.0).all()
    d_bad = hip.array(host)
    assert gpu._par_cast_rays_device(sc.h, d_rays, 1, C.byref(p), d_bad, None, None) == ERR_INVALID and "mode > 1" in gpu.last_error()
    assert hip.read(d_bad, host).tobytes() == host.tobytes()
    # the handle still renders
    frame = sc.cast_rays(rays, nx, ny, ns, per_sample=True, seed=SEED)
    assert np.isfinite(frame).all() and frame.max() > 0
    with pytest.raises(pkg.capi.RtError):
        sc.set_option("ray_pool", 2)


# ---- the binding on torch tensors --------------------------------------------------------------------------------------------

TORCH_CHILD = r"""
import sys
import numpy as np
import torch
assert torch.cuda.is_available()   # torch's HIP runtime first (INTEGRATION.md: one HIP runtime per process), then the library
sys.path[:0] = [%(root)r, %(tests)r]
import __graft_entry__ as graft
import ray_frame_ref as R
pkg = graft.load_package()
gpu = pkg.load()
nx, ny, ns = 48, 32, 4
sc, cam = R.build(pkg, gpu, "book1", nx, ny)
rays = pkg.rays.camera_rays(cam, nx, ny, ns, 7)
want = sc.par_cast(cam, nx, ny, ns, seed=7)
sky = {"bottom": (1.0, 1.0, 1.0), "top": (0.5, 0.7, 1.0)}
for route in (1, 0):
    sc.set_option("ray_pool", route)
    assert sc.cast_rays(rays, nx, ny, ns, per_sample=True, seed=7).tobytes() == want.tobytes()
    stream = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    got = sc.cast_rays(d_rays, nx, ny, ns, per_sample=True, seed=7, stream=stream)
    stream.synchronize()
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (ny, nx, 3)
    assert got.cpu().numpy().tobytes() == want.tobytes(), route
    acc = sc.cast_rays(d_rays[:2 * nx * ny].contiguous(), nx, ny, 2, per_sample=True, seed=7, flags=pkg.capi.FLAG_PARTIAL, stream=stream)
    res = sc.cast_rays(d_rays, nx, ny, ns, per_sample=True, seed=7, flags=pkg.capi.FLAG_RESUME, sample_begin=2, out=acc, stream=stream)
    stream.synchronize()
    assert res.data_ptr() == acc.data_ptr() and res.cpu().numpy().tobytes() == want.tobytes(), route
    with torch.cuda.stream(stream):   # no stream given: the current torch stream; a background block written by the binding
        bg = sc.cast_rays(d_rays, nx, ny, ns, per_sample=True, seed=7, background=sky)
    stream.synchronize()
    assert bg.cpu().numpy().tobytes() == sc.par_cast(cam, nx, ny, ns, seed=7, background=sky).tobytes()
    for bad in (d_rays.double(), d_rays.t(), d_rays.cpu(), d_rays[:5].contiguous()):
        try:
            sc.cast_rays(bad, nx, ny, ns, per_sample=True)
        except ValueError:
            continue
        raise AssertionError("a tensor that is not the frame's contiguous float32 rays on the device was accepted")
    print("torch tensors on a stream: ray_pool", route, "ok")
print("TORCH CHILD OK")
"""


def test_torch_tensors_on_a_stream_give_the_host_path_bytes():
    """Scene.cast_rays on torch tensors, in and out, on a non-default stream: the host path's bytes on both routes.  In a process
    of its own, which is what the test is about: a process that uses torch and the library initialises torch's HIP runtime
    first, and this one has loaded the library long ago."""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    code = TORCH_CHILD % {"root": os.path.dirname(tests), "tests": tests}
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "TORCH CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
