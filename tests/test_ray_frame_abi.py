"""Ray frames, CPU side (include/rtiow_gpu_rays.h; Scene.cast_rays; rays.py): the header declares exactly its two entry points
with the prototypes the binding and the Rust module give them, the library exports them and they stay out of the ABI of
rtiow_gpu.h; the refusals that need no device; the host restatement of the camera's rays -- its Philox words against the
oracle's, its rays against the camera in float64; the 64-bit ray index."""
import ctypes as C
import os
import re

import numpy as np

import ray_frame_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu_rays.h")
RAYS_RS = os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "rays.rs")
NAMES = ["par_cast_rays", "par_cast_rays_device"]
ERR_INVALID = -1


def _prototypes(text, strip, pattern):
    text = re.sub(strip, "", text, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip()] for m in re.finditer(pattern, text, flags=re.S)}


def test_the_header_declares_exactly_the_two_entry_points(pkg):
    text = open(HEADER).read()
    c_fns = _prototypes(text, r"/\*.*?\*/", r"\b(rtg_\w+)\s*\(([^)]*)\)\s*;")
    assert sorted(c_fns) == sorted("rtg_" + n for n in NAMES)
    assert pkg.capi.RAY_FRAME_SYMBOLS == NAMES
    assert '#include "rtiow_gpu.h"' in text and "not part of the ABI of rtiow_gpu.h" in text
    assert re.search(r"#define RTG_RAYS_PER_PIXEL 0u", text) and re.search(r"#define RTG_RAYS_PER_SAMPLE 1u", text)
    assert (pkg.capi.RAYS_PER_PIXEL, pkg.capi.RAYS_PER_SAMPLE) == (0, 1)
    # the declared prototypes: (scene, rays, mode, params, out[, stream], stats)
    host, dev = c_fns["rtg_par_cast_rays"], c_fns["rtg_par_cast_rays_device"]
    assert [a.split()[-1].lstrip("*") for a in host] == ["s", "rays7", "ray_mode", "params", "out_rgb", "stats_or_null"]
    assert [a.split()[-1].lstrip("*") for a in dev] == ["s", "d_rays7", "ray_mode", "params", "d_out_rgb", "hip_stream", "stats_or_null"]
    assert "uint32_t ray_mode" in host[2] and "const rtg_params" in host[3] and "const float" in host[1]


def test_the_header_states_the_refusals():
    text = " ".join(open(HEADER).read().split())
    for word in ("RTG_ERR_UNSUPPORTED", "RTG_FLAG_COUNTERS", "TRACE_KERNEL", "SAMPLE_COUNTS", "RETIRE", "DENOISE", "FEATURES",
                 "DENOISE_ERROR", "light_sampling = 1", "RTG_ERR_INVALID", "ray_mode > 1", "sample_begin > ns", "RTG_ERR_DEVICE",
                 "ray_pool"):
        assert word in text, word


def test_the_library_exports_them_with_the_binding_s_prototypes(pkg):
    be = pkg.load()
    for n, argc in zip(NAMES, (6, 7)):
        fn = getattr(be.lib, "rtg_" + n)
        assert fn.restype is C.c_int and len(fn.argtypes) == argc, n
        assert fn.argtypes[2] is C.c_uint32 and fn.argtypes[3] is C.POINTER(pkg.capi.Params)


def test_they_stay_out_of_the_abi_and_the_rust_module_follows_the_header(pkg):
    capi = pkg.capi
    assert not set(NAMES) & set(capi.ABI_SYMBOLS) and not set(NAMES) & set(capi.QUERY_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "rtiow_gpu.h")).read()
    assert "rtg_par_cast_rays" not in main and "RTG_RAYS_PER" not in main
    c_fns = _prototypes(open(HEADER).read(), r"/\*.*?\*/", r"\b(rtg_\w+)\s*\(([^)]*)\)\s*;")
    rs_fns = _prototypes(open(RAYS_RS).read(), r"//[^\n]*", r"pub fn (rtg_\w+)\s*\(([^)]*)\)")
    assert sorted(rs_fns) == sorted(c_fns)
    for name in c_fns:
        assert len(rs_fns[name]) == len(c_fns[name]), name
    lib_rs = open(os.path.join(os.path.dirname(RAYS_RS), "lib.rs")).read()
    assert "pub mod rays;" in lib_rs


def test_scene_option(pkg):
    assert "ray_pool" in pkg.capi.Scene.ENV_OPTIONS


def test_a_null_scene_is_refused(pkg):
    be = pkg.load()
    p = pkg.capi.make_params(2, 1, 1)
    rays = np.zeros((2, 7), np.float32)
    out = np.full((1, 2, 3), 7, np.float32)
    for mode in (0, 1, 2):
        assert be._par_cast_rays(None, rays.ctypes.data, mode, C.byref(p), out.ctypes.data, None) == ERR_INVALID
        assert be._par_cast_rays_device(None, rays.ctypes.data, mode, C.byref(p), out.ctypes.data, None, None) == ERR_INVALID
        assert "null" in be.last_error()
    assert (out == 7).all()


def test_philox_words_equal_the_oracle_s(pkg, oracle):
    """64 random (seed, pixel, sample) keys: the first 12 words of event 0, three blocks."""
    rs = np.random.RandomState(20261020)
    for _ in range(64):
        seed = int(rs.randint(0, 1 << 32)) | (int(rs.randint(0, 1 << 32)) << 32)
        pixel, sample = int(rs.randint(0, 1 << 32)), int(rs.randint(0, 1 << 32))
        want = (C.c_uint32 * 12)()
        oracle.lib.rto_debug_sample_rng_u32(C.c_uint64(seed), C.c_uint32(pixel), C.c_uint32(sample), C.c_uint32(0), C.c_size_t(12), want)
        got = pkg.rays.philox4x32(np.arange(3), sample, pixel, 0, seed).reshape(-1)
        assert got.dtype == np.uint32 and [int(w) for w in got] == [int(w) for w in want], (seed, pixel, sample)


def test_philox_words_broadcast(pkg, oracle):
    """The vectorised generator over arrays of keys gives every key's own words."""
    seed = 0x0123456789ABCDEF
    pixel, sample = np.arange(5, dtype=np.uint32) * 977 + 3, np.arange(5, dtype=np.uint32) + 11
    got = pkg.rays.philox4x32(1, sample, pixel, 0, seed)
    for i in range(5):
        want = (C.c_uint32 * 8)()
        oracle.lib.rto_debug_sample_rng_u32(C.c_uint64(seed), C.c_uint32(int(pixel[i])), C.c_uint32(int(sample[i])), C.c_uint32(0), C.c_size_t(8), want)
        assert [int(w) for w in got[i]] == [int(w) for w in want][4:8]


# Tolerance of the float64 check below.  A ray's coordinates come out of at most 8 chained float32 operations on magnitudes of
# at most 16 (look_from = (13, 2, 3), focus distance 10), each with a relative rounding error of 2^-24 = 6e-8; the camera block
# itself carries the same kind of error from rtg_camera_look.  16 operations x 16 x 6e-8 = 1.5e-5.
TOL = 1.5e-5


def test_camera_rays_lie_on_the_lens_and_the_image_plane(pkg):
    be = pkg.load()
    nx, ny, ns = 10, 10, 4
    pose = ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 1.0, 0.1, 10.0)
    cam = be.camera_look(*pose, (0.0, 1.0))
    rays = pkg.rays.camera_rays(cam, nx, ny, ns, 0xDEADBEEF)
    assert rays.shape == (ns * nx * ny, 7) and rays.dtype == np.float32
    R.check_camera_rays(rays, pose, nx, ny, ns, TOL)
    # another seed gives other rays, the same seed the same ones
    assert np.array_equal(rays, pkg.rays.camera_rays(cam, nx, ny, ns, 0xDEADBEEF))
    assert not np.array_equal(rays, pkg.rays.camera_rays(cam, nx, ny, ns, 1))


def test_camera_rays_of_a_narrow_exposure(pkg):
    """gen_range's scale and offset: every time in [0.25, 0.5)."""
    be = pkg.load()
    cam = be.camera_look((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 1.0, 0.0, 10.0, (0.25, 0.5))
    rays = pkg.rays.camera_rays(cam, 6, 5, 3, 9)
    assert ((rays[:, 6] >= 0.25) & (rays[:, 6] < 0.5)).all()
    assert (rays[:, 0:3] == np.array([13.0, 2.0, 3.0], np.float32)).all()   # a pinhole: every origin is the camera's


def test_the_pixel_centre_generators(pkg):
    G = pkg.rays
    eq = G.equirect_rays((1.0, 2.0, 3.0), 8, 4, time=0.5)
    assert eq.shape == (32, 7) and eq.dtype == np.float32 and (eq[:, 0:3] == (1.0, 2.0, 3.0)).all() and (eq[:, 6] == 0.5).all()
    assert np.allclose(np.linalg.norm(eq[:, 3:6], axis=1), 1.0, atol=1e-6)
    assert (eq[:8, 4] > 0).all() and (eq[-8:, 4] < 0).all()                     # row 0 looks up
    assert np.allclose(eq[:, 3:6].reshape(4, 8, 3).sum(axis=(0, 1)), 0.0, atol=1e-5)   # the sphere is covered evenly about its centre
    fe = G.fisheye_rays((0, 0, 0), (0, 0, -1), (0, 1, 0), 180.0, 5, 5)
    assert np.allclose(fe[12, 3:6], (0, 0, -1), atol=1e-7)                      # the centre pixel looks along the axis
    assert fe[2, 4] > 0 and fe[10, 3] < 0 and fe[14, 3] > 0                     # top looks up, left looks left
    assert np.allclose(np.linalg.norm(fe[:, 3:6], axis=1), 1.0, atol=1e-6)
    assert np.isclose(np.degrees(np.arccos(-fe[10, 5])), 0.8 * 90.0, atol=1e-4)  # equidistant: 0.8 of the radius = 0.8 of fov / 2
    orr = G.ortho_rays((0, 0, 5), (0, 0, 0), (0, 1, 0), 4.0, 2.0, 4, 2)
    assert (orr[:, 3:6] == (0, 0, -1)).all() and (orr[:, 2] == 5).all()
    assert np.allclose(orr[:, 0].reshape(2, 4), [[-1.5, -0.5, 0.5, 1.5]] * 2) and np.allclose(orr[:, 1].reshape(2, 4), [[0.5] * 4, [-0.5] * 4])


def test_the_ray_index_is_exact_beyond_32_bits(pkg):
    """Arithmetic only: sample s of pixel p sits at s * nx * ny + p, also where nx * ny * ns > 2^32."""
    idx = pkg.capi.ray_index
    nx = ny = 65535
    ns = 3
    assert nx * ny * ns > 1 << 32
    assert idx(nx, ny, 0, 0, 0, True) == 0 and idx(nx, ny, 0, 1, 2, True) == nx + 2
    last = idx(nx, ny, ns - 1, ny - 1, nx - 1, True)
    assert last == nx * ny * ns - 1 == 12884508674 and last > 1 << 32
    assert idx(nx, ny, 1, 0, 0, True) - idx(nx, ny, 0, ny - 1, nx - 1, True) == 1     # sample-major, no gap
    assert idx(nx, ny, 2, 7, 9, False) == 7 * nx + 9                                  # per-pixel: the sample does not matter
    # numpy integers are widened, not wrapped
    assert idx(np.uint32(nx), np.uint32(ny), np.uint32(2), np.uint32(ny - 1), np.uint32(nx - 1), True) == last
    assert 7 * 4 * last > 1 << 38                                                      # ... and neither is the byte offset
