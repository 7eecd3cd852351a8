"""Per-pixel sample counts, CPU side: RTG_FLAG_SAMPLE_COUNTS in the header, the ctypes binding and the Rust `-sys` crate, the ABI
structs and symbol list unchanged, the count frame's layout, noise.standard_error_counts against a direct float64 computation,
the adaptive retire rule on synthetic sums, and the oracle refusing counts=."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu.h")
SYS_RS = os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "lib.rs")


def _header_flags():
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RTG_FLAG_[A-Z_]+) (\d+)u", open(HEADER).read())}


def test_header_declares_the_flag():
    flags = _header_flags()
    assert flags["RTG_FLAG_SAMPLE_COUNTS"] == 32
    others = 0
    for name, v in flags.items():
        assert v & (v - 1) == 0, (name, v)   # one bit each
        if name != "RTG_FLAG_SAMPLE_COUNTS":
            others |= v
    assert not others & 32


def test_capi_and_rust_match_the_header(pkg):
    assert pkg.capi.FLAG_SAMPLE_COUNTS == _header_flags()["RTG_FLAG_SAMPLE_COUNTS"]
    assert re.search(r"pub const RTG_FLAG_SAMPLE_COUNTS: u32 = 32;", open(SYS_RS).read())
    p = pkg.capi.make_params(8, 8, 4, counts=True, squares=True, partial=True)
    assert p.flags == pkg.capi.FLAG_SAMPLE_COUNTS | pkg.capi.FLAG_SUM_SQUARES | pkg.capi.FLAG_PARTIAL
    assert pkg.capi.make_params(8, 8, 4).flags == 0


def test_abi_sizes_and_symbols_unchanged(pkg):
    capi = pkg.capi
    assert C.sizeof(capi.Params) == 56 and C.sizeof(capi.Stats) == 56
    assert len(capi.ABI_SYMBOLS) == 42
    declared = set(re.findall(r"\brtg_([a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(capi.ABI_SYMBOLS), declared ^ set(capi.ABI_SYMBOLS)


def test_header_places_the_count_plane_after_the_float_planes():
    text = re.sub(r"\s+", " ", re.sub(r"\n \* ", " ", open(HEADER).read()))
    assert "at word 3 * nx * ny without RTG_FLAG_SUM_SQUARES and at word 6 * nx * ny with it" in text


@pytest.mark.parametrize("squares", [False, True])
def test_counts_frame_layout(pkg, squares):
    nx, ny = 7, 5
    f = pkg.capi.counts_frame(nx, ny, squares=squares)
    planes = 2 if squares else 1
    assert f.buf.dtype == np.float32 and f.buf.size == planes * nx * ny * 3 + nx * ny
    assert f.planes.shape == ((2, ny, nx, 3) if squares else (ny, nx, 3)) and f.planes.dtype == np.float32
    assert f.counts.shape == (ny, nx) and f.counts.dtype == np.uint32
    base = f.buf.ctypes.data
    assert f.planes.ctypes.data == base
    assert f.counts.ctypes.data == base + 4 * planes * 3 * nx * ny   # word 3 nx ny, or 6 nx ny with squares
    f.counts[2, 3] = 0xdeadbeef
    assert f.buf.view(np.uint32)[planes * 3 * nx * ny + 2 * nx + 3] == 0xdeadbeef   # row-major, row 0 first
    # the in-place route of par_cast: a frame's own views need no staging copy
    dst, staging = pkg.capi._counts_call(f.planes, f.counts, nx, ny, squares)
    assert staging is None and dst is f.planes
    dst, staging = pkg.capi._counts_call(np.zeros(f.planes.shape, np.float32), f.counts.copy(), nx, ny, squares)
    assert staging is not None and staging.counts[2, 3] == 0xdeadbeef


def test_standard_error_counts_against_a_direct_computation(pkg):
    noise = pkg.noise
    rs = np.random.RandomState(11)
    ny, nx = 6, 5
    n = rs.randint(0, 40, size=(ny, nx))
    n[0, 0], n[0, 1], n[0, 2] = 0, 1, 2
    s = np.zeros((ny, nx, 3), np.float32)
    q = np.zeros((ny, nx, 3), np.float32)
    want = np.full((ny, nx, 3), np.inf)
    for y in range(ny):
        for x in range(nx):
            samples = rs.gamma(0.5, 0.4, size=(n[y, x], 3)).astype(np.float32)
            for c in samples:
                s[y, x] = s[y, x] + c
                q[y, x] = q[y, x] + c * c
            if n[y, x] >= 2:
                want[y, x] = np.sqrt(samples.astype(np.float64).var(axis=0, ddof=1) / n[y, x])
    got = noise.standard_error_counts(s, q, n.astype(np.uint32))
    assert got.dtype == np.float64 and got.shape == s.shape
    assert np.isinf(got[0, 0]).all() and np.isinf(got[0, 1]).all()
    np.testing.assert_allclose(got, want, rtol=2e-3, atol=1e-6)
    # a uniform count gives exactly standard_error
    k = np.full((ny, nx), 9, np.uint32)
    np.testing.assert_array_equal(noise.standard_error_counts(s, q, k), noise.standard_error(s, q, 9))
    with pytest.raises(ValueError):
        noise.standard_error_counts(s, q, k[:, :3])


def test_retire_rule_on_synthetic_sums(pkg):
    noise = pkg.noise
    ny, nx = 4, 6
    se = np.full((ny, nx, 3), 0.5)
    se[0, :, :] = 0.01             # row 0: converged in every channel
    se[1, :, 1] = 0.01             # row 1: one channel still noisy
    se[1, :, 0] = se[1, :, 2] = 0.2
    se[2, :, :] = 0.05             # row 2: exactly at the target
    active = np.ones((ny, nx), bool)
    active[0, 0] = False           # already retired: stays out of the mask
    # before min_samples nothing retires
    assert not noise.retire(active, 8, se, 16, 0.05).any()
    r = noise.retire(active, 16, se, 16, 0.05)
    assert r.dtype == bool and r.shape == (ny, nx)
    want = np.zeros((ny, nx), bool)
    want[0, 1:] = True
    want[2, :] = True
    np.testing.assert_array_equal(r, want)
    # the rule as Scene.adaptive applies it: n_p becomes k for the retiring pixels
    counts = np.full((ny, nx), 100, np.uint32)
    counts[r] = 16
    assert (counts[0, 1:] == 16).all() and (counts[1] == 100).all() and counts[0, 0] == 100
    # infinite estimates (fewer than 2 samples) never retire
    assert not noise.retire(active, 16, np.full((ny, nx, 3), np.inf), 0, 1e9).any()


def test_counts_on_the_oracle_backend_raises(pkg, oracle):
    b = oracle.builder()
    world, cam, _ = pkg.scenes.random_scene(b, 8, 8)
    so = b.scene(world)
    with pytest.raises(ValueError, match="SAMPLE_COUNTS"):
        so.par_cast(cam, 8, 8, 2, counts=np.full((8, 8), 2, np.uint32))
    with pytest.raises(ValueError, match="SAMPLE_COUNTS"):
        so.par_cast_device(cam, pkg.capi.make_params(8, 8, 2), 0, counts=True)
    with pytest.raises(ValueError, match="SUM_SQUARES|SAMPLE_COUNTS"):
        next(so.adaptive(cam, 8, 8, 4, 2, 0.1))


def test_counts_must_match_the_frame(pkg):
    """A count array of the wrong shape is refused on the host, before the library is called."""
    capi = pkg.capi

    class _NoLib(capi.Scene):
        def __init__(self):
            self.be = type("B", (), {"prefix": "rtg_", "path": "-"})()
    with pytest.raises(ValueError, match="shape"):
        _NoLib().par_cast(capi.Camera(), 8, 8, 4, counts=np.zeros((8, 4), np.uint32))
    with pytest.raises(ValueError, match="step"):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 0, 0.1))
