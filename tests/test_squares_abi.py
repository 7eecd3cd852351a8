"""Per-pixel noise estimates, CPU side: RTG_FLAG_SUM_SQUARES in the header, the ctypes binding and the Rust `-sys` crate, the ABI
structs and symbol list unchanged, noise.py against a direct float64 computation, and the oracle refusing squares=True."""
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
    assert flags["RTG_FLAG_SUM_SQUARES"] == 16
    others = 0
    for name, v in flags.items():
        assert v & (v - 1) == 0, (name, v)   # one bit each
        if name != "RTG_FLAG_SUM_SQUARES":
            others |= v
    assert not others & 16


def test_capi_and_rust_match_the_header(pkg):
    assert pkg.capi.FLAG_SUM_SQUARES == _header_flags()["RTG_FLAG_SUM_SQUARES"]
    rs = open(SYS_RS).read()
    assert re.search(r"pub const RTG_FLAG_SUM_SQUARES: u32 = 16;", rs)
    p = pkg.capi.make_params(8, 8, 4, squares=True, partial=True)
    assert p.flags == pkg.capi.FLAG_SUM_SQUARES | pkg.capi.FLAG_PARTIAL
    assert pkg.capi.make_params(8, 8, 4).flags == 0


def test_abi_sizes_and_symbols_unchanged(pkg):
    capi = pkg.capi
    assert C.sizeof(capi.Params) == 56 and C.sizeof(capi.Stats) == 56
    assert len(capi.ABI_SYMBOLS) == 42 and "par_cast" in capi.ABI_SYMBOLS
    declared = set(re.findall(r"\brtg_([a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    assert declared == set(capi.ABI_SYMBOLS), declared ^ set(capi.ABI_SYMBOLS)


def _direct(samples):
    """samples [n, ...] (float32): the float32 left folds the library computes, and the float64 standard error of the mean
    computed from the samples themselves."""
    s = np.zeros(samples.shape[1:], dtype=np.float32)
    q = np.zeros(samples.shape[1:], dtype=np.float32)
    for c in samples:
        s = s + c
        q = q + c * c
    n = samples.shape[0]
    x = samples.astype(np.float64)
    se = np.sqrt(x.var(axis=0, ddof=1) / n) if n > 1 else np.full(samples.shape[1:], np.inf)
    return s, q, se


def test_standard_error_against_a_direct_computation(pkg):
    noise = pkg.noise
    rs = np.random.RandomState(7)
    for n in (2, 5, 64):
        samples = (rs.gamma(0.5, 0.4, size=(n, 6, 5, 3))).astype(np.float32)
        s, q, se = _direct(samples)
        got = noise.standard_error(s, q, n)
        assert got.dtype == np.float64 and got.shape == s.shape
        np.testing.assert_allclose(got, se, rtol=2e-3, atol=1e-6)
        assert noise.estimated_rmse(s, q, n) == pytest.approx(float(np.sqrt(np.mean(se * se))), rel=2e-3)


def test_standard_error_edge_cases(pkg):
    noise = pkg.noise
    one = np.array([[0.25, 1.0, 3.0]], dtype=np.float32)
    assert np.isinf(noise.standard_error(one, one * one, 1)).all()
    assert np.isinf(noise.estimated_rmse(one, one * one, 1))
    # constant samples: zero variance
    c = np.full((4, 2, 2, 3), 0.3, dtype=np.float32)
    s, q, _ = _direct(c)
    assert (noise.standard_error(s, q, 4) == 0.0).all()
    # a sum of squares below n m^2 (what rounding can leave for near-constant samples): clamped to 0, not NaN
    s = np.array([3.0], dtype=np.float32)
    q = np.array([np.nextafter(np.float32(3.0), np.float32(0))], dtype=np.float32)   # 3 samples of 1.0 would give exactly 3
    assert (3.0 * (3.0 / 3) ** 2) > float(q[0])
    got = noise.standard_error(s, q, 3)
    assert got[0] == 0.0 and not np.isnan(got).any()
    with pytest.raises(ValueError):
        noise.standard_error(s, q, 0)


def test_squares_on_the_oracle_backend_raises(pkg, oracle):
    b = oracle.builder()
    world, cam, _ = pkg.scenes.random_scene(b, 8, 8)
    so = b.scene(world)
    with pytest.raises(ValueError, match="SUM_SQUARES"):
        so.par_cast(cam, 8, 8, 2, squares=True)
    with pytest.raises(ValueError, match="SUM_SQUARES"):
        next(so.progressive(cam, 8, 8, 2, 1, target_rmse=0.1))


def test_squares_out_must_have_two_planes(pkg):
    """The library writes two planes: a one-plane out= is refused on the host, before the library is called."""
    capi = pkg.capi

    class _NoLib(capi.Scene):
        def __init__(self):
            self.be = type("B", (), {"prefix": "rtg_", "path": "-"})()
    for out in (np.zeros((8, 8, 3), np.float32), np.zeros((2, 8, 8, 3), np.float64), np.zeros((2, 8, 4, 3), np.float32)):
        with pytest.raises(ValueError, match="shape"):
            _NoLib().par_cast(capi.Camera(), 8, 8, 4, out=out, squares=True)
