"""The error plane of the filtered frame, CPU side: RTG_FLAG_DENOISE_ERROR in the header and its mirrors; the frame layout with
the plane at the old end; denoise.nlm_error / nlm_guided_error against a brute-force per-pixel loop written from the header's
prose; noise.retire_filtered against a brute-force loop; how the estimate compares with the true error of the filtered frame on
the oracle's renders; the Python refusals."""
import itertools
import os
import re

import numpy as np
import pytest

from conftest import assert_bit_equal, bits
from test_denoise_abi import _oracle_sums, random_sums
from test_features_abi import _feature_weight_brute, random_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu.h")
HOST = os.path.join(ROOT, "rtiow-rust_amd", "host")
f32 = np.float32
INF_BITS = 0x7F800000


def test_header_and_mirrors_declare_the_flag(pkg):
    text = open(HEADER).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RTG_FLAG_[A-Z_]+) (\d+)u", text)}
    assert flags["RTG_FLAG_DENOISE_ERROR"] == 512
    assert sum(1 for v in flags.values() if v & 512) == 1
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values())
    nc = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "rtg_denoise_error" not in nc and "rtg_error" not in nc   # no new block, no new entry point
    capi = pkg.capi
    assert capi.FLAG_DENOISE_ERROR == 512
    p = capi.make_params(8, 8, 4, squares=True, denoise=True, error=True)
    assert p.flags == capi.FLAG_SUM_SQUARES | capi.FLAG_DENOISE | capi.FLAG_DENOISE_ERROR
    assert capi.make_params(8, 8, 4, squares=True, denoise=True).flags == capi.FLAG_SUM_SQUARES | capi.FLAG_DENOISE
    rs = re.sub(r"//[^\n]*", "", open(os.path.join(HOST, "rust", "rtiow-gpu-sys", "src", "lib.rs")).read())
    assert re.search(r"pub const RTG_FLAG_DENOISE_ERROR: u32 = 512;", rs)
    safe = open(os.path.join(HOST, "rust", "rtiow-gpu", "src", "lib.rs")).read()
    assert "RTG_FLAG_DENOISE_ERROR" in safe and "denoise_error" in safe
    hpp = open(os.path.join(HOST, "rtiow.hpp")).read()
    assert "RTG_FLAG_DENOISE_ERROR" in hpp and "denoise_error" in hpp


COMBOS = [c for c in itertools.product((False, True), repeat=5)]   # squares, counts, retire, denoise, features


@pytest.mark.parametrize("nx,ny", [(7, 5), (8, 4), (1, 1), (37, 29)])
def test_layout_puts_the_plane_at_the_old_end(pkg, nx, ny):
    capi = pkg.capi
    n = nx * ny
    parts = ("counts", "retire", "denoise", "denoised", "features", "albedo", "normal", "depth")
    for squares, counts, retire, denoise, features in COMBOS:
        old = capi.FrameLayout(nx, ny, squares, counts, retire, denoise, features)
        assert old.error is None
        if not denoise:
            with pytest.raises(ValueError, match="denoise"):
                capi.FrameLayout(nx, ny, squares, counts, retire, denoise, features, error=True)
            continue
        new = capi.FrameLayout(nx, ny, squares, counts, retire, denoise, features, error=True)
        for part in parts + ("squares",):
            assert getattr(new, part) == getattr(old, part), (part, squares, counts, retire, features)
        assert new.error == (old.words + 1) & ~1 and new.error % 2 == 0
        assert new.words == new.error + 3 * n
        # ... the old end is behind the output plane or, with features, behind the depth plane
        assert old.words == (old.depth + n if features else old.denoised + 3 * n)
    f = capi.denoise_frame(nx, ny, True, True, error=True)
    assert f.error.shape == (ny, nx, 3) and f.error.dtype == np.float32
    assert f.error.ctypes.data == f.buf.ctypes.data + 4 * f.layout.error and f.buf.nbytes == 4 * f.layout.words
    assert f.buf.nbytes == capi.denoise_frame_bytes(nx, ny, True, True, error=True)
    assert f.flags() == {"squares": True, "counts": True, "retire": True, "denoise": True, "features": False, "error": True}
    g = capi.features_frame(nx, ny, denoise=True, error=True)
    assert g.error.ctypes.data == g.depth.ctypes.data + 4 * (n + n % 2)
    assert g.buf.nbytes == capi.features_frame_bytes(nx, ny, True, False, False, True, error=True)
    # a frame without the part: exactly the five keys of before
    assert capi.denoise_frame(nx, ny).error is None
    assert capi.denoise_frame(nx, ny).flags() == {"squares": True, "counts": False, "retire": False, "denoise": True, "features": False}


def _brute_error(pkg, S, Q, e, R, F, k, guide=None):
    """(out, ev) pixel by pixel from the prose of include/rtiow_gpu.h: the filter's loop with one more accumulator per channel,
    acc2 = acc2 + (w * w) * v_q after the pair's final weight; ev = (acc2 / wsum) / wsum; +inf where a pixel is not valid."""
    ny, nx = e.shape
    m, v, valid = pkg.denoise.mean_var(S, Q, e)   # (checked against the prose by test_denoise_abi)
    k2, eps = f32(k) * f32(k), f32(1e-10)
    out, ev = m.copy(), np.full((ny, nx, 3), np.inf, f32)
    cache = {}

    def pd(ay, ax, by, bx):
        key = (ay, ax, by, bx)
        if key not in cache:
            t = None
            if 0 <= ay < ny and 0 <= ax < nx and 0 <= by < ny and 0 <= bx < nx and valid[ay, ax] and valid[by, bx]:
                d2 = []
                for c in range(3):
                    diff = f32(m[ay, ax, c] - m[by, bx, c])
                    num = f32(f32(diff * diff) - f32(v[ay, ax, c] + min(v[by, bx, c], v[ay, ax, c])))
                    den = f32(eps + f32(k2 * f32(v[ay, ax, c] + v[by, bx, c])))
                    d2.append(f32(num / den))
                t = f32(f32(d2[0] + d2[1]) + d2[2])
            cache[key] = t
        return cache[key]
    with np.errstate(all="ignore"):
        for y in range(ny):
            for x in range(nx):
                if not valid[y, x]:
                    continue
                acc, acc2, ws = [f32(0)] * 3, [f32(0)] * 3, f32(0)
                for dy in range(-R, R + 1):
                    for dx in range(-R, R + 1):
                        qy, qx = y + dy, x + dx
                        if not (0 <= qy < ny and 0 <= qx < nx and valid[qy, qx]):
                            continue   # w = 0
                        D, cnt = f32(0), 0
                        for oy in range(-F, F + 1):
                            r = f32(0)
                            for ox in range(-F, F + 1):
                                t = pd(y + oy, x + ox, qy + oy, qx + ox)
                                if t is not None:
                                    r, cnt = f32(r + t), cnt + 1
                            D = f32(D + r)
                        xx = f32(D / f32(f32(3) * f32(cnt)))
                        xx = xx if xx > 0 else f32(0)
                        u = f32(f32(1) - f32(xx * f32(0.25)))
                        u = u if u > 0 else f32(0)
                        u2 = f32(u * u)
                        w = f32(u2 * u2)
                        if guide is not None:
                            wf = _feature_weight_brute(guide[0], guide[1], guide[2], (y, x), (qy, qx), *guide[3:])
                            w = wf if wf < w else w
                        w2 = f32(w * w)
                        for c in range(3):
                            acc[c] = f32(acc[c] + f32(w * m[qy, qx, c]))
                            acc2[c] = f32(acc2[c] + f32(w2 * v[qy, qx, c]))
                        ws = f32(ws + w)
                for c in range(3):
                    out[y, x, c] = f32(acc[c] / ws)
                    ev[y, x, c] = f32(f32(acc2[c] / ws) / ws)
    return out, ev


@pytest.mark.parametrize("shape", [(5, 7), (1, 1), (9, 13)])
@pytest.mark.parametrize("R,F", [(0, 0), (1, 0), (3, 1)])
def test_nlm_error_against_brute_force(pkg, shape, R, F):
    ny, nx = shape
    dn = pkg.denoise
    S, Q, e = random_sums(ny, nx, 100 * ny + nx + R)
    a, n, z = random_features(ny, nx, 7 * ny + nx + F)
    sig = (0.3, 0.2, 0.1)
    m, v, valid = dn.mean_var(S, Q, e)
    for k in (0.7, 2.0):
        what = "%s R %d F %d k %g" % (shape, R, F, k)
        out, ev = dn.nlm_error(S, Q, e, R, F, k)
        assert out.dtype == ev.dtype == np.float32 and ev.shape == (ny, nx, 3)
        want_out, want_ev = _brute_error(pkg, S, Q, e, R, F, k)
        assert_bit_equal(out, want_out, "nlm_error out " + what)
        assert_bit_equal(ev, want_ev, "nlm_error ev " + what)
        assert_bit_equal(out, dn.nlm(S, Q, e, R, F, k), "nlm_error out is nlm " + what)
        assert (bits(ev)[~valid] == INF_BITS).all() and np.isfinite(ev[valid]).all() and (ev[valid] >= 0).all()
        if R == 0:
            assert_bit_equal(ev[valid], v[valid], "radius 0: the error is the variance of the mean " + what)
        gout, gev = dn.nlm_guided_error(S, Q, e, a, n, z, R, F, k, *sig)
        want_out, want_ev = _brute_error(pkg, S, Q, e, R, F, k, (a, n, z) + sig)
        assert_bit_equal(gout, want_out, "nlm_guided_error out " + what)
        assert_bit_equal(gev, want_ev, "nlm_guided_error ev " + what)
        assert_bit_equal(gout, dn.nlm_guided(S, Q, e, a, n, z, R, F, k, *sig), "nlm_guided_error out is nlm_guided " + what)
        assert (bits(gev)[~valid] == INF_BITS).all()
    off = dn.nlm_guided_error(S, Q, e, a, n, z, R, F, 0.7, 1e18, 1e18, 1e18)[1]
    assert_bit_equal(off, dn.nlm_error(S, Q, e, R, F, 0.7)[1], "sigmas 1e18 %s" % (shape,))


def _retire_brute(active, k, ev, counts, min_samples, target_se, radius):
    ny, nx = counts.shape
    t2 = float(target_se) * float(target_se)
    out = np.zeros((ny, nx), bool)
    for y in range(ny):
        for x in range(nx):
            if not active[y, x] or k < min_samples:
                continue
            ok = True
            for qy in range(max(0, y - radius), min(ny, y + radius + 1)):
                for qx in range(max(0, x - radius), min(nx, x + radius + 1)):
                    if counts[qy, qx] == 0:
                        continue   # not part of the frame
                    for c in range(3):
                        val = float(ev[qy, qx, c])
                        ok = ok and np.isfinite(val) and val <= t2
            out[y, x] = ok
    return out


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("shape", [(9, 13), (1, 1), (6, 5)])
def test_retire_filtered_against_brute_force(pkg, shape, radius):
    ny, nx = shape
    rs = np.random.RandomState(31 * ny + nx + radius)
    target = 0.25
    ev = (rs.rand(ny, nx, 3) * 0.09).astype(f32)   # about two thirds of the values below target^2 = 0.0625
    ev[rs.rand(ny, nx) < 0.1] = np.inf
    ev[rs.rand(ny, nx) < 0.05, 1] = np.nan
    ev[rs.rand(ny, nx) < 0.1] = f32(0.0625)       # ties: exactly target^2 is OK
    counts = rs.randint(0, 12, size=(ny, nx)).astype(np.uint32)
    counts[rs.rand(ny, nx) < 0.2] = 0              # holes
    active = rs.rand(ny, nx) < 0.8
    for k, min_samples in ((8, 4), (3, 4)):
        got = pkg.noise.retire_filtered(active, k, ev, counts, min_samples, target, radius=radius)
        want = _retire_brute(active, k, ev, counts, min_samples, target, radius)
        assert got.dtype == bool and (got == want).all(), (shape, radius, k)
    # one ulp above the tie is not OK
    one = np.full((1, 1, 3), f32(0.0625), f32)
    on, n1 = np.ones((1, 1), bool), np.ones((1, 1), np.uint32)
    assert pkg.noise.retire_filtered(on, 4, one, n1, 2, 0.25).all()
    one[0, 0, 2] = np.nextafter(f32(0.0625), f32(1))
    assert not pkg.noise.retire_filtered(on, 4, one, n1, 2, 0.25).any()
    est, s2 = pkg.noise.filtered_estimate(ev, counts)
    fin = np.isfinite(ev).all(axis=-1) & (counts > 0)
    assert est == int(fin.sum()) and np.isclose(s2, ev[fin].astype(np.float64).sum(), rtol=1e-12)


@pytest.mark.parametrize("scene,nx,ny,ns,ref_ns,lo,hi", [("cornell_box_scene", 96, 96, 32, 2048, 0.9, 1.8),
                                                         ("random_scene", 192, 128, 8, 512, 0.9, 1.4)])
def test_estimate_against_the_true_error_of_the_filtered_frame(pkg, oracle, scene, nx, ny, ns, ref_ns, lo, hi):
    """True RMSE of the filtered frame against a high-sample render with another seed, over sqrt(mean ev), at the defaults
    (5, 2, 0.7) on the oracle's renders of test_denoise_abi.test_filter_lowers_the_true_error.  The estimate ignores the filter's
    bias, so the ratio lies above 1; the bounds are the issue's (it measured 1.485 and 1.154)."""
    b = oracle.builder()
    world, cam, _ = getattr(pkg.scenes, scene)(b, nx, ny)
    so = b.scene(world)
    S, Q = _oracle_sums(so, cam, nx, ny, ns)
    ref = so.par_cast(cam, nx, ny, ref_ns, seed=12345).astype(np.float64)
    e = np.full((ny, nx), ns, np.uint32)
    out, ev = pkg.denoise.nlm_error(S, Q, e)
    assert_bit_equal(out, pkg.denoise.nlm(S, Q, e), scene + ": out is nlm")
    fin = np.isfinite(ev).all(axis=-1)
    assert fin.all()
    true = np.sqrt(np.mean((out.astype(np.float64) - ref) ** 2))
    est = np.sqrt(np.mean(ev.astype(np.float64)))
    print("%s %dx%dx%d: filtered true RMSE %.5f estimated %.5f ratio %.3f" % (scene, nx, ny, ns, true, est, true / est))
    assert lo <= true / est <= hi, (true, est)


def test_error_on_the_oracle_backend_raises(pkg, oracle):
    """Every way in names the new flag: its refusal comes before those of the flags the oracle lacks as well."""
    b = oracle.builder()
    world, cam, _ = pkg.scenes.random_scene(b, 8, 8)
    so = b.scene(world)
    with pytest.raises(ValueError, match="DENOISE_ERROR"):
        so.par_cast(cam, 8, 8, 2, squares=True, denoise=True, error=True)
    with pytest.raises(ValueError, match="DENOISE_ERROR"):
        so.par_cast(cam, 8, 8, 2, out=pkg.capi.denoise_frame(8, 8, error=True), squares=True, denoise=True, error=True)
    with pytest.raises(ValueError, match="DENOISE_ERROR"):
        so.par_cast_device(cam, pkg.capi.make_params(8, 8, 2, squares=True, denoise=True), 0, error=True)
    with pytest.raises(ValueError, match="DENOISE_ERROR"):
        next(so.adaptive(cam, 8, 8, 4, 2, 0.1, denoise=True, filtered_error=True))
    with pytest.raises(ValueError, match="DENOISE_ERROR"):
        oracle.par_cast_multi([so], cam, 8, 8, 2, out=pkg.capi.denoise_frame(8, 8, error=True), denoise=True, squares=True, error=True)
    with pytest.raises(ValueError, match="DENOISE_ERROR"):
        oracle.par_cast_multi([so], cam, 8, 8, 2, squares=True, denoise=True, error=True)   # (plain flags, forwarded)
    with pytest.raises(ValueError, match="DENOISE_ERROR"):
        next(oracle.adaptive_multi([so], cam, 8, 8, 4, 2, 0.1, denoise=True, filtered_error=True))
    # without error= the refusals are the earlier ones
    with pytest.raises(ValueError, match="SUM_SQUARES"):
        so.par_cast(cam, 8, 8, 2, squares=True, denoise=True)


def test_validation_before_any_library_call(pkg):
    capi = pkg.capi

    class _NoLib(capi.Scene):
        def __init__(self):
            self.be = type("B", (), {"prefix": "rtg_", "path": "-"})()
    with pytest.raises(ValueError, match="error=True needs denoise"):
        _NoLib().par_cast(capi.Camera(), 8, 8, 4, squares=True, error=True)
    with pytest.raises(ValueError, match="error=True needs"):
        _NoLib().par_cast_device(capi.Camera(), capi.make_params(8, 8, 4, squares=True), 0, error=True)
    with pytest.raises(ValueError, match="error="):
        _NoLib().par_cast(capi.Camera(), 8, 8, 4, squares=True, denoise=True, error=True, out=capi.denoise_frame(8, 8))
    with pytest.raises(ValueError, match="error="):
        _NoLib().par_cast(capi.Camera(), 8, 8, 4, squares=True, denoise=True, out=capi.denoise_frame(8, 8, error=True))
    with pytest.raises(ValueError, match="filtered_error=True needs denoise"):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 2, 0.1, filtered_error=True))
    with pytest.raises(ValueError, match="step"):   # the existing arguments are checked first
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 0, 0.1, filtered_error=True))
    with pytest.raises(ValueError, match="error=True"):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 2, 0.1, denoise=True, filtered_error=True, out=capi.denoise_frame(8, 8, True)))
    with pytest.raises(ValueError, match="denoise"):
        capi.FrameLayout(8, 8, True, error=True)
