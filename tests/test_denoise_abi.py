"""Denoising from the noise estimates, CPU side: RTG_FLAG_DENOISE and rtg_denoise in the header, the ctypes binding, the Rust
`-sys` crate and the C++ header; the denoise frame's layout; denoise.nlm against a brute-force per-pixel loop written from the
header's prose; what the filter buys on the oracle's renders; the Python refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import assert_bit_equal, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu.h")
SYS_RS = os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "lib.rs")
FIELDS = ["k", "radius", "patch", "reserved_in", "filtered", "passed", "reserved"]
f32 = np.float32


def test_header_declares_the_flag_and_the_block():
    text = open(HEADER).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RTG_FLAG_[A-Z_]+) (\d+)u", text)}
    assert flags["RTG_FLAG_DENOISE"] == 128
    assert sum(1 for v in flags.values() if v & 128) == 1
    assert re.search(r"#define RTG_DENOISE_MAX_RADIUS 8u", text) and re.search(r"#define RTG_DENOISE_MAX_PATCH 3u", text)
    nc = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct rtg_denoise \{(.*?)\} rtg_denoise;", nc, flags=re.S).group(1)
    names = [re.findall(r"([a-z_0-9]+)(?:\[\d+\])?$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert names == FIELDS
    assert "rtg_denoise(" not in nc.replace(" ", "")   # no new entry point


def test_ctypes_denoise_matches_the_compiled_header(pkg, tmp_path):
    capi = pkg.capi
    assert capi.FLAG_DENOISE == 128 and capi.DENOISE_MAX_RADIUS == 8 and capi.DENOISE_MAX_PATCH == 3
    assert [f for f, _ in capi.Denoise._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtiow_gpu.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(rtg_denoise));\n' +
                   "".join('  printf("%%zu\\n", offsetof(rtg_denoise, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(capi.Denoise) == 64
    assert got[1:] == [getattr(capi.Denoise, f).offset for f in FIELDS]
    assert capi.Denoise.OUT_OFFSET == capi.Denoise.filtered.offset == 16
    p = capi.make_params(8, 8, 4, squares=True, denoise=True)
    assert p.flags == capi.FLAG_SUM_SQUARES | capi.FLAG_DENOISE
    d = capi.make_denoise({"k": 0.5, "radius": 3})
    assert (d.k, d.radius, d.patch, d.reserved_in) == (np.float32(0.5), 3, 2, 0) and d.as_dict() == {"filtered": 0, "passed": 0}
    with pytest.raises(ValueError):
        capi.make_denoise({"strength": 1.0})


def test_rust_and_cpp_declare_the_block():
    rs = re.sub(r"//[^\n]*", "", open(SYS_RS).read())
    assert re.search(r"pub const RTG_FLAG_DENOISE: u32 = 128;", rs)
    assert re.search(r"pub const RTG_DENOISE_MAX_RADIUS: u32 = 8;", rs) and re.search(r"pub const RTG_DENOISE_MAX_PATCH: u32 = 3;", rs)
    body = re.search(r"#\[repr\(C\)\][^{]*pub struct rtg_denoise \{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+):", body) == FIELDS
    assert not re.search(r"pub fn rtg_denoise", rs)
    hpp = open(os.path.join(ROOT, "rtiow-rust_amd", "host", "rtiow.hpp")).read()
    assert "RTG_FLAG_DENOISE" in hpp and "par_cast_denoised" in hpp and "rtg_denoise" in hpp
    safe = open(os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu", "src", "lib.rs")).read()
    assert "pub fn par_cast_denoised" in safe and "RTG_FLAG_DENOISE" in safe


@pytest.mark.parametrize("counts,retire", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("nx,ny", [(7, 5), (8, 4), (1, 1), (37, 29)])
def test_denoise_frame_layout(pkg, nx, ny, counts, retire):
    capi = pkg.capi
    n = nx * ny
    off = capi.denoise_block_offset(nx, ny, counts, retire)
    if retire:
        want = 4 * (7 * n + (7 * n) % 2) + 64
    elif counts:
        want = 4 * (7 * n + (7 * n) % 2)
    else:
        want = 4 * (6 * n + (6 * n) % 2)
    assert off % 8 == 0 and off == want
    assert capi.denoise_frame_bytes(nx, ny, counts, retire) == off + 64 + 12 * n
    f = capi.denoise_frame(nx, ny, counts, retire, {"k": 1.5, "radius": 4, "patch": 1})
    base = f.buf.ctypes.data
    assert f.buf.nbytes == capi.denoise_frame_bytes(nx, ny, counts, retire)
    assert f.planes.shape == (2, ny, nx, 3) and f.planes.ctypes.data == base
    if counts:
        assert f.counts.shape == (ny, nx) and f.counts.dtype == np.uint32 and f.counts.ctypes.data == base + 24 * n
    else:
        assert f.counts is None
    if retire:
        assert C.addressof(f.retire) == base + capi.retire_block_offset(nx, ny)
    else:
        assert f.retire is None
    assert C.addressof(f.denoise) == base + off
    assert f.denoised.shape == (ny, nx, 3) and f.denoised.dtype == np.float32 and f.denoised.ctypes.data == base + off + 64
    words = f.buf.view(np.uint32)
    assert words[off // 4] == np.float32(1.5).view(np.uint32) and tuple(words[off // 4 + 1:off // 4 + 4]) == (4, 1, 0)
    f.denoise.filtered = 0xdeadbeef
    f.denoised[-1, -1, 2] = 2.5
    assert words[off // 4 + 4] == 0xdeadbeef and f.buf[-1] == 2.5
    assert not isinstance(f, capi.CountsFrame)   # a sibling: its count plane is optional


def _brute(pkg, S, Q, e, R, F, k):
    """The filter, pixel by pixel, from the prose of include/rtiow_gpu.h; every operation rounded to float32 on its own."""
    ny, nx = e.shape
    m, v, valid = np.zeros((ny, nx, 3), f32), np.zeros((ny, nx, 3), f32), np.zeros((ny, nx), bool)
    with np.errstate(all="ignore"):
        for y in range(ny):
            for x in range(nx):   # per pixel and channel, from the prose: m = S / e, d = Q - S * m clamped, v = d / (e * (e - 1))
                held = int(e[y, x])
                ef = f32(held if held >= 1 else 1)
                ok = held >= 2
                for c in range(3):
                    m[y, x, c] = f32(f32(S[y, x, c]) / ef)
                    d = f32(f32(Q[y, x, c]) - f32(f32(S[y, x, c]) * m[y, x, c]))
                    d = d if d > 0 else f32(0)   # negative or NaN becomes 0
                    vc = f32(d / f32(ef * f32(ef - f32(1))))
                    ok = ok and bool(np.isfinite(m[y, x, c])) and bool(np.isfinite(vc))
                    v[y, x, c] = vc
                valid[y, x] = ok
                if not ok:
                    v[y, x] = 0
    k2 = f32(k) * f32(k)
    eps = f32(1e-10)
    out = m.copy()

    def pd(ay, ax, by, bx):
        if not (0 <= ay < ny and 0 <= ax < nx and 0 <= by < ny and 0 <= bx < nx) or not (valid[ay, ax] and valid[by, bx]):
            return None
        d2 = []
        for c in range(3):
            diff = f32(m[ay, ax, c] - m[by, bx, c])
            num = f32(f32(diff * diff) - f32(v[ay, ax, c] + min(v[by, bx, c], v[ay, ax, c])))
            den = f32(eps + f32(k2 * f32(v[ay, ax, c] + v[by, bx, c])))
            d2.append(f32(num / den))
        return f32(f32(d2[0] + d2[1]) + d2[2])
    with np.errstate(all="ignore"):
        for y in range(ny):
            for x in range(nx):
                if not valid[y, x]:
                    continue
                acc, ws = [f32(0)] * 3, f32(0)
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
                        for c in range(3):
                            acc[c] = f32(acc[c] + f32(w * m[qy, qx, c]))
                        ws = f32(ws + w)
                for c in range(3):
                    out[y, x, c] = f32(acc[c] / ws)
    return out


def random_sums(ny, nx, seed, max_count=11, plant=True):
    """Running sums of up to `max_count` random samples per pixel (counts 0 .. max_count), the upper half of the frame ten times
    darker, NaN and inf planted in S and Q."""
    rs = np.random.RandomState(seed)
    e = rs.randint(0, max_count + 1, size=(ny, nx)).astype(np.uint32)
    c = rs.rand(max_count + 1, ny, nx, 3).astype(f32) * f32(2)
    c[:, :ny // 2] *= f32(0.1)
    S, Q = np.zeros((ny, nx, 3), f32), np.zeros((ny, nx, 3), f32)
    for s in range(max_count + 1):
        on = (s < e)[..., None]
        S, Q = np.where(on, S + c[s], S), np.where(on, Q + c[s] * c[s], Q)
    if plant and ny > 3 and nx > 2:
        S[2, 1, 0], S[3, 2, 1], Q[1, 1, 2] = np.nan, np.inf, np.inf
        e[2, 1] = e[3, 2] = e[1, 1] = 5
    elif plant:
        S[0, nx // 2, 1] = np.nan
        e[0, nx // 2] = 4
    return S.astype(f32), Q.astype(f32), e


@pytest.mark.parametrize("shape,R,F", [((9, 13), 2, 1), ((7, 5), 3, 2), ((1, 6), 2, 1), ((12, 10), 8, 3), ((9, 13), 0, 0),
                                       ((7, 5), 2, 0), ((12, 10), 3, 2), ((1, 6), 8, 3)])
def test_nlm_against_brute_force(pkg, shape, R, F):
    ny, nx = shape
    S, Q, e = random_sums(ny, nx, 100 * ny + nx + R)
    m, v, valid = pkg.denoise.mean_var(S, Q, e)
    assert valid.any() and (~valid).any()
    for k in (0.7, 2.0):
        got = pkg.denoise.nlm(S, Q, e, R, F, k)
        assert got.dtype == np.float32
        assert_bit_equal(got, _brute(pkg, S, Q, e, R, F, k), "nlm %s R %d F %d k %g" % (shape, R, F, k))
        assert not np.isnan(got[valid]).any()   # planted NaNs stay where they are
        assert_bit_equal(got[~valid], m[~valid], "pixels that take no part keep their mean")
    if R == 0:
        assert_bit_equal(pkg.denoise.nlm(S, Q, e, 0, F, 0.7), m, "radius 0 returns the means")
    assert (bits(pkg.denoise.nlm(S, Q, e, 0, 3, 0.3)) == bits(m))[valid].all()


def test_flat_regions_keep_their_edge(pkg):
    """Every sample of a pixel equal (v = 0): the two flat regions come back bit for bit, weights across the edge are 0."""
    ny, nx, n = 12, 16, 6
    val = np.where(np.arange(nx)[None, :, None] < 7, f32(0.25), f32(0.75)) * np.ones((ny, nx, 3), f32)
    val[..., 1] *= f32(0.5)
    S, Q = np.zeros_like(val), np.zeros_like(val)
    for _ in range(n):
        S, Q = S + val, Q + val * val
    e = np.full((ny, nx), n, np.uint32)
    m, v, valid = pkg.denoise.mean_var(S, Q, e)
    assert valid.all() and (v == 0).all()
    for R, F in ((5, 2), (8, 3), (2, 0)):
        assert_bit_equal(pkg.denoise.nlm(S, Q, e, R, F, 0.7), m, "flat regions R %d F %d" % (R, F))
    assert_bit_equal(pkg.denoise.denoise(np.stack([S, Q]), n), m, "denoise() of planes and one count")


def _oracle_sums(so, cam, nx, ny, ns):
    """(S, Q) as numpy folds them in float32 from the oracle's colour of every sample, in sample order, from +0."""
    rows, xs = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    n = nx * ny
    rgb, _ = so.debug_samples(cam, nx, ny, ns, np.tile(xs.ravel(), ns), np.tile((ny - 1 - rows).ravel(), ns),
                              np.repeat(np.arange(ns), n))
    c = rgb.reshape(ns, ny, nx, 3)
    S, Q = np.zeros((ny, nx, 3), f32), np.zeros((ny, nx, 3), f32)
    for s in range(ns):
        S, Q = S + c[s], Q + c[s] * c[s]
    return S, Q


@pytest.mark.parametrize("scene,nx,ny,ns,ref_ns,bound", [("random_scene", 192, 128, 8, 512, 0.80),
                                                         ("cornell_box_scene", 96, 96, 32, 2048, 0.55)])
def test_filter_lowers_the_true_error(pkg, oracle, scene, nx, ny, ns, ref_ns, bound):
    """RMSE against a high-sample render with another seed: filtered / plain at the defaults (5, 2, 0.7).  The bounds are the
    issue's (measured with this reference on these oracle renders: 0.694 and 0.458)."""
    b = oracle.builder()
    world, cam, _ = getattr(pkg.scenes, scene)(b, nx, ny)
    so = b.scene(world)
    S, Q = _oracle_sums(so, cam, nx, ny, ns)
    ref = so.par_cast(cam, nx, ny, ref_ns, seed=12345).astype(np.float64)
    plain = (S / f32(ns)).astype(np.float64)
    filt = pkg.denoise.nlm(S, Q, np.full((ny, nx), ns, np.uint32)).astype(np.float64)
    rmse_plain, rmse_filt = np.sqrt(np.mean((plain - ref) ** 2)), np.sqrt(np.mean((filt - ref) ** 2))
    print("%s %dx%dx%d: RMSE plain %.5f filtered %.5f ratio %.3f" % (scene, nx, ny, ns, rmse_plain, rmse_filt, rmse_filt / rmse_plain))
    assert rmse_filt / rmse_plain <= bound, (rmse_plain, rmse_filt)


def test_denoise_on_the_oracle_backend_raises(pkg, oracle):
    b = oracle.builder()
    world, cam, _ = pkg.scenes.random_scene(b, 8, 8)
    so = b.scene(world)
    with pytest.raises(ValueError, match="SUM_SQUARES|DENOISE"):
        so.par_cast(cam, 8, 8, 2, squares=True, denoise=True)
    with pytest.raises(ValueError, match="DENOISE"):
        so.par_cast_device(cam, pkg.capi.make_params(8, 8, 2, squares=True), 0, denoise=True)
    with pytest.raises(ValueError, match="SUM_SQUARES|DENOISE"):
        next(so.progressive(cam, 8, 8, 4, 2, denoise=True))
    with pytest.raises(ValueError, match="SUM_SQUARES|SAMPLE_COUNTS|DENOISE"):
        next(so.adaptive(cam, 8, 8, 4, 2, 0.1, denoise=True))


def test_validation_before_any_library_call(pkg):
    capi = pkg.capi

    class _NoLib(capi.Scene):
        def __init__(self):
            self.be = type("B", (), {"prefix": "rtg_", "path": "-"})()
    with pytest.raises(ValueError, match="squares=True"):
        _NoLib().par_cast(capi.Camera(), 8, 8, 4, denoise=True)
    with pytest.raises(ValueError, match="squares=True"):
        _NoLib().par_cast(capi.Camera(), 8, 8, 4, denoise=capi.Denoise(), out=capi.denoise_frame(8, 8))
    # the existing arguments are checked first, in the order they were
    with pytest.raises(ValueError, match="step"):
        next(_NoLib().progressive(capi.Camera(), 8, 8, 4, 0, denoise={"bad": 1}))
    with pytest.raises(ValueError, match="step"):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 0, 0.1, out=1 << 20, preview=1 << 21, radius=99, denoise=True))
    with pytest.raises(ValueError, match="radius"):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 2, 0.1, radius=9, denoise=True))
    with pytest.raises(ValueError, match="preview"):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 2, 0.1, out=1 << 20, denoise=True))
    with pytest.raises(ValueError, match="denoised="):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 2, 0.1, out=1 << 20, preview=1 << 21, denoise=True))
    with pytest.raises(ValueError, match="preview"):
        next(_NoLib().progressive(capi.Camera(), 8, 8, 4, 2, out=1 << 20, denoise=True))
    with pytest.raises(ValueError, match="denoised="):
        next(_NoLib().progressive(capi.Camera(), 8, 8, 4, 2, out=1 << 20, preview=1 << 21, denoise=True))
    with pytest.raises(ValueError, match="unknown key"):
        next(_NoLib().progressive(capi.Camera(), 8, 8, 4, 2, denoise={"bad": 1}))
    with pytest.raises(ValueError, match="DenoiseFrame"):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 2, 0.1, out=capi.counts_frame(8, 8, squares=True), denoise=True))
