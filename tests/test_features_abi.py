"""Feature planes, CPU side: RTG_FLAG_FEATURES and rtg_features in the header, the ctypes binding, the Rust `-sys` crate and the
C++ header; where the features block lies for every flag combination; denoise.nlm_guided against a brute-force per-pixel loop
written from the header's prose; the reference planes on the oracle; what guiding buys on the oracle's renders; the Python
refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import assert_bit_equal
from feature_ref import build_recorded, reference_planes
from test_denoise_abi import _brute, _oracle_sums, random_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu.h")
SYS_RS = os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "lib.rs")
FIELDS = ["grid", "compute", "sigma_normal", "sigma_albedo", "sigma_depth", "reserved_in", "traced", "missed", "reserved"]
f32 = np.float32


def test_header_declares_the_flag_and_the_block():
    text = open(HEADER).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RTG_FLAG_[A-Z_]+) (\d+)u", text)}
    assert flags["RTG_FLAG_FEATURES"] == 256
    assert sum(1 for v in flags.values() if v & 256) == 1
    assert re.search(r"#define RTG_FEATURES_MAX_GRID 4u", text)
    nc = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct rtg_features \{(.*?)\} rtg_features;", nc, flags=re.S).group(1)
    names = [re.findall(r"([a-z_0-9]+)(?:\[\d+\])?$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert names == FIELDS
    assert "rtg_features(" not in nc.replace(" ", "")   # no new entry point
    # rtg_denoise keeps its fields
    body = re.search(r"typedef struct rtg_denoise \{(.*?)\} rtg_denoise;", nc, flags=re.S).group(1)
    assert [re.findall(r"([a-z_0-9]+)(?:\[\d+\])?$", d.strip())[0] for d in body.split(";") if d.strip()] == \
        ["k", "radius", "patch", "reserved_in", "filtered", "passed", "reserved"]


def test_ctypes_features_matches_the_compiled_header(pkg, tmp_path):
    capi = pkg.capi
    assert capi.FLAG_FEATURES == 256 and capi.FEATURES_MAX_GRID == 4 and pkg.features.MAX_GRID == 4
    assert [f for f, _ in capi.Features._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtiow_gpu.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(rtg_features));\n' +
                   "".join('  printf("%%zu\\n", offsetof(rtg_features, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(capi.Features) == 64
    assert got[1:] == [getattr(capi.Features, f).offset for f in FIELDS]
    assert capi.Features.OUT_OFFSET == capi.Features.traced.offset == 24
    p = capi.make_params(8, 8, 4, features=True)
    assert p.flags == capi.FLAG_FEATURES
    d = capi.make_features({"grid": 3, "sigma_depth": 2.0})
    assert (d.grid, d.compute, d.sigma_depth, d.reserved_in) == (3, 1, 2.0, 0) and d.as_dict() == {"traced": 0, "missed": 0}
    assert d.sigma_normal == np.float32(capi.FEATURES_DEFAULTS["sigma_normal"])
    with pytest.raises(ValueError):
        capi.make_features({"sigma": 1.0})


def test_rust_and_cpp_declare_the_block():
    rs = re.sub(r"//[^\n]*", "", open(SYS_RS).read())
    assert re.search(r"pub const RTG_FLAG_FEATURES: u32 = 256;", rs) and re.search(r"pub const RTG_FEATURES_MAX_GRID: u32 = 4;", rs)
    body = re.search(r"#\[repr\(C\)\][^{]*pub struct rtg_features \{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+):", body) == FIELDS
    assert not re.search(r"pub fn rtg_features", rs)
    hpp = open(os.path.join(ROOT, "rtiow-rust_amd", "host", "rtiow.hpp")).read()
    assert "RTG_FLAG_FEATURES" in hpp and "rtg_features" in hpp


def _prose_offset(n, squares, counts, retire, denoise):
    """The block's word from the header's prose: behind everything the other flags put in the frame, rounded up to even."""
    up = lambda w: w + (w & 1)
    end = (6 if squares else 3) * n
    if counts:
        end += n
    if retire:
        end = up(7 * n) + 16
    if denoise:
        end = up(end) + 16 + 3 * n
    return 4 * up(end)


COMBOS = [(sq, c, r, d) for sq in (False, True) for c in (False, True) for r in (False, True) for d in (False, True)
          if (not r or (c and sq)) and (not d or sq)]


@pytest.mark.parametrize("nx,ny", [(7, 5), (8, 4), (1, 1), (37, 29), (3, 3)])
def test_features_block_offset(pkg, nx, ny):
    capi = pkg.capi
    n = nx * ny
    assert len(COMBOS) == 8
    for squares, counts, retire, denoise in COMBOS:
        what = (nx, ny, squares, counts, retire, denoise)
        off = capi.features_block_offset(nx, ny, squares, counts, retire, denoise)
        assert off % 8 == 0 and off == _prose_offset(n, squares, counts, retire, denoise), what
        assert capi.features_frame_bytes(nx, ny, squares, counts, retire, denoise) == off + 64 + 28 * n
        f = capi.features_frame(nx, ny, squares, counts, retire, {"k": 1.5} if denoise else None, {"grid": 3, "sigma_albedo": 0.5})
        base = f.buf.ctypes.data
        assert f.buf.nbytes == off + 64 + 28 * n, what
        assert f.planes.shape == ((2, ny, nx, 3) if squares else (ny, nx, 3)) and f.planes.ctypes.data == base
        assert (f.counts is not None) == counts and (f.retire is not None) == retire and (f.denoise is not None) == denoise
        if counts:
            assert f.counts.ctypes.data == base + (24 if squares else 12) * n and f.counts.dtype == np.uint32
        if retire:
            assert C.addressof(f.retire) == base + capi.retire_block_offset(nx, ny)
        if denoise:
            d_off = capi.denoise_block_offset(nx, ny, counts, retire)
            assert C.addressof(f.denoise) == base + d_off and f.denoised.ctypes.data == base + d_off + 64
            assert f.denoised.ctypes.data + 12 * n <= base + off and f.denoise.k == 1.5
        assert C.addressof(f.features) == base + off
        assert f.albedo.shape == f.normal.shape == (ny, nx, 3) and f.depth.shape == (ny, nx)
        assert f.albedo.ctypes.data == base + off + 64 and f.normal.ctypes.data == base + off + 64 + 12 * n
        assert f.depth.ctypes.data == base + off + 64 + 24 * n
        words = f.buf.view(np.uint32)
        assert tuple(words[off // 4:off // 4 + 2]) == (3, 1) and words[off // 4 + 3] == np.float32(0.5).view(np.uint32)
        assert (words[off // 4 + 5:off // 4 + 16] == 0).all()
        f.features.missed = 0xdeadbeef
        f.depth[-1, -1] = 2.5
        assert words[off // 4 + 7] == 0xdeadbeef and f.buf[-1] == 2.5
        assert f.flags() == {"squares": squares, "counts": counts, "retire": retire, "denoise": denoise, "features": True}
    # frames larger than 2^31 bytes: the offsets are plain Python integers
    assert capi.features_block_offset(40000, 40000, True, True, True, True) == 4 * (7 * 1600000000 + 16 + 16 + 3 * 1600000000)


def _feature_weight_brute(a, n, z, p, q, sn, sa, sz):
    """wf of the pair (p, q) from the prose of include/rtiow_gpu.h; every operation rounded to float32 on its own."""
    vals = [a[p][c] for c in range(3)] + [n[p][c] for c in range(3)] + [z[p]] + [a[q][c] for c in range(3)] + \
        [n[q][c] for c in range(3)] + [z[q]]
    if not all(np.isfinite(v) for v in vals):
        return f32(1)

    def dist(u, v):
        d = [f32(u[c] - v[c]) for c in range(3)]
        return f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
    xn = f32(dist(n[p], n[q]) / f32(f32(sn) * f32(sn)))
    xa = f32(dist(a[p], a[q]) / f32(f32(sa) * f32(sa)))
    dz, s = f32(z[p] - z[q]), f32(z[p] + z[q])
    xz = f32(f32(f32(dz * dz) / f32(f32(s * s) + f32(1e-20))) / f32(f32(sz) * f32(sz)))
    x = xn
    x = xa if xa > x else x
    x = xz if xz > x else x
    u = f32(f32(1) - f32(x * f32(0.25)))
    u = u if u > 0 else f32(0)
    return f32(f32(u * u) * f32(u * u))


def _brute_guided(pkg, S, Q, e, a, n, z, R, F, k, sn, sa, sz):
    """test_denoise_abi._brute with the one change of the guided filter: w = wf < w ? wf : w."""
    ny, nx = e.shape
    m, v, valid = pkg.denoise.mean_var(S, Q, e)   # (checked against the prose by test_denoise_abi)
    k2, eps = f32(k) * f32(k), f32(1e-10)
    out = m.copy()

    cache = {}   # (a pair's distance serves every patch that holds it)

    def pd(ay, ax, by, bx):
        key = (ay, ax, by, bx)
        if key not in cache:
            cache[key] = pd_of(ay, ax, by, bx)
        return cache[key]

    def pd_of(ay, ax, by, bx):
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
                        wf = _feature_weight_brute(a, n, z, (y, x), (qy, qx), sn, sa, sz)
                        w = wf if wf < w else w
                        for c in range(3):
                            acc[c] = f32(acc[c] + f32(w * m[qy, qx, c]))
                        ws = f32(ws + w)
                for c in range(3):
                    out[y, x, c] = f32(acc[c] / ws)
    return out


def random_features(ny, nx, seed, plant=True):
    """Planted feature planes: piecewise-constant albedos and normals with noise, depths in a few layers -- zeros, equal
    depths, NaN and inf among them."""
    rs = np.random.RandomState(seed)
    a = (rs.randint(0, 3, size=(ny, nx, 1)) * f32(0.4) + rs.rand(ny, nx, 3) * f32(0.1)).astype(f32)
    n = rs.randn(ny, nx, 3).astype(f32)
    n = (n / np.sqrt((n * n).sum(axis=-1, keepdims=True))).astype(f32)
    n[rs.rand(ny, nx) < 0.4] = (0, 1, 0)
    z = (rs.randint(0, 4, size=(ny, nx)) * f32(2.5) + rs.rand(ny, nx) * f32(0.2)).astype(f32)
    z[rs.rand(ny, nx) < 0.2] = 5.0    # equal depths
    miss = rs.rand(ny, nx) < 0.15      # pixels that hit nothing: seven zeros
    a[miss], n[miss], z[miss] = 0, 0, 0
    if plant and ny > 4 and nx > 3:
        a[1, 2, 0], n[3, 1, 2], z[2, 3] = np.nan, np.inf, -np.inf
        z[4, 0], a[0, 3, 1] = np.nan, np.inf
    elif plant and nx > 1:
        z[0, nx // 2] = np.nan
    return a, n, z


@pytest.mark.parametrize("shape", [(9, 13), (1, 1), (3, 200), (12, 10)])
@pytest.mark.parametrize("R,F", [(0, 0), (1, 0), (5, 2), (8, 3)])
def test_nlm_guided_against_brute_force(pkg, shape, R, F):
    ny, nx = shape
    S, Q, e = random_sums(ny, nx, 100 * ny + nx + R)
    a, n, z = random_features(ny, nx, 7 * ny + nx + F)
    sig = (0.3, 0.2, 0.1)
    got = pkg.denoise.nlm_guided(S, Q, e, a, n, z, R, F, 1.5, *sig)
    assert got.dtype == np.float32 and got.shape == (ny, nx, 3)
    assert_bit_equal(got, _brute_guided(pkg, S, Q, e, a, n, z, R, F, 1.5, *sig), "nlm_guided %s R %d F %d" % (shape, R, F))
    plain = pkg.denoise.nlm(S, Q, e, R, F, 1.5)
    if R > 0 and ny * nx > 1:
        assert (got.view(np.uint32) != plain.view(np.uint32)).any(), "the features change nothing"
    # every feature off: nlm bit for bit
    assert_bit_equal(pkg.denoise.nlm_guided(S, Q, e, a, n, z, R, F, 1.5, 1e18, 1e18, 1e18), plain, "sigmas 1e18 %s" % (shape,))
    m, _, valid = pkg.denoise.mean_var(S, Q, e)
    assert_bit_equal(got[~valid], m[~valid], "pixels that take no part keep their mean")


def test_feature_weight_cases(pkg):
    """Single pairs: equal features weigh 1, a not-finite value switches the pair's features off, two misses (depth 0 + 0) are
    equal, the largest of the three distances decides."""
    fw = pkg.denoise.feature_weight
    a = np.zeros((1, 2, 3), f32)
    n = np.zeros((1, 2, 3), f32)
    z = np.zeros((1, 2), f32)
    assert fw(a, n, z, 0, 1, 0.1, 0.1, 0.1)[0, 0] == 1.0            # two misses: 0 / 1e-20 = 0
    z[0] = (2.0, 2.0)
    n[0, 0], n[0, 1] = (0, 1, 0), (1, 0, 0)
    assert fw(a, n, z, 0, 1, 0.1, 1.0, 1.0)[0, 0] == 0.0             # xn = 2 / 0.01: u clamps to 0
    assert fw(a, n, z, 0, 1, 2.0, 1.0, 1.0)[0, 0] == f32(f32(0.875 * 0.875) * f32(0.875 * 0.875))   # xn = 0.5
    z[0, 1] = np.nan
    assert fw(a, n, z, 0, 1, 0.1, 1.0, 1.0)[0, 0] == 1.0
    z[0] = (1.0, 3.0)
    n[...] = 0
    assert fw(a, n, z, 0, 1, 1.0, 1.0, 1.0)[0, 0] == f32(f32(0.9375 * 0.9375) * f32(0.9375 * 0.9375))   # xz = (4 / 16) / 1


def _outside_opening(cam, nx, ny, pkg):
    """Cornell: pixels whose g = 1 ray passes the plane z = 0 outside the box's opening [0, 555]^2 (float64 geometry)."""
    r = pkg.features.subpixel_rays(cam, nx, ny, 1)[0].astype(np.float64)
    t = -r[..., 2] / r[..., 5]
    x, y = r[..., 0] + t * r[..., 3], r[..., 1] + t * r[..., 4]
    return (x < 0) | (x > 555) | (y < 0) | (y > 555)


def test_reference_planes_on_the_oracle(pkg, oracle):
    """Cornell 32 x 32, g = 1: the normals are the walls' axis vectors (and the two turned boxes' faces), the albedos the walls'
    colours.  The box is open towards the camera, whose view is wider than the opening (half-width 800 tan 20 deg = 291 at
    z = 0 against 277.5), so the frame's outermost pixels look past the box and their rays miss.  The only other misses are rays
    that run exactly into the seam of two walls (direction x = +-direction y on this square frame: x = y = 555 at the same t,
    and both rectangles' open ranges turn the point down).  book-1 48 x 32: the sky dome catches every ray."""
    nx = ny = 32
    a, n, z, missed = reference_planes(pkg, oracle, "cornell", nx, ny, 1)
    _, _, cam = build_recorded(pkg, oracle, "cornell", nx, ny)
    out = _outside_opening(cam, nx, ny, pkg)
    hit = z > 0
    r = pkg.features.subpixel_rays(cam, nx, ny, 1)[0]
    seam = np.abs(r[..., 3]) == np.abs(r[..., 4])
    assert not hit[out].any() and (hit | out | seam).all() and missed == int((~hit).sum()) and out.sum() <= missed < 4 * nx + 4
    assert (a[~hit] == 0).all() and (n[~hit] == 0).all() and (z[~hit] == 0).all()
    colours = {(0.65, 0.05, 0.05), (0.73, 0.73, 0.73), (0.12, 0.45, 0.15), (15.0, 15.0, 15.0)}
    seen = {tuple(float(c) for c in np.round(v.astype(np.float64), 6)) for v in np.unique(a[hit], axis=0)}
    assert seen == colours, seen
    axis = (np.abs(n[hit]) == 1).sum(axis=-1) == 1
    turned = (n[hit][:, 1] == 0) & (np.abs((n[hit] ** 2).sum(axis=-1) - 1) < 1e-6)   # faces of the boxes rotated about y
    assert (axis | turned).all() and axis.sum() > 0.6 * hit.sum() and (~axis).sum() > 0
    for wall, colour in (((1, 0, 0), 0.65), ((-1, 0, 0), 0.12)):   # the red wall (x = 0) faces +x, the green one (x = 555, FlipNormals) -x
        at = hit & (n == np.array(wall, f32)).all(axis=-1)
        assert at.any() and (a[at][:, 0] == f32(colour)).all(), wall
    nx, ny = 48, 32
    for g in (1, 2):
        a, n, z, missed = reference_planes(pkg, oracle, "book1", nx, ny, g)
        assert missed == 0 and (z > 0).all() and np.isfinite(a).all() and np.isfinite(n).all()
    a1 = reference_planes(pkg, oracle, "book1", nx, ny, 1)[0]
    assert (a != a1).any() and a.min() >= 0 and a.max() <= 1.0


_renders = {}


def _render(pkg, oracle, name):
    """(S, Q, ns, reference, the g = 2 feature planes) of one of the two renders of the benefit test; computed once."""
    if name not in _renders:
        scene, nx, ny, ns, ref_ns = {"cornell": ("cornell_box_scene", 96, 96, 32, 2048), "book1": ("random_scene", 192, 128, 8, 512)}[name]
        b = oracle.builder()
        world, cam, _ = getattr(pkg.scenes, scene)(b, nx, ny)
        so = b.scene(world)
        S, Q = _oracle_sums(so, cam, nx, ny, ns)
        ref = so.par_cast(cam, nx, ny, ref_ns, seed=12345).astype(np.float64)
        _renders[name] = (S, Q, ns, ref, reference_planes(pkg, oracle, name, nx, ny, 2)[:3])
    return _renders[name]


def _rmse_pair(pkg, oracle, name, k, sigma):
    S, Q, ns, ref, (a, n, z) = _render(pkg, oracle, name)
    e = np.full(S.shape[:2], ns, np.uint32)
    rmse = lambda img: float(np.sqrt(np.mean((img.astype(np.float64) - ref) ** 2)))
    return rmse(pkg.denoise.nlm(S, Q, e, 5, 2, k)), rmse(pkg.denoise.nlm_guided(S, Q, e, a, n, z, 5, 2, k, sigma, sigma, sigma))


def test_guiding_lowers_the_true_error(pkg, oracle):
    """RMSE against a high-sample render with another seed (test_denoise_abi's set-up: R = 5, F = 2, seed 12345).  The bounds
    are the issue's; measured with this reference on these oracle renders: Cornell 96x96x32 at sigma 0.1: guided / colour-only
    0.826 at k = 2.5, best over k 0.859; book-1 192x128x8 at sigma 0.5, k = 1: 0.988."""
    ks = (0.7, 1.0, 1.5, 2.5)
    pairs = {k: _rmse_pair(pkg, oracle, "cornell", k, 0.1) for k in ks}
    for k in ks:
        print("cornell 96x96x32 k %.1f: colour-only %.4f guided %.4f ratio %.3f" % (k, pairs[k][0], pairs[k][1], pairs[k][1] / pairs[k][0]))
    best_plain, best_guided = min(p[0] for p in pairs.values()), min(p[1] for p in pairs.values())
    print("cornell best: colour-only %.4f guided %.4f ratio %.3f" % (best_plain, best_guided, best_guided / best_plain))
    assert pairs[2.5][1] / pairs[2.5][0] <= 0.87
    assert best_guided <= 0.90 * best_plain
    plain, guided = _rmse_pair(pkg, oracle, "book1", 1.0, 0.5)
    print("book-1 192x128x8 k 1.0: colour-only %.4f guided %.4f ratio %.3f" % (plain, guided, guided / plain))
    assert guided <= plain


def test_features_on_the_oracle_backend_raises(pkg, oracle):
    b = oracle.builder()
    world, cam, _ = pkg.scenes.random_scene(b, 8, 8)
    so = b.scene(world)
    with pytest.raises(ValueError, match="FEATURES"):
        so.par_cast(cam, 8, 8, 2, features=True)
    with pytest.raises(ValueError, match="FEATURES"):
        so.par_cast_device(cam, pkg.capi.make_params(8, 8, 2), 0, features=True)
    with pytest.raises(ValueError, match="FEATURES"):
        next(so.progressive(cam, 8, 8, 4, 2, features=True))
    with pytest.raises(ValueError, match="SUM_SQUARES|SAMPLE_COUNTS|FEATURES"):
        next(so.adaptive(cam, 8, 8, 4, 2, 0.1, features=True))


def test_validation_before_any_library_call(pkg):
    capi = pkg.capi

    class _NoLib(capi.Scene):
        def __init__(self):
            self.be = type("B", (), {"prefix": "rtg_", "path": "-"})()
    cam = capi.Camera()
    with pytest.raises(ValueError, match="squares=True"):
        _NoLib().par_cast(cam, 8, 8, 4, features=True, denoise=True)
    with pytest.raises(ValueError, match="unknown key"):
        _NoLib().par_cast(cam, 8, 8, 4, features={"sigma": 1})
    with pytest.raises(ValueError, match="another size"):
        _NoLib().par_cast(cam, 8, 8, 4, features=True, out=capi.features_frame(4, 4))
    with pytest.raises(ValueError, match="what the frame holds"):
        _NoLib().par_cast(cam, 8, 8, 4, features=True, out=capi.features_frame(8, 8, squares=True))
    with pytest.raises(ValueError, match="own counts"):
        _NoLib().par_cast(cam, 8, 8, 4, features=True, out=capi.features_frame(8, 8), counts=np.zeros((8, 8), np.uint32))
    with pytest.raises(ValueError, match="FeaturesFrame or an array"):
        _NoLib().par_cast(cam, 8, 8, 4, features=True, squares=True, out=capi.denoise_frame(8, 8))
    with pytest.raises(ValueError, match="retire="):
        _NoLib().par_cast(cam, 8, 8, 4, features=True, squares=True, retire=capi.Retire())
    with pytest.raises(ValueError, match="resume=True needs out="):
        _NoLib().par_cast(cam, 8, 8, 4, features=True, resume=True, sample_begin=2)
    # the loops: the existing arguments are checked first, in the order they were
    with pytest.raises(ValueError, match="step"):
        next(_NoLib().progressive(cam, 8, 8, 4, 0, features={"bad": 1}))
    with pytest.raises(ValueError, match="unknown key"):
        next(_NoLib().progressive(cam, 8, 8, 4, 2, features={"bad": 1}))
    with pytest.raises(ValueError, match="radius"):
        next(_NoLib().adaptive(cam, 8, 8, 4, 2, 0.1, radius=9, features={"bad": 1}))
    with pytest.raises(ValueError, match="unknown key"):
        next(_NoLib().adaptive(cam, 8, 8, 4, 2, 0.1, features={"bad": 1}))
    with pytest.raises(ValueError, match="preview"):
        next(_NoLib().adaptive(cam, 8, 8, 4, 2, 0.1, out=1 << 20, features=True))
    with pytest.raises(ValueError, match="FeaturesFrame"):
        next(_NoLib().adaptive(cam, 8, 8, 4, 2, 0.1, out=capi.counts_frame(8, 8, squares=True), features=True))
    with pytest.raises(ValueError, match="grid"):
        pkg.features.subpixel_rays(cam, 8, 8, 5)
