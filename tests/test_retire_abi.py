"""Adaptive sampling in the library, CPU side: RTG_FLAG_RETIRE and rtg_retire in the header, the ctypes binding, the Rust `-sys`
crate and the C++ header; the retire frame's layout; noise.retire's window rule against a brute-force loop; the Python refusals
(oracle backend, validation order)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu.h")
SYS_RS = os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "lib.rs")
FIELDS = ["target_se", "min_samples", "radius", "active", "retired", "estimated", "reserved", "sum_se2", "samples_held",
          "reserved2"]


def _header():
    return open(HEADER).read()


def test_header_declares_the_flag_and_the_block():
    text = _header()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RTG_FLAG_[A-Z_]+) (\d+)u", text)}
    assert flags["RTG_FLAG_RETIRE"] == 64
    assert sum(1 for v in flags.values() if v & 64) == 1
    assert re.search(r"#define RTG_RETIRE_MAX_RADIUS 8u", text)
    nc = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct rtg_retire \{(.*?)\} rtg_retire;", nc, flags=re.S).group(1)
    names = [re.findall(r"([a-z_0-9]+)(?:\[\d+\])?$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert names == FIELDS
    # no new entry point: the symbol scan of the ABI tests still sees the same 42 functions
    assert "rtg_retire(" not in nc.replace(" ", "")


def test_ctypes_retire_matches_the_compiled_header(pkg, tmp_path):
    capi = pkg.capi
    assert capi.FLAG_RETIRE == 64 and capi.RETIRE_MAX_RADIUS == 8
    assert [f for f, _ in capi.Retire._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtiow_gpu.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(rtg_retire));\n' +
                   "".join('  printf("%%zu\\n", offsetof(rtg_retire, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(capi.Retire) == 64
    assert got[1:] == [getattr(capi.Retire, f).offset for f in FIELDS]
    p = capi.make_params(8, 8, 4, counts=True, squares=True, retire=True)
    assert p.flags == capi.FLAG_SAMPLE_COUNTS | capi.FLAG_SUM_SQUARES | capi.FLAG_RETIRE


def test_rust_and_cpp_declare_the_block():
    rs = re.sub(r"//[^\n]*", "", open(SYS_RS).read())
    assert re.search(r"pub const RTG_FLAG_RETIRE: u32 = 64;", rs) and re.search(r"pub const RTG_RETIRE_MAX_RADIUS: u32 = 8;", rs)
    body = re.search(r"#\[repr\(C\)\][^{]*pub struct rtg_retire \{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub ([a-z_0-9]+):", body) == FIELDS
    assert not re.search(r"pub fn rtg_retire", rs)
    hpp = open(os.path.join(ROOT, "rtiow-rust_amd", "host", "rtiow.hpp")).read()
    assert "RTG_FLAG_RETIRE" in hpp and "par_cast_adaptive" in hpp


@pytest.mark.parametrize("nx,ny", [(7, 5), (8, 4), (1, 1), (37, 29)])
def test_retire_frame_layout(pkg, nx, ny):
    capi = pkg.capi
    n = nx * ny
    off = capi.retire_block_offset(nx, ny)
    assert off % 8 == 0 and off == 4 * (7 * n + (7 * n) % 2)
    assert capi.retire_frame_bytes(nx, ny) == off + 64
    f = capi.counts_frame(nx, ny, squares=True, retire=True)
    base = f.buf.ctypes.data
    assert f.buf.nbytes == capi.retire_frame_bytes(nx, ny)
    assert f.planes.shape == (2, ny, nx, 3) and f.planes.ctypes.data == base
    assert f.counts.shape == (ny, nx) and f.counts.ctypes.data == base + 24 * n
    assert C.addressof(f.retire) == base + off
    f.retire.active = 0xdeadbeef
    f.retire.sum_se2 = 2.5
    assert f.buf.view(np.uint32)[off // 4 + 4] == 0xdeadbeef and f.buf[off // 4:].view(np.float64)[4] == 2.5
    # the frame's own views render in place; other arrays go through a staging frame that carries the block
    dst, staging = capi._counts_call(f.planes, f.counts, nx, ny, True, f.retire)
    assert staging is None and dst is f.planes
    r = capi.Retire()
    r.radius = 3
    dst, staging = capi._counts_call(f.planes, f.counts, nx, ny, True, r)
    assert staging is not None and staging.retire.radius == 3 and staging.retire.active == 0
    with pytest.raises(ValueError):
        capi.counts_frame(nx, ny, squares=False, retire=True)


def _brute(active, k, se, min_samples, target, radius, present):
    ny, nx = active.shape
    out = np.zeros_like(active)
    if k < min_samples:
        return out
    for y in range(ny):
        for x in range(nx):
            if not active[y, x]:
                continue
            ok = True
            for yy in range(max(0, y - radius), min(ny, y + radius + 1)):
                for xx in range(max(0, x - radius), min(nx, x + radius + 1)):
                    if present[yy, xx] and not all(se[yy, xx, c] <= target for c in range(3)):
                        ok = False
            out[y, x] = ok
    return out


@pytest.mark.parametrize("radius", [0, 1, 2, 3, 8])
def test_window_rule_against_brute_force(pkg, radius):
    noise = pkg.noise
    rs = np.random.RandomState(100 + radius)
    for ny, nx in ((9, 13), (1, 7), (20, 3)):
        se = rs.choice([0.01, 0.02, 0.04, 0.06], size=(ny, nx, 3))
        se[rs.rand(ny, nx, 3) < 0.02] = np.inf
        se[rs.rand(ny, nx, 3) < 0.02] = np.nan
        active = rs.rand(ny, nx) < 0.7
        present = rs.rand(ny, nx) < 0.85
        for target in (0.015, 0.05, 0.1):
            got = noise.retire(active, 16, se, 8, target, radius=radius, present=present)
            want = _brute(active, 16, se, 8, target, radius, present)
            assert got.dtype == bool and (got == want).all(), (radius, ny, nx, target)
            # the default present: every pixel takes part
            everyone = noise.retire(active, 16, se, 8, target, radius=radius)
            assert (everyone == _brute(active, 16, se, 8, target, radius, np.ones_like(active))).all()
        assert not noise.retire(active, 4, se, 8, 1.0, radius=radius, present=present).any()


def test_radius_zero_is_the_old_rule(pkg):
    noise = pkg.noise
    rs = np.random.RandomState(3)
    se = rs.uniform(0, 0.1, size=(12, 10, 3))
    se[rs.rand(12, 10, 3) < 0.05] = np.nan
    active = rs.rand(12, 10) < 0.8
    for k, t in ((16, 0.05), (8, 0.05), (16, 0.0), (16, np.inf)):
        old = np.zeros_like(active) if k < 16 else active & (np.max(se, axis=-1) <= t)
        assert (noise.retire(active, k, se, 16, t) == old).all()
        assert (noise.retire(active, k, se, 16, t, radius=0) == old).all()


def test_retire_on_the_oracle_backend_raises(pkg, oracle):
    b = oracle.builder()
    world, cam, _ = pkg.scenes.random_scene(b, 8, 8)
    so = b.scene(world)
    f = pkg.capi.counts_frame(8, 8, squares=True, retire=True)
    with pytest.raises(ValueError, match="SUM_SQUARES|SAMPLE_COUNTS|RETIRE"):
        so.par_cast(cam, 8, 8, 2, out=f.planes, counts=f.counts, squares=True, retire=f.retire)
    with pytest.raises(ValueError, match="RETIRE"):
        so.par_cast_device(cam, pkg.capi.make_params(8, 8, 2), 0, retire=True)
    with pytest.raises(ValueError, match="SUM_SQUARES|SAMPLE_COUNTS"):
        next(so.adaptive(cam, 8, 8, 4, 2, 0.1, out=1 << 20, preview=1 << 21))
    with pytest.raises(ValueError, match="SUM_SQUARES|SAMPLE_COUNTS"):
        next(so.adaptive(cam, 8, 8, 4, 2, 0.1, radius=1))


def test_adaptive_validation_order(pkg):
    capi = pkg.capi

    class _NoLib(capi.Scene):
        def __init__(self):
            self.be = type("B", (), {"prefix": "rtg_", "path": "-"})()
    with pytest.raises(ValueError, match="step"):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 0, 0.1, out=1 << 20, preview=1 << 21, radius=99))
    with pytest.raises(ValueError, match="radius"):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 2, 0.1, radius=9))
    with pytest.raises(ValueError, match="preview"):
        next(_NoLib().adaptive(capi.Camera(), 8, 8, 4, 2, 0.1, out=1 << 20))
    with pytest.raises(ValueError, match="retire="):
        _NoLib().par_cast(capi.Camera(), 8, 8, 4, counts=np.zeros((8, 8), np.uint32), retire=capi.Retire())
