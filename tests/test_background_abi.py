"""A background, CPU side (include/rtiow_gpu.h RTG_FLAG_BACKGROUND): the flag and the block in the header and its mirrors; the
block's place in the frame for every flag combination, in the binding and in the library's own FrameLayout (a stand-alone C++
program); background.sky against a float64 evaluation; and the premise of the GPU tests -- on the oracle, book-1 with the dome
inside the Bvh and book-1 with the dome behind the Bvh in a list world are the same frame, ray for ray."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu.h")
CSRC = os.path.join(ROOT, "rtiow-rust_amd", "csrc")
SIZES = [(1, 1), (7, 5), (8, 4), (37, 29), (65536, 65535)]   # (the last: offsets beyond 2^32 bytes)
PARTS = ("counts", "retire", "denoise", "denoised", "features", "albedo", "normal", "depth", "error")


def _combos():
    """The legal (squares, counts, retire, denoise, features, error) combinations (test_multi_planes_abi._combos)."""
    return [c for c in itertools.product((0, 1), repeat=6)
            if not (c[2] and not (c[0] and c[1])) and not (c[3] and not c[0]) and not (c[5] and not c[3])]


def test_header_and_mirrors(pkg):
    text = open(HEADER).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RTG_FLAG_\w+) (\d+)u", text)}
    assert flags["RTG_FLAG_BACKGROUND"] == 1024 == pkg.capi.FLAG_BACKGROUND
    assert sorted(flags.values()) == [1 << k for k in range(11)]   # every flag its own bit
    body = re.search(r"typedef struct rtg_background \{(.*?)\} rtg_background;", text, re.S).group(1)
    fields = re.findall(r"(uint32_t|float) (\w+)(?:\[(\d+)\])?;", body)
    assert [(t, n, int(k or 1)) for t, n, k in fields] == [("uint32_t", "mode", 1), ("uint32_t", "reserved_in", 1), ("float", "bottom", 3),
                                                            ("float", "top", 3), ("uint32_t", "reserved", 8)]
    B = pkg.capi.Background
    assert C.sizeof(B) == 64 and B.OUT_OFFSET == 32 == B.reserved.offset
    assert [(n, getattr(B, n).offset) for n, _ in B._fields_] == [("mode", 0), ("reserved_in", 4), ("bottom", 8), ("top", 20), ("reserved", 32)]
    assert C.sizeof(pkg.capi.Params) == 56   # rtg_params keeps its size
    assert len(pkg.capi.ABI_SYMBOLS) == 42   # (the feature adds no symbol)
    rs = open(os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "lib.rs")).read()
    assert re.search(r"pub const RTG_FLAG_BACKGROUND: u32 = 1024;", rs) and "pub struct rtg_background" in rs
    hpp = open(os.path.join(ROOT, "rtiow-rust_amd", "host", "rtiow.hpp")).read()
    assert "RTG_FLAG_BACKGROUND" in hpp and "rtg_background" in hpp


def test_block_offset_in_the_binding(pkg):
    """The header's rule: the first even word behind everything the other flags put in the frame; no other offset moves."""
    capi = pkg.capi
    for nx, ny in SIZES:
        for c in _combos():
            off, on = capi.FrameLayout(nx, ny, *c), capi.FrameLayout(nx, ny, *c, background=True)
            assert off.background is None and off.words == capi.FrameLayout(nx, ny, *c, False).words
            assert on.background == (off.words + 1) & ~1 and on.words == on.background + 16
            for part in PARTS + ("squares", "n"):
                assert getattr(on, part) == getattr(off, part), (nx, ny, c, part)
        assert capi.FrameLayout(nx, ny, background=True).background == (3 * nx * ny + 1) & ~1
    f = capi.Frame(5, 3, background={"bottom": (1, 2, 3), "top": (4, 5, 6)})
    assert f.flags()["background"] and f.layout.background == 46 and f.buf.size == 62
    assert (f.background.mode, tuple(f.background.bottom), tuple(f.background.top)) == (1, (1.0, 2.0, 3.0), (4.0, 5.0, 6.0))
    assert (f.buf[46:48].view(np.uint32) == (1, 0)).all() and (f.buf[48:54] == (1, 2, 3, 4, 5, 6)).all() and not f.buf[54:].any()
    g = capi.make_background((0.25, 0.5, 0.75))
    assert (g.mode, g.reserved_in, tuple(g.bottom), tuple(g.top)) == (0, 0, (0.25, 0.5, 0.75), (0.0, 0.0, 0.0))
    assert capi.make_params(4, 4, 1, background=True).flags == 1024
    for bad in (True, None, (1, 2), {"top": (1, 1, 1)}, {"bottom": (1, 1, 1), "colour": 1}, {"bottom": (1, 1, 1), "mode": 1}):
        with pytest.raises(ValueError):
            capi.make_background(bad)


PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "rt_multi_planes.h"
using namespace rtg;
int main() {
  const uint32_t sizes[][2] = {%(sizes)s};
  const uint32_t flag_of[6] = {RTG_FLAG_SUM_SQUARES, RTG_FLAG_SAMPLE_COUNTS, RTG_FLAG_RETIRE, RTG_FLAG_DENOISE, RTG_FLAG_FEATURES, RTG_FLAG_DENOISE_ERROR};
  static_assert(sizeof(rtg_background) == 64 && sizeof(rtg_params) == 56, "ABI sizes");
  for (auto& sz : sizes)
    for (int bitsv = 0; bitsv < 64; bitsv++) {
      uint32_t flags = RTG_FLAG_BACKGROUND;
      for (int k = 0; k < 6; k++) if (bitsv & (1 << k)) flags |= flag_of[k];
      const FrameLayout L(sz[0], sz[1], flags), O(sz[0], sz[1], flags & ~RTG_FLAG_BACKGROUND);
      std::printf("lay %%u %%u %%d : %%llu %%llu %%llu :", sz[0], sz[1], bitsv, (unsigned long long)L.background, (unsigned long long)L.words, (unsigned long long)O.words);
      for (uint64_t part : {L.counts, L.retire, L.denoise, L.denoised, L.features, L.albedo, L.normal, L.depth, L.error})
        std::printf(" %%lld", L.has(part) ? (long long)part : -1ll);
      std::printf(" : %%d :", (int)O.has(O.background));
      // the block travels to the device whatever else does, and never back
      for (int keeps = 0; keeps < 2; keeps++) {
        const Extents up = upload_extents(L, false, (uint32_t)keeps, 1u), back = copy_back_extents(L, 1u);
        std::printf(" %%d %%d", up.n > 0 && up.e[up.n - 1].lo == 4u * L.background && up.e[up.n - 1].hi == 4u * L.words,
                    back.n > 0 && back.e[back.n - 1].hi <= 4u * L.background);
        for (int i = 0; i + 1 < up.n; i++) if (up.e[i].hi > up.e[i + 1].lo) std::printf(" OVERLAP");
      }
      std::printf("\n");
    }
  return 0;
}
"""


def test_block_offset_in_the_library(pkg, tmp_path):
    """csrc/rt_multi_planes.h FrameLayout, field for field the binding's; rtg_par_cast uploads the block and never copies it back."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the stand-alone FrameLayout program")
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text(PROGRAM % {"sizes": ", ".join("{%du, %du}" % s for s in SIZES)})
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    legal, seen = set(_combos()), 0
    for ln in r.stdout.splitlines():
        a, b, c, d, e = [x.strip().split() for x in ln[4:].split(":")]
        nx, ny, bitsv = int(a[0]), int(a[1]), int(a[2])
        combo = tuple((bitsv >> k) & 1 for k in range(6))
        if combo not in legal:
            continue
        seen += 1
        lay = pkg.capi.FrameLayout(nx, ny, *combo, background=True)
        assert [int(x) for x in b] == [lay.background, lay.words, pkg.capi.FrameLayout(nx, ny, *combo).words], ln
        assert [int(x) for x in c] == [-1 if getattr(lay, p) is None else getattr(lay, p) for p in PARTS], ln
        assert d == ["0"] and e == ["1", "1", "1", "1"], ln
    assert seen == len(SIZES) * len(legal)


def _sky64(d, bottom, top):
    d = np.asarray(d, np.float64)
    t = 0.5 * (d[..., 1] / np.sqrt((d * d).sum(axis=-1)) + 1.0)
    return (1.0 - t)[..., None] * np.asarray(bottom, np.float64) + t[..., None] * np.asarray(top, np.float64)


def test_sky_against_float64(pkg):
    """A rounding bound: float32 against float64 on colours in [0, 1] is a few 1e-7; a wrong axis, a missing normalisation or
    swapped colours move the answer by 0.1 or more."""
    sky = pkg.background.sky
    rs = np.random.RandomState(7)
    d = (rs.standard_normal((4096, 3)) * np.exp(rs.uniform(-6, 6, (4096, 1)))).astype(np.float32)
    d = np.concatenate([d, np.eye(3, dtype=np.float32), -np.eye(3, dtype=np.float32), np.float32([[3e-20, 4e-20, 0], [1e18, -1e18, 1e18]])])
    for bottom, top in (((1.0, 1.0, 1.0), (0.5, 0.7, 1.0)), ((0.1, 0.9, 0.3), (0.8, 0.05, 0.6))):
        got = sky(d, bottom, top, 1)
        assert got.dtype == np.float32 and got.shape == d.shape
        err = np.abs(got.astype(np.float64) - _sky64(d.astype(np.float64), bottom, top)).max()
        print("sky vs float64: max abs error %.3g" % err)
        assert err <= 1e-6
        # the properties a wrong formula breaks: straight up is `top`, straight down `bottom`, the horizon their mean
        assert_bit_equal(sky(np.float32([[0, 2, 0], [0, -3, 0]]), bottom, top, 1), np.float32([top, bottom]))
        assert np.abs(sky(np.float32([[5, 0, -1]]), bottom, top, 1) - (np.float32(bottom) + np.float32(top)) / 2).max() <= 1e-6
        const = sky(d, bottom, top, 0)
        assert (const.view(np.uint32) == np.float32(bottom).view(np.uint32)).all()   # mode 0: `bottom`, exactly
    assert np.isnan(sky(np.float32([[0, 0, 0]]), (1, 1, 1), (0, 0, 0), 1)).all()      # 0 / 0: NaN propagates, as in the kernels
    assert_bit_equal(pkg.background.miss_colour(np.float32([[0, 1, 0]]), (1, 1, 1), (0.5, 0.7, 1.0), 1, strength=(0.5, 0.5, 2.0)),
                     np.float32([[0.25, 0.35, 2.0]]))


@pytest.mark.parametrize("nx,ny,ns", [(48, 32, 4), (96, 64, 8)])
def test_premise_dome_inside_and_behind_the_bvh(pkg, oracle, nx, ny, ns):
    """What lets the GPU tests check a constant background against the oracle bit for bit: the dome is hit exactly when nothing
    else is, wherever it stands in the world."""
    S = pkg.scenes

    def render(inside):
        b = oracle.builder()
        objs = S.random_scene_objects(b, pkg.small_rng.SmallRng(0xDEADBEEF), dome=False)
        dome = b.flip_normals(b.sphere(10000.0, b.diffuse_light(b.constant(S.v(*S.DOME_COLOUR)), 1.0)))
        world = [b.bvh(objs + [dome], (0.0, 1.0))] if inside else [b.bvh(objs, (0.0, 1.0)), dome]
        _, cam, _ = S.random_scene(oracle.builder(), nx, ny)
        return b.scene(world).par_cast(cam, nx, ny, ns, stats=True)
    (img_in, st_in), (img_out, st_out) = render(True), render(False)
    assert_bit_equal(img_in, img_out, "dome inside the Bvh vs behind it")
    assert st_in["rays"] == st_out["rays"] and st_in["draws"] == st_out["draws"]
    # ... and the scene helper's two forms are that world
    b = oracle.builder()
    world, cam, _ = S.random_scene(b, nx, ny)
    assert_bit_equal(b.scene(world).par_cast(cam, nx, ny, ns), img_in, "random_scene(sky='dome')")
    b2 = oracle.builder()
    world2, cam2, _, bg = S.random_scene(b2, nx, ny, sky="background")
    assert bytes(cam2) == bytes(cam) and bg == {"bottom": S.DOME_COLOUR}
    assert len(world2) == 1 and world2 != world
