"""Flagged frames over several handles, the parts that need no GPU: the scene option and its block in the header; PlaneSet
(csrc/rt_multi_planes.h, host part) against the binding's layout helpers and the plane-major packed index, through a stand-alone
C++ program built with the address and undefined-behaviour sanitizers and run as a child process; the binding's own checks; and
that host/rtiow.hpp's multi calls compile."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu.h")
CSRC = os.path.join(ROOT, "rtiow-rust_amd", "csrc")
SIZES = [(1, 1), (7, 5), (8, 4), (37, 29), (44, 28)]
PIX_WORK = [0, 1, 255, 256, 257]

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rt_multi_planes.h"
using namespace rtg;
struct Slice { bool squares, counts, retire, denoise, features; };
static void fail(const char* what) { std::printf("FAIL %%s\n", what); std::exit(1); }
int main() {
  const uint32_t sizes[][2] = {%(sizes)s};
  for (auto& sz : sizes)
    for (int bitsv = 0; bitsv < 64; bitsv++) {
      const Slice sl{(bitsv & 1) != 0, (bitsv & 2) != 0, (bitsv & 4) != 0, (bitsv & 8) != 0, (bitsv & 16) != 0};
      const bool compute = (bitsv & 32) != 0;
      if ((sl.retire && !(sl.squares && sl.counts)) || (sl.denoise && !sl.squares) || (compute && !sl.features)) continue;
      const PlaneSet ps = make_plane_set(sz[0], sz[1], sl, compute);
      std::printf("set %%u %%u %%d %%d %%d %%d %%d %%d : %%u %%u :", sz[0], sz[1], sl.squares, sl.counts, sl.retire, sl.denoise, sl.features, compute,
                  ps.n_groups, ps.words_per_pixel);
      for (uint32_t g = 0; g < ps.n_groups; g++) std::printf(" %%llu/%%u/%%u", (unsigned long long)ps.g[g].first, ps.g[g].wpp, ps.g[g].k0);
      std::printf(" : %%llu %%llu %%llu\n", (unsigned long long)retire_block_word(sz[0], sz[1]),
                  (unsigned long long)denoise_block_word(sz[0], sz[1], sl.counts, sl.retire), (unsigned long long)features_block_word(sz[0], sz[1], sl));
    }
  // pack and unpack a host frame of pix_work pixels through the plane-major index: every packed word visited once, none beyond
  // pix_work * words_per_pixel (the vectors are exactly that long: the address sanitizer sees an overrun)
  const uint32_t works[] = {%(works)s};
  for (int full = 0; full < 2; full++) {
    const Slice sl{full != 0, false, false, false, full != 0};
    for (uint32_t pw : works) {
      const PlaneSet ps = make_plane_set(pw ? pw : 1u, 1u, sl, full != 0);  // a frame of pw x 1 pixels: work item w = pixel w
      const uint64_t n = pw, frame_words = features_block_word(pw ? pw : 1u, 1u, sl) + 16u + 7u * n;
      std::vector<uint32_t> frame(frame_words), back(frame_words, 0u), packed((size_t)pw * ps.words_per_pixel, 0xdeadbeefu);
      std::vector<uint32_t> seen(packed.size(), 0u);
      for (uint64_t i = 0; i < frame_words; i++) frame[i] = (uint32_t)(i * 2654435761u + 17u);
      for (uint32_t w = 0; w < pw; w++)
        for (uint32_t g = 0; g < ps.n_groups; g++)
          for (uint32_t c = 0; c < ps.g[g].wpp; c++) {
            const uint64_t at = packed_word(ps.g[g].k0 + c, w, pw);
            if (at >= packed.size()) fail("packed index beyond pix_work * words_per_pixel");
            packed[at] = frame[frame_word(ps.g[g], c, w)], seen[at]++;
          }
      for (uint32_t v : seen) if (v != 1u) fail("a packed word not visited exactly once");
      uint64_t moved = 0;
      for (uint32_t w = 0; w < pw; w++)
        for (uint32_t g = 0; g < ps.n_groups; g++)
          for (uint32_t c = 0; c < ps.g[g].wpp; c++) back[frame_word(ps.g[g], c, w)] = packed[packed_word(ps.g[g].k0 + c, w, pw)], moved++;
      for (uint32_t g = 0; g < ps.n_groups; g++)
        for (uint64_t i = 0; i < (uint64_t)ps.g[g].wpp * n; i++)
          if (back[ps.g[g].first + i] != frame[ps.g[g].first + i]) fail("a word did not come back");
      std::printf("pack %%u %%u %%llu\n", pw, ps.words_per_pixel, (unsigned long long)moved);
    }
  }
  return 0;
}
"""


def test_option_and_header(pkg):
    assert "multi_planes" in pkg.capi.Scene.ENV_OPTIONS
    text = open(HEADER).read()
    at = text.index("int rtg_par_cast_multi(")
    block = text[text.rindex("/*", 0, at):at]
    assert '"multi_planes"' in block and "RTG_ERR_UNSUPPORTED" in block and "plane-major" in block
    assert len(pkg.capi.ABI_SYMBOLS) == 42   # (the feature adds no symbol)


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the stand-alone PlaneSet program")
    d = tmp_path_factory.mktemp("plane_set")
    src = d / "plane_set.cpp"
    src.write_text(PROGRAM % {"sizes": ", ".join("{%d, %d}" % s for s in SIZES), "works": ", ".join("%du" % w for w in PIX_WORK)})
    exe = d / "plane_set"
    # (the sanitizers' runtimes are linked INTO the program: it needs nothing preloaded and runs in the environment it inherits)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


def test_plane_set_against_the_layout_helpers(pkg, program_output):
    capi = pkg.capi
    lines = [ln for ln in program_output if ln.startswith("set ")]
    combos = [c for c in itertools.product((0, 1), repeat=6)
              if not (c[2] and not (c[0] and c[1])) and not (c[3] and not c[0]) and not (c[5] and not c[4])]
    assert len(lines) == len(SIZES) * len(combos) and len(combos) == 24
    seen = set()
    for ln in lines:
        head, sizes, groups, blocks = [part.split() for part in ln[4:].split(":")]
        nx, ny, squares, counts, retire, denoise, features, compute = map(int, head)
        seen.add((nx, ny, squares, counts, retire, denoise, features, compute))
        n = nx * ny
        want = [(0, 3)]
        if squares:
            want.append((3 * n, 3))
        if features and compute:
            albedo = capi.features_block_offset(nx, ny, bool(squares), bool(counts), bool(retire), bool(denoise)) // 4 + 16
            want += [(albedo, 3), (albedo + 3 * n, 3), (albedo + 6 * n, 1)]
        got = [tuple(map(int, g.split("/"))) for g in groups]
        k0 = list(itertools.accumulate([0] + [w for _, w in want[:-1]]))
        assert got == [(f, w, k) for (f, w), k in zip(want, k0)], ln
        wpp = sum(w for _, w in want)
        assert list(map(int, sizes)) == [len(want), wpp] and 3 <= wpp <= 13, ln
        r_word, d_word, f_word = map(int, blocks)
        assert r_word * 4 == capi.retire_block_offset(nx, ny), ln
        if denoise:
            assert d_word * 4 == capi.denoise_block_offset(nx, ny, bool(counts), bool(retire)), ln
        if features:
            assert f_word * 4 == capi.features_block_offset(nx, ny, bool(squares), bool(counts), bool(retire), bool(denoise)), ln
            # the planes end where the frame ends
            assert (f_word + 16 + 7 * n) * 4 == capi.features_frame_bytes(nx, ny, bool(squares), bool(counts), bool(retire), bool(denoise)), ln
    assert seen == {(nx, ny) + c for nx, ny in SIZES for c in combos}


def test_plane_major_pack_and_unpack(program_output):
    lines = [ln.split() for ln in program_output if ln.startswith("pack ")]
    assert not [ln for ln in program_output if ln.startswith("FAIL")]
    assert [(int(pw), int(wpp)) for _, pw, wpp, _ in lines] == [(pw, wpp) for wpp in (3, 13) for pw in PIX_WORK]
    assert all(int(moved) == int(pw) * int(wpp) for _, pw, wpp, moved in lines)


class _Handle:
    h = None


def test_binding_checks_frames_before_the_library_call(pkg, monkeypatch):
    capi = pkg.capi
    be = pkg.load()
    calls = []

    def record(arr, n, cam, p, out, st):
        calls.append((n, p._obj.flags))
        return 0

    monkeypatch.setattr(be, "_par_cast_multi", record)
    cam = capi.Camera()
    scenes = [_Handle(), _Handle()]
    nx, ny = 12, 8
    with pytest.raises(ValueError, match="another size"):
        be.par_cast_multi(scenes, cam, nx, ny, 4, out=capi.counts_frame(nx + 1, ny, squares=True))
    with pytest.raises(ValueError, match="another size"):
        be.par_cast_multi(scenes, cam, nx, ny, 4, out=capi.features_frame(nx, ny + 1))
    with pytest.raises(ValueError, match="shape"):
        be.par_cast_multi(scenes, cam, nx, ny, 4, out=np.zeros((2, ny, nx, 3), np.float32), squares=True, counts=np.zeros((ny, nx + 1), np.uint32))
    with pytest.raises(ValueError, match="squares=True"):
        be.par_cast_multi(scenes, cam, nx, ny, 4, out=np.zeros((ny, nx, 3), np.float32), denoise={"k": 0.5})
    assert calls == []
    # a plain array with a plain flag is the library's to answer: forwarded as it is
    be.par_cast_multi(scenes, cam, nx, ny, 4, out=np.zeros((ny, nx, 3), np.float32), features=True)
    assert calls == [(2, capi.FLAG_FEATURES)]
    # frames: the flags of the parts they have
    f = capi.features_frame(nx, ny, squares=True, counts=True, retire=True, denoise={"k": 0.5})
    assert be.par_cast_multi(scenes, cam, nx, ny, 4, out=f, partial=True) is f
    want = capi.FLAG_SUM_SQUARES | capi.FLAG_SAMPLE_COUNTS | capi.FLAG_RETIRE | capi.FLAG_DENOISE | capi.FLAG_FEATURES | capi.FLAG_PARTIAL
    assert calls[-1] == (2, want)
    g = capi.counts_frame(nx, ny, squares=True)
    out, st = be.par_cast_multi(scenes, cam, nx, ny, 4, out=g, stats=True)
    assert out is g and calls[-1] == (2, capi.FLAG_SUM_SQUARES | capi.FLAG_SAMPLE_COUNTS | capi.FLAG_COUNTERS) and "samples" in st
    # arrays of the caller's go through a staging frame and come back
    planes, counts = np.zeros((2, ny, nx, 3), np.float32), np.full((ny, nx), 4, np.uint32)
    d = be.par_cast_multi(scenes, cam, nx, ny, 4, out=planes, squares=True, counts=counts, denoise={"k": 0.5, "radius": 2, "patch": 1})
    assert isinstance(d, capi.DenoiseFrame) and d.denoise.radius == 2 and (d.counts == 4).all()
    assert calls[-1] == (2, capi.FLAG_SUM_SQUARES | capi.FLAG_SAMPLE_COUNTS | capi.FLAG_DENOISE)


def test_cpp_multi_calls_compile(tmp_path):
    """host/rtiow.hpp is header-only: its rtg_par_cast_multi wrappers are compiled here (every inline function instantiated by
    taking its address; nothing is linked or run)."""
    src = tmp_path / "multi_calls.cpp"
    src.write_text('#include "rtiow.hpp"\n'
                   "int main() {\n"
                   "  (void)&rtiow::make_scenes; (void)&rtiow::par_cast_multi; (void)&rtiow::par_cast_multi_squares;\n"
                   "  (void)&rtiow::par_cast_multi_denoised; (void)&rtiow::par_cast_multi_features;\n"
                   "  (void)&rtiow::par_cast_denoised; (void)&rtiow::par_cast_features;\n"
                   "  return 0;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "rtiow-rust_amd", "host"), str(src),
                           "-o", str(tmp_path / "multi_calls.o")])
