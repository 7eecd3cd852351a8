"""Flagged frames over several handles, the parts that need no GPU: the scene option and its block in the header; FrameLayout,
the upload / copy-back extents and PlaneSet (csrc/rt_multi_planes.h, host part) against the binding's layout and the plane-major
packed index, through a stand-alone
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
static void fail(const char* what) { std::printf("FAIL %%s\n", what); std::exit(1); }
static void print_extents(const Extents& x) {
  for (int i = 0; i < x.n; i++) std::printf(" %%llu-%%llu", (unsigned long long)x.e[i].lo, (unsigned long long)x.e[i].hi);
}
int main() {
  const uint32_t sizes[][2] = {%(sizes)s};
  const uint32_t flag_of[6] = {RTG_FLAG_SUM_SQUARES, RTG_FLAG_SAMPLE_COUNTS, RTG_FLAG_RETIRE, RTG_FLAG_DENOISE, RTG_FLAG_FEATURES, RTG_FLAG_DENOISE_ERROR};
  for (auto& sz : sizes)
    for (int bitsv = 0; bitsv < 128; bitsv++) {
      const bool squares = (bitsv & 1) != 0, counts = (bitsv & 2) != 0, retire = (bitsv & 4) != 0, denoise = (bitsv & 8) != 0, features = (bitsv & 16) != 0;
      const bool error = (bitsv & 32) != 0, compute = (bitsv & 64) != 0;
      if ((retire && !(squares && counts)) || (denoise && !squares) || (error && !denoise) || (compute && !features)) continue;
      uint32_t flags = 0;
      for (int k = 0; k < 6; k++) if (bitsv & (1 << k)) flags |= flag_of[k];
      const FrameLayout L(sz[0], sz[1], flags);
      const PlaneSet ps = make_plane_set(L, compute);
      std::printf("set %%u %%u %%d %%d %%d %%d %%d %%d %%d : %%u %%u :", sz[0], sz[1], squares, counts, retire, denoise, features, error, compute,
                  ps.n_groups, ps.words_per_pixel);
      for (uint32_t g = 0; g < ps.n_groups; g++) std::printf(" %%llu/%%u/%%u", (unsigned long long)ps.g[g].first, ps.g[g].wpp, ps.g[g].k0);
      // the parts, -1 = absent; first the retire block of the frame that has one, whatever this frame's flags
      const FrameLayout R(sz[0], sz[1], RTG_FLAG_SUM_SQUARES | RTG_FLAG_SAMPLE_COUNTS | RTG_FLAG_RETIRE);
      std::printf(" : %%lld", (long long)R.retire);
      for (uint64_t part : {L.n, L.counts, L.retire, L.denoise, L.denoised, L.features, L.albedo, L.normal, L.depth, L.error, L.words})
        std::printf(" %%lld", L.has(part) ? (long long)part : -1ll);
      std::printf("\n");
      for (int other = 0; other < 2; other++)
        for (uint32_t begin = 0; begin < 2; begin++)
          for (uint32_t cmp = 0; cmp < 2; cmp++) {
            std::printf("ext %%u %%u %%d %%d %%u %%u :", sz[0], sz[1], bitsv & 63, other, begin, cmp);
            print_extents(upload_extents(L, other != 0, begin, cmp));
            std::printf(" :");
            print_extents(copy_back_extents(L, cmp));
            std::printf("\n");
          }
    }
  // pack and unpack a host frame of pix_work pixels through the plane-major index: every packed word visited once, none beyond
  // pix_work * words_per_pixel (the vectors are exactly that long: the address sanitizer sees an overrun)
  const uint32_t works[] = {%(works)s};
  for (int full = 0; full < 2; full++) {
    for (uint32_t pw : works) {
      const FrameLayout L(pw ? pw : 1u, 1u, RTG_FLAG_FEATURES | (full ? RTG_FLAG_SUM_SQUARES : 0u));  // a frame of pw x 1 pixels: work item w = pixel w
      const PlaneSet ps = make_plane_set(L, full != 0);
      const uint64_t n = pw, frame_words = L.features + 16u + 7u * n;
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


def _combos():
    """The legal (squares, counts, retire, denoise, features, error) combinations: retire needs squares and counts, denoise
    needs squares, error needs denoise."""
    return [c for c in itertools.product((0, 1), repeat=6)
            if not (c[2] and not (c[0] and c[1])) and not (c[3] and not c[0]) and not (c[5] and not c[3])]


def test_plane_set_against_the_layout_helpers(pkg, program_output):
    capi = pkg.capi
    lines = [ln for ln in program_output if ln.startswith("set ")]
    combos = [c + (k,) for c in _combos() for k in ((0, 1) if c[4] else (0,))]
    assert len(_combos()) == 22 and len(combos) == 33
    assert len([c for c in combos if not c[5]]) == 24   # (the combinations without the error flag, as before it existed)
    assert len(lines) == len(SIZES) * len(combos)
    seen = set()
    for ln in lines:
        head, sizes, groups, blocks = [part.split() for part in ln[4:].split(":")]
        nx, ny, squares, counts, retire, denoise, features, error, compute = map(int, head)
        seen.add((nx, ny, squares, counts, retire, denoise, features, error, compute))
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
        r_any, n_got, c_word, r_word, d_word, dd_word, f_word, a_word, nm_word, dp_word, e_word, words = map(int, blocks)
        assert r_any * 4 == capi.retire_block_offset(nx, ny), ln
        if retire:
            assert r_word == r_any, ln
        if denoise:
            assert d_word * 4 == capi.denoise_block_offset(nx, ny, bool(counts), bool(retire)), ln
        if features:
            assert f_word * 4 == capi.features_block_offset(nx, ny, bool(squares), bool(counts), bool(retire), bool(denoise)), ln
            # the planes end where the frame ends (or, with the error flag, where the error plane's padding begins)
            assert (f_word + 16 + 7 * n) * 4 == capi.features_frame_bytes(nx, ny, bool(squares), bool(counts), bool(retire), bool(denoise)), ln
        # ... and field for field the binding's layout: absent parts are absent in both
        L = capi.FrameLayout(nx, ny, bool(squares), bool(counts), bool(retire), bool(denoise), bool(features), bool(error))
        have = (n_got, c_word, r_word, d_word, dd_word, f_word, a_word, nm_word, dp_word, e_word, words)
        ref = (L.n, L.counts, L.retire, L.denoise, L.denoised, L.features, L.albedo, L.normal, L.depth, L.error, L.words)
        assert have == tuple(-1 if v is None else v for v in ref), ln
        assert (e_word >= 0) == bool(error) and words * 4 == L.words * 4, ln
        if error:
            assert e_word * 4 == L.error * 4 and e_word % 2 == 0 and words == e_word + 3 * n, ln
            if features:
                assert words * 4 == capi.features_frame_bytes(nx, ny, True, bool(counts), bool(retire), True, error=True), ln
            else:
                assert words * 4 == capi.denoise_frame_bytes(nx, ny, bool(counts), bool(retire), error=True), ln
    assert seen == {(nx, ny) + c for nx, ny in SIZES for c in combos}


def test_upload_and_copy_back_extents(pkg, program_output):
    """upload_extents / copy_back_extents (csrc/rt_multi_planes.h) for every legal flag combination, other_ranks, begin and
    compute in {0, 1}: ascending, disjoint byte ranges inside the frame; nothing copied back covers a block's in-fields."""
    capi = pkg.capi
    lines = [ln for ln in program_output if ln.startswith("ext ")]
    combos = _combos()
    assert len(lines) == len(SIZES) * 33 * 8
    seen = set()
    for ln in lines:
        head, up, back = [part.split() for part in ln[4:].split(":")]
        nx, ny, bits, other, begin, compute = map(int, head)
        c = tuple((bits >> k) & 1 for k in range(6))
        assert c in combos, ln
        seen.add((nx, ny) + c + (other, begin, compute))
        L = capi.FrameLayout(nx, ny, *map(bool, c))
        in_fields = [(4 * at, 4 * at + getattr(cls, first_out).offset)
                     for at, cls, first_out in ((L.retire, capi.Retire, "active"), (L.denoise, capi.Denoise, "filtered"), (L.features, capi.Features, "traced"))
                     if at is not None]
        assert len(in_fields) == c[2] + c[3] + c[4] and all(hi > lo for lo, hi in in_fields), ln
        for name, ranges in (("upload", up), ("copy back", back)):
            r = [tuple(map(int, x.split("-"))) for x in ranges]
            assert all(lo < hi for lo, hi in r), (name, ln)
            assert all(a[1] <= b[0] for a, b in zip(r, r[1:])), (name, ln)       # ascending and disjoint
            assert all(0 <= lo and hi <= 4 * L.words for lo, hi in r), (name, ln)
            assert len(r) <= 6, (name, ln)
        for lo, hi in [tuple(map(int, x.split("-"))) for x in back]:
            assert all(hi <= f_lo or lo >= f_hi for f_lo, f_hi in in_fields), ln
        # the float planes always come back, and the in-fields of every block the frame has always travel up
        assert back and back[0].startswith("0-"), ln
        ups = [tuple(map(int, x.split("-"))) for x in up]
        assert all(any(lo <= f_lo and f_hi <= hi for lo, hi in ups) for f_lo, f_hi in in_fields), ln
    assert seen == {(nx, ny) + c + okc for nx, ny in SIZES for c in combos for okc in itertools.product((0, 1), repeat=3)}


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
