"""The walks of the lean query kernel (csrc/rt_query_walk.h: the closest walk and the any-hit walk, the source the device
kernel steps through), without a GPU: a stand-alone g++ program (-ffp-contract=off) includes the header, reads the flat words
of a lean world, a ray set and the ORACLE's debug_hit_top answer from files, and checks

  closest   every output word and every material equal to the oracle's (NaNs count as equal);
  any-hit   with t* the oracle's t:  t_max = F32_MAX -> exactly the hit flag;  t_max = t* -> exactly 0;  t_max = 0.5 t*
            (t* > 0) -> exactly 0.  Both walks run the same box tests until the first hit, and an any-hit answer of 1 implies a
            closest t < t_max, so these three are exact.
            t_max = 2 t*: occluded => (hit and t* < t_max) for every ray.  The converse can fail only where a box test with
            end = t_max rounds differently from one with end = best; the program counts those rays, and the cap is 0.1 % of
            the rays with a hit.

Worlds: the scene cases book1 and book1_sah and every lean world the box-plan tests walk (test_box_prune.WORLD_NAMES: hand
built, domes, fuzz, big_lean, the list world).  Rays: probe_rays("book1") -- random and edge cases: zero components, -0,
1e30 / 1e-30 directions, d = 0 -- plus probe_rays("book1", n_random=2048, seed=99).  The program runs plain at -O2 and with
the address and undefined-behaviour sanitizers linked into it.

Recorded: over all worlds and both builds the converse of the t_max = 2 t* rule failed for 0 rays (the figure the test prints)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from probe_rays import probe_rays
from scene_cases import CASES
from test_box_prune import WORLD_NAMES, _worlds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtiow-rust_amd", "csrc")
SEED, T_MIN = 77, 0.001
CAP = 0.001   # of the rays with a hit: the converse of the t_max = 2 t* rule

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rt_query_walk.h"
struct V3 { float x, y, z; };
struct Rec { uint32_t x, y, z, w; };
template <class T>
static std::vector<T> slurp(const char* path) {
  std::vector<T> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::printf("cannot open %s\n", path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / sizeof(T));
  if (bytes && std::fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) { std::printf("short read %s\n", path); std::exit(2); }
  std::fclose(f);
  return v;
}
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const float t_min = (float)std::atof(argv[5]);
  const std::vector<uint32_t> words = slurp<uint32_t>(argv[1]);
  const std::vector<float> rays = slurp<float>(argv[2]);
  const std::vector<float> want = slurp<float>(argv[3]);
  const std::vector<uint32_t> want_mat = slurp<uint32_t>(argv[4]);
  const uint32_t n = (uint32_t)(words.size() / 8);
  const size_t n_rays = rays.size() / 7;
  if (words.size() % 8 || rays.size() % 7 || want.size() != 8 * n_rays || want_mat.size() != n_rays) { std::printf("bad sizes\n"); return 2; }
  std::vector<Rec> lo(n), hi(n);
  for (uint32_t i = 0; i < n; i++) {
    std::memcpy(&lo[i], &words[8 * i], 16), std::memcpy(&hi[i], &words[8 * i + 4], 16);
    const uint32_t op = hi[i].w & 0xffu;
    if (op != rtg::OP_BOX && op != rtg::OP_SPHERE && op != rtg::OP_END) { std::printf("record %u: op %u is not lean\n", i, op); return 2; }
  }
  long hits = 0, diffs = 0, bad_max = 0, bad_at = 0, bad_half = 0, bad_two = 0, converse = 0;
  for (size_t i = 0; i < n_rays; i++) {
    const float* r = &rays[7 * i];
    const rtg::QueryRay<V3> q = rtg::query_ray<V3>(r[0], r[1], r[2], r[3], r[4], r[5], t_min);
    float out[8];
    uint32_t mat = 0;
    rtg::query_closest_walk(lo.data(), hi.data(), n, q, out, &mat);
    bool same = mat == want_mat[i];
    for (int k = 0; k < 8; k++) same = same && (bits(out[k]) == bits(want[8 * i + k]) || (out[k] != out[k] && want[8 * i + k] != want[8 * i + k]));
    if (!same && diffs++ < 5)
      std::printf("DIFF ray %zu: got %a %a %a %a mat %u, want %a %a %a %a mat %u\n", i, out[0], out[1], out[2], out[5], mat, want[8 * i], want[8 * i + 1],
                  want[8 * i + 2], want[8 * i + 5], want_mat[i]);
    const bool hit = want[8 * i] != 0.f;
    const float ts = want[8 * i + 1];
    hits += hit;
    if (rtg::query_occluded_walk(lo.data(), hi.data(), n, q, rtg::QUERY_F32_MAX) != hit) bad_max++;
    if (rtg::query_occluded_walk(lo.data(), hi.data(), n, q, ts)) bad_at++;
    if (ts > 0.f && rtg::query_occluded_walk(lo.data(), hi.data(), n, q, 0.5f * ts)) bad_half++;
    const float two = 2.f * ts;
    const bool occ = rtg::query_occluded_walk(lo.data(), hi.data(), n, q, two);
    if (occ && !(hit && ts < two)) bad_two++;
    if (!occ && hit && ts < two && two > t_min) converse++;
  }
  std::printf("rays %zu records %u hits %ld diffs %ld bad_max %ld bad_at %ld bad_half %ld bad_two %ld converse %ld\n", n_rays, n, hits, diffs, bad_max,
              bad_at, bad_half, bad_two, converse);
  return 0;
}
"""


def _world_fn(pkg, name):
    if name in CASES:
        return lambda p, b: CASES[name][0](p, b, CASES[name][1], CASES[name][2])[0]
    return _worlds(pkg)[name]


NAMES = ["book1", "book1_sah"] + WORLD_NAMES


@pytest.fixture(scope="module")
def rays():
    return np.concatenate([probe_rays("book1"), probe_rays("book1", n_random=2048, seed=99)])


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the stand-alone walk program")
    d = tmp_path_factory.mktemp("query_walk")
    src = d / "query_walk.cpp"
    src.write_text(PROGRAM)
    exes = {}
    for name, extra in (("plain", ["-O2"]),
                        ("san", ["-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined"])):
        exes[name] = d / ("query_walk_" + name)
        subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"] + extra
                              + ["-I", CSRC, str(src), "-o", str(exes[name])])
    return d, exes


@pytest.fixture(scope="module")
def totals():
    return {"hits": 0, "converse": 0, "worlds": 0}


@pytest.mark.parametrize("name", NAMES)
def test_walks_against_the_oracle(pkg, oracle, programs, rays, totals, name):
    d, exes = programs
    fn = _world_fn(pkg, name)
    b = pkg.load().builder()
    words, feat = b.flatten(fn(pkg, b))
    assert feat == 0, name
    ob = oracle.builder()
    want, want_mat = ob.scene(fn(pkg, ob)).debug_hit_top(rays, seed=SEED, t_near=T_MIN)
    paths = {}
    for key, arr in (("words", np.ascontiguousarray(words, np.uint32)), ("rays", rays), ("want", want), ("mat", want_mat)):
        paths[key] = d / ("%s_%s.bin" % (name, key))
        arr.tofile(str(paths[key]))
    for build, exe in exes.items():
        r = subprocess.run([str(exe), str(paths["words"]), str(paths["rays"]), str(paths["want"]), str(paths["mat"]), repr(T_MIN)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        last = r.stdout.splitlines()[-1].split()
        print(name, build, " ".join(last))
        got = dict(zip(last[0::2], map(int, last[1::2])))
        assert got["rays"] == len(rays) and got["records"] == len(words)
        assert got["diffs"] == 0, r.stdout[-2000:]
        assert got["bad_max"] == 0 and got["bad_at"] == 0 and got["bad_half"] == 0 and got["bad_two"] == 0, got
        assert got["converse"] <= CAP * got["hits"], got
    totals["hits"] += got["hits"]
    totals["converse"] += got["converse"]
    totals["worlds"] += 1


def test_the_ray_sets_hit_and_miss(totals):
    """(runs last: what the fixed sets covered, and the converse count the docstring records)"""
    print("worlds %d, rays with a hit %d, converse failures of the t_max = 2 t* rule %d" % (totals["worlds"], totals["hits"], totals["converse"]))
    assert totals["worlds"] == len(NAMES) and totals["hits"] > 1000
    assert totals["converse"] <= CAP * totals["hits"]
