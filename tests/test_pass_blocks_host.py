"""csrc/rt_device.h on the host: the SCATTER pass's shared form of the attempts (in_unit_sphere_tries_shared + next_u32_primed)
hands every consumer the same words in the same order as the lazy form (set_event, seek, in_unit_sphere_tries / gen_f32), with
the same `draws`, over a few million seeded (seed, pixel, sample, event, tries) tuples.

rt_device.h is device code (it includes the HIP runtime header for `__device__` and the bit casts, and so does rt_libm.h), so the
g++ program below is compiled against a stand-in `hip/hip_runtime.h` of a dozen lines that this test writes next to it: the
qualifiers expand to nothing and the bit casts to memcpy.  Nothing of HIP is needed to run SampleRng -- Philox is integer
arithmetic -- and the program is built plainly and with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtiow-rust_amd", "csrc")

HIP_STAND_IN = r"""
#pragma once
#include <stdint.h>
#include <string.h>
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline long long __double_as_longlong(double d) { long long u; memcpy(&u, &d, 8); return u; }
static inline double __longlong_as_double(long long u) { double d; memcpy(&d, &u, 8); return d; }
"""

PROGRAM = r"""
#include "rt_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
using namespace rtg;

static uint64_t state;
static uint64_t next64() {  // splitmix64
  uint64_t z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 1000000;
  state = 0xDEADBEEFull;
  long deferred = 0, found_late = 0, glass = 0, longest = 0;
  for (long i = 0; i < n; i++) {
    const uint64_t seed = next64();
    const uint64_t r = next64();
    const uint32_t pixel = (uint32_t)r % (1200u * 800u), sample = (uint32_t)(r >> 32) % 500u;
    const uint64_t q = next64();
    const uint32_t event = 1u + (uint32_t)q % 51u, tries = (uint32_t)(q >> 32) & 3u;
    const bool wanted = ((q >> 40) & 3u) != 0u;      // a quarter of the lanes are Dielectric ones
    const bool refracted = ((q >> 42) & 1u) != 0u;   // ... half of which draw
    const uint32_t max_tries = tries < 3u ? 4u : 0xffffffffu;
    // the lazy form: what the pass did before
    SampleRng a;
    a.init(seed, pixel, sample);
    a.set_event(event);
    a.seek(12u * tries);
    V3 va = mk(0.f, 0.f, 0.f);
    bool fa = false;
    float da = -1.f;
    if (wanted) fa = in_unit_sphere_tries(a, max_tries, va);
    else if (refracted) da = a.gen_f32();
    // the shared form
    SampleRng b;
    b.init(seed, pixel, sample);
    b.set_event(event);
    b.seek(12u * tries);
    V3 vb = mk(0.f, 0.f, 0.f);
    float db = -1.f;
    const bool fb = in_unit_sphere_tries_shared(b, wanted, max_tries, vb);
    if (!wanted && refracted) db = b.gen_f32_primed();
    if (fa != fb || bits(va.x) != bits(vb.x) || bits(va.y) != bits(vb.y) || bits(va.z) != bits(vb.z) || bits(da) != bits(db) || a.draws != b.draws) {
      printf("MISMATCH at tuple %ld: seed %llx pixel %u sample %u event %u tries %u wanted %d refracted %d: found %d / %d, draws %u / %u\n", i,
             (unsigned long long)seed, pixel, sample, event, tries, (int)wanted, (int)refracted, (int)fa, (int)fb, a.draws, b.draws);
      return 1;
    }
    // the words of the shared block that are still unread are the lazy stream's next ones, in order
    if (!wanted) {
      for (int k = refracted ? 1 : 0; k < 4; k++)
        if (a.next_u32() != b.next_u32_primed() || a.draws != b.draws) { printf("MISMATCH in word %d of the block at tuple %ld\n", k, i); return 1; }
      if (b.left != 0u) { printf("MISMATCH: %u words left behind the fourth at tuple %ld\n", b.left, i); return 1; }
      glass++;
    }
    deferred += wanted && !fa;
    found_late += wanted && fa && a.draws > 12u;
    if ((long)a.draws > longest) longest = (long)a.draws;
  }
  printf("OK %ld tuples: %ld Dielectric, %ld deferred after four attempts, %ld found behind the twelfth draw, longest %ld draws\n", n, glass, deferred, found_late, longest);
  return (deferred > 0 && found_late > 0 && glass > 0) ? 0 : 2;
}
"""


def _build(tmp_path, name, extra):
    (tmp_path / "hip").mkdir(exist_ok=True)
    (tmp_path / "hip" / "hip_runtime.h").write_text(HIP_STAND_IN)
    src = tmp_path / "pass_blocks.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-attributes", "-I", str(tmp_path), "-I", CSRC] + extra +
                          [str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("name,extra,n", [("plain", ["-O2"], 3000000),
                                          ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 1000000)])
def test_shared_form_hands_out_the_lazy_forms_words(tmp_path, name, extra, n):
    exe = _build(tmp_path, name, extra)
    out = subprocess.run([exe, str(n)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout
