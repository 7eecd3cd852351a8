// rt_sphere_hit.h -- Sphere::hit (object.rs:84-111, sphere at the local origin) in two forms that give the same answer bit for
// bit: the reference form, literally the reference's two roots, and the one-division form of the lean pool's sphere pass.
// No HIP in here: the header compiles for the device (through rt_trace.h) and for the host (tests/test_sphere_one_divide.py
// builds a g++ program that compares the two forms).  V is any struct with float members x, y, z (rtg::V3 on the device).
// Compile with -ffp-contract=off, like everything that restates the reference's arithmetic.
#pragma once

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif

namespace rtg {

template <class V>
RT_HD float sphere_dot(V a, V b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }  // vec3.rs:43,100 (= vdot)

// The reference form, with a = dot(d, d) handed in: it depends on the ray alone, so a walk that keeps its ray in registers
// forms it once per ray (rt_pool.h, the refill) instead of once per sphere.
template <class V>
RT_HD bool sphere_hit_t_a(V o, V d, float a, float radius, float t0, float t1, float& t_out) {
  float b = sphere_dot(o, d);
  float c = sphere_dot(o, o) - radius * radius;
  float disc = b * b - a * c;
  if (disc > 0.f) {
    float sq = __builtin_sqrtf(disc);
    float t = (-b - sq) / a;
    if (t < t1 && t >= t0) {
      t_out = t;
      return true;
    }
    t = (-b + sq) / a;
    if (t < t1 && t >= t0) {
      t_out = t;
      return true;
    }
  }
  return false;
}

// The one-division form.  Same b, c, disc, sq and the same two numerators n1 = -b - sq, n2 = -b + sq as above; the reference's
// roots are r1 = RN(n1 / a) and r2 = RN(n2 / a), and it returns r1 if r1 is in [t0, t1), else r2 if r2 is, else nothing.  Here
// a lane divides ONE numerator -- n1 where r1 can still be accepted, n2 where r1 is refused whatever it is -- and divides a
// second time only in the arm that is the reference's own code.  `t0_pos` is the caller's WAVE-UNIFORM `t0 > 0` (the lean pool
// forms it once per launch from P.t_near, on the scalar unit): claim 1 needs it, and without it `first` is true for every
// lane, which leaves claim 2 and the slow arm -- both hold for any t0 -- so the form is the reference's for every launch.
//
// Facts used below.  a = dot(d, d) is a rounded sum of three squares: a >= +0, +inf or NaN, never negative and never -0.
// Past `disc > 0`, disc is a positive number or +inf, so sq = sqrt(disc) is > 0 or +inf and no NaN.  A correctly rounded
// quotient x / a is monotone non-decreasing in x for a fixed a >= +0 wherever both quotients are numbers (rounding is
// monotone; for a = 0 the quotients are -inf / +inf by the sign of x, for a = +inf they are -0 / +0); comparisons do not tell
// -0 from +0, and every comparison with a NaN is false.
//
// Claim 1 (t0 > 0): a lane with first == false has r1 outside [t0, t1).  !(n1 >= 0) means n1 < 0 or n1 is NaN (n1 = -0 is
//   `first`).  n1 < 0 divided by a gives: a negative number or -0 (a finite > 0, or the quotient underflows), -0 (a = +inf, n1
//   finite), -inf (a = +0), NaN (a = +inf with n1 = -inf, or a NaN) -- each fails `>= t0` because t0 > 0.  A NaN n1 gives a
//   NaN r1, which fails too.  So the reference goes on to r2 = RN(n2 / a), which is the q of this lane: `hit iff in, t = q`.
// Claim 2 (any t0): a lane with first == true and q = r1 >= t1 has no hit.  r1 >= t1 says r1 is no NaN, so neither n1 nor a
//   is, and r1 fails `< t1`: the reference goes on to r2.  n1 = RN(-b - sq) and n2 = RN(-b + sq) with sq >= 0: -b - sq <=
//   -b + sq in the extended reals where both are defined, rounding is monotone, so n1 <= n2 -- or n2 is NaN (b = +inf, sq =
//   +inf).  Then r2 is NaN, or r2 >= r1 >= t1 by the monotone quotient; either way r2 fails `< t1`.
// A `first` lane with r1 in [t0, t1) returns r1 as the reference does.  Every other `first` lane -- r1 < t0, or r1 a NaN (a = 0
// with n1 = 0, a = inf with n1 = inf) -- runs the reference's second division and test literally: that arm needs no claim.
// In every arm t_out is the quotient of the same two floats the reference divides: the same bits, signed zeros included.
// `arm` (host tests; the device passes none): 0 = no real roots, 1 = first root accepted, 2 = first root refused by `q >= t1`,
// 3 = the slow arm, 4 = second numerator divided directly.
template <class V>
RT_HD bool sphere_hit_t_a_1div(V o, V d, float a, float radius, float t0, float t1, bool t0_pos, float& t_out, int* arm = nullptr) {
  float b = sphere_dot(o, d);
  float c = sphere_dot(o, o) - radius * radius;
  float disc = b * b - a * c;
  if (disc > 0.f) {
    float sq = __builtin_sqrtf(disc);
    const float n1 = -b - sq, n2 = -b + sq;
    const bool first = !t0_pos || n1 >= 0.f;  // (false for a NaN n1 when t0 > 0)
    const float q = (first ? n1 : n2) / a;
    if (arm) *arm = first ? 2 : 4;
    if (q < t1 && q >= t0) {  // first: the reference's first root; !first: its second, the first being refused (claim 1)
      if (arm && first) *arm = 1;
      t_out = q;
      return true;
    }
    if (first && !(q >= t1)) {  // r1 < t0 or NaN; (first && q >= t1: no hit, claim 2)
      if (arm) *arm = 3;
      const float q2 = n2 / a;
      if (q2 < t1 && q2 >= t0) {
        t_out = q2;
        return true;
      }
    }
  }
  return false;
}

}  // namespace rtg
