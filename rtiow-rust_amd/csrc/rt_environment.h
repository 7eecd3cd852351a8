// rt_environment.h -- the environment's direction mapping (include/rtiow_gpu_environment.h), ONE host-and-device function: the miss
// branches of the textured kernels call it on the GPU (rt_trace.h environment_colour), rtg_debug_environment_host calls the very
// same source on the host, and rtiow-rust_amd/environment.py direction() is the same arithmetic in numpy, bit for bit.  Compile
// with -ffp-contract=off: every operation is rounded on its own.
#pragma once
#include "rt_libm.h"

namespace rtg {

// q for the direction d of a ray that left the scene: u = d / |d| (vec3.rs:66: one sqrt, three divides), then RotateY's rot()
// (object.rs:349-355) with the pair (s, c), every product of the three dot products written out (a zero factor still turns an
// infinity or a NaN into a NaN, as in the reference's rot()).
RT_LIBM_HD inline void environment_direction(float dx, float dy, float dz, float s, float c, float q[3]) {
  const float len = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
  const float ux = dx / len, uy = dy / len, uz = dz / len;
  q[0] = (ux * c + uy * 0.f) + uz * s;
  q[1] = (ux * 0.f + uy * 1.f) + uz * 0.f;
  q[2] = (ux * (-s) + uy * 0.f) + uz * c;
}

}  // namespace rtg
