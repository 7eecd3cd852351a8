//! Raw bindings to the ray frames of `librtiow_gpu.so`: the two entry points `include/rtiow_gpu_rays.h` declares.
//!
//! A module of its own because `lib.rs` mirrors `include/rtiow_gpu.h` symbol for symbol, and ray frames are not part of that
//! header's ABI.  UNTESTED like the rest of the crate (no Rust toolchain in the build image);
//! `tests/test_ray_frame_abi.py` compares the names and the argument counts with the header.
use std::os::raw::{c_float, c_int, c_void};

use crate::{rtg_params, rtg_scene, rtg_stats};

/// `rays7` holds `nx * ny` rays: ray `p` starts every sample of pixel `p`.
pub const RTG_RAYS_PER_PIXEL: u32 = 0;
/// `rays7` holds `ns * nx * ny` rays, sample-major: sample `s` of pixel `p` at `s * nx * ny + p`.
pub const RTG_RAYS_PER_SAMPLE: u32 = 1;

extern "C" {
    pub fn rtg_par_cast_rays(s: *mut rtg_scene, rays7: *const c_float, ray_mode: u32, params: *const rtg_params, out_rgb: *mut c_float, stats_or_null: *mut rtg_stats) -> c_int;
    pub fn rtg_par_cast_rays_device(
        s: *mut rtg_scene,
        d_rays7: *const c_float,
        ray_mode: u32,
        params: *const rtg_params,
        d_out_rgb: *mut c_float,
        hip_stream: *mut c_void,
        stats_or_null: *mut rtg_stats,
    ) -> c_int;
}
