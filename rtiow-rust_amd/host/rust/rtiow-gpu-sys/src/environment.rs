//! Raw bindings to the scene's environment of `librtiow_gpu.so`: the four entry points `include/rtiow_gpu_environment.h` declares.
//!
//! A module of its own because `lib.rs` mirrors `include/rtiow_gpu.h` symbol for symbol, and the environment is not part of that
//! header's ABI.  UNTESTED like the rest of the crate (no Rust toolchain in the build image);
//! `tests/test_environment_abi.py` compares the names and the argument counts with the header.
use std::os::raw::{c_float, c_int};

use crate::{rtg_builder, rtg_id, rtg_scene};

/// `rtg_environment_params`: the texture a ray that leaves the scene sees, its scale and its rotation about world +y.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rtg_environment_params {
    /// `= size_of::<rtg_environment_params>()`
    pub struct_size: u32,
    /// `RTG_INVALID_ID` clears the environment
    pub texture: rtg_id,
    pub scale: [c_float; 3],
    pub rotate_y_degrees: c_float,
    /// must be 0
    pub reserved_in: [u32; 2],
}

extern "C" {
    pub fn rtg_builder_set_environment(b: *mut rtg_builder, p: *const rtg_environment_params) -> c_int;
    pub fn rtg_builder_get_environment(b: *const rtg_builder, out: *mut rtg_environment_params, sin_cos: *mut c_float) -> c_int;
    pub fn rtg_debug_environment_host(b: *mut rtg_builder, n: usize, d: *const c_float, out: *mut c_float) -> c_int;
    pub fn rtg_debug_environment(s: *mut rtg_scene, n: usize, d: *const c_float, out: *mut c_float) -> c_int;
}
