//! Raw bindings to the image textures of `librtiow_gpu.so`: the four entry points `include/rtiow_gpu_image.h` declares.
//!
//! A module of its own because `lib.rs` mirrors `include/rtiow_gpu.h` symbol for symbol, and the image kind is not part of that
//! header's ABI.  UNTESTED like the rest of the crate (no Rust toolchain in the build image);
//! `tests/test_image_texture_abi.py` compares the names and the argument counts with the header.
use std::os::raw::{c_float, c_int};

use crate::{rtg_builder, rtg_id, rtg_scene};

pub const RTG_IMAGE_PLANAR: u32 = 0;
pub const RTG_IMAGE_SPHERICAL: u32 = 1;
pub const RTG_IMAGE_NEAREST: u32 = 0;
pub const RTG_IMAGE_BILINEAR: u32 = 1;
pub const RTG_IMAGE_REPEAT: u32 = 0;
pub const RTG_IMAGE_CLAMP: u32 = 1;

/// `rtg_image_params`: how a point becomes (u, v) and how the texels are filtered.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rtg_image_params {
    /// `= size_of::<rtg_image_params>()`
    pub struct_size: u32,
    pub mapping: u32,
    pub filter: u32,
    pub wrap_u: u32,
    pub wrap_v: u32,
    /// must be 0
    pub reserved_in: u32,
    pub m: [c_float; 8],
}

extern "C" {
    pub fn rtg_texture_image(b: *mut rtg_builder, params: *const rtg_image_params, w: u32, h: u32, rgb: *const c_float) -> rtg_id;
    pub fn rtg_debug_texture_host(b: *mut rtg_builder, texture: rtg_id, n: usize, p: *const c_float, out: *mut c_float) -> c_int;
    pub fn rtg_debug_texture(s: *mut rtg_scene, texture: rtg_id, n: usize, p: *const c_float, out: *mut c_float) -> c_int;
    pub fn rtg_debug_atan2f_host(n: usize, y: *const c_float, x: *const c_float, out: *mut c_float) -> c_int;
}
