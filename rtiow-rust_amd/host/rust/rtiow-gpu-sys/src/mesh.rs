//! Raw bindings to the triangles and meshes of `librtiow_gpu.so`: the three entry points `include/rtiow_gpu_mesh.h` declares.
//!
//! A module of its own because `lib.rs` mirrors `include/rtiow_gpu.h` symbol for symbol, and the triangle is not part of that
//! header's ABI.  UNTESTED like the rest of the crate (no Rust toolchain in the build image);
//! `tests/test_mesh_abi.py` compares the names and the argument counts with the header.
use std::os::raw::{c_float, c_int};

use crate::{rtg_builder, rtg_id};

extern "C" {
    pub fn rtg_object_triangle(b: *mut rtg_builder, v0: *const c_float, v1: *const c_float, v2: *const c_float, material: rtg_id) -> rtg_id;
    pub fn rtg_object_mesh(b: *mut rtg_builder, vertices: *const c_float, n_vertices: usize, indices: *const u32, n_triangles: usize, material: rtg_id, sah: u32) -> rtg_id;
    pub fn rtg_debug_triangle_host(n: usize, tri9: *const c_float, rays8: *const c_float, t_min: c_float, out8: *mut c_float) -> c_int;
}
