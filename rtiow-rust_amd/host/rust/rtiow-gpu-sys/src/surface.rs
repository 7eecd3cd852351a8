//! Raw bindings to the surface attributes of `librtiow_gpu.so`: the five entry points `include/rtiow_gpu_surface.h` declares --
//! per-vertex normals and UVs on triangles and meshes, and textures evaluated at a hit's surface coordinates.
//!
//! A module of its own because `lib.rs` mirrors `include/rtiow_gpu.h` symbol for symbol, and these calls are not part of that
//! header's ABI.  `normals9` / `uvs6` and `normals` / `uvs` may be null.  UNTESTED like the rest of the crate (no Rust toolchain
//! in the build image); `tests/test_surface_abi.py` compares the names and the argument counts with the header.
use std::os::raw::{c_float, c_int};

use crate::{rtg_builder, rtg_id, rtg_scene};

extern "C" {
    pub fn rtg_object_triangle_attr(b: *mut rtg_builder, v0: *const c_float, v1: *const c_float, v2: *const c_float, normals9: *const c_float, uvs6: *const c_float, material: rtg_id) -> rtg_id;
    pub fn rtg_object_mesh_attr(b: *mut rtg_builder, vertices: *const c_float, n_vertices: usize, indices: *const u32, n_triangles: usize, normals: *const c_float, uvs: *const c_float, material: rtg_id, sah: u32) -> rtg_id;
    pub fn rtg_texture_surface(b: *mut rtg_builder, child: rtg_id) -> rtg_id;
    pub fn rtg_debug_triangle_attr_host(n: usize, tri9: *const c_float, attr15: *const c_float, has: u32, rays8: *const c_float, t_min: c_float, out10: *mut c_float) -> c_int;
    pub fn rtg_debug_hit_surface(s: *mut rtg_scene, n: usize, rays7: *const c_float, seed: u64, t_near: c_float, out10: *mut c_float, mat: *mut u32) -> c_int;
}
