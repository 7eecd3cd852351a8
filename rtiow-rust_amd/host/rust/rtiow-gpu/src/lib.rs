//! Safe Rust side of the boundary: `gpu_cast(nx, ny, ns, &camera, world)` with the shape of the reference's
//! `par_cast(nx, ny, ns, &camera, world)` (cbiffle/rtiow-rust `src/lib.rs:363`).
//!
//! UNTESTED -- no Rust toolchain exists in the build image; this is the source a maintainer would start from.
//! The identical call sequence is exercised by the test-suite through C++ (`host/rtiow.hpp`, whose `par_cast` this file
//! transliterates) and ctypes (`capi.py`).
//!
//! How the reference plugs in: its objects are opaque `Box<dyn Object>` values, so `trait Object` (object.rs:15)
//! gains ONE method, `fn flatten(&self, b: &mut GpuBuilder) -> Result<ObjectId>`, with one-line impls that call the
//! builder method of the same name; `World` types implement [`FlattenWorld`].
use rtiow_gpu_sys as sys;
use std::ffi::CStr;
use std::ops::Range;
use std::ptr;

#[derive(Debug, Clone)]
pub struct Error {
    pub code: i32,
    pub message: String,
}
impl std::fmt::Display for Error {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "rtiow-gpu error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for Error {}
pub type Result<T> = std::result::Result<T, Error>;

fn last_error(code: i32) -> Error {
    // rtg_last_error() is thread-local and never null
    let message = unsafe { CStr::from_ptr(sys::rtg_last_error()) }.to_string_lossy().into_owned();
    Error { code, message }
}
fn check(rc: i32) -> Result<()> {
    if rc == sys::RTG_OK {
        Ok(())
    } else {
        Err(last_error(rc))
    }
}

#[derive(Copy, Clone, Debug, PartialEq, Eq)]
pub struct TextureId(sys::rtg_id);
#[derive(Copy, Clone, Debug, PartialEq, Eq)]
pub struct MaterialId(sys::rtg_id);
#[derive(Copy, Clone, Debug, PartialEq, Eq)]
pub struct ObjectId(sys::rtg_id);

/// object.rs:147-181 `StaticX / StaticY / StaticZ`
#[derive(Copy, Clone, Debug, PartialEq, Eq)]
pub enum Axis {
    X = 0,
    Y = 1,
    Z = 2,
}

pub type Vec3 = [f32; 3];

/// A scene under construction: one method per reference constructor.
pub struct GpuBuilder {
    raw: *mut sys::rtg_builder,
}
impl GpuBuilder {
    pub fn new() -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::rtg_builder_create(&mut raw) })?;
        Ok(GpuBuilder { raw })
    }
    fn id(&self, id: sys::rtg_id) -> Result<sys::rtg_id> {
        if id == sys::RTG_INVALID_ID {
            Err(last_error(sys::RTG_ERR_INVALID))
        } else {
            Ok(id)
        }
    }
    // texture.rs
    pub fn constant(&mut self, color: Vec3) -> Result<TextureId> {
        self.id(unsafe { sys::rtg_texture_constant(self.raw, color.as_ptr()) }).map(TextureId)
    }
    pub fn checker(&mut self, t0: TextureId, t1: TextureId) -> Result<TextureId> {
        self.id(unsafe { sys::rtg_texture_checker(self.raw, t0.0, t1.0) }).map(TextureId)
    }
    pub fn perlin(&mut self, scale: f32) -> Result<TextureId> {
        self.id(unsafe { sys::rtg_texture_perlin(self.raw, scale) }).map(TextureId)
    }
    /// perlin.rs:24-29 (the reference seeds these from thread_rng; any fixed tables are admissible)
    pub fn set_perlin_tables(&mut self, vecs: &[Vec3; 256], px: &[u8; 256], py: &[u8; 256], pz: &[u8; 256]) -> Result<()> {
        check(unsafe { sys::rtg_builder_set_perlin_tables(self.raw, vecs.as_ptr() as *const f32, px.as_ptr(), py.as_ptr(), pz.as_ptr()) })
    }
    // material.rs:10-39
    pub fn lambertian(&mut self, albedo: TextureId) -> Result<MaterialId> {
        self.id(unsafe { sys::rtg_material_lambertian(self.raw, albedo.0) }).map(MaterialId)
    }
    pub fn metal(&mut self, albedo: Vec3, fuzz: f32) -> Result<MaterialId> {
        self.id(unsafe { sys::rtg_material_metal(self.raw, albedo.as_ptr(), fuzz) }).map(MaterialId)
    }
    pub fn dielectric(&mut self, ref_idx: f32) -> Result<MaterialId> {
        self.id(unsafe { sys::rtg_material_dielectric(self.raw, ref_idx) }).map(MaterialId)
    }
    pub fn diffuse_light(&mut self, emission: TextureId, brightness: f32) -> Result<MaterialId> {
        self.id(unsafe { sys::rtg_material_diffuse_light(self.raw, emission.0, brightness) }).map(MaterialId)
    }
    pub fn isotropic(&mut self, albedo: TextureId) -> Result<MaterialId> {
        self.id(unsafe { sys::rtg_material_isotropic(self.raw, albedo.0) }).map(MaterialId)
    }
    // object.rs / bvh.rs
    pub fn sphere(&mut self, radius: f32, material: MaterialId) -> Result<ObjectId> {
        self.id(unsafe { sys::rtg_object_sphere(self.raw, radius, material.0) }).map(ObjectId)
    }
    pub fn rect(&mut self, orthogonal_to: Axis, range0: Range<f32>, range1: Range<f32>, k: f32, material: MaterialId) -> Result<ObjectId> {
        self.id(unsafe { sys::rtg_object_rect(self.raw, orthogonal_to as i32, range0.start, range0.end, range1.start, range1.end, k, material.0) })
            .map(ObjectId)
    }
    pub fn flip_normals(&mut self, object: ObjectId) -> Result<ObjectId> {
        self.id(unsafe { sys::rtg_object_flip_normals(self.raw, object.0) }).map(ObjectId)
    }
    pub fn translate(&mut self, offset: Vec3, object: ObjectId) -> Result<ObjectId> {
        self.id(unsafe { sys::rtg_object_translate(self.raw, offset.as_ptr(), object.0) }).map(ObjectId)
    }
    pub fn scale(&mut self, factor: Vec3, object: ObjectId) -> Result<ObjectId> {
        self.id(unsafe { sys::rtg_object_scale(self.raw, factor.as_ptr(), object.0) }).map(ObjectId)
    }
    pub fn rotate_y(&mut self, degrees: f32, object: ObjectId) -> Result<ObjectId> {
        self.id(unsafe { sys::rtg_object_rotate_y(self.raw, degrees, object.0) }).map(ObjectId)
    }
    pub fn and(&mut self, a: ObjectId, b: ObjectId) -> Result<ObjectId> {
        self.id(unsafe { sys::rtg_object_and(self.raw, a.0, b.0) }).map(ObjectId)
    }
    pub fn rect_prism(&mut self, p0: Vec3, p1: Vec3, material: MaterialId) -> Result<ObjectId> {
        self.id(unsafe { sys::rtg_object_rect_prism(self.raw, p0.as_ptr(), p1.as_ptr(), material.0) }).map(ObjectId)
    }
    pub fn linear_move(&mut self, object: ObjectId, motion: Vec3) -> Result<ObjectId> {
        self.id(unsafe { sys::rtg_object_linear_move(self.raw, object.0, motion.as_ptr()) }).map(ObjectId)
    }
    pub fn constant_medium(&mut self, boundary: ObjectId, density: f32, material: MaterialId) -> Result<ObjectId> {
        self.id(unsafe { sys::rtg_object_constant_medium(self.raw, boundary.0, density, material.0) }).map(ObjectId)
    }
    /// bvh::from_scene (bvh.rs:128): the library runs the same widest-axis median split over the leaves, in order.
    pub fn bvh(&mut self, objects: &[ObjectId], exposure: Range<f32>) -> Result<ObjectId> {
        let ids: Vec<sys::rtg_id> = objects.iter().map(|o| o.0).collect();
        self.id(unsafe { sys::rtg_object_bvh(self.raw, ids.as_ptr(), ids.len(), exposure.start, exposure.end) }).map(ObjectId)
    }
    /// Not in the reference: SAH split (same image up to exact-t ties, fewer Aabb tests).
    pub fn bvh_sah(&mut self, objects: &[ObjectId], exposure: Range<f32>) -> Result<ObjectId> {
        let ids: Vec<sys::rtg_id> = objects.iter().map(|o| o.0).collect();
        self.id(unsafe { sys::rtg_object_bvh_sah(self.raw, ids.as_ptr(), ids.len(), exposure.start, exposure.end) }).map(ObjectId)
    }
    /// Flatten `world` (the `[Box<dyn Object>]` of lib.rs:33, or a one-element list holding a Bvh) once into `device`'s HBM.
    pub fn scene(&self, world: &[ObjectId], device: i32) -> Result<GpuScene> {
        let ids: Vec<sys::rtg_id> = world.iter().map(|o| o.0).collect();
        let mut raw = ptr::null_mut();
        check(unsafe { sys::rtg_scene_create(self.raw, ids.as_ptr(), ids.len(), device, &mut raw) })?;
        Ok(GpuScene { raw })
    }
}
impl Drop for GpuBuilder {
    fn drop(&mut self) {
        unsafe { sys::rtg_builder_destroy(self.raw) }
    }
}

/// camera.rs:6-15; built by the library so that `tan` / rounding order match the GPU path's checker exactly.
#[derive(Copy, Clone, Debug)]
pub struct Camera(pub sys::rtg_camera);
impl Camera {
    /// Camera::look, camera.rs:18-50
    #[allow(clippy::too_many_arguments)]
    pub fn look(look_from: Vec3, look_at: Vec3, up: Vec3, fov: f32, aspect: f32, aperture: f32, focus_dist: f32, exposure: Range<f32>) -> Result<Camera> {
        let mut c = sys::rtg_camera::default();
        check(unsafe {
            sys::rtg_camera_look(look_from.as_ptr(), look_at.as_ptr(), up.as_ptr(), fov, aspect, aperture, focus_dist, exposure.start, exposure.end, &mut c)
        })?;
        Ok(Camera(c))
    }
}

/// A flattened scene resident in one GPU's HBM.  One frame in flight per scene; different scenes are independent.
pub struct GpuScene {
    raw: *mut sys::rtg_scene,
}
unsafe impl Send for GpuScene {}
impl Drop for GpuScene {
    fn drop(&mut self) {
        unsafe { sys::rtg_scene_destroy(self.raw) }
    }
}

/// lib.rs:321 `Image(Vec<Vec<Vec3>>)`: row 0 = top scanline (lib.rs:328), linear radiance.
pub struct Image {
    pub nx: usize,
    pub ny: usize,
    pub rgb: Vec<f32>,
}
impl Image {
    pub fn pixel(&self, x: usize, row: usize) -> Vec3 {
        let i = 3 * (row * self.nx + x);
        [self.rgb[i], self.rgb[i + 1], self.rgb[i + 2]]
    }
    /// print_ppm's per-channel quantisation (lib.rs:348-356), computed on `device`.
    pub fn to_u8(&self, device: i32) -> Result<Vec<u8>> {
        let mut out = vec![0u8; self.rgb.len()];
        check(unsafe { sys::rtg_tonemap(device, self.rgb.len(), self.rgb.as_ptr(), out.as_mut_ptr()) })?;
        Ok(out)
    }
}

/// What par_cast bakes in (bounce cap 50 at lib.rs:93, NEAR = 0.001 at lib.rs:35) plus the counter-RNG seed.
#[derive(Copy, Clone, Debug)]
pub struct CastOptions {
    pub seed: u64,
    pub max_bounces: u32,
    pub t_near: f32,
    /// `par_cast_denoised`: also ask for the error plane (`RTG_FLAG_DENOISE_ERROR`)
    pub denoise_error: bool,
}
impl Default for CastOptions {
    fn default() -> Self {
        CastOptions { seed: 0xDEAD_BEEF, max_bounces: 50, t_near: 0.001, denoise_error: false }
    }
}
fn params(nx: usize, ny: usize, ns: usize, o: &CastOptions) -> sys::rtg_params {
    sys::rtg_params {
        struct_size: std::mem::size_of::<sys::rtg_params>() as u32,
        nx: nx as u32,
        ny: ny as u32,
        ns: ns as u32,
        max_bounces: o.max_bounces,
        t_near: o.t_near,
        seed: o.seed,
        nranks: 1,
        ..Default::default()
    }
}

impl GpuScene {
    /// Scheduling / resource switches of this handle (`rtg_scene_set_option`; none changes a bit of the result): e.g.
    /// `("scratch_mb", 4096)` bounds the per-sample colour scratch (larger frames render in sample passes),
    /// `("frames_in_flight", 2)` lets two asynchronous frames of this handle overlap, `("force_rccl", 1)` sends
    /// `gpu_cast_multi` through the RCCL collective even on one device.  The one exception: `("light_sampling", 1)` renders
    /// with direct light sampling of the world's list-level rect lights -- another estimator of the same image, not the
    /// reference's samples (`include/rtiow_gpu.h`, at `rtg_scene_set_option`).
    pub fn set_option(&mut self, name: &str, value: i32) -> Result<()> {
        let c = std::ffi::CString::new(name).map_err(|_| last_error(sys::RTG_ERR_INVALID))?;
        check(unsafe { sys::rtg_scene_set_option(self.raw, c.as_ptr(), value) })
    }

    /// par_cast (lib.rs:363) on this scene's GPU.
    pub fn par_cast(&mut self, nx: usize, ny: usize, ns: usize, camera: &Camera, options: &CastOptions) -> Result<Image> {
        let mut rgb = vec![0f32; nx * ny * 3];
        let p = params(nx, ny, ns, options);
        check(unsafe { sys::rtg_par_cast(self.raw, &camera.0, &p, rgb.as_mut_ptr(), ptr::null_mut()) })?;
        Ok(Image { nx, ny, rgb })
    }

    /// Not in the reference: par_cast with `RTG_FLAG_SUM_SQUARES`.  Returns the image exactly as `par_cast` does and, in the
    /// same layout, the running sum of the squared sample colours of every pixel and channel (the input of a per-pixel
    /// standard error, see `standard_error`).
    pub fn par_cast_squares(&mut self, nx: usize, ny: usize, ns: usize, camera: &Camera, options: &CastOptions) -> Result<(Image, Vec<f32>)> {
        let n = nx * ny * 3;
        let mut planes = vec![0f32; 2 * n]; // plane 0: the image, plane 1: the sum of squares
        let mut p = params(nx, ny, ns, options);
        p.flags = sys::RTG_FLAG_SUM_SQUARES;
        check(unsafe { sys::rtg_par_cast(self.raw, &camera.0, &p, planes.as_mut_ptr(), ptr::null_mut()) })?;
        let sum_sq = planes.split_off(n);
        Ok((Image { nx, ny, rgb: planes }, sum_sq))
    }

    /// Not in the reference: par_cast with `RTG_FLAG_SAMPLE_COUNTS`.  `counts` (`nx * ny`, row 0 = top) gives every pixel its
    /// own sample count n_p: pixel p is `par_cast(nx, ny, min(n_p, ns), ..)` at p, bit for bit; pixels with n_p = 0 stay black.
    /// (Uncompiled, like the rest of this crate.)
    pub fn par_cast_counts(&mut self, nx: usize, ny: usize, ns: usize, counts: &[u32], camera: &Camera, options: &CastOptions) -> Result<Image> {
        let n = nx * ny;
        if counts.len() != n {
            return Err(Error { code: sys::RTG_ERR_INVALID, message: "par_cast_counts: counts must hold nx * ny values".into() });
        }
        let mut frame = vec![0f32; 4 * n]; // the image, then the count plane (u32 words)
        for (w, &c) in frame[3 * n..].iter_mut().zip(counts) {
            *w = f32::from_bits(c);
        }
        let mut p = params(nx, ny, ns, options);
        p.flags = sys::RTG_FLAG_SAMPLE_COUNTS;
        check(unsafe { sys::rtg_par_cast(self.raw, &camera.0, &p, frame.as_mut_ptr(), ptr::null_mut()) })?;
        frame.truncate(3 * n);
        Ok(Image { nx, ny, rgb: frame })
    }

    /// Not in the reference: adaptive sampling with the retire rule in the library (`RTG_FLAG_RETIRE`, see the header).  Every
    /// slice renders `step` more samples of the active pixels and retires, in the same call, those whose `(2 radius + 1)^2`
    /// window has every standard error `<= target_se` (once `k >= min_samples`).  Returns the running sums' frame resolved per
    /// pixel (pixel p = `par_cast(nx, ny, counts[p], ..)` at p, bit for bit), the samples each pixel got and the last slice's
    /// block.  (Uncompiled, like the rest of this crate.)
    pub fn par_cast_adaptive(&mut self, nx: usize, ny: usize, ns: usize, step: usize, target_se: f64, min_samples: u32, radius: u32,
                             camera: &Camera, options: &CastOptions) -> Result<(Image, Vec<u32>, sys::rtg_retire)> {
        if step == 0 {
            return Err(Error { code: sys::RTG_ERR_INVALID, message: "par_cast_adaptive: step must be > 0".into() });
        }
        let n = nx * ny;
        let block_word = (7 * n + 1) & !1; // planes, count plane, padding to 8 bytes, then the block
        let mut frame = vec![0f32; block_word + 16];
        for w in frame[6 * n..7 * n].iter_mut() {
            *w = f32::from_bits(ns as u32);
        }
        let mut block = sys::rtg_retire { target_se, min_samples, radius, ..Default::default() };
        unsafe { ptr::write_unaligned(frame.as_mut_ptr().add(block_word) as *mut sys::rtg_retire, block) };
        let mut done = 0;
        while done < ns {
            let end = ns.min(done + step);
            let mut p = params(nx, ny, end, options);
            p.flags = sys::RTG_FLAG_SUM_SQUARES | sys::RTG_FLAG_SAMPLE_COUNTS | sys::RTG_FLAG_RETIRE | sys::RTG_FLAG_PARTIAL | sys::RTG_FLAG_RESUME;
            p.sample_begin = done as u32;
            check(unsafe { sys::rtg_par_cast(self.raw, &camera.0, &p, frame.as_mut_ptr(), ptr::null_mut()) })?;
            done = end;
            block = unsafe { ptr::read_unaligned(frame.as_ptr().add(block_word) as *const sys::rtg_retire) };
            if block.active == 0 {
                break;
            }
        }
        // resolve a copy of plane 0 with the count plane: each pixel divided by the samples it holds
        let counts: Vec<u32> = frame[6 * n..7 * n].iter().map(|w| w.to_bits().min(done as u32)).collect();
        let mut pv = frame[..3 * n].to_vec();
        pv.extend(counts.iter().map(|&c| f32::from_bits(c)));
        let mut p = params(nx, ny, done, options);
        p.flags = sys::RTG_FLAG_SAMPLE_COUNTS | sys::RTG_FLAG_RESUME;
        p.sample_begin = done as u32;
        check(unsafe { sys::rtg_par_cast(self.raw, &camera.0, &p, pv.as_mut_ptr(), ptr::null_mut()) })?;
        pv.truncate(3 * n);
        Ok((Image { nx, ny, rgb: pv }, counts, block))
    }

    /// Not in the reference: par_cast with `RTG_FLAG_SUM_SQUARES | RTG_FLAG_DENOISE` (see the header): the image exactly as
    /// `par_cast` returns it, the frame filtered by the library's variance-driven non-local-means filter (strength `k`, search
    /// radius `radius`, patch radius `patch`), and the block with its out-fields.  (Uncompiled, like the rest of this crate.)
    /// With `options.denoise_error` the call sets `RTG_FLAG_DENOISE_ERROR` too and the last item is the error plane as an image of
    /// its own: the variance of every filtered pixel (+inf where a pixel was passed through); `None` without the option.
    pub fn par_cast_denoised(&mut self, nx: usize, ny: usize, ns: usize, k: f32, radius: u32, patch: u32, camera: &Camera,
                             options: &CastOptions) -> Result<(Image, Image, sys::rtg_denoise, Option<Image>)> {
        let n = nx * ny;
        let block_word = (6 * n + 1) & !1; // two planes, padding to 8 bytes, the block, then the output plane
        // (the error plane: on the first even word behind the output plane)
        let error_word = (block_word + 16 + 3 * n + 1) & !1;
        let mut frame = vec![0f32; if options.denoise_error { error_word + 3 * n } else { block_word + 16 + 3 * n }];
        let block = sys::rtg_denoise { k, radius, patch, ..Default::default() };
        unsafe { ptr::write_unaligned(frame.as_mut_ptr().add(block_word) as *mut sys::rtg_denoise, block) };
        let mut p = params(nx, ny, ns, options);
        p.flags = sys::RTG_FLAG_SUM_SQUARES | sys::RTG_FLAG_DENOISE | if options.denoise_error { sys::RTG_FLAG_DENOISE_ERROR } else { 0 };
        check(unsafe { sys::rtg_par_cast(self.raw, &camera.0, &p, frame.as_mut_ptr(), ptr::null_mut()) })?;
        let block = unsafe { ptr::read_unaligned(frame.as_ptr().add(block_word) as *const sys::rtg_denoise) };
        let denoised = frame[block_word + 16..block_word + 16 + 3 * n].to_vec();
        let error = if options.denoise_error { Some(Image { nx, ny, rgb: frame[error_word..error_word + 3 * n].to_vec() }) } else { None };
        frame.truncate(3 * n);
        Ok((Image { nx, ny, rgb: frame }, Image { nx, ny, rgb: denoised }, block, error))
    }

    /// Not in the reference: the same frame rendered `step` samples at a time (`RTG_FLAG_PARTIAL` / `RTG_FLAG_RESUME`).
    /// After each slice `on_preview(n_done, &preview)` gets the frame resolved at `n_done` samples -- bit-identical to
    /// `par_cast(nx, ny, n_done, ..)` -- and returns `false` to stop early (time budget, cancel).  The preview at
    /// `n_done == ns` is bit-identical to `par_cast(nx, ny, ns, ..)`.  Returns the samples rendered.
    pub fn progressive<F: FnMut(usize, &Image) -> bool>(&mut self, nx: usize, ny: usize, ns: usize, step: usize, camera: &Camera,
                                                         options: &CastOptions, mut on_preview: F) -> Result<usize> {
        if step == 0 {
            return Err(Error { code: sys::RTG_ERR_INVALID, message: "progressive: step must be > 0".into() });
        }
        let mut sum = vec![0f32; nx * ny * 3]; // the running sum of the samples so far
        let mut done = 0;
        while done < ns {
            let end = ns.min(done + step);
            let mut p = params(nx, ny, end, options);
            p.flags = sys::RTG_FLAG_PARTIAL | sys::RTG_FLAG_RESUME;
            p.sample_begin = done as u32;
            check(unsafe { sys::rtg_par_cast(self.raw, &camera.0, &p, sum.as_mut_ptr(), ptr::null_mut()) })?;
            done = end;
            let mut preview = Image { nx, ny, rgb: sum.clone() }; // the resolve step divides a copy
            let mut p = params(nx, ny, done, options);
            p.flags = sys::RTG_FLAG_RESUME;
            p.sample_begin = done as u32;
            check(unsafe { sys::rtg_par_cast(self.raw, &camera.0, &p, preview.rgb.as_mut_ptr(), ptr::null_mut()) })?;
            if !on_preview(done, &preview) {
                break;
            }
        }
        Ok(done)
    }
}

/// Standard error of a pixel channel's mean over `n` samples from its mean and its sum of squared samples
/// (`GpuScene::par_cast_squares`), in f64: s2 = max(0, (sum_sq - n m^2) / (n - 1)), se = sqrt(s2 / n); infinite for n = 1.
pub fn standard_error(mean: f32, sum_sq: f32, n: usize) -> f64 {
    if n < 2 {
        return f64::INFINITY;
    }
    let (m, q, nf) = (mean as f64, sum_sq as f64, n as f64);
    (((q - nf * m * m) / (nf - 1.0)).max(0.0) / nf).sqrt()
}

/// Implemented by the reference's `World` types (lib.rs:23-55): `[Box<dyn Object>]` flattens each object in order,
/// `Bvh` flattens its leaves and calls `GpuBuilder::bvh`.
pub trait FlattenWorld {
    fn flatten_world(&self, b: &mut GpuBuilder) -> Result<Vec<ObjectId>>;
}

/// Drop-in for `par_cast(nx, ny, ns, &camera, world)` (lib.rs:363): flatten once, render on GPU 0.
pub fn gpu_cast<W: FlattenWorld + ?Sized>(nx: usize, ny: usize, ns: usize, camera: &Camera, world: &W) -> Result<Image> {
    let mut b = GpuBuilder::new()?;
    let ids = world.flatten_world(&mut b)?;
    b.scene(&ids, 0)?.par_cast(nx, ny, ns, camera, &CastOptions::default())
}

/// The same on every GPU of the node: the world is flattened onto each device, pixel tiles are sharded over them and
/// ONE RCCL reduce(sum) of the float3 framebuffer (inside the library) assembles the frame -- bit-identical to `gpu_cast`.
pub fn gpu_cast_multi<W: FlattenWorld + ?Sized>(nx: usize, ny: usize, ns: usize, camera: &Camera, world: &W, n_devices: i32) -> Result<Image> {
    let mut b = GpuBuilder::new()?;
    let ids = world.flatten_world(&mut b)?;
    let scenes: Vec<GpuScene> = (0..n_devices).map(|d| b.scene(&ids, d)).collect::<Result<_>>()?;
    let raws: Vec<*mut sys::rtg_scene> = scenes.iter().map(|s| s.raw).collect();
    let mut rgb = vec![0f32; nx * ny * 3];
    let p = params(nx, ny, ns, &CastOptions::default());
    check(unsafe { sys::rtg_par_cast_multi(raws.as_ptr(), raws.len() as i32, &camera.0, &p, rgb.as_mut_ptr(), ptr::null_mut()) })?;
    Ok(Image { nx, ny, rgb })
}

/// The flagged frames over every GPU of the node (scene option `multi_planes` on the first handle; see the header at
/// `rtg_par_cast_multi`): `flags` are `RTG_FLAG_*` bits and `frame` the host frame of exactly the layout `rtg_par_cast` defines
/// for them, blocks' in-fields set by the caller.  Every plane is gathered on the first device, which retires, filters and
/// divides: the frame ends word for word as `rtg_par_cast` on one device leaves it.  (Uncompiled, like the rest of this crate.)
pub fn gpu_cast_multi_frame<W: FlattenWorld + ?Sized>(nx: usize, ny: usize, ns: usize, camera: &Camera, world: &W, n_devices: i32,
                                                      flags: u32, sample_begin: u32, frame: &mut [f32]) -> Result<()> {
    let mut b = GpuBuilder::new()?;
    let ids = world.flatten_world(&mut b)?;
    let mut scenes: Vec<GpuScene> = (0..n_devices).map(|d| b.scene(&ids, d)).collect::<Result<_>>()?;
    scenes[0].set_option("multi_planes", 1)?;
    let raws: Vec<*mut sys::rtg_scene> = scenes.iter().map(|s| s.raw).collect();
    let mut p = params(nx, ny, ns, &CastOptions::default());
    p.flags = flags;
    p.sample_begin = sample_begin;
    check(unsafe { sys::rtg_par_cast_multi(raws.as_ptr(), raws.len() as i32, &camera.0, &p, frame.as_mut_ptr(), ptr::null_mut()) })
}

/// `GpuScene::par_cast_denoised` over every GPU of the node: (image, filtered image, block), equal to the one-device call's.
pub fn gpu_cast_multi_denoised<W: FlattenWorld + ?Sized>(nx: usize, ny: usize, ns: usize, k: f32, radius: u32, patch: u32, camera: &Camera,
                                                         world: &W, n_devices: i32) -> Result<(Image, Image, sys::rtg_denoise)> {
    let n = nx * ny;
    let block_word = (6 * n + 1) & !1; // two planes, padding to 8 bytes, the block, then the output plane
    let mut frame = vec![0f32; block_word + 16 + 3 * n];
    let block = sys::rtg_denoise { k, radius, patch, ..Default::default() };
    unsafe { ptr::write_unaligned(frame.as_mut_ptr().add(block_word) as *mut sys::rtg_denoise, block) };
    gpu_cast_multi_frame(nx, ny, ns, camera, world, n_devices, sys::RTG_FLAG_SUM_SQUARES | sys::RTG_FLAG_DENOISE, 0, &mut frame)?;
    let block = unsafe { ptr::read_unaligned(frame.as_ptr().add(block_word) as *const sys::rtg_denoise) };
    let denoised = frame[block_word + 16..].to_vec();
    frame.truncate(3 * n);
    Ok((Image { nx, ny, rgb: frame }, Image { nx, ny, rgb: denoised }, block))
}

/// Forget the library's multi-GPU state: destroy the cached RCCL communicators, unload librccl (the next `gpu_cast_multi`
/// loads it again).  Returns the number of `ncclReduce` calls issued since the last reset.
pub fn multi_reset() -> Result<u64> {
    let mut n = 0u64;
    check(unsafe { sys::rtg_multi_reset(ptr::null(), &mut n) })?;
    Ok(n)
}

pub fn device_count() -> Result<i32> {
    let mut n = 0;
    check(unsafe { sys::rtg_device_count(&mut n) })?;
    Ok(n)
}
