// rtiow.hpp -- C++ spelling of the reference crate's surface over the C ABI (include/rtiow_gpu.h), so
// scene code from the reference's src/lib.rs / src/main.rs transliterates line for line:
//
//   Rust                                               C++
//   Box::new(object::Translate { offset, object })     boxed(object::Translate{offset, object})
//   object::Sphere { radius: 50., material: glass }    object::Sphere{50.f, glass}
//   object::Rect { orthogonal_to: StaticY, range0: 123. ..423., range1: 147. ..412., k: 554., material }
//                                                      object::Rect<StaticY>{{123.f,423.f},{147.f,412.f},554.f,material}
//   object::rotate_y(15., bvh)                         object::rotate_y(15.f, bvh)
//   bvh::from_scene(boxes, exposure)                   bvh::from_scene(std::move(boxes), exposure)
//   Camera::look(from, at, up, fov, aspect, ap, fd, exposure)   same
//   par_cast(NX, NY, NS, &camera, world)               par_cast(NX, NY, NS, camera, world)
//
// Objects are plain value types (like the Rust structs); they become builder handles only when
// par_cast flattens the world, mirroring how a Rust `-sys` binding would add `fn flatten(&self, b)`
// to `trait Object`.  The reference's panics surface as rtiow::Error.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rtiow_gpu.h"
#include "../../include/rtiow_gpu_environment.h"
#include "../../include/rtiow_gpu_image.h"
#include "../../include/rtiow_gpu_mesh.h"

namespace rtiow {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
  if (rc != RTG_OK) throw Error(rc, rtg_last_error());
}
inline rtg_id check_id(rtg_id id) {
  if (id == RTG_INVALID_ID) throw Error(RTG_ERR_INVALID, rtg_last_error());
  return id;
}

// vec3.rs:13 -- only what scene construction needs (the hot-path arithmetic lives on the GPU)
struct Vec3 {
  float x = 0, y = 0, z = 0;
  Vec3() = default;
  Vec3(float a, float b, float c) : x(a), y(b), z(c) {}
  static Vec3 from(float v) { return Vec3(v, v, v); }
  const float* data() const { return &x; }
};
inline Vec3 operator+(Vec3 a, Vec3 b) { return Vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline Vec3 operator*(float s, Vec3 v) { return Vec3(s * v.x, s * v.y, s * v.z); }
inline Vec3 operator+(float s, Vec3 v) { return Vec3(s + v.x, s + v.y, s + v.z); }
inline Vec3 operator*(Vec3 a, Vec3 b) { return Vec3(a.x * b.x, a.y * b.y, a.z * b.z); }

struct Range {  // std::ops::Range<f32>
  float start, end;
};

// texture.rs:6 `Texture = Arc<dyn Fn(Vec3)->Vec3>`: closed here (H3: closures cannot be flattened)
struct Texture {
  std::function<rtg_id(rtg_builder*)> emit;
};
namespace texture {
inline Texture constant(Vec3 c) {
  return Texture{[c](rtg_builder* b) { return check_id(rtg_texture_constant(b, c.data())); }};
}
inline Texture checker(Texture t0, Texture t1) {
  return Texture{[t0, t1](rtg_builder* b) { return check_id(rtg_texture_checker(b, t0.emit(b), t1.emit(b))); }};
}
inline Texture perlin(float scale) {
  return Texture{[scale](rtg_builder* b) { return check_id(rtg_texture_perlin(b, scale)); }};
}
// Not in the reference (include/rtiow_gpu_image.h): w x h texels of three floats, row-major, row 0 at the top, looked up through
// `params` (mapping, filter, wraps and the eight mapping floats; struct_size is filled in here).  The texels are shared, not
// copied, until the scene is built.
inline Texture image(rtg_image_params params, uint32_t w, uint32_t h, std::vector<float> rgb) {
  if (rgb.size() != (size_t)w * h * 3) throw Error(RTG_ERR_INVALID, "texture::image: rgb must hold w * h * 3 floats");
  params.struct_size = sizeof(rtg_image_params);
  auto texels = std::make_shared<const std::vector<float>>(std::move(rgb));
  return Texture{[params, w, h, texels](rtg_builder* b) { return check_id(rtg_texture_image(b, &params, w, h, texels->data())); }};
}
}  // namespace texture

// material.rs:10-39
struct Material {
  std::function<rtg_id(rtg_builder*)> emit;
  static Material Lambertian(Texture albedo) {
    return Material{[albedo](rtg_builder* b) { return check_id(rtg_material_lambertian(b, albedo.emit(b))); }};
  }
  static Material Metal(Vec3 albedo, float fuzz) {
    return Material{[albedo, fuzz](rtg_builder* b) { return check_id(rtg_material_metal(b, albedo.data(), fuzz)); }};
  }
  static Material Dielectric(float ref_idx) {
    return Material{[ref_idx](rtg_builder* b) { return check_id(rtg_material_dielectric(b, ref_idx)); }};
  }
  static Material DiffuseLight(Texture emission, float brightness) {
    return Material{[emission, brightness](rtg_builder* b) {
      return check_id(rtg_material_diffuse_light(b, emission.emit(b), brightness));
    }};
  }
  static Material Isotropic(Texture albedo) {
    return Material{[albedo](rtg_builder* b) { return check_id(rtg_material_isotropic(b, albedo.emit(b))); }};
  }
};

// `Box<dyn Object>` (object.rs:42): type-erased object that knows how to flatten itself
struct BoxedObject {
  std::function<rtg_id(rtg_builder*)> emit;
};
template <class O>
BoxedObject boxed(O o) {
  return BoxedObject{[o](rtg_builder* b) { return o.flatten(b); }};
}
using Scene = std::vector<BoxedObject>;  // Vec<Box<dyn Object>>

struct StaticX { static constexpr int AXIS = 0; };
struct StaticY { static constexpr int AXIS = 1; };
struct StaticZ { static constexpr int AXIS = 2; };

namespace object {
struct Sphere {  // object.rs:75-80
  float radius;
  Material material;
  rtg_id flatten(rtg_builder* b) const { return check_id(rtg_object_sphere(b, radius, material.emit(b))); }
};
template <class A>
struct Rect {  // object.rs:131-144
  Range range0, range1;
  float k;
  Material material;
  rtg_id flatten(rtg_builder* b) const {
    return check_id(rtg_object_rect(b, A::AXIS, range0.start, range0.end, range1.start, range1.end, k, material.emit(b)));
  }
};
template <class O>
struct FlipNormals {  // object.rs:239
  O object;
  rtg_id flatten(rtg_builder* b) const { return check_id(rtg_object_flip_normals(b, object.flatten(b))); }
};
template <class O>
FlipNormals<O> flip_normals(O o) { return FlipNormals<O>{std::move(o)}; }
template <class O>
struct Translate {  // object.rs:262-265
  Vec3 offset;
  O object;
  rtg_id flatten(rtg_builder* b) const { return check_id(rtg_object_translate(b, offset.data(), object.flatten(b))); }
};
template <class O>
Translate(Vec3, O) -> Translate<O>;
template <class O>
struct Scale {  // object.rs:296-299
  Vec3 factor;
  O object;
  rtg_id flatten(rtg_builder* b) const { return check_id(rtg_object_scale(b, factor.data(), object.flatten(b))); }
};
template <class O>
Scale(Vec3, O) -> Scale<O>;
template <class O>
struct RotateY {  // object.rs:335-339; built by rotate_y
  O object;
  float degrees;
  rtg_id flatten(rtg_builder* b) const { return check_id(rtg_object_rotate_y(b, degrees, object.flatten(b))); }
};
template <class O>
RotateY<O> rotate_y(float degrees, O o) { return RotateY<O>{std::move(o), degrees}; }  // object.rs:477
template <class T, class S>
struct And {  // object.rs:394
  T first;
  S second;
  rtg_id flatten(rtg_builder* b) const { return check_id(rtg_object_and(b, first.flatten(b), second.flatten(b))); }
};
template <class T, class S>
And(T, S) -> And<T, S>;
struct RectPrism {  // object.rs:420-473 rect_prism
  Vec3 p0, p1;
  Material material;
  rtg_id flatten(rtg_builder* b) const {
    return check_id(rtg_object_rect_prism(b, p0.data(), p1.data(), material.emit(b)));
  }
};
inline RectPrism rect_prism(Vec3 p0, Vec3 p1, Material m) { return RectPrism{p0, p1, std::move(m)}; }
template <class O>
struct LinearMove {  // object.rs:489-494
  O object;
  Vec3 motion;
  rtg_id flatten(rtg_builder* b) const { return check_id(rtg_object_linear_move(b, object.flatten(b), motion.data())); }
};
template <class O>
LinearMove(O, Vec3) -> LinearMove<O>;
template <class O>
struct ConstantMedium {  // object.rs:533-541
  O boundary;
  float density;
  Material material;
  rtg_id flatten(rtg_builder* b) const {
    return check_id(rtg_object_constant_medium(b, boundary.flatten(b), density, material.emit(b)));
  }
};
template <class O>
ConstantMedium(O, float, Material) -> ConstantMedium<O>;
// Not in the reference (include/rtiow_gpu_mesh.h): a triangle, counter-clockwise front face, two-sided like Rect ...
struct Triangle {
  Vec3 v0, v1, v2;
  Material material;
  rtg_id flatten(rtg_builder* b) const { return check_id(rtg_object_triangle(b, v0.data(), v1.data(), v2.data(), material.emit(b))); }
};
// ... and an indexed mesh of them under one Bvh (sah: the SAH builder instead of Bvh::new's median split).  The arrays are
// shared, not copied, until the scene is built.
struct Mesh {
  std::shared_ptr<const std::vector<float>> vertices;    // 3 per vertex
  std::shared_ptr<const std::vector<uint32_t>> indices;  // 3 per triangle
  Material material;
  bool sah = false;
  rtg_id flatten(rtg_builder* b) const {
    return check_id(rtg_object_mesh(b, vertices->data(), vertices->size() / 3, indices->data(), indices->size() / 3, material.emit(b), sah ? 1u : 0u));
  }
};
inline Mesh mesh(std::vector<float> vertices, std::vector<uint32_t> indices, Material m, bool sah = false) {
  if (vertices.size() % 3 || indices.size() % 3) throw Error(RTG_ERR_INVALID, "object::mesh: three floats per vertex, three indices per triangle");
  return Mesh{std::make_shared<const std::vector<float>>(std::move(vertices)), std::make_shared<const std::vector<uint32_t>>(std::move(indices)),
              std::move(m), sah};
}
}  // namespace object

namespace bvh {
struct Bvh {  // bvh.rs:9-19; itself an Object (bvh.rs:84)
  std::shared_ptr<Scene> objects;
  Range exposure;
  rtg_id flatten(rtg_builder* b) const {
    std::vector<rtg_id> ids;
    for (const auto& o : *objects) ids.push_back(o.emit(b));
    return check_id(rtg_object_bvh(b, ids.data(), ids.size(), exposure.start, exposure.end));
  }
};
inline Bvh from_scene(Scene scene, Range exposure) {  // bvh.rs:128
  return Bvh{std::make_shared<Scene>(std::move(scene)), exposure};
}
}  // namespace bvh

// camera.rs
struct Camera {
  rtg_camera c;
  static Camera look(Vec3 look_from, Vec3 look_at, Vec3 up, float fov, float aspect, float aperture,
                     float focus_dist, Range exposure) {
    Camera cam;
    check(rtg_camera_look(look_from.data(), look_at.data(), up.data(), fov, aspect, aperture, focus_dist,
                          exposure.start, exposure.end, &cam.c));
    return cam;
  }
};

// lib.rs:321 `pub struct Image(Vec<Vec<Vec3>>)`: rows top to bottom
struct Image {
  size_t nx = 0, ny = 0;
  std::vector<float> rgb;  // ny * nx * 3
};

// Not in the reference (include/rtiow_gpu_environment.h): what a ray that leaves the scene sees -- `scale` times `texture` at the point
// rot_y(unit(d)).  texture::image with mapping 1 (spherical) about (0, 0, 0) is a lat-long map, row 0 = world +y.  The builder of
// this header lives inside make_scene, so the environment rides in the CastOptions: rtg_builder_set_environment is called there.
struct Environment {
  Texture texture;
  float scale[3] = {1.f, 1.f, 1.f};
  float rotate_y_degrees = 0.f;
};

struct CastOptions {
  std::shared_ptr<const Environment> environment;  // null: none (a miss is black, or the call's background)
  uint64_t seed = 0xDEADBEEF;
  int device = 0;
  // perlin.rs:24-29 tables (only needed when a perlin texture is used)
  const float* perlin_vecs = nullptr;
  const uint8_t *perm_x = nullptr, *perm_y = nullptr, *perm_z = nullptr;
  // par_cast_denoised / par_cast_multi_denoised: also ask for the error plane (RTG_FLAG_DENOISE_ERROR)
  bool denoise_error = false;
};

using SceneHandle = std::unique_ptr<rtg_scene, void (*)(rtg_scene*)>;

// flatten `world` once onto opt.device
// (Not in the reference, and not switched on by anything in this header: rtg_scene_set_option(handle.get(), "light_sampling", 1)
// renders every frame of the handle with direct light sampling of the world's list-level rect lights -- another estimator of
// the same image, not the reference's samples; include/rtiow_gpu.h, at rtg_scene_set_option, states it.)
inline SceneHandle make_scene(const Scene& world, const CastOptions& opt) {
  rtg_builder* b = nullptr;
  check(rtg_builder_create(&b));
  std::unique_ptr<rtg_builder, void (*)(rtg_builder*)> guard(b, rtg_builder_destroy);
  if (opt.perlin_vecs) check(rtg_builder_set_perlin_tables(b, opt.perlin_vecs, opt.perm_x, opt.perm_y, opt.perm_z));
  std::vector<rtg_id> ids;
  for (const auto& o : world) ids.push_back(o.emit(b));
  if (opt.environment) {
    rtg_environment_params ep{};
    ep.struct_size = sizeof(ep);
    ep.texture = opt.environment->texture.emit(b);
    for (int c = 0; c < 3; c++) ep.scale[c] = opt.environment->scale[c];
    ep.rotate_y_degrees = opt.environment->rotate_y_degrees;
    check(rtg_builder_set_environment(b, &ep));
  }
  rtg_scene* s = nullptr;
  check(rtg_scene_create(b, ids.data(), ids.size(), opt.device, &s));
  return SceneHandle(s, rtg_scene_destroy);
}

inline rtg_params cast_params(size_t nx, size_t ny, size_t ns, const CastOptions& opt) {
  rtg_params p{};
  p.struct_size = sizeof(p);
  p.nx = (uint32_t)nx, p.ny = (uint32_t)ny, p.ns = (uint32_t)ns;
  p.max_bounces = 50;  // lib.rs:93
  p.t_near = 0.001f;   // lib.rs:35
  p.seed = opt.seed;
  return p;
}

// par_cast, lib.rs:363: `world` is the list world of lib.rs:33; pass {boxed(bvh::from_scene(..))}
// for the `impl World for Bvh` of lib.rs:51.
inline Image par_cast(size_t nx, size_t ny, size_t ns, const Camera& camera, const Scene& world,
                      const CastOptions& opt = CastOptions()) {
  SceneHandle s = make_scene(world, opt);
  rtg_params p = cast_params(nx, ny, ns, opt);
  Image img;
  img.nx = nx, img.ny = ny;
  img.rgb.assign(nx * ny * 3, 0.f);
  check(rtg_par_cast(s.get(), &camera.c, &p, img.rgb.data(), nullptr));
  return img;
}

// Not in the reference: par_cast with RTG_FLAG_BACKGROUND -- a ray that leaves the scene sees `background` instead of black
// (lib.rs:100), so an open scene needs no emitting dome around it.  sky(bottom) is the constant background, sky(bottom, top)
// the gradient along world +y; book_sky() the book's (white to (0.5, 0.7, 1.0)).  The image has par_cast's layout.
inline rtg_background sky(const float (&bottom)[3]) {
  rtg_background g{};
  for (int c = 0; c < 3; c++) g.bottom[c] = bottom[c];
  return g;
}
inline rtg_background sky(const float (&bottom)[3], const float (&top)[3]) {
  rtg_background g = sky(bottom);
  g.mode = 1;
  for (int c = 0; c < 3; c++) g.top[c] = top[c];
  return g;
}
inline rtg_background book_sky() { return sky({1.f, 1.f, 1.f}, {0.5f, 0.7f, 1.f}); }

inline Image par_cast_background(size_t nx, size_t ny, size_t ns, const Camera& camera, const Scene& world, const rtg_background& background,
                                 const CastOptions& opt = CastOptions()) {
  SceneHandle s = make_scene(world, opt);
  rtg_params p = cast_params(nx, ny, ns, opt);
  p.flags = RTG_FLAG_BACKGROUND;
  const size_t n = nx * ny, block_word = (3 * n + 1) & ~size_t(1);  // the plane, padding to 8 bytes, the block
  std::vector<float> frame(block_word + sizeof(rtg_background) / sizeof(float), 0.f);
  std::memcpy(frame.data() + block_word, &background, sizeof(background));
  check(rtg_par_cast(s.get(), &camera.c, &p, frame.data(), nullptr));
  Image img;
  img.nx = nx, img.ny = ny;
  img.rgb.assign(frame.begin(), frame.begin() + 3 * n);
  return img;
}

// Not in the reference: the same frame rendered `step` samples at a time (include/rtiow_gpu.h RTG_FLAG_PARTIAL /
// RTG_FLAG_RESUME).  After each slice `on_preview(n_done, preview)` receives the frame resolved at n_done samples --
// bit-identical to par_cast(nx, ny, n_done, ...) -- and returns false to stop early (a time budget, a cancel button).  The
// last preview, at n_done == ns, is bit-identical to par_cast(nx, ny, ns, ...).  Returns the samples rendered.
template <typename OnPreview>
inline size_t par_cast_progressive(size_t nx, size_t ny, size_t ns, size_t step, const Camera& camera, const Scene& world,
                                   OnPreview&& on_preview, const CastOptions& opt = CastOptions()) {
  if (step == 0) throw Error(RTG_ERR_INVALID, "par_cast_progressive: step must be > 0");
  SceneHandle s = make_scene(world, opt);
  std::vector<float> sum(nx * ny * 3, 0.f);  // the running sum of the samples so far
  Image preview;
  preview.nx = nx, preview.ny = ny;
  size_t done = 0;
  while (done < ns) {
    const size_t end = std::min(ns, done + step);
    rtg_params p = cast_params(nx, ny, end, opt);
    p.flags = RTG_FLAG_PARTIAL | RTG_FLAG_RESUME, p.sample_begin = (uint32_t)done;
    check(rtg_par_cast(s.get(), &camera.c, &p, sum.data(), nullptr));
    done = end;
    preview.rgb = sum;  // the resolve step divides a copy
    p = cast_params(nx, ny, done, opt);
    p.flags = RTG_FLAG_RESUME, p.sample_begin = (uint32_t)done;
    check(rtg_par_cast(s.get(), &camera.c, &p, preview.rgb.data(), nullptr));
    if (!on_preview(done, static_cast<const Image&>(preview))) break;
  }
  return done;
}

// Not in the reference: par_cast with RTG_FLAG_SUM_SQUARES.  `image` is exactly what par_cast returns; `sum_sq` (same layout)
// holds per pixel and channel the f32 running sum of the squared sample colours, from which standard_error estimates the
// noise of every pixel's mean.
struct SquaresImage {
  Image image;
  std::vector<float> sum_sq;  // ny * nx * 3
  size_t ns = 0;
};

inline SquaresImage par_cast_squares(size_t nx, size_t ny, size_t ns, const Camera& camera, const Scene& world,
                                     const CastOptions& opt = CastOptions()) {
  SceneHandle s = make_scene(world, opt);
  rtg_params p = cast_params(nx, ny, ns, opt);
  p.flags = RTG_FLAG_SUM_SQUARES;
  std::vector<float> planes(2 * nx * ny * 3, 0.f);  // plane 0: the image, plane 1: the sum of squares
  check(rtg_par_cast(s.get(), &camera.c, &p, planes.data(), nullptr));
  SquaresImage r;
  r.image.nx = nx, r.image.ny = ny, r.ns = ns;
  r.image.rgb.assign(planes.begin(), planes.begin() + nx * ny * 3);
  r.sum_sq.assign(planes.begin() + nx * ny * 3, planes.end());
  return r;
}

// Not in the reference: par_cast with RTG_FLAG_SAMPLE_COUNTS.  `counts` (nx * ny, row 0 = top) gives every pixel its own sample
// count n_p: pixel p of the result is par_cast(nx, ny, min(n_p, ns), ...) at p, bit for bit; pixels with n_p = 0 stay black.
inline Image par_cast_counts(size_t nx, size_t ny, size_t ns, const std::vector<uint32_t>& counts, const Camera& camera,
                             const Scene& world, const CastOptions& opt = CastOptions()) {
  if (counts.size() != nx * ny) throw Error(RTG_ERR_INVALID, "par_cast_counts: counts must hold nx * ny values");
  SceneHandle s = make_scene(world, opt);
  rtg_params p = cast_params(nx, ny, ns, opt);
  p.flags = RTG_FLAG_SAMPLE_COUNTS;
  std::vector<float> frame(4 * nx * ny, 0.f);  // the image, then the count plane (uint32_t words)
  std::memcpy(frame.data() + 3 * nx * ny, counts.data(), counts.size() * sizeof(uint32_t));
  check(rtg_par_cast(s.get(), &camera.c, &p, frame.data(), nullptr));
  Image img;
  img.nx = nx, img.ny = ny;
  img.rgb.assign(frame.begin(), frame.begin() + 3 * nx * ny);
  return img;
}

// Not in the reference: adaptive sampling with the retire rule in the library (RTG_FLAG_RETIRE).  Every pixel starts at n_p = ns;
// each slice renders `step` more samples of the pixels still active and retires, in the same call, those whose (2 radius + 1)^2
// window has every standard error <= target_se (once k >= min_samples).  Stops when no pixel is active or at ns.  `image` is the
// frame resolved per pixel (pixel p = par_cast(nx, ny, counts[p], ...) at p, bit for bit), `counts` the samples each pixel got,
// `block` the retire block of the last slice.
struct AdaptiveImage {
  Image image;
  std::vector<uint32_t> counts;  // ny * nx
  size_t slices = 0;
  rtg_retire block{};
};

inline AdaptiveImage par_cast_adaptive(size_t nx, size_t ny, size_t ns, size_t step, double target_se, uint32_t min_samples,
                                       uint32_t radius, const Camera& camera, const Scene& world,
                                       const CastOptions& opt = CastOptions()) {
  if (step == 0) throw Error(RTG_ERR_INVALID, "par_cast_adaptive: step must be > 0");
  SceneHandle s = make_scene(world, opt);
  const size_t n = nx * ny, block_word = (7 * n + 1) & ~size_t(1);  // planes, count plane, padding to 8 bytes, the block
  std::vector<float> frame(block_word + sizeof(rtg_retire) / sizeof(float), 0.f);
  std::vector<uint32_t> counts(n, (uint32_t)ns);
  std::memcpy(frame.data() + 6 * n, counts.data(), n * sizeof(uint32_t));
  rtg_retire r{};
  r.target_se = target_se, r.min_samples = min_samples, r.radius = radius;
  std::memcpy(frame.data() + block_word, &r, sizeof(r));
  AdaptiveImage out;
  size_t done = 0;
  while (done < ns) {
    const size_t end = std::min(ns, done + step);
    rtg_params p = cast_params(nx, ny, end, opt);
    p.flags = RTG_FLAG_SUM_SQUARES | RTG_FLAG_SAMPLE_COUNTS | RTG_FLAG_RETIRE | RTG_FLAG_PARTIAL | RTG_FLAG_RESUME;
    p.sample_begin = (uint32_t)done;
    check(rtg_par_cast(s.get(), &camera.c, &p, frame.data(), nullptr));
    done = end, out.slices++;
    std::memcpy(&out.block, frame.data() + block_word, sizeof(rtg_retire));
    if (out.block.active == 0) break;
  }
  // resolve a copy of plane 0 with the count plane: each pixel divided by the samples it holds
  std::memcpy(counts.data(), frame.data() + 6 * n, n * sizeof(uint32_t));
  for (uint32_t& c : counts) c = std::min<uint32_t>(c, (uint32_t)done);
  std::vector<float> pv(4 * n);
  std::memcpy(pv.data(), frame.data(), 3 * n * sizeof(float));
  std::memcpy(pv.data() + 3 * n, counts.data(), n * sizeof(uint32_t));
  rtg_params p = cast_params(nx, ny, done, opt);
  p.flags = RTG_FLAG_SAMPLE_COUNTS | RTG_FLAG_RESUME;
  p.sample_begin = (uint32_t)done;
  check(rtg_par_cast(s.get(), &camera.c, &p, pv.data(), nullptr));
  out.image.nx = nx, out.image.ny = ny;
  out.image.rgb.assign(pv.begin(), pv.begin() + 3 * n);
  out.counts = std::move(counts);
  return out;
}

// Not in the reference: par_cast with RTG_FLAG_SUM_SQUARES | RTG_FLAG_DENOISE.  `image` is exactly what par_cast returns;
// `denoised` is the frame filtered by the library's variance-driven non-local-means filter (strength k, search radius `radius`,
// patch radius `patch`: see the header), `block` the denoise block with its out-fields.  With CastOptions::denoise_error the
// call sets RTG_FLAG_DENOISE_ERROR too and `error` is the variance of every filtered pixel (+inf where a pixel was passed
// through); else `error` stays empty.
struct DenoisedImage {
  Image image, denoised, error;
  rtg_denoise block{};
};

// (`cast(params, frame)`: rtg_par_cast on one handle, or rtg_par_cast_multi on several)
template <typename Cast>
inline DenoisedImage denoised_frame(size_t nx, size_t ny, size_t ns, float k, uint32_t radius, uint32_t patch, const CastOptions& opt, Cast&& cast) {
  const size_t n = nx * ny, block_word = (6 * n + 1) & ~size_t(1);  // two planes, padding to 8 bytes, the block, the output plane
  const size_t error_word = (block_word + 16 + 3 * n + 1) & ~size_t(1);  // the error plane: the first even word behind the output plane
  std::vector<float> frame(opt.denoise_error ? error_word + 3 * n : block_word + sizeof(rtg_denoise) / sizeof(float) + 3 * n, 0.f);
  rtg_denoise d{};
  d.k = k, d.radius = radius, d.patch = patch;
  std::memcpy(frame.data() + block_word, &d, sizeof(d));
  rtg_params p = cast_params(nx, ny, ns, opt);
  p.flags = RTG_FLAG_SUM_SQUARES | RTG_FLAG_DENOISE | (opt.denoise_error ? RTG_FLAG_DENOISE_ERROR : 0u);
  cast(p, frame.data());
  DenoisedImage out;
  out.image.nx = out.denoised.nx = nx, out.image.ny = out.denoised.ny = ny;
  out.image.rgb.assign(frame.begin(), frame.begin() + 3 * n);
  out.denoised.rgb.assign(frame.begin() + block_word + 16, frame.begin() + block_word + 16 + 3 * n);
  if (opt.denoise_error) {
    out.error.nx = nx, out.error.ny = ny;
    out.error.rgb.assign(frame.begin() + error_word, frame.end());
  }
  std::memcpy(&out.block, frame.data() + block_word, sizeof(rtg_denoise));
  return out;
}

inline DenoisedImage par_cast_denoised(size_t nx, size_t ny, size_t ns, const Camera& camera, const Scene& world, float k = 0.7f,
                                       uint32_t radius = 5, uint32_t patch = 2, const CastOptions& opt = CastOptions()) {
  SceneHandle s = make_scene(world, opt);
  return denoised_frame(nx, ny, ns, k, radius, patch, opt, [&](const rtg_params& p, float* frame) { check(rtg_par_cast(s.get(), &camera.c, &p, frame, nullptr)); });
}

// Not in the reference: par_cast with RTG_FLAG_FEATURES.  `image` is exactly what par_cast returns; `albedo` and `normal` (three
// floats per pixel) and `depth` (one) are the first-hit feature planes a denoiser or compositor takes beside the colour, from
// grid x grid primary rays per pixel (see the header); `block` the features block with its out-fields.
struct FeatureImages {
  Image image, albedo, normal;
  std::vector<float> depth;
  rtg_features block{};
};

template <typename Cast>
inline FeatureImages features_frame(size_t nx, size_t ny, size_t ns, uint32_t grid, const CastOptions& opt, Cast&& cast) {
  const size_t n = nx * ny, block_word = (3 * n + 1) & ~size_t(1);  // one plane, padding to 8 bytes, the block, the three planes
  std::vector<float> frame(block_word + sizeof(rtg_features) / sizeof(float) + 7 * n, 0.f);
  rtg_features f{};
  f.grid = grid, f.compute = 1;
  std::memcpy(frame.data() + block_word, &f, sizeof(f));
  rtg_params p = cast_params(nx, ny, ns, opt);
  p.flags = RTG_FLAG_FEATURES;
  cast(p, frame.data());
  FeatureImages out;
  out.image.nx = out.albedo.nx = out.normal.nx = nx, out.image.ny = out.albedo.ny = out.normal.ny = ny;
  const auto at = frame.begin() + block_word + 16;
  out.image.rgb.assign(frame.begin(), frame.begin() + 3 * n);
  out.albedo.rgb.assign(at, at + 3 * n);
  out.normal.rgb.assign(at + 3 * n, at + 6 * n);
  out.depth.assign(at + 6 * n, at + 7 * n);
  std::memcpy(&out.block, frame.data() + block_word, sizeof(rtg_features));
  return out;
}

inline FeatureImages par_cast_features(size_t nx, size_t ny, size_t ns, const Camera& camera, const Scene& world, uint32_t grid = 2,
                                       const CastOptions& opt = CastOptions()) {
  SceneHandle s = make_scene(world, opt);
  return features_frame(nx, ny, ns, grid, opt, [&](const rtg_params& p, float* frame) { check(rtg_par_cast(s.get(), &camera.c, &p, frame, nullptr)); });
}

// Not in the reference: the frame sharded over `n_devices` GPUs of this process (rtg_par_cast_multi): `world` is flattened once
// per device (opt.device is not used), the tiles are sharded inside the library and the frame is assembled on the first device --
// bit-identical to par_cast.  The flagged frames (par_cast_multi_squares / _denoised / _features) set scene option multi_planes:
// every plane is gathered on the first device, which filters and divides; they equal their one-device namesakes word for word.
struct MultiScenes {
  std::vector<SceneHandle> handles;
  std::vector<rtg_scene*> raw;
};
inline MultiScenes make_scenes(const Scene& world, int n_devices, const CastOptions& opt, bool planes) {
  int have = 0;
  check(rtg_device_count(&have));
  if (n_devices < 1 || n_devices > have) throw Error(RTG_ERR_INVALID, "par_cast_multi: n_devices must be 1 .. the devices the host has");
  MultiScenes m;
  for (int d = 0; d < n_devices; d++) {
    CastOptions o = opt;
    o.device = d;
    m.handles.push_back(make_scene(world, o));
    m.raw.push_back(m.handles.back().get());
  }
  if (planes) check(rtg_scene_set_option(m.raw[0], "multi_planes", 1));
  return m;
}

inline Image par_cast_multi(size_t nx, size_t ny, size_t ns, const Camera& camera, const Scene& world, int n_devices,
                            const CastOptions& opt = CastOptions()) {
  MultiScenes m = make_scenes(world, n_devices, opt, false);
  rtg_params p = cast_params(nx, ny, ns, opt);
  Image img;
  img.nx = nx, img.ny = ny;
  img.rgb.assign(nx * ny * 3, 0.f);
  check(rtg_par_cast_multi(m.raw.data(), (int)m.raw.size(), &camera.c, &p, img.rgb.data(), nullptr));
  return img;
}

inline SquaresImage par_cast_multi_squares(size_t nx, size_t ny, size_t ns, const Camera& camera, const Scene& world, int n_devices,
                                           const CastOptions& opt = CastOptions()) {
  MultiScenes m = make_scenes(world, n_devices, opt, true);
  rtg_params p = cast_params(nx, ny, ns, opt);
  p.flags = RTG_FLAG_SUM_SQUARES;
  std::vector<float> planes(2 * nx * ny * 3, 0.f);
  check(rtg_par_cast_multi(m.raw.data(), (int)m.raw.size(), &camera.c, &p, planes.data(), nullptr));
  SquaresImage r;
  r.image.nx = nx, r.image.ny = ny, r.ns = ns;
  r.image.rgb.assign(planes.begin(), planes.begin() + nx * ny * 3);
  r.sum_sq.assign(planes.begin() + nx * ny * 3, planes.end());
  return r;
}

inline DenoisedImage par_cast_multi_denoised(size_t nx, size_t ny, size_t ns, const Camera& camera, const Scene& world, int n_devices,
                                             float k = 0.7f, uint32_t radius = 5, uint32_t patch = 2, const CastOptions& opt = CastOptions()) {
  MultiScenes m = make_scenes(world, n_devices, opt, true);
  return denoised_frame(nx, ny, ns, k, radius, patch, opt, [&](const rtg_params& p, float* frame) {
    check(rtg_par_cast_multi(m.raw.data(), (int)m.raw.size(), &camera.c, &p, frame, nullptr));
  });
}

inline FeatureImages par_cast_multi_features(size_t nx, size_t ny, size_t ns, const Camera& camera, const Scene& world, int n_devices,
                                             uint32_t grid = 2, const CastOptions& opt = CastOptions()) {
  MultiScenes m = make_scenes(world, n_devices, opt, true);
  return features_frame(nx, ny, ns, grid, opt, [&](const rtg_params& p, float* frame) {
    check(rtg_par_cast_multi(m.raw.data(), (int)m.raw.size(), &camera.c, &p, frame, nullptr));
  });
}

// Standard error of a pixel channel's mean over n samples (rtiow-rust_amd/noise.py, in double): s2 = max(0, (sum_sq - n m^2) /
// (n - 1)), se = sqrt(s2 / n); +inf for n = 1.  `mean` = sum / n (par_cast's image; a PARTIAL running sum divided by n).
inline double standard_error(double mean, double sum_sq, size_t n) {
  if (n < 2) return INFINITY;
  const double nd = (double)n, var = std::max(0.0, (sum_sq - nd * mean * mean) / (nd - 1.0));
  return std::sqrt(var / nd);
}

// ... of every pixel channel of a par_cast_squares frame (ny * nx * 3 values)
inline std::vector<double> standard_error(const SquaresImage& f) {
  std::vector<double> se(f.sum_sq.size());
  for (size_t i = 0; i < se.size(); i++) se[i] = standard_error((double)f.image.rgb[i], (double)f.sum_sq[i], f.ns);
  return se;
}

// print_ppm, lib.rs:344-361 (host post-process)
inline void print_ppm(const Image& image, FILE* out = stdout) {
  std::fprintf(out, "P3\n%zu %zu\n255\n", image.nx, image.ny);
  auto to_u8 = [](float x) {
    float v = 255.99f * x;
    int i = (v != v) ? 0 : (v >= 2147483648.f ? 2147483647 : (v <= -2147483648.f ? (-2147483647 - 1) : (int)v));
    return i < 0 ? 0 : (i > 255 ? 255 : i);
  };
  for (size_t i = 0; i < image.nx * image.ny; i++) {
    const float* c = &image.rgb[3 * i];
    std::fprintf(out, "%d %d %d\n", to_u8(std::sqrt(c[0])), to_u8(std::sqrt(c[1])), to_u8(std::sqrt(c[2])));
  }
}

}  // namespace rtiow
