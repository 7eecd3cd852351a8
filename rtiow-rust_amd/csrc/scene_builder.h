// scene_builder.h -- host side of the boundary: the builder behind the rtg_object_* / rtg_material_* /
// rtg_texture_* calls, Bvh::new (bvh.rs:22-81), bounding boxes (object.rs) and the flattener that
// turns the object graph into the flat program of flat_scene.h.  Pure host C++ (no HIP).
#pragma once
#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "flat_scene.h"

namespace rtg {

struct Box3 {
  float mn[3], mx[3];
};

struct Packet {
  uint32_t w[4];
};

struct HostObject {
  enum Kind : uint8_t { SPHERE, RECT, FLIP, TRANSLATE, SCALE, ROTATE_Y, AND, MOVE, MEDIUM, BVH, TRI } kind;
  float f[6] = {0, 0, 0, 0, 0, 0};  // kind-specific scalars (see scene_builder.cpp)
  uint32_t a = 0xffffffffu, b = 0xffffffffu;  // children (object ids) / bvh root node id / TRI: index into SceneBuilder::triangles
  uint32_t mat = 0xffffffffu;
  int axis = 0;
};

struct HostTriangle {  // include/rtiow_gpu_mesh.h: the vertices as given (the bounding box is theirs) and the record rt_triangle.h tri_record makes
  float v[9];    // v0, v1, v2
  float rec[9];  // e1, e2, N
  // include/rtiow_gpu_surface.h: bit 0 = per-vertex normals, bit 1 = per-vertex UVs; attr = n0, n1, n2, (u0, v0), (u1, v1), (u2, v2), as
  // given, +0 where the triangle has none.  has = 0: a plain triangle, two records as ever (flat_scene.h OP_TRI)
  uint32_t has = 0;
  float attr[15] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

struct HostBvhNode {  // bvh.rs:9-19
  Box3 box;
  int32_t left = -1, right = -1;  // BvhContents::Node
  uint32_t leaf = 0xffffffffu;    // BvhContents::Leaf (object id)
};

struct HostMaterial {
  uint32_t kind;
  uint32_t tex = 0xffffffffu;
  float albedo[3] = {0, 0, 0};
  float param = 0.f;  // fuzz / ref_idx / brightness
};

struct HostTexture {
  uint32_t kind;
  float rgb[3] = {0, 0, 0};
  float scale = 0.f;
  uint32_t t0 = 0, t1 = 0;
  // TEX_IMAGE (flat_scene.h): size, rt_image.h flag word and the texels as float4 packets; the mapping floats live in the
  // TEX_EXT slot behind it (m)
  uint32_t w = 0, h = 0, flags = 0;
  std::vector<float> texels;
  float m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct FlatScene {
  std::vector<Packet> lo, hi;    // program
  std::vector<Packet> mat, tex;  // 2 packets per record; tex: then the texels of its images, one packet each (flat_scene.h TEX_IMAGE)
  uint32_t n_tex = 0;            // texture records in tex
  std::array<float, 1024> perlin_vecs{};  // 256 x float4
  std::array<uint8_t, 768> perlin_perm{};
  uint32_t features = 0;
  bool has_perlin = false;
  int deep_wrappers = 0;  // most wrappers (PUSH) open at once in any one stream of the program
  int deep_media = 0;     // deepest level of boundary queries a walk of the program recurses into (0 = no object-graph boundary)
  // the SECOND program (flat_scene.h "the list level, hoisted"): empty unless the world has the shape the pool-2 kernel walks
  std::vector<Packet> lo2, hi2;
  P2Table p2{};
};

class SceneBuilder {
 public:
  std::vector<HostObject> objects;
  std::vector<HostBvhNode> bvh_nodes;
  std::vector<HostTriangle> triangles;  // one per TRI object
  std::vector<HostMaterial> materials;
  std::vector<HostTexture> textures;
  std::array<float, 1024> perlin_vecs{};
  std::array<uint8_t, 768> perlin_perm{};
  bool has_perlin = false;
  // include/rtiow_gpu_environment.h: what a ray that leaves the scene sees; texture = 0xffffffff: none.  (s, c) from the degrees
  // by rotate_y_pair (rtg_api.hip), the pair rtg_object_rotate_y makes.
  struct Environment {
    uint32_t texture = 0xffffffffu;
    float scale[3] = {1.f, 1.f, 1.f};
    float degrees = 0.f, s = 0.f, c = 1.f;
  } environment;

  // All return an id or throw BuildError.
  uint32_t add_object(const HostObject& o);
  uint32_t add_bvh(const uint32_t* objs, size_t n, float e0, float e1, bool sah = false);
  // include/rtiow_gpu_mesh.h: one triangle (v: 9 floats), and n_triangles of them under one Bvh; a refusal leaves the builder as it was
  // (normals9 / uvs6, normals / uvs: include/rtiow_gpu_surface.h, null = none -- then exactly the plain triangle and mesh)
  uint32_t add_triangle(const float* v, uint32_t material, const float* normals9 = nullptr, const float* uvs6 = nullptr);
  uint32_t add_mesh(const float* vertices, size_t n_vertices, const uint32_t* indices, size_t n_triangles, uint32_t material, bool sah,
                    const float* normals = nullptr, const float* uvs = nullptr);
  // is `material` built on an rtg_texture_surface texture?  Only a triangle with UVs takes such a material
  bool surface_material(uint32_t material) const {
    return material < materials.size() && materials[material].tex < textures.size() && textures[materials[material].tex].kind == TEX_SURFACE;
  }
  Box3 bounding_box(uint32_t obj, float e0, float e1) const;
  void flatten(const uint32_t* world, size_t n, FlatScene* out) const;
  // The light table of `world` (flat_scene.h LightRect) and, per material, whether it is sampled (scene option light_sampling)
  void light_table(const uint32_t* world, size_t n, std::vector<LightRect>* lights, std::vector<uint8_t>* sampled) const;
  bool hoist_segments = true;  // flatten() may put an OP_SEG record in front of a list world's longest run of plain primitives

 private:
  int32_t build_bvh(std::vector<uint32_t> objs, float e0, float e1);
  int32_t build_bvh_sah(std::vector<uint32_t> objs, float e0, float e1);
  // `boundary` = nesting level of medium boundaries the stream belongs to (0 = the main walk); `mark_roots`: outermost Bvhs of
  // this stream get F_BVH_ROOT (always in the main walk; in a boundary stream only when it holds a medium itself)
  void emit(uint32_t obj, bool under_bvh, int depth, FlatScene* out, int boundary = 0, bool mark_roots = true, int saves = 0) const;
  void emit_bvh(int32_t node, int depth, FlatScene* out, int boundary, bool mark_roots, int saves) const;
  bool holds_medium(uint32_t obj) const;
  void flatten_program(const uint32_t* world, size_t n, FlatScene* out, size_t seg0, size_t seg1) const;
  bool flatten_pool2(const uint32_t* world, size_t n, FlatScene* out) const;
  void finish_materials(FlatScene* out) const;
};

struct BuildError {
  int code;
  std::string msg;
};

}  // namespace rtg
