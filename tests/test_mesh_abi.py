"""Triangles and meshes, CPU side (include/rtiow_gpu_mesh.h; Builder.triangle / Builder.mesh; triangle.py): the header declares
exactly its three entry points with the prototypes the binding and the Rust module give them, and they stay out of the ABI of
rtiow_gpu.h; the refusals; the host probe against the numpy definition, bit for bit; the definition against an independent
float64 reference (triangle_ref.py); the flattener's records, boxes and routing bits; the mesh generators and the OBJ reader; and
rt_triangle.h in a stand-alone program, plain and under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import assert_bit_equal
import mesh_cases as MC
import triangle_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu_mesh.h")
MESH_RS = os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "mesh.rs")
CSRC = os.path.join(ROOT, "rtiow-rust_amd", "csrc")
NAMES = ["object_triangle", "object_mesh", "debug_triangle_host"]
INVALID_ID = 0xFFFFFFFF
OP_BOX, OP_SPHERE, OP_EXT, OP_TRI = 1, 2, 12, 14             # csrc/flat_scene.h
F_FLIP, F_BVH_ROOT, F_MATKIND_SHIFT, F_TEXTURED = 1 << 9, 1 << 13, 16, 1 << 19
FEAT_XFORM, FEAT_RECT, FEAT_DEEP, FEAT_TRI = 1, 4, 128, 1024
f32 = np.float32


def _prototypes(text, strip, pattern):
    text = re.sub(strip, "", text, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip()] for m in re.finditer(pattern, text, flags=re.S)}


def test_the_header_declares_exactly_the_three_entry_points(pkg):
    text = open(HEADER).read()
    c_fns = _prototypes(text, r"/\*.*?\*/", r"\b(rtg_\w+)\s*\(([^)]*)\)\s*;")
    assert sorted(c_fns) == sorted("rtg_" + n for n in NAMES)
    assert pkg.capi.MESH_SYMBOLS == NAMES
    assert '#include "rtiow_gpu.h"' in text and "not part of the ABI of rtiow_gpu.h" in text
    names = lambda fn: [re.sub(r"\[\d*\]", "", a.split()[-1]).lstrip("*") for a in c_fns[fn]]   # noqa: E731
    assert names("rtg_object_triangle") == ["b", "v0", "v1", "v2", "material"]
    assert names("rtg_object_mesh") == ["b", "vertices", "n_vertices", "indices", "n_triangles", "material", "sah"]
    assert names("rtg_debug_triangle_host") == ["n", "tri9", "rays8", "t_min", "out8"]


def test_the_library_exports_them_with_the_binding_s_prototypes(pkg):
    be = pkg.load()
    for n, argc, res in zip(NAMES, (5, 7, 5), (C.c_uint32, C.c_uint32, C.c_int)):
        fn = getattr(be.lib, "rtg_" + n)
        assert fn.restype is res and len(fn.argtypes) == argc, n
    assert be.lib.rtg_object_mesh.argtypes[2] is C.c_size_t and be.lib.rtg_object_mesh.argtypes[6] is C.c_uint32
    assert be.lib.rtg_debug_triangle_host.argtypes[3] is C.c_float


def test_they_stay_out_of_the_abi_and_the_rust_module_follows_the_header(pkg):
    capi = pkg.capi
    for other in (capi.ABI_SYMBOLS, capi.QUERY_SYMBOLS, capi.RAY_FRAME_SYMBOLS, capi.IMAGE_SYMBOLS):
        assert not set(NAMES) & set(other)
    main = open(os.path.join(ROOT, "include", "rtiow_gpu.h")).read()
    assert "rtg_object_triangle" not in main and "rtg_object_mesh" not in main and "rtg_debug_triangle_host" not in main
    c_fns = _prototypes(open(HEADER).read(), r"/\*.*?\*/", r"\b(rtg_\w+)\s*\(([^)]*)\)\s*;")
    rs_fns = _prototypes(open(MESH_RS).read(), r"//[^\n]*", r"pub fn (rtg_\w+)\s*\(([^)]*)\)")
    assert sorted(rs_fns) == sorted(c_fns)
    for name in c_fns:
        assert len(rs_fns[name]) == len(c_fns[name]), name
    lib_rs = open(os.path.join(os.path.dirname(MESH_RS), "lib.rs")).read()
    assert "pub mod mesh;" in lib_rs
    for n in NAMES:
        assert "rtg_" + n not in lib_rs, n


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _counts(b, world_probe):
    """The records of a probe world.  The builder exposes no counts: what a refusal may not move is read off its surface -- the
    next object and material ids ARE the object and material counts; of the Bvh nodes only those an object references show
    (the BOX records of the Bvhs flattened), so a node left behind by a refusal that no object names would go unseen here."""
    words, _ = b.flatten(world_probe)
    return len(words)


def test_every_refusal_leaves_the_builder_as_it_was(pkg):
    be = pkg.load()
    T = pkg.triangle
    b = be.builder()
    mat = b.lambertian(b.constant((0.5, 0.5, 0.5)))
    first = b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), mat)
    v, f = T.icosphere(1)
    good_mesh = b.mesh(v, f, mat)
    assert good_mesh == first + 1 + len(f)          # the triangles took the ids in between, the Bvh the one behind them
    before = _counts(b, [first, good_mesh])
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    vp, ip = v.ctypes.data_as(fp), f.ctypes.data_as(up)

    def tri(v0, v1, v2, m=mat, builder=b.h):
        a = [None if x is None else (C.c_float * 3)(*x) for x in (v0, v1, v2)]
        got = be._object_triangle(builder, a[0], a[1], a[2], m)
        return got == INVALID_ID and be.last_error() != ""

    A, B_, C_ = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    assert tri(None, B_, C_) and tri(A, None, C_) and tri(A, B_, None) and tri(A, B_, C_, builder=None)
    assert tri(A, B_, C_, m=mat + 1) and tri(A, B_, C_, m=INVALID_ID)
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            for c in range(3):
                vs = [list(A), list(B_), list(C_)]
                vs[k][c] = bad
                assert tri(*vs), (bad, k, c)
    assert tri(A, A, C_) and tri(A, B_, (2.0, 0.0, 0.0))            # len == 0: a repeated vertex, three on a line
    assert tri(A, (1e-30, 0.0, 0.0), (0.0, 1e-30, 0.0))            # len underflows to 0
    assert tri(A, (1e30, 0.0, 0.0), (0.0, 1e30, 0.0))              # len overflows
    assert tri((-3e38, 0.0, 0.0), (3e38, 0.0, 0.0), C_)            # an edge overflows

    def mesh(vertices=vp, n_v=len(v), indices=ip, n_t=len(f), m=mat, sah=0, builder=b.h):
        got = be._object_mesh(builder, vertices, n_v, indices, n_t, m, sah)
        return got == INVALID_ID and be.last_error() != ""

    assert mesh(builder=None) and mesh(vertices=None) and mesh(indices=None)
    assert mesh(m=mat + 1) and mesh(sah=2) and mesh(sah=0xFFFFFFFF)
    assert mesh(n_t=0) and "zero objects" in be.last_error()         # RTG_ERR_EMPTY_BVH's message
    assert mesh(n_v=len(v) - 1)                                      # an index >= n_vertices ...
    late = f.copy()
    late[-1, 2] = len(v)                                             # ... found in the LAST triangle: nothing of the mesh stays
    assert mesh(indices=late.ctypes.data_as(up))
    flat = f.copy()
    flat[-1] = (0, 0, 1)                                             # a triangle rtg_object_triangle would refuse, again the last
    assert mesh(indices=flat.ctypes.data_as(up))
    nanv = v.copy()
    nanv[int(f[-1, 1]), 1] = np.nan
    assert mesh(vertices=nanv.ctypes.data_as(fp))
    # nothing moved: the next object and material ids, and the records (the Bvh nodes among them) of what was built before
    assert _counts(b, [first, good_mesh]) == before
    assert b.lambertian(b.constant((0.1, 0.1, 0.1))) == mat + 1
    assert b.triangle(A, B_, C_, mat) == good_mesh + 1
    again = b.mesh(v, f, mat, sah=True)
    assert again == good_mesh + 2 + len(f)
    # a Bvh over the second mesh's triangle ids has as many nodes as the mesh's own: no node was left behind by a refusal
    hand = b.bvh_sah(list(range(good_mesh + 2, good_mesh + 2 + len(f))), exposure=(0.0, 0.0))
    assert_same_words(b.flatten([again])[0], b.flatten([hand])[0])


def assert_same_words(a, b):
    assert a.shape == b.shape and np.array_equal(a, b)


# ---- the host probe against the definition --------------------------------------------------------------------------------------
def _definition_out8(T, tri9, rays8, t_min):
    rec = T.record(tri9[:, 0:3], tri9[:, 3:6], tri9[:, 6:9])
    ok, t, p, nn = T.hit(rec, rays8[:, 0:3], rays8[:, 3:6], f32(t_min), rays8[:, 7])
    ref = np.zeros((len(tri9), 8), f32)
    ref[ok, 0], ref[ok, 1], ref[ok, 2:5], ref[ok, 5:8] = 1.0, t[ok], p[ok], nn[ok]
    return ref, ok


def test_the_host_probe_equals_the_definition_bit_for_bit(pkg):
    be, T = pkg.load(), pkg.triangle
    tri9, rays8 = MC.edge_pairs()
    ref, ok = _definition_out8(T, tri9, rays8, MC.T_MIN)
    got = be.triangle_host(tri9, rays8, MC.T_MIN)
    assert_bit_equal(got, ref, "rtg_debug_triangle_host against triangle.hit")
    n_random = 4096
    print("pairs %d (%d edge cases), hits %d random + %d edge" % (len(tri9), len(tri9) - n_random, ok[:n_random].sum(), ok[n_random:].sum()))
    assert 0.25 * n_random < ok[:n_random].sum() < 0.75 * n_random
    assert ok[n_random:].sum() > 50 and (~ok[n_random:]).sum() > 50
    # the range is half open: t == t_min hits, t == t_max misses -- on a pair where t is exact
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], f32)
    ray = lambda t_max: np.array([[0.25, 0.25, 2.0, 0, 0, -1.0, 0, t_max]], f32)   # noqa: E731
    assert be.triangle_host(tri, ray(3.0), 2.0)[0, 0] == 1.0 and be.triangle_host(tri, ray(3.0), np.nextafter(f32(2.0), f32(3.0)))[0, 0] == 0.0
    assert be.triangle_host(tri, ray(2.0), 0.001)[0, 0] == 0.0 and be.triangle_host(tri, ray(np.nextafter(f32(2.0), f32(3.0))), 0.001)[0, 0] == 1.0
    # both edges inclusive: u = 0, v = 0 and u + v = 1 hit
    for x, y in ((0.0, 0.5), (0.5, 0.0), (0.5, 0.5), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0)):
        r = np.array([[x, y, 1.0, 0, 0, -1.0, 0, 10.0]], f32)
        assert be.triangle_host(tri, r, 0.001)[0, 0] == 1.0, (x, y)
    assert be.triangle_host(tri9[:0], rays8[:0]).shape == (0, 8)


# ---- the definition against float64 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def references(pkg):
    """Per graph: the groups, the float32 rays and the float64 answer -- computed once, shared, left unchanged."""
    out = {}
    be = pkg.load()
    for name, fn in MC.GRAPHS.items():
        b = be.builder()
        world, groups = fn(pkg, b)
        rays = MC.aimed_rays(groups).astype(f32)
        r64 = rays.astype(np.float64)
        out[name] = (b, world, groups, rays, TR.closest_hit64(groups, r64[:, 0:3], r64[:, 3:6], r64[:, 6]))
    return out


@pytest.mark.parametrize("name", list(MC.GRAPHS))
def test_the_definition_against_the_float64_reference(pkg, references, name):
    _, _, groups, rays, ref = references[name]
    out, mat, index = TR.closest32(pkg.triangle, groups, rays)
    TR.assert_hits(TR.compare(ref, out, mat, index), name)


# ---- flattening -------------------------------------------------------------------------------------------------------------------
def test_the_records_hold_the_definition_s_words(pkg):
    be, T = pkg.load(), pkg.triangle
    b = be.builder()
    lam = b.lambertian(b.constant((0.5, 0.5, 0.5)))
    met = b.metal((0.5, 0.5, 0.5), 0.0)
    lit = b.diffuse_light(b.checker(b.constant((1, 1, 1)), b.constant((0, 0, 0))), 2.0)
    v = np.array([[0.25, -0.5, 1.0], [1.5, 0.25, 0.75], [-0.25, 1.25, 1.5]], f32)
    t0 = b.triangle(v[0], v[1], v[2], lam)
    t1 = b.flip_normals(b.triangle(v[0], v[1], v[2], met))
    t2 = b.flip_normals(b.flip_normals(b.triangle(v[0], v[1], v[2], lit)))
    words, feat = b.flatten([t0, t1, t2])
    assert feat & FEAT_TRI and not feat & (FEAT_XFORM | FEAT_RECT | FEAT_DEEP)     # (FlipNormals fused into F_FLIP: no PUSH / POP)
    assert [int(w) & 0xFF for w in words[:, 7]] == [OP_TRI, OP_EXT] * 3 + [0]
    _, e1, e2, nn = T.record(v[0], v[1], v[2])
    for k, (mat, flip, kind, textured) in enumerate(((lam, False, 0, False), (met, True, 1, False), (lit, False, 3, True))):
        head, ext = words[2 * k], words[2 * k + 1]
        assert_bit_equal(head[:6].view(f32), np.concatenate([v[0], e1]), "v0, e1")
        assert_bit_equal(ext[:6].view(f32), np.concatenate([e2, nn]), "e2, N")
        assert head[6] == mat and bool(head[7] & F_FLIP) == flip and (head[7] >> F_MATKIND_SHIFT) & 7 == kind and bool(head[7] & F_TEXTURED) == textured
        assert ext[6] == 0 and ext[7] == OP_EXT
    # the BOX over a leaf is the definition's box, and a world without a triangle flattens without the bit
    leaf = b.bvh([t0], exposure=(0.0, 0.0))
    words, feat = b.flatten([leaf])
    lo, hi = T.bounding_box(v[0], v[1], v[2])
    assert words[0, 7] & 0xFF == OP_BOX and words[1, 7] & 0xFF == OP_TRI and words[0, 6] == 3
    assert_bit_equal(words[0, :6].view(f32), np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], f32), "leaf box")
    assert not b.flatten([b.sphere(1.0, lam)])[1] & FEAT_TRI
    # a triangle flat in an axis still has a box with end > start on it
    flat = b.bvh([b.triangle((0, 0, 0), (1, 0, 0), (0, 0, 1), lam)], exposure=(0.0, 0.0))
    box = b.flatten([flat])[0][0, :6].view(f32)
    assert (box[1::2] > box[0::2]).all()


def test_a_triangle_is_no_plain_primitive(pkg):
    """No second program, no hoisted segment: a world of the pool-2 shape gets neither once one triangle is added."""
    be = pkg.load()
    OP_SEG = 9

    def world(b, with_triangle):
        lam = b.lambertian(b.constant((0.5, 0.5, 0.5)))
        spheres = [b.translate((float(i), 0.0, 0.0), b.sphere(0.4, lam)) for i in range(4)]
        w = [b.rect(1, (-5, 5), (-5, 5), -1.0, lam), b.rect(1, (-5, 5), (-5, 5), 3.0, lam), b.bvh(spheres)]
        return w + ([b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), lam)] if with_triangle else [])

    b = be.builder()
    w = world(b, False)
    assert len(b.flatten_pool2(w)[0]) > 0 and OP_SEG in (b.flatten(w)[0][:, 7] & 0xFF)
    b = be.builder()
    w = world(b, True)
    words, feat = b.flatten(w)
    assert feat & FEAT_TRI and OP_SEG not in (words[:, 7] & 0xFF)
    p2_words, items, n_media, n_wrapped = b.flatten_pool2(w)
    assert len(p2_words) == 0 and items == []
    # ... and below a Bvh of that world, and under a wrapper
    b = be.builder()
    w = world(b, False)
    lam = b.lambertian(b.constant((0.5, 0.5, 0.5)))
    for extra in (b.bvh([b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), lam), b.sphere(1.0, lam)]),
                  b.flip_normals(b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), lam))):
        assert len(b.flatten_pool2(w + [extra])[0]) == 0 and OP_SEG not in (b.flatten(w + [extra])[0][:, 7] & 0xFF)


@pytest.mark.parametrize("sah", [False, True])
def test_a_mesh_is_the_hand_made_bvh_over_triangles(pkg, sah):
    be, T = pkg.load(), pkg.triangle
    for v, f in (T.icosphere(2), T.box((-1, -2, -3), (1, 2, 3)), T.grid(5, 3, lambda x, z: x * z)):
        b = be.builder()
        lam = b.lambertian(b.constant((0.5, 0.5, 0.5)))
        mesh = b.mesh(v, f, lam, sah=sah)
        tv = T.vertices_of(v, f)
        ids = [b.triangle(t[0], t[1], t[2], lam) for t in tv]
        hand = (b.bvh_sah if sah else b.bvh)(ids, exposure=(0.0, 0.0))
        a, fa = b.flatten([mesh])
        c, fc = b.flatten([hand])
        assert_same_words(a, c)
        assert fa == fc and fa & FEAT_TRI and a[0, 7] & F_BVH_ROOT
        assert (a[:, 7] & 0xFF == OP_TRI).sum() == len(f) and (a[:, 7] & 0xFF == OP_BOX).sum() == 2 * len(f) - 1


def test_a_mesh_of_2000_triangles_builds(pkg):
    be, T = pkg.load(), pkg.triangle
    v, f = T.grid(40, 25, lambda x, z: 0.1 * np.sin(9 * x) + 0.05 * np.cos(7 * z))
    assert len(f) == 2000
    for sah in (False, True):
        b = be.builder()
        words, feat = b.flatten([b.mesh(v, f, b.lambertian(b.constant((0.5, 0.5, 0.5))), sah=sah)])
        assert len(words) == 2 * 2000 + 3999 + 1 and feat & FEAT_TRI


# ---- generators and the OBJ reader ------------------------------------------------------------------------------------------------
def test_the_generators_wind_outwards(pkg):
    T = pkg.triangle
    for sub, count in ((0, 20), (1, 80), (2, 320), (3, 1280)):
        v, f = T.icosphere(sub, radius=2.5, centre=(1.0, -2.0, 3.0))
        assert v.dtype == np.float32 and f.dtype == np.uint32 and len(f) == count and len(v) == 10 * 4 ** sub + 2
        tv = T.vertices_of(v, f)
        _, _, _, nn = T.record(tv[:, 0], tv[:, 1], tv[:, 2])
        assert (((tv.mean(axis=1) - np.array([1.0, -2.0, 3.0], f32)) * nn).sum(axis=1) > 0.9 * 2.5 * 0.75).all()
        assert np.allclose(np.linalg.norm(v - np.array([1.0, -2.0, 3.0]), axis=1), 2.5, rtol=1e-6)
        assert np.isfinite(T.length(tv[:, 0], tv[:, 1], tv[:, 2])).all() and (T.length(tv[:, 0], tv[:, 1], tv[:, 2]) > 0).all()
    v, f = T.box((-1.0, 0.0, 2.0), (1.0, 3.0, 2.5))
    assert len(v) == 8 and len(f) == 12
    tv = T.vertices_of(v, f)
    _, _, _, nn = T.record(tv[:, 0], tv[:, 1], tv[:, 2])
    out = tv.mean(axis=1) - np.array([0.0, 1.5, 2.25], f32)
    assert ((out * nn).sum(axis=1) > 0).all() and (np.abs(nn).max(axis=1) == 1.0).all()       # axis normals, away from the centre
    assert sorted(map(tuple, nn.astype(int))) == sorted([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] * 2)
    v, f = T.grid(4, 3, lambda x, z: 0.5 * x - 0.25 * z, (0.0, 0.0), (4.0, 3.0))
    assert len(v) == 20 and len(f) == 24
    tv = T.vertices_of(v, f)
    assert (T.record(tv[:, 0], tv[:, 1], tv[:, 2])[3][:, 1] > 0).all()                         # front faces look up
    assert np.allclose(v[:, 1], 0.5 * v[:, 0] - 0.25 * v[:, 2])


def test_load_obj_reads_the_fixture(pkg, tmp_path):
    T = pkg.triangle
    v, f = T.load_obj(os.path.join(ROOT, "tests", "golden", "mesh_fixture.obj"))
    assert v.dtype == np.float32 and f.dtype == np.uint32
    assert_bit_equal(v, np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1], [0.5, 1, 0.5]], f32))
    # the quad is a fan of two; `/vt/vn` suffixes are ignored; -2 -1 -5 count back from the five vertices
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 4, 1], [1, 4, 2], [2, 4, 3], [3, 4, 0]]
    tv = T.vertices_of(v, f)
    nn = T.record(tv[:, 0], tv[:, 1], tv[:, 2])[3]
    assert (((tv.mean(axis=1) - np.array([0.5, 0.3, 0.5], f32)) * nn).sum(axis=1) > 0).all()      # a closed pyramid, outward
    b = pkg.load().builder()
    b.mesh(v, f, b.lambertian(b.constant((0.5, 0.5, 0.5))))
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        T.load_obj(str(bad))


# ---- rt_triangle.h on its own -----------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rt_triangle.h"
template <class T>
static std::vector<T> slurp(const char* path) {
  std::vector<T> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::printf("cannot open %s\n", path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / sizeof(T));
  if (bytes && std::fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) { std::printf("short read %s\n", path); std::exit(2); }
  std::fclose(f);
  return v;
}
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const std::vector<float> tri = slurp<float>(argv[1]), rays = slurp<float>(argv[2]), want = slurp<float>(argv[3]);
  const float t_min = (float)std::atof(argv[4]);
  const size_t n = tri.size() / 9;
  if (tri.size() % 9 || rays.size() != 8 * n || want.size() != 8 * n) { std::printf("bad sizes\n"); return 2; }
  long hits = 0, diffs = 0;
  for (size_t i = 0; i < n; i++) {
    const float *v = &tri[9 * i], *r = &rays[8 * i];
    rtg::Tri3 e1, e2, nn;
    const rtg::Tri3 v0{v[0], v[1], v[2]}, o{r[0], r[1], r[2]}, d{r[3], r[4], r[5]};
    (void)rtg::tri_record(v0, rtg::Tri3{v[3], v[4], v[5]}, rtg::Tri3{v[6], v[7], v[8]}, e1, e2, nn);
    float out[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t = 0.f;
    if (rtg::tri_hit_t(v0, e1, e2, o, d, t_min, r[7], t)) {
      out[0] = 1.f, out[1] = t, out[2] = o.x + t * d.x, out[3] = o.y + t * d.y, out[4] = o.z + t * d.z, out[5] = nn.x, out[6] = nn.y, out[7] = nn.z;
      hits++;
    }
    bool same = true;
    for (int k = 0; k < 8; k++) same = same && (bits(out[k]) == bits(want[8 * i + k]) || (out[k] != out[k] && want[8 * i + k] != want[8 * i + k]));
    if (!same && diffs++ < 5) std::printf("DIFF pair %zu: got %a %a, want %a %a\n", i, out[0], out[1], want[8 * i], want[8 * i + 1]);
  }
  std::printf("pairs %zu hits %ld diffs %ld\n", n, hits, diffs);
  return 0;
}
"""


def test_rt_triangle_h_stands_alone_plain_and_sanitized(pkg, tmp_path):
    """A g++ program of its own includes csrc/rt_triangle.h and answers the edge cases of the host probe with the definition's
    bits -- at -O2, and with the address and undefined-behaviour sanitizers linked into that program (none is loaded into
    Python)."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the stand-alone triangle program")
    tri9, rays8 = MC.edge_pairs()
    want, ok = _definition_out8(pkg.triangle, tri9, rays8, MC.T_MIN)
    src = tmp_path / "triangle_alone.cpp"
    src.write_text(PROGRAM)
    paths = {}
    for key, arr in (("tri", tri9), ("rays", rays8), ("want", want)):
        paths[key] = tmp_path / (key + ".bin")
        np.ascontiguousarray(arr, f32).tofile(str(paths[key]))
    for name, extra in (("plain", ["-O2"]),
                        ("san", ["-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / ("triangle_alone_" + name)
        subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"] + extra
                              + ["-I", CSRC, str(src), "-o", str(exe)])
        r = subprocess.run([str(exe), str(paths["tri"]), str(paths["rays"]), str(paths["want"]), repr(MC.T_MIN)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        last = r.stdout.splitlines()[-1].split()
        got = dict(zip(last[0::2], map(int, last[1::2])))
        print(name, got)
        assert got == {"pairs": len(tri9), "hits": int(ok.sum()), "diffs": 0}, r.stdout[-2000:]
