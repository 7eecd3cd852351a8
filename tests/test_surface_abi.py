"""Surface attributes, CPU side (include/rtiow_gpu_surface.h; Builder.triangle_attr / mesh(normals, uvs) / surface; triangle.py
shade): the header declares exactly its five entry points with the binding's and the Rust module's prototypes and stays out of the
other symbol lists; the refusals; the records; the host probe against the numpy definition, bit for bit; the definition against
float64 (surface_cases.py); the closed-form anchor on the icosphere; the OBJ reader; rt_triangle.h stand-alone, plain and
sanitized."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import assert_bit_equal
import mesh_cases as MC
import surface_cases as SC
import triangle_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtiow_gpu_surface.h")
SURFACE_RS = os.path.join(ROOT, "rtiow-rust_amd", "host", "rust", "rtiow-gpu-sys", "src", "surface.rs")
CSRC = os.path.join(ROOT, "rtiow-rust_amd", "csrc")
NAMES = ["object_triangle_attr", "object_mesh_attr", "texture_surface", "debug_triangle_attr_host", "debug_hit_surface"]
INVALID_ID = 0xFFFFFFFF
OP_BOX, OP_EXT, OP_TRI = 1, 12, 14                                   # csrc/flat_scene.h
F_FLIP, F_TRI_NORMALS, F_TRI_UVS, F_TEXTURED = 1 << 9, 1 << 10, 1 << 11, 1 << 19
FEAT_TEXTURE, FEAT_TRI, FEAT_SURFACE = 8, 1024, 2048
f32 = np.float32
fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def _prototypes(text, strip, pattern):
    text = re.sub(strip, "", text, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip()] for m in re.finditer(pattern, text, flags=re.S)}


def test_the_header_declares_exactly_the_five_entry_points(pkg):
    text = open(HEADER).read()
    c_fns = _prototypes(text, r"/\*.*?\*/", r"\b(rtg_\w+)\s*\(([^)]*)\)\s*;")
    assert sorted(c_fns) == sorted("rtg_" + n for n in NAMES)
    assert pkg.capi.SURFACE_SYMBOLS == NAMES
    assert '#include "rtiow_gpu.h"' in text and "not part of the ABI of rtiow_gpu.h" in text
    names = lambda fn: [re.sub(r"\[\d*\]", "", a.split()[-1]).lstrip("*") for a in c_fns[fn]]   # noqa: E731
    assert names("rtg_object_triangle_attr") == ["b", "v0", "v1", "v2", "normals9", "uvs6", "material"]
    assert names("rtg_object_mesh_attr") == ["b", "vertices", "n_vertices", "indices", "n_triangles", "normals", "uvs", "material", "sah"]
    assert names("rtg_texture_surface") == ["b", "child"]
    assert names("rtg_debug_triangle_attr_host") == ["n", "tri9", "attr15", "has", "rays8", "t_min", "out10"]
    assert names("rtg_debug_hit_surface") == ["s", "n", "rays7", "seed", "t_near", "out10", "mat"]
    be = pkg.load()
    for n, argc, res in zip(NAMES, (7, 9, 2, 7, 7), (C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int)):
        fn = getattr(be.lib, "rtg_" + n)
        assert fn.restype is res and len(fn.argtypes) == argc, n


def test_they_stay_out_of_the_other_lists_and_the_rust_module_follows_the_header(pkg):
    capi = pkg.capi
    for other in (capi.ABI_SYMBOLS, capi.QUERY_SYMBOLS, capi.RAY_FRAME_SYMBOLS, capi.IMAGE_SYMBOLS, capi.MESH_SYMBOLS):
        assert not set(NAMES) & set(other)
    for header in ("rtiow_gpu.h", "rtiow_gpu_mesh.h", "rtiow_gpu_image.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for n in NAMES:
            assert "rtg_" + n not in text, (header, n)
    c_fns = _prototypes(open(HEADER).read(), r"/\*.*?\*/", r"\b(rtg_\w+)\s*\(([^)]*)\)\s*;")
    rs_fns = _prototypes(open(SURFACE_RS).read(), r"//[^\n]*", r"pub fn (rtg_\w+)\s*\(([^)]*)\)")
    assert sorted(rs_fns) == sorted(c_fns)
    for name in c_fns:
        assert len(rs_fns[name]) == len(c_fns[name]), name
    lib_rs = open(os.path.join(os.path.dirname(SURFACE_RS), "lib.rs")).read()
    assert "pub mod surface;" in lib_rs
    for n in NAMES:
        assert "rtg_" + n not in lib_rs, n


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_builder_as_it_was(pkg):
    be, T = pkg.load(), pkg.triangle
    b = be.builder()
    grey = b.constant((0.5, 0.5, 0.5))
    mat = b.lambertian(grey)
    surf = b.surface(grey)
    smat, slit = b.lambertian(surf), b.diffuse_light(surf, 2.0)
    v, f, nn, uv = T.icosphere_attr(1)
    A, B_, C_ = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    N9, U6 = np.array([0, 0, 1] * 3, f32), np.array([0, 0, 1, 0, 0, 1], f32)
    first = b.triangle_attr(A, B_, C_, smat, normals=N9, uvs=U6)
    good = b.mesh(v, f, slit, normals=nn, uvs=uv)
    assert good == first + 1 + len(f)
    before, feat_before = b.flatten([first, good])
    next_tex = surf + 1

    def refused(got):
        return got == INVALID_ID and be.last_error() != ""

    def tri(v0=A, v1=B_, v2=C_, n9=N9, u6=U6, m=smat, builder=b.h):
        a = [None if x is None else (C.c_float * 3)(*x) for x in (v0, v1, v2)]
        return refused(be._object_triangle_attr(builder, a[0], a[1], a[2], None if n9 is None else n9.ctypes.data_as(fp),
                                                None if u6 is None else u6.ctypes.data_as(fp), m))

    # everything rtg_object_triangle refuses
    assert tri(v0=None) and tri(v1=None) and tri(v2=None) and tri(builder=None) and tri(m=slit + 1) and tri(m=INVALID_ID)
    assert tri(v1=A) and tri(v2=(2.0, 0.0, 0.0)) and tri(v1=(np.nan, 0.0, 0.0)) and tri(v1=(1e30, 0.0, 0.0), v2=(0.0, 1e30, 0.0))
    # a non-finite normal or UV component; a surface material on a triangle without UVs
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(9):
            n9 = N9.copy()
            n9[k] = bad
            assert tri(n9=n9), (bad, k)
        for k in range(6):
            u6 = U6.copy()
            u6[k] = bad
            assert tri(u6=u6), (bad, k)
    assert tri(u6=None) and tri(u6=None, n9=None) and tri(u6=None, m=slit)
    assert refused(be._object_triangle(b.h, (C.c_float * 3)(*A), (C.c_float * 3)(*B_), (C.c_float * 3)(*C_), smat))
    # the mesh: as a whole
    vp, ip, np_, uvp = v.ctypes.data_as(fp), f.ctypes.data_as(up), nn.ctypes.data_as(fp), uv.ctypes.data_as(fp)

    def mesh(vertices=vp, n_v=len(v), indices=ip, n_t=len(f), normals=np_, uvs=uvp, m=slit, sah=0, builder=b.h):
        return refused(be._object_mesh_attr(builder, vertices, n_v, indices, n_t, normals, uvs, m, sah))

    assert mesh(builder=None) and mesh(vertices=None) and mesh(indices=None) and mesh(m=slit + 1) and mesh(sah=2) and mesh(n_t=0)
    assert mesh(n_v=len(v) - 1) and mesh(uvs=None) and mesh(uvs=None, normals=None)        # (a surface material without UVs)
    late_n, late_uv = nn.copy(), uv.copy()
    late_n[int(f[-1, 2]), 1] = np.nan                                                          # found in the LAST triangle
    late_uv[int(f[-1, 1]), 0] = np.inf
    assert mesh(normals=late_n.ctypes.data_as(fp)) and mesh(uvs=late_uv.ctypes.data_as(fp))
    assert refused(be._object_mesh(b.h, vp, len(v), ip, len(f), smat, 0))
    # the surface texture: not a checker child, not its own child, not an isotropic albedo; no other object takes its materials
    assert refused(be._texture_checker(b.h, surf, grey)) and refused(be._texture_checker(b.h, grey, surf))
    assert refused(be._texture_surface(b.h, surf)) and refused(be._texture_surface(b.h, next_tex)) and refused(be._texture_surface(None, grey))
    assert refused(be._material_isotropic(b.h, surf))
    img = b.image(np.ones((2, 2, 3), f32), pkg.image.planar((1, 0, 0), 0.0, (0, 1, 0), 0.0))
    assert refused(be._texture_surface(b.h, img + 1))                                          # (an image's continuation slot)
    next_tex = img + 2
    assert refused(be._object_sphere(b.h, 1.0, smat)) and refused(be._object_rect(b.h, 1, 0.0, 1.0, 0.0, 1.0, 0.0, slit))
    assert refused(be._object_rect_prism(b.h, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), smat))
    assert refused(be._object_constant_medium(b.h, first, 0.5, smat))
    # nothing moved
    after, feat_after = b.flatten([first, good])
    assert np.array_equal(before, after) and feat_before == feat_after
    assert b.constant((0.1, 0.1, 0.1)) == next_tex
    assert b.lambertian(grey) == slit + 1
    assert b.triangle_attr(A, B_, C_, smat, uvs=U6) == good + 1
    again = b.mesh(v, f, slit, sah=True, normals=nn, uvs=uv)
    assert again == good + 2 + len(f)
    hand = b.bvh_sah(list(range(good + 2, good + 2 + len(f))), exposure=(0.0, 0.0))
    assert np.array_equal(b.flatten([again])[0], b.flatten([hand])[0])
    # every texture rtg_material_lambertian takes is a child; the host probe answers with the child at (p.x, p.y, 0)
    p = np.random.RandomState(3).uniform(-2, 2, (64, 3)).astype(f32)
    s_img = b.surface(img)
    flat = p.copy()
    flat[:, 2] = 0.0
    assert_bit_equal(b.texture_host(s_img, p), b.texture_host(img, flat), "rtg_debug_texture_host of a surface texture")
    assert_bit_equal(b.texture_host(surf, p), b.texture_host(grey, p))


def test_without_attributes_they_are_the_plain_calls(pkg):
    be, T = pkg.load(), pkg.triangle
    v, f = T.icosphere(1)
    worlds = []
    for attr in (False, True):
        b = be.builder()
        mat = b.lambertian(b.constant((0.5, 0.5, 0.5)))
        if attr:
            t = b.triangle_attr((0, 0, 0), (1, 0, 0), (0, 1, 0), mat)
            m = be.check_id(be._object_mesh_attr(b.h, v.ctypes.data_as(fp), len(v), f.ctypes.data_as(up), len(f), None, None, mat, 1))
        else:
            t = b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), mat)
            m = b.mesh(v, f, mat, sah=True)
        worlds.append((t, m, b.flatten([t, b.flip_normals(t), m])))
    (t0, m0, (w0, f0)), (t1, m1, (w1, f1)) = worlds
    assert (t0, m0) == (t1, m1) and np.array_equal(w0, w1) and f0 == f1
    assert f0 & FEAT_TRI and not f0 & FEAT_SURFACE


# ---- records ------------------------------------------------------------------------------------------------------------------
def test_the_records_hold_the_definition_s_words(pkg):
    be, T = pkg.load(), pkg.triangle
    b = be.builder()
    grey = b.constant((0.5, 0.5, 0.5))
    lam = b.lambertian(grey)
    img = b.image(np.ones((2, 2, 3), f32), pkg.image.planar((1, 0, 0), 0.0, (0, 1, 0), 0.0))
    mapped, flat_mapped = b.lambertian(b.surface(img)), b.lambertian(b.surface(grey))
    v = np.array([[0.25, -0.5, 1.0], [1.5, 0.25, 0.75], [-0.25, 1.25, 1.5]], f32)
    nn = np.array([[0.1, 0.2, 0.9], [0.0, 0.0, 0.0], [-0.3, 0.4, 1.5]], f32)           # as given: not normalised, one zero
    uv = np.array([[0.0, 0.25], [1.0, 0.5], [0.5, -2.0]], f32)
    plain = b.triangle(v[0], v[1], v[2], lam)
    both = b.triangle_attr(v[0], v[1], v[2], mapped, normals=nn, uvs=uv)
    only_n = b.flip_normals(b.triangle_attr(v[0], v[1], v[2], lam, normals=nn))
    only_uv = b.triangle_attr(v[0], v[1], v[2], flat_mapped, uvs=uv)
    words, feat = b.flatten([plain, both, only_n, only_uv])
    assert feat & FEAT_TRI and feat & FEAT_SURFACE and feat & FEAT_TEXTURE
    assert [int(w) & 0xFF for w in words[:, 7]] == [OP_TRI, OP_EXT] + [OP_TRI, OP_EXT, OP_EXT, OP_EXT] * 3 + [0]
    _, e1, e2, face = T.record(v[0], v[1], v[2])
    assert words[0, 7] & (F_TRI_NORMALS | F_TRI_UVS) == 0 and words[1, 6] == 0
    zero9, zero6 = np.zeros(9, f32), np.zeros(6, f32)
    for k, (mat, flip, has_n, has_uv, textured) in enumerate(((mapped, False, True, True, True), (lam, True, True, False, False),
                                                              (flat_mapped, False, False, True, False))):
        r = words[2 + 4 * k: 6 + 4 * k]
        assert_bit_equal(r[0, :6].view(f32), np.concatenate([v[0], e1]), "v0, e1")
        assert_bit_equal(r[1, :6].view(f32), np.concatenate([e2, face]), "e2, N")
        assert r[0, 6] == mat and bool(r[0, 7] & F_FLIP) == flip and bool(r[0, 7] & F_TEXTURED) == textured
        assert bool(r[0, 7] & F_TRI_NORMALS) == has_n and bool(r[0, 7] & F_TRI_UVS) == has_uv
        attr = np.concatenate([r[1, 6:7], r[2, :7], r[3, :7]]).view(f32)
        assert_bit_equal(attr, np.concatenate([nn.ravel() if has_n else zero9, uv.ravel() if has_uv else zero6]), "n0 n1 n2 uv0 uv1 uv2")
        assert (r[1:, 7] == OP_EXT).all()
    # the BOX above an attribute triangle is the plain triangle's, its skip pointer behind the four records
    lo, hi = T.bounding_box(v[0], v[1], v[2])
    a, fa = b.flatten([b.bvh([both], exposure=(0.0, 0.0))])
    p, fpl = b.flatten([b.bvh([plain], exposure=(0.0, 0.0))])
    assert np.array_equal(a[0, :6], p[0, :6]) and a[0, 7] == p[0, 7] and a[0, 6] == 5 and p[0, 6] == 3
    assert_bit_equal(a[0, :6].view(f32), np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]], f32), "leaf box")
    assert fa & FEAT_SURFACE and not fpl & FEAT_SURFACE
    assert not b.flatten([plain, b.sphere(1.0, lam)])[1] & FEAT_SURFACE
    # under wrappers the PUSH / POP pointers count the four records
    w, _ = b.flatten([b.translate((1.0, 0.0, 0.0), b.scale((2.0, 2.0, 2.0), both))])
    assert [int(x) & 0xFF for x in w[:, 7]] == [4, 4, OP_TRI, OP_EXT, OP_EXT, OP_EXT, 5, 5, 0] and w[0, 6] == 7 and w[1, 6] == 6


@pytest.mark.parametrize("sah", [False, True])
def test_a_mesh_is_the_hand_made_bvh_over_attribute_triangles(pkg, sah):
    be, T = pkg.load(), pkg.triangle
    for v, f in (T.icosphere(2), T.box((-1, -2, -3), (1, 2, 3)), T.grid(5, 3, lambda x, z: x * z)):
        nn, uv = SC.vertex_attributes(T, v, f)
        for use_n, use_uv in ((True, True), (True, False), (False, True)):
            b = be.builder()
            lam = b.lambertian(b.constant((0.5, 0.5, 0.5)))
            mesh = b.mesh(v, f, lam, sah=sah, normals=nn if use_n else None, uvs=uv if use_uv else None)
            ids = [b.triangle_attr(v[t[0]], v[t[1]], v[t[2]], lam, normals=nn[t] if use_n else None, uvs=uv[t] if use_uv else None) for t in f.astype(np.int64)]
            hand = (b.bvh_sah if sah else b.bvh)(ids, exposure=(0.0, 0.0))
            a, fa = b.flatten([mesh])
            c, fc = b.flatten([hand])
            assert np.array_equal(a, c) and fa == fc and fa & FEAT_SURFACE
            assert (a[:, 7] & 0xFF == OP_TRI).sum() == len(f) and (a[:, 7] & 0xFF == OP_BOX).sum() == 2 * len(f) - 1 and len(a) == 4 * len(f) + 2 * len(f)


# ---- the host probe against the definition --------------------------------------------------------------------------------------
def _definition_out10(T, tri9, attr15, has, rays8, t_min):
    rec = T.record(tri9[:, 0:3], tri9[:, 3:6], tri9[:, 6:9])
    ok, t, p, _ = T.hit(rec, rays8[:, 0:3], rays8[:, 3:6], f32(t_min), rays8[:, 7])
    nn, tu, tv = T.shade(rec, attr15[:, 0:9].reshape(-1, 3, 3) if has & 1 else None, attr15[:, 9:15].reshape(-1, 3, 2) if has & 2 else None,
                         rays8[:, 0:3], rays8[:, 3:6])
    ref = np.zeros((len(tri9), 10), f32)
    ref[ok, 0], ref[ok, 1], ref[ok, 2:5], ref[ok, 5:8], ref[ok, 8], ref[ok, 9] = 1.0, t[ok], p[ok], nn[ok], tu[ok], tv[ok]
    return ref, ok


def _edge_attr_pairs():
    """edge_pairs() with random attributes, then hits on u = 0, v = 0, u + v = 1 and the corners of a triangle where the
    arithmetic is exact, then zero and opposing normal triples."""
    tri9, rays8 = MC.edge_pairs()
    rs = np.random.RandomState(17)
    attr = np.concatenate([rs.normal(0, 1, (len(tri9), 9)), rs.uniform(-2, 3, (len(tri9), 6))], axis=1).astype(f32)
    base = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], f32)
    t_x, r_x, a_x = [], [], []
    corner_attr = np.array([0, 0, 2, 3, 0, 4, 0, -5, 12, 0.25, 0.5, 0.75, -1.0, 2.0, 8.0], f32)
    points = [(0.0, 0.5), (0.5, 0.0), (0.5, 0.5), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.25, 0.25)]
    for x, y in points:
        t_x.append(base), r_x.append([x, y, 1.0, 0, 0, -1.0, 0, 10.0]), a_x.append(corner_attr)
    for triple in ([0] * 9, [0, 0, 1, 0, 0, -1, 0, 0, 0], [1, 0, 0, -1, 0, 0, 5, 0, 0], [np.float32(3e38)] * 9, [1e-30] * 9):
        for x, y in ((0.5, 0.0), (0.25, 0.25), (0.0, 0.0)):
            t_x.append(base), r_x.append([x, y, 1.0, 0, 0, -1.0, 0, 10.0]), a_x.append(np.concatenate([np.asarray(triple, f32), corner_attr[9:]]))
    return (np.concatenate([tri9, np.asarray(t_x, f32)]), np.concatenate([attr, np.asarray(a_x, f32)]),
            np.concatenate([rays8, np.asarray(r_x, f32)]), len(tri9), len(points))


def test_the_host_probe_equals_the_definition_bit_for_bit(pkg):
    be, T = pkg.load(), pkg.triangle
    tri9, attr, rays8, n_edge, n_points = _edge_attr_pairs()
    for has in (3, 1, 2, 0):
        ref, ok = _definition_out10(T, tri9, attr, has, rays8, MC.T_MIN)
        got = be.triangle_attr_host(tri9, attr, has, rays8, MC.T_MIN)
        assert_bit_equal(got, ref, "rtg_debug_triangle_attr_host against triangle.hit + triangle.shade, has = %d" % has)
        if has == 0:
            assert_bit_equal(got[:, :8], be.triangle_host(tri9, rays8, MC.T_MIN), "has = 0: the plain probe")
            assert not got[:, 8:].any()
    ref, ok = _definition_out10(T, tri9, attr, 3, rays8, MC.T_MIN)
    print("pairs %d, hits %d" % (len(tri9), ok.sum()))
    assert ok[n_edge:].all() and 0.25 * 4096 < ok[:4096].sum() < 0.75 * 4096
    # at a corner: that vertex's normalised normal and its UV exactly; on an edge the two ends' alone
    x = ref[n_edge:n_edge + n_points]
    unit = lambda n: (np.asarray(n, f32) / np.sqrt(np.sum(np.asarray(n, f32) ** 2, dtype=f32)))   # noqa: E731
    assert_bit_equal(x[3, 5:10], np.array([0, 0, 1, 0.25, 0.5], f32), "corner v0")
    assert_bit_equal(x[4, 5:10], np.array([0.6, 0, 0.8, 0.75, -1.0], f32), "corner v1")
    assert_bit_equal(x[5, 5:10], np.concatenate([unit([0, -5, 12]), [2.0, 8.0]]).astype(f32), "corner v2")
    assert_bit_equal(x[1, 8:10], np.array([0.5, -0.25], f32), "edge v = 0: halfway between uv0 and uv1")
    assert_bit_equal(x[0, 8:10], np.array([1.125, 4.25], f32), "edge u = 0: halfway between uv0 and uv2")
    assert_bit_equal(x[2, 8:10], np.array([1.375, 3.5], f32), "edge u + v = 1: halfway between uv1 and uv2")
    # len == 0 (a zero triple, an opposing pair), len overflowing: the face normal; a tiny triple normalises
    y = ref[n_edge + n_points:].reshape(5, 3, 10)
    face = np.array([0, 0, 1], f32)
    for k in (0, 3):
        assert_bit_equal(y[k, :, 5:8], np.broadcast_to(face, (3, 3)), "fallback to N")
    assert_bit_equal(y[1, 0, 5:8], face, "n0 = -n1 at the midpoint of their edge")
    assert_bit_equal(y[2, 0, 5:8], face, "n0 = -n1 (x) at the midpoint")
    assert np.allclose(np.linalg.norm(y[4, :, 5:8], axis=1), 1.0, atol=1e-6)
    assert be.triangle_attr_host(tri9[:0], attr[:0], 3, rays8[:0]).shape == (0, 10)
    with pytest.raises(Exception):
        be.triangle_attr_host(tri9[:1], attr[:1], 4, rays8[:1])


def test_flips_and_the_list_fold(pkg):
    T = pkg.triangle
    tris = MC.list_triangles(7)
    attrs = SC.list_attributes(T, tris)
    rays = MC.edge_rays(tris)
    flips = [i % 3 == 1 for i in range(7)]
    out, index = T.closest_attr(tris, [a[0] for a in attrs], [a[1] for a in attrs], rays, MC.T_MIN, flips=flips)
    plain, p_index = T.closest(tris, rays, MC.T_MIN, flips=flips)
    assert np.array_equal(index, p_index)
    assert_bit_equal(out[:, :5], plain[:, :5], "attributes do not move the hit flag, t or p")
    no_n = np.isin(index, [i for i, a in enumerate(attrs) if a[0] is None])
    assert_bit_equal(out[no_n, 5:8], plain[no_n, 5:8], "a triangle without normals shades with N")
    no_uv = np.isin(index, [i for i, a in enumerate(attrs) if a[1] is None])
    assert not out[no_uv, 8:].any() and out[~no_uv & (index >= 0), 8:].any()
    unflipped, _ = T.closest_attr(tris, [a[0] for a in attrs], [a[1] for a in attrs], rays, MC.T_MIN)
    fl = np.isin(index, [i for i in range(7) if flips[i]])
    assert_bit_equal(out[fl, 5:8], -unflipped[fl, 5:8])
    assert_bit_equal(out[~fl], unflipped[~fl])


# ---- the definition against float64 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def references(pkg):
    out = {}
    be = pkg.load()
    for name in MC.GRAPHS:
        world, groups = SC.graph(pkg, be.builder(), name)
        rays = MC.aimed_rays(groups).astype(f32)
        r64 = rays.astype(np.float64)
        out[name] = (groups, rays, TR.closest_hit64(groups, r64[:, 0:3], r64[:, 3:6], r64[:, 6]))
    return out


@pytest.mark.parametrize("name", list(MC.GRAPHS))
def test_the_definition_against_float64(pkg, references, name):
    groups, rays, ref = references[name]
    out, mat, index = SC.closest32_attr(pkg.triangle, groups, rays)
    plain, p_mat, p_index = TR.closest32(pkg.triangle, groups, rays)
    assert np.array_equal(index, p_index) and np.array_equal(out[:, :5].view(np.uint32), plain[:, :5].view(np.uint32))
    use = ref["margin"] > TR.MARGIN
    assert not (use & ref["hit"] & (index != ref["triangle"])).any()
    SC.assert_attr(SC.compare_attr(groups, ref, rays, out), name)


def test_the_closed_form_anchor_on_the_icosphere(pkg):
    """On icosphere_attr the interpolated, normalised normal is (p - centre) / |p - centre|: p - centre = r (w n0 + u n1 + v n2)
    in real arithmetic."""
    T = pkg.triangle
    centre, radius = np.array([0.5, -0.25, 1.0]), 1.5
    v, f, nn, uv = T.icosphere_attr(2, radius, tuple(centre))
    ix = f.astype(np.int64)
    groups = [{"tri": T.vertices_of(v, f), "chain": (), "sign": 1, "mat": 0, "normals": nn[ix], "uvs": uv[ix]}]
    rays = MC.aimed_rays(groups).astype(f32)
    r64 = rays.astype(np.float64)
    ref = TR.closest_hit64(groups, r64[:, 0:3], r64[:, 3:6], r64[:, 6])
    out, _, _ = SC.closest32_attr(T, groups, rays)
    use = (ref["margin"] > TR.MARGIN) & ref["hit"] & (out[:, 0] != 0)
    want = ref["p"][use] - centre
    want /= np.linalg.norm(want, axis=1)[:, None]
    worst = float(np.abs(out[use, 5:8].astype(np.float64) - want).max())
    print("anchor: %d rays, left out %.2f %%, worst %.2e" % (use.sum(), 100 * (1 - (ref["margin"] > TR.MARGIN).mean()), worst))
    assert (1 - (ref["margin"] > TR.MARGIN).mean()) <= TR.CAP_RAYS and use.sum() > 1000
    assert worst <= SC.ANCHOR_TOL
    assert np.abs(np.linalg.norm(nn, axis=1) - 1).max() < 1e-6 and (uv >= 0).all() and (uv <= 1).all()
    # vertex_normals: unit, and inside the cone of the faces around the vertex -- every face normal of this mesh is within an edge's
    # angle of its corners' radial directions (an icosahedron's 63.4 degrees, halved twice), and a normalised sum of vectors of a
    # convex cone stays in it
    vn = T.vertex_normals(v, f)
    assert np.abs(np.linalg.norm(vn, axis=1) - 1).max() < 1e-6 and ((vn * nn).sum(axis=1) > np.cos(np.deg2rad(63.435 / 4))).all()
    flat_v, flat_f = T.grid(3, 2, lambda x, z: 0.0)
    assert_bit_equal(T.vertex_normals(flat_v, flat_f), np.broadcast_to(np.array([0, 1, 0], f32), (12, 3)), "a flat grid: +y everywhere")


# ---- the OBJ reader -------------------------------------------------------------------------------------------------------------
def test_load_obj_attr_reads_the_fixture(pkg, tmp_path):
    T = pkg.triangle
    path = os.path.join(ROOT, "tests", "golden", "surface_fixture.obj")
    v, f, nn, uv = T.load_obj_attr(path)
    assert v.dtype == np.float32 and f.dtype == np.uint32 and nn.dtype == np.float32 and uv.dtype == np.float32
    # 5 positions, but the apex is used with two (vt, vn) pairs and base corners with up to three: unified, in order of first use
    assert len(v) == len(nn) == len(uv) == 10
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 8, 9]]                   # the quad is a fan of two; negative indices count back
    assert_bit_equal(v[[0, 1, 2, 3]], np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1]], f32))
    assert_bit_equal(v[6], np.array([0.5, 1, 0.5], f32))
    assert_bit_equal(v[4], v[0])
    assert_bit_equal(v[5], v[1])
    assert_bit_equal(uv[[0, 1, 2, 3]], np.array([[0, 0], [1, 0], [1, 1], [0, 1]], f32))
    assert_bit_equal(nn[0], np.array([0, -1, 0], f32))
    assert_bit_equal(nn[4], np.array([0, 0.5, -1], f32))
    assert_bit_equal(uv[6], np.array([0.5, 1], f32))
    assert_bit_equal(uv[9], np.array([0.25, 0.75], f32))
    assert_bit_equal(v[9], v[6])
    assert_bit_equal(v[7], v[1])
    assert_bit_equal(nn[9], np.array([1, 0.5, 0], f32))
    pv, pf = T.load_obj(path)                                                           # load_obj: its old answer on the same file
    assert len(pv) == 5 and pf.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4]]
    assert np.array_equal(T.vertices_of(pv, pf), T.vertices_of(v, f))
    b = pkg.load().builder()
    tex = b.surface(b.constant((0.5, 0.5, 0.5)))
    b.mesh(v, f, b.lambertian(tex), normals=nn, uvs=uv)
    # a file without vn gives None for the normals; one without vt for the UVs; the plain fixture for both
    no_vn = tmp_path / "no_vn.obj"
    no_vn.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nf 1/1 2/2 3/3\n")
    v2, f2, n2, uv2 = T.load_obj_attr(str(no_vn))
    assert n2 is None and uv2.tolist() == [[0, 0], [1, 0], [0, 1]] and f2.tolist() == [[0, 1, 2]]
    no_vt = tmp_path / "no_vt.obj"
    no_vt.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 3//1\nf 1 2 3\n")
    v3, f3, n3, uv3 = T.load_obj_attr(str(no_vt))
    assert uv3 is None and n3 is None and len(v3) == 6 and f3.tolist() == [[0, 1, 2], [3, 4, 5]]   # (one face names no vn: None for all)
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/2 3/1\n")
    with pytest.raises(ValueError):
        T.load_obj_attr(str(bad))


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
  if (argc != 6) return 2;
  const std::vector<float> tri = slurp<float>(argv[1]), attr = slurp<float>(argv[2]), rays = slurp<float>(argv[3]), want = slurp<float>(argv[4]);
  const float t_min = (float)std::atof(argv[5]);
  const size_t n = tri.size() / 9;
  if (tri.size() % 9 || attr.size() != 15 * n || rays.size() != 8 * n || want.size() != 10 * n) { std::printf("bad sizes\n"); return 2; }
  long hits = 0, diffs = 0;
  for (size_t i = 0; i < n; i++) {
    const float *v = &tri[9 * i], *a = &attr[15 * i], *r = &rays[8 * i];
    rtg::Tri3 e1, e2, nn;
    const rtg::Tri3 v0{v[0], v[1], v[2]}, o{r[0], r[1], r[2]}, d{r[3], r[4], r[5]};
    (void)rtg::tri_record(v0, rtg::Tri3{v[3], v[4], v[5]}, rtg::Tri3{v[6], v[7], v[8]}, e1, e2, nn);
    float out[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, t = 0.f, bu = 0.f, bv = 0.f, ru = 0.f, rv = 0.f;
    if (rtg::tri_hit_uv(v0, e1, e2, o, d, t_min, r[7], t, bu, bv)) {
      rtg::tri_uv(v0, e1, e2, o, d, ru, rv);
      if (bits(ru) != bits(bu) || bits(rv) != bits(bv)) { diffs++; std::printf("DIFF pair %zu: tri_uv and tri_hit_uv disagree\n", i); }
      const rtg::TriAttr at{rtg::Tri3{a[0], a[1], a[2]}, rtg::Tri3{a[3], a[4], a[5]}, rtg::Tri3{a[6], a[7], a[8]}, a[9], a[10], a[11], a[12], a[13], a[14]};
      const rtg::Tri3 sn = rtg::tri_shade(bu, bv, at, nn, true, true, out[8], out[9]);
      out[0] = 1.f, out[1] = t, out[2] = o.x + t * d.x, out[3] = o.y + t * d.y, out[4] = o.z + t * d.z, out[5] = sn.x, out[6] = sn.y, out[7] = sn.z;
      hits++;
    }
    bool same = true;
    for (int k = 0; k < 10; k++) same = same && (bits(out[k]) == bits(want[10 * i + k]) || (out[k] != out[k] && want[10 * i + k] != want[10 * i + k]));
    if (!same && diffs++ < 5) std::printf("DIFF pair %zu: got %a %a %a, want %a %a %a\n", i, out[5], out[8], out[9], want[10 * i + 5], want[10 * i + 8], want[10 * i + 9]);
  }
  std::printf("pairs %zu hits %ld diffs %ld\n", n, hits, diffs);
  return 0;
}
"""


def test_rt_triangle_h_stands_alone_plain_and_sanitized(pkg, tmp_path):
    """A g++ program of its own includes csrc/rt_triangle.h and answers the attribute edge cases with the definition's bits -- at
    -O2, and with the address and undefined-behaviour sanitizers linked into that program (none is loaded into Python)."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the stand-alone triangle program")
    tri9, attr, rays8, _, _ = _edge_attr_pairs()
    want, ok = _definition_out10(pkg.triangle, tri9, attr, 3, rays8, MC.T_MIN)
    src = tmp_path / "surface_alone.cpp"
    src.write_text(PROGRAM)
    paths = {}
    for key, arr in (("tri", tri9), ("attr", attr), ("rays", rays8), ("want", want)):
        paths[key] = tmp_path / (key + ".bin")
        np.ascontiguousarray(arr, f32).tofile(str(paths[key]))
    for name, extra in (("plain", ["-O2"]),
                        ("san", ["-O1", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined"])):
        exe = tmp_path / ("surface_alone_" + name)
        subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math"] + extra
                              + ["-I", CSRC, str(src), "-o", str(exe)])
        r = subprocess.run([str(exe), str(paths["tri"]), str(paths["attr"]), str(paths["rays"]), str(paths["want"]), repr(MC.T_MIN)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        last = r.stdout.splitlines()[-1].split()
        got = dict(zip(last[0::2], map(int, last[1::2])))
        print(name, got)
        assert got == {"pairs": len(tri9), "hits": int(ok.sum()), "diffs": 0}, r.stdout[-2000:]
