"""Attributes, worlds and references shared by test_surface_abi.py (CPU) and test_surface_gpu.py (GPU): per-vertex normals and UVs
(include/rtiow_gpu_surface.h) on the triangles, rays and graphs of mesh_cases.py.

AttrBuilder        a Builder that gives every triangle() and mesh() call of a graph function deterministic attributes -- normals:
                   the area-weighted vertex normals plus a perturbation of a fifth of their length, un-normalised (length 0.6 ..
                   1.5); UVs: a smooth function of the vertex -- and remembers them per triangle
attach(groups, ab) the groups of a mesh_cases graph with "normals" [m, 3, 3] and "uvs" [m, 3, 2] beside "tri"
shade64            the definition's formulas in float64 from the same float32 inputs, on the triangle the float64 reference
                   (triangle_ref.closest_hit64) found: Moeller-Trumbore's u, v, the interpolation, the normalisation, the
                   wrappers' way out (physics_ref._to_world)
closest32_attr     triangle_ref.closest32 with triangle.shade: the float32 side on the CPU, as rtg_debug_hit_surface answers
compare_attr       worst deviations of the normal (absolute) and of (tu, tv) (absolute) among the rays triangle_ref.MARGIN keeps

Measured here on the CPU, closest32_attr against shade64, the four graphs of mesh_cases.GRAPHS with AttrBuilder's attributes,
4096 aimed rays each (test_surface_abi.py prints them; MARGIN and CAP_RAYS are triangle_ref's, as they stand):
    left out 0.10 % .. 2.05 % of a graph's rays (the very rays test_mesh_abi.py leaves out: the margin is the geometry's);
    worst deviations        normal (absolute)   (tu, tv) (absolute)
      ico                   1.03e-04            3.69e-05
      box                   1.26e-06            2.08e-07
      wrapped               5.16e-05            1.36e-05
      deep                  3.88e-04            3.89e-05
    (u, v carry the error of t, which grows with 1 / margin on grazing rays: the icosphere's silhouette; below the seven
    wrappers of "deep" the ray itself has gathered rounding before the triangle sees it, and three non-uniform Scales divide
    the normal without renormalising, so that its components are not bounded by 1 there.)
WORST_N, WORST_UV are the worst of each column and TOL_N, TOL_UV 4 x that, the project's rule (triangle_ref.py).
The closed-form anchor -- on icosphere_attr the interpolated, normalised normal is (p - centre) / |p - centre| -- measured the same
way, float32 shade against that float64 expression at the float64 reference's p (3108 rays, 2.12 % left out): worst 1.83e-04
-- the point's own deviation on grazing rays (triangle_ref: 1.3e-04 relative) turned into a direction; ANCHOR_TOL is 4 x that."""
import numpy as np

import mesh_cases as MC
import physics_ref as PR
import triangle_ref as TR

F = np.float64
f32 = np.float32
WORST_N, WORST_UV = 3.88e-4, 3.89e-5
TOL_N, TOL_UV = 4 * WORST_N, 4 * WORST_UV
WORST_ANCHOR = 1.83e-4
ANCHOR_TOL = 4 * WORST_ANCHOR


def vertex_attributes(T, v, f):
    """(normals [n, 3], uvs [n, 2]) float32 for an indexed mesh: see AttrBuilder."""
    v64 = np.asarray(v, F)
    n = T.vertex_normals(v, f).astype(F)
    bump = 0.2 * np.stack([np.sin(3.0 * v64[:, 1] + 1.0), np.cos(2.0 * v64[:, 2]), np.sin(5.0 * v64[:, 0])], axis=1)
    scale = 1.0 + 0.4 * np.sin(7.0 * v64[:, 0] + 2.0 * v64[:, 1])[:, None]
    uv = np.stack([0.5 + 0.25 * v64[:, 0] - 0.125 * v64[:, 2], 0.5 + 0.3 * v64[:, 1] + 0.1 * np.sin(v64[:, 0])], axis=1)
    return ((n + bump) * scale).astype(f32), uv.astype(f32)


class AttrBuilder:
    """Every other call goes to the Builder as it is."""

    def __init__(self, pkg, builder):
        self._pkg, self._b, self.made = pkg, builder, []

    def __getattr__(self, name):
        return getattr(self._b, name)

    def mesh(self, vertices, indices, material, sah=False):
        T = self._pkg.triangle
        n, uv = vertex_attributes(T, vertices, indices)
        ix = np.asarray(indices, np.int64)
        self.made.append((T.vertices_of(vertices, indices), n[ix], uv[ix]))
        return self._b.mesh(vertices, indices, material, sah=sah, normals=n, uvs=uv)

    def triangle(self, v0, v1, v2, material):
        T = self._pkg.triangle
        v = np.asarray([v0, v1, v2], f32)
        n, uv = vertex_attributes(T, v, np.array([[0, 1, 2]], np.uint32))
        self.made.append((v[None], n[None], uv[None]))
        return self._b.triangle_attr(v0, v1, v2, material, normals=n, uvs=uv)


def attach(groups, ab):
    out = []
    for g in groups:
        tri = np.asarray(g["tri"], f32)
        found = [m for m in ab.made if m[0].shape == tri.shape and np.array_equal(m[0], tri)]
        assert found, "a group without a recorded mesh"
        out.append(dict(g, normals=found[0][1], uvs=found[0][2]))
    return out


def graph(pkg, b, name):
    """(world, groups with attributes) of mesh_cases.GRAPHS[name], built through an AttrBuilder."""
    ab = AttrBuilder(pkg, b)
    world, groups = MC.GRAPHS[name](pkg, ab)
    return world, attach(groups, ab)


def _locate(groups, number):
    """group index and triangle index inside it of the running triangle numbers triangle_ref uses"""
    sizes = np.array([len(g["tri"]) for g in groups])
    ends = np.cumsum(sizes)
    gi = np.searchsorted(ends, number, side="right")
    return gi, number - (ends[gi] - sizes[gi])


def shade64(groups, ref, rays7):
    """(n [k, 3], tu [k], tv [k]) float64 for the rays ref["hit"] names, in their order; NaN rows elsewhere."""
    rays = np.asarray(rays7, F)
    n_out, tu, tv = np.full((len(rays), 3), np.nan), np.full(len(rays), np.nan), np.full(len(rays), np.nan)
    hit = np.asarray(ref["hit"], bool)
    number = np.asarray(ref["triangle"], np.int64)
    gi_all, ti_all = _locate(groups, np.maximum(number, 0))
    with np.errstate(all="ignore"):
        for gi, g in enumerate(groups):
            at = hit & (gi_all == gi)
            if not at.any():
                continue
            ti = ti_all[at]
            tri, nn, uv = np.asarray(g["tri"], F)[ti], np.asarray(g["normals"], F)[ti], np.asarray(g["uvs"], F)[ti]
            o, d = PR._to_local(g["chain"], rays[at, 0:3], rays[at, 3:6], rays[at, 6])
            e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
            pv = np.cross(d, e2)
            inv = 1.0 / PR._dot(e1, pv)
            tvec = o - tri[:, 0]
            u = PR._dot(tvec, pv) * inv
            v = PR._dot(d, np.cross(tvec, e1)) * inv
            w = (1.0 - u) - v
            s = w[:, None] * nn[:, 0] + u[:, None] * nn[:, 1] + v[:, None] * nn[:, 2]
            n = s / np.sqrt(PR._dot(s, s))[:, None] * float(g["sign"])
            _, n = PR._to_world(g["chain"], np.zeros_like(n), n)
            n_out[at] = n
            tu[at] = w * uv[:, 0, 0] + u * uv[:, 1, 0] + v * uv[:, 2, 0]
            tv[at] = w * uv[:, 0, 1] + u * uv[:, 1, 1] + v * uv[:, 2, 1]
    return n_out, tu, tv


def closest32_attr(T, groups, rays7, t_near=TR.T_NEAR):
    """(out [n, 10] float32, material [n], triangle [n]): triangle_ref.closest32 with the shading normal and (tu, tv)."""
    rays7 = np.asarray(rays7, f32)
    n = len(rays7)
    best = np.full(n, np.finfo(f32).max, f32)
    out, mat, index = np.zeros((n, 10), f32), np.full(n, 0xFFFFFFFF, np.uint32), np.full(n, -1, np.int64)
    number = 0
    with np.errstate(all="ignore"):
        for g in groups:
            o, d, time = rays7[:, 0:3], rays7[:, 3:6], rays7[:, 6]
            for k, a in g["chain"]:
                a32 = np.asarray(a, f32)
                if k == "translate":
                    o = o - a32
                elif k == "scale":
                    o, d = o / a32, d / a32
                elif k == "rotate":
                    s, c = TR._sin_cos32(a)
                    o, d = TR._rot32(o, -s, c), TR._rot32(d, -s, c)
                else:
                    o = o - time[:, None] * a32
            for ti, tri in enumerate(np.asarray(g["tri"], f32)):
                rec = T.record(tri[0], tri[1], tri[2])
                ok, t, p, _ = T.hit(rec, o, d, f32(t_near), best)
                nn, tu, tv = T.shade(rec, g["normals"][ti], g["uvs"][ti], o, d, flip=g["sign"] < 0)
                nn = np.array(nn)
                for k, a in reversed(g["chain"]):
                    a32 = np.asarray(a, f32)
                    if k == "translate":
                        p = p + a32
                    elif k == "scale":
                        p, nn = p * a32, nn / a32
                    elif k == "rotate":
                        s, c = TR._sin_cos32(a)
                        p, nn = TR._rot32(p, s, c), TR._rot32(nn, s, c)
                out[ok, 0], out[ok, 1], out[ok, 2:5], out[ok, 5:8], out[ok, 8], out[ok, 9] = 1.0, t[ok], p[ok], nn[ok], tu[ok], tv[ok]
                mat[ok], index[ok] = g["mat"], number
                best = np.where(ok, t, best)
                number += 1
    return out, mat, index


def compare_attr(groups, ref, rays7, out10):
    """dict: left_out, compared, dn, duv among the rays with margin > triangle_ref.MARGIN that both sides hit."""
    n64, tu, tv = shade64(groups, ref, rays7)
    use = ref["margin"] > TR.MARGIN
    both = use & (out10[:, 0] != 0) & ref["hit"]
    o = out10.astype(F)
    return {"left_out": 1.0 - use.mean(), "compared": int(both.sum()),
            "dn": float(np.abs(o[both, 5:8] - n64[both]).max()) if both.any() else 0.0,
            "duv": float(max(np.abs(o[both, 8] - tu[both]).max(), np.abs(o[both, 9] - tv[both]).max())) if both.any() else 0.0}


def assert_attr(res, what):
    print("%-10s left out %5.2f %%  compared %5d  dn %.2e  duv %.2e" % (what, 100 * res["left_out"], res["compared"], res["dn"], res["duv"]))
    assert res["left_out"] <= TR.CAP_RAYS, (what, res)
    assert res["compared"] > 500, (what, res)
    assert res["dn"] <= TOL_N and res["duv"] <= TOL_UV, (what, res)


def list_attributes(T, tris):
    """Per triangle of mesh_cases.list_triangles: (normals or None, uvs or None) -- both, normals only, UVs only, plain, in turn."""
    out = []
    for i, tri in enumerate(np.asarray(tris, f32)):
        n, uv = vertex_attributes(T, tri, np.array([[0, 1, 2]], np.uint32))
        out.append((n if i % 4 in (0, 1) else None, uv if i % 4 in (0, 2) else None))
    return out
