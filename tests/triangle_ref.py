"""An independent float64 closest hit over triangles under wrapper chains, for test_mesh_abi.py (the numpy definition,
rtiow-rust_amd/triangle.py, on the CPU) and test_mesh_gpu.py (the HIP kernels).  The chain conventions are physics_ref's, by
import: Translate / Scale / RotateY / LinearMove above a group of triangles, the parity of its FlipNormals, Scale dividing the
normal without renormalising, LinearMove leaving p where the inner object put it.

A graph is a list of GROUPS (mesh_cases.py makes them beside the builder calls): {"tri": [m, 3, 3] float32 vertices, "chain":
((kind, parameter), ...) outermost first, "sign": +1 / -1, "mat": material id}.

closest_hit64   physics_ref.closest_hit over the groups' triangles (its triangle branch is the statement; this module keeps the
                name and the description): geometry in float64: per triangle the plane crossing t = n.(v0 - o) / n.d with n = e1 x e2 and the barycentric
                coordinates by Cramer's rule on the Gram matrix of (e1, e2) -- not Moeller-Trumbore's cross products; the
                unit normal is n / |n| in float64.
                Per ray the conditioning margin is the smallest of: the barycentric distances |u|, |v|, |1 - u - v|;
                |det| / (|e1| |e2| |d|) (det = -n.d); the crossing's distance from t_near, |t - t_near| |d| / max(1, |o|); -- each
                over the triangles whose crossing is not beyond the accepted hit (a crossing behind the origin counts with its
                distance from t_near alone) -- and the relative gap (t2 - t1) / t1 to the second-best t.
closest32       the float32 side on the CPU: the chains in float32 numpy (one rounding per operation, as the kernels' PUSH / POP
                arms do them; sin and cos of RotateY from numpy's float32, which may differ from the builder's sinf / cosf by an
                ulp -- nothing the tolerances notice) around triangle.hit, folded in list order.

Measured here on the CPU, closest32 against closest_hit64, mesh_cases.GRAPHS, 4096 aimed rays each (test_mesh_abi.py prints them;
MARGIN = 1e-4, the cap on the share left out is physics_ref.CAP_RAYS = 5 %):
    left out 0.10 % (box) .. 2.05 % (ico, 320 triangles) of a graph's rays; no hit-flag, triangle or material mismatch among
    the rest; at least 70 % of the compared rays hit and at least 22 % miss;
    worst deviations        t (relative)   p (relative to max(1, |p|))   normal (absolute)
      ico                   8.3e-05        1.3e-04                       8.8e-08
      box                   1.8e-07        4.8e-07                       0
      wrapped               6.0e-06        2.1e-05                       1.2e-07
      deep                  2.1e-05        4.3e-05                       2.5e-07
    (t and p are worst on the icosphere, whose silhouette rays cross a triangle at a grazing angle: the error grows with
    1 / margin; the normal is worst below the seven wrappers of "deep", three of them non-uniform Scales.)
TOL_T, TOL_P, TOL_N are 4 x the worst figure of each column, the project's rule: 3.3e-04, 5.2e-04, 1.0e-06."""
import numpy as np

import physics_ref as PR
from physics_ref import CAP_RAYS, MARGIN, _dot, _to_local, _to_world, point_to_world  # noqa: F401

F = np.float64
f32 = np.float32
T_NEAR = 0.001
WORST_T, WORST_P, WORST_N = 8.3e-5, 1.3e-4, 2.5e-7      # measured: see the docstring
TOL_T, TOL_P, TOL_N = 4 * WORST_T, 4 * WORST_P, 4 * WORST_N
MIN_HIT_SHARE, MIN_MISS_SHARE = 0.25, 0.10


def prims_of(groups):
    """The groups as physics_ref primitives: one Prim("tri", ...) per triangle, in order."""
    return [PR.Prim("tri", (tri[0], tri[1], tri[2]), g["mat"], tuple(g["chain"]), g["sign"]) for g in groups for tri in np.asarray(g["tri"], F)]


def closest_hit64(groups, o, d, time, t_near=T_NEAR):
    """dict of hit, t, p, n, material, triangle (a running number over the groups in order, -1 on a miss) and margin:
    physics_ref.closest_hit over the groups' triangles -- the one statement of the triangle."""
    ref = PR.closest_hit(prims_of(groups), o, d, time, t_near=t_near)
    ref["triangle"] = ref["prim"]
    return ref


# ---- the float32 side on the CPU ----------------------------------------------------------------------------------------------
def _rot32(v, s, c):   # rt_trace.h rot_y: (v.(c, 0, s), v.(0, 1, 0), v.(-s, 0, c)), dot = (x*x' + y*y') + z*z'
    z, one = f32(0.0), f32(1.0)
    return np.stack([(v[:, 0] * c + v[:, 1] * z) + v[:, 2] * s, (v[:, 0] * z + v[:, 1] * one) + v[:, 2] * z,
                     (v[:, 0] * (-s) + v[:, 1] * z) + v[:, 2] * c], axis=1)


def _sin_cos32(deg):
    rad = f32(deg) * f32(3.14159265358979323846) / f32(180.0)
    return np.sin(rad, dtype=f32), np.cos(rad, dtype=f32)


def closest32(T, groups, rays7, t_near=T_NEAR):
    """The definition under float32 chains, folded over the groups' triangles in order: (out [n, 8] float32, material [n]
    uint32 -- 0xffffffff on a miss --, triangle [n] int64), as rtg_debug_hit_top answers a list world of the groups."""
    rays7 = np.asarray(rays7, f32)
    n = len(rays7)
    best = np.full(n, np.finfo(f32).max, f32)
    out, mat, index = np.zeros((n, 8), f32), np.full(n, 0xFFFFFFFF, np.uint32), np.full(n, -1, np.int64)
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
                    s, c = _sin_cos32(a)
                    o, d = _rot32(o, -s, c), _rot32(d, -s, c)
                else:
                    o = o - time[:, None] * a32
            for tri in np.asarray(g["tri"], f32):
                ok, t, p, nn = T.hit(T.record(tri[0], tri[1], tri[2]), o, d, f32(t_near), best, flip=g["sign"] < 0)
                nn = np.array(nn)
                for k, a in reversed(g["chain"]):
                    a32 = np.asarray(a, f32)
                    if k == "translate":
                        p = p + a32
                    elif k == "scale":
                        p, nn = p * a32, nn / a32
                    elif k == "rotate":
                        s, c = _sin_cos32(a)
                        p, nn = _rot32(p, s, c), _rot32(nn, s, c)
                out[ok, 0], out[ok, 1], out[ok, 2:5], out[ok, 5:8] = 1.0, t[ok], p[ok], nn[ok]
                mat[ok], index[ok] = g["mat"], number
                best = np.where(ok, t, best)
                number += 1
    return out, mat, index


def compare(ref, out, mat, index=None):
    """physics_ref.compare_hits, plus the triangle mismatches when the float32 side names its triangle."""
    res = PR.compare_hits(ref, out, mat)
    use = ref["margin"] > MARGIN
    both = use & (out[:, 0] != 0) & ref["hit"]
    res["triangle_mismatch"] = int((both & (index != ref["triangle"])).sum()) if index is not None else 0
    res["misses"] = int((use & ~ref["hit"]).sum())
    return res


def assert_hits(res, what):
    print("%-10s left out %5.2f %%  compared %5d (%5d hits, %5d misses)  dt %.2e  dp %.2e  dn %.2e" % (
        what, 100 * res["left_out"], res["compared"], res["hits"], res["misses"], res["dt"], res["dp"], res["dn"]))
    assert res["left_out"] <= CAP_RAYS, (what, res)
    assert res["hits"] >= MIN_HIT_SHARE * res["compared"] and res["misses"] >= MIN_MISS_SHARE * res["compared"], (what, res)
    assert res["flag_mismatch"] == 0 and res["material_mismatch"] == 0 and res["triangle_mismatch"] == 0, (what, res)
    assert res["dt"] <= TOL_T and res["dp"] <= TOL_P and res["dn"] <= TOL_N, (what, res)
