"""The random worlds with meshes and image textures that test_fuzz_mesh.py (CPU) and test_fuzz_mesh_gpu.py (GPU) share: the seed
sets, the builds, and the first-hit comparison per hit kind.

SCHEDULED   32 worlds (meshes, images, general_boundaries): programs the scheduled kernels take
DEEP        12 worlds (+ deep_shapes) whose programs carry FEAT_DEEP: the general walk
FREE        12 worlds without media, Perlin textures and the enclosing emitter (rays can miss them; every texture has a closed
            form), the last 4 with deep_shapes: the float64 references
The seeds of SCHEDULED are the first 32 from 20000 whose program does not carry FEAT_DEEP (20015 does: a ConstantMedium in a Bvh
below And below the world's Bvh, which the generator's rule does not see), those of DEEP the first twelve from 21000 whose program does, those of FREE the first from 22000 / 23000
whose aimed rays meet the shares below against the float64 reference alone (test_fuzz_mesh.py checks both); no seed was chosen
by what a kernel answers.

Measured on the CPU (test_fuzz_mesh.py prints them), 2048 rays per world (aimed_and_stray), MARGIN = 1e-4:
  analytic fuzz worlds (ANALYTIC: meshes=False, media=False, sky=False) on the oracle's debug_hit_top against closest_hit:
      left out 0.10 .. 0.54 % of a world's rays; no flag or material mismatch; 67 .. 83 % of the compared rays hit;
      worst t 1.5e-03 (relative)   p 7.3e-06 (relative to max(1, |p|))   normal 1.1e-04 (absolute)
      (t: origins up to 1500 units away from spheres of radius 20 .. 90 under Scale: b^2 - a c cancels)
  the triangles of the FREE and FREE_DEEP worlds through triangle_ref.closest32 against the world's closest_hit, on the rays of
  the world's own set (the GPU test's) whose float64 winner is a triangle (120 .. 1319 a world):
      left out 0.00 .. 1.23 % of them; no flag, material or triangle mismatch;
      worst t 5.3e-04   p 8.3e-06   normal 2.0e-07
      (t: world 22005, an origin 0.03 units in front of a triangle at coordinates of 150: the root margin is 1.9e-04)
  the FREE and FREE_DEEP worlds' whole ray sets (what the GPU test compares) leave out 0.15 .. 1.22 %; 71 .. 90 % of the
  compared rays hit and 10 .. 29 % miss; at least 120 compared hits are on triangles and at least 500 on spheres and rects.
Per hit kind the tolerance is the larger of the recorded one (physics_ref.TOL_* for spheres and rects, triangle_ref.TOL_* for
triangles) and 4 x the worst above: analytic 6.0e-03 (4 x 1.5e-03), 4.8e-04, 6.8e-04 (recorded); triangle 2.2e-03 (4 x 5.3e-04),
5.2e-04, 1.0e-06 (recorded)."""
import numpy as np

import physics_ref as PR
import triangle_ref as TR
from fuzz_scenes import random_camera, random_world

F = np.float64
f32 = np.float32
FEAT_DEEP, FEAT_TRI = 128, 1024
N_RAYS = 2048
SCHEDULED = tuple(s for s in range(20000, 20033) if s != 20015)
DEEP = (21000, 21001, 21002, 21003, 21005, 21006, 21007, 21008, 21009, 21010, 21011, 21013)
FREE = (22000, 22001, 22002, 22003, 22004, 22005, 22006, 22007)
FREE_DEEP = (23004, 23008, 23009, 23010)
ANALYTIC = tuple(range(24000, 24008))
FUZZ_WORST = {"analytic": (1.5e-3, 7.3e-6, 1.1e-4), "tri": (5.3e-4, 8.3e-6, 2.0e-7)}     # measured: see the docstring
RECORDED = {"analytic": (PR.TOL_T, PR.TOL_P, PR.TOL_N), "tri": (TR.TOL_T, TR.TOL_P, TR.TOL_N)}
TOL = {k: tuple(max(r, 4 * w) for r, w in zip(RECORDED[k], FUZZ_WORST[k])) for k in RECORDED}
MIN_HIT_SHARE, MIN_MISS_SHARE = 0.25, 0.10


def flags(seed):
    if seed in SCHEDULED:
        return dict(meshes=True, images=True, general_boundaries=True)
    if seed in DEEP:
        return dict(meshes=True, images=True, general_boundaries=True, deep_shapes=True)
    if seed in ANALYTIC:
        return dict(media=False, perlin=False, sky=False)
    return dict(meshes=True, images=True, general_boundaries=True, deep_shapes=seed in FREE_DEEP, media=False, perlin=False, sky=False)


def build(pkg, backend, seed, nx, ny, record=False, **override):
    """(builder or Recorder, world, camera, marks) of world `seed`."""
    rs = np.random.RandomState(seed)
    b = backend.builder()
    if record:
        b = PR.Recorder(b)
    marks = {}
    world = random_world(pkg, b, rs, marks=marks, **dict(flags(seed), **override))
    return b, world, random_camera(pkg, backend, rs, nx, ny), marks


def aimed_and_stray(prims, seed):
    """float32 [N_RAYS, 7]: physics_ref.aimed_rays (origins within 1500 units), 35 % of them turned to a direction drawn uniformly
    from the sphere (same origin, length and time): in worlds this crowded an aimed ray hardly ever misses everything."""
    rays = PR.aimed_rays(prims, N_RAYS, seed, origin_box=((-1500.0,) * 3, (1500.0,) * 3))
    rs = np.random.RandomState(seed + 1)
    stray = rs.uniform(size=N_RAYS) < 0.35
    v = rs.normal(size=(N_RAYS, 3))
    v *= (np.sqrt((rays[:, 3:6] ** 2).sum(axis=1)) / np.sqrt((v * v).sum(axis=1)))[:, None]
    rays[stray, 3:6] = v[stray]
    return rays.astype(f32)


_refs = {}


def hit_reference(pkg, backend, seed, fault=None):
    """(recorder, world, primitives, float32 rays [N_RAYS, 7], float64 hits) of a media-free world: the rays of aimed_and_stray;
    computed once per (seed, fault) and shared (callers must not write them)."""
    rec, world, _, _ = build(pkg, backend, seed, 24, 16, record=True)
    key = (seed, fault)
    if key not in _refs:
        prims = PR.primitives(rec, world)
        rays = aimed_and_stray(prims, seed)
        r64 = rays.astype(F)
        _refs[key] = (prims, rays, PR.closest_hit(prims, r64[:, 0:3], r64[:, 3:6], r64[:, 6], fault=fault))
    return (rec, world) + _refs[key]


def compare_by_kind(prims, ref, out, mat, index=None):
    """physics_ref.compare_hits, with the deviations split by the kind of the primitive the reference hit: res["analytic"] and
    res["tri"] are (dt, dp, dn); plus the misses among the compared rays and, when the float32 side names its primitive, the
    mismatches of that."""
    res = PR.compare_hits(ref, out, mat)
    use = ref["margin"] > PR.MARGIN
    both = use & (out[:, 0] != 0) & ref["hit"]
    res["misses"] = int((use & ~ref["hit"]).sum())
    res["prim_mismatch"] = int((both & (index != ref["prim"])).sum()) if index is not None else 0
    is_tri = np.array([pr.kind == "tri" for pr in prims] + [False])[ref["prim"]]
    o64 = out.astype(F)
    plen = np.maximum(1.0, np.sqrt((ref["p"] * ref["p"]).sum(axis=1)))
    for kind, at in (("analytic", both & ~is_tri), ("tri", both & is_tri)):
        res[kind] = (0.0, 0.0, 0.0)
        if at.any():
            res[kind] = (float((np.abs(o64[at, 1] - ref["t"][at]) / np.abs(ref["t"][at])).max()),
                         float((np.abs(o64[at, 2:5] - ref["p"][at]).max(axis=1) / plen[at]).max()),
                         float(np.abs(o64[at, 5:8] - ref["n"][at]).max()))
        res["n_" + kind] = int(at.sum())
    return res


def assert_by_kind(res, what, shares=True):
    print("%-12s left out %5.2f %%  compared %5d (%5d hits, %5d misses)  analytic (%4d) dt %.2e dp %.2e dn %.2e   tri (%4d) dt %.2e dp %.2e dn %.2e" % (
        (what, 100 * res["left_out"], res["compared"], res["hits"], res["misses"], res["n_analytic"]) + res["analytic"] + (res["n_tri"],) + res["tri"]))
    assert res["left_out"] <= PR.CAP_RAYS, (what, res)
    assert not shares or (res["hits"] >= MIN_HIT_SHARE * res["compared"] and res["misses"] >= MIN_MISS_SHARE * res["compared"]), (what, res)
    assert res["flag_mismatch"] == 0 and res["material_mismatch"] == 0 and res["prim_mismatch"] == 0, (what, res)
    for kind in ("analytic", "tri"):
        assert all(d <= t for d, t in zip(res[kind], TOL[kind])), (what, kind, res[kind], TOL[kind])
