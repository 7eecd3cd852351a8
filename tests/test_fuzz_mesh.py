"""Random worlds with triangles, meshes and image textures, on the CPU: the generator reaches every place and setting it is meant
to, the worlds flatten to well-formed programs, the float64 image sampler (image_ref.py) agrees with the numpy definition and
the host probe and its planted faults are noticed, and the float64 closest hit (physics_ref.py, now with triangles) holds its
tolerances at these worlds' scale against float32 sides that are not the kernels."""
import numpy as np
import pytest

import fuzz_mesh_cases as C
import fuzz_scenes as FS
import image_cases as IC
import image_ref as IR
import physics_ref as PR
import triangle_ref as TR
from test_fuzz import _deep_wrappers

f32 = np.float32
F = np.float64
OP_BOX, OP_PUSH, OP_POP, OP_MEDIUM, OP_SAVE, OP_MERGE, OP_EXT, OP_TRI = 1, 4, 5, 6, 10, 11, 12, 14   # flat_scene.h
ALL_SEEDS = C.SCHEDULED + C.DEEP + C.FREE + C.FREE_DEEP


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def test_the_seed_sets_reach_every_place_and_image_setting(pkg):
    """From the Recorder's description of every world of the seed sets: each place of fuzz_scenes.PLACES holds a triangle in some
    world, every image setting of IMAGE_SETTINGS occurs, every world holds a triangle (else the GPU tests prove nothing).  The
    media-free worlds alone reach an image on a triangle and every wrapper."""
    be = pkg.load()
    seen, settings, free_seen = set(), set(), set()
    for seed in ALL_SEEDS:
        rec, world, _, _ = C.build(pkg, be, seed, 24, 16, record=True)
        here = FS.places(rec, world)
        assert any(r[0] in ("tri", "mesh") for r in rec.objects.values()) and here, seed
        seen |= here
        settings |= FS.image_settings(rec)
        if seed in C.FREE + C.FREE_DEEP:
            free_seen |= here
    print("places:", sorted(seen))
    print("image settings:", sorted(settings))
    assert seen == set(FS.PLACES), set(FS.PLACES) - seen
    assert settings == set(FS.IMAGE_SETTINGS), set(FS.IMAGE_SETTINGS) - settings
    assert {"under Translate", "under RotateY", "under Scale (non-uniform)", "under LinearMove", "one side of And", "below 5-7 wrappers"} <= free_seen
    assert len(set(ALL_SEEDS)) == 32 + 12 + 12


def test_some_worlds_are_marked_as_holding_a_list_level_rect_light(pkg):
    be = pkg.load()
    marked = [seed for seed in C.SCHEDULED if C.build(pkg, be, seed, 24, 16)[3]["rect_light"]]
    print("list-level rect lights:", marked)
    assert len(marked) >= 4


# ---- flattening ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_mesh_worlds_flatten_on_host(pkg, seed):
    b, world, _, _ = C.build(pkg, pkg.load(), seed, 24, 16)
    words, feat = b.flatten(world)
    ops = words[:, 7] & 0xff
    assert ops[-1] == 0 and (ops[:-1] != 0).all()
    box = ops == OP_BOX
    assert (words[box, 6] > np.nonzero(box)[0]).all() and (words[box, 6] < len(words)).all()
    assert int((ops == OP_PUSH).sum()) == int((ops == OP_POP).sum())
    tri = np.nonzero(ops == OP_TRI)[0]
    assert len(tri) > 0 and (ops[tri + 1] == OP_EXT).all() and (ops[tri + 2] != OP_EXT).all()   # exactly one data record each
    assert feat & C.FEAT_TRI and len(b.flatten_pool2(world)[0]) == 0
    for m in np.nonzero(ops == OP_MEDIUM)[0]:                        # (test_fuzz_graph_boundaries_flatten_on_host's invariants)
        end = int(words[m, 4])
        assert m + 1 < end <= len(words) - 1
        inner = ops[m + 1:end]
        assert not (inner == 0).any() and int((inner == OP_PUSH).sum()) == int((inner == OP_POP).sum())
        general = bool(words[m, 7] & (1 << 14))
        assert (general or end == m + 2 or (end == m + 3 and ops[m + 1] == OP_TRI)) and ((not general) or (feat & 16))
    assert int((ops == OP_SAVE).sum()) == int((ops == OP_MERGE).sum())
    med = np.nonzero(ops == OP_MEDIUM)[0]
    nested = any((ops[m + 1:int(words[m, 4])] == OP_MEDIUM).any() for m in med)
    needs_deep = bool((ops == OP_SAVE).any() or nested or _deep_wrappers(words))
    assert bool(feat & C.FEAT_DEEP) == needs_deep, (seed, hex(feat))
    if seed in C.SCHEDULED + C.FREE:
        assert not feat & C.FEAT_DEEP                                   # the scheduled kernels take it
    if seed in C.DEEP + C.FREE_DEEP:
        assert feat & C.FEAT_DEEP                                       # the general walk alone


# ---- the image sampler -----------------------------------------------------------------------------------------------------------
SAMPLER_SIZES = IC.SIZES + [(8, 8)]


def sampler_points(size, k):
    """4096 random points in +-4, per image size and setting"""
    return ((np.random.RandomState(1000 * size[0] + size[1] + k).rand(4096, 3) - 0.5) * 8).astype(f32)


def check_sampler(size, prm, got, p, fault=None):
    """float32 values `got` at the points p against image_ref.sample64: (share left out, worst deviation); asserts the cap,
    exactness outside the margin (nearest) and the size's tolerance (bilinear)."""
    ref, margin = IR.sample64(IC.image(size), prm, p.astype(F), fault=fault)
    use = margin > IR.NEAREST_MARGIN
    dev = float(np.abs(got.astype(F) - ref)[use].max())
    left = 1.0 - use.mean()
    assert left <= PR.CAP_RAYS, (size, IC.name(prm), left)
    assert dev <= (0.0 if prm["filter"] == IR.NEAREST else IR.BILINEAR_TOL[size]), (size, IC.name(prm), fault, dev)
    return left, dev


@pytest.mark.parametrize("size", SAMPLER_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_float64_sampler_against_the_definition_and_the_host_probe(pkg, size):
    I = pkg.image
    b = pkg.load().builder()
    img = IC.image(size)
    worst, left = 0.0, 0.0
    for k, prm in enumerate(IC.settings(I, size)):
        p = sampler_points(size, k)
        got = I.sample(img, prm, p)
        l, d = check_sampler(size, prm, got, p)
        check_sampler(size, prm, b.texture_host(b.image(img, prm), p), p)
        left, worst = max(left, l), max(worst, d if prm["filter"] == IR.BILINEAR else 0.0)
    print("%dx%d: nearest exact outside the margin, at most %.3f %% left out; bilinear worst %.2e (recorded %.2e)" % (
        size + (100 * left, worst, IR.BILINEAR_WORST[size])))


def test_the_image_checks_notice_planted_faults(pkg):
    """Each wrong convention of image_ref makes the sampler check fail against the (unchanged) definition, at every size with
    more than one texel; physics_ref's rotate_neg and scale_normal make the first-hit check of the mesh worlds fail against the
    float32 triangle definition."""
    I = pkg.image
    for size in SAMPLER_SIZES[1:]:
        img = IC.image(size)
        for fault in IR.FAULTS:
            noticed = 0
            for k, prm in enumerate(IC.settings(I, size)):
                p = sampler_points(size, k)
                try:
                    check_sampler(size, prm, I.sample(img, prm, p), p, fault=fault)
                except AssertionError:
                    noticed += 1
            assert noticed >= 4, (size, fault, noticed)
    be = pkg.load()
    for fault, seeds in (("rotate_neg", C.FREE + C.FREE_DEEP), ("scale_normal", C.FREE + C.FREE_DEEP)):
        noticed = 0
        for seed in seeds:
            try:
                _triangles_against_float64(pkg, be, seed, fault=fault)
            except AssertionError:
                noticed += 1
        assert noticed >= 4, (fault, noticed)


# ---- the mixed closest hit at the fuzz worlds' scale ----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", C.ANALYTIC)
def test_analytic_fuzz_worlds_on_the_oracle_against_float64(pkg, oracle, seed):
    """spheres, rects and prisms under the generator's wrappers, at its scale: the oracle's debug_hit_top against closest_hit"""
    rec, world, prims, rays, ref = C.hit_reference(pkg, oracle, seed)
    assert not any(pr.kind == "tri" for pr in prims)
    out, mat = rec.scene(world).debug_hit_top(rays, seed=7, t_near=PR.T_NEAR)
    C.assert_by_kind(C.compare_by_kind(prims, ref, out, mat), "analytic %d" % seed)


def _triangles_against_float64(pkg, be, seed, fault=None):
    """The rays of the world's own set (the GPU test's) whose float64 winner is a triangle: the float32 definition over the
    world's triangles must hit that triangle, within the triangle tolerances."""
    rec, world, prims, rays, ref = C.hit_reference(pkg, be, seed, fault=fault)
    number = np.array([i for i, pr in enumerate(prims) if pr.kind == "tri"])
    groups = [{"tri": np.array([prims[i].params], f32), "chain": prims[i].chain, "sign": prims[i].sign, "mat": prims[i].material} for i in number]
    sel = ref["hit"] & np.isin(ref["prim"], number)
    out, mat, index = TR.closest32(pkg.triangle, groups, rays[sel], PR.T_NEAR)
    res = C.compare_by_kind(prims, {k: v[sel] for k, v in ref.items()}, out, mat, np.where(index >= 0, number[np.maximum(index, 0)], -1))
    C.assert_by_kind(res, "triangles %d" % seed, shares=False)
    return res


@pytest.mark.parametrize("seed", C.FREE + C.FREE_DEEP)
def test_the_mesh_worlds_triangles_against_float64(pkg, seed):
    """the triangles of a media-free mesh world under their chains: triangle_ref.closest32 (float32 numpy) against the world's
    closest_hit, on the rays that the GPU test sends"""
    res = _triangles_against_float64(pkg, pkg.load(), seed)
    assert res["n_tri"] > 0 and res["n_analytic"] == 0


@pytest.mark.parametrize("seed", C.FREE + C.FREE_DEEP)
def test_the_mesh_worlds_ray_sets_are_usable(pkg, seed):
    """what the GPU test compares: the whole world's rays leave out at most the cap, enough hit and enough miss, and both hit
    kinds occur -- from the float64 side alone"""
    _, _, prims, rays, ref = C.hit_reference(pkg, pkg.load(), seed)
    use = ref["margin"] > PR.MARGIN
    hits, n = int((use & ref["hit"]).sum()), int(use.sum())
    is_tri = np.array([pr.kind == "tri" for pr in prims] + [False])[ref["prim"]]
    print("%d: %d primitives, left out %.2f %%, %d hits (%d on triangles), %d misses" % (
        seed, len(prims), 100 * (1 - use.mean()), hits, int((use & ref["hit"] & is_tri).sum()), n - hits))
    assert 1 - use.mean() <= PR.CAP_RAYS and hits >= C.MIN_HIT_SHARE * n and n - hits >= C.MIN_MISS_SHARE * n
    assert (use & ref["hit"] & is_tri).sum() >= 20 and (use & ref["hit"] & ~is_tri).sum() >= 20
