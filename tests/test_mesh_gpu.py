"""Triangles and meshes on the GPU (include/rtiow_gpu_mesh.h): list worlds against the numpy definition bit for bit, meshes under
a Bvh against the same triangles as a list, wrapper chains against the float64 reference (triangle_ref.py, with the CPU test's
tolerances and cap), exact radiance, the feature planes, a closed mesh as a medium boundary, light sampling, and the rest of the
surface (two handles, ray frames, progressive frames, counts).

A scene that holds a triangle renders on the full-feature pool kernel or the lock-step kernel (their TRI instantiations) under
scene option `kernel` = 3 and on the one-lane kernel under `kernel` = 1: the tests that compare the two read from `verbose` which
kernel took the frame.  Frames are at most 48 x 32 x 8 and ray sets at most 4 096."""
import numpy as np
import pytest

import mesh_cases as MC
import physics_ref as PR
import triangle_ref as TR
from conftest import assert_bit_equal
from test_image_texture_gpu import COUNTERS, _fold, _render_named

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 0xDEADBEEF
FEAT_DEEP, FEAT_TRI = 128, 1024
L_EMIT = PR.L_EMIT


def _rays8(rays7, t_max):
    return np.concatenate([np.asarray(rays7, f32), np.broadcast_to(np.asarray(t_max, f32), (len(rays7),))[:, None]], axis=1).astype(f32)


# ---- 1. list worlds, bit-exact --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 7])
def test_a_list_world_equals_the_definition(pkg, gpu, k):
    T = pkg.triangle
    tris = MC.list_triangles(k)
    b = gpu.builder()
    mats = [b.lambertian(b.constant((0.1 * (i + 1), 0.5, 0.5))) for i in range(k)]
    flips = [i % 3 == 1 for i in range(k)]
    world = []
    for i in range(k):
        t = b.triangle(tris[i, 0], tris[i, 1], tris[i, 2], mats[i])
        world.append(b.flip_normals(t) if flips[i] else t)
    words, feat = b.flatten(world)
    assert feat & FEAT_TRI and not feat & FEAT_DEEP
    sc = b.scene(world)
    rays = MC.edge_rays(tris)
    want, index = T.closest(tris, rays, MC.T_MIN, flips=flips)
    want_mat = np.where(index >= 0, np.asarray(mats, np.uint32)[np.maximum(index, 0)], 0xFFFFFFFF).astype(np.uint32)
    out, mat = sc.debug_hit_top(rays, seed=7, t_near=MC.T_MIN)
    assert_bit_equal(out, want, "rtg_debug_hit_top against triangle.closest, %d triangles" % k)
    assert np.array_equal(mat, want_mat)
    hit = want[:, 0] != 0
    assert hit.sum() > len(rays) // 4 and (~hit).sum() > len(rays) // 10
    q_out, q_mat = sc.closest_hit(rays, seed=7, t_min=MC.T_MIN)
    assert_bit_equal(q_out, out, "rtg_query_closest against rtg_debug_hit_top")
    assert np.array_equal(q_mat, mat)
    # occlusion: t_max beyond everything, at the closest t (a miss of that triangle: the range is half open), in between, NaN, 0
    t_hit = np.where(hit, want[:, 1], f32(1.0))
    for t_max in (np.full(len(rays), np.finfo(f32).max, f32), t_hit, (t_hit * f32(1.5)).astype(f32), (t_hit * f32(0.5)).astype(f32),
                  np.full(len(rays), np.nan, f32), np.zeros(len(rays), f32)):
        r8 = _rays8(rays, t_max)
        assert np.array_equal(sc.occluded(r8, seed=7, t_min=MC.T_MIN), T.occluded(tris, r8, MC.T_MIN))
    assert T.occluded(tris, _rays8(rays, np.finfo(f32).max), MC.T_MIN).sum() == hit.sum()


# ---- 2. a mesh under a Bvh against the same triangles as a list ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def references(pkg, gpu):
    """Per graph of mesh_cases: the float32 rays and the float64 answer, computed once and left unchanged."""
    out = {}
    for name, fn in MC.GRAPHS.items():
        b = gpu.builder()
        _, groups = fn(pkg, b)
        rays = MC.aimed_rays(groups).astype(f32)
        r64 = rays.astype(np.float64)
        out[name] = (groups, rays, TR.closest_hit64(groups, r64[:, 0:3], r64[:, 3:6], r64[:, 6]))
    return out


@pytest.mark.parametrize("name", ["ico", "box"])
@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
def test_a_mesh_under_a_bvh_equals_its_triangles_as_a_list(pkg, gpu, references, name, sah):
    T = pkg.triangle
    groups, rays, ref = references[name]
    rays = rays[ref["margin"] > TR.MARGIN]                     # the rays the CPU test found well conditioned
    tris, mat_id = groups[0]["tri"], groups[0]["mat"]
    b = gpu.builder()
    world, _ = MC.GRAPHS[name](pkg, b, sah=sah)
    assert b.flatten(world)[1] & FEAT_TRI
    out, mat = b.scene(world).debug_hit_top(rays, seed=3, t_near=MC.T_MIN)
    lb = gpu.builder()
    MC._mats(lb)                                               # (the same material ids)
    lw = [lb.triangle(t[0], t[1], t[2], mat_id) for t in tris]
    l_out, l_mat = lb.scene(lw).debug_hit_top(rays, seed=3, t_near=MC.T_MIN)
    want, index = T.closest(tris, rays, MC.T_MIN)
    assert_bit_equal(l_out, want, name + ": the list world against triangle.closest")
    # flag, t and p do not depend on the visiting order ...
    assert_bit_equal(out[:, 0:5], l_out[:, 0:5], name + ": hit flag, t and p, Bvh against list")
    # ... normal and material wherever only one triangle attains the minimum t
    all_t = T.all_t(tris, rays, MC.T_MIN)
    best = all_t.min(axis=0)
    tie = np.isfinite(best) & ((all_t == best).sum(axis=0) > 1)
    print("%s %s: %d rays, %d hits, %d ties left out" % (name, "sah" if sah else "median", len(rays), int(np.isfinite(best).sum()), int(tie.sum())))
    assert tie.mean() <= TR.CAP_RAYS
    assert_bit_equal(out[~tie], l_out[~tie], name + ": normal, Bvh against list")
    assert np.array_equal(mat[~tie], l_mat[~tie])
    assert np.isfinite(best).sum() > len(rays) // 4


# ---- 3. wrappers against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MC.GRAPHS))
def test_hits_against_the_float64_reference(pkg, gpu, references, name):
    groups, rays, ref = references[name]
    b = gpu.builder()
    world, _ = MC.GRAPHS[name](pkg, b)
    feat = b.flatten(world)[1]
    assert feat & FEAT_TRI and bool(feat & FEAT_DEEP) == (name == "deep")
    sc = b.scene(world)
    out, mat = sc.debug_hit_top(rays, seed=5, t_near=TR.T_NEAR)
    TR.assert_hits(TR.compare(ref, out, mat), name)
    q_out, q_mat = sc.closest_hit(rays, seed=5, t_min=TR.T_NEAR)
    assert_bit_equal(q_out, out, name + ": rtg_query_closest against rtg_debug_hit_top")
    assert np.array_equal(q_mat, mat)
    # occlusion agrees with the closest hit: t_max beyond it blocks, t_max in front of it does not
    hit = out[:, 0] != 0
    far = sc.occluded(_rays8(rays, np.finfo(f32).max), seed=5, t_min=TR.T_NEAR)
    assert np.array_equal(far != 0, hit)
    near = sc.occluded(_rays8(rays, np.where(hit, out[:, 1] * f32(0.5), f32(1.0))), seed=5, t_min=TR.T_NEAR)
    assert not near[hit].any()


# ---- 4. every kernel, the same bits ---------------------------------------------------------------------------------------------
class _Swap:
    """A Builder that puts meshes where a scene function puts analytic shapes; every other call goes to the Builder as it is."""

    def __init__(self, pkg, builder, sphere_at=None, prisms=False):
        self._pkg, self._b, self._sphere_at, self._prisms, self._centres, self.swapped = pkg, builder, sphere_at, prisms, {}, 0

    def __getattr__(self, name):
        return getattr(self._b, name)

    def translate(self, offset, obj):
        i = self._b.translate(offset, obj)
        self._centres[i] = np.asarray(offset, np.float64)
        return i

    def rect_prism(self, p0, p1, material):
        if not self._prisms:
            return self._b.rect_prism(p0, p1, material)
        self.swapped += 1
        return self._b.mesh(*self._pkg.triangle.box(tuple(map(float, p0)), tuple(map(float, p1))), material)

    def bvh(self, objs, exposure=(0.0, 1.0)):
        objs = list(objs)
        if self._sphere_at is not None and len(objs) > self._sphere_at:   # one small sphere of book-1 becomes an icosphere mesh LEAF
            v, f = self._pkg.triangle.icosphere(1, 0.2, tuple(self._centres[objs[self._sphere_at]]))
            objs[self._sphere_at] = self._b.mesh(v, f, self._b.metal((0.7, 0.6, 0.5), 0.1))
            self.swapped += 1
        return self._b.bvh(objs, exposure)


def _world_a(pkg, b, nx, ny):
    return pkg.scenes.cornell_mesh_scene(b, nx, ny)[:2]


def _world_b(pkg, b, nx, ny):
    """six triangles and two rects without any Bvh: the lock-step kernel"""
    S = pkg.scenes
    grey, red = b.lambertian(b.constant(S.vfrom(0.5))), b.lambertian(b.constant(S.v(0.65, 0.05, 0.05)))
    light = b.diffuse_light(b.constant(S.vfrom(1.0)), 4.0)
    tris = MC.list_triangles(6)
    world = [b.rect(S.Y, (-3.0, 3.0), (-3.0, 3.0), 3.0, light), b.rect(S.Y, (-5.0, 5.0), (-5.0, 5.0), -1.5, grey)]
    world += [b.triangle(t[0], t[1], t[2], red if i % 2 else grey) for i, t in enumerate(tris)]
    cam = b.be.camera_look(S.v(0.5, 1.0, 6.0), S.v(0.0, 0.0, 0.0), S.v(0.0, 1.0, 0.0), 40.0, float(f32(nx) / f32(ny)), 0.0, 6.0)
    return world, cam


def _world_c(pkg, b, nx, ny):
    """book-1 with one small sphere (in front of the camera) replaced by an icosphere mesh leaf of its Bvh: it leaves the lean
    pool for the full-feature pool"""
    sw = _Swap(pkg, b, sphere_at=387)
    world, cam, _ = pkg.scenes.random_scene(sw, nx, ny)
    assert sw.swapped == 1
    return world, cam


def _world_d(pkg, b, nx, ny):
    """the book-2 final scene with the boxes of its ground Bvh as box meshes: media, Perlin and a light beside triangles"""
    sw = _Swap(pkg, b, prisms=True)
    world, cam, _ = pkg.scenes.book_final_scene(sw, nx, ny, pkg.small_rng.SmallRng(SEED))
    assert sw.swapped == 400
    return world, cam


WORLDS = {"a": _world_a, "b": _world_b, "c": _world_c, "d": _world_d}
# scene option "sync": 1 the lock-step kernel, 0 the full-feature pool kernel (the automatic choice sends frames this small to
# the lock-step kernel whenever the program fits LDS whole); world (d)'s program does not fit: the pool kernel with a program window
FORCED = [("a", 32, 32, 8, 1), ("a", 32, 32, 8, 0), ("b", 32, 24, 8, 1), ("b", 32, 24, 8, 0), ("c", 48, 32, 4, 1), ("c", 48, 32, 4, 0),
          ("d", 32, 32, 4, 0)]


@pytest.mark.parametrize("which,nx,ny,ns,sync", FORCED, ids=["%s-%s" % (w[0], "lockstep" if w[4] else "pool") for w in FORCED])
def test_every_kernel_gives_the_same_bits(pkg, gpu, capfd, which, nx, ny, ns, sync):
    b = gpu.builder()
    world, cam = WORLDS[which](pkg, b, nx, ny)
    assert b.flatten(world)[1] & FEAT_TRI and len(b.flatten_pool2(world)[0]) == 0
    sc = b.scene(world)
    sc.set_option("sync", sync)
    base, c_base, took_1 = _render_named(sc, cam, nx, ny, ns, 1, capfd)
    prod, c_prod, took_3 = _render_named(sc, cam, nx, ny, ns, 3, capfd)
    assert (took_1, took_3) == ("one-lane", "full")
    assert_bit_equal(prod, base, which + ": production kernel against one lane per pixel")
    assert c_prod == c_base and c_base["prim_tests"] > 0, (c_prod, c_base)
    assert np.isfinite(prod).all() and prod.max() > 0
    s_i, row_i, x_i = np.meshgrid(np.arange(ns), np.arange(ny), np.arange(nx), indexing="ij")
    rgb, info = sc.debug_samples(cam, nx, ny, ns, x_i.ravel(), (ny - 1 - row_i).ravel(), s_i.ravel(), seed=SEED)
    assert_bit_equal(_fold(rgb.reshape(ns, ny, nx, 3), ns), prod, which + ": the fold of rtg_debug_samples")
    rs = np.random.RandomState(64)
    xs, ys, ss = rs.randint(0, nx, 64), rs.randint(0, ny, 64), rs.randint(0, ns, 64)
    one, i_one = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, seed=SEED)
    traced, i_traced = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, seed=SEED, trace_kernel=True)
    assert_bit_equal(traced, one, which + ": RTG_FLAG_TRACE_KERNEL against the one-lane probe")
    assert np.array_equal(i_traced, i_one)


# ---- 5. exact radiance ------------------------------------------------------------------------------------------------------------
def _radiance_world(pkg, b):
    """An emitter box of 12 flipped triangles radiating L_EMIT around grey (0.5) triangle meshes and one metal mesh."""
    S, T = pkg.scenes, pkg.triangle
    grey, shiny = b.lambertian(b.constant(S.vfrom(0.5))), b.metal(S.vfrom(0.5), 0.4)
    light = b.diffuse_light(b.constant(S.v(*L_EMIT)), 1.0)
    v, f = T.box((-8.0, -8.0, -8.0), (8.0, 8.0, 8.0))
    world = [b.flip_normals(b.triangle(t[0], t[1], t[2], light)) for t in T.vertices_of(v, f)]
    world.append(b.mesh(*T.grid(4, 4, lambda x, z: -0.5 + 0.1 * np.sin(2 * x + z), (-4.0, -4.0), (4.0, 4.0)), grey))
    world.append(b.mesh(*T.icosphere(1, 0.75, (-1.0, 0.25, -1.5)), grey, sah=True))
    world.append(b.translate(S.v(1.0, 0.0, -1.0), b.rotate_y(25.0, b.mesh(*T.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), shiny))))
    cam = b.be.camera_look(S.v(-2, 2, 1), S.v(0, 0, -1), S.v(0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 1.0)
    return world, cam


@pytest.mark.parametrize("kernel", [1, 3])
def test_exact_radiance(pkg, gpu, kernel):
    nx, ny, ns, max_bounces = 48, 32, 8, 50
    b = gpu.builder()
    world, cam = _radiance_world(pkg, b)
    sc = b.scene(world)
    sc.set_option("kernel", kernel)
    ys, xs, ss = (a.ravel().astype(np.uint32) for a in np.meshgrid(np.arange(ny), np.arange(nx), np.arange(ns), indexing="ij"))
    rgb, info = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, max_bounces=max_bounces)
    k = info[:, 0].astype(np.int64)
    want = (np.ldexp(1.0, -k)[:, None] * np.array(L_EMIT)).astype(f32)
    lit = (rgb == want).all(axis=1)
    black = (rgb.view(np.uint32) == 0).all(axis=1)     # a metal that absorbed, or a path stopped at the bounce cap
    print("kernel %d: %d samples, bounces %d .. %d, %d black" % (kernel, len(k), k.min(), k.max(), black.sum()))
    bad = ~(lit | black)
    assert not bad.any(), ("%d samples are neither 0.5^k L nor an allowed zero; first" % bad.sum(), rgb[bad][0], k[bad][0])
    assert k.max() >= 4 and k.min() <= 1 and lit.sum() > len(k) // 2
    img = sc.par_cast(cam, nx, ny, ns, max_bounces=max_bounces)
    assert_bit_equal(img, _fold(np.moveaxis(rgb.reshape(ny, nx, ns, 3)[::-1], 2, 0), ns), "the frame is the ordered fold of its samples")


# ---- 6. normals reach the shader ------------------------------------------------------------------------------------------------
def test_the_feature_planes_hold_the_definition_s_normals(pkg, gpu):
    """RTG_FLAG_FEATURES, grid 1 and 2, on world (a), cornell_mesh_scene: the normal, albedo and depth planes are the fold of the
    first hits of features.subpixel_rays -- and wherever the first hit is a triangle of the icosphere mesh (which stands in the
    world unwrapped) t, p and the normal are triangle.closest's, bit for bit.  The rects and the box mesh under Translate{RotateY}
    are not triangle.py's to define: their hits come from the one-lane probe.  Rays with a tie among the icosphere's triangles
    are left out, as in test 2."""
    S, T = pkg.scenes, pkg.triangle
    nx, ny = 32, 32
    b = gpu.builder()
    world, cam = _world_a(pkg, b, nx, ny)
    sc = b.scene(world)
    tris = T.vertices_of(*T.icosphere(2, radius=82.5, centre=(212.5, 82.5, 147.5)))
    white = np.array([0.73, 0.73, 0.73], f32)
    for grid in (1, 2):
        rays = pkg.features.subpixel_rays(cam, nx, ny, grid)
        g2 = grid * grid
        flat = rays.reshape(-1, 7)
        # the probe's key is the ray's index: ray k of pixel (row, x) is asked as ray (ny - 1 - row) * nx + x of call k, as the
        # feature pass seeds it (rt_features.h) -- no medium in this world, so no draw depends on it
        out, mat = sc.debug_hit_top(flat, seed=SEED, t_near=0.001)
        hit = (out[:, 0] != 0).reshape(g2, ny, nx)
        want, index = T.closest(tris, flat, 0.001)
        all_t = T.all_t(tris, flat, 0.001)
        best = all_t.min(axis=0)
        tie = np.isfinite(best) & ((all_t == best).sum(axis=0) > 1)
        on_mesh = (want[:, 0] != 0) & (out[:, 0] != 0) & (out[:, 1] == want[:, 1]) & ~tie      # the icosphere is the first hit
        assert not ((want[:, 0] != 0) & ((out[:, 0] == 0) | (out[:, 1] > want[:, 1]))).any()     # nothing is hit behind a triangle the definition hits
        print("grid %d: %d rays, %d first hits on the icosphere, %d ties left out" % (grid, len(flat), int(on_mesh.sum()), int(tie.sum())))
        assert on_mesh.sum() > len(flat) // 50 and tie.mean() <= TR.CAP_RAYS
        assert_bit_equal(out[on_mesh], want[on_mesh], "grid %d: t, p and normal on the icosphere are the definition's" % grid)
        f = pkg.capi.features_frame(nx, ny, features={"grid": grid})
        sc.par_cast(cam, nx, ny, 2, seed=SEED, out=f, features=True)
        assert_bit_equal(f.normal, pkg.features.fold(out[:, 5:8].reshape(g2, ny, nx, 3), hit), "grid %d: normal plane" % grid)
        assert_bit_equal(f.depth, pkg.features.fold(out[:, 1].reshape(g2, ny, nx), hit), "grid %d: depth plane" % grid)
        mesh_px = on_mesh.reshape(g2, ny, nx).all(axis=0)
        assert mesh_px.any()
        assert_bit_equal(f.albedo[mesh_px], np.broadcast_to(pkg.features.fold(np.broadcast_to(white, (g2, 1, 3)), np.ones((g2, 1), bool)), (int(mesh_px.sum()), 3)),
                         "grid %d: albedo plane on the icosphere" % grid)
        assert (f.features.traced, f.features.missed) == (nx * ny, int((~hit.any(axis=0)).sum()))


def test_an_image_texture_on_a_mesh_shows_in_the_albedo_plane(pkg, gpu):
    S, T, I = pkg.scenes, pkg.triangle, pkg.image
    nx, ny = 24, 16
    img = np.random.RandomState(11).rand(8, 8, 3).astype(f32)
    prm = I.planar((0.25, 0, 0), 0.5, (0, 0.25, 0), 0.5, filter=I.BILINEAR)
    b = gpu.builder()
    v, f = T.grid(2, 2, lambda x, z: 0.0, (-2.0, -2.0), (2.0, 2.0))
    v = v[:, [0, 2, 1]].copy()                                  # the grid stood up: in the plane z = 0 ...
    f = f[:, [0, 2, 1]].copy()                                  # ... wound to face +z
    world = [b.mesh(v, f, b.lambertian(b.image(img, prm)))]
    tris = T.vertices_of(v, f)
    cam = gpu.camera_look(S.v(0.2, 0.1, 5.0), S.v(0.0, 0.0, 0.0), S.v(0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 5.0)
    rays = pkg.features.subpixel_rays(cam, nx, ny, 1).reshape(-1, 7)
    out, index = T.closest(tris, rays, 0.001)
    hit = out[:, 0] != 0
    vals = np.zeros((len(rays), 3), f32)
    vals[hit] = I.sample(img, prm, out[hit, 2:5])
    fr = pkg.capi.features_frame(nx, ny, features={"grid": 1})
    b.scene(world).par_cast(cam, nx, ny, 2, seed=SEED, out=fr, features=True)
    all_t = T.all_t(tris, rays, 0.001)
    keep = ~((all_t == all_t.min(axis=0)).sum(axis=0) > 1).reshape(ny, nx) | ~hit.reshape(ny, nx)
    assert hit.mean() > 0.3 and keep.mean() >= 1 - TR.CAP_RAYS
    assert_bit_equal(fr.albedo[keep], pkg.features.fold(vals.reshape(1, ny, nx, 3), hit.reshape(1, ny, nx))[keep], "albedo plane: the image")
    assert len(np.unique(fr.albedo.reshape(-1, 3), axis=0)) > hit.sum() // 4


# ---- 7. a closed mesh as a medium boundary ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [0.4, 1.5])
def test_a_box_mesh_bounds_a_medium(pkg, gpu, capfd, rho):
    S, T = pkg.scenes, pkg.triangle
    side, n = 1.25, 4096
    b = gpu.builder()
    v, f = T.box((-1.0, -1.0, 0.0), (1.0, 1.0, side))
    fog = b.constant_medium(b.mesh(v, f, b.lambertian(b.constant(S.vfrom(0.5)))), rho, b.isotropic(b.constant(S.vfrom(0.5))))
    light = b.diffuse_light(b.constant(S.vfrom(1.0)), 2.0)
    world = [fog, b.rect(S.Z, (-3.0, 3.0), (-3.0, 3.0), -2.0, light)]
    sc = b.scene(world)
    # parallel rays along -z through the box, well inside its faces and away from its diagonals; |d| = 2: t is not a length
    rs = np.random.RandomState(17)
    x, y = rs.uniform(-0.9, 0.9, n), rs.uniform(-0.9, 0.9, n)
    y = np.where(np.abs(np.abs(x) - np.abs(y)) < 0.02, y * 0.5, y)
    rays = np.stack([x, y, np.full(n, 3.0), np.zeros(n), np.zeros(n), np.full(n, -2.0), np.zeros(n), np.full(n, 2.0)], axis=1).astype(f32)
    clear = int((sc.occluded(rays, seed=23, t_min=0.001) == 0).sum())    # t_max = 2: the ray ends at z = -1, in front of the light
    p = float(np.exp(-rho * side))
    print("rho %g: exp(-rho l) N = %.1f +- %.1f, unblocked %d" % (rho, n * p, np.sqrt(n * p * (1 - p)), clear))
    assert PR.within(clear, n, p, sigmas=5)
    nx, ny, ns = 24, 16, 4
    cam = gpu.camera_look(S.v(0.3, 0.4, 4.0), S.v(0.0, 0.0, 0.0), S.v(0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 4.0)
    base, c_base, took_1 = _render_named(sc, cam, nx, ny, ns, 1, capfd)
    prod, c_prod, took_3 = _render_named(sc, cam, nx, ny, ns, 3, capfd)
    assert (took_1, took_3) == ("one-lane", "full")          # (F_GENERAL_BOUNDARY: the GENB instantiation walks the mesh as a boundary stream)
    assert_bit_equal(prod, base, "a mesh boundary: kernel 3 against kernel 1")
    assert c_prod == c_base and prod.max() > 0


# ---- 8. light sampling --------------------------------------------------------------------------------------------------------------
def _cornell_with_blocker(pkg, b, nx, ny, light_on_triangle):
    S = pkg.scenes
    cam, _ = S._cornell_camera(b.be, nx, ny)
    world = S.cornell_box(b)
    white = b.lambertian(b.constant(S.vfrom(0.73)))
    blocker = [(128.0, 100.0, 180.0), (428.0, 100.0, 180.0), (278.0, 100.0, 440.0)]   # 100 above the floor, under the light
    world.append(b.triangle(*blocker, white))
    if light_on_triangle:   # the light's own material (cornell_box makes it fourth: id 3) on a triangle: no longer "list-level rects only"
        world.append(b.triangle((10.0, 554.0, 300.0), (60.0, 554.0, 300.0), (35.0, 554.0, 340.0), 3))
    return world, cam, np.array([blocker], f32)


def test_light_sampling_with_a_triangle_blocker(pkg, gpu, capfd):
    S, T = pkg.scenes, pkg.triangle
    nx, ny, ns = 32, 32, 4
    b = gpu.builder()
    world, cam, blocker = _cornell_with_blocker(pkg, b, nx, ny, False)
    sc = b.scene(world)
    plain = sc.par_cast(cam, nx, ny, ns, seed=SEED, max_bounces=1)
    sc.set_option("light_sampling", 1)
    sc.set_option("verbose", 1)
    capfd.readouterr()
    lit = sc.par_cast(cam, nx, ny, ns, seed=SEED, max_bounces=1)
    sc.set_option("verbose", 0)
    assert "light table of 1 rect(s)" in capfd.readouterr().err
    assert np.isfinite(lit).all() and not np.array_equal(lit, plain)
    # the umbra: floor points from which EVERY point of the light is behind the blocker get no direct term.  The camera ray
    # through a pixel centre meets the floor at p; the light's four corners are tested with the numpy occlusion answer.
    rays = pkg.features.subpixel_rays(cam, nx, ny, 1).reshape(-1, 7).astype(np.float64)
    t_floor = -rays[:, 1] / rays[:, 4]
    p = rays[:, 0:3] + t_floor[:, None] * rays[:, 3:6]
    on_floor = (rays[:, 4] < 0) & (p[:, 0] > 5) & (p[:, 0] < 550) & (p[:, 2] > 5) & (p[:, 2] < 550)
    blocked = np.ones(len(p), bool)
    for lx in (213.0, 343.0):
        for lz in (227.0, 332.0):
            corner = np.array([lx, 554.0, lz])
            r8 = np.concatenate([p, corner - p, np.zeros((len(p), 1)), np.ones((len(p), 1))], axis=1).astype(f32)
            blocked &= T.occluded(blocker, r8, 0.001) != 0
    # The umbra is convex (an intersection of the triangle's shadows).  A pixel whose eight neighbours' centres lie in it, like
    # its own, lies in it whole: its jittered samples meet the floor inside the hull of those nine points.
    umbra = (on_floor & blocked).reshape(ny, nx)
    assert umbra.sum() >= 9, "the blocker must shade some pixel centres from the whole light"
    core = umbra.copy()
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            core &= np.roll(np.roll(umbra, dr, axis=0), dc, axis=1)
    core[[0, -1], :] = False
    core[:, [0, -1]] = False
    assert core.sum() >= 1
    rows, cols = np.nonzero(core.reshape(ny, nx))
    xs = np.repeat(cols, ns).astype(np.uint32)
    ys = np.repeat(ny - 1 - rows, ns).astype(np.uint32)
    ss = np.tile(np.arange(ns), len(rows)).astype(np.uint32)
    # (max_bounces = 1: the first hit takes the light sample, the hit behind it none, and the sampled light it may find is not
    # counted again -- a sample's colour is its direct term alone)
    rgb, info = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, seed=SEED, max_bounces=1)
    assert (rgb.view(np.uint32) == 0).all(), "a floor point in the umbra gets no direct light"
    far = on_floor & ~blocked & (np.abs(p[:, 0] - 278.0) > 200.0)
    rows, cols = np.nonzero(far.reshape(ny, nx))
    rgb, _ = sc.debug_samples(cam, nx, ny, 1, cols.astype(np.uint32), (ny - 1 - rows).astype(np.uint32), np.zeros(len(rows), np.uint32), seed=SEED, max_bounces=1)
    assert (rgb > 0).any(), "floor points that see the light get a direct term"


def test_a_light_on_a_triangle_is_never_sampled(pkg, gpu, capfd):
    nx, ny, ns = 24, 24, 4
    b = gpu.builder()
    world, cam, _ = _cornell_with_blocker(pkg, b, nx, ny, True)
    sc = b.scene(world)
    plain = sc.par_cast(cam, nx, ny, ns, seed=SEED)
    sc.set_option("light_sampling", 1)
    sc.set_option("verbose", 1)
    capfd.readouterr()
    same = sc.par_cast(cam, nx, ny, ns, seed=SEED)
    sc.set_option("verbose", 0)
    assert "light table of 0 rect(s)" in capfd.readouterr().err
    assert_bit_equal(same, plain, "an empty light table: the frame without the option")
    assert plain.max() > 0


# ---- 9. the rest of the surface, on world (a) -----------------------------------------------------------------------------------------
def _scene_a(pkg, gpu, nx, ny):
    b = gpu.builder()
    world, cam = _world_a(pkg, b, nx, ny)
    return b.scene(world), cam


def test_two_handles_give_the_one_handle_frame(pkg, gpu):
    nx, ny, ns = 32, 32, 4
    one, cam = _scene_a(pkg, gpu, nx, ny)
    want = one.par_cast(cam, nx, ny, ns, seed=SEED)
    scenes = []
    for _ in range(2):
        sc, cam = _scene_a(pkg, gpu, nx, ny)
        sc.set_option("force_rccl", 1)
        scenes.append(sc)
    assert_bit_equal(gpu.par_cast_multi(scenes, cam, nx, ny, ns, seed=SEED), want, "rtg_par_cast_multi, two handles on one device")


def test_ray_frames_progressive_frames_and_counts(pkg, gpu):
    nx, ny, ns = 24, 24, 4
    sc, cam = _scene_a(pkg, gpu, nx, ny)
    want = sc.par_cast(cam, nx, ny, ns, seed=SEED)
    assert want.max() > 0
    rays = pkg.rays.camera_rays(cam, nx, ny, ns, SEED)
    assert_bit_equal(sc.cast_rays(rays, nx, ny, ns, per_sample=True, seed=SEED), want, "a ray frame of the camera's own rays")
    part = sc.par_cast(cam, nx, ny, 2, seed=SEED, partial=True)
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns, seed=SEED, out=part, sample_begin=2, resume=True), want, "a progressive frame in two slices")
    counts = np.full((ny, nx), ns, np.uint32)
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns, seed=SEED, counts=counts), want, "a counts call with n_p == ns")
