"""Surface attributes on the GPU (include/rtiow_gpu_surface.h): list worlds against the numpy definition bit for bit, attribute
meshes under a Bvh against the same triangles as a list, wrapper chains against float64 (surface_cases.py, with the CPU test's
tolerances and cap), every kernel on the new Cornell scene, the feature planes (the image follows the surface), exact radiance, and
the rest of the surface.  Frames are at most 48 x 32 x 8 and ray sets at most 4 096."""
import numpy as np
import pytest

import mesh_cases as MC
import physics_ref as PR
import surface_cases as SC
import triangle_ref as TR
from conftest import assert_bit_equal
from test_image_texture_gpu import COUNTERS, _fold, _render_named

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 0xDEADBEEF
FEAT_DEEP, FEAT_TRI, FEAT_SURFACE = 128, 1024, 2048
L_EMIT = PR.L_EMIT


# ---- 1. list worlds, bit-exact --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 7])
def test_a_list_world_equals_the_definition(pkg, gpu, k):
    T = pkg.triangle
    tris = MC.list_triangles(k)
    attrs = SC.list_attributes(T, tris)             # both, normals only, UVs only, plain, in turn
    b = gpu.builder()
    mats = [b.lambertian(b.constant((0.1 * (i + 1), 0.5, 0.5))) for i in range(k)]
    flips = [i % 3 == 1 for i in range(k)]
    world = []
    for i in range(k):
        t = b.triangle_attr(tris[i, 0], tris[i, 1], tris[i, 2], mats[i], normals=attrs[i][0], uvs=attrs[i][1])
        world.append(b.flip_normals(t) if flips[i] else t)
    feat = b.flatten(world)[1]
    assert feat & FEAT_TRI and feat & FEAT_SURFACE and not feat & FEAT_DEEP
    sc = b.scene(world)
    rays = MC.edge_rays(tris)
    want, index = T.closest_attr(tris, [a[0] for a in attrs], [a[1] for a in attrs], rays, MC.T_MIN, flips=flips)
    want_mat = np.where(index >= 0, np.asarray(mats, np.uint32)[np.maximum(index, 0)], 0xFFFFFFFF).astype(np.uint32)
    out, mat = sc.debug_hit_surface(rays, seed=7, t_near=MC.T_MIN)
    assert_bit_equal(out, want, "rtg_debug_hit_surface against triangle.closest_attr, %d triangles" % k)
    assert np.array_equal(mat, want_mat)
    hit = want[:, 0] != 0
    assert hit.sum() > len(rays) // 4 and (~hit).sum() > len(rays) // 10
    top, t_mat = sc.debug_hit_top(rays, seed=7, t_near=MC.T_MIN)
    assert_bit_equal(top, want[:, :8], "rtg_debug_hit_top: the shading normal")
    assert np.array_equal(t_mat, want_mat)
    q_out, q_mat = sc.closest_hit(rays, seed=7, t_min=MC.T_MIN)
    assert_bit_equal(q_out, want[:, :8], "rtg_query_closest: the shading normal")
    assert np.array_equal(q_mat, want_mat)
    # attributes do not move t: occlusion as the plain triangles answer it
    r8 = np.concatenate([rays, np.where(hit, want[:, 1] * f32(1.5), f32(1.0))[:, None]], axis=1).astype(f32)
    assert np.array_equal(sc.occluded(r8, seed=7, t_min=MC.T_MIN), T.occluded(tris, r8, MC.T_MIN))


def test_a_world_without_attributes_answers_zeros(pkg, gpu):
    T = pkg.triangle
    tris = MC.list_triangles(3)
    b = gpu.builder()
    lam = b.lambertian(b.constant((0.5, 0.5, 0.5)))
    world = [b.triangle(t[0], t[1], t[2], lam) for t in tris] + [b.translate((0.0, 0.0, -3.0), b.sphere(1.0, lam))]
    assert not b.flatten(world)[1] & FEAT_SURFACE
    sc = b.scene(world)
    rays = MC.edge_rays(tris)
    out, mat = sc.debug_hit_surface(rays, seed=7, t_near=MC.T_MIN)
    top, t_mat = sc.debug_hit_top(rays, seed=7, t_near=MC.T_MIN)
    assert_bit_equal(out[:, :8], top)
    assert np.array_equal(mat, t_mat)
    assert not out[:, 8:].any()


# ---- 2. a mesh under a Bvh against the same triangles as a list -----------------------------------------------------------------
@pytest.fixture(scope="module")
def references(pkg, gpu):
    out = {}
    for name in MC.GRAPHS:
        _, groups = SC.graph(pkg, gpu.builder(), name)
        rays = MC.aimed_rays(groups).astype(f32)
        r64 = rays.astype(np.float64)
        out[name] = (groups, rays, TR.closest_hit64(groups, r64[:, 0:3], r64[:, 3:6], r64[:, 6]))
    return out


@pytest.mark.parametrize("name", ["ico", "box"])
@pytest.mark.parametrize("sah", [False, True], ids=["median", "sah"])
def test_a_mesh_under_a_bvh_equals_its_triangles_as_a_list(pkg, gpu, references, name, sah):
    T = pkg.triangle
    groups, rays, ref = references[name]
    rays = rays[ref["margin"] > TR.MARGIN]
    g = groups[0]
    b = gpu.builder()
    ab = SC.AttrBuilder(pkg, b)
    world, _ = MC.GRAPHS[name](pkg, ab, sah=sah)
    assert b.flatten(world)[1] & FEAT_SURFACE
    out, mat = b.scene(world).debug_hit_surface(rays, seed=3, t_near=MC.T_MIN)
    lb = gpu.builder()
    MC._mats(lb)
    lw = [lb.triangle_attr(t[0], t[1], t[2], g["mat"], normals=g["normals"][i], uvs=g["uvs"][i]) for i, t in enumerate(g["tri"])]
    l_out, l_mat = lb.scene(lw).debug_hit_surface(rays, seed=3, t_near=MC.T_MIN)
    want, index = T.closest_attr(g["tri"], g["normals"], g["uvs"], rays, MC.T_MIN)
    assert_bit_equal(l_out, want, name + ": the list world against triangle.closest_attr")
    assert_bit_equal(out[:, 0:5], l_out[:, 0:5], name + ": hit flag, t and p, Bvh against list")
    all_t = T.all_t(g["tri"], rays, MC.T_MIN)
    best = all_t.min(axis=0)
    tie = np.isfinite(best) & ((all_t == best).sum(axis=0) > 1)
    print("%s %s: %d rays, %d hits, %d ties left out" % (name, "sah" if sah else "median", len(rays), int(np.isfinite(best).sum()), int(tie.sum())))
    assert tie.mean() <= TR.CAP_RAYS
    assert_bit_equal(out[~tie], l_out[~tie], name + ": normal and (tu, tv), Bvh against list")
    assert np.array_equal(mat[~tie], l_mat[~tie])


# ---- 3. wrappers against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wrapped", "deep"])
def test_under_wrappers_against_float64(pkg, gpu, references, name):
    groups, rays, ref = references[name]
    b = gpu.builder()
    world, _ = SC.graph(pkg, b, name)
    feat = b.flatten(world)[1]
    assert feat & FEAT_SURFACE and bool(feat & FEAT_DEEP) == (name == "deep")
    sc = b.scene(world)
    out, mat = sc.debug_hit_surface(rays, seed=5, t_near=TR.T_NEAR)
    res = TR.compare(ref, out[:, :8], mat)
    res["dn"] = 0.0                                   # (the shading normal is compared below, with its own tolerance)
    TR.assert_hits(res, name)
    SC.assert_attr(SC.compare_attr(groups, ref, rays, out), name)
    q_out, q_mat = sc.closest_hit(rays, seed=5, t_min=TR.T_NEAR)
    assert_bit_equal(q_out, out[:, :8], name + ": rtg_query_closest against rtg_debug_hit_surface")


def test_a_translate_by_powers_of_two_leaves_tu_tv_bit_equal(pkg, gpu):
    """Wrappers do not touch (tu, tv): under Translate by (4, -2, 8) a ray moved by the same offset on the host -- exact for these
    origins, multiples of 2^-10 below 16 -- sees the very primitive-space ray, so every output but p is bit-equal."""
    T = pkg.triangle
    v, f, nn, uv = T.icosphere_attr(1, 1.0)
    off = np.array([4.0, -2.0, 8.0], f32)
    rs = np.random.RandomState(4)
    o = (np.round(rs.uniform(-3, 3, (2048, 3)) * 1024) / 1024).astype(f32)
    target = rs.normal(0, 0.6, (2048, 3)).astype(f32)
    rays = np.concatenate([o, target - o, np.zeros((2048, 1), f32)], axis=1).astype(f32)
    moved = rays.copy()
    moved[:, 0:3] += off
    assert np.array_equal((moved[:, 0:3] - off), rays[:, 0:3])
    outs = []
    for wrapped in (False, True):
        b = gpu.builder()
        m = b.mesh(v, f, b.lambertian(b.constant((0.5, 0.5, 0.5))), normals=nn, uvs=uv)
        sc = b.scene([b.translate(off, m) if wrapped else m])
        outs.append(sc.debug_hit_surface(moved if wrapped else rays, seed=1, t_near=0.001)[0])
    plain, wrapped = outs
    assert (plain[:, 0] != 0).sum() > 500
    assert_bit_equal(wrapped[:, [0, 1, 5, 6, 7, 8, 9]], plain[:, [0, 1, 5, 6, 7, 8, 9]], "flag, t, normal, (tu, tv) under an exact Translate")


# ---- 4. every kernel, the same bits ---------------------------------------------------------------------------------------------
def _surface_world(pkg, b, nx, ny, subdivisions=2):
    world, cam, _, info = pkg.scenes.cornell_surface_scene(b, nx, ny, subdivisions=subdivisions)
    return world, cam, info


FORCED = [(2, 32, 32, 8, 1), (2, 32, 32, 8, 0), (4, 32, 24, 4, 0)]


@pytest.mark.parametrize("sub,nx,ny,ns,sync", FORCED, ids=["lockstep", "pool", "pool-window"])
def test_every_kernel_gives_the_same_bits(pkg, gpu, capfd, sub, nx, ny, ns, sync):
    """The new Cornell scene on the lock-step kernel, the pool kernel and the one-lane kernel; once more with an icosphere of
    5 120 attribute triangles (30 720 records: more than the 5 000-odd a CU's LDS holds), which runs through the pool kernel's
    program window."""
    b = gpu.builder()
    world, cam, _ = _surface_world(pkg, b, nx, ny, sub)
    words, feat = b.flatten(world)
    assert feat & FEAT_SURFACE and len(b.flatten_pool2(world)[0]) == 0
    sc = b.scene(world)
    sc.set_option("sync", sync)
    base, c_base, took_1 = _render_named(sc, cam, nx, ny, ns, 1, capfd)
    sc.set_option("verbose", 1)
    capfd.readouterr()
    prod, c_prod, took_3 = _render_named(sc, cam, nx, ny, ns, 3, capfd)
    assert (took_1, took_3) == ("one-lane", "full")
    if sub == 4:
        assert len(words) * 32 > 160 * 1024
    assert_bit_equal(prod, base, "production kernel against one lane per pixel")
    assert c_prod == c_base and c_base["prim_tests"] > 0, (c_prod, c_base)
    assert np.isfinite(prod).all() and prod.max() > 0
    rs = np.random.RandomState(64)
    xs, ys, ss = rs.randint(0, nx, 64), rs.randint(0, ny, 64), rs.randint(0, ns, 64)
    one, i_one = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, seed=SEED)
    traced, i_traced = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, seed=SEED, trace_kernel=True)
    assert_bit_equal(traced, one, "RTG_FLAG_TRACE_KERNEL against the one-lane probe")
    assert np.array_equal(i_traced, i_one)


def test_the_window_is_reported(pkg, gpu, capfd):
    nx, ny = 16, 16
    b = gpu.builder()
    world, cam, _ = _surface_world(pkg, b, nx, ny, 4)
    sc = b.scene(world)
    sc.set_option("sync", 0)
    sc.set_option("verbose", 1)
    capfd.readouterr()
    sc.par_cast(cam, nx, ny, 1, seed=SEED)
    err = capfd.readouterr().err
    import re
    m = re.search(r"program window: (\d+) of (\d+) records", err)
    assert m and int(m.group(1)) < int(m.group(2)), err[-500:]


# ---- 5. the feature planes: the image follows the surface ---------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [0, 1], ids=["nearest", "bilinear"])
def test_the_feature_planes(pkg, gpu, filt):
    S, I = pkg.scenes, pkg.image
    nx, ny = 32, 32
    planes = {}
    for wrapped in (True, False):
        b = gpu.builder()
        world, cam, _, info = S.cornell_surface_scene(b, nx, ny, filter=filt, box_wrapped=wrapped)
        sc = b.scene(world)
        rays = pkg.features.subpixel_rays(cam, nx, ny, 1).reshape(-1, 7)
        out, mat = sc.debug_hit_surface(rays, seed=SEED, t_near=0.001)
        hit = (out[:, 0] != 0).reshape(1, ny, nx)
        fr = pkg.capi.features_frame(nx, ny, features={"grid": 1})
        sc.par_cast(cam, nx, ny, 2, seed=SEED, out=fr, features=True)
        assert_bit_equal(fr.normal, pkg.features.fold(out[:, 5:8].reshape(1, ny, nx, 3), hit), "normal plane: the fold of rtg_debug_hit_surface's normals")
        on_box = (out[:, 0] != 0) & ((out[:, 8] != 0) | (out[:, 9] != 0)) & (out[:, 3] < 400.0)       # UVs, and below the emissive triangle at y = 500
        assert on_box.sum() > 40
        uvz = np.concatenate([out[:, 8:10], np.zeros((len(out), 1), f32)], axis=1)
        vals = I.sample(info["image"], info["params"], uvz[on_box])
        assert_bit_equal(fr.albedo.reshape(-1, 3)[on_box], pkg.features.fold(vals.reshape(1, -1, 3), np.ones((1, int(on_box.sum())), bool)),
                         "albedo plane over the UV-mapped mesh: image.sample at (tu, tv, 0)")
        planes[wrapped] = (out, on_box, fr.albedo.reshape(-1, 3).copy())
        assert len(np.unique(vals, axis=0)) > 4
    # The second frame: the same mesh without its Translate{RotateY}.  The image follows the surface: on both frames the albedo is
    # the image at the hit's (tu, tv) (above), whatever p is -- and on the wrapped mesh a planar mapping of p, which is all an image
    # could do before, reads other texels
    (o_w, on_w, a_w), (o_u, on_u, a_u) = planes[True], planes[False]
    assert on_u.sum() > 40 and not np.array_equal(o_w[on_w][:, 2:5][:40], o_u[on_u][:, 2:5][:40])
    p_vals = I.sample(info["image"], info["params"], o_w[on_w, 2:5])
    assert not np.array_equal(pkg.features.fold(p_vals.reshape(1, -1, 3), np.ones((1, len(p_vals)), bool)), a_w[on_w])
    # corresponding hits: the unwrapped frame's hit whose (tu, tv) is nearest to a wrapped hit's, within the CPU test's tolerance,
    # on a face where (tu, tv) names the point (the faces orthogonal to z), shows the albedo of the same texel under the nearest filter
    if filt == 0:
        face_w, face_u = on_w & (np.abs(o_w[:, 7]) > 0.9), on_u & (np.abs(o_u[:, 7]) > 0.9)
        w_img, h_img = info["image"].shape[1], info["image"].shape[0]
        texel = lambda o: (np.floor(o[:, 8] * w_img).astype(int), np.floor((1 - o[:, 9]) * h_img).astype(int))   # noqa: E731
        tw, tu_ = texel(o_w[face_w]), texel(o_u[face_u])
        seen = {}
        for x, y, a in zip(tu_[0], tu_[1], a_u[face_u]):
            seen.setdefault((x, y), a)
        matched = [(seen[(x, y)], a) for x, y, a in zip(tw[0], tw[1], a_w[face_w]) if (x, y) in seen]
        assert len(matched) > 10
        for a, c in matched:
            assert_bit_equal(a, c, "the same texel on the wrapped and the unwrapped mesh")


# ---- 6. exact radiance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 3])
def test_exact_radiance(pkg, gpu, kernel):
    """A grey smooth mesh inside a flipped emitter box: every sample is 0.5^k L or an allowed zero (a path stopped at the cap)."""
    S, T = pkg.scenes, pkg.triangle
    nx, ny, ns, max_bounces = 48, 32, 8, 50
    b = gpu.builder()
    grey = b.lambertian(b.constant(S.vfrom(0.5)))
    light = b.diffuse_light(b.surface(b.constant(S.v(*L_EMIT))), 1.0)
    v, f = T.box((-8.0, -8.0, -8.0), (8.0, 8.0, 8.0))
    world = [b.flip_normals(b.triangle_attr(t[0], t[1], t[2], light, uvs=((0, 0), (1, 0), (0, 1)))) for t in T.vertices_of(v, f)]
    for centre, radius in (((0.0, 0.5, -1.0), 1.5), ((2.4, 0.0, 0.2), 1.0), ((-1.6, -0.4, 1.2), 0.6)):   # smooth spheres close to one another ...
        vs, fs, ns_, uvs = T.icosphere_attr(2, radius, centre)
        world.append(b.mesh(vs, fs, grey, normals=ns_, uvs=uvs))
    vg, fg = T.grid(4, 4, lambda x, z: -1.0 + 0.1 * np.sin(2 * x + z), (-4.0, -4.0), (4.0, 4.0))                 # ... on a smooth floor
    world.append(b.mesh(vg, fg, grey, normals=T.vertex_normals(vg, fg)))
    cam = b.be.camera_look(S.v(-2, 2, 4), S.v(0, 0, -1), S.v(0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 1.0)
    assert b.flatten(world)[1] & FEAT_SURFACE
    sc = b.scene(world)
    sc.set_option("kernel", kernel)
    ys, xs, ss = (a.ravel().astype(np.uint32) for a in np.meshgrid(np.arange(ny), np.arange(nx), np.arange(ns), indexing="ij"))
    rgb, info = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, max_bounces=max_bounces)
    k = info[:, 0].astype(np.int64)
    want = (np.ldexp(1.0, -k)[:, None] * np.array(L_EMIT)).astype(f32)
    lit = (rgb == want).all(axis=1)
    black = (rgb.view(np.uint32) == 0).all(axis=1)
    print("kernel %d: %d samples, bounces %d .. %d, %d black" % (kernel, len(k), k.min(), k.max(), black.sum()))
    bad = ~(lit | black)
    assert not bad.any(), ("%d samples are neither 0.5^k L nor an allowed zero; first" % bad.sum(), rgb[bad][0], k[bad][0])
    assert k.max() >= 3 and k.min() == 0 and lit.sum() > len(k) // 2
    assert black.sum() <= (k == max_bounces).sum()
    img = sc.par_cast(cam, nx, ny, ns, max_bounces=max_bounces)
    assert_bit_equal(img, _fold(np.moveaxis(rgb.reshape(ny, nx, ns, 3)[::-1], 2, 0), ns), "the frame is the ordered fold of its samples")


# ---- 7. the rest of the surface -------------------------------------------------------------------------------------------------
def _scene(pkg, gpu, nx, ny):
    b = gpu.builder()
    world, cam, _ = _surface_world(pkg, b, nx, ny)
    return b.scene(world), cam


def test_two_handles_give_the_one_handle_frame(pkg, gpu):
    nx, ny, ns = 32, 32, 4
    one, cam = _scene(pkg, gpu, nx, ny)
    want = one.par_cast(cam, nx, ny, ns, seed=SEED)
    scenes = []
    for _ in range(2):
        sc, cam = _scene(pkg, gpu, nx, ny)
        sc.set_option("force_rccl", 1)
        scenes.append(sc)
    assert_bit_equal(gpu.par_cast_multi(scenes, cam, nx, ny, ns, seed=SEED), want, "rtg_par_cast_multi, two handles on one device")


def test_ray_frames_progressive_frames_and_counts(pkg, gpu):
    nx, ny, ns = 24, 24, 4
    sc, cam = _scene(pkg, gpu, nx, ny)
    want = sc.par_cast(cam, nx, ny, ns, seed=SEED)
    assert want.max() > 0
    rays = pkg.rays.camera_rays(cam, nx, ny, ns, SEED)
    assert_bit_equal(sc.cast_rays(rays, nx, ny, ns, per_sample=True, seed=SEED), want, "a ray frame of the camera's own rays")
    part = sc.par_cast(cam, nx, ny, 2, seed=SEED, partial=True)
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns, seed=SEED, out=part, sample_begin=2, resume=True), want, "a progressive frame in two slices")
    counts = np.full((ny, nx), ns, np.uint32)
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns, seed=SEED, counts=counts), want, "a counts call with n_p == ns")


def test_light_sampling_with_an_attribute_mesh_as_blocker(pkg, gpu):
    """The umbra stays black: a smooth mesh between the rect light and the floor blocks every shadow ray its plain twin blocks --
    attributes do not move t."""
    S, T = pkg.scenes, pkg.triangle
    nx, ny, ns = 32, 24, 8
    imgs = {}
    for smooth in (False, True):
        b = gpu.builder()
        white = b.lambertian(b.constant(S.vfrom(0.73)))
        light = b.diffuse_light(b.constant(S.vfrom(1.0)), 15.0)
        vs, fs, nn, _ = T.icosphere_attr(1, 120.0, (278.0, 300.0, 278.0))
        world = [b.rect(S.Y, (213.0, 343.0), (227.0, 332.0), 554.0, light), b.rect(S.Y, (0.0, 555.0), (0.0, 555.0), 0.0, white),
                 b.mesh(vs, fs, white, normals=nn if smooth else None)]
        cam, _ = S._cornell_camera(b.be, nx, ny)
        sc = b.scene(world)
        for ls in (0, 1):
            sc.set_option("light_sampling", ls)
            imgs[(smooth, ls)] = sc.par_cast(cam, nx, ny, ns, seed=SEED, max_bounces=0 if ls else 50)
    # with max_bounces 0 and light sampling only direct light reaches a pixel: where the plain mesh's frame is black on the floor
    # (the umbra), the smooth mesh's is black too
    umbra = (imgs[(False, 1)] == 0).all(axis=2)
    assert umbra.sum() > 20 and (imgs[(True, 1)][umbra] == 0).all()
    assert np.isfinite(imgs[(True, 0)]).all() and imgs[(True, 0)].max() > 0
    assert not np.array_equal(imgs[(True, 0)], imgs[(False, 0)])          # smooth shading changes the picture
