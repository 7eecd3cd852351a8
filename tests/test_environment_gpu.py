"""The scene's environment on the GPU (include/rtiow_gpu_environment.h): the device probe against the host probe and the numpy
definition; a miss is E(d) on every kernel; a constant environment is the flag's constant background, frame and counters; a
furnace; an image environment renders the same bits on every kernel, through every frame kind and entry point; a mirror bounce;
light sampling books it at full weight.  Every comparison is bitwise."""
import numpy as np
import pytest

import environment_cases as EC
from conftest import assert_bit_equal, bits
from test_retire_gpu import _DeviceBuf, _hip

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEF
COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")   # all six
f32 = np.float32
ROT, SCALE = 33.3, (1.0, 0.5, 2.0)   # the image environment of the frame tests
KERNELS = (1, 3)                      # scene option "kernel": 1 = one lane per pixel, 3 = the production kernels (the default)


def _render_named(sc, cam, nx, ny, ns, kernel, capfd, **kw):
    """(frame, the six counters, what option verbose says ran, its text): "lean" (the lean pool kernel), "pool2", "full" (the
    full-feature pool kernel or the lock-step kernel, which reports with that kernel's line: scene option sync = 0 / 1 picks
    between them) or "one-lane" (none of their lines).  Switching verbose on also prints the environment's own line."""
    sc.set_option("kernel", kernel)
    capfd.readouterr()
    sc.set_option("verbose", 1)
    try:
        out, st = sc.par_cast(cam, nx, ny, ns, seed=SEED, stats=True, **kw)
    finally:
        sc.set_option("verbose", 0)
    err = capfd.readouterr().err
    if "[rtg] pool: samples [" in err:
        took = "lean"
    elif "[rtg] full pool 2" in err:
        took = "pool2"
    elif "[rtg] full pool" in err:
        took = "full"
    else:
        took = "one-lane"
    return out, {k: st[k] for k in COUNTERS}, took, err


def _fold(samples, ns):
    """[ns, ...] per-sample colours -> the left fold from +0, divided by float32(ns) (lib.rs:365-374)."""
    acc = np.zeros(samples.shape[1:], f32)
    for s in range(ns):
        acc = (acc + samples[s]).astype(f32)
    return (acc / f32(ns)).astype(f32)


def _all_keys(nx, ny, ns):
    s_i, row_i, x_i = np.meshgrid(np.arange(ns), np.arange(ny), np.arange(nx), indexing="ij")
    return x_i.ravel(), (ny - 1 - row_i).ravel(), s_i.ravel()


# ---- 1. the device probe ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", EC.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_device_probe_equals_the_host_probe_and_numpy(pkg, gpu, size):
    I, E = pkg.image, pkg.environment
    b = gpu.builder()
    world = EC.far_sphere_world(b)
    img = EC.image(size)
    d = EC.directions()
    k = 0
    for prm in EC.settings(I):
        t = b.image(img, prm)
        deg, scale = EC.ROTATIONS[k % 4], EC.SCALES[k % 3]     # (every rotation and scale comes up; the host test takes the product)
        k += 1
        b.environment(t, scale=scale, rotate_y=deg)
        e = b.get_environment()
        sc = b.scene(world)
        got = sc.debug_environment(d)
        what = "%s, %g degrees, scale %r" % (EC.name(prm), deg, scale)
        assert_bit_equal(got, E.colour(d, img, prm, scale, e["s"], e["c"]), what + ": device against numpy")
        assert_bit_equal(got, b.environment_host(d), what + ": device against host")


def test_the_device_probe_on_constant_checker_and_perlin(pkg, gpu):
    E = pkg.environment
    b = gpu.builder()
    b.set_perlin_tables(*pkg.scenes.perlin_tables(SEED))
    world = EC.far_sphere_world(b)
    d = EC.directions()
    con = b.constant(EC.CONSTANT)
    chk = b.checker(con, b.image(EC.image((5, 3)), pkg.image.spherical()))
    per = b.perlin(0.7)
    plain = b.scene(world)
    with pytest.raises(pkg.capi.RtError):
        plain.debug_environment(d[:4])                                      # a scene without an environment has no probe
    for deg, scale in zip(EC.ROTATIONS, EC.SCALES + EC.SCALES[:1]):
        b.environment(con, scale=scale, rotate_y=deg)
        e = b.get_environment()
        assert_bit_equal(b.scene(world).debug_environment(d), E.colour(d, EC.CONSTANT, None, scale, e["s"], e["c"]), "constant")
        for tex, what in ((chk, "checker"), (per, "perlin")):
            b.environment(tex, scale=scale, rotate_y=deg)
            sc = b.scene(world)
            q = E.direction(d, e["s"], e["c"])
            with np.errstate(all="ignore"):
                want = (np.array(scale, f32)[None, :] * sc.debug_texture(tex, q)).astype(f32)
            assert_bit_equal(sc.debug_environment(d), want, "%s: scale * rtg_debug_texture(q)" % what)


# ---- 2. a miss is E(d), on every kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["image", "checker"])
def test_a_miss_is_the_environment_colour(pkg, gpu, capfd, kind):
    E = pkg.environment
    nx = ny = 16
    b = gpu.builder()
    world = EC.far_sphere_world(b)
    tex, img, prm = EC.lat_long(pkg, b)
    if kind == "checker":
        tex = b.checker(tex, b.constant((0.1, 0.9, 0.4)))
    b.environment(tex, scale=SCALE, rotate_y=ROT)
    e = b.get_environment()
    sc = b.scene(world)
    rays = EC.miss_rays(nx * ny)
    assert not sc.closest_hit(rays)[0][:, 0].any()                                    # none of them hits
    if kind == "image":
        env = E.colour(rays[:, 3:6], img, prm, SCALE, e["s"], e["c"])
    else:
        env = sc.debug_environment(rays[:, 3:6])
    want = EC.miss_colour(np.zeros(3, f32), np.ones(3, f32), env).reshape(ny, nx, 3)     # 0 + 1 * E(d), ns = 1: divided by 1
    assert len(np.unique(bits(want).reshape(-1, 3), axis=0)) > 32                      # a picture, not a colour
    for kernel in KERNELS:
        sc.set_option("kernel", kernel)
        capfd.readouterr()
        sc.set_option("verbose", 1)
        got = sc.cast_rays(rays, nx, ny, 1, seed=SEED)
        sc.set_option("verbose", 0)
        err = capfd.readouterr().err
        assert "[rtg] ray frame: general kernel" in err and "lean pool" not in err, err  # never the lean ray-frame path
        assert "[rtg] environment: texture %d" % tex in err
        assert_bit_equal(got, want, "ray frame, kernel %d" % kernel)
    # ... and the camera frames of the same empty world, whose every path is one miss (a list world without a Bvh: the lock-step kernel)
    cam = EC.deep_camera(gpu, nx, ny)
    frames = {}
    for kernel in KERNELS:
        frames[kernel], _, took, _ = _render_named(sc, cam, nx, ny, 2, kernel, capfd)
        assert took == ("one-lane" if kernel == 1 else "full"), took
    crays = pkg.rays.camera_rays(cam, nx, ny, 2, SEED)
    if kind == "image":
        cenv = E.colour(crays[:, 3:6], img, prm, SCALE, e["s"], e["c"])
    else:
        cenv = sc.debug_environment(crays[:, 3:6])
    cwant = _fold(EC.miss_colour(np.zeros(3, f32), np.ones(3, f32), cenv).reshape(2, ny, nx, 3), 2)
    for kernel in KERNELS:
        assert_bit_equal(frames[kernel], cwant, "camera frame of misses, kernel %d" % kernel)


# ---- 3. a constant environment is the constant background ------------------------------------------------------------------------
K, K_SCALE, K_PRODUCT = (0.5, 0.25, 2.0), (1.5, 4.0, 0.5), (0.75, 1.0, 1.0)   # scale * k is exact


def _constant_world(pkg, b, name, nx, ny):
    if name == "book1":
        world, cam, _, _ = pkg.scenes.random_scene(b, nx, ny, sky="background")
        return world, cam
    return EC.open_cornell(pkg, b, nx, ny)


@pytest.mark.parametrize("name", ["book1", "cornell"])
def test_a_constant_environment_is_the_constant_background(pkg, gpu, capfd, name):
    nx, ny, ns = 32, 32, 8
    assert (np.array(K, f32) * np.array(K_SCALE, f32) == np.array(K_PRODUCT, f32)).all()
    b0 = gpu.builder()
    world0, cam = _constant_world(pkg, b0, name, nx, ny)
    plain = b0.scene(world0)
    want = {k: _render_named(plain, cam, nx, ny, ns, k, capfd, background=K_PRODUCT) for k in KERNELS}
    assert want[3][2] == ("lean" if name == "book1" else "full"), want[3][2]
    assert_bit_equal(want[1][0], want[3][0], name + ": the flag's background on both kernels")
    black = plain.par_cast(cam, nx, ny, ns, seed=SEED)
    assert not np.array_equal(black, want[3][0])
    other = (0.1, 0.2, 0.3)
    block_frame = plain.par_cast(cam, nx, ny, ns, seed=SEED, background=other)
    for variant in ("constant", "image1x1"):
        b = gpu.builder()
        world, cam_e = _constant_world(pkg, b, name, nx, ny)
        if variant == "constant":
            tex = b.constant(K)
        else:
            tex = b.image(np.array(K, f32).reshape(1, 1, 3), pkg.environment.lat_long_params())
        b.environment(tex, scale=K_SCALE, rotate_y=ROT)
        sc = b.scene(world)
        for k in KERNELS:
            got, counters, took, err = _render_named(sc, cam_e, nx, ny, ns, k, capfd)
            what = "%s, %s environment, kernel %d" % (name, variant, k)
            assert took == ("one-lane" if k == 1 else "full"), (what, took)   # (book-1: off the lean pool, onto the full-feature pool kernel)
            assert_bit_equal(got, want[k][0], what)
            assert counters == want[k][1], (what, counters, want[k][1])
            # with the flag set on the environment scene, the block wins
            assert_bit_equal(sc.par_cast(cam_e, nx, ny, ns, seed=SEED, background=other), block_frame, what + ": the block wins")


# ---- 4. furnace --------------------------------------------------------------------------------------------------------------------
def test_furnace(pkg, gpu, capfd):
    """One Lambertian sphere of albedo a under a constant environment L: every path ends in the environment after k bounces (or is
    cut off after 50 and is black -- no such pixel here), so every pixel is s_k * L with s_k the running product the kernel forms."""
    nx = ny = 32
    a, L = np.array((0.5, 0.75, 0.25), f32), np.array((1.0, 2.0, 4.0), f32)
    b = gpu.builder()
    world = [b.sphere(1.0, b.lambertian(b.constant(a)))]
    b.environment(b.constant(L))
    sc = b.scene(world)
    cam = EC.deep_camera(gpu, nx, ny)
    s_k, allowed = np.ones(3, f32), []
    for _ in range(52):
        allowed.append(bits((np.zeros(3, f32) + (s_k * L).astype(f32)).astype(f32)))
        s_k = (s_k * a).astype(f32)
    allowed = np.stack(allowed)
    for kernel in KERNELS:
        out, _, took, _ = _render_named(sc, cam, nx, ny, 1, kernel, capfd)
        px = bits(out).reshape(-1, 3)
        which = (px[:, None, :] == allowed[None, :, :]).all(axis=2)
        assert which.any(axis=1).all(), "kernel %d: %d pixels are no s_k * L" % (kernel, int((~which.any(axis=1)).sum()))
        assert (out > 0).all()                                                          # no pixel is black
        ks = which.argmax(axis=1)
        assert (ks == 0).any() and (ks == 1).sum() > 50 and (ks <= 1).all()             # misses, and one bounce: a convex body is left at once


# ---- 5. every kernel, the same bits ------------------------------------------------------------------------------------------------
def _image_world(pkg, gpu, name, nx, ny, n_spheres=24):
    """(scene, camera) of world `name` under the 8 x 4 bilinear lat-long image, rotated by 33.3 degrees, scale (1, 0.5, 2)."""
    b = gpu.builder()
    if name == "spheres":
        world, cam = EC.random_spheres(pkg, b, n_spheres), EC.spheres_camera(gpu, nx, ny)
    elif name == "mesh":
        world, cam = EC.open_cornell(pkg, b, nx, ny, mesh=True)
    elif name == "volume":
        world, cam = EC.open_volume(pkg, b, nx, ny)
    else:
        world, cam = EC.deep_world(b), EC.deep_camera(gpu, nx, ny)
    tex, _, _ = EC.lat_long(pkg, b)
    b.environment(tex, scale=SCALE, rotate_y=ROT)
    return b.scene(world), cam, b, world


PRODUCTION = {"spheres": "full", "mesh": "full", "volume": "full", "deep": "one-lane"}


@pytest.mark.parametrize("name", ["spheres", "mesh", "volume", "deep"])
def test_an_image_environment_renders_the_same_bits_on_every_kernel(pkg, gpu, capfd, name):
    nx, ny, ns = 32, 32, 8
    sc, cam, b, world = _image_world(pkg, gpu, name, nx, ny)
    feats = b.flatten(world)[1]
    assert feats & 4096 and feats & 8 and bool(feats & 128) == (name == "deep") and bool(feats & 2048) == (name == "mesh")
    base, c_base, took1, _ = _render_named(sc, cam, nx, ny, ns, 1, capfd)
    prod, c_prod, took3, err = _render_named(sc, cam, nx, ny, ns, 3, capfd)
    assert took1 == "one-lane" and took3 == PRODUCTION[name], (name, took1, took3)     # never the lean pool, never pool-2
    assert "[rtg] environment: texture" in err
    assert_bit_equal(prod, base, name + ": production kernel against one lane per pixel")
    assert c_prod == c_base, (name, c_prod, c_base)
    assert np.isfinite(prod).all() and len(np.unique(bits(prod).reshape(-1, 3), axis=0)) > nx * ny // 4
    if name != "deep":    # both scheduled kernels, whichever the default picked: sync = 0 the full-feature pool kernel, 1 the lock-step kernel
        for sync in (0, 1):
            sc.set_option("sync", sync)
            got, c, took, _ = _render_named(sc, cam, nx, ny, ns, 3, capfd)
            assert took == "full", (sync, took)
            assert_bit_equal(got, base, "%s: sync = %d" % (name, sync))
            assert c == c_base, (name, sync, c, c_base)
        sc.set_option("sync", -1)
    # the environment matters: the same world without it renders another frame
    b.environment(None)
    assert not np.array_equal(b.scene(world).par_cast(cam, nx, ny, ns, seed=SEED), prod)
    # 64 fixed keys of rtg_debug_samples, with and without RTG_FLAG_TRACE_KERNEL
    rs = np.random.RandomState(64)
    xs, ys, ss = rs.randint(0, nx, 64), rs.randint(0, ny, 64), rs.randint(0, ns, 64)
    sc.set_option("kernel", 3)
    one, info = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, seed=SEED)
    if name != "deep":                   # (a FEAT_DEEP world renders on the one-lane kernels: nothing to trace)
        for sync in (0, 1):
            sc.set_option("sync", sync)
            traced, _ = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, seed=SEED, trace_kernel=True)
            assert_bit_equal(traced, one, "%s: RTG_FLAG_TRACE_KERNEL against the one-lane probe, sync = %d" % (name, sync))
        sc.set_option("sync", -1)
    full = sc.debug_samples(cam, nx, ny, ns, *_all_keys(nx, ny, ns), seed=SEED)[0].reshape(ns, ny, nx, 3)
    assert_bit_equal(full[ss, ny - 1 - ys, xs], one, name + ": the keys among all samples")
    assert_bit_equal(_fold(full, ns), prod, name + ": the frame is the fold of rtg_debug_samples")


def test_a_window_sized_program_through_the_pool_kernel_s_window(pkg, gpu, capfd):
    """A few thousand spheres (a lean program without the environment) with a part of the program staged in LDS (option window)
    and with none of it."""
    nx, ny, ns = 16, 16, 2
    sc, cam, _, _ = _image_world(pkg, gpu, "spheres", nx, ny, n_spheres=2000)
    base, c_base, _, _ = _render_named(sc, cam, nx, ny, ns, 1, capfd)
    sc.set_option("sync", 0)
    for window in (-1, 1000, 0):
        sc.set_option("window", window)
        got, c, took, err = _render_named(sc, cam, nx, ny, ns, 3, capfd)
        assert took == "full", (window, took)
        if window == 1000:
            assert "program window: 1000 of" in err
        assert_bit_equal(got, base, "window %d" % window)
        assert c == c_base, (window, c, c_base)


# ---- 6. the frame machinery --------------------------------------------------------------------------------------------------------
def test_the_frame_machinery(pkg, gpu):
    capi = pkg.capi
    nx, ny, ns = 32, 32, 8
    sc, cam, _, _ = _image_world(pkg, gpu, "spheres", nx, ny)
    want = sc.par_cast(cam, nx, ny, ns, seed=SEED)
    # slices of 2
    acc = np.zeros((ny, nx, 3), f32)
    for s0 in range(0, ns, 2):
        sc.par_cast(cam, nx, ny, s0 + 2, seed=SEED, out=acc, sample_begin=s0, resume=True, partial=s0 + 2 < ns)
    assert_bit_equal(acc, want, "slices of 2")
    # plane 0 of a SUM_SQUARES call; a SAMPLE_COUNTS call with n_p = ns
    planes, _ = sc.par_cast(cam, nx, ny, ns, seed=SEED, squares=True, stats=True)
    assert_bit_equal(planes[0], want, "SUM_SQUARES: plane 0")
    counted, _ = sc.par_cast(cam, nx, ny, ns, seed=SEED, counts=np.full((ny, nx), ns, np.uint32), stats=True)
    assert_bit_equal(counted, want, "SAMPLE_COUNTS, n_p = ns")
    # rtg_par_cast_device
    hip = _hip()
    p = capi.make_params(nx, ny, ns, seed=SEED)
    dev = _DeviceBuf(hip, want.nbytes)
    try:
        dev.put(np.zeros(want.size, np.uint32))
        sc.par_cast_device(cam, p, dev.p.value)
        assert hip.hipDeviceSynchronize() == 0
        assert_bit_equal(dev.get().view(f32).reshape(ny, nx, 3), want, "rtg_par_cast_device")
    finally:
        dev.free()
    # rtg_par_cast_multi over two handles on one device
    scenes = [_image_world(pkg, gpu, "spheres", nx, ny)[0] for _ in range(2)]
    scenes[-1].set_option("force_rccl", 1)
    assert_bit_equal(gpu.par_cast_multi(scenes, cam, nx, ny, ns, seed=SEED), want, "rtg_par_cast_multi, two handles")
    # tiles and ranks
    canvas = np.zeros((ny, nx, 3), f32)
    for r in range(2):
        sc.par_cast(cam, nx, ny, ns, seed=SEED, out=canvas, tile_w=8, tile_h=8, rank=r, nranks=2)
    assert_bit_equal(canvas, want, "rank 0 of 2 + rank 1 of 2")
    # the ordered float32 fold of rtg_debug_samples over all keys, at 16 x 16 x 4
    nx, ny, ns = 16, 16, 4
    sc, cam, _, _ = _image_world(pkg, gpu, "spheres", nx, ny)
    rgb, _ = sc.debug_samples(cam, nx, ny, ns, *_all_keys(nx, ny, ns), seed=SEED)
    assert_bit_equal(_fold(rgb.reshape(ns, ny, nx, 3), ns), sc.par_cast(cam, nx, ny, ns, seed=SEED), "the fold of rtg_debug_samples")
    # a ray frame of the camera's own rays is the camera frame
    rays = pkg.rays.camera_rays(cam, nx, ny, ns, SEED)
    assert_bit_equal(sc.cast_rays(rays, nx, ny, ns, per_sample=True, seed=SEED), sc.par_cast(cam, nx, ny, ns, seed=SEED), "ray frame")


# ---- 7. mirror ---------------------------------------------------------------------------------------------------------------------
def test_a_mirror_shows_the_environment(pkg, gpu):
    """One bare Metal sphere, fuzz 0: a ray that hits it leaves along reflect(unit(d), n) (material.rs:66-80; + 0 * a draw) and
    misses everything: the sample is 0 + albedo * E(nd).  (p, n) from a closest-hit query; reflect in float32, the kernel's order."""
    E = pkg.environment
    nx = ny = 16
    albedo = np.array((0.5, 0.75, 1.0), f32)
    b = gpu.builder()
    world = [b.sphere(1.0, b.metal(albedo, 0.0))]
    tex, img, prm = EC.lat_long(pkg, b)
    b.environment(tex, scale=SCALE, rotate_y=ROT)
    e = b.get_environment()
    sc = b.scene(world)
    rs = np.random.RandomState(77)
    o = rs.randn(4 * nx * ny, 3)
    o = (o / np.linalg.norm(o, axis=1, keepdims=True) * rs.uniform(2.5, 6.0, (len(o), 1))).astype(f32)
    target = (rs.rand(len(o), 3) - 0.5).astype(f32) * f32(0.9)                      # inside the sphere: every ray hits
    rays = np.concatenate([o, (target - o) * rs.uniform(0.5, 2.0, (len(o), 1)).astype(f32), rs.rand(len(o), 1).astype(f32)], axis=1).astype(f32)
    out, _ = sc.closest_hit(rays)
    d, n = rays[:, 3:6], out[:, 5:8]
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    v = d / ln[:, None]                                                               # vec3.rs:66
    dot = (v[:, 0] * n[:, 0] + v[:, 1] * n[:, 1]) + v[:, 2] * n[:, 2]
    nd = (v - (f32(2.0) * dot)[:, None] * n).astype(f32)                              # vec3.rs:313
    ndn = (nd[:, 0] * n[:, 0] + nd[:, 1] * n[:, 1]) + nd[:, 2] * n[:, 2]
    ok = (out[:, 0] == 1) & (nd != 0).all(axis=1) & (ndn > 0)
    assert ok.sum() >= nx * ny
    rays, nd = rays[ok][:nx * ny], nd[ok][:nx * ny]
    want = EC.miss_colour(np.zeros(3, f32), albedo, E.colour(nd, img, prm, SCALE, e["s"], e["c"])).reshape(ny, nx, 3)
    for kernel in KERNELS:
        sc.set_option("kernel", kernel)
        assert_bit_equal(sc.cast_rays(rays, nx, ny, 1, seed=SEED), want, "mirror, kernel %d" % kernel)
    # the same bounce in a camera frame on the lock-step kernel: the frame of the camera's rays is the ray frame of them
    cam = EC.deep_camera(gpu, nx, ny)
    crays = pkg.rays.camera_rays(cam, nx, ny, 1, SEED)
    sc.set_option("kernel", 3)
    assert_bit_equal(sc.par_cast(cam, nx, ny, 1, seed=SEED), sc.cast_rays(crays, nx, ny, 1, per_sample=True, seed=SEED), "camera frame")


# ---- 8. light sampling -------------------------------------------------------------------------------------------------------------
def test_light_sampling_books_the_environment_at_full_weight(pkg, gpu):
    S = pkg.scenes
    nx, ny, ns = 16, 16, 4
    b = gpu.builder()
    grey = b.lambertian(b.constant(S.vfrom(0.6)))
    world = [b.rect(S.Y, (-4.0, 4.0), (-4.0, 4.0), 0.0, grey),                                                       # a floor
             b.flip_normals(b.rect(S.Y, (-1.0, 1.0), (-1.0, 1.0), 3.0, b.diffuse_light(b.constant(S.vfrom(1.0)), 8.0))),   # a rect light
             b.translate(S.v(0.0, 0.7, 0.0), b.sphere(0.7, grey))]
    tex, _, _ = EC.lat_long(pkg, b)
    b.environment(tex, scale=SCALE, rotate_y=ROT)
    sc = b.scene(world)
    cam = gpu.camera_look(S.v(0.0, 2.0, 7.0), S.v(0.0, 0.5, 0.0), S.v(0.0, 1.0, 0.0), 45.0, 1.0, 0.0, 7.0)
    plain = sc.par_cast(cam, nx, ny, ns, seed=SEED)
    plain0 = sc.par_cast(cam, nx, ny, ns, seed=SEED, max_bounces=0)
    sc.set_option("light_sampling", 1)
    ls = sc.par_cast(cam, nx, ny, ns, seed=SEED)
    assert not np.array_equal(ls, plain)                                               # another estimator
    rgb, _ = sc.debug_samples(cam, nx, ny, ns, *_all_keys(nx, ny, ns), seed=SEED)
    assert_bit_equal(_fold(rgb.reshape(ns, ny, nx, 3), ns), ls, "light sampling: the frame is the fold of rtg_debug_samples")
    assert_bit_equal(sc.par_cast(cam, nx, ny, ns, seed=SEED, max_bounces=0), plain0, "max_bounces = 0: the plain frame")
    sky = plain0[0]                                                                     # the top row sees the environment alone
    assert (sky != 0).any()
