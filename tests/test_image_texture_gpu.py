"""Image textures on the GPU (include/rtiow_gpu_image.h): the device probe against the numpy definition on the cases of the host
test; a constant image is the constant, bit for bit and counter for counter, on every kernel; a real image renders the same
bits on every kernel, equals the fold of its samples and shows in the albedo plane; an emitting image; multi-handle frames and
ray frames."""

import numpy as np
import pytest

import feature_ref as FR
import image_cases as IC
import physics_ref as PR
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

SEED = 0xDEADBEEF
COUNTERS = ("samples", "aabb_tests", "prim_tests", "shaded_hits", "rays", "draws")
f32 = np.float32


class Swap:
    """A Builder whose constant(colour) makes something else where the colour is `match`; every other call goes to the Builder
    as it is.  `made` lists the handles it gave out for the match."""

    def __init__(self, builder, match, make=None):
        self._b, self.match, self.make, self.made = builder, np.asarray(match, f32), make, []

    def __getattr__(self, name):
        return getattr(self._b, name)

    def constant(self, color):
        c = np.array([color[0], color[1], color[2]], f32)
        if (c == self.match).all():
            t = self.make(self._b, c) if self.make else self._b.constant(color)
            self.made.append(t)
            return t
        return self._b.constant(color)


def _scene_fn(pkg, name):
    S = pkg.scenes
    return {"cornell": lambda b, nx, ny: S.cornell_box_scene(b, nx, ny),
            "book1": lambda b, nx, ny: S.random_scene(b, nx, ny),
            "book2": lambda b, nx, ny: S.book_final_scene(b, nx, ny, pkg.small_rng.SmallRng(SEED))}[name]


WHITE, GROUND1, GROUND2, BROWN = (0.73, 0.73, 0.73), (0.5, 0.5, 0.5), (0.48, 0.83, 0.53), (0.4, 0.2, 0.1)


KERNELS = (1, 3)   # scene option "kernel": 1 = one lane per pixel, 3 = the production kernels (the default).  The option stays
#                    set on a handle, so every render names it.


def _render(sc, cam, nx, ny, ns, kernel):
    sc.set_option("kernel", kernel)
    out, st = sc.par_cast(cam, nx, ny, ns, seed=SEED, stats=True)
    return out, {k: st[k] for k in COUNTERS}


def _render_named(sc, cam, nx, ny, ns, kernel, capfd):
    """_render, and which kernel option verbose says the frame took: "lean" (the lean pool kernel), "full" (a full-feature
    schedule: the full-feature pool kernel, the pool-2 kernel or the lock-step kernel) or "one-lane" (neither line)."""
    sc.set_option("verbose", 1)
    capfd.readouterr()
    try:
        out, counters = _render(sc, cam, nx, ny, ns, kernel)
    finally:
        sc.set_option("verbose", 0)
    err = capfd.readouterr().err
    took = "full" if "[rtg] full pool" in err else "lean" if "[rtg] pool: samples [" in err else "one-lane"
    return out, counters, took


# ---- 1. the probes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", IC.SIZES, ids=lambda s: "%dx%d" % s)
def test_the_device_probe_equals_the_numpy_definition(pkg, gpu, size):
    I = pkg.image
    b = gpu.builder()
    img = IC.image(size)
    cases = [(prm, b.image(img, prm)) for prm in IC.settings(I, size)]
    sc = b.scene([b.sphere(1.0, b.lambertian(cases[0][1]))])
    for prm, t in cases:
        p = IC.points(I, prm, size)
        assert_bit_equal(sc.debug_texture(t, p), I.sample(img, prm, p), IC.name(prm))
        assert_bit_equal(sc.debug_texture(t, p[:300]), b.texture_host(t, p[:300]), IC.name(prm) + ": device against host")
    info = sc.info()
    assert info["textures"] == 2 * len(cases)                         # records, not texels
    assert info["hbm_bytes"] >= 16 * len(cases) * size[0] * size[1]   # ... which the bytes include
    with pytest.raises(pkg.capi.RtError):
        sc.debug_texture(cases[0][1] + 1, np.zeros((1, 3), f32))     # the record of the mapping floats is no texture
    with pytest.raises(pkg.capi.RtError):
        sc.debug_texture(10 ** 6, np.zeros((1, 3), f32))


def test_checker_perlin_and_constant_through_the_device_probe(pkg, gpu, oracle):
    """A checker of two images picks its child by the pinned sine, at every point, the child being image.sample;
    physics_ref.texture_value (float64 sines) agrees wherever the product of sines is not within 1e-6 of zero; a Perlin
    texture is the oracle's turbulence; a constant is itself."""
    I = pkg.image
    rs = np.random.RandomState(4)
    b = gpu.builder()
    b.set_perlin_tables(*pkg.scenes.perlin_tables(SEED))
    a0, a1 = IC.image((5, 4)), IC.image((2, 3))
    p0 = I.planar((0.3, 0.1, -0.2), 0.25, (0.05, -0.4, 0.7), -0.5, filter=I.BILINEAR)
    p1 = I.spherical(IC.CENTRE, filter=I.NEAREST, wrap_v=I.CLAMP)
    t0, t1 = b.image(a0, p0), b.image(a1, p1)
    chk, per, con = b.checker(t0, t1), b.perlin(0.7), b.constant((0.1, 0.2, 0.3))
    nested = b.checker(con, chk)
    sc = b.scene([b.sphere(1.0, b.lambertian(nested))])
    p = ((rs.rand(2000, 3) - 0.5) * 6).astype(f32)

    class Rec:
        textures = {0: ("constant", np.zeros(3)), 1: ("constant", np.ones(3)), 2: ("checker", 0, 1), 3: ("constant", np.full(3, 2.0)),
                    4: ("checker", 3, 2)}
    # the child at EVERY point: the pick made with the oracle's pinned sine (feature_ref.eval_texture), which is the device's
    pick = FR.eval_texture(oracle, Rec, 2, p)
    want = np.where(pick[:, :1] == 1, I.sample(a1, p1, p), I.sample(a0, p0, p))
    assert_bit_equal(sc.debug_texture(chk, p), want, "checker of two images")
    pick4 = FR.eval_texture(oracle, Rec, 4, p)
    want4 = np.where(pick4[:, :1] == 2, f32([0.1, 0.2, 0.3]), want)
    assert_bit_equal(sc.debug_texture(nested, p), want4, "checker of a constant and a checker of two images")
    # ... and physics_ref's float64 evaluator makes the same picks wherever its sines are clear of zero
    for tex, mine in ((2, pick), (4, pick4)):
        ref, eps = PR.texture_value(Rec, tex, p.astype(np.float64))
        sure = eps > 1e-6
        assert sure.sum() > 1900 and (ref[sure] == mine[sure]).all()
    assert_bit_equal(sc.debug_texture(con, p), np.broadcast_to(f32([0.1, 0.2, 0.3]), p.shape), "constant")
    ob = oracle.builder()
    ob.set_perlin_tables(*pkg.scenes.perlin_tables(SEED))
    q = p[:200]
    turb = FR._perlin_turb(oracle, ob, (f32(0.7) * q).astype(f32))
    assert_bit_equal(sc.debug_texture(per, q), np.repeat(turb[:, None], 3, axis=1), "perlin")


def test_atan2f_on_the_device_equals_the_definition(pkg, gpu):
    y, x = IC.atan2_pairs(1 << 16)
    assert_bit_equal(gpu.debug_math(6, y, x), pkg.image.atan2f(y, x), "rtg_debug_math op 6")
    assert_bit_equal(gpu.debug_math(6, y, x), gpu.atan2f_host(y, x), "device against host")


# ---- 2. a constant image is the constant ---------------------------------------------------------------------------------------
CONSTANT_CASES = [("cornell", 32, 32, 8, WHITE), ("book1", 48, 32, 8, GROUND1), ("book2", 32, 32, 8, GROUND2)]


@pytest.mark.parametrize("name,nx,ny,ns,colour", CONSTANT_CASES, ids=[c[0] for c in CONSTANT_CASES])
def test_a_constant_image_is_the_constant(pkg, gpu, capfd, name, nx, ny, ns, colour):
    """The frame and every counter: the world with constant(c) against the world with a 1 x 1 or a 4 x 4 image of c in its
    place, both filters, a planar and a spherical mapping, under scene option kernel = 1 (one lane per pixel) and kernel = 3 (the
    default: the production kernels; option verbose tells which kind ran).  Cornell is a list world on the lock-step kernel;
    book-1 moves from the lean pool to the full-feature pool: another kernel, the same bits and counters; book-2 runs on a
    full-feature pool kernel with a Perlin sphere, media and a light beside the image."""
    I = pkg.image
    fn = _scene_fn(pkg, name)
    b = gpu.builder()
    world, cam, _ = fn(b, nx, ny)
    plain = b.scene(world)
    want = {k: _render_named(plain, cam, nx, ny, ns, k, capfd) for k in KERNELS}
    assert (want[1][2], want[3][2]) == ("one-lane", "lean" if name == "book1" else "full"), (name, want[1][2], want[3][2])
    assert_bit_equal(want[1][0], want[3][0], name + ": the constant world on both kernels")
    variants = [(1, 1, I.planar((0.01, 0, 0), 0.0, (0, 0, 0.01), 0.0, filter=I.NEAREST)),
                (1, 1, I.spherical((0.0, 1.0, 0.0), filter=I.BILINEAR)),
                (4, 4, I.planar((0.013, 0.002, 0), 0.3, (0, 0.001, 0.017), 0.1, filter=I.BILINEAR, wrap_u=I.CLAMP)),
                (4, 4, I.spherical((100.0, 50.0, -20.0), filter=I.NEAREST, wrap_v=I.CLAMP))]
    for w, h, prm in variants:
        sb = Swap(gpu.builder(), colour, lambda bb, c: bb.image(np.broadcast_to(c, (h, w, 3)).copy(), prm))
        world, cam_i, _ = fn(sb, nx, ny)
        assert len(sb.made) >= 1   # (the Cornell scene makes its white twice: the walls' and the boxes')
        sc = sb.scene(world)
        assert sc.info()["textures"] == plain.info()["textures"] + len(sb.made)
        for k in KERNELS:
            got, counters, took = _render_named(sc, cam_i, nx, ny, ns, k, capfd)
            assert took == ("one-lane" if k == 1 else "full"), (name, k, took)   # (book-1 with an image: off the lean pool)
            what = "%s: %d x %d image, %s, kernel %d" % (name, w, h, IC.name(prm), k)
            assert_bit_equal(got, want[k][0], what)
            assert counters == want[k][1], (what, counters, want[k][1])


# ---- 3. a real image -----------------------------------------------------------------------------------------------------------
def _real_image():
    return np.random.RandomState(16 * 8).rand(8, 16, 3).astype(f32)


def _cornell_floor(pkg, b, nx, ny, texture):
    """The Cornell box with a floor material of its own (the last material of the builder)."""
    S = pkg.scenes
    world, cam, exp = S.cornell_box_scene(b, nx, ny)
    world[1] = b.rect(S.Y, (0.0, 555.0), (0.0, 555.0), 0.0, b.lambertian(texture(b)))
    return world, cam, exp


FLOOR_PRM = dict(u_axis=(1.0 / 555.0, 0, 0), u_offset=0.0, v_axis=(0, 0, 1.0 / 555.0), v_offset=0.0)


def _real_scene(pkg, backend, name, nx, ny, image=True):
    """(scene, camera, the image's parameters, the material that carries it): the 16 x 8 image, bilinear, planar on the Cornell
    floor or spherical on book-1's brown sphere; image=False: a constant in its place (the oracle's copy: same ids)."""
    I = pkg.image
    img = _real_image()
    if name == "cornell":
        prm = I.planar(FLOOR_PRM["u_axis"], 0.0, FLOOR_PRM["v_axis"], 0.0, filter=I.BILINEAR)
        rb = FR.RecordingBuilder(backend.builder())
        made = []
        tex = (lambda bb: bb.image(img, prm)) if image else (lambda bb: bb.constant((0.5, 0.5, 0.5)))
        world, cam, _ = _cornell_floor(pkg, rb, nx, ny, lambda bb: made.append(tex(bb)) or made[-1])
        mat = [m for m, rec in rb.materials.items() if rec[0] == "texture" and rec[1] == made[0]]
        assert len(mat) == 1
        return rb.scene(world), cam, prm, mat[0], rb
    prm = I.spherical((-4.0, 1.0, 0.0), filter=I.BILINEAR)
    sb = Swap(backend.builder(), BROWN, (lambda bb, c: bb.image(img, prm)) if image else None)
    rb = FR.RecordingBuilder(sb)
    world, cam, _ = pkg.scenes.random_scene(rb, nx, ny)
    mat = [m for m, rec in rb.materials.items() if rec[0] == "texture" and rec[1] == sb.made[0]]
    assert len(mat) == 1
    return rb.scene(world), cam, prm, mat[0], rb


def _fold(samples, ns):
    """[ns, ...] per-sample colours -> the left fold from +0, divided by float32(ns) (lib.rs:365-374)."""
    acc = np.zeros(samples.shape[1:], f32)
    for s in range(ns):
        acc = (acc + samples[s]).astype(f32)
    return (acc / f32(ns)).astype(f32)


@pytest.mark.parametrize("name,nx,ny,ns", [("cornell", 32, 32, 8), ("book1", 48, 32, 8)])
def test_a_real_image_renders_the_same_bits_on_every_kernel(pkg, gpu, name, nx, ny, ns):
    sc, cam, prm, mat, _ = _real_scene(pkg, gpu, name, nx, ny)
    base, c_base = _render(sc, cam, nx, ny, ns, 1)
    prod, c_prod = _render(sc, cam, nx, ny, ns, 3)
    assert_bit_equal(prod, base, name + ": production kernel against one lane per pixel")
    assert np.isfinite(prod).all() and prod.max() > 0
    # the frame is the left fold of the per-sample colours of the one-lane probe
    s_i, row_i, x_i = np.meshgrid(np.arange(ns), np.arange(ny), np.arange(nx), indexing="ij")
    rgb, _ = sc.debug_samples(cam, nx, ny, ns, x_i.ravel(), (ny - 1 - row_i).ravel(), s_i.ravel(), seed=SEED)
    assert_bit_equal(_fold(rgb.reshape(ns, ny, nx, 3), ns), prod, name + ": the fold of rtg_debug_samples")
    # the production kernel's own samples at 64 fixed keys
    rs = np.random.RandomState(64)
    xs, ys, ss = rs.randint(0, nx, 64), rs.randint(0, ny, 64), rs.randint(0, ns, 64)
    one, _ = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, seed=SEED)
    traced, _ = sc.debug_samples(cam, nx, ny, ns, xs, ys, ss, seed=SEED, trace_kernel=True)
    assert_bit_equal(traced, one, name + ": RTG_FLAG_TRACE_KERNEL against the one-lane probe")
    # the image matters: the world with a constant in its place renders another frame
    other, cam_o, _, _, _ = _real_scene(pkg, gpu, name, nx, ny, image=False)
    assert not np.array_equal(other.par_cast(cam_o, nx, ny, ns, seed=SEED), prod)


@pytest.mark.parametrize("name,nx,ny", [("cornell", 32, 32), ("book1", 48, 32)])
def test_the_albedo_plane_shows_the_image(pkg, gpu, oracle, name, nx, ny):
    """RTG_FLAG_FEATURES, grid 1 and 2: the albedo plane is the fold of image.sample at the oracle's first-hit points (the
    oracle's copy of the world holds a constant in the image's place: same geometry, same material ids)."""
    I = pkg.image
    img = _real_image()
    sc, cam, prm, mat, _ = _real_scene(pkg, gpu, name, nx, ny)
    so, cam_o, _, mat_o, rb = _real_scene(pkg, oracle, name, nx, ny, image=False)
    assert mat_o == mat
    for grid in (1, 2):
        rays = pkg.features.subpixel_rays(cam_o, nx, ny, grid)
        g2, n = grid * grid, nx * ny
        vals, hits = np.zeros((g2, ny, nx, 3), f32), np.zeros((g2, ny, nx), bool)
        on_image = 0
        for k in range(g2):
            by_pixel = rays[k][::-1].reshape(n, 7)   # ascending y, then x: the key of the oracle's probe
            out, m = so.debug_hit_top(by_pixel, seed=SEED, t_near=0.001)
            hit = out[:, 0] != 0
            v = np.zeros((n, 3), f32)
            at = hit & (m == mat)
            v[at] = I.sample(img, prm, out[at, 2:5])
            rest = hit & ~at
            v[rest] = FR.albedo_of(oracle, rb, m[rest], out[rest, 2:5])
            on_image += int(at.sum())
            vals[k], hits[k] = v.reshape(ny, nx, 3)[::-1], hit.reshape(ny, nx)[::-1]
            image_px = at.reshape(ny, nx)[::-1] if k == 0 else image_px | at.reshape(ny, nx)[::-1]
        assert on_image > g2 * n // 50, (name, on_image)
        want = pkg.features.fold(vals, hits)
        f = pkg.capi.features_frame(nx, ny, features={"grid": grid})
        sc.par_cast(cam, nx, ny, 2, seed=SEED, out=f, features=True)
        assert image_px.sum() > n // 50
        assert_bit_equal(f.albedo, want, "%s grid %d: albedo plane" % (name, grid))
        assert (f.features.traced, f.features.missed) == (n, int((~hits.any(axis=0)).sum()))


# ---- 4. an emitting image ------------------------------------------------------------------------------------------------------
def test_an_emitting_image(pkg, gpu, oracle):
    I = pkg.image
    S = pkg.scenes
    nx, ny, ns, brightness = 16, 16, 4, 2.5
    img = np.random.RandomState(8 * 8).rand(8, 8, 3).astype(f32)
    prm = I.planar((0.5, 0, 0), 0.5, (0, 0.5, 0), 0.5, filter=I.BILINEAR, wrap_u=I.CLAMP, wrap_v=I.CLAMP)

    def build(be, texture):
        b = be.builder()
        world = [b.rect(S.Z, (-1.0, 1.0), (-1.0, 1.0), 0.0, b.diffuse_light(texture(b), brightness))]
        cam = be.camera_look(S.v(0.3, 0.2, 4.0), S.v(0.0, 0.0, 0.0), S.v(0.0, 1.0, 0.0), 35.0, 1.0, 0.0, 4.0)
        return b.scene(world), cam
    sc, cam = build(gpu, lambda b: b.image(img, prm))
    so, cam_o = build(oracle, lambda b: b.constant((1.0, 1.0, 1.0)))
    rays = pkg.rays.camera_rays(cam, nx, ny, ns, SEED)           # sample s of pixel p = row * nx + x at s * nx * ny + p
    out, _ = so.debug_hit_top(rays, seed=SEED, t_near=0.001)
    hit = out[:, 0] != 0
    assert 0.2 < hit.mean() < 0.98                                # the rect does not fill the frame: some samples miss
    want = np.zeros((len(rays), 3), f32)
    want[hit] = (f32(brightness) * I.sample(img, prm, out[hit, 2:5])).astype(f32)
    s_i, row_i, x_i = np.meshgrid(np.arange(ns), np.arange(ny), np.arange(nx), indexing="ij")
    rgb, info = sc.debug_samples(cam, nx, ny, ns, x_i.ravel(), (ny - 1 - row_i).ravel(), s_i.ravel(), seed=SEED, max_bounces=0)
    assert_bit_equal(rgb, want, "every sample is brightness * image.sample(p)")
    frame = _fold(want.reshape(ns, ny, nx, 3), ns)
    for k in (1, 3):
        sc.set_option("kernel", k)
        assert_bit_equal(sc.par_cast(cam, nx, ny, ns, seed=SEED, max_bounces=0), frame, "the frame is their fold, kernel %d" % k)
    assert len(np.unique(frame.reshape(-1, 3), axis=0)) > nx * ny // 4   # a pattern, not a colour


# ---- 5. multi-handle frames and ray frames -------------------------------------------------------------------------------------
def test_two_handles_give_the_one_handle_frame(pkg, gpu):
    nx, ny, ns = 48, 32, 4
    one, cam, _, _, _ = _real_scene(pkg, gpu, "book1", nx, ny)
    want = one.par_cast(cam, nx, ny, ns, seed=SEED)
    scenes = []
    for _ in range(2):
        sc, cam, _, _, _ = _real_scene(pkg, gpu, "book1", nx, ny)
        sc.set_option("force_rccl", 1)
        scenes.append(sc)
    assert_bit_equal(gpu.par_cast_multi(scenes, cam, nx, ny, ns, seed=SEED), want, "rtg_par_cast_multi, two handles on one device")


@pytest.mark.parametrize("name,nx,ny,ns", [("cornell", 24, 24, 4), ("book1", 48, 32, 4)])
def test_a_ray_frame_of_the_camera_s_rays_gives_the_camera_frame(pkg, gpu, name, nx, ny, ns):
    sc, cam, _, _, _ = _real_scene(pkg, gpu, name, nx, ny)
    want = sc.par_cast(cam, nx, ny, ns, seed=SEED)
    rays = pkg.rays.camera_rays(cam, nx, ny, ns, SEED)
    assert_bit_equal(sc.cast_rays(rays, nx, ny, ns, per_sample=True, seed=SEED), want, name + ": ray frame")
