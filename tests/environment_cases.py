"""The cases the environment tests share (test_environment_abi.py on the host, test_environment_gpu.py on the device): the
directions, images, settings, rotations and scales of the probe comparisons, and the worlds the frames are rendered on.
Everything is deterministic: the host test and the GPU test see the same arrays."""
import numpy as np

f32 = np.float32

N_DIRECTIONS = 4096
SIZES = [(1, 1), (5, 3), (8, 4)]                       # (w, h)
ROTATIONS = [0.0, 90.0, 33.3, -120.0]                  # degrees about world +y
SCALES = [(1.0, 1.0, 1.0), (0.0, 2.5, 1e3), (-1.0, 1.0, 1.0)]
CONSTANT = (0.25, 0.5, 2.0)


def image(size, seed=20261021):
    w, h = size
    return (np.random.RandomState(seed + 17 * w + h).rand(h, w, 3) * 4.0).astype(f32)


def settings(I):
    """A lat-long map (spherical about the origin) under both filters and the four wrap pairs."""
    return [I.spherical((0.0, 0.0, 0.0), filter=flt, wrap_u=wu, wrap_v=wv)
            for flt in (I.NEAREST, I.BILINEAR) for wu in (I.REPEAT, I.CLAMP) for wv in (I.REPEAT, I.CLAMP)]


def name(prm):
    return "filter %d wrap %d%d" % (prm["filter"], prm["wrap_u"], prm["wrap_v"])


def directions():
    """4 096 directions: the six axes, both poles at several lengths, the seam (d.x < 0 with d.z = +0 and -0), denormal
    components, (0, 0, 0), NaN and the infinities, lengths that overflow and underflow the squared norm, and random directions of
    every length."""
    rs = np.random.RandomState(4096)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    poles = np.array([[0, 1e-30, 0], [0, -1e-30, 0], [0, 3e4, 0], [0, -3e4, 0], [1e-30, 1, 0], [0, 1, 1e-30], [-0.0, 1, -0.0], [0, -1, -0.0],
                      [1e-8, 1, 1e-8], [-1e-8, -1, 1e-8]], f32)
    seam = np.array([[-1, 0, 0.0], [-1, 0, -0.0], [-2, 0.5, 0.0], [-2, 0.5, -0.0], [-1, 0, 1e-45], [-1, 0, -1e-45], [-3, -0.25, 1e-30],
                     [-3, -0.25, -1e-30], [-1e-3, 0.7, 0.0], [-1e-3, 0.7, -0.0]], f32)
    den = np.array([[1e-40, 0, 0], [0, 1e-40, 0], [0, 0, -1e-40], [1e-40, 1e-41, -1e-42], [1e-45, 1e-45, 1e-45], [-1e-45, 0, 1e-45], [1e-38, 1e-39, 0],
                    [1, 1e-40, 0], [1e-40, 1, 1e-40], [1e-20, 1e-20, 1e-20], [1e-19, -1e-19, 1e-30]], f32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -2.0], f32)
    special = np.stack(np.meshgrid(sp, sp, sp), axis=-1).reshape(-1, 3).astype(f32)      # 343, (0, 0, 0) among them
    big = np.array([[1e30, 1, 1], [1e19, 1e19, 1e19], [3e38, 3e38, 3e38], [-1e20, 1, 1e20], [1e25, -1e-25, 0]], f32)
    fixed = np.concatenate([axes, poles, seam, den, special, big]).astype(f32)
    n = N_DIRECTIONS - len(fixed)
    unit = rs.randn(n, 3)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    length = np.where(rs.rand(n) < 0.5, 1.0, 10.0 ** rs.uniform(-12, 12, n))
    d = np.concatenate([fixed, (unit * length[:, None]).astype(f32)]).astype(f32)
    assert d.shape == (N_DIRECTIONS, 3)
    return d


def miss_colour(accum, strength, e):
    """accum + strength * E(d), in miss_colour's order (csrc/rt_device.h), float32."""
    with np.errstate(all="ignore"):
        return (np.asarray(accum, f32) + (np.asarray(strength, f32) * np.asarray(e, f32)).astype(f32)).astype(f32)


# ---- worlds --------------------------------------------------------------------------------------------------------------------
def lat_long(pkg, b, img=None, filter=1):
    """The 8 x 4 lat-long image of the frame tests as a texture of `b`: (texture, image, parameters)."""
    I = pkg.image
    img = image((8, 4)) if img is None else img
    prm = I.spherical((0.0, 0.0, 0.0), filter=filter, wrap_u=I.REPEAT, wrap_v=I.CLAMP)
    return b.image(img, prm), img, prm


def far_sphere_world(b):
    """One sphere of radius 0.01 at (0, -1000, 0): every ray the tests send misses it."""
    S_v = np.array([0.0, -1000.0, 0.0], f32)
    return [b.translate(S_v, b.sphere(0.01, b.lambertian(b.constant((0.5, 0.5, 0.5)))))]


def miss_rays(n=256, seed=5):
    """n rays from near the origin, none of which comes near (0, -1000, 0): directions with d.y >= -0.5 |d|."""
    rs = np.random.RandomState(seed)
    d = rs.randn(4 * n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d[d[:, 1] > -0.5][:n] * (10.0 ** rs.uniform(-2, 2, (n, 1)))
    o = rs.rand(n, 3) - 0.5
    return np.concatenate([o, d, rs.rand(n, 1)], axis=1).astype(f32)


def random_spheres(pkg, b, n=24, seed=7, bvh=True):
    """n random spheres (Lambertian, metal, glass) over a ground sphere, under a Bvh: a lean program until it gets an environment."""
    S = pkg.scenes
    rng = pkg.small_rng.SmallRng(seed)
    objs = [b.translate(S.v(0.0, -1000.0, 0.0), b.sphere(1000.0, b.lambertian(b.constant(S.vfrom(0.5)))))]
    for i in range(n):
        c = S.v(f32(8.0) * rng.gen_f32() - f32(4.0), f32(0.2) + f32(0.8) * rng.gen_f32(), f32(8.0) * rng.gen_f32() - f32(4.0))
        pick = rng.gen_f32()
        if pick < f32(0.5):
            mat = b.lambertian(b.constant(rng.gen_vec3() * rng.gen_vec3()))
        elif pick < f32(0.8):
            mat = b.metal(f32(0.5) * (f32(1.0) + rng.gen_vec3()), float(f32(0.5) * rng.gen_f32()))
        else:
            mat = b.dielectric(1.5)
        objs.append(b.translate(c, b.sphere(float(f32(0.2) + f32(0.3) * rng.gen_f32()), mat)))
    world = [b.bvh(objs, (0.0, 1.0))] if bvh else objs
    return world


def spheres_camera(be, nx, ny):
    S_v = lambda *a: np.array(a, f32)   # noqa: E731
    return be.camera_look(S_v(9.0, 2.5, 6.0), S_v(0.0, 0.5, 0.0), S_v(0.0, 1.0, 0.0), 35.0, float(f32(nx) / f32(ny)), 0.0, 10.0, (0.0, 1.0))


def open_cornell(pkg, b, nx, ny, mesh=False):
    """The Cornell box without its rear wall and ceiling, so that paths leave it; mesh=True: with a 320-triangle icosphere with
    per-vertex normals in place of the boxes.  The reference's camera looks in through the open front."""
    S, T = pkg.scenes, pkg.triangle
    cam, _ = S._cornell_camera(b.be, nx, ny)
    world = S.cornell_box(b)
    world = [world[0], world[1], world[4], world[5]]          # light, floor, right and left walls
    white = b.lambertian(b.constant(S.vfrom(0.73)))
    if mesh:
        vs, fs = T.icosphere(2, radius=120.0, centre=(278.0, 120.0, 278.0))
        assert len(fs) == 320
        normals = ((vs - np.array([278.0, 120.0, 278.0])) / 120.0).astype(f32)
        world.append(b.mesh(vs, fs, white, normals=normals))
    else:
        world.append(b.translate(S.v(130.0, 0.0, 65.0), b.rotate_y(-18.0, b.rect_prism(S.v(0, 0, 0), S.v(165.0, 165.0, 165.0), white))))
    return world, cam


def open_volume(pkg, b, nx, ny):
    """volume_test's media world (main.rs) without its ceiling."""
    S = pkg.scenes
    world, cam, _ = S.volume_test(b, nx, ny)
    del world[3]   # cornell_box: light, floor, rear wall, CEILING, right wall, left wall; then the medium
    return world, cam


def deep_world(b):
    """A FEAT_DEEP world: a sphere under five Translates by zero (five nested wrappers: one more than the scheduled kernels' ray
    stack holds), on a ground.  The flattener fuses the innermost Translate{Sphere} into one SPHERE record, so the sphere gets
    that one first and the five wrappers around it."""
    z = np.zeros(3, f32)
    o = b.translate(z, b.sphere(1.0, b.lambertian(b.constant((0.8, 0.3, 0.3)))))
    for _ in range(5):
        o = b.translate(z, o)
    ground = b.translate(np.array([0.0, -101.0, 0.0], f32), b.sphere(100.0, b.lambertian(b.constant((0.5, 0.5, 0.5)))))
    return [o, ground]


def deep_camera(be, nx, ny):
    a = lambda *x: np.array(x, f32)   # noqa: E731
    return be.camera_look(a(0.0, 1.0, 5.0), a(0.0, 0.0, 0.0), a(0.0, 1.0, 0.0), 40.0, float(f32(nx) / f32(ny)), 0.0, 5.0, (0.0, 1.0))
