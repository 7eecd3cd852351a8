"""Float64 statements about scene option light_sampling (include/rtiow_gpu.h, at rtg_scene_set_option), for
test_light_sampling_abi.py and test_light_sampling_gpu.py.  Nothing here is computed by the library: the inputs are a
physics_ref.Recorder's description of a world and the frames the tests render.

A. light_table: which rects the option samples.  A DiffuseLight material is sampled when every primitive of the world's graph
   that uses it is a Rect at the world's list level, bare or under any number of FlipNormals; the table is the rects of the
   sampled materials in world order (rects with an empty range left out: nothing ever hits them).
B. lobe / direct: the direct light of one rect at a surface point, by a midpoint rule over the rect -- the density of the
   reference's Lambertian, which scatters towards p + n + (a point of the unit BALL), along w is the ball's share of the ray:
   (r_hi^3 - r_lo^3) / (4 pi) with r = b -+ sqrt(b^2 - (n.n - 1)), b = n.w / |w|; for |n| = 1 that is 2 cos^3 / pi.
   `variant=` plants a wrong estimator: "cosine" (the cos / pi lobe), "no_cos_l", "no_area" (the sum without the area factor).
C. the statistics of frames rendered with RTG_FLAG_SUM_SQUARES: the variance of every pixel mean, and z scores between frames."""
import numpy as np

F = np.float64
MAX_LIGHTS = 64
VARIANTS = ("cosine", "no_cos_l", "no_area")


# ---------------------------------------------------------------------------------------------------------------------------
# A. the light table
# ---------------------------------------------------------------------------------------------------------------------------
def _materials_below(rec, o, into):
    """Every material a primitive at or below object `o` uses (a medium's phase material included)."""
    r = rec.objects[o]
    k = r[0]
    if k == "sphere":
        into.add(r[2])
    elif k == "rect":
        into.add(r[5])
    elif k == "prism":
        into.add(r[3])
    elif k == "flip":
        _materials_below(rec, r[1], into)
    elif k in ("translate", "scale", "rotate", "move"):
        _materials_below(rec, r[2], into)
    elif k == "and":
        _materials_below(rec, r[1], into)
        _materials_below(rec, r[2], into)
    elif k == "bvh":
        for c in r[1]:
            _materials_below(rec, c, into)
    elif k == "medium":
        into.add(r[3])
        _materials_below(rec, r[1], into)
    else:
        raise ValueError(k)


def light_table(rec, world):
    """The light table of the recorded world: a list of (axis, range0, range1, k, material) in world order."""
    at_list_level, elsewhere = [], set()
    for o in world:
        inner = o
        while rec.objects[inner][0] == "flip":
            inner = rec.objects[inner][1]
        r = rec.objects[inner]
        if r[0] == "rect":
            at_list_level.append(r)
        else:
            _materials_below(rec, o, elsewhere)
    table = []
    for r in at_list_level:
        axis, r0, r1, k, m = r[1], r[2], r[3], r[4], r[5]
        if rec.materials[m][0] == "light" and m not in elsewhere and r0[0] < r0[1] and r1[0] < r1[1]:
            table.append((axis, r0, r1, k, m))
    return table


def area(entry):
    return float((entry[1][1] - entry[1][0]) * (entry[2][1] - entry[2][0]))


# ---------------------------------------------------------------------------------------------------------------------------
# B. direct light by quadrature
# ---------------------------------------------------------------------------------------------------------------------------
def lobe(n, w):
    """Density (per steradian) of the direction of n + (uniform point of the unit ball) along the unit vectors w [..., 3]."""
    n = np.asarray(n, F)
    b = w @ n
    disc = b * b - (n @ n - 1.0)
    sq = np.sqrt(np.maximum(disc, 0.0))
    r_hi, r_lo = b + sq, np.maximum(b - sq, 0.0)
    out = (r_hi ** 3 - r_lo ** 3) / (4.0 * np.pi)
    return np.where((disc > 0.0) & (r_hi > 0.0), out, 0.0)


def direct_all(p, n, axis, r0, r1, k, m=400):
    """Integral over the rect of lobe * cos_l / r2 dA at the point p with normal n -- the factor of albedo * Le in the radiance a
    Lambertian surface scatters from that light, unoccluded -- by an m x m midpoint rule: {None: the integral, variant: what
    that planted estimator would converge to}."""
    o1, o2 = [a for a in range(3) if a != axis]
    u = r0[0] + (np.arange(m, dtype=F) + 0.5) * (r0[1] - r0[0]) / m
    v = r1[0] + (np.arange(m, dtype=F) + 0.5) * (r1[1] - r1[0]) / m
    q = np.empty((m, m, 3), F)
    q[..., o1], q[..., o2], q[..., axis] = u[:, None], v[None, :], k
    w = q - np.asarray(p, F)
    r2 = (w * w).sum(-1)
    wu = w / np.sqrt(r2)[..., None]
    cos_l = np.abs(wu[..., axis])
    dens = lobe(n, wu)
    a = float((r0[1] - r0[0]) * (r1[1] - r1[0]))
    exact = (dens * cos_l / r2).mean()
    return {None: exact * a,
            "cosine": (np.maximum(wu @ np.asarray(n, F), 0.0) / np.pi * cos_l / r2).mean() * a,
            "no_cos_l": (dens / r2).mean() * a,
            "no_area": exact}


def direct(p, n, axis, r0, r1, k, m=400, variant=None):
    return direct_all(p, n, axis, r0, r1, k, m)[variant]


# ---------------------------------------------------------------------------------------------------------------------------
# C. statistics of two-plane frames
# ---------------------------------------------------------------------------------------------------------------------------
def mean_and_variance(planes, ns):
    """planes [2, ny, nx, 3] of a divided RTG_FLAG_SUM_SQUARES frame of ns samples: (pixel means, variances of those means),
    float64 -- the unbiased sample variance over ns."""
    mean = np.asarray(planes[0], F)
    q = np.asarray(planes[1], F)
    var = np.maximum(q - ns * mean * mean, 0.0) / (ns * (ns - 1.0))
    return mean, var


def block_z(a, ns_a, b, ns_b, block=8):
    """z scores between two frames over block x block pixel blocks and channels, and over the whole frame per channel:
    (mean_a - mean_b) / sqrt(var_a + var_b), a mean's variance the sum of its pixels' divided by their number squared."""
    ma, va = mean_and_variance(a, ns_a)
    mb, vb = mean_and_variance(b, ns_b)
    ny, nx, _ = ma.shape
    assert ny % block == 0 and nx % block == 0

    def blocks(x):
        return x.reshape(ny // block, block, nx // block, block, 3).sum(axis=(1, 3))

    def z(diff, var):   # (a block both frames leave black: 0; a difference without any variance: infinite)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(var > 0.0, diff / np.sqrt(var), np.where(diff == 0.0, 0.0, np.inf))
    zb = z(blocks(ma) - blocks(mb), blocks(va) + blocks(vb))   # (the 1 / n of the means and the 1 / n^2 of the variances cancel)
    zf = z(ma.sum((0, 1)) - mb.sum((0, 1)), va.sum((0, 1)) + vb.sum((0, 1)))
    return zb, zf


# ---------------------------------------------------------------------------------------------------------------------------
# the worlds of the tests: name -> (builder of (world, camera) over a Recorder `b`, expected table length)
# ---------------------------------------------------------------------------------------------------------------------------
def _small(pkg, b, lights):
    """A floor under `lights(b, light material)`, seen from the side."""
    S = pkg.scenes
    floor = b.rect(S.Y, (-4.0, 4.0), (-4.0, 4.0), 0.0, b.lambertian(b.constant(S.vfrom(0.5))))
    world = [floor] + lights(b, b.diffuse_light(b.constant(S.v(4.0, 2.0, 1.0)), 1.0))
    cam = b.be.camera_look(S.v(3.0, 1.2, 3.0), S.v(0.0, 0.0, 0.0), S.v(0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0)
    return world, cam


def _rect_light(pkg, b, m):
    return b.rect(pkg.scenes.Y, (-1.0, 1.0), (-0.5, 0.5), 2.0, m)


def _occluded_world(pkg, b, wrappers):
    S = pkg.scenes

    def objects(b, m):
        ball = b.translate(S.v(0.3, 0.6, 0.2), b.sphere(0.5, b.lambertian(b.constant(S.v(0.7, 0.6, 0.5)))))
        for _ in range(wrappers):
            ball = b.translate(S.v(0.0, 0.0, 0.0), ball)
        fog = b.constant_medium(b.sphere(3.0, b.dielectric(1.5)), 0.2, b.isotropic(b.constant(S.vfrom(0.8))))
        return [_rect_light(pkg, b, m), ball, fog]
    return _small(pkg, b, objects)


def quadrature_world(pkg, b):
    """The world of the quadrature test: floor rect(Y, (-4, 4), (-4, 4), 0), Lambertian 0.5; light rect(Y, (-1, 1),
    (-0.5, 0.5), 2) emitting (4, 2, 1); camera (3, 1.2, 3) -> (0, 0, 0), fov 10, aspect 1, aperture 0."""
    S = pkg.scenes
    world, _ = _small(pkg, b, lambda b, m: [_rect_light(pkg, b, m)])
    cam = b.be.camera_look(S.v(3.0, 1.2, 3.0), S.v(0.0, 0.0, 0.0), S.v(0.0, 1.0, 0.0), 10.0, 1.0, 0.0, 10.0)
    return world, cam


WORLDS = {
    "cornell": (lambda pkg, b: pkg.scenes.cornell_box_scene(b, 48, 48)[:2], 1),
    "book2": (lambda pkg, b: pkg.scenes.book_final_scene(b, 48, 48, pkg.small_rng.SmallRng(0xDEADBEEF))[:2], 1),
    "book1": (lambda pkg, b: pkg.scenes.random_scene(b, 48, 32)[:2], 0),
    "volume": (lambda pkg, b: pkg.scenes.volume_test(b, 48, 48)[:2], 1),
    "flipped": (lambda pkg, b: _small(pkg, b, lambda b, m: [b.flip_normals(b.flip_normals(b.flip_normals(_rect_light(pkg, b, m))))]), 1),
    "shared": (lambda pkg, b: _small(pkg, b, lambda b, m: [_rect_light(pkg, b, m), b.translate(pkg.scenes.v(-2.0, 1.0, -2.0), b.sphere(0.3, m))]), 0),
    "translated": (lambda pkg, b: _small(pkg, b, lambda b, m: [b.translate(pkg.scenes.v(0.0, 0.5, 0.0), _rect_light(pkg, b, m))]), 0),
    "two_materials": (lambda pkg, b: _small(pkg, b, lambda b, m: [
        _rect_light(pkg, b, m), b.bvh([b.rect(pkg.scenes.X, (0.5, 1.5), (-1.0, 1.0), -3.0, b.diffuse_light(b.constant(pkg.scenes.vfrom(1.0)), 2.0)),
                                       b.sphere(0.2, b.lambertian(b.constant(pkg.scenes.vfrom(0.5))))])]), 1),
    # two sampled materials, two axes, two areas, one of the rects flipped: the order and every field of the table matter
    "two_lights": (lambda pkg, b: _small(pkg, b, lambda b, m: [
        _rect_light(pkg, b, m),
        b.flip_normals(b.rect(pkg.scenes.X, (0.5, 1.0), (-1.0, 1.0), -3.0, b.diffuse_light(b.constant(pkg.scenes.v(1.0, 2.0, 4.0)), 2.0)))]), 2),
    # the same world twice: an occluding sphere and a fog under the light, the sphere bare ("shallow": the flat interpreter) or
    # under five Translates by zero ("deep": more wrappers than the scheduled walks hold, so the general walk) -- x - 0 = x
    # and p + 0 = p exactly, so the two render the same bits
    "shallow": (lambda pkg, b: _occluded_world(pkg, b, 0), 1),
    "deep": (lambda pkg, b: _occluded_world(pkg, b, 5), 1),
    "too_many": (lambda pkg, b: _small(pkg, b, lambda b, m: [
        b.rect(pkg.scenes.Y, (-1.0 + 0.03 * i, -0.98 + 0.03 * i), (-0.5, 0.5), 2.0, m) for i in range(MAX_LIGHTS + 1)]), MAX_LIGHTS + 1),
}


def build(pkg, backend, name):
    """(Recorder, world, camera, expected table length) of WORLDS[name] on `backend`."""
    import physics_ref
    b = physics_ref.Recorder(backend.builder())
    fn, n = WORLDS[name]
    world, cam = fn(pkg, b)
    return b, world, cam, n
