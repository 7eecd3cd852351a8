"""Triangles, rays and graphs shared by test_mesh_abi.py (CPU) and test_mesh_gpu.py (GPU).

edge_pairs()        (tri9, rays8): (triangle, ray) pairs for the host probe -- random pairs and the edge cases: rays through vertices and
                    along edges, parallel to the plane and in it, -0 components, directions of length 1e-30 / 1e30 / 0, NaN and
                    infinite components, t at t_min and at t_max, slivers of aspect 1e-6, coordinates near 1e4
list_triangles(k)   k triangles standing in each other's way, for list worlds without a Bvh
edge_rays(tris)     rays7 against a list of triangles: the edge cases again, aimed at those triangles
GRAPHS              name -> fn(pkg, b) -> (world, groups): builder calls and, beside them, the description triangle_ref reads
aimed_rays(groups)  seeded float64 rays aimed at (and past) the groups' triangles"""
import numpy as np

import triangle_ref as TR

f32 = np.float32
F32_MAX = np.finfo(np.float32).max
T_MIN = 0.001


def _pairs(tris, rays):
    return np.asarray(tris, f32).reshape(-1, 9), np.asarray(rays, f32).reshape(-1, 8)


def edge_pairs(n_random=4096, seed=5):
    rs = np.random.RandomState(seed)
    tris, rays = [], []

    def add(tri, o, d, t_max=F32_MAX):
        tris.append(np.asarray(tri, f32).reshape(9))
        rays.append(np.concatenate([np.asarray(o, f32), np.asarray(d, f32), [f32(0.0), f32(t_max)]]).astype(f32))

    # random pairs, aimed so that about half hit
    t = rs.uniform(-2, 2, (n_random, 3, 3))
    o = rs.uniform(-3, 3, (n_random, 3))
    target = t.mean(axis=1) + rs.normal(0, 0.4, (n_random, 3))
    for k in range(n_random):
        add(t[k], o[k], target[k] - o[k])
    base = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    skew = np.array([[0.25, -0.5, 1.0], [1.5, 0.25, 0.75], [-0.25, 1.25, 1.5]])
    for tri in (base, skew, skew * 1e4 + 1e4):
        e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
        nn = np.cross(e1, e2)
        nn = nn / np.linalg.norm(nn)
        scale = np.linalg.norm(e1)
        for sgn in (1.0, -1.0):
            start = lambda q: q + sgn * 2.0 * scale * nn   # noqa: E731
            # through the vertices, the edge midpoints, points on the edges, the centroid
            for u, v in ((0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.25, 0.75), (1 / 3, 1 / 3), (0.3, 0), (0, 0.7)):
                q = tri[0] + u * e1 + v * e2
                add(tri, start(q), q - start(q))
                add(tri, start(q), 0.37 * (q - start(q)))
            # along the edges (in the plane), parallel to the plane above it, in the plane across the triangle
            for a, b in ((0, 1), (1, 2), (2, 0)):
                add(tri, tri[a] - (tri[b] - tri[a]), tri[b] - tri[a])
                add(tri, tri[a] + sgn * 0.5 * scale * nn, tri[b] - tri[a])
            add(tri, tri[0] - e1 - e2, e1 + e2)
            # t exactly at t_min and at t_max: the origin one unit-direction step in front of the centroid
            q = tri[0] + 0.25 * e1 + 0.25 * e2
            d = -sgn * nn * scale
            for t_hit in (T_MIN, 0.5, 2.0):
                oo = (q - t_hit * d)
                add(tri, oo, d)
                add(tri, oo, d, t_max=t_hit)
                add(tri, oo, d, t_max=np.nextafter(f32(t_hit), f32(10.0)))
    # -0 components, zero components
    for o, d in (([0.25, 0.25, 1.0], [-0.0, -0.0, -1.0]), ([0.25, 0.25, 1.0], [0.0, 0.0, -1.0]), ([-0.0, -0.0, 1.0], [0.0, -0.0, -1.0]),
                 ([0.25, 0.25, -0.0], [0.0, 0.0, 1.0]), ([0.25, -0.0, 1.0], [0.0, 0.0, -1.0])):
        add(base, o, d)
    # directions of length 1e-30 and 1e30, d = 0
    for ln in (1e-30, 1e30, 1e-38, 1e38, 0.0):
        add(base, [0.25, 0.25, 1.0], [0.0, 0.0, -ln])
        add(skew, [0.0, 0.0, 3.0], np.array([0.3, 0.2, -1.0]) * ln)
    # NaN and infinite ray components
    for bad in (np.nan, np.inf, -np.inf):
        for slot in range(6):
            r = [0.25, 0.25, 1.0, 0.0, 0.0, -1.0]
            r[slot] = bad
            add(base, r[:3], r[3:])
        add(base, [0.25, 0.25, 1.0], [0.0, 0.0, -1.0], t_max=bad)
    # slivers with a 1e-6 aspect, hit through the middle and past the thin side
    for w in (1e-6, 3e-6):
        sliver = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, w, 0.0]])
        for y in (0.25 * w, 0.5 * w, w, 2 * w, -0.25 * w, 0.0):
            add(sliver, [0.5, y, 1.0], [0.0, 0.0, -1.0])
            add(sliver, [0.3, y, 1.0], [0.2, 0.0, -1.0])
    # triangles at coordinates near 1e4
    far = rs.uniform(-1, 1, (64, 3, 3)) + 1e4
    for k in range(64):
        q = far[k].mean(axis=0) + rs.normal(0, 0.2, 3)
        oo = q + rs.normal(0, 3, 3)
        add(far[k], oo, q - oo)
    return _pairs(tris, rays)


def list_triangles(k):
    """k triangles of a list world: overlapping in projection along z, at different depths, one back-facing, two sharing an
    edge (k >= 3) and two in ONE plane with equal t along shared rays (k = 7: the first of the list wins)."""
    all7 = np.array([
        [[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]],
        [[-1.0, -1.0, -0.5], [0.0, 1.0, -0.5], [1.0, -1.0, -0.5]],      # behind the first, back-facing towards +z
        [[1.0, -1.0, 0.0], [2.0, 1.0, 0.25], [0.0, 1.0, 0.0]],          # shares the edge (1, -1, 0) - (0, 1, 0) with the first
        [[-2.0, -0.5, 0.5], [2.0, -0.5, 0.75], [0.0, 0.75, -1.0]],      # cuts through the others
        [[-0.5, -0.5, 1.0], [0.5, -0.5, 1.0], [0.0, 0.5, 1.0]],         # in front
        [[-0.25, -0.5, 1.0], [0.75, -0.5, 1.0], [0.25, 0.5, 1.0]],      # the same plane as the one before, overlapping it
        [[0.0, -2.0, -1.0], [0.0, 2.0, -1.0], [0.0, 0.0, 2.0]],         # edge on to rays along z
    ], dtype=f32)
    return all7[:k]


def edge_rays(tris, n_random=1024, seed=9):
    """rays7 for a list world of `tris`: random rays, rays along z through every vertex and edge midpoint, in-plane rays, -0
    and zero components, tiny / huge / zero directions, NaN and infinite components."""
    tris = np.asarray(tris, np.float64)
    rs = np.random.RandomState(seed)
    rays = []
    o = rs.uniform(-3, 3, (n_random, 3))
    which = rs.randint(0, len(tris), n_random)
    w = rs.dirichlet((1, 1, 1), n_random)
    target = (tris[which] * w[:, :, None]).sum(axis=1) + rs.normal(0, 0.3, (n_random, 3)) * (rs.uniform(size=(n_random, 1)) < 0.3)
    astray = rs.uniform(size=n_random) < 0.35              # ... and a third of them anywhere: a list of seven leaves few gaps
    target[astray] = rs.uniform(-4, 4, (int(astray.sum()), 3))
    rays += list(np.concatenate([o, target - o], axis=1))
    for tri in tris:
        pts = [tri[0], tri[1], tri[2], 0.5 * (tri[0] + tri[1]), 0.5 * (tri[1] + tri[2]), 0.5 * (tri[2] + tri[0]), tri.mean(axis=0)]
        for q in pts:
            for dz in (3.0, -3.0):
                rays.append(np.concatenate([q + [0, 0, dz], [0.0, 0.0, -dz]]))
                rays.append(np.concatenate([q + [0, 0, dz], [-0.0, 0.0, -0.25 * dz]]))
        for a, b in ((0, 1), (1, 2), (2, 0)):
            rays.append(np.concatenate([tri[a] - (tri[b] - tri[a]), tri[b] - tri[a]]))
    for ln in (1e-30, 1e30, 0.0):
        rays.append(np.array([0.1, -0.2, 3.0, 0.0, 0.0, -ln]))
        rays.append(np.array([0.1, -0.2, 3.0, 0.01 * ln, 0.02 * ln, -ln]))
    for bad in (np.nan, np.inf, -np.inf):
        for slot in range(6):
            r = np.array([0.1, -0.2, 3.0, 0.0, 0.0, -1.0])
            r[slot] = bad
            rays.append(r)
    rays = np.asarray(rays, f32)
    return np.concatenate([rays, np.zeros((len(rays), 1), f32)], axis=1)


# ---- graphs -------------------------------------------------------------------------------------------------------------------
def _mats(b):
    return [b.lambertian(b.constant((0.5, 0.5, 0.5))), b.metal((0.5, 0.5, 0.5), 0.0), b.lambertian(b.constant((0.5, 0.5, 0.5)))]


def _mesh(pkg, b, vf, mat, sah=False):
    v, f = vf
    return b.mesh(v, f, mat, sah=sah), pkg.triangle.vertices_of(v, f)


def graph_ico(pkg, b, sah=False):
    m = _mats(b)
    obj, tri = _mesh(pkg, b, pkg.triangle.icosphere(2, 1.0), m[0], sah)
    return [obj], [{"tri": tri, "chain": (), "sign": 1, "mat": m[0]}]


def graph_box(pkg, b, sah=False):
    m = _mats(b)
    obj, tri = _mesh(pkg, b, pkg.triangle.box((-1.0, -0.5, -0.75), (0.5, 1.0, 1.25)), m[1], sah)
    return [obj], [{"tri": tri, "chain": (), "sign": 1, "mat": m[1]}]


def graph_wrapped(pkg, b):
    """A mesh under Translate, RotateY, Scale (non-uniform), LinearMove, FlipNormals and And."""
    T = pkg.triangle
    m = _mats(b)
    ico, t_ico = _mesh(pkg, b, T.icosphere(1, 0.8), m[0])
    box, t_box = _mesh(pkg, b, T.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), m[1], sah=True)
    grid, t_grid = _mesh(pkg, b, T.grid(3, 2, lambda x, z: 0.2 * np.sin(3 * x) * np.cos(2 * z), (-1.0, -1.0), (1.0, 1.0)), m[2])
    one = b.triangle((-0.5, 0.0, 0.3), (0.5, 0.0, 0.3), (0.0, 0.8, -0.3), m[2])
    t_one = np.array([[[-0.5, 0.0, 0.3], [0.5, 0.0, 0.3], [0.0, 0.8, -0.3]]], f32)
    world = [
        b.translate((2.0, 0.5, 0.0), b.rotate_y(30.0, b.scale((1.5, 0.5, 0.75), ico))),
        b.flip_normals(b.translate((-2.0, 0.0, 0.5), b.rotate_y(-50.0, box))),
        b.linear_move(b.translate((0.0, -1.5, 0.0), grid), (0.5, 0.0, 0.25)),
        b.and_(b.translate((0.0, 1.5, 0.0), one), b.flip_normals(b.scale((2.0, 2.0, 2.0), b.translate((0.0, 1.0, -1.0), one)))),
    ]
    groups = [
        {"tri": t_ico, "chain": (("translate", TR.PR._r32((2.0, 0.5, 0.0))), ("rotate", 30.0), ("scale", TR.PR._r32((1.5, 0.5, 0.75)))), "sign": 1, "mat": m[0]},
        {"tri": t_box, "chain": (("translate", TR.PR._r32((-2.0, 0.0, 0.5))), ("rotate", -50.0)), "sign": -1, "mat": m[1]},
        {"tri": t_grid, "chain": (("move", TR.PR._r32((0.5, 0.0, 0.25))), ("translate", TR.PR._r32((0.0, -1.5, 0.0)))), "sign": 1, "mat": m[2]},
        {"tri": t_one, "chain": (("translate", TR.PR._r32((0.0, 1.5, 0.0))),), "sign": 1, "mat": m[2]},
        {"tri": t_one, "chain": (("scale", TR.PR._r32((2.0, 2.0, 2.0))), ("translate", TR.PR._r32((0.0, 1.0, -1.0)))), "sign": -1, "mat": m[2]},
    ]
    return world, groups


def graph_deep(pkg, b):
    """A mesh below six wrappers (more than MAX_XFORM_DEPTH = 4: FEAT_DEEP, the general walk), beside a plain one."""
    T = pkg.triangle
    m = _mats(b)
    ico, t_ico = _mesh(pkg, b, T.icosphere(1, 0.7), m[0])
    box, t_box = _mesh(pkg, b, T.box((-0.4, -0.4, -0.4), (0.4, 0.4, 0.4)), m[1])
    # (Translate{RotateY} would fuse into one level: none here does)
    chain = (("scale", (1.25, 0.8, 1.0)), ("rotate", 20.0), ("scale", (0.8, 1.25, 1.0)), ("rotate", -35.0), ("translate", (1.0, 0.5, 0.0)),
             ("scale", (0.5, 1.5, 2.0)), ("translate", (0.0, 0.25, -0.5)))
    obj = ico
    for k, a in reversed(chain):
        obj = b.translate(a, obj) if k == "translate" else (b.rotate_y(a, obj) if k == "rotate" else b.scale(a, obj))
    world = [obj, b.translate((-1.5, 0.0, 0.0), box)]
    groups = [{"tri": t_ico, "chain": tuple((k, a if k == "rotate" else TR.PR._r32(a)) for k, a in chain), "sign": 1, "mat": m[0]},
              {"tri": t_box, "chain": (("translate", TR.PR._r32((-1.5, 0.0, 0.0))),), "sign": 1, "mat": m[1]}]
    return world, groups


GRAPHS = {"ico": graph_ico, "box": graph_box, "wrapped": graph_wrapped, "deep": graph_deep}
N_RAYS = 4096


def aimed_rays(groups, n=N_RAYS, seed=21):
    """Float64 [n, 7] rays: origins on a shell around the graph, 70 % aimed at a point of a triangle (in the world, at the ray's
    time), 30 % at a point well beside the graph; un-normalised directions of length 0.1 .. 10."""
    rs = np.random.RandomState(seed)
    time = rs.uniform(0.0, 1.0, n)
    which_g = rs.randint(0, len(groups), n)
    target = np.zeros((n, 3))
    for gi, g in enumerate(groups):
        at = which_g == gi
        k = int(at.sum())
        tri = np.asarray(g["tri"], np.float64)[rs.randint(0, len(g["tri"]), k)]
        w = rs.dirichlet((1, 1, 1), k)
        target[at] = TR.point_to_world(g["chain"], (tri * w[:, :, None]).sum(axis=1), time[at])
    centre, radius = target.mean(axis=0), np.sqrt(((target - target.mean(axis=0)) ** 2).sum(axis=1)).max()
    v = rs.normal(size=(n, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    origin = centre + v * radius * rs.uniform(1.3, 2.5, n)[:, None]
    away = rs.uniform(size=n) < 0.3
    w = rs.normal(size=(n, 3))
    w /= np.sqrt((w * w).sum(axis=1))[:, None]
    target[away] = centre + w[away] * radius * rs.uniform(1.5, 3.0, int(away.sum()))[:, None]
    d = target - origin
    d *= (10.0 ** rs.uniform(-1.0, 1.0, n) / np.sqrt((d * d).sum(axis=1)))[:, None]
    return np.concatenate([origin, d, time[:, None]], axis=1)
