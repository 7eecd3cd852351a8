"""Random object graphs built through the public builder API -- exercised identically on the oracle and
on the HIP product.  Every reference constructor can appear: Sphere, Rect, FlipNormals, Translate, Scale,
RotateY, And, rect_prism, LinearMove, ConstantMedium, nested Bvh, list or Bvh world; all five materials;
constant / checker / Perlin textures.  By default the shapes only the general walk handles are avoided (at most 4 nested
non-fused wrappers, no medium below And below Bvh, no medium inside a medium's boundary), so that these scenes run on the
scheduled kernels.  `general_boundaries=True` additionally draws ConstantMedium boundaries that are object graphs (prisms,
And, Bvh, transform wrappers) instead of one primitive; `deep_shapes=True` draws exactly the avoided shapes as well (up to 7
nested wrappers, media inside boundary graphs, media anywhere below And below Bvh): FEAT_DEEP programs, baseline kernel.

`meshes=True` draws triangles and meshes (include/rtiow_gpu_mesh.h) at the worlds' own scale wherever the builder takes an
object: as a primitive in every place a sphere or a rect can stand (list level, Bvh leaves, below wrappers, either side of And,
below the 5-7 wrappers of deep_shapes), as a closed mesh bounding a ConstantMedium (bare, under Translate, under FlipNormals,
inside graph_boundary()), and in two more list-level items per world drawn from a menu of those places, each of which
holds a triangle.  `images=True` lets texture() return an image texture (include/rtiow_gpu_image.h).  `media=False`
draws no ConstantMedium, `perlin=False` no Perlin texture (worlds a float64 reference has a closed form for) and `sky=False`
leaves out the emitting sphere of radius 3000 around everything (rays can miss such a world).  The new
branches consume random numbers only when switched on: with the defaults a seed gives the world it always gave.
`marks` (a dict) receives "rect_light": the world is a list that holds a rect with a DiffuseLight directly (light_sampling has
a light to sample).

places(rec, world) and image_settings(rec) read from a physics_ref.Recorder where a world put its triangles and what its
images are: the coverage test's evidence."""
import numpy as np


def random_world(pkg, b, rs, n_top=6, general_boundaries=False, deep_shapes=False, meshes=False, images=False, media=True, perlin=True,
                 sky=True, marks=None):
    S = pkg.scenes
    T, I = pkg.triangle, pkg.image
    lights, rects = set(), set()
    b.set_perlin_tables(*pkg.small_rng.perlin_tables(int(rs.randint(1, 1 << 30))))

    def f(lo, hi):
        return float(np.float32(rs.uniform(lo, hi)))

    def vec(lo, hi):
        return S.v(f(lo, hi), f(lo, hi), f(lo, hi))

    def image_texture():
        w, h = ((1, 1), (2, 3), (5, 4), (8, 8))[rs.randint(0, 4)]
        kw = dict(filter=int(rs.randint(0, 2)), wrap_u=int(rs.randint(0, 2)), wrap_v=int(rs.randint(0, 2)))
        img = rs.uniform(0.05, 0.95, (h, w, 3)).astype(np.float32)
        if rs.rand() < 0.5:   # planar: axes of order 1 / 100 (a texel is tens of units wide), with an offset
            prm = I.planar((f(-0.01, 0.01), f(-0.01, 0.01), f(-0.01, 0.01)), f(0.0, 1.0), (f(-0.01, 0.01), f(-0.01, 0.01), f(-0.01, 0.01)), f(0.0, 1.0), **kw)
        else:                 # spherical about a centre near the origin, where the objects are made
            prm = I.spherical((f(-30, 30), f(-30, 30), f(-30, 30)), **kw)
        return b.image(img, prm)

    def texture(depth=0):
        if images and rs.rand() < 0.35:
            return image_texture()
        k = rs.randint(0, 4 if depth < 2 else 2)
        if k <= 1 or (k == 2 and not perlin):
            return b.constant(vec(0.1, 0.95))
        if k == 2:
            return b.perlin(f(0.02, 0.3))
        return b.checker(texture(depth + 1), texture(depth + 1))

    def material(allow_light=True):
        k = rs.randint(0, 5 if allow_light else 4)
        if k == 0:
            return b.lambertian(texture())
        if k == 1:
            return b.metal(vec(0.3, 0.95), f(0.0, 1.0))
        if k == 2:
            return b.dielectric(f(1.1, 2.0))
        if k == 3:
            return b.isotropic(texture())
        m = b.diffuse_light(texture(), f(0.5, 6.0))
        lights.add(m)
        return m

    def tri_material(closed):
        """every material; a dielectric only on a closed mesh"""
        k = int(rs.randint(0, 5)) if closed else int(rs.choice([0, 1, 3, 4]))
        if k == 0:
            return b.lambertian(texture())
        if k == 1:
            return b.metal(vec(0.3, 0.95), f(0.0, 1.0))
        if k == 2:
            return b.dielectric(f(1.1, 2.0))
        if k == 3:
            return b.isotropic(texture())
        return b.diffuse_light(texture(), f(0.5, 6.0))

    def triangle():
        c, s = vec(-100, 100), f(40, 160)
        while True:   # (a sliver is no use to a random ray: the cross product of the edges is at least a fifth of s^2 long)
            e1, e2 = np.array([f(-1, 1), f(-1, 1), f(-1, 1)]), np.array([f(-1, 1), f(-1, 1), f(-1, 1)])
            if np.sqrt((np.cross(e1, e2) ** 2).sum()) >= 0.2:
                break
        v0 = np.array([c[0], c[1], c[2]], dtype=np.float64)
        return b.triangle(tuple(v0), tuple(v0 + s * e1), tuple(v0 + s * e2), tri_material(False))

    def mesh(closed=False):
        """at most 80 triangles: a box (12), an icosphere of 20 or 80, a grid of up to 4 x 4 cells; the median or the SAH split"""
        k = rs.randint(0, 3 if closed else 4)
        if k == 0:
            p0 = (f(-100, 20), f(-100, 20), f(-100, 20))
            vf = T.box(p0, (p0[0] + f(40, 160), p0[1] + f(40, 160), p0[2] + f(40, 160)))
        elif k <= 2:
            vf = T.icosphere(k - 1, f(30, 100), (f(-60, 60), f(-60, 60), f(-60, 60)))
        else:
            a, wx, wz, amp = f(-120, 0), f(0.01, 0.05), f(0.01, 0.05), f(5, 40)
            vf = T.grid(int(rs.randint(1, 5)), int(rs.randint(1, 5)), lambda x, z: amp * np.sin(wx * x) * np.cos(wz * z), (a, a), (a + f(80, 240), a + f(80, 240)))
        return b.mesh(vf[0], vf[1], tri_material(k <= 2), sah=bool(rs.rand() < 0.5))

    def tri_shape():
        return triangle() if rs.rand() < 0.4 else mesh()

    def wrapper(w, o):
        return (b.translate(vec(-150, 150), o) if w == 0 else b.rotate_y(f(-170, 170), o) if w == 1 else
                b.scale(S.v(f(0.5, 2), f(0.5, 2), f(0.5, 2)), o) if w == 2 else b.linear_move(o, vec(-40, 40)))

    def primitive():
        if meshes and rs.rand() < 0.35:
            return tri_shape()
        if rs.rand() < 0.6:
            return b.sphere(f(20, 90), material())
        a0, b0 = f(-120, 0), f(-120, 0)
        ax, r0, r1, k = int(rs.randint(0, 3)), (a0, a0 + f(40, 220)), (b0, b0 + f(40, 220)), f(-60, 60)
        m = material()
        o = b.rect(ax, r0, r1, k, m)
        if m in lights:
            rects.add(o)
        return o

    max_wrappers = 6 if deep_shapes else 3

    def graph_boundary(level=0):
        """object.rs:441 `ConstantMedium<O: Object>`: any object can bound a medium (main.rs only uses spheres)."""
        def solid():
            if deep_shapes and level < 2 and rs.rand() < 0.3:   # a medium inside the boundary of a medium
                return b.constant_medium(graph_boundary(level + 1), f(0.002, 0.05), b.isotropic(texture()))
            if meshes and rs.rand() < 0.4:
                return mesh(closed=True)
            if rs.rand() < 0.5:
                p0 = vec(-80, 0)
                return b.rect_prism(p0, p0 + S.v(f(60, 200), f(60, 200), f(60, 200)), material())
            return b.translate(vec(-60, 60), b.sphere(f(40, 120), material()))
        k = rs.randint(0, 5)
        if k == 0:
            return solid()
        if k == 1:
            return b.and_(solid(), solid())
        if k == 2:
            return b.bvh([solid() for _ in range(rs.randint(1, 5))], (0.0, 1.0))
        if k == 3:
            return b.rotate_y(f(-170, 170), solid())
        return b.linear_move(b.scale(S.v(f(0.5, 2), f(0.5, 2), f(0.5, 2)), solid()), vec(-40, 40))

    def obj(depth, wrappers, under_bvh, in_and_under_bvh):
        if deep_shapes and wrappers == 0 and rs.rand() < 0.1:   # 5-7 wrappers around one object (object.rs:241-512, any order)
            o = obj(depth + 1, 7, under_bvh, in_and_under_bvh)
            for _ in range(rs.randint(5, 8)):
                w = rs.randint(0, 5)
                o = (b.scale(S.v(f(0.7, 1.5), f(0.7, 1.5), f(0.7, 1.5)), o) if w == 0 else b.linear_move(o, vec(-20, 20)) if w == 1 else
                     b.flip_normals(o) if w == 2 else b.rotate_y(f(-170, 170), o) if w == 3 else b.translate(vec(-60, 60), o))
            return o
        k = rs.randint(0, 10)
        if depth >= (5 if deep_shapes else 3) or k <= 1:
            o = primitive()
        elif k == 2:
            p0 = vec(-80, 0)
            o = b.rect_prism(p0, p0 + S.v(f(30, 120), f(30, 120), f(30, 120)), material())
        elif k == 3:
            o = b.and_(obj(depth + 1, wrappers, under_bvh, under_bvh), obj(depth + 1, wrappers, under_bvh, under_bvh))
        elif k == 4 and wrappers < max_wrappers:
            o = b.translate(vec(-150, 150), obj(depth + 1, wrappers + 1, under_bvh, in_and_under_bvh))
        elif k == 5 and wrappers < max_wrappers:
            o = b.rotate_y(f(-170, 170), obj(depth + 1, wrappers + 1, under_bvh, in_and_under_bvh))
        elif k == 6 and wrappers < max_wrappers:
            w = rs.randint(0, 3)
            inner = obj(depth + 1, wrappers + 1, under_bvh, in_and_under_bvh)
            o = (b.scale(S.v(f(0.5, 2), f(0.5, 2), f(0.5, 2)), inner) if w == 0 else
                 b.linear_move(inner, vec(-40, 40)) if w == 1 else b.flip_normals(inner))
        elif k == 7 and media and (deep_shapes or not in_and_under_bvh):
            if meshes and rs.rand() < 0.4:
                boundary = mesh(closed=True)
            else:
                boundary = graph_boundary() if general_boundaries else b.sphere(f(40, 160), material())
            if rs.rand() < 0.5:
                boundary = b.translate(vec(-100, 100), boundary)
            if rs.rand() < 0.3:
                boundary = b.flip_normals(boundary)
            o = b.constant_medium(boundary, f(0.002, 0.05), b.isotropic(texture()))
        elif k == 8:
            o = b.bvh([obj(depth + 1, wrappers, True, False) for _ in range(rs.randint(1, 6))], (0.0, 1.0))
        else:
            o = b.translate(vec(-200, 200), b.sphere(f(10, 60), material()))
        return o

    bvh_world = rs.rand() < 0.4  # lib.rs:51 `impl World for Bvh`: then every top-level object sits below a Bvh
    world = [obj(0, 0, bvh_world, False) for _ in range(n_top)]
    if meshes:
        def extra(e):
            if e == 0:
                return triangle()
            if e == 1:
                return b.flip_normals(triangle())
            if e == 2:
                return mesh()
            if e == 3:
                return wrapper(rs.randint(0, 4), tri_shape())
            if e == 4:
                return wrapper(rs.randint(0, 4), wrapper(rs.randint(0, 4), wrapper(rs.randint(0, 4), tri_shape())))
            if e == 5:
                sides = [tri_shape(), b.translate(vec(-100, 100), b.sphere(f(20, 90), material()))]
                return b.and_(*(sides if rs.rand() < 0.5 else sides[::-1]))
            if e == 6 and media:
                w = rs.randint(0, 3)
                boundary = mesh(closed=True)
                boundary = b.translate(vec(-100, 100), boundary) if w == 1 else b.flip_normals(boundary) if w == 2 else boundary
                return b.constant_medium(boundary, f(0.002, 0.05), b.isotropic(texture()))
            leaves = [mesh()] + [b.translate(vec(-200, 200), b.sphere(f(10, 60), material())) for _ in range(rs.randint(1, 4))]
            return b.bvh([leaves[i] for i in rs.permutation(len(leaves))], (0.0, 1.0))
        world += [extra(rs.randint(0, 8)), extra(rs.randint(0, 8))]
        if rs.rand() < 0.3:   # a rect light at list level: light_sampling has something to sample
            a0, b0 = f(-120, 0), f(-120, 0)
            m = b.diffuse_light(b.constant(vec(0.5, 0.95)), f(2.0, 6.0))
            world.append(b.rect(int(rs.randint(0, 3)), (a0, a0 + f(40, 220)), (b0, b0 + f(40, 220)), f(100, 300), m))
            rects.add(world[-1])
    if marks is not None:
        marks["rect_light"] = (not bvh_world) and any(o in rects for o in world)
    if sky:
        world.append(b.flip_normals(b.sphere(3000.0, b.diffuse_light(b.constant(S.v(0.6, 0.7, 0.9)), 1.0))))
    if bvh_world:
        world = [b.bvh(world, (0.0, 1.0))]
    return world


def random_camera(pkg, be, rs, nx, ny):
    S = pkg.scenes
    frm = S.v(float(rs.uniform(-500, 500)), float(rs.uniform(-100, 400)), float(rs.uniform(-900, -400)))
    return be.camera_look(frm, S.v(0, 0, 0), S.v(0, 1, 0), float(rs.uniform(20, 60)), nx / ny,
                          float(rs.choice([0.0, 5.0, 30.0])), float(rs.uniform(300, 900)),
                          (0.0, float(rs.choice([1.0, 0.25]))))


# ---- what a recorded world holds (physics_ref.Recorder) -------------------------------------------------------------------------
PLACES = ("triangle at list level", "flipped triangle at list level", "mesh at list level", "mesh leaf of a nested Bvh beside analytic leaves",
          "top-level Bvh world", "under Translate", "under RotateY", "under Scale (non-uniform)", "under LinearMove", "under a chain of three",
          "one side of And", "medium boundary: bare mesh", "medium boundary: mesh under Translate", "medium boundary: mesh under FlipNormals",
          "mesh inside a graph boundary", "below 5-7 wrappers", "median split", "SAH split",
          "lambertian triangle", "metal triangle", "dielectric triangle", "isotropic triangle", "light triangle")
IMAGE_SETTINGS = tuple(["size %dx%d" % s for s in ((1, 1), (2, 3), (5, 4), (8, 8))] + ["filter 0", "filter 1", "mapping 0", "mapping 1"] +
                       ["wraps %d%d" % (u, v) for u in (0, 1) for v in (0, 1)] +
                       ["under lambertian", "under isotropic", "under light", "checker child 0", "checker child 1"])
_WRAP = {"translate": "under Translate", "rotate": "under RotateY", "scale": "under Scale (non-uniform)", "move": "under LinearMove"}


def places(rec, world):
    """The places of PLACES in which the recorded world holds a triangle or a mesh."""
    seen = set()
    O = rec.objects

    def child(r):
        return r[1] if r[0] == "flip" else r[2]

    def has_tri(o):
        r = O[o]
        if r[0] in ("tri", "mesh"):
            return True
        if r[0] in ("flip", "translate", "scale", "rotate", "move"):
            return has_tri(child(r))
        if r[0] == "and":
            return has_tri(r[1]) or has_tri(r[2])
        if r[0] == "bvh":
            return any(has_tri(c) for c in r[1])
        return r[0] == "medium" and has_tri(r[1])

    def walk(o, above, top):
        """above: the kinds of the ancestors, nearest first"""
        r = O[o]
        k = r[0]
        if k in ("tri", "mesh"):
            if k == "mesh":
                seen.add("SAH split" if r[3] else "median split")
            seen.add(rec.materials[r[2]][0] + " triangle")
            if above and above[0] in _WRAP:
                if above[0] != "scale" or len(set(float(x) for x in O[top[0]][1])) == 3:
                    seen.add(_WRAP[above[0]])
                if len(above) >= 3 and all(a in _WRAP for a in above[:3]):
                    seen.add("under a chain of three")
            n_wrap = 0
            for a in above:
                if a not in _WRAP and a != "flip":
                    break
                n_wrap += 1
            if n_wrap >= 5:
                seen.add("below 5-7 wrappers")
        elif k in ("flip", "translate", "scale", "rotate", "move"):
            walk(child(r), (k,) + above, (o,) + top)
        elif k == "and":
            for a, c in ((r[1], r[2]), (r[2], r[1])):
                if has_tri(a) and not has_tri(c):
                    seen.add("one side of And")
            walk(r[1], ("and",) + above, (o,) + top)
            walk(r[2], ("and",) + above, (o,) + top)
        elif k == "bvh":
            if above and any(O[c][0] == "mesh" for c in r[1]) and any(not has_tri(c) for c in r[1]):
                seen.add("mesh leaf of a nested Bvh beside analytic leaves")
            for c in r[1]:
                walk(c, ("bvh",) + above, (o,) + top)
        elif k == "medium":
            bd = O[r[1]]
            if bd[0] == "mesh":
                seen.add("medium boundary: bare mesh")
            elif bd[0] == "translate" and O[bd[2]][0] == "mesh":
                seen.add("medium boundary: mesh under Translate")
            elif bd[0] == "flip" and (O[bd[1]][0] == "mesh" or (O[bd[1]][0] == "translate" and O[O[bd[1]][2]][0] == "mesh")):
                seen.add("medium boundary: mesh under FlipNormals")
            elif has_tri(r[1]):
                seen.add("mesh inside a graph boundary")
            walk(r[1], ("medium",) + above, (o,) + top)

    if len(world) == 1 and O[world[0]][0] == "bvh":
        if has_tri(world[0]):
            seen.add("top-level Bvh world")
        for c in O[world[0]][1]:
            walk(c, ("bvh",), (world[0],))
    else:
        for o in world:
            r = O[o]
            if r[0] == "tri":
                seen.add("triangle at list level")
            elif r[0] == "flip" and O[r[1]][0] == "tri":
                seen.add("flipped triangle at list level")
            elif r[0] == "mesh":
                seen.add("mesh at list level")
            walk(o, (), ())
    return seen


def image_settings(rec):
    """The settings of IMAGE_SETTINGS the recorded builder's image textures show, and where the images sit."""
    seen = set()
    for t, r in rec.textures.items():
        if r[0] == "image":
            prm = r[2]
            seen |= {"size %dx%d" % (r[1].shape[1], r[1].shape[0]), "filter %d" % prm["filter"], "mapping %d" % prm["mapping"],
                     "wraps %d%d" % (prm["wrap_u"], prm["wrap_v"])}
        elif r[0] == "checker":
            seen |= {"checker child %d" % i for i in (0, 1) if rec.textures[r[1 + i]][0] == "image"}
    for m, r in rec.materials.items():
        if r[0] in ("lambertian", "isotropic", "light") and rec.textures[r[1]][0] == "image":
            seen.add("under " + r[0])
    return seen
