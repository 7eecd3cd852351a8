"""An independent float64 statement of what the renderer computes, for test_physics_oracle.py (the CPU restatement),
test_physics_gpu.py (the HIP kernels) and the random mesh worlds of test_fuzz_mesh.py / test_fuzz_mesh_gpu.py.  Nothing here is computed by either: the one thing shared with the project is the
builder surface -- Recorder wraps a Builder and keeps a Python description of every texture, material and object beside its
handle -- and every expectation below comes from that description in numpy float64.

A. closest_hit: the closest hit of rays with a recorded graph, written from the geometry.  A graph is flattened to its
   primitives (spheres, axis rects, triangles; a prism is six rects, a mesh its triangles, a Bvh its leaves, And both
   sides), each with the chain of Translate / Scale / RotateY / LinearMove above it and the parity of its FlipNormals; the
   closest hit is the smallest
   admissible ray parameter over the primitives.  Conventions (the reference's, read as a specification): a rect's ranges are
   half open and its normal is +axis; RotateY(theta) maps a local point (x, y, z) to (c x + s z, y, -s x + c z); Scale
   multiplies points by the factor and DIVIDES the normal by it, without renormalising; LinearMove shifts the ray origin by
   -time * motion and leaves p where the inner object put it; a sphere's normal is p / radius.
   Every ray also gets a conditioning margin, the smallest of: |disc| / (b^2 + a |c|) of every sphere the ray can reach;
   |t - t_near| |d| / max(1, |origin|) of every root; the relative gap (t2 - t1) / t1 between the best and the second-best t;
   every rect crossing's distance from the rect's four edges, relative to the rect's extent on that axis.  (Primitives whose
   nearest root or crossing lies beyond the accepted hit, and spheres wholly behind the origin, are not counted: nothing
   there can change the answer.)
   Measured on the CPU restatement, float32, over the ten scenes of A, 4096 rays each (test_physics_oracle.py prints them):
     MARGIN = 1e-4 leaves out 0.07 .. 3.6 % of a scene's rays (cap 5 %; most in cornell, whose prisms stand on the floor);
     no hit-flag or material mismatch among the rest;
     worst deviations  t 5.2e-04 (relative)   p 1.2e-04 (relative to max(1, |p|))   normal 1.7e-04 (absolute)
     (t and p: book 1, rays that skim its ground sphere of radius 1000 from 0.05 above it; the hand-built graphs stay
     below 7e-05, 8e-05 and 1.7e-04.)
   TOL_T, TOL_P, TOL_N are 4 x those figures: 2.1e-03, 4.8e-04, 6.8e-04.  Float32 error grows with 1 / margin, a wrong formula moves answers by O(1).
   The feature planes use the same margin and tolerances per pixel (cap 10 % of pixels); under a checker a pixel is also
   left out when |sin sin sin| at one of its hits is within TOL_P of zero.
   Triangles (Recorder.triangle / mesh; one Prim("tri", (v0, v1, v2)) each): the plane crossing t = n.(v0 - o) / n.d with
   n = e1 x e2 and the barycentric coordinates by Cramer's rule on the Gram matrix of (e1, e2) -- not Moeller-Trumbore's cross
   products --, edges inclusive, the unit normal n / |n|.  Margin terms: the barycentric distances |u|, |v|, |1 - u - v|;
   |n.d| / (|e1| |e2| |d|); the crossing's distance from t_near (alone, when the crossing lies behind the origin).  This is
   the one statement of the triangle: triangle_ref.closest_hit64 calls it, and its docstring holds what was measured on
   mesh_cases' graphs (worst t 8.3e-05, p 1.3e-04, normal 2.5e-07; 0.10 .. 2.05 % left out).
   At the scale of the random worlds (fuzz_scenes.py: tens to hundreds of units, origins up to 1500 away; 2048 rays a world;
   fuzz_mesh_cases.py holds the seed sets and test_fuzz_mesh.py prints the figures), measured on the CPU, float32:
     spheres, rects and prisms, eight analytic worlds on the restatement: 0.10 .. 0.54 % left out; worst t 1.5e-03, p 7.3e-06,
     normal 1.1e-04;
     triangles, the twelve media-free mesh worlds through triangle_ref.closest32: 0.00 .. 1.23 % left out; worst t 5.3e-04,
     p 8.3e-06, normal 2.0e-07;
     no flag, material or primitive mismatch in either.  Per hit kind the tolerance there is the larger of the recorded one
     and 4 x these (fuzz_mesh_cases.TOL).
   Image textures (Recorder.image) are evaluated by image_ref.sample64, also as a checker's child.  A nearest-filtered image
   joins the leave-the-pixel-out rule with its margin (texels to the next texel change) against what the position tolerance
   TOL_P max(1, |p|) can move (x, y), plus image_ref.NEAREST_MARGIN.  A bilinear image gets a per-point allowance on the albedo,
   derived and not measured: the local slope of the tent sum times that shift (image_ref.bilinear_allowance), plus the
   measured BILINEAR_TOL of the image's size (image_ref's docstring: 1.4e-06 at 2 x 3 .. 2.4e-06 at 8 x 8, worst, on the CPU).
B. exact_radiance: no reference at all -- all albedos 0.5 and one emitter colour of powers of two make every sample's colour
   exactly 0.5^bounces * L in float32.
C. trace_tree: a float64 tracer of deterministic interfaces (mirror metal, dielectric with Schlick) that returns, for one
   narrow-beam pose, every outcome (colour, bounces) with its probability, to depth DEPTH; paths longer than that are one
   "deep" outcome.  A pose is admissible when the centre ray and the four corner rays of a frame twice as wide give the same
   tree with every margin above POSE_MARGIN.
D. lobe_shares: float64 Monte Carlo of one scattering lobe alone (numpy's generator), and exp(-rho l) for a medium slab.

`fault=` plants a deliberately wrong variant (test_the_checks_notice_planted_faults only): "rotate_neg", "scale_normal",
"ni_over_nt", "schlick4", "unit_sphere", "free_path"."""
import numpy as np

F = np.float64
f32 = np.float32

MARGIN = 1e-4
WORST_T, WORST_P, WORST_N = 5.2e-4, 1.2e-4, 1.7e-4      # measured: see the docstring
TOL_T, TOL_P, TOL_N = 4 * WORST_T, 4 * WORST_P, 4 * WORST_N
CAP_RAYS, CAP_PIXELS = 0.05, 0.10
DEPTH = 6
POSE_MARGIN = 5e-3
T_NEAR = 0.001
GLASS_FIRST_SHARES = 14   # of GLASS_POSES: the first hit is a dielectric interface whose two subtrees share no outcome
FAULTS = ("rotate_neg", "scale_normal", "ni_over_nt", "schlick4", "unit_sphere", "free_path")


def _r32(x):
    """What the binding hands the library: the value rounded to float32 (here as float64)."""
    return np.asarray(np.asarray(x, dtype=f32), dtype=F)


class Recorder:
    """A Builder that remembers what every handle it gave out stands for; every other call goes to the Builder as it is."""

    def __init__(self, builder):
        self._b = builder
        self.textures, self.materials, self.objects = {}, {}, {}

    def __getattr__(self, name):
        return getattr(self._b, name)

    def _put(self, table, handle, rec):
        table[handle] = rec
        return handle

    def constant(self, color):
        return self._put(self.textures, self._b.constant(color), ("constant", _r32([color[0], color[1], color[2]])))

    def checker(self, t0, t1):
        return self._put(self.textures, self._b.checker(t0, t1), ("checker", t0, t1))

    def perlin(self, scale):
        return self._put(self.textures, self._b.perlin(scale), ("perlin", float(f32(scale))))

    def lambertian(self, albedo):
        return self._put(self.materials, self._b.lambertian(albedo), ("lambertian", albedo))

    def isotropic(self, albedo):
        return self._put(self.materials, self._b.isotropic(albedo), ("isotropic", albedo))

    def diffuse_light(self, emission, brightness):
        return self._put(self.materials, self._b.diffuse_light(emission, brightness), ("light", emission, float(f32(brightness))))

    def metal(self, albedo, fuzz):
        return self._put(self.materials, self._b.metal(albedo, fuzz), ("metal", _r32([albedo[0], albedo[1], albedo[2]]), float(f32(fuzz))))

    def dielectric(self, ref_idx):
        return self._put(self.materials, self._b.dielectric(ref_idx), ("dielectric", float(f32(ref_idx))))

    def sphere(self, radius, material):
        return self._put(self.objects, self._b.sphere(radius, material), ("sphere", float(f32(radius)), material))

    def rect(self, orthogonal_to, range0, range1, k, material):
        return self._put(self.objects, self._b.rect(orthogonal_to, range0, range1, k, material),
                         ("rect", int(orthogonal_to), _r32(range0), _r32(range1), float(f32(k)), material))

    def flip_normals(self, obj):
        return self._put(self.objects, self._b.flip_normals(obj), ("flip", obj))

    def translate(self, offset, obj):
        return self._put(self.objects, self._b.translate(offset, obj), ("translate", _r32(offset), obj))

    def scale(self, factor, obj):
        return self._put(self.objects, self._b.scale(factor, obj), ("scale", _r32(factor), obj))

    def rotate_y(self, degrees, obj):
        return self._put(self.objects, self._b.rotate_y(degrees, obj), ("rotate", float(f32(degrees)), obj))

    def and_(self, a, b):
        return self._put(self.objects, self._b.and_(a, b), ("and", a, b))

    def rect_prism(self, p0, p1, material):
        return self._put(self.objects, self._b.rect_prism(p0, p1, material), ("prism", _r32(p0), _r32(p1), material))

    def linear_move(self, obj, motion):
        return self._put(self.objects, self._b.linear_move(obj, motion), ("move", _r32(motion), obj))

    def constant_medium(self, boundary, density, material):
        return self._put(self.objects, self._b.constant_medium(boundary, density, material),
                         ("medium", boundary, float(f32(density)), material))

    def bvh(self, objs, exposure=(0.0, 1.0)):
        return self._put(self.objects, self._b.bvh(objs, exposure), ("bvh", tuple(objs)))

    def bvh_sah(self, objs, exposure=(0.0, 1.0)):
        return self._put(self.objects, self._b.bvh_sah(objs, exposure), ("bvh", tuple(objs)))

    def image(self, img, params):
        """texels [h, w, 3] and the in-fields of the parameters, the eight floats rounded to float32"""
        prm = dict(mapping=int(params["mapping"]), filter=int(params["filter"]), wrap_u=int(params["wrap_u"]), wrap_v=int(params["wrap_v"]),
                   m=_r32(np.asarray(params["m"]).reshape(-1)[:8]))
        return self._put(self.textures, self._b.image(img, params), ("image", _r32(img), prm))

    def triangle(self, v0, v1, v2, material):
        tri = _r32([[v0[0], v0[1], v0[2]], [v1[0], v1[1], v1[2]], [v2[0], v2[1], v2[2]]])
        return self._put(self.objects, self._b.triangle(v0, v1, v2, material), ("tri", tri, material))

    def mesh(self, vertices, indices, material, sah=False):
        """[m, 3, 3]: the three vertices of every face, in the order of `indices`"""
        tris = _r32(np.asarray(vertices).reshape(-1, 3))[np.asarray(indices, dtype=np.int64).reshape(-1, 3)]
        return self._put(self.objects, self._b.mesh(vertices, indices, material, sah=sah), ("mesh", tris, material, bool(sah)))


# ---------------------------------------------------------------------------------------------------------------------------
# A. the closest hit
# ---------------------------------------------------------------------------------------------------------------------------
class Prim:
    def __init__(self, kind, params, material, chain, sign):
        self.kind, self.params, self.material, self.chain, self.sign = kind, params, material, chain, sign


def primitives(rec, world, media=None):
    """The primitives of the recorded graph `world` (a list of object handles).  A ConstantMedium is not a surface: it is
    appended to `media` as (boundary primitives, density, material) when a list is given, and refused otherwise."""
    out = []

    def walk(o, chain, sign, into):
        r = rec.objects[o]
        k = r[0]
        if k == "sphere":
            into.append(Prim("sphere", (r[1],), r[2], chain, sign))
        elif k == "rect":
            into.append(Prim("rect", r[1:5], r[5], chain, sign))
        elif k == "tri":
            into.append(Prim("tri", (r[1][0], r[1][1], r[1][2]), r[2], chain, sign))
        elif k == "mesh":
            for tri in r[1]:
                into.append(Prim("tri", (tri[0], tri[1], tri[2]), r[2], chain, sign))
        elif k == "prism":
            p0, p1, m = r[1], r[2], r[3]
            for ax in range(3):
                a0, a1 = [a for a in range(3) if a != ax]
                for kk, s in ((p1[ax], sign), (p0[ax], -sign)):
                    into.append(Prim("rect", (ax, np.array([p0[a0], p1[a0]]), np.array([p0[a1], p1[a1]]), float(kk)), m, chain, s))
        elif k == "flip":
            walk(r[1], chain, -sign, into)
        elif k in ("translate", "scale", "rotate", "move"):
            walk(r[2], chain + ((k, r[1]),), sign, into)
        elif k == "and":
            walk(r[1], chain, sign, into)
            walk(r[2], chain, sign, into)
        elif k == "bvh":
            for c in r[1]:
                walk(c, chain, sign, into)
        elif k == "medium":
            if media is None or chain:
                raise ValueError("a ConstantMedium is not part of the closest-hit evaluator")
            inner = []
            walk(r[1], chain, sign, inner)
            media.append((inner, r[2], r[3]))
        else:
            raise ValueError(k)

    for o in world:
        walk(o, (), 1, out)
    return out


def _rot(v, theta):
    """A point or vector turned by theta about +y: (x, y, z) -> (c x + s z, y, -s x + c z)."""
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([c * v[:, 0] + s * v[:, 2], v[:, 1], -s * v[:, 0] + c * v[:, 2]], axis=1)


def _theta(deg, fault):
    return np.deg2rad(-deg if fault == "rotate_neg" else deg)


def _to_local(chain, o, d, time, fault=None):
    for k, a in chain:
        if k == "translate":
            o = o - a
        elif k == "scale":
            o, d = o / a, d / a
        elif k == "rotate":
            o, d = _rot(o, -_theta(a, fault)), _rot(d, -_theta(a, fault))
        else:
            o = o - time[:, None] * a
    return o, d


def _to_world(chain, p, n, fault=None):
    for k, a in reversed(chain):
        if k == "translate":
            p = p + a
        elif k == "scale":
            p, n = p * a, (n * a if fault == "scale_normal" else n / a)
        elif k == "rotate":
            p, n = _rot(p, _theta(a, fault)), _rot(n, _theta(a, fault))
    return p, n


def point_to_world(chain, q, time):
    """Where the local point q of a primitive under `chain` is in the world at `time` (for aiming rays)."""
    for k, a in reversed(chain):
        if k == "translate":
            q = q + a
        elif k == "scale":
            q = q * a
        elif k == "rotate":
            q = _rot(q, np.deg2rad(a))
        else:
            q = q + time[:, None] * a
    return q


def _dot(a, b):
    return (a * b).sum(axis=1)


def _rect_centre(pr):
    ax, r0, r1, k = pr.params
    a0, a1 = [a for a in range(3) if a != ax]
    q = np.zeros((1, 3))
    q[0, ax], q[0, a0], q[0, a1] = k, 0.5 * (r0[0] + r0[1]), 0.5 * (r1[0] + r1[1])
    return q


def _centre(pr):
    if pr.kind == "sphere":
        return np.zeros((1, 3))
    if pr.kind == "tri":
        return ((pr.params[0] + pr.params[1] + pr.params[2]) / 3.0)[None, :]
    return _rect_centre(pr)


def closest_hit(prims, o, d, time, t_near=T_NEAR, fault=None, roots=True):
    """The closest hit of the rays (o, d, time: float64 [n, 3], [n, 3], [n]) with `prims`: a dict of hit (bool), t, p, n,
    material (uint32 handle), prim (the index of the winning primitive in `prims`, -1 on a miss) and margin (the conditioning
    margin of the docstring).  roots=False leaves the roots' distance
    from t_near out of the margin: a ray that starts ON a surface has a root at 0, t_near away from t_near by construction."""
    o, d, time = np.asarray(o, F), np.asarray(d, F), np.asarray(time, F)
    n = len(o)
    inf = np.full(n, np.inf)
    best, second = inf.copy(), inf.copy()
    bp, bn, bm, bi = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.uint32), np.full(n, -1, np.int64)
    dlen = np.sqrt(_dot(d, d))
    size = np.maximum(1.0, np.sqrt(_dot(o, o)))
    seen = []
    with np.errstate(all="ignore"):
        for number, pr in enumerate(prims):
            lo, ld = _to_local(pr.chain, o, d, time, fault)
            if pr.kind == "sphere":
                r = pr.params[0]
                a, b, c = _dot(ld, ld), _dot(lo, ld), _dot(lo, lo) - r * r
                disc = b * b - a * c
                ok = disc > 0
                sq = np.sqrt(np.where(ok, disc, 0.0))
                t0, t1 = (-b - sq) / a, (-b + sq) / a
                t = np.where(ok & (t0 >= t_near), t0, np.where(ok & (t1 >= t_near), t1, np.inf))
                m = np.abs(disc) / (b * b + a * np.abs(c))
                rootm = np.minimum(np.abs(t0 - t_near), np.abs(t1 - t_near)) * dlen / size if roots else np.inf
                m = np.where(ok, np.minimum(m, rootm), m)
                front = np.where(ok, t0, -b / a)
                front = np.where(np.where(ok, t1, -b / a) * dlen / size > -1e-3, front, np.inf)   # (wholly behind the origin)
                ts = np.where(np.isfinite(t), t, 0.0)
                pl = lo + ts[:, None] * ld
                nl = pl / r
            elif pr.kind == "tri":
                # the plane crossing t = n.(v0 - o) / n.d with n = e1 x e2, barycentrics by Cramer's rule on the Gram matrix of
                # (e1, e2), inclusive edges.  Margin: the barycentric distances |u|, |v|, |1 - u - v|; |n.d| / (|e1| |e2| |d|);
                # the crossing's distance from t_near (alone, when the crossing is behind the origin)
                v0, e1, e2 = pr.params[0], pr.params[1] - pr.params[0], pr.params[2] - pr.params[0]
                nn = np.cross(e1, e2)
                den = ld @ nn
                tt = ((v0 - lo) @ nn) / den
                ts = np.where(np.isfinite(tt), tt, 0.0)
                q = lo + ts[:, None] * ld - v0
                a11, a12, a22 = e1 @ e1, e1 @ e2, e2 @ e2
                b1, b2 = q @ e1, q @ e2
                gram = a11 * a22 - a12 * a12
                u, v = (b1 * a22 - b2 * a12) / gram, (b2 * a11 - b1 * a12) / gram
                inside = (u >= 0) & (v >= 0) & (u + v <= 1)
                t = np.where(np.isfinite(tt) & (tt >= t_near) & inside, tt, np.inf)
                bary = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(1.0 - u - v))
                detm = np.abs(den) / (np.sqrt(a11) * np.sqrt(a22) * np.sqrt(_dot(ld, ld)))
                rootm = np.abs(tt - t_near) * dlen / size if roots else inf
                m = np.where(np.isfinite(tt), np.where(tt >= 0, np.minimum(np.minimum(bary, detm), rootm), rootm), detm)
                front = np.where(np.isfinite(tt), tt, -np.inf)
                pl = lo + ts[:, None] * ld
                nl = np.broadcast_to(nn / np.sqrt(nn @ nn), (n, 3))
            else:
                ax, r0, r1, k = pr.params
                a0, a1 = [i for i in range(3) if i != ax]
                tt = (k - lo[:, ax]) / ld[:, ax]
                ts = np.where(np.isfinite(tt), tt, 0.0)
                x, y = lo[:, a0] + ts * ld[:, a0], lo[:, a1] + ts * ld[:, a1]
                inside = (x >= r0[0]) & (x < r0[1]) & (y >= r1[0]) & (y < r1[1])
                t = np.where(np.isfinite(tt) & (tt >= t_near) & inside, tt, np.inf)
                edge = np.minimum(np.minimum(np.abs(x - r0[0]), np.abs(x - r0[1])) / (r0[1] - r0[0]),
                                  np.minimum(np.abs(y - r1[0]), np.abs(y - r1[1])) / (r1[1] - r1[0]))
                rootm = np.abs(tt - t_near) * dlen / size if roots else inf
                m = np.where(np.isfinite(tt), np.where(tt >= 0, np.minimum(edge, rootm), rootm), np.inf)
                front = np.where(np.isfinite(tt), tt, np.inf)
                pl = lo + ts[:, None] * ld
                nl = np.zeros((n, 3))
                nl[:, ax] = 1.0
            pw, nw = _to_world(pr.chain, pl, pr.sign * nl, fault)
            better = t < best
            second = np.where(better, best, np.minimum(second, t))
            best = np.where(better, t, best)
            bp[better], bn[better], bm[better], bi[better] = pw[better], nw[better], pr.material, number
            seen.append((front, m))
        hit = np.isfinite(best)
        margin = np.where(np.isfinite(second), (second - best) / np.abs(best), np.inf)
        for front, m in seen:
            margin = np.where(front <= best, np.minimum(margin, m), margin)
    return {"hit": hit, "t": np.where(hit, best, 0.0), "p": bp, "n": bn, "material": bm, "prim": bi, "margin": margin}


def aimed_rays(prims, n, seed, origin_box=None, near=None):
    """n seeded rays (float64 [n, 7]: origin, direction, time) aimed at the primitives: the origin sits inside or outside one
    primitive, the target on or just beside another (or the same), the direction is un-normalised with a length of 0.1 .. 10
    (log-uniform), the time uniform in [0, 1).  origin_box (lo, hi): origins are clipped into it.  near: the other primitive is
    one whose centre lies within that distance of the first one's."""
    rs = np.random.RandomState(seed)
    time = rs.uniform(0.0, 1.0, n)

    def unit(k):
        v = rs.normal(size=(k, 3))
        return v / np.sqrt(_dot(v, v))[:, None]

    def around(which, spread, target=False):
        out = np.zeros((n, 3))
        for i in np.unique(which):
            at = which == i
            k, pr = int(at.sum()), prims[i]
            if pr.kind == "sphere":
                q = pr.params[0] * spread(k)[:, None] * unit(k)
            elif pr.kind == "tri":
                # a target: the point of the plane with barycentrics from -0.1 .. 1.1 (u, v drawn; a pair beyond the third edge
                # is mirrored back, so that about a sixth of the targets lie just outside an edge); an origin: such a point moved
                # off the plane by 0.05 .. 3.05 times the triangle's size, to either side
                v0, e1, e2 = pr.params[0], pr.params[1] - pr.params[0], pr.params[2] - pr.params[0]
                u, v = rs.uniform(-0.1, 1.1, k), rs.uniform(-0.1, 1.1, k)
                over = u + v > 1.1
                u, v = np.where(over, 1.0 - u, u), np.where(over, 1.0 - v, v)
                q = v0 + u[:, None] * e1 + v[:, None] * e2
                if not target:
                    nn = np.cross(e1, e2)
                    off = 0.5 * (np.sqrt(e1 @ e1) + np.sqrt(e2 @ e2)) * (0.05 + spread(k)) * rs.choice([-1.0, 1.0], k)
                    q = q + off[:, None] * (nn / np.sqrt(nn @ nn))
            else:
                ax, r0, r1, kk = pr.params
                a0, a1 = [a for a in range(3) if a != ax]
                e0, e1 = r0[1] - r0[0], r1[1] - r1[0]
                q = np.zeros((k, 3))
                q[:, a0] = r0[0] + e0 * rs.uniform(-0.1, 1.1, k)
                q[:, a1] = r1[0] + e1 * rs.uniform(-0.1, 1.1, k)
                q[:, ax] = kk + 0.5 * (e0 + e1) * (spread(k) - 1.0) * rs.choice([-1.0, 1.0], k)
            out[at] = point_to_world(pr.chain, q, time[at])
        return out

    src = rs.randint(0, len(prims), n)
    dst = np.where(rs.uniform(size=n) < 0.5, src, rs.randint(0, len(prims), n))
    if near is not None:
        zero = np.zeros(1)
        centre = np.array([point_to_world(pr.chain, _centre(pr), zero)[0] for pr in prims])
        for i in np.unique(src):
            close = np.nonzero(np.sqrt(((centre - centre[i]) ** 2).sum(axis=1)) <= near)[0]
            at = (src == i) & (dst != src)
            dst[at] = close[rs.randint(0, len(close), int(at.sum()))]
    origin = around(src, lambda k: rs.uniform(0.0, 3.0, k))          # < 1: inside a sphere, > 1: outside
    target = around(dst, lambda k: rs.uniform(0.0, 1.15, k) ** 0.5, target=True)  # spheres: a chord, sometimes a near miss
    if origin_box is not None:
        origin = np.clip(origin, np.array(origin_box[0], F), np.array(origin_box[1], F))
    d = target - origin
    d *= (10.0 ** rs.uniform(-1.0, 1.0, n) / np.sqrt(_dot(d, d)))[:, None]
    return np.concatenate([origin, d, time[:, None]], axis=1)


def compare_hits(ref, out, mat, threshold=MARGIN):
    """The float64 hits `ref` (closest_hit) against debug_hit_top's (out [n, 8] float32, mat [n]): a dict of the share left out,
    the mismatch counts and the worst deviations among the rays whose margin exceeds `threshold`."""
    use = ref["margin"] > threshold
    hit = out[:, 0] != 0
    both = use & hit & ref["hit"]
    o64 = out.astype(F)
    plen = np.maximum(1.0, np.sqrt(_dot(ref["p"], ref["p"])))
    res = {"left_out": 1.0 - use.mean(), "compared": int(use.sum()), "hits": int(both.sum()),
           "flag_mismatch": int((use & (hit != ref["hit"])).sum()),
           "material_mismatch": int((both & (mat != ref["material"])).sum()), "dt": 0.0, "dp": 0.0, "dn": 0.0}
    if both.any():
        res["dt"] = float((np.abs(o64[both, 1] - ref["t"][both]) / np.abs(ref["t"][both])).max())
        res["dp"] = float((np.abs(o64[both, 2:5] - ref["p"][both]).max(axis=1) / plen[both]).max())
        res["dn"] = float(np.abs(o64[both, 5:8] - ref["n"][both]).max())
    return res


def assert_hits(res, what, cap=CAP_RAYS):
    print("%-14s left out %5.2f %%  compared %5d (%5d hits)  dt %.2e  dp %.2e  dn %.2e" % (
        what, 100 * res["left_out"], res["compared"], res["hits"], res["dt"], res["dp"], res["dn"]))
    assert res["left_out"] <= cap, (what, res)
    assert res["hits"] >= res["compared"] // 4, (what, "the rays hardly hit anything", res)
    assert res["flag_mismatch"] == 0 and res["material_mismatch"] == 0, (what, res)
    assert res["dt"] <= TOL_T and res["dp"] <= TOL_P and res["dn"] <= TOL_N, (what, res)


# hand-built graphs ----------------------------------------------------------------------------------------------------------
def _mats(S, b):
    """A palette of distinguishable materials (constant and checker textures only): the handle is part of every comparison."""
    chk = b.checker(b.constant(S.v(0.2, 0.3, 0.1)), b.constant(S.vfrom(0.9)))
    chk2 = b.checker(b.constant(S.v(0.9, 0.1, 0.1)), b.checker(b.constant(S.v(0.1, 0.1, 0.9)), b.constant(S.vfrom(0.5))))
    return [b.lambertian(b.constant(S.v(0.7, 0.3, 0.2))), b.lambertian(chk), b.metal(S.v(0.8, 0.85, 0.88), 0.3), b.dielectric(1.5),
            b.diffuse_light(b.constant(S.v(0.5, 1.0, 0.25)), 2.0), b.lambertian(chk2), b.isotropic(b.constant(S.v(0.1, 0.6, 0.4))),
            b.diffuse_light(chk, 3.0)]


def graph_nest3(S, b):
    """Wrappers three and four deep over spheres and a prism, in a list."""
    m = _mats(S, b)
    return [b.translate(S.v(-2.0, 0.5, 0.0), b.rotate_y(30.0, b.scale(S.v(1.0, 2.0, 0.5), b.sphere(1.0, m[0])))),
            b.flip_normals(b.translate(S.v(2.0, -1.0, 1.0), b.rotate_y(-40.0, b.rect_prism(S.v(-1.0, -0.5, -0.75), S.v(1.0, 0.5, 0.75), m[1])))),
            b.linear_move(b.translate(S.v(0.0, 2.5, -1.0), b.scale(S.v(0.5, 0.5, 2.0), b.sphere(1.5, m[2]))), S.v(0.5, -0.25, 0.0)),
            b.scale(S.v(2.0, 1.0, 1.0), b.rotate_y(75.0, b.translate(S.v(0.0, -2.5, 0.0), b.flip_normals(b.sphere(0.8, m[3]))))),
            b.rect(S.Y, (-6.0, 6.0), (-6.0, 6.0), -4.0, m[5])]


def graph_bvh_leaves(S, b):
    """Every wrapper as a leaf of one Bvh."""
    m = _mats(S, b)
    leaves = [b.translate(S.v(2.0 * (i % 4) - 3.0, 0.7 * (i // 4) - 1.0, 1.5 * (i % 3) - 1.5), b.sphere(0.45 + 0.05 * i, m[i % 8])) for i in range(8)]
    leaves += [b.rotate_y(20.0, b.translate(S.v(0.0, 2.5, 0.0), b.rect_prism(S.v(-1.0, -0.3, -1.0), S.v(1.0, 0.3, 1.0), m[1]))),
               b.scale(S.v(1.5, 0.5, 1.0), b.translate(S.v(0.0, -5.0, 2.0), b.sphere(0.8, m[5]))),
               b.flip_normals(b.sphere(12.0, m[4])),
               b.linear_move(b.translate(S.v(-3.0, 3.0, -2.0), b.sphere(0.6, m[0])), S.v(0.0, 0.0, 1.0)),
               b.and_(b.rect(S.X, (-1.0, 1.0), (-1.0, 1.0), 4.5, m[2]), b.flip_normals(b.rect(S.Z, (-2.0, 2.0), (-1.0, 1.0), -4.0, m[7])))]
    return [b.bvh(leaves, (0.0, 1.0))]


def graph_rects(S, b):
    """Rects on all three axes, plain, flipped, under And and under every wrapper."""
    m = _mats(S, b)
    return [b.rect(S.X, (-1.0, 1.0), (-2.0, 2.0), -3.0, m[0]), b.flip_normals(b.rect(S.X, (-1.5, 1.0), (-2.0, 1.0), 3.0, m[1])),
            b.rect(S.Y, (-3.0, 3.0), (-3.0, 3.0), -2.5, m[5]), b.flip_normals(b.rect(S.Y, (-2.0, 2.0), (-2.0, 2.0), 2.5, m[4])),
            b.and_(b.rect(S.Z, (-1.0, 0.0), (-1.0, 1.0), -2.0, m[2]), b.and_(b.rect(S.Z, (0.0, 1.0), (-1.0, 1.0), -2.25, m[3]),
                                                                          b.flip_normals(b.rect(S.Z, (-2.0, 2.0), (-2.0, 2.0), 3.5, m[6])))),
            b.translate(S.v(0.5, 0.25, 0.0), b.rotate_y(45.0, b.rect(S.Z, (-1.0, 1.0), (-1.0, 1.0), 0.0, m[7]))),
            b.scale(S.v(0.5, 2.0, 1.0), b.rect(S.X, (-0.5, 0.5), (-1.0, 1.0), 1.0, m[1])),
            b.rotate_y(-30.0, b.scale(S.v(1.0, 1.0, 3.0), b.translate(S.v(0.0, 1.0, 0.0), b.rect(S.Y, (-1.0, 1.0), (-0.3, 0.3), 0.0, m[0]))))]


def graph_moving(S, b):
    """LinearMove above and below the other wrappers."""
    m = _mats(S, b)
    return [b.linear_move(b.translate(S.v(-2.0, 0.0, 0.0), b.sphere(1.0, m[0])), S.v(0.0, 1.0, 0.0)),
            b.translate(S.v(2.0, 0.0, 0.0), b.linear_move(b.sphere(1.0, m[1]), S.v(0.0, -1.0, 0.5))),
            b.linear_move(b.rotate_y(35.0, b.rect_prism(S.v(-0.5, -3.0, -0.5), S.v(0.5, -2.0, 0.5), m[2])), S.v(1.0, 0.0, 0.0)),
            b.scale(S.v(1.0, 0.5, 1.0), b.linear_move(b.translate(S.v(0.0, 5.0, 0.0), b.sphere(0.7, m[5])), S.v(0.0, 0.0, -1.5))),
            b.flip_normals(b.sphere(9.0, m[4]))]


def graph_deep(S, b):
    """One object five wrappers deep (with an And of a sphere and a prism at the bottom) inside a dome."""
    m = _mats(S, b)
    inner = b.and_(b.sphere(1.0, m[0]), b.translate(S.v(1.5, 0.0, 0.0), b.rect_prism(S.v(-0.5, -0.5, -0.5), S.v(0.5, 0.5, 0.5), m[1])))
    deep = b.translate(S.v(0.5, 0.5, 0.0), b.scale(S.v(1.5, 1.0, 0.75), b.rotate_y(-25.0, b.translate(S.v(0.0, -0.5, 0.5), b.flip_normals(inner)))))
    return [deep, b.translate(S.v(-3.0, 0.0, 0.0), b.scale(S.v(0.5, 1.5, 0.5), b.sphere(1.0, m[5]))),
            b.flip_normals(b.sphere(10.0, m[7]))]


def graph_wrapped_bvh(S, b):
    """Bvhs below Translate{RotateY} and below Scale, beside plain list items."""
    m = _mats(S, b)
    one = [b.translate(S.v(1.2 * i - 2.4, 0.3 * i, 0.5 * (i % 2)), b.sphere(0.5, m[i % 8])) for i in range(5)]
    one.append(b.rect_prism(S.v(-2.0, -1.5, -1.0), S.v(2.0, -1.0, 1.0), m[5]))
    two = [b.translate(S.v(0.0, 1.0 * i, 0.0), b.sphere(0.4, m[(i + 3) % 8])) for i in range(3)]
    two.append(b.rotate_y(10.0, b.rect(S.Z, (-1.0, 1.0), (0.0, 2.0), 0.8, m[2])))
    return [b.translate(S.v(0.0, 0.0, -1.0), b.rotate_y(25.0, b.bvh(one, (0.0, 1.0)))),
            b.scale(S.v(1.0, 1.5, 1.0), b.translate(S.v(3.5, -1.0, 1.0), b.bvh(two, (0.0, 1.0)))),
            b.translate(S.v(-4.0, 1.0, 1.0), b.sphere(0.9, m[1])), b.rect(S.Y, (-6.0, 6.0), (-6.0, 6.0), -3.0, m[0])]


GRAPHS = {"nest3": graph_nest3, "bvh_leaves": graph_bvh_leaves, "rects": graph_rects, "moving": graph_moving, "deep": graph_deep,
          "wrapped_bvh": graph_wrapped_bvh}
CASE_SCENES = ("cornell", "book1", "checker_scale", "motion")
HIT_SCENES = tuple(GRAPHS) + CASE_SCENES
# where the rays of a scene case start: inside the Cornell room (its prisms stand ON the floor: from below, the floor and a
# prism's bottom face are one surface with two materials), and in the air over book 1's ground (a sphere of radius 1000:
# origins thousands of units away see its 0.2-unit spheres at a relative discriminant of 1e-8)
ORIGIN_BOX = {"cornell": ((2.0, 2.0, 2.0), (552.0, 552.0, 552.0)), "book1": ((-15.0, 0.05, -15.0), (15.0, 8.0, 15.0))}
NEAR = {"book1": 2.0}   # (a ray from one small sphere's side goes to a neighbour, not to one 20 units away)
FEATURE_GRAPHS = ("nest3", "bvh_leaves", "wrapped_bvh")


def build_graph(pkg, be, name, nx=24, ny=16):
    """(recorder, world, camera) of a hand-built graph or of a scene case, on backend `be`."""
    rec = Recorder(be.builder())
    if name in GRAPHS:
        S = pkg.scenes
        world = GRAPHS[name](S, rec)
        cam = be.camera_look(S.v(1.0, 2.0, 11.0), S.v(0.0, 0.0, 0.0), S.v(0.0, 1.0, 0.0), 40.0, float(f32(nx) / f32(ny)), 0.0, 1.0, (0.0, 1.0))
    else:
        from scene_cases import CASES
        world, cam, _ = CASES[name][0](pkg, rec, nx, ny)
    return rec, world, cam


_hit_refs = {}


def hit_reference(pkg, be, name, n=4096, fault=None):
    """(scene on `be`, rays float32 [n, 7], float64 hits of those rays) for a scene of A; the rays and the float64 hits are
    computed once per scene and shared (callers must not write them)."""
    rec, world, _ = build_graph(pkg, be, name)
    key = (name, n, fault)
    if key not in _hit_refs:
        prims = primitives(rec, world)
        rays = aimed_rays(prims, n, 1000 + sorted(HIT_SCENES).index(name), ORIGIN_BOX.get(name), NEAR.get(name)).astype(f32)   # (the library gets float32 rays: so does the reference)
        r64 = rays.astype(F)
        _hit_refs[key] = (rays, closest_hit(prims, r64[:, 0:3], r64[:, 3:6], r64[:, 6], fault=fault))
    return (rec.scene(world),) + _hit_refs[key]


def check_hits(pkg, be, name, fault=None):
    """A: debug_hit_top of backend `be` against the float64 closest hit, on the 4096 rays of scene `name`."""
    scene, rays, ref = hit_reference(pkg, be, name, fault=fault)
    out, mat = scene.debug_hit_top(rays, seed=7, t_near=T_NEAR)
    res = compare_hits(ref, out, mat)
    assert_hits(res, name)
    return res


# feature planes ------------------------------------------------------------------------------------------------------------
def texture_value3(rec, tex, p, fault=None):
    """(value [n, 3], eps [n], allowance [n]) of a constant / checker / image texture at the points p.  eps is the "leave the
    pixel out when eps <= TOL_P" figure: the smallest |sin sin sin| met on the way and, for a nearest-filtered image, TOL_P times
    the ratio of the sampler's margin (texels to the next texel change) to what can move (x, y): the position tolerance
    TOL_P max(1, |p|) through image_ref.texel_shift, plus image_ref.NEAREST_MARGIN.  allowance is what a bilinear image's value
    may deviate by: image_ref.bilinear_allowance for that position tolerance (derived: slope times shift) plus the measured
    BILINEAR_TOL of the image's size."""
    import image_ref as IR
    r = rec.textures[tex]
    none, zero = np.full(len(p), np.inf), np.zeros(len(p))
    if r[0] == "constant":
        return np.broadcast_to(r[1], p.shape).copy(), none, zero
    if r[0] == "image":
        img, prm = r[1], r[2]
        h, w = img.shape[0], img.shape[1]
        val, margin = IR.sample64(img, prm, p, fault=fault)
        dp = TOL_P * np.maximum(1.0, np.sqrt(_dot(p, p)))
        if prm["filter"] == IR.NEAREST:
            dx, dy = IR.texel_shift(prm, w, h, p, dp)
            return val, TOL_P * margin / (np.maximum(dx, dy) + IR.NEAREST_MARGIN), zero
        return val, none, IR.bilinear_allowance(img, prm, p, dp) + IR.BILINEAR_TOL[(w, h)]
    if r[0] != "checker":
        raise ValueError("only constant, checker and image textures have a closed form here")
    s = np.sin(10.0 * p).prod(axis=1)
    v0, e0, a0 = texture_value3(rec, r[1], p, fault)
    v1, e1, a1 = texture_value3(rec, r[2], p, fault)
    odd = s < 0
    return np.where(odd[:, None], v1, v0), np.minimum(np.abs(s), np.where(odd, e1, e0)), np.where(odd, a1, a0)


def texture_value(rec, tex, p):
    """(value [n, 3], the smallest eps met on the way [n]) of a constant / checker / image texture at the points p."""
    return texture_value3(rec, tex, p)[0:2]


def albedo_value3(rec, mats, p, hit=None, fault=None):
    """What the feature pass calls the albedo: Lambertian / Isotropic the texture, Metal its colour, Dielectric 1,
    DiffuseLight brightness * texture -- with eps and the allowance of texture_value3 (a light's times its brightness)."""
    out, eps, allow = np.zeros((len(p), 3)), np.full(len(p), np.inf), np.zeros(len(p))
    hit = np.ones(len(p), bool) if hit is None else hit
    for m in np.unique(mats[hit]):
        at = hit & (mats == m)
        r = rec.materials[int(m)]
        if r[0] == "metal":
            out[at] = r[1]
        elif r[0] == "dielectric":
            out[at] = 1.0
        else:
            v, e, a = texture_value3(rec, r[1], p[at], fault)
            out[at], eps[at], allow[at] = (r[2] * v if r[0] == "light" else v), e, (r[2] * a if r[0] == "light" else a)
    return out, eps, allow


def albedo_value(rec, mats, p, hit=None):
    return albedo_value3(rec, mats, p, hit)[0:2]


def feature_reference(rec, world, cam, nx, ny, grid, fault=None, allowance=False, image_fault=None):
    """The albedo / normal / depth planes of RTG_FLAG_FEATURES in float64 from the camera block: (planes [ny, nx, 7], usable
    [ny, nx]).  Rays: pixel (x, row), y = ny - 1 - row, cell centres (i + 0.5) / g of a g x g grid, from the camera origin, at
    mid exposure; a plane is the mean over the g * g rays, a miss counting as zero.  allowance=True: also the albedo allowance
    per pixel [ny, nx] (the mean of the rays' allowances of texture_value3) and, per pixel, whether a ray met an image texture on
    a triangle."""
    prims = primitives(rec, world)
    v3 = lambda a: np.array([a[0], a[1], a[2]], dtype=F)
    origin, llc, hor, ver = v3(cam.origin), v3(cam.lower_left_corner), v3(cam.horizontal), v3(cam.vertical)
    time = float(cam.exposure_start) + 0.5 * (float(cam.exposure_end) - float(cam.exposure_start))
    x, row = np.meshgrid(np.arange(nx, dtype=F), np.arange(ny, dtype=F))
    y = ny - 1 - row
    acc, usable, allow, on_tri = np.zeros((ny * nx, 7)), np.ones(ny * nx, bool), np.zeros(ny * nx), np.zeros(ny * nx, bool)
    kinds = np.array([pr.kind == "tri" for pr in prims] + [False])
    for j in range(grid):
        for i in range(grid):
            u, v = ((x + (i + 0.5) / grid) / nx).ravel(), ((y + (j + 0.5) / grid) / ny).ravel()
            d = llc + u[:, None] * hor + v[:, None] * ver - origin
            h = closest_hit(prims, np.broadcast_to(origin, d.shape), d, np.full(len(d), time), fault=fault)
            hit = h["hit"]
            alb, eps, alw = albedo_value3(rec, h["material"], h["p"], hit, image_fault)
            usable &= h["margin"] > MARGIN
            usable &= ~hit | (eps > TOL_P)
            acc += np.where(hit[:, None], np.concatenate([alb, h["n"], h["t"][:, None]], axis=1), 0.0)
            allow += np.where(hit, alw, 0.0)
            on_tri |= hit & kinds[h["prim"]] & _shows_image(rec, h["material"], hit)
    planes, usable = (acc / (grid * grid)).reshape(ny, nx, 7), usable.reshape(ny, nx)
    if allowance:
        return planes, usable, (allow / (grid * grid)).reshape(ny, nx), on_tri.reshape(ny, nx)
    return planes, usable


def _has_image(rec, tex):
    r = rec.textures[tex]
    return r[0] == "image" or (r[0] == "checker" and (_has_image(rec, r[1]) or _has_image(rec, r[2])))


def _shows_image(rec, mats, hit):
    """per ray: the material's texture is an image or a checker that holds one"""
    out = np.zeros(len(mats), bool)
    for m in np.unique(mats[hit]):
        r = rec.materials[int(m)]
        if r[0] in ("lambertian", "isotropic", "light") and _has_image(rec, r[1]):
            out |= hit & (mats == m)
    return out


def compare_planes(ref, usable, albedo, normal, depth, what, allow=None):
    """allow [ny, nx]: the albedo allowance per pixel of feature_reference (image textures), beyond TOL_N"""
    da = np.abs(albedo.astype(F) - ref[..., 0:3])
    da = float((da if allow is None else np.maximum(da - allow[..., None], 0.0))[usable].max())
    dn = float(np.abs(normal.astype(F) - ref[..., 3:6])[usable].max())
    z = ref[..., 6]
    dz = float((np.abs(depth.astype(F) - z) / np.where(z > 0, z, 1.0))[usable].max())
    left = 1.0 - usable.mean()
    print("%-18s left out %5.2f %% of the pixels  albedo %.2e  normal %.2e  depth %.2e (hit pixels: %d)" % (
        what, 100 * left, da, dn, dz, int((z > 0).sum())))
    assert left <= CAP_PIXELS, (what, left)
    assert (z > 0).mean() > 0.25, (what, "the frame is mostly sky")
    assert da <= TOL_N and dn <= TOL_N and dz <= TOL_T, (what, da, dn, dz)


def planes_from_hit_top(scene, cam, nx, ny, grid, rec_albedo):
    """The planes as the header defines them, put together from debug_hit_top of any backend (float32 rays built the header's
    way, float32 fold): what a backend without RTG_FLAG_FEATURES can be asked for.  rec_albedo(mat, p, hit) -> float albedo."""
    v3 = lambda a: np.array([a[0], a[1], a[2]], dtype=f32)
    origin, llc, hor, ver = v3(cam.origin), v3(cam.lower_left_corner), v3(cam.horizontal), v3(cam.vertical)
    time = f32(f32(cam.exposure_start) + f32(f32(0.5) * f32(f32(cam.exposure_end) - f32(cam.exposure_start))))
    x, row = np.meshgrid(np.arange(nx).astype(f32), np.arange(ny).astype(f32))
    y = (f32(ny - 1) - row).astype(f32)
    acc = np.zeros((ny * nx, 7), f32)
    for j in range(grid):
        for i in range(grid):
            su, sv = f32(f32(i + 0.5) / f32(grid)), f32(f32(j + 0.5) / f32(grid))
            u, v = ((x + su).astype(f32) / f32(nx)).astype(f32).ravel(), ((y + sv).astype(f32) / f32(ny)).astype(f32).ravel()
            d = (((llc + u[:, None] * hor).astype(f32) + (v[:, None] * ver).astype(f32)).astype(f32) - origin).astype(f32)
            rays = np.concatenate([np.broadcast_to(origin, d.shape), d, np.full((len(d), 1), time, f32)], axis=1).astype(f32)
            order = (y.ravel().astype(np.int64) * nx + x.ravel().astype(np.int64)).argsort()   # ray index = y * nx + x
            out, mat = scene.debug_hit_top(rays[order], seed=0xDEADBEEF, t_near=T_NEAR)
            back = np.empty_like(order)
            back[order] = np.arange(len(order))
            out, mat = out[back], mat[back]
            hit = out[:, 0] != 0
            vals = np.concatenate([rec_albedo(mat, out[:, 2:5].astype(F), hit).astype(f32), out[:, 5:8], out[:, 1:2]], axis=1)
            acc = (acc + np.where(hit[:, None], vals, f32(0))).astype(f32)
    acc = (acc / f32(grid * grid)).astype(f32).reshape(ny, nx, 7)
    return acc[..., 0:3], acc[..., 3:6], acc[..., 6]


def check_feature_planes(pkg, be, name, grid, fault=None, nx=24, ny=16):
    """A, second kernel: the normal, depth and albedo planes of a 24 x 16 frame against float64.  A backend that implements
    RTG_FLAG_FEATURES is asked for the frame; any other one for the same rays through debug_hit_top."""
    rec, world, cam = build_graph(pkg, be, name, nx, ny)
    ref, usable = feature_reference(rec, world, cam, nx, ny, grid, fault=fault)
    scene = rec.scene(world)
    if be.prefix == "rtg_":
        fr = scene.par_cast(cam, nx, ny, 1, features={"grid": grid})
        planes = (fr.albedo, fr.normal, fr.depth)
    else:
        planes = planes_from_hit_top(scene, cam, nx, ny, grid, lambda mat, p, hit: albedo_value(rec, mat, p, hit)[0])
    compare_planes(ref, usable, *planes, what="%s grid %d" % (name, grid))


# ---------------------------------------------------------------------------------------------------------------------------
# B. exact radiance
# ---------------------------------------------------------------------------------------------------------------------------
L_EMIT = (1.0, 0.5, 0.25)


def radiance_world(pkg, b, kind, metal=False):
    """kind "lean": spheres under one Bvh inside a flipped emitter sphere.  kind "list": rects, a prism and a Bvh of spheres
    in a box of six emitter rects (a world the second flat program takes).  Every non-emitter has albedo 0.5 (Lambertian, or
    metal(0.5, 0.4) with metal=True), the emitter radiates L_EMIT."""
    S = pkg.scenes
    grey = b.lambertian(b.constant(S.vfrom(0.5)))
    shiny = b.metal(S.vfrom(0.5), 0.4) if metal else grey
    light = b.diffuse_light(b.constant(S.v(*L_EMIT)), 1.0)
    balls = [b.translate(S.v(0.0, -100.5, -1.0), b.sphere(100.0, grey)), b.translate(S.v(0.0, 0.0, -1.0), b.sphere(0.5, shiny)),
             b.translate(S.v(1.0, 0.0, -1.0), b.sphere(0.5, shiny)), b.translate(S.v(-1.0, 0.25, -1.5), b.sphere(0.75, grey))]
    if kind == "lean":
        world = [b.bvh(balls + [b.flip_normals(b.sphere(50.0, light))], (0.0, 1.0))]
    else:
        box = [b.rect(ax, (-8.0, 8.0), (-8.0, 8.0), k, light) for ax in (S.X, S.Y, S.Z) for k in (-8.0, 8.0)]
        world = box + [b.rect(S.Y, (-4.0, 4.0), (-4.0, 4.0), -0.5, grey), b.rect_prism(S.v(-2.5, -0.5, -2.5), S.v(-1.5, 1.0, -1.5), shiny),
                       b.rect(S.X, (-0.5, 2.0), (-3.0, 0.0), 2.0, shiny), b.bvh(balls[1:], (0.0, 1.0))]
    cam = b.be.camera_look(S.v(-2, 2, 1), S.v(0, 0, -1), S.v(0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 1.0)
    return world, cam


def check_exact_radiance(pkg, be, kind, metal=False, options=(), trace_kernel=False, need_pool2=False, nx=48, ny=32, ns=8, max_bounces=50):
    """B: every sample of the full key grid is exactly 0.5^bounces * L (or exactly zero: a path stopped at the bounce cap, a
    metal that absorbed), and the frame is the ordered float32 fold of its samples."""
    b = be.builder()
    world, cam = radiance_world(pkg, b, kind, metal)
    if need_pool2:
        assert len(b.flatten_pool2(world)[0]) != 0, "the list world must have a second program"
    scene = b.scene(world)
    for k, v in options:
        scene.set_option(k, v)
    ys, xs, ss = (a.ravel().astype(np.uint32) for a in np.meshgrid(np.arange(ny), np.arange(nx), np.arange(ns), indexing="ij"))
    rgb, info = scene.debug_samples(cam, nx, ny, ns, xs, ys, ss, trace_kernel=trace_kernel, max_bounces=max_bounces)
    k = info[:, 0].astype(np.int64)
    want = (np.ldexp(1.0, -k)[:, None] * np.array(L_EMIT)).astype(f32)
    assert (want.astype(F) == np.ldexp(1.0, -k)[:, None] * np.array(L_EMIT)).all()      # (exact in float32)
    lit = (rgb == want).all(axis=1)
    black = (rgb.view(np.uint32) == 0).all(axis=1)
    dark_ok = black if metal else black & (k >= max_bounces)
    print("%s metal=%s %s: %d samples, bounces %d .. %d, %d black" % (kind, metal, dict(options), len(k), k.min(), k.max(), black.sum()))
    bad = ~(lit | dark_ok)
    assert not bad.any(), ("%d samples are neither 0.5^k L nor an allowed zero; first" % bad.sum(), rgb[bad][0], k[bad][0])
    assert k.max() >= min(4, max_bounces) and k.min() <= 1, "the world must give short and long paths"
    if metal:
        assert black.any(), "the metal world must absorb some paths"
    img = scene.par_cast(cam, nx, ny, ns, max_bounces=max_bounces)
    per = rgb.reshape(ny, nx, ns, 3)[::-1]                                                  # (row 0 = top; y counts from the bottom)
    acc = np.zeros((ny, nx, 3), f32)
    for s in range(ns):
        acc = (acc + per[:, :, s]).astype(f32)
    fold = (acc / f32(ns)).astype(f32)
    assert np.array_equal(img.view(np.uint32), fold.view(np.uint32)), "the frame is not the ordered float32 fold of its samples"


# ---------------------------------------------------------------------------------------------------------------------------
# C. narrow beams: deterministic interfaces
# ---------------------------------------------------------------------------------------------------------------------------
FACES = {(0, 1): (1.0, 0.0, 0.0), (0, -1): (0.5, 0.0, 0.0), (1, 1): (0.0, 1.0, 0.0), (1, -1): (0.0, 0.5, 0.0),
         (2, 1): (0.0, 0.0, 1.0), (2, -1): (0.0, 0.0, 0.5)}
BEAM_FOV, BEAM_N = 0.02, (16, 16, 64)


def beam_world(pkg, b, pose):
    """The world of a pose: the object(s) of pose["objects"] inside six emitters of distinct power-of-two colours -- rects at
    +-10 (pose["world"] == "list") or six spheres of radius 9 at +-14 on the axes, with gaps, all under one Bvh ("lean").
    An object is (shape, material): shape ("sphere", centre, radius), ("prism", p0, p1), ("floor", y) or ("slab", p0, p1,
    density); material ("metal", fuzz), ("dielectric", index), ("lambertian",)."""
    S = pkg.scenes
    objs = []
    for shape, mat in pose["objects"]:
        if mat[0] == "metal":
            m = b.metal(S.vfrom(0.5), mat[1])
        elif mat[0] == "dielectric":
            m = b.dielectric(mat[1])
        else:
            m = b.lambertian(b.constant(S.vfrom(0.5)))
        if shape[0] == "sphere":
            objs.append(b.translate(S.v(*shape[1]), b.sphere(shape[2], m)))
        elif shape[0] == "prism":
            objs.append(b.rect_prism(S.v(*shape[1]), S.v(*shape[2]), m))
        elif shape[0] == "floor":
            objs.append(b.rect(S.Y, (-10.0, 10.0), (-10.0, 10.0), shape[1], m))
        else:
            objs.append(b.constant_medium(b.rect_prism(S.v(*shape[1]), S.v(*shape[2]), m), shape[3], b.isotropic(b.constant(S.vfrom(0.5)))))
    if pose["world"] == "list":
        faces = [b.rect(ax, (-10.0, 10.0), (-10.0, 10.0), 10.0 * sg, b.diffuse_light(b.constant(S.v(*FACES[(ax, sg)])), 1.0))
                 for ax in range(3) for sg in (1, -1)]
        return faces + objs
    faces = []
    for ax in range(3):
        for sg in (1, -1):
            c = [0.0, 0.0, 0.0]
            c[ax] = 14.0 * sg
            faces.append(b.translate(S.v(*c), b.sphere(9.0, b.diffuse_light(b.constant(S.v(*FACES[(ax, sg)])), 1.0))))
    return [b.bvh(faces + objs, (0.0, 1.0))]


def beam_camera(pkg, be, pose):
    S = pkg.scenes
    o, d = np.array(pose["origin"], F), np.array(pose["direction"], F)
    up = S.v(1.0, 0.0, 0.0) if abs(d[1]) > 0.9 * np.sqrt(d @ d) else S.v(0.0, 1.0, 0.0)
    return be.camera_look(S.v(*o), S.v(*(o + d / np.sqrt(d @ d))), up, BEAM_FOV, 1.0, 0.0, pose.get("focus_dist", 1.0), (0.0, 1.0))


def beam_rays(pose):
    """The centre ray and the four corner rays of a frame twice as wide as the camera's: float64 (origins [5, 3], unit
    directions [5, 3])."""
    o, d = np.array(pose["origin"], F), np.array(pose["direction"], F)
    d = d / np.sqrt(d @ d)
    up = np.array([1.0, 0.0, 0.0]) if abs(d[1]) > 0.9 else np.array([0.0, 1.0, 0.0])
    u = np.cross(up, -d)
    u /= np.sqrt(u @ u)
    v = np.cross(-d, u)
    h = 2.0 * np.tan(np.deg2rad(BEAM_FOV) / 2)
    ds = [d] + [d + sx * h * u + sy * h * v for sx in (-1, 1) for sy in (-1, 1)]
    ds = np.array([x / np.sqrt(x @ x) for x in ds])
    return np.broadcast_to(o, ds.shape).copy(), ds


def _schlick(cosine, idx, fault=None):
    r0 = ((1.0 - idx) / (1.0 + idx)) ** 2
    return r0 + (1.0 - r0) * (1.0 - cosine) ** (4 if fault == "schlick4" else 5)


def trace_tree(rec, prims, o, d, fault=None, depth=DEPTH):
    """Every outcome of one ray through mirrors, dielectrics and emitters: (leaves, shape, margin, first).  leaves: a dict
    {(r, g, b, bounces) or "deep": probability}; shape: a nested tuple of what happened (equal shapes = equal trees);
    margin: the smallest conditioning margin on the way (hits, refraction discriminants, facing tests); first: (reflected
    probability, keys of the reflected subtree, keys of the refracted subtree) of the first dielectric interface when it is
    the first hit and both branches exist, else None."""
    leaves, state = {}, {"margin": np.inf, "first": None}

    def add(key, p):
        leaves[key] = leaves.get(key, 0.0) + p

    def go(o, d, k, strength, p, keys):
        def leaf(key):
            add(key, p)
            keys.add(key)
            return key
        if k > depth:
            return leaf("deep")
        h = closest_hit(prims, o[None], d[None], np.array([0.5]), roots=k == 0)
        state["margin"] = min(state["margin"], float(h["margin"][0]))
        if not h["hit"][0]:
            return leaf((0.0, 0.0, 0.0, k))
        m, n, at = rec.materials[int(h["material"][0])], h["n"][0], h["p"][0]
        dn = d @ n / np.sqrt(d @ d)
        state["margin"] = min(state["margin"], abs(dn))
        if m[0] == "light":
            c = strength * m[2] * rec.textures[m[1]][1]
            return leaf((float(c[0]), float(c[1]), float(c[2]), k))
        if m[0] == "metal" and m[2] == 0.0:
            u = d / np.sqrt(d @ d)
            r = u - 2.0 * (u @ n) * n
            if r @ n > 0:
                return ("mirror", go(at, r, k + 1, strength * m[1][0], p, keys))
            return leaf((0.0, 0.0, 0.0, k))
        if m[0] != "dielectric":
            raise ValueError("the tracer follows deterministic interfaces only")
        idx = m[1]
        if d @ n > 0:
            outward, ratio, cosine = -n, idx, idx * dn
        else:
            outward, ratio, cosine = n, 1.0 / idx, -dn
        if fault == "ni_over_nt":
            ratio = 1.0 / ratio
        u = d / np.sqrt(d @ d)
        dt = u @ outward
        disc = 1.0 - ratio * ratio * (1.0 - dt * dt)
        state["margin"] = min(state["margin"], abs(disc))
        refl = d - 2.0 * (d @ n) * n
        if disc <= 0:
            return ("tir", go(at, refl, k + 1, strength, p, keys))
        refr = ratio * (u - dt * outward) - np.sqrt(disc) * outward
        pr = min(1.0, max(0.0, _schlick(cosine, idx, fault)))
        ka, kb = set(), set()
        sa = go(at, refl, k + 1, strength, p * pr, ka) if pr > 0 else None
        sb = go(at, refr, k + 1, strength, p * (1.0 - pr), kb) if pr < 1 else None
        if k == 0 and sa is not None and sb is not None:
            state["first"] = (pr, frozenset(ka), frozenset(kb))
        keys |= ka | kb
        return ("glass", sa, sb)

    shape = go(np.asarray(o, F), np.asarray(d, F), 0, 1.0, 1.0, set())
    return leaves, shape, state["margin"], state["first"]


def pose_tree(pkg, be, pose, fault=None):
    """(world handles' scene recorder, the centre ray's leaves, its first-interface record, admissible) of a pose."""
    rec = Recorder(be.builder())
    world = beam_world(pkg, rec, pose)
    prims = primitives(rec, world)
    os_, ds = beam_rays(pose)
    trees = [trace_tree(rec, prims, os_[i], ds[i], fault=fault) for i in range(5)]
    ok = all(t[1] == trees[0][1] for t in trees) and min(t[2] for t in trees) > POSE_MARGIN
    return rec, world, trees[0][0], trees[0][3], ok


def sample_outcomes(scene, cam, options=(), trace_kernel=False, seed=0xDEADBEEF):
    """{(r, g, b, bounces): count} over all 16 x 16 x 64 samples of a beam frame."""
    nx, ny, ns = BEAM_N
    for k, v in options:
        scene.set_option(k, v)
    ys, xs, ss = (a.ravel().astype(np.uint32) for a in np.meshgrid(np.arange(ny), np.arange(nx), np.arange(ns), indexing="ij"))
    rgb, info = scene.debug_samples(cam, nx, ny, ns, xs, ys, ss, seed=seed, trace_kernel=trace_kernel)
    rows = np.concatenate([rgb.astype(F), info[:, 0:1].astype(F)], axis=1)
    keys, counts = np.unique(rows, axis=0, return_counts=True)
    return {(float(r[0]), float(r[1]), float(r[2]), int(r[3])): int(c) for r, c in zip(keys, counts)}


def within(count, n, p, sigmas=5.0):
    return abs(count - n * p) <= sigmas * np.sqrt(n * p * (1.0 - p)) + 1e-9


def check_beam(pkg, be, pose, options=(), trace_kernel=False, fault=None):
    """C: one pose.  Mirror metal: every sample is the one predicted outcome.  Dielectric: every sample is a leaf of the
    predicted tree (paths longer than DEPTH: the "deep" leaf), every leaf expected at least 50 times is observed within
    5 sigma, and so is the first interface's reflected share when its two subtrees share no outcome.  Returns whether the
    first-interface share was checked."""
    rec, world, leaves, first, ok = pose_tree(pkg, be, pose, fault=fault)
    assert ok, ("the pose is not admissible", pose)
    got = sample_outcomes(rec.scene(world), beam_camera(pkg, be, pose), options, trace_kernel)
    n = sum(got.values())
    assert n == BEAM_N[0] * BEAM_N[1] * BEAM_N[2]
    deep = sum(c for key, c in got.items() if key[3] > DEPTH)
    shallow = {key: c for key, c in got.items() if key[3] <= DEPTH}
    unknown = {key: c for key, c in shallow.items() if key not in leaves}
    assert not unknown, ("outcomes the float64 tree does not have", unknown, leaves, pose)
    assert deep == 0 or "deep" in leaves, ("paths longer than the tree allows", deep, pose)
    for key, p in leaves.items():
        if n * p >= 50:
            c = deep if key == "deep" else shallow.get(key, 0)
            assert within(c, n, p), ("leaf %s: %d samples, expected %.1f +- %.1f" % (key, c, n * p, np.sqrt(n * p * (1 - p))), pose)
    if first is not None and not (first[1] & first[2]) and "deep" not in first[1]:
        c = sum(shallow.get(key, 0) for key in first[1])
        assert within(c, n, first[0]), ("first interface: %d reflected, Schlick gives %.1f +- %.1f" % (
            c, n * first[0], np.sqrt(n * first[0] * (1 - first[0]))), pose)
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------------------
# D. narrow beams: random lobes and media
# ---------------------------------------------------------------------------------------------------------------------------
MC_DRAWS = 2000000
_shares = {}


def _ball(rs, n):
    out = np.zeros((0, 3))
    while len(out) < n:
        v = rs.uniform(-1.0, 1.0, (int(1.3 * (n - len(out)) / 0.5236) + 16, 3))
        out = np.concatenate([out, v[_dot(v, v) < 1.0]])
    return out[:n]


def lobe_shares(point, direction, fuzz=None, fault=None):
    """Float64 Monte Carlo of one scatter off a floor with normal +y at `point` inside the box of six faces at +-10: the share
    of draws that end on each face (FACES order) and, last, the absorbed share.  fuzz None: the Lambertian lobe, normal +
    uniform-in-unit-ball; else the metal lobe, reflect(unit direction) + fuzz * ball, absorbed when it does not leave the
    floor's side."""
    key = (tuple(point), tuple(direction), fuzz, fault)
    if key in _shares:
        return _shares[key]
    rs = np.random.RandomState(20240611)
    ball = _ball(rs, MC_DRAWS)
    if fault == "unit_sphere":
        ball = ball / np.sqrt(_dot(ball, ball))[:, None]
    nrm = np.array([0.0, 1.0, 0.0])
    if fuzz is None:
        out = nrm + ball
    else:
        u = np.array(direction, F)
        u = u / np.sqrt(u @ u)
        out = (u - 2.0 * (u @ nrm) * nrm) + fuzz * ball
    alive = out[:, 1] > 0
    p = np.array(point, F)
    with np.errstate(all="ignore"):
        t = np.stack([np.where(out[:, ax] * sg > 0, (10.0 * sg - p[ax]) / out[:, ax], np.inf) for ax, sg in FACES], axis=1)
    face = t.argmin(axis=1)
    shares = [float(((face == i) & alive).mean()) for i in range(6)] + [float((~alive).mean())]
    _shares[key] = shares
    return shares


def check_lobe(pkg, be, pose, options=(), trace_kernel=False, fault=None):
    """D: a beam onto a floor at y = pose floor height.  Lambertian: every sample has exactly one bounce.  Each face's share
    (colour 0.5 * face colour, one bounce) and the absorbed share (colour zero, no bounce) are within 5 sigma of the Monte Carlo."""
    (shape, mat), = pose["objects"]
    o, d = np.array(pose["origin"], F), np.array(pose["direction"], F)
    point = o + d * ((shape[1] - o[1]) / d[1])
    fuzz = mat[1] if mat[0] == "metal" else None
    shares = lobe_shares(point, d, fuzz, fault)
    rec = Recorder(be.builder())
    world = beam_world(pkg, rec, pose)
    got = sample_outcomes(rec.scene(world), beam_camera(pkg, be, pose), options, trace_kernel)
    n = sum(got.values())
    want = {tuple(0.5 * c for c in FACES[f]) + (1,): shares[i] for i, f in enumerate(FACES)}
    want[(0.0, 0.0, 0.0, 0)] = shares[6]
    print("lobe %s at %s: Monte Carlo %s, observed %s" % (mat, np.round(point, 3), np.round(shares, 4),
                                                          np.round([got.get(k, 0) / n for k in want], 4)))
    assert not set(got) - set(want), ("outcomes the lobe cannot give", set(got) - set(want))
    if fuzz is None:
        assert all(k[3] == 1 for k in got), "a Lambertian floor scatters every sample exactly once"
    for k, p in want.items():
        if p <= 0:
            assert got.get(k, 0) == 0, (k, got.get(k, 0))
        else:
            assert within(got.get(k, 0), n, p), ("%s: %d samples, Monte Carlo %.1f +- %.1f" % (k, got.get(k, 0), n * p, np.sqrt(n * p * (1 - p))), pose)


def check_slab(pkg, be, pose, options=(), trace_kernel=False, fault=None):
    """D: a beam through a ConstantMedium slab.  The share of unscattered samples (no bounce) is within 5 sigma of
    exp(-rho * l), l the geometric chord, whatever the length of the camera's direction vector; those samples carry the far
    face's colour exactly."""
    (shape, _), = pose["objects"]
    rec = Recorder(be.builder())
    world = beam_world(pkg, rec, pose)
    media = []
    faces = primitives(rec, world, media)
    (boundary, rho, _), = media
    o, d = np.array(pose["origin"], F), np.array(pose["direction"], F)
    d = d / np.sqrt(d @ d)
    one = closest_hit(boundary, o[None], d[None], np.array([0.5]))
    two = closest_hit(boundary, o[None], d[None], np.array([0.5]), t_near=float(one["t"][0]) + 1e-4, roots=False)
    far = closest_hit(faces, o[None], d[None], np.array([0.5]))
    assert one["hit"][0] and two["hit"][0] and far["hit"][0] and min(one["margin"][0], two["margin"][0], far["margin"][0]) > POSE_MARGIN
    chord = float(two["t"][0] - one["t"][0])          # (|d| = 1: a length)
    if fault == "free_path":
        chord /= pose.get("focus_dist", 1.0)          # (the parameter interval of the camera's own direction vector)
    p = float(np.exp(-rho * chord))
    m = rec.materials[int(far["material"][0])]
    colour = tuple(float(c) for c in m[2] * rec.textures[m[1]][1]) + (0,)
    got = sample_outcomes(rec.scene(world), beam_camera(pkg, be, pose), options, trace_kernel)
    n = sum(got.values())
    clear = {k: c for k, c in got.items() if k[3] == 0}
    print("slab rho %g chord %.4f focus %g: exp(-rho l) N = %.1f +- %.1f, observed %d" % (
        rho, chord, pose.get("focus_dist", 1.0), n * p, np.sqrt(n * p * (1 - p)), sum(clear.values())))
    assert set(clear) == {colour}, ("unscattered samples must carry the far face's colour", clear, colour)
    assert within(clear[colour], n, p), (clear[colour], n * p, np.sqrt(n * p * (1 - p)), pose)


# curated poses --------------------------------------------------------------------------------------------------------------
# Found by a random search with pose_tree (float64 only) and fixed here; every test asserts that each pose it uses is admissible.
# The comment names what the first hit is (outside / inside incidence, grazing: |cos| < 0.35, tir: total internal reflection
# somewhere in the tree) and the number of distinct outcomes.
METAL_POSES = [
    {'world': 'list', 'objects': [(('sphere', [-1.368, 0.837, -0.023], 0.814), ('metal', 0.0)), (('prism', [1.755, -1.176, -1.245], [2.636, 0.363, -0.004]), ('metal', 0.0))], 'origin': [-2.772, -2.901, 1.238], 'direction': [0.292, 0.885, -0.363]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('sphere', [0.92, -0.951, -0.591], 1.23), ('metal', 0.0))], 'origin': [3.666, -2.92, -0.029], 'direction': [-0.696, 0.689, -0.204]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('sphere', [0.542, -0.942, -0.827], 0.7), ('metal', 0.0))], 'origin': [4.116, -1.441, -0.431], 'direction': [-0.999, 0.03, -0.038]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('sphere', [-1.669, 0.167, 0.879], 0.93), ('metal', 0.0)), (('prism', [0.753, -0.963, -1.679], [1.937, 0.347, 0.082]), ('metal', 0.0))], 'origin': [4.219, -0.75, 0.159], 'direction': [-0.965, 0.247, 0.092]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-2.881, 0.342, -0.626], [-1.183, 1.472, 0.257]), ('metal', 0.0)), (('prism', [1.1, 0.006, 0.175], [2.67, 1.566, 1.685]), ('metal', 0.0))], 'origin': [-2.844, -0.861, -3.045], 'direction': [0.349, 0.42, 0.837]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('sphere', [-0.472, -0.516, -0.83], 1.327), ('metal', 0.0))], 'origin': [1.164, 4.041, 0.237], 'direction': [-0.29, -0.955, -0.069]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-1.427, -0.485, -0.64], [-0.143, 0.377, 1.249]), ('metal', 0.0))], 'origin': [3.758, -2.3, 1.145], 'direction': [-0.901, 0.411, -0.139]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-0.312, -1.282, -0.914], [1.336, 0.156, 0.617]), ('metal', 0.0))], 'origin': [0.158, -1.95, -3.598], 'direction': [0.037, 0.403, 0.915]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-0.894, -0.704, -0.551], [1.138, 1.273, 1.459]), ('metal', 0.0))], 'origin': [-3.17, -2.378, -0.606], 'direction': [0.79, 0.576, 0.21]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-2.578, -0.516, -1.33], [-0.885, 1.015, -0.032]), ('metal', 0.0)), (('prism', [1.143, -1.449, -0.208], [2.931, 0.122, 0.774]), ('metal', 0.0))], 'origin': [-1.852, 2.644, 2.528], 'direction': [0.109, -0.608, -0.786]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-1.982, -1.848, -0.521], [-0.016, 0.493, 1.478]), ('metal', 0.0))], 'origin': [2.832, -1.886, 2.216], 'direction': [-0.857, 0.226, -0.462]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('sphere', [-1.406, -0.563, 0.692], 0.801), ('metal', 0.0)), (('prism', [1.619, -0.247, -1.224], [2.429, 1.103, 0.284]), ('metal', 0.0))], 'origin': [-1.48, -4.129, 0.471], 'direction': [0.024, 0.981, 0.192]},   # outside, 1 outcomes
    {'world': 'list', 'objects': [(('sphere', [0.717, 0.528, -0.358], 1.054), ('metal', 0.0))], 'origin': [3.686, 0.101, -2.24], 'direction': [-0.956, 0.024, 0.292]},   # grazing outside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-2.262, -0.735, -2.193], [0.399, 0.435, 0.528]), ('metal', 0.0))], 'origin': [2.627, -1.956, 3.326], 'direction': [-0.718, 0.217, -0.662]},   # grazing outside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-0.78, -0.294, -0.631], [0.812, 1.647, 1.622]), ('metal', 0.0))], 'origin': [-1.596, 3.112, 2.753], 'direction': [0.214, -0.813, -0.542]},   # grazing outside, 1 outcomes
    {'world': 'list', 'objects': [(('sphere', [-0.179, 0.354, 0.835], 1.397), ('metal', 0.0))], 'origin': [-3.187, 0.39, 2.737], 'direction': [0.947, -0.216, -0.236]},   # grazing outside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-0.826, -0.186, -0.922], [1.085, 1.495, 0.402]), ('metal', 0.0))], 'origin': [3.197, 2.24, -1.269], 'direction': [-0.859, -0.5, 0.109]},   # grazing outside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-0.455, -1.058, -2.096], [0.903, 1.071, 0.55]), ('metal', 0.0))], 'origin': [0.324, 0.533, -0.158], 'direction': [0.866, -0.402, -0.297]},   # inside, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-0.042, -0.281, 0.436], [1.098, 1.475, 1.443]), ('metal', 0.0))], 'origin': [0.412, 0.16, 1.095], 'direction': [0.906, 0.36, -0.222]},   # inside, 1 outcomes
    {'world': 'list', 'objects': [(('sphere', [-0.085, 0.652, -0.975], 0.894), ('metal', 0.0))], 'origin': [-0.084, 0.523, -0.963], 'direction': [0.285, 0.932, 0.223]},   # inside, 1 outcomes
    {'world': 'lean', 'objects': [(('sphere', [0.973, 0.367, 0.038], 0.759), ('metal', 0.0))], 'origin': [1.095, 2.886, 2.759], 'direction': [0.044, -0.587, -0.809]},   # outside, 1 outcomes
    {'world': 'lean', 'objects': [(('sphere', [0.875, 0.943, -0.954], 0.985), ('metal', 0.0))], 'origin': [-0.29, 1.22, 4.092], 'direction': [0.213, -0.01, -0.977]},   # outside, 1 outcomes
    {'world': 'lean', 'objects': [(('sphere', [-0.408, -0.58, -0.531], 1.466), ('metal', 0.0))], 'origin': [4.288, -0.198, 1.211], 'direction': [-0.889, -0.126, -0.44]},   # outside, 1 outcomes
    {'world': 'lean', 'objects': [(('sphere', [0.867, -0.318, 0.76], 1.202), ('metal', 0.0))], 'origin': [3.867, -1.191, 0.889], 'direction': [-0.833, 0.5, 0.239]},   # grazing outside, 1 outcomes
    {'world': 'lean', 'objects': [(('sphere', [-0.831, 0.862, 0.965], 1.434), ('metal', 0.0))], 'origin': [2.211, 1.154, 3.591], 'direction': [-0.898, -0.219, -0.381]},   # grazing outside, 1 outcomes
]
GLASS_POSES = [
    {'world': 'list', 'objects': [(('sphere', [-0.044, -0.615, -0.84], 1.483), ('dielectric', 1.5))], 'origin': [3.823, 0.686, -1.648], 'direction': [-0.983, -0.16, 0.086]},   # outside, 7 outcomes, first-interface share
    {'world': 'list', 'objects': [(('sphere', [0.253, -0.212, -0.195], 1.012), ('dielectric', 1.5))], 'origin': [-3.485, -2.545, 0.103], 'direction': [0.784, 0.618, -0.062]},   # outside, 7 outcomes, first-interface share
    {'world': 'list', 'objects': [(('sphere', [0.751, 0.755, -0.639], 1.201), ('dielectric', 1.5))], 'origin': [-4.057, -0.232, 0.233], 'direction': [0.975, 0.221, -0.008]},   # outside, 7 outcomes, first-interface share
    {'world': 'list', 'objects': [(('prism', [-1.075, -0.004, -1.128], [0.9, 1.128, 1.541]), ('dielectric', 1.5))], 'origin': [-1.581, -1.906, -3.49], 'direction': [0.339, 0.437, 0.833]},   # outside tir, 5 outcomes, first-interface share
    {'world': 'list', 'objects': [(('sphere', [-0.488, -0.006, 0.417], 1.42), ('dielectric', 1.5))], 'origin': [0.756, 1.877, 3.821], 'direction': [0.02, -0.413, -0.91]},   # grazing outside, 7 outcomes, first-interface share
    {'world': 'list', 'objects': [(('prism', [-2.013, -1.257, -1.224], [0.445, -0.062, 1.524]), ('dielectric', 1.5))], 'origin': [-2.998, 0.611, 3.007], 'direction': [0.597, -0.235, -0.767]},   # grazing outside tir, 5 outcomes, first-interface share
    {'world': 'list', 'objects': [(('sphere', [-0.414, -0.777, 0.469], 1.041), ('dielectric', 1.5))], 'origin': [-0.5, -0.876, 0.41], 'direction': [0.151, 0.959, -0.241]},   # inside, 7 outcomes
    {'world': 'list', 'objects': [(('sphere', [-0.409, 0.911, -0.434], 1.303), ('dielectric', 1.5))], 'origin': [-0.318, 1.441, -0.496], 'direction': [-0.862, 0.307, -0.403]},   # inside, 7 outcomes
    {'world': 'list', 'objects': [(('sphere', [-0.674, -0.635, -0.372], 0.978), ('dielectric', 1.5))], 'origin': [-0.82, -0.471, 0.105], 'direction': [0.562, 0.261, 0.785]},   # inside, 7 outcomes
    {'world': 'list', 'objects': [(('prism', [-1.505, -1.292, -0.311], [1.118, -0.127, 1.873]), ('dielectric', 1.5))], 'origin': [0.047, -0.502, 0.449], 'direction': [0.607, -0.683, 0.407]},   # inside tir, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-0.634, -0.757, -0.47], [0.626, 0.799, 0.857]), ('dielectric', 1.5))], 'origin': [-0.081, 0.113, 0.341], 'direction': [-0.178, -0.003, -0.984]},   # inside tir, 6 outcomes
    {'world': 'list', 'objects': [(('prism', [-1.323, -1.985, -1.325], [-0.05, 0.672, -0.044]), ('dielectric', 1.5))], 'origin': [-0.33, -1.178, -0.341], 'direction': [-0.825, 0.468, 0.315]},   # grazing inside tir, 4 outcomes
    {'world': 'lean', 'objects': [(('sphere', [0.086, -0.692, 0.694], 0.788), ('dielectric', 1.5))], 'origin': [-3.769, 2.098, 0.582], 'direction': [0.868, -0.495, 0.047]},   # outside, 7 outcomes, first-interface share
    {'world': 'lean', 'objects': [(('sphere', [-0.758, -0.83, -0.31], 0.78), ('dielectric', 1.5))], 'origin': [-0.727, 1.087, 4.255], 'direction': [-0.017, -0.484, -0.875]},   # outside, 7 outcomes, first-interface share
    {'world': 'lean', 'objects': [(('sphere', [-0.32, 0.138, -0.864], 0.641), ('dielectric', 1.5))], 'origin': [-0.316, 0.184, -0.563], 'direction': [0.606, 0.523, -0.599]},   # inside, 7 outcomes
    {'world': 'list', 'objects': [(('sphere', [-0.385, -0.388, 0.64], 1.039), ('dielectric', 0.6667))], 'origin': [3.05, -1.13, -2.615], 'direction': [-0.684, 0.033, 0.729]},   # outside, 7 outcomes, first-interface share
    {'world': 'list', 'objects': [(('prism', [-0.313, -1.092, -0.092], [1.364, 1.572, 1.662]), ('dielectric', 0.6667))], 'origin': [-3.309, 2.683, -0.18], 'direction': [0.794, -0.548, 0.265]},   # outside, 7 outcomes, first-interface share
    {'world': 'list', 'objects': [(('sphere', [0.722, 0.245, -0.309], 0.937), ('dielectric', 0.6667))], 'origin': [-0.785, 3.625, -1.76], 'direction': [0.388, -0.895, 0.219]},   # outside, 7 outcomes, first-interface share
    {'world': 'list', 'objects': [(('sphere', [0.495, -0.904, -0.287], 0.889), ('dielectric', 0.6667))], 'origin': [0.486, -4.307, -0.312], 'direction': [-0.106, 0.994, 0.035]},   # outside, 7 outcomes, first-interface share
    {'world': 'list', 'objects': [(('prism', [0.299, -1.418, -1.207], [1.147, 0.773, 1.294]), ('dielectric', 0.6667))], 'origin': [0.78, -0.87, -0.547], 'direction': [-0.327, -0.939, 0.106]},   # inside, 7 outcomes
    {'world': 'list', 'objects': [(('sphere', [0.764, 0.363, 0.47], 0.854), ('dielectric', 0.6667))], 'origin': [0.708, 0.212, 0.565], 'direction': [-0.069, 0.943, -0.326]},   # inside, 7 outcomes
    {'world': 'list', 'objects': [(('sphere', [0.221, -0.422, 0.664], 0.683), ('dielectric', 0.6667))], 'origin': [-0.151, -0.421, 0.641], 'direction': [-0.196, -0.967, -0.163]},   # inside, 7 outcomes
    {'world': 'lean', 'objects': [(('sphere', [0.065, 0.711, -0.385], 0.947), ('dielectric', 0.6667))], 'origin': [-3.778, -0.119, -1.74], 'direction': [0.93, 0.293, 0.22]},   # outside, 7 outcomes, first-interface share
    {'world': 'lean', 'objects': [(('sphere', [-0.953, 0.515, 0.614], 0.755), ('dielectric', 0.6667))], 'origin': [-0.415, 3.018, -2.791], 'direction': [-0.12, -0.553, 0.825]},   # outside, 7 outcomes, first-interface share
    {'world': 'lean', 'objects': [(('sphere', [-0.294, 0.284, -0.531], 0.978), ('dielectric', 0.6667))], 'origin': [-0.321, -0.238, -0.554], 'direction': [0.826, 0.545, 0.146]},   # inside, 7 outcomes
    {'world': 'list', 'objects': [(('prism', [-0.427, -0.454, -1.196], [0.942, 0.853, 0.259]), ('dielectric', 0.6667))], 'origin': [-0.663, 3.222, 2.304], 'direction': [0.218, -0.776, -0.592]},   # outside tir, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-0.991, -1.805, 0.203], [1.55, 0.841, 1.007]), ('dielectric', 0.6667))], 'origin': [0.588, 3.969, -0.258], 'direction': [-0.225, -0.966, 0.123]},   # grazing outside tir, 1 outcomes
    {'world': 'list', 'objects': [(('prism', [-0.918, -2.344, -1.056], [0.705, 0.426, 1.347]), ('dielectric', 0.6667))], 'origin': [2.539, -2.174, 2.627], 'direction': [-0.495, 0.572, -0.654]},   # outside tir, 1 outcomes
    {'world': 'list', 'objects': [(('sphere', [0.797, -0.835, 0.053], 1.195), ('dielectric', 0.6667))], 'origin': [3.932, -0.259, 0.972], 'direction': [-0.959, -0.28, -0.033]},   # outside tir, 1 outcomes
    {'world': 'lean', 'objects': [(('sphere', [0.973, -0.785, 0.162], 1.026), ('dielectric', 0.6667))], 'origin': [-1.92, -0.396, 3.819], 'direction': [0.59, 0.072, -0.805]},   # outside tir, 1 outcomes
]

_LAMB, _FLOOR0 = ("lambertian",), ("floor", 0.0)
LOBE_POSES = [
    {"world": "list", "objects": [(_FLOOR0, _LAMB)], "origin": [0.6, 5.0, 0.3], "direction": [0.0, -1.0, 0.0]},
    {"world": "list", "objects": [(_FLOOR0, _LAMB)], "origin": [4.0, 3.0, -5.0], "direction": [-0.5, -0.6, 0.62]},
    {"world": "list", "objects": [(("floor", -3.0), _LAMB)], "origin": [-5.0, 2.0, 2.0], "direction": [0.7, -0.7, -0.1]},
    {"world": "list", "objects": [(_FLOOR0, ("metal", 0.3))], "origin": [-6.0, 1.5, -1.0], "direction": [0.9, -0.2, 0.1]},
    {"world": "list", "objects": [(_FLOOR0, ("metal", 0.3))], "origin": [1.0, 4.0, 2.0], "direction": [0.3, -0.8, 0.1]},
    {"world": "list", "objects": [(_FLOOR0, ("metal", 0.8))], "origin": [-4.0, 2.0, 1.0], "direction": [0.8, -0.3, 0.2]},
    {"world": "list", "objects": [(("floor", -3.0), ("metal", 0.8))], "origin": [2.0, 3.0, 3.0], "direction": [-0.2, -0.9, -0.3]},
]
_SLAB = lambda rho: (("slab", [-2.0, -1.0, -3.0], [2.0, 1.0, 3.0], rho), _LAMB)
SLAB_POSES = [   # two densities, an oblique chord, and the first chord again through a camera whose direction vector is 4 long
    {"world": "list", "objects": [_SLAB(0.4)], "origin": [0.3, 5.0, 0.5], "direction": [0.0, -1.0, 0.0]},
    {"world": "list", "objects": [_SLAB(1.0)], "origin": [0.3, 5.0, 0.5], "direction": [0.0, -1.0, 0.0]},
    {"world": "list", "objects": [_SLAB(0.4)], "origin": [-3.5, 5.0, 0.5], "direction": [0.6, -0.8, 0.0]},
    {"world": "list", "objects": [_SLAB(0.4)], "origin": [0.3, 5.0, 0.5], "direction": [0.0, -1.0, 0.0], "focus_dist": 4.0},
]
