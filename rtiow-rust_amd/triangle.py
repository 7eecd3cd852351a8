"""The triangle primitive (include/rtiow_gpu_mesh.h) in numpy: the AUTHORITY.  csrc/rt_triangle.h, the one host-and-device
function every walk calls, equals this module bit for bit (tests/test_mesh_abi.py on the host, tests/test_mesh_gpu.py on the GPU).

Everything is float32.  Every operation is rounded on its own and nothing is contracted: numpy evaluates `a * b - c * d` on
float32 arrays as three float32 operations, which is the definition.

  record(v0, v1, v2)            -> (v0, e1, e2, N)
  hit(rec, o, d, t_min, t_max)  -> (hit, t, p, n) per (triangle, ray) pair
  bounding_box(v0, v1, v2)      -> (min, max)
  closest(triangles, rays7, t_min), occluded(triangles, rays8, t_min): what a list world of the triangles answers
  icosphere, box, grid, load_obj: ways to make a mesh (vertices [n, 3] float32, indices [m, 3] uint32)

Surface attributes (include/rtiow_gpu_surface.h) -- per-vertex normals and UVs; this module is their authority too:

  barycentric(rec, o, d)        -> (u, v): the floats hit()'s accept test uses
  shade(rec, normals, uvs, o, d, flip) -> (n, tu, tv): the shading normal and the surface coordinates of a hit
      w = (1 - u) - v;  s = (w n0 + u n1) + v n2 per component, each product rounded, left to right;
      len = sqrt((s.x s.x + s.y s.y) + s.z s.z);  n = s / len if len > 0 and len <= f32::MAX, else N;  -n under flip;
      tu = (w u0 + u u1) + v u2, tv likewise.  normals None: n = N.  uvs None: (tu, tv) = (0, 0).
  closest_attr(triangles, normals, uvs, rays7, t_min, flips): closest() with the shading normal and (tu, tv): [n, 10]
  vertex_normals, icosphere_attr, load_obj_attr: ways to make the attributes
"""
import numpy as np

F = np.float32
PAD = F(0.0001)   # Rect's pad (object.rs:220), on every axis


def _f(a):
    return np.asarray(a, dtype=np.float32)


def cross(a, b):
    """cross(a, b).x = a.y*b.z - a.z*b.y, cyclic for y and z; each product is rounded before the subtraction."""
    a, b = _f(a), _f(b)
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def dot(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z"""
    a, b = _f(a), _f(b)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def record(v0, v1, v2):
    """The stored form of a triangle: (v0, e1, e2, N), each [..., 3].  A counter-clockwise winding gives the front face.
    (`length` below is what rtg_object_triangle refuses when it is 0 or not finite.)"""
    v0, v1, v2 = _f(v0), _f(v1), _f(v2)
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        c = cross(e1, e2)
        ln = np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2])
        n = c / ln[..., None]
    return v0, e1, e2, n


def length(v0, v1, v2):
    """len of the definition: |cross(v1 - v0, v2 - v0)| in its float32 arithmetic."""
    v0, v1, v2 = _f(v0), _f(v1), _f(v2)
    with np.errstate(all="ignore"):
        c = cross(v1 - v0, v2 - v0)
        return np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2])


def hit(rec, o, d, t_min, t_max, flip=False):
    """Moeller-Trumbore for broadcastable (triangle, ray) pairs over [t_min, t_max).  Returns (hit [..] bool, t, p [.., 3],
    n [.., 3]); t, p, n hold whatever the arithmetic gives where hit is False.  flip: an odd number of FlipNormals."""
    v0, e1, e2, n = rec
    o, d = _f(o), _f(d)
    t_min, t_max = _f(t_min), _f(t_max)
    with np.errstate(all="ignore"):
        pv = cross(d, e2)
        det = dot(e1, pv)
        inv = F(1.0) / det
        tv = o - v0
        u = dot(tv, pv) * inv
        qv = cross(tv, e1)
        v = dot(d, qv) * inv
        t = dot(e2, qv) * inv
        ok = (u >= 0) & (v >= 0) & (u + v <= F(1.0)) & (t >= t_min) & (t < t_max)
        p = o + t[..., None] * d
    nn = np.broadcast_to(-n if flip else n, p.shape)
    return ok, t, p, nn


def barycentric(rec, o, d):
    """(u, v) of Moeller-Trumbore for broadcastable (triangle, ray) pairs: the very floats hit()'s accept test uses (the same
    operations in the same order)."""
    v0, e1, e2, _ = rec
    o, d = _f(o), _f(d)
    with np.errstate(all="ignore"):
        pv = cross(d, e2)
        det = dot(e1, pv)
        inv = F(1.0) / det
        tv = o - v0
        u = dot(tv, pv) * inv
        qv = cross(tv, e1)
        v = dot(d, qv) * inv
    return u, v


def shade(rec, normals, uvs, o, d, flip=False):
    """The shading normal and the surface coordinates (include/rtiow_gpu_surface.h) of broadcastable (triangle, ray) pairs:
    normals [.., 3, 3] = n0, n1, n2 or None (the face normal N), uvs [.., 3, 2] or None ((0, 0)).  Returns (n [.., 3], tu, tv);
    they hold whatever the arithmetic gives where hit() says miss.  Vertex normals are used as given."""
    u, v = barycentric(rec, o, d)
    face = np.broadcast_to(rec[3], u.shape + (3,))
    with np.errstate(all="ignore"):
        w = (F(1.0) - u) - v
        if uvs is None:
            tu, tv = np.zeros_like(u), np.zeros_like(u)
        else:
            t = _f(uvs)
            tu = (w * t[..., 0, 0] + u * t[..., 1, 0]) + v * t[..., 2, 0]
            tv = (w * t[..., 0, 1] + u * t[..., 1, 1]) + v * t[..., 2, 1]
        if normals is None:
            n = face
        else:
            m = _f(normals)
            s = (w[..., None] * m[..., 0, :] + u[..., None] * m[..., 1, :]) + v[..., None] * m[..., 2, :]
            ln = np.sqrt((s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2])
            ok = (ln > 0) & (ln <= np.finfo(np.float32).max)
            n = np.where(ok[..., None], s / ln[..., None], face)
    return (-n if flip else n).astype(np.float32), tu.astype(np.float32), tv.astype(np.float32)


def bounding_box(v0, v1, v2):
    """Per axis min(v0, v1, v2) - 0.0001f and max(v0, v1, v2) + 0.0001f."""
    v0, v1, v2 = _f(v0), _f(v1), _f(v2)
    return np.minimum(np.minimum(v0, v1), v2) - PAD, np.maximum(np.maximum(v0, v1), v2) + PAD


def vertices_of(vertices, indices):
    """[m, 3, 3] float32: the three vertices of every triangle of an indexed mesh."""
    return _f(vertices)[np.asarray(indices, dtype=np.int64)]


def closest(triangles, rays, t_min, flips=None):
    """What a list world of `triangles` ([m, 3, 3]) answers for rays [n, >= 6] (o, d, ...): the left fold over the list in order
    with a shrinking t_max, so on an exact tie the first triangle wins.  Returns (out [n, 8] float32 = hit, t, p, n -- zeros on
    a miss, as rtg_debug_hit_top writes them -- and index [n] int64, -1 on a miss).  flips: per triangle, under FlipNormals."""
    tri = _f(triangles).reshape(-1, 3, 3)
    rays = _f(rays)
    o, d = rays[:, 0:3], rays[:, 3:6]
    n = len(rays)
    best = np.full(n, np.finfo(np.float32).max, dtype=np.float32)
    out = np.zeros((n, 8), dtype=np.float32)
    index = np.full(n, -1, dtype=np.int64)
    for k in range(len(tri)):
        rec = record(tri[k, 0], tri[k, 1], tri[k, 2])
        ok, t, p, nn = hit(rec, o, d, F(t_min), best, flip=bool(flips[k]) if flips is not None else False)
        out[ok, 0] = 1.0
        out[ok, 1] = t[ok]
        out[ok, 2:5] = p[ok]
        out[ok, 5:8] = nn[ok]
        index[ok] = k
        best = np.where(ok, t, best)
    return out, index


def closest_attr(triangles, normals, uvs, rays, t_min, flips=None):
    """closest() for triangles with attributes: normals / uvs are lists with one entry per triangle, [3, 3] / [3, 2] or None
    (or None for the whole list).  Folds in list order like closest.  Returns (out [n, 10] float32 = hit, t, p, shading
    normal, tu, tv -- zeros on a miss, as rtg_debug_hit_surface writes them -- and index [n] int64)."""
    tri = _f(triangles).reshape(-1, 3, 3)
    rays = _f(rays)
    o, d = rays[:, 0:3], rays[:, 3:6]
    n = len(rays)
    best = np.full(n, np.finfo(np.float32).max, dtype=np.float32)
    out = np.zeros((n, 10), dtype=np.float32)
    index = np.full(n, -1, dtype=np.int64)
    for k in range(len(tri)):
        rec = record(tri[k, 0], tri[k, 1], tri[k, 2])
        flip = bool(flips[k]) if flips is not None else False
        ok, t, p, _ = hit(rec, o, d, F(t_min), best)
        nn, tu, tv = shade(rec, None if normals is None else normals[k], None if uvs is None else uvs[k], o, d, flip=flip)
        out[ok, 0] = 1.0
        out[ok, 1] = t[ok]
        out[ok, 2:5] = p[ok]
        out[ok, 5:8] = nn[ok]
        out[ok, 8] = tu[ok]
        out[ok, 9] = tv[ok]
        index[ok] = k
        best = np.where(ok, t, best)
    return out, index


def all_t(triangles, rays, t_min):
    """[m, n] float32: every triangle's t for every ray, +inf where it is not hit over [t_min, f32::MAX) -- for tests that look
    for ties."""
    tri = _f(triangles).reshape(-1, 3, 3)
    rays = _f(rays)
    res = np.full((len(tri), len(rays)), np.inf, dtype=np.float32)
    for k in range(len(tri)):
        ok, t, _, _ = hit(record(tri[k, 0], tri[k, 1], tri[k, 2]), rays[:, 0:3], rays[:, 3:6], F(t_min), np.finfo(np.float32).max)
        res[k, ok] = t[ok]
    return res


def occluded(triangles, rays8, t_min):
    """rtg_query_occluded of a list world of `triangles`: [n] uint8, 1 where some triangle is hit over [t_min, rays8[:, 7]);
    0 unless t_max > t_min (a NaN t_max included)."""
    tri = _f(triangles).reshape(-1, 3, 3)
    rays = _f(rays8)
    with np.errstate(all="ignore"):
        live = rays[:, 7] > F(t_min)
    res = np.zeros(len(rays), dtype=bool)
    for k in range(len(tri)):
        ok, _, _, _ = hit(record(tri[k, 0], tri[k, 1], tri[k, 2]), rays[:, 0:3], rays[:, 3:6], F(t_min), rays[:, 7])
        res |= ok
    return (res & live).astype(np.uint8)


# ---- procedural meshes (float64 construction, rounded to float32 once) --------------------------------------------------------
def icosphere(subdivisions, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """A subdivided icosahedron on the sphere: 20 * 4^subdivisions triangles, counter-clockwise seen from outside."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    verts = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(subdivisions)):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        nxt = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    vv = np.asarray(verts) * float(radius) + np.asarray(centre, dtype=np.float64)
    return vv.astype(np.float32), np.asarray(faces, dtype=np.uint32)


def box(p0, p1):
    """The box p0 .. p1 as 12 triangles with outward (counter-clockwise) winding."""
    (x0, y0, z0), (x1, y1, z1) = p0, p1
    v = np.array([(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)],
                 dtype=np.float32)
    f = [(0, 2, 1), (0, 3, 2),   # -z
         (4, 5, 6), (4, 6, 7),   # +z
         (0, 1, 5), (0, 5, 4),   # -y
         (3, 6, 2), (3, 7, 6),   # +y
         (0, 4, 7), (0, 7, 3),   # -x
         (1, 2, 6), (1, 6, 5)]   # +x
    return v, np.asarray(f, dtype=np.uint32)


def grid(nx, nz, height_fn, p0=(0.0, 0.0), p1=(1.0, 1.0)):
    """A height field over [p0, p1] in (x, z): (nx + 1) * (nz + 1) vertices at y = height_fn(x, z), 2 * nx * nz triangles whose
    front faces look up (+y)."""
    xs = np.linspace(p0[0], p1[0], nx + 1)
    zs = np.linspace(p0[1], p1[1], nz + 1)
    v = np.array([(x, float(height_fn(x, z)), z) for z in zs for x in xs], dtype=np.float32)
    f = []
    for j in range(nz):
        for i in range(nx):
            a, b = j * (nx + 1) + i, j * (nx + 1) + i + 1
            c, d = a + nx + 1, b + nx + 1
            f += [(a, c, b), (b, c, d)]
    return v, np.asarray(f, dtype=np.uint32)


def load_obj(path):
    """A minimal Wavefront reader: `v x y z` and `f a b c ...` lines only.  Polygons are fan-triangulated, negative indices count
    back from the vertices read so far, `/vt/vn` suffixes are ignored, every other line is skipped."""
    verts, faces = [], []
    with open(path) as fh:
        for line in fh:
            w = line.split("#", 1)[0].split()
            if not w:
                continue
            if w[0] == "v":
                verts.append([float(x) for x in w[1:4]])
            elif w[0] == "f":
                ix = []
                for tok in w[1:]:
                    i = int(tok.split("/")[0])
                    if i == 0 or i > len(verts) or -i > len(verts):
                        raise ValueError("%s: face index %d out of range" % (path, i))
                    ix.append(i - 1 if i > 0 else len(verts) + i)
                faces += [(ix[0], ix[k], ix[k + 1]) for k in range(1, len(ix) - 1)]
    return np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(faces, dtype=np.uint32).reshape(-1, 3)


# ---- surface attributes (include/rtiow_gpu_surface.h) ------------------------------------------------------------------------
def vertex_normals(vertices, indices):
    """Area-weighted vertex normals of an indexed mesh: the sum of cross(v1 - v0, v2 - v0) over the triangles at a vertex,
    normalised; built in float64 and rounded once.  A vertex no triangle uses (or whose sum is zero) gets (0, 0, 0), which the
    builder accepts: shading falls back to the face normal there."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, f[:, k], c)
    ln = np.linalg.norm(acc, axis=1)
    out = np.where(ln[:, None] > 0, acc / np.where(ln > 0, ln, 1.0)[:, None], 0.0)
    return out.astype(np.float32)


def icosphere_attr(subdivisions, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """icosphere() with attributes: (v, f, normals, uvs) -- normals (v - centre) / radius, spherical UVs
    u = 0.5 + atan2(z, x) / (2 pi), v = 0.5 + asin(y) / pi of that direction.  Built in float64 from the float32 vertices
    icosphere() returns, rounded once.  (The UV seam at u = 0 / 1 is not split: triangles across it interpolate through it.)"""
    v, f = icosphere(subdivisions, radius, centre)
    dirs = (v.astype(np.float64) - np.asarray(centre, dtype=np.float64)) / float(radius)
    unit = dirs / np.linalg.norm(dirs, axis=1)[:, None]
    uu = 0.5 + np.arctan2(unit[:, 2], unit[:, 0]) / (2.0 * np.pi)
    vv = 0.5 + np.arcsin(np.clip(unit[:, 1], -1.0, 1.0)) / np.pi
    return v, f, dirs.astype(np.float32), np.stack([uu, vv], axis=1).astype(np.float32)


def load_obj_attr(path):
    """A Wavefront reader with attributes: `v`, `vt u v`, `vn x y z` and `f a/b/c ...` lines (also `a`, `a/b`, `a//c`).  The three
    index streams are unified into ONE vertex list -- a new vertex per distinct (v, vt, vn) triple, in order of first use --
    polygons are fan-triangulated and negative indices count back from what was read so far, as in load_obj.  Returns
    (vertices [n, 3], indices [m, 3], normals [n, 3] or None, uvs [n, 2] or None): an attribute is None unless EVERY face
    corner names one."""
    pos, tex, nrm = [], [], []
    keys, corners, faces = {}, [], []
    all_vt, all_vn = True, True

    def resolve(tok, have, what):
        i = int(tok)
        if i == 0 or i > have or -i > have:
            raise ValueError("%s: %s index %d out of range" % (path, what, i))
        return i - 1 if i > 0 else have + i
    with open(path) as fh:
        for line in fh:
            w = line.split("#", 1)[0].split()
            if not w:
                continue
            if w[0] == "v":
                pos.append([float(x) for x in w[1:4]])
            elif w[0] == "vt":
                tex.append([float(x) for x in w[1:3]])
            elif w[0] == "vn":
                nrm.append([float(x) for x in w[1:4]])
            elif w[0] == "f":
                ix = []
                for tok in w[1:]:
                    part = tok.split("/")
                    a = resolve(part[0], len(pos), "face")
                    b = resolve(part[1], len(tex), "vt") if len(part) > 1 and part[1] else -1
                    c = resolve(part[2], len(nrm), "vn") if len(part) > 2 and part[2] else -1
                    all_vt, all_vn = all_vt and b >= 0, all_vn and c >= 0
                    key = (a, b, c)
                    if key not in keys:
                        keys[key] = len(corners)
                        corners.append(key)
                    ix.append(keys[key])
                faces += [(ix[0], ix[k], ix[k + 1]) for k in range(1, len(ix) - 1)]
    p = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    v = np.asarray([p[a] for a, _, _ in corners], dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.uint32).reshape(-1, 3)
    uvs = np.asarray([tex[b] for _, b, _ in corners], dtype=np.float32).reshape(-1, 2) if (all_vt and corners) else None
    normals = np.asarray([nrm[c] for _, _, c in corners], dtype=np.float32).reshape(-1, 3) if (all_vn and corners) else None
    return v, f, normals, uvs
