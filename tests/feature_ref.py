"""Reference planes for RTG_FLAG_FEATURES (include/rtiow_gpu.h), shared by test_features_abi.py and test_features_gpu.py: a
recording proxy around a Builder (what every material handle is), a numpy albedo evaluator, and the planes themselves from
features.subpixel_rays, the ORACLE's debug_hit_top and the fold.  Nothing here touches the GPU library."""
import ctypes as C

import numpy as np

from scene_cases import CASES

f32 = np.float32


class RecordingBuilder:
    """A Builder that remembers the kind, colour and texture of every texture and material handle it gives out; every other
    call goes to the Builder as it is."""

    def __init__(self, builder):
        self._b = builder
        self.textures, self.materials = {}, {}

    def __getattr__(self, name):
        return getattr(self._b, name)

    def _c(self, color):
        return np.array([color[0], color[1], color[2]], dtype=f32)   # (the binding rounds to float32 the same way)

    def constant(self, color):
        t = self._b.constant(color)
        self.textures[t] = ("constant", self._c(color))
        return t

    def checker(self, t0, t1):
        t = self._b.checker(t0, t1)
        self.textures[t] = ("checker", t0, t1)
        return t

    def perlin(self, scale):
        t = self._b.perlin(scale)
        self.textures[t] = ("perlin", f32(scale))
        return t

    def lambertian(self, albedo):
        m = self._b.lambertian(albedo)
        self.materials[m] = ("texture", albedo, f32(1))
        return m

    def isotropic(self, albedo):
        m = self._b.isotropic(albedo)
        self.materials[m] = ("texture", albedo, f32(1))
        return m

    def diffuse_light(self, emission, brightness):
        m = self._b.diffuse_light(emission, brightness)
        self.materials[m] = ("light", emission, f32(brightness))
        return m

    def metal(self, albedo, fuzz):
        m = self._b.metal(albedo, fuzz)
        self.materials[m] = ("colour", self._c(albedo))
        return m

    def dielectric(self, ref_idx):
        m = self._b.dielectric(ref_idx)
        self.materials[m] = ("colour", np.ones(3, f32))
        return m


def _perlin_turb(oracle, rb, q):
    fn = oracle.lib.rto_debug_perlin_turb
    fn.restype, fn.argtypes = C.c_float, [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    out = np.zeros(len(q), f32)
    for i, p in enumerate(q):
        out[i] = fn(rb.h, (C.c_float * 3)(*[float(c) for c in p]), 7)
    return out


def eval_texture(oracle, rb, tex, p):
    """The texture `tex` at the points p (float32 [n, 3]) -> float32 [n, 3] (texture.rs): constant textures directly, checker
    textures through the oracle's pinned sine (debug_math op 2), Perlin textures through the oracle's turbulence of scale * p."""
    p = np.ascontiguousarray(p, dtype=f32)
    rec = rb.textures[tex]
    if rec[0] == "constant":
        return np.broadcast_to(rec[1], p.shape).astype(f32)
    if rec[0] == "perlin":
        return np.repeat(_perlin_turb(oracle, rb, (rec[1] * p).astype(f32))[:, None], 3, axis=1)
    q = (f32(10) * p).astype(f32)
    sn = oracle.debug_math(2, q.ravel()).reshape(-1, 3)
    s = ((sn[:, 0] * sn[:, 1]).astype(f32) * sn[:, 2]).astype(f32)
    return np.where((s < 0)[:, None], eval_texture(oracle, rb, rec[2], p), eval_texture(oracle, rb, rec[1], p)).astype(f32)


def albedo_of(oracle, rb, mat, p):
    """What the feature pass calls the albedo of material handles `mat` (uint32 [n]) at p (float32 [n, 3]): Lambertian and
    Isotropic the texture, Metal its colour, Dielectric (1, 1, 1), DiffuseLight brightness * texture."""
    out = np.zeros((len(mat), 3), f32)
    for m in np.unique(mat):
        at = mat == m
        rec = rb.materials[int(m)]
        if rec[0] == "colour":
            out[at] = rec[1]
        else:
            t = eval_texture(oracle, rb, rec[1], p[at])
            out[at] = (rec[2] * t).astype(f32) if rec[0] == "light" else t
    return out


def build_recorded(pkg, oracle, name_or_fn, nx, ny):
    """A scene case (scene_cases.CASES name, or a (pkg, b, nx, ny) builder function) on the oracle through a RecordingBuilder:
    (recording builder, oracle scene, camera)."""
    fn = CASES[name_or_fn][0] if isinstance(name_or_fn, str) else name_or_fn
    rb = RecordingBuilder(oracle.builder())
    world, cam, _ = fn(pkg, rb, nx, ny)
    return rb, rb.scene(world), cam


_planes = {}


def reference_planes(pkg, oracle, name, nx, ny, grid, seed=0xDEADBEEF, t_near=0.001):
    """(albedo [ny, nx, 3], normal [ny, nx, 3], depth [ny, nx], missed) of scene case `name`: the rays of
    features.subpixel_rays, ordered by pixel index y * nx + x for the oracle's debug_hit_top (whose RNG stream is keyed by the
    ray's index), the albedo evaluator and the fold.  Computed once per argument set; callers must not write the arrays."""
    key = (name, nx, ny, grid, seed, t_near)
    if key in _planes:
        return _planes[key]
    rb, so, cam = build_recorded(pkg, oracle, name, nx, ny)
    rays = pkg.features.subpixel_rays(cam, nx, ny, grid)
    g2, n = grid * grid, nx * ny
    vals, hits = np.zeros((g2, ny, nx, 7), f32), np.zeros((g2, ny, nx), bool)
    for k in range(g2):
        by_pixel = rays[k][::-1].reshape(n, 7)   # row = ny - 1 - y: rows reversed = ascending y, then x
        out, mat = so.debug_hit_top(by_pixel, seed=seed, t_near=t_near)
        hit = out[:, 0] != 0
        v = np.zeros((n, 7), f32)
        v[hit, 0:3] = albedo_of(oracle, rb, mat[hit], out[hit, 2:5])
        v[hit, 3:6] = out[hit, 5:8]
        v[hit, 6] = out[hit, 1]
        vals[k] = v.reshape(ny, nx, 7)[::-1]
        hits[k] = hit.reshape(ny, nx)[::-1]
    planes = pkg.features.fold(vals, hits)
    missed = int((~hits.any(axis=0)).sum())
    res = (np.ascontiguousarray(planes[..., 0:3]), np.ascontiguousarray(planes[..., 3:6]), np.ascontiguousarray(planes[..., 6]), missed)
    for a in res[:3]:
        a.setflags(write=False)
    _planes[key] = res
    return res
