"""An independent float64 statement of the image texture (include/rtiow_gpu_image.h), for test_fuzz_mesh.py (the numpy definition
image.sample and the host probe, on the CPU) and test_fuzz_mesh_gpu.py (the device probe, the feature planes).  It is written
from the header's CONVENTIONS, not from image.py's operations, and shares no code with the package:

  the image       [h, w, 3], row 0 at the top: texel (i, j) covers the cell [i, i + 1) x [j, j + 1) of the texel plane, its
                  centre is (i + 0.5, j + 0.5); x = u w runs to the right, y = (1 - v) h runs DOWN (v = 1 is the top edge)
  planar          u = p . (m0, m1, m2) + m3,  v = p . (m4, m5, m6) + m7 (a plain dot product)
  spherical       d = p - (m0, m1, m2);  phi = arctan2(d.z, d.x), theta = arctan2(d.y, hypot(d.x, d.z));
                  u = 0.5 - phi / (2 pi) (u falls as phi grows; the seam u = 0 | 1 is the half plane d.x < 0, d.z = 0),
                  v = 0.5 + theta / pi (the +y pole is the top row)
  nearest         the texel whose cell holds (x, y)
  bilinear        the tent-weighted sum over the four texel centres around (x, y): weight max(0, 1 - |x - (i + 0.5)|) times
                  max(0, 1 - |y - (j + 0.5)|)
  wraps           on the indices: repeat = the index modulo the side, clamp = the index held inside 0 .. side - 1

sample64 returns the value and a margin.  Nearest: the distance of x and of y, in texels, from the next integer at which the
texel changes (none on a side of one texel; under clamp only the integers 1 .. side - 1 are such).  Bilinear is continuous:
its margin is infinite.

`fault=` plants a wrong convention (test_the_image_checks_notice_planted_faults only): "v_unflipped" (y = v h), "no_half_texel"
(bilinear centres at the integers), "phi_sign" (u = 0.5 + phi / (2 pi)), "clamp_as_repeat".

Measured here on the CPU against image.sample (float32), image_cases.image(size) x image_cases.settings(size), 4096 random
points in +-4 per case (test_fuzz_mesh.py prints them):
    nearest   exact at every point whose margin exceeds NEAREST_MARGIN = 1e-4 texel; at most 0.10 % of a case's points are left
              out (cap physics_ref.CAP_RAYS = 5 %)
    bilinear  worst absolute deviation per size   1x1 2.3e-16   2x3 1.4e-06   5x4 1.7e-06   8x8 2.4e-06   64x64 2.2e-05
              (1x1: the float64 rounding of the four weights' sum; else the error is the float32 rounding of x and y, of
              order 1e-7 |u| w texels, times the texel differences: it grows with the side)
BILINEAR_TOL is 4 x the worst of each size, the project's rule."""
import numpy as np

F = np.float64
PLANAR, SPHERICAL = 0, 1
NEAREST, BILINEAR = 0, 1
REPEAT, CLAMP = 0, 1
FAULTS = ("v_unflipped", "no_half_texel", "phi_sign", "clamp_as_repeat")
NEAREST_MARGIN = 1e-4
BILINEAR_WORST = {(1, 1): 2.3e-16, (2, 3): 1.4e-6, (5, 4): 1.7e-6, (8, 8): 2.4e-6, (64, 64): 2.2e-5}      # measured: see the docstring
BILINEAR_TOL = {size: 4 * worst for size, worst in BILINEAR_WORST.items()}


def texel_xy(prm, w, h, p, fault=None):
    """(x, y) of the points p [n, 3] in the texel plane."""
    p = np.asarray(p, F).reshape(-1, 3)
    m = np.asarray(prm["m"], F)
    if prm["mapping"] == SPHERICAL:
        d = p - m[0:3]
        phi = np.arctan2(d[:, 2], d[:, 0])
        theta = np.arctan2(d[:, 1], np.hypot(d[:, 0], d[:, 2]))
        u = 0.5 + phi / (2.0 * np.pi) if fault == "phi_sign" else 0.5 - phi / (2.0 * np.pi)
        v = 0.5 + theta / np.pi
    else:
        u = p @ m[0:3] + m[3]
        v = p @ m[4:7] + m[7]
    return u * w, (v if fault == "v_unflipped" else 1.0 - v) * h


def _index(k, side, mode, fault):
    if mode == CLAMP and fault != "clamp_as_repeat":
        return np.minimum(np.maximum(k, 0), side - 1)
    return k % side


def _change(x, side, mode):
    """The distance of x from the next integer at which the nearest texel changes."""
    if side == 1:
        return np.full(len(x), np.inf)
    edge = np.rint(x)
    if mode == CLAMP:
        edge = np.clip(edge, 1, side - 1)
    return np.abs(x - edge)


def sample64(img, prm, p, fault=None):
    """(value [n, 3], margin [n]) of the image texture (img [h, w, 3], prm: mapping, filter, wrap_u, wrap_v, m) at p [n, 3]."""
    img = np.asarray(img, F)
    h, w = img.shape[0], img.shape[1]
    x, y = texel_xy(prm, w, h, p, fault)
    if prm["filter"] == NEAREST:
        i = _index(np.floor(x).astype(np.int64), w, prm["wrap_u"], fault)
        j = _index(np.floor(y).astype(np.int64), h, prm["wrap_v"], fault)
        return img[j, i], np.minimum(_change(x, w, prm["wrap_u"]), _change(y, h, prm["wrap_v"]))
    half = 0.0 if fault == "no_half_texel" else 0.5
    i0, j0 = np.floor(x - half).astype(np.int64), np.floor(y - half).astype(np.int64)
    out = np.zeros((len(x), 3))
    for dj in (0, 1):
        for di in (0, 1):
            wx = np.maximum(0.0, 1.0 - np.abs(x - (i0 + di + half)))
            wy = np.maximum(0.0, 1.0 - np.abs(y - (j0 + dj + half)))
            out += (wx * wy)[:, None] * img[_index(j0 + dj, h, prm["wrap_v"], fault), _index(i0 + di, w, prm["wrap_u"], fault)]
    return out, np.full(len(x), np.inf)


def texel_shift(prm, w, h, p, dp):
    """(dx, dy) [n]: how far, in texels, a displacement of p by at most dp [n] on every axis can move (x, y).  Planar: x = w (a . p
    + c), so |dx| <= w |a|_1 dp.  Spherical: an angle about an axis moves by at most |delta| / (the distance from that axis),
    |delta| <= sqrt(2) dp in the xz plane and sqrt(3) dp in space: |dx| <= w sqrt(2) dp / (2 pi rho), |dy| <= h sqrt(3) dp / (pi r)."""
    p = np.asarray(p, F).reshape(-1, 3)
    m = np.asarray(prm["m"], F)
    if prm["mapping"] == SPHERICAL:
        d = p - m[0:3]
        rho, r = np.hypot(d[:, 0], d[:, 2]), np.sqrt((d * d).sum(axis=1))
        with np.errstate(divide="ignore"):
            return w * np.sqrt(2.0) * dp / (2.0 * np.pi * rho), h * np.sqrt(3.0) * dp / (np.pi * r)
    return w * np.abs(m[0:3]).sum() * dp, h * np.abs(m[4:7]).sum() * dp


def bilinear_allowance(img, prm, p, dp):
    """How far the bilinear value at p can move when p moves by at most dp [n] on every axis: the local slope of the tent sum
    -- at most the largest difference of neighbouring texels, per axis, among the 4 x 4 texels around (x, y): the cell that holds
    the point and the cells beside it, which a shift below one texel can reach -- times texel_shift.  Infinite where the shift
    is a texel or more."""
    img = np.asarray(img, F)
    h, w = img.shape[0], img.shape[1]
    x, y = texel_xy(prm, w, h, p)
    i0, j0 = np.floor(x - 0.5).astype(np.int64), np.floor(y - 0.5).astype(np.int64)
    ii = np.stack([_index(i0 + k, w, prm["wrap_u"], None) for k in (-1, 0, 1, 2)], axis=1)     # [n, 4]
    jj = np.stack([_index(j0 + k, h, prm["wrap_v"], None) for k in (-1, 0, 1, 2)], axis=1)
    t = img[jj[:, :, None], ii[:, None, :]]                                                    # [n, 4 (j), 4 (i), 3]
    sx = np.abs(np.diff(t, axis=2)).max(axis=(1, 2, 3))
    sy = np.abs(np.diff(t, axis=1)).max(axis=(1, 2, 3))
    dx, dy = texel_shift(prm, w, h, p, dp)
    with np.errstate(invalid="ignore"):
        out = np.where(sx > 0, sx * dx, 0.0) + np.where(sy > 0, sy * dy, 0.0)
    return np.where((dx < 1.0) & (dy < 1.0) | ((sx == 0) & (sy == 0)), out, np.inf)
