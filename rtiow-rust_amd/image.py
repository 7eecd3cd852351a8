"""Image textures (include/rtiow_gpu_image.h; Builder.image): the definition in numpy, and ways to make an image.  Numpy only.

`sample` and `atan2f` ARE the specification of the image kind: the library's sampler (csrc/rt_image.h) and its rt_atan2f
(csrc/rt_libm.h) equal them bit for bit, on the host and on the device.  Every float32 operation is rounded on its own and
written in the header's operand order; numpy never contracts a multiply and an add.

An image is float32 [h, w, 3], row 0 at the top -- the layout of the frames the library renders, so a frame is a texture as it
stands.  `from_u8` brings an 8-bit picture in; `bake` turns any Python closure of the point p into an image.
"""
import numpy as np

f32 = np.float32
f64 = np.float64

PLANAR, SPHERICAL = 0, 1
NEAREST, BILINEAR = 0, 1
REPEAT, CLAMP = 0, 1
MAX_SIDE, MAX_TEXELS = 16384, 1 << 24

INV_2PI = f32(1.0 / (2.0 * np.pi))  # the float32 nearest to 1 / (2 pi) and to 1 / pi
INV_PI = f32(1.0 / np.pi)
_TAN_PI_8 = f64(0.41421356237309503)
_PI_4, _PI_2, _PI = f64(0.78539816339744828), f64(1.5707963267948966), f64(3.1415926535897931)


class ImageParams(dict):
    """The in-fields of rtg_image_params as a dict: mapping, filter, wrap_u, wrap_v, m (eight floats)."""


def params(mapping=PLANAR, filter=BILINEAR, wrap_u=REPEAT, wrap_v=REPEAT, m=None, reserved_in=0):
    m = np.zeros(8, dtype=f32) if m is None else np.asarray(m, dtype=f32).reshape(-1)
    if m.size < 8:
        m = np.concatenate([m, np.zeros(8 - m.size, dtype=f32)])
    return ImageParams(mapping=int(mapping), filter=int(filter), wrap_u=int(wrap_u), wrap_v=int(wrap_v), m=m[:8].copy(),
                       reserved_in=int(reserved_in))


def planar(u_axis, u_offset, v_axis, v_offset, **kw):
    """u = dot(p, u_axis) + u_offset, v = dot(p, v_axis) + v_offset."""
    return params(PLANAR, m=[u_axis[0], u_axis[1], u_axis[2], u_offset, v_axis[0], v_axis[1], v_axis[2], v_offset], **kw)


def spherical(centre=(0.0, 0.0, 0.0), **kw):
    """The book's get_sphere_uv about `centre`."""
    return params(SPHERICAL, m=[centre[0], centre[1], centre[2]], **kw)


def atan2f(y, x):
    """rt_atan2f (csrc/rt_libm.h): float64 inside -- one divide and the Taylor series of atan on |t| <= tan(pi/8) -- rounded to
    float32 once.  (+-0, +-0), the infinities and NaN as C's atan2f."""
    y, x = np.broadcast_arrays(np.asarray(y, dtype=f32), np.asarray(x, dtype=f32))
    with np.errstate(all="ignore"):
        nan = np.isnan(x) | np.isnan(y)
        neg_x, neg_y = np.signbit(x), np.signbit(y)
        ax, ay = np.abs(x.astype(f64)), np.abs(y.astype(f64))
        inf = np.isinf(ax) | np.isinf(ay)
        ax, ay = np.where(inf, np.where(np.isinf(ax), 1.0, 0.0), ax), np.where(inf, np.where(np.isinf(ay), 1.0, 0.0), ay)
        swap = ay > ax
        n, d = np.where(swap, ax, ay), np.where(swap, ay, ax)
        upper = n > _TAN_PI_8 * d
        num, den = np.where(upper, n - d, n), np.where(upper, n + d, d)
        t = np.where(num == 0.0, 0.0, num / np.where(num == 0.0, 1.0, den))
        z = t * t
        s = f64(1.0) / f64(43.0)
        for k in range(41, 0, -2):
            s = f64(1.0) / f64(k) - z * s
        r = t * s
        r = np.where(upper, _PI_4 + r, r)
        r = np.where(swap, _PI_2 - r, r)
        r = np.where(neg_x, _PI - r, r)
        r = np.where(neg_y, -r, r)
        out = r.astype(f32)
        return np.where(nan, x + y, out)


def as_i32(f):
    """Rust's `as i32`: saturating, NaN -> 0 (csrc/rt_trace.h f32_as_i32).  Returns int64."""
    f = np.asarray(f, dtype=f32)
    with np.errstate(invalid="ignore"):
        g = np.where(np.isnan(f), f32(0.0), f).astype(f64)
    return np.clip(np.trunc(g), -2147483648.0, 2147483647.0).astype(np.int64)


def wrap(i, n, mode):
    """In 64 bits: repeat = the Euclidean remainder, clamp = min(max(i, 0), n - 1)."""
    i = np.asarray(i, dtype=np.int64)
    return np.clip(i, 0, n - 1) if mode == CLAMP else np.mod(i, np.int64(n))


def uv(prm, p):
    """(u, v) of the points p [n, 3] under the mapping of `prm`: float32 [n] each."""
    p = np.asarray(p, dtype=f32).reshape(-1, 3)
    m = np.asarray(prm["m"], dtype=f32)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        if prm["mapping"] == SPHERICAL:
            dx, dy, dz = px - m[0], py - m[1], pz - m[2]
            phi = atan2f(dz, dx)
            rho = np.sqrt(dx * dx + dz * dz)
            theta = atan2f(dy, rho)
            return f32(0.5) - phi * INV_2PI, f32(0.5) + theta * INV_PI
        u = ((px * m[0] + py * m[1]) + pz * m[2]) + m[3]
        v = ((px * m[4] + py * m[5]) + pz * m[6]) + m[7]
        return u, v


def sample(img, prm, p):
    """The value of the image texture (img, prm) at the points p [n, 3]: float32 [n, 3].  THE definition."""
    img = np.asarray(img, dtype=f32)
    h, w = img.shape[0], img.shape[1]
    u, v = uv(prm, p)
    with np.errstate(all="ignore"):
        x = u * f32(w)
        y = (f32(1.0) - v) * f32(h)
        if prm["filter"] == NEAREST:
            i = wrap(as_i32(np.floor(x)), w, prm["wrap_u"])
            j = wrap(as_i32(np.floor(y)), h, prm["wrap_v"])
            return img[j, i].copy()
        x, y = x - f32(0.5), y - f32(0.5)
        fx, fy = np.floor(x), np.floor(y)
        tx, ty = (x - fx)[:, None], (y - fy)[:, None]
        i0, j0 = as_i32(fx), as_i32(fy)
        i1, j1 = wrap(i0 + 1, w, prm["wrap_u"]), wrap(j0 + 1, h, prm["wrap_v"])
        i0, j0 = wrap(i0, w, prm["wrap_u"]), wrap(j0, h, prm["wrap_v"])
        a = img[j0, i0] + tx * (img[j0, i1] - img[j0, i0])
        b = img[j1, i0] + tx * (img[j1, i1] - img[j1, i0])
        return (a + ty * (b - a)).astype(f32)


def from_u8(img, gamma=True):
    """An 8-bit picture [h, w, 3] as float32 texels.  gamma=True inverts rtg_tonemap's quantisation (sqrt, then * 255.99):
    (b / 255)^2; gamma=False is b / 255."""
    x = np.asarray(img, dtype=np.uint8).astype(f32) / f32(255.0)
    return (x * x).astype(f32) if gamma else x


def texel_centres(prm, w, h):
    """The points p [h * w, 3] whose (u, v) under the PLANAR mapping `prm` are the texel centres ((i + 0.5) / w,
    1 - (j + 0.5) / h), row-major from the top row: the minimum-norm solution of the two mapping equations (in float64,
    rounded to float32), so p lies in the plane spanned by the two axes."""
    if prm["mapping"] != PLANAR:
        raise ValueError("texel_centres needs a planar mapping")
    m = np.asarray(prm["m"], dtype=f64)
    a = np.stack([m[0:3], m[4:7]])
    if np.linalg.matrix_rank(a) < 2:
        raise ValueError("the mapping's u and v axes are parallel or zero")
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    uvs = np.stack([(ii.reshape(-1) + 0.5) / w - m[3], 1.0 - (jj.reshape(-1) + 0.5) / h - m[7]])
    return (np.linalg.pinv(a) @ uvs).T.astype(f32)


def bake(fn, prm, w, h):
    """Evaluate the closure fn(p [n, 3]) -> [n, 3] at the texel centres of the planar mapping `prm`: float32 [h, w, 3].  With
    the nearest filter the image texture then returns fn at the centre of the texel p falls into."""
    out = np.asarray(fn(texel_centres(prm, w, h)), dtype=f32)
    return np.ascontiguousarray(np.broadcast_to(out.reshape(h * w, -1), (h * w, 3)).reshape(h, w, 3))
