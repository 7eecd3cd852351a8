"""The filter of RTG_FLAG_DENOISE (include/rtiow_gpu.h) in numpy: a variance-driven non-local-means filter (Rousselle, Knaus,
Zwicker, "Adaptive rendering with non-local means filtering", 2012) over the pixel means and the variances of those means,
which a RTG_FLAG_SUM_SQUARES frame already holds.  This is the normative definition: the library's output plane equals nlm()
bit for bit.  Everything is float32 and every operation is rounded on its own; the weight is the n = 4 member of
(1 - x / n)^n -> exp(-x), so no transcendental function takes part."""
import numpy as np

f32 = np.float32


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx]; `fill` where (y + dy, x + dx) lies outside the image."""
    ny, nx = a.shape[:2]
    out = np.full_like(a, fill)
    y0, y1 = max(0, -dy), min(ny, ny - dy)
    x0, x1 = max(0, -dx), min(nx, nx - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def mean_var(sum_, sq, held):
    """(m, v, valid) of a frame's running sums [ny, nx, 3], sums of squares [ny, nx, 3] and held samples e [ny, nx]: the pixel
    means m = S / e, the variances of those means v = max(0, Q - S m) / (e (e - 1)) (0 where not valid) and which pixels take
    part in the filter: e >= 2 and three finite m and v.  Pixels with e = 0 get m = S."""
    s, q = np.asarray(sum_, dtype=f32), np.asarray(sq, dtype=f32)
    e = np.asarray(held, dtype=np.uint32)
    ef = np.maximum(e, 1).astype(f32)[..., None]
    with np.errstate(all="ignore"):
        m = s / ef
        d = q - s * m
        d = np.where(d > 0, d, f32(0))
        v = d / (ef * (ef - f32(1)))
    valid = (e >= 2) & np.isfinite(m).all(axis=-1) & np.isfinite(v).all(axis=-1)
    return m.astype(f32), np.where(valid[..., None], v, f32(0)).astype(f32), valid


def nlm(sum_, sq, held, radius=5, patch=2, k=0.7):
    """The filtered frame, float32 [ny, nx, 3]: for every valid pixel the weighted mean of the valid pixels of its
    (2 radius + 1)^2 window, the weight of a neighbour falling with the variance-normalised distance of the (2 patch + 1)^2
    patches around the two; every other pixel keeps its mean m."""
    m, v, valid = mean_var(sum_, sq, held)
    ny, nx = valid.shape
    mz = np.where(valid[..., None], m, f32(0)).astype(f32)
    k2, eps = f32(k) * f32(k), f32(1e-10)
    acc, wsum = np.zeros((ny, nx, 3), f32), np.zeros((ny, nx), f32)
    R, F = int(radius), int(patch)
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                mb, vb = _shift(mz, dy, dx, f32(0)), _shift(v, dy, dx, f32(0))
                pv = valid & _shift(valid, dy, dx, False)
                diff = mz - mb
                d2 = (diff * diff - (v + np.minimum(vb, v))) / (eps + k2 * (v + vb))
                pd = np.where(pv, (d2[..., 0] + d2[..., 1]) + d2[..., 2], f32(0)).astype(f32)
                pc = pv.astype(np.int32)
                r, rc = np.zeros((ny, nx), f32), np.zeros((ny, nx), np.int32)
                for ox in range(-F, F + 1):
                    r, rc = r + _shift(pd, 0, ox, f32(0)), rc + _shift(pc, 0, ox, 0)
                dsum, cnt = np.zeros((ny, nx), f32), np.zeros((ny, nx), np.int32)
                for oy in range(-F, F + 1):
                    dsum, cnt = dsum + _shift(r, oy, 0, f32(0)), cnt + _shift(rc, oy, 0, 0)
                x = dsum / (f32(3) * cnt.astype(f32))
                x = np.where(x > 0, x, f32(0))
                u = f32(1) - x * f32(0.25)
                u = np.where(u > 0, u, f32(0))
                u2 = u * u
                w = np.where(pv, u2 * u2, f32(0)).astype(f32)
                acc, wsum = acc + w[..., None] * mb, wsum + w
        out = np.where(valid[..., None], acc / np.where(valid, wsum, f32(1))[..., None], m)
    return out.astype(f32)


def denoise(frame_or_planes, held, radius=5, patch=2, k=0.7):
    """nlm() of a frame's planes: `frame_or_planes` is a float32 [2, ny, nx, 3] array (running sums, sums of squares) or an
    object with such a `planes` view (capi.CountsFrame / capi.DenoiseFrame); `held` the samples every pixel holds, an int or a
    [ny, nx] array."""
    planes = np.asarray(getattr(frame_or_planes, "planes", frame_or_planes))
    if planes.ndim != 4 or planes.shape[0] != 2 or planes.shape[-1] != 3:
        raise ValueError("denoise needs the two planes of a squares=True frame: [2, ny, nx, 3]")
    e = np.broadcast_to(np.asarray(held, dtype=np.uint32), planes.shape[1:3])
    return nlm(planes[0], planes[1], e, radius, patch, k)
