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


def feature_weight(albedo, normal, depth, dy, dx, sigma_normal, sigma_albedo, sigma_depth):
    """The guided filter's weight of every pixel p with q = p + (dy, dx), float32 [ny, nx]: the n = 4 member of
    (1 - x / n)^n at x = the largest of the three squared feature distances, each over its sigma squared; 1 where any of the
    fourteen feature values is not finite.  (q outside the image: zeros take its place; the colour weight is 0 there.)"""
    a, n, z = np.asarray(albedo, dtype=f32), np.asarray(normal, dtype=f32), np.asarray(depth, dtype=f32)
    sn, sa, sz = f32(sigma_normal), f32(sigma_albedo), f32(sigma_depth)
    fin = np.isfinite(a).all(axis=-1) & np.isfinite(n).all(axis=-1) & np.isfinite(z)
    with np.errstate(all="ignore"):
        dn, da = n - _shift(n, dy, dx, f32(0)), a - _shift(a, dy, dx, f32(0))
        zq = _shift(z, dy, dx, f32(0))
        xn = ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]) / (sn * sn)
        xa = ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) / (sa * sa)
        dz, s = z - zq, z + zq
        xz = ((dz * dz) / (s * s + f32(1e-20))) / (sz * sz)
        x = xn
        x = np.where(xa > x, xa, x)
        x = np.where(xz > x, xz, x)
        u = f32(1) - x * f32(0.25)
        u = np.where(u > 0, u, f32(0))
        wf = (u * u) * (u * u)
    return np.where(fin & _shift(fin, dy, dx, True), wf, f32(1)).astype(f32)


def _nlm(sum_, sq, held, radius, patch, k, guide=None, error=False):
    """The loop of nlm / nlm_guided (guide = (albedo, normal, depth, sigma_normal, sigma_albedo, sigma_depth)): (out, ev), ev the
    error plane of nlm_error when `error`, else None."""
    m, v, valid = mean_var(sum_, sq, held)
    ny, nx = valid.shape
    mz = np.where(valid[..., None], m, f32(0)).astype(f32)
    k2, eps = f32(k) * f32(k), f32(1e-10)
    acc, wsum = np.zeros((ny, nx, 3), f32), np.zeros((ny, nx), f32)
    acc2 = np.zeros((ny, nx, 3), f32)
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
                w = u2 * u2
                if guide is not None:
                    wf = feature_weight(guide[0], guide[1], guide[2], dy, dx, guide[3], guide[4], guide[5])
                    w = np.where(wf < w, wf, w)
                w = np.where(pv, w, f32(0)).astype(f32)
                acc, wsum = acc + w[..., None] * mb, wsum + w
                if error:
                    acc2 = acc2 + (w * w)[..., None] * vb
        one = np.where(valid, wsum, f32(1))[..., None]
        out = np.where(valid[..., None], acc / one, m).astype(f32)
        ev = None
        if error:
            ev = np.where(valid[..., None], (acc2 / one) / one, f32(np.inf)).astype(f32)
    return out, ev


def nlm(sum_, sq, held, radius=5, patch=2, k=0.7):
    """The filtered frame, float32 [ny, nx, 3]: for every valid pixel the weighted mean of the valid pixels of its
    (2 radius + 1)^2 window, the weight of a neighbour falling with the variance-normalised distance of the (2 patch + 1)^2
    patches around the two; every other pixel keeps its mean m."""
    return _nlm(sum_, sq, held, radius, patch, k)[0]


def nlm_error(sum_, sq, held, radius=5, patch=2, k=0.7):
    """(out, ev) of RTG_FLAG_DENOISE_ERROR: out is nlm() bit for bit; ev, float32 [ny, nx, 3], the variance of every filtered
    pixel with the weights taken as given -- for out = sum_q w_q m_q / sum_q w_q it is sum_q w_q^2 v_q / (sum_q w_q)^2.  Per
    displacement, after the pair's final weight w (the mask of valid pairs included): acc2 = acc2 + (w * w) * v_q from +0; after
    the loop ev = (acc2 / wsum) / wsum.  +inf in the three channels of every pixel that is not valid (the library leaves the
    plane of pixels with e = 0 alone)."""
    return _nlm(sum_, sq, held, radius, patch, k, error=True)


def nlm_guided(sum_, sq, held, albedo, normal, depth, radius=5, patch=2, k=0.7, sigma_normal=0.1, sigma_albedo=0.1,
               sigma_depth=0.1):
    """nlm() guided by first-hit feature planes (RTG_FLAG_DENOISE | RTG_FLAG_FEATURES): albedo and normal float32 [ny, nx, 3],
    depth float32 [ny, nx].  The one change: after the colour weight w of a displacement is computed and before the mask of
    valid pairs, w = wf < w ? wf : w with wf = feature_weight() of the pair.  Sigmas of 1e18 give nlm() bit for bit."""
    return _nlm(sum_, sq, held, radius, patch, k, (albedo, normal, depth, sigma_normal, sigma_albedo, sigma_depth))[0]


def nlm_guided_error(sum_, sq, held, albedo, normal, depth, radius=5, patch=2, k=0.7, sigma_normal=0.1, sigma_albedo=0.1,
                     sigma_depth=0.1):
    """(out, ev) of RTG_FLAG_DENOISE_ERROR | RTG_FLAG_FEATURES: nlm_error() with nlm_guided()'s weights (the feature cap is
    part of the final weight)."""
    return _nlm(sum_, sq, held, radius, patch, k, (albedo, normal, depth, sigma_normal, sigma_albedo, sigma_depth), error=True)


def denoise(frame_or_planes, held, radius=5, patch=2, k=0.7):
    """nlm() of a frame's planes: `frame_or_planes` is a float32 [2, ny, nx, 3] array (running sums, sums of squares) or an
    object with such a `planes` view (capi.CountsFrame / capi.DenoiseFrame); `held` the samples every pixel holds, an int or a
    [ny, nx] array."""
    planes = np.asarray(getattr(frame_or_planes, "planes", frame_or_planes))
    if planes.ndim != 4 or planes.shape[0] != 2 or planes.shape[-1] != 3:
        raise ValueError("denoise needs the two planes of a squares=True frame: [2, ny, nx, 3]")
    e = np.broadcast_to(np.asarray(held, dtype=np.uint32), planes.shape[1:3])
    return nlm(planes[0], planes[1], e, radius, patch, k)
