"""Per-pixel noise estimates from the running sums of a frame rendered with RTG_FLAG_SUM_SQUARES (include/rtiow_gpu.h).

A pixel's n samples c_1 .. c_n give, per channel, the running sum S = sum c_i (plane 0 of a PARTIAL call) and the running sum
of squares Q = sum c_i^2 (plane 1).  From (S, Q, n):

    mean            m  = S / n
    sample variance s2 = max(0, (Q - n m^2) / (n - 1))      (clamped: cancellation may round below zero)
    standard error  se = sqrt(s2 / n)                        (of the pixel's mean; +inf for n = 1)

and the frame's estimated RMS error against the converged image is sqrt(mean over pixels and channels of se^2).
Everything is computed in float64.  With RTG_FLAG_SAMPLE_COUNTS every pixel has its own n (standard_error_counts), and
adaptive sampling retires a pixel once its estimate -- or, with a radius, every estimate around it -- is good enough (retire;
RTG_FLAG_RETIRE runs the same rule on the device).  retire_filtered is the rule on the error plane of a filtered frame
(RTG_FLAG_DENOISE_ERROR).
"""
import numpy as np


def standard_error(sum_, sq, n):
    """Standard error of every pixel's mean, per channel: float64 array of the shape of `sum_`."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    s = np.asarray(sum_, dtype=np.float64)
    q = np.asarray(sq, dtype=np.float64)
    if n == 1:
        return np.full(s.shape, np.inf)
    m = s / n
    var = np.maximum(0.0, (q - n * m * m) / (n - 1))
    return np.sqrt(var / n)


def estimated_rmse(sum_, sq, n):
    """sqrt(mean of standard_error^2 over pixels and channels): the estimated RMS error of the frame's mean image."""
    se = standard_error(sum_, sq, n)
    return float(np.sqrt(np.mean(se * se)))


def standard_error_counts(sum_, sq, counts):
    """standard_error with a per-pixel sample count: `counts` has the shape of `sum_` without its last (channel) axis.
    +inf where a pixel holds fewer than 2 samples."""
    s = np.asarray(sum_, dtype=np.float64)
    q = np.asarray(sq, dtype=np.float64)
    n = np.asarray(counts, dtype=np.float64)[..., None]
    if n.shape[:-1] != s.shape[:-1]:
        raise ValueError("counts must have the shape of sum_ without its channel axis")
    ok = n >= 2
    nn = np.where(ok, n, 2.0)
    m = s / nn
    var = np.maximum(0.0, (q - nn * m * m) / (nn - 1))
    return np.where(ok, np.sqrt(var / nn), np.inf)


def retire(active, k, stderr, min_samples, target_se, radius=0, present=None):
    """The retire rule of adaptive sampling (Scene.adaptive), after the slice that ends at k samples: the active pixels with
    k >= min_samples whose largest per-channel standard error is <= target_se.  Returns a bool mask of the pixel grid.
    radius > 0: every pixel of the (2 radius + 1)^2 window around a pixel (clipped to the image) must meet the target, not only
    the pixel itself.  present: bool mask of the pixels that are part of the frame (n > 0; default: all); the others never
    veto a window.  This is the rule include/rtiow_gpu.h RTG_FLAG_RETIRE applies on the device (with a finite target_se)."""
    active = np.asarray(active, dtype=bool)
    if k < min_samples:
        return np.zeros_like(active)
    ok = np.max(np.asarray(stderr, dtype=np.float64), axis=-1) <= target_se
    if present is not None:
        ok |= ~np.asarray(present, dtype=bool)
    if radius:
        ok = window_all(ok, int(radius))
    return active & ok


def retire_filtered(active, k, ev, counts, min_samples, target_se, radius=0):
    """The retire rule of RTG_FLAG_RETIRE | RTG_FLAG_DENOISE | RTG_FLAG_DENOISE_ERROR, after the slice that ends at k samples:
    `ev` (float32 [ny, nx, 3]) is the error plane the filter wrote (denoise.nlm_error), `counts` the count plane n.  A pixel
    is OK when its three ev are finite and float64(ev) <= target_se * target_se (the float64 product; no square root); pixels
    with n == 0 are not part of the frame and never veto a window.  Returns the bool mask of the active pixels with
    k >= min_samples whose (2 radius + 1)^2 window, clipped to the image, is OK."""
    active = np.asarray(active, dtype=bool)
    if k < min_samples:
        return np.zeros_like(active)
    e = np.asarray(ev, dtype=np.float32)
    target2 = float(target_se) * float(target_se)
    ok = np.isfinite(e).all(axis=-1) & (e.astype(np.float64) <= target2).all(axis=-1)
    ok |= np.asarray(counts) == 0
    if radius:
        ok = window_all(ok, int(radius))
    return active & ok


def filtered_estimate(ev, counts):
    """(estimated, sum_se2) of the retire block under RTG_FLAG_DENOISE_ERROR: the pixels with n > 0 and three finite ev, and the
    sum of (float64(ev_0) + ev_1) + ev_2 over them (here in numpy's order: the library's fixed order agrees to rounding);
    sqrt(sum_se2 / (3 estimated)) is the estimated RMSE of the filtered frame."""
    e = np.asarray(ev, dtype=np.float32).astype(np.float64)
    est = np.isfinite(e).all(axis=-1) & (np.asarray(counts) > 0)
    return int(est.sum()), float(((e[..., 0] + e[..., 1]) + e[..., 2])[est].sum())


def window_all(ok, radius):
    """AND of a bool [ny, nx] grid over the (2 radius + 1)^2 window of every pixel, clipped to the grid (rows, then columns)."""
    ny, nx = ok.shape
    r = int(radius)
    pad = np.ones((ny + 2 * r, nx + 2 * r), dtype=bool)
    pad[r:r + ny, r:r + nx] = ok
    rows = np.ones((ny + 2 * r, nx), dtype=bool)
    for d in range(2 * r + 1):
        rows &= pad[:, d:d + nx]
    out = np.ones((ny, nx), dtype=bool)
    for d in range(2 * r + 1):
        out &= rows[d:d + ny]
    return out
