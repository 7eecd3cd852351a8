"""Per-pixel noise estimates from the running sums of a frame rendered with RTG_FLAG_SUM_SQUARES (include/rtiow_gpu.h).

A pixel's n samples c_1 .. c_n give, per channel, the running sum S = sum c_i (plane 0 of a PARTIAL call) and the running sum
of squares Q = sum c_i^2 (plane 1).  From (S, Q, n):

    mean            m  = S / n
    sample variance s2 = max(0, (Q - n m^2) / (n - 1))      (clamped: cancellation may round below zero)
    standard error  se = sqrt(s2 / n)                        (of the pixel's mean; +inf for n = 1)

and the frame's estimated RMS error against the converged image is sqrt(mean over pixels and channels of se^2).
Everything is computed in float64.  With RTG_FLAG_SAMPLE_COUNTS every pixel has its own n (standard_error_counts), and
adaptive sampling retires a pixel once its estimate is good enough (retire).
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


def retire(active, k, stderr, min_samples, target_se):
    """The retire rule of adaptive sampling (Scene.adaptive), after the slice that ends at k samples: the active pixels with
    k >= min_samples whose largest per-channel standard error is <= target_se.  Returns a bool mask of the pixel grid."""
    active = np.asarray(active, dtype=bool)
    if k < min_samples:
        return np.zeros_like(active)
    return active & (np.max(np.asarray(stderr, dtype=np.float64), axis=-1) <= target_se)
