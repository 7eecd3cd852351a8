"""The background of RTG_FLAG_BACKGROUND (include/rtiow_gpu.h) in numpy.  This is the normative definition of B(d): float32, every
operation rounded on its own, in the order the header states -- the kernels (csrc/rt_device.h background_colour) match it bit for
bit.

    sky(d, bottom, top, mode)       B(d) for directions d [..., 3]
    miss_colour(d, bottom, top, mode, accum, strength)   accum + strength * B(d): the colour of a path whose ray d missed
    BOOK_SKY                        the book's gradient: white at the bottom, (0.5, 0.7, 1.0) at the top
"""
import numpy as np

MODE_CONSTANT, MODE_GRADIENT = 0, 1
BOOK_SKY = {"bottom": (1.0, 1.0, 1.0), "top": (0.5, 0.7, 1.0)}

_f = np.float32


def sky(d, bottom, top=None, mode=MODE_CONSTANT):
    """B(d), float32 [..., 3], for ray directions d [..., 3] (not normalised).  mode 0: `bottom`, whatever d is.  mode 1:
    len = sqrt((dx * dx + dy * dy) + dz * dz); uy = dy / len; t = 0.5 * (uy + 1); B_c = (1 - t) * bottom_c + t * top_c."""
    d = np.asarray(d, dtype=_f)
    bottom = np.asarray(bottom, dtype=_f)
    if mode == MODE_CONSTANT:
        return np.broadcast_to(bottom, d.shape).copy()
    if mode != MODE_GRADIENT:
        raise ValueError("mode must be 0 (constant) or 1 (gradient)")
    top = np.asarray(top, dtype=_f)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):   # (NaN and infinity propagate, as in the kernels)
        length = np.sqrt((dx * dx + dy * dy) + dz * dz, dtype=_f)
        uy = dy / length
        t = (_f(0.5) * (uy + _f(1.0)))[..., None]
        return ((_f(1.0) - t) * bottom + t * top).astype(_f)


def miss_colour(d, bottom, top=None, mode=MODE_CONSTANT, accum=None, strength=None):
    """accum + strength * B(d), float32: what a path books when its ray d leaves the scene (lib.rs:76 for a light of emission
    B, then scatter() == None).  accum defaults to (0, 0, 0) and strength to (1, 1, 1): the camera ray."""
    b = sky(d, bottom, top, mode)
    accum = np.zeros(3, dtype=_f) if accum is None else np.asarray(accum, dtype=_f)
    strength = np.ones(3, dtype=_f) if strength is None else np.asarray(strength, dtype=_f)
    with np.errstate(all="ignore"):
        return (accum + strength * b).astype(_f)
