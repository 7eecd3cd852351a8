"""The cases the image-texture tests share (test_image_texture_abi.py on the host, test_image_texture_gpu.py on the device): the
images, the settings and the points of the probe comparisons, and the pairs rt_atan2f is checked on.  Everything is
deterministic: the host test and the GPU test see the same arrays."""
import numpy as np

f32 = np.float32

SIZES = [(1, 1), (2, 3), (5, 4), (64, 64)]   # (w, h)
CENTRE = (0.5, -0.25, 1.0)


def image(size, seed=20261021):
    w, h = size
    return np.random.RandomState(seed + 131 * w + h).rand(h, w, 3).astype(f32)


def settings(I, size):
    """Both filters x the four wrap pairs x three mappings: planar with u = x, v = y; a skewed planar mapping with offsets; the
    spherical one about CENTRE."""
    out = []
    for flt in (I.NEAREST, I.BILINEAR):
        for wu in (I.REPEAT, I.CLAMP):
            for wv in (I.REPEAT, I.CLAMP):
                kw = dict(filter=flt, wrap_u=wu, wrap_v=wv)
                out.append(I.planar((1, 0, 0), 0.0, (0, 1, 0), 0.0, **kw))
                out.append(I.planar((0.3, 0.1, -0.2), 0.25, (0.05, -0.4, 0.7), -0.5, **kw))
                out.append(I.spherical(CENTRE, **kw))
    return out


def name(prm):
    return "mapping %d filter %d wrap %d%d" % (prm["mapping"], prm["filter"], prm["wrap_u"], prm["wrap_v"])


def centres(size):
    """p with (x, y) = the texel centres in (u, v), for the mapping u = x, v = y; row-major from the top row."""
    w, h = size
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u = (ii.reshape(-1).astype(f32) + f32(0.5)) / f32(w)
    v = f32(1.0) - (jj.reshape(-1).astype(f32) + f32(0.5)) / f32(h)
    return np.stack([u, v, np.zeros_like(u)], axis=1).astype(f32)


_SPECIAL = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e30, -1e30, 3e9, -3e9, 2147483648.0, -2147483648.0, 1e-40]


def points(I, prm, size):
    """Texel centres and texel edges (and the points half an ulp to either side of them), negative and large coordinates,
    1e30 (which saturates the cast), signed zeros, infinities, NaN, and random points.  For the spherical mapping the same
    set is also laid around CENTRE, with the poles, the seam (d.x < 0, d.z = +-0) and the centre itself."""
    w, h = size
    rs = np.random.RandomState(7 + 31 * w + h)
    c = centres(size)[: 16 * 16]
    edges_u = np.arange(-2 * w, 3 * w + 1, dtype=f32) / f32(w)
    edges_v = np.arange(-2 * h, 3 * h + 1, dtype=f32) / f32(h)
    eu, ev = edges_u[:40], edges_v[:40]
    grid = np.stack(np.meshgrid(np.concatenate([eu, np.nextafter(eu, f32(9)), np.nextafter(eu, f32(-9))]),
                                np.concatenate([ev[::3], np.nextafter(ev[::3], f32(9))])), axis=-1).reshape(-1, 2).astype(f32)
    grid = np.concatenate([grid, np.zeros((len(grid), 1), f32)], axis=1)
    sp = np.array(_SPECIAL, dtype=f32)
    special = np.stack(np.meshgrid(sp, sp, sp[:6]), axis=-1).reshape(-1, 3)
    rnd = ((rs.rand(256, 3) - 0.5) * 8).astype(f32)
    far = ((rs.rand(64, 3) - 0.5) * 1e6).astype(f32)
    p = np.concatenate([c, grid, special, rnd, far]).astype(f32)
    if prm["mapping"] == I.SPHERICAL:
        ctr = np.array(CENTRE, f32)
        d = rs.randn(256, 3).astype(f32)
        axes = np.array([[0, 1, 0], [0, -1, 0], [-1, 0, 0.0], [-1, 0, -0.0], [1, 0, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [-1, 1e-30, 1e-30],
                         [1e-30, 1, 0], [-2, 0.5, 1e-45], [-2, 0.5, -1e-45]], dtype=f32)
        p = np.concatenate([p, ctr + d, ctr + axes, ctr + f32(1e-3) * d[:32], ctr + f32(1e4) * d[:32]]).astype(f32)
    return p


def atan2_pairs(n=1 << 20, seed=20261021):
    """(y, x): n pairs of random float32 bit patterns (every exponent, both signs, subnormals, a few NaNs and infinities among
    them), then the full grid over signed zeros, infinities, NaN, the extremes, equal magnitudes and the axes."""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(f32)
    x = rs.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(f32)
    # random pairs of nearby exponents too: the quotient is then of order one, where the reduction switches branches
    k = n // 4
    with np.errstate(all="ignore"):
        y2 = (rs.rand(k).astype(f32) * f32(4) - f32(2)) * x[:k]
    tiny, big = np.finfo(f32).tiny, np.finfo(f32).max
    g = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 1e-45, -1e-45, tiny, -tiny, big, -big, 3.0, -3.0,
                  0.41421357, 0.41421354, 2.4142137, 2.4142134, 1e-20, -1e-20, 1e20, -1e20], dtype=f32)
    gy, gx = (a.reshape(-1) for a in np.meshgrid(g, g))
    return np.concatenate([y, y2, gy]).astype(f32), np.concatenate([x, x[:k], gx]).astype(f32)
