"""The feature rays of RTG_FLAG_FEATURES (include/rtiow_gpu.h) in numpy.  This is the normative definition of the rays: the
library sends exactly these, one hit_top each, and folds what they hit into the albedo, normal and depth planes.  Everything
is float32 and every operation is rounded on its own."""
import numpy as np

f32 = np.float32
MAX_GRID = 4


def subpixel_rays(camera, nx, ny, grid):
    """The g * g primary rays of every pixel, float32 [g * g, ny, nx, 7]: (origin, direction, time) of ray k = j * g + i of
    the pixel in row `row` (row 0 = top, y = ny - 1 - row) and column x.  The ray goes from the lens centre through the centre
    of cell (i, j) of a g x g grid over the pixel's area, at the middle of the exposure: Camera::get_ray (camera.rs:52-63)
    with a zero lens offset."""
    g = int(grid)
    if not 1 <= g <= MAX_GRID:
        raise ValueError("grid must be in 1 .. %d" % MAX_GRID)
    v3 = lambda a: np.array([a[0], a[1], a[2]], dtype=f32)
    origin, llc = v3(camera.origin), v3(camera.lower_left_corner)
    hor, ver = v3(camera.horizontal), v3(camera.vertical)
    e0, e1 = f32(camera.exposure_start), f32(camera.exposure_end)
    time = f32(e0 + f32(f32(0.5) * f32(e1 - e0)))
    x = np.arange(nx, dtype=np.uint32).astype(f32)[None, :]
    y = (ny - 1 - np.arange(ny, dtype=np.int64)).astype(f32)[:, None]
    rays = np.zeros((g * g, ny, nx, 7), dtype=f32)
    for j in range(g):
        for i in range(g):
            su = f32(f32(f32(i) + f32(0.5)) / f32(g))
            sv = f32(f32(f32(j) + f32(0.5)) / f32(g))
            u = ((x + su) / f32(nx)).astype(f32) * np.ones((ny, 1), f32)
            v = ((y + sv) / f32(ny)).astype(f32) * np.ones((1, nx), f32)
            d = ((llc + u[..., None] * hor).astype(f32) + v[..., None] * ver).astype(f32) - origin
            r = rays[j * g + i]
            r[..., 0:3] = origin
            r[..., 3:6] = d.astype(f32)
            r[..., 6] = time
    return rays


def fold(values, hit):
    """The planes' fold: `values` float32 [g * g, ...] per ray, `hit` bool [g * g, ...] (a miss counts as +0); the left fold
    over the rays from +0, divided by float32(g * g)."""
    values = np.asarray(values, dtype=f32)
    mask = np.asarray(hit, dtype=bool)
    while mask.ndim < values.ndim:
        mask = mask[..., None]
    acc = np.zeros(values.shape[1:], dtype=f32)
    with np.errstate(all="ignore"):
        for k in range(values.shape[0]):
            acc = (acc + np.where(mask[k], values[k], f32(0))).astype(f32)
        return (acc / f32(values.shape[0])).astype(f32)
