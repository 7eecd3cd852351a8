"""Ray generators for ray frames (include/rtiow_gpu_rays.h; Scene.cast_rays).  Numpy only.

`camera_rays` restates the library's own camera on the host: the counter RNG (Philox4x32-10 with the counter layout of
csrc/rt_device.h SampleRng::refill), its float draws, the lens disc's rejection loop, the exposure draw and get_ray's operand
order (csrc/rt_trace.h), every float32 operation rounded on its own.  A ray frame of these rays is the rtg_par_cast frame, bit
for bit.  The other generators return one ray per pixel through the pixel centres, for cameras the library does not have:
`equirect_rays`, `fisheye_rays`, `ortho_rays`.

Every generator returns float32 [n, 7]: origin, direction, time; pixel p = row * nx + x, row 0 = top.
"""
import math

import numpy as np

f32 = np.float32
u32 = np.uint32
u64 = np.uint64

_M0, _M1 = u64(0xD2511F53), u64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = u64(0xFFFFFFFF)
_S32 = u64(32)


def philox4x32(block, sample, pixel, event, seed):
    """The four words of block `block` of the stream (seed, pixel, sample, event): Philox4x32-10 over the counter
    (block, sample, pixel, event) with the key (seed's low word, seed's high word).  Arrays broadcast; returns uint32 [..., 4]."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(a, dtype=u64) & _MASK for a in (block, sample, pixel, event)))
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _MASK, p1 >> _S32, p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ u64(k0), lo1, hi0 ^ c3 ^ u64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(u32)


class _Stream:
    """One stream of the counter RNG per lane, event 0: the words in order, a lane at a time advancing only where asked."""

    def __init__(self, seed, pixel, sample):
        self.seed, self.pixel, self.sample = seed, np.asarray(pixel, dtype=u64), np.asarray(sample, dtype=u64)
        self.pos = np.zeros(self.pixel.shape, dtype=np.int64)
        self.block = np.full(self.pixel.shape, -1, dtype=np.int64)
        self.words = np.zeros(self.pixel.shape + (4,), dtype=u32)

    def next_u32(self, take):
        """The next word of every lane; the lanes of `take` consume it."""
        need = (self.pos >> 2) != self.block
        if need.any():
            self.words[need] = philox4x32((self.pos >> 2)[need], self.sample[need], self.pixel[need], 0, self.seed)
            self.block[need] = (self.pos >> 2)[need]
        w = np.take_along_axis(self.words, (self.pos & 3)[..., None], axis=-1)[..., 0]
        self.pos = self.pos + take.astype(np.int64)
        return w

    def gen_f32(self, take):
        """rand 0.6.5 Standard for f32: (u32 >> 8) * 2^-24"""
        return (self.next_u32(take) >> u32(8)).astype(f32) * f32(1.0 / 16777216.0)


def _vec(c_array):
    return np.array(list(c_array), dtype=f32)


def camera_rays(camera, nx, ny, ns, seed):
    """The library's own camera rays for `camera` (a capi.Camera), in per-sample layout: float32 [ns * nx * ny, 7], sample s of
    pixel p = row * nx + x at s * nx * ny + p.  par_cast's closure (lib.rs:366-371) and Camera::get_ray (camera.rs:52-63) on the
    stream (seed, y * nx + x, s), event 0, with y = ny - 1 - row."""
    s_i, row_i, x_i = np.meshgrid(np.arange(ns), np.arange(ny), np.arange(nx), indexing="ij")
    y_i = ny - 1 - row_i
    rng = _Stream(seed, (y_i * nx + x_i) & 0xFFFFFFFF, s_i)
    every = np.ones(s_i.shape, dtype=bool)
    u = (x_i.astype(f32) + rng.gen_f32(every)) / f32(nx)
    v = (y_i.astype(f32) + rng.gen_f32(every)) / f32(ny)
    # in_unit_disc (vec3.rs:32-39): 2 * (a, b, 0) - (1, 1, 0) until its squared length is < 1
    dx, dy = np.zeros(s_i.shape, dtype=f32), np.zeros(s_i.shape, dtype=f32)
    todo = every.copy()
    while todo.any():
        a, b = rng.gen_f32(todo), rng.gen_f32(todo)
        px, py = f32(2.0) * a - f32(1.0), f32(2.0) * b - f32(1.0)
        ok = todo & ((px * px + py * py) + f32(0.0) < f32(1.0))
        dx[ok], dy[ok] = px[ok], py[ok]
        todo &= ~ok
    lens = f32(camera.lens_radius)
    rdx, rdy = lens * dx, lens * dy
    cu, cv, origin = _vec(camera.u), _vec(camera.v), _vec(camera.origin)
    llc, hor, ver = _vec(camera.lower_left_corner), _vec(camera.horizontal), _vec(camera.vertical)
    offset = rdx[..., None] * cu + rdy[..., None] * cv
    # gen_range (rand 0.6.5 UniformFloat::sample_single, camera.rs:55)
    low, high = f32(camera.exposure_start), f32(camera.exposure_end)
    scale = f32(high - low)
    time = np.zeros(s_i.shape, dtype=f32)
    todo = every.copy()
    while todo.any():
        w = rng.next_u32(todo)
        v12 = ((w >> u32(9)) | u32(0x3F800000)).view(f32)
        res = (v12 - f32(1.0)) * scale + low
        ok = todo & (res < high)
        time[ok] = res[ok]
        todo &= ~ok
    out = np.empty(s_i.shape + (7,), dtype=f32)
    out[..., 0:3] = origin + offset
    out[..., 3:6] = (((llc + u[..., None] * hor) + v[..., None] * ver) - origin) - offset
    out[..., 6] = time
    return out.reshape(-1, 7)


def _unit(a):
    a = np.asarray(a, dtype=np.float64)
    return a / math.sqrt(float(a @ a))


def _pixel_centres(nx, ny):
    """(sx, sy) of every pixel centre in [-1, 1], +sy up; pixel p = row * nx + x, row 0 = top."""
    row, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    return (2.0 * (x + 0.5) / nx - 1.0).reshape(-1), (1.0 - 2.0 * (row + 0.5) / ny).reshape(-1)


def _pack(origin, direction, time):
    n = direction.shape[0]
    out = np.empty((n, 7), dtype=f32)
    out[:, 0:3] = np.broadcast_to(origin, (n, 3))
    out[:, 3:6] = direction
    out[:, 6] = time
    return out


def equirect_rays(origin, nx, ny, time=0.0):
    """A full sphere of directions around `origin`: longitude over x (-pi at the left edge, 0 = -z, growing towards +x), latitude
    over rows (+pi / 2 = +y at the top)."""
    sx, sy = _pixel_centres(nx, ny)
    lon, lat = math.pi * sx, 0.5 * math.pi * sy
    d = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), -np.cos(lat) * np.cos(lon)], axis=-1)
    return _pack(np.asarray(origin, dtype=np.float64), d, time)


def fisheye_rays(origin, forward, up, fov_degrees, nx, ny, time=0.0):
    """An equidistant fisheye around `forward`: the angle from the axis grows linearly with the distance from the image centre,
    fov_degrees / 2 at the edge of the inscribed circle (pixels outside it continue the same rule)."""
    w = _unit(forward)
    right = _unit(np.cross(w, np.asarray(up, dtype=np.float64)))
    upv = np.cross(right, w)
    sx, sy = _pixel_centres(nx, ny)
    r = np.hypot(sx, sy)
    theta = r * math.radians(fov_degrees) / 2.0
    k = np.where(r > 0.0, np.sin(theta) / np.where(r > 0.0, r, 1.0), 0.0)
    d = (k * sx)[:, None] * right + (k * sy)[:, None] * upv + np.cos(theta)[:, None] * w
    return _pack(np.asarray(origin, dtype=np.float64), d, time)


def ortho_rays(look_from, look_at, up, width, height, nx, ny, time=0.0):
    """Parallel rays along look_from -> look_at from a width x height window centred on look_from."""
    o = np.asarray(look_from, dtype=np.float64)
    w = _unit(np.asarray(look_at, dtype=np.float64) - o)
    right = _unit(np.cross(w, np.asarray(up, dtype=np.float64)))
    upv = np.cross(right, w)
    sx, sy = _pixel_centres(nx, ny)
    origin = o + (0.5 * width * sx)[:, None] * right + (0.5 * height * sy)[:, None] * upv
    return _pack(origin, np.broadcast_to(w, (nx * ny, 3)), time)
