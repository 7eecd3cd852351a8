"""Environment maps (include/rtiow_gpu_environment.h; Builder.environment): the definition in numpy, a Radiance .hdr reader and
writer, and a small procedural sky.  Numpy only.

`direction` and `colour` ARE the specification of the environment: the library (csrc/rt_environment.h, csrc/rt_trace.h
environment_colour) equals them bit for bit, on the host and on the device.  Every float32 operation is rounded on its own and
written in the header's operand order; numpy never contracts a multiply and an add.

A lat-long map is an image texture with image.spherical() about (0, 0, 0): float32 [h, w, 3], row 0 = world +y, u as image.py
says.  `load_hdr` brings a Radiance RGBE picture in as such an array; `sun_sky` makes one without a file.
"""
import numpy as np

from . import image

f32 = np.float32


def rotate_y_pair(degrees):
    """(s, c) as rtg_object_rotate_y and rtg_builder_set_environment derive them: radians = degrees * PI / 180 in float32, then
    sinf / cosf.  The library's pair comes from the platform's libm (rtg_builder_get_environment reports it); this is numpy's,
    for callers that need no bit-exact pair."""
    r = f32(degrees) * f32(3.14159265358979323846) / f32(180.0)
    return np.sin(r, dtype=f32), np.cos(r, dtype=f32)


def direction(d, s, c):
    """q [n, 3] for the directions d [n, 3] of rays that left the scene: u = d / |d|, then RotateY's rot() (object.rs:349-355)
    with the pair (s, c).  THE definition."""
    d = np.asarray(d, dtype=f32).reshape(-1, 3)
    s, c = f32(s), f32(c)
    zero, one = f32(0.0), f32(1.0)
    with np.errstate(all="ignore"):
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        ln = np.sqrt((dx * dx + dy * dy) + dz * dz)
        ux, uy, uz = dx / ln, dy / ln, dz / ln
        qx = (ux * c + uy * zero) + uz * s
        qy = (ux * zero + uy * one) + uz * zero
        qz = (ux * (-s) + uy * zero) + uz * c
    return np.stack([qx, qy, qz], axis=-1).astype(f32)


def colour(d, texels, image_params, scale, s, c):
    """E(d) [n, 3] for the directions d [n, 3]: scale * T(q), q = direction(d, s, c).  `texels` with `image_params` (image.params
    / image.spherical) is an image texture, sampled by image.sample; `texels` of three floats with image_params=None is a
    constant texture.  THE definition."""
    q = direction(d, s, c)
    scale = np.asarray(scale, dtype=f32).reshape(3)
    if image_params is None:
        t = np.broadcast_to(np.asarray(texels, dtype=f32).reshape(3), q.shape)
    else:
        t = image.sample(texels, image_params, q)
    with np.errstate(all="ignore"):
        return (scale[None, :] * t).astype(f32)


def lat_long_params(filter=image.BILINEAR):
    """The image parameters of a lat-long map: spherical about the origin, u repeats (the seam), v clamps (the poles)."""
    return image.spherical((0.0, 0.0, 0.0), filter=filter, wrap_u=image.REPEAT, wrap_v=image.CLAMP)


def texel_directions(w, h):
    """Unit directions [h, w, 3] (float64) through the texel centres of a w x h lat-long map under image.spherical():
    u = 0.5 - atan2(z, x) / (2 pi), v = 0.5 + atan2(y, rho) / pi, texel (i, j) = (u * w, (1 - v) * h)."""
    u = (np.arange(w) + 0.5) / w
    v = 1.0 - (np.arange(h) + 0.5) / h
    phi = (0.5 - u) * 2.0 * np.pi
    theta = (v - 0.5) * np.pi
    ct, st = np.cos(theta)[:, None], np.sin(theta)[:, None]
    return np.stack([ct * np.cos(phi)[None, :], np.broadcast_to(st, (h, w)), ct * np.sin(phi)[None, :]], axis=-1)


def sun_sky(w, h, sun_direction=(0.4, 0.6, -0.7), sun_radiance=(60.0, 54.0, 42.0), sun_degrees=3.0, zenith=(0.25, 0.45, 0.9),
            horizon=(0.85, 0.9, 1.0), ground=(0.3, 0.27, 0.24)):
    """A small procedural lat-long sky, float32 [h, w, 3]: a zenith-to-horizon blend above y = 0, a constant ground below, and
    a sun disc of `sun_degrees` across with a soft edge.  What the examples and tools/environment_cost.py render under, so that
    nothing has to be downloaded."""
    d = texel_directions(w, h)
    y = d[..., 1]
    t = np.sqrt(np.clip(y, 0.0, 1.0))[..., None]
    sky = (1.0 - t) * np.asarray(horizon, dtype=np.float64) + t * np.asarray(zenith, dtype=np.float64)
    out = np.where((y >= 0.0)[..., None], sky, np.asarray(ground, dtype=np.float64))
    sd = np.asarray(sun_direction, dtype=np.float64)
    sd = sd / np.linalg.norm(sd)
    ang = np.degrees(np.arccos(np.clip(d @ sd, -1.0, 1.0)))
    r = 0.5 * sun_degrees
    disc = np.clip((1.25 * r - ang) / (0.25 * r), 0.0, 1.0)[..., None]  # 1 inside the disc, fading out over a quarter radius
    return (out + disc * np.asarray(sun_radiance, dtype=np.float64)).astype(f32)


# ---- Radiance RGBE (.hdr) ------------------------------------------------------------------------------------------------
# A pixel is four bytes (r, g, b, e): channel value = mantissa * 2^(e - 136), all three +0 when e = 0 (the convention of the
# common decoders; Ward's own adds half a mantissa step).  The file: text lines up to an empty line, a resolution line
# "-Y h +X w" (top row first, the image layout of this package), then the scanlines, each either flat (w pixels of four bytes)
# or new-style run-length: bytes 2, 2, w >> 8, w & 255, then the four channels one after the other, each a sequence of
# (count > 128: count - 128 copies of the next byte | count <= 128: count literal bytes).

def rgbe_encode(rgb):
    """float [.., 3] -> uint8 [.., 4]: the shared exponent of the largest channel, mantissas truncated; negative, NaN and values
    below 2^-136 become 0, values above the format's range its largest."""
    rgb = np.asarray(rgb, dtype=np.float64)
    with np.errstate(all="ignore"):
        x = np.where(np.isfinite(rgb) & (rgb > 0.0), rgb, np.where(rgb == np.inf, np.inf, 0.0))
        vmax = x.max(axis=-1)
        _, e = np.frexp(np.where(np.isfinite(vmax), vmax, 1.0))
        e = np.where(np.isfinite(vmax), e, 128)
        e = np.clip(e, -127, 127)
        mant = np.floor(np.ldexp(np.where(np.isfinite(x), x, 0.0), (8 - e)[..., None]))
        mant = np.where(np.isfinite(x), mant, 255.0)
    mant = np.clip(mant, 0.0, 255.0)
    out = np.concatenate([mant, (e + 128)[..., None].astype(np.float64)], axis=-1).astype(np.uint8)
    out[mant.max(axis=-1) == 0.0] = 0
    return out


def rgbe_decode(rgbe):
    """uint8 [.., 4] -> float32 [.., 3]: mantissa * 2^(e - 136), exactly; e = 0 is black."""
    rgbe = np.asarray(rgbe, dtype=np.uint8)
    e = rgbe[..., 3].astype(np.int32)
    out = np.ldexp(rgbe[..., :3].astype(np.float64), (e - 136)[..., None])
    return np.where((e == 0)[..., None], 0.0, out).astype(f32)


def _rle_channel(row):
    """One channel of one scanline (uint8 [w]) as new-style run-length bytes: runs of >= 4 equal bytes, literals otherwise."""
    out = bytearray()
    w, i = len(row), 0
    change = np.flatnonzero(np.diff(row)) + 1           # starts of runs of equal bytes
    starts = np.concatenate([[0], change]).tolist()
    ends = np.concatenate([change, [w]]).tolist()
    lit = bytearray()

    def flush():
        for k in range(0, len(lit), 128):
            chunk = lit[k:k + 128]
            out.append(len(chunk))
            out.extend(chunk)
        lit.clear()

    for a, b in zip(starts, ends):
        n, val = b - a, int(row[a])
        if n >= 4:
            flush()
            while n > 0:
                k = min(n, 127)
                out.append(128 + k)
                out.append(val)
                n -= k
        else:
            lit.extend([val] * n)
    flush()
    return bytes(out)


def save_hdr(path, rgb, rle=True):
    """Write float [h, w, 3] (row 0 at the top) as a Radiance RGBE file.  rle=True writes new-style run-length scanlines where
    the format allows them (8 <= w < 32768), flat ones otherwise."""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("an image is [h, w, 3]")
    h, w = rgb.shape[:2]
    px = rgbe_encode(rgb)
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w))
        if not rle or w < 8 or w >= 32768:
            f.write(px.tobytes())
            return
        for j in range(h):
            f.write(bytes([2, 2, w >> 8, w & 255]))
            for ch in range(4):
                f.write(_rle_channel(px[j, :, ch]))


def load_hdr(path):
    """Read a Radiance RGBE file with flat or new-style run-length scanlines (or both): float32 [h, w, 3], row 0 at the top, as
    Builder.image takes it."""
    with open(path, "rb") as f:
        data = f.read()
    if not (data.startswith(b"#?RADIANCE") or data.startswith(b"#?RGBE")):
        raise ValueError("%s: not a Radiance picture (no #?RADIANCE line)" % path)
    pos, fmt = 0, None
    while True:
        end = data.find(b"\n", pos)
        if end < 0:
            raise ValueError("%s: the header does not end" % path)
        line, pos = data[pos:end].strip(), end + 1
        if not line:
            break
        if line.startswith(b"FORMAT="):
            fmt = line[7:]
    if fmt is not None and fmt != b"32-bit_rle_rgbe":
        raise ValueError("%s: FORMAT=%s is not supported" % (path, fmt.decode("ascii", "replace")))
    end = data.find(b"\n", pos)
    res = data[pos:end].split()
    pos = end + 1
    if len(res) != 4 or res[0] != b"-Y" or res[2] != b"+X":
        raise ValueError("%s: only the standard orientation '-Y h +X w' is supported" % path)
    h, w = int(res[1]), int(res[3])
    if h < 1 or w < 1:
        raise ValueError("%s: empty picture" % path)
    buf = np.frombuffer(data, dtype=np.uint8)
    px = np.empty((h, w, 4), dtype=np.uint8)
    for j in range(h):
        rle = 8 <= w < 32768 and pos + 4 <= len(buf) and buf[pos] == 2 and buf[pos + 1] == 2 and ((int(buf[pos + 2]) << 8) | int(buf[pos + 3])) == w
        if not rle:
            if pos + 4 * w > len(buf):
                raise ValueError("%s: the file ends inside scanline %d" % (path, j))
            px[j] = buf[pos:pos + 4 * w].reshape(w, 4)
            pos += 4 * w
            continue
        pos += 4
        for ch in range(4):
            i = 0
            while i < w:
                if pos >= len(buf):
                    raise ValueError("%s: the file ends inside scanline %d" % (path, j))
                n = int(buf[pos])
                pos += 1
                if n > 128:
                    n -= 128
                    if n == 0 or i + n > w or pos >= len(buf):
                        raise ValueError("%s: bad run in scanline %d" % (path, j))
                    px[j, i:i + n, ch] = buf[pos]
                    pos += 1
                else:
                    if n == 0 or i + n > w or pos + n > len(buf):
                        raise ValueError("%s: bad run in scanline %d" % (path, j))
                    px[j, i:i + n, ch] = buf[pos:pos + n]
                    pos += n
                i += n
    return rgbe_decode(px)
