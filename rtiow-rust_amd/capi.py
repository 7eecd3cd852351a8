"""ctypes binding of the C ABI declared in include/rtiow_gpu.h (librtiow_gpu.so, prefix ``rtg_``).

Method names mirror the reference crate's constructors (object.rs / material.rs / texture.rs /
camera.rs / lib.rs) so scene code reads like the reference's `src/main.rs`.  The symbol prefix is a
parameter so that a test harness can drive another library exporting the same entry points with the
same calls.
"""
import ctypes as C
import os
import time

import numpy as np

from . import noise

c_f32p = C.POINTER(C.c_float)
c_u32p = C.POINTER(C.c_uint32)
c_u8p = C.POINTER(C.c_uint8)

INVALID_ID = 0xFFFFFFFF
FLAG_COUNTERS = 1
FLAG_TRACE_KERNEL = 2
FLAG_PARTIAL = 4   # leave the unnormalised running sum of the samples in the framebuffer
FLAG_RESUME = 8    # the framebuffer holds the running sum of samples [0, sample_begin): render [sample_begin, ns)
FLAG_SUM_SQUARES = 16   # the framebuffer has a second plane: the running sum of the squared sample colours
FLAG_SAMPLE_COUNTS = 32  # the framebuffer ends with a count plane: every pixel's own sample count (uint32)
FLAG_RETIRE = 64         # after the slice, retire converged pixels in the count plane; the framebuffer ends with a Retire block
RETIRE_MAX_RADIUS = 8
FLAG_DENOISE = 128       # after the slice, filter the frame: the framebuffer ends with a Denoise block and the output plane
DENOISE_MAX_RADIUS = 8
DENOISE_MAX_PATCH = 3
FLAG_FEATURES = 256      # the framebuffer ends with a Features block and the first-hit albedo / normal / depth planes
FEATURES_MAX_GRID = 4


class Camera(C.Structure):
    """camera.rs:6-15"""
    _fields_ = [("origin", C.c_float * 3), ("lower_left_corner", C.c_float * 3),
                ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3),
                ("u", C.c_float * 3), ("v", C.c_float * 3),
                ("lens_radius", C.c_float), ("exposure_start", C.c_float), ("exposure_end", C.c_float)]


class Params(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("nx", C.c_uint32), ("ny", C.c_uint32), ("ns", C.c_uint32),
                ("max_bounces", C.c_uint32), ("t_near", C.c_float), ("seed", C.c_uint64),
                ("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("rank", C.c_uint32),
                ("nranks", C.c_uint32), ("flags", C.c_uint32), ("sample_begin", C.c_uint32)]


class Retire(C.Structure):
    """include/rtiow_gpu.h rtg_retire: the block behind the count plane of an RTG_FLAG_RETIRE frame (64 bytes).  The caller
    sets target_se / min_samples / radius; every accepted call writes the out-fields active .. samples_held."""
    _fields_ = [("target_se", C.c_double), ("min_samples", C.c_uint32), ("radius", C.c_uint32),
                ("active", C.c_uint32), ("retired", C.c_uint32), ("estimated", C.c_uint32), ("reserved", C.c_uint32),
                ("sum_se2", C.c_double), ("samples_held", C.c_uint64), ("reserved2", C.c_uint64 * 2)]
    OUT_FIELDS = ("active", "retired", "estimated", "reserved", "sum_se2", "samples_held")

    def as_dict(self):
        """The out-fields, plus est_rmse = sqrt(sum_se2 / (3 estimated)) (inf when no pixel has an estimate)."""
        d = {k: getattr(self, k) for k in self.OUT_FIELDS}
        d["est_rmse"] = float(np.sqrt(self.sum_se2 / (3 * self.estimated))) if self.estimated else float("inf")
        return d


def retire_block_offset(nx, ny):
    """Byte offset of the Retire block in an RTG_FLAG_RETIRE frame: word 7 * nx * ny (two float planes and the count plane),
    rounded up to an even word."""
    return ((7 * nx * ny + 1) & ~1) * 4


def retire_frame_bytes(nx, ny):
    """Bytes of an RTG_FLAG_RETIRE frame: two float planes, the count plane, padding to 8 bytes, the 64-byte Retire block."""
    return retire_block_offset(nx, ny) + C.sizeof(Retire)


class Denoise(C.Structure):
    """include/rtiow_gpu.h rtg_denoise: the block in front of the output plane of an RTG_FLAG_DENOISE frame (64 bytes).  The
    caller sets k / radius / patch; every accepted call writes the out-fields filtered / passed."""
    _fields_ = [("k", C.c_float), ("radius", C.c_uint32), ("patch", C.c_uint32), ("reserved_in", C.c_uint32),
                ("filtered", C.c_uint32), ("passed", C.c_uint32), ("reserved", C.c_uint32 * 10)]
    OUT_FIELDS = ("filtered", "passed")
    OUT_OFFSET = 16   # bytes: the in-fields end here

    def as_dict(self):
        """The out-fields."""
        return {k: getattr(self, k) for k in self.OUT_FIELDS}


def make_denoise(denoise=None, k=0.7, radius=5, patch=2):
    """A Denoise with the in-fields set: from a Denoise (copied), a dict of k / radius / patch, or True / None (the defaults
    0.7, 5, 2)."""
    d = Denoise()
    if isinstance(denoise, Denoise):
        C.memmove(C.addressof(d), C.addressof(denoise), C.sizeof(Denoise))
        return d
    if isinstance(denoise, dict):
        unknown = set(denoise) - {"k", "radius", "patch"}
        if unknown:
            raise ValueError("denoise=: unknown key(s) %s (k, radius, patch)" % sorted(unknown))
        k, radius, patch = denoise.get("k", k), denoise.get("radius", radius), denoise.get("patch", patch)
    d.k, d.radius, d.patch = float(k), int(radius), int(patch)
    return d


def denoise_block_offset(nx, ny, counts=False, retire=False):
    """Byte offset of the Denoise block in an RTG_FLAG_DENOISE frame: the first even word behind the two float planes, the
    count plane (counts=True) or the Retire block (retire=True, which implies the count plane)."""
    if retire:
        return retire_block_offset(nx, ny) + C.sizeof(Retire)
    return (((7 if counts else 6) * nx * ny + 1) & ~1) * 4


def denoise_frame_bytes(nx, ny, counts=False, retire=False):
    """Bytes of an RTG_FLAG_DENOISE frame: everything the other flags put in it, the 64-byte Denoise block, the output plane."""
    return denoise_block_offset(nx, ny, counts, retire) + C.sizeof(Denoise) + nx * ny * 3 * 4


class Features(C.Structure):
    """include/rtiow_gpu.h rtg_features: the block in front of the albedo / normal / depth planes of an RTG_FLAG_FEATURES frame
    (64 bytes).  The caller sets grid / compute and, for the guided filter (RTG_FLAG_DENOISE in the same call), the three
    sigmas; every accepted call writes the out-fields traced / missed."""
    _fields_ = [("grid", C.c_uint32), ("compute", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_depth", C.c_float), ("reserved_in", C.c_uint32), ("traced", C.c_uint32), ("missed", C.c_uint32),
                ("reserved", C.c_uint32 * 8)]
    OUT_FIELDS = ("traced", "missed")
    OUT_OFFSET = 24   # bytes: the in-fields end here

    def as_dict(self):
        """The out-fields."""
        return {k: getattr(self, k) for k in self.OUT_FIELDS}


FEATURES_DEFAULTS = {"grid": 2, "compute": 1, "sigma_normal": 1.0, "sigma_albedo": 1.0, "sigma_depth": 1.0}


def make_features(features=None, **fields):
    """A Features with the in-fields set: from a Features (copied), a dict of grid / compute / sigma_normal / sigma_albedo /
    sigma_depth, or True / None (FEATURES_DEFAULTS: a 2 x 2 grid, traced in the call; the sigmas DESIGN.md section 6 chose)."""
    f = Features()
    if isinstance(features, Features):
        C.memmove(C.addressof(f), C.addressof(features), C.sizeof(Features))
        return f
    v = dict(FEATURES_DEFAULTS)
    for src in (features if isinstance(features, dict) else {}, fields):
        unknown = set(src) - set(v)
        if unknown:
            raise ValueError("features=: unknown key(s) %s (%s)" % (sorted(unknown), ", ".join(FEATURES_DEFAULTS)))
        v.update(src)
    f.grid, f.compute = int(v["grid"]), int(v["compute"])
    f.sigma_normal, f.sigma_albedo, f.sigma_depth = float(v["sigma_normal"]), float(v["sigma_albedo"]), float(v["sigma_depth"])
    return f


def features_block_offset(nx, ny, squares=False, counts=False, retire=False, denoise=False):
    """Byte offset of the Features block in an RTG_FLAG_FEATURES frame: the first even word behind everything the call's other
    flags put in the frame -- the float planes (one, or two with squares), the count plane, the Retire block (implies counts
    and squares) or the Denoise block and its output plane (implies squares)."""
    n = nx * ny
    if denoise:
        end = denoise_block_offset(nx, ny, counts or retire, retire) // 4 + 16 + 3 * n
    elif retire:
        end = retire_block_offset(nx, ny) // 4 + 16
    else:
        end = ((6 if squares else 3) + (1 if counts else 0)) * n
    return ((end + 1) & ~1) * 4


def features_frame_bytes(nx, ny, squares=False, counts=False, retire=False, denoise=False):
    """Bytes of an RTG_FLAG_FEATURES frame: everything the other flags put in it, the 64-byte Features block, the albedo,
    normal and depth planes (7 floats per pixel)."""
    return features_block_offset(nx, ny, squares, counts, retire, denoise) + C.sizeof(Features) + nx * ny * 7 * 4


class Stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kernel_ms", C.c_float), ("samples", C.c_uint64),
                ("aabb_tests", C.c_uint64), ("prim_tests", C.c_uint64), ("shaded_hits", C.c_uint64),
                ("rays", C.c_uint64), ("draws", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


def make_params(nx, ny, ns, seed=0xDEADBEEF, max_bounces=50, t_near=0.001, tile_w=0, tile_h=0, rank=0,
                nranks=1, flags=0, sample_begin=0, partial=False, resume=False, squares=False, counts=False, retire=False,
                denoise=False, features=False):
    """`features`: RTG_FLAG_FEATURES, the features block and the albedo / normal / depth planes at the framebuffer's end.
    `partial` / `resume` / `sample_begin`: one slice of a progressive frame (include/rtiow_gpu.h RTG_FLAG_PARTIAL /
    RTG_FLAG_RESUME); `squares`: RTG_FLAG_SUM_SQUARES, the framebuffer's second plane; `counts`: RTG_FLAG_SAMPLE_COUNTS,
    the count plane at the framebuffer's end; `retire`: RTG_FLAG_RETIRE, the retire block behind it; `denoise`:
    RTG_FLAG_DENOISE, the denoise block and the output plane at the framebuffer's end."""
    flags |= (FLAG_DENOISE if denoise else 0) | (FLAG_FEATURES if features else 0)
    flags |= (FLAG_PARTIAL if partial else 0) | (FLAG_RESUME if resume else 0) | (FLAG_SUM_SQUARES if squares else 0)
    flags |= (FLAG_SAMPLE_COUNTS if counts else 0) | (FLAG_RETIRE if retire else 0)
    p = Params()
    p.struct_size = C.sizeof(Params)
    p.nx, p.ny, p.ns = nx, ny, ns
    p.max_bounces = max_bounces
    p.t_near = t_near
    p.seed = seed
    p.tile_w, p.tile_h, p.rank, p.nranks, p.flags = tile_w, tile_h, rank, nranks, flags
    p.sample_begin = sample_begin
    return p


def _device_ptr(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else int(x)


_hip = None


def _hip_runtime():
    """The HIP runtime librtiow_gpu.so itself links (device-to-device copies of Scene.progressive)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        _hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        _hip.hipMemsetD32Async.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    return _hip


def _resumes(kw):
    return bool(kw.get("resume")) and kw.get("sample_begin", 0) > 0


def _squares_supported(be):
    """RTG_FLAG_SUM_SQUARES is the HIP library's (prefix rtg_): a library that exports the same entry points under another
    prefix ignores flags it does not know and would write one plane where the caller expects two."""
    if be.prefix != "rtg_":
        raise ValueError("squares=True: %s (prefix %s) does not implement RTG_FLAG_SUM_SQUARES" % (be.path, be.prefix))


def _retire_supported(be):
    """RTG_FLAG_RETIRE is the HIP library's (prefix rtg_), like the flags it builds on."""
    if be.prefix != "rtg_":
        raise ValueError("retire=: %s (prefix %s) does not implement RTG_FLAG_RETIRE" % (be.path, be.prefix))


def _denoise_supported(be):
    """RTG_FLAG_DENOISE is the HIP library's (prefix rtg_), like the flags it builds on."""
    if be.prefix != "rtg_":
        raise ValueError("denoise=: %s (prefix %s) does not implement RTG_FLAG_DENOISE" % (be.path, be.prefix))


def _features_supported(be):
    """RTG_FLAG_FEATURES is the HIP library's (prefix rtg_): another library would ignore the flag and write no plane."""
    if be.prefix != "rtg_":
        raise ValueError("features=: %s (prefix %s) does not implement RTG_FLAG_FEATURES" % (be.path, be.prefix))


def _counts_supported(be):
    """RTG_FLAG_SAMPLE_COUNTS is the HIP library's (prefix rtg_), like RTG_FLAG_SUM_SQUARES: another library would ignore the
    count plane and render every pixel to ns."""
    if be.prefix != "rtg_":
        raise ValueError("counts=: %s (prefix %s) does not implement RTG_FLAG_SAMPLE_COUNTS" % (be.path, be.prefix))


class CountsFrame:
    """One contiguous host framebuffer for RTG_FLAG_SAMPLE_COUNTS: the float planes ([ny, nx, 3], or [2, ny, nx, 3] with
    squares) followed by the count plane (uint32 [ny, nx]), as include/rtiow_gpu.h lays them out.  `planes` and `counts` are
    views of `buf`; passing them as par_cast(out=frame.planes, counts=frame.counts) renders in place, without copies.
    retire=True (needs squares): `buf` also holds the RTG_FLAG_RETIRE block, and `retire` is a Retire view of it
    (par_cast(..., retire=frame.retire) renders in place too)."""

    def __init__(self, nx, ny, squares=False, retire=False):
        if retire and not squares:
            raise ValueError("a retire frame has two float planes: squares=True")
        n_f = (2 if squares else 1) * ny * nx * 3
        self.buf = np.zeros(retire_frame_bytes(nx, ny) // 4 if retire else n_f + ny * nx, dtype=np.float32)
        self.planes = self.buf[:n_f].reshape((2, ny, nx, 3) if squares else (ny, nx, 3))
        self.counts = self.buf[n_f:n_f + ny * nx].view(np.uint32).reshape(ny, nx)
        self.retire = Retire.from_buffer(self.buf, retire_block_offset(nx, ny)) if retire else None


class DenoiseFrame:
    """A sibling of CountsFrame (always two float planes; the count plane is optional).  One contiguous host framebuffer for RTG_FLAG_DENOISE, as include/rtiow_gpu.h lays it out: the two float planes
    (`planes`, [2, ny, nx, 3]), with counts=True the count plane (`counts`, uint32 [ny, nx], else None), with retire=True
    (implies counts) the Retire block (`retire`, else None), then the Denoise block (`denoise`) and the output plane
    (`denoised`, float32 [ny, nx, 3]).  All are views of `buf`; par_cast(out=frame, denoise=...) renders in place."""

    def __init__(self, nx, ny, counts=False, retire=False, denoise=None):
        counts = bool(counts or retire)
        n = nx * ny
        off = denoise_block_offset(nx, ny, counts, retire)
        self.nx, self.ny = nx, ny
        self.buf = np.zeros(denoise_frame_bytes(nx, ny, counts, retire) // 4, dtype=np.float32)
        self.planes = self.buf[:6 * n].reshape(2, ny, nx, 3)
        self.counts = self.buf[6 * n:7 * n].view(np.uint32).reshape(ny, nx) if counts else None
        self.retire = Retire.from_buffer(self.buf, retire_block_offset(nx, ny)) if retire else None
        self.denoise = Denoise.from_buffer(self.buf, off)
        self.denoised = self.buf[off // 4 + 16:off // 4 + 16 + 3 * n].reshape(ny, nx, 3)
        block = make_denoise(denoise)
        C.memmove(C.addressof(self.denoise), C.addressof(block), Denoise.OUT_OFFSET)


class FeaturesFrame:
    """One contiguous host framebuffer for RTG_FLAG_FEATURES, as include/rtiow_gpu.h lays it out, with the views of its
    siblings: `planes` ([ny, nx, 3], or [2, ny, nx, 3] with squares), `counts` (uint32 [ny, nx]) with counts=True, `retire`
    with retire=True (implies counts and squares), `denoise` / `denoised` with denoise= (a Denoise, a dict or True; implies
    squares) -- each None when the frame has no such part -- then `features` (the Features block) and the planes `albedo`,
    `normal` (float32 [ny, nx, 3]) and `depth` (float32 [ny, nx]).  All are views of `buf`;
    par_cast(out=frame, features=True) renders in place."""

    def __init__(self, nx, ny, squares=False, counts=False, retire=False, denoise=None, features=None):
        has_dn = denoise is not None and denoise is not False
        counts, squares = bool(counts or retire), bool(squares or retire or has_dn)
        n = nx * ny
        self.nx, self.ny, self.squares = nx, ny, squares
        off = features_block_offset(nx, ny, squares, counts, retire, has_dn)
        self.buf = np.zeros(features_frame_bytes(nx, ny, squares, counts, retire, has_dn) // 4, dtype=np.float32)
        n_f = (6 if squares else 3) * n
        self.planes = self.buf[:n_f].reshape((2, ny, nx, 3) if squares else (ny, nx, 3))
        self.counts = self.buf[n_f:n_f + n].view(np.uint32).reshape(ny, nx) if counts else None
        self.retire = Retire.from_buffer(self.buf, retire_block_offset(nx, ny)) if retire else None
        self.denoise = self.denoised = None
        if has_dn:
            d_off = denoise_block_offset(nx, ny, counts, retire)
            self.denoise = Denoise.from_buffer(self.buf, d_off)
            self.denoised = self.buf[d_off // 4 + 16:d_off // 4 + 16 + 3 * n].reshape(ny, nx, 3)
            block = make_denoise(None if denoise is True else denoise)
            C.memmove(C.addressof(self.denoise), C.addressof(block), Denoise.OUT_OFFSET)
        self.features = Features.from_buffer(self.buf, off)
        w = off // 4 + 16
        self.albedo = self.buf[w:w + 3 * n].reshape(ny, nx, 3)
        self.normal = self.buf[w + 3 * n:w + 6 * n].reshape(ny, nx, 3)
        self.depth = self.buf[w + 6 * n:w + 7 * n].reshape(ny, nx)
        block = make_features(None if features is True else features)
        C.memmove(C.addressof(self.features), C.addressof(block), Features.OUT_OFFSET)

    def flags(self):
        """make_params keywords of the parts the frame has."""
        return {"squares": self.squares, "counts": self.counts is not None, "retire": self.retire is not None,
                "denoise": self.denoise is not None, "features": True}


def features_frame(nx, ny, squares=False, counts=False, retire=False, denoise=None, features=None):
    """A zeroed FeaturesFrame whose blocks hold the in-fields of `features` (make_features) and `denoise` (make_denoise)."""
    return FeaturesFrame(nx, ny, squares, counts, retire, denoise, features)


def denoise_frame(nx, ny, counts=False, retire=False, denoise=None):
    """A zeroed DenoiseFrame whose block holds the in-fields of `denoise` (make_denoise: the defaults when None)."""
    return DenoiseFrame(nx, ny, counts, retire, denoise)


def counts_frame(nx, ny, squares=False, retire=False):
    """A zeroed CountsFrame (float planes + count plane in one buffer; retire=True: + the Retire block)."""
    return CountsFrame(nx, ny, squares, retire)


def _counts_call(out, counts, nx, ny, squares, retire=None):
    """(buffer to render into, float planes view): `out` / `counts` (/ `retire`) themselves when they already lie in memory
    as include/rtiow_gpu.h lays out the frame (a CountsFrame's views), else a staging CountsFrame holding copies of them."""
    counts = np.asarray(counts)
    if counts.shape != (ny, nx):
        raise ValueError("counts= must have shape (ny, nx) = %s" % ((ny, nx),))
    if (out.dtype == np.float32 and out.flags.c_contiguous and counts.dtype == np.uint32 and counts.flags.c_contiguous
            and out.ctypes.data + out.nbytes == counts.ctypes.data
            and (retire is None or C.addressof(retire) == out.ctypes.data + retire_block_offset(nx, ny))):
        return out, None
    f = CountsFrame(nx, ny, squares, retire is not None)
    f.planes[...] = out
    f.counts[...] = counts
    if retire is not None:
        C.memmove(C.addressof(f.retire), C.addressof(retire), C.sizeof(Retire))
    return f.planes, f


def _host_frame(out, nx, ny, kw):
    """The host framebuffer of a par_cast call: `out`, checked, or a new zeroed one -- [ny, nx, 3] float32, or [2, ny, nx, 3]
    with squares=True (the library writes both planes: a smaller array would be overrun)."""
    shape = (2, ny, nx, 3) if kw.get("squares") else (ny, nx, 3)
    if out is None:
        if _resumes(kw):
            raise ValueError("resume=True needs out= (the running sum to continue)")
        return np.zeros(shape, dtype=np.float32)
    if kw.get("squares") and not (isinstance(out, np.ndarray) and out.shape == shape and out.dtype == np.float32
                                  and out.flags.c_contiguous):
        raise ValueError("squares=True needs out= a C-contiguous float32 array of shape %s" % (shape,))
    return out


def _adaptive_host(cast, nx, ny, ns, step, target_se, min_samples, budget_s, out, seed, stats, radius, denoise, features, kw):
    """The host-frame loop of Scene.adaptive and Backend.adaptive_multi: `cast(ns, **keywords)` is the par_cast of either
    (camera and frame size bound); denoise / features: a checked Denoise / Features, or None."""
    if features is not None:
        f = FeaturesFrame(nx, ny, squares=True, counts=True, denoise=denoise) if out is None else out
        if (not isinstance(f, FeaturesFrame) or f.counts is None or f.retire is not None or not f.squares
                or (f.denoise is None) != (denoise is None)):
            raise ValueError("features=: out= must be a FeaturesFrame(nx, ny, squares=True, counts=True, denoise=...)")
        C.memmove(C.addressof(f.features), C.addressof(features), Features.OUT_OFFSET)
        if denoise is not None:
            C.memmove(C.addressof(f.denoise), C.addressof(denoise), Denoise.OUT_OFFSET)
    elif denoise is not None:
        f = DenoiseFrame(nx, ny, counts=True) if out is None else out
        if not isinstance(f, DenoiseFrame) or f.counts is None or f.retire is not None:
            raise ValueError("denoise=: out= must be a DenoiseFrame(nx, ny, counts=True)")
        C.memmove(C.addressof(f.denoise), C.addressof(denoise), Denoise.OUT_OFFSET)
    else:
        f = CountsFrame(nx, ny, squares=True) if out is None else out
        if not isinstance(f, CountsFrame):
            raise ValueError("out= must be a CountsFrame(nx, ny, squares=True)")
    more = () if features is None else (f,)
    if f.planes.shape != (2, ny, nx, 3):
        raise ValueError("out= must be a CountsFrame(nx, ny, squares=True)")
    f.counts[...] = ns
    active = np.ones((ny, nx), dtype=bool)
    t0 = time.perf_counter()
    done = 0
    while done < ns:
        end = min(ns, done + step)
        if features is not None:
            _, st = cast(end, seed=seed, out=f, denoise=True if denoise is not None else None, features=True, sample_begin=done,
                         resume=True, partial=True, squares=True, stats=True, counters=False, **kw)
            f.features.compute = 0   # (the planes are traced once)
        elif denoise is not None:
            _, st = cast(end, seed=seed, out=f, denoise=True, sample_begin=done, resume=True, partial=True, squares=True,
                         stats=True, counters=False, **kw)
        else:
            _, st = cast(end, seed=seed, out=f.planes, counts=f.counts, sample_begin=done, resume=True, partial=True, squares=True,
                         stats=True, counters=False, **kw)
        if stats is not None:
            stats.append(st)
        done = end
        held = np.minimum(f.counts, done).astype(np.uint32)
        se = noise.standard_error_counts(f.planes[0], f.planes[1], held)
        if radius:
            retire = noise.retire(active, done, se, min_samples, target_se, radius=radius, present=f.counts > 0)
        else:
            retire = noise.retire(active, done, se, min_samples, target_se)
        f.counts[retire] = done
        active &= ~retire
        pv = CountsFrame(nx, ny)   # resolve a copy: the running sums go on
        pv.planes[...] = f.planes[0]
        pv.counts[...] = held
        cast(done, seed=seed, out=pv.planes, counts=pv.counts, sample_begin=done, resume=True, **kw)
        if denoise is not None:
            yield (held, pv.planes, se, f.denoised.copy()) + more
        else:
            yield (held, pv.planes, se) + more
        if not active.any():
            return
        if budget_s is not None and time.perf_counter() - t0 >= budget_s:
            return


# error codes of include/rtiow_gpu.h
ERR_INVALID, ERR_EMPTY_BVH, ERR_NAN, ERR_RANGE, ERR_UNSUPPORTED, ERR_DEVICE = -1, -2, -3, -4, -5, -6


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rt error %d: %s" % (code, msg))
        self.code = code


def _f3(v):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))


# every symbol include/rtiow_gpu.h declares (suffix after the prefix); test_abi checks all of them
ABI_SYMBOLS = [
    "version", "last_error", "device_count", "builder_create", "builder_destroy",
    "texture_constant", "texture_checker", "texture_perlin", "builder_set_perlin_tables",
    "material_lambertian", "material_metal", "material_dielectric", "material_diffuse_light",
    "material_isotropic", "object_sphere", "object_rect", "object_flip_normals", "object_translate",
    "object_scale", "object_rotate_y", "object_and", "object_rect_prism", "object_linear_move",
    "object_constant_medium", "object_bvh", "object_bvh_sah", "camera_look", "scene_create", "scene_destroy",
    "scene_set_option", "scene_info", "par_cast", "par_cast_device", "par_cast_multi", "multi_reset", "debug_hit_top", "debug_samples", "debug_math", "debug_flatten", "debug_flatten_pool2", "tonemap", "tonemap_device",
]


class Backend:
    """A loaded library + symbol prefix."""

    def __init__(self, path, prefix):
        if not os.path.exists(path):
            raise FileNotFoundError(
                "%s not found -- build it first (python -c 'import __graft_entry__ as g; g.build()')" % path)
        self.path = path
        self.prefix = prefix
        self.lib = C.CDLL(path)
        f = self._fn
        f("last_error", C.c_char_p, [])
        f("version", C.c_char_p, [])
        f("builder_create", C.c_int, [C.POINTER(C.c_void_p)])
        f("builder_destroy", None, [C.c_void_p])
        f("texture_constant", C.c_uint32, [C.c_void_p, c_f32p])
        f("texture_checker", C.c_uint32, [C.c_void_p, C.c_uint32, C.c_uint32])
        f("texture_perlin", C.c_uint32, [C.c_void_p, C.c_float])
        f("builder_set_perlin_tables", C.c_int, [C.c_void_p, c_f32p, c_u8p, c_u8p, c_u8p])
        f("material_lambertian", C.c_uint32, [C.c_void_p, C.c_uint32])
        f("material_metal", C.c_uint32, [C.c_void_p, c_f32p, C.c_float])
        f("material_dielectric", C.c_uint32, [C.c_void_p, C.c_float])
        f("material_diffuse_light", C.c_uint32, [C.c_void_p, C.c_uint32, C.c_float])
        f("material_isotropic", C.c_uint32, [C.c_void_p, C.c_uint32])
        f("object_sphere", C.c_uint32, [C.c_void_p, C.c_float, C.c_uint32])
        f("object_rect", C.c_uint32, [C.c_void_p, C.c_int] + [C.c_float] * 5 + [C.c_uint32])
        f("object_flip_normals", C.c_uint32, [C.c_void_p, C.c_uint32])
        f("object_translate", C.c_uint32, [C.c_void_p, c_f32p, C.c_uint32])
        f("object_scale", C.c_uint32, [C.c_void_p, c_f32p, C.c_uint32])
        f("object_rotate_y", C.c_uint32, [C.c_void_p, C.c_float, C.c_uint32])
        f("object_and", C.c_uint32, [C.c_void_p, C.c_uint32, C.c_uint32])
        f("object_rect_prism", C.c_uint32, [C.c_void_p, c_f32p, c_f32p, C.c_uint32])
        f("object_linear_move", C.c_uint32, [C.c_void_p, C.c_uint32, c_f32p])
        f("object_constant_medium", C.c_uint32, [C.c_void_p, C.c_uint32, C.c_float, C.c_uint32])
        f("object_bvh", C.c_uint32, [C.c_void_p, c_u32p, C.c_size_t, C.c_float, C.c_float])
        f("object_bvh_sah", C.c_uint32, [C.c_void_p, c_u32p, C.c_size_t, C.c_float, C.c_float])
        f("camera_look", C.c_int, [c_f32p, c_f32p, c_f32p] + [C.c_float] * 6 + [C.POINTER(Camera)])
        f("scene_create", C.c_int, [C.c_void_p, c_u32p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)])
        f("scene_destroy", None, [C.c_void_p])
        self._declare_render()
        f("debug_hit_top", C.c_int, [C.c_void_p, C.c_size_t, c_f32p, C.c_uint64, C.c_float, c_f32p, c_u32p])
        f("debug_samples", C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_size_t,
                                     c_u32p, c_u32p, c_u32p, c_f32p, c_u32p])
        f("debug_math", C.c_int, [C.c_int, C.c_int, C.c_size_t, c_f32p, c_f32p, c_f32p])
        f("tonemap", C.c_int, [C.c_int, C.c_size_t, c_f32p, c_u8p])

    def _declare_render(self):
        f = self._fn
        f("device_count", C.c_int, [C.POINTER(C.c_int)])
        f("scene_set_option", C.c_int, [C.c_void_p, C.c_char_p, C.c_int])
        f("scene_info", C.c_int, [C.c_void_p, c_u32p, c_u32p, c_u32p, C.POINTER(C.c_uint64), c_u32p])
        f("par_cast", C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), c_f32p, C.POINTER(Stats)])
        f("par_cast_device", C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(Params), C.c_void_p,
                                       C.c_void_p, C.POINTER(Stats)])
        f("par_cast_multi", C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Camera), C.POINTER(Params), c_f32p,
                                      C.POINTER(Stats)])
        f("multi_reset", C.c_int, [C.c_char_p, C.POINTER(C.c_uint64)])
        f("debug_flatten", C.c_int, [C.c_void_p, c_u32p, C.c_size_t, c_u32p, c_u32p, c_u32p, C.c_size_t])
        f("debug_flatten_pool2", C.c_int, [C.c_void_p, c_u32p, C.c_size_t, c_u32p, c_u32p, c_u32p, C.c_size_t])
        f("tonemap_device", C.c_int, [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p])

    def _fn(self, name, restype, argtypes):
        try:
            fn = getattr(self.lib, self.prefix + name)
        except AttributeError:   # an OLDER build of the library (RTIOW_GPU_LIB A/B runs): the call fails when it is made
            def fn(*_a, _n=self.prefix + name):
                raise RtError(ERR_INVALID, "%s: symbol %s is not exported by this build" % (self.path, _n))
            setattr(self, "_" + name, fn)
            return fn
        fn.restype = restype
        fn.argtypes = argtypes
        setattr(self, "_" + name, fn)
        return fn

    def last_error(self):
        return (self._last_error() or b"").decode()

    def check(self, code):
        if code != 0:
            raise RtError(code, self.last_error())

    def check_id(self, i):
        if i == INVALID_ID:
            raise RtError(-1, self.last_error())
        return i

    def builder(self):
        return Builder(self)

    def device_count(self):
        n = C.c_int(0)
        self.check(self._device_count(C.byref(n)))
        return n.value

    def camera_look(self, look_from, look_at, up, fov, aspect, aperture, focus_dist, exposure=(0.0, 1.0)):
        """Camera::look, camera.rs:18-50"""
        cam = Camera()
        self.check(self._camera_look(_f3(look_from), _f3(look_at), _f3(up), fov, aspect, aperture,
                                     focus_dist, exposure[0], exposure[1], C.byref(cam)))
        return cam

    def par_cast_multi(self, scenes, camera, nx, ny, ns, seed=0xDEADBEEF, stats=False, out=None, counters=None, **kw):
        """rtg_par_cast_multi: one scene handle per device (the same world flattened on each), tiles sharded over
        them, ONE RCCL reduce(sum) of the float3 framebuffer inside the library.  Returns the assembled frame.
        resume=True, sample_begin=k: `out` holds the running sum of samples [0, k) (as a partial=True call left it).
        With scene option "multi_planes" on a handle the call also takes the flagged frames of Scene.par_cast: out= a
        CountsFrame, DenoiseFrame or FeaturesFrame is rendered in place and returned, its flags those of the parts it has
        (denoise= / features= other than True replace the blocks' in-fields first, retire= a Retire those of its block); a
        [2, ny, nx, 3] array with squares=True as before; and counts= an array, retire= a Retire, denoise= / features= a
        block or a dict beside an array `out` go through a staging frame as in Scene.par_cast (a denoise / features call
        returns that frame).  Plain flags beside a plain array (counts=True, ...) are forwarded to the library as they are.
        stats=True returns (frame, rtg_stats as a dict), with the instrumented counters unless counters=False."""
        counts, retire, denoise, features = kw.get("counts"), kw.get("retire"), kw.get("denoise"), kw.get("features")
        if (isinstance(out, (CountsFrame, DenoiseFrame, FeaturesFrame)) or isinstance(counts, np.ndarray) or isinstance(retire, Retire)
                or isinstance(denoise, (dict, Denoise)) or isinstance(features, (dict, Features))):
            return self._par_cast_multi_planes(scenes, camera, nx, ny, ns, seed, stats, out, counters, kw)
        p = make_params(nx, ny, ns, seed=seed, flags=FLAG_COUNTERS if stats and counters is not False else 0, **kw)
        out = _host_frame(out, nx, ny, kw)
        st = self._par_cast_multi_call(scenes, camera, p, out)
        return (out, st.as_dict()) if stats else out

    def _par_cast_multi_call(self, scenes, camera, p, buf):
        st = Stats()
        st.struct_size = C.sizeof(Stats)
        arr = (C.c_void_p * len(scenes))(*[s.h for s in scenes])
        self.check(self._par_cast_multi(arr, len(scenes), C.byref(camera), C.byref(p), buf.ctypes.data_as(c_f32p), C.byref(st)))
        return st

    def _par_cast_multi_planes(self, scenes, camera, nx, ny, ns, seed, stats, out, counters, kw):
        """par_cast_multi on a frame object (in place) or through a staging frame: every check is made before the library call."""
        kw = dict(kw)
        counts, retire, denoise, features = (kw.pop(k, None) for k in ("counts", "retire", "denoise", "features"))
        squares = kw.pop("squares", None)
        has_dn = denoise is not None and denoise is not False
        has_ft = features is not None and features is not False
        in_place = isinstance(out, (CountsFrame, DenoiseFrame, FeaturesFrame))
        if in_place:
            f = out
            if f.planes.shape[-3:] != (ny, nx, 3):
                raise ValueError("out= is a %s of another size" % type(f).__name__)
            if isinstance(counts, np.ndarray):
                raise ValueError("out= a %s brings its own counts view" % type(f).__name__)
            f_dn, f_ft = getattr(f, "denoise", None), getattr(f, "features", None)
            if squares is not None and bool(squares) != (f.planes.ndim == 4):
                raise ValueError("out= a %s: squares= must say what the frame holds" % type(f).__name__)
            if (has_dn and f_dn is None) or (has_ft and f_ft is None) or (retire is not None and retire is not False and f.retire is None):
                raise ValueError("out= a %s has no such block" % type(f).__name__)
            if isinstance(retire, Retire):
                C.memmove(C.addressof(f.retire), C.addressof(retire), Retire.active.offset)
            if has_dn and denoise is not True:
                block = make_denoise(denoise)
                C.memmove(C.addressof(f_dn), C.addressof(block), Denoise.OUT_OFFSET)
            if has_ft and features is not True:
                block = make_features(features)
                C.memmove(C.addressof(f_ft), C.addressof(block), Features.OUT_OFFSET)
            flags = {"squares": f.planes.ndim == 4, "counts": f.counts is not None, "retire": f.retire is not None,
                     "denoise": f_dn is not None, "features": f_ft is not None}
        else:
            if counts is not None and not isinstance(counts, np.ndarray):
                raise ValueError("counts= must be a uint32 array beside retire= / denoise= / features= blocks (or pass a frame as out=)")
            if retire is not None and (not isinstance(retire, Retire) or counts is None or not squares):
                raise ValueError("retire= needs a Retire, squares=True and counts= a uint32 array (the call writes it)")
            if has_dn and not squares:
                raise ValueError("denoise= needs squares=True (the filter reads both planes)")
            if counts is not None and np.asarray(counts).shape != (ny, nx):
                raise ValueError("counts= must have shape (ny, nx) = %s" % ((ny, nx),))
            sq = {"squares": True} if squares else {}
            if out is None and _resumes(kw):
                raise ValueError("resume=True needs out= (the running sum to continue)")
            if has_ft:
                f = FeaturesFrame(nx, ny, squares, counts is not None, retire is not None, denoise if has_dn else None,
                                  None if features is True else features)
            elif has_dn:
                f = DenoiseFrame(nx, ny, counts is not None, retire is not None, None if denoise is True else denoise)
            else:
                f = None
            if f is None:   # counts (and retire) alone: in place when `out` and `counts` are one CountsFrame's views
                out = _host_frame(out, nx, ny, sq)
                dst, f = _counts_call(out, counts, nx, ny, squares, retire)
                buf = dst if f is None else f.buf
            else:
                if out is not None:
                    f.planes[...] = _host_frame(out, nx, ny, sq)
                if counts is not None:
                    f.counts[...] = counts
                if retire is not None:
                    C.memmove(C.addressof(f.retire), C.addressof(retire), C.sizeof(Retire))
                buf = f.buf
            flags = {"squares": bool(squares), "counts": counts is not None, "retire": retire is not None, "denoise": has_dn,
                     "features": has_ft}
        if in_place:
            buf = f.buf
        for part, check in ((flags["squares"], _squares_supported), (flags["counts"], _counts_supported),
                            (flags["retire"], _retire_supported), (flags["denoise"], _denoise_supported),
                            (flags["features"], _features_supported)):
            if part:
                check(self)
        p = make_params(nx, ny, ns, seed=seed, flags=FLAG_COUNTERS if stats and counters is not False else 0, **flags, **kw)
        st = self._par_cast_multi_call(scenes, camera, p, buf)
        if in_place:
            ret = f
        else:
            if f is not None and out is not None:
                out[...] = f.planes
            if f is not None and retire is not None:   # (the library wrote the count plane and the block's out-fields)
                counts[...] = f.counts
                C.memmove(C.addressof(retire), C.addressof(f.retire), C.sizeof(Retire))
            ret = f if (has_dn or has_ft) else out
        return (ret, st.as_dict()) if stats else ret

    def adaptive_multi(self, scenes, camera, nx, ny, ns, step, target_se, min_samples=16, budget_s=None, out=None, seed=0xDEADBEEF,
                       stats=None, radius=0, denoise=None, features=None, **kw):
        """Scene.adaptive's host-frame loop over several handles (scene option "multi_planes" on one of them): every slice is
        one par_cast_multi call, the retire rule is noise.retire on the host, and the loop yields the same tuples --
        (counts, preview, stderr), then the filtered frame with denoise=, then the FeaturesFrame with features=."""
        if step < 1:
            raise ValueError("step must be >= 1")
        if not 0 <= radius <= RETIRE_MAX_RADIUS:
            raise ValueError("radius must be in 0 .. %d" % RETIRE_MAX_RADIUS)
        _squares_supported(self)
        _counts_supported(self)
        features = make_features(None if features is True else features) if features is not None and features is not False else None
        denoise = make_denoise(None if denoise is True else denoise) if denoise is not None and denoise is not False else None
        yield from _adaptive_host(lambda n, **k: self.par_cast_multi(scenes, camera, nx, ny, n, **k), nx, ny, ns, step,
                                  target_se, min_samples, budget_s, out, seed, stats, radius, denoise, features, kw)

    def multi_reset(self, rccl_library=None):
        """rtg_multi_reset: drop the cached RCCL communicators, unload librccl, choose the library to load next (None =
        default search).  Returns the number of ncclReduce calls issued since the last reset."""
        n = C.c_uint64(0)
        self.check(self._multi_reset(rccl_library.encode() if rccl_library else None, C.byref(n)))
        return n.value

    def tonemap(self, img, device=0):
        """print_ppm's sqrt-gamma + `(255.99 * x) as i32` clamp (lib.rs:348-356) -> uint8 array of img's shape."""
        x = np.ascontiguousarray(img, dtype=np.float32)
        out = np.empty(x.shape, dtype=np.uint8)
        self.check(self._tonemap(device, x.size, x.ctypes.data_as(c_f32p), out.ctypes.data_as(c_u8p)))
        return out

    def debug_math(self, op, x, y=None, device=0):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float32)
            yp = y.ctypes.data_as(c_f32p)
        self.check(self._debug_math(device, op, x.size, x.ctypes.data_as(c_f32p), yp,
                                    out.ctypes.data_as(c_f32p)))
        return out


class Builder:
    """Scene under construction.  One method per reference constructor."""

    def __init__(self, backend):
        self.be = backend
        h = C.c_void_p()
        backend.check(backend._builder_create(C.byref(h)))
        self.h = h
        self._scenes = []

    def close(self):
        if self.h:
            self.be._builder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # texture.rs
    def constant(self, color):
        return self.be.check_id(self.be._texture_constant(self.h, _f3(color)))

    def checker(self, t0, t1):
        return self.be.check_id(self.be._texture_checker(self.h, t0, t1))

    def perlin(self, scale):
        return self.be.check_id(self.be._texture_perlin(self.h, scale))

    def set_perlin_tables(self, vecs, perm_x, perm_y, perm_z):
        vecs = np.ascontiguousarray(vecs, dtype=np.float32).reshape(768)
        px, py, pz = (np.ascontiguousarray(a, dtype=np.uint8) for a in (perm_x, perm_y, perm_z))
        self.be.check(self.be._builder_set_perlin_tables(
            self.h, vecs.ctypes.data_as(c_f32p), px.ctypes.data_as(c_u8p), py.ctypes.data_as(c_u8p),
            pz.ctypes.data_as(c_u8p)))

    # material.rs
    def lambertian(self, albedo):
        return self.be.check_id(self.be._material_lambertian(self.h, albedo))

    def metal(self, albedo, fuzz):
        return self.be.check_id(self.be._material_metal(self.h, _f3(albedo), fuzz))

    def dielectric(self, ref_idx):
        return self.be.check_id(self.be._material_dielectric(self.h, ref_idx))

    def diffuse_light(self, emission, brightness):
        return self.be.check_id(self.be._material_diffuse_light(self.h, emission, brightness))

    def isotropic(self, albedo):
        return self.be.check_id(self.be._material_isotropic(self.h, albedo))

    # object.rs / bvh.rs
    def sphere(self, radius, material):
        return self.be.check_id(self.be._object_sphere(self.h, radius, material))

    def rect(self, orthogonal_to, range0, range1, k, material):
        return self.be.check_id(self.be._object_rect(self.h, orthogonal_to, range0[0], range0[1],
                                                     range1[0], range1[1], k, material))

    def flip_normals(self, obj):
        return self.be.check_id(self.be._object_flip_normals(self.h, obj))

    def translate(self, offset, obj):
        return self.be.check_id(self.be._object_translate(self.h, _f3(offset), obj))

    def scale(self, factor, obj):
        return self.be.check_id(self.be._object_scale(self.h, _f3(factor), obj))

    def rotate_y(self, degrees, obj):
        return self.be.check_id(self.be._object_rotate_y(self.h, degrees, obj))

    def and_(self, a, b):
        return self.be.check_id(self.be._object_and(self.h, a, b))

    def rect_prism(self, p0, p1, material):
        return self.be.check_id(self.be._object_rect_prism(self.h, _f3(p0), _f3(p1), material))

    def linear_move(self, obj, motion):
        return self.be.check_id(self.be._object_linear_move(self.h, obj, _f3(motion)))

    def constant_medium(self, boundary, density, material):
        return self.be.check_id(self.be._object_constant_medium(self.h, boundary, density, material))

    def bvh(self, objs, exposure=(0.0, 1.0)):
        """bvh::from_scene, bvh.rs:128"""
        arr = (C.c_uint32 * max(1, len(objs)))(*objs)
        return self.be.check_id(self.be._object_bvh(self.h, arr, len(objs), exposure[0], exposure[1]))

    def flatten(self, world):
        """Host-only (product library): the flat program as uint32 [n, 8] plus the feature mask."""
        arr = (C.c_uint32 * max(1, len(world)))(*world)
        n, feat = C.c_uint32(), C.c_uint32()
        self.be.check(self.be._debug_flatten(self.h, arr, len(world), C.byref(n), C.byref(feat), None, 0))
        words = np.zeros((n.value, 8), dtype=np.uint32)
        self.be.check(self.be._debug_flatten(self.h, arr, len(world), C.byref(n), C.byref(feat),
                                             words.ctypes.data_as(c_u32p), n.value))
        return words, feat.value

    def flatten_pool2(self, world):
        """The second flat program (pool-2 kernel) and its item table: (words [n, 8], items [(kind, a, b, c)], n_media, n_wrapped);
        words has 0 rows when the world has another shape."""
        arr = (C.c_uint32 * max(1, len(world)))(*world)
        n = C.c_uint32()
        table = np.zeros(24, dtype=np.uint32)
        self.be.check(self.be._debug_flatten_pool2(self.h, arr, len(world), C.byref(n), table.ctypes.data_as(c_u32p), None, 0))
        words = np.zeros((n.value, 8), dtype=np.uint32)
        self.be.check(self.be._debug_flatten_pool2(self.h, arr, len(world), C.byref(n), table.ctypes.data_as(c_u32p),
                                                   words.ctypes.data_as(c_u32p), n.value))
        items = [tuple(int(v) for v in table[4 * k:4 * k + 4]) for k in range(int(table[20]))]
        return words, items, int(table[21]), int(table[22])

    def bvh_sah(self, objs, exposure=(0.0, 1.0)):
        """Not in the reference: SAH-built Bvh; same results up to exact-t ties, fewer box tests."""
        arr = (C.c_uint32 * max(1, len(objs)))(*objs)
        return self.be.check_id(self.be._object_bvh_sah(self.h, arr, len(objs), exposure[0], exposure[1]))

    def scene(self, world, device=0):
        """Flatten `world` (the `[Box<dyn Object>]` of lib.rs:33) once into device memory."""
        arr = (C.c_uint32 * max(1, len(world)))(*world)
        h = C.c_void_p()
        self.be.check(self.be._scene_create(self.h, arr, len(world), device, C.byref(h)))
        sc = self.be.scene_class(self.be, h, self)
        sc.apply_env_options()
        return sc


class Scene:
    def __init__(self, backend, handle, builder):
        self.be = backend
        self.h = handle
        self._builder = builder  # keep alive

    def close(self):
        if self.h:
            self.be._scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # measurement / test hook: RTG_<OPTION>=<int> in the environment of the PYTHON process becomes
    # rtg_scene_set_option(scene, "<option>", <int>) -- the library itself reads no environment variable
    ENV_OPTIONS = ("kernel", "chunks", "lpt", "lpt_phase1", "lpt_deep", "lpt_shift", "ray_lds", "sync", "block", "wg_per_cu", "window",
                   "box_leave", "refill_min", "gather_min", "run_ahead", "run_ahead_min", "sphere_min", "verbose", "bvh4", "box_chains", "force_rccl", "multi_gather", "multi_planes", "scratch_mb", "frames_in_flight", "small_frames", "drain_share", "hoist", "deep_sized", "mat_lds", "pool2", "p2_refill", "p2_box_leave", "p2_park", "p2_sphere", "p2_prism", "p2_list", "p2_push")

    def set_option(self, name, value):
        self.be.check(self.be._scene_set_option(self.h, name.encode(), int(value)))

    def apply_env_options(self):
        if not hasattr(self.be, "_scene_set_option"):
            return
        for name in self.ENV_OPTIONS:
            v = os.environ.get("RTG_" + name.upper())
            if v is not None:
                self.set_option(name, int(v))

    def info(self):
        a, b, c, d, e = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
        self.be.check(self.be._scene_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
        return {"instructions": a.value, "materials": b.value, "textures": c.value, "hbm_bytes": d.value, "box_followers": e.value}

    def _par_cast_args(self, args, threads):
        return args

    def par_cast(self, camera, nx, ny, ns, seed=0xDEADBEEF, stats=False, out=None, threads=0, counts=None, counters=None,
                 retire=None, denoise=None, features=None, **kw):
        """par_cast, lib.rs:363.  Returns float32 [ny, nx, 3], row 0 = top, linear radiance.
        One slice of a progressive frame: partial=True leaves the running sum in `out`; resume=True, sample_begin=k
        continues the running sum of samples [0, k) that `out` holds (include/rtiow_gpu.h).
        squares=True (RTG_FLAG_SUM_SQUARES): float32 [2, ny, nx, 3] instead -- [0] as without the flag, [1] the running sum
        of the squared sample colours; `out`, when given, must have that shape.
        counts= (RTG_FLAG_SAMPLE_COUNTS): uint32 [ny, nx], every pixel's own sample count n_p -- the call renders samples
        [sample_begin, min(n_p, ns)) of each pixel; pixels with n_p = 0 are left as `out` holds them.  `out` and `counts` of
        one CountsFrame are rendered in place; anything else goes through a staging copy.
        retire= (RTG_FLAG_RETIRE; needs counts= and squares=True): a Retire whose target_se / min_samples / radius the call
        applies after its slice -- retiring pixels get n_p = ns in `counts` -- and whose out-fields it fills.  counts= must then
        be a uint32 array the call can write (a CountsFrame(retire=True)'s counts and retire render in place).
        denoise= (RTG_FLAG_DENOISE; needs squares=True): the call also filters the frame (denoise.nlm) and returns a DenoiseFrame
        instead of an array -- views `planes`, `counts`, `retire`, `denoise` (the block, out-fields filled) and `denoised` (the
        output plane).  denoise: a Denoise or a dict of k / radius / patch (True: the defaults).  out= a DenoiseFrame is
        rendered in place and returned (denoise=True: its block as it stands; its own counts / retire views are used); with
        any other out / counts / retire a new frame carries copies of them, and they are written back as without denoise=.
        features= (RTG_FLAG_FEATURES): the call also traces the first-hit albedo, normal and depth planes and returns a
        FeaturesFrame -- the views above where the frame has them, plus `features` (the block, out-fields filled), `albedo`,
        `normal` and `depth`.  features: a Features or a dict of grid / compute / sigma_* (True: FEATURES_DEFAULTS).  With
        denoise= the filter is the guided one (denoise.nlm_guided) over the frame's feature planes.  out= a FeaturesFrame is
        rendered in place and returned (features=True / denoise=True: its blocks as they stand); anything else is copied into
        a new frame and written back as without features=.
        stats=True returns (out, rtg_stats as a dict), with the instrumented counters unless counters=False."""
        if features is not None and features is not False:
            if denoise is not None and denoise is not False and not kw.get("squares"):
                raise ValueError("denoise= needs squares=True (the filter reads both planes)")
            _features_supported(self.be)
            return self._par_cast_features(camera, nx, ny, ns, seed, stats, out, threads, counts, counters, retire, denoise,
                                           features, kw)
        if denoise is not None and denoise is not False:
            if not kw.get("squares"):
                raise ValueError("denoise= needs squares=True (the filter reads both planes)")
            _denoise_supported(self.be)
            return self._par_cast_denoise(camera, nx, ny, ns, seed, stats, out, threads, counts, counters, retire, denoise, kw)
        if kw.get("squares"):
            _squares_supported(self.be)
        if counts is not None:
            _counts_supported(self.be)
        if retire is not None:
            _retire_supported(self.be)
            if counts is None or not kw.get("squares") or not isinstance(counts, np.ndarray):
                raise ValueError("retire= needs squares=True and counts= a uint32 array (the call writes it)")
        if counters is None:
            counters = stats
        p = make_params(nx, ny, ns, seed=seed, flags=FLAG_COUNTERS if stats and counters else 0, counts=counts is not None,
                        retire=retire is not None, **kw)
        out = _host_frame(out, nx, ny, kw)
        dst, staging = (out, None) if counts is None else _counts_call(out, counts, nx, ny, kw.get("squares"), retire)
        st = Stats()
        st.struct_size = C.sizeof(Stats)
        args = self._par_cast_args([self.h, C.byref(camera), C.byref(p), dst.ctypes.data_as(c_f32p), C.byref(st)],
                                   threads)
        self.be.check(self.be._par_cast(*args))
        if staging is not None:
            out[...] = staging.planes
            if retire is not None:   # (the library wrote the count plane and the block's out-fields)
                counts[...] = staging.counts
                C.memmove(C.addressof(retire), C.addressof(staging.retire), C.sizeof(Retire))
        return (out, st.as_dict()) if stats else out

    def _par_cast_denoise(self, camera, nx, ny, ns, seed, stats, out, threads, counts, counters, retire, denoise, kw):
        _squares_supported(self.be)
        in_place = isinstance(out, DenoiseFrame)
        if in_place:
            f = out
            if (f.nx, f.ny) != (nx, ny):
                raise ValueError("out= is a DenoiseFrame of another size")
            if counts is not None or retire is not None:
                raise ValueError("out= a DenoiseFrame brings its own counts / retire views")
            if denoise is not True:
                block = make_denoise(denoise)
                C.memmove(C.addressof(f.denoise), C.addressof(block), Denoise.OUT_OFFSET)
        else:
            if retire is not None and (counts is None or not isinstance(counts, np.ndarray)):
                raise ValueError("retire= needs squares=True and counts= a uint32 array (the call writes it)")
            f = DenoiseFrame(nx, ny, counts is not None, retire is not None, None if denoise is True else denoise)
            if out is not None:
                f.planes[...] = _host_frame(out, nx, ny, kw)
            elif _resumes(kw):
                raise ValueError("resume=True needs out= (the running sum to continue)")
            if counts is not None:
                counts = np.asarray(counts)
                if counts.shape != (ny, nx):
                    raise ValueError("counts= must have shape (ny, nx) = %s" % ((ny, nx),))
                f.counts[...] = counts
            if retire is not None:
                C.memmove(C.addressof(f.retire), C.addressof(retire), C.sizeof(Retire))
        if f.counts is not None:
            _counts_supported(self.be)
        if f.retire is not None:
            _retire_supported(self.be)
        if counters is None:
            counters = stats
        p = make_params(nx, ny, ns, seed=seed, flags=FLAG_COUNTERS if stats and counters else 0, counts=f.counts is not None,
                        retire=f.retire is not None, denoise=True, **kw)
        st = Stats()
        st.struct_size = C.sizeof(Stats)
        args = self._par_cast_args([self.h, C.byref(camera), C.byref(p), f.buf.ctypes.data_as(c_f32p), C.byref(st)], threads)
        self.be.check(self.be._par_cast(*args))
        if not in_place:
            if out is not None:
                out[...] = f.planes
            if retire is not None:
                counts[...] = f.counts
                C.memmove(C.addressof(retire), C.addressof(f.retire), C.sizeof(Retire))
        return (f, st.as_dict()) if stats else f

    def _par_cast_features(self, camera, nx, ny, ns, seed, stats, out, threads, counts, counters, retire, denoise, features, kw):
        has_dn = denoise is not None and denoise is not False
        in_place = isinstance(out, FeaturesFrame)
        if in_place:
            f = out
            if (f.nx, f.ny) != (nx, ny):
                raise ValueError("out= is a FeaturesFrame of another size")
            if counts is not None or retire is not None:
                raise ValueError("out= a FeaturesFrame brings its own counts / retire views")
            if has_dn != (f.denoise is not None) or bool(kw.get("squares")) != f.squares:
                raise ValueError("out= a FeaturesFrame: squares= / denoise= must say what the frame holds")
            if has_dn and denoise is not True:
                block = make_denoise(denoise)
                C.memmove(C.addressof(f.denoise), C.addressof(block), Denoise.OUT_OFFSET)
            if features is not True:
                block = make_features(features)
                C.memmove(C.addressof(f.features), C.addressof(block), Features.OUT_OFFSET)
        else:
            if retire is not None and (counts is None or not kw.get("squares") or not isinstance(counts, np.ndarray)):
                raise ValueError("retire= needs squares=True and counts= a uint32 array (the call writes it)")
            if isinstance(out, (DenoiseFrame, CountsFrame)):
                raise ValueError("features=: out= must be a FeaturesFrame or an array")
            f = FeaturesFrame(nx, ny, kw.get("squares"), counts is not None, retire is not None, denoise if has_dn else None,
                              None if features is True else features)
            if out is not None:
                f.planes[...] = _host_frame(out, nx, ny, kw)
            elif _resumes(kw):
                raise ValueError("resume=True needs out= (the running sum to continue)")
            if counts is not None:
                counts = np.asarray(counts)
                if counts.shape != (ny, nx):
                    raise ValueError("counts= must have shape (ny, nx) = %s" % ((ny, nx),))
                f.counts[...] = counts
            if retire is not None:
                C.memmove(C.addressof(f.retire), C.addressof(retire), C.sizeof(Retire))
        for part, check in ((f.squares, _squares_supported), (f.counts is not None, _counts_supported),
                            (f.retire is not None, _retire_supported), (f.denoise is not None, _denoise_supported)):
            if part:
                check(self.be)
        if counters is None:
            counters = stats
        kw = {k: v for k, v in kw.items() if k != "squares"}
        p = make_params(nx, ny, ns, seed=seed, flags=FLAG_COUNTERS if stats and counters else 0, **f.flags(), **kw)
        st = Stats()
        st.struct_size = C.sizeof(Stats)
        args = self._par_cast_args([self.h, C.byref(camera), C.byref(p), f.buf.ctypes.data_as(c_f32p), C.byref(st)], threads)
        self.be.check(self.be._par_cast(*args))
        if not in_place:
            if out is not None:
                out[...] = f.planes
            if retire is not None:
                counts[...] = f.counts
                C.memmove(C.addressof(retire), C.addressof(f.retire), C.sizeof(Retire))
        return (f, st.as_dict()) if stats else f

    def par_cast_device(self, camera, params, d_out_ptr, stream=None, want_stats=False, sample_begin=None, partial=None,
                        resume=None, squares=None, counts=None, retire=None, denoise=None, features=None):
        """rtg_par_cast_device.  sample_begin / partial / resume / squares, when given, override those of `params` (a copy).
        With RTG_FLAG_SUM_SQUARES `d_out_ptr` must hold 2 * nx * ny * 3 floats.
        counts= (RTG_FLAG_SAMPLE_COUNTS): a uint32 [ny, nx] array -- numpy (copied host to device) or a device tensor
        (copied device to device) -- written to the count plane behind the float planes of `d_out_ptr` on `stream` before the
        call; True: the flag alone, the caller has filled the count plane.  `d_out_ptr` then holds nx * ny more words.
        retire= (RTG_FLAG_RETIRE): True, the flag alone (the caller has written the block's in-fields on the device); a Retire,
        written to the block before the call and filled from it afterwards (the call then synchronises `stream`).  `d_out_ptr`
        then holds retire_frame_bytes(nx, ny).
        denoise= (RTG_FLAG_DENOISE): True, the flag alone (the caller has written the block's in-fields on the device); a
        Denoise, written to the block before the call and filled from it afterwards (the call then synchronises `stream`).
        `d_out_ptr` then holds denoise_frame_bytes(nx, ny, counts, retire) for the flags the call ends up with.
        features= (RTG_FLAG_FEATURES): True, the flag alone (the caller has written the block's in-fields on the device); a
        Features, written to the block before the call and filled from it afterwards (the call then synchronises `stream`).
        `d_out_ptr` then holds features_frame_bytes(nx, ny, squares, counts, retire, denoise) for the flags the call ends up with."""
        dblock = fblock = None   # (every refusal first: a refused call has written nothing to the caller's frame)
        if features is not None and features is not False:
            _features_supported(self.be)
        if denoise is not None and denoise is not False:
            _denoise_supported(self.be)
        if squares or (squares is None and params.flags & FLAG_SUM_SQUARES):
            _squares_supported(self.be)
        if counts is not None and counts is not False:
            _counts_supported(self.be)
        if retire is not None and retire is not False:
            _retire_supported(self.be)
        if denoise is not None and denoise is not False:
            has = [bool(params.flags & bit) if on is None else on is not False
                   for on, bit in ((counts, FLAG_SAMPLE_COUNTS), (retire, FLAG_RETIRE))]
            d_off = denoise_block_offset(params.nx, params.ny, has[0], has[1])
            if denoise is not True:
                dblock = denoise
                self._block_copy(params.nx, params.ny, d_out_ptr, dblock, stream, to_device=True, offset=d_off, nbytes=Denoise.OUT_OFFSET)
                denoise = True
        if features is not None and features is not False:
            has = [bool(params.flags & bit) if on is None else on is not False
                   for on, bit in ((squares, FLAG_SUM_SQUARES), (counts, FLAG_SAMPLE_COUNTS), (retire, FLAG_RETIRE), (denoise, FLAG_DENOISE))]
            f_off = features_block_offset(params.nx, params.ny, *has)
            if features is not True:
                fblock = features
                self._block_copy(params.nx, params.ny, d_out_ptr, fblock, stream, to_device=True, offset=f_off, nbytes=Features.OUT_OFFSET)
                features = True
        block = None
        if retire is not None and retire is not False:
            if retire is not True:
                block = retire
                self._block_copy(params.nx, params.ny, d_out_ptr, block, stream, to_device=True)
                retire = True
        if counts is not None and counts is not True and counts is not False:
            sq = squares if squares is not None else bool(params.flags & FLAG_SUM_SQUARES)
            self._upload_counts(params.nx, params.ny, sq, counts, d_out_ptr, stream)
            counts = True
        if (sample_begin is not None or partial is not None or resume is not None or squares is not None or counts is not None
                or retire is not None or denoise is not None or features is not None):
            q = Params()
            C.pointer(q)[0] = params
            if sample_begin is not None:
                q.sample_begin = sample_begin
            for on, bit in ((partial, FLAG_PARTIAL), (resume, FLAG_RESUME), (squares, FLAG_SUM_SQUARES), (counts, FLAG_SAMPLE_COUNTS),
                            (retire, FLAG_RETIRE), (denoise, FLAG_DENOISE), (features, FLAG_FEATURES)):
                if on is not None:
                    q.flags = (q.flags | bit) if on else (q.flags & ~bit)
            params = q
        st = Stats()
        st.struct_size = C.sizeof(Stats)
        self.be.check(self.be._par_cast_device(self.h, C.byref(camera), C.byref(params), d_out_ptr, stream,
                                               C.byref(st) if want_stats else None))
        if block is not None:
            self._block_copy(params.nx, params.ny, d_out_ptr, block, stream, to_device=False)
        if dblock is not None:
            self._block_copy(params.nx, params.ny, d_out_ptr, dblock, stream, to_device=False, offset=d_off, nbytes=C.sizeof(Denoise))
        if fblock is not None:
            self._block_copy(params.nx, params.ny, d_out_ptr, fblock, stream, to_device=False, offset=f_off, nbytes=C.sizeof(Features))
        return st.as_dict() if want_stats else None

    def _block_copy(self, nx, ny, d_out_ptr, block, stream, to_device, offset=None, nbytes=None):
        """Copy a Retire to (or from) the retire block of a device frame on `stream`, and wait for it (`block` is host memory);
        offset / nbytes: another block of the frame (a Denoise) and how much of it."""
        hip = _hip_runtime()
        hs = C.c_void_p(getattr(stream, "cuda_stream", stream) or None)
        dev = C.c_void_p(_device_ptr(d_out_ptr) + (retire_block_offset(nx, ny) if offset is None else offset))
        host = C.c_void_p(C.addressof(block))
        n = C.sizeof(Retire) if nbytes is None else nbytes
        rc = hip.hipMemcpyAsync(*((dev, host, n, 1) if to_device else (host, dev, n, 2)), hs)
        if rc == 0:
            rc = hip.hipStreamSynchronize(hs)
        if rc != 0:
            raise RtError(ERR_DEVICE, "hipMemcpyAsync(%s block) failed: %d" % (type(block).__name__.lower(), rc))

    def _upload_counts(self, nx, ny, squares, counts, d_out_ptr, stream):
        """Copy a uint32 [ny, nx] count array into the count plane of a device frame, on `stream`."""
        hip = _hip_runtime()
        hs = C.c_void_p(getattr(stream, "cuda_stream", stream) or None)
        dst = C.c_void_p(_device_ptr(d_out_ptr) + (2 if squares else 1) * nx * ny * 3 * 4)
        if hasattr(counts, "data_ptr") and getattr(counts, "is_cuda", False):
            if tuple(counts.shape) != (ny, nx) or counts.element_size() != 4 or not counts.is_contiguous():
                raise ValueError("counts= must be a contiguous 4-byte [ny, nx] tensor")
            rc = hip.hipMemcpyAsync(dst, C.c_void_p(counts.data_ptr()), nx * ny * 4, 3, hs)   # 3 = hipMemcpyDeviceToDevice
        else:
            host = np.ascontiguousarray(counts, dtype=np.uint32)
            if host.shape != (ny, nx):
                raise ValueError("counts= must have shape (ny, nx) = %s" % ((ny, nx),))
            rc = hip.hipMemcpyAsync(dst, C.c_void_p(host.ctypes.data), nx * ny * 4, 1, hs)   # 1 = hipMemcpyHostToDevice
            if rc == 0:
                rc = hip.hipStreamSynchronize(hs)   # (the host array may go away when this call returns)
        if rc != 0:
            raise RtError(ERR_DEVICE, "hipMemcpyAsync(count plane) failed: %d" % rc)

    def adaptive(self, camera, nx, ny, ns, step, target_se, min_samples=16, budget_s=None, out=None, seed=0xDEADBEEF,
                 stats=None, radius=0, preview=None, stream=None, denoise=None, denoised=None, features=None, **kw):
        """Adaptive sampling (include/rtiow_gpu.h RTG_FLAG_SAMPLE_COUNTS).  Every slice renders `step` more samples of the
        pixels still active, with RTG_FLAG_SUM_SQUARES + RTG_FLAG_SAMPLE_COUNTS + RTG_FLAG_PARTIAL.  After the slice that ends
        at k samples, an active pixel retires when noise.retire says so (k >= min_samples and its largest per-channel standard
        error <= target_se -- with radius > 0, that of every pixel of its (2 radius + 1)^2 window): its count n_p becomes k and
        it gets no more samples.  Stops when no pixel is active, at ns, or after the first slice that ends past budget_s seconds.
        Host frames (default): yields (counts, preview, stderr) after each slice: counts (uint32 [ny, nx]) the samples every
        pixel holds, preview (float32 [ny, nx, 3]) the frame resolved per pixel -- preview[p] is bit for bit
        par_cast(ns = counts[p])[p] -- and stderr (float64 [ny, nx, 3]) noise.standard_error_counts of every pixel.  out: a
        CountsFrame(nx, ny, squares=True) to hold the running sums and counts (default: a new one).
        Device frames: `out` is a device buffer of retire_frame_bytes(nx, ny) and `preview` one of 4 * nx * ny words (a
        pointer, or an object with data_ptr()), `stream` a hipStream_t (int, an object with .cuda_stream, or None).  The rule
        runs in the library (RTG_FLAG_RETIRE): a slice is one RETIRE call on `out`, a device-to-device copy of plane 0 and the
        count plane into `preview`, the resolve-only counts call on `preview`, and one read-back of the retire block.  Yields
        (k, preview, info), info = Retire.as_dict() of the block (active, retired, estimated, sum_se2, samples_held,
        est_rmse).  The slices, counts and previews are those of the host loop.
        stats: a list to which every slice's rtg_stats (no counters) is appended.  **kw: tiling / max_bounces / t_near.
        denoise= (a Denoise, a dict of k / radius / patch, or True; RTG_FLAG_DENOISE): every slice's call also filters the
        frame, and the loop yields the filtered frame as a fourth item.  Host frames: `out`, when given, is a
        DenoiseFrame(nx, ny, counts=True); the item is a copy of its output plane.  Device frames: `out` holds
        denoise_frame_bytes(nx, ny, counts=True, retire=True) and `denoised` is a device buffer of nx * ny * 3 floats, rewritten
        every slice by a device-to-device copy of the output plane.
        features= (a Features, a dict of grid / sigma_*, or True; RTG_FLAG_FEATURES): the first slice's call also traces the
        feature planes, the later ones pass compute = 0; with denoise= the filter is the guided one.  The loop yields one more
        item at the end of its tuple.  Host frames: `out`, when given, is a FeaturesFrame(nx, ny, counts=True, squares=True,
        denoise=...); the item is that frame (views `albedo`, `normal`, `depth`).  Device frames: `out` holds
        features_frame_bytes(nx, ny, True, True, True, denoise) and the item is the byte offset of the features block in it
        (the planes start 64 bytes behind it)."""
        if step < 1:
            raise ValueError("step must be >= 1")
        _squares_supported(self.be)
        _counts_supported(self.be)
        if not 0 <= radius <= RETIRE_MAX_RADIUS:
            raise ValueError("radius must be in 0 .. %d" % RETIRE_MAX_RADIUS)
        if features is not None and features is not False:
            _features_supported(self.be)
            features = make_features(None if features is True else features)
        else:
            features = None
        if denoise is not None and denoise is not False:
            _denoise_supported(self.be)
            denoise = make_denoise(None if denoise is True else denoise)
        else:
            denoise = None
        if out is not None and not isinstance(out, (CountsFrame, DenoiseFrame, FeaturesFrame)):
            _retire_supported(self.be)
            if preview is None:
                raise ValueError("a device frame needs a device preview buffer (preview=)")
            if denoise is not None and denoised is None:
                raise ValueError("denoise= on a device frame needs a device buffer for the filtered frame (denoised=)")
            yield from self._adaptive_device(camera, nx, ny, ns, step, target_se, min_samples, budget_s, out, seed, stats,
                                             radius, preview, stream, kw, denoise, denoised, features)
            return
        yield from _adaptive_host(lambda n, **k: self.par_cast(camera, nx, ny, n, **k), nx, ny, ns, step, target_se,
                                  min_samples, budget_s, out, seed, stats, radius, denoise, features, kw)

    def _adaptive_device(self, camera, nx, ny, ns, step, target_se, min_samples, budget_s, out, seed, stats, radius, preview,
                         stream, kw, denoise=None, denoised=None, features=None):
        hip = _hip_runtime()
        d_out, d_pv = _device_ptr(out), _device_ptr(preview)
        hs = C.c_void_p(getattr(stream, "cuda_stream", stream) or None)
        plane = nx * ny
        counts_at = d_out + 6 * plane * 4

        def ok(rc, what):
            if rc != 0:
                raise RtError(ERR_DEVICE, "%s failed: %d" % (what, rc))
        # every pixel's target count is ns; the block's in-fields are written once (the library never writes them)
        ok(hip.hipMemsetD32Async(C.c_void_p(counts_at), ns - (1 << 32) if ns >= 1 << 31 else ns, plane, hs), "hipMemsetD32Async(counts)")
        block = Retire()
        block.target_se, block.min_samples, block.radius = float(target_se), int(min_samples), int(radius)
        self._block_copy(nx, ny, d_out, block, stream, to_device=True)
        if denoise is not None:   # (likewise: its in-fields once; the output plane sits 64 bytes behind the block)
            d_off = denoise_block_offset(nx, ny, True, True)
            self._block_copy(nx, ny, d_out, denoise, stream, to_device=True, offset=d_off, nbytes=Denoise.OUT_OFFSET)
        more = ()
        if features is not None:   # (its in-fields before the first slice, and once more, with compute = 0, behind it)
            f_off = features_block_offset(nx, ny, True, True, True, denoise is not None)
            self._block_copy(nx, ny, d_out, features, stream, to_device=True, offset=f_off, nbytes=Features.OUT_OFFSET)
            more = (f_off,)
        t0 = time.perf_counter()
        done = 0
        while done < ns:
            end = min(ns, done + step)
            st = self.par_cast_device(camera, make_params(nx, ny, end, seed=seed, sample_begin=done, resume=True, partial=True,
                                                          squares=True, counts=True, retire=True, denoise=denoise is not None,
                                                          features=features is not None, **kw), d_out, hs,
                                      want_stats=stats is not None)
            if features is not None and features.compute:
                features.compute = 0
                self._block_copy(nx, ny, d_out, features, stream, to_device=True, offset=f_off, nbytes=Features.OUT_OFFSET)
            if denoise is not None:
                ok(hip.hipMemcpyAsync(C.c_void_p(_device_ptr(denoised)), C.c_void_p(d_out + d_off + C.sizeof(Denoise)), plane * 3 * 4,
                                      3, hs), "hipMemcpyAsync(denoised)")
            if stats is not None:
                stats.append(st)
            done = end
            # the preview: plane 0 and the count plane, resolved per pixel (e_p = min(n_p, k): the samples each pixel holds)
            ok(hip.hipMemcpyAsync(C.c_void_p(d_pv), C.c_void_p(d_out), plane * 3 * 4, 3, hs), "hipMemcpyAsync(preview)")
            ok(hip.hipMemcpyAsync(C.c_void_p(d_pv + plane * 3 * 4), C.c_void_p(counts_at), plane * 4, 3, hs), "hipMemcpyAsync(preview counts)")
            self.par_cast_device(camera, make_params(nx, ny, done, seed=seed, sample_begin=done, resume=True, counts=True, **kw),
                                 d_pv, hs)
            self._block_copy(nx, ny, d_out, block, stream, to_device=False)
            info = block.as_dict()
            if denoise is not None:
                yield (done, preview, info, denoised) + more
            else:
                yield (done, preview, info) + more
            if info["active"] == 0:
                return
            if budget_s is not None and time.perf_counter() - t0 >= budget_s:
                return

    def progressive(self, camera, nx, ny, ns, step, seed=0xDEADBEEF, budget_s=None, out=None, preview=None, stream=None,
                    squares=False, target_rmse=None, denoise=None, denoised=None, features=None, **kw):
        """Render a frame `step` samples at a time (include/rtiow_gpu.h progressive rendering).  Yields (n_done, preview)
        after each slice: the preview is bit-identical to par_cast(ns = n_done), and the one at n_done == ns is the final
        image, bit-identical to par_cast(ns).  Stops at ns, or after the first slice that ends past `budget_s` seconds.
        Host frames (default): the running sum lives in `out`, a float32 [ny, nx, 3] array (default: zeros); every preview
        is a new array.  Device frames: `out` and `preview` are device buffers of nx * ny * 3 floats on the scene's device
        (a pointer, or an object with data_ptr() such as a torch tensor) and `stream` a hipStream_t (int, an object with
        .cuda_stream, or None = the default stream): the same loop over par_cast_device, every slice, copy and resolve
        enqueued on that stream; `preview` is rewritten by each slice.
        squares=True (RTG_FLAG_SUM_SQUARES): the running sums have two planes -- `out` is [2, ny, nx, 3] on the host, 2 * nx * ny
        * 3 floats on the device -- and the loop yields (n_done, preview, stderr).  On the host, stderr is
        noise.standard_error of every pixel and channel (float64 [ny, nx, 3]); on the device it is `out` itself, the two
        planes the estimate is computed from (no device-side reduction).
        target_rmse (host frames; implies squares): stop after the first slice whose noise.estimated_rmse is <= target_rmse
        -- or at ns, or at budget_s, whichever comes first.  **kw: tiling / max_bounces / t_near.
        denoise= (a Denoise, a dict of k / radius / patch, or True; RTG_FLAG_DENOISE; implies squares): every slice's call also
        filters the frame (denoise.nlm of the running sums), and the loop yields (n_done, preview, stderr, denoised).  Host
        frames: denoised is a new float32 [ny, nx, 3] array per slice.  Device frames: `out` holds denoise_frame_bytes(nx, ny)
        and `denoised` is a device buffer of nx * ny * 3 floats, rewritten every slice by a device-to-device copy of the
        output plane, and yielded as the fourth item.
        features= (a Features, a dict of grid / sigma_*, or True; RTG_FLAG_FEATURES): the first slice's call also traces the
        feature planes, the later ones pass compute = 0; with denoise= the filter is the guided one (denoise.nlm_guided).  The
        loop yields one more item at the end of its tuple.  Host frames: the FeaturesFrame the slices render into (views
        `albedo`, `normal`, `depth`).  Device frames: `out` holds features_frame_bytes(nx, ny, squares, False, False, denoise)
        and the item is the byte offset of the features block in it (the planes start 64 bytes behind it)."""
        if step < 1:
            raise ValueError("step must be >= 1")
        if features is not None and features is not False:
            _features_supported(self.be)
            features = make_features(None if features is True else features)
        else:
            features = None
        if denoise is not None and denoise is not False:
            _squares_supported(self.be)
            _denoise_supported(self.be)
            denoise = make_denoise(None if denoise is True else denoise)
        else:
            denoise = None
        squares = bool(squares) or target_rmse is not None or denoise is not None
        if squares:
            _squares_supported(self.be)
        if out is not None and not isinstance(out, np.ndarray):
            if target_rmse is not None:
                raise ValueError("target_rmse needs host frames: there is no device-side error reduction")
            if preview is None:
                raise ValueError("a device running sum needs a device preview buffer (preview=)")
            if denoise is not None and denoised is None:
                raise ValueError("denoise= on a device frame needs a device buffer for the filtered frame (denoised=)")
            yield from self._progressive_device(camera, nx, ny, ns, step, seed, budget_s, out, preview, stream, squares, kw,
                                                denoise, denoised, features)
            return
        shape = (2, ny, nx, 3) if squares else (ny, nx, 3)
        acc = np.zeros(shape, dtype=np.float32) if out is None else out
        frame = None
        if features is not None:   # the slices render into a FeaturesFrame; a caller's `out` is kept up to date beside it
            frame = FeaturesFrame(nx, ny, squares, denoise=denoise, features=features)
            frame.planes[...] = acc
        elif denoise is not None:   # ... or into a DenoiseFrame
            frame = DenoiseFrame(nx, ny, denoise=denoise)
            frame.planes[...] = acc
        more = () if features is None else (frame,)
        sums = acc[0] if squares else acc
        t0 = time.perf_counter()
        done = 0
        while done < ns:
            end = min(ns, done + step)
            if features is not None:
                self.par_cast(camera, nx, ny, end, seed=seed, out=frame, denoise=True if denoise is not None else None, features=True,
                              sample_begin=done, resume=True, partial=True, squares=squares, **kw)
                frame.features.compute = 0   # (the planes are traced once)
                acc[...] = frame.planes
            elif frame is not None:
                self.par_cast(camera, nx, ny, end, seed=seed, out=frame, denoise=True, sample_begin=done, resume=True, partial=True,
                              squares=True, **kw)
                acc[...] = frame.planes
            else:
                self.par_cast(camera, nx, ny, end, seed=seed, out=acc, sample_begin=done, resume=True, partial=True, squares=squares, **kw)
            done = end
            pv = sums.copy()   # resolve a copy: the running sum goes on
            self.par_cast(camera, nx, ny, done, seed=seed, out=pv, sample_begin=done, resume=True, **kw)
            if squares:
                se = noise.standard_error(acc[0], acc[1], done)
                if denoise is not None:
                    yield (done, pv, se, frame.denoised.copy()) + more
                else:
                    yield (done, pv, se) + more
                if target_rmse is not None and float(np.sqrt(np.mean(se * se))) <= target_rmse:
                    return
            else:
                yield (done, pv) + more
            if budget_s is not None and time.perf_counter() - t0 >= budget_s:
                return

    def _progressive_device(self, camera, nx, ny, ns, step, seed, budget_s, acc, preview, stream, squares, kw, denoise=None,
                            denoised=None, features=None):
        hip = _hip_runtime()
        d_acc, d_preview = C.c_void_p(_device_ptr(acc)), C.c_void_p(_device_ptr(preview))
        hs = C.c_void_p(getattr(stream, "cuda_stream", stream) or None)
        if denoise is not None:   # the block's in-fields are written once (the library never writes them)
            d_off = denoise_block_offset(nx, ny)
            self._block_copy(nx, ny, acc, denoise, stream, to_device=True, offset=d_off, nbytes=Denoise.OUT_OFFSET)
        more = ()
        if features is not None:   # (its in-fields before the first slice, and once more, with compute = 0, behind it)
            f_off = features_block_offset(nx, ny, squares, False, False, denoise is not None)
            self._block_copy(nx, ny, acc, features, stream, to_device=True, offset=f_off, nbytes=Features.OUT_OFFSET)
            more = (f_off,)
        t0 = time.perf_counter()
        done = 0
        while done < ns:
            end = min(ns, done + step)
            self.par_cast_device(camera, make_params(nx, ny, end, seed=seed, sample_begin=done, resume=True, partial=True,
                                                     squares=squares, denoise=denoise is not None, features=features is not None,
                                                     **kw), d_acc, hs)
            if features is not None and features.compute:
                features.compute = 0
                self._block_copy(nx, ny, acc, features, stream, to_device=True, offset=f_off, nbytes=Features.OUT_OFFSET)
            done = end
            if denoise is not None:
                rc = hip.hipMemcpyAsync(C.c_void_p(_device_ptr(denoised)), C.c_void_p(d_acc.value + d_off + C.sizeof(Denoise)),
                                        nx * ny * 3 * 4, 3, hs)
                if rc != 0:
                    raise RtError(ERR_DEVICE, "hipMemcpyAsync(denoised) failed: %d" % rc)
            rc = hip.hipMemcpyAsync(d_preview, d_acc, nx * ny * 3 * 4, 3, hs)   # plane 0; 3 = hipMemcpyDeviceToDevice
            if rc != 0:
                raise RtError(ERR_DEVICE, "hipMemcpyAsync(preview) failed: %d" % rc)
            self.par_cast_device(camera, make_params(nx, ny, done, seed=seed, sample_begin=done, resume=True, **kw), d_preview, hs)
            if denoise is not None:
                yield (done, preview, acc, denoised) + more
            else:
                yield ((done, preview, acc) if squares else (done, preview)) + more
            if budget_s is not None:
                if hip.hipStreamSynchronize(hs) != 0:
                    raise RtError(ERR_DEVICE, "hipStreamSynchronize failed")
                if time.perf_counter() - t0 >= budget_s:
                    return

    def debug_hit_top(self, rays, seed=1, t_near=0.001):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
        n = rays.shape[0]
        out = np.zeros((n, 8), dtype=np.float32)
        mat = np.zeros(n, dtype=np.uint32)
        self.be.check(self.be._debug_hit_top(self.h, n, rays.ctypes.data_as(c_f32p), seed, t_near,
                                             out.ctypes.data_as(c_f32p), mat.ctypes.data_as(c_u32p)))
        return out, mat

    def debug_samples(self, camera, nx, ny, ns, xs, ys, samples, seed=0xDEADBEEF, trace_kernel=False, **kw):
        """trace_kernel=True: read the keys out of the production ray-pool kernel's per-sample trace (whole frame rendered)."""
        p = make_params(nx, ny, ns, seed=seed, flags=FLAG_TRACE_KERNEL if trace_kernel else 0, **kw)
        xs, ys, samples = (np.ascontiguousarray(a, dtype=np.uint32) for a in (xs, ys, samples))
        n = xs.size
        rgb = np.zeros((n, 3), dtype=np.float32)
        info = np.zeros((n, 4), dtype=np.uint32)
        self.be.check(self.be._debug_samples(self.h, C.byref(camera), C.byref(p), n,
                                             xs.ctypes.data_as(c_u32p), ys.ctypes.data_as(c_u32p),
                                             samples.ctypes.data_as(c_u32p), rgb.ctypes.data_as(c_f32p),
                                             info.ctypes.data_as(c_u32p)))
        return rgb, info


Backend.scene_class = Scene
