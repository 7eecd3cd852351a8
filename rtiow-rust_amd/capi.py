"""ctypes binding of the C ABI declared in include/rtiow_gpu.h (librtiow_gpu.so, prefix ``rtg_``).

Method names mirror the reference crate's constructors (object.rs / material.rs / texture.rs /
camera.rs / lib.rs) so scene code reads like the reference's `src/main.rs`.  The symbol prefix is a
parameter so that a test harness can drive another library exporting the same entry points with the
same calls.
"""
import ctypes as C
import math
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
FLAG_DENOISE_ERROR = 512  # (needs FLAG_DENOISE) the framebuffer ends with the error plane: the variance of every filtered pixel
FEATURES_MAX_GRID = 4
FLAG_BACKGROUND = 1024    # the framebuffer ends with a Background block: what a ray that leaves the scene sees


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


class QueryParams(C.Structure):
    """include/rtiow_gpu_query.h rtg_query_params (32 bytes)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64), ("first_index", C.c_uint64),
                ("t_min", C.c_float), ("reserved2", C.c_uint32)]


def make_query_params(seed=1, t_min=0.001, first_index=0):
    return QueryParams(struct_size=C.sizeof(QueryParams), seed=seed, first_index=first_index, t_min=t_min)


class Retire(C.Structure):
    """include/rtiow_gpu.h rtg_retire: the block behind the count plane of an RTG_FLAG_RETIRE frame (64 bytes).  The caller
    sets target_se / min_samples / radius; every accepted call writes the out-fields active .. samples_held."""
    _fields_ = [("target_se", C.c_double), ("min_samples", C.c_uint32), ("radius", C.c_uint32),
                ("active", C.c_uint32), ("retired", C.c_uint32), ("estimated", C.c_uint32), ("reserved", C.c_uint32),
                ("sum_se2", C.c_double), ("samples_held", C.c_uint64), ("reserved2", C.c_uint64 * 2)]
    OUT_FIELDS = ("active", "retired", "estimated", "reserved", "sum_se2", "samples_held")
    OUT_OFFSET = 16   # bytes: the in-fields end here

    def as_dict(self):
        """The out-fields, plus est_rmse = sqrt(sum_se2 / (3 estimated)) (inf when no pixel has an estimate)."""
        d = {k: getattr(self, k) for k in self.OUT_FIELDS}
        d["est_rmse"] = float(np.sqrt(self.sum_se2 / (3 * self.estimated))) if self.estimated else float("inf")
        return d


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


class Background(C.Structure):
    """include/rtiow_gpu.h rtg_background: the block at the very end of an RTG_FLAG_BACKGROUND frame (64 bytes).  The caller sets
    mode (0 = constant `bottom`, 1 = gradient from `bottom` to `top` along world +y) and the colours; the library never writes
    the block."""
    _fields_ = [("mode", C.c_uint32), ("reserved_in", C.c_uint32), ("bottom", C.c_float * 3), ("top", C.c_float * 3),
                ("reserved", C.c_uint32 * 8)]
    OUT_FIELDS = ()
    OUT_OFFSET = 32   # bytes: the in-fields end here

    def as_dict(self):
        """The in-fields (the block has no out-fields)."""
        return {"mode": self.mode, "bottom": tuple(self.bottom), "top": tuple(self.top)}


def make_background(background):
    """A Background with the in-fields set: from a Background (copied), a colour (r, g, b) -- the constant background -- or a
    dict of bottom / top (/ mode): with `top` the gradient from bottom to top along world +y (background.sky), without it the
    constant background `bottom`."""
    g = Background()
    if isinstance(background, Background):
        C.memmove(C.addressof(g), C.addressof(background), C.sizeof(Background))
        return g
    if isinstance(background, dict):
        unknown = set(background) - {"bottom", "top", "mode"}
        if unknown or "bottom" not in background:
            raise ValueError("background=: a dict of bottom / top / mode, with bottom (unknown: %s)" % sorted(unknown))
        top = background.get("top")
        g.mode = int(background.get("mode", 0 if top is None else 1))
        if g.mode == 1 and top is None:
            raise ValueError("background=: mode 1 (the gradient) needs top")
        g.bottom = _f3(background["bottom"])
        g.top = _f3(top if top is not None else (0.0, 0.0, 0.0))
        return g
    if background is None or isinstance(background, bool) or len(background) != 3:
        raise ValueError("background= must be a colour (r, g, b), a dict of bottom / top, or a Background")
    g.bottom = _f3(background)
    return g


def _given(x):
    """An optional part of a call or of a frame was asked for: anything but None and False."""
    return x is not None and x is not False


class FrameLayout:
    """Where every part of a framebuffer starts, in 4-byte words: the one rule of include/rtiow_gpu.h, field for field the
    library's own struct FrameLayout (csrc/rt_multi_planes.h, host part).  The float planes (one, or two with
    squares) start at word 0; behind them, each only with its flag: the count plane (`counts`, n = nx * ny words), the Retire
    block (`retire`), the Denoise block (`denoise`) and its output plane (`denoised`, 3n), the Features block (`features`) and
    the `albedo` (3n), `normal` (3n) and `depth` (n) planes, and at the very end, on an even word, the `error` plane (3n;
    RTG_FLAG_DENOISE_ERROR, needs denoise) and, behind everything else, the Background block (`background`;
    RTG_FLAG_BACKGROUND).  A block is 16 words and starts on an even word.  retire implies
    counts and squares, denoise implies squares (the library refuses a call without them).  The offset of a part the frame
    does not have is None; `words` is the frame's length.  Plain Python integers: exact for frames beyond 2^31 bytes."""

    def __init__(self, nx, ny, squares=False, counts=False, retire=False, denoise=False, features=False, error=False,
                 background=False):
        if error and not denoise:
            raise ValueError("error=True needs denoise= (the filter writes the error plane)")
        n = self.n = nx * ny
        self.nx, self.ny, self.squares = nx, ny, bool(squares or retire or denoise)
        self.counts = self.retire = self.denoise = self.denoised = self.features = self.albedo = self.normal = self.depth = None
        self.error = self.background = None
        w = (6 if self.squares else 3) * n
        if counts or retire:
            self.counts, w = w, w + n
        if retire:
            self.retire = (w + 1) & ~1
            w = self.retire + 16
        if denoise:
            self.denoise = (w + 1) & ~1
            self.denoised = self.denoise + 16
            w = self.denoised + 3 * n
        if features:
            self.features = (w + 1) & ~1
            self.albedo = self.features + 16
            self.normal, self.depth = self.albedo + 3 * n, self.albedo + 6 * n
            w = self.depth + n
        if error:
            self.error = (w + 1) & ~1
            w = self.error + 3 * n
        if background:
            self.background = (w + 1) & ~1
            w = self.background + 16
        self.words = w


def retire_block_offset(nx, ny):
    """Byte offset of the Retire block in an RTG_FLAG_RETIRE frame (two float planes and the count plane in front of it)."""
    return FrameLayout(nx, ny, retire=True).retire * 4


def retire_frame_bytes(nx, ny):
    """Bytes of an RTG_FLAG_RETIRE frame: it ends with the 64-byte Retire block."""
    return FrameLayout(nx, ny, retire=True).words * 4


def denoise_block_offset(nx, ny, counts=False, retire=False):
    """Byte offset of the Denoise block in an RTG_FLAG_DENOISE frame, behind what counts / retire put in it."""
    return FrameLayout(nx, ny, True, counts, retire, True).denoise * 4


def denoise_frame_bytes(nx, ny, counts=False, retire=False, error=False):
    """Bytes of an RTG_FLAG_DENOISE frame: it ends with the 64-byte Denoise block and the output plane (error=True: and the
    error plane)."""
    return FrameLayout(nx, ny, True, counts, retire, True, error=error).words * 4


def features_block_offset(nx, ny, squares=False, counts=False, retire=False, denoise=False):
    """Byte offset of the Features block in an RTG_FLAG_FEATURES frame, behind everything the call's other flags put in it."""
    return FrameLayout(nx, ny, squares, counts, retire, denoise, True).features * 4


def features_frame_bytes(nx, ny, squares=False, counts=False, retire=False, denoise=False, error=False):
    """Bytes of an RTG_FLAG_FEATURES frame: it ends with the 64-byte Features block and the albedo, normal and depth planes
    (error=True: and the error plane)."""
    return FrameLayout(nx, ny, squares, counts, retire, denoise, True, error).words * 4


class Stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kernel_ms", C.c_float), ("samples", C.c_uint64),
                ("aabb_tests", C.c_uint64), ("prim_tests", C.c_uint64), ("shaded_hits", C.c_uint64),
                ("rays", C.c_uint64), ("draws", C.c_uint64)]

    @classmethod
    def new(cls):
        """A zeroed Stats that states its size, as every call expects it."""
        return cls(struct_size=C.sizeof(cls))

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


def make_params(nx, ny, ns, seed=0xDEADBEEF, max_bounces=50, t_near=0.001, tile_w=0, tile_h=0, rank=0,
                nranks=1, flags=0, sample_begin=0, partial=False, resume=False, squares=False, counts=False, retire=False,
                denoise=False, features=False, error=False, background=False):
    """`background`: RTG_FLAG_BACKGROUND, the background block at the framebuffer's very end.
    `error`: RTG_FLAG_DENOISE_ERROR, the error plane at the framebuffer's very end (needs denoise).
    `features`: RTG_FLAG_FEATURES, the features block and the albedo / normal / depth planes at the framebuffer's end.
    `partial` / `resume` / `sample_begin`: one slice of a progressive frame (include/rtiow_gpu.h RTG_FLAG_PARTIAL /
    RTG_FLAG_RESUME); `squares`: RTG_FLAG_SUM_SQUARES, the framebuffer's second plane; `counts`: RTG_FLAG_SAMPLE_COUNTS,
    the count plane at the framebuffer's end; `retire`: RTG_FLAG_RETIRE, the retire block behind it; `denoise`:
    RTG_FLAG_DENOISE, the denoise block and the output plane at the framebuffer's end."""
    flags |= (FLAG_DENOISE if denoise else 0) | (FLAG_FEATURES if features else 0) | (FLAG_DENOISE_ERROR if error else 0)
    flags |= (FLAG_PARTIAL if partial else 0) | (FLAG_RESUME if resume else 0) | (FLAG_SUM_SQUARES if squares else 0)
    flags |= (FLAG_SAMPLE_COUNTS if counts else 0) | (FLAG_RETIRE if retire else 0) | (FLAG_BACKGROUND if background else 0)
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


def _stream(stream):
    """The hipStream_t of `stream`: an int, an object with .cuda_stream, or None (the default stream)."""
    return C.c_void_p(getattr(stream, "cuda_stream", stream) or None)


class _no_context:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _hip_ok(rc, what):
    if rc != 0:
        raise RtError(ERR_DEVICE, "%s failed: %d" % (what, rc))


def _resumes(kw):
    return bool(kw.get("resume")) and kw.get("sample_begin", 0) > 0


_FLAG_OF = {"squares": ("squares=True", "SUM_SQUARES"), "counts": ("counts=", "SAMPLE_COUNTS"), "retire": ("retire=", "RETIRE"),
            "denoise": ("denoise=", "DENOISE"), "features": ("features=", "FEATURES"), "error": ("error=True", "DENOISE_ERROR"),
            "background": ("background=", "BACKGROUND")}


def _supported(be, part):
    """The flag of `part` (a make_params keyword) is the HIP library's (prefix rtg_): a library that exports the same entry
    points under another prefix ignores flags it does not know -- it would write one plane where the caller expects two,
    render every pixel to ns, write no block and no plane."""
    if be.prefix != "rtg_":
        raise ValueError("%s: %s (prefix %s) does not implement RTG_FLAG_%s" % (_FLAG_OF[part][0], be.path, be.prefix, _FLAG_OF[part][1]))


class Frame:
    """One contiguous, zeroed host framebuffer `buf`, laid out by FrameLayout (`layout`), and a view of every part: `planes`
    ([ny, nx, 3], or [2, ny, nx, 3] with squares), `counts` (uint32 [ny, nx]), `retire`, `denoise`, `features` (the blocks),
    `denoised`, `albedo`, `normal`, `error` (float32 [ny, nx, 3]) and `depth` (float32 [ny, nx]) -- None when the frame has no
    such part.  denoise / features: a block, a dict or True (make_denoise / make_features), whose in-fields the block gets.
    error=True (needs denoise): the error plane of RTG_FLAG_DENOISE_ERROR at the frame's end.
    background= (a colour, a dict of bottom / top, or a Background: make_background): the `background` block of
    RTG_FLAG_BACKGROUND behind everything else."""

    def __init__(self, nx, ny, squares=False, counts=False, retire=False, denoise=None, features=None, error=False, background=None):
        lay = self.layout = FrameLayout(nx, ny, squares, counts, retire, _given(denoise), _given(features), bool(error), _given(background))
        self.nx, self.ny, self.squares = nx, ny, lay.squares
        self.buf = np.zeros(lay.words, dtype=np.float32)

        def plane(at, *shape):
            return None if at is None else self.buf[at:at + math.prod(shape)].reshape(shape)

        def block(cls, at):
            return None if at is None else cls.from_buffer(self.buf, at * 4)
        self.planes = plane(0, *((2, ny, nx, 3) if lay.squares else (ny, nx, 3)))
        self.counts = None if lay.counts is None else plane(lay.counts, ny, nx).view(np.uint32)
        self.denoised, self.albedo, self.normal = (plane(at, ny, nx, 3) for at in (lay.denoised, lay.albedo, lay.normal))
        self.depth = plane(lay.depth, ny, nx)
        self.error = plane(lay.error, ny, nx, 3)
        self.retire, self.denoise, self.features = block(Retire, lay.retire), block(Denoise, lay.denoise), block(Features, lay.features)
        self.background = block(Background, lay.background)
        if self.background is not None and background is not True:
            self.set_in(make_background(background))
        if self.denoise is not None:
            self.set_in(make_denoise(denoise))
        if self.features is not None:
            self.set_in(make_features(features))

    def flags(self):
        """make_params keywords of the parts the frame has ("error" / "background" only when the frame has that part)."""
        on = {"squares": self.squares, "counts": self.counts is not None, "retire": self.retire is not None,
              "denoise": self.denoise is not None, "features": self.features is not None}
        if self.error is not None:
            on["error"] = True
        if self.background is not None:
            on["background"] = True
        return on

    def set_in(self, block):
        """Write the in-fields of `block` (a Retire, Denoise, Features or Background) to the frame's block of that class; the out-fields,
        which only the library writes, stay."""
        C.memmove(C.addressof(getattr(self, type(block).__name__.lower())), C.addressof(block), block.OUT_OFFSET)

    def copy_in(self, out=None, counts=None, retire=None):
        """The caller's float planes, count plane and Retire (all of it) into the frame."""
        if out is not None:
            self.planes[...] = out
        if counts is not None:
            self.counts[...] = counts
        if retire is not None:
            C.memmove(C.addressof(self.retire), C.addressof(retire), C.sizeof(Retire))

    def copy_back(self, out=None, counts=None, retire=None):
        """The frame's float planes, count plane and Retire block back to the caller's."""
        if out is not None:
            out[...] = self.planes
        if counts is not None:
            counts[...] = self.counts
        if retire is not None:
            C.memmove(C.addressof(retire), C.addressof(self.retire), C.sizeof(Retire))


class CountsFrame(Frame):
    """The frame of RTG_FLAG_SAMPLE_COUNTS: the float planes and the count plane; retire=True (needs squares): and the
    RTG_FLAG_RETIRE block.  par_cast(out=frame.planes, counts=frame.counts[, retire=frame.retire]) renders in place, without
    copies, as par_cast(out=frame) does."""

    def __init__(self, nx, ny, squares=False, retire=False, background=None):
        if retire and not squares:
            raise ValueError("a retire frame has two float planes: squares=True")
        super().__init__(nx, ny, squares, True, retire, background=background)


class DenoiseFrame(Frame):
    """The frame of RTG_FLAG_DENOISE, a sibling of CountsFrame: always two float planes, the count plane with counts=True, the
    Retire block with retire=True (implies counts), then the Denoise block and the output plane.  par_cast(out=frame,
    denoise=...) renders in place."""

    def __init__(self, nx, ny, counts=False, retire=False, denoise=None, error=False, background=None):
        super().__init__(nx, ny, True, counts, retire, denoise if _given(denoise) else True, None, error, background)


class FeaturesFrame(Frame):
    """The frame of RTG_FLAG_FEATURES: what its siblings hold -- the count plane with counts=True, the Retire block with
    retire=True (implies counts and squares), the Denoise block and its output plane with denoise= (a Denoise, a dict or
    True; implies squares) -- then the Features block and the albedo, normal and depth planes.  par_cast(out=frame,
    features=True) renders in place."""

    def __init__(self, nx, ny, squares=False, counts=False, retire=False, denoise=None, features=None, error=False, background=None):
        super().__init__(nx, ny, squares, counts, retire, denoise, features if _given(features) else True, error, background)


def features_frame(nx, ny, squares=False, counts=False, retire=False, denoise=None, features=None, error=False):
    """A zeroed FeaturesFrame whose blocks hold the in-fields of `features` (make_features) and `denoise` (make_denoise);
    error=True: with the error plane."""
    return FeaturesFrame(nx, ny, squares, counts, retire, denoise, features, error)


def denoise_frame(nx, ny, counts=False, retire=False, denoise=None, error=False):
    """A zeroed DenoiseFrame whose block holds the in-fields of `denoise` (make_denoise: the defaults when None); error=True:
    with the error plane."""
    return DenoiseFrame(nx, ny, counts, retire, denoise, error)


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
    f.copy_in(out, counts, retire)
    return f.planes, f


def _host_frame(out, nx, ny, squares, kw):
    """The host framebuffer of a par_cast call: `out`, checked, or a new zeroed one -- [ny, nx, 3] float32, or [2, ny, nx, 3]
    with squares (the library writes both planes: a smaller array would be overrun)."""
    shape = (2, ny, nx, 3) if squares else (ny, nx, 3)
    if out is None:
        if _resumes(kw):
            raise ValueError("resume=True needs out= (the running sum to continue)")
        return np.zeros(shape, dtype=np.float32)
    if squares and not (isinstance(out, np.ndarray) and out.shape == shape and out.dtype == np.float32 and out.flags.c_contiguous):
        raise ValueError("squares=True needs out= a C-contiguous float32 array of shape %s" % (shape,))
    return out


def _render(supported, call, nx, ny, ns, seed, stats, out, counters, counts, retire, denoise, features, kw, exact, forward=False):
    """The one path of Scene.par_cast and Backend.par_cast_multi into the library: `supported(part)` is _supported on the
    backend of either, `call(params, buffer)` makes the library call and returns its Stats; `counters`: whether a stats=True call asks for the instrumented counters.  The frame is
    `out` itself (a Frame: rendered in place, its flags those of the parts it has), a staging frame that carries copies of
    the caller's out / counts / retire and gives them back, or a plain array.  Every check is made before anything of the
    caller's is written.
    exact (Scene.par_cast): beside a Frame, squares= / denoise= / features= must say what the frame holds, and it brings its
    own counts and retire.  Otherwise (par_cast_multi) they may say less, and retire= a Retire sets the block's in-fields.
    forward (par_cast_multi): plain flags beside a plain array (counts=True, ...) go to the library as they are.
    kw["background"] (RTG_FLAG_BACKGROUND): a colour, a dict of bottom / top or a Background (make_background), written to the
    frame's block; True beside a Frame that has the block: the block as it stands.  Beside an array the call goes through a
    staging frame and still returns the array."""
    kw = dict(kw)
    squares = kw.pop("squares", None)
    error = kw.pop("error", None)   # (RTG_FLAG_DENOISE_ERROR: True, or None / False)
    background = kw.pop("background", None)
    has_rt, has_dn, has_ft, has_er = _given(retire), _given(denoise), _given(features), _given(error)
    has_bg = _given(background)
    in_place = isinstance(out, Frame)
    f = None
    plain = forward and not (in_place or isinstance(counts, np.ndarray) or isinstance(retire, Retire) or has_bg
                             or isinstance(denoise, (dict, Denoise)) or isinstance(features, (dict, Features)))
    if plain:   # (the library's to answer)
        flags, parts = {"squares": squares, "counts": counts, "retire": retire, "denoise": denoise, "features": features}, ()
        if has_er:
            flags["error"], parts = True, ("error",)
    else:
        if has_er and not (has_dn or (in_place and out.denoise is not None)):
            raise ValueError("error=True needs denoise= (the filter writes the error plane)")
        if has_dn and not squares and (exact or not in_place):
            raise ValueError("denoise= needs squares=True (the filter reads both planes)")
        blocks = [make(x) for x, make in ((denoise, make_denoise), (features, make_features), (background, make_background))
                  if _given(x) and x is not True]
        if in_place:
            f, name = out, type(out).__name__
            if (f.nx, f.ny) != (nx, ny):
                raise ValueError("out= is a %s of another size" % name)
            if isinstance(counts, np.ndarray) or (exact and (counts is not None or retire is not None)):
                raise ValueError("out= a %s brings its own counts / retire views" % name)
            if has_ft and f.features is None:
                raise ValueError("features=: out= must be a FeaturesFrame or an array")
            if (has_dn and f.denoise is None) or (has_rt and f.retire is None):
                raise ValueError("out= a %s has no such block" % name)
            if ((squares is not None or exact) and bool(squares) != f.squares) or (
                    exact and (has_dn != (f.denoise is not None) or has_ft != (f.features is not None))):
                raise ValueError("out= a %s: squares= / denoise= / features= must say what the frame holds" % name)
            if (has_er and f.error is None) or (exact and not has_er and f.error is not None):
                raise ValueError("out= a %s: error= must say whether the frame has an error plane" % name)
            if has_bg and f.background is None:
                raise ValueError("background=: out= a %s has no background block (make the frame with background=)" % name)
            if isinstance(retire, Retire):
                blocks.append(retire)
            flags = f.flags()
        else:
            if has_rt and not (isinstance(retire, Retire) and isinstance(counts, np.ndarray) and squares):
                raise ValueError("retire= needs a Retire, squares=True and counts= a uint32 array (the call writes it)")
            if counts is not None and np.asarray(counts).shape != (ny, nx):
                raise ValueError("counts= must have shape (ny, nx) = %s" % ((ny, nx),))
            if out is None and _resumes(kw):
                raise ValueError("resume=True needs out= (the running sum to continue)")
            flags = {"squares": bool(squares), "counts": counts is not None, "retire": has_rt, "denoise": has_dn, "features": has_ft}
            if has_er:
                flags["error"] = True
            if has_bg:
                if background is True:
                    raise ValueError("background=True needs out= a frame that has the block")
                flags["background"] = True
        parts = sorted((part for part, on in flags.items() if on), key=lambda part: part != "error")   # (the newest flag first)
    for part in parts:
        supported(part)
    if in_place:
        for block in blocks:
            f.set_in(block)
        ret, buf = f, f.buf
    elif (has_dn or has_ft or has_bg) and not plain:
        bg = background if has_bg else None
        f = (FeaturesFrame(nx, ny, squares, counts is not None, has_rt, denoise if has_dn else None, features, has_er, bg) if has_ft else
             DenoiseFrame(nx, ny, counts is not None, has_rt, denoise, has_er, bg) if has_dn else
             Frame(nx, ny, squares, counts is not None, has_rt, background=bg))
        if not (has_dn or has_ft):   # (a background alone changes no plane: the caller gets the array)
            out = _host_frame(out, nx, ny, squares, kw)
        f.copy_in(None if out is None else _host_frame(out, nx, ny, squares, kw), counts, retire if has_rt else None)
        ret, buf = f if has_dn or has_ft else out, f.buf
    else:
        ret = out = buf = _host_frame(out, nx, ny, squares, kw)
        if counts is not None and not plain:   # in place when `out` and `counts` are one CountsFrame's views
            buf, f = _counts_call(out, counts, nx, ny, squares, retire if has_rt else None)
    p = make_params(nx, ny, ns, seed=seed, flags=FLAG_COUNTERS if stats and counters else 0, **flags, **kw)
    st = call(p, buf)
    if f is not None and not in_place:   # (with retire the library wrote the count plane and the block's out-fields)
        f.copy_back(out, counts if has_rt else None, retire if has_rt else None)
    return (ret, st.as_dict()) if stats else ret


def _adaptive_host(cast, nx, ny, ns, step, target_se, min_samples, budget_s, out, seed, stats, radius, denoise, features, kw,
                   error=False, background=None):
    """The host-frame loop of Scene.adaptive and Backend.adaptive_multi: `cast(ns, **keywords)` is the par_cast of either
    (camera and frame size bound); denoise / features: a checked Denoise / Features, or None; error: the frame has the error
    plane of RTG_FLAG_DENOISE_ERROR and the rule is noise.retire_filtered on it; background: a checked Background (the frame
    ends with the block of RTG_FLAG_BACKGROUND and every slice renders with it), or None."""
    if features is not None:
        f = FeaturesFrame(nx, ny, True, True, False, denoise, None, error, background) if out is None else out
        what = "features=: out= must be a FeaturesFrame(nx, ny, squares=True, counts=True, denoise=...)"
    elif denoise is not None:
        f = DenoiseFrame(nx, ny, True, error=error, background=background) if out is None else out
        what = "denoise=: out= must be a DenoiseFrame(nx, ny, counts=True)"
    else:
        f = CountsFrame(nx, ny, True, background=background) if out is None else out
        what = "out= must be a CountsFrame(nx, ny, squares=True)"
    on = {"denoise": True if denoise is not None else None, "features": True if features is not None else None}
    want = {"squares": True, "counts": True, "retire": False, "denoise": denoise is not None, "features": features is not None}
    if error:
        on["error"] = want["error"] = True
        what += " with error=True"
    if background is not None:
        on["background"] = want["background"] = True
        what += " with background="
    if not isinstance(f, Frame) or (f.nx, f.ny) != (nx, ny) or f.flags() != want:
        raise ValueError(what)
    for block in (features, denoise, background):
        if block is not None:
            f.set_in(block)
    more = () if features is None else (f,)
    f.counts[...] = ns
    active = np.ones((ny, nx), dtype=bool)
    t0 = time.perf_counter()
    done = 0
    while done < ns:
        end = min(ns, done + step)
        _, st = cast(end, seed=seed, out=f, sample_begin=done, resume=True, partial=True, squares=True, stats=True, counters=False,
                     **on, **kw)
        if features is not None:
            f.features.compute = 0   # (the planes are traced once)
        if stats is not None:
            stats.append(st)
        done = end
        held = np.minimum(f.counts, done).astype(np.uint32)
        se = f.error.copy() if error else noise.standard_error_counts(f.planes[0], f.planes[1], held)
        if error:   # (the library wrote the plane of every pixel that holds samples: the filter ran in the slice's call)
            retire = noise.retire_filtered(active, done, se, f.counts, min_samples, target_se, radius=radius)
        elif radius:
            retire = noise.retire(active, done, se, min_samples, target_se, radius=radius, present=f.counts > 0)
        else:
            retire = noise.retire(active, done, se, min_samples, target_se)
        f.counts[retire] = done
        active &= ~retire
        pv = CountsFrame(nx, ny)   # resolve a copy: the running sums go on
        pv.copy_in(f.planes[0], held)
        cast(done, seed=seed, out=pv, sample_begin=done, resume=True, **kw)
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
# every symbol include/rtiow_gpu_query.h declares: beside the ABI above, not part of it (no CPU restatement mirrors ray queries)
QUERY_SYMBOLS = ["query_closest", "query_closest_device", "query_occluded", "query_occluded_device"]
# include/rtiow_gpu_rays.h: ray frames (not part of ABI_SYMBOLS either)
RAY_FRAME_SYMBOLS = ["par_cast_rays", "par_cast_rays_device"]
RAYS_PER_PIXEL, RAYS_PER_SAMPLE = 0, 1
# include/rtiow_gpu_image.h: image textures and their probes (not part of ABI_SYMBOLS either: the oracle has no image kind)
IMAGE_SYMBOLS = ["texture_image", "debug_texture_host", "debug_texture", "debug_atan2f_host"]
# include/rtiow_gpu_mesh.h: triangles and meshes (not part of ABI_SYMBOLS either: the oracle has no triangle)
MESH_SYMBOLS = ["object_triangle", "object_mesh", "debug_triangle_host"]
# include/rtiow_gpu_surface.h: per-vertex normals and UVs, surface-mapped textures (not part of ABI_SYMBOLS either)
SURFACE_SYMBOLS = ["object_triangle_attr", "object_mesh_attr", "texture_surface", "debug_triangle_attr_host", "debug_hit_surface"]
FEAT_SURFACE = 2048   # flat_scene.h: the flattened program holds a triangle with per-vertex normals or UVs
# include/rtiow_gpu_environment.h: the scene's environment and its probes (not part of ABI_SYMBOLS either)
ENVIRONMENT_SYMBOLS = ["builder_set_environment", "builder_get_environment", "debug_environment_host", "debug_environment"]
FEAT_TEXTURE = 8          # flat_scene.h: a non-constant texture is referenced, or the scene carries an environment
FEAT_ENVIRONMENT = 4096   # flat_scene.h: the scene carries an environment


class EnvironmentParams(C.Structure):
    """rtg_environment_params (include/rtiow_gpu_environment.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("texture", C.c_uint32), ("scale", C.c_float * 3), ("rotate_y_degrees", C.c_float),
                ("reserved_in", C.c_uint32 * 2)]

    @classmethod
    def new(cls, texture, scale=(1.0, 1.0, 1.0), rotate_y=0.0):
        p = cls()
        p.struct_size = C.sizeof(cls)
        p.texture = INVALID_ID if texture is None else int(texture)
        for i in range(3):
            p.scale[i] = float(scale[i])
        p.rotate_y_degrees = float(rotate_y)
        return p


class ImageParams(C.Structure):
    """rtg_image_params (include/rtiow_gpu_image.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("mapping", C.c_uint32), ("filter", C.c_uint32), ("wrap_u", C.c_uint32),
                ("wrap_v", C.c_uint32), ("reserved_in", C.c_uint32), ("m", C.c_float * 8)]

    @classmethod
    def new(cls, params):
        """From the dict image.params() makes (or any mapping with its keys)."""
        p = cls()
        p.struct_size = C.sizeof(cls)
        p.mapping, p.filter = int(params.get("mapping", 0)), int(params.get("filter", 0))
        p.wrap_u, p.wrap_v = int(params.get("wrap_u", 0)), int(params.get("wrap_v", 0))
        p.reserved_in = int(params.get("reserved_in", 0))
        m = np.zeros(8, dtype=np.float32)
        given = np.asarray(params.get("m", ()), dtype=np.float32).reshape(-1)
        m[:min(8, given.size)] = given[:8]
        for i in range(8):
            p.m[i] = float(m[i])
        return p


def ray_index(nx, ny, sample, row, x, per_sample):
    """Which ray of a ray frame's array starts sample `sample` of pixel (x, row): include/rtiow_gpu_rays.h.  Plain Python
    integers: exact beyond 2^32 rays."""
    p = int(row) * int(nx) + int(x)
    return int(sample) * int(nx) * int(ny) + p if per_sample else p


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
        # include/rtiow_gpu_debug.h (not part of ABI_SYMBOLS: no CPU restatement mirrors it)
        f("debug_box_plan", C.c_int, [C.c_void_p, c_u32p, C.c_size_t, c_u32p, C.c_size_t, c_u8p, C.c_size_t])
        f("debug_production_program", C.c_int, [C.c_void_p, c_u32p, C.c_size_t, c_u32p, C.c_size_t, c_u32p, c_u32p, c_u8p, C.c_size_t])
        f("debug_camera_plan", C.c_int, [C.c_void_p, c_u32p, C.c_size_t, c_u32p, C.c_size_t, c_u32p, C.c_uint64, c_u8p, C.c_size_t])
        # include/rtiow_gpu_query.h (QUERY_SYMBOLS): pointers as void*, so that host arrays and device addresses both pass
        qp, st = C.POINTER(QueryParams), C.POINTER(Stats)
        f("query_closest", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, qp, C.c_void_p, C.c_void_p, st])
        f("query_closest_device", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, qp, C.c_void_p, C.c_void_p, C.c_void_p, st])
        f("query_occluded", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, qp, C.c_void_p, st])
        f("query_occluded_device", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, qp, C.c_void_p, C.c_void_p, st])
        # include/rtiow_gpu_rays.h (RAY_FRAME_SYMBOLS): the same convention
        f("par_cast_rays", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(Params), C.c_void_p, st])
        f("par_cast_rays_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(Params), C.c_void_p, C.c_void_p, st])
        # include/rtiow_gpu_image.h (IMAGE_SYMBOLS)
        f("texture_image", C.c_uint32, [C.c_void_p, C.POINTER(ImageParams), C.c_uint32, C.c_uint32, c_f32p])
        f("debug_texture_host", C.c_int, [C.c_void_p, C.c_uint32, C.c_size_t, c_f32p, c_f32p])
        f("debug_texture", C.c_int, [C.c_void_p, C.c_uint32, C.c_size_t, c_f32p, c_f32p])
        f("debug_atan2f_host", C.c_int, [C.c_size_t, c_f32p, c_f32p, c_f32p])
        # include/rtiow_gpu_mesh.h (MESH_SYMBOLS)
        f("object_triangle", C.c_uint32, [C.c_void_p, c_f32p, c_f32p, c_f32p, C.c_uint32])
        f("object_mesh", C.c_uint32, [C.c_void_p, c_f32p, C.c_size_t, c_u32p, C.c_size_t, C.c_uint32, C.c_uint32])
        f("debug_triangle_host", C.c_int, [C.c_size_t, c_f32p, c_f32p, C.c_float, c_f32p])
        # include/rtiow_gpu_surface.h (SURFACE_SYMBOLS)
        f("object_triangle_attr", C.c_uint32, [C.c_void_p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_uint32])
        f("object_mesh_attr", C.c_uint32, [C.c_void_p, c_f32p, C.c_size_t, c_u32p, C.c_size_t, c_f32p, c_f32p, C.c_uint32, C.c_uint32])
        f("texture_surface", C.c_uint32, [C.c_void_p, C.c_uint32])
        f("debug_triangle_attr_host", C.c_int, [C.c_size_t, c_f32p, c_f32p, C.c_uint32, c_f32p, C.c_float, c_f32p])
        f("debug_hit_surface", C.c_int, [C.c_void_p, C.c_size_t, c_f32p, C.c_uint64, C.c_float, c_f32p, c_u32p])
        # include/rtiow_gpu_environment.h (ENVIRONMENT_SYMBOLS)
        f("builder_set_environment", C.c_int, [C.c_void_p, C.POINTER(EnvironmentParams)])
        f("builder_get_environment", C.c_int, [C.c_void_p, C.POINTER(EnvironmentParams), c_f32p])
        f("debug_environment_host", C.c_int, [C.c_void_p, C.c_size_t, c_f32p, c_f32p])
        f("debug_environment", C.c_int, [C.c_void_p, C.c_size_t, c_f32p, c_f32p])

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
        background= (RTG_FLAG_BACKGROUND; a colour, a dict of bottom / top or a Background): as in Scene.par_cast, with and
        without "multi_planes" -- every handle renders with the same block.
        stats=True returns (frame, rtg_stats as a dict), with the instrumented counters unless counters=False."""
        kw = dict(kw)
        counts, retire, denoise, features = (kw.pop(k, None) for k in ("counts", "retire", "denoise", "features"))
        return _render(lambda part: _supported(self, part), lambda p, buf: self._par_cast_multi_call(scenes, camera, p, buf),
                       nx, ny, ns, seed, stats, out, True if counters is None else counters, counts, retire, denoise, features, kw,
                       exact=False, forward=True)

    def _par_cast_multi_call(self, scenes, camera, p, buf):
        """The library call alone, on any params and buffer."""
        st = Stats.new()
        arr = (C.c_void_p * len(scenes))(*[s.h for s in scenes])
        self.check(self._par_cast_multi(arr, len(scenes), C.byref(camera), C.byref(p), buf.ctypes.data_as(c_f32p), C.byref(st)))
        return st

    def adaptive_multi(self, scenes, camera, nx, ny, ns, step, target_se, min_samples=16, budget_s=None, out=None, seed=0xDEADBEEF,
                       stats=None, radius=0, denoise=None, features=None, filtered_error=False, **kw):
        """Scene.adaptive's host-frame loop over several handles (scene option "multi_planes" on one of them): every slice is
        one par_cast_multi call, the retire rule is noise.retire on the host, and the loop yields the same tuples --
        (counts, preview, stderr), then the filtered frame with denoise=, then the FeaturesFrame with features=.
        filtered_error=True (needs denoise=): as in Scene.adaptive -- the rule is noise.retire_filtered on the error plane.
        background= (RTG_FLAG_BACKGROUND): as in Scene.adaptive."""
        if step < 1:
            raise ValueError("step must be >= 1")
        if not 0 <= radius <= RETIRE_MAX_RADIUS:
            raise ValueError("radius must be in 0 .. %d" % RETIRE_MAX_RADIUS)
        if filtered_error:
            _supported(self, "error")
        _supported(self, "squares")
        _supported(self, "counts")
        if filtered_error and not _given(denoise):
            raise ValueError("filtered_error=True needs denoise= (the filter writes the error plane)")
        features = make_features(features) if _given(features) else None
        denoise = make_denoise(denoise) if _given(denoise) else None
        background = kw.pop("background", None)
        if _given(background):
            _supported(self, "background")
        background = make_background(background) if _given(background) else None
        yield from _adaptive_host(lambda n, **k: self.par_cast_multi(scenes, camera, nx, ny, n, **k), nx, ny, ns, step,
                                  target_se, min_samples, budget_s, out, seed, stats, radius, denoise, features, kw, bool(filtered_error),
                                  background)

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


    def atan2f_host(self, y, x):
        """rtg_debug_atan2f_host: rt_atan2f(y, x) on the host (image.atan2f is its definition)."""
        y, x = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in np.broadcast_arrays(y, x))
        out = np.empty_like(y)
        self.check(self._debug_atan2f_host(y.size, y.ctypes.data_as(c_f32p), x.ctypes.data_as(c_f32p), out.ctypes.data_as(c_f32p)))
        return out

    def triangle_host(self, tri9, rays8, t_min=0.001):
        """rtg_debug_triangle_host: n (triangle, ray) pairs -- tri9 [n, 9] = v0, v1, v2; rays8 [n, 8] = o, d, time, t_max --
        through the function the kernels call, on the host.  [n, 8] = hit, t, p, n; zeros on a miss (triangle.hit is its
        definition)."""
        tri9 = np.ascontiguousarray(tri9, dtype=np.float32).reshape(-1, 9)
        rays8 = np.ascontiguousarray(rays8, dtype=np.float32).reshape(-1, 8)
        if len(tri9) != len(rays8):
            raise ValueError("triangle_host: one ray per triangle")
        out = np.empty((len(tri9), 8), dtype=np.float32)
        self.check(self._debug_triangle_host(len(tri9), tri9.ctypes.data_as(c_f32p), rays8.ctypes.data_as(c_f32p), float(t_min),
                                             out.ctypes.data_as(c_f32p)))
        return out

    def triangle_attr_host(self, tri9, attr15, has, rays8, t_min=0.001):
        """rtg_debug_triangle_attr_host (include/rtiow_gpu_surface.h): n (triangle, ray) pairs -- tri9 [n, 9]; attr15 [n, 15] =
        n0, n1, n2, uv0, uv1, uv2; has: bit 0 use the normals, bit 1 use the UVs; rays8 [n, 8] -- through the functions the
        kernels call, on the host.  [n, 10] = hit, t, p, n, tu, tv; zeros on a miss (triangle.hit + triangle.shade define it)."""
        tri9 = np.ascontiguousarray(tri9, dtype=np.float32).reshape(-1, 9)
        attr15 = np.ascontiguousarray(attr15, dtype=np.float32).reshape(-1, 15)
        rays8 = np.ascontiguousarray(rays8, dtype=np.float32).reshape(-1, 8)
        if len(tri9) != len(rays8) or len(tri9) != len(attr15):
            raise ValueError("triangle_attr_host: one ray and one attribute row per triangle")
        out = np.empty((len(tri9), 10), dtype=np.float32)
        self.check(self._debug_triangle_attr_host(len(tri9), tri9.ctypes.data_as(c_f32p), attr15.ctypes.data_as(c_f32p), int(has),
                                                  rays8.ctypes.data_as(c_f32p), float(t_min), out.ctypes.data_as(c_f32p)))
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

    def image(self, img, params):
        """rtg_texture_image (include/rtiow_gpu_image.h): img float32 [h, w, 3], row 0 at the top; params from image.params /
        image.planar / image.spherical (or an ImageParams).  Returns an ordinary texture id."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("an image is [h, w, 3]")
        p = params if isinstance(params, ImageParams) else ImageParams.new(params)
        return self.be.check_id(self.be._texture_image(self.h, C.byref(p), img.shape[1], img.shape[0], img.ctypes.data_as(c_f32p)))

    def surface(self, texture):
        """rtg_texture_surface (include/rtiow_gpu_surface.h): `texture` evaluated at a hit's surface coordinates (tu, tv, 0)
        instead of p.  For lambertian() and diffuse_light() only, and only on triangles with UVs."""
        return self.be.check_id(self.be._texture_surface(self.h, texture))

    def texture_host(self, texture, p):
        """rtg_debug_texture_host: the texture's value at the points p [n, 3] on the host (image and constant textures)."""
        p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
        out = np.empty_like(p)
        self.be.check(self.be._debug_texture_host(self.h, texture, len(p), p.ctypes.data_as(c_f32p), out.ctypes.data_as(c_f32p)))
        return out

    def environment(self, texture, scale=(1.0, 1.0, 1.0), rotate_y=0.0):
        """rtg_builder_set_environment (include/rtiow_gpu_environment.h): what a ray that leaves the scene sees -- `scale` times
        `texture` at the point rot_y(unit(d)); an image with image.spherical() is a lat-long map.  texture=None clears; a second
        call replaces.  Scenes made afterwards carry it."""
        p = texture if isinstance(texture, EnvironmentParams) else EnvironmentParams.new(texture, scale, rotate_y)
        self.be.check(self.be._builder_set_environment(self.h, C.byref(p)))

    def get_environment(self):
        """rtg_builder_get_environment: dict(texture (None when there is none), scale, rotate_y, s, c)."""
        p, sc = EnvironmentParams(), (C.c_float * 2)()
        self.be.check(self.be._builder_get_environment(self.h, C.byref(p), sc))
        return dict(texture=None if p.texture == INVALID_ID else int(p.texture), scale=np.array(list(p.scale), dtype=np.float32),
                    rotate_y=float(p.rotate_y_degrees), s=np.float32(sc[0]), c=np.float32(sc[1]), struct_size=int(p.struct_size))

    def environment_host(self, d):
        """rtg_debug_environment_host: E(d) for the directions d [n, 3] on the host (image and constant textures)."""
        d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
        out = np.empty_like(d)
        self.be.check(self.be._debug_environment_host(self.h, len(d), d.ctypes.data_as(c_f32p), out.ctypes.data_as(c_f32p)))
        return out

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

    def box_plan(self, world=None, words=None):
        """Host-only (product library): the box plan of a lean program, one uint8 per record -- 0 kept, 1 box-chain follower,
        2 pruned interior box (csrc/rt_box_plan.h).  `words` ([n, 8] uint32, as flatten returns them) replaces the world."""
        if words is not None:
            words = np.ascontiguousarray(words, dtype=np.uint32)
            mask = np.zeros(len(words), dtype=np.uint8)
            n = self.be._debug_box_plan(None, None, 0, words.ctypes.data_as(c_u32p), len(words), mask.ctypes.data_as(c_u8p), len(mask))
        else:
            arr = (C.c_uint32 * max(1, len(world)))(*world)
            n = self.be._debug_box_plan(self.h, arr, len(world), None, 0, None, 0)
            if n < 0:
                self.be.check(n)
            mask = np.zeros(n, dtype=np.uint8)
            n = self.be._debug_box_plan(self.h, arr, len(world), None, 0, mask.ctypes.data_as(c_u8p), len(mask))
        if n < 0:
            self.be.check(n)
        return mask

    def production_program(self, world=None, words=None):
        """Host-only (product library): the production program of a lean program (csrc/rt_box_plan.h box_tree_rebuild; scene
        option box_tree) as (words [n, 8] uint32, origin [n] uint32, mask [n] uint8): origin[i] is the record of the given
        program that record i copies (0xffffffff: a new interior box), mask the box plan over the production program.
        `words` ([n, 8] uint32, as flatten returns them) replaces the world."""
        if words is not None:
            words = np.ascontiguousarray(words, dtype=np.uint32)
            head = (None, None, 0, words.ctypes.data_as(c_u32p), len(words))
            n = len(words)
        else:
            arr = (C.c_uint32 * max(1, len(world)))(*world)
            head = (self.h, arr, len(world), None, 0)
            n = self.be._debug_production_program(*head, None, None, None, 0)
            if n < 0:
                self.be.check(n)
        out = np.zeros((n, 8), dtype=np.uint32)
        origin = np.zeros(n, dtype=np.uint32)
        mask = np.zeros(n, dtype=np.uint8)
        n = self.be._debug_production_program(*head, out.ctypes.data_as(c_u32p), origin.ctypes.data_as(c_u32p), mask.ctypes.data_as(c_u8p), n)
        if n < 0:
            self.be.check(n)
        return out, origin, mask

    def camera_plan(self, words, counts, n_rays):
        """Host-only (product library): the camera plan (scene option box_camera; csrc/rt_box_plan.h BOX_PLAN_COUNTS) of the lean
        program `words` ([n, 8] uint32, as flatten / production_program return them) from pass counts: counts[i] walks out of
        n_rays passed BOX record i.  One uint8 per record as box_plan returns them; any counts are accepted."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        if len(counts) != len(words):
            raise ValueError("camera_plan: one count per record")
        mask = np.zeros(len(words), dtype=np.uint8)
        n = self.be._debug_camera_plan(None, None, 0, words.ctypes.data_as(c_u32p), len(words), counts.ctypes.data_as(c_u32p), int(n_rays),
                                       mask.ctypes.data_as(c_u8p), len(mask))
        if n < 0:
            self.be.check(n)
        return mask

    def bvh_sah(self, objs, exposure=(0.0, 1.0)):
        """Not in the reference: SAH-built Bvh; same results up to exact-t ties, fewer box tests."""
        arr = (C.c_uint32 * max(1, len(objs)))(*objs)
        return self.be.check_id(self.be._object_bvh_sah(self.h, arr, len(objs), exposure[0], exposure[1]))

    def triangle(self, v0, v1, v2, material):
        """rtg_object_triangle (include/rtiow_gpu_mesh.h): an ordinary object id; counter-clockwise is the front face."""
        return self.be.check_id(self.be._object_triangle(self.h, _f3(v0), _f3(v1), _f3(v2), material))

    def triangle_attr(self, v0, v1, v2, material, normals=None, uvs=None):
        """rtg_object_triangle_attr (include/rtiow_gpu_surface.h): normals [3, 3] and / or uvs [3, 2] of v0, v1, v2; with both
        None it is triangle()."""
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(9)
        t = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(6)
        return self.be.check_id(self.be._object_triangle_attr(self.h, _f3(v0), _f3(v1), _f3(v2),
                                                              None if n is None else n.ctypes.data_as(c_f32p),
                                                              None if t is None else t.ctypes.data_as(c_f32p), material))

    def mesh(self, vertices, indices, material, sah=False, normals=None, uvs=None):
        """rtg_object_mesh: vertices [n, 3] float32, indices [m, 3] uint32 (triangle.icosphere / box / grid / load_obj make
        them) -> the m triangle objects and one Bvh object over them (sah: the SAH builder); returns the Bvh's id.
        normals [n, 3] / uvs [n, 2] (triangle.icosphere_attr / vertex_normals / load_obj_attr make them): rtg_object_mesh_attr
        (include/rtiow_gpu_surface.h); with both None, today's call."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        ix = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        if normals is not None or uvs is not None:
            nn = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
            uv = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 2)
            if (nn is not None and len(nn) != len(v)) or (uv is not None and len(uv) != len(v)):
                raise ValueError("mesh: one normal and one UV per vertex")
            return self.be.check_id(self.be._object_mesh_attr(self.h, v.ctypes.data_as(c_f32p), len(v), ix.ctypes.data_as(c_u32p), len(ix),
                                                              None if nn is None else nn.ctypes.data_as(c_f32p),
                                                              None if uv is None else uv.ctypes.data_as(c_f32p), material, int(sah)))
        return self.be.check_id(self.be._object_mesh(self.h, v.ctypes.data_as(c_f32p), len(v), ix.ctypes.data_as(c_u32p), len(ix),
                                                     material, int(sah)))

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
                   "box_leave", "refill_min", "gather_min", "run_ahead", "run_ahead_min", "sphere_min", "verbose", "bvh4", "box_chains", "box_prune", "box_tree", "box_camera", "force_rccl", "multi_gather", "multi_planes", "scratch_mb", "frames_in_flight", "small_frames", "drain_share", "hoist", "deep_sized", "mat_lds", "pool2", "p2_refill", "p2_box_leave", "p2_park", "p2_sphere", "p2_prism", "p2_list", "p2_push", "light_sampling", "query_lds", "query_refill", "ray_pool")

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
        [sample_begin, min(n_p, ns)) of each pixel; pixels with n_p = 0 are left as `out` holds them.  out= a CountsFrame, or
        `out` and `counts` that are one CountsFrame's views, are rendered in place; anything else goes through a staging copy.
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
        error=True (RTG_FLAG_DENOISE_ERROR; needs denoise=): the frame the call returns also has the `error` view, the variance
        of every filtered pixel (denoise.nlm_error / nlm_guided_error), +inf where a pixel was passed through; with retire= the
        rule is noise.retire_filtered on that plane.  out= a frame made with error=True is rendered in place.
        background= (RTG_FLAG_BACKGROUND): what a ray that leaves the scene sees instead of black -- a colour (r, g, b), the
        constant background, or a dict of bottom / top, the gradient along world +y (background.sky; make_background).  It
        changes no plane's place: beside an array the call still returns the array.  out= a frame made with background= is
        rendered in place (background=True: its block as it stands).
        stats=True returns (out, rtg_stats as a dict), with the instrumented counters unless counters=False."""
        def call(p, buf):
            st = Stats.new()
            self.be.check(self.be._par_cast(*self._par_cast_args(
                [self.h, C.byref(camera), C.byref(p), buf.ctypes.data_as(c_f32p), C.byref(st)], threads)))
            return st
        return _render(lambda part: _supported(self.be, part), call, nx, ny, ns, seed, stats, out,
                       stats if counters is None else counters, counts, retire, denoise, features, kw, exact=True)

    def par_cast_device(self, camera, params, d_out_ptr, stream=None, want_stats=False, sample_begin=None, partial=None,
                        resume=None, squares=None, counts=None, retire=None, denoise=None, features=None, error=None,
                        background=None):
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
        `d_out_ptr` then holds features_frame_bytes(nx, ny, squares, counts, retire, denoise) for the flags the call ends up with.
        error= (RTG_FLAG_DENOISE_ERROR; needs the denoise part): True, the flag -- `d_out_ptr` then ends with the error plane
        (FrameLayout(..., error=True).words words in all).
        background= (RTG_FLAG_BACKGROUND): True, the flag alone (the caller has written the block on the device); a colour, a
        dict of bottom / top or a Background (make_background), written to the block before the call.  `d_out_ptr` then ends
        with the 64-byte block (FrameLayout(..., background=True).words words in all)."""
        if _given(background) and background is not True:
            background = make_background(background)
        over = {"squares": squares, "counts": counts, "retire": retire, "denoise": denoise, "features": features, "error": error,
                "background": background}
        bits = {"squares": FLAG_SUM_SQUARES, "counts": FLAG_SAMPLE_COUNTS, "retire": FLAG_RETIRE, "denoise": FLAG_DENOISE,
                "features": FLAG_FEATURES, "error": FLAG_DENOISE_ERROR, "background": FLAG_BACKGROUND}
        # the parts the call ends up with: those of `params` unless overridden (an array or a block turns its part on).
        # Every refusal first: a refused call has written nothing to the caller's frame
        has = {part: bool(params.flags & bits[part] if on is None else on if isinstance(on, (bool, int)) else True)
               for part, on in over.items()}
        for part in ("background", "error", "features", "denoise", "squares", "counts", "retire"):
            if has[part] if part == "squares" else _given(over[part]):
                _supported(self.be, part)
        if has["error"] and not has["denoise"]:
            raise ValueError("error=True needs the denoise part (the filter writes the error plane)")
        lay = FrameLayout(params.nx, params.ny, **has)
        # blocks of the caller's: (block, byte offset, bytes written before the call); all of a block is read back after it
        blocks = [(over[part], 4 * at, n) for part, at, n in (("retire", lay.retire, C.sizeof(Retire)),
                                                             ("denoise", lay.denoise, Denoise.OUT_OFFSET),
                                                             ("features", lay.features, Features.OUT_OFFSET),
                                                             ("background", lay.background, Background.OUT_OFFSET))
                  if isinstance(over[part], C.Structure)]
        for block, at, n in blocks:
            self._block_copy(d_out_ptr, block, stream, True, at, n)
        if _given(counts) and counts is not True:
            self._upload_counts(lay, counts, d_out_ptr, stream)
        if sample_begin is not None or partial is not None or resume is not None or any(on is not None for on in over.values()):
            q = Params()
            C.pointer(q)[0] = params
            if sample_begin is not None:
                q.sample_begin = sample_begin
            for on, bit in [(partial, FLAG_PARTIAL), (resume, FLAG_RESUME)] + [(on if on is None else has[part], bits[part])
                                                                             for part, on in over.items()]:
                if on is not None:
                    q.flags = (q.flags | bit) if on else (q.flags & ~bit)
            params = q
        st = Stats.new()
        self.be.check(self.be._par_cast_device(self.h, C.byref(camera), C.byref(params), d_out_ptr, stream,
                                               C.byref(st) if want_stats else None))
        for block, at, _ in blocks:
            self._block_copy(d_out_ptr, block, stream, False, at, C.sizeof(block))
        return st.as_dict() if want_stats else None

    def _block_copy(self, d_out_ptr, block, stream, to_device, offset, nbytes):
        """Copy `nbytes` of a block (host memory) to, or from, byte `offset` of a device frame on `stream`, and wait for it."""
        hip, hs = _hip_runtime(), _stream(stream)
        dev, host = C.c_void_p(_device_ptr(d_out_ptr) + offset), C.c_void_p(C.addressof(block))
        what = "hipMemcpyAsync(%s block)" % type(block).__name__.lower()
        _hip_ok(hip.hipMemcpyAsync(*((dev, host, nbytes, 1) if to_device else (host, dev, nbytes, 2)), hs), what)
        _hip_ok(hip.hipStreamSynchronize(hs), what)

    def _upload_counts(self, lay, counts, d_out_ptr, stream):
        """Copy a uint32 [ny, nx] count array into the count plane of a device frame (layout `lay`), on `stream`."""
        hip, hs = _hip_runtime(), _stream(stream)
        dst = C.c_void_p(_device_ptr(d_out_ptr) + 4 * lay.counts)
        if hasattr(counts, "data_ptr") and getattr(counts, "is_cuda", False):
            if tuple(counts.shape) != (lay.ny, lay.nx) or counts.element_size() != 4 or not counts.is_contiguous():
                raise ValueError("counts= must be a contiguous 4-byte [ny, nx] tensor")
            _hip_ok(hip.hipMemcpyAsync(dst, C.c_void_p(counts.data_ptr()), 4 * lay.n, 3, hs), "hipMemcpyAsync(count plane)")   # 3: device to device
        else:
            host = np.ascontiguousarray(counts, dtype=np.uint32)
            if host.shape != (lay.ny, lay.nx):
                raise ValueError("counts= must have shape (ny, nx) = %s" % ((lay.ny, lay.nx),))
            _hip_ok(hip.hipMemcpyAsync(dst, C.c_void_p(host.ctypes.data), 4 * lay.n, 1, hs), "hipMemcpyAsync(count plane)")   # 1: host to device
            _hip_ok(hip.hipStreamSynchronize(hs), "hipMemcpyAsync(count plane)")   # (the host array may go away when this call returns)

    def _loop_block(self, part, given, make):
        """The block a loop writes to its frame: make(given), checked, when the loop was asked for `part`, else None."""
        if not _given(given):
            return None
        _supported(self.be, part)
        return make(given)

    def adaptive(self, camera, nx, ny, ns, step, target_se, min_samples=16, budget_s=None, out=None, seed=0xDEADBEEF,
                 stats=None, radius=0, preview=None, stream=None, denoise=None, denoised=None, features=None,
                 filtered_error=False, **kw):
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
        (the planes start 64 bytes behind it).
        filtered_error=True (needs denoise=; RTG_FLAG_DENOISE_ERROR): every slice's call also writes the error plane of the
        filtered frame, and the retire rule is noise.retire_filtered on it -- a pixel retires once the estimated variance of
        its FILTERED value (every one of its window) is <= target_se^2.  Host frames: `out`, when given, is a frame made with
        error=True; the loop's third item is the error plane (float32 [ny, nx, 3]: variances, +inf where unknown) instead of
        stderr.  Device frames: `out` ends with the error plane (FrameLayout(nx, ny, True, True, True, True, features,
        True).words words); info's estimated / sum_se2 / est_rmse are those of the filtered frame.
        background= (RTG_FLAG_BACKGROUND; a colour, a dict of bottom / top or a Background): every slice renders with it.  Host
        frames: `out`, when given, is a frame made with background=.  Device frames: `out` ends with the 64-byte block."""
        if step < 1:
            raise ValueError("step must be >= 1")
        if filtered_error:
            _supported(self.be, "error")
        _supported(self.be, "squares")
        _supported(self.be, "counts")
        if not 0 <= radius <= RETIRE_MAX_RADIUS:
            raise ValueError("radius must be in 0 .. %d" % RETIRE_MAX_RADIUS)
        if filtered_error and not _given(denoise):
            raise ValueError("filtered_error=True needs denoise= (the filter writes the error plane)")
        features, denoise = self._loop_block("features", features, make_features), self._loop_block("denoise", denoise, make_denoise)
        background = self._loop_block("background", kw.pop("background", None), make_background)
        if out is not None and not isinstance(out, Frame):
            _supported(self.be, "retire")
            if preview is None:
                raise ValueError("a device frame needs a device preview buffer (preview=)")
            if denoise is not None and denoised is None:
                raise ValueError("denoise= on a device frame needs a device buffer for the filtered frame (denoised=)")
            yield from self._adaptive_device(camera, nx, ny, ns, step, target_se, min_samples, budget_s, out, seed, stats,
                                             radius, preview, stream, kw, denoise, denoised, features, bool(filtered_error), background)
            return
        yield from _adaptive_host(lambda n, **k: self.par_cast(camera, nx, ny, n, **k), nx, ny, ns, step, target_se,
                                  min_samples, budget_s, out, seed, stats, radius, denoise, features, kw, bool(filtered_error), background)

    def _adaptive_device(self, camera, nx, ny, ns, step, target_se, min_samples, budget_s, out, seed, stats, radius, preview,
                         stream, kw, denoise=None, denoised=None, features=None, error=False, background=None):
        hip, hs, ok = _hip_runtime(), _stream(stream), _hip_ok
        d_out, d_pv = _device_ptr(out), _device_ptr(preview)
        lay = FrameLayout(nx, ny, True, True, True, denoise is not None, features is not None, error, background is not None)
        if background is not None:   # (in-only: written once)
            self._block_copy(d_out, background, stream, True, 4 * lay.background, Background.OUT_OFFSET)
        plane, counts_at = lay.n, d_out + 4 * lay.counts
        # every pixel's target count is ns; the block's in-fields are written once (the library never writes them)
        ok(hip.hipMemsetD32Async(C.c_void_p(counts_at), ns - (1 << 32) if ns >= 1 << 31 else ns, plane, hs), "hipMemsetD32Async(counts)")
        block = Retire(target_se=float(target_se), min_samples=int(min_samples), radius=int(radius))
        self._block_copy(d_out, block, stream, True, 4 * lay.retire, C.sizeof(Retire))
        if denoise is not None:   # (likewise: its in-fields once)
            self._block_copy(d_out, denoise, stream, True, 4 * lay.denoise, Denoise.OUT_OFFSET)
        more = ()
        if features is not None:   # (its in-fields before the first slice, and once more, with compute = 0, behind it)
            self._block_copy(d_out, features, stream, True, 4 * lay.features, Features.OUT_OFFSET)
            more = (4 * lay.features,)
        t0 = time.perf_counter()
        done = 0
        while done < ns:
            end = min(ns, done + step)
            st = self.par_cast_device(camera, make_params(nx, ny, end, seed=seed, sample_begin=done, resume=True, partial=True,
                                                          squares=True, counts=True, retire=True, denoise=denoise is not None,
                                                          features=features is not None, error=error,
                                                          background=background is not None, **kw), d_out, hs,
                                      want_stats=stats is not None)
            if features is not None and features.compute:
                features.compute = 0
                self._block_copy(d_out, features, stream, True, 4 * lay.features, Features.OUT_OFFSET)
            if denoise is not None:
                ok(hip.hipMemcpyAsync(C.c_void_p(_device_ptr(denoised)), C.c_void_p(d_out + 4 * lay.denoised), plane * 3 * 4, 3, hs),
                   "hipMemcpyAsync(denoised)")
            if stats is not None:
                stats.append(st)
            done = end
            # the preview: plane 0 and the count plane, resolved per pixel (e_p = min(n_p, k): the samples each pixel holds)
            ok(hip.hipMemcpyAsync(C.c_void_p(d_pv), C.c_void_p(d_out), plane * 3 * 4, 3, hs), "hipMemcpyAsync(preview)")
            ok(hip.hipMemcpyAsync(C.c_void_p(d_pv + plane * 3 * 4), C.c_void_p(counts_at), plane * 4, 3, hs), "hipMemcpyAsync(preview counts)")
            self.par_cast_device(camera, make_params(nx, ny, done, seed=seed, sample_begin=done, resume=True, counts=True, **kw),
                                 d_pv, hs)
            self._block_copy(d_out, block, stream, False, 4 * lay.retire, C.sizeof(Retire))
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
        and the item is the byte offset of the features block in it (the planes start 64 bytes behind it).
        background= (RTG_FLAG_BACKGROUND; a colour, a dict of bottom / top or a Background): every slice renders with it.
        Device frames: `out` then ends with the 64-byte block (FrameLayout(..., background=True).words words in all)."""
        if step < 1:
            raise ValueError("step must be >= 1")
        features = self._loop_block("features", features, make_features)
        background = self._loop_block("background", kw.pop("background", None), make_background)
        squares = bool(squares) or target_rmse is not None or _given(denoise)
        if squares:
            _supported(self.be, "squares")
        denoise = self._loop_block("denoise", denoise, make_denoise)
        if out is not None and not isinstance(out, np.ndarray):
            if target_rmse is not None:
                raise ValueError("target_rmse needs host frames: there is no device-side error reduction")
            if preview is None:
                raise ValueError("a device running sum needs a device preview buffer (preview=)")
            if denoise is not None and denoised is None:
                raise ValueError("denoise= on a device frame needs a device buffer for the filtered frame (denoised=)")
            yield from self._progressive_device(camera, nx, ny, ns, step, seed, budget_s, out, preview, stream, squares, kw,
                                                denoise, denoised, features, background)
            return
        shape = (2, ny, nx, 3) if squares else (ny, nx, 3)
        acc = np.zeros(shape, dtype=np.float32) if out is None else out
        frame = None   # with a block the slices render into a frame; a caller's `out` is kept up to date beside it
        if features is not None:
            frame = FeaturesFrame(nx, ny, squares, denoise=denoise, features=features, background=background)
        elif denoise is not None:
            frame = DenoiseFrame(nx, ny, denoise=denoise, background=background)
        elif background is not None:
            frame = Frame(nx, ny, squares, background=background)
        if frame is not None:
            frame.copy_in(acc)
        on = {"denoise": True if denoise is not None else None, "features": True if features is not None else None}
        if background is not None:
            on["background"] = True
        more = () if features is None else (frame,)
        sums = acc[0] if squares else acc
        t0 = time.perf_counter()
        done = 0
        while done < ns:
            end = min(ns, done + step)
            self.par_cast(camera, nx, ny, end, seed=seed, out=acc if frame is None else frame, sample_begin=done, resume=True, partial=True,
                          squares=squares, **on, **kw)
            if frame is not None:
                frame.copy_back(acc)
            if features is not None:
                frame.features.compute = 0   # (the planes are traced once)
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
                            denoised=None, features=None, background=None):
        hip, hs = _hip_runtime(), _stream(stream)
        d_acc, d_preview = C.c_void_p(_device_ptr(acc)), C.c_void_p(_device_ptr(preview))
        lay = FrameLayout(nx, ny, squares, False, False, denoise is not None, features is not None, background=background is not None)
        if background is not None:   # (in-only: written once)
            self._block_copy(acc, background, stream, True, 4 * lay.background, Background.OUT_OFFSET)
        if denoise is not None:   # the block's in-fields are written once (the library never writes them)
            self._block_copy(acc, denoise, stream, True, 4 * lay.denoise, Denoise.OUT_OFFSET)
        more = ()
        if features is not None:   # (its in-fields before the first slice, and once more, with compute = 0, behind it)
            self._block_copy(acc, features, stream, True, 4 * lay.features, Features.OUT_OFFSET)
            more = (4 * lay.features,)
        t0 = time.perf_counter()
        done = 0
        while done < ns:
            end = min(ns, done + step)
            self.par_cast_device(camera, make_params(nx, ny, end, seed=seed, sample_begin=done, resume=True, partial=True,
                                                     squares=squares, denoise=denoise is not None, features=features is not None,
                                                     background=background is not None, **kw), d_acc, hs)
            if features is not None and features.compute:
                features.compute = 0
                self._block_copy(acc, features, stream, True, 4 * lay.features, Features.OUT_OFFSET)
            done = end
            if denoise is not None:
                _hip_ok(hip.hipMemcpyAsync(C.c_void_p(_device_ptr(denoised)), C.c_void_p(d_acc.value + 4 * lay.denoised), lay.n * 3 * 4, 3, hs),
                        "hipMemcpyAsync(denoised)")
            _hip_ok(hip.hipMemcpyAsync(d_preview, d_acc, lay.n * 3 * 4, 3, hs), "hipMemcpyAsync(preview)")   # plane 0; 3 = hipMemcpyDeviceToDevice
            self.par_cast_device(camera, make_params(nx, ny, done, seed=seed, sample_begin=done, resume=True, **kw), d_preview, hs)
            if denoise is not None:
                yield (done, preview, acc, denoised) + more
            else:
                yield ((done, preview, acc) if squares else (done, preview)) + more
            if budget_s is not None:
                _hip_ok(hip.hipStreamSynchronize(hs), "hipStreamSynchronize")
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

    def debug_hit_surface(self, rays, seed=1, t_near=0.001):
        """rtg_debug_hit_surface (include/rtiow_gpu_surface.h): debug_hit_top with (tu, tv) behind the normal.  ([n, 10], mat)"""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
        n = rays.shape[0]
        out = np.zeros((n, 10), dtype=np.float32)
        mat = np.zeros(n, dtype=np.uint32)
        self.be.check(self.be._debug_hit_surface(self.h, n, rays.ctypes.data_as(c_f32p), seed, t_near,
                                                 out.ctypes.data_as(c_f32p), mat.ctypes.data_as(c_u32p)))
        return out, mat

    def debug_texture(self, texture, p):
        """rtg_debug_texture (include/rtiow_gpu_image.h): the texture's value at the points p [n, 3] on the scene's device,
        through the function every kernel evaluates a texture with.  Every texture kind."""
        p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
        out = np.empty_like(p)
        self.be.check(self.be._debug_texture(self.h, texture, len(p), p.ctypes.data_as(c_f32p), out.ctypes.data_as(c_f32p)))
        return out

    def debug_environment(self, d):
        """rtg_debug_environment (include/rtiow_gpu_environment.h): E(d) for the directions d [n, 3] on the scene's device,
        through the function the kernels' miss branches call.  Every texture kind."""
        d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
        out = np.empty_like(d)
        self.be.check(self.be._debug_environment(self.h, len(d), d.ctypes.data_as(c_f32p), out.ctypes.data_as(c_f32p)))
        return out

    # ---- ray queries (include/rtiow_gpu_query.h) ---------------------------------------------------------------------
    def _query(self, what, width, rays, seed, t_min, first_index, stream, stats, outputs):
        """One query call.  `rays`: a numpy array -> the host entry point, numpy results; a torch tensor on the scene's
        device -> the device entry point on `stream` (default: the current torch stream), torch results, no host round
        trip.  `outputs`: ((columns or None, numpy dtype, torch dtype name), ...)."""
        p = make_query_params(seed, t_min, first_index)
        st = Stats.new() if stats else None
        st_arg = C.byref(st) if stats else None
        if hasattr(rays, "data_ptr"):
            import torch
            if not rays.is_cuda:
                raise ValueError("%s: a torch tensor must live on the scene's device (pass a numpy array for host rays)" % what)
            if rays.dtype != torch.float32 or not rays.is_contiguous():   # (no temporary copy: the call returns before the kernel reads it)
                raise ValueError("%s: the rays must be a contiguous float32 tensor" % what)
            rays = rays.reshape(-1, width)
            n = rays.shape[0]
            outs = [torch.empty((n, c) if c else (n,), dtype=getattr(torch, t), device=rays.device) for c, _, t in outputs]
            if stream is None:
                stream = torch.cuda.current_stream(rays.device)
            if isinstance(stream, torch.cuda.Stream):   # the results are written on `stream`, whatever stream allocated them
                for o in outs:
                    o.record_stream(stream)
            hs = _stream(stream)
            fn = getattr(self.be, "_query_%s_device" % what)
            self.be.check(fn(self.h, n, _device_ptr(rays), C.byref(p), *[_device_ptr(o) for o in outs], hs, st_arg))
        else:
            rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, width)
            n = rays.shape[0]
            outs = [np.zeros((n, c) if c else (n,), dtype=d) for c, d, _ in outputs]
            fn = getattr(self.be, "_query_%s" % what)
            self.be.check(fn(self.h, n, rays.ctypes.data, C.byref(p), *[o.ctypes.data for o in outs], st_arg))
        res = outs[0] if len(outs) == 1 else tuple(outs)
        return (res, st.as_dict()) if stats else res

    def closest_hit(self, rays, seed=1, t_min=0.001, first_index=0, stream=None, stats=False):
        """Closest hit of the caller's rays, [n, 7] (origin, direction, time): (out [n, 8] float32 = (hit, t, p, normal),
        material [n] -- uint32 in numpy, int32 in torch, 0xffffffff / -1 on a miss).  One World::hit_top per ray over
        [t_min, f32::MAX); media draw from the stream (seed, first_index + i).  stats=True: ((out, material), stats)."""
        return self._query("closest", 7, rays, seed, t_min, first_index, stream, stats, ((8, np.float32, "float32"), (None, np.uint32, "int32")))

    def occluded(self, rays, seed=1, t_min=0.001, first_index=0, stream=None, stats=False):
        """Is anything hit in [t_min, t_max)?  rays [n, 8]: (origin, direction, time, t_max); uint8 [n].  A ConstantMedium
        blocks with probability 1 - transmittance.  stats=True: (out, stats)."""
        return self._query("occluded", 8, rays, seed, t_min, first_index, stream, stats, ((None, np.uint8, "uint8"),))

    # ---- ray frames (include/rtiow_gpu_rays.h) -----------------------------------------------------------------------
    def cast_rays(self, rays, nx, ny, ns, per_sample=False, seed=0xDEADBEEF, max_bounces=50, flags=0, sample_begin=0, out=None,
                  background=None, rank=0, nranks=1, stream=None, t_near=0.001, tile_w=0, tile_h=0, stats=False):
        """Path-trace the caller's rays into a frame: float32 [ny, nx, 3] (row 0 = top), or [2, ny, nx, 3] with
        FLAG_SUM_SQUARES in `flags`.  rays: [nx * ny, 7] (origin, direction, time), ray p = row * nx + x starting every sample
        of pixel p; per_sample=True: [ns * nx * ny, 7], sample s of pixel p at s * nx * ny + p (rays.camera_rays makes the
        library's own camera rays in that layout).  A numpy array takes the host entry point and returns numpy; a torch
        tensor on the scene's device takes the device entry point on `stream` (default: the current torch stream) and returns
        a torch tensor, without a host round trip.
        flags: FLAG_PARTIAL / FLAG_RESUME (with sample_begin) / FLAG_SUM_SQUARES; out: the frame to continue or to write into
        (the same kind and shape as the result; rendered in place when it is contiguous and the call has no background).
        background= (FLAG_BACKGROUND): a colour, a dict of bottom / top, or a Background (make_background).
        rank / nranks / tile_w / tile_h: as in par_cast -- pixels of other ranks keep what `out` held.
        stats=True returns (frame, rtg_stats as a dict)."""
        mode = RAYS_PER_SAMPLE if per_sample else RAYS_PER_PIXEL
        n_rays = ray_index(nx, ny, ns if per_sample else 1, 0, 0, True)
        if _given(background):
            flags |= FLAG_BACKGROUND
        squares = bool(flags & FLAG_SUM_SQUARES)
        lay = FrameLayout(nx, ny, squares=squares, background=bool(flags & FLAG_BACKGROUND))
        shape = (2, ny, nx, 3) if squares else (ny, nx, 3)
        planes = (6 if squares else 3) * nx * ny
        p = make_params(nx, ny, ns, seed=seed, max_bounces=max_bounces, t_near=t_near, tile_w=tile_w, tile_h=tile_h, rank=rank,
                        nranks=nranks, flags=flags, sample_begin=sample_begin)
        block = make_background(background) if _given(background) and background is not True else None
        st = Stats.new() if stats else None
        st_arg = C.byref(st) if stats else None
        if hasattr(rays, "data_ptr"):
            import torch
            if not rays.is_cuda:
                raise ValueError("cast_rays: a torch tensor must live on the scene's device (pass a numpy array for host rays)")
            if rays.dtype != torch.float32 or not rays.is_contiguous():   # (no temporary copy: the call returns before the kernel reads it)
                raise ValueError("cast_rays: the rays must be a contiguous float32 tensor")
            if rays.numel() != 7 * n_rays:
                raise ValueError("cast_rays: %d floats of rays, expected %d x 7" % (rays.numel(), n_rays))
            if stream is None:
                stream = torch.cuda.current_stream(rays.device)
            in_place = out is not None and lay.words == planes and out.is_contiguous() and out.dtype == torch.float32
            if out is not None and tuple(out.shape) != shape:
                raise ValueError("cast_rays: out must have shape %r" % (shape,))
            with torch.cuda.stream(stream) if isinstance(stream, torch.cuda.Stream) else _no_context():
                buf = out.reshape(-1) if in_place else torch.zeros(lay.words, dtype=torch.float32, device=rays.device)
                if out is not None and not in_place:
                    buf[:planes].copy_(out.reshape(-1))
            if isinstance(stream, torch.cuda.Stream):
                buf.record_stream(stream)
            if block is not None:
                self._block_copy(buf, block, stream, True, 4 * lay.background, Background.OUT_OFFSET)
            self.be.check(self.be._par_cast_rays_device(self.h, _device_ptr(rays), mode, C.byref(p), _device_ptr(buf), _stream(stream), st_arg))
            res = out if in_place else buf[:planes].reshape(shape)
            if out is not None and not in_place:
                with torch.cuda.stream(stream) if isinstance(stream, torch.cuda.Stream) else _no_context():
                    out.copy_(res)
                res = out
        else:
            rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 7)
            if rays.shape[0] != n_rays:
                raise ValueError("cast_rays: %d rays, expected %d" % (rays.shape[0], n_rays))
            if out is not None and tuple(out.shape) != shape:
                raise ValueError("cast_rays: out must have shape %r" % (shape,))
            in_place = (out is not None and lay.words == planes and isinstance(out, np.ndarray) and out.dtype == np.float32
                        and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"])
            buf = out.reshape(-1) if in_place else np.zeros(lay.words, dtype=np.float32)
            if out is not None and not in_place:
                buf[:planes] = np.asarray(out, dtype=np.float32).reshape(-1)
            if block is not None:
                C.memmove(buf.ctypes.data + 4 * lay.background, C.addressof(block), C.sizeof(Background))
            self.be.check(self.be._par_cast_rays(self.h, rays.ctypes.data, mode, C.byref(p), buf.ctypes.data, st_arg))
            res = out if in_place else buf[:planes].reshape(shape)
            if out is not None and not in_place:
                out[...] = res
                res = out
        return (res, st.as_dict()) if stats else res

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
