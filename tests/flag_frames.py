"""The flagged frames of test_flag_frames_gpu.py, shared with tools/gen_flag_frame_digests.py: one small frame, every legal
combination of (squares, counts, retire, denoise, features, error), rendered whole and as two slices through rtg_par_cast,
rtg_par_cast_device and rtg_par_cast_multi, and the SHA-256 of every 32-bit word the call leaves in the frame."""
import ctypes as C
import hashlib
import itertools

import numpy as np

from scene_cases import CASES

NX, NY, NS, CUT, SEED = 23, 17, 5, 2, 0x5EED1234   # n = 391 is odd: so are 3n and 7n, and every even-word rounding bites
RETIRE = {"target_se": 0.05, "min_samples": 2, "radius": 1}
DENOISE = {"k": 0.7, "radius": 2, "patch": 1}
FEATURES = {"grid": 2, "compute": 1}
PARTS = ("squares", "counts", "retire", "denoise", "features", "error")
# retire needs squares and counts, denoise needs squares, error needs denoise
COMBOS = [c for c in itertools.product((0, 1), repeat=6)
          if not (c[2] and not (c[0] and c[1])) and not (c[3] and not c[0]) and not (c[5] and not c[3])]
SETUPS = {"book1": ("book1", {}), "cornell": ("cornell", {}), "book1_baseline": ("book1", {"kernel": 1})}
PATHS = ("par_cast", "par_cast_device", "par_cast_multi")
WAYS = {"whole": [(NS, {})], "slices": [(CUT, {"partial": True}), (NS, {"sample_begin": CUT, "resume": True})]}


def count_plane():
    """n_p = (7x + 3y) % 7: zeros, values below ns and values above it."""
    y, x = np.mgrid[0:NY, 0:NX]
    return ((7 * x + 3 * y) % 7).astype(np.uint32)


def combo_name(combo):
    return "+".join(p for p, on in zip(PARTS, combo) if on) or "plain"


def make_frame(capi, combo):
    """The frame of the combination's layout, every word 0.25, then the count plane and the blocks' in-fields."""
    squares, counts, retire, denoise, features, error = map(bool, combo)
    f = capi.Frame(NX, NY, squares, counts, retire, DENOISE if denoise else None, FEATURES if features else None, error)
    f.buf[...] = 0.25
    if counts:
        f.counts[...] = count_plane()
    if retire:
        block = capi.Retire()
        block.target_se, block.min_samples, block.radius = RETIRE["target_se"], RETIRE["min_samples"], RETIRE["radius"]
        f.set_in(block)
    if denoise:
        f.set_in(capi.make_denoise(DENOISE))
    if features:
        f.set_in(capi.make_features(FEATURES))
    return f


def make_scenes(pkg, gpu, setup, path):
    """The handle(s) of a set-up for a path, and the camera: two handles on device 0 for rtg_par_cast_multi, multi_planes on."""
    name, options = SETUPS[setup]
    scenes, cam = [], None
    for _ in range(2 if path == "par_cast_multi" else 1):
        b = gpu.builder()
        world, cam, _ = CASES[name][0](pkg, b, NX, NY)
        sg = b.scene(world, device=0)
        for k, v in options.items():
            sg.set_option(k, v)
        scenes.append(sg)
    if path == "par_cast_multi":
        scenes[-1].set_option("multi_planes", 1)
    return scenes, cam


def _call(pkg, gpu, scenes, cam, path, p, f):
    """One library call on the frame, in place; the device path through a device copy of the whole frame."""
    capi = pkg.capi
    if path == "par_cast":
        sg = scenes[0]
        st = capi.Stats.new()
        gpu.check(gpu._par_cast(sg.h, capi.C.byref(cam), capi.C.byref(p), f.buf.ctypes.data_as(capi.c_f32p), capi.C.byref(st)))
    elif path == "par_cast_multi":
        gpu._par_cast_multi_call(scenes, cam, p, f.buf)
    else:
        dev = _device_frame(f.buf.nbytes)
        hip = dev.hip
        assert hip.hipMemcpy(dev.p, f.buf.ctypes.data, f.buf.nbytes, 1) == 0
        try:
            scenes[0].par_cast_device(cam, p, dev.p.value)
        finally:   # (a refused call has enqueued nothing; the copy waits for an accepted one on the default stream)
            assert hip.hipMemcpy(f.buf.ctypes.data, dev.p, f.buf.nbytes, 2) == 0


class _DeviceFrame:
    """hipMalloc'ed bytes, kept for the process and grown on demand."""
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.p, self.nbytes = C.c_void_p(), 0


_DEV = None


def _device_frame(nbytes):
    global _DEV
    if _DEV is None:
        _DEV = _DeviceFrame()
    if nbytes > _DEV.nbytes:
        if _DEV.nbytes:
            _DEV.hip.hipFree(_DEV.p)
        assert _DEV.hip.hipMalloc(C.byref(_DEV.p), nbytes) == 0
        _DEV.nbytes = nbytes
    return _DEV


def digests(pkg, gpu, setup, path):
    """{"<combination>/<way>": [digest after each call, or "error <code>" where the library refuses the call]}."""
    capi = pkg.capi
    scenes, cam = make_scenes(pkg, gpu, setup, path)
    out = {}
    for combo in COMBOS:
        flags = dict(zip(PARTS, map(bool, combo)))
        for way, calls in WAYS.items():
            f = make_frame(capi, combo)
            got = []
            for ns, kw in calls:
                p = capi.make_params(NX, NY, ns, seed=SEED, **flags, **kw)
                try:
                    _call(pkg, gpu, scenes, cam, path, p, f)
                    got.append(hashlib.sha256(f.buf.tobytes()).hexdigest())
                except capi.RtError as e:
                    got.append("error %d" % e.code)
            out["%s/%s" % (combo_name(combo), way)] = got
    return out
