"""The binding's call transcript: what capi.py hands to the library, and what it hands back to the caller, for every kind of
flagged frame -- compared with tests/golden/capi_transcript.json, which was recorded from the binding as it was before its frame
classes and call paths were merged.  No GPU: the library's render entry points are replaced by a stand-in that records the
params, the buffer's size and the buffer's bytes at entry, then fills the frame (block in-fields excepted) with a fixed pattern,
so that write-back shows; the HIP runtime of the device loops is replaced by one that records every copy and performs it on host
memory.

Run as a script, the module writes the fixture.  That is done with the capi.py of the commit BEFORE the one under test (this file
copied into a worktree of it, RTIOW_GPU_LIB naming a built library), never with the code under test."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_transcript.json")
SIZES = [(6, 5), (7, 5)]   # 30 pixels, and 35: an odd count puts the padding word in front of a block
COMBOS = [(sq, c, r, d, f) for f in (False, True) for sq in (False, True) for c in (False, True) for r in (False, True)
          for d in (False, True) if (not r or (c and sq)) and (not d or sq)]
PARAM_FIELDS = ("struct_size", "nx", "ny", "ns", "max_bounces", "t_near", "seed", "tile_w", "tile_h", "rank", "nranks", "flags",
                "sample_begin")
IN_WORDS = {"retire": 4, "denoise": 4, "features": 6}   # the in-fields of the 16-word blocks: the library never writes them


def sha(data):
    return hashlib.sha256(bytes(data)).hexdigest()[:16]


def sha_at(addr, nbytes):
    return sha(C.string_at(addr, nbytes))


def layout(n, flags):
    """Word offsets of a frame's parts from the flags of a call, as include/rtiow_gpu.h states them (the test's own copy)."""
    def even(w):
        return (w + 1) & ~1
    lay = {}
    w = (6 if flags & 16 else 3) * n
    if flags & 32:
        lay["counts"] = w
        w += n
    if flags & 64:
        lay["retire"] = w = even(w)
        w += 16
    if flags & 128:
        lay["denoise"] = w = even(w)
        w += 16 + 3 * n
    if flags & 256:
        lay["features"] = w = even(w)
        w += 16 + 7 * n
    lay["end"] = w
    return lay


def val(x):
    return getattr(x, "value", x) or 0


class Recorder:
    """The stand-in library and HIP runtime: one log of every call, in order."""

    def __init__(self, capi):
        self.capi = capi
        self.log = []
        self.device = {}   # name -> uint32 array standing in for a device buffer

    def device_buffer(self, name, words):
        self.device[name] = np.zeros(words, np.uint32)
        return self.device[name].ctypes.data

    def where(self, addr, nbytes=0):
        for name, a in self.device.items():
            if a.ctypes.data <= addr and addr + nbytes <= a.ctypes.data + a.nbytes:
                return [name, addr - a.ctypes.data]
        return None

    def _render(self, fn, p, addr, room, st, extra):
        k = sum(1 for e in self.log if e[0] in ("par_cast", "par_cast_multi", "par_cast_device"))
        n = p.nx * p.ny
        lay = layout(n, p.flags)
        nbytes = lay["end"] * 4
        self.log.append([fn, [getattr(p, name) for name in PARAM_FIELDS], room, sha_at(addr, min(room, nbytes)),
                         None if st is None else st.struct_size] + extra)
        if room < nbytes:   # (a frame too small for the call's flags: recorded above, never written)
            return -1
        words = np.frombuffer((C.c_uint32 * lay["end"]).from_address(addr), np.uint32)
        keep = [(lay[b], words[lay[b]:lay[b] + IN_WORDS[b]].copy()) for b in IN_WORDS if b in lay]
        i = np.arange(lay["end"], dtype=np.int64)
        words[:] = (((i * 7 + k * 3) % 64).astype(np.float32) * np.float32(0.25)).view(np.uint32)
        if "counts" in lay:
            words[lay["counts"]:lay["counts"] + n] = (np.arange(n) + k) % 4 + k
        for at, saved in keep:
            words[at:at + len(saved)] = saved
        if st is not None:
            st.kernel_ms = 1.5
            for j, (name, _) in enumerate(self.capi.Stats._fields_[2:]):
                setattr(st, name, 100 * k + j)
        return 0

    def par_cast(self, h, cam, p, out, st, *more):
        a = out._arr
        while isinstance(a.base, np.ndarray):
            a = a.base
        addr = C.cast(out, C.c_void_p).value
        return self._render("par_cast", p._obj, addr, a.ctypes.data + a.nbytes - addr, st._obj, [len(more)])

    def par_cast_multi(self, arr, n, cam, p, out, st):
        a = out._arr
        while isinstance(a.base, np.ndarray):
            a = a.base
        addr = C.cast(out, C.c_void_p).value
        return self._render("par_cast_multi", p._obj, addr, a.ctypes.data + a.nbytes - addr, st._obj, [n, len(arr)])

    def par_cast_device(self, h, cam, p, d_out, stream, st):
        addr = val(d_out)
        at = self.where(addr)
        assert at is not None, "par_cast_device on an address outside the stand-in device buffers"
        a = self.device[at[0]]
        return self._render("par_cast_device", p._obj, addr, a.nbytes - at[1], None if st is None else st._obj, [at, val(stream)])

    # the HIP runtime
    def hipMemcpyAsync(self, dst, src, n, kind, stream):
        d, s = val(dst), val(src)
        dev_d, dev_s = self.where(d, n), self.where(s, n)
        self.log.append(["memcpy", kind, dev_d, dev_s, n, sha_at(s, n) if kind == 1 else None, val(stream)])
        assert (dev_d is not None or kind == 2) and (dev_s is not None or kind == 1), "a copy outside the stand-in device buffers"
        C.memmove(d, s, n)
        return 0

    def hipMemsetD32Async(self, dst, value, count, stream):
        d = val(dst)
        at = self.where(d, 4 * count)
        self.log.append(["memset", at, value, count, val(stream)])
        assert at is not None, "a memset outside the stand-in device buffers"
        np.frombuffer((C.c_uint32 * count).from_address(d), np.uint32)[:] = value & 0xFFFFFFFF
        return 0

    def hipStreamSynchronize(self, stream):
        self.log.append(["sync", val(stream)])
        return 0


@contextlib.contextmanager
def stand_ins(capi, be):
    rec = Recorder(capi)
    saved = (be._par_cast, be._par_cast_multi, be._par_cast_device, capi._hip_runtime)
    be._par_cast, be._par_cast_multi, be._par_cast_device = rec.par_cast, rec.par_cast_multi, rec.par_cast_device
    capi._hip_runtime = lambda: rec
    try:
        yield rec
    finally:
        be._par_cast, be._par_cast_multi, be._par_cast_device, capi._hip_runtime = saved


class _Handle:
    h = None


class _Stream:
    cuda_stream = 7


def plain(capi, x):
    """`x` as JSON: arrays, frames and blocks as hashes, floats as their repr."""
    if isinstance(x, np.ndarray):
        return ["array", list(x.shape), str(x.dtype), sha(np.ascontiguousarray(x).tobytes())]
    if isinstance(x, (capi.CountsFrame, capi.DenoiseFrame, capi.FeaturesFrame)):
        return [type(x).__name__, x.buf.nbytes, sha(x.buf.tobytes())]
    if isinstance(x, C.Structure):
        return [type(x).__name__, sha(C.string_at(C.addressof(x), C.sizeof(x)))]
    if isinstance(x, dict):
        return {k: plain(capi, v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [plain(capi, v) for v in x]
    if isinstance(x, (float, np.floating)):
        return repr(float(x))
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    return x


def caller_arrays(capi, nx, ny, sq, c, r):
    """out / counts / retire as a caller would hold them, with contents that show in a hash (the Retire's out-fields too)."""
    n = nx * ny
    own = {"out": (np.arange((6 if sq else 3) * n, dtype=np.float32) * np.float32(0.5)).reshape((2, ny, nx, 3) if sq else (ny, nx, 3))}
    if c:
        own["counts"] = (np.arange(n, dtype=np.uint32) % 7).reshape(ny, nx)
    if r:
        own["retire"] = capi.Retire(target_se=0.125, min_samples=2, radius=1, active=9, retired=8, samples_held=77)
    return own


def run_call(capi, rec, call, own, refused=False):
    """One case: `call(**own)` with the caller's objects `own`, recorded."""
    before = plain(capi, own)
    start = len(rec.log)
    try:
        ret = call(**own)
    except Exception as e:   # (the wording is the other suites' business)
        assert refused, repr(e)
        assert rec.log[start:] == [], "a refused call reached the library"
        assert plain(capi, own) == before, "a refused call wrote to the caller's objects"
        return {"raises": type(e).__name__}
    assert not refused
    stats = None
    if isinstance(ret, tuple):
        ret, stats = ret
    return {"calls": plain(capi, rec.log[start:]), "returns": plain(capi, ret), "stats": plain(capi, stats),
            "same": [k for k, v in own.items() if v is ret], "after": plain(capi, own)}


def transcript(pkg):
    capi = pkg.capi
    be = pkg.load()
    cam = capi.Camera()
    t = {}
    with stand_ins(capi, be) as rec:
        sc = capi.Scene(be, None, None)
        scenes = [_Handle(), _Handle()]
        entries = {"scene": lambda nx, ny, ns, **kw: sc.par_cast(cam, nx, ny, ns, seed=11, **kw),
                   "multi": lambda nx, ny, ns, **kw: be.par_cast_multi(scenes, cam, nx, ny, ns, seed=11, **kw)}
        dn, ft = {"k": 0.5, "radius": 2, "patch": 1}, {"grid": 3, "sigma_albedo": 0.5}
        for (nx, ny), combo, (entry, cast) in [(s, c, e) for s in SIZES for c in COMBOS for e in entries.items()]:
            sq, c, r, d, f = combo
            name = "%dx%d %s %s" % (nx, ny, "".join(ch for ch, on in zip("SCRDF", combo) if on) or "-", entry)
            kw = dict({"squares": sq, "partial": True}, **({"denoise": dn} if d else {}), **({"features": ft} if f else {}))
            # caller arrays: through a staging frame as soon as the call has a count plane or a block
            t[name + " arrays"] = run_call(capi, rec, lambda **own: cast(nx, ny, 4, **own, **kw), caller_arrays(capi, nx, ny, sq, c, r))
            # a frame object, rendered in place (Scene.par_cast takes a CountsFrame as its views)
            arrays = caller_arrays(capi, nx, ny, sq, c, r)
            if f:
                frame = capi.features_frame(nx, ny, sq, c, r, True if d else None)
            elif d:
                frame = capi.denoise_frame(nx, ny, c, r)
            elif c:
                frame = capi.counts_frame(nx, ny, sq, r)
            else:
                continue
            frame.planes[...] = arrays["out"]
            if c:
                frame.counts[...] = arrays["counts"]
            if r:
                frame.retire.target_se, frame.retire.min_samples, frame.retire.radius, frame.retire.active = 0.125, 2, 1, 9
            if isinstance(frame, capi.CountsFrame) and entry == "scene":
                views = dict({"out": frame.planes, "counts": frame.counts}, **({"retire": frame.retire} if r else {}))
                res = run_call(capi, rec, lambda **own: cast(nx, ny, 4, **own, **kw), views)
                res["frame"] = plain(capi, frame)
            else:
                res = run_call(capi, rec, lambda **own: cast(nx, ny, 4, **own, **kw), {"out": frame})
            t[name + " frame"] = res
        nx, ny = SIZES[0]
        n = nx * ny
        for entry, cast in entries.items():
            for counters in (None, True, False):
                t["stats counters=%s %s" % (counters, entry)] = run_call(
                    capi, rec, lambda **own: cast(nx, ny, 4, stats=True, counters=counters, **own), {"out": np.zeros((ny, nx, 3), np.float32)})
            t["stats no out " + entry] = run_call(capi, rec, lambda **own: cast(nx, ny, 4, stats=True, **own), {})
            t["resume with out " + entry] = run_call(capi, rec, lambda **own: cast(nx, ny, 4, resume=True, sample_begin=2, **own),
                                                     {"out": np.ones((ny, nx, 3), np.float32)})
            t["resume without out " + entry] = run_call(capi, rec, lambda **own: cast(nx, ny, 4, resume=True, sample_begin=2, **own), {}, refused=True)
            t["resume without out, features " + entry] = run_call(
                capi, rec, lambda **own: cast(nx, ny, 4, resume=True, sample_begin=2, features=ft, **own), {}, refused=True)
            t["resume with out, features " + entry] = run_call(
                capi, rec, lambda **own: cast(nx, ny, 4, resume=True, sample_begin=2, features=ft, **own), {"out": np.ones((ny, nx, 3), np.float32)})
            # refusals: nothing reaches the library, nothing of the caller's is written
            t["wrong-size frame " + entry] = run_call(
                capi, rec, lambda **own: cast(nx, ny, 4, squares=True, features=True, denoise=True, **own),
                {"out": capi.features_frame(nx + 1, ny, squares=True, denoise=True)}, refused=True)
            t["wrong-shape counts " + entry] = run_call(
                capi, rec, lambda **own: cast(nx, ny, 4, squares=True, **own),
                {"out": np.ones((2, ny, nx, 3), np.float32), "counts": np.ones((ny, nx + 1), np.uint32)}, refused=True)
            t["wrong-shape counts, denoise " + entry] = run_call(
                capi, rec, lambda **own: cast(nx, ny, 4, squares=True, denoise=dn, **own),
                {"out": np.ones((2, ny, nx, 3), np.float32), "counts": np.ones((ny + 1, nx), np.uint32)}, refused=True)
            t["retire without squares " + entry] = run_call(
                capi, rec, lambda **own: cast(nx, ny, 4, **own), caller_arrays(capi, nx, ny, False, True, True), refused=True)
            t["denoise without squares " + entry] = run_call(
                capi, rec, lambda **own: cast(nx, ny, 4, denoise=dn, **own), caller_arrays(capi, nx, ny, False, True, False), refused=True)
        # par_cast_multi alone: plain flags beside a plain array are the library's to answer, forwarded as they are
        t["forwarded flags multi"] = run_call(capi, rec, lambda **own: entries["multi"](nx, ny, 4, counts=True, features=True, **own),
                                              {"out": np.ones((8 * ny, nx, 3), np.float32)})
        # the host loops: two slices each
        for label, more in (("plain", {}), ("denoise", {"denoise": dn}), ("denoise features", {"denoise": dn, "features": ft})):
            start = len(rec.log)
            items = list(sc.progressive(cam, nx, ny, 4, 2, seed=11, **more))
            t["progressive host " + label] = {"calls": plain(capi, rec.log[start:]), "yields": plain(capi, items)}
            start, stats = len(rec.log), []
            items = list(sc.adaptive(cam, nx, ny, 4, 2, 0.05, min_samples=2, seed=11, stats=stats, radius=1, **more))
            t["adaptive host " + label] = {"calls": plain(capi, rec.log[start:]), "yields": plain(capi, items), "stats": plain(capi, stats)}
            start = len(rec.log)
            items = list(be.adaptive_multi(scenes, cam, nx, ny, 4, 2, 0.05, min_samples=2, seed=11, **more))
            t["adaptive_multi host " + label] = {"calls": plain(capi, rec.log[start:]), "yields": plain(capi, items)}
        # the device loops, on host memory behind the stand-in runtime
        for label, more in (("plain", {}), ("denoise", {"denoise": dn}), ("denoise features", {"denoise": dn, "features": ft})):
            for loop in ("progressive", "adaptive"):
                out, preview, denoised = (rec.device_buffer(name, 24 * n + 64) for name in ("out", "preview", "denoised"))
                if more:
                    more = dict(more, denoised=denoised)
                start, stats = len(rec.log), []
                if loop == "progressive":
                    items = list(sc.progressive(cam, nx, ny, 4, 2, seed=11, out=out, preview=preview, stream=_Stream(), **more))
                else:
                    items = list(sc.adaptive(cam, nx, ny, 4, 2, 0.05, min_samples=2, seed=11, stats=stats, radius=1, out=out, preview=preview,
                                             stream=_Stream(), **more))
                items = [[rec.where(v) or v if isinstance(v, int) and v > 1 << 20 else v for v in item] for item in items]
                t["%s device %s" % (loop, label)] = {"calls": plain(capi, rec.log[start:]), "yields": plain(capi, items), "stats": plain(capi, stats),
                                                     "buffers": plain(capi, [rec.device[k] for k in ("out", "preview", "denoised")])}
        start = len(rec.log)
        out, preview = rec.device_buffer("out", 24 * n + 64), rec.device_buffer("preview", 4 * n)
        items = list(sc.progressive(cam, nx, ny, 4, 2, seed=11, out=out, preview=preview, squares=True, budget_s=1e9))
        t["progressive device squares budget"] = {"calls": plain(capi, rec.log[start:]), "yields": len(items)}
        # par_cast_device: no override (the caller's own Params reach the library), and one block each
        out = rec.device_buffer("out", 24 * n + 64)
        own_params = []

        def spy(h, cam_, p, d_out, stream, st):
            own_params.append(p._obj)
            return rec.par_cast_device(h, cam_, p, d_out, stream, st)
        be._par_cast_device = spy
        params = capi.make_params(nx, ny, 4, seed=11)
        start = len(rec.log)
        assert sc.par_cast_device(cam, params, out) is None and own_params[-1] is params
        t["par_cast_device plain"] = {"calls": plain(capi, rec.log[start:])}
        blocks = {"retire": (capi.Retire(target_se=0.125, min_samples=2, radius=1, active=9), dict(squares=True, counts=True)),
                  "denoise": (capi.make_denoise(dn), dict(squares=True)), "features": (capi.make_features(ft), {})}
        for part, (block, flags) in blocks.items():
            start = len(rec.log)
            st = sc.par_cast_device(cam, capi.make_params(nx, ny, 4, seed=11, **flags), out, 7, want_stats=True, **{part: block})
            t["par_cast_device " + part] = {"calls": plain(capi, rec.log[start:]), "stats": plain(capi, st), "block": plain(capi, block)}
        start = len(rec.log)
        counts = (np.arange(n, dtype=np.uint32) % 5).reshape(ny, nx)
        sc.par_cast_device(cam, params, out, counts=counts, squares=True, sample_begin=2, resume=True, partial=False,
                           retire=blocks["retire"][0], denoise=blocks["denoise"][0], features=True)
        # (the three block copies touch disjoint words and each waits for its own: their order among themselves is free)
        calls = plain(capi, rec.log[start:])
        at = [i for i, e in enumerate(calls) if e[0] == "par_cast_device"][0]
        t["par_cast_device overrides"] = {"before": sorted(calls[:at], key=json.dumps), "call": calls[at], "after": sorted(calls[at + 1:], key=json.dumps)}
    return t


@pytest.fixture(scope="module")
def pair(pkg):
    return transcript(pkg), json.load(open(GOLDEN))


def test_every_case_is_recorded(pair):
    got, want = pair
    assert sorted(got) == sorted(want)
    assert len([k for k in got if k.endswith(" arrays")]) == len(SIZES) * 16 * 2
    assert len([k for k in got if k.endswith(" frame")]) == len(SIZES) * 14 * 2   # (no frame class without a count plane or a block)


def test_transcript_is_the_recorded_one(pair):
    got, want = pair
    got = json.loads(json.dumps(got))
    different = [k for k in want if got.get(k) != want[k]]
    for k in different[:3]:
        print(k, "\n  recorded:", json.dumps(want[k]), "\n  now:     ", json.dumps(got.get(k)))
    assert different == []


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    cases = transcript(graft.load_package())
    with open(GOLDEN, "w") as fh:   # one case per line
        fh.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(cases[k], sort_keys=True, separators=(",", ":")))
                                    for k in sorted(cases)) + "\n}\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
