"""Ray queries on the GPU (include/rtiow_gpu_query.h; Scene.closest_hit / Scene.occluded): closest hits against the oracle's
and the GPU's own debug_hit_top, bit for bit and material for material, on both kernels; sizes, splits and first_index;
occlusion against the closest hit's t (exact identities, and the one-sided rule where a box test may round differently);
media (a binomial bound on the blocked share, surfaces behind media); the device path on torch tensors and streams; refusals."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from probe_rays import probe_rays
from scene_cases import CASES, build_case

pytestmark = pytest.mark.gpu

SEED, T_MIN = 77, 0.001
F32_MAX = np.float32(3.402823466e+38)
ERR_INVALID = -1
CAP = 0.001   # of the rays with a hit: rays on which a box test with end = t_max may round differently from one with end = best
CLOSEST_CASES = ["cornell", "book1", "book2", "volume_bvh", "checker_scale", "motion", "book1_sah", "big_lean", "cornell_smoke"]

_scenes, _oracle_hits = {}, {}


def scene_of(pkg, gpu, name):
    if name not in _scenes:
        _scenes[name] = build_case(pkg, gpu, name)[0]
    _scenes[name].set_option("query_lds", 1)
    return _scenes[name]


def rays_of(name):
    return probe_rays(name, n_random=512, seed=99)


def oracle_hits(pkg, oracle, name, rays=None, key=None):
    """The oracle's debug_hit_top for the case's rays: computed once, shared, never written to."""
    k = (name, key)
    if k not in _oracle_hits:
        out, mat = build_case(pkg, oracle, name)[0].debug_hit_top(rays_of(name) if rays is None else rays, seed=SEED, t_near=T_MIN)
        out.setflags(write=False), mat.setflags(write=False)
        _oracle_hits[k] = (out, mat)
    return _oracle_hits[k]


def with_t_max(rays, t_max):
    return np.concatenate([rays, np.broadcast_to(np.asarray(t_max, np.float32), (len(rays),))[:, None]], axis=1).astype(np.float32)


# ---- 1. closest, against the oracle --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CLOSEST_CASES)
def test_closest_equals_the_oracle_and_debug_hit_top(pkg, gpu, oracle, name):
    sc, rays = scene_of(pkg, gpu, name), rays_of(name)
    want, want_mat = oracle_hits(pkg, oracle, name)
    own, own_mat = sc.debug_hit_top(rays, seed=SEED, t_near=T_MIN)
    got, got_mat = sc.closest_hit(rays, seed=SEED, t_min=T_MIN)
    assert got.dtype == np.float32 and got.shape == (len(rays), 8) and got_mat.dtype == np.uint32
    assert_bit_equal(got, want, name + ": closest_hit vs the oracle")
    assert_bit_equal(got, own, name + ": closest_hit vs debug_hit_top")
    assert (got_mat == want_mat).all() and (got_mat == own_mat).all()
    assert ((got[:, 0] == 0) == (got_mat == 0xffffffff)).all()
    if name in ("book1", "book1_sah"):
        res = {}
        for lds in (0, 2):
            sc.set_option("query_lds", lds)
            res[lds] = sc.closest_hit(rays, seed=SEED, t_min=T_MIN)
            assert_bit_equal(res[lds][0], want, "%s: query_lds %d vs the oracle" % (name, lds))
        assert res[0][0].tobytes() == res[2][0].tobytes() and res[0][1].tobytes() == res[2][1].tobytes()


# ---- 2. sizes and splits -------------------------------------------------------------------------------------------------

N_BIG = 4096 + 37


def test_sizes_and_splits_on_the_lean_kernel(pkg, gpu, oracle):
    sc = scene_of(pkg, gpu, "book1")
    rays = probe_rays("book1", n_random=4200, seed=5)[:N_BIG]
    want, want_mat = oracle_hits(pkg, oracle, "book1", rays, "sizes")
    sc.set_option("query_lds", 2)
    for n in (0, 1, 63, 64, 65, N_BIG):   # the last: more than one workgroup, and lanes that take a second ray
        got, mat = sc.closest_hit(rays[:n], seed=SEED, t_min=T_MIN)
        assert got.shape == (n, 8) and mat.shape == (n,)
        assert_bit_equal(got, want[:n], "book1, %d rays" % n)
        assert (mat == want_mat[:n]).all()
        occ = sc.occluded(with_t_max(rays[:n], F32_MAX), seed=SEED, t_min=T_MIN)
        assert occ.dtype == np.uint8 and occ.shape == (n,) and (occ == (want[:n, 0] != 0)).all()
    a, am = sc.closest_hit(rays[:1000], seed=SEED, t_min=T_MIN)
    b, bm = sc.closest_hit(rays[1000:], seed=SEED, t_min=T_MIN, first_index=1000)
    assert_bit_equal(np.concatenate([a, b]), want, "book1: two calls split at 1000")
    assert (np.concatenate([am, bm]) == want_mat).all()


def test_splits_on_a_world_with_media(pkg, gpu, oracle):
    """volume: a ConstantMedium in a list world (the general kernel).  The draws are keyed by first_index + i, so the split
    gives the bits of one call -- and the second half asked with first_index = 0 does not."""
    sc = scene_of(pkg, gpu, "volume")
    rays = probe_rays("volume", n_random=2048, seed=5)
    want, want_mat = oracle_hits(pkg, oracle, "volume", rays, "split")
    one, one_mat = sc.closest_hit(rays, seed=SEED, t_min=T_MIN)
    assert_bit_equal(one, want, "volume: one call vs the oracle")
    assert (one_mat == want_mat).all()
    a, am = sc.closest_hit(rays[:1000], seed=SEED, t_min=T_MIN)
    b, bm = sc.closest_hit(rays[1000:], seed=SEED, t_min=T_MIN, first_index=1000)
    assert_bit_equal(np.concatenate([a, b]), want, "volume: two calls split at 1000")
    assert (np.concatenate([am, bm]) == want_mat).all()
    c, _ = sc.closest_hit(rays[1000:], seed=SEED, t_min=T_MIN)
    assert c.tobytes() != b.tobytes()
    r8 = with_t_max(rays, F32_MAX)
    occ = sc.occluded(r8, seed=SEED, t_min=T_MIN)
    halves = np.concatenate([sc.occluded(r8[:1000], seed=SEED, t_min=T_MIN), sc.occluded(r8[1000:], seed=SEED, t_min=T_MIN, first_index=1000)])
    assert occ.tobytes() == halves.tobytes()


# ---- 3. occlusion without media ------------------------------------------------------------------------------------------

def _t_max_sets(ts, seed):
    rs = np.random.RandomState(seed)
    with np.errstate(over="ignore"):
        return {"max": np.full(len(ts), F32_MAX), "at": ts, "half": (np.float32(0.5) * ts).astype(np.float32),
                "two": (np.float32(2.0) * ts).astype(np.float32),
                "random": (rs.uniform(0.0, 4.0, len(ts)).astype(np.float32) * ts).astype(np.float32)}


@pytest.mark.parametrize("name", ["cornell", "book1_list", "checker_scale"])
def test_occluded_on_list_worlds_is_exact(pkg, gpu, oracle, name):
    """occluded == (hit and t* < t_max), exactly -- for every ray but the three edge rays of probe_rays that lie IN the plane of a
    Cornell wall.  Such a ray hits that wall with t = 0 / 0 = NaN: Rect::hit's range test is two comparisons, both false for a
    NaN, so the reference accepts the hit, and so do hit_top and occluded.  From then on the closest walk's range end is NaN and
    every later object the line meets replaces the hit, whatever its t: t* is the LAST such object's t (or NaN), not the smallest,
    and `t* < t_max` says nothing about what lies in front of t_max (on checker_scale one of the three ends on an added sphere
    with a wall's finite t in front of it).  For these rays, picked by their geometry alone, the test asks what the predicates
    do give: the hit flag at t_max = F32_MAX (as on the Bvh worlds, and as the rule for surfaces behind media demands of the
    same walls), 0 where t_max is NaN, and occluded => hit everywhere."""
    sc, rays = scene_of(pkg, gpu, name), rays_of(name)
    want, _ = oracle_hits(pkg, oracle, name)
    hit, ts = want[:, 0] != 0, want[:, 1].copy()
    in_plane = np.zeros(len(rays), bool)
    if name != "book1_list":   # (book-1 has no rect)
        for axis in range(3):
            in_plane |= (rays[:, 3 + axis] == 0) & np.isin(rays[:, axis], np.float32([0.0, 554.0, 555.0])) & (np.abs(rays[:, 3:6]).sum(axis=1) > 0)
        assert in_plane.sum() == 3
    assert not np.isnan(ts[~in_plane]).any() and (hit & ~in_plane).sum() > 300
    for label, t_max in _t_max_sets(ts, 11).items():
        occ = sc.occluded(with_t_max(rays, t_max), seed=SEED, t_min=T_MIN).astype(bool)
        with np.errstate(invalid="ignore"):
            expect = hit & (ts < t_max)
        bad = (occ != expect) & ~in_plane
        assert not bad.any(), (name, label, int(bad.sum()))
        assert not (occ & ~hit).any()
        if label == "max":
            assert (occ == hit).all()
        assert not occ[np.isnan(t_max)].any()


@pytest.mark.parametrize("name,lds", [("book1", 0), ("book1", 2), ("book1_sah", 1), ("big_lean", 1)])
def test_occluded_on_bvh_worlds(pkg, gpu, oracle, name, lds):
    sc, rays = scene_of(pkg, gpu, name), rays_of(name)
    sc.set_option("query_lds", lds)
    want, _ = oracle_hits(pkg, oracle, name)
    hit, ts = want[:, 0] != 0, want[:, 1].copy()
    sets = _t_max_sets(ts, 11)
    occ = {k: sc.occluded(with_t_max(rays, sets[k]), seed=SEED, t_min=T_MIN) for k in ("max", "at", "half", "two")}
    assert (occ["max"] == hit).all()
    assert not occ["at"].any()
    assert not occ["half"][ts > 0].any()
    expect = hit & (ts < sets["two"])
    assert not (occ["two"].astype(bool) & ~expect).any()          # occluded => t* < t_max, for every ray
    missed = int((expect & ~occ["two"].astype(bool)).sum())       # the converse: a box test rounded differently
    print("%s query_lds %d: %d of %d rays with a hit miss the converse" % (name, lds, missed, int(hit.sum())))
    assert missed <= CAP * hit.sum()


def test_t_max_nan_or_not_above_t_min_gives_zero(pkg, gpu):
    rays = rays_of("book1")[:256]
    t_max = np.resize(np.float32([np.nan, T_MIN, 0.0, -1.0, -np.inf, np.float32(T_MIN) * np.float32(0.5)]), len(rays))
    for name, lds in (("book1", 0), ("book1", 2), ("cornell", 1)):
        sc = scene_of(pkg, gpu, name)
        sc.set_option("query_lds", lds)
        assert not sc.occluded(with_t_max(rays_of(name)[:256], t_max), seed=SEED, t_min=T_MIN).any()


# ---- 4. occlusion with media ---------------------------------------------------------------------------------------------

def test_one_medium_blocks_its_share(pkg, gpu):
    """One ConstantMedium, a sphere of radius 50 and density 0.02; 65 536 rays through its centre from outside, t_max beyond
    it.  Each ray is blocked with probability p = 1 - exp(-0.02 x 100): the blocked share is a binomial mean, and the bound is
    five of its standard deviations (the chord's float32 length differs from 100 by parts in 1e7: far below the bound)."""
    S = pkg.scenes
    b = gpu.builder()
    boundary = b.sphere(50.0, b.lambertian(b.constant(S.vfrom(0.5))))
    sc = b.scene([b.constant_medium(boundary, 0.02, b.isotropic(b.constant(S.vfrom(1.0))))])
    n = 65536
    rs = np.random.RandomState(3)
    u = rs.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    rays = np.concatenate([200.0 * u, -u, np.full((n, 1), 0.5), np.full((n, 1), 1000.0)], axis=1).astype(np.float32)
    occ = sc.occluded(rays, seed=SEED, t_min=T_MIN)
    p = 1.0 - np.exp(-0.02 * 100.0)
    share, bound = occ.mean(), 5.0 * np.sqrt(p * (1.0 - p) / n)
    print("blocked share %.5f, p %.5f, bound %.5f" % (share, p, bound))
    assert abs(share - p) <= bound
    assert set(np.unique(occ)) <= {0, 1}
    assert sc.occluded(rays, seed=SEED, t_min=T_MIN).tobytes() == occ.tobytes()
    assert sc.occluded(rays, seed=SEED + 1, t_min=T_MIN).tobytes() != occ.tobytes()   # (another seed: other draws)


@pytest.mark.parametrize("name", ["volume", "book2", "cornell_smoke"])
def test_a_surface_behind_media_still_occludes(pkg, gpu, oracle, name):
    """t_max = F32_MAX: a ray whose closest hit (the oracle's) is a surface -- a material that is no medium's phase material --
    meets that surface in the any-hit walk too, whatever the media on the way draw."""
    ob = oracle.builder()
    phase, make = [], ob.isotropic
    ob.isotropic = lambda albedo: (phase.append(make(albedo)), phase[-1])[1]
    fn, nx, ny, _ = CASES[name]
    world = fn(pkg, ob, nx, ny)[0]
    rays = rays_of(name)
    want, want_mat = ob.scene(world).debug_hit_top(rays, seed=SEED, t_near=T_MIN)
    assert phase, name
    surface = (want[:, 0] != 0) & ~np.isin(want_mat, phase)
    assert surface.sum() > 100, name
    occ = scene_of(pkg, gpu, name).occluded(with_t_max(rays, F32_MAX), seed=SEED, t_min=T_MIN)
    assert occ[surface].all(), (name, int((~occ[surface].astype(bool)).sum()))


# ---- 5. the device path --------------------------------------------------------------------------------------------------

class Hip:
    """The HIP runtime the library links, through ctypes: device arrays and streams of the test's own."""

    def __init__(self):
        h = self.lib = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipFree.argtypes = [C.c_void_p]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        h.hipStreamSynchronize.argtypes = [C.c_void_p]
        h.hipStreamDestroy.argtypes = [C.c_void_p]
        self.held = []

    def array(self, host):
        host = np.ascontiguousarray(host)
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), max(host.nbytes, 16)) == 0
        assert self.lib.hipMemcpy(p, host.ctypes.data, host.nbytes, 1) == 0
        self.held.append(p)
        return p.value

    def read(self, ptr, like):
        out = np.empty_like(like)
        assert self.lib.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
        return out

    def stream(self):
        st = C.c_void_p()
        assert self.lib.hipStreamCreate(C.byref(st)) == 0
        return st

    def close(self):
        assert self.lib.hipDeviceSynchronize() == 0
        for p in self.held:
            self.lib.hipFree(p)
        self.held = []


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.close()


def test_two_streams_one_synchronise_and_stats(pkg, gpu, hip):
    """The device entry points on device arrays of the test's own: two calls on two streams, one synchronise at the end, both
    right; a call with stats is synchronous and reports its rays and its kernel time."""
    capi = pkg.capi
    sc = scene_of(pkg, gpu, "book1")
    sc.set_option("query_lds", 2)
    rays = probe_rays("book1", n_random=4200, seed=5)[:N_BIG]
    halves, firsts = [np.ascontiguousarray(rays[:2000]), np.ascontiguousarray(rays[2000:])], (0, 2000)
    want = [sc.closest_hit(h, seed=SEED, t_min=T_MIN, first_index=k) for h, k in zip(halves, firsts)]
    d_rays = [hip.array(h) for h in halves]
    d_out = [hip.array(np.zeros((len(h), 8), np.float32)) for h in halves]
    d_mat = [hip.array(np.zeros(len(h), np.uint32)) for h in halves]
    streams = [hip.stream(), hip.stream()]
    assert hip.lib.hipDeviceSynchronize() == 0
    for i in (0, 1):
        p = capi.make_query_params(SEED, T_MIN, firsts[i])
        gpu.check(gpu._query_closest_device(sc.h, len(halves[i]), d_rays[i], C.byref(p), d_out[i], d_mat[i], streams[i], None))
    assert hip.lib.hipDeviceSynchronize() == 0
    for i in (0, 1):
        assert hip.read(d_out[i], want[i][0]).tobytes() == want[i][0].tobytes()
        assert hip.read(d_mat[i], want[i][1]).tobytes() == want[i][1].tobytes()
    r8 = with_t_max(halves[0], F32_MAX)
    d_r8, d_occ = hip.array(r8), hip.array(np.zeros(2000, np.uint8))
    for lds in (0, 2):
        sc.set_option("query_lds", lds)
        st, p = capi.Stats.new(), capi.make_query_params(SEED, T_MIN)
        d_o = hip.array(np.zeros((2000, 8), np.float32))
        gpu.check(gpu._query_closest_device(sc.h, 2000, d_rays[0], C.byref(p), d_o, d_mat[0], streams[0], C.byref(st)))
        assert hip.read(d_o, want[0][0]).tobytes() == want[0][0].tobytes()   # (synchronous: the result is there)
        assert st.rays == 2000 and st.kernel_ms > 0 and st.samples == 0 and st.aabb_tests == 0 and st.prim_tests == 0 and st.draws == 0
        st = capi.Stats.new()
        gpu.check(gpu._query_occluded_device(sc.h, 2000, d_r8, C.byref(p), d_occ, streams[1], C.byref(st)))
        assert st.rays == 2000 and st.kernel_ms > 0
        assert (hip.read(d_occ, np.zeros(2000, np.uint8)) == (want[0][0][:, 0] != 0)).all()
    for st in streams:
        assert hip.lib.hipStreamSynchronize(st) == 0 and hip.lib.hipStreamDestroy(st) == 0


TORCH_CHILD = r"""
import sys
import numpy as np
import torch
assert torch.cuda.is_available()   # torch's HIP runtime first (INTEGRATION.md: one HIP runtime per process), then the library
sys.path[:0] = [%(root)r, %(tests)r]
import __graft_entry__ as graft
from probe_rays import probe_rays
from scene_cases import build_case
SEED, T_MIN = %(seed)d, %(t_min)r
pkg = graft.load_package()
gpu = pkg.load()
for name in ("book1", "cornell"):
    sc = build_case(pkg, gpu, name)[0]
    rays = probe_rays(name, n_random=512, seed=99)
    ts = sc.closest_hit(rays, seed=SEED, t_min=T_MIN)[0][:, 1]
    with np.errstate(over="ignore"):
        r8 = np.concatenate([rays, (np.float32(2.0) * ts).astype(np.float32)[:, None]], axis=1)
    for lds in ((0, 2) if name == "book1" else (1,)):
        sc.set_option("query_lds", lds)
        out, mat = sc.closest_hit(rays, seed=SEED, t_min=T_MIN)
        occ = sc.occluded(r8, seed=SEED, t_min=T_MIN)
        assert isinstance(out, np.ndarray) and occ.dtype == np.uint8
        stream = torch.cuda.Stream()
        d7, d8 = torch.from_numpy(rays).cuda(), torch.from_numpy(r8).cuda()
        torch.cuda.synchronize()
        d_out, d_mat = sc.closest_hit(d7, seed=SEED, t_min=T_MIN, stream=stream)
        d_occ = sc.occluded(d8, seed=SEED, t_min=T_MIN, stream=stream)
        stream.synchronize()
        assert d_out.is_cuda and d_out.dtype == torch.float32 and d_mat.dtype == torch.int32 and d_occ.dtype == torch.uint8
        assert d_out.cpu().numpy().tobytes() == out.tobytes(), (name, lds)
        assert d_mat.cpu().numpy().view(np.uint32).tobytes() == mat.tobytes(), (name, lds)
        assert d_occ.cpu().numpy().tobytes() == occ.tobytes(), (name, lds)
        with torch.cuda.stream(stream):   # no stream given: the current torch stream
            e_out, e_mat = sc.closest_hit(d7, seed=SEED, t_min=T_MIN)
        stream.synchronize()
        assert e_out.cpu().numpy().tobytes() == out.tobytes()
        print("torch tensors on a stream:", name, "query_lds", lds, "ok")
    if name == "book1":   # two streams, one synchronise; stats
        sc.set_option("query_lds", 2)
        halves = [d7[:256].contiguous(), d7[256:].contiguous()]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        got = [sc.closest_hit(h, seed=SEED, t_min=T_MIN, first_index=k, stream=s) for h, k, s in zip(halves, (0, 256), streams)]
        torch.cuda.synchronize()
        assert torch.cat([g[0] for g in got]).cpu().numpy().tobytes() == out.tobytes()
        assert torch.cat([g[1] for g in got]).cpu().numpy().view(np.uint32).tobytes() == mat.tobytes()
        (s_out, s_mat), st = sc.closest_hit(d7, seed=SEED, t_min=T_MIN, stats=True)
        assert st["rays"] == len(rays) and st["kernel_ms"] > 0 and s_out.cpu().numpy().tobytes() == out.tobytes()
        s_occ, st = sc.occluded(d8, seed=SEED, t_min=T_MIN, stats=True)
        assert st["rays"] == len(rays) and st["kernel_ms"] > 0 and s_occ.cpu().numpy().tobytes() == occ.tobytes()
        for bad in (d7.double(), d7.t(), d7.cpu()):
            try:
                sc.closest_hit(bad)
            except ValueError:
                continue
            raise AssertionError("a tensor that is not contiguous float32 on the device was accepted")
        print("two streams and stats: ok")
print("TORCH CHILD OK")
"""


def test_torch_tensors_on_a_stream_give_the_host_path_bytes():
    """Scene.closest_hit / Scene.occluded on torch tensors, in and out, on a non-default stream: the host path's bytes on book1
    (both kernels) and cornell; two calls on two streams with one synchronise; stats.  In a process of its own, which is what
    the test is about: a process that uses torch and the library must initialise torch's HIP runtime first (INTEGRATION.md
    section 3), and this one has loaded the library long ago."""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    code = TORCH_CHILD % {"root": os.path.dirname(tests), "tests": tests, "seed": SEED, "t_min": T_MIN}
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "TORCH CHILD OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(pkg, gpu, hip):
    capi = pkg.capi
    sc = scene_of(pkg, gpu, "book1")
    n = 8
    rays = with_t_max(rays_of("book1")[:n], F32_MAX)
    sentinel = (np.full((n, 8), 7, np.float32), np.full(n, 7, np.uint32), np.full(n, 7, np.uint8))

    def bad_params():
        for field, value in (("struct_size", 28), ("struct_size", 0), ("reserved", 1), ("reserved2", 7), ("first_index", (1 << 32) - n + 1),
                             ("first_index", 1 << 40), ("t_min", float("nan"))):
            p = capi.make_query_params(SEED, T_MIN)
            setattr(p, field, value)
            yield field, p

    for host in (True, False):
        if host:
            out, mat, occ = (a.copy() for a in sentinel)
            rays_ptr, p_out, p_mat, p_occ = rays.ctypes.data, out.ctypes.data, mat.ctypes.data, occ.ctypes.data
        else:
            rays_ptr, p_out, p_mat, p_occ = hip.array(rays), hip.array(sentinel[0]), hip.array(sentinel[1]), hip.array(sentinel[2])
        tail = () if host else (None,)   # (the device variants' stream)
        closest = gpu._query_closest if host else gpu._query_closest_device
        occluded = gpu._query_occluded if host else gpu._query_occluded_device
        for field, p in bad_params():
            assert closest(sc.h, n, rays_ptr, C.byref(p), p_out, p_mat, *tail, None) == ERR_INVALID, (host, field)
            assert gpu.last_error()
            assert occluded(sc.h, n, rays_ptr, C.byref(p), p_occ, *tail, None) == ERR_INVALID, (host, field)
        good = capi.make_query_params(SEED, T_MIN)
        assert closest(sc.h, n, None, C.byref(good), p_out, p_mat, *tail, None) == ERR_INVALID           # null rays
        assert occluded(sc.h, n, None, C.byref(good), p_occ, *tail, None) == ERR_INVALID
        assert closest(sc.h, n, rays_ptr, C.byref(good), None, p_mat, *tail, None) == ERR_INVALID        # null outputs
        assert closest(sc.h, n, rays_ptr, C.byref(good), p_out, None, *tail, None) == ERR_INVALID
        assert occluded(sc.h, n, rays_ptr, C.byref(good), None, *tail, None) == ERR_INVALID
        assert closest(sc.h, n, rays_ptr, None, p_out, p_mat, *tail, None) == ERR_INVALID                # null params
        assert occluded(sc.h, n, rays_ptr, None, p_occ, *tail, None) == ERR_INVALID
        st = capi.Stats.new()
        st.struct_size = 8
        assert closest(sc.h, n, rays_ptr, C.byref(good), p_out, p_mat, *tail, C.byref(st)) == ERR_INVALID
        # n = 0: RTG_OK, nothing enqueued, null pointers allowed
        assert closest(sc.h, 0, None, C.byref(good), None, None, *tail, None) == 0
        assert occluded(sc.h, 0, None, C.byref(good), None, *tail, None) == 0
        if not host:
            assert hip.lib.hipDeviceSynchronize() == 0
            out, mat, occ = hip.read(p_out, sentinel[0]), hip.read(p_mat, sentinel[1]), hip.read(p_occ, sentinel[2])
        assert (out == 7).all() and (mat == 7).all() and (occ == 7).all(), host
    # the last index a call may use is 2^32 - 1
    p = capi.make_query_params(SEED, T_MIN, first_index=(1 << 32) - n)
    out, mat, rays7 = np.zeros((n, 8), np.float32), np.zeros(n, np.uint32), np.ascontiguousarray(rays[:, :7])
    assert gpu._query_closest(sc.h, n, rays7.ctypes.data, C.byref(p), out.ctypes.data, mat.ctypes.data, None) == 0
    with pytest.raises(capi.RtError):
        sc.set_option("query_lds", 3)
