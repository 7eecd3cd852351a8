"""The checks of physics_ref.py (answers in numpy float64, closed forms and binomial bounds -- none of them the oracle's)
against the HIP kernels: rtg_debug_hit_top, the feature kernel of RTG_FLAG_FEATURES, the probe kernel of rtg_debug_samples
and, with RTG_FLAG_TRACE_KERNEL, the production kernels -- the lean pool, the lock-step kernel (sync 1), the first pool
kernel (sync 0) and the pool-2 kernel (pool2 2) where the world has a second program.  test_physics_oracle.py runs the same
bodies on the CPU restatement."""
import pytest

import physics_ref as P

pytestmark = pytest.mark.gpu

PROBE = ((), False)
LOCK_STEP, POOL, POOL2 = ((("sync", 1),), True), ((("sync", 0), ("pool2", 0)), True), ((("sync", 0), ("pool2", 2)), True)
LEAN_POOL = ((), True)
IDS = {PROBE: "probe", LOCK_STEP: "lock-step", POOL: "pool", POOL2: "pool2", LEAN_POOL: "production"}


def first(poses, world, **kw):
    return next(p for p in poses if p["world"] == world and all(p.get(k) == v for k, v in kw.items()))


def routes_of(pkg, gpu, pose):
    """The production kernels the world of `pose` admits, forced one by one."""
    if pose["world"] == "lean":
        return [LEAN_POOL]
    b = gpu.builder()
    second = len(b.flatten_pool2(P.beam_world(pkg, b, pose))[0]) != 0
    return [LOCK_STEP, POOL] + ([POOL2] if second else [])


@pytest.mark.parametrize("name", P.HIT_SCENES)
def test_hit_top_against_float64(pkg, gpu, name):
    P.check_hits(pkg, gpu, name)


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("name", P.FEATURE_GRAPHS)
def test_feature_planes_against_float64(pkg, gpu, name, grid):
    P.check_feature_planes(pkg, gpu, name, grid)


@pytest.mark.parametrize("kind,route", [("lean", PROBE), ("lean", LEAN_POOL), ("list", PROBE), ("list", LOCK_STEP), ("list", POOL), ("list", POOL2)],
                         ids=lambda v: IDS.get(v, v) if isinstance(v, tuple) else v)
@pytest.mark.parametrize("metal", [False, True], ids=["lambertian", "metal"])
def test_radiance_is_exactly_a_power_of_the_albedo(pkg, gpu, kind, route, metal):
    options, trace = route
    P.check_exact_radiance(pkg, gpu, kind, metal, options=options, trace_kernel=trace, need_pool2=route is POOL2)


def test_radiance_at_the_bounce_cap(pkg, gpu):
    for kind in ("lean", "list"):
        P.check_exact_radiance(pkg, gpu, kind, max_bounces=3)


@pytest.mark.parametrize("i", range(len(P.METAL_POSES)))
def test_mirror_beam(pkg, gpu, i):
    P.check_beam(pkg, gpu, P.METAL_POSES[i])


def test_glass_beams(pkg, gpu):
    shares = sum(P.check_beam(pkg, gpu, pose) for pose in P.GLASS_POSES)
    assert shares >= P.GLASS_FIRST_SHARES, "the first interface's reflected share must be checked on at least that many poses"


@pytest.mark.parametrize("i", range(len(P.LOBE_POSES)))
def test_lobe_shares(pkg, gpu, i):
    P.check_lobe(pkg, gpu, P.LOBE_POSES[i])


@pytest.mark.parametrize("i", range(len(P.SLAB_POSES)))
def test_medium_slab(pkg, gpu, i):
    P.check_slab(pkg, gpu, P.SLAB_POSES[i])


@pytest.mark.parametrize("world", ["list", "lean"])
@pytest.mark.parametrize("material", ["mirror", "glass"])
def test_beams_on_the_production_kernels(pkg, gpu, material, world):
    pose = first(P.METAL_POSES if material == "mirror" else P.GLASS_POSES, world)
    routes = routes_of(pkg, gpu, pose)
    assert len(routes) >= (1 if world == "lean" else 2)
    for options, trace in routes:
        P.check_beam(pkg, gpu, pose, options=options, trace_kernel=trace)


def test_lobes_and_slabs_on_the_production_kernels(pkg, gpu):
    for check, pose in ((P.check_lobe, P.LOBE_POSES[1]), (P.check_lobe, P.LOBE_POSES[3]), (P.check_lobe, P.LOBE_POSES[5]),
                        (P.check_slab, P.SLAB_POSES[2]), (P.check_slab, P.SLAB_POSES[3])):
        routes = routes_of(pkg, gpu, pose)
        assert len(routes) >= 2
        for options, trace in routes:
            check(pkg, gpu, pose, options=options, trace_kernel=trace)
