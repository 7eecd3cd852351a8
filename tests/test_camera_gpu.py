"""The frame checks of camera_ref.py (every pixel's share of samples that meet an emitter, in numpy float64 -- none of it the
oracle's or the library's) against par_cast frames of the HIP kernels, each kernel forced in turn: the default choice, the
lock-step kernel (sync 1), the first pool kernel (sync 0, pool2 0), the pool-2 kernel (sync 0, pool2 2) where the world has a
second program, the baseline (kernel 1) and, with light_sampling 1, the kernel of rt_light.h; for the lean program the lean
pool (asserted from the verbose line), chunks 1, bvh4 1 and the baseline.  Beside the float64 check every route's counts must
equal the CPU restatement's.  test_camera_oracle.py runs the same checks, the planted variants and the camera block on the
CPU.  Run with -s to see the figures."""
import numpy as np
import pytest

import camera_ref as C

pytestmark = pytest.mark.gpu

NX, NY, NS = C.NX, C.NY, C.NS
DEFAULT, LOCK_STEP, POOL, POOL2, BASELINE = (), (("sync", 1),), (("sync", 0), ("pool2", 0)), (("sync", 0), ("pool2", 2)), (("kernel", 1),)
LIGHT = (("light_sampling", 1),)
LIST_WORLDS = [n for n in C.WORLDS if C.WORLDS[n]["kind"] == "rect"]


@pytest.fixture(scope="module")
def restated(pkg, oracle):
    """The CPU restatement's counts of every world, rendered once (read only)."""
    out = {}
    for name in C.WORLDS:
        out[name] = C.render_counts(pkg, oracle, name)
        out[name].setflags(write=False)
    return out


def has_second_program(pkg, gpu, name):
    b = gpu.builder()
    return len(b.flatten_pool2(C.build(pkg, b, name)[0])[0]) != 0


def check_route(pkg, gpu, restated, name, options):
    k, _ = C.check_world(pkg, gpu, name, options)
    assert np.array_equal(k, restated[name]), "%s %s: the counts differ from the restatement's in %d pixels" % (
        name, dict(options), (k != restated[name]).sum())
    return k


@pytest.mark.parametrize("name", LIST_WORLDS)
def test_list_worlds_on_every_kernel(pkg, gpu, restated, name):
    """Worlds 1, 3 and 4: a rect at three distances seen along -z and along +x, the rect moving, the rect moving behind a lens."""
    second = has_second_program(pkg, gpu, name)
    assert second == bool(C.WORLDS[name]["company"]), "the worlds with company, and only they, have a second program"
    plain = check_route(pkg, gpu, restated, name, DEFAULT)
    for options in [LOCK_STEP, POOL] + ([POOL2] if second else []) + [BASELINE]:
        check_route(pkg, gpu, restated, name, options)
    # no diffuse surface: the shadow-ray kernel draws the same camera rays and nothing else
    assert np.array_equal(C.render_counts(pkg, gpu, name, LIGHT), plain), name + ": light_sampling 1 changes the counts"


def test_the_pool2_kernel_is_reached(pkg, gpu):
    assert sum(has_second_program(pkg, gpu, name) for name in LIST_WORLDS) >= 2


def test_spheres_on_the_lean_pool(pkg, gpu, restated, capfd):
    """World 2 on the default choice, which must be the lean pool kernel: the verbose line says which kernel ran."""
    b = gpu.builder()
    world, cam = C.build(pkg, b, "spheres")
    scene = b.scene(world)
    scene.set_option("verbose", 1)
    capfd.readouterr()
    frame = scene.par_cast(cam, NX, NY, NS, partial=True)
    err = capfd.readouterr().err
    scene.set_option("verbose", 0)
    assert "[rtg] pool: samples [0, %d) of %d" % (NS, NS) in err and "full pool" not in err, err[-800:]
    k = C.counts_of(frame, NS, True)
    C.check_world(pkg, gpu, "spheres", counts=k)
    assert np.array_equal(k, restated["spheres"])


@pytest.mark.parametrize("options", [(("chunks", 1),), (("bvh4", 1),), BASELINE], ids=["chunks", "bvh4", "baseline"])
def test_spheres_on_other_routes(pkg, gpu, restated, options):
    check_route(pkg, gpu, restated, "spheres", options)


@pytest.mark.parametrize("name", ["spheres", "moving_lens", "rect_+x_2.5"])
def test_two_slices_give_the_one_call_counts(pkg, gpu, restated, name):
    """A frame as two PARTIAL / RESUME slices of 512 samples."""
    b = gpu.builder()
    world, cam = C.build(pkg, b, name)
    scene = b.scene(world)
    acc = scene.par_cast(cam, NX, NY, NS // 2, partial=True)
    half = C.counts_of(acc, NS // 2, True)
    scene.par_cast(cam, NX, NY, NS, out=acc, sample_begin=NS // 2, resume=True, partial=True)
    k = C.counts_of(acc, NS, True)
    assert (half <= k).all() and half.sum() < k.sum()
    assert np.array_equal(k, restated[name])
    C.check_world(pkg, gpu, name, counts=k)


def test_two_handles_give_the_one_call_counts(pkg, gpu, restated):
    """World 2 through par_cast_multi over two scene handles."""
    scenes = []
    for _ in range(2):
        b = gpu.builder()
        world, cam = C.build(pkg, b, "spheres")
        scenes.append(b.scene(world))
    k = C.counts_of(gpu.par_cast_multi(scenes, cam, NX, NY, NS), NS, False)
    assert np.array_equal(k, restated["spheres"])
    C.check_world(pkg, gpu, "spheres", counts=k)
