"""The checks of camera_ref.py (the camera block and the emitter shares of every pixel in numpy float64 -- none of it the oracle's
or the GPU library's) against the CPU restatement, oracle/liboracle.so, and -- for the camera block, which is host code -- against
the HIP library as well.  test_camera_gpu.py runs the frame checks on every kernel route.  Run with -s to see the figures that
camera_ref.py's docstring and DESIGN.md quote: the worst deviations of the block, and per world the class sizes, worst |z|,
chi2 / dof, frame z and each planted variant's chi2."""
import numpy as np
import pytest

import camera_ref as C


@pytest.fixture(scope="module")
def frames(pkg, oracle):
    """The restatement's counts of every world: rendered once, shared (read only) among the tests below."""
    out = {}
    for name in C.WORLDS:
        out[name] = C.render_counts(pkg, oracle, name)
        out[name].setflags(write=False)
    return out


def test_the_poses_cover_what_they_should():
    assert len(C.POSES) >= 12
    assert {0.02, 20.0, 90.0, 150.0} <= {p["fov"] for p in C.POSES}
    assert {0.5, 10.0, 1000.0} <= {p["focus"] for p in C.POSES}
    assert min(p["aspect"] for p in C.POSES) < 1.0 < max(p["aspect"] for p in C.POSES)
    assert any(np.linalg.norm(p["from"]) >= 1e3 for p in C.POSES)
    angles = []
    for p in C.POSES:
        d = np.subtract(p["at"], p["from"])
        cos = abs(np.dot(d, p["up"])) / (np.linalg.norm(d) * np.linalg.norm(p["up"]))
        angles.append(np.degrees(np.arccos(min(1.0, cos))))
    assert min(angles) < 5.0, "an `up` within a few degrees of the view"
    assert sum(5.0 < a < 85.0 for a in angles) >= 3, "`up` not perpendicular to the view"


def test_camera_block_against_float64(pkg, oracle):
    """A, on both back ends: rtg_camera_look is host code and needs no GPU."""
    for be in (oracle, pkg.load()):
        worst = C.check_look(be)
        print("%s: worst deviation of the points %.2e (relative), of u / v %.2e" % (be.prefix, *worst))


def test_the_block_tolerances_are_four_times_the_measured_worst(oracle):
    worst = C.check_look(oracle)
    for got, written in zip(worst, (C.WORST_POINT, C.WORST_BASIS)):
        assert 0.9 * written <= got <= written, (got, written)


@pytest.mark.parametrize("variant", C.LOOK_VARIANTS)
def test_a_wrong_block_is_noticed(oracle, variant):
    with pytest.raises(AssertionError, match="is off by"):
        C.check_look(oracle, variant=variant)


@pytest.mark.parametrize("name", list(C.WORLDS))
def test_hit_shares_against_float64(pkg, oracle, frames, name):
    C.check_world(pkg, oracle, name, counts=frames[name])


def test_views_along_two_axes_see_the_same_frame(frames):
    """The +x worlds are the -z worlds turned: a handedness error would move their emitter, and with unequal margins the
    expectation would no longer fit (test_hit_shares_against_float64); the two expectations themselves agree."""
    for d in ("2.5", "4", "7"):
        assert np.abs(C.shares("rect_-z_" + d)[0] - C.shares("rect_+x_" + d)[0]).max() < 1e-6


def test_the_company_changes_no_count(frames):
    """The worlds that add a Bvh behind the camera (for the pool-2 kernel) render the counts of the worlds without it."""
    for name in C.WORLDS:
        if C.WORLDS[name].get("company"):
            assert np.array_equal(frames[name], frames[name[:-len("_company")]]), name


@pytest.mark.parametrize("name", [n for n in C.WORLDS if not C.WORLDS[n].get("company")])
def test_the_quadrature_has_converged(name):
    """Doubling every quadrature resolution moves no statistical-class pixel's share by more than a tenth of its standard
    error, and no other pixel's expected count by more than a tenth of the slack of 4 hits it is given."""
    p, _ = C.shares(name)
    q, _ = C.shares(name, res=2)
    var = C.NS * q * (1.0 - q)
    cls = var >= 9.0
    moved = C.NS * np.abs(p - q)
    rel = (moved[cls] / np.sqrt(var[cls])).max()
    print("%-14s doubling moves a class pixel by %.4f standard errors at the most, another pixel by %.3f hits" % (
        name, rel, moved[~cls].max()))
    assert rel <= 0.1
    assert moved[~cls].max() <= 0.4


def test_every_planted_variant_is_rejected(frames):
    """Each wrong camera's expectation is refused by accept, on the very frames the true expectation passes (the tests
    above), on every world where it differs from the truth -- and it differs on at least one."""
    for variant in C.VARIANTS:
        rejected = []
        for name in C.WORLDS:
            if C.WORLDS[name].get("company"):      # (the counts and the expectation of the world without it)
                continue
            if C.coincides(variant, name):
                assert variant == "time_from_lens_x" or np.abs(C.shares(name, variant)[0] - C.shares(name)[0]).max() < 1e-9, (variant, name)
                continue
            p, _ = C.shares(name, variant)
            fig = C.figures(frames[name], p, C.NS)
            with pytest.raises(AssertionError):
                C.accept(frames[name], p, C.NS, None, 0, "%s as %s" % (name, variant))
            rejected.append("%s %.3g / %d" % (name, fig["chi2"], fig["dof"]))
        print("%-24s chi2: %s" % (variant, "; ".join(rejected)))
        assert rejected, variant
