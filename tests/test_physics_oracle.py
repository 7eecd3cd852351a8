"""The checks of physics_ref.py (answers in numpy float64, closed forms and binomial bounds -- none of them the oracle's or the
GPU library's) against the CPU restatement, oracle/liboracle.so.  test_physics_gpu.py runs the same bodies on the HIP
kernels.  Run with -s to see, per scene, the share of rays or pixels left out for conditioning and the worst deviations: the
figures in physics_ref.py's docstring, from which its tolerances are derived."""
import pytest

import physics_ref as P


@pytest.mark.parametrize("name", P.HIT_SCENES)
def test_hit_top_against_float64(pkg, oracle, name):
    P.check_hits(pkg, oracle, name)


def test_the_measured_worst_case_is_the_one_the_tolerances_come_from(pkg, oracle):
    """TOL_T / TOL_P / TOL_N are 4 x the worst deviations over the scenes of A: the worst case measured here must be the one
    written down (to the two digits given), not something smaller that would leave the tolerance looser than derived."""
    res = [P.check_hits(pkg, oracle, name) for name in P.HIT_SCENES]
    worst = [max(r[k] for r in res) for k in ("dt", "dp", "dn")]
    print("worst over A: dt %.3e dp %.3e dn %.3e; left out %.2f .. %.2f %%" % (
        *worst, 100 * min(r["left_out"] for r in res), 100 * max(r["left_out"] for r in res)))
    for got, written in zip(worst, (P.WORST_T, P.WORST_P, P.WORST_N)):
        assert 0.95 * written <= got <= written, (got, written)


@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("name", P.FEATURE_GRAPHS)
def test_feature_planes_against_float64(pkg, oracle, name, grid):
    P.check_feature_planes(pkg, oracle, name, grid)


@pytest.mark.parametrize("max_bounces", [50, 3])
@pytest.mark.parametrize("metal", [False, True])
@pytest.mark.parametrize("kind", ["lean", "list"])
def test_radiance_is_exactly_a_power_of_the_albedo(pkg, oracle, kind, metal, max_bounces):
    P.check_exact_radiance(pkg, oracle, kind, metal, max_bounces=max_bounces)


@pytest.mark.parametrize("i", range(len(P.METAL_POSES)))
def test_mirror_beam(pkg, oracle, i):
    P.check_beam(pkg, oracle, P.METAL_POSES[i])


def test_glass_beams(pkg, oracle):
    shares = sum(P.check_beam(pkg, oracle, pose) for pose in P.GLASS_POSES)
    assert shares >= P.GLASS_FIRST_SHARES, "the first interface's reflected share must be checked on at least that many poses"


@pytest.mark.parametrize("i", range(len(P.LOBE_POSES)))
def test_lobe_shares(pkg, oracle, i):
    P.check_lobe(pkg, oracle, P.LOBE_POSES[i])


@pytest.mark.parametrize("i", range(len(P.SLAB_POSES)))
def test_medium_slab(pkg, oracle, i):
    P.check_slab(pkg, oracle, P.SLAB_POSES[i])


def test_the_curated_poses_cover_what_they_should():
    for poses in (P.METAL_POSES, P.GLASS_POSES):
        assert len(poses) >= 24
        assert {"list", "lean"} == {p["world"] for p in poses}
        assert {"sphere", "prism"} == {p["objects"][0][0][0] for p in poses}
    assert {1.5, 0.6667} == {p["objects"][0][1][1] for p in P.GLASS_POSES}


def _failure(check, *args, **kw):
    """The message of the AssertionError `check` raises; a pose the fault makes inadmissible does not count as noticed."""
    with pytest.raises(AssertionError) as e:
        check(*args, **kw)
    assert "not admissible" not in str(e.value), e.value
    return str(e.value)


def test_the_checks_notice_planted_faults(pkg, oracle):
    """Each deliberately wrong variant of the float64 side makes the matching check fail against the (unchanged) oracle: the
    tolerances and caps are tight enough to see a fault of that kind in the code under test."""
    assert "dn" in _failure(P.check_hits, pkg, oracle, "nest3", fault="rotate_neg")
    assert "dn" in _failure(P.check_hits, pkg, oracle, "deep", fault="scale_normal")
    _failure(P.check_feature_planes, pkg, oracle, "nest3", 1, fault="rotate_neg")
    glass = [p for p in P.GLASS_POSES if p["objects"][0][1][1] == 1.5 and p["world"] == "list"]
    _failure(P.check_beam, pkg, oracle, glass[0], fault="ni_over_nt")
    msg = _failure(P.check_beam, pkg, oracle, glass[4], fault="schlick4")      # (incidence at 60 degrees and more)
    assert "expected" in msg or "Schlick gives" in msg, msg
    _failure(P.check_lobe, pkg, oracle, P.LOBE_POSES[0], fault="unit_sphere")
    _failure(P.check_slab, pkg, oracle, P.SLAB_POSES[3], fault="free_path")
    for pose in (glass[0], P.LOBE_POSES[0], P.SLAB_POSES[3]):   # (and the same calls pass without the fault)
        {"sphere": P.check_beam, "prism": P.check_beam, "floor": P.check_lobe, "slab": P.check_slab}[pose["objects"][0][0][0]](pkg, oracle, pose)
