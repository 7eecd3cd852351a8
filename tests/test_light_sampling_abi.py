"""Scene option light_sampling without a GPU: the eligibility rule of light_ref.py on the worlds the GPU tests render, the
quadrature's lobe against closed forms, and what the header and the binding say."""
import os

import numpy as np
import pytest

import light_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(L.WORLDS))
def test_light_table_of_each_world(pkg, oracle, name):
    b, world, _, n = L.build(pkg, oracle, name)
    table = L.light_table(b, world)
    assert len(table) == n, (name, len(table), n)
    for axis, r0, r1, k, m in table:
        assert b.materials[m][0] == "light"
    if name == "cornell":
        assert L.area(table[0]) == 13650.0 and table[0][0] == 1 and table[0][3] == 554.0
    if name == "book2":
        assert L.area(table[0]) == 300.0 * 265.0
    if name == "two_materials":   # the light inside the Bvh is found by scattered rays, the list-level one is sampled
        assert L.area(table[0]) == 2.0


def test_lobe_is_a_density_and_2cos3_over_pi_for_unit_normals():
    rs = np.random.default_rng(7)
    w = rs.normal(size=(200000, 3))
    w /= np.linalg.norm(w, axis=1)[:, None]
    n = np.array([0.0, 1.0, 0.0])
    cos = np.maximum(w[:, 1], 0.0)
    assert np.allclose(L.lobe(n, w), 2.0 * cos ** 3 / np.pi, atol=1e-12)
    # any |n| (Scale leaves normals unnormalised): the density still integrates to 1 over the sphere -- Monte Carlo over
    # 200 000 uniform directions, standard error below 0.5 % of the integral for these normals
    for n in ([0.0, 0.6, 0.0], [0.3, 1.7, -0.4], [0.0, 1.0, 0.0]):
        vals = L.lobe(np.array(n), w) * 4.0 * np.pi
        se = vals.std() / np.sqrt(len(vals))
        assert abs(vals.mean() - 1.0) < 5.0 * se, (n, vals.mean(), se)
    # ... and matches where the reference's own construction sends its directions: n + a uniform point of the unit ball
    n = np.array([0.3, 1.7, -0.4])
    v = rs.uniform(-1.0, 1.0, size=(400000, 3))
    v = v[(v * v).sum(1) < 1.0]
    d = n + v
    d /= np.linalg.norm(d, axis=1)[:, None]
    axis = n / np.linalg.norm(n)
    for lo, hi in ((0.95, 1.0), (0.85, 0.95), (0.0, 0.85)):
        share = np.mean((d @ axis >= lo) & (d @ axis < hi))
        in_band = (w @ axis >= lo) & (w @ axis < hi)
        want = np.mean(L.lobe(n, w) * 4.0 * np.pi * in_band)
        assert abs(share - want) < 5.0 * np.sqrt(want * (1.0 - want) / len(d) + (L.lobe(n, w) * 4.0 * np.pi * in_band).var() / len(w)), (lo, hi, share, want)


def test_quadrature_converges_and_the_planted_variants_differ():
    p, n = np.array([0.1, 0.0, -0.2]), np.array([0.0, 1.0, 0.0])
    rect = (1, np.array([-1.0, 1.0]), np.array([-0.5, 0.5]), 2.0)
    fine, coarse = L.direct(p, n, *rect, m=400), L.direct(p, n, *rect, m=100)
    # a midpoint rule's error falls as 1 / m^2: 100 -> 400 points a side leaves 1 / 16 of the difference seen here
    assert abs(fine - coarse) < 1e-4 * fine
    for variant in L.VARIANTS:
        # (under the light cos_l is near 1: leaving it out moves the answer by 5 %, still tens of the GPU test's standard errors)
        assert abs(L.direct(p, n, *rect, variant=variant) - fine) > 0.02 * fine, variant


def test_the_header_states_the_estimator_and_the_binding_forwards_the_option(pkg):
    assert "light_sampling" in pkg.capi.Scene.ENV_OPTIONS
    with open(os.path.join(ROOT, "include", "rtiow_gpu.h")) as f:
        text = f.read()
    at = text.index('"light_sampling" = 1')
    doc = text[at:text.index("int rtg_scene_set_option(", at)]
    for phrase in ("non-parity", "RT_MAX_LIGHTS = 64", "RTG_ERR_INVALID", "FlipNormals", "2 cos^3 / pi", "(r_hi^3 - r_lo^3) / (4 pi)", "1 / (4 pi)",
                   "[t_near, 1 - 1e-3)", "bounces < max_bounces", "lobe * N * area_i * cos_l / r2", "rtg_par_cast_multi", "RTG_ERR_UNSUPPORTED"):
        assert phrase in doc, phrase
    assert "with one\n * exception" in text[:at] or "exception" in text[text.index("Scheduling / measurement switches"):at]
