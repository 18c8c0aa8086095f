"""GNC-TLS re-weighting of the range measurements (score_amd/robust.py) on the CPU: the weight rule, the loop's readable twin
(engine="python") on the oracle's CPU twin of the library, and the weighted refinement (refine_estimate(range_weights=...))."""
import logging

import numpy as np
import pytest

from conftest import graph_by_name
from score_amd.manhattan import make_manhattan
from score_amd.native import ArrayGraph, graph_arrays
from score_amd.refine import refine_estimate
from score_amd.robust import corrupt_ranges, gnc_tls_weight, initial_mu, relaxed_range_residuals, solve_score_robust
from score_amd.solve_score import solve_score

# Calibrated on the twin (engine="python"): two robots x 60 poses, three beacons, p_range 0.5, range sigma 0.1, 8 % of the
# ranges shortened by U(0.3, 0.6).  Measured for seed 2: 220 ranges, 18 corrupted, 3 flagged (all corrupted ones), 0 false,
# 7 outer solves; robot A's translations 1.8e-2 from the plain solve of the clean graph, 4.0 for the plain solve of the
# corrupted one.  Seeds 1-4: the robust estimate 4e-6 .. 9e-2 from the clean one, the plain one 2.0 .. 7.9.  Most corrupted
# ranges are not flagged: they touch the second robot or a beacon that the relaxation leaves free to follow them (a range that
# can be met exactly costs nothing), so they do not move the determined part of the estimate either.
CORRUPT = dict(n_robots=2, n_poses=60, n_beacons=3, p_range=0.5, sigma_range=0.1)


def _robot_a_gap(a, b, fg):
    names = [p.name for p in fg.pose_variables[0]]
    return max(float(np.max(np.abs(a.poses[k][:-1, -1] - b.poses[k][:-1, -1]))) for k in names)


def test_weight_rule_band_edges_monotone_and_mu0():
    c, mu = 3.0, 0.7
    lo, hi = np.sqrt(mu / (mu + 1) * c * c), np.sqrt((mu + 1) / mu * c * c)
    # at both edges of the band the middle formula meets the constant pieces
    assert gnc_tls_weight([lo], mu, c)[0] == 1.0
    assert gnc_tls_weight([hi], mu, c)[0] == 0.0
    assert c / (lo * (1 + 1e-12)) * np.sqrt(mu * (mu + 1)) - mu == pytest.approx(1.0, abs=1e-9)
    assert c / (hi * (1 - 1e-12)) * np.sqrt(mu * (mu + 1)) - mu == pytest.approx(0.0, abs=1e-9)
    inside = gnc_tls_weight([lo * 1.001, hi * 0.999], mu, c)
    assert 0.99 < inside[0] < 1.0 and 0.0 < inside[1] < 0.01
    r = np.linspace(0.0, 3 * hi, 2001)
    w = gnc_tls_weight(r, mu, c)
    assert np.all(np.diff(w) <= 0) and w[0] == 1.0 and w[-1] == 0.0 and np.all((w >= 0) & (w <= 1))
    # the sign of a residual does not matter
    np.testing.assert_array_equal(gnc_tls_weight(-r, mu, c), w)
    # mu0 = c^2 / (2 r2max - c^2): the largest residual then sits on the upper band edge (weight 0 only beyond it)
    r2max = 20.0
    mu0 = initial_mu(r2max, c)
    assert mu0 == pytest.approx(9.0 / 31.0)
    assert (mu0 + 1) / mu0 * c * c == pytest.approx(2 * r2max)
    # a larger mu narrows the band around c
    assert gnc_tls_weight([c * 1.05], 100.0, c)[0] < gnc_tls_weight([c * 1.05], 1.0, c)[0]


def test_clean_graph_is_one_plain_solve(fixtures, twin_lib):
    fg = graph_by_name("manhattan", fixtures)
    rob = solve_score_robust(fg, engine="python", lib_path=twin_lib)
    ref = solve_score(fg, lib_path=twin_lib)
    info = rob.info["robust"]
    assert info["outer_iterations"] == 1 and info["converged"] and len(info["outliers"]) == 0
    np.testing.assert_array_equal(info["weights"], np.ones(len(fg.range_measurements)))
    for nm in ref.poses:
        np.testing.assert_array_equal(rob.poses[nm], ref.poses[nm])
    # the residuals are the relaxed ones of that solve
    r = relaxed_range_residuals(graph_arrays(fg), ref.relaxed_poses.array, ref.landmarks.array)
    np.testing.assert_array_equal(info["residuals"], r)
    assert 2 * float(np.max(r)) ** 2 <= 9.0


def test_short_outliers_are_discounted(twin_lib):
    logging.disable(logging.WARNING)  # (the twin's ADMM loop reaches its iteration cap on these graphs: it says so)
    try:
        fg = make_manhattan(seed=2, **CORRUPT)
        bad_g, bad = corrupt_ranges(fg, 0.08, seed=2)
        nr = len(bad_g.arrays["rng_a"])
        assert len(bad) == round(0.08 * nr)
        rob = solve_score_robust(bad_g, "SOCP", engine="python", lib_path=twin_lib)
        clean = solve_score(fg, "SOCP", lib_path=twin_lib)
        plain = solve_score(bad_g, "SOCP", lib_path=twin_lib)
    finally:
        logging.disable(logging.NOTSET)
    info = rob.info["robust"]
    flagged, injected = set(info["outliers"].tolist()), set(bad.tolist())
    assert info["converged"] and 1 < info["outer_iterations"] < 50
    assert len(flagged) >= 2 and flagged <= injected             # measured: 3 flagged, every one of them corrupted
    assert len(flagged - injected) <= 0.02 * (nr - len(injected))
    assert np.all((info["weights"] < 1e-6) | (info["weights"] > 1 - 1e-6))
    near, far = _robot_a_gap(rob, clean, fg), _robot_a_gap(plain, clean, fg)
    assert near < 0.1 and far > 1.0, (near, far)                  # measured: 1.8e-2 and 4.0


def test_range_weights_in_the_refinement(twin_lib):
    fg = make_manhattan(n_robots=1, n_poses=40, n_beacons=3, seed=21, p_range=0.6)
    res = solve_score(fg, "SOCP", lib_path=twin_lib)
    nr = len(fg.range_measurements)
    a, ia = refine_estimate(fg, res, lib_path=twin_lib)
    b, ib = refine_estimate(fg, res, lib_path=twin_lib, range_weights=np.ones(nr))
    assert ia["cost_final"] == ib["cost_final"]
    for nm in a.poses:
        np.testing.assert_array_equal(a.poses[nm], b.poses[nm])
    # a zero weight is the range taken out (the beacon it measured keeps others)
    arr = graph_arrays(fg)
    lm = arr["rng_b"][5]
    assert np.count_nonzero(arr["rng_b"] == lm) > 2
    w = np.ones(nr)
    w[5] = 0.0
    c, ic = refine_estimate(fg, res, lib_path=twin_lib, range_weights=w)
    fg2 = make_manhattan(n_robots=1, n_poses=40, n_beacons=3, seed=21, p_range=0.6)
    del fg2.range_measurements[5]
    d, id_ = refine_estimate(fg2, res, lib_path=twin_lib)
    assert ic["cost_final"] == pytest.approx(id_["cost_final"], rel=1e-9, abs=1e-12)
    for nm in c.poses:
        np.testing.assert_allclose(c.poses[nm], d.poses[nm], atol=1e-7)
    for nm in c.landmarks:
        np.testing.assert_allclose(c.landmarks[nm], d.landmarks[nm], atol=1e-7)
    assert ic["cost_final"] < ia["cost_final"]


def test_argument_errors(fixtures, twin_lib):
    fg = graph_by_name("manhattan", fixtures)
    with pytest.raises(ValueError, match="via_socp"):
        solve_score_robust(fg, "QCQP", qcqp_mode="direct", engine="python", lib_path=twin_lib)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="inlier_threshold"):
            solve_score_robust(fg, inlier_threshold=bad, engine="python", lib_path=twin_lib)
    with pytest.raises(ValueError, match="min_weight"):
        solve_score_robust(fg, min_weight=0.0, engine="python", lib_path=twin_lib)
    with pytest.raises(ValueError, match="mu_step"):
        solve_score_robust(fg, mu_step=1.0, engine="python", lib_path=twin_lib)
    with pytest.raises(ValueError, match="engine"):
        solve_score_robust(fg, engine="gpu", lib_path=twin_lib)
    a = dict(graph_arrays(fg))
    a["rng_prec"] = a["rng_prec"].copy()
    a["rng_prec"][3] = 0.0
    with pytest.raises(ValueError, match="precision"):
        solve_score_robust(ArrayGraph(a), engine="python", lib_path=twin_lib)
    small = make_manhattan(n_robots=1, n_poses=20, n_beacons=2, seed=3, p_range=0.5)
    res = solve_score(small, "SOCP", lib_path=twin_lib)
    n = len(small.range_measurements)
    for w in (np.ones(n + 1), np.ones(n - 1), np.ones((n, 1))):
        with pytest.raises(ValueError, match="range_weights"):
            refine_estimate(small, res, lib_path=twin_lib, range_weights=w)
    with pytest.raises(ValueError, match="range_weights"):
        refine_estimate(small, res, lib_path=twin_lib, range_weights=-np.ones(n))
