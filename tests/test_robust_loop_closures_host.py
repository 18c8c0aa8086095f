"""GNC-TLS re-weighting of the loop closures (score_amd/robust.py: robust_loop_closures=True) on the CPU: the residual's NumPy
statement, the loop's readable twin (engine="python") on the oracle's CPU twin of the library, alone and together with the
ranges, and the weighted refinement (refine_estimate(loop_closure_weights=...))."""
import logging

import numpy as np
import pytest

from conftest import graph_by_name
from score_amd.manhattan import make_manhattan, make_manhattan_3d
from score_amd.native import ArrayGraph, graph_arrays
from score_amd.refine import refine_estimate
from score_amd.robust import corrupt_loop_closures, corrupt_ranges, relaxed_loop_closure_residuals, solve_score_robust
from score_amd.solve_score import solve_score

# Calibrated on the twin (engine="python").  False place recognitions: corrupt_loop_closures' draw (translation U(-8, 8)^d, a
# uniform rotation angle / rotation vector), precisions kept.  "gap": robot A's translations against the plain solve of the
# uncorrupted graph.
#   G2 = 1 robot x 80 poses, 3 beacons, 10 loop closures, 2 corrupted, the loop closures' family alone:
#     seed 3: injected {0, 7}, flagged {0, 7, 9}, 15 outer solves, gap 5.7e-2, plain solve of the corrupted graph 12.5
#     seed 5: injected {6, 8}, flagged {6, 8}, 24 outer solves, gap 2.8e-2, plain 10.9
#   G2 seed 5, plus 5 % of the ranges shortened, both families: flagged exactly {6, 8} and the ranges {2, 53, 59, 73, 89, 91}
#     (the injected ones), 24 outer solves, gap 2.8e-2
#   G3 = 3-D, 1 robot x 40 poses, 3 beacons, 6 loop closures, 1 corrupted, seed 2: injected = flagged = {5}, 24 outer solves,
#     gap 2.1e-2, plain 11.0
G2 = dict(n_robots=1, n_poses=80, n_beacons=3, p_range=0.5, sigma_range=0.1, n_loop_closures=10)
G3 = dict(n_robots=1, n_poses=40, n_beacons=3, p_range=0.5, sigma_range=0.1, n_loop_closures=6)


def _robot_a_gap(a, b, fg):
    names = [p.name for p in fg.pose_variables[0]]
    return max(float(np.max(np.abs(a.poses[k][:-1, -1] - b.poses[k][:-1, -1]))) for k in names)


def _quiet(fn):
    logging.disable(logging.WARNING)  # (the twin's ADMM loop reaches its iteration cap on these graphs: it says so)
    try:
        return fn()
    finally:
        logging.disable(logging.NOTSET)


def _literal_residuals(fg, res):
    """r_e of every loop closure, measurement object by measurement object, from the relaxed blocks [R | t]."""
    d = fg.dimension
    first = fg.pose_variables[0][0].name
    out = []
    for m in fg.loop_closure_measurements:
        Xi = np.hstack([np.eye(d), np.zeros((d, 1))]) if m.base_pose == first else np.asarray(res.relaxed_poses[m.base_pose])
        Xj = np.hstack([np.eye(d), np.zeros((d, 1))]) if m.to_pose == first else np.asarray(res.relaxed_poses[m.to_pose])
        dt = Xj[:, d] - Xi[:, d] - Xi[:, :d] @ np.asarray(m.translation_vector, dtype=np.float64)
        dR = Xj[:, :d] - Xi[:, :d] @ np.asarray(m.rotation_matrix, dtype=np.float64)
        out.append(np.sqrt(m.translation_precision * float(dt @ dt) + m.rotation_precision * float(np.sum(dR * dR))))
    return np.array(out)


@pytest.mark.parametrize("name", ["synth_b", "graph3d"])
def test_residual_function_is_the_objective_term(name, fixtures, twin_lib):
    fg = graph_by_name(name, fixtures)
    res = solve_score(fg, "SOCP", lib_path=twin_lib)
    r = relaxed_loop_closure_residuals(graph_arrays(fg), res.relaxed_poses.array)
    ref = _literal_residuals(fg, res)
    print(name, r)                                              # measured: synth_b [0.273, 0, 0, 0]; graph3d [5.489]
    assert r.shape == (len(fg.loop_closure_measurements),)
    np.testing.assert_allclose(r, ref, rtol=1e-12, atol=1e-12 * float(np.max(ref)))
    assert float(np.max(r)) > 0.1


def test_clean_graph_is_one_plain_solve(fixtures, twin_lib):
    fg = graph_by_name("synth_b", fixtures)
    rob = solve_score_robust(fg, engine="python", lib_path=twin_lib, robust_loop_closures=True)
    ref = solve_score(fg, lib_path=twin_lib)
    info = rob.info["robust"]
    assert info["outer_iterations"] == 1 and info["converged"]
    assert len(info["outliers"]) == 0 and len(info["loop_closure_outliers"]) == 0
    np.testing.assert_array_equal(info["weights"], np.ones(len(fg.range_measurements)))
    np.testing.assert_array_equal(info["loop_closure_weights"], np.ones(len(fg.loop_closure_measurements)))
    for nm in ref.poses:
        np.testing.assert_array_equal(rob.poses[nm], ref.poses[nm])
    r = relaxed_loop_closure_residuals(graph_arrays(fg), ref.relaxed_poses.array)
    np.testing.assert_array_equal(info["loop_closure_residuals"], r)
    # measured: the largest loop-closure r is 0.273, the largest range r 4.5e-7
    assert 2 * float(np.max(r)) ** 2 <= 9.0 and 2 * float(np.max(info["residuals"])) ** 2 <= 9.0
    # the defaults keep today's keys
    plain = solve_score_robust(fg, engine="python", lib_path=twin_lib)
    assert sorted(plain.info["robust"]) == ["converged", "mu", "outer_iterations", "outliers", "residuals", "weights"]


@pytest.mark.parametrize("seed", [3, 5])
def test_corrupted_loop_closures_are_discounted(seed, twin_lib):
    fg = make_manhattan(seed=seed, **G2)
    bad_g, bad = corrupt_loop_closures(fg, 2, seed=seed)
    assert len(bad) == 2 and len(set(bad.tolist())) == 2
    rob = _quiet(lambda: solve_score_robust(bad_g, "SOCP", engine="python", lib_path=twin_lib, robust_ranges=False,
                                            robust_loop_closures=True))
    clean = _quiet(lambda: solve_score(fg, "SOCP", lib_path=twin_lib))
    plain = _quiet(lambda: solve_score(bad_g, "SOCP", lib_path=twin_lib))
    info = rob.info["robust"]
    w = info["loop_closure_weights"]
    flagged, injected = set(info["loop_closure_outliers"].tolist()), set(bad.tolist())
    near, far = _robot_a_gap(rob, clean, fg), _robot_a_gap(plain, clean, fg)
    print(seed, sorted(flagged), sorted(injected), info["outer_iterations"], near, far)
    assert info["converged"] and 1 < info["outer_iterations"] < 50
    assert w.shape == (10,) and np.all((w < 1e-6) | (w > 1 - 1e-6))
    assert injected <= flagged
    assert len(flagged - injected) <= 1
    np.testing.assert_array_equal(info["weights"], np.ones(len(bad_g.arrays["rng_a"])))   # (the ranges keep weight 1)
    assert near < 0.1 and far > 5.0, (near, far)


def test_both_families(twin_lib):
    fg = make_manhattan(seed=5, **G2)
    g1, bad_lc = corrupt_loop_closures(fg, 2, seed=5)
    g2, bad_rng = corrupt_ranges(g1, 0.05, seed=5)
    nr = len(g2.arrays["rng_a"])
    rob = _quiet(lambda: solve_score_robust(g2, "SOCP", engine="python", lib_path=twin_lib, robust_loop_closures=True))
    clean = _quiet(lambda: solve_score(fg, "SOCP", lib_path=twin_lib))
    info = rob.info["robust"]
    f_lc, i_lc = set(info["loop_closure_outliers"].tolist()), set(bad_lc.tolist())
    f_rng, i_rng = set(info["outliers"].tolist()), set(bad_rng.tolist())
    near = _robot_a_gap(rob, clean, fg)
    print(sorted(f_lc), sorted(i_lc), sorted(f_rng), sorted(i_rng), info["outer_iterations"], near)
    assert i_lc <= f_lc and i_rng <= f_rng
    assert len(f_lc - i_lc) <= 1 and len(f_rng - i_rng) <= 0.02 * (nr - len(i_rng))
    assert near < 0.1, near


def test_three_dimensions(twin_lib):
    fg = make_manhattan_3d(seed=2, **G3)
    bad_g, bad = corrupt_loop_closures(fg, 1, seed=2)
    rob = _quiet(lambda: solve_score_robust(bad_g, "SOCP", engine="python", lib_path=twin_lib, robust_ranges=False,
                                            robust_loop_closures=True))
    clean = _quiet(lambda: solve_score(fg, "SOCP", lib_path=twin_lib))
    plain = _quiet(lambda: solve_score(bad_g, "SOCP", lib_path=twin_lib))
    info = rob.info["robust"]
    near, far = _robot_a_gap(rob, clean, fg), _robot_a_gap(plain, clean, fg)
    print(info["loop_closure_outliers"], bad, info["outer_iterations"], near, far)
    np.testing.assert_array_equal(info["loop_closure_outliers"], bad)
    assert near < 0.1 and far > 3.0, (near, far)


def test_loop_closure_weights_in_the_refinement(twin_lib):
    kw = dict(n_robots=1, n_poses=40, n_beacons=3, seed=21, p_range=0.6, n_loop_closures=4)
    fg = make_manhattan(**kw)
    res = solve_score(fg, "SOCP", lib_path=twin_lib)
    n = len(fg.loop_closure_measurements)
    assert n == 4
    a, ia = refine_estimate(fg, res, lib_path=twin_lib)
    b, ib = refine_estimate(fg, res, lib_path=twin_lib, loop_closure_weights=np.ones(n))
    assert ia["cost_final"] == ib["cost_final"]
    for nm in a.poses:
        np.testing.assert_array_equal(a.poses[nm], b.poses[nm])
    # a zero weight is the loop closure taken out
    w = np.ones(n)
    w[2] = 0.0
    fg2 = make_manhattan(**kw)
    del fg2.loop_closure_measurements[2]
    for engine in ("native", "python"):
        c, ic = refine_estimate(fg, res, lib_path=twin_lib, loop_closure_weights=w, engine=engine)
        d, id_ = refine_estimate(fg2, res, lib_path=twin_lib, engine=engine)
        assert ic["cost_final"] == pytest.approx(id_["cost_final"], rel=1e-9, abs=1e-12)
        for nm in c.poses:
            np.testing.assert_allclose(c.poses[nm], d.poses[nm], atol=1e-7)
        for nm in c.landmarks:
            np.testing.assert_allclose(c.landmarks[nm], d.landmarks[nm], atol=1e-7)
        assert ic["cost_final"] < ia["cost_final"]
    for bad in (np.ones(n + 1), np.ones(n - 1), np.ones((n, 1)), -np.ones(n)):
        with pytest.raises(ValueError, match="loop_closure_weights"):
            refine_estimate(fg, res, lib_path=twin_lib, loop_closure_weights=bad)


def test_loop_closure_weights_in_the_refinement_3d(twin_lib):
    fg = make_manhattan_3d(n_robots=1, n_poses=20, n_beacons=3, seed=4, p_range=0.6, n_loop_closures=3)
    res = solve_score(fg, "SOCP", lib_path=twin_lib)
    a, ia = refine_estimate(fg, res, lib_path=twin_lib)
    b, ib = refine_estimate(fg, res, lib_path=twin_lib, loop_closure_weights=np.ones(3))
    assert ia["cost_final"] == ib["cost_final"]
    for nm in a.poses:
        np.testing.assert_array_equal(a.poses[nm], b.poses[nm])
    w = np.array([1.0, 0.0, 1.0])
    fg2 = make_manhattan_3d(n_robots=1, n_poses=20, n_beacons=3, seed=4, p_range=0.6, n_loop_closures=3)
    del fg2.loop_closure_measurements[1]
    c, ic = refine_estimate(fg, res, lib_path=twin_lib, loop_closure_weights=w)
    d, id_ = refine_estimate(fg2, res, lib_path=twin_lib)
    assert ic["cost_final"] == pytest.approx(id_["cost_final"], rel=1e-9, abs=1e-12)
    for nm in c.poses:
        np.testing.assert_allclose(c.poses[nm], d.poses[nm], atol=1e-7)
    with pytest.raises(ValueError, match="loop_closure_weights"):
        refine_estimate(fg, res, lib_path=twin_lib, loop_closure_weights=np.ones(4))


def test_argument_errors(fixtures, twin_lib):
    fg = graph_by_name("synth_b", fixtures)
    with pytest.raises(ValueError, match="both off"):
        solve_score_robust(fg, engine="python", lib_path=twin_lib, robust_ranges=False)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="loop_closure_threshold"):
            solve_score_robust(fg, engine="python", lib_path=twin_lib, robust_loop_closures=True, loop_closure_threshold=bad)
    a = dict(graph_arrays(fg))
    a["rel_kappa"] = a["rel_kappa"].copy()
    a["rel_kappa"][-2] = 0.0
    with pytest.raises(ValueError, match="precision"):
        solve_score_robust(ArrayGraph(a), engine="python", lib_path=twin_lib, robust_loop_closures=True)
    a["rel_kappa"][-2] = a["rel_kappa"][-1]
    a["rel_tau"] = a["rel_tau"].copy()
    a["rel_tau"][-1] = float("inf")
    with pytest.raises(ValueError, match="precision"):
        solve_score_robust(ArrayGraph(a), engine="python", lib_path=twin_lib, robust_loop_closures=True)
