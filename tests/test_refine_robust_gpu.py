"""Outlier-robust refinement on the device (include/score_refine_robust.h, csrc/score_gn_robust.hpp) against the Python engine.

Tolerances.  Residuals: rtol 1e-11 between the kernel and the NumPy twin -- both fp64 with the same operations; 100 x the 1e-13
the suite holds for the summed cost between the native and the Python engine.  A weight strictly between the thresholds is
w = c / r sqrt(mu (mu + 1)) - mu: the product carries the residual's relative error, so |w - w_ref| <= 1e-11 (w_ref + mu) plus
the rounding of the subtraction; beyond the thresholds (by more than the residual's tolerance on r^2) it is exactly 0 or 1.
The loop: outer counts, outlier sets and final weights equal; mu rel 1e-9; poses atol 1e-7 and cost rel 1e-7 between the native
and the Python engine on the same library (what test_native_refinement_blocks_match_the_python_jacobian holds between them),
poses 1e-5 against SciPy's LU (what tests/test_refine.py holds between the two linear solvers)."""
import numpy as np
import pytest

from refine_robust_helpers import THRESHOLD, corrupt, graph, point_of, start_of, twin
from score_amd.manhattan import make_manhattan
from score_amd.refine import refine_estimate
from score_amd.refine_robust import (RobustRefineHandle, loop_closure_residuals, range_residuals, refine_estimate_robust)
from score_amd.robust import gnc_tls_weight, n_loop_closures_of

pytestmark = pytest.mark.gpu

RTOL = 1e-11
SCHEDULE = {"G1": {}, "G2": {}, "G3": dict(max_iters=3, inner_iters=3)}


def _g2_touching_the_pinned_pose():
    """G2's graph with range 0 and loop closure 1 re-attached to pose 0 (the pinned pose: the first entry of the state, which never receives a step)."""
    fg = make_manhattan(seed=9, n_robots=2, n_poses=25, n_beacons=2, p_range=0.5, n_loop_closures=3)
    corrupt(fg, 9, (0,))
    first = fg.pose_variables[0][0].name
    m = fg.range_measurements[0]
    m.association = (first, m.association[1])
    fg.loop_closure_measurements[1].base_pose = first
    return fg


def _check_entries(fg, hip_lib, c=3.0, c_rel=2.5):
    """score_refine_residuals at the noisy start against the NumPy twin, entry by entry, for every mu."""
    prob, point = point_of(fg, start_of(fg))
    n_lc = n_loop_closures_of(prob.a)
    ne = len(prob.bi)
    ref = {"ranges": (range_residuals(prob, point, prob.a["rng_prec"]), c),
           "loop closures": (loop_closure_residuals(prob, point, prob.a["rel_kappa"][ne - n_lc:], prob.a["rel_tau"][ne - n_lc:]), c_rel)}
    classes = set()
    with RobustRefineHandle(prob, hip_lib) as h:
        for mu in (0.0, 1e-3, 1.0, 1e3):
            r, rl, w, wl = h.residuals(point, mu, c, c_rel)
            for name, got_r, got_w in (("ranges", r, w), ("loop closures", rl, wl)):
                want_r, cf = ref[name]
                assert got_r.shape == want_r.shape == got_w.shape
                if len(want_r):
                    print(name, "mu", mu, "worst relative residual difference", float(np.max(np.abs(got_r - want_r) / np.maximum(want_r, 1e-300))))
                np.testing.assert_allclose(got_r, want_r, rtol=RTOL, atol=0)
                if mu == 0.0:
                    assert np.all(got_w == 1.0)
                    continue
                want_w = gnc_tls_weight(want_r, mu, cf)
                r2, lo, hi = want_r * want_r, mu / (mu + 1.0) * cf * cf, (mu + 1.0) / mu * cf * cf
                margin = 4.0 * RTOL  # on r^2: twice the residual's tolerance, twice over
                inl, out = r2 <= lo * (1.0 - margin), r2 >= hi * (1.0 + margin)
                mid = (r2 >= lo * (1.0 + margin)) & (r2 <= hi * (1.0 - margin))
                assert np.all(got_w[inl] == 1.0) and np.all(got_w[out] == 0.0)
                assert np.all(np.abs(got_w[mid] - want_w[mid]) <= RTOL * (want_w[mid] + mu) + 4 * np.finfo(float).eps * (1.0 + mu))
                assert np.all((got_w >= 0.0) & (got_w <= 1.0))
                if name == "ranges":
                    classes |= {k for k, m in (("in", inl), ("mid", mid), ("out", out)) if np.any(m)}
    return classes, len(ref["ranges"][0]), n_lc


def test_kernels_entry_by_entry_2d(hip_lib):
    fg = graph("G1")[0]
    classes, nr, n_lc = _check_entries(fg, hip_lib)
    assert (nr, n_lc) == (185, 4)  # one block: the ranges, then the loop closures
    assert classes == {"in", "mid", "out"}  # every branch of the weight rule was taken


def test_kernels_entry_by_entry_3d(hip_lib):
    classes, nr, n_lc = _check_entries(graph("G3")[0], hip_lib)
    assert (nr, n_lc) == (78, 3) and classes == {"in", "mid", "out"}


def test_kernels_at_the_pinned_pose(hip_lib):
    fg = _g2_touching_the_pinned_pose()
    prob, _ = point_of(fg, start_of(fg))
    assert prob.ra[0] == 0 and prob.bi[len(prob.bi) - 2] == 0
    _check_entries(fg, hip_lib)


def test_more_than_one_block(hip_lib):
    """300 ranges and 4 loop closures: two blocks, the loop closures in the second one behind the last ranges."""
    fg = make_manhattan(seed=3, n_robots=3, n_poses=60, n_beacons=3, p_range=0.6, n_loop_closures=4)
    corrupt(fg, 3, (2,))
    _, nr, n_lc = _check_entries(fg, hip_lib)
    print("ranges", nr, "loop closures", n_lc)
    assert 256 < nr < 512 and nr + n_lc > 256


def test_empty_families(hip_lib):
    # no loop closures, that family enabled
    fg = make_manhattan(seed=2, n_robots=2, n_poses=15, n_beacons=2, p_range=0.5, n_loop_closures=0)
    bad, _ = corrupt(fg, 2)
    _, nr, n_lc = _check_entries(fg, hip_lib)
    assert n_lc == 0 and nr > 0
    start = start_of(fg)
    res, info = refine_estimate_robust(fg, start, robust_loop_closures=True, lib_path=hip_lib)
    ref, rinfo = refine_estimate_robust(fg, start, robust_loop_closures=True, engine="python", linear_solver="device", lib_path=hip_lib)
    rb = info["robust"]
    assert rb["loop_closure_weights"].shape == (0,) and rb["outer_iterations"] == rinfo["robust"]["outer_iterations"] > 1
    np.testing.assert_array_equal(rb["weights"], rinfo["robust"]["weights"])
    # no ranges (and no beacons): 2 x 15 poses, 2 loop closures
    fg = make_manhattan(seed=2, n_robots=2, n_poses=15, n_beacons=0, p_range=0.0, n_loop_closures=2)
    assert len(fg.range_measurements) == 0
    _, nr, n_lc = _check_entries(fg, hip_lib)
    assert (nr, n_lc) == (0, 2)
    start = start_of(fg)
    plain, pinfo = refine_estimate(fg, start, lib_path=hip_lib)
    for kw in (dict(robust_loop_closures=True), dict()):  # both families | the ranges alone: every enabled family is empty
        res, info = refine_estimate_robust(fg, start, lib_path=hip_lib, **kw)
        rb = info["robust"]
        assert rb["outer_iterations"] == 1 and rb["converged"] and rb["weights"].shape == (0,)
        assert info["cost_final"] == pinfo["cost_final"]
        for nm in plain.poses:
            np.testing.assert_array_equal(res.poses[nm], plain.poses[nm])


@pytest.mark.parametrize("key", ["G1", "G2", "G3"])
def test_device_loop_matches_the_python_engine(key, hip_lib):
    fg, start, bad, _, lc_bad = graph(key)
    res, info = refine_estimate_robust(fg, start, inlier_threshold=THRESHOLD[key], robust_loop_closures=True, lib_path=hip_lib,
                                       **SCHEDULE[key])
    ref, rinfo = twin(key, "device", hip_lib, **SCHEDULE[key])
    a, b = info["robust"], rinfo["robust"]
    print(key, "native: outer", a["outer_iterations"], "mu", a["mu"], "lm", info["iterations"], "pcg", info["pcg_iters"], "solve ms", info["solve_ms"],
          "| python: outer", b["outer_iterations"], "mu", b["mu"], "lm", rinfo["iterations"])
    print(key, "worst pose difference", max(float(np.max(np.abs(res.poses[nm] - ref.poses[nm]))) for nm in ref.poses),
          "cost", info["cost_final"], rinfo["cost_final"])
    assert info["engine"] == "native"
    assert a["outer_iterations"] == b["outer_iterations"] and a["converged"] == b["converged"] and a["converged"]
    np.testing.assert_array_equal(a["outliers"], b["outliers"])
    np.testing.assert_array_equal(a["loop_closure_outliers"], b["loop_closure_outliers"])
    np.testing.assert_array_equal(a["weights"], b["weights"])
    np.testing.assert_array_equal(a["loop_closure_weights"], b["loop_closure_weights"])
    assert a["mu"] == pytest.approx(b["mu"], rel=1e-9)
    assert info["cost_final"] == pytest.approx(rinfo["cost_final"], rel=1e-7)
    for nm in ref.poses:
        np.testing.assert_allclose(res.poses[nm], ref.poses[nm], atol=1e-7)
    for nm in ref.landmarks:
        np.testing.assert_allclose(res.landmarks[nm], ref.landmarks[nm], atol=1e-7)
    # the reported residuals are those of the final estimate
    prob, point = point_of(fg, res)
    np.testing.assert_allclose(a["residuals"], range_residuals(prob, point, prob.a["rng_prec"]), rtol=1e-9)
    # against SciPy's LU: the same sets, the estimate to what the two linear solvers agree to
    sres, sinfo = twin(key, **SCHEDULE[key])
    np.testing.assert_array_equal(a["outliers"], sinfo["robust"]["outliers"])
    np.testing.assert_array_equal(a["loop_closure_outliers"], sinfo["robust"]["loop_closure_outliers"])
    for nm in sres.poses:
        np.testing.assert_allclose(res.poses[nm], sres.poses[nm], atol=1e-5)
    # the planted sets
    np.testing.assert_array_equal(a["outliers"], bad)
    np.testing.assert_array_equal(a["loop_closure_outliers"], lc_bad)


def test_no_outliers_is_refine_estimate_bit_for_bit(hip_lib):
    fg, start, *_ = graph("G4")
    res, info = refine_estimate_robust(fg, start, inlier_threshold=THRESHOLD["G4"], robust_loop_closures=True, lib_path=hip_lib)
    plain, pinfo = refine_estimate(fg, start, lib_path=hip_lib)
    rb = info["robust"]
    assert rb["outer_iterations"] == 1 and rb["converged"] and rb["mu"] == 0.0
    assert np.all(rb["weights"] == 1.0) and np.all(rb["loop_closure_weights"] == 1.0)
    assert len(rb["outliers"]) == 0 and len(rb["loop_closure_outliers"]) == 0
    assert info["cost_final"] == pinfo["cost_final"] and info["iterations"] == pinfo["iterations"]
    assert info["cost_initial"] == pinfo["cost_initial"] and info["grad_inf"] == pinfo["grad_inf"]
    for nm in plain.poses:
        np.testing.assert_array_equal(res.poses[nm], plain.poses[nm])
    for nm in plain.landmarks:
        np.testing.assert_array_equal(res.landmarks[nm], plain.landmarks[nm])


def test_the_handle_afterwards(hip_lib):
    fg, start, bad, _, lc_bad = graph("G2")
    prob, point = point_of(fg, start)
    with RobustRefineHandle(prob, hip_lib) as fresh:
        want, want_info = fresh.run(point)
    with RobustRefineHandle(prob, hip_lib) as h:
        rs = h.default_settings()
        rs.families = 3
        u, w, r, wl, rl, info = h.robust_run(point, rs)
        assert info["converged"] == 1 and info["outliers"] == len(bad) and info["rel_outliers"] == len(lc_bad)
        np.testing.assert_array_equal(np.nonzero(w < 0.5)[0], bad)
        got, got_info = h.run(point)  # the measured precisions are back
        np.testing.assert_array_equal(got, want)
        for k in ("cost_initial", "cost_final", "grad_inf", "iterations", "linear_solves", "pcg_iters"):
            assert got_info[k] == want_info[k], k
        # stopped by max_outer: not converged, outputs written
        rs.max_outer = 2
        u2, w2, r2, wl2, rl2, info2 = h.robust_run(point, rs)
        assert info2["converged"] == 0 and info2["outer_iterations"] == 2 and info2["mu"] > 0
        assert np.all(np.isfinite(u2)) and np.all(np.isfinite(r2)) and np.all((w2 >= 0) & (w2 <= 1)) and np.any((w2 > 0) & (w2 < 1))
        assert info2["cost_final"] < info2["cost_initial"]
        np.testing.assert_array_equal(h.run(point)[0], want)
        # an error return leaves the handle as it was, too
        rs.families = 0
        with pytest.raises(RuntimeError, match="families"):
            h.robust_run(point, rs)
        rs.families, rs.min_weight = 3, 0.0
        with pytest.raises(RuntimeError, match="min_weight"):
            h.robust_run(point, rs)
        np.testing.assert_array_equal(h.run(point)[0], want)
        # score_refine_residuals does not touch the precisions either
        h.residuals(point, 1.0, 3.0, 3.0)
        np.testing.assert_array_equal(h.run(point)[0], want)


def test_pipeline_relaxation_refinement_marginals(hip_lib):
    """solve_score_robust -> refine_estimate_robust on its weights -> marginal_covariances on the final weights.  The relaxation
    cannot see a range measured too long (weight 1 there); the refinement's loop takes every planted long range out."""
    from marginals_helpers import Reference, check_columns
    from score_amd.marginals import marginal_covariances
    from score_amd.robust import solve_score_robust

    fg, _, bad, long_, _ = graph("G1")
    relaxed = solve_score_robust(fg, solver_settings=dict(device=0), lib_path=hip_lib)
    rw = relaxed.info["robust"]["weights"]
    assert np.all(rw[bad[long_]] == 1.0)
    res, info = refine_estimate_robust(fg, relaxed, range_weights=rw, lib_path=hip_lib)
    w = info["robust"]["weights"]
    print("relaxation flagged", relaxed.info["robust"]["outliers"], "refinement: outer", info["robust"]["outer_iterations"], "flagged",
          len(info["robust"]["outliers"]))
    assert np.all(w[bad[long_]] == 0.0)
    assert np.all(w <= rw)  # prior x GNC
    cov, minfo = marginal_covariances(fg, res, joint=True, range_weights=w, lib_path=hip_lib)
    ref = Reference(fg, res, range_weights=w)
    names, cols = ref.columns(None)
    A = minfo["joint_raw"]
    _, bound, _ = check_columns(ref, cols, A, minfo["residuals"], "G1 pipeline")
    assert np.all(np.isfinite(A)) and all(np.all(np.isfinite(b)) for b in cov.values())
    assert np.all(np.abs(A - A.T) <= bound[:, None] + bound[None, :])
    for b in cov.values():
        np.testing.assert_array_equal(b, b.T)
