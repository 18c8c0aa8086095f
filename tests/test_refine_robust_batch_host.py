"""Batched outlier-robust refinement without a GPU: the Python lock-step engine (score_amd/refine_robust_batch.py) against
``refine_estimate_robust`` on every member alone -- it only reorders independent work, so the results are EQUAL --, the argument
checks, and the binding of include/score_refine_robust_batch.h.

The graphs (tests/refine_robust_batch_helpers.py), Python engine with SciPy's LU, both families on: G1 33 outer solves / 211 LM
iterations, G2 26 / 168, G3 (schedule 3 / 3) 17 / 54; G4 (c = 5) and the clean 3-D graph (seed 43, c = 5, schedule 3 / 3) stop
after solve 1 with max r^2 = 7.93 and 5.38 against the outlier bound c^2 / 2 = 12.5: in a group the members leave the schedule at
different times."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from refine_robust_batch_helpers import CLEAN3, LM_ITERATIONS, OUTER, THRESHOLD, batch, graph, landmarks_of, poses_of, single
from score_amd.manhattan import make_manhattan
from score_amd.refine_robust_batch import REFINE_ROBUST_BATCH_SYMBOLS, refine_estimate_robust_batch
from score_amd.solver import load_library


def _assert_equal_to_single(key, got):
    fg = graph(key)[0]
    (res, info), (res_s, info_s) = got, single(key)
    np.testing.assert_array_equal(poses_of(fg, res), poses_of(fg, res_s))
    np.testing.assert_array_equal(landmarks_of(fg, res), landmarks_of(fg, res_s))
    rb, rs = info["robust"], info_s["robust"]
    for name in ("weights", "residuals", "outliers", "loop_closure_weights", "loop_closure_residuals", "loop_closure_outliers"):
        np.testing.assert_array_equal(rb[name], rs[name], err_msg=f"{key}: {name}")
    assert rb["outer_iterations"] == rs["outer_iterations"] == OUTER[key]
    assert rb["mu"] == rs["mu"] and rb["converged"] == rs["converged"]
    for name in ("iterations", "cost_initial", "cost_final", "grad_inf"):
        assert info[name] == info_s[name], (key, name)
    if key in LM_ITERATIONS:
        assert info["iterations"] == LM_ITERATIONS[key]


def test_python_engine_equals_the_single_loop_member_by_member():
    keys = ["G1", "G4", "G2"]
    out = batch(keys)
    for key, got in zip(keys, out):
        _assert_equal_to_single(key, got)
    assert {info["group"] for _, info in out} == {0}
    # the members leave the schedule at different times: the group runs as long as its longest member
    assert out[0][1]["rounds"] == max(info["linear_solves"] for _, info in out)
    assert out[0][1]["stage_rounds"] >= OUTER["G1"]


def test_python_engine_equals_the_single_loop_in_3d():
    keys = ["G3", CLEAN3]
    for key, got in zip(keys, batch(keys)):
        _assert_equal_to_single(key, got)


def test_mixed_dimensions_come_back_in_input_order_in_two_groups():
    keys = ["G3", "G1", CLEAN3, "G4"]
    out = batch(keys, max_iters=3, inner_iters=3)
    assert [info["group"] for _, info in out] == [1, 0, 1, 0]
    for key, (res, info) in zip(keys, out):
        fg = graph(key)[0]
        assert len(info["robust"]["weights"]) == len(fg.range_measurements)
        assert poses_of(fg, res).shape[1] == fg.dimension + 1
    for key, got in zip(keys, out):
        if graph(key)[0].dimension == 3:  # (their own schedule)
            _assert_equal_to_single(key, got)


@pytest.mark.parametrize("key", ["G4", CLEAN3])
def test_clean_members_stay_clear_of_the_outlier_bound(key):
    """After solve 1, max r^2 over the enabled families is at most two thirds of c^2 / 2: the rounding of the device's
    conjugate-gradient solves cannot flip the "no outliers" decision."""
    _, info = single(key)
    rb = info["robust"]
    assert rb["outer_iterations"] == 1 and rb["converged"] and rb["mu"] == 0.0
    r = np.concatenate([rb["residuals"], rb["loop_closure_residuals"]])
    worst, bound = float(np.max(r * r)), THRESHOLD[key] ** 2 / 2.0
    print(key, "max r^2", worst, "bound", bound)
    assert worst <= 2.0 / 3.0 * bound


def test_argument_checks():
    fgs, starts = [graph(k)[0] for k in ("G1", "G2")], [graph(k)[1] for k in ("G1", "G2")]
    run = lambda *a, **kw: refine_estimate_robust_batch(*a, engine="python", **kw)  # noqa: E731
    with pytest.raises(ValueError, match="inlier_threshold: a scalar or one entry per graph"):
        run(fgs, starts, inlier_threshold=[3.0, 3.0, 3.0])
    with pytest.raises(ValueError, match="loop_closure_threshold: a scalar or one entry per graph"):
        run(fgs, starts, robust_loop_closures=True, loop_closure_threshold=[3.0])
    with pytest.raises(ValueError, match=r"^graph 1: inlier_threshold must be positive"):
        run(fgs, starts, inlier_threshold=[3.0, -1.0])
    with pytest.raises(ValueError, match="one estimate per graph expected"):
        run(fgs, starts[:1])
    with pytest.raises(ValueError, match="range_weights: one entry per graph"):
        run(fgs, starts, range_weights=[None])
    with pytest.raises(ValueError, match="engine must be"):
        refine_estimate_robust_batch(fgs, starts, engine="eager")
    with pytest.raises(ValueError, match="max_group must be at least 1"):
        run(fgs, starts, max_group=0)
    with pytest.raises(ValueError, match="nothing to re-weight"):
        run(fgs, starts, robust_ranges=False)
    with pytest.raises(ValueError, match="max_outer must be >= 1"):
        run(fgs, starts, max_outer=0)


def test_a_bad_precision_names_its_graph():
    fg_bad = make_manhattan(seed=9, n_robots=2, n_poses=25, n_beacons=2, p_range=0.5, n_loop_closures=3)
    fg_bad.range_measurements[3].stddev = float("inf")  # precision 0
    fgs, starts = [graph("G2")[0], fg_bad], [graph("G2")[1], graph("G2")[1]]
    with pytest.raises(ValueError, match=r"^graph 1: every range precision must be positive and finite"):
        refine_estimate_robust_batch(fgs, starts, engine="python")
    # ... only in an enabled family
    out = refine_estimate_robust_batch(fgs, starts, engine="python", robust_ranges=False, robust_loop_closures=True, max_outer=1)
    assert len(out) == 2


def test_a_graph_without_unknowns_is_answered_on_the_host():
    from refine_robust_helpers import start_of

    fg0 = make_manhattan(seed=2, n_robots=1, n_poses=1, n_beacons=0, p_range=0.0, n_loop_closures=0)

    keys = ["G2"]
    out = refine_estimate_robust_batch([fg0, graph("G2")[0]], [start_of(fg0), graph("G2")[1]], inlier_threshold=[3.0, THRESHOLD["G2"]],
                                       robust_loop_closures=True, engine="python")
    (res0, info0), got = out
    from score_amd.refine_robust import refine_estimate_robust

    _, alone = refine_estimate_robust(fg0, start_of(fg0), robust_loop_closures=True, engine="python", linear_solver="scipy")
    assert info0["iterations"] == alone["iterations"] and info0["cost_final"] == alone["cost_final"] == 0.0
    assert info0["robust"]["outer_iterations"] == 1 and len(info0["robust"]["weights"]) == 0 and "group" not in info0
    _assert_equal_to_single(keys[0], got)


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "score_refine_robust_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(score_[a-z_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert _declared_symbols() == sorted(REFINE_ROBUST_BATCH_SYMBOLS)
    for sym in ("score_refine_batch_robust_run", "score_refine_batch_residuals", "score_refine_batch_restore"):
        assert sym in REFINE_ROBUST_BATCH_SYMBOLS


def test_hip_library_exports_the_declared_symbols(hip_lib):
    lib = load_library(hip_lib)
    for sym in _declared_symbols():
        assert hasattr(lib, sym), sym
