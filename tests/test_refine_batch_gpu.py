"""Batched refinement on the device (include/score_refine_batch.h, csrc/score_gn_batch.hpp) against the single handle
(``refine_estimate(engine="native")`` on every member alone) and against the Python engine with SciPy's sparse LU.

Tolerances are the project's own (tests/test_refine.py): between two device runs of the same loop that differ only in the
rounding of their conjugate-gradient solves, poses and landmarks agree to atol 1e-7 in 2-D and 1e-5 in 3-D; against SciPy's LU
to 1e-5.  Every member ends with |g|_inf < 1e-5 max(1, cost) and a cost no larger than it started with."""
import ctypes as C
import functools

import numpy as np
import pytest

from marginals_helpers import undetermined_graph
from refine_batch_helpers import (KEYS_2D, MILD, arrays_of, check_fixture, group, member, native_alone, noisy_truth, rough_start,
                                  twin_alone)
from refine_robust_helpers import point_of, start_of
from score_amd import compat
from score_amd.manhattan import make_manhattan, make_manhattan_3d
from score_amd.refine import _as_results, refine_estimate
from score_amd.refine_batch import RefineBatchHandle, _bind, _problem_of, refine_estimate_batch
from score_amd.refine_robust import RobustRefineHandle
from score_amd.robust import n_loop_closures_of

pytestmark = pytest.mark.gpu

ATOL = {2: 1e-7, 3: 1e-5}
ATOL_LU = 1e-5


def _close(fg, got, want, atol):
    worst = 0.0
    for a, b in zip(arrays_of(fg, got), arrays_of(fg, want)):
        assert a.shape == b.shape
        if a.size:
            worst = max(worst, float(np.max(np.abs(a - b))))
    return worst, worst <= atol


def _check_member(label, fg, got, info, single, sinfo, lu=None):
    print(f"{label}: batch iterations {info['iterations']} solves {info['linear_solves']} pcg {info['pcg_iters']} | single handle "
          f"iterations {sinfo['iterations']} solves {sinfo['linear_solves']} pcg {sinfo['pcg_iters']} | cost {info['cost_final']:.12g} "
          f"vs {sinfo['cost_final']:.12g} | grad {info['grad_inf']:.3e}")
    worst, ok = _close(fg, got, single, ATOL[fg.dimension])
    print(f"{label}: worst difference to the single handle {worst:.3e}")
    assert ok, f"{label}: differs from the single handle by {worst:.3e}"
    if lu is not None:
        worst, ok = _close(fg, got, lu, ATOL_LU)
        print(f"{label}: worst difference to SciPy's LU {worst:.3e}")
        assert ok, f"{label}: differs from the SciPy-LU engine by {worst:.3e}"
    assert info["grad_inf"] < 1e-5 * max(1.0, info["cost_final"])
    assert info["cost_final"] <= info["cost_initial"]
    if fg.dimension == 3:
        R = arrays_of(fg, got)[0][:, :3, :3]
        assert np.max(np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3))) < 1e-12


def test_group_agrees_with_the_single_handle_and_the_reference(hip_lib):
    print(check_fixture())
    fgs, starts = group(KEYS_2D)
    out = refine_estimate_batch(fgs, starts, lib_path=hip_lib)
    assert [info["group"] for _, info in out] == [0] * len(KEYS_2D)
    for k, fg, (res, info) in zip(KEYS_2D, fgs, out):
        single, sinfo = native_alone(k, hip_lib)
        _check_member(k, fg, res, info, single, sinfo, twin_alone(k)[0])
        assert info["engine"] == "native" and info["linear_solves"] >= info["iterations"] - 1


def test_member_started_at_its_own_optimum(hip_lib):
    """E goes in where the single handle left it, between B and D at their rough starts: it comes back as it went in, bit for
    bit, after as many iterations as the single handle reports from that point; B and D do not notice.

    "Its own optimum" is meant by the loop's own test, |g|_inf <= tol max(1, f): tol is twice what the single handle's run
    reports there (2 |g|_inf / max(1, f) = 2.2e-8 for E), so the loop stops before its first solve.  At the default
    tol = 1e-10 the point is no optimum to the loop: the single handle itself takes one more step from it (cost
    51.45891242849835 -> 51.45891242849831, the point moves by 1.7e-7) and so, by the same decisions, does the batch -- both
    figures measured on an MI355X and printed below; that run is held to the single handle's."""
    fg_e = member("E")[0]
    optimum, oinfo = native_alone("E", hip_lib)
    tol = 2.0 * oinfo["grad_inf"] / max(1.0, oinfo["cost_final"])
    # at the default tolerance: what the single handle does from that point, the batch does
    again, ainfo = refine_estimate(fg_e, optimum, engine="native", lib_path=hip_lib)
    fgs, starts = group(("B", "E", "D"))
    out = refine_estimate_batch(fgs, [starts[0], optimum, starts[2]], lib_path=hip_lib)
    print("E from its optimum at tol 1e-10: batch iterations", out[1][1]["iterations"], "solves", out[1][1]["linear_solves"],
          "| single handle iterations", ainfo["iterations"], "solves", ainfo["linear_solves"], "| cost", out[1][1]["cost_initial"], "->",
          out[1][1]["cost_final"], "| moved by",
          max(float(np.max(np.abs(a - b))) for a, b in zip(arrays_of(fg_e, out[1][0]), arrays_of(fg_e, optimum))))
    assert out[1][1]["iterations"] == ainfo["iterations"]
    assert _close(fg_e, out[1][0], again, ATOL[2])[1]
    # at the tolerance the point satisfies, in the library's own form of a point (theta, x, y: a SolverResults holds
    # cos / sin, and theta -> (cos, sin) -> atan2 is not the identity in the last bit)
    again, ainfo = refine_estimate(fg_e, optimum, engine="native", lib_path=hip_lib, tol=tol)
    assert ainfo["linear_solves"] == 0
    probs, points = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, [starts[0], optimum, starts[2]])])
    with RefineBatchHandle(probs, hip_lib) as h:
        pts, infos = h.run(list(points), tol=tol)
    print("E at its optimum: batch iterations", infos[1]["iterations"], "solves", infos[1]["linear_solves"], "| single handle iterations",
          ainfo["iterations"], "solves", ainfo["linear_solves"], "| cost", infos[1]["cost_initial"], "->", infos[1]["cost_final"],
          "| moved by", float(np.max(np.abs(pts[1] - points[1]))))
    assert np.array_equal(pts[1], points[1])
    assert infos[1]["iterations"] == ainfo["iterations"] and infos[1]["linear_solves"] == 0
    assert infos[1]["cost_final"] == infos[1]["cost_initial"]
    for i, k in ((0, "B"), (2, "D")):  # (against runs at the same tolerance)
        single, sinfo = refine_estimate(fgs[i], starts[i], engine="native", lib_path=hip_lib, tol=tol)
        lu, _ = refine_estimate(fgs[i], starts[i], engine="python", linear_solver="scipy", tol=tol)
        _check_member(k, fgs[i], _as_results(probs[i], pts[i], starts[i], infos[i]["cost_final"]), infos[i], single, sinfo, lu)


def test_group_of_one(hip_lib):
    fg, start = member("A")
    (res, info), = refine_estimate_batch([fg], [start], lib_path=hip_lib)
    _check_member("A alone", fg, res, info, *native_alone("A", hip_lib), twin_alone("A")[0])


def test_3d_group(hip_lib):
    keys = ("3D0", "3D1")
    fgs, starts = group(keys)
    out = refine_estimate_batch(fgs, starts, lib_path=hip_lib)
    for k, fg, (res, info) in zip(keys, fgs, out):
        _check_member(k, fg, res, info, *native_alone(k, hip_lib), twin_alone(k)[0])


def test_member_without_ranges_and_landmarks(hip_lib):
    """A pure pose graph beside a member with landmarks, and as a group of its own (no landmark arrays at all)."""
    fg = make_manhattan(seed=23, n_robots=1, n_poses=30, n_beacons=0, n_loop_closures=2)
    assert not fg.landmark_variables and not fg.range_measurements
    start = noisy_truth(fg, 23, *MILD)
    single, sinfo = refine_estimate(fg, start, engine="native", lib_path=hip_lib)
    lu, _ = refine_estimate(fg, start, engine="python", linear_solver="scipy")
    fg_c, start_c = member("C")
    out = refine_estimate_batch([fg_c, fg, fg_c], [start_c, start, start_c], lib_path=hip_lib)
    _check_member("pose graph", fg, out[1][0], out[1][1], single, sinfo, lu)
    for i in (0, 2):
        _check_member("C", fg_c, out[i][0], out[i][1], *native_alone("C", hip_lib), twin_alone("C")[0])
    (res, info), = refine_estimate_batch([fg], [start], lib_path=hip_lib)
    _check_member("pose graph alone", fg, res, info, single, sinfo, lu)


def test_member_with_an_undetermined_landmark(hip_lib):
    """One pose and one beacon: J'J is singular, and only lambda > 0 lets the conjugate-gradient solve through.  The single
    handle solves it; the batch reports what the single handle reports."""
    fg = undetermined_graph()
    start = noisy_truth(fg, 3, *MILD)
    single, sinfo = refine_estimate(fg, start, engine="native", lib_path=hip_lib)
    fg_c, start_c = member("C")
    out = refine_estimate_batch([fg, fg_c], [start, start_c], lib_path=hip_lib)
    res, info = out[0]
    print("undetermined: batch", {k: info[k] for k in ("iterations", "linear_solves", "pcg_iters", "cost_final", "grad_inf")},
          "| single", {k: sinfo[k] for k in ("iterations", "linear_solves", "pcg_iters", "cost_final", "grad_inf")})
    worst, ok = _close(fg, res, single, ATOL[2])
    print("undetermined: worst difference to the single handle", worst)
    assert ok
    assert info["iterations"] == sinfo["iterations"] and info["linear_solves"] == sinfo["linear_solves"]
    assert abs(info["cost_final"] - sinfo["cost_final"]) <= 1e-12 * max(1.0, sinfo["cost_initial"])
    _check_member("C", fg_c, out[1][0], out[1][1], *native_alone("C", hip_lib), twin_alone("C")[0])


def test_handle_reuse(hip_lib):
    """A second run on the same handle from other start points equals a fresh handle's, bit for bit."""
    keys = ("B", "C", "E")
    fgs, starts = group(keys)
    probs, first = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, starts)])
    second = [_problem_of(fg, rough_start(k), None, None)[1] for k, fg in zip(keys, fgs)]
    with RefineBatchHandle(probs, hip_lib) as h:
        h.run(list(first))
        pts, infos = h.run(second)
    with RefineBatchHandle(probs, hip_lib) as h:
        fresh, finfos = h.run(second)
    for k, a, b, ia, ib in zip(keys, pts, fresh, infos, finfos):
        print(k, "second run iterations", ia["iterations"], "solves", ia["linear_solves"], "pcg", ia["pcg_iters"])
        assert np.array_equal(a, b)
        for f in ("iterations", "linear_solves", "pcg_iters", "cost_initial", "cost_final", "grad_inf"):
            assert ia[f] == ib[f]


def test_errors_are_reported_not_faults(hip_lib):
    from score_amd.native import ScoreGraph, score_graph_struct
    from score_amd.solver import load_library

    lib = _bind(load_library(hip_lib))
    p2 = _problem_of(*member("C"), None, None)[0]
    p3 = _problem_of(*member("3D0"), None, None)[0]
    h = C.c_void_p()
    mixed = (ScoreGraph * 2)(score_graph_struct(p2.a), score_graph_struct(p3.a))
    assert lib.score_refine_batch_create(mixed, 2, None, C.byref(h)) != 0 and not h
    assert b"dim" in lib.score_last_error()
    one = (ScoreGraph * 1)(score_graph_struct(p2.a))
    assert lib.score_refine_batch_create(None, 1, None, C.byref(h)) != 0 and not h
    assert lib.score_refine_batch_create(one, 1, None, None) != 0
    assert lib.score_refine_batch_create(one, 0, None, C.byref(h)) != 0 and not h
    assert lib.score_refine_batch_run(None, None, None, 50, 1e-10, None, None, None) != 0
    assert lib.score_refine_batch_create(one, 1, None, C.byref(h)) == 0 and h
    try:
        poses = np.zeros(3 * p2.Np)
        assert lib.score_refine_batch_run(h, None, None, 50, 1e-10, None, None, None) != 0
        assert lib.score_refine_batch_run(h, poses.ctypes.data_as(C.POINTER(C.c_double)), None, 50, 1e-10,
                                          poses.ctypes.data_as(C.POINTER(C.c_double)), None, None) != 0  # the member has landmarks
    finally:
        lib.score_refine_batch_destroy(h)
    lib.score_refine_batch_destroy(None)
    with pytest.raises(RuntimeError, match="share dim"):
        RefineBatchHandle([p2, p3], hip_lib)


# ---------------------------------------------------------------------------------------------------------------------
# One lane function per job: what a lane does with a measurement is the same code in the single handle's kernels and in the
# group's (csrc/score_gn.hpp: gn_measurement, gn_robust_residual; csrc/score_gn_robust.hpp: gn_robust_weight), and a member's
# measurements lie over workgroups as a handle on it alone lays them.  So a group of one IS the single handle, value for
# value: equalities between two paths of the product, no tolerance.
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_workgroup_graph(dim):
    """Two chains of 60 poses whose measurements, and whose ranges + loop closures, fill more than one workgroup of 256 and at
    most two; range 0 and loop closure 1 re-attached to pose 0 (the pinned pose, which also has its odometry neighbour); one
    landmark prior."""
    make = make_manhattan if dim == 2 else make_manhattan_3d
    fg = make(seed=7, n_robots=2, n_poses=60, n_beacons=4, p_range=0.6, n_loop_closures=4)
    first = fg.pose_variables[0][0].name
    m = fg.range_measurements[0]
    m.association = (first, m.association[1])
    fg.loop_closure_measurements[1].base_pose = first
    lm = fg.landmark_variables[1]
    prior = compat.LandmarkPrior2D if dim == 2 else compat.LandmarkPrior3D
    fg.landmark_priors = [prior(lm.name, tuple(float(v) + 0.25 for v in lm.true_position), 2.0)]
    start = start_of(fg)
    a = point_of(fg, start)[0].a
    n_rel, n_rng, n_lc, n_pri = len(a["rel_base"]), len(a["rng_a"]), n_loop_closures_of(a), len(a["lprior_lm"])
    assert len(fg.pose_variables) == 2 and n_pri == 1 and n_lc == 4
    assert 256 < n_rel + n_rng + n_pri <= 512 and 256 < n_rng + n_lc <= 512, (n_rel, n_rng, n_lc, n_pri)
    assert a["rng_a"][0] == 0 and a["rel_base"][n_rel - n_lc + 1] == 0 and a["rel_base"][0] == 0 and a["rel_to"][0] == 1
    return fg, start


@pytest.mark.parametrize("dim", [2, 3])
def test_group_of_one_residuals_and_weights_are_the_single_handle_s(dim, hip_lib):
    fg, start = _two_workgroup_graph(dim)
    prob, point = point_of(fg, start)
    mu, c, c_rel = 0.7, 3.0, 2.5
    with RobustRefineHandle(prob, hip_lib) as h:
        single = h.residuals(point, mu, c, c_rel)
    with RefineBatchHandle([prob], hip_lib) as h:
        (alone,) = h.residuals([point], mu, c, c_rel)
    for name, a, b in zip(("residuals", "loop-closure residuals", "weights", "loop-closure weights"), single, alone):
        assert a.shape == b.shape and a.size > 0, name
        np.testing.assert_array_equal(a, b, err_msg=name)
    w, wl = single[2], single[3]
    assert np.any(w == 1.0) and np.any(w < 1.0) and np.all((wl >= 0.0) & (wl <= 1.0))  # (the weight rule was at work)


@pytest.mark.parametrize("dim", [2, 3])
def test_group_of_one_starts_at_the_single_handle_s_cost(dim, hip_lib):
    fg, start = _two_workgroup_graph(dim)
    _, sinfo = refine_estimate(fg, start, max_iters=2, engine="native", lib_path=hip_lib)
    ((_, info),) = refine_estimate_batch([fg], [start], max_iters=2, lib_path=hip_lib)
    assert isinstance(info["cost_initial"], float) and info["cost_initial"] == sinfo["cost_initial"] > 0.0
