"""GNC-TLS re-weighting of the loop closures on the MI355X: the device loop (score_robust_solve_rel, csrc/score_robust.hpp)
against its readable twin (engine="python"), against solve_score, against the oracle, through the host assembler, in lock-step
batches, and the old entry point against the new one."""
import ctypes as C

import numpy as np
import pytest

from conftest import graph_by_name
from robust_helpers import _bit_equal, _poses_close
from score_amd import compat
from score_amd.manhattan import make_manhattan, make_manhattan_3d
from score_amd.native import ArrayGraph, ScoreGraph, graph_arrays, score_graph_struct
from score_amd.robust import (ScoreRobustInfo, ScoreRobustSettings, _bind, corrupt_loop_closures, corrupt_ranges,
                              relaxed_loop_closure_residuals, relaxed_range_residuals, solve_score_robust, solve_score_robust_batch)
from score_amd.solve_score import solve_score
from score_amd.solver import ScoreInfo, ScoreSettings, _f64p, _i32p, load_library

pytestmark = pytest.mark.gpu

G2 = dict(n_robots=1, n_poses=80, n_beacons=3, p_range=0.5, sigma_range=0.1, n_loop_closures=10)
G3 = dict(n_robots=1, n_poses=40, n_beacons=3, p_range=0.5, sigma_range=0.1, n_loop_closures=6)
LC_ONLY = dict(robust_ranges=False, robust_loop_closures=True)
BOTH = dict(robust_loop_closures=True)


def _arrays(g):
    return {k: v for k, v in (g.arrays if isinstance(g, ArrayGraph) else graph_arrays(g)).items() if k != "_cstruct"}


def _g2_seed3():
    return corrupt_loop_closures(make_manhattan(seed=3, **G2), 2, seed=3)[0], LC_ONLY


def _g2_seed5_both():
    g1, _ = corrupt_loop_closures(make_manhattan(seed=5, **G2), 2, seed=5)
    return corrupt_ranges(g1, 0.05, seed=5)[0], BOTH


def _g3_seed2():
    return corrupt_loop_closures(make_manhattan_3d(seed=2, **G3), 1, seed=2)[0], LC_ONLY


def _graph3d():
    # 3-D, a landmark prior, and one loop closure that is inconsistent by construction (r = 5.49)
    return graph_by_name("graph3d", {}), BOTH


def _same_decisions(a, b):
    assert a["outer_iterations"] == b["outer_iterations"] and a["converged"] == b["converged"]
    np.testing.assert_array_equal(a["outliers"], b["outliers"])
    np.testing.assert_array_equal(a["loop_closure_outliers"], b["loop_closure_outliers"])


@pytest.mark.parametrize("case", [_g2_seed3, _g2_seed5_both, _g3_seed2, _graph3d])
def test_device_engine_matches_python_engine(case, hip_lib):
    g, kw = case()
    dev = solve_score_robust(g, "SOCP", engine="device", **kw)
    py = solve_score_robust(g, "SOCP", engine="python", **kw)
    a, b = dev.info["robust"], py.info["robust"]
    print(case.__name__, a["outer_iterations"], a["loop_closure_outliers"], a["outliers"], a["mu"])
    _same_decisions(a, b)
    assert a["outer_iterations"] > 1
    np.testing.assert_allclose(a["weights"], b["weights"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(a["loop_closure_weights"], b["loop_closure_weights"], rtol=0, atol=1e-9)
    assert a["mu"] == pytest.approx(b["mu"], rel=1e-9)
    _poses_close(dev, py, 1e-7)
    # the last outer solve is solve_score on the graph re-weighted with the returned weights, bit for bit
    arr = _arrays(g)
    n_lc = len(a["loop_closure_weights"])
    arr["rng_prec"] = arr["rng_prec"] * np.maximum(a["weights"], 1e-6)
    for key in ("rel_kappa", "rel_tau"):
        v = np.array(arr[key], dtype=np.float64)
        v[len(v) - n_lc:] *= np.maximum(a["loop_closure_weights"], 1e-6)
        arr[key] = v
    ref = solve_score(ArrayGraph(arr), "SOCP")
    _bit_equal(dev, ref)
    assert dev.info["pobj"] == ref.info["pobj"]


@pytest.mark.parametrize("case", [_g2_seed5_both, _g2_seed3])
def test_reported_residuals_are_those_of_the_returned_solution(case, hip_lib):
    g, kw = case()
    res = solve_score_robust(g, "SOCP", **kw)
    info = res.info["robust"]
    arrays = _arrays(g)
    for got, r in ((info["residuals"], relaxed_range_residuals(arrays, res.relaxed_poses.array, res.landmarks.array)),
                   (info["loop_closure_residuals"], relaxed_loop_closure_residuals(arrays, res.relaxed_poses.array))):
        assert got.shape == r.shape and len(r) > 0
        err = np.abs(got - r) / np.maximum(1.0, r)
        print(case.__name__, len(r), info["outer_iterations"], float(np.max(err)))
        assert float(np.max(err)) <= 1e-9, float(np.max(err))
    if kw is LC_ONLY:  # the ranges are measured, not re-weighted
        np.testing.assert_array_equal(info["weights"], np.ones(len(arrays["rng_a"])))


def _indexing_graph(n_lc, seed):
    """2 robots x 40 poses with n_lc loop closures and one more from the pinned pose A0 to B7 (their true relative pose)."""
    fg = make_manhattan(n_robots=2, n_poses=40, n_beacons=3, p_range=0.5, sigma_range=0.1, seed=seed, n_loop_closures=n_lc)
    Ti = fg.pose_variables[0][0].transformation_matrix
    Tj = fg.pose_variables[1][7].transformation_matrix
    rel = np.linalg.inv(Ti) @ Tj
    fg.loop_closure_measurements.append(compat.PoseMeasurement2D(
        "A0", "B7", float(rel[0, 2]), float(rel[1, 2]), float(np.arctan2(rel[1, 0], rel[0, 0])), 1e4, 2.5e5))
    return corrupt_loop_closures(fg, 3, seed=seed)[0]


def test_residual_kernel_indexing_across_problems(hip_lib):
    # 71 + 6 + 131 loop closures: one 256-thread block whose waves straddle the problems' boundaries (both branches of the
    # per-problem reduction); a loop closure from the pinned pose and into the second chain in every graph
    graphs = [_indexing_graph(n, 40 + i) for i, n in enumerate((70, 5, 130))]
    batch = solve_score_robust_batch(graphs, "SOCP", group_size=3, **LC_ONLY)
    for g, b in zip(graphs, batch):
        info = b.info["robust"]
        a = g.arrays
        assert a["rel_base"][-1] == 0 and a["rel_to"][-1] == 40 + 7
        r = relaxed_loop_closure_residuals(a, b.relaxed_poses.array)
        assert info["loop_closure_residuals"].shape == r.shape
        err = np.abs(info["loop_closure_residuals"] - r) / np.maximum(1.0, r)
        assert float(np.max(err)) <= 1e-9, float(np.max(err))
        one = solve_score_robust(g, "SOCP", **LC_ONLY)
        print(len(r), info["outer_iterations"], info["loop_closure_outliers"], float(np.max(err)))
        _same_decisions(info, one.info["robust"])
        _poses_close(b, one, 1e-7)


def test_last_solve_against_the_oracle(hip_lib):
    from oracle import score_oracle as so

    fg = make_manhattan(seed=5, **G2)
    g, bad = corrupt_loop_closures(fg, 2, seed=5)
    dev = solve_score_robust(g, "SOCP", **LC_ONLY)
    w = dev.info["robust"]["loop_closure_weights"]
    assert set(bad.tolist()) <= set(np.nonzero(w < 0.5)[0].tolist())
    # the object graph of the last solve: the corrupted measurements, precisions times max(w, 1e-6)
    a = g.arrays
    first = len(a["rel_base"]) - len(w)
    for k in range(len(w)):
        e = first + k
        f = max(float(w[k]), 1e-6)
        m = fg.loop_closure_measurements[k]
        R = np.asarray(a["rel_R"]).reshape(-1, 2, 2)[e]
        t = np.asarray(a["rel_t"]).reshape(-1, 2)[e]
        fg.loop_closure_measurements[k] = compat.PoseMeasurement2D(
            m.base_pose, m.to_pose, float(t[0]), float(t[1]), float(np.arctan2(R[1, 0], R[0, 0])),
            float(a["rel_kappa"][e]) * f, float(a["rel_tau"][e]) * f)
    rp, u, info = so.newton_solve(fg, tol=1e-13)
    ref = so.reduced_to_values(rp, u, "SOCP")
    scale = max(np.max(np.abs(v)) for v in ref["poses"].values())
    worst = max(float(np.max(np.abs(dev.poses[nm][:2, 2] - X[:, 2]))) / scale for nm, X in ref["poses"].items())
    print(dev.info["pobj"], info["objective"], worst)
    assert abs(dev.info["pobj"] - info["objective"]) < 1e-5 * max(1.0, abs(info["objective"]))
    assert worst < 1e-4, worst


def test_host_assembler_fallback_reads_the_weighted_precisions(hip_lib, monkeypatch):
    g, kw = _g2_seed3()
    dev = solve_score_robust(g, "SOCP", **kw)
    monkeypatch.setenv("SCORE_HOST_ASSEMBLE", "1")
    host = solve_score_robust(g, "SOCP", **kw)
    _same_decisions(host.info["robust"], dev.info["robust"])
    assert dev.info["robust"]["outer_iterations"] > 1
    _poses_close(host, dev, 1e-7)


def test_lockstep_batch_members_stop_on_their_own(hip_lib):
    graphs = []
    for s in range(16):
        fg = make_manhattan(seed=500 + s, **G2)
        graphs.append(corrupt_loop_closures(fg, 2 if s % 2 else 0, seed=s)[0])
    batch = solve_score_robust_batch(graphs, "SOCP", group_size=16, **LC_ONLY)
    counts = [r.info["robust"]["outer_iterations"] for r in batch]
    print(counts)
    assert len(set(counts)) > 1, counts
    for g, b in zip(graphs, batch):
        one = solve_score_robust(g, "SOCP", **LC_ONLY)
        _same_decisions(b.info["robust"], one.info["robust"])
        _poses_close(b, one, 1e-7)


def _call(lib, fn, arrays, families=None):
    """score_robust_solve (families None) or score_robust_solve_rel through ctypes on one graph."""
    st, rs = ScoreSettings(), ScoreRobustSettings()
    lib.score_default_settings(C.byref(st))
    lib.score_robust_default_settings(C.byref(rs))
    gs = (ScoreGraph * 1)()
    C.memmove(C.byref(gs[0]), C.byref(score_graph_struct(arrays, 0)), C.sizeof(ScoreGraph))
    d, Np, Nl, Nr = int(arrays["dim"]), len(arrays["pose_names"]), len(arrays["landmark_names"]), len(arrays["rng_a"])
    W, Rr = np.empty(Nr), np.empty(Nr)
    T, B, Lm, Rg = np.empty((Np, d + 1, d + 1)), np.empty((Np, d, d + 1)), np.empty((max(1, Nl), d)), np.empty((Nr, 1))
    F = np.empty(Np, dtype=np.int32)
    infos, rinfos = (ScoreInfo * 1)(), (ScoreRobustInfo * 1)()
    p = lambda x: x.ctypes.data_as(_f64p)  # noqa: E731
    head = (gs, 1, C.byref(st), C.byref(rs))
    tail = (p(T), p(B), p(Lm), p(Rg), F.ctypes.data_as(_i32p), infos, rinfos)
    if families is None:
        rc = fn(*head, p(W), p(Rr), *tail)
    else:
        rc = fn(*head, families, 0.0, p(W), p(Rr), None, None, *tail)
    assert rc == 0, lib.score_last_error().decode()
    return W, Rr, T, B, Lm, infos[0].as_dict(), rinfos[0]


def test_old_entry_point_is_the_new_one_with_the_range_family(hip_lib):
    fg = make_manhattan(n_robots=2, n_poses=60, n_beacons=3, p_range=0.5, sigma_range=0.1, seed=2, n_loop_closures=6)
    arrays = corrupt_ranges(fg, 0.08, seed=2)[0].arrays
    lib = _bind(load_library(None))
    old = _call(lib, lib.score_robust_solve, arrays)
    new = _call(lib, lib.score_robust_solve_rel, arrays, families=1)
    for x, y in zip(old[:5], new[:5]):
        np.testing.assert_array_equal(x, y)
    for key in old[5]:
        if key not in ("setup_ms", "solve_ms"):
            assert old[5][key] == new[5][key], key
    for key in ("outer_iterations", "converged", "outliers", "rel_outliers", "mu"):
        assert getattr(old[6], key) == getattr(new[6], key), key
    assert old[6].outer_iterations > 1 and old[6].outliers > 0 and old[6].rel_outliers == 0
    # families = 0 is an error
    st, rs = ScoreSettings(), ScoreRobustSettings()
    lib.score_default_settings(C.byref(st))
    lib.score_robust_default_settings(C.byref(rs))
    gs = (ScoreGraph * 1)()
    C.memmove(C.byref(gs[0]), C.byref(score_graph_struct(arrays, 0)), C.sizeof(ScoreGraph))
    assert lib.score_robust_solve_rel(gs, 1, C.byref(st), C.byref(rs), 0, 3.0, *([None] * 11)) < 0
    assert "families" in lib.score_last_error().decode()
