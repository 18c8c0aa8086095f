"""GNC-TLS re-weighting on the MI355X: the device loop (score_robust_solve, csrc/score_robust.hpp) against its readable twin
(engine="python"), against solve_score, and in lock-step batches."""
import numpy as np
import pytest

from conftest import graph_by_name
from robust_helpers import _bit_equal, _poses_close
from score_amd.manhattan import make_manhattan
from score_amd.native import ArrayGraph, graph_arrays
from score_amd.robust import corrupt_ranges, solve_score_robust, solve_score_robust_batch
from score_amd.solve_score import solve_score

pytestmark = pytest.mark.gpu

CORRUPT = dict(n_robots=2, n_poses=60, n_beacons=3, p_range=0.5, sigma_range=0.1)


@pytest.mark.parametrize("seed", [2, 4])
def test_device_engine_matches_python_engine(seed, hip_lib):
    fg = make_manhattan(seed=seed, **CORRUPT)
    bad_g, _ = corrupt_ranges(fg, 0.08, seed=seed)
    dev = solve_score_robust(bad_g, "SOCP", engine="device")
    py = solve_score_robust(bad_g, "SOCP", engine="python")
    a, b = dev.info["robust"], py.info["robust"]
    assert a["outer_iterations"] == b["outer_iterations"] and a["converged"] == b["converged"]
    np.testing.assert_array_equal(a["outliers"], b["outliers"])
    np.testing.assert_allclose(a["weights"], b["weights"], rtol=0, atol=1e-9)
    assert a["mu"] == pytest.approx(b["mu"], rel=1e-9)
    _poses_close(dev, py, 1e-7)
    # the last outer solve is solve_score on the graph re-weighted with the returned weights, bit for bit
    arr = {k: v for k, v in graph_arrays_of(bad_g).items() if k != "_cstruct"}
    arr["rng_prec"] = arr["rng_prec"] * np.maximum(a["weights"], 1e-6)
    ref = solve_score(ArrayGraph(arr), "SOCP")
    _bit_equal(dev, ref)
    assert dev.info["pobj"] == ref.info["pobj"]


def graph_arrays_of(g):
    return g.arrays if isinstance(g, ArrayGraph) else graph_arrays(g)


@pytest.mark.parametrize("name", ["manhattan", "goats", "graph3d"])
@pytest.mark.parametrize("relax", ["QCQP", "SOCP"])
def test_clean_fixtures_take_one_plain_solve(name, relax, fixtures, hip_lib):
    fg = graph_by_name(name, fixtures)
    rob = solve_score_robust(fg, relax)
    ref = solve_score(fg, relax)
    info = rob.info["robust"]
    assert info["outer_iterations"] == 1 and info["converged"] and len(info["outliers"]) == 0
    np.testing.assert_array_equal(info["weights"], np.ones(len(fg.range_measurements)))
    _bit_equal(rob, ref)
    for k in ref.distances:
        np.testing.assert_array_equal(rob.distances[k], ref.distances[k])
    assert rob.info["pobj"] == ref.info["pobj"] and rob.info["iters"] == ref.info["iters"]


def test_lockstep_batch_members_stop_on_their_own(hip_lib):
    graphs = []
    for s in range(16):
        fg = make_manhattan(n_robots=4, n_poses=80, n_beacons=4, seed=500 + s, p_range=0.3, sigma_range=0.1)
        graphs.append(corrupt_ranges(fg, 0.05 if s % 2 else 0.0, seed=s)[0])
    batch = solve_score_robust_batch(graphs, "SOCP", group_size=16)
    counts = [r.info["robust"]["outer_iterations"] for r in batch]
    assert len(set(counts)) > 1, counts
    for g, b in zip(graphs, batch):
        one = solve_score_robust(g, "SOCP")
        assert b.info["robust"]["outer_iterations"] == one.info["robust"]["outer_iterations"]
        np.testing.assert_array_equal(b.info["robust"]["outliers"], one.info["robust"]["outliers"])
        _poses_close(b, one, 1e-7)


def test_both_families_without_loop_closures_is_the_range_family(hip_lib):
    # a graph without loop closures: the second family has no item, launches nothing, and its zeroed control records do not
    # lower the graph's mu -- every decision and every bit is the range family's
    g, _ = corrupt_ranges(make_manhattan(seed=2, **CORRUPT), 0.08, seed=2)
    both = solve_score_robust(g, "SOCP", robust_loop_closures=True)
    rng = solve_score_robust(g, "SOCP")
    a, b = both.info["robust"], rng.info["robust"]
    print(a["outer_iterations"], a["mu"], a["outliers"])
    assert a["outer_iterations"] == b["outer_iterations"] and a["converged"] == b["converged"]
    np.testing.assert_array_equal(a["outliers"], b["outliers"])
    np.testing.assert_array_equal(a["weights"], b["weights"])
    np.testing.assert_array_equal(a["residuals"], b["residuals"])
    assert a["mu"] == b["mu"]
    _bit_equal(both, rng)
    assert len(a["loop_closure_weights"]) == 0 and len(a["loop_closure_outliers"]) == 0
    assert a["outer_iterations"] > 1
