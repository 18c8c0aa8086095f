"""What the seven batch front ends share (score_amd/groups.py): the grouping rule, the per-graph broadcaster, the shared argument
errors with their full texts, the placement of the results, and the follow-up analyses of ``refine_estimate_batch``.  Everything
here runs ``engine="python"`` on the small graphs of tests/refine_batch_helpers.py: no library and no device."""
import types

import numpy as np
import pytest

from refine_batch_helpers import group, member
from score_amd import compat
from score_amd.leverage_batch import predicted_range_variances_batch, range_leverage_batch
from score_amd.marginals import _select
from score_amd.marginals_batch import group_marginals, marginal_covariances_batch
from score_amd.refine_batch import _problem_of, _python_lock_step, refine_estimate_batch
from score_amd.refine_robust_batch import refine_estimate_robust_batch
from score_amd.samples_batch import group_samples, posterior_samples_batch
from score_amd.spectrum_batch import information_spectrum_batch

MIXED = ("3D0", "C", "B", "3D1", "E")  # dimensions 3, 2, 2, 3, 2
MIXED_GROUPS = [2, 0, 0, 2, 1]         # max_group = 2: chunks (C, B), (E), (3D0, 3D1), numbered 0, 1, 2


def _variances(fgs, starts, **kw):
    return predicted_range_variances_batch(fgs, starts, [[] for _ in fgs], **kw)


# name -> (the call with engine="python", the keyword that asks for little work)
FRONT_ENDS = {
    "refine_estimate_batch": (refine_estimate_batch, {}),
    "refine_estimate_robust_batch": (refine_estimate_robust_batch, {}),
    "marginal_covariances_batch": (marginal_covariances_batch, {}),
    "information_spectrum_batch": (information_spectrum_batch, dict(k=2)),
    "posterior_samples_batch": (posterior_samples_batch, dict(n_samples=2)),
    "range_leverage_batch": (range_leverage_batch, dict(n_samples=2)),
    "predicted_range_variances_batch": (_variances, {}),
}


def _call(name, fgs, starts, **kw):
    fn, little = FRONT_ENDS[name]
    return fn(fgs, starts, engine="python", **{**little, **kw})


# ---------------------------------------------------------------------------------------------------------------------
# the rule on its own
# ---------------------------------------------------------------------------------------------------------------------
def _rule(dims, max_group, answered=()):
    from score_amd.groups import chunks, grouped

    datas = [types.SimpleNamespace(dimension=d) for d in dims]
    groups = grouped(datas, list(range(len(dims))), lambda i, data, res: None if i in answered else (f"prob{i}", f"point{res}", i * i))
    return [(number, [m[0] for m in chunk]) for number, chunk in chunks(groups, max_group)], groups


def test_grouping_rule():
    got, groups = _rule([3, 2, 2, 3, 2], 2)
    assert got == [(0, [1, 2]), (1, [4]), (2, [0, 3])]
    assert groups[3] == [(0, "prob0", "point0", 0), (3, "prob3", "point3", 9)]  # (graph number, what the callback returned)
    assert _rule([3, 2, 2, 3, 2], 1)[0] == [(0, [1]), (1, [2]), (2, [4]), (3, [0]), (4, [3])]
    assert _rule([3, 2, 2, 3, 2], 64)[0] == [(0, [1, 2, 4]), (1, [0, 3])]
    assert _rule([], 2)[0] == []
    # a graph the callback answers itself is in no chunk and takes no number
    assert _rule([3, 2, 2, 3, 2], 2, answered=(1, 2, 4))[0] == [(0, [0, 3])]
    assert _rule([3, 2, 2, 3, 2], 2, answered=(2,))[0] == [(0, [1, 4]), (1, [0, 3])]


def test_grouping_pass_names_the_graph():
    from score_amd.groups import grouped

    datas = [types.SimpleNamespace(dimension=d) for d in (2, 4)]
    with pytest.raises(ValueError) as e:
        grouped(datas, [None, None], lambda i, data, res: ((), ()))
    assert str(e.value) == "graph 1: dimension must be 2 or 3"

    def member_of(i, data, res):
        if i == 1:
            raise ValueError("marginal_covariances: unknown variable 'X'")
        return (), ()

    datas = [types.SimpleNamespace(dimension=2) for _ in range(2)]
    with pytest.raises(ValueError) as e:
        grouped(datas, [None, None], member_of)
    assert str(e.value) == "graph 1: marginal_covariances: unknown variable 'X'"
    with pytest.raises(ValueError) as e:
        grouped(datas, [None, None], member_of, who="posterior_samples")
    assert str(e.value) == "graph 1: posterior_samples: unknown variable 'X'"
    with pytest.raises(ValueError) as e:  # (the two refine functions: the callback's errors as they are)
        grouped(datas, [None, None], member_of, named=False)
    assert str(e.value) == "marginal_covariances: unknown variable 'X'"


def test_runner_places_results_and_opens_a_handle_per_device_chunk():
    from score_amd.groups import grouped, run_chunks

    opened = []

    class Handle:
        def __init__(self, probs, lib_path, solver_settings):
            opened.append(("create", list(probs), lib_path, solver_settings))

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            opened.append(("destroy",))

    datas = [types.SimpleNamespace(dimension=d) for d in (3, 2, 2, 3, 2)]
    groups = grouped(datas, "abcde", lambda i, data, res: (f"prob{i}", res, 10 * i))
    seen = []

    def body(handle, number, idx, probs, points, extras):
        seen.append((handle is not None, number, idx, probs, points, extras))
        return [f"{number}:{i}" for i in idx]

    out = [None] * 5
    run_chunks(groups, 2, out, body, False)
    assert out == ["2:0", "0:1", "0:2", "2:3", "1:4"] and opened == []
    assert seen[0] == (False, 0, [1, 2], ["prob1", "prob2"], ["b", "c"], [[10, 20]])
    out = [None] * 5
    run_chunks(groups, 2, out, body, True, "lib", {"a": 1}, handle=Handle)
    assert out == ["2:0", "0:1", "0:2", "2:3", "1:4"] and all(s[0] for s in seen[3:])
    assert opened == [("create", ["prob1", "prob2"], "lib", {"a": 1}), ("destroy",), ("create", ["prob4"], "lib", {"a": 1}), ("destroy",),
                      ("create", ["prob0", "prob3"], "lib", {"a": 1}), ("destroy",)]


def test_broadcaster():
    from score_amd.groups import per_graph

    assert per_graph(None, 3, "pairs") == [None, None, None]
    assert per_graph(["a", None, "c"], 3, "pairs") == ["a", None, "c"] and per_graph(iter("ab"), 2, "pairs") == ["a", "b"]
    assert per_graph(2.5, 2, "inlier_threshold", scalar=True) == [2.5, 2.5] and per_graph(None, 2, "x", scalar=True) == [None, None]
    assert per_graph(np.float64(3), 2, "n_samples", none=False, scalar=True) == [3.0, 3.0]
    with pytest.raises(ValueError) as e:
        per_graph([1, 2, 3], 2, "range_weights")
    assert str(e.value) == "range_weights: one entry per graph expected (2), got 3"
    with pytest.raises(ValueError) as e:
        per_graph([1], 2, "n_samples", none=False, scalar=True)
    assert str(e.value) == "n_samples: one entry per graph expected (2), got 1"
    with pytest.raises(ValueError) as e:
        per_graph([1.0, 2.0, 3.0], 2, "inlier_threshold", scalar=True)
    assert str(e.value) == "inlier_threshold: a scalar or one entry per graph expected (2), got 3"
    with pytest.raises(TypeError):  # a scalar only where asked for
        per_graph(2.5, 2, "range_weights")
    with pytest.raises(TypeError):  # and None
        per_graph(None, 2, "pairs", none=False)


def test_pairing_check():
    from score_amd.groups import paired

    assert paired(iter("ab"), iter("cd"), 1) == (["a", "b"], ["c", "d"])
    with pytest.raises(ValueError) as e:
        paired("ab", "c", 0)  # (the lengths first)
    assert str(e.value) == "one estimate per graph expected: 2 graphs, 1 estimates"
    with pytest.raises(ValueError) as e:
        paired("ab", "cd", 0)
    assert str(e.value) == "max_group must be at least 1"
    assert paired("ab", "cd") == (["a", "b"], ["c", "d"])


# ---------------------------------------------------------------------------------------------------------------------
# the errors every front end shares, with their texts
# ---------------------------------------------------------------------------------------------------------------------
SHARED_ERRORS = {
    "lengths": (lambda fgs, starts: (fgs, starts[:1], {}), "one estimate per graph expected: 2 graphs, 1 estimates"),
    "max_group": (lambda fgs, starts: (fgs, starts, dict(max_group=0)), "max_group must be at least 1"),
    "dimension": (lambda fgs, starts: ([fgs[0], types.SimpleNamespace(dimension=4)], starts, {}), "graph 1: dimension must be 2 or 3"),
    "range_weights": (lambda fgs, starts: (fgs, starts, dict(range_weights=[None])), "range_weights: one entry per graph expected (2), got 1"),
}
# (front end, error) pairs that front end does not raise today: none -- all seven check all four
NOT_RAISED = set()


@pytest.mark.parametrize("what", sorted(SHARED_ERRORS))
@pytest.mark.parametrize("name", sorted(FRONT_ENDS))
def test_shared_argument_errors(name, what):
    assert (name, what) not in NOT_RAISED
    fgs, starts = group(("C", "B"))
    arrange, text = SHARED_ERRORS[what]
    fgs, starts, kw = arrange(fgs, starts)
    with pytest.raises(ValueError) as e:
        _call(name, fgs, starts, **kw)
    assert str(e.value) == text


@pytest.mark.parametrize("name", sorted(FRONT_ENDS))
def test_no_graphs_no_results(name):
    assert _call(name, [], []) == []


# ---------------------------------------------------------------------------------------------------------------------
# the front ends on the mixed list
# ---------------------------------------------------------------------------------------------------------------------
def _figures(name, fg, result):
    """The arrays of one graph's result that the comparison reads."""
    got, info = result
    if name.startswith("refine"):
        return [np.asarray(got.poses[p.name]) for ch in fg.pose_variables for p in ch] + [np.asarray(info["cost_final"])]
    if name == "marginal_covariances_batch":
        return [got[nm] for nm in sorted(got)]
    if name == "information_spectrum_batch":
        return [got.values, got.vectors]
    if name == "posterior_samples_batch":
        return [got.steps[nm] for nm in got.order]
    if name == "range_leverage_batch":
        return [got.leverage, got.redundancy]
    return [got.variance, got.distance]


@pytest.mark.parametrize("name", sorted(FRONT_ENDS))
def test_front_end_on_the_mixed_list(name):
    """Dimensions 3, 2, 2, 3, 2 in groups of at most two: graph i's result stands at place i -- it is what the call gives on
    that graph alone (stream seed + i) -- and ``info["group"]`` is the chunk's number."""
    fgs, starts = group(MIXED)
    kw = {}
    if name == "predicted_range_variances_batch":
        kw["pairs"] = [[(fg.pose_variables[0][1].name, fg.pose_variables[0][4].name)] for fg in fgs]
        fn = lambda f, s, **k: predicted_range_variances_batch(f, s, k.pop("pairs"), engine="python", **k)  # noqa: E731
    else:
        fn = lambda f, s, **k: _call(name, f, s, **k)  # noqa: E731
    seeded = name in ("posterior_samples_batch", "range_leverage_batch")
    out = fn(fgs, starts, max_group=2, **kw, **(dict(seed=30) if seeded else {}))
    assert len(out) == len(MIXED)
    if name in ("range_leverage_batch", "predicted_range_variances_batch"):  # graph by graph under engine="python": no groups
        assert all("group" not in info and "passes" not in info for _, info in out)
    else:
        assert [info["group"] for _, info in out] == MIXED_GROUPS
    for i, (fg, start) in enumerate(zip(fgs, starts)):
        own = {k: [v[i]] for k, v in kw.items()}
        alone = fn([fg], [start], **own, **(dict(seed=30 + i) if seeded else {}))[0]
        for a, b in zip(_figures(name, fg, out[i]), _figures(name, fg, alone)):
            np.testing.assert_array_equal(a, b, err_msg=f"{name}, graph {i}")
        if "group" in alone[1]:
            assert alone[1]["group"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the follow-up analyses of refine_estimate_batch
# ---------------------------------------------------------------------------------------------------------------------
def _lone():
    """A graph of one fixed pose: no unknowns."""
    lone = compat.FactorGraphData(dimension=2)
    lone.pose_variables = [[compat.PoseVariable2D("A0", (0.5, -0.25), 0.3)]]
    lone.odom_measurements = [[]]
    T = np.eye(3)
    T[:2, 2] = (0.5, -0.25)
    vals = compat.VariableValues(2, compat.ArrayDict(["A0"], T[None]), compat.ArrayDict([], np.zeros((0, 2))), None)
    return lone, compat.SolverResults(variables=vals, total_time=0.0, solved=True, pose_chain_names=[["A0"]], solver_cost=0.0, info={})


def test_refine_estimate_batch_with_all_three_follow_ups():
    """marginals, samples and leverage in one call: a graph without unknowns gets None for all three, graph i of the others what
    the stand-alone batch calls give at the refined estimates from the streams of seed + i."""
    lone, lone_start = _lone()
    (c, b), (c_start, b_start) = group(("C", "B"))
    fgs, starts = [c, lone, b], [c_start, lone_start, b_start]
    out = refine_estimate_batch(fgs, starts, engine="python", marginals=True, samples=4, samples_seed=20, leverage=4, leverage_seed=50)
    plain = refine_estimate_batch(fgs, starts, engine="python")
    assert [info["group"] for _, info in out if "group" in info] == [0, 0] and "group" not in out[1][1]
    assert out[1][1]["marginals"] is None and out[1][1]["samples"] is None and out[1][1]["leverage"] is None
    for (res, info), (res_p, info_p) in zip(out, plain):
        assert not {"marginals", "samples", "leverage"} & set(info_p) and info["cost_final"] == info_p["cost_final"]
        for nm in res_p.poses:
            np.testing.assert_array_equal(res.poses[nm], res_p.poses[nm])
    kept = [0, 2]
    refined = [out[i][0] for i in kept]
    graphs = [fgs[i] for i in kept]
    levs = range_leverage_batch(graphs, refined, n_samples=4, seed=[50 + i for i in kept], engine="python")
    # Marginals and draws are formed at the refined POINTS.  A stand-alone call reads the point back from the estimate's
    # rotation matrices (angle -> matrix -> angle), which moves an angle by an ulp or two, so its figures agree to rounding
    # only: compared bit for bit are the group calls the stand-alone front ends make, at the points themselves; the
    # stand-alone front ends then have to agree to 1e-9 relative -- some 1e-16 in the point times the condition of J'J
    # (below 1e6 on these graphs), and far below the O(1) difference another graph or another stream would show.
    probs, first = zip(*[_problem_of(fgs[i], starts[i], None, None) for i in kept])
    pts, _, _ = _python_lock_step(list(probs), list(first), 50, 1e-10)
    sels = [_select(p, None) for p in probs]
    covs = group_marginals(None, probs, pts, sels, kept, 0, engine="python")
    draws = group_samples(None, probs, pts, refined, sels, kept, 0, [4, 4], [20 + i for i in kept], engine="python")
    covs_alone = marginal_covariances_batch(graphs, refined, engine="python")
    draws_alone = posterior_samples_batch(graphs, refined, n_samples=4, seed=[20 + i for i in kept], engine="python")
    for k, i in enumerate(kept):
        info = out[i][1]
        cov, cov_info = info["marginals"]
        assert sorted(cov) == sorted(covs[k][0]) == sorted(covs_alone[k][0]) and cov_info["engine"] == "python" and cov_info["group"] == 0
        for nm in cov:
            np.testing.assert_array_equal(cov[nm], covs[k][0][nm], err_msg=nm)
            np.testing.assert_allclose(cov[nm], covs_alone[k][0][nm], rtol=1e-9, atol=1e-9 * np.abs(cov[nm]).max(), err_msg=nm)
        smp, smp_info = info["samples"]
        assert smp.order == draws[k][0].order == draws_alone[k][0].order and smp.count == 4
        assert smp_info["group"] == 0 and smp_info["engine"] == "python"
        for nm in smp.order:
            np.testing.assert_array_equal(smp.steps[nm], draws[k][0].steps[nm], err_msg=nm)
            np.testing.assert_array_equal(smp.covariance(nm), draws[k][0].covariance(nm), err_msg=nm)
            np.testing.assert_allclose(smp.steps[nm], draws_alone[k][0].steps[nm], rtol=1e-9, atol=1e-9 * np.abs(smp.steps[nm]).max(), err_msg=nm)
        lev, lev_info = info["leverage"]
        assert lev.count == 4 and lev_info["engine"] == "python" and "group" not in lev_info
        np.testing.assert_array_equal(lev.leverage, levs[k][0].leverage)
        np.testing.assert_array_equal(lev.redundancy, levs[k][0].redundancy)
