"""Batched range leverage and predicted range variances (score_amd/leverage_batch.py): what runs without a GPU -- the binding
table of include/score_leverage_batch.h, the python engine graph by graph, the identity sum h = n, the argument errors, and the
plan of csrc/score_leverage_batch_plan.hpp as a stand-alone program under the host sanitizers.  The device path is
tests/test_leverage_batch_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from refine_batch_helpers import member
from samples_batch_helpers import member_twin
from score_amd.bindings import LATER_TABLES, LEVERAGE_BATCH, TABLES, bind
from score_amd.leverage import predicted_range_variances, range_leverage
from score_amd.leverage_batch import LEVERAGE_BATCH_SYMBOLS, predicted_range_variances_batch, range_leverage_batch
from score_amd.refine_batch import RefineBatchHandle, refine_estimate_batch
from score_amd.samples_batch import _seeds_of
from test_binding_tables_host import SCALARS, _declarations, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY_SEED = 3  # graph i draws from the stream of IDENTITY_SEED + i


def test_table_matches_header():
    table = LEVERAGE_BATCH
    assert LATER_TABLES == (LEVERAGE_BATCH,) and table not in TABLES and table.name == "leverage_batch"
    assert LEVERAGE_BATCH in RefineBatchHandle.headers
    declared = _declarations(table.name)
    assert sorted(declared) == sorted(table) == sorted(LEVERAGE_BATCH_SYMBOLS)
    assert sorted(declared) == ["score_refine_batch_leverage", "score_refine_batch_range_variances"]
    lib = bind(_Stub(), table)
    assert bind(lib, table) is lib  # (bound once)
    for sym, params in declared.items():
        argtypes = getattr(lib, sym).argtypes
        assert argtypes == table[sym][0] and getattr(lib, sym).restype == table[sym][1]
        assert len(params) == len(argtypes), sym
        for param, typ in zip(params, argtypes):
            is_pointer = typ is C.c_void_p or hasattr(typ, "contents")
            assert ("*" in param) == is_pointer, (sym, param, typ)
            if not is_pointer:
                assert SCALARS[param.split()[-2]] is typ, (sym, param, typ)


def test_missing_symbol():
    sym = list(LEVERAGE_BATCH)[-1]
    with pytest.raises(RuntimeError) as e:
        bind(_Stub(lacks=sym), LEVERAGE_BATCH)
    assert str(e.value) == f"{sym} is missing from the library: rebuild it (the CPU twin has no leverages: engine='python' runs there)"


def _pose(fg, k):
    return fg.pose_variables[0][k].name


def test_python_engine_equals_the_single_calls_graph_by_graph():
    """Mixed dimensions, weights for one graph, a count and a pair list per graph: every graph comes back at its own place
    with exactly what range_leverage / predicted_range_variances(engine="python") give on it alone, seeds seed + i."""
    keys = ("B", "3D0", "C")
    fgs, starts = [member(k)[0] for k in keys], [member(k)[1] for k in keys]
    w = np.ones(len(fgs[0].range_measurements))
    w[[1, 5, 9]] = 0.0
    weights = [w, None, None]
    counts = [5, 3, 4]
    pairs = [[(_pose(fgs[0], 2), _pose(fgs[0], 5))], None, [(_pose(fgs[2], 0), fgs[2].landmark_variables[0].name), (_pose(fgs[2], 1), _pose(fgs[2], 3))]]
    assert _seeds_of(40, 3) == [40, 41, 42]
    out = range_leverage_batch(fgs, starts, n_samples=counts, seed=40, first_sample=2, pairs=pairs, range_weights=weights, engine="python",
                               max_group=2)
    for i, (fg, st, rw, S, nm, (lev, info)) in enumerate(zip(fgs, starts, weights, counts, pairs, out)):
        alone, info1 = range_leverage(fg, st, n_samples=S, seed=40 + i, first_sample=2, pairs=nm, range_weights=rw, engine="python")
        assert lev.count == alone.count == S and lev.pairs == alone.pairs and info["engine"] == "python"
        for f in ("leverage", "leverage_error", "redundancy", "redundancy_error", "residuals", "studentized"):
            np.testing.assert_array_equal(getattr(lev, f), getattr(alone, f), err_msg=f)
        if nm is not None:
            np.testing.assert_array_equal(lev.pair_variance, alone.pair_variance)
        np.testing.assert_array_equal(info["residuals"], info1["residuals"])
    again = range_leverage_batch(fgs[:2], starts[:2], n_samples=counts[:2], seed=[40, 41], first_sample=2, range_weights=weights[:2], engine="python")
    for (a, _), (b, _) in zip(again, out[:2]):
        np.testing.assert_array_equal(a.leverage, b.leverage)
    lists = [pairs[0], [], pairs[2]]
    got = predicted_range_variances_batch(fgs, starts, lists, range_weights=weights, engine="python")
    for fg, st, rw, nm, (pred, info) in zip(fgs, starts, weights, lists, got):
        if not nm:
            assert pred.pairs == [] and pred.variance.shape == (0,) and info["engine"] == "python"
            continue
        alone, _ = predicted_range_variances(fg, st, nm, range_weights=rw, engine="python")
        assert pred.pairs == alone.pairs
        np.testing.assert_array_equal(pred.variance, alone.variance)
        np.testing.assert_array_equal(pred.distance, alone.distance)


def test_total_leverage_is_the_number_of_unknowns():
    """sum_m h_m = n.  Per draw, sum_m t = |J delta|^2 = z'P z with P a projection of rank n: its mean is n and its variance
    2 n, so the mean over S draws has the standard error sqrt(2 n / S) -- the condition is three of those."""
    keys, S = ("B", "C"), 64
    tws = [member_twin(k) for k in keys]
    out = range_leverage_batch([t.fg for t in tws], [t.results for t in tws], n_samples=S, seed=IDENTITY_SEED, engine="python")
    for k, tw, (lev, _) in zip(keys, tws, out):
        n, err = tw.ref.n, np.sqrt(2.0 * tw.ref.n / S)
        print(f"{k}: total leverage {lev.total_leverage:.3f} for n = {n} (standard error {err:.3f}), total redundancy "
              f"{lev.total_redundancy:.3f} for rows - n = {lev.rows - n}")
        assert lev.unknowns == n and abs(lev.total_leverage - n) <= 3 * err
        assert abs(lev.total_redundancy - (lev.rows - n)) <= 3 * np.sqrt(2.0 * (lev.rows - n) / S)


def test_argument_errors_carry_the_graph_index():
    fgs, starts = [member(k)[0] for k in ("C", "B")], [member(k)[1] for k in ("C", "B")]
    kw = dict(engine="python", n_samples=2)
    some = _pose(fgs[1], 3)
    with pytest.raises(ValueError, match=r"graph 1: .*range_weights"):
        range_leverage_batch(fgs, starts, range_weights=[None, np.ones(len(fgs[1].range_measurements) + 1)], **kw)
    with pytest.raises(ValueError, match=r"graph 0: .*unknown variable"):
        range_leverage_batch(fgs, starts, pairs=[[("nobody", some)], None], **kw)
    with pytest.raises(ValueError, match=r"graph 1: .*joins a variable to itself"):
        predicted_range_variances_batch(fgs, starts, [[], [(some, some)]], engine="python")
    for what in ("range_weights", "loop_closure_weights", "pairs"):
        with pytest.raises(ValueError, match=rf"{what}: one entry per graph"):
            range_leverage_batch(fgs, starts, **{**kw, what: [None]})
    with pytest.raises(ValueError, match="pairs: one entry per graph"):
        predicted_range_variances_batch(fgs, starts, [[]], engine="python")
    with pytest.raises(ValueError, match="n_samples: one entry per graph"):
        range_leverage_batch(fgs, starts, engine="python", n_samples=[2, 2, 2])
    with pytest.raises(ValueError, match="seed: one entry per graph"):
        range_leverage_batch(fgs, starts, seed=[1], **kw)
    with pytest.raises(ValueError, match="one estimate per graph"):
        range_leverage_batch(fgs, starts[:1], **kw)
    for call in (lambda **k: range_leverage_batch(fgs, starts, **k), lambda **k: predicted_range_variances_batch(fgs, starts, [[], []], **k)):
        with pytest.raises(ValueError, match="engine"):
            call(engine="host")
        with pytest.raises(ValueError, match="max_group"):
            call(engine="python", max_group=0)
        for bad, words in ((dict(block_width=0), "block_width"), (dict(block_width=17), "block_width"), (dict(rel_tol=0.0), "rel_tol"),
                           (dict(max_iters=0), "max_iters")):
            with pytest.raises(ValueError, match=words):
                call(engine="python", **bad)
    for bad, words in ((dict(n_samples=0), "n_samples"), (dict(n_samples=2.5), "n_samples"), (dict(n_samples=[2, 0]), "n_samples"),
                       (dict(first_sample=-1), "first_sample"), (dict(first_sample=2 ** 32 - 1), "first_sample")):
        with pytest.raises(ValueError, match=words):
            range_leverage_batch(fgs, starts, **{**kw, **bad})


def test_refine_estimate_batch_forms_the_leverage_at_the_refined_points():
    """refine_estimate_batch(leverage=S) on the python engine: the refinement is what it is without the keyword, and graph i's
    leverage is range_leverage's at the refined estimate from the stream leverage_seed + i."""
    keys = ("C", "B")
    fgs, starts = [member(k)[0] for k in keys], [member(k)[1] for k in keys]
    out = refine_estimate_batch(fgs, starts, engine="python", leverage=4, leverage_seed=9)
    plain = refine_estimate_batch(fgs, starts, engine="python")
    for i, (fg, (res, info), (res_p, info_p)) in enumerate(zip(fgs, out, plain)):
        lev, li = info["leverage"]
        assert "leverage" not in info_p and info["cost_final"] == info_p["cost_final"] and info["iterations"] == info_p["iterations"]
        for nm in res_p.poses:
            np.testing.assert_array_equal(res.poses[nm], res_p.poses[nm])
        alone, _ = range_leverage(fg, res_p, n_samples=4, seed=9 + i, engine="python")
        assert lev.count == 4 and li["engine"] == "python"
        np.testing.assert_array_equal(lev.leverage, alone.leverage)
        np.testing.assert_array_equal(lev.redundancy, alone.redundancy)
    with pytest.raises(ValueError, match="n_samples"):
        refine_estimate_batch(fgs, starts, engine="python", leverage=0)


def test_plan_on_hand_written_cases_under_sanitizers(tmp_path):
    """tests/tools/leverage_batch_plan_check.cpp: the plan of csrc/score_leverage_batch_plan.hpp -- where the members' sums and
    pairs start, the member, pass and slot of every pair, NV per pass -- against tables written by hand there, for the draw
    counts [17, 5, 0, 16, 1] at width 4, the pair counts [5, 0, 3, 260, 1], an all-empty list and every argument error; it
    exits non-zero unless every branch is reached."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / "leverage_batch_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "score_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "leverage_batch_plan_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "every branch reached" in run.stdout
