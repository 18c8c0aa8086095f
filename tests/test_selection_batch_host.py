"""Batched greedy selection of candidate ranges (score_amd/selection_batch.py): what runs without a GPU -- the plan of
csrc/score_select_batch_plan.hpp as a stand-alone program (plain and under the host sanitizers), the binding table of
include/score_select_batch.h field by field, the python engine graph by graph, the argument errors with their graph index, and
the pivot-gap precondition of tests/test_selection_batch_gpu.py on the dense P."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from refine_batch_helpers import member
from score_amd import bindings
from score_amd.bindings import (LATER_TABLES, SELECT_BATCH, TABLES, TABLES_AFTER, TABLES_GROUP_PAIRS, TABLES_GROUP_SELECTION,
                                TABLES_LATEST, TABLES_SELECTION, TABLES_SINCE, ScoreMarginalsBatchInfo, ScoreSelectBatchInfo, bind)
from score_amd.refine_batch import RefineBatchHandle, refine_estimate_batch
from score_amd.selection import Selection, greedy_reference, select_ranges
from score_amd.selection_batch import SELECT_BATCH_SYMBOLS, select_ranges_batch
from selection_batch_helpers import BASE_PRECISIONS, PRECONDITION, candidates, dense_matrix, member_twin, names_of, precisions
from selection_helpers import MIN_GAP, bounded_reference
from test_binding_tables_host import SCALARS, _declarations, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitizers"])
def test_plan_program(tmp_path, flags):
    """tests/tools/select_batch_plan_check.cpp: the offsets mat0, l0, pick0, the workgroup -> (member, tile pair) table for
    members of 0, 1, 32, 33 and 260 candidates, every argument error with its message, the 2^28 cap."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / "select_batch_plan_check")
    subprocess.run([gxx, "-std=c++17", *flags, "-I", os.path.join(ROOT, "score_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "select_batch_plan_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "every branch reached" and run.stderr == ""


def test_table_matches_header():
    table = SELECT_BATCH
    assert TABLES_GROUP_SELECTION == (SELECT_BATCH,) and table.name == "select_batch"
    assert all(table not in group for group in (TABLES, LATER_TABLES, TABLES_SINCE, TABLES_AFTER, TABLES_LATEST, TABLES_GROUP_PAIRS,
                                                TABLES_SELECTION))
    assert hasattr(RefineBatchHandle, "select_ranges")
    declared = _declarations(table.name)
    assert sorted(declared) == sorted(table) == sorted(SELECT_BATCH_SYMBOLS) == ["score_refine_batch_select_ranges"]
    lib = bind(_Stub(), table)
    assert bind(lib, table) is lib  # (bound once)
    for sym, params in declared.items():
        argtypes, restype = table[sym]
        assert restype is C.c_int and lib.__dict__[sym].argtypes == argtypes and len(argtypes) == len(params) == 24, sym
        assert argtypes[-1]._type_ is ScoreSelectBatchInfo
        for param, typ in zip(params, argtypes):
            is_pointer = typ is C.c_void_p or hasattr(typ, "contents")
            assert ("*" in param) == is_pointer, (sym, param, typ)
            if is_pointer and typ is not C.c_void_p and typ is not argtypes[-1]:
                assert SCALARS[param.split()[-2].rstrip("*")] is typ._type_, (sym, param, typ)
            if not is_pointer:
                assert SCALARS[param.split()[-2]] is typ, (sym, param, typ)
    # the record, field by field, against the header's struct
    with open(os.path.join(ROOT, "include", "score_select_batch.h")) as f:
        body = re.search(r"typedef struct score_select_batch_info \{(.*?)\} score_select_batch_info;", f.read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        fields += [(name, words[0]) for name in words[1:]]
    kinds = {"score_marginals_batch_info": ScoreMarginalsBatchInfo, "int32_t": C.c_int32, "double": C.c_double}
    assert [(n, kinds[t]) for n, t in fields] == list(ScoreSelectBatchInfo._fields_)
    assert [n for n, _ in fields] == ["solve", "members", "candidates", "picked", "excluded", "total_gain", "asymmetry", "cross_ms", "greedy_ms"]
    assert ScoreSelectBatchInfo().as_dict()["solve"] == ScoreMarginalsBatchInfo().as_dict()
    # the tuple after TABLES_SELECTION in the module's text: the earlier tuples are pinned by their tests
    with open(bindings.__file__) as f:
        text = f.read()
    assert text.index("TABLES_SELECTION = ") < text.index("TABLES_GROUP_SELECTION = ")


def test_missing_symbol():
    sym = list(SELECT_BATCH)[-1]
    with pytest.raises(RuntimeError, match=re.escape(f"{sym} is missing from the library: rebuild it "
                                                     "(the CPU twin has no selection of ranges: engine='python' runs there)")):
        bind(_Stub(lacks=sym), SELECT_BATCH)


def _same(a, b, info_a, info_b):
    assert isinstance(a, Selection) and a.pairs == b.pairs and a.candidates == b.candidates and a.total_gain == b.total_gain
    for f in ("order", "gains", "pick_variance", "variance", "distance", "remaining_variance", "excluded"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    for f in ("residuals", "iterations"):
        np.testing.assert_array_equal(info_a[f], info_b[f], err_msg=f)
    assert info_a["asymmetry"] == info_b["asymmetry"] and info_a["engine"] == info_b["engine"] == "python"


def _lists(keys, counts):
    tws = [member_twin(k) for k in keys]
    ids = [candidates(k, c) for k, c in zip(keys, counts)]
    return [t.fg for t in tws], [t.results for t in tws], [names_of(k, i) for k, i in zip(keys, ids)]


def test_python_engine_equals_the_single_call_graph_by_graph():
    """A 2-D and a 3-D list mixed in one call, k and precision per graph (a scalar, one per candidate), a graph that lists
    none: every graph comes back at its own place with exactly what select_ranges(engine="python") gives on it alone."""
    keys, counts, ks = ("C", "3D1", "E", "B", "3D0"), [9, 7, 0, 5, 6], [4, 7, 3, 5, 2]
    fgs, results, names = _lists(keys, counts)
    ws = [precisions(9, 4.0), 400.0, 1.0, precisions(5, 400.0), 4.0]
    out = select_ranges_batch(fgs, results, names, ks, precision=ws, min_gain=1e-4, engine="python", max_group=2)
    assert len(out) == 5
    for fg, res, nm, k, w, (sel, info) in zip(fgs, results, names, ks, ws, out):
        if not nm:
            assert sel.pairs == [] and sel.order.size == 0 and sel.total_gain == 0.0 and sel.variance.shape == (0,)
            assert info["engine"] == "python" and info["residuals"].shape == (0,) and info["asymmetry"] == 0.0
            continue
        alone, info1 = select_ranges(fg, res, nm, k, precision=w, min_gain=1e-4, engine="python")
        _same(sel, alone, info, info1)
    # one k and one precision for all
    again = select_ranges_batch(fgs[:2], results[:2], names[:2], 3, precision=4.0, engine="python")
    for fg, res, nm, (sel, info) in zip(fgs, results, names, again):
        alone, info1 = select_ranges(fg, res, nm, 3, precision=4.0, engine="python")
        _same(sel, alone, info, info1)
    assert select_ranges_batch([], [], [], 1, engine="python") == []


def test_argument_errors_carry_the_graph_index():
    keys, counts = ("C", "B"), [9, 5]
    fgs, results, names = _lists(keys, counts)
    for engine in ("python", "device"):  # (these errors come before any work: no library is opened)
        kw = dict(engine=engine, lib_path="/nonexistent/libscore_hip.so")
        with pytest.raises(ValueError, match="select_ranges_batch: graph 1: unknown variable Z9"):
            select_ranges_batch(fgs, results, [names[0], [("Z9", names[1][0][1])]], 1, **kw)
        with pytest.raises(ValueError, match="select_ranges_batch: graph 0: the pair .* joins a variable to itself"):
            select_ranges_batch(fgs, results, [[(names[0][0][0], names[0][0][0])], names[1]], 1, **kw)
        with pytest.raises(ValueError, match=r"select_ranges_batch: graph 1: k must be 1..min\(candidates, 256\)"):
            select_ranges_batch(fgs, results, names, [9, 6], **kw)
        with pytest.raises(ValueError, match=r"select_ranges_batch: graph 0: k must be 1..min\(candidates, 256\)"):
            select_ranges_batch(fgs, results, names, 0, **kw)
        with pytest.raises(ValueError, match=r"select_ranges_batch: graph 1: k must be 1..min\(candidates, 256\)"):
            select_ranges_batch(fgs, results, names, 6, **kw)
        with pytest.raises(ValueError, match="select_ranges_batch: graph 0: min_gain must be >= 0"):
            select_ranges_batch(fgs, results, names, 2, min_gain=-1.0, **kw)
        with pytest.raises(ValueError, match="select_ranges_batch: min_gain must be >= 0"):
            select_ranges_batch(fgs, results, [[], []], 2, min_gain=-1.0, **kw)
        for bad in (0.0, np.nan, [4.0, np.inf], [4.0, np.ones(4)], [4.0, -precisions(5, 4.0)]):
            with pytest.raises(ValueError, match=r"select_ranges_batch: graph [01]: one finite, positive precision per candidate"):
                select_ranges_batch(fgs, results, names, 2, precision=bad, **kw)
        with pytest.raises(ValueError, match=r"k: one entry per graph expected \(2\), got 3"):
            select_ranges_batch(fgs, results, names, [1, 1, 1], **kw)
        with pytest.raises(ValueError, match=r"precision: one entry per graph expected \(2\), got 3"):
            select_ranges_batch(fgs, results, names, 1, precision=[1.0, 1.0, 1.0], **kw)
        with pytest.raises(ValueError, match=r"pairs: one entry per graph expected \(2\), got 1"):
            select_ranges_batch(fgs, results, names[:1], 1, **kw)
        with pytest.raises(ValueError, match="block_width"):
            select_ranges_batch(fgs, results, names, 2, block_width=17, **kw)
        with pytest.raises(ValueError, match="max_group"):
            select_ranges_batch(fgs, results, names, 2, max_group=0, **kw)
    with pytest.raises(ValueError, match="engine must be 'device' or 'python'"):
        select_ranges_batch(fgs, results, names, 2, engine="numpy")
    with pytest.raises(ValueError, match="refine_estimate_batch: graph 1: unknown variable Z9"):
        refine_estimate_batch(fgs, results, engine="python", select=dict(pairs=[None, [("Z9", names[1][0][1])]], k=1))
    with pytest.raises(ValueError, match=r"refine_estimate_batch: graph 0: k must be 1..min\(candidates, 256\)"):
        refine_estimate_batch(fgs, results, engine="python", select=dict(pairs=names, k=[10, 1]))
    with pytest.raises(ValueError, match="select: a dict with 'pairs' and 'k'"):
        refine_estimate_batch(fgs, results, engine="python", select=dict(pairs=names))


def test_refine_estimate_batch_python_engine_with_select():
    """The follow-up on the python engine is select_ranges(engine="python") at the refined estimates; without the keyword
    nothing changes."""
    keys = ("C", "B")
    fgs, starts = [member(k)[0] for k in keys], [member(k)[1] for k in keys]
    names = [None, names_of("B", candidates("B", 5))]
    out = refine_estimate_batch(fgs, starts, engine="python", select=dict(pairs=names, k=3, precision=4.0))
    plain = refine_estimate_batch(fgs, starts, engine="python")
    for fg, nm, (res, info), (res_p, info_p) in zip(fgs, names, out, plain):
        sel, sinfo = info["selection"]
        assert "selection" not in info_p and info["cost_final"] == info_p["cost_final"]
        for name in res_p.poses:
            np.testing.assert_array_equal(res.poses[name], res_p.poses[name])
        if nm is None:
            assert sel.pairs == [] and sel.order.size == 0
            continue
        alone, info1 = select_ranges(fg, res_p, nm, 3, precision=4.0, engine="python")
        _same(sel, alone, sinfo, info1)


@pytest.mark.parametrize("base", BASE_PRECISIONS)
@pytest.mark.parametrize("key,count,k", PRECONDITION)
def test_the_lists_of_the_gpu_tests_satisfy_the_gap_precondition(key, count, k, base):
    """The precondition of tests/test_selection_batch_gpu.py, checked where no GPU is, on the dense P of every list at both base
    precisions: the reference's smallest relative gap between the two best pivots is at least MIN_GAP = 1e-6 and the bound E_d of
    every pivot stays below half of it (bounded_reference asserts both; never skipped), and the double and long-double orders
    agree."""
    P, w = dense_matrix(key, count), precisions(count, base)
    ref = bounded_reference(P, w, k)
    print(f"{key}, C = {count}, k = {k}, base {base}: smallest pivot gap {ref['min_gap']:.3e}")
    assert ref["picked"] == k and (count == 1 or ref["min_gap"] >= MIN_GAP)
    np.testing.assert_array_equal(greedy_reference(P, w, k)["order"], ref["order"])
