"""Greedy selection of candidate ranges (score_amd/selection.py): what runs without a GPU -- the python engine against the
dense H (slogdet increments, the brute-force argmax, Woodbury's remaining variances), the rule of csrc/score_select_rule.hpp
as a stand-alone program (plain and under the host sanitizers), the NumPy restatement on the same hand-written tables, the
argument errors and the binding table of include/score_select.h.  The device path is tests/test_selection_gpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from score_amd import bindings
from score_amd.bindings import (LATER_TABLES, SELECT, TABLES, TABLES_AFTER, TABLES_GROUP_PAIRS, TABLES_LATEST, TABLES_SELECTION,
                                TABLES_SINCE, ScoreMarginalsInfo, ScoreSelectInfo, bind)
from score_amd.selection import SELECT_SYMBOLS, Selection, SelectionHandle, greedy_reference, select_ranges
from selection_helpers import (BASE_PRECISIONS, CASES, LONG_CASES, MIN_GAP, SEEDS, SHAPES, SLOT_SHAPES, bounded_reference, candidates,
                               dense_candidates, dense_long_matrix, dense_rtol, long_candidates, precisions, random_matrix, reference,
                               slogdet_gains, slot_matrix)
from test_binding_tables_host import SCALARS, _declarations, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names(prob, ids):
    names = [str(nm) for nm in prob.a["pose_names"]] + [str(nm) for nm in prob.a["landmark_names"]]
    return [(names[a], names[b]) for a, b in ids]


@pytest.mark.parametrize("base", BASE_PRECISIONS)
@pytest.mark.parametrize("key", sorted(CASES))
def test_python_engine_against_the_dense_information(key, base):
    """gains[j] are the slogdet increments of H + sum w g g' (1e-9: selection_helpers), the first three picks the brute-force
    argmax of that increment, the gains do not increase, and the remaining variance of an unpicked candidate is
    g_c'(H + G_S W_S G_S')^-1 g_c from a dense solve (within dense_rtol: selection_helpers)."""
    fg, results, ref = reference(key)
    ids, count, k = candidates(key)
    w = precisions(count, base)
    sel, info = select_ranges(fg, results, _names(ref.prob, ids), k, precision=w, engine="python")
    assert isinstance(sel, Selection) and info["engine"] == "python" and len(sel.order) == k == len(sel.pairs)
    assert len(set(sel.order.tolist())) == k and sel.excluded.size == 0
    G, dist, P, _ = dense_candidates(key)
    want = slogdet_gains(ref.H, G, w, sel.order)
    err = float(np.max(np.abs(sel.gains - want)))
    print(f"{key}, precision {base}: gains {sel.gains.min():.3f} .. {sel.gains.max():.3f}, worst |gain - slogdet increment| {err:.3e}")
    assert err <= 1e-9
    assert abs(sel.total_gain - float(np.sum(want))) <= 1e-9 * k
    assert np.all(sel.gains[1:] <= sel.gains[:-1] * (1 + 1e-12))
    rtol = dense_rtol(key, w)
    print(f"{key}, precision {base}: dense_rtol = n eps cond(H) (1 + 2 sum w / lambda_max) = {rtol:.3e}")
    np.testing.assert_allclose(sel.variance, np.diag(P), rtol=rtol)
    np.testing.assert_array_equal(sel.distance, dist)
    # the first three picks by brute force: the candidate whose addition raises logdet most
    M = ref.H.copy()
    for j in range(3):
        base_ld = np.linalg.slogdet(M)[1]
        inc = np.full(count, -np.inf)
        for c in range(count):
            if c not in sel.order[:j]:
                inc[c] = np.linalg.slogdet(M + w[c] * np.outer(G[:, c], G[:, c]))[1] - base_ld
        assert int(np.argmax(inc)) == sel.order[j], (j, np.sort(inc)[-2:])
        M = M + w[sel.order[j]] * np.outer(G[:, sel.order[j]], G[:, sel.order[j]])
    # Woodbury: the variances once the picks are measured
    S = sel.order
    Hs = ref.H + (G[:, S] * w[S]) @ G[:, S].T
    left = np.setdiff1d(np.arange(count), S)
    after = np.einsum("ic,ic->c", G[:, left], np.linalg.solve(Hs, G[:, left]))
    np.testing.assert_allclose(sel.remaining_variance[left], after, rtol=rtol)
    assert np.all(np.isnan(sel.remaining_variance[S])) and np.all(sel.remaining_variance[left] <= sel.variance[left] * (1 + 1e-12))
    # the variance of a pick given the picks before it
    for j in (0, k - 1):
        Hj = ref.H + (G[:, S[:j]] * w[S[:j]]) @ G[:, S[:j]].T
        g = G[:, S[j]]
        np.testing.assert_allclose(sel.pick_variance[j], g @ np.linalg.solve(Hj, g), rtol=rtol)


def test_a_scalar_precision_and_min_gain():
    fg, results, ref = reference("a")
    ids, count, k = candidates("a")
    names = _names(ref.prob, ids)
    full, _ = select_ranges(fg, results, names, k, precision=4.0, engine="python")
    same, _ = select_ranges(fg, results, names, k, precision=np.full(count, 4.0), engine="python")
    np.testing.assert_array_equal(full.order, same.order)
    np.testing.assert_array_equal(full.gains, same.gains)
    cut = 0.5 * (full.gains[3] + full.gains[4])
    assert full.gains[4] < cut < full.gains[3]
    short, _ = select_ranges(fg, results, names, k, precision=4.0, min_gain=cut, engine="python")
    np.testing.assert_array_equal(short.order, full.order[:4])
    assert short.pairs == full.pairs[:4] and np.count_nonzero(np.isnan(short.remaining_variance)) == 4


def test_reference_on_the_tables_of_the_rule_program():
    """greedy_reference on tables of tests/tools/select_rule_check.cpp (A = I + D S D given as P = A - I with unit precisions, or
    as stated there): the tie, the duplicate, the exclusion, d <= 1, the min_gain stop."""
    def run(A, w, k, min_gain=0.0, excluded=None):
        A, w = np.asarray(A, dtype=np.float64), np.asarray(w, dtype=np.float64)
        sw = np.sqrt(w)
        return greedy_reference((A - np.eye(len(w))) / np.outer(sw, sw), w, k, min_gain, excluded)

    out = run(np.diag([3.0, 3.0, 2.0]), [1, 1, 1], 3)
    assert out["order"].tolist() == [0, 1, 2] and out["picked"] == 3 and out["min_gap"] == 0.0
    np.testing.assert_allclose(out["gains"], 0.5 * np.log([3, 3, 2]), rtol=4e-16)
    out = run([[5, 4], [4, 5]], [4, 4], 2)
    assert out["order"].tolist() == [0, 1] and out["gains"][1] < out["gains"][0]
    np.testing.assert_allclose(out["pick_variances"], [1.0, 0.2], rtol=1e-15)
    out = run(np.diag([3.0, 9.0, 2.0]), [1, 2, 1], 3, excluded=[0, 1, 0])
    assert out["order"].tolist() == [0, 2, -1] and out["picked"] == 2 and out["remaining"][1] == 4.0
    out = run(np.diag([2.0, 1.0, 1.0]), [1, 1, 1], 3)
    assert out["order"].tolist() == [0, -1, -1] and out["picked"] == 1 and out["remaining"].tolist() == [1.0, 0.0, 0.0]
    out = run(np.diag([4.0, 9.0, 1.5]), [1, 1, 2], 3, min_gain=0.5)
    assert out["order"].tolist() == [1, 0, -1] and out["gains"][2] == 0.0 and out["remaining"][2] == 0.25
    out = run([[4, 2, 0], [2, 3, 1], [0, 1, 3.5]], [1, 1, 1], 3)
    assert out["order"].tolist() == [0, 2, 1]
    np.testing.assert_allclose(out["gains"], 0.5 * np.log([4, 3.5, 2 - 1 / 3.5]), rtol=1e-15)


@pytest.mark.parametrize("n,k", SHAPES)
def test_the_seeds_of_the_kernel_tests_satisfy_the_gap_precondition(n, k):
    """The precondition of tests/test_selection_gpu.py, checked where no GPU is: on every shape the reference alone has a
    smallest relative pivot gap >= MIN_GAP (bounded_reference asserts it) and its double and long-double orders agree."""
    P, w = random_matrix(n, SEEDS[n])
    ref = bounded_reference(P, w, k)
    assert ref["picked"] == k and (n == 1 or ref["min_gap"] >= MIN_GAP)
    np.testing.assert_array_equal(greedy_reference(P, w, k)["order"], ref["order"])
    assert np.all(ref["gain_bound"] < 1e-9) and (ref["asymmetry"] > 0 or n == 1)


@pytest.mark.parametrize("n,k", SLOT_SHAPES)
def test_the_seeds_of_the_slot_shapes_satisfy_the_gap_precondition(n, k):
    """The same for the shapes that reach the ownership slots and the caps, with the rule alone (the bounds, 11 s at the caps,
    are the GPU test's, which asserts the whole precondition): the long-double rule's smallest relative pivot gap >= MIN_GAP,
    and the double rule's order equal to it."""
    P, w = slot_matrix(n)
    ref = greedy_reference(P, w, k, dtype=np.longdouble)
    print(f"C = {n}, k = {k}: smallest pivot gap {ref['min_gap']:.3e}")
    assert ref["picked"] == k and ref["min_gap"] >= MIN_GAP and ref["asymmetry"] > 0
    np.testing.assert_array_equal(greedy_reference(P, w, k)["order"], ref["order"])


@pytest.mark.parametrize("base", BASE_PRECISIONS)
@pytest.mark.parametrize("key", sorted(LONG_CASES))
def test_the_long_list_satisfies_the_gap_precondition(key, base):
    """The precondition of the long list of tests/test_selection_gpu.py on the dense P, at both base precisions: the smallest
    gap >= MIN_GAP and the bound E_d of every pivot below half of it (bounded_reference asserts both; never skipped)."""
    ids, count, k = long_candidates(key)
    P, w = dense_long_matrix(key), precisions(count, base)
    ref = bounded_reference(P, w, k)
    pairs = {tuple(sorted(p)) for p in ids.tolist()}
    print(f"{key}, C = {count} ({len(pairs)} different unordered pairs), k = {k}, base {base}: smallest pivot gap {ref['min_gap']:.3e}")
    assert ref["picked"] == k and ref["min_gap"] >= MIN_GAP and 600 <= count <= 700 and k >= 16
    np.testing.assert_array_equal(greedy_reference(P, w, k)["order"], ref["order"])


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitizers"])
def test_rule_program(tmp_path, flags):
    """tests/tools/select_rule_check.cpp: sel_greedy_host, sel_better, sel_stop and sel_check on tables written by hand."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / "select_rule_check")
    subprocess.run([gxx, "-std=c++17", *flags, "-I", os.path.join(ROOT, "score_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "select_rule_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "every branch reached" and run.stderr == ""


def test_argument_errors():
    fg, results, ref = reference("a")
    ids, count, k = candidates("a")
    names = _names(ref.prob, ids)
    for engine in ("python", "device"):  # (these errors come before any work: no library is opened)
        kw = dict(engine=engine, lib_path="/nonexistent/libscore_hip.so")
        with pytest.raises(ValueError, match="select_ranges: no pairs"):
            select_ranges(fg, results, [], 1, **kw)
        with pytest.raises(ValueError, match="select_ranges: unknown variable Z9"):
            select_ranges(fg, results, [("Z9", names[0][1])], 1, **kw)
        with pytest.raises(ValueError, match=r"k must be 1..min\(candidates, 256\)"):
            select_ranges(fg, results, names, 0, **kw)
        with pytest.raises(ValueError, match=r"k must be 1..min\(candidates, 256\)"):
            select_ranges(fg, results, names, count + 1, **kw)
        with pytest.raises(ValueError, match="min_gain must be >= 0"):
            select_ranges(fg, results, names, k, min_gain=-1.0, **kw)
        for bad in (0.0, -1.0, np.nan, np.inf, np.ones(count - 1)):
            with pytest.raises(ValueError, match="one finite, positive precision per candidate"):
                select_ranges(fg, results, names, k, precision=bad, **kw)
        with pytest.raises(ValueError, match="block_width"):
            select_ranges(fg, results, names, k, block_width=17, **kw)
    with pytest.raises(ValueError, match="engine must be 'device' or 'python'"):
        select_ranges(fg, results, names, k, engine="numpy")


def test_table_matches_header():
    table = SELECT
    assert TABLES_SELECTION == (SELECT,) and table.name == "select"
    assert all(table not in group for group in (TABLES, LATER_TABLES, TABLES_SINCE, TABLES_AFTER, TABLES_LATEST, TABLES_GROUP_PAIRS))
    assert SelectionHandle.headers[-1] is SELECT and hasattr(SelectionHandle, "select_ranges")
    declared = _declarations(table.name)
    assert sorted(declared) == sorted(table) == sorted(SELECT_SYMBOLS) == ["score_refine_select_ranges", "score_select_greedy"]
    lib = bind(_Stub(), table)
    assert bind(lib, table) is lib  # (bound once)
    for sym, params in declared.items():
        argtypes, restype = table[sym]
        assert restype is C.c_int and lib.__dict__[sym].argtypes == argtypes and len(argtypes) == len(params), sym
        for param, typ in zip(params, argtypes):
            is_pointer = typ is C.c_void_p or hasattr(typ, "contents")
            assert ("*" in param) == is_pointer, (sym, param, typ)
            if not is_pointer:
                assert SCALARS[param.split()[-2]] is typ, (sym, param, typ)
    assert len(table["score_refine_select_ranges"][0]) == 22 and len(table["score_select_greedy"][0]) == 12
    assert table["score_refine_select_ranges"][0][-1]._type_ is ScoreSelectInfo
    # the record, field by field, against the header's struct
    with open(os.path.join(ROOT, "include", "score_select.h")) as f:
        body = re.search(r"typedef struct score_select_info \{(.*?)\} score_select_info;", f.read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        fields += [(name, words[0]) for name in words[1:]]
    kinds = {"score_marginals_info": ScoreMarginalsInfo, "int32_t": C.c_int32, "double": C.c_double}
    assert [(n, kinds[t]) for n, t in fields] == list(ScoreSelectInfo._fields_)
    assert ScoreSelectInfo().as_dict()["solve"] == ScoreMarginalsInfo().as_dict()
    # the tuple after TABLES_GROUP_PAIRS in the module's text: the earlier tuples are pinned by their tests
    with open(bindings.__file__) as f:
        text = f.read()
    assert text.index("TABLES_GROUP_PAIRS = ") < text.index("TABLES_SELECTION = ")


def test_missing_symbol():
    for sym in SELECT:
        with pytest.raises(RuntimeError, match=re.escape(f"{sym} is missing from the library: rebuild it "
                                                         "(the CPU twin has no selection of ranges: engine='python' runs there)")):
            bind(_Stub(lacks=sym), SELECT)
