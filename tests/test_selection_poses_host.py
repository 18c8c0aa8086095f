"""Greedy selection of candidate loop closures (score_amd/selection_poses.py): what runs without a GPU -- the rule of
csrc/score_select_poses_rule.hpp as a stand-alone program (plain and under the host sanitizers), the NumPy restatement against
the tables that program prints, the python engine against the dense H (slogdet increments of H + sum G_c' N_c^-1 G_c, the
brute-force argmax, the single gains of predicted_relative_poses), the precondition of the kernel tests, the argument errors
and the binding table of include/score_select_poses.h.  The device path is tests/test_selection_poses_gpu.py."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from marginals_helpers import EPS
from score_amd import bindings
from score_amd.bindings import (LATER_TABLES, SELECT_POSES, TABLES, TABLES_AFTER, TABLES_GROUP_PAIRS, TABLES_GROUP_SELECTION,
                                TABLES_LATEST, TABLES_POSE_SELECTION, TABLES_SELECTION, TABLES_SINCE, ScoreMarginalsInfo,
                                ScoreSelectPosesInfo, bind)
from score_amd.relative import measurement_noise, predicted_relative_poses
from score_amd.selection_poses import (SELECT_POSES_SYMBOLS, PoseSelection, PoseSelectionHandle, block_greedy_reference,
                                       column_precisions, select_loop_closures)
from selection_poses_helpers import (BASE_PRECISIONS, CASES, LONG_CASES, MIN_GAP, SHAPES, SLOT_SHAPES, bounded_block_reference, candidates,
                                     dense_candidates, dense_long_matrix, dof, long_candidates, precisions, random_block_matrix, reference,
                                     slogdet_block_gains, slot_block_matrix)
from test_binding_tables_host import SCALARS, _declarations, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"plain": ("-O2",), "sanitizers": ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")}


def _names(prob, ids):
    names = [str(nm) for nm in prob.a["pose_names"]]
    return [(names[a], names[b]) for a, b in ids]


@functools.lru_cache(maxsize=None)
def _rule_program(kind):
    """tests/tools/select_poses_rule_check.cpp built with FLAGS[kind] and run once: its completed process."""
    import tempfile

    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "select_poses_rule_check")
        subprocess.run([gxx, "-std=c++17", *FLAGS[kind], "-I", os.path.join(ROOT, "score_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "tools", "select_poses_rule_check.cpp")], check=True)
        return subprocess.run([exe], capture_output=True, text=True)


@pytest.mark.parametrize("kind", sorted(FLAGS))
def test_rule_program(kind):
    """selp_greedy_host, selp_gain, selp_stop, selp_scaled, selp_weights and selp_check on tables written by hand: the identity,
    a duplicate, a zero block, an exclusion, the min_gain stop, coupled blocks in 2-D and 3-D, the argument checks."""
    run = _rule_program(kind)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip().splitlines()[-1] == "every branch reached" and run.stderr == ""


def _tables(text):
    """The tables the program printed: a list of dicts."""
    out = []
    for line in text.splitlines():
        words = line.split()
        if words[0] == "case":
            out.append({"name": words[1], "dim": int(words[3]), "C": int(words[5]), "k": int(words[7]), "min_gain": float(words[9])})
        elif words[0] != "every":
            out[-1][words[0]] = np.array([float(x) for x in words[1:]])
    return out


def test_reference_on_the_tables_of_the_rule_program():
    """block_greedy_reference on every table the program prints, against what selp_greedy_host returned there.  Both sides do
    the same IEEE additions, products, divisions and square roots in the same order (g++ contracts nothing on plain x86-64), so
    the order, the pick covariances and the remaining covariances are equal.  A gain is half a sum of dp logarithms, each
    within 1 ulp on either side (libm's and NumPy's: 2 eps |log pi_q| between them), with dp - 1 additions of eps / 2 each per
    side; every pivot of these tables is >= 1, so sum |log pi_q| = 2 gain and the two sides differ by at most (dp + 1) eps gain."""
    tables = _tables(_rule_program("plain").stdout)
    assert sorted(t["name"] for t in tables) == sorted(["identity", "duplicate", "duplicate_k1", "duplicate_3d", "zero_block", "excluded",
                                                        "min_gain", "coupled", "coupled_k2", "coupled_3d"])
    for t in tables:
        dp, n, k = dof(t["dim"]), t["C"], t["k"]
        N = n * dp
        w = column_precisions(t["dim"], t["kappa"], t["tau"], n)
        excluded = t["excluded"].astype(np.int32)
        out = block_greedy_reference(t["P"].reshape(N, N), w, dp, k, t["min_gain"], excluded if excluded.any() else None)
        assert out["picked"] == int(t["picked"][0]), t["name"]
        np.testing.assert_array_equal(out["order"], t["order"].astype(np.int32), err_msg=t["name"])
        np.testing.assert_array_equal(out["pick_covariances"].reshape(-1), t["pick"], err_msg=t["name"])
        np.testing.assert_array_equal(out["remaining"].reshape(-1), t["remaining"], err_msg=t["name"])
        assert np.all(np.abs(out["gains"] - t["gains"]) <= (dp + 1) * EPS * np.abs(t["gains"])), t["name"]
        both = block_greedy_reference(t["P"].reshape(N, N), w, dp, k, t["min_gain"], excluded if excluded.any() else None, dtype=np.longdouble)
        np.testing.assert_array_equal(both["order"], out["order"], err_msg=t["name"])
    by = {t["name"]: t for t in tables}
    assert by["identity"]["order"].tolist() == [0, 1, 2] and len(set(by["identity"]["gains"].tolist())) == 1
    assert by["duplicate"]["order"].tolist() == [0, 1] and by["duplicate"]["gains"][1] < by["duplicate"]["gains"][0]
    assert by["zero_block"]["picked"][0] == 1 and by["excluded"]["order"].tolist() == [0, 2, -1] and by["min_gain"]["picked"][0] == 2


@pytest.mark.parametrize("base", BASE_PRECISIONS)
@pytest.mark.parametrize("key", sorted(CASES))
def test_python_engine_against_the_dense_information(key, base):
    """gains[j] are the slogdet increments of H + sum G_c' N_c^-1 G_c (1e-9: selection_poses_helpers), the first two picks the
    brute-force argmax of that increment, the gains do not increase, the covariances are those of predicted_relative_poses,
    the first gain is the largest single information_gain, and a remaining covariance is G_c (H + sum_S ...)^-1 G_c'."""
    fg, results, ref = reference(key)
    ids, count, k = candidates(key)
    dim = fg.dimension
    dp = dof(dim)
    kappa, tau = precisions(count, base)
    names = _names(ref.prob, ids)
    sel, info = select_loop_closures(fg, results, names, k, translation_precision=kappa, rotation_precision=tau, engine="python")
    assert isinstance(sel, PoseSelection) and info["engine"] == "python" and len(sel.order) == k == len(sel.pairs)
    assert len(set(sel.order.tolist())) == k and sel.excluded.size == 0 and sel.pick_covariance.shape == (k, dp, dp)
    G, X, P = dense_candidates(key)
    w = column_precisions(dim, kappa, tau, count)
    np.testing.assert_array_equal(1.0 / w.reshape(count, dp), np.diagonal(measurement_noise(dim, kappa, tau, count), axis1=1, axis2=2))
    want = slogdet_block_gains(ref.H, G, w, dp, sel.order)
    err = float(np.max(np.abs(sel.gains - want)))
    print(f"{key}, base {base}: gains {sel.gains.min():.3f} .. {sel.gains.max():.3f}, total {sel.total_gain:.3f}, "
          f"worst |gain - slogdet increment| {err:.3e}")
    assert err <= 1e-9
    assert abs(sel.total_gain - float(np.sum(want))) <= 1e-9 * k
    assert np.all(sel.gains[1:] <= sel.gains[:-1] * (1 + 1e-12))
    # the single gains: predicted_relative_poses' on the same pairs; the first pick is their argmax, its gain their maximum
    pred, _ = predicted_relative_poses(fg, results, names, engine="python")
    single = pred.information_gain(kappa, tau)
    # (two groupings of the same dot products of n terms: n eps |G_c|'|X_c| apart at most, entry by entry; through
    # total_gain_bound's argument that moves 1/2 logdet(I + D P_c D) by at most 1/2 dp e / (1 - e), e = |D dP D|_F)
    dP = np.stack([ref.n * EPS * (np.abs(G[:, c * dp:(c + 1) * dp]).T @ np.abs(X[:, c * dp:(c + 1) * dp])) for c in range(count)])
    assert np.all(np.abs(sel.covariance - pred.covariance) <= dP)
    first = int(sel.order[0])
    sw = np.sqrt(w[first * dp:(first + 1) * dp])
    e = float(np.linalg.norm(sw[:, None] * dP[first] * sw[None, :]))
    assert int(np.argmax(single)) == first and abs(single.max() - sel.gains[0]) <= 0.5 * dp * e / (1 - e) + 2 * (dp + 1) * EPS * sel.gains[0]
    ranked = np.argsort(-single)[:k]
    print(f"{key}, base {base}: joint gain {sel.total_gain:.1f} against the sum of the {k} best single gains "
          f"{float(np.sum(single[ranked])):.1f}, {len(set(ranked.tolist()) & set(sel.order.tolist()))} of {k} picks shared")
    assert sel.total_gain <= float(np.sum(single[ranked])) * (1 + 1e-12)   # (submodular: single gains only over-promise)
    # the first two picks by brute force: the candidate whose addition raises logdet most
    M = ref.H.copy()
    for j in range(2):
        base_ld = np.linalg.slogdet(M)[1]
        inc = np.full(count, -np.inf)
        for c in range(count):
            if c not in sel.order[:j]:
                Gc = G[:, c * dp:(c + 1) * dp]
                inc[c] = np.linalg.slogdet(M + (Gc * w[c * dp:(c + 1) * dp]) @ Gc.T)[1] - base_ld
        assert int(np.argmax(inc)) == sel.order[j], (j, np.sort(inc)[-2:])
        Gp = G[:, sel.order[j] * dp:(sel.order[j] + 1) * dp]
        M = M + (Gp * w[sel.order[j] * dp:(sel.order[j] + 1) * dp]) @ Gp.T
    # the covariances once the picks are measured, from a dense solve with H + sum_S G_c' N_c^-1 G_c: both sides are
    # backward-stable dense solves in double, held within selection_helpers.dense_rtol's n eps cond_2 argument -- cond_2 of the
    # updated matrix computed here
    Hs = ref.H.copy()
    for c in sel.order:
        Gc = G[:, c * dp:(c + 1) * dp]
        Hs = Hs + (Gc * w[c * dp:(c + 1) * dp]) @ Gc.T
    ev = np.linalg.eigvalsh(Hs)
    rtol = ref.n * EPS * float(ev[-1] / min(ev[0], ref.lambda_min))
    left = np.setdiff1d(np.arange(count), sel.order)
    for c in left[:4]:
        Gc = G[:, c * dp:(c + 1) * dp]
        after = Gc.T @ np.linalg.solve(Hs, Gc)
        assert np.all(np.abs(sel.remaining_covariance[c] - after) <= rtol * np.abs(after).max()), (c, rtol)
    assert np.all(np.isnan(sel.remaining_covariance[sel.order])) and np.all(np.isnan(sel.remaining_gain[sel.order]))
    assert np.all(sel.remaining_gain[left] <= sel.gains[-1] * (1 + 1e-12)) and np.all(sel.remaining_gain[left] >= 0)


def test_scalar_precisions_and_min_gain():
    fg, results, ref = reference("a")
    ids, count, k = candidates("a")
    names = _names(ref.prob, ids)
    full, _ = select_loop_closures(fg, results, names, k, translation_precision=4.0, rotation_precision=10.0, engine="python")
    same, _ = select_loop_closures(fg, results, names, k, translation_precision=np.full(count, 4.0), rotation_precision=np.full(count, 10.0),
                                   engine="python")
    np.testing.assert_array_equal(full.order, same.order)
    np.testing.assert_array_equal(full.gains, same.gains)
    cut = 0.5 * (full.gains[3] + full.gains[4])
    assert full.gains[4] < cut < full.gains[3]
    short, _ = select_loop_closures(fg, results, names, k, translation_precision=4.0, rotation_precision=10.0, min_gain=cut, engine="python")
    np.testing.assert_array_equal(short.order, full.order[:4])
    assert short.pairs == full.pairs[:4] and np.count_nonzero(np.isnan(short.remaining_gain)) == 4


@pytest.mark.parametrize("dim,n,k", SHAPES)
def test_the_seeds_of_the_kernel_tests_satisfy_the_gap_precondition(dim, n, k):
    """The precondition of tests/test_selection_poses_gpu.py, checked where no GPU is: on every shape the reference alone has a
    smallest relative gap >= MIN_GAP and the bound of the two best gains below half their gap (bounded_block_reference asserts
    both), and its double and long-double orders agree."""
    P, kappa, tau = random_block_matrix(n, dim)
    ref = bounded_block_reference(P, kappa, tau, dim, k)
    print(f"dim {dim}, C = {n}, k = {k}: smallest gap {ref['min_gap']:.3e}, largest gain bound {ref['gain_bound'].max():.3e}")
    assert ref["picked"] == k and (n == 1 or ref["min_gap"] >= MIN_GAP)
    np.testing.assert_array_equal(block_greedy_reference(P, column_precisions(dim, kappa, tau, n), dof(dim), k)["order"], ref["order"])
    assert ref["asymmetry"] > 0


@pytest.mark.parametrize("dim,n,k", SLOT_SHAPES)
def test_the_seeds_of_the_slot_shapes_satisfy_the_gap_precondition(dim, n, k):
    """The same for the shapes that reach the ownership slots and the caps, with the rule alone (the bounds, 10 s at the caps,
    are the GPU test's, which asserts the whole precondition): the long-double rule's smallest relative gap >= MIN_GAP, and
    the double rule's order equal to it."""
    P, kappa, tau = slot_block_matrix(n, dim)
    w = column_precisions(dim, kappa, tau, n)
    ref = block_greedy_reference(P, w.astype(np.longdouble), dof(dim), k, dtype=np.longdouble)
    print(f"dim {dim}, C = {n}, k = {k}: smallest gap {ref['min_gap']:.3e}")
    assert ref["picked"] == k and ref["min_gap"] >= MIN_GAP and ref["asymmetry"] > 0
    np.testing.assert_array_equal(block_greedy_reference(P, w, dof(dim), k)["order"], ref["order"])


@pytest.mark.parametrize("base", BASE_PRECISIONS)
@pytest.mark.parametrize("key", sorted(LONG_CASES))
def test_the_long_list_satisfies_the_gap_precondition(key, base):
    """The precondition of the long list of tests/test_selection_poses_gpu.py on the dense P, at both bases: the smallest gap
    >= MIN_GAP and the bound of the two best gains below half their gap (bounded_block_reference asserts both; never
    skipped)."""
    ids, count, k = long_candidates(key)
    dim = reference(key)[0].dimension
    kappa, tau = precisions(count, base)
    ref = bounded_block_reference(dense_long_matrix(key), kappa, tau, dim, k)
    pairs = {tuple(sorted(p)) for p in ids.tolist()}
    print(f"{key}, C = {count} ({len(pairs)} different unordered pairs), k = {k}, base {base}: smallest gap {ref['min_gap']:.3e}")
    assert ref["picked"] == k and ref["min_gap"] >= MIN_GAP and 300 <= count <= 400 and k >= 8 and len(pairs) == count
    want = block_greedy_reference(dense_long_matrix(key), column_precisions(dim, kappa, tau, count), dof(dim), k)["order"]
    np.testing.assert_array_equal(want, ref["order"])


def test_argument_errors():
    fg, results, ref = reference("a")
    ids, count, k = candidates("a")
    names = _names(ref.prob, ids)
    landmark = str(ref.prob.a["landmark_names"][0])
    for engine in ("python", "device"):  # (these errors come before any work: no library is opened)
        kw = dict(engine=engine, lib_path="/nonexistent/libscore_hip.so")
        with pytest.raises(ValueError, match="select_loop_closures: no pairs"):
            select_loop_closures(fg, results, [], 1, **kw)
        with pytest.raises(ValueError, match="select_loop_closures: unknown variable Z9"):
            select_loop_closures(fg, results, [("Z9", names[0][1])], 1, **kw)
        with pytest.raises(ValueError, match="is a landmark: a relative pose joins two poses"):
            select_loop_closures(fg, results, [(names[0][1], landmark)], 1, **kw)
        with pytest.raises(ValueError, match=r"k must be 1..min\(candidates, 85\)"):
            select_loop_closures(fg, results, names, 0, **kw)
        with pytest.raises(ValueError, match=r"k must be 1..min\(candidates, 85\)"):
            select_loop_closures(fg, results, names, count + 1, **kw)
        with pytest.raises(ValueError, match="min_gain must be >= 0"):
            select_loop_closures(fg, results, names, k, min_gain=-1.0, **kw)
        for bad in (0.0, -1.0, np.nan, np.inf, np.ones(count - 1)):
            with pytest.raises(ValueError, match="one finite, positive precision per candidate"):
                select_loop_closures(fg, results, names, k, translation_precision=bad, **kw)
            with pytest.raises(ValueError, match="one finite, positive precision per candidate"):
                select_loop_closures(fg, results, names, k, rotation_precision=bad, **kw)
        with pytest.raises(ValueError, match="block_width"):
            select_loop_closures(fg, results, names, k, block_width=17, **kw)
    with pytest.raises(ValueError, match="engine must be 'device' or 'python'"):
        select_loop_closures(fg, results, names, k, engine="numpy")


def test_table_matches_header():
    table = SELECT_POSES
    assert TABLES_POSE_SELECTION == (SELECT_POSES,) and table.name == "select_poses"
    assert all(table not in group for group in (TABLES, LATER_TABLES, TABLES_SINCE, TABLES_AFTER, TABLES_LATEST, TABLES_GROUP_PAIRS,
                                                TABLES_SELECTION, TABLES_GROUP_SELECTION))
    assert PoseSelectionHandle.headers[-1] is SELECT_POSES and hasattr(PoseSelectionHandle, "select_relative_poses")
    assert hasattr(PoseSelectionHandle, "select_ranges") and hasattr(PoseSelectionHandle, "relative_covariances")
    declared = _declarations(table.name)
    assert sorted(declared) == sorted(table) == sorted(SELECT_POSES_SYMBOLS) == ["score_refine_select_relative_poses",
                                                                                "score_select_block_greedy"]
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
    assert len(table["score_refine_select_relative_poses"][0]) == 24 and len(table["score_select_block_greedy"][0]) == 14
    assert table["score_refine_select_relative_poses"][0][-1]._type_ is ScoreSelectPosesInfo
    # the record, field by field, against the header's struct
    with open(os.path.join(ROOT, "include", "score_select_poses.h")) as f:
        body = re.search(r"typedef struct score_select_poses_info \{(.*?)\} score_select_poses_info;", f.read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        fields += [(name, words[0]) for name in words[1:]]
    kinds = {"score_marginals_info": ScoreMarginalsInfo, "int32_t": C.c_int32, "double": C.c_double}
    assert [(n, kinds[t]) for n, t in fields] == list(ScoreSelectPosesInfo._fields_)
    assert ScoreSelectPosesInfo().as_dict()["solve"] == ScoreMarginalsInfo().as_dict()
    # the tuple after TABLES_GROUP_SELECTION in the module's text: the earlier tuples are pinned by their tests
    with open(bindings.__file__) as f:
        text = f.read()
    assert text.index("TABLES_GROUP_SELECTION = ") < text.index("TABLES_POSE_SELECTION = ")


def test_missing_symbol():
    for sym in SELECT_POSES:
        with pytest.raises(RuntimeError, match=re.escape(f"{sym} is missing from the library: rebuild it "
                                                         "(the CPU twin has no selection of loop closures: engine='python' runs there)")):
            bind(_Stub(lacks=sym), SELECT_POSES)
