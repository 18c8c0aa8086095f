"""Greedy selection of candidate ranges on the device (score_select_greedy, score_refine_select_ranges,
csrc/score_select.hpp): the kernels alone on random matrices against the rule in np.longdouble on the same matrix, under the
bounds derived in tests/selection_helpers.py, the exact ties and stops, and the call on a handle -- its columns bit for bit
those of score_refine_range_variances, its matrix under the bound of the range variances, its order held to the rule on its
OWN matrix (near-ties are in the data: never to the dense one).  The same checks reach every ownership slot of k_sel_greedy
and both caps (selection_helpers.SLOT_SHAPES, the exact graded diagonal and the identity at C = 4096, k = 256) and, on a
handle, a list of 650 candidates on graph b."""
import functools

import numpy as np
import pytest

from marginals_helpers import EPS
from selection_helpers import (BASE_PRECISIONS, CAP, CAP_PICKS, CASES, LONG_CASES, SEEDS, SHAPES, SLOT_SHAPES, bounded_reference, candidates,
                               check_against_reference, graded, long_candidates, matrix_bound, precisions, random_matrix, slot_matrix,
                               slot_reference, total_gain_bound, twin)
from score_amd.selection import SelectionHandle, greedy_from_matrix, greedy_reference, select_ranges

pytestmark = pytest.mark.gpu

VALUES = ("order", "gains", "pick_variances", "remaining")


def _same_bits(a, b, keys=VALUES):
    for key in keys:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# ---- the kernels alone ----
@pytest.mark.parametrize("n,k", SHAPES)
def test_kernels_against_the_reference(hip_lib, n, k):
    P, w = random_matrix(n, SEEDS[n])
    ref = bounded_reference(P, w, k)
    out = greedy_from_matrix(P, w, k, lib_path=hip_lib)
    assert out["rc"] == 0 and out["picked"] == ref["picked"] == k
    check_against_reference(out, ref, f"C = {n}, k = {k}")
    assert out["asymmetry"] == float(np.max(np.abs(P - P.T)))  # (a subtraction of two doubles and a max: exact)
    again = greedy_from_matrix(P, w, k, lib_path=hip_lib)
    _same_bits(out, again)
    assert again["asymmetry"] == out["asymmetry"]


@pytest.mark.parametrize("n,k", SLOT_SHAPES)
def test_kernels_against_the_reference_at_every_slot_and_cap(hip_lib, n, k):
    """The checks above where a lane owns up to 16 candidates (selection_helpers.SLOT_SHAPES), up to both caps: the host's
    share is the long-double reference (11 s at C = 4096, k = 256; computed once)."""
    P, w = slot_matrix(n)
    ref = slot_reference(n, k)
    out = greedy_from_matrix(P, w, k, lib_path=hip_lib)
    assert out["rc"] == 0 and out["picked"] == ref["picked"] == k
    check_against_reference(out, ref, f"C = {n}, k = {k}")
    assert out["asymmetry"] == float(np.max(np.abs(P - P.T)))  # (a subtraction of two doubles and a max: exact)
    again = greedy_from_matrix(P, w, k, lib_path=hip_lib)
    _same_bits(out, again)
    assert again["asymmetry"] == out["asymmetry"]


def _graded():
    """(pi, the diagonal 1 + pi / 4096, its dense matrix, the precisions 4, the order argsort(-pi)) at the cap."""
    pi, value = graded(CAP, 4096)
    return pi, value, np.diag(value), np.full(CAP, 4.0), np.argsort(-pi, kind="stable")


def _check_graded(out, value, order, picks, excluded=()):
    """Every product is exact (sqrt 4 = 2, the diagonal a multiple of 2^-12 below 2, exact zeros elsewhere): d_c =
    5 + pi(c) / 1024, the pick variance is the diagonal entry back, every l off the pivot an exact zero -- so `remaining` is
    the diagonal whatever was picked.  The gain is the device's log of an exact d: 2 eps of 1/2 log d in long double, the
    margin of the identity test."""
    assert out["rc"] == 0 and out["picked"] == picks and out["asymmetry"] == 0.0
    np.testing.assert_array_equal(out["order"][:picks], order[:picks])
    assert np.all(out["order"][picks:] == -1) and np.all(out["gains"][picks:] == 0) and np.all(out["pick_variances"][picks:] == 0)
    np.testing.assert_array_equal(out["pick_variances"][:picks], value[order[:picks]])
    np.testing.assert_array_equal(out["remaining"], value)
    want = 0.5 * np.log(np.asarray(1.0 + 4.0 * value[order[:picks]], dtype=np.longdouble))
    assert np.all(np.abs(out["gains"][:picks] - want) <= 2 * EPS)
    assert not np.any(np.isin(out["order"], np.asarray(excluded, dtype=np.int64)))


def test_a_graded_diagonal_at_the_caps(hip_lib):
    """C = 4096, P = diag(1 + pi(c) / 4096), pi(c) = (1001 c) mod 4096 (selection_helpers.graded), every precision 4: the argmax
    across all 16 slots, the four waves and the 64 lanes bit for bit, k = 256 -- alone, with the 100 leading candidates
    excluded (the next 256 are picked; the excluded keep their remaining variance), and under a min_gain between two gains."""
    pi, value, P, w, order = _graded()
    out = greedy_from_matrix(P, w, CAP_PICKS, lib_path=hip_lib)
    _check_graded(out, value, order, CAP_PICKS)
    assert np.all(np.diff(pi[out["order"]]) < 0) and pi[out["order"][0]] == CAP - 1
    excluded = np.zeros(CAP, dtype=np.int32)
    excluded[order[:100]] = 1
    rest = greedy_from_matrix(P, w, CAP_PICKS, excluded=excluded, lib_path=hip_lib)
    _check_graded(rest, value, order[100:], CAP_PICKS, excluded=order[:100])
    np.testing.assert_array_equal(rest["gains"][:CAP_PICKS - 100], out["gains"][100:])
    # min_gain between the gains of picks 9 and 10 (from 0): ten picks, the padding after them
    d = np.asarray(1.0 + 4.0 * value[order[:11]], dtype=np.longdouble)
    cut = float(0.25 * (np.log(d[9]) + np.log(d[10])))
    assert out["gains"][10] < cut < out["gains"][9]
    short = greedy_from_matrix(P, w, CAP_PICKS, min_gain=cut, lib_path=hip_lib)
    _check_graded(short, value, order, 10)
    np.testing.assert_array_equal(short["gains"][:10], out["gains"][:10])


def test_identity_at_the_caps(hip_lib):
    """P = I, every precision 4, C = 4096, k = 256: exact ties across every slot, wave and lane, broken to the lowest index; with
    the first 3900 candidates excluded the 196 others are picked in index order and the rule stops."""
    P, w = np.eye(CAP), np.full(CAP, 4.0)
    out = greedy_from_matrix(P, w, CAP_PICKS, lib_path=hip_lib)
    np.testing.assert_array_equal(out["order"], np.arange(CAP_PICKS))
    assert out["rc"] == 0 and out["picked"] == CAP_PICKS and out["asymmetry"] == 0.0
    np.testing.assert_array_equal(out["gains"], np.full(CAP_PICKS, out["gains"][0]))
    assert abs(out["gains"][0] - 0.5 * np.log(5.0)) <= 2 * EPS and np.all(out["pick_variances"] == 1.0) and np.all(out["remaining"] == 1.0)
    excluded = np.zeros(CAP, dtype=np.int32)
    excluded[:3900] = 1
    rest = greedy_from_matrix(P, w, CAP_PICKS, excluded=excluded, lib_path=hip_lib)
    assert rest["rc"] == 0 and rest["picked"] == CAP - 3900 == 196
    np.testing.assert_array_equal(rest["order"], np.concatenate([np.arange(3900, CAP), np.full(CAP_PICKS - 196, -1)]))
    np.testing.assert_array_equal(rest["gains"], np.concatenate([out["gains"][:196], np.zeros(CAP_PICKS - 196)]))
    np.testing.assert_array_equal(rest["pick_variances"], np.concatenate([np.ones(196), np.zeros(CAP_PICKS - 196)]))
    assert np.all(rest["remaining"] == 1.0)


def test_identity_and_equal_precisions_pick_in_index_order(hip_lib):
    for n in (5, 65, 257):
        k = min(n, 256)
        out = greedy_from_matrix(np.eye(n), np.full(n, 4.0), k, lib_path=hip_lib)   # (sqrt 4 is exact: d = 5 everywhere)
        np.testing.assert_array_equal(out["order"], np.arange(k))
        assert out["picked"] == k and out["asymmetry"] == 0.0
        np.testing.assert_array_equal(out["gains"], np.full(k, out["gains"][0]))
        assert abs(out["gains"][0] - 0.5 * np.log(5.0)) <= 2 * EPS and np.all(out["pick_variances"] == 1.0)


def test_a_duplicated_candidate(hip_lib):
    """Equal rows and columns: the lower index first, and the other's later gain is strictly smaller."""
    n = 40
    P, w = random_matrix(n, 7)
    P = 0.5 * (P + P.T)
    lo, hi = 9, 33
    P[hi, :], P[:, hi] = P[lo, :], P[:, lo]
    P[hi, hi] = P[lo, lo]
    P[lo, :] *= 50.0; P[:, lo] *= 50.0; P[hi, :] *= 50.0; P[:, hi] *= 50.0   # (the pair leads)
    w[hi] = w[lo]
    assert np.array_equal(P[lo], P[hi]) and np.array_equal(P[:, lo], P[:, hi]) and np.array_equal(P, P.T)
    out = greedy_from_matrix(P, w, n, lib_path=hip_lib)
    order = out["order"].tolist()
    assert order[0] == lo and hi in order and out["picked"] == n
    assert out["gains"][order.index(hi)] < out["gains"][0]
    ref = greedy_reference(P, w, n)
    np.testing.assert_array_equal(ref["order"][:1], [lo])


def test_a_zero_row_an_exclusion_and_the_min_gain_stop(hip_lib):
    n, k = 33, 33
    P, w = random_matrix(n, SEEDS[33])
    P[4, :], P[:, 4] = 0.0, 0.0
    excluded = np.zeros(n, dtype=np.int32)
    ref_free = bounded_reference(P, w, k)
    best = int(ref_free["order"][0])
    excluded[best] = 1
    ref = bounded_reference(P, w, k, excluded=excluded)
    out = greedy_from_matrix(P, w, k, excluded=excluded, lib_path=hip_lib)
    # d = 1 exactly at the zero row: the rule stops there, after every other candidate
    assert out["picked"] == ref["picked"] == n - 2 and 4 not in out["order"] and best not in out["order"]
    check_against_reference(out, ref, "zero row + exclusion")
    assert out["remaining"][4] == 0.0 and out["remaining"][best] > 0
    # min_gain between two of the reference's gains
    j = 5
    cut = 0.5 * (ref["gains"][j - 1] + ref["gains"][j])
    assert ref["gains"][j] < cut < ref["gains"][j - 1]
    ref_cut = bounded_reference(P, w, k, min_gain=cut, excluded=excluded)
    short = greedy_from_matrix(P, w, k, min_gain=cut, excluded=excluded, lib_path=hip_lib)
    assert short["picked"] == ref_cut["picked"] == j and np.all(short["order"][j:] == -1)
    check_against_reference(short, ref_cut, "min_gain stop")
    np.testing.assert_array_equal(short["order"][:j], out["order"][:j])
    np.testing.assert_array_equal(short["gains"][:j], out["gains"][:j])


def test_the_library_refuses_bad_arguments(hip_lib):
    P, w = random_matrix(4, 1)
    big = np.zeros((1, 1))
    cases = [(big, np.ones(4097), 1, "candidates must be 1..4096"), (P, w, 0, "k must be 1.."), (P, w, 5, "k must be 1.."),
             (np.eye(300), np.ones(300), 257, "k must be 1.."), (P, np.array([1.0, 0.0, 1.0, 1.0]), 2, "finite and positive"),
             (P, np.array([1.0, np.nan, 1.0, 1.0]), 2, "finite and positive")]
    for M, ww, k, words in cases:
        with pytest.raises(RuntimeError, match="score_select_greedy: .*" + words):
            greedy_from_matrix(M, ww, k, lib_path=hip_lib)
    with pytest.raises(RuntimeError, match="min_gain must be >= 0"):
        greedy_from_matrix(P, w, 2, min_gain=-1.0, lib_path=hip_lib)
    assert greedy_from_matrix(P, w, 2, lib_path=hip_lib)["picked"] == 2  # (the library goes on)


# ---- the call on a handle ----
# the lists of CASES by their graph's name, and the long list of graph b (650 candidates, k = 40: three workgroups of k_sel_cross
# a column, a third ownership slot in the factorisation) as "b650"
LISTS = {**{key: (key, candidates) for key in CASES}, **{f"{key}{LONG_CASES[key][0]}": (key, long_candidates) for key in LONG_CASES}}


def _list(name):
    """(graph, ids, count, k) of a list of LISTS."""
    key, get = LISTS[name]
    return (key, *get(key))


@functools.lru_cache(maxsize=None)
def _runs(name, hip_lib):
    """One handle per list: the range variances, then the selection at both base precisions (the first twice, and at width
    5).  Computed once and left unchanged."""
    key, ids, count, k = _list(name)
    tw = twin(key)
    out = {}
    with SelectionHandle(tw.ref.prob, hip_lib) as h:
        out["variances"] = h.range_variances(tw.ref.point, ids)
        for base in BASE_PRECISIONS:
            out[base] = h.select_ranges(tw.ref.point, ids, precisions(count, base), k, with_matrix=True)
        out["again"] = h.select_ranges(tw.ref.point, ids, precisions(count, BASE_PRECISIONS[0]), k, with_matrix=True)
        out["narrow"] = h.select_ranges(tw.ref.point, ids, precisions(count, BASE_PRECISIONS[0]), k, block_width=5, with_matrix=True)
        out["after"] = h.range_variances(tw.ref.point, ids)
    return out


@pytest.mark.parametrize("key", sorted(LISTS))
def test_columns_are_those_of_the_range_variances(hip_lib, key):
    runs = _runs(key, hip_lib)
    _, ids, count, k = _list(key)
    var = runs["variances"]
    assert var["rc"] == 0 and np.all(var["converged"])
    for name in (*BASE_PRECISIONS, "again"):
        sel = runs[name]
        assert sel["rc"] == 0 and sel["info"]["candidates"] == count and sel["info"]["excluded"] == 0 and sel["info"]["picked"] == k
        assert sel["info"]["solve"]["columns"] == count and sel["info"]["solve"]["batches"] == (count + 15) // 16
        for f in ("variances", "distances", "residuals", "iterations"):
            np.testing.assert_array_equal(sel[f], var[f], err_msg=f)
        np.testing.assert_array_equal(np.diag(sel["matrix"]), sel["variances"])
    for f in ("variances", "distances", "residuals", "iterations"):  # (and the selection leaves the other call as it was)
        np.testing.assert_array_equal(runs["after"][f], var[f], err_msg=f)


@pytest.mark.parametrize("key", sorted(LISTS))
def test_matrix_and_total_gain_against_the_dense_reference(hip_lib, key):
    runs = _runs(key, hip_lib)
    graph, ids, count, k = _list(key)
    tw = twin(graph)
    for base in BASE_PRECISIONS:
        sel = runs[base]
        P_ref, bound = matrix_bound(tw, ids, sel)
        err = np.abs(sel["matrix"] - P_ref)
        print(f"{key}: worst |P - G'Sigma G| / bound = {float(np.max(err / bound)):.3e}, asymmetry {sel['info']['asymmetry']:.3e}")
        assert np.all(err <= bound)
        assert sel["info"]["asymmetry"] == float(np.max(np.abs(sel["matrix"] - sel["matrix"].T)))
        w = precisions(count, base)
        ref = bounded_reference(sel["matrix"], w, k)
        want, slack = total_gain_bound(P_ref, bound, w, sel["order"])
        total = sel["info"]["total_gain"]
        slack += float(np.sum(ref["gain_bound"])) + (k + 1) * EPS * abs(want)
        print(f"{key}, precision {base}: total gain {total:.12f}, dense {want:.12f}, |difference| / bound {abs(total - want) / slack:.3e}")
        assert abs(total - want) <= slack
        assert total == sum(sel["gains"][:k].tolist())  # (the host adds them in the order of the picks)


@pytest.mark.parametrize("key", sorted(LISTS))
def test_order_and_gains_against_the_rule_on_the_calls_own_matrix(hip_lib, key):
    runs = _runs(key, hip_lib)
    _, ids, count, k = _list(key)
    for base in BASE_PRECISIONS:
        sel = runs[base]
        ref = bounded_reference(sel["matrix"], precisions(count, base), k)
        check_against_reference(sel, ref, f"{key}, precision {base}")
        assert np.all(np.diff(sel["gains"]) <= 1e-12 * sel["gains"][:-1])


@pytest.mark.parametrize("key", sorted(LISTS))
def test_widths_and_repeats_give_the_same_bits(hip_lib, key):
    runs = _runs(key, hip_lib)
    first = runs[BASE_PRECISIONS[0]]
    for other in ("again", "narrow"):
        np.testing.assert_array_equal(runs[other]["matrix"], first["matrix"], err_msg=other)
        _same_bits(first, runs[other])
    assert runs["narrow"]["info"]["solve"]["batches"] == (_list(key)[2] + 4) // 5


@pytest.mark.parametrize("key", sorted(LISTS))
def test_the_call_equals_the_selection_alone_on_its_matrix(hip_lib, key):
    """The handle's k_sel_sym and k_sel_greedy on its kept buffers against score_select_greedy on the returned matrix."""
    runs = _runs(key, hip_lib)
    _, ids, count, k = _list(key)
    for base in BASE_PRECISIONS:
        sel = runs[base]
        alone = greedy_from_matrix(sel["matrix"], precisions(count, base), k, lib_path=hip_lib)
        _same_bits(sel, alone)
        assert alone["picked"] == sel["info"]["picked"] and alone["asymmetry"] == sel["info"]["asymmetry"]


def test_unconverged_columns_exclude_their_candidates(hip_lib):
    """check_iteration_caps' pattern: under max_iters = max(steps) - 1 the call returns 1, the candidates beyond the cap are
    excluded and never picked, and the rest is the rule on the eligible set of the call's own matrix."""
    tw = twin("a")
    ids, count, k = candidates("a")
    w = precisions(count, BASE_PRECISIONS[0])
    steps = _runs("a", hip_lib)["variances"]["iterations"]
    cap = int(steps.max()) - 1
    with SelectionHandle(tw.ref.prob, hip_lib) as h:
        sel = h.select_ranges(tw.ref.point, ids, w, k, max_iters=cap, with_matrix=True)
    late = steps > cap
    print(f"a, cap {cap}: steps {steps.tolist()}, {int(np.count_nonzero(late))} beyond it")
    assert sel["rc"] == 1 and 0 < np.count_nonzero(late) < count
    np.testing.assert_array_equal(~sel["converged"], late)
    assert sel["info"]["excluded"] == int(np.count_nonzero(late)) == sel["info"]["solve"]["unconverged"]
    assert not np.any(np.isin(sel["order"], np.flatnonzero(late)))
    assert np.all(np.isfinite(sel["matrix"]))
    ref = bounded_reference(sel["matrix"], w, k, excluded=late.astype(np.int32))
    check_against_reference(sel, ref, f"a, cap {cap}")
    assert sel["info"]["picked"] == ref["picked"]


def test_the_library_refuses_bad_selections(hip_lib):
    tw = twin("a")
    ids, count, k = candidates("a")
    w = precisions(count, 4.0)
    with SelectionHandle(tw.ref.prob, hip_lib) as h:
        for kw, words in ((dict(k=0), "k must be 1.."), (dict(k=count + 1), "k must be 1.."), (dict(k=k, min_gain=-1.0), "min_gain"),
                          (dict(k=k, block_width=17), "block_width must be 1..16")):
            with pytest.raises(RuntimeError, match="score_refine_select_ranges: .*" + words):
                h.select_ranges(tw.ref.point, ids, w, **kw)
        bad = w.copy()
        bad[3] = 0.0
        with pytest.raises(RuntimeError, match="score_refine_select_ranges: .*finite and positive"):
            h.select_ranges(tw.ref.point, ids, bad, k)
        with pytest.raises(RuntimeError, match="score_refine_select_ranges: .*joins a variable to itself"):
            h.select_ranges(tw.ref.point, [(3, 3)], w[:1], 1)
        dup = np.concatenate([ids[:5], ids[:5]])   # (duplicate pairs are allowed)
        out = h.select_ranges(tw.ref.point, dup, np.full(10, 4.0), 10)
        assert out["rc"] == 0 and out["info"]["picked"] == 10 and sorted(out["order"].tolist()) == list(range(10))
        _same_bits(h.select_ranges(tw.ref.point, ids, w, k), _runs("a", hip_lib)[4.0])


def test_select_ranges_by_name(hip_lib):
    tw = twin("a")
    prob = tw.ref.prob
    ids, count, k = candidates("a")
    names = [str(nm) for nm in prob.a["pose_names"]] + [str(nm) for nm in prob.a["landmark_names"]]
    pairs = [(names[a], names[b]) for a, b in ids]
    w = precisions(count, 4.0)
    host, _ = select_ranges(tw.fg, tw.results, pairs, k, precision=w, engine="python")
    dev, info = select_ranges(tw.fg, tw.results, pairs, k, precision=w, lib_path=hip_lib)
    np.testing.assert_array_equal(dev.order, host.order)
    assert dev.pairs == host.pairs and info["engine"] == "device" and dev.excluded.size == 0
    assert np.all(np.isnan(dev.remaining_variance[dev.order])) and np.all(np.isfinite(np.delete(dev.remaining_variance, dev.order)))
    _same_bits({"order": dev.order, "gains": dev.gains}, {kk: _runs("a", hip_lib)[4.0][kk][:k] for kk in ("order", "gains")},
               keys=("order", "gains"))
