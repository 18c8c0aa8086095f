"""Greedy selection of candidate loop closures on the device (score_select_block_greedy, score_refine_select_relative_poses,
csrc/score_select_poses.hpp): the kernels alone on random matrices against the rule in np.longdouble on the same matrix, under
the bounds derived in tests/selection_poses_helpers.py, the exact ties and stops, and the call on a handle -- its relative
outputs bit for bit those of score_refine_relative_covariances, its matrix under the bound of the relative covariances, its
order held to the rule on its OWN matrix (never to the dense one).  The same checks reach every ownership slot of
k_selp_greedy and the caps in both dimensions (selection_poses_helpers.SLOT_SHAPES, the exact graded diagonal and the identity
at the caps), a list of 320 candidates on graph b, and the buffers a handle keeps between calls of other sizes."""
import functools

import numpy as np
import pytest

from marginals_helpers import EPS
from selection_helpers import candidates as range_candidates, precisions as range_precisions
from selection_poses_helpers import (BASE_PRECISIONS, CAPS, CASES, LONG_CASES, SHAPES, SLOT_SHAPES, bounded_block_reference, candidates,
                                     check_against_reference, dof, graded_blocks, long_candidates, matrix_bound, precisions,
                                     random_block_matrix, slot_block_matrix, slot_block_reference, total_gain_bound, twin)
from score_amd.selection_poses import (PoseSelectionHandle, block_greedy_from_matrix, block_greedy_reference, column_precisions,
                                       select_loop_closures)

pytestmark = pytest.mark.gpu

VALUES = ("order", "gains", "pick_covariances", "remaining")
RELATIVE = ("rotations", "translations", "covariances", "residuals", "iterations")


def _same_bits(a, b, keys=VALUES):
    for key in keys:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# ---- the kernels alone ----
@pytest.mark.parametrize("dim,n,k", SHAPES)
def test_kernels_against_the_reference(hip_lib, dim, n, k):
    P, kappa, tau = random_block_matrix(n, dim)
    ref = bounded_block_reference(P, kappa, tau, dim, k)
    out = block_greedy_from_matrix(P, kappa, tau, dim, k, lib_path=hip_lib)
    assert out["rc"] == 0 and out["picked"] == ref["picked"] == k
    check_against_reference(out, ref, f"dim {dim}, C = {n}, k = {k}")
    assert out["asymmetry"] == float(np.max(np.abs(P - P.T)))  # (a subtraction of two doubles and a max: exact)
    np.testing.assert_array_equal(out["remaining"], np.swapaxes(out["remaining"], 1, 2))
    again = block_greedy_from_matrix(P, kappa, tau, dim, k, lib_path=hip_lib)
    _same_bits(out, again)
    assert again["asymmetry"] == out["asymmetry"]


@pytest.mark.parametrize("dim,n,k", SLOT_SHAPES)
def test_kernels_against_the_reference_at_every_slot_and_cap(hip_lib, dim, n, k):
    """The checks above where a lane owns up to 3 (3-D) or 6 (2-D) candidates (selection_poses_helpers.SLOT_SHAPES), up to the
    caps: the host's share is the long-double reference (10 s at the caps; computed once)."""
    P, kappa, tau = slot_block_matrix(n, dim)
    ref = slot_block_reference(dim, n, k)
    out = block_greedy_from_matrix(P, kappa, tau, dim, k, lib_path=hip_lib)
    assert out["rc"] == 0 and out["picked"] == ref["picked"] == k
    check_against_reference(out, ref, f"dim {dim}, C = {n}, k = {k}")
    assert out["asymmetry"] == float(np.max(np.abs(P - P.T)))  # (a subtraction of two doubles and a max: exact)
    np.testing.assert_array_equal(out["remaining"], np.swapaxes(out["remaining"], 1, 2))
    again = block_greedy_from_matrix(P, kappa, tau, dim, k, lib_path=hip_lib)
    _same_bits(out, again)
    assert again["asymmetry"] == out["asymmetry"]


def _check_graded(out, value, order, picks, dp, excluded=()):
    """Every column weighs 4 (kappa = 4, tau = 2: sqrt 4 is exact), the diagonal 1 + pi(c) / 4096 is a multiple of 2^-12 below 2
    and everything else an exact zero: every block is (5 + pi(c) / 1024) I exactly, every l off the pivot's own coordinate an
    exact zero, so the pick covariance is the diagonal entry times I and `remaining` the diagonal blocks whatever was picked.
    The gain is half a sum of dp device logarithms of an exact pivot: the (dp + 1) eps relative margin that
    tests/test_selection_poses_host.py derives for two sides of this rule."""
    assert out["rc"] == 0 and out["picked"] == picks and out["asymmetry"] == 0.0
    np.testing.assert_array_equal(out["order"][:picks], order[:picks])
    assert np.all(out["order"][picks:] == -1) and np.all(out["gains"][picks:] == 0) and np.all(out["pick_covariances"][picks:] == 0)
    eye = np.eye(dp)
    np.testing.assert_array_equal(out["pick_covariances"][:picks], value[order[:picks], None, None] * eye)
    np.testing.assert_array_equal(out["remaining"], value[:, None, None] * eye)
    want = 0.5 * dp * np.log(np.asarray(1.0 + 4.0 * value[order[:picks]], dtype=np.longdouble))
    assert np.all(np.abs(out["gains"][:picks] - want) <= (dp + 1) * EPS * want)
    assert not np.any(np.isin(out["order"], np.asarray(excluded, dtype=np.int64)))


@pytest.mark.parametrize("dim", [2, 3])
def test_a_graded_diagonal_at_the_caps(hip_lib, dim):
    """C = 1365 | 682 and k = 85 | 42, P = 1 + pi(c) / 4096 on all dp coordinates of candidate c, pi(c) = (1001 c) mod 2048
    (selection_poses_helpers.graded_blocks): the argmax across every ownership slot, the four waves and the 64 lanes bit for
    bit -- alone, with the 100 leading candidates excluded (the next k are picked; the excluded keep their remaining
    covariance), and under a min_gain between two gains."""
    dp = dof(dim)
    n, k = CAPS[dim]
    pi, P = graded_blocks(n, dim)
    value = 1.0 + pi / 4096.0
    order = np.argsort(-pi, kind="stable")
    kappa, tau = np.full(n, 4.0), np.full(n, 2.0)
    np.testing.assert_array_equal(column_precisions(dim, kappa, tau, n), np.full(n * dp, 4.0))
    out = block_greedy_from_matrix(P, kappa, tau, dim, k, lib_path=hip_lib)
    _check_graded(out, value, order, k, dp)
    excluded = np.zeros(n, dtype=np.int32)
    excluded[order[:100]] = 1
    rest = block_greedy_from_matrix(P, kappa, tau, dim, k, excluded=excluded, lib_path=hip_lib)
    _check_graded(rest, value, order[100:], k, dp, excluded=order[:100])
    # min_gain between the gains of picks 9 and 10 (from 0): ten picks, the padding after them
    d = np.asarray(1.0 + 4.0 * value[order[:11]], dtype=np.longdouble)
    cut = float(0.25 * dp * (np.log(d[9]) + np.log(d[10])))
    assert out["gains"][10] < cut < out["gains"][9]
    short = block_greedy_from_matrix(P, kappa, tau, dim, k, min_gain=cut, lib_path=hip_lib)
    _check_graded(short, value, order, 10, dp)
    np.testing.assert_array_equal(short["gains"][:10], out["gains"][:10])


@pytest.mark.parametrize("dim", [2, 3])
def test_identity_at_the_caps(hip_lib, dim):
    """P = I, every column's weight 4, C and k at their caps: exact ties across every slot, wave and lane, broken to the lowest
    index; with all but the last 40 candidates excluded those 40 are picked in index order and the rule stops short of k."""
    dp = dof(dim)
    n, k = CAPS[dim]
    P, kappa, tau = np.eye(n * dp), np.full(n, 4.0), np.full(n, 2.0)
    out = block_greedy_from_matrix(P, kappa, tau, dim, k, lib_path=hip_lib)
    np.testing.assert_array_equal(out["order"], np.arange(k))
    assert out["rc"] == 0 and out["picked"] == k and out["asymmetry"] == 0.0
    np.testing.assert_array_equal(out["gains"], np.full(k, out["gains"][0]))
    assert abs(out["gains"][0] - 0.5 * dp * np.log(5.0)) <= (dp + 1) * EPS * 0.5 * dp * np.log(5.0)
    np.testing.assert_array_equal(out["pick_covariances"], np.broadcast_to(np.eye(dp), (k, dp, dp)))
    np.testing.assert_array_equal(out["remaining"], np.broadcast_to(np.eye(dp), (n, dp, dp)))
    left = 40
    assert left < k
    excluded = np.zeros(n, dtype=np.int32)
    excluded[:n - left] = 1
    rest = block_greedy_from_matrix(P, kappa, tau, dim, k, excluded=excluded, lib_path=hip_lib)
    assert rest["rc"] == 0 and rest["picked"] == left
    np.testing.assert_array_equal(rest["order"], np.concatenate([np.arange(n - left, n), np.full(k - left, -1)]))
    np.testing.assert_array_equal(rest["gains"], np.concatenate([out["gains"][:left], np.zeros(k - left)]))
    np.testing.assert_array_equal(rest["pick_covariances"][:left], np.broadcast_to(np.eye(dp), (left, dp, dp)))
    assert np.all(rest["pick_covariances"][left:] == 0)
    np.testing.assert_array_equal(rest["remaining"], np.broadcast_to(np.eye(dp), (n, dp, dp)))


@pytest.mark.parametrize("dim", [2, 3])
def test_identity_and_equal_precisions_pick_in_index_order(hip_lib, dim):
    dp = dof(dim)
    for n in (5, 65, 257):
        k = min(n, 256 // dp)
        # kappa = 4, tau = 2: every column weighs 4, sqrt 4 is exact: every block is 5 I
        out = block_greedy_from_matrix(np.eye(n * dp), np.full(n, 4.0), np.full(n, 2.0), dim, k, lib_path=hip_lib)
        np.testing.assert_array_equal(out["order"], np.arange(k))
        assert out["picked"] == k and out["asymmetry"] == 0.0
        np.testing.assert_array_equal(out["gains"], np.full(k, out["gains"][0]))
        assert abs(out["gains"][0] - 0.5 * dp * np.log(5.0)) <= (dp + 1) * EPS * 0.5 * dp * np.log(5.0)
        np.testing.assert_array_equal(out["pick_covariances"], np.broadcast_to(np.eye(dp), (k, dp, dp)))
        np.testing.assert_array_equal(out["remaining"], np.broadcast_to(np.eye(dp), (n, dp, dp)))


@pytest.mark.parametrize("dim", [2, 3])
def test_a_duplicated_candidate(hip_lib, dim):
    """Equal block rows and columns: the lower index first, and the other's later gain is strictly smaller."""
    dp, n = dof(dim), 20
    P, kappa, tau = (a.copy() for a in random_block_matrix(n, dim))
    P = 0.5 * (P + P.T)
    lo, hi = 4, 13
    rl, rh = slice(lo * dp, (lo + 1) * dp), slice(hi * dp, (hi + 1) * dp)
    P[rl, :] *= 50.0; P[:, rl] *= 50.0   # (the pair leads)
    P[rh, :], P[:, rh] = P[rl, :], P[:, rl]
    P[rh, rh] = P[rl, rl]
    P[rl, rh] = P[rh, rl] = P[rl, rl]
    kappa[hi], tau[hi] = kappa[lo], tau[lo]
    assert np.array_equal(P[rl], P[rh]) and np.array_equal(P[:, rl], P[:, rh]) and np.array_equal(P, P.T)
    out = block_greedy_from_matrix(P, kappa, tau, dim, n, lib_path=hip_lib)
    order = out["order"].tolist()
    assert order[0] == lo and hi in order and out["picked"] == n
    assert out["gains"][order.index(hi)] < out["gains"][0]
    ref = block_greedy_reference(P, column_precisions(dim, kappa, tau, n), dp, n)
    np.testing.assert_array_equal(ref["order"][:1], [lo])


def test_a_zero_block_an_exclusion_and_the_min_gain_stop(hip_lib):
    dim, n, k = 2, 22, 22
    dp = dof(dim)
    P, kappa, tau = (a.copy() for a in random_block_matrix(n, dim))
    P[4 * dp:5 * dp, :], P[:, 4 * dp:5 * dp] = 0.0, 0.0
    excluded = np.zeros(n, dtype=np.int32)
    ref_free = bounded_block_reference(P, kappa, tau, dim, k)
    best = int(ref_free["order"][0])
    excluded[best] = 1
    ref = bounded_block_reference(P, kappa, tau, dim, k, excluded=excluded)
    out = block_greedy_from_matrix(P, kappa, tau, dim, k, excluded=excluded, lib_path=hip_lib)
    # B = I exactly at the zero block: its gain is 0 and the rule stops there, after every other candidate
    assert out["picked"] == ref["picked"] == n - 2 and 4 not in out["order"] and best not in out["order"]
    check_against_reference(out, ref, "zero block + exclusion")
    assert np.all(out["remaining"][4] == 0.0) and np.all(np.diag(out["remaining"][best]) > 0)
    # min_gain between two of the reference's gains
    j = 5
    cut = 0.5 * (ref["gains"][j - 1] + ref["gains"][j])
    assert ref["gains"][j] < cut < ref["gains"][j - 1]
    ref_cut = bounded_block_reference(P, kappa, tau, dim, k, min_gain=cut, excluded=excluded)
    short = block_greedy_from_matrix(P, kappa, tau, dim, k, min_gain=cut, excluded=excluded, lib_path=hip_lib)
    assert short["picked"] == ref_cut["picked"] == j and np.all(short["order"][j:] == -1)
    check_against_reference(short, ref_cut, "min_gain stop")
    np.testing.assert_array_equal(short["order"][:j], out["order"][:j])
    np.testing.assert_array_equal(short["gains"][:j], out["gains"][:j])


def test_the_library_refuses_bad_arguments(hip_lib):
    P, kappa, tau = random_block_matrix(2, 2)
    one = np.ones(2)
    cases = [(np.zeros((1, 1)), np.ones(1366), np.ones(1366), 2, 1, "candidates must be 1..1365"),
             (np.zeros((1, 1)), np.ones(683), np.ones(683), 3, 1, "candidates must be 1..682"),
             (P, kappa, tau, 2, 0, "k must be 1.."), (P, kappa, tau, 2, 3, "k must be 1.."),
             (np.eye(300), np.ones(100), np.ones(100), 2, 86, "k must be 1.."), (np.eye(300), np.ones(50), np.ones(50), 3, 43, "k must be 1.."),
             (P, kappa, tau, 4, 1, "dim must be 2 or 3"),
             (P, np.array([1.0, 0.0]), one, 2, 2, "finite and positive"), (P, one, np.array([np.nan, 1.0]), 2, 2, "finite and positive"),
             (P, one, np.array([1.0, np.inf]), 2, 2, "finite and positive"), (P, np.array([-1.0, 1.0]), one, 2, 2, "finite and positive")]
    for M, ka, ta, dim, k, words in cases:
        with pytest.raises(RuntimeError, match="score_select_block_greedy: .*" + words):
            block_greedy_from_matrix(M, ka, ta, dim, k, lib_path=hip_lib)
    with pytest.raises(RuntimeError, match="min_gain must be >= 0"):
        block_greedy_from_matrix(P, kappa, tau, 2, 2, min_gain=-1.0, lib_path=hip_lib)
    assert block_greedy_from_matrix(P, kappa, tau, 2, 2, lib_path=hip_lib)["picked"] == 2  # (the library goes on)


# ---- the call on a handle ----
# the lists of CASES by their graph's name, and the long list of graph b (320 candidates = 960 columns, k = 12: two workgroups of
# k_selp_cross a column slot, 60 solved blocks, a second ownership slot in the factorisation) as "b320"
LISTS = {**{key: (key, candidates) for key in CASES}, **{f"{key}{LONG_CASES[key][0]}": (key, long_candidates) for key in LONG_CASES}}


def _list(name):
    """(graph, ids, count, k) of a list of LISTS."""
    key, get = LISTS[name]
    return (key, *get(key))


@functools.lru_cache(maxsize=None)
def _runs(name, hip_lib):
    """One handle per list: the relative covariances, then the selection at both base precisions (the first twice, and at
    width 5).  Computed once and left unchanged."""
    key, ids, count, k = _list(name)
    tw = twin(key)
    out = {}
    with PoseSelectionHandle(tw.ref.prob, hip_lib) as h:
        out["relative"] = h.relative_covariances(tw.ref.point, ids)
        for base in BASE_PRECISIONS:
            out[base] = h.select_relative_poses(tw.ref.point, ids, *precisions(count, base), k, with_matrix=True)
        first = precisions(count, BASE_PRECISIONS[0])
        out["again"] = h.select_relative_poses(tw.ref.point, ids, *first, k, with_matrix=True)
        out["narrow"] = h.select_relative_poses(tw.ref.point, ids, *first, k, block_width=5, with_matrix=True)
        out["narrow relative"] = h.relative_covariances(tw.ref.point, ids, block_width=5)
        out["after"] = h.relative_covariances(tw.ref.point, ids)
    return out


@pytest.mark.parametrize("key", sorted(LISTS))
def test_relative_outputs_are_those_of_the_relative_covariances(hip_lib, key):
    """(i) and (ii): the relative outputs bit for bit, that call unchanged afterwards, every diagonal block of the matrix."""
    runs = _runs(key, hip_lib)
    graph, ids, count, k = _list(key)
    dp = dof(twin(graph).fg.dimension)
    rel = runs["relative"]
    assert rel["rc"] == 0 and np.all(rel["converged"])
    for name in (*BASE_PRECISIONS, "again"):
        sel = runs[name]
        assert sel["rc"] == 0 and sel["info"]["candidates"] == count and sel["info"]["excluded"] == 0 and sel["info"]["picked"] == k
        assert sel["info"]["solve"]["columns"] == count * dp and sel["info"]["solve"]["batches"] == (count * dp + 15) // 16
        for f in RELATIVE:
            np.testing.assert_array_equal(sel[f], rel[f], err_msg=f)
        for c in range(count):
            np.testing.assert_array_equal(sel["matrix"][c * dp:(c + 1) * dp, c * dp:(c + 1) * dp], sel["covariances"][c], err_msg=f"block {c}")
    for f in RELATIVE:
        np.testing.assert_array_equal(runs["narrow"][f], runs["narrow relative"][f], err_msg=f)
        np.testing.assert_array_equal(runs["after"][f], rel[f], err_msg=f)  # (and the selection leaves the other call as it was)


@pytest.mark.parametrize("key", sorted(LISTS))
def test_matrix_and_total_gain_against_the_dense_reference(hip_lib, key):
    """(iii)"""
    runs = _runs(key, hip_lib)
    graph, ids, count, k = _list(key)
    tw = twin(graph)
    dim = tw.fg.dimension
    dp = dof(dim)
    for base in BASE_PRECISIONS:
        sel = runs[base]
        P_ref, bound = matrix_bound(tw, ids, sel)
        err = np.abs(sel["matrix"] - P_ref)
        print(f"{key}: worst |P - G Sigma G'| / bound = {float(np.max(err / bound)):.3e}, asymmetry {sel['info']['asymmetry']:.3e}")
        assert np.all(err <= bound)
        assert sel["info"]["asymmetry"] == float(np.max(np.abs(sel["matrix"] - sel["matrix"].T)))
        kappa, tau = precisions(count, base)
        ref = bounded_block_reference(sel["matrix"], kappa, tau, dim, k)
        want, slack = total_gain_bound(P_ref, bound, column_precisions(dim, kappa, tau, count), dp, sel["order"])
        total = sel["info"]["total_gain"]
        slack += float(np.sum(ref["gain_bound"])) + (k + 1) * EPS * abs(want)
        print(f"{key}, base {base}: total gain {total:.12f}, dense {want:.12f}, |difference| / bound {abs(total - want) / slack:.3e}")
        assert abs(total - want) <= slack
        assert total == sum(sel["gains"][:k].tolist())  # (the host adds them in the order of the picks)


@pytest.mark.parametrize("key", sorted(LISTS))
def test_order_and_values_against_the_rule_on_the_calls_own_matrix(hip_lib, key):
    """(iv)"""
    runs = _runs(key, hip_lib)
    graph, ids, count, k = _list(key)
    dim = twin(graph).fg.dimension
    for base in BASE_PRECISIONS:
        sel = runs[base]
        ref = bounded_block_reference(sel["matrix"], *precisions(count, base), dim, k)
        check_against_reference(sel, ref, f"{key}, base {base}")
        assert np.all(np.diff(sel["gains"]) <= 1e-12 * sel["gains"][:-1])


@pytest.mark.parametrize("key", sorted(LISTS))
def test_widths_and_repeats_give_the_same_bits(hip_lib, key):
    """(v)"""
    runs = _runs(key, hip_lib)
    first = runs[BASE_PRECISIONS[0]]
    graph, _, count, _ = _list(key)
    dp = dof(twin(graph).fg.dimension)
    for other in ("again", "narrow"):
        np.testing.assert_array_equal(runs[other]["matrix"], first["matrix"], err_msg=other)
        _same_bits(first, runs[other])
    assert runs["narrow"]["info"]["solve"]["batches"] == (count * dp + 4) // 5


@pytest.mark.parametrize("key", sorted(LISTS))
def test_the_call_equals_the_selection_alone_on_its_matrix(hip_lib, key):
    """The handle's k_sel_sym and k_selp_greedy on its kept buffers against score_select_block_greedy on the returned matrix."""
    runs = _runs(key, hip_lib)
    graph, _, count, k = _list(key)
    dim = twin(graph).fg.dimension
    for base in BASE_PRECISIONS:
        sel = runs[base]
        alone = block_greedy_from_matrix(sel["matrix"], *precisions(count, base), dim, k, lib_path=hip_lib)
        _same_bits(sel, alone)
        assert alone["picked"] == sel["info"]["picked"] and alone["asymmetry"] == sel["info"]["asymmetry"]


def test_the_kept_buffers_between_calls_of_other_sizes(hip_lib):
    """SelWork::reserve and SelpWork::reserve on ONE handle of graph a: ranges (C = 37, k = 12), relative poses (C = 23, k = 8:
    69 columns, P grows and L with it), ranges (C = 20, k = 20: L indexed at a stride below the room), the first call again,
    ranges with every pair three times over two directions (C = 60, k = 30: 1800 entries of L against the 1656 kept, so L grows
    at the room of 69 and is indexed at the stride 60) and the relative poses again.  Every call gives the bits of the same
    call on a fresh handle; the fourth gives those of the first."""
    tw = twin("a")
    r_ids, r_count, r_k = range_candidates("a")
    p_ids, p_count, p_k = candidates("a")
    assert (r_count, r_k, p_count, p_k) == (37, 12, 23, 8)
    many = np.concatenate([r_ids[:20], r_ids[:20][:, ::-1], r_ids[:20]])
    calls = [("ranges", r_ids, range_precisions(37, 4.0), 12), ("poses", p_ids, precisions(23, 4.0), 8),
             ("ranges", r_ids[:20], range_precisions(20, 4.0), 20), ("ranges", r_ids, range_precisions(37, 4.0), 12),
             ("ranges", many, range_precisions(60, 4.0), 30), ("poses", p_ids, precisions(23, 4.0), 8)]

    def call(h, kind, ids, w, k):
        if kind == "ranges":
            return h.select_ranges(tw.ref.point, ids, w, k, with_matrix=True)
        return h.select_relative_poses(tw.ref.point, ids, *w, k, with_matrix=True)

    with PoseSelectionHandle(tw.ref.prob, hip_lib) as h:
        kept = [call(h, *c) for c in calls]
    for i, (c, out) in enumerate(zip(calls, kept)):
        with PoseSelectionHandle(tw.ref.prob, hip_lib) as h:
            fresh = call(h, *c)
        values = ("order", "gains", "remaining", "matrix", "residuals", "iterations", "rc") + (
            ("pick_variances", "variances", "distances") if c[0] == "ranges" else ("pick_covariances", "covariances", "rotations", "translations"))
        _same_bits(out, fresh, keys=values)
        for f in ("candidates", "picked", "excluded", "total_gain", "asymmetry"):
            assert out["info"][f] == fresh["info"][f], (i, f)
        assert out["rc"] == 0 and out["info"]["picked"] == c[3], i
    _same_bits(kept[3], kept[0], keys=("order", "gains", "pick_variances", "remaining", "matrix", "variances"))
    _same_bits(kept[5], kept[1], keys=VALUES + ("matrix", "covariances"))


@pytest.mark.parametrize("key", ["a", "d"])
def test_unconverged_columns_exclude_their_candidates(hip_lib, key):
    """(vi): under max_iters = max(steps) - 1 the call returns 1, every candidate with a late column is excluded and never
    picked, and the rest is the rule on the eligible set of the call's own matrix."""
    tw = twin(key)
    ids, count, k = candidates(key)
    dim = tw.fg.dimension
    kappa, tau = precisions(count, BASE_PRECISIONS[0])
    steps = _runs(key, hip_lib)["relative"]["iterations"]
    cap = int(steps.max()) - 1
    with PoseSelectionHandle(tw.ref.prob, hip_lib) as h:
        sel = h.select_relative_poses(tw.ref.point, ids, kappa, tau, k, max_iters=cap, with_matrix=True)
    late = steps > cap                      # (C x dp)
    out_of = np.any(late, axis=1)
    print(f"{key}, cap {cap}: {int(np.count_nonzero(late))} late columns in {int(np.count_nonzero(out_of))} of {count} candidates")
    assert sel["rc"] == 1 and 0 < np.count_nonzero(out_of) < count
    np.testing.assert_array_equal(~sel["converged"], late)
    assert sel["info"]["excluded"] == int(np.count_nonzero(out_of)) and sel["info"]["solve"]["unconverged"] == int(np.count_nonzero(late))
    assert not np.any(np.isin(sel["order"], np.flatnonzero(out_of)))
    assert np.all(np.isfinite(sel["matrix"]))
    ref = bounded_block_reference(sel["matrix"], kappa, tau, dim, k, excluded=out_of.astype(np.int32))
    check_against_reference(sel, ref, f"{key}, cap {cap}")
    assert sel["info"]["picked"] == ref["picked"]


def test_the_library_refuses_bad_selections(hip_lib):
    tw = twin("a")
    ids, count, k = candidates("a")
    kappa, tau = precisions(count, 4.0)
    with PoseSelectionHandle(tw.ref.prob, hip_lib) as h:
        for kw, words in ((dict(k=0), "k must be 1.."), (dict(k=count + 1), "k must be 1.."), (dict(k=k, min_gain=-1.0), "min_gain must be >= 0"),
                          (dict(k=k, block_width=17), "block_width must be 1..16")):
            with pytest.raises(RuntimeError, match="score_refine_select_relative_poses: .*" + words):
                h.select_relative_poses(tw.ref.point, ids, kappa, tau, **kw)
        for which in (0, 1):
            bad = [kappa.copy(), tau.copy()]
            bad[which][3] = 0.0
            with pytest.raises(RuntimeError, match="score_refine_select_relative_poses: .*finite and positive"):
                h.select_relative_poses(tw.ref.point, ids, *bad, k)
        with pytest.raises(RuntimeError, match="score_refine_select_relative_poses: .*joins a pose to itself"):
            h.select_relative_poses(tw.ref.point, [(3, 3)], kappa[:1], tau[:1], 1)
        dup = np.concatenate([ids[:5], ids[:5]])   # (duplicate pairs are allowed)
        out = h.select_relative_poses(tw.ref.point, dup, np.full(10, 4.0), np.full(10, 10.0), 10)
        assert out["rc"] == 0 and out["info"]["picked"] == 10 and sorted(out["order"].tolist()) == list(range(10))
        _same_bits(h.select_relative_poses(tw.ref.point, ids, kappa, tau, k), _runs("a", hip_lib)[4.0])   # (the library goes on)


@pytest.mark.parametrize("key", ["a", "d"])
def test_select_loop_closures_by_name(hip_lib, key):
    """(vii)"""
    tw = twin(key)
    prob = tw.ref.prob
    ids, count, k = candidates(key)
    names = [str(nm) for nm in prob.a["pose_names"]]
    pairs = [(names[a], names[b]) for a, b in ids]
    kappa, tau = precisions(count, 4.0)
    kw = dict(translation_precision=kappa, rotation_precision=tau)
    host, _ = select_loop_closures(tw.fg, tw.results, pairs, k, engine="python", **kw)
    dev, info = select_loop_closures(tw.fg, tw.results, pairs, k, lib_path=hip_lib, **kw)
    np.testing.assert_array_equal(dev.order, host.order)
    assert dev.pairs == host.pairs and info["engine"] == "device" and dev.excluded.size == 0
    left = np.setdiff1d(np.arange(count), dev.order)
    assert np.all(np.isnan(dev.remaining_covariance[dev.order])) and np.all(np.isfinite(dev.remaining_covariance[left]))
    assert np.all(np.isnan(dev.remaining_gain[dev.order])) and np.all(dev.remaining_gain[left] <= dev.gains[-1] * (1 + 1e-12))
    ran = _runs(key, hip_lib)[4.0]
    _same_bits({"order": dev.order, "gains": dev.gains}, {kk: ran[kk][:k] for kk in ("order", "gains")}, keys=("order", "gains"))
    np.testing.assert_array_equal(dev.covariance, 0.5 * (ran["covariances"] + np.swapaxes(ran["covariances"], 1, 2)))
