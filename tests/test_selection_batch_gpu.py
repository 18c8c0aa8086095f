"""Batched greedy selection of candidate ranges on the device (score_refine_batch_select_ranges,
csrc/score_select_batch.hpp).

Every member of every group is judged as tests/test_selection_gpu.py judges a single graph: its columns bit for bit those of
the group's range variances, its matrix under ``matrix_bound`` against its own dense reference, its order held to the rule on
its OWN returned matrix (near-ties are in the data: never to the dense one), and equal bits with ``score_select_greedy`` on
that matrix, with the member alone in a group, under another width, in another member order and on a second call.  No
tolerance is chosen here: every bound is the derived one of tests/selection_helpers.py and tests/leverage_helpers.py.

The group A..E (tests/selection_batch_helpers.py) lists [37, 0, 9, 260, 1] candidates with k = [12, 0, 9, 32, 1]; the group
(3D0, 3D1) lists [20, 7] with k = [8, 7]; the group "slots", (D, B, C, A), lists [600, 37, 0, 513] with k = [40, 12, 0, 3]: unequal
members on either side of the ownership slots of the factorisation (a lane owns the candidates t + 256 m), every one of them held
to the reference (its precondition is asserted on the CPU).  Everything runs on one handle per group, computed once."""
import ctypes as C
import functools

import numpy as np
import pytest

from marginals_helpers import EPS
from refine_batch_helpers import group
from score_amd.bindings import SELECT_BATCH, ScoreSelectBatchInfo, bind
from score_amd.refine_batch import RefineBatchHandle, _problem_of, refine_estimate_batch
from score_amd.refine_robust import _point_arrays
from score_amd.selection import Selection, greedy_from_matrix
from score_amd.selection_batch import select_ranges_batch
from selection_batch_helpers import (BASE_PRECISIONS, COUNTS_2D, COUNTS_3D, COUNTS_SLOTS, KEYS_2D, KEYS_3D, KEYS_SLOTS, KS_2D, KS_3D, KS_SLOTS,
                                     PRECONDITION, candidates, member_twin, names_of, precisions)
from selection_helpers import bounded_reference, check_against_reference, matrix_bound, total_gain_bound

pytestmark = pytest.mark.gpu

VALUES = ("order", "gains", "pick_variances", "remaining")
COLUMNS = ("variances", "distances", "residuals", "iterations", "converged")
EVERYTHING = VALUES + COLUMNS + ("matrix", "picked", "total_gain", "rc")
SOLVE = ("columns", "passes", "pcg_iters", "unconverged", "max_residual")
GROUPS = {"2d": (KEYS_2D, COUNTS_2D, KS_2D), "3d": (KEYS_3D, COUNTS_3D, KS_3D), "slots": (KEYS_SLOTS, COUNTS_SLOTS, KS_SLOTS)}
CAPPED = ("2d", "3d")   # the groups that also run under an iteration cap


def _same_bits(a, b, label, keys=EVERYTHING):
    for key in keys:
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{label}: {key}")


def _handle(keys, hip_lib):
    return RefineBatchHandle([member_twin(k).ref.prob for k in keys], hip_lib)


def _points(keys):
    return [member_twin(k).ref.point for k in keys]


def _ids(keys, counts):
    return [candidates(k, c) for k, c in zip(keys, counts)]


def _weights(counts, base):
    return [precisions(c, base) if c else None for c in counts]


@functools.lru_cache(maxsize=None)
def runs_of(name, hip_lib):
    """The calls on a group, on ONE handle, shared by the tests below and left unchanged: the range variances before and after
    at widths 16 and 5, the selection at both base precisions, a repeat, width 5, the iteration cap and (2-D) the min_gain cut."""
    keys, counts, ks = GROUPS[name]
    ids, pts = _ids(keys, counts), _points(keys)
    w4 = _weights(counts, BASE_PRECISIONS[0])
    out = {}
    with _handle(keys, hip_lib) as h:
        out["rv"] = {w: h.range_variances(pts, ids, block_width=w) for w in (16, 5)}
        for base in BASE_PRECISIONS:
            out[base] = h.select_ranges(pts, ids, _weights(counts, base), ks, with_matrix=True)
        out["again"] = h.select_ranges(pts, ids, w4, ks, with_matrix=True)
        out["narrow"] = h.select_ranges(pts, ids, w4, ks, block_width=5, with_matrix=True)
        out["rv_after"] = {w: h.range_variances(pts, ids, block_width=w) for w in (16, 5)}
        if name in CAPPED:
            steps = np.concatenate([m["iterations"] for m in out["rv"][16][1]])
            out["cap"] = int(steps.max()) - 1
            out["capped"] = h.select_ranges(pts, ids, w4, ks, max_iters=out["cap"], with_matrix=True)
        if name == "2d":
            gains = out[BASE_PRECISIONS[0]][1][KEYS_2D.index("C")]["gains"]
            out["cut"] = 0.5 * (gains[4] + gains[5])
            out["short"] = h.select_ranges(pts, ids, w4, ks, min_gain=out["cut"], with_matrix=True)
        out["last"] = h.select_ranges(pts, ids, w4, ks, with_matrix=True)
    return out


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_columns_are_those_of_the_group_range_variances(hip_lib, name):
    """Contract 1: columns and info.solve equal h.range_variances before and after, bit for bit, at width 16 and at width 5."""
    runs = runs_of(name, hip_lib)
    keys, counts, ks = GROUPS[name]
    for width, which in ((16, (*BASE_PRECISIONS, "again", "last")), (5, ("narrow",))):
        rc_v, var, rec_v = runs["rv"][width]
        assert rc_v == 0 and rec_v["columns"] == sum(counts) and rec_v["passes"] == -(-max(counts) // width)
        for run in which:
            rc, members, rec = runs[run]
            assert rc == 0 and rec["members"] == len(keys) and rec["candidates"] == sum(counts) and rec["excluded"] == 0
            assert rec["picked"] == sum(ks) and {f: rec["solve"][f] for f in SOLVE} == {f: rec_v[f] for f in SOLVE}
            for key, m, v, c, k in zip(keys, members, var, counts, ks):
                _same_bits(m, v, f"{key}, {run} against the range variances", keys=COLUMNS)
                assert m["order"].shape == m["gains"].shape == m["pick_variances"].shape == (k,) and m["matrix"].shape == (c, c)
                assert m["info"]["candidates"] == c and m["info"]["solve"]["columns"] == c and m["picked"] == k
        for key, a, b in zip(keys, runs["rv_after"][width][1], var):  # (and the selection leaves the other call as it was)
            _same_bits(a, b, f"{key}: the range variances after the selections, width {width}", keys=COLUMNS)
        assert {f: runs["rv_after"][width][2][f] for f in SOLVE} == {f: rec_v[f] for f in SOLVE}


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_matrix_and_total_gain_against_the_dense_reference(hip_lib, name):
    """Contract 2: the diagonal is `variances` bit for bit, every member's matrix is under matrix_bound, its total gain under
    total_gain_bound -- test_selection_gpu.py's check of a single graph, member by member."""
    runs = runs_of(name, hip_lib)
    keys, counts, ks = GROUPS[name]
    ids = _ids(keys, counts)
    for base in BASE_PRECISIONS:
        rc, members, rec = runs[base]
        worst_asym, group_total = 0.0, 0.0
        for key, m, i, c, k in zip(keys, members, ids, counts, ks):
            if c == 0:
                assert m["picked"] == 0 and m["total_gain"] == 0.0 and m["matrix"].shape == (0, 0)
                continue
            np.testing.assert_array_equal(np.diag(m["matrix"]), m["variances"])
            P_ref, bound = matrix_bound(member_twin(key), i, m)
            err = np.abs(m["matrix"] - P_ref)
            print(f"{key}: worst |P - G'Sigma G| / bound = {float(np.max(err / bound)):.3e}")
            assert np.all(err <= bound)
            worst_asym = max(worst_asym, float(np.max(np.abs(m["matrix"] - m["matrix"].T))))
            w = precisions(c, base)
            ref = bounded_reference(m["matrix"], w, k)
            want, slack = total_gain_bound(P_ref, bound, w, m["order"])
            slack += float(np.sum(ref["gain_bound"])) + (k + 1) * EPS * abs(want)
            total = m["total_gain"]
            print(f"{key}, precision {base}: total gain {total:.12f}, dense {want:.12f}, |difference| / bound {abs(total - want) / slack:.3e}")
            assert abs(total - want) <= slack
            assert total == sum(m["gains"][:k].tolist())  # (the host adds them in the order of the picks)
            group_total += total
        assert rec["asymmetry"] == worst_asym and rec["total_gain"] == group_total


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_order_and_gains_against_the_rule_on_the_members_own_matrix(hip_lib, name):
    runs = runs_of(name, hip_lib)
    keys, counts, ks = GROUPS[name]
    for base in BASE_PRECISIONS:
        for key, m, c, k in zip(keys, runs[base][1], counts, ks):
            if c:   # (every list of every group has its precondition asserted on the CPU: tests/test_selection_batch_host.py)
                assert (key, c, k) in PRECONDITION
                check_against_reference(m, bounded_reference(m["matrix"], precisions(c, base), k), f"{key}, precision {base}")


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_every_member_equals_the_selection_alone_on_its_matrix(hip_lib, name):
    """Contract 3: order, gains, pick variances and remaining equal score_select_greedy on the member's returned matrix."""
    runs = runs_of(name, hip_lib)
    keys, counts, ks = GROUPS[name]
    for base in BASE_PRECISIONS:
        for key, m, c, k in zip(keys, runs[base][1], counts, ks):
            if c:
                alone = greedy_from_matrix(m["matrix"], precisions(c, base), k, lib_path=hip_lib)
                _same_bits(m, alone, f"{key}, precision {base}: the member against score_select_greedy", keys=VALUES + ("picked",))


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_widths_and_repeats_give_the_same_bits(hip_lib, name):
    runs = runs_of(name, hip_lib)
    keys, counts, _ = GROUPS[name]
    first = runs[BASE_PRECISIONS[0]]
    for other in ("again", "narrow", "last"):
        for key, a, b in zip(keys, first[1], runs[other][1]):
            _same_bits(a, b, f"{key}: {other}")
        assert runs[other][2]["total_gain"] == first[2]["total_gain"] and runs[other][2]["asymmetry"] == first[2]["asymmetry"]
    assert runs["narrow"][2]["solve"]["passes"] == -(-max(counts) // 5)


@pytest.mark.parametrize("key", [k for k, c in zip(KEYS_SLOTS, COUNTS_SLOTS) if c])
def test_a_member_of_the_unequal_group_alone_in_a_group(hip_lib, key):
    """Contract 4 for (D, B, C, A) with [600, 37, 0, 513] candidates: every member that lists candidates, alone in a group of
    one, gives its bits from the full group."""
    runs = runs_of("slots", hip_lib)
    g = KEYS_SLOTS.index(key)
    c, k = COUNTS_SLOTS[g], KS_SLOTS[g]
    with _handle((key,), hip_lib) as h:
        rc, (alone,), rec = h.select_ranges(_points((key,)), _ids((key,), [c]), [precisions(c, BASE_PRECISIONS[0])], [k], with_matrix=True)
    assert rc == 0 and rec["members"] == 1 and rec["candidates"] == c and rec["picked"] == k
    _same_bits(alone, runs[BASE_PRECISIONS[0]][1][g], f"{key} alone against {key} in {KEYS_SLOTS}")


def test_another_member_order_of_the_unequal_group(hip_lib):
    """Contract 4: (D, B, C, A) as (A, C, D, B) -- the pair kernel's workgroups now begin in A -- gives each member the same bits."""
    runs = runs_of("slots", hip_lib)
    perm = [3, 2, 0, 1]
    keys, counts, ks = ([v[p] for p in perm] for v in (KEYS_SLOTS, COUNTS_SLOTS, KS_SLOTS))
    with _handle(keys, hip_lib) as h:
        rc, members, rec = h.select_ranges(_points(keys), _ids(keys, counts), _weights(counts, BASE_PRECISIONS[0]), ks, with_matrix=True)
    assert rc == 0 and rec["asymmetry"] == runs[BASE_PRECISIONS[0]][2]["asymmetry"] and rec["picked"] == sum(KS_SLOTS)
    for p, key, m in zip(perm, keys, members):
        _same_bits(m, runs[BASE_PRECISIONS[0]][1][p], f"{key} in the order {keys}")


@pytest.mark.parametrize("key", ["A", "D"])
def test_a_member_alone_in_a_group(hip_lib, key):
    """Contract 4: the member alone in a group of one gives its bits from the full group."""
    runs = runs_of("2d", hip_lib)
    g = KEYS_2D.index(key)
    c, k = COUNTS_2D[g], KS_2D[g]
    with _handle((key,), hip_lib) as h:
        rc, (alone,), rec = h.select_ranges(_points((key,)), _ids((key,), [c]), [precisions(c, BASE_PRECISIONS[0])], [k], with_matrix=True)
    assert rc == 0 and rec["members"] == 1 and rec["candidates"] == c and rec["picked"] == k
    _same_bits(alone, runs[BASE_PRECISIONS[0]][1][g], f"{key} alone against {key} in A..E")


def test_another_member_order(hip_lib):
    """Contract 4: a group in another member order gives each member the same bits."""
    runs = runs_of("2d", hip_lib)
    perm = [3, 4, 1, 0, 2]
    keys, counts, ks = ([v[p] for p in perm] for v in (KEYS_2D, COUNTS_2D, KS_2D))
    with _handle(keys, hip_lib) as h:
        rc, members, rec = h.select_ranges(_points(keys), _ids(keys, counts), _weights(counts, BASE_PRECISIONS[0]), ks, with_matrix=True)
    assert rc == 0 and rec["asymmetry"] == runs[BASE_PRECISIONS[0]][2]["asymmetry"]
    for p, key, m in zip(perm, keys, members):
        _same_bits(m, runs[BASE_PRECISIONS[0]][1][p], f"{key} in the order {keys}")


@pytest.mark.parametrize("name", CAPPED)
def test_unconverged_columns_exclude_their_candidates(hip_lib, name):
    """max_iters = max(steps) - 1 over the group: the call returns 1, exactly the late columns are excluded in their members,
    those members follow the rule on the eligible set of their own matrix, and members with no late column keep their bits."""
    runs = runs_of(name, hip_lib)
    keys, counts, ks = GROUPS[name]
    cap = runs["cap"]
    rc, members, rec = runs["capped"]
    full = runs[BASE_PRECISIONS[0]][1]
    n_late = 0
    for key, m, f, c, k in zip(keys, members, full, counts, ks):
        late = f["iterations"] > cap
        n_late += int(np.count_nonzero(late))
        np.testing.assert_array_equal(~m["converged"], late, err_msg=key)
        assert m["info"]["excluded"] == int(np.count_nonzero(late)) and m["rc"] == (1 if np.any(late) else 0)
        if not np.any(late):
            _same_bits(m, f, f"{key}: no late column under the cap {cap}")
            continue
        print(f"{key}, cap {cap}: {int(np.count_nonzero(late))} of {c} columns beyond it")
        assert not np.any(np.isin(m["order"], np.flatnonzero(late))) and np.all(np.isfinite(m["matrix"]))
        w = precisions(c, BASE_PRECISIONS[0])
        ref = bounded_reference(m["matrix"], w, k, excluded=late.astype(np.int32))
        check_against_reference(m, ref, f"{key}, cap {cap}")
        assert m["picked"] == ref["picked"]
        alone = greedy_from_matrix(m["matrix"], w, k, excluded=late.astype(np.int32), lib_path=hip_lib)
        _same_bits(m, alone, f"{key}, cap {cap}: the member against score_select_greedy", keys=VALUES + ("picked",))
    assert rc == 1 and 0 < n_late < sum(counts) and rec["excluded"] == n_late == rec["solve"]["unconverged"]


def test_min_gain_stops_one_member_early(hip_lib):
    """min_gain between C's fifth and sixth gain: C stops after five picks (padding after them), the others -- whose every
    gain lies above the cut -- stay as they were."""
    runs = runs_of("2d", hip_lib)
    cut = runs["cut"]
    rc, members, rec = runs["short"]
    full = runs[BASE_PRECISIONS[0]][1]
    assert rc == 0
    for key, m, f, c, k in zip(KEYS_2D, members, full, COUNTS_2D, KS_2D):
        if key != "C":
            assert c == 0 or np.min(f["gains"]) > cut
            _same_bits(m, f, f"{key} under min_gain = {cut:.4f}")
            continue
        assert f["gains"][5] < cut < f["gains"][4] and m["picked"] == 5 < k
        assert np.all(m["order"][5:] == -1) and np.all(m["gains"][5:] == 0) and np.all(m["pick_variances"][5:] == 0)
        _same_bits({v: m[v][:5] for v in VALUES[:3]}, {v: f[v][:5] for v in VALUES[:3]}, "C: the picks before the stop", keys=VALUES[:3])
        check_against_reference(m, bounded_reference(m["matrix"], precisions(c, BASE_PRECISIONS[0]), k, min_gain=cut), "C, min_gain stop")
    assert rec["picked"] == sum(KS_2D) - 4


def test_errors_are_reported_not_faults(hip_lib):
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    keys = ("C", "B")
    tws = [member_twin(k) for k in keys]
    probs = [t.ref.prob for t in tws]
    arrays = [_point_arrays(t.ref.prob, t.ref.point) for t in tws]
    poses = np.ascontiguousarray(np.concatenate([a[0].ravel() for a in arrays]))
    lms = np.ascontiguousarray(np.concatenate([a[1].ravel() for a in arrays]))
    nv = [p.Np + p.Nl for p in probs]
    good = dict(ptr=[0, 1, 3], pa=[1, 0, 2], pb=[0, 3, nv[1] - 1], w=[4.0, 5.0, 6.0], k=[1, 2])
    who = "score_refine_batch_select_ranges: "
    ints = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    p = lambda v, kind: None if v is None or not v.size else v.ctypes.data_as(kind)  # noqa: E731

    def call(h, lib, ptr, pa, pb, w, k, min_gain=0.0, rel_tol=1e-10, max_iters=4000, width=16, with_points=True):
        ptr, pa, pb, k = ints(ptr), ints(pa), ints(pb), ints(k)
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        info = ScoreSelectBatchInfo()
        picked = np.full(2, -7, dtype=np.int32)
        rc = lib.score_refine_batch_select_ranges(h, p(poses, f64) if with_points else None, p(lms, f64), p(ptr, i32), p(pa, i32),
                                                  p(pb, i32), p(w, f64), p(k, i32), min_gain, rel_tol, max_iters, width, None, None, None,
                                                  p(picked, i32), None, None, None, None, None, None, None, C.byref(info))
        return rc, lib.score_last_error().decode(), info, picked

    many = 4097
    with RefineBatchHandle(probs, hip_lib) as h:
        lib = bind(h.lib, SELECT_BATCH)
        for what, kw in (
            ("null handle", dict(good, h=None)),
            ("the points are missing", dict(good, h=h.h, with_points=False)),
            ("member 1: a pair joins a variable to itself", dict(good, h=h.h, pb=[0, 0, nv[1] - 1])),
            ("member 0: a pair's variable is out of range", dict(good, h=h.h, pb=[nv[0], 3, 4])),
            ("member 1: a pair's variable is out of range", dict(good, h=h.h, pa=[1, -1, 2])),
            ("pair_ptr must start at 0", dict(good, h=h.h, ptr=[1, 1, 3])),
            ("pair_ptr must not decrease", dict(good, h=h.h, ptr=[0, 3, 1])),
            ("pairs without their lists", dict(good, h=h.h, pa=None)),
            ("block_width must be 1..16", dict(good, h=h.h, width=0)),
            ("block_width must be 1..16", dict(good, h=h.h, width=17)),
            ("rel_tol must be positive", dict(good, h=h.h, rel_tol=0.0)),
            ("max_iters >= 1", dict(good, h=h.h, max_iters=0)),
            ("min_gain must be >= 0", dict(good, h=h.h, min_gain=-1.0)),
            ("min_gain must be >= 0", dict(good, h=h.h, min_gain=float("nan"))),
            ("k is missing", dict(good, h=h.h, k=None)),
            ("the precisions are missing", dict(good, h=h.h, w=None)),
            ("member 0: k must be 1..min(candidates, 256)", dict(good, h=h.h, k=[0, 2])),
            ("member 0: k must be 1..min(candidates, 256)", dict(good, h=h.h, k=[2, 2])),
            ("member 1: k must be 1..min(candidates, 256)", dict(good, h=h.h, k=[1, 3])),
            ("member 1: k must be 0 for a member without candidates", dict(good, h=h.h, ptr=[0, 3, 3], pb=[0, 3, 4], k=[1, 1])),
            ("member 1: a precision must be finite and positive", dict(good, h=h.h, w=[4.0, 5.0, 0.0])),
            ("member 0: a precision must be finite and positive", dict(good, h=h.h, w=[np.inf, 5.0, 6.0])),
            ("member 1: a precision must be finite and positive", dict(good, h=h.h, w=[4.0, np.nan, 6.0])),
            ("member 0: the number of candidates must be at most 4096",
             dict(h=h.h, ptr=[0, many, many], pa=[1] * many, pb=[0] * many, w=[4.0] * many, k=[1, 0])),
            ("member 0: k must be 1..min(candidates, 256)",
             dict(h=h.h, ptr=[0, 300, 300], pa=[1] * 300, pb=[0] * 300, w=[4.0] * 300, k=[257, 0])),
        ):
            rc, msg, _, _ = call(lib=lib, **kw)
            print(what, "->", rc, msg)
            assert rc < 0 and what in msg and msg.startswith(who), (what, rc, msg)
            # ... and the handle still works after every one of them
            rc, msg, info, picked = call(h.h, lib, **good)
            assert rc == 0 and info.solve.columns == 3 and info.picked == 3 and picked.tolist() == [1, 2] and info.members == 2, (what, rc, msg)
        # nothing listed: no work, no error, zeros
        for kw in (dict(good, ptr=[0, 0, 0], pa=None, pb=None, w=None, k=[0, 0]), dict(good, ptr=[0, 0, 0], pa=None, pb=None, w=None, k=None),
                   dict(good, ptr=None, pa=None, pb=None, w=None, k=None)):
            rc, msg, info, picked = call(h.h, lib, **kw)
            assert rc == 0 and info.solve.columns == 0 and info.solve.passes == 0 and info.candidates == 0 and info.picked == 0, msg
            assert info.members == 2 and info.total_gain == 0.0 and picked.tolist() == [0, 0]
        pts = [t.ref.point for t in tws]
        rc, members, rec = h.select_ranges(pts, [None, []], [None, None], 3)
        assert rc == 0 and rec["candidates"] == 0 and all(m["order"].shape == (0,) and m["matrix"] is None and m["rc"] == 0 for m in members)
        # duplicate pairs within a member are allowed
        ids = candidates("C", 4)
        dup = np.concatenate([ids, ids])
        rc, (c_out, b_out), _ = h.select_ranges(pts, [dup, None], [np.full(8, 4.0), None], [8, 0], with_matrix=True)
        assert rc == 0 and c_out["picked"] == 8 and sorted(c_out["order"].tolist()) == list(range(8)) and b_out["picked"] == 0
        # (a pair and its copy tie or nearly tie: no order is compared with a reference's, only with the rule's own kernels)
        alone = greedy_from_matrix(c_out["matrix"], np.full(8, 4.0), 8, lib_path=hip_lib)
        _same_bits(c_out, alone, "C with every pair twice: the member against score_select_greedy", keys=VALUES + ("picked",))


def _graphs(keys, counts):
    tws = [member_twin(k) for k in keys]
    ids = _ids(keys, counts)
    return [t.fg for t in tws], [t.results for t in tws], ids, [names_of(k, i) for k, i in zip(keys, ids)]


def test_select_ranges_batch_by_name(hip_lib):
    """The front end against its python engine: equal orders (the lists' pivot gaps are held by the host test), the raw call's
    bits on the same groups, a 2-D and a 3-D list in one call."""
    keys, counts, ks = ("A", "3D1", "B", "C"), [37, 7, 0, 9], [12, 7, 5, 9]
    fgs, results, ids, names = _graphs(keys, counts)
    ws = [precisions(37, 4.0), precisions(7, 4.0), 1.0, precisions(9, 400.0)]
    dev = select_ranges_batch(fgs, results, names, ks, precision=ws, lib_path=hip_lib)
    host = select_ranges_batch(fgs, results, names, ks, precision=ws, engine="python")
    with _handle(("A", "B", "C"), hip_lib) as h:
        _, raw, rec = h.select_ranges(_points(("A", "B", "C")), [ids[0], None, ids[3]], [ws[0], None, ws[3]], [12, 0, 9])
    for key, nm, k, (sel, info), (hs, hinfo) in zip(keys, names, ks, dev, host):
        assert isinstance(sel, Selection) and sel.pairs == hs.pairs and info["engine"] == "device" and hinfo["engine"] == "python"
        np.testing.assert_array_equal(sel.order, hs.order, err_msg=key)
        assert info["group"] == (1 if key.startswith("3D") else 0) and sel.excluded.size == 0
        if not nm:
            assert sel.order.size == 0 and sel.total_gain == 0.0 and info["passes"] == 3
            continue
        assert len(sel.order) == k and np.all(np.isnan(sel.remaining_variance[sel.order])) and info["batches"] == -(-len(nm) // 16)
    for g, m in ((0, raw[0]), (3, raw[2])):
        np.testing.assert_array_equal(dev[g][0].gains, m["gains"])
        np.testing.assert_array_equal(dev[g][0].variance, m["variances"])
        np.testing.assert_array_equal(dev[g][1]["residuals"], m["residuals"])
    assert dev[0][1]["passes"] == rec["solve"]["passes"] == 3


def test_refine_estimate_batch_with_select(hip_lib):
    """refine_estimate_batch(select=...) returns the refinement it returns without the keyword, bit for bit, and the Selection
    of the two-step use (run, then the selection at the refined points on the kept handle)."""
    keys = ("B", "C", "E")
    fgs, starts = group(keys)
    probs, first = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, starts)])
    ids = [candidates("B", 5), None, candidates("E", 6)]
    names = [names_of(k, i) if i is not None else None for k, i in zip(keys, ids)]
    with RefineBatchHandle(probs, hip_lib) as h:
        refined, _ = h.run(list(first))
        rc, raw, rec = h.select_ranges(refined, ids, [np.full(5, 4.0), None, np.full(6, 4.0)], [3, 0, 3])
    assert rc == 0
    out = refine_estimate_batch(fgs, starts, lib_path=hip_lib, select=dict(pairs=names, k=3, precision=4.0))
    plain = refine_estimate_batch(fgs, starts, lib_path=hip_lib)
    for nm, m, (res_r, info), (res_p, info_p) in zip(names, raw, out, plain):
        sel, sinfo = info["selection"]
        assert isinstance(sel, Selection) and sel.pairs == [(nm or [])[c] for c in m["order"][: m["picked"]]] and sinfo["engine"] == "device"
        np.testing.assert_array_equal(sel.order, m["order"][: m["picked"]])
        np.testing.assert_array_equal(sel.gains, m["gains"][: m["picked"]])
        np.testing.assert_array_equal(sel.variance, m["variances"])
        np.testing.assert_array_equal(sinfo["residuals"], m["residuals"])
        assert "selection" not in info_p and info["cost_final"] == info_p["cost_final"] and info["iterations"] == info_p["iterations"]
        for name in res_p.poses:
            np.testing.assert_array_equal(res_r.poses[name], res_p.poses[name])
        for name in res_p.landmarks:
            np.testing.assert_array_equal(res_r.landmarks[name], res_p.landmarks[name])
