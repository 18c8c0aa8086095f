"""Batched marginal covariances on the device (score_refine_batch_marginals, csrc/score_marginals_batch.hpp).

Every device column is judged by the derived bound of tests/marginals_helpers.py (``check_columns``) against the dense
Cholesky ``Reference`` of its member at the same point: every term of the bound comes from the reference, the library's own
reported residual and the number format -- no tolerance is chosen.  So that the bound cannot go vacuous, its worst value
over the largest covariance entry must stay below 1e-3 on every member (the reference's own share is at most 3.2e-6).

The points are ``twin_alone(key)[0]``, the host-refined estimates of tests/refine_batch_helpers.py: every member's H is
positive definite there (lambda_min 1.5e-2 .. 2.2e-1).  The group A..E meets every boundary of the device code: C (37
unknowns, 7 default columns) leaves 9 of 16 slots dead from the start, D has the only long row (158 > 128) and its tile
sits between short-row members, and at width 4 the members drop out at different passes."""
import ctypes as C
import functools

import numpy as np
import pytest

from marginals_helpers import (Reference, check_columns, check_iteration_caps, landmark_names, pose_names, reference,
                               undetermined_graph)
from marginals_helpers import noisy_truth as plain_noisy_truth
from refine_batch_helpers import KEYS_2D, group, member, rough_start, twin_alone
from score_amd.manhattan import make_manhattan
from score_amd.marginals import _problem_and_point, _select, marginal_covariances
from score_amd.marginals_batch import ScoreMarginalsBatchInfo, _bind, marginal_covariances_batch
from score_amd.refine_batch import RefineBatchHandle, _problem_of, refine_estimate_batch
from score_amd.refine_robust import _point_arrays

pytestmark = pytest.mark.gpu

VACUOUS = 1e-3  # worst bound / largest covariance entry beyond which the bound says nothing


@functools.lru_cache(maxsize=None)
def weights_a():
    w = np.ones(len(member("A")[0].range_measurements))
    w[[1, 5, 9]] = 0.0
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def ref_of(key, weighted=False):
    """The dense reference of a member at its host-refined point (A: optionally with three of its ranges weighted 0)."""
    return Reference(member(key)[0], twin_alone(key)[0], range_weights=weights_a() if weighted else None)


def _points(keys):
    return [member(k)[0] for k in keys], [twin_alone(k)[0] for k in keys]


def _check(label, ref, variables, info):
    """One member of a batch result under its bound; returns (cols, A, bound, delta)."""
    names, cols = ref.columns(variables)
    assert info["order"] == names
    A = info["joint_raw"]
    assert A.shape == (len(cols), len(cols))
    figures, bound, delta = check_columns(ref, cols, A, info["residuals"], label)
    assert figures["worst_bound_over_max_sigma"] < VACUOUS, f"{label}: the bound is vacuous"
    return cols, A, bound, delta


_cache = {}


def group_a_to_e(hip_lib, width):
    """The group A..E, default variables, three of A's ranges weighted 0: computed once per width."""
    if (hip_lib, width) not in _cache:
        fgs, pts = _points(KEYS_2D)
        _cache[(hip_lib, width)] = marginal_covariances_batch(fgs, pts, joint=True, range_weights=[weights_a()] + [None] * 4,
                                                              block_width=width, lib_path=hip_lib)
    return _cache[(hip_lib, width)]


def test_group_of_five_in_one_pass(hip_lib):
    plain = ref_of("A")
    assert np.max(np.abs(ref_of("A", True).H - plain.H)) > 1e-3  # the three ranges matter
    out = group_a_to_e(hip_lib, 16)
    columns = {}
    for k, (cov, info) in zip(KEYS_2D, out):
        cols, *_ = _check(k, ref_of(k, k == "A"), None, info)
        columns[k] = len(cols)
        assert info["passes"] == 1 and info["batches"] == 1 and info["group"] == 0 and info["engine"] == "device"
        assert list(cov) == info["order"]
    assert columns == {"A": 15, "B": 10, "C": 7, "D": 14, "E": 8}
    assert ref_of("D").longest_row > 128 and all(ref_of(k).longest_row <= 128 for k in "BCE")


def test_width_four_members_drop_out_at_different_passes(hip_lib):
    wide, narrow = group_a_to_e(hip_lib, 16), group_a_to_e(hip_lib, 4)
    fgs, pts = _points(KEYS_2D)
    for k, fg, pt, (_, info16), (_, info4) in zip(KEYS_2D, fgs, pts, wide, narrow):
        ref = ref_of(k, k == "A")
        assert info4["passes"] == 4  # 15 columns of A; C and E (7, 8) are out after two passes, B (10) after three
        assert info4["batches"] == -(-len(info4["residuals"]) // 4)
        _, A4, bound4, _ = _check(f"{k}, width 4", ref, None, info4)
        _, A16, bound16, _ = _check(f"{k}, width 16", ref, None, info16)
        _, single = marginal_covariances(fg, pt, joint=True, range_weights=weights_a() if k == "A" else None, lib_path=hip_lib)
        _, A1, bound1, _ = _check(f"{k}, alone", ref, None, single)
        for other, bound, what in ((A16, bound16, "width 16"), (A1, bound1, "the single handle")):
            diff = np.linalg.norm(A4 - other, axis=0)
            print(f"{k}: width 4 against {what}: worst column difference / allowed {float(np.max(diff / (bound4 + bound))):.3e}")
            assert np.all(diff <= bound4 + bound)
    assert [len(info["residuals"]) for _, info in narrow] == [15, 10, 7, 14, 8]


def test_all_variables_of_three_members(hip_lib):
    keys = ("B", "C", "E")
    fgs, pts = _points(keys)
    everything = [[nm for ch in pose_names(fg) for nm in ch][1:] + landmark_names(fg) for fg in fgs]
    out = marginal_covariances_batch(fgs, pts, everything, joint=True, lib_path=hip_lib)
    for k, names, (cov, info) in zip(keys, everything, out):
        ref = ref_of(k)
        cols, A, bound, delta = _check(f"{k}, all variables", ref, names, info)
        assert len(cols) == ref.n and info["passes"] == 13  # 151, 37, 197 columns: 10, 3 and 13 passes of 16
        assert info["batches"] == -(-ref.n // 16)
        # all rows are selected: the reported residual is |e_c - H x_c|_2 of the dense H, to the rounding of that product
        mine = np.linalg.norm(np.eye(ref.n)[:, cols] - ref.H[:, cols] @ A, axis=0)
        print(f"{k}: residual recomputation: worst |reported - recomputed| / delta =",
              float(np.max(np.abs(info["residuals"] - mine) / delta)))
        assert np.all(np.abs(info["residuals"] - mine) <= delta)
        # H^-1 is symmetric: what is left of A - A' is the two columns' errors
        asym = np.abs(A - A.T)
        assert np.all(asym <= bound[:, None] + bound[None, :])
        assert info["asymmetry"] == float(asym.max())
    assert [ref_of(k).n for k in keys] == [151, 37, 197]


def test_3d_group(hip_lib):
    keys = ("3D0", "3D1")
    fgs, pts = _points(keys)
    out = marginal_covariances_batch(fgs, pts, joint=True, lib_path=hip_lib)
    for k, fg, (cov, info) in zip(keys, fgs, out):
        cols, *_ = _check(k, ref_of(k), None, info)
        want = landmark_names(fg) + [ch[-1] for ch in pose_names(fg)]
        assert info["order"] == want and len(cols) == 21 and info["passes"] == 2  # 16 slots, then 8 with 5 live
        assert [cov[nm].shape for nm in want] == [(3, 3)] * 3 + [(6, 6)] * 2
        off = np.concatenate([[0], np.cumsum([cov[nm].shape[0] for nm in want])])
        for j, nm in enumerate(want):
            np.testing.assert_array_equal(info["joint"][off[j]:off[j + 1], off[j]:off[j + 1]], cov[nm])


def test_segmented_chain_inside_a_union(hip_lib):
    """One chain of 1100 poses (the second level of score_join.hpp, applied to all vectors of the pass) beside C."""
    fg, results, ref = reference("c")
    poses = pose_names(fg)[0]
    wanted = landmark_names(fg) + [poses[550], poses[1099]]
    fg_c, pt_c = member("C")[0], twin_alone("C")[0]
    out = marginal_covariances_batch([fg, fg_c], [results, pt_c], [wanted, None], joint=True, lib_path=hip_lib)
    cols, *_ = _check("1100 poses", ref, wanted, out[0][1])
    assert len(cols) == 10
    _check("C beside it", ref_of("C"), None, out[1][1])


def test_iteration_cap_at_the_chunk_boundaries(hip_lib):
    """(A, C) at width 4 under max_iters at and around the boundaries of the queued chunks: see check_iteration_caps."""
    keys = ("A", "C")
    probs, points = zip(*[_problem_and_point(member(k)[0], twin_alone(k)[0], None, None) for k in keys])
    ids = [_select(p, None)[1] for p in probs]
    with RefineBatchHandle(probs, hip_lib) as h:
        check_iteration_caps(lambda cap: h.marginals(list(points), ids, max_iters=cap, block_width=4)[:2], "(A, C), width 4")


def test_undetermined_member_is_a_verdict_for_that_member_only(hip_lib):
    fg = undetermined_graph()  # one range fixes the landmark's distance only: H is singular
    results = plain_noisy_truth(fg)
    lm = landmark_names(fg)[0]
    fg_c, pt_c = member("C")[0], twin_alone("C")[0]
    probs, points = zip(*[_problem_and_point(g, r, None, None) for g, r in ((fg, results), (fg_c, pt_c))])
    sels = [_select(p, None) for p in probs]
    ref_c = ref_of("C")
    with RefineBatchHandle(probs, hip_lib) as h:
        rc, cols, info = h.marginals(list(points), [s[1] for s in sels], max_iters=50)
        print("undetermined member:", info, "steps", cols[0][2], "converged", cols[0][3])
        assert rc == 1 and 0 < info["unconverged"] <= len(sels[0][3])
        assert not np.all(cols[0][3]) and np.all(cols[0][2] <= 50)
        # only member 0 is flagged: C's columns are under their bound in the same call
        A, res, steps, converged = cols[1]
        assert np.all(converged) and info["unconverged"] == int(np.sum(~cols[0][3]))
        figures, _, _ = check_columns(ref_c, sels[1][3], A, res, "C beside the undetermined member")
        assert figures["worst_bound_over_max_sigma"] < VACUOUS
        with pytest.raises(RuntimeError, match=rf"graph 0: .*{lm}"):
            marginal_covariances_batch([fg, fg_c], [results, pt_c], max_iters=50, lib_path=hip_lib)
        # a well-posed call on the same handle afterwards: the undetermined member lists nothing
        rc, cols, info = h.marginals(list(points), [[], sels[1][1]])
        assert rc == 0 and info["unconverged"] == 0 and info["columns"] == len(sels[1][3])
        assert cols[0][0].shape == (0, 0) and cols[0][1].size == 0
        figures, _, _ = check_columns(ref_c, sels[1][3], cols[1][0], cols[1][1], "C after the singular call")
        assert figures["worst_bound_over_max_sigma"] < VACUOUS


def test_handle_state_survives_the_marginals(hip_lib):
    """run, marginals at the refined points, run from other starts: the second run equals a fresh handle's bit for bit; and
    refine_estimate_batch(marginals=True) returns the covariances of that two-step use."""
    keys = ("B", "C", "E")
    fgs, starts = group(keys)
    probs, first = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, starts)])
    second = [_problem_of(fg, rough_start(k), None, None)[1] for k, fg in zip(keys, fgs)]
    sels = [_select(p, None) for p in probs]
    with RefineBatchHandle(probs, hip_lib) as h:
        refined, _ = h.run(list(first))
        rc, cols, minfo = h.marginals(refined, [s[1] for s in sels])
        assert rc == 0
        pts, infos = h.run(second)
    with RefineBatchHandle(probs, hip_lib) as h:
        fresh, finfos = h.run(second)
    for k, a, b, ia, ib in zip(keys, pts, fresh, infos, finfos):
        print(k, "run after the marginals: iterations", ia["iterations"], "solves", ia["linear_solves"], "pcg", ia["pcg_iters"])
        assert np.array_equal(a, b)
        for f in ("iterations", "linear_solves", "pcg_iters", "cost_initial", "cost_final", "grad_inf"):
            assert ia[f] == ib[f]
    out = refine_estimate_batch(fgs, starts, lib_path=hip_lib, marginals=True)
    plain = refine_estimate_batch(fgs, starts, lib_path=hip_lib)
    for (names, _, size, _), (A, res, steps, converged), (res_m, info), (res_p, info_p) in zip(sels, cols, out, plain):
        cov, mi = info["marginals"]
        assert mi["order"] == names and mi["passes"] == minfo["passes"] == 1 and np.all(converged)
        S = 0.5 * (A + A.T)
        off = np.concatenate([[0], np.cumsum(size)])
        for j, nm in enumerate(names):
            np.testing.assert_array_equal(cov[nm], S[off[j]:off[j + 1], off[j]:off[j + 1]])
        np.testing.assert_array_equal(mi["residuals"], res)
        # ... and the refinement itself is what it is without the keyword
        assert "marginals" not in info_p and info["cost_final"] == info_p["cost_final"]
        for nm in names:
            src = res_m.landmarks if nm in res_m.landmarks else res_m.poses
            ref = res_p.landmarks if nm in res_p.landmarks else res_p.poses
            np.testing.assert_array_equal(src[nm], ref[nm])


def test_errors_are_reported_not_faults(hip_lib):
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    keys = ("C", "B")
    probs, points = zip(*[_problem_and_point(member(k)[0], twin_alone(k)[0], None, None) for k in keys])
    arrays = [_point_arrays(p, x) for p, x in zip(probs, points)]
    poses = np.ascontiguousarray(np.concatenate([a[0].ravel() for a in arrays]))
    lms = np.ascontiguousarray(np.concatenate([a[1].ravel() for a in arrays]))
    # a member large enough for the 1 GiB limit: 3899 free poses x 3 = 11697 columns, 11697^2 > 2^27
    big = make_manhattan(n_robots=1, n_poses=3900, n_beacons=0, seed=1)
    p_big, x_big = _problem_and_point(big, plain_noisy_truth(big), None, None)
    assert (3 * (p_big.Np - 1)) ** 2 > 1 << 27

    def call(h, lib, ptr, ids, pp=poses, ll=lms, rel_tol=1e-10, max_iters=4000, width=16):
        ptr = None if ptr is None else np.ascontiguousarray(ptr, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        info = ScoreMarginalsBatchInfo()
        rc = lib.score_refine_batch_marginals(h, pp.ctypes.data_as(f64), ll.ctypes.data_as(f64) if ll.size else None,
                                              None if ptr is None else ptr.ctypes.data_as(i32),
                                              ids.ctypes.data_as(i32) if ids.size else None, rel_tol, max_iters, width,
                                              None, None, None, C.byref(info))
        return rc, lib.score_last_error().decode(), info

    lm_c = probs[0].Np  # C's first landmark, member-local
    with RefineBatchHandle(probs, hip_lib) as h:
        lib = _bind(h.lib)
        good = ([0, 1, 3], [lm_c, 3, probs[1].Np])
        for what, kw in (
            ("null handle", dict(h=None, ptr=good[0], ids=good[1])),
            ("var_ptr", dict(h=h.h, ptr=None, ids=good[1])),
            ("pose 0", dict(h=h.h, ptr=[0, 1, 2], ids=[lm_c, 0])),
            ("twice", dict(h=h.h, ptr=[0, 1, 3], ids=[lm_c, 3, 3])),
            ("out of range", dict(h=h.h, ptr=[0, 1, 2], ids=[probs[0].Np + probs[0].Nl, 3])),
            ("out of range", dict(h=h.h, ptr=[0, 1, 2], ids=[-1, 3])),
            ("block_width", dict(h=h.h, ptr=good[0], ids=good[1], width=0)),
            ("block_width", dict(h=h.h, ptr=good[0], ids=good[1], width=17)),
            ("rel_tol", dict(h=h.h, ptr=good[0], ids=good[1], rel_tol=0.0)),
            ("rel_tol", dict(h=h.h, ptr=good[0], ids=good[1], rel_tol=-1.0)),
            ("max_iters", dict(h=h.h, ptr=good[0], ids=good[1], max_iters=0)),
        ):
            rc, msg, _ = call(lib=lib, **kw)
            print(what, "->", rc, msg)
            assert rc < 0 and what in msg, (what, rc, msg)
        # ... and the handle still solves: member C's first landmark, two variables of B
        rc, msg, info = call(h.h, lib, *good)
        assert rc == 0 and info.columns == 2 + 3 + 2 and info.unconverged == 0 and info.passes == 1
        ref = ref_of("C")
        _, cols, _ = h.marginals(list(points), [[lm_c], [3, probs[1].Np]])
        check_columns(ref, ref.columns([landmark_names(member("C")[0])[0]])[1], cols[0][0], cols[0][1], "C after the errors")
    with RefineBatchHandle([p_big], hip_lib) as h:
        pa, la = _point_arrays(p_big, x_big)
        rc, msg, _ = call(h.h, _bind(h.lib), [0, p_big.Np - 1], np.arange(1, p_big.Np), pp=pa.ravel(), ll=la.ravel())
        print("1 GiB ->", rc, msg)
        assert rc < 0 and "1 GiB" in msg
