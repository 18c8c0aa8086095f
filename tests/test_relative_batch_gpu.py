"""Batched predicted relative poses and their covariances on the device (score_refine_batch_relative_covariances,
csrc/score_relative_batch.hpp).

Every member of every group is judged as tests/test_relative_gpu.py judges a single graph: ``check_relative`` against its own
dense reference (NumPy's Jacobian, the dense Cholesky solve) under the bounds derived in tests/relative_helpers.py.  No
tolerance is chosen here.

The group A..E (tests/refine_batch_helpers.py, at the host-refined points) with the pair counts [6, 0, 1, 11, 2] has 18, 0, 3,
33 and 6 columns: at width 16 three passes with the live slots (16, 0, 3, 16, 6), (2, 0, 0, 16, 0), (0, 0, 0, 1, 0) -- A's pair
5 and D's pairs 5 and 10 straddle passes, B lists nothing, C is below one wave between larger members."""
import ctypes as C
import functools

import numpy as np
import pytest

import relative_helpers as rh
from marginals_helpers import noisy_truth as plain_noisy_truth
from refine_batch_helpers import KEYS_2D, group, rough_start
from samples_batch_helpers import member_twin, same_bits
from score_amd.bindings import RELATIVE_BATCH, ScoreMarginalsBatchInfo, bind
from score_amd.manhattan import make_manhattan
from score_amd.marginals import _problem_and_point, _select, dense_information
from score_amd.refine import unknown_sizes
from score_amd.refine_batch import RefineBatchHandle, _problem_of, refine_estimate_batch
from score_amd.refine_robust import _point_arrays
from score_amd.relative import PredictedRelativePoses, RelativeHandle
from score_amd.relative_batch import predicted_relative_poses_batch

pytestmark = pytest.mark.gpu

KEYS_3D = ("3D0", "3D1")
PAIRS = [6, 0, 1, 11, 2]
OUTPUTS = ("rotations", "translations", "covariances", "residuals", "iterations", "converged", "rc")


def _handle(keys, hip_lib):
    return RefineBatchHandle([member_twin(k).ref.prob for k in keys], hip_lib)


def _points(keys):
    return [member_twin(k).ref.point for k in keys]


def _pairs(keys, counts):
    return [rh.pair_list(member_twin(k).ref.prob, c) if c else None for k, c in zip(keys, counts)]


def _names(prob, ids):
    names = [str(nm) for nm in prob.a["pose_names"]]
    return [(names[a], names[b]) for a, b in ids]


@functools.lru_cache(maxsize=None)
def a_to_e(hip_lib):
    """The calls on the group A..E, on one handle, shared by the tests below and left unchanged."""
    pairs = _pairs(KEYS_2D, PAIRS)
    rng_pairs = [rh.pair_list(member_twin(k).ref.prob, c) if c else None for k, c in zip(KEYS_2D, [5, 0, 3, 17, 1])]
    pts = _points(KEYS_2D)
    with _handle(KEYS_2D, hip_lib) as h:
        out = dict(pairs=pairs,
                   wide=h.relative_covariances(pts, pairs),
                   again=h.relative_covariances(pts, pairs),
                   five=h.relative_covariances(pts, pairs, block_width=5),
                   one=h.relative_covariances(pts, pairs, block_width=1),
                   rv={w: h.range_variances(pts, rng_pairs, block_width=w) for w in (16, 3, 1)})
        rv = h.range_variances(pts, rng_pairs)
        lev = h.leverage(pts, [None] * 5, 3, [1, 2, 3, 4, 5])
        mar = h.marginals(pts, [member_twin(k).ids for k in KEYS_2D])
        assert rv[0] == 0 and lev[0] == 0 and mar[0] == 0
        out["after"] = h.relative_covariances(pts, pairs)
    return out


def _check_members(keys, members, pairs, label, **kw):
    for k, m, ids in zip(keys, members, pairs):
        count = 0 if ids is None else len(ids)
        d, dp = unknown_sizes(member_twin(k).ref.prob)
        assert m["covariances"].shape == (count, dp, dp) and m["rotations"].shape == (count, d, d)
        assert m["translations"].shape == (count, d) and m["residuals"].shape == m["iterations"].shape == (count, dp)
        assert m["info"]["columns"] == count * dp
        if count == 0:
            continue
        rh.check_relative(member_twin(k).ref, ids, m, f"{k} {label}, {count} pairs", **kw)
        if kw.get("need_converged", True):
            assert np.all(np.linalg.eigvalsh(0.5 * (m["covariances"] + np.swapaxes(m["covariances"], 1, 2))) > 0)


def test_group_under_the_bounds(hip_lib):
    runs = a_to_e(hip_lib)
    rc, members, info = runs["wide"]
    assert [0 if p is None else len(p) for p in runs["pairs"]] == PAIRS
    assert rc == 0 and info["passes"] == 3 and info["columns"] == 60 and info["unconverged"] == 0 and info["pcg_iters"] > 0
    _check_members(KEYS_2D, members, runs["pairs"], "in A..E")
    for k, ids in zip(KEYS_2D, runs["pairs"]):
        if ids is not None and len(ids) > 1:
            assert ids[0, 0] == 0 and ids[1, 1] == 0  # the fixed first pose as a, and as b
        assert member_twin(k).ref.lambda_min > 0


def test_block_widths(hip_lib):
    """Widths 5 and 1 against 16: the same bounds, 7 and 33 passes.  The outputs are bit-equal where the group's lock-step
    iteration is column-independent; whether it is, the ranges' group call shows first on the same handle."""
    runs = a_to_e(hip_lib)
    wide = runs["wide"][1]
    r16 = runs["rv"][16][1]
    independent = all(np.array_equal(a[k], b[k]) for w in (3, 1) for a, b in zip(r16, runs["rv"][w][1])
                      for k in ("variances", "residuals", "iterations"))
    print(f"the ranges' group call gives equal bits under widths 16, 3, 1: {independent}")
    for name, passes in (("five", 7), ("one", 33)):
        rc, members, info = runs[name]
        assert rc == 0 and info["passes"] == passes and info["columns"] == 60 and info["unconverged"] == 0
        _check_members(KEYS_2D, members, runs["pairs"], f"in A..E, {passes} passes")
        same = all(np.array_equal(a[k], b[k]) for a, b in zip(members, wide) for k in OUTPUTS)
        print(f"A..E: {passes} passes give the bits of width 16: {same}")
        if independent:
            for key, a, b in zip(KEYS_2D, members, wide):
                same_bits(a, b, f"{key}: {passes} passes against width 16", keys=OUTPUTS)


def test_two_calls_and_a_call_after_the_others(hip_lib):
    runs = a_to_e(hip_lib)
    for key, a, b, c in zip(KEYS_2D, runs["wide"][1], runs["again"][1], runs["after"][1]):
        same_bits(a, b, f"{key}: the second identical call", keys=OUTPUTS)
        same_bits(a, c, f"{key}: after range variances, leverage and marginals", keys=OUTPUTS)
    assert runs["wide"][2]["pcg_iters"] == runs["again"][2]["pcg_iters"] == runs["after"][2]["pcg_iters"]


def test_handle_state_survives(hip_lib):
    """run, the relative covariances at the refined points, run from other starts: the second run and the marginals equal a
    fresh handle's bit for bit."""
    keys = ("B", "C", "E")
    fgs, starts = group(keys)
    probs, first = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, starts)])
    second = [_problem_of(fg, rough_start(k), None, None)[1] for k, fg in zip(keys, fgs)]
    ids = [_select(p, None)[1] for p in probs]
    with RefineBatchHandle(probs, hip_lib) as h:
        refined, _ = h.run(list(first))
        rc, _, _ = h.relative_covariances(refined, [rh.pair_list(p, 3) for p in probs])
        assert rc == 0
        pts, infos = h.run(second)
        _, cols, _ = h.marginals(refined, ids)
    with RefineBatchHandle(probs, hip_lib) as h:
        fresh, finfos = h.run(second)
    with RefineBatchHandle(probs, hip_lib) as h:
        _, fresh_cols, _ = h.marginals(refined, ids)
    for k, a, b, ia, ib in zip(keys, pts, fresh, infos, finfos):
        assert np.array_equal(a, b), k
        for f in ("iterations", "linear_solves", "pcg_iters", "cost_initial", "cost_final", "grad_inf"):
            assert ia[f] == ib[f]
    for k, a, b in zip(keys, cols, fresh_cols):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y, err_msg=k)


@pytest.mark.parametrize("key", ["A", "D"])
def test_a_member_alone_and_the_single_handle(hip_lib, key):
    """The member alone in a group equals the member in A..E bit for bit; the group member and the single handle both sit
    inside check_relative's bounds of the one reference they share."""
    runs = a_to_e(hip_lib)
    g = KEYS_2D.index(key)
    tw, ids = member_twin(key), runs["pairs"][g]
    with _handle((key,), hip_lib) as h:
        rc1, (alone,), info1 = h.relative_covariances([tw.ref.point], [ids])
    assert rc1 == 0 and info1["passes"] == -(-3 * PAIRS[g] // 16) and info1["columns"] == 3 * PAIRS[g]
    same_bits(alone, runs["wide"][1][g], f"{key} alone against {key} in A..E", keys=OUTPUTS)
    with RelativeHandle(tw.ref.prob, hip_lib) as h:
        single = h.relative_covariances(tw.ref.point, ids, with_solutions=True)
    rh.check_relative(tw.ref, ids, single, f"{key} on a single handle")
    rh.check_relative(tw.ref, ids, runs["wide"][1][g], f"{key} in A..E")


def test_3d_group(hip_lib):
    pairs = _pairs(KEYS_3D, [3, 2])
    with _handle(KEYS_3D, hip_lib) as h:
        rc, members, info = h.relative_covariances(_points(KEYS_3D), pairs)
    assert rc == 0 and info["columns"] == 30 and info["passes"] == 2 and info["unconverged"] == 0
    _check_members(KEYS_3D, members, pairs, "in (3D0, 3D1)")


def test_iteration_cap(hip_lib):
    keys = ("A", "C")
    pairs = _pairs(keys, [6, 1])
    with _handle(keys, hip_lib) as h:
        rc0, full, _ = h.relative_covariances(_points(keys), pairs, block_width=4)
        cap = max(int(m["iterations"].max()) for m in full) - 1
        rc, out, info = h.relative_covariances(_points(keys), pairs, block_width=4, max_iters=cap)
    missed = sum(int(np.count_nonzero(~m["converged"])) for m in out)
    print(f"(A, C), 21 columns, cap {cap}: converged {[m['converged'].ravel().tolist() for m in out]}")
    assert rc0 == 0 and rc == 1 and info["unconverged"] == missed and 0 < missed < 21
    for k, m, f in zip(keys, out, full):
        keep = m["converged"]
        np.testing.assert_array_equal(keep, f["iterations"] <= cap)
        assert m["rc"] == (0 if np.all(keep) else 1)
        assert np.all(m["iterations"][~keep] == cap)  # (reported by the call as -(cap + 1))
        np.testing.assert_array_equal(m["iterations"][keep], f["iterations"][keep])
        np.testing.assert_array_equal(m["residuals"][keep], f["residuals"][keep])
        live = np.broadcast_to(keep[:, None, :], m["covariances"].shape)  # (column q of P_c is column j's)
        np.testing.assert_array_equal(m["covariances"][live], f["covariances"][live])
    _check_members(keys, out, pairs, f"cap {cap}", need_converged=False)


def _floating_chain():
    """Two chains of three poses tied by ONE range between the robots: the second chain can still turn about the range's end
    on it, so J'J is singular along a direction that moves its poses (the graph of tests/test_relative_gpu.py)."""
    fg = make_manhattan(n_robots=2, n_poses=3, n_beacons=0, seed=3, p_range=1.0)
    assert len(fg.range_measurements) == 3
    fg.range_measurements = fg.range_measurements[:1]
    return fg


def test_singular_member_is_a_verdict_for_that_member_only(hip_lib):
    fg = _floating_chain()
    results = plain_noisy_truth(fg)
    prob, point = _problem_and_point(fg, results, None, None)
    lam = np.linalg.eigvalsh(dense_information(prob, point))
    assert abs(lam[0]) <= 1e-9 * lam[-1] < lam[1]  # one null direction
    tw = member_twin("C")
    ids = rh.pair_list(tw.ref.prob, 3)
    bad_names = [("A1", "B1"), ("B2", "A0")]
    bad_ids = np.array([[1, 4], [5, 0]], dtype=np.int32)
    with RefineBatchHandle([prob, tw.ref.prob], hip_lib) as h:
        rc, (bad, good), info = h.relative_covariances([point, tw.ref.point], [bad_ids, ids], max_iters=64)
        missed = int(np.count_nonzero(~bad["converged"]))
        assert rc == 1 and bad["rc"] == 1 and missed >= 1 and info["unconverged"] == missed and good["rc"] == 0
        rh.check_relative(tw.ref, ids, good, "C beside the singular member")
        # a later call on a healthy group (the singular member lists nothing)
        rc, (none, later), info = h.relative_covariances([point, tw.ref.point], [None, ids])
        assert rc == 0 and info["unconverged"] == 0 and none["covariances"].shape == (0, 3, 3)
        rh.check_relative(tw.ref, ids, later, "C after the singular call")
    with _handle(("C",), hip_lib) as h:
        _, (alone,), _ = h.relative_covariances([tw.ref.point], [ids], max_iters=64)
    same_bits(alone, good, "C alone against C beside the singular member", keys=OUTPUTS)
    with pytest.raises(RuntimeError, match=r"predicted_relative_poses_batch: graph 1: \d of 6 columns did not converge"
                                           r".*information_spectrum\(\.\.\.\)\.undetermined\(\)"):
        predicted_relative_poses_batch([tw.fg, fg], [tw.results, results], [_names(tw.ref.prob, ids), bad_names], max_iters=64,
                                       lib_path=hip_lib)


def test_errors_are_reported_not_faults(hip_lib):
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    keys = ("C", "B")
    tws = [member_twin(k) for k in keys]
    probs = [t.ref.prob for t in tws]
    arrays = [_point_arrays(t.ref.prob, t.ref.point) for t in tws]
    poses = np.ascontiguousarray(np.concatenate([a[0].ravel() for a in arrays]))
    lms = np.ascontiguousarray(np.concatenate([a[1].ravel() for a in arrays]))
    assert probs[0].Nl > 0
    good = dict(ptr=[0, 1, 3], pa=[1, 0, 2], pb=[0, 3, probs[1].Np - 1])
    who = "score_refine_batch_relative_covariances: "
    arr = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    p = lambda v, kind: None if v is None or not v.size else v.ctypes.data_as(kind)  # noqa: E731

    def call(h, lib, ptr, pa, pb, rel_tol=1e-10, max_iters=4000, width=16, with_points=True):
        ptr, pa, pb = arr(ptr), arr(pa), arr(pb)
        info = ScoreMarginalsBatchInfo()
        rc = lib.score_refine_batch_relative_covariances(h, p(poses, f64) if with_points else None, p(lms, f64), p(ptr, i32), p(pa, i32),
                                                         p(pb, i32), rel_tol, max_iters, width, None, None, None, None, None, C.byref(info))
        return rc, lib.score_last_error().decode(), info

    with RefineBatchHandle(probs, hip_lib) as h:
        lib = bind(h.lib, RELATIVE_BATCH)
        for what, kw in (
            ("null handle", dict(good, h=None)),
            ("the points are missing", dict(good, h=h.h, with_points=False)),
            ("member 1: a pair joins a pose to itself", dict(good, h=h.h, pb=[0, 0, probs[1].Np - 1])),
            ("member 0: a pair's pose is out of range (a landmark has no relative pose)", dict(good, h=h.h, pb=[probs[0].Np, 3, 4])),
            ("member 1: a pair's pose is out of range (a landmark has no relative pose)", dict(good, h=h.h, pb=[0, 3, probs[1].Np])),
            ("member 0: a pair's pose is out of range", dict(good, h=h.h, pa=[-1, 0, 2])),
            ("pair_ptr must start at 0", dict(good, h=h.h, ptr=[1, 1, 3])),
            ("pair_ptr must not decrease", dict(good, h=h.h, ptr=[0, 3, 1])),
            ("pairs without their lists", dict(good, h=h.h, pa=None)),
            ("pairs without their lists", dict(good, h=h.h, pb=None)),
            ("block_width must be 1..16", dict(good, h=h.h, width=0)),
            ("block_width must be 1..16", dict(good, h=h.h, width=17)),
            ("rel_tol must be positive", dict(good, h=h.h, rel_tol=0.0)),
            ("rel_tol must be positive", dict(good, h=h.h, rel_tol=-1e-10)),
            ("max_iters >= 1", dict(good, h=h.h, max_iters=0)),
        ):
            rc, msg, _ = call(lib=lib, **kw)
            print(what, "->", rc, msg)
            assert rc < 0 and what in msg and msg.startswith(who), (what, rc, msg)
            # ... and the handle still works after every one of them
            rc, msg, info = call(h.h, lib, **good)
            assert rc == 0 and info.columns == 9 and info.unconverged == 0 and info.passes == 1, (what, rc, msg)
        # nothing listed: no work, no error
        for kw in (dict(good, ptr=[0, 0, 0], pa=None, pb=None), dict(good, ptr=None, pa=None, pb=None), dict(good, ptr=None)):
            rc, msg, info = call(h.h, lib, **kw)
            assert rc == 0 and info.columns == 0 and info.passes == 0 and info.pcg_iters == 0, msg
        rc, members, info = h.relative_covariances([t.ref.point for t in tws], [None, []])
        assert rc == 0 and info["columns"] == 0 and all(m["covariances"].shape == (0, 3, 3) and m["rc"] == 0 for m in members)
        ids = rh.pair_list(probs[0], 2)
        rc, (c_out, _), _ = h.relative_covariances([t.ref.point for t in tws], [ids, None])
        rh.check_relative(tws[0].ref, ids, c_out, "C after the errors")


def test_end_to_end(hip_lib):
    keys = ("A", "C", "B")
    tws = [member_twin(k) for k in keys]
    fgs, results = [t.fg for t in tws], [t.results for t in tws]
    rws, lws = [], []
    for fg in fgs:
        w = np.ones(len(fg.range_measurements))
        w[::5], w[3::7] = 0.25, 0.0
        rws.append(w)
        n_lc = len(fg.loop_closure_measurements)
        lws.append(np.where(np.arange(n_lc) % 2 == 1, 0.5, 1.0) if n_lc else None)
    assert all(np.any(w == 0.0) and np.any(w == 0.25) for w in rws) and any(lw is not None and np.any(lw == 0.5) for lw in lws)
    refs = [rh.WeightedReference(fg, res, w, lw) for fg, res, w, lw in zip(fgs, results, rws, lws)]
    ids = [rh.pair_list(refs[0].prob, 6), None, rh.pair_list(refs[2].prob, 2)]
    names = [_names(r.prob, i) if i is not None else [] for r, i in zip(refs, ids)]
    out = predicted_relative_poses_batch(fgs, results, names, range_weights=rws, loop_closure_weights=lws, lib_path=hip_lib)
    host = predicted_relative_poses_batch(fgs, results, names, range_weights=rws, loop_closure_weights=lws, engine="python")
    with RefineBatchHandle([r.prob for r in refs], hip_lib) as h:
        rc, raw, rec = h.relative_covariances([r.point for r in refs], ids)
    assert rc == 0 and rec["passes"] == 2
    kappa, tau = 4.0, 9.0
    for k, ref, i, nm, (pred, info), (hp, hinfo), m in zip(keys, refs, ids, names, out, host, raw):
        assert isinstance(pred, PredictedRelativePoses) and pred.pairs == nm and info["engine"] == "device" and hinfo["engine"] == "python"
        assert info["group"] == 0 and info["passes"] == 2 and info["batches"] == -(-3 * len(nm) // 16)
        np.testing.assert_array_equal(pred.covariance, 0.5 * (m["covariances"] + np.swapaxes(m["covariances"], 1, 2)))
        np.testing.assert_array_equal(pred.rotation, m["rotations"])
        np.testing.assert_array_equal(pred.translation, m["translations"])
        np.testing.assert_array_equal(info["residuals"], m["residuals"])
        np.testing.assert_array_equal(info["iterations"], m["iterations"])
        if not nm:
            assert pred.covariance.shape == (0, 3, 3) and hp.pairs == [] and info["asymmetry"] == 0.0
            continue
        want, bound = rh.check_relative(ref, i, m, f"{k} under weights, in (A, C, B)")
        sym_want, sym_bound = 0.5 * (want + np.swapaxes(want, 1, 2)), 0.5 * (bound + np.swapaxes(bound, 1, 2))
        np.testing.assert_array_equal(hp.covariance, sym_want)  # (the python engine is dense_covariances' computation)
        assert np.all(np.abs(pred.covariance - hp.covariance) <= sym_bound)
        assert info["asymmetry"] <= 2 * bound.max() + np.abs(want - np.swapaxes(want, 1, 2)).max()
        # the gate of the host's prediction on the device's, bounded as in tests/test_relative_gpu.py
        d2, dof = pred.gate(list(zip(hp.rotation, hp.translation)), kappa, tau)
        e_max = 2 * rh.JAC_ULPS * rh.EPS * (1.0 + np.abs(hp.translation).max() * 2)
        assert dof == 3 and np.all(d2 <= 3 * e_max ** 2 * max(2 * tau, kappa))


def test_refine_estimate_batch_with_relative(hip_lib):
    """refine_estimate_batch(relative=...) returns the refinement it returns without the keyword, bit for bit, and the
    predictions of the two-step use (run, then the relative covariances at the refined points on the same handle)."""
    keys = ("B", "C", "E")
    fgs, starts = group(keys)
    probs, first = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, starts)])
    ids = [rh.pair_list(probs[0], 3), None, rh.pair_list(probs[2], 6)]
    names = [_names(p, i) if i is not None else None for p, i in zip(probs, ids)]
    with RefineBatchHandle(probs, hip_lib) as h:
        refined, _ = h.run(list(first))
        rc, raw, rec = h.relative_covariances(refined, ids)
    assert rc == 0 and rec["passes"] == 2
    out = refine_estimate_batch(fgs, starts, lib_path=hip_lib, relative=names)
    plain = refine_estimate_batch(fgs, starts, lib_path=hip_lib)
    for nm, m, (res_r, info), (res_p, info_p) in zip(names, raw, out, plain):
        pred, pinfo = info["relative"]
        assert isinstance(pred, PredictedRelativePoses) and pred.pairs == (nm or []) and pinfo["passes"] == 2 and pinfo["engine"] == "device"
        np.testing.assert_array_equal(pred.covariance, 0.5 * (m["covariances"] + np.swapaxes(m["covariances"], 1, 2)))
        np.testing.assert_array_equal(pred.rotation, m["rotations"])
        np.testing.assert_array_equal(pred.translation, m["translations"])
        np.testing.assert_array_equal(pinfo["residuals"], m["residuals"])
        assert "relative" not in info_p and info["cost_final"] == info_p["cost_final"] and info["iterations"] == info_p["iterations"]
        for name in res_p.poses:
            np.testing.assert_array_equal(res_r.poses[name], res_p.poses[name])
        for name in res_p.landmarks:
            np.testing.assert_array_equal(res_r.landmarks[name], res_p.landmarks[name])
