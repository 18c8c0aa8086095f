"""Batched range leverage and predicted range variances on the device (score_refine_batch_leverage,
score_refine_batch_range_variances, csrc/score_leverage_batch.hpp).

Every member of every group is judged as tests/test_leverage_gpu.py judges a single graph: its six sums against
``expected_sums`` from the DEVICE's own steps (those of ``RefineBatchHandle.samples`` with the same seeds on the same handle:
the draws are the same bit for bit, which test 1 holds first), NumPy's J and NumPy's noise, under the bounds derived in
tests/leverage_helpers.py; its range variances under ``check_range_variances``.  No tolerance is chosen here.

The group A..E (tests/refine_batch_helpers.py, at the host-refined points) has 306, 119, 27, 461 and 113 measurements: A and D
span two 256-lane workgroups with a partly filled second one, C is less than one wave between larger members.  The pair
counts [5, 0, 3, 260, 1] end the pair kernel's first workgroup inside D's list, its lanes crossing three members."""
import ctypes as C
import functools

import numpy as np
import pytest

from leverage_helpers import SUMS, THINNED, check_range_variances, check_sums, expected_sums, pair_list, thinned_twin
from marginals_helpers import graph_a, undetermined_graph
from marginals_helpers import noisy_truth as plain_noisy_truth
from refine_batch_helpers import KEYS_2D, group, rough_start
from samples_batch_helpers import group_draws, member_twin, same_bits, seed_of
from samples_helpers import weighted_twin
from score_amd.bindings import LEVERAGE_BATCH, ScoreMarginalsBatchInfo, ScoreSamplesBatchInfo, bind
from score_amd.leverage import Leverage, LeverageHandle, measurement_counts, pair_ids
from score_amd.leverage_batch import predicted_range_variances_batch, range_leverage_batch
from score_amd.marginals import _problem_and_point, _select
from score_amd.refine_batch import RefineBatchHandle, _problem_of, refine_estimate_batch
from score_amd.refine_robust import _point_arrays

pytestmark = pytest.mark.gpu

KEYS_3D = ("3D0", "3D1")
COUNTS = [17, 5, 0, 16, 1]
PAIRS = [5, 0, 3, 260, 1]
RV_PAIRS = [17, 0, 1, 16, 3]
ALL = SUMS + ("pair_sum", "pair_sq")
DRAWS = ("residuals", "iterations", "converged", "determined")
LEV_OUTPUTS = ALL + DRAWS + ("rc",)
RV_OUTPUTS = ("variances", "distances", "residuals", "iterations", "converged", "rc")


def _handle(keys, hip_lib):
    return RefineBatchHandle([member_twin(k).ref.prob for k in keys], hip_lib)


def _points(keys):
    return [member_twin(k).ref.point for k in keys]


def _pairs(keys, counts, **kw):
    return [pair_list(member_twin(k).ref.prob, c, **kw) if c else None for k, c in zip(keys, counts)]


def _seeds(keys):
    return [seed_of(k) for k in keys]


def _leverage(h, keys, pairs, n_samples, **kw):
    return h.leverage(_points(keys), pairs, n_samples, _seeds(keys), **kw)


@functools.lru_cache(maxsize=None)
def a_to_e(hip_lib):
    """The calls on the group A..E, on one handle, shared by the tests below and left unchanged."""
    pairs = _pairs(KEYS_2D, PAIRS)
    no_c = [p if s else None for p, s in zip(pairs, COUNTS)]  # (a member without draws may list no pair)
    rv_pairs = _pairs(KEYS_2D, RV_PAIRS)
    with _handle(KEYS_2D, hip_lib) as h:
        out = dict(pairs=pairs, rv_pairs=rv_pairs,
                   samples=group_draws(h, KEYS_2D, 17),
                   wide=_leverage(h, KEYS_2D, pairs, 17),
                   sixteen=_leverage(h, KEYS_2D, pairs, 16),
                   narrow=_leverage(h, KEYS_2D, no_c, COUNTS, block_width=4),
                   narrow_samples=group_draws(h, KEYS_2D, COUNTS, block_width=4),
                   last=_leverage(h, KEYS_2D, pairs, 1, first_sample=16),
                   again=_leverage(h, KEYS_2D, pairs, 17),
                   rv=h.range_variances(_points(KEYS_2D), rv_pairs),
                   rv3=h.range_variances(_points(KEYS_2D), rv_pairs, block_width=3))
    return out


def _check_member(key, out, smp, ids, n_samples, label, first_sample=0, keep=None):
    """check_sums of member `key`: the sums `out` against the steps of the samples call `smp` over the draws `keep`."""
    tw = member_twin(key)
    z = tw.noise(seed_of(key), first_sample, n_samples)
    steps = smp["steps"]
    if keep is not None:
        steps, z = steps[keep], z[keep]
    has = ids is not None and len(ids) > 0
    return check_sums(tw, out, steps, z, ids if has else None, label, keys=ALL if has else SUMS)


def test_same_draws_as_the_group_samples(hip_lib):
    runs = a_to_e(hip_lib)
    (rc_s, smp, info_s), (rc, lev, info) = runs["samples"], runs["wide"]
    assert rc == rc_s == 0 and info["passes"] == info_s["passes"] == 2 and info["pcg_iters"] == info_s["pcg_iters"]
    for f in ("members", "samples", "unconverged", "singular", "max_residual"):
        assert info[f] == info_s[f], f
    for k, a, b in zip(KEYS_2D, lev, smp):
        same_bits(a, b, f"{k}: leverage against samples", keys=DRAWS)
    assert [sum(measurement_counts(member_twin(k).ref.prob)) for k in KEYS_2D] == [306, 119, 27, 461, 113]


def test_sums_under_the_bound(hip_lib):
    runs = a_to_e(hip_lib)
    (_, smp, _), (_, lev, _) = runs["samples"], runs["wide"]
    assert [0 if p is None else len(p) for p in runs["pairs"]] == PAIRS
    nonzero = {k: False for k in ALL}
    for key, out, s, ids, count in zip(KEYS_2D, lev, smp, runs["pairs"], PAIRS):
        assert out["pair_sum"].shape == out["pair_sq"].shape == (count,)
        _check_member(key, out, s, ids, 17, f"{key} in A..E, 17 draws, {count} pairs")
        for k in ALL:
            nonzero[k] = nonzero[k] or bool(np.any(out[k] != 0))
    assert all(nonzero.values()), nonzero


def test_different_counts_at_width_four(hip_lib):
    runs = a_to_e(hip_lib)
    (rc, narrow, info), (_, wide, _), (_, sixteen, _), (rc1, last, info1), (_, again, info2) = (
        runs[k] for k in ("narrow", "wide", "sixteen", "last", "again"))
    smp = runs["samples"][1]
    assert rc == 0 and info["passes"] == 5 and info["samples"] == sum(COUNTS) and info["unconverged"] == 0
    for key, S, out4, s4, ids in zip(KEYS_2D, COUNTS, narrow, runs["narrow_samples"][1], runs["pairs"]):
        M = sum(measurement_counts(member_twin(key).ref.prob))
        assert all(out4[k].shape == (M,) for k in SUMS) and out4["residuals"].shape == (S,)
        if S == 0:  # C takes no part and no room
            assert out4["determined"] == -1 and not any(np.any(out4[k]) for k in SUMS) and out4["pair_sum"].shape == (0,)
            continue
        assert out4["determined"] == 1 and out4["info"]["batches"] == -(-S // 4)
        same_bits(out4, s4, f"{key}: leverage against samples at width 4", keys=DRAWS)
        _check_member(key, out4, s4, ids, S, f"{key}, {S} draws at width 4")
    # no sum depends on block_width: equal counts, equal bits (A: the 17-draw call, D: the 16-draw call)
    for k in ALL:
        np.testing.assert_array_equal(narrow[0][k], wide[0][k], err_msg=f"A: {k}")
        np.testing.assert_array_equal(narrow[3][k], sixteen[3][k], err_msg=f"D: {k}")
    # draw 16 alone against what the 17-draw and the 16-draw runs imply, within the bound of the 17-draw sums
    assert rc1 == 0 and info1["passes"] == 1 and info1["samples"] == 5
    for key, full, part, one, s, ids in zip(KEYS_2D, wide, sixteen, last, smp, runs["pairs"]):
        tw = member_twin(key)
        has = ids is not None
        _, bound = expected_sums(tw, s["steps"], tw.noise(seed_of(key), 0, 17), ids if has else None)
        for k in (ALL if has else SUMS):
            assert np.all(np.abs((full[k] - part[k]) - one[k]) <= bound[k]), (key, k)
        assert np.any(one["lev_sum"] != 0)
    # a second identical call gives the same bits
    for key, a, b in zip(KEYS_2D, wide, again):
        same_bits(a, b, f"{key}: the second identical call", keys=LEV_OUTPUTS)
    assert info2["pcg_iters"] == runs["wide"][2]["pcg_iters"]


def test_a_member_alone_equals_the_member_in_the_group_bit_for_bit(hip_lib):
    runs = a_to_e(hip_lib)
    wide = runs["wide"][1]
    for k in ("B", "D"):
        g = KEYS_2D.index(k)
        with _handle((k,), hip_lib) as h:
            rc1, (alone,), info1 = _leverage(h, (k,), [runs["pairs"][g]], 17)
        assert rc1 == 0 and info1["passes"] == 2
        same_bits(alone, wide[g], f"{k} alone against {k} in A..E", keys=LEV_OUTPUTS)


@pytest.mark.parametrize("key", ["A", "D"])
def test_against_the_single_handle(hip_lib, key):
    """Both sides are held to expected_sums from their own steps; the two sums then differ by at most the two bounds plus
    the difference of the two expectations (the two iterations' steps differ within their solves' residuals)."""
    runs = a_to_e(hip_lib)
    g = KEYS_2D.index(key)
    tw, ids = member_twin(key), runs["pairs"][g]
    out, smp = runs["wide"][1][g], runs["samples"][1][g]
    with LeverageHandle(tw.ref.prob, hip_lib) as h:
        single = h.leverage(tw.ref.point, ids, 17, seed=seed_of(key))
        single_smp = h.draw(tw.ref.point, tw.ids, 17, seed=seed_of(key))
    assert single["rc"] == 0
    z = tw.noise(seed_of(key), 0, 17)
    _, want_g, bound_g = check_sums(tw, out, smp["steps"], z, ids, f"{key} in A..E")
    _, want_s, bound_s = check_sums(tw, single, single_smp["steps"], z, ids, f"{key} on a single handle")
    for k in ALL:
        allowed = bound_g[k] + bound_s[k] + np.abs(want_g[k] - want_s[k])
        assert np.all(np.abs(out[k] - single[k]) <= allowed), k


@pytest.mark.parametrize("keys", [("b", "C"), ("c", "C")])
def test_long_contribution_list_and_join_level(hip_lib, keys):
    """b: 599 measurements, 300 lanes on one beacon (the long contribution list); c: 1774 measurements over 7 workgroups, the
    join level of the chain kernel."""
    pairs = _pairs(keys, [5, 3])
    with _handle(keys, hip_lib) as h:
        rc_s, smp, _ = group_draws(h, keys, 16)
        rc, lev, info = _leverage(h, keys, pairs, 16)
    assert rc == rc_s == 0 and info["passes"] == 1
    assert sum(measurement_counts(member_twin(keys[0]).ref.prob)) == {"b": 599, "c": 1774}[keys[0]]
    for k, out, s, ids in zip(keys, lev, smp, pairs):
        same_bits(out, s, f"{k} in {keys}", keys=DRAWS)
        _check_member(k, out, s, ids, 16, f"{k} in {keys}, 16 draws")


def test_3d_group(hip_lib):
    pairs = _pairs(KEYS_3D, [5, 5])
    with _handle(KEYS_3D, hip_lib) as h:
        rc_s, smp, _ = group_draws(h, KEYS_3D, 17)
        rc, lev, info = _leverage(h, KEYS_3D, pairs, 17)
        rrc, rv, rinfo = h.range_variances(_points(KEYS_3D), pairs)
    assert rc == rc_s == 0 and info["passes"] == 2 and info["samples"] == 34
    for k, out, s, ids in zip(KEYS_3D, lev, smp, pairs):
        same_bits(out, s, f"{k}", keys=DRAWS)
        _check_member(k, out, s, ids, 17, f"{k}, 17 draws")
    assert rrc == 0 and rinfo["columns"] == 10 and rinfo["passes"] == 1
    for k, out, ids in zip(KEYS_3D, rv, pairs):
        check_range_variances(member_twin(k), ids, out, f"{k}, 5 pairs")


def test_unconverged_draws_stay_out_of_the_sums(hip_lib):
    keys = ("A", "C")
    pairs = _pairs(keys, [5, 3])
    with _handle(keys, hip_lib) as h:
        _, full, _ = _leverage(h, keys, pairs, 6, block_width=4)
        cap = max(int(m["iterations"].max()) for m in full) - 1
        rc, lev, info = _leverage(h, keys, pairs, 6, block_width=4, max_iters=cap)
        rc_s, smp, _ = group_draws(h, keys, 6, block_width=4, max_iters=cap)
    missed = sum(int(np.count_nonzero(~m["converged"])) for m in lev)
    print(f"(A, C), 6 draws, cap {cap}: converged {[m['converged'].tolist() for m in lev]}")
    assert rc == rc_s == 1 and info["unconverged"] == missed and 0 < missed < 12
    for k, out, s, f, ids in zip(keys, lev, smp, full, pairs):
        np.testing.assert_array_equal(out["converged"], s["converged"])
        np.testing.assert_array_equal(out["converged"], f["iterations"] <= cap)
        assert out["rc"] == (0 if np.all(out["converged"]) else 1)
        _check_member(k, out, s, ids, 6, f"{k}, cap {cap}", keep=out["converged"])


def test_singular_member_is_a_verdict_for_that_member_only(hip_lib):
    fg = undetermined_graph()  # one range fixes the landmark's distance only: H is singular
    results = plain_noisy_truth(fg)
    prob, point = _problem_and_point(fg, results, None, None)
    tw = member_twin("C")
    ids = pair_list(tw.ref.prob, 3)
    points, seeds = [point, tw.ref.point], [5, seed_of("C")]
    with RefineBatchHandle([prob, tw.ref.prob], hip_lib) as h:
        rc, (bad, good), info = h.leverage(points, [None, ids], 3, seeds, max_iters=64)
        _, (_, smp), _ = h.samples(points, [_select(prob, None)[1], tw.ids], 3, seeds, max_iters=64)
        assert rc == 1 and bad["determined"] == 0 and bad["rc"] == 1 and not np.any(bad["converged"])
        assert info["singular"] == 1 and info["unconverged"] == 3
        assert all(np.all(bad[k] == 0) for k in SUMS)
        # C is untouched by its neighbour: fully converged and under its bounds in the same call
        assert good["determined"] == 1 and good["rc"] == 0
        _check_member("C", good, smp, ids, 3, "C beside the singular member")
        # a well-posed call on the same handle afterwards: the singular member draws nothing
        rc, (none, good), info = h.leverage(points, [None, ids], [0, 3], seeds)
        _, (_, smp), _ = h.samples(points, [[], tw.ids], [0, 3], seeds)
        assert rc == 0 and none["determined"] == -1 and info["singular"] == 0 and info["samples"] == 3
        _check_member("C", good, smp, ids, 3, "C after the singular call")
    with pytest.raises(RuntimeError, match=r"range_leverage_batch: graph 0: 3 of 3 draws did not converge.*undetermined\(\)"):
        range_leverage_batch([fg, tw.fg], [results, tw.results], n_samples=3, max_iters=64, lib_path=hip_lib)


def test_range_weights(hip_lib):
    fg = graph_a()
    results = plain_noisy_truth(fg)
    w = np.ones(len(fg.range_measurements))
    w[::3] = 0.0
    tw, c = weighted_twin(fg, results, w), member_twin("C")
    prob = tw.ref.prob
    ids, seeds = pair_list(prob, 5), [11, seed_of("C")]
    points = [tw.ref.point, c.ref.point]
    with RefineBatchHandle([prob, c.ref.prob], hip_lib) as h:
        rc, (lev, lev_c), _ = h.leverage(points, [ids, None], 16, seeds)
        _, (smp, smp_c), _ = h.samples(points, [tw.ids, c.ids], 16, seeds)
    assert rc == 0
    z = tw.noise(11, 0, 16)
    _, want, bound = check_sums(tw, lev, smp["steps"], z, ids, "a, a third of the ranges off, beside C")
    _check_member("C", lev_c, smp_c, None, 16, "C beside the weighted graph")
    n_rel, n_rng, _ = measurement_counts(prob)
    off = n_rel + np.flatnonzero(w == 0)
    assert np.all(lev["lev_sum"][off] == 0) and np.all(lev["lev_sq"][off] == 0) and np.all(bound["lev_sum"][off] == 0)
    first_row = tw.J.shape[0] - n_rng - 2  # (the ranges' rows: one each, before the prior's two)
    z2 = np.sum(z[:, first_row + np.flatnonzero(w == 0)] ** 2, axis=0)
    assert np.all(np.abs(lev["red_sum"][off] - z2) <= bound["red_sum"][off])


def test_range_variances(hip_lib):
    runs = a_to_e(hip_lib)
    (rc, wide, info), (rc3, narrow, info3), pairs = runs["rv"], runs["rv3"], runs["rv_pairs"]
    assert rc == rc3 == 0 and info["columns"] == info3["columns"] == sum(RV_PAIRS) and info["passes"] == 2 and info3["passes"] == 6
    assert info["unconverged"] == 0
    for key, count, a, b, ids in zip(KEYS_2D, RV_PAIRS, wide, narrow, pairs):
        assert a["variances"].shape == (count,) and a["info"]["columns"] == count
        if count == 0:
            continue
        check_range_variances(member_twin(key), ids, a, f"{key} in A..E, {count} pairs")
        check_range_variances(member_twin(key), ids, b, f"{key} in A..E, {count} pairs, width 3")
    # against the single handle through the reference they share; a member alone against the member in the group
    for key in ("A", "D"):
        g = KEYS_2D.index(key)
        tw = member_twin(key)
        with LeverageHandle(tw.ref.prob, hip_lib) as h:
            check_range_variances(tw, pairs[g], h.range_variances(tw.ref.point, pairs[g], with_solutions=True), f"{key} on a single handle")
        with _handle((key,), hip_lib) as h:
            rc1, (alone,), info1 = h.range_variances([tw.ref.point], [pairs[g]])
        assert rc1 == 0 and info1["passes"] == -(-RV_PAIRS[g] // 16)
        same_bits(alone, wide[g], f"{key} alone against {key} in A..E", keys=RV_OUTPUTS)
    keys = ("b", "C")
    on_beacon = [pair_list(member_twin("b").ref.prob, 16, on_first_landmark=True), None]
    with _handle(keys, hip_lib) as h:
        rc, (b_out, c_out), info = h.range_variances(_points(keys), on_beacon)
        assert rc == 0 and info["passes"] == 1 and c_out["variances"].shape == (0,)
        check_range_variances(member_twin("b"), on_beacon[0], b_out, "b beside C, 16 pairs on the one beacon")
        rc, members, info = h.range_variances(_points(keys), [None, []])
        assert rc == 0 and info["columns"] == 0 and info["passes"] == 0 and all(m["variances"].shape == (0,) for m in members)


def test_handle_state_survives(hip_lib):
    """run, leverage and range variances at the refined points, run from other starts: the second run and the marginals equal
    a fresh handle's bit for bit; refine_estimate_batch(leverage=8) returns the sums of the two-step use and the refinement
    it returns without the keyword."""
    keys = ("B", "C", "E")
    fgs, starts = group(keys)
    probs, first = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, starts)])
    second = [_problem_of(fg, rough_start(k), None, None)[1] for k, fg in zip(keys, fgs)]
    ids = [_select(p, None)[1] for p in probs]
    with RefineBatchHandle(probs, hip_lib) as h:
        refined, _ = h.run(list(first))
        rc, lev, linfo = h.leverage(refined, [None] * 3, 8, [3, 4, 5])
        rrc, _, _ = h.range_variances(refined, [pair_list(p, 3) for p in probs])
        assert rc == 0 and rrc == 0
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
    out = refine_estimate_batch(fgs, starts, lib_path=hip_lib, leverage=8, leverage_seed=3)
    plain = refine_estimate_batch(fgs, starts, lib_path=hip_lib)
    for p, m, (res_l, info), (res_p, info_p) in zip(probs, lev, out, plain):
        got, li = info["leverage"]
        n_rel, n_rng, _ = measurement_counts(p)
        assert isinstance(got, Leverage) and got.count == 8 and li["passes"] == linfo["passes"] == 1 and li["determined"] == 1
        np.testing.assert_array_equal(got.leverage, m["lev_sum"][n_rel : n_rel + n_rng] / 8)
        np.testing.assert_array_equal(got.redundancy, m["red_sum"][n_rel : n_rel + n_rng] / 8)
        np.testing.assert_array_equal(li["residuals"], m["residuals"])
        assert "leverage" not in info_p and info["cost_final"] == info_p["cost_final"] and info["iterations"] == info_p["iterations"]
        for nm in res_p.poses:
            np.testing.assert_array_equal(res_l.poses[nm], res_p.poses[nm])
        for nm in res_p.landmarks:
            np.testing.assert_array_equal(res_l.landmarks[nm], res_p.landmarks[nm])


def test_end_to_end(hip_lib):
    tw, c = thinned_twin(), member_twin("C")
    out = range_leverage_batch([tw.fg, c.fg], [tw.results, c.results], n_samples=16, seed=7, lib_path=hip_lib)
    (lev, info), (lev_c, info_c) = out
    others = np.delete(lev.redundancy, THINNED)
    print(f"thinned beside C: redundancy of the two {lev.redundancy[THINNED]}, the others >= {others.min():.3f}")
    assert info["engine"] == "device" and lev.count == lev_c.count == 16 and info["group"] == info_c["group"] == 0 and info["passes"] == 1
    assert lev.uncontrolled().tolist() == THINNED and np.all(lev.redundancy[THINNED] < 1e-6)
    pairs = [("A10", "L1"), ("A10", "A3"), ("A0", "L0")]
    (pred, pinfo), (none, ninfo) = predicted_range_variances_batch([tw.fg, c.fg], [tw.results, c.results], [pairs, []], lib_path=hip_lib)
    assert pred.pairs == pairs and pinfo["engine"] == "device" and pinfo["batches"] == 1 and none.pairs == [] and none.variance.shape == (0,)
    got = {"rc": 0, "converged": np.ones(3, dtype=bool), "variances": pred.variance, "distances": pred.distance,
           "residuals": pinfo["residuals"], "iterations": pinfo["iterations"]}
    check_range_variances(tw, pair_ids(tw.ref.prob, pairs, "test"), got, "thinned beside C, by name")


def test_errors_are_reported_not_faults(hip_lib):
    i32, f64, u64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    keys = ("C", "B")
    tws = [member_twin(k) for k in keys]
    probs = [t.ref.prob for t in tws]
    arrays = [_point_arrays(t.ref.prob, t.ref.point) for t in tws]
    poses = np.ascontiguousarray(np.concatenate([a[0].ravel() for a in arrays]))
    lms = np.ascontiguousarray(np.concatenate([a[1].ravel() for a in arrays]))
    top_c = probs[0].Np + probs[0].Nl
    good = dict(ptr=[0, 1, 3], pa=[1, 0, 2], pb=[probs[0].Np, 3, probs[1].Np], counts=[2, 3], seeds=[1, 2])
    arr = lambda v, t: None if v is None else np.ascontiguousarray(v, dtype=t)  # noqa: E731
    p = lambda v, kind: None if v is None or not v.size else v.ctypes.data_as(kind)  # noqa: E731

    def call(h, lib, ptr, pa, pb, counts, seeds, first=0, rel_tol=1e-10, max_iters=4000, width=16):
        ptr, pa, pb, counts, seeds = arr(ptr, np.int32), arr(pa, np.int32), arr(pb, np.int32), arr(counts, np.int32), arr(seeds, np.uint64)
        info = ScoreSamplesBatchInfo()
        rc = lib.score_refine_batch_leverage(h, p(poses, f64), p(lms, f64), p(seeds, u64), first, p(counts, i32), p(ptr, i32), p(pa, i32),
                                             p(pb, i32), rel_tol, max_iters, width, None, None, None, None, None, None, None, None, None,
                                             C.byref(info))
        return rc, lib.score_last_error().decode(), info

    def columns(h, lib, ptr, pa, pb, rel_tol=1e-10, max_iters=4000, width=16, **_):
        ptr, pa, pb = arr(ptr, np.int32), arr(pa, np.int32), arr(pb, np.int32)
        info = ScoreMarginalsBatchInfo()
        rc = lib.score_refine_batch_range_variances(h, p(poses, f64), p(lms, f64), p(ptr, i32), p(pa, i32), p(pb, i32), rel_tol, max_iters,
                                                    width, None, None, None, None, C.byref(info))
        return rc, lib.score_last_error().decode(), info

    with RefineBatchHandle(probs, hip_lib) as h:
        lib = bind(h.lib, LEVERAGE_BATCH)
        for what, kw, both in (
            ("null handle", dict(good, h=None), True),
            ("seeds is null", dict(good, h=h.h, seeds=None), False),
            ("n_samples is null", dict(good, h=h.h, counts=None), False),
            ("zero for every member", dict(good, h=h.h, ptr=[0, 0, 0], counts=[0, 0]), False),
            ("n_samples is negative", dict(good, h=h.h, counts=[2, -1]), False),
            ("must start at 0", dict(good, h=h.h, ptr=[1, 1, 3]), True),
            ("must not decrease", dict(good, h=h.h, ptr=[0, 3, 1]), True),
            ("joins a variable to itself", dict(good, h=h.h, pb=[1, 3, probs[1].Np]), True),
            ("out of range", dict(good, h=h.h, pb=[top_c, 3, probs[1].Np]), True),
            ("out of range", dict(good, h=h.h, pa=[-1, 0, 2]), True),
            ("without draws", dict(good, h=h.h, counts=[0, 3]), False),
            ("block_width", dict(good, h=h.h, width=0), True),
            ("block_width", dict(good, h=h.h, width=17), True),
            ("rel_tol", dict(good, h=h.h, rel_tol=0.0), True),
            ("max_iters", dict(good, h=h.h, max_iters=0), True),
            ("first_sample", dict(good, h=h.h, first=-1), False),
            ("first_sample", dict(good, h=h.h, first=2 ** 32 - 2), False),
        ):
            rc, msg, _ = call(lib=lib, **kw)
            print(what, "->", rc, msg)
            assert rc < 0 and what in msg and "score_refine_batch_leverage" in msg, (what, rc, msg)
            if both:
                rc, msg, _ = columns(lib=lib, **kw)
                assert rc < 0 and what in msg and "score_refine_batch_range_variances" in msg, (what, rc, msg)
            # ... and the handle still works after every one of them
            rc, msg, info = call(h.h, lib, **good)
            assert rc == 0 and info.samples == 5 and info.unconverged == 0 and info.passes == 1 and info.members == 2, (what, rc, msg)
            rc, msg, cinfo = columns(h.h, lib, **good)
            assert rc == 0 and cinfo.columns == 3 and cinfo.unconverged == 0 and cinfo.passes == 1, (what, rc, msg)
        # no pairs for anyone
        rc, msg, info = call(h.h, lib, **dict(good, ptr=None, pa=None, pb=None))
        assert rc == 0 and info.samples == 5, msg
        rc, (c_out, _), _ = _leverage(h, keys, [pair_list(probs[0], 3), None], [2, 0])
        _, (c_smp, _), _ = group_draws(h, keys, [2, 0])
        _check_member("C", c_out, c_smp, pair_list(probs[0], 3), 2, "C after the errors")
