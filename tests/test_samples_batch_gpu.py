"""Batched posterior samples on the device (score_refine_batch_samples, csrc/score_samples_batch.hpp).

Every member of every group is judged as tests/test_samples_gpu.py judges a single graph: its noise against the NumPy
restatement of the stream of ITS seed, its right-hand sides against J'z from the host Jacobian, its steps against the dense
Cholesky solve, under the bounds derived in tests/samples_helpers.py -- every term comes from the member's reference, the
library's own reported residual and the number format; no tolerance is chosen.  Two device results are compared through the
reference they share: by the sum of their two bounds.

The group A..E (tests/refine_batch_helpers.py, at the host-refined points) meets the boundaries of the device code: C (37
unknowns, less than one tile) sits between larger members, 17 draws at width 16 give a second pass with one live slot
(NV = 1), the counts [17, 5, 0, 16, 1] at width 4 let the members drop out at different passes and leave one out altogether.
No member of A..E has a contribution list beyond 128 entries; graph b beside C brings the long list, graph c the join level
of the chain kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

from marginals_helpers import check_iteration_caps, undetermined_graph
from marginals_helpers import noisy_truth as plain_noisy_truth
from refine_batch_helpers import KEYS_2D, group, rough_start
from samples_batch_helpers import DISTRIBUTION_SEED, group_draws, member_twin, same_bits, seed_of, solve_bound
from samples_helpers import EPS, NOISE_ATOL, check_distribution, check_noise, check_rhs, check_solve, dims, fixed_order_moments
from score_amd.marginals import _problem_and_point, _select
from score_amd.refine_batch import RefineBatchHandle, _problem_of, refine_estimate_batch
from score_amd.refine_robust import _point_arrays
from score_amd.samples import SamplesHandle
from score_amd.samples_batch import ScoreSamplesBatchInfo, _bind, posterior_samples_batch

pytestmark = pytest.mark.gpu

KEYS_3D = ("3D0", "3D1")
COUNTS = [17, 5, 0, 16, 1]


def _handle(keys, hip_lib):
    return RefineBatchHandle([member_twin(k).ref.prob for k in keys], hip_lib)


@functools.lru_cache(maxsize=None)
def a_to_e(hip_lib):
    """The calls on the group A..E, on one handle, shared by the tests below and left unchanged: 17 draws at width 16 (twice),
    the counts [17, 5, 0, 16, 1] at width 4, draw 16 alone."""
    with _handle(KEYS_2D, hip_lib) as h:
        wide = group_draws(h, KEYS_2D, 17)
        narrow = group_draws(h, KEYS_2D, COUNTS, block_width=4)
        last = group_draws(h, KEYS_2D, 1, first_sample=16)
        again = group_draws(h, KEYS_2D, 17)
    return dict(wide=wide, narrow=narrow, last=last, again=again)


@functools.lru_cache(maxsize=None)
def three_d(hip_lib):
    with _handle(KEYS_3D, hip_lib) as h:
        return group_draws(h, KEYS_3D, 17)


def _under_bounds(key, out, label, first_sample=0):
    tw = member_twin(key)
    z = check_noise(tw, out, seed_of(key), first_sample, label)
    b_py = check_rhs(tw, out, z, label)
    check_solve(tw, out, b_py, label)
    return b_py


def test_group_of_five_two_passes(hip_lib):
    rc, members, info = a_to_e(hip_lib)["wide"]
    assert rc == 0 and info["passes"] == 2 and info["members"] == 5 and info["samples"] == 5 * 17
    assert info["unconverged"] == 0 and info["singular"] == 0
    for k, out in zip(KEYS_2D, members):
        _under_bounds(k, out, f"{k} in A..E, 17 draws")
        assert out["determined"] == 1 and out["info"]["passes"] == 2 and out["info"]["batches"] == 2
    assert member_twin("C").ref.n == 37 < 64  # less than one tile, between larger members
    assert len(set(seed_of(k) for k in KEYS_2D)) == 5


def test_different_counts_at_width_four(hip_lib):
    runs = a_to_e(hip_lib)
    (rc, narrow, info), (_, wide, _), (rc1, last, info1) = runs["narrow"], runs["wide"], runs["last"]
    assert rc == 0 and info["passes"] == 5 and info["samples"] == sum(COUNTS) and info["unconverged"] == 0
    for k, S, out4, out16, one in zip(KEYS_2D, COUNTS, narrow, wide, last):
        tw = member_twin(k)
        assert out4["steps"].shape == (S, tw.ref.n) and out4["rhs"].shape == (S, tw.ref.n) and out4["residuals"].shape == (S,)
        if S == 0:  # C takes no part and no room: its neighbours B and D are checked bit for bit below
            assert out4["determined"] == -1 and out4["noise"].shape[0] == 0 and not np.any(out4["moments"]) and not np.any(out4["means"])
            continue
        assert out4["determined"] == 1 and out4["info"]["batches"] == -(-S // 4)
        b_py = _under_bounds(k, out4, f"{k}, {S} draws at width 4")
        # a draw does not depend on the call it is part of: noise and right-hand sides of the common draws, bit for bit
        np.testing.assert_array_equal(out4["noise"], out16["noise"][:S])
        np.testing.assert_array_equal(out4["rhs"], out16["rhs"][:S])
        # the steps of the two widths through the reference they share
        cut = {f: out16[f][:S] for f in ("rhs", "residuals")}
        allowed = solve_bound(tw, out4, b_py) + solve_bound(tw, cut, b_py)
        diff = np.linalg.norm(out4["steps"] - out16["steps"][:S], axis=1)
        print(f"{k}: width 4 against width 16: worst step difference / allowed = {float(np.max(diff / allowed)):.3e}")
        assert np.all(diff <= allowed)
    assert rc1 == 0 and info1["passes"] == 1 and info1["samples"] == 5
    for k, one, out16 in zip(KEYS_2D, last, wide):
        np.testing.assert_array_equal(one["noise"][0], out16["noise"][16], err_msg=k)
        np.testing.assert_array_equal(one["rhs"][0], out16["rhs"][16], err_msg=k)


def test_a_member_alone_equals_the_member_in_the_group_bit_for_bit(hip_lib):
    runs = a_to_e(hip_lib)
    (rc, wide, info), (rc2, again, info2) = runs["wide"], runs["again"]
    assert rc == rc2 == 0
    for k, a, b in zip(KEYS_2D, wide, again):
        same_bits(a, b, f"{k}: the second identical call")
    assert info["pcg_iters"] == info2["pcg_iters"]
    for k in ("B", "D"):
        with _handle((k,), hip_lib) as h:
            rc1, (alone,), info1 = group_draws(h, (k,), 17)
        assert rc1 == 0 and info1["passes"] == 2
        same_bits(alone, wide[KEYS_2D.index(k)], f"{k} alone against {k} in A..E")


@pytest.mark.parametrize("key", ["A", "D"])
def test_against_the_single_handle(hip_lib, key):
    tw = member_twin(key)
    out = a_to_e(hip_lib)["wide"][1][KEYS_2D.index(key)]
    with SamplesHandle(tw.ref.prob, hip_lib) as h:
        single = h.draw(tw.ref.point, tw.ids, 17, seed=seed_of(key), with_rhs=True, with_noise=True)
    assert single["rc"] == 0
    z = tw.noise(seed_of(key), 0, 17)
    b_py = tw.rhs(z)
    worst_z = float(np.max(np.abs(out["noise"] - single["noise"])))
    rhs_allowed = 2 * tw.rhs_bound(z)
    worst_b = float(np.max(np.abs(out["rhs"] - single["rhs"]) / rhs_allowed))
    allowed = solve_bound(tw, out, b_py) + solve_bound(tw, single, b_py)
    diff = np.linalg.norm(out["steps"] - single["steps"], axis=1)
    print(f"{key}: group against single handle: noise {worst_z:.3e}, rhs / allowed {worst_b:.3e}, steps / allowed "
          f"{float(np.max(diff / allowed)):.3e}")
    assert worst_z <= NOISE_ATOL
    assert np.all(np.abs(out["rhs"] - single["rhs"]) <= rhs_allowed)
    assert np.all(diff <= allowed)


def test_long_contribution_list_beside_a_small_member(hip_lib):
    keys = ("b", "C")
    assert member_twin("b").longest_column > 128
    assert all(member_twin(k).longest_column <= 128 for k in KEYS_2D)
    with _handle(keys, hip_lib) as h:
        rc, members, info = group_draws(h, keys, 16)
    assert rc == 0 and info["passes"] == 1
    for k, out in zip(keys, members):
        _under_bounds(k, out, f"{k} in (b, C)")


def test_join_level_inside_a_union(hip_lib):
    """One chain of 1100 poses (the second level of score_join.hpp, applied to all vectors of the pass) beside C."""
    keys = ("c", "C")
    with _handle(keys, hip_lib) as h:
        rc, members, info = group_draws(h, keys, 16)
    assert rc == 0 and info["passes"] == 1
    for k, out in zip(keys, members):
        _under_bounds(k, out, f"{k} in (c, C)")


def test_3d_group(hip_lib):
    rc, members, info = three_d(hip_lib)
    assert rc == 0 and info["passes"] == 2 and info["samples"] == 34
    for k, out in zip(KEYS_3D, members):
        _under_bounds(k, out, f"{k}, 17 draws")
        assert out["determined"] == 1


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_moments_are_the_sums_of_the_members_steps(hip_lib, which):
    keys, (_, members, _) = (KEYS_2D, a_to_e(hip_lib)["wide"]) if which == "2d" else (KEYS_3D, three_d(hip_lib))
    S = 17
    for k, out in zip(keys, members):
        tw = member_twin(k)
        M, mean, absM, absmean = fixed_order_moments(dims(tw.ref.prob), out["steps"])
        print(f"{k}: worst |moments - sums| / ((S + 1) eps sum |terms|) = "
              f"{float(np.max(np.abs(out['moments'] - M) / ((S + 1) * EPS * absM + np.finfo(np.float64).tiny))):.3e}")
        assert out["moments"].shape == M.shape and np.all(np.abs(out["moments"] - M) <= (S + 1) * EPS * absM)
        assert out["means"].shape == mean.shape and np.all(np.abs(out["means"] - mean) <= (S + 1) * EPS * absmean)
        assert np.any(out["moments"] != 0) and np.any(out["means"] != 0)


def test_iteration_cap_at_the_chunk_boundaries(hip_lib):
    """check_iteration_caps of tests/marginals_helpers.py on (A, C), 6 draws each at width 4: the draws within the cap are the
    full run's bit for bit, the others report -(cap + 1) and are left out of that member's moments."""
    keys = ("A", "C")
    kept = {}

    def run(cap):
        rc, members, info = group_draws(h, keys, 6, max_iters=cap, block_width=4)
        kept[cap] = (members, info)
        return rc, [(m["steps"].T, m["residuals"], m["iterations"], m["converged"]) for m in members]

    with _handle(keys, hip_lib) as h:
        top = check_iteration_caps(run, "(A, C), 6 draws, width 4")
    members, info = kept[top - 1]
    missed = sum(int(np.count_nonzero(~m["converged"])) for m in members)
    assert info["unconverged"] == missed > 0 and info["singular"] == 0
    for k, m in zip(keys, members):
        tw = member_twin(k)
        assert m["rc"] == (0 if np.all(m["converged"]) else 1)
        M, mean, absM, absmean = fixed_order_moments(dims(tw.ref.prob), m["steps"][m["converged"]])
        assert np.all(np.abs(m["moments"] - M) <= (6 + 1) * EPS * absM) and np.all(np.abs(m["means"] - mean) <= (6 + 1) * EPS * absmean)


def test_singular_member_is_a_verdict_for_that_member_only(hip_lib):
    fg = undetermined_graph()  # one range fixes the landmark's distance only: H is singular
    results = plain_noisy_truth(fg)
    prob, point = _problem_and_point(fg, results, None, None)
    ids = _select(prob, None)[1]
    tw = member_twin("C")
    points, all_ids, seeds = [point, tw.ref.point], [ids, tw.ids], [5, seed_of("C")]
    with RefineBatchHandle([prob, tw.ref.prob], hip_lib) as h:
        rc, (bad, good), info = h.samples(points, all_ids, 3, seeds, max_iters=64, with_rhs=True, with_noise=True)
        print("singular member:", info, bad["iterations"], bad["converged"], bad["residuals"])
        assert rc == 1 and bad["determined"] == 0 and bad["rc"] == 1 and not np.any(bad["converged"])
        assert info["singular"] == 1 and info["unconverged"] == 3
        assert not np.any(bad["moments"]) and not np.any(bad["means"])
        # C is untouched by its neighbour: fully converged and under its bounds in the same call
        assert good["determined"] == 1 and good["rc"] == 0
        _under_bounds("C", good, "C beside the singular member")
        with pytest.raises(RuntimeError, match=r"posterior_samples_batch: graph 0: 3 of 3 draws did not converge.*undetermined\(\)"):
            posterior_samples_batch([fg, tw.fg], [results, tw.results], n_samples=3, max_iters=64, lib_path=hip_lib)
        # a well-posed call on the same handle afterwards: the singular member draws nothing
        rc, (none, good), info = h.samples(points, all_ids, [0, 3], seeds, with_rhs=True, with_noise=True)
        assert rc == 0 and none["determined"] == -1 and info["singular"] == 0 and info["samples"] == 3
        _under_bounds("C", good, "C after the singular call")


def test_handle_state_survives_the_samples(hip_lib):
    """run, samples at the refined points, run from other starts: the second run equals a fresh handle's bit for bit; the
    marginals after the samples equal a fresh handle's; refine_estimate_batch(samples=8) returns the draws of the two-step
    use and the refinement it returns without the keyword."""
    keys = ("B", "C", "E")
    fgs, starts = group(keys)
    probs, first = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, starts)])
    second = [_problem_of(fg, rough_start(k), None, None)[1] for k, fg in zip(keys, fgs)]
    sels = [_select(p, None) for p in probs]
    ids = [s[1] for s in sels]
    with RefineBatchHandle(probs, hip_lib) as h:
        refined, _ = h.run(list(first))
        rc, draws, sinfo = h.samples(refined, ids, 8, [3, 4, 5])
        assert rc == 0
        _, cols, _ = h.marginals(refined, ids)
        pts, infos = h.run(second)
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
    out = refine_estimate_batch(fgs, starts, lib_path=hip_lib, samples=8, samples_seed=3)
    plain = refine_estimate_batch(fgs, starts, lib_path=hip_lib)
    for (names, _, size, _), m, (res_s, info), (res_p, info_p) in zip(sels, draws, out, plain):
        smp, si = info["samples"]
        assert si["order"] == names and smp.count == 8 and si["passes"] == sinfo["passes"] == 1 and si["determined"] == 1
        off = np.concatenate([[0], np.cumsum(size)])
        for j, nm in enumerate(names):
            np.testing.assert_array_equal(smp.steps[nm], m["steps"][:, off[j]:off[j + 1]])
        np.testing.assert_array_equal(si["residuals"], m["residuals"])
        np.testing.assert_array_equal(smp._moments, m["moments"])
        # ... and the refinement itself is what it is without the keyword
        assert "samples" not in info_p and info["cost_final"] == info_p["cost_final"] and info["iterations"] == info_p["iterations"]
        for nm in names:
            src = res_s.landmarks if nm in res_s.landmarks else res_s.poses
            ref = res_p.landmarks if nm in res_p.landmarks else res_p.poses
            np.testing.assert_array_equal(src[nm], ref[nm])


@pytest.mark.parametrize("keys", [("B", "E"), ("3D0",)])
def test_distribution(hip_lib, keys):
    tws = [member_twin(k) for k in keys]
    out = posterior_samples_batch([t.fg for t in tws], [t.results for t in tws], n_samples=64, seed=DISTRIBUTION_SEED,
                                  variables=[t.names for t in tws], lib_path=hip_lib)
    for k, tw, (smp, info) in zip(keys, tws, out):
        delta = np.concatenate([smp.steps[nm] for nm in tw.names], axis=1)
        assert info["passes"] == 4 and info["batches"] == 4 and info["engine"] == "device" and delta.shape == (64, tw.ref.n)
        check_distribution(tw, delta, smp.covariance, f"{k}, device")


def test_errors_are_reported_not_faults(hip_lib):
    i32, f64, u64 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    keys = ("C", "B")
    tws = [member_twin(k) for k in keys]
    probs = [t.ref.prob for t in tws]
    arrays = [_point_arrays(t.ref.prob, t.ref.point) for t in tws]
    poses = np.ascontiguousarray(np.concatenate([a[0].ravel() for a in arrays]))
    lms = np.ascontiguousarray(np.concatenate([a[1].ravel() for a in arrays]))
    lm_c = probs[0].Np  # C's first landmark, member-local
    good = dict(ptr=[0, 1, 3], ids=[lm_c, 3, probs[1].Np], counts=[2, 3], seeds=[1, 2])

    def call(h, lib, ptr, ids, counts, seeds, first=0, rel_tol=1e-10, max_iters=4000, width=16):
        arr = lambda v, t: None if v is None else np.ascontiguousarray(v, dtype=t)  # noqa: E731
        ptr, ids, counts, seeds = arr(ptr, np.int32), arr(ids, np.int32), arr(counts, np.int32), arr(seeds, np.uint64)
        p = lambda v, kind: None if v is None or not v.size else v.ctypes.data_as(kind)  # noqa: E731
        info = ScoreSamplesBatchInfo()
        rc = lib.score_refine_batch_samples(h, p(poses, f64), p(lms, f64), p(seeds, u64), first, p(counts, i32), p(ptr, i32), p(ids, i32),
                                            rel_tol, max_iters, width, None, None, None, None, None, None, None, None, C.byref(info))
        return rc, lib.score_last_error().decode(), info

    with RefineBatchHandle(probs, hip_lib) as h:
        lib = _bind(h.lib)
        for what, kw in (
            ("null handle", dict(good, h=None)),
            ("seeds is null", dict(good, h=h.h, seeds=None)),
            ("n_samples is null", dict(good, h=h.h, counts=None)),
            ("var_ptr is null", dict(good, h=h.h, ptr=None)),
            ("zero for every member", dict(good, h=h.h, counts=[0, 0])),
            ("n_samples is negative", dict(good, h=h.h, counts=[2, -1])),
            ("pose 0", dict(good, h=h.h, ptr=[0, 1, 2], ids=[lm_c, 0])),
            ("twice", dict(good, h=h.h, ids=[lm_c, 3, 3])),
            ("out of range", dict(good, h=h.h, ptr=[0, 1, 2], ids=[probs[0].Np + probs[0].Nl, 3])),
            ("out of range", dict(good, h=h.h, ptr=[0, 1, 2], ids=[-1, 3])),
            ("must start at 0", dict(good, h=h.h, ptr=[1, 1, 3])),
            ("must not decrease", dict(good, h=h.h, ptr=[0, 3, 1])),
            ("block_width", dict(good, h=h.h, width=0)),
            ("block_width", dict(good, h=h.h, width=17)),
            ("rel_tol", dict(good, h=h.h, rel_tol=0.0)),
            ("rel_tol", dict(good, h=h.h, rel_tol=-1.0)),
            ("max_iters", dict(good, h=h.h, max_iters=0)),
            ("first_sample", dict(good, h=h.h, first=-1)),
            ("first_sample", dict(good, h=h.h, first=2 ** 32 - 2)),
        ):
            rc, msg, _ = call(lib=lib, **kw)
            print(what, "->", rc, msg)
            assert rc < 0 and what in msg, (what, rc, msg)
            # ... and the handle still draws after every one of them
            rc, msg, info = call(h.h, lib, **good)
            assert rc == 0 and info.samples == 5 and info.unconverged == 0 and info.passes == 1 and info.members == 2, (what, rc, msg)
        # the last index of the counter is a draw like any other
        rc, msg, info = call(h.h, lib, **dict(good, first=2 ** 32 - 3))
        assert rc == 0 and info.samples == 5, msg
        rc, (c_out, _), _ = group_draws(h, keys, [2, 0])
        _under_bounds("C", c_out, "C after the errors")
