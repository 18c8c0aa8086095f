"""Predicted relative poses and their covariances on the device (score_refine_relative_covariances, csrc/score_relative.hpp)
through the C ABI, against NumPy's Jacobian and the dense Cholesky solve, under the bounds derived in
tests/relative_helpers.py.

Shapes: graph a (2-D, two chains of 25, loop closures and a prior), b (300 poses on one chain), d (3-D).  1, 5 and 6 pairs in
2-D are 3, 15 and 18 columns, 1, 2 and 3 pairs in 3-D 6, 12 and 18: below a block of 16, and past it with a pair that straddles
the block edge (columns 15 .. 17 of pair 5 in 2-D, 12 .. 17 of pair 2 in 3-D).  Every list of two pairs or more has pose 0 once
as a and once as b (a list of one pair: as a)."""
import ctypes as C
import functools

import numpy as np
import pytest

import relative_helpers as rh
from marginals_helpers import noisy_truth, reference
from score_amd.bindings import ScoreMarginalsInfo, ptr
from score_amd.leverage import pair_ids
from score_amd.manhattan import make_manhattan
from score_amd.marginals import _problem_and_point, dense_information
from score_amd.refine import _point_arrays, unknown_sizes
from score_amd.refine_robust import refine_estimate_robust
from score_amd.relative import RelativeHandle, predicted_relative_poses
from score_amd.solver import _i32p

pytestmark = pytest.mark.gpu

COUNTS = {"a": (1, 5, 6), "b": (1, 5, 6), "d": (1, 2, 3)}
OUTPUTS = ("rotations", "translations", "covariances", "residuals", "iterations", "converged")


@functools.lru_cache(maxsize=None)
def _six_pairs_of_a(hip_lib):
    """graph a, 6 pairs (18 columns), width 16, with the solutions: shared by the tests below and left unchanged."""
    _, _, ref = reference("a")
    ids = rh.pair_list(ref.prob, 6)
    with RelativeHandle(ref.prob, hip_lib) as h:
        out = h.relative_covariances(ref.point, ids, with_solutions=True)
    return ids, out


@pytest.mark.parametrize("key", ["a", "b", "d"])
def test_covariances_against_the_dense_solve(hip_lib, key):
    _, _, ref = reference(key)
    prob = ref.prob
    _, dp = unknown_sizes(prob)
    with RelativeHandle(prob, hip_lib) as h:
        for count in COUNTS[key]:
            ids = rh.pair_list(prob, count)
            out = h.relative_covariances(ref.point, ids, with_solutions=True)
            assert out["info"]["columns"] == count * dp and out["info"]["batches"] == (count * dp + 15) // 16
            assert out["info"]["unconverged"] == 0 and out["covariances"].shape == (count, dp, dp)
            rh.check_relative(ref, ids, out, f"{key}, {count} pairs")
            assert ids[0, 0] == 0 and (count == 1 or ids[1, 1] == 0)  # the fixed first pose as a, and as b
            assert np.all(np.linalg.eigvalsh(0.5 * (out["covariances"] + np.swapaxes(out["covariances"], 1, 2))) > 0)
    assert max(c * dp for c in COUNTS[key]) == 18  # (past a block, the last pair across its edge)


def test_block_widths(hip_lib):
    """Widths 3, 5 and 1 against 16 on graph a: the same bounds, ceil(18 / width) blocks.  The outputs are bit-equal where the
    lock-step iteration is column-independent; whether it is, the ranges' call shows first on the same handle."""
    _, _, ref = reference("a")
    ids, wide = _six_pairs_of_a(hip_lib)
    rng_ids = np.array([[3, 30], [0, 12], [40, 7], [5, ref.prob.Np], [ref.prob.Np + 1, 20]], dtype=np.int32)
    with RelativeHandle(ref.prob, hip_lib) as h:
        r16 = h.range_variances(ref.point, rng_ids)
        independent = all(np.array_equal(r16[k], h.range_variances(ref.point, rng_ids, block_width=w)[k])
                          for w in (3, 1) for k in ("variances", "residuals", "iterations"))
        print(f"the ranges' call gives equal bits under widths 16, 3, 1: {independent}")
        for width in (3, 5, 1):
            out = h.relative_covariances(ref.point, ids, block_width=width, with_solutions=True)
            assert out["info"]["columns"] == 18 and out["info"]["batches"] == -(-18 // width)
            rh.check_relative(ref, ids, out, f"a, 6 pairs, width {width}")
            same = all(np.array_equal(out[k], wide[k]) for k in OUTPUTS + ("solutions",))
            print(f"a, 6 pairs: width {width} gives the bits of width 16: {same}")
            if independent:
                for k in OUTPUTS + ("solutions",):
                    np.testing.assert_array_equal(out[k], wide[k], err_msg=f"width {width}, {k}")


def test_two_calls_and_a_call_after_the_others(hip_lib):
    _, _, ref = reference("a")
    ids, first = _six_pairs_of_a(hip_lib)
    with RelativeHandle(ref.prob, hip_lib) as h:
        one = h.relative_covariances(ref.point, ids, with_solutions=True)
        two = h.relative_covariances(ref.point, ids, with_solutions=True)
        rv = h.range_variances(ref.point, [(3, 30), (0, ref.prob.Np)])
        lev = h.leverage(ref.point, [(3, 30)], 3, seed=7)
        three = h.relative_covariances(ref.point, ids, with_solutions=True)
    assert rv["rc"] == 0 and lev["rc"] == 0
    for k in OUTPUTS + ("solutions",):
        np.testing.assert_array_equal(one[k], two[k], err_msg=k)
        np.testing.assert_array_equal(one[k], three[k], err_msg=k)
        np.testing.assert_array_equal(one[k], first[k], err_msg=k)  # (and on another handle)
    assert one["info"]["pcg_iters"] == three["info"]["pcg_iters"] == first["info"]["pcg_iters"]


def test_a_long_lever_arm(hip_lib):
    """b, one chain of 300: the relative pose of the ends is far less certain than that of two neighbours, in every block of
    the error coordinates -- a wrong sign between the two ends' columns would cancel the chain's drift or double a step's."""
    _, _, ref = reference("b")
    ids = np.array([[1, 299], [150, 151], [299, 1]], dtype=np.int32)
    with RelativeHandle(ref.prob, hip_lib) as h:
        out = h.relative_covariances(ref.point, ids, with_solutions=True)
    want, _ = rh.check_relative(ref, ids, out, "b, the ends and two neighbours")
    P = out["covariances"]
    tr = np.trace(P, axis1=1, axis2=2)
    print(f"b: trace P of (1, 299) {tr[0]:.4f}, of (150, 151) {tr[1]:.6f}, of (299, 1) {tr[2]:.4f}")
    assert tr[0] > tr[1] and tr[2] > tr[1] and P[0, 0, 0] > P[1, 0, 0] and P[2, 0, 0] > P[1, 0, 0]
    assert np.all(tr > 0) and np.all(want[:, 0, 0] > 0)
    # the heading's variance does not depend on the direction of the pair: the same bound holds both ways
    assert abs(P[0, 0, 0] - P[2, 0, 0]) <= abs(want[0, 0, 0] - want[2, 0, 0]) + 2 * np.abs(P[[0, 2], 0, 0] - want[[0, 2], 0, 0]).max()


def test_the_library_refuses_bad_arguments(hip_lib):
    _, _, ref = reference("a")
    prob = ref.prob
    who = "score_refine_relative_covariances: "
    bad = [([(3, 3)], "a pair joins a pose to itself"), ([(3, prob.Np)], "a pair's pose is out of range"),
           ([(-1, 4)], "a pair's pose is out of range"), ([(4, prob.Np + prob.Nl)], "a pair's pose is out of range")]
    with RelativeHandle(prob, hip_lib) as h:
        for ids, words in bad:
            with pytest.raises(RuntimeError, match=who + ".*" + words):
                h.relative_covariances(ref.point, ids)
        with pytest.raises(RuntimeError, match=who + "block_width must be 1..16"):
            h.relative_covariances(ref.point, [(3, 4)], block_width=17)
        with pytest.raises(RuntimeError, match=who + "block_width must be 1..16"):
            h.relative_covariances(ref.point, [(3, 4)], block_width=0)
        # n_pairs < 0 and pairs without their lists: the raw call
        poses, lms = _point_arrays(prob, ref.point)
        pa = np.array([3], dtype=np.int32)
        info = ScoreMarginalsInfo()
        for args, words in (((ptr(pa, _i32p), ptr(pa, _i32p), -1), "n_pairs must be >= 0"),
                            ((None, ptr(pa, _i32p), 1), "n_pairs pairs without their lists"),
                            ((ptr(pa, _i32p), None, 1), "n_pairs pairs without their lists")):
            rc = h.lib.score_refine_relative_covariances(h.h, ptr(poses), ptr(lms), *args, 1e-10, 4000, 16, None, None, None, None, None,
                                                         None, C.byref(info))
            assert rc < 0 and h.lib.score_last_error().decode() == who + words
        none = h.relative_covariances(ref.point, np.zeros((0, 2), dtype=np.int32))  # (no pairs: nothing to do, no error)
        assert none["rc"] == 0 and none["info"]["columns"] == 0 and none["info"]["batches"] == 0 and none["info"]["pcg_iters"] == 0
        ids = rh.pair_list(prob, 2)
        rh.check_relative(ref, ids, h.relative_covariances(ref.point, ids, with_solutions=True), "a, after the refusals")


def test_iteration_cap(hip_lib):
    """Under max_iters = max(steps) - 1 the columns beyond the cap report -(cap + 1), the call returns 1, `unconverged`
    counts them, and the columns that converged are within their bounds."""
    _, _, ref = reference("a")
    ids = rh.pair_list(ref.prob, 6)
    with RelativeHandle(ref.prob, hip_lib) as h:
        full = h.relative_covariances(ref.point, ids, block_width=4)
        steps = full["iterations"]
        cap = int(steps.max()) - 1
        out = h.relative_covariances(ref.point, ids, block_width=4, max_iters=cap, with_solutions=True)
    keep = out["converged"]
    print(f"a, 18 columns, cap {cap}: steps {steps.ravel().tolist()}, converged {keep.ravel().tolist()}")
    assert full["rc"] == 0 and out["rc"] == 1 and 0 < np.count_nonzero(keep) < keep.size
    assert out["info"]["unconverged"] == int(np.count_nonzero(~keep))
    np.testing.assert_array_equal(keep, steps <= cap)
    assert np.all(out["iterations"][~keep] == cap)  # (reported by the call as -(cap + 1))
    np.testing.assert_array_equal(out["iterations"][keep], steps[keep])
    rh.check_relative(ref, ids, out, f"a, cap {cap}", need_converged=False)


def test_end_to_end_with_the_weights_of_a_robust_result(hip_lib):
    fg, start, _ = reference("a")
    nr = len(fg.range_measurements)
    prior = np.ones(nr)
    prior[::5], prior[3::7] = 0.25, 0.0
    results, info = refine_estimate_robust(fg, start, robust_loop_closures=True, engine="python", linear_solver="scipy",
                                           range_weights=prior, loop_closure_weights=np.array([1.0, 0.5, 1.0]))
    w, wl = info["robust"]["weights"], info["robust"]["loop_closure_weights"]
    assert np.any(w == 0.0) and np.any(w == 0.25) and np.any(wl == 0.5)
    pairs = [("A10", "B7"), ("A0", "B20"), ("B3", "A0"), ("A11", "A12"), ("B24", "A1"), ("B2", "B19")]
    pred, pinfo = predicted_relative_poses(fg, results, pairs, range_weights=w, loop_closure_weights=wl, lib_path=hip_lib)
    host, hinfo = predicted_relative_poses(fg, results, pairs, range_weights=w, loop_closure_weights=wl, engine="python")
    assert pinfo["engine"] == "device" and hinfo["engine"] == "python" and pinfo["batches"] == 2 and pred.pairs == pairs
    ref = rh.WeightedReference(fg, results, w, wl)
    ids = pair_ids(ref.prob, pairs, "test")
    # the public function symmetrises: the raw call on the same problem gives what it was formed from, held by the bounds
    with RelativeHandle(ref.prob, hip_lib) as h:
        raw = h.relative_covariances(ref.point, ids)
    want, bound = rh.check_relative(ref, ids, raw, "a under a robust result's weights")
    np.testing.assert_array_equal(pred.covariance, 0.5 * (raw["covariances"] + np.swapaxes(raw["covariances"], 1, 2)))
    np.testing.assert_array_equal(pred.rotation, raw["rotations"])
    np.testing.assert_array_equal(pinfo["residuals"], raw["residuals"])
    # the Python engine is rh.dense_covariances' computation -- the same H, G and Cholesky solve -- symmetrised
    sym_want, sym_bound = 0.5 * (want + np.swapaxes(want, 1, 2)), 0.5 * (bound + np.swapaxes(bound, 1, 2))
    np.testing.assert_array_equal(host.covariance, sym_want)
    assert np.all(np.abs(pred.covariance - host.covariance) <= sym_bound)
    assert pinfo["asymmetry"] <= 2 * bound.max() + np.abs(want - np.swapaxes(want, 1, 2)).max()
    # and the weights matter: the unweighted covariances differ by far more than the bounds
    plain, _ = predicted_relative_poses(fg, results, pairs, engine="python")
    assert np.abs(plain.covariance - host.covariance).max() > 100 * sym_bound.max()
    # the gate of the host's prediction on the device's: an innovation of the two sides' rounding (JAC_ULPS eps of the terms of
    # t_ab and of the rotation's entries, the arctangent's few eps), so d2 <= dp |e|_max^2 |(P + N)^-1| <= 3 |e|_max^2 max(2 tau, kappa)
    kappa, tau = 4.0, 9.0
    d2, dof = pred.gate(list(zip(host.rotation, host.translation)), kappa, tau)
    e_max = 2 * rh.JAC_ULPS * rh.EPS * (1.0 + np.abs(host.translation).max() * 2)
    assert dof == 3 and np.all(d2 <= 3 * e_max ** 2 * max(2 * tau, kappa))


def _floating_chain():
    """Two chains of three poses tied by ONE range between the robots: the second chain can still turn about the range's end
    on it, so J'J is singular along a direction that moves its poses."""
    fg = make_manhattan(n_robots=2, n_poses=3, n_beacons=0, seed=3, p_range=1.0)
    assert len(fg.range_measurements) == 3
    fg.range_measurements = fg.range_measurements[:1]
    return fg


def test_singular_information_raises_and_the_library_goes_on(hip_lib):
    """marginals_helpers.undetermined_graph has a single pose, so no pair of poses; the graph here is singular in the same way
    along pose directions."""
    fg = _floating_chain()
    results = noisy_truth(fg)
    prob, point = _problem_and_point(fg, results, None, None)
    lam = np.linalg.eigvalsh(dense_information(prob, point))
    assert abs(lam[0]) <= 1e-9 * lam[-1] < lam[1]  # one null direction
    with pytest.raises(RuntimeError, match=r"of 6 columns did not converge.*information_spectrum\(\.\.\.\)\.undetermined\(\)"):
        predicted_relative_poses(fg, results, [("A1", "B1"), ("B2", "A0")], max_iters=64, lib_path=hip_lib)
    _, _, ref = reference("a")
    ids = rh.pair_list(ref.prob, 2)
    with RelativeHandle(ref.prob, hip_lib) as h:
        rh.check_relative(ref, ids, h.relative_covariances(ref.point, ids, with_solutions=True), "a, after the singular graph")
