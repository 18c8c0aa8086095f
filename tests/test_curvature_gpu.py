"""The second-order check on the device (include/score_curvature.h): the product with E and with J'J, the lowest eigenpairs
of E, what a curvature call leaves of the handle, and the argument errors.  The reference and the bounds are
curvature_helpers'."""
import numpy as np
import pytest

import curvature_helpers as ch
from curvature_helpers import EPS, MAX_ITERS, REL_TOL, SHIFT
from marginals_helpers import two_pose_graph
from score_amd.curvature import Curvature, CurvatureHandle, hessian_spectrum
from score_amd.marginals import _problem_and_point, _select

pytestmark = pytest.mark.gpu


def _block_of_vectors(n):
    """16 columns: 8 unit columns spread over the unknowns (the first and the last among them), 8 seeded uniform ones."""
    V = np.zeros((n, 16))
    V[np.linspace(0, n - 1, 8).astype(np.int64), np.arange(8)] = 1.0
    V[:, 8:] = np.random.default_rng(11).uniform(-1.0, 1.0, size=(n, 8))
    return V


@pytest.mark.parametrize("key", ch.DENSE_CASES)
def test_product_with_E_and_with_JtJ(hip_lib, key):
    fg, results, ref = ch.reference(key)
    ch.check_input_conditions(key, ref)
    V = _block_of_vectors(ref.n)
    with CurvatureHandle(ref.prob) as h:
        exact = h.product(ref.point, V, exact=True)
        plain = h.product(ref.point, V, exact=False)
        one = h.product(ref.point, V[:, 9], exact=True)
        seven = h.product(ref.point, V[:, 5:12], exact=True)
        again = h.product(ref.point, V, exact=True)
    bound = (ref.longest_row + ref.c) * EPS * (ref.B @ np.abs(V))
    for label, got, want in (("E V", exact, ref.E @ V), ("(J'J) V", plain, ref.JtJ @ V)):
        err = np.abs(got - want)
        ratio = float(np.max(err[bound > 0] / bound[bound > 0]))
        print(f"{key}: {label}: n = {ref.n}, longest row {ref.longest_row}, c = {ref.c}, worst |difference| / bound = {ratio:.3e}")
        assert np.all(err <= bound), f"{key}: {label}: worst entry at {ratio:.3e} of its bound"
    assert np.max(np.abs(exact - plain)) > 0.0
    # fewer columns: the bits of the same columns at 16; and two calls give the same bits
    assert one.shape == (ref.n,) and np.array_equal(one, exact[:, 9])
    assert np.array_equal(seven, exact[:, 5:12])
    assert np.array_equal(again, exact)


def _gn_quotient_bound(ref, V, sigma):
    """|device v'(J'J)v - host v'(J'J)v|: the product's rounding (longest row + c) eps |v|'(|J|'|J|)|v| with c the entry's
    contributions (at most longest row again) + 128, the dot's n eps of the same, and the shift taken out again: a few eps sigma;
    both sides."""
    _, J = ref.prob.residuals(ref.point, jac=True)
    Ja = abs(J)
    mass = np.einsum("ij,ij->j", Ja @ np.abs(V), Ja @ np.abs(V))
    return 2.0 * (2 * ref.longest_row + 128 + ref.n + 8) * EPS * (mass + sigma)


@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("key", ch.ALL_CASES)
def test_lowest_eigenpairs_of_E(hip_lib, key, k):
    fg, results, ref = ch.reference(key)
    ch.check_input_conditions(key, ref)
    cur, info = hessian_spectrum(fg, results, k=k, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT)
    print(key, "k =", k, info)
    assert isinstance(cur, Curvature)
    assert info["engine"] == "device" and info["unconverged"] == 0 and 1 <= info["iterations"] <= MAX_ITERS
    assert abs(info["h_max"] - ref.h_max) <= (ref.n + 1) * EPS * ref.h_max and info["shift"] == SHIFT * info["h_max"]
    ch.check_pairs(ref, k, cur.values, cur.vectors, REL_TOL, f"{key}, k = {k}")
    # the Gauss-Newton quotients
    want = np.einsum("ij,ij->j", cur.vectors, ref.Hs @ cur.vectors)
    bound = _gn_quotient_bound(ref, cur.vectors, info["shift"])
    print(f"{key}: gauss_newton {cur.gauss_newton[:3]}, worst |difference| / bound = {np.max(np.abs(cur.gauss_newton - want) / bound):.3e}")
    assert np.all(np.abs(cur.gauss_newton - want) <= bound), (cur.gauss_newton, want, bound)
    # c_max: the largest entry of |E - J'J|, each side a sum of at most c contributions
    if ref.E is not None:
        D = np.abs(ref.E - ref.JtJ)
        i, j = np.unravel_index(np.argmax(D), D.shape)
        assert abs(info["c_max"] - D[i, j]) <= 2 * ref.c * EPS * np.max(ref.B), (info["c_max"], D[i, j])
    if key == "line":
        assert abs(cur.values[0] - (-16.43)) < 0.005 and cur.kind == "saddle"
        assert cur.negative()[0][2][0][0] == "L0"
    if key == "2x20_refined":
        assert cur.kind == "minimum" and cur.negative() == []
    if key == "c":
        assert ref.E is None and ref.n == 3301  # the chain is segmented (the join level); the reference is eigsh


def test_a_curvature_call_leaves_the_handle_as_it_was(hip_lib):
    fg, results, ref = ch.reference("a")
    ids = _select(ref.prob, None)[1]
    V = _block_of_vectors(ref.n)
    with CurvatureHandle(ref.prob) as h:
        spectrum_before = h.spectrum(ref.point, 8, REL_TOL, MAX_ITERS, SHIFT)
        marginals_before = h.columns(ref.point, ids)
        first = h.curvature(ref.point, 8, REL_TOL, MAX_ITERS, SHIFT)
        spectrum_after = h.spectrum(ref.point, 8, REL_TOL, MAX_ITERS, SHIFT)
        marginals_after = h.columns(ref.point, ids)
        h.product(ref.point, V, exact=True)
        second = h.curvature(ref.point, 8, REL_TOL, MAX_ITERS, SHIFT)
        spectrum_last = h.spectrum(ref.point, 8, REL_TOL, MAX_ITERS, SHIFT)
    assert first[0] == second[0] == 0 and first[5]["iterations"] == second[5]["iterations"]
    for a, b in zip(first[1:5], second[1:5]):  # values, vectors, residuals, quotients
        np.testing.assert_array_equal(a, b)
    assert first[5]["c_max"] == second[5]["c_max"]
    for after in (spectrum_after, spectrum_last):
        assert spectrum_before[0] == after[0] == 0 and spectrum_before[4]["iterations"] == after[4]["iterations"]
        for a, b in zip(spectrum_before[1:4], after[1:4]):
            np.testing.assert_array_equal(a, b)
    assert marginals_before[0] == marginals_after[0] == 0
    for a, b in zip(marginals_before[1:4], marginals_after[1:4]):  # the columns, their residuals, their steps
        np.testing.assert_array_equal(a, b)
    assert first[1][0] < -1.0 and spectrum_before[1][0] > 0.0  # (the two calls do answer different questions here)


def test_argument_errors(hip_lib):
    fg, results, ref = ch.reference("2x20")
    V = _block_of_vectors(ref.n)
    with CurvatureHandle(ref.prob) as h:
        good = h.curvature(ref.point, 4, REL_TOL, MAX_ITERS, SHIFT)
        assert good[0] == 0
        for args, words in (((0, REL_TOL, MAX_ITERS, SHIFT), "score_refine_curvature: k must be 1..16"),
                            ((17, REL_TOL, MAX_ITERS, SHIFT), "score_refine_curvature: k must be 1..16"),
                            ((4, 0.0, MAX_ITERS, SHIFT), "rel_tol must be positive and max_iters >= 1"),
                            ((4, REL_TOL, 0, SHIFT), "rel_tol must be positive and max_iters >= 1"),
                            ((4, REL_TOL, MAX_ITERS, 0.0), "shift_rel must be positive"),
                            ((4, REL_TOL, MAX_ITERS, float("nan")), "shift_rel must be positive")):
            with pytest.raises(RuntimeError, match=words):
                h.curvature(ref.point, *args)
        with pytest.raises(RuntimeError, match="n_cols must be 1..16"):
            h.product(ref.point, np.zeros((ref.n, 17)))
        with pytest.raises(RuntimeError, match="score_refine_hessian_product failed"):
            h.product(ref.point, np.zeros((ref.n, 0)))
        # the handle goes on after the refusals, with the bits it gave before them
        again = h.curvature(ref.point, 4, REL_TOL, MAX_ITERS, SHIFT)
        assert again[0] == 0
        np.testing.assert_array_equal(good[1], again[1])
        np.testing.assert_array_equal(good[2], again[2])
        rc, values, vectors, res, gn, info = h.curvature(ref.point, 16, REL_TOL, 2, SHIFT)
        assert rc == 1 and info["unconverged"] > 0 and info["iterations"] == 2
        assert np.all(np.isfinite(values)) and np.all(np.isfinite(vectors)) and np.all(np.isfinite(res)) and np.all(np.isfinite(gn))
    with pytest.raises(RuntimeError, match="did not reach"):
        hessian_spectrum(fg, results, k=16, max_iters=2)
    small = two_pose_graph()
    from marginals_helpers import noisy_truth
    prob, point = _problem_and_point(small, noisy_truth(small), None, None)
    with CurvatureHandle(prob) as h:
        with pytest.raises(RuntimeError, match="score_refine_curvature: fewer than 48 unknowns"):
            h.curvature(point, 1)
        out = h.product(point, np.eye(prob.n), exact=True)  # (the product has no such limit)
        assert out.shape == (3, 3) and np.all(np.isfinite(out))
    with pytest.raises(ValueError, match="fewer than the 48"):
        hessian_spectrum(small, noisy_truth(small), k=1)
