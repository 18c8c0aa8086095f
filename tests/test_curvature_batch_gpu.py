"""The batched second-order check on the device (score_refine_batch_curvature, score_refine_batch_hessian_product,
csrc/score_curvature_batch.hpp) and the device Rayleigh-Ritz kernel with the indefinite rule (score_curvature_ritz).

Every member of a group is judged against its own ``curvature_helpers.CurvatureReference`` (torch autograd, dense, written
from ``graph_arrays`` alone; ``eigsh`` beyond the dense limit) by ``check_pairs`` (A-D) and, for the product, by the entrywise
bound ``(longest_row + c) eps B|V|``: every bound is computed on the spot, no tolerance is chosen.  REL_TOL = 1e-9,
SHIFT = 1e-8, MAX_ITERS = 200 (conditions, not measurements).

The points (evaluated on the host with the dense path): ``line`` n = 59, saddle (-16.43, 19.7); ``2x20`` at the noisy truth
n = 121, saddle (-41.4, 0.178); ``long_rows`` n = 451, saddle (-2.23, 0.88); ``2x20_refined`` n = 121, minimum (0.201); ``a``
n = 151, saddle (-24.8, 0.38); ``d`` 3-D n = 303, saddle with three negatives (-6.92, -4.29, -0.69, 0.031); member ``3D0`` at
its host-refined point n = 303, minimum (0.0101); ``c`` n = 3301, one segmented chain, reference ``eigsh``; member ``E`` at its
start n = 197, saddle (-2.49), kept in reserve for the gating condition.  59 = 32 + 27 and 451 = 14 x 32 + 3: tail tiles of the
Gram pass end on member boundaries, and ``long_rows`` (a row of 186 entries > 128) sits between short-row members."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import curvature_helpers as ch
import ritz_pencils as rp
from conftest import ROOT
from curvature_helpers import EPS, MAX_ITERS, REL_TOL, SHIFT, CurvatureReference, check_pairs
from refine_batch_helpers import group, member, rough_start, twin_alone
from score_amd.bindings import CURVATURE_BATCH
from score_amd.curvature import CurvatureHandle, escape, sparse_hessian
from score_amd.curvature_batch import CURVATURE_BATCH_SYMBOLS, _bind, _curvature_of, hessian_spectrum_batch, indefinite_ritz
from score_amd.marginals import _problem_and_point
from score_amd.refine import refine_estimate
from score_amd.refine_batch import RefineBatchHandle, _problem_of, refine_estimate_batch
from score_amd.spectrum_batch import RITZ_BREAKDOWN, RITZ_NO_P, RITZ_OK, device_ritz
from test_curvature_gpu import _block_of_vectors
from test_spectrum_batch_gpu import _deflated

pytestmark = pytest.mark.gpu

FIVE = ("line", "2x20", "long_rows", "2x20_refined", "a")
RESERVE = "E@start"
KIND = {"line": "saddle", "2x20": "saddle", "long_rows": "saddle", "2x20_refined": "minimum", "a": "saddle", RESERVE: "saddle",
        "d": "saddle", "3D0": "minimum"}
F64, I32 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)


@functools.lru_cache(maxsize=None)
def at(name):
    """(graph, results, CurvatureReference) of a named point, computed once: a case of curvature_helpers (lower case),
    member E of refine_batch_helpers at its start, or a member ("A".."E", "3D0") at its host-refined point."""
    if name in ch.ALL_CASES:
        return ch.reference(name)
    fg = member(name.split("@")[0])[0]
    results = member("E")[1] if name == RESERVE else twin_alone(name)[0]
    return fg, results, CurvatureReference(fg, results)


def _refs(names):
    refs = [at(n)[2] for n in names]
    for n, r in zip(names, refs):
        ch.check_input_conditions(n, r)
    return refs


_cache = {}


def raw_group(hip_lib, names, k, max_iters=MAX_ITERS):
    """One ``RefineBatchHandle.curvature`` call on the group ``names`` at the members' points: (rc, per member, info); once."""
    key = (hip_lib, names, k, max_iters)
    if key not in _cache:
        refs = _refs(names)
        with RefineBatchHandle([r.prob for r in refs], hip_lib) as h:
            _cache[key] = h.curvature([r.point for r in refs], k, REL_TOL, max_iters, SHIFT)
        print(names, "k =", k, _cache[key][2], "iterations", [m[4] for m in _cache[key][1]])
    return _cache[key]


def single(hip_lib, name, k):
    """``CurvatureHandle.curvature`` on a handle of the member's own (the single-graph call): once."""
    key = (hip_lib, name, k, "single")
    if key not in _cache:
        ref = at(name)[2]
        with CurvatureHandle(ref.prob, hip_lib) as h:
            _cache[key] = h.curvature(ref.point, k, REL_TOL, MAX_ITERS, SHIFT)
    return _cache[key]


def five(hip_lib):
    """The group of five.  Its gating condition needs single-handle iteration counts that are not all equal: where they are,
    ``a`` gives its place to member E at its start."""
    its = [single(hip_lib, n, 8)[5]["iterations"] for n in FIVE]
    return FIVE if len(set(its)) > 1 else FIVE[:4] + (RESERVE,)


def _gn_quotient_bound(ref, V, sigma):
    """tests/test_curvature_gpu.py's, restated.  |device v'(J'J)v - host v'(J'J)v|: the product's rounding (longest row + c)
    eps |v|'(|J|'|J|)|v| with c the entry's contributions (at most longest row again) + 128, the dot's n eps of the same, and
    the shift taken out again: a few eps sigma; both sides."""
    _, J = ref.prob.residuals(ref.point, jac=True)
    Ja = abs(J)
    mass = np.einsum("ij,ij->j", Ja @ np.abs(V), Ja @ np.abs(V))
    return 2.0 * (2 * ref.longest_row + 128 + ref.n + 8) * EPS * (mass + sigma)


def _c_max_bound(ref):
    """each side of |E - J'J|_max is a sum of at most c contributions"""
    return 2 * ref.c * EPS * np.max(ref.B)


def _check_member(label, ref, k, got):
    """A member's raw outputs: check_pairs, h_max, c_max against the dense max |E - J'J| (where the reference is dense) and
    the Gauss-Newton quotients.  Returns the member as a ``Curvature`` and the residuals recomputed on the host."""
    values, Vt, res, gn, its, converged, h_max, c_max = got
    V = np.ascontiguousarray(Vt.T)
    assert converged and 1 <= its <= MAX_ITERS
    assert abs(h_max - ref.h_max) <= (ref.n + 1) * EPS * ref.h_max
    figures, rho = check_pairs(ref, k, values, V, REL_TOL, label)
    assert np.all(np.isfinite(res)) and res.shape == (k,)
    if ref.E is not None:
        D = np.abs(ref.E - ref.JtJ)
        print(f"{label}: c_max {c_max!r}, dense {float(np.max(D))!r}, bound {_c_max_bound(ref):.3e}")
        assert abs(c_max - np.max(D)) <= _c_max_bound(ref), (c_max, float(np.max(D)))
    want = np.einsum("ij,ij->j", V, ref.Hs @ V)
    bound = _gn_quotient_bound(ref, V, SHIFT * h_max)
    print(f"{label}: gauss_newton {gn[:3]}, worst |difference| / bound = {np.max(np.abs(gn - want) / bound):.3e}")
    assert np.all(np.abs(gn - want) <= bound), (gn, want, bound)
    return _curvature_of(ref.prob, values, V, res, gn, h_max, REL_TOL), rho


def test_product_with_E_and_with_JtJ_of_every_member(hip_lib):
    refs = _refs(FIVE)
    assert [r.n for r in refs] == [59, 121, 451, 121, 151] and 59 == 32 + 27 and 451 == 14 * 32 + 3
    assert refs[2].longest_row > 128 and all(r.longest_row <= 128 for r in refs[:2] + refs[3:])
    probs, points = [r.prob for r in refs], [r.point for r in refs]
    Vs = [_block_of_vectors(r.n) for r in refs]
    with RefineBatchHandle(probs, hip_lib) as h:
        exact = h.hessian_product(points, Vs, exact=True)
        plain = h.hessian_product(points, Vs, exact=False)
        one = h.hessian_product(points, [V[:, 9] for V in Vs], exact=True)
        seven = h.hessian_product(points, [V[:, 5:12] for V in Vs], exact=True)
        again = h.hessian_product(points, Vs, exact=True)
    for key, ref, V, ex, pl, o1, o7, ag in zip(FIVE, refs, Vs, exact, plain, one, seven, again):
        bound = (ref.longest_row + ref.c) * EPS * (ref.B @ np.abs(V))
        for label, got, want in (("E V", ex, ref.E @ V), ("(J'J) V", pl, ref.JtJ @ V)):
            err = np.abs(got - want)
            ratio = float(np.max(err[bound > 0] / bound[bound > 0]))
            print(f"{key}: {label}: n = {ref.n}, longest row {ref.longest_row}, c = {ref.c}, worst |difference| / bound = {ratio:.3e}")
            assert got.shape == V.shape and np.all(err <= bound), f"{key}: {label}: worst entry at {ratio:.3e} of its bound"
        assert np.max(np.abs(ex - pl)) > 0.0
        # fewer columns: the bits of the same columns at 16; and two calls give the same bits
        assert o1.shape == (ref.n,) and np.array_equal(o1, ex[:, 9])
        assert np.array_equal(o7, ex[:, 5:12])
        assert np.array_equal(ag, ex)
    # a member in the group is the member alone, bit for bit
    a = FIVE.index("a")
    with RefineBatchHandle([probs[a]], hip_lib) as h:
        alone = h.hessian_product([points[a]], [Vs[a]], exact=True)[0]
        alone_plain = h.hessian_product([points[a]], [Vs[a]], exact=False)[0]
    assert np.array_equal(alone, exact[a]) and np.array_equal(alone_plain, plain[a])


def test_group_of_five(hip_lib):
    names = five(hip_lib)
    single_its = [single(hip_lib, n, 8)[5]["iterations"] for n in names]
    assert len(set(single_its)) > 1, f"the single handles' iteration counts are all equal ({single_its}): the gating would go untested"
    rc, per, info = raw_group(hip_lib, names, 8)
    assert rc == 0 and info["unconverged"] == 0 and info["members"] == 5 and info["modes"] == 8 and info["block"] == 16
    assert info["saddles"] == 4
    refs = _refs(names)
    for name, ref, got in zip(names, refs, per):
        cur, _ = _check_member(f"{name} in {names}, k = 8", ref, 8, got)
        assert cur.kind == KIND[name], (name, cur.values[:3])
        if name == "line":
            assert abs(cur.values[0] - (-16.43)) < 0.005
            assert cur.negative()[0][2][0][0] == "L0"
        if name == "2x20_refined":
            assert cur.negative() == []
    its = [m[4] for m in per]
    assert len(set(its)) > 1, f"the members' iteration counts are all equal ({its}): the gating went untested"
    assert info["rounds"] > max(its)  # (every member takes at least one verifying round)
    assert info["max_residual"] == max(float(np.max(m[2])) for m in per)


@pytest.mark.parametrize("k", [1, 16])
def test_one_and_sixteen_modes(hip_lib, k):
    names = ("2x20", "a")
    rc, per, info = raw_group(hip_lib, names, k)
    assert rc == 0 and info["unconverged"] == 0 and info["saddles"] == 2
    for name, ref, got in zip(names, _refs(names), per):
        assert got[0].shape == (k,) and got[1].shape == (k, ref.n) and got[3].shape == (k,)
        _check_member(f"{name} in {names}, k = {k}", ref, k, got)


def test_3d_group(hip_lib):
    names = ("d", "3D0")
    rc, per, info = raw_group(hip_lib, names, 8)
    assert rc == 0 and info["unconverged"] == 0 and info["saddles"] == 1
    for name, ref, got in zip(names, _refs(names), per):
        assert ref.n == 303
        cur, _ = _check_member(f"{name} in {names}", ref, 8, got)
        assert cur.kind == KIND[name], (name, cur.values[:4])
        if name == "d":
            assert int(np.sum(cur.values < -REL_TOL * got[6])) == 3 and len(cur.negative()) == 3


def test_segmented_chain_inside_a_union(hip_lib):
    """One chain of 1100 poses (the join level of score_join.hpp, applied to all 16 vectors, under an indefinite operator)
    beside ``2x20``."""
    names = ("c", "2x20")
    ref = at("c")[2]
    assert ref.E is None and ref.n == 3301  # the reference is eigsh
    rc, per, info = raw_group(hip_lib, names, 4)
    assert rc == 0 and info["unconverged"] == 0
    for name, r, got in zip(names, _refs(names), per):
        _check_member(f"{name} in {names}", r, 4, got)


def test_against_the_single_handle(hip_lib):
    names = five(hip_lib)
    _, per, _ = raw_group(hip_lib, names, 8)
    for name, ref, got in zip(names, _refs(names), per):
        rc, values, Vt, res, gn, info = single(hip_lib, name, 8)
        assert rc == 0
        rho_group = ref.residuals(got[0], np.ascontiguousarray(got[1].T))
        rho_single = ref.residuals(values, np.ascontiguousarray(Vt.T))
        print(f"{name}: worst |lambda_group - lambda_single| / (rho_group + rho_single) = "
              f"{float(np.max(np.abs(got[0] - values) / (rho_group + rho_single))):.3e}")
        assert np.all(np.abs(got[0] - values) <= rho_group + rho_single), (name, got[0] - values)
        one = _curvature_of(ref.prob, values, np.ascontiguousarray(Vt.T), res, gn, info["h_max"], REL_TOL)
        many = _curvature_of(ref.prob, got[0], np.ascontiguousarray(got[1].T), got[2], got[3], got[6], REL_TOL)
        assert one.kind == many.kind == KIND[name]
        assert abs(got[7] - info["c_max"]) <= _c_max_bound(ref), (got[7], info["c_max"])


def _same_member(a, b):
    for x, y in zip(a[:4], b[:4]):  # values, vectors, residuals, quotients
        np.testing.assert_array_equal(x, y)
    assert a[4:] == b[4:]  # iterations, converged, h_max, c_max


def test_a_member_does_not_depend_on_its_group(hip_lib):
    names = five(hip_lib)
    _, per, _ = raw_group(hip_lib, names, 8)
    _, alone, info = raw_group(hip_lib, ("2x20",), 8)
    assert info["members"] == 1 and info["saddles"] == 1
    _same_member(per[names.index("2x20")], alone[0])


def test_two_calls_give_the_same_bits(hip_lib):
    refs = _refs(("2x20", "a"))
    probs, points = [r.prob for r in refs], [r.point for r in refs]
    with RefineBatchHandle(probs, hip_lib) as h:
        first = h.curvature(points, 8, REL_TOL, MAX_ITERS, SHIFT)
        second = h.curvature(points, 8, REL_TOL, MAX_ITERS, SHIFT)
    assert first[0] == second[0] == 0 and first[2]["rounds"] == second[2]["rounds"]
    for a, b in zip(first[1], second[1]):
        _same_member(a, b)


def test_the_calls_leave_the_handle_as_it_was(hip_lib):
    refs = _refs(("2x20", "a"))
    probs, points = [r.prob for r in refs], [r.point for r in refs]
    Vs = [_block_of_vectors(r.n) for r in refs]
    with RefineBatchHandle(probs, hip_lib) as h:
        spectrum_before = h.spectrum(points, 8, REL_TOL, MAX_ITERS, SHIFT)
        first = h.curvature(points, 8, REL_TOL, MAX_ITERS, SHIFT)
        spectrum_after = h.spectrum(points, 8, REL_TOL, MAX_ITERS, SHIFT)
        h.hessian_product(points, Vs, exact=True)
        second = h.curvature(points, 8, REL_TOL, MAX_ITERS, SHIFT)
        spectrum_last = h.spectrum(points, 8, REL_TOL, MAX_ITERS, SHIFT)
    assert first[0] == second[0] == 0 and first[2]["rounds"] == second[2]["rounds"]
    for a, b in zip(first[1], second[1]):
        _same_member(a, b)
    for after in (spectrum_after, spectrum_last):
        assert spectrum_before[0] == after[0] == 0 and spectrum_before[2]["rounds"] == after[2]["rounds"]
        for a, b in zip(spectrum_before[1], after[1]):
            for x, y in zip(a[:3], b[:3]):
                np.testing.assert_array_equal(x, y)
            assert a[3:] == b[3:]
    assert first[1][0][0][0] < -1.0 and spectrum_before[1][0][0][0] > 0.0  # (the two calls do answer different questions here)


def test_handle_state_survives_the_curvature(hip_lib):
    """run, curvature at the refined points, run from other starts: the second run equals a fresh handle's bit for bit."""
    keys = ("B", "E")
    fgs, starts = group(keys)
    probs, first = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, starts)])
    second = [_problem_of(fg, rough_start(k), None, None)[1] for k, fg in zip(keys, fgs)]
    with RefineBatchHandle(probs, hip_lib) as h:
        refined, _ = h.run(list(first))
        rc, per, info = h.curvature(refined, 8, REL_TOL, MAX_ITERS, SHIFT)
        assert rc == 0 and info["unconverged"] == 0
        pts, infos = h.run(second)
    with RefineBatchHandle(probs, hip_lib) as h:
        fresh, finfos = h.run(second)
    for k, a, b, ia, ib in zip(keys, pts, fresh, infos, finfos):
        print(k, "run after the curvature: iterations", ia["iterations"], "solves", ia["linear_solves"], "pcg", ia["pcg_iters"])
        assert np.array_equal(a, b)
        for f in ("iterations", "linear_solves", "pcg_iters", "cost_initial", "cost_final", "grad_inf"):
            assert ia[f] == ib[f]


def test_iteration_cap(hip_lib):
    names = ("2x20", "a")
    rc, per, info = raw_group(hip_lib, names, 16, max_iters=2)
    assert rc == 1 and info["unconverged"] == 2
    for values, Vt, res, gn, its, converged, h_max, c_max in per:
        assert not converged and its == 2  # (reported as -(2 + 1), decoded by batch_curvature)
        assert all(np.all(np.isfinite(x)) for x in (values, Vt, res, gn, h_max, c_max))
    refs = _refs(names)
    with RefineBatchHandle([r.prob for r in refs], hip_lib) as h:  # the raw words
        _, poses, lms = h._flat_points([r.point for r in refs])
        its = np.zeros(2, dtype=np.int32)
        rc = _bind(h.lib).score_refine_batch_curvature(h.h, poses.ctypes.data_as(F64), lms.ctypes.data_as(F64), 16, REL_TOL, 2, SHIFT,
                                                       None, None, None, None, its.ctypes.data_as(I32), None, None, None)
        assert rc == 1 and list(its) == [-3, -3]
    with pytest.raises(RuntimeError, match=r"graph 0: .*did not reach"):
        hessian_spectrum_batch([at(n)[0] for n in names], [at(n)[1] for n in names], k=16, max_iters=2, lib_path=hip_lib)


def test_errors_are_reported_not_faults(hip_lib):
    keys = ("A", "B", "C")
    probs, points = zip(*[_problem_and_point(member(k)[0], twin_alone(k)[0], None, None) for k in keys])
    with RefineBatchHandle(probs, hip_lib) as h:
        with pytest.raises(RuntimeError, match=r"score_refine_batch_curvature: member 2: 37 unknowns"):
            h.curvature(list(points), 8, REL_TOL, MAX_ITERS, SHIFT)
        out = h.hessian_product(list(points), [np.eye(p.n)[:, :3] for p in probs], exact=True)  # (the product has no such limit)
        assert [o.shape for o in out] == [(p.n, 3) for p in probs] and all(np.all(np.isfinite(o)) for o in out)
    refs = _refs(("2x20", "a"))
    probs, points = [r.prob for r in refs], [r.point for r in refs]
    with RefineBatchHandle(probs, hip_lib) as h:
        good = h.curvature(points, 4, REL_TOL, MAX_ITERS, SHIFT)
        assert good[0] == 0
        for words, args in (("score_refine_batch_curvature: k must be 1..16", (0, REL_TOL, MAX_ITERS, SHIFT)),
                            ("score_refine_batch_curvature: k must be 1..16", (17, REL_TOL, MAX_ITERS, SHIFT)),
                            ("rel_tol must be positive and max_iters >= 1", (4, 0.0, MAX_ITERS, SHIFT)),
                            ("rel_tol must be positive and max_iters >= 1", (4, REL_TOL, 0, SHIFT)),
                            ("shift_rel must be positive", (4, REL_TOL, MAX_ITERS, 0.0)),
                            ("shift_rel must be positive", (4, REL_TOL, MAX_ITERS, float("nan")))):
            with pytest.raises(RuntimeError, match=words):
                h.curvature(points, *args)
        with pytest.raises(RuntimeError, match="score_refine_batch_hessian_product: n_cols must be 1..16"):
            h.hessian_product(points, [np.zeros((r.n, 17)) for r in refs])
        with pytest.raises(RuntimeError, match="score_refine_batch_hessian_product failed"):
            h.hessian_product(points, [np.zeros((r.n, 0)) for r in refs])
        lib = _bind(h.lib)
        assert lib.score_refine_batch_curvature(None, None, None, 8, REL_TOL, MAX_ITERS, SHIFT, None, None, None, None, None, None, None, None) < 0
        assert lib.score_refine_batch_hessian_product(None, None, None, 1, None, 1, None) < 0
        assert b"null handle" in lib.score_last_error()
        # the handle goes on after the refusals, with the bits it gave before them
        again = h.curvature(points, 4, REL_TOL, MAX_ITERS, SHIFT)
        assert again[0] == 0 and again[2]["rounds"] == good[2]["rounds"]
        for a, b in zip(good[1], again[1]):
            _same_member(a, b)


def test_device_rayleigh_ritz_with_the_indefinite_rule(hip_lib):
    """score_curvature_ritz on the five pencils of test_spectrum_batch_gpu.py::test_device_rayleigh_ritz_alone: the three
    definite ones give the bits score_spectrum_ritz gives, the NaN one breaks down, and the negated one -- a breakdown under
    the positive-definite rule -- is answered: theta against scipy.linalg.eigh of the deflated pencil under that test's bound
    48 eps |A|_2 cond(G), all of it negative, |C'BC - I| under its bound."""
    rng = np.random.default_rng(5)
    m, nb, rows = 48, 16, 400
    Aop = rng.normal(size=(rows, rows))
    Aop = Aop @ Aop.T / rows + 0.1 * np.eye(rows)  # SPD operator
    S1 = rng.normal(size=(rows, m))
    S2 = S1.copy()
    S2[:, 40:] = S2[:, :8] + 1e-14 * rng.normal(size=(rows, 8))  # S'S of rank 40
    S3 = S1.copy()
    S3[:, 32:] = 0.0  # an empty P
    good = [(S.T @ Aop @ S, S.T @ S) for S in (S1, S2, S3)]
    with_nan = good[0][0].copy()
    with_nan[3, 7] = np.nan
    pencils = good + [(with_nan, good[0][1]), (-good[0][0], good[0][1])]
    GA, GB = np.array([p[0] for p in pencils]), np.array([p[1] for p in pencils])
    theta, coef, status, kept = indefinite_ritz(GA, GB, hip_lib)
    theta_pd, coef_pd, status_pd, kept_pd = device_ritz(GA, GB, hip_lib)
    print("status", status, "kept", kept, "positive-definite rule: status", status_pd)
    assert list(status) == [RITZ_OK, RITZ_OK, RITZ_OK, RITZ_BREAKDOWN, RITZ_OK]
    assert list(status_pd) == [RITZ_OK, RITZ_OK, RITZ_OK, RITZ_BREAKDOWN, RITZ_BREAKDOWN]
    assert list(kept[:3]) == [48, 40, 32] and kept[4] == 48
    np.testing.assert_array_equal(theta[:3], theta_pd[:3])
    np.testing.assert_array_equal(coef[:3], coef_pd[:3])
    assert list(kept[:3]) == list(kept_pd[:3])
    A, B = pencils[4]
    T, G, kept_ref = _deflated(A, B, 1e-10)
    assert kept_ref == 48
    want = sla.eigh(T, G, eigvals_only=True)[:nb]
    bound = 48 * EPS * np.linalg.norm(0.5 * (A + A.T), 2) * np.linalg.cond(G)
    print("negated pencil: worst |theta - eigh| / bound:", float(np.max(np.abs(theta[4] - want)) / bound), "lowest", theta[4][0])
    assert np.all(np.abs(theta[4] - want) <= bound), (theta[4] - want, bound)
    assert np.all(theta[4] < 0.0) and np.all(np.diff(theta[4]) >= 0.0)
    Bsym = 0.5 * (B + B.T)
    ortho = float(np.max(np.abs(coef[4].T @ Bsym @ coef[4] - np.eye(nb))))
    print("negated pencil: |C'BC - I| / bound:", ortho / (48 * EPS * np.linalg.cond(G) * 48))
    assert ortho <= 48 * EPS * np.linalg.cond(G) * 48


@functools.lru_cache(maxsize=None)
def _family_in_one_launch(hip_lib):
    return rp.judge_launch(lambda GA, GB: indefinite_ritz(GA, GB, hip_lib), True)


def test_device_rayleigh_ritz_on_the_family_with_the_indefinite_rule(hip_lib):
    """score_curvature_ritz on the family of tests/ritz_pencils.py in ONE launch, under the assertions the host routine passes
    with ``indefinite`` in test_spectrum_host.py::test_rayleigh_ritz_under_sanitizers.  The rule is read by one sign test: the
    pencils without a negative value give the bits score_spectrum_ritz gives (a retry for a non-finite P block included), and
    the two pencils the definite rule answers without P keep P here -- 16 negative values (negP), 3 among positive ones
    (shift3).  profiles/ritz_pencils.md holds the measured ratios."""
    per = _family_in_one_launch(hip_lib)
    labels = [p.label for p in rp.family()]
    by = dict(zip(labels, per))
    assert [by[label][2:] for label in ("nanP", "infP", "negP", "shift3", "negated")] == [(RITZ_NO_P, 32)] * 2 + [(RITZ_OK, 48)] * 3
    assert [int(np.sum(by[label][0] < 0.0)) for label in ("negP", "shift3", "negated")] == [16, 3, 16]
    assert by["rank15"][2:] == (RITZ_BREAKDOWN, 15) and by["few"][2:] == (RITZ_BREAKDOWN, 0)
    theta, coef, status, kept = device_ritz(*rp.stacked(rp.family()), hip_lib)
    positive = rp.positive_labels()
    assert len(positive) == len(labels) - 3
    for label in positive:
        i = labels.index(label)
        assert rp.same_bits((theta[i], coef[i], status[i], kept[i]), by[label]), f"{label}: the rules give different bits"
    for label in ("negP", "shift3"):  # the definite rule dropped P
        i = labels.index(label)
        assert (status[i], kept[i]) == (RITZ_NO_P, 32) and not coef[i][32:].any() and by[label][1][32:].any()


def test_device_rayleigh_ritz_with_the_indefinite_rule_whatever_the_launch(hip_lib):
    """A pencil's bits under the indefinite rule are those of the one launch of the family: in the family reversed, alone in a
    launch, and among 600 pencils (two resident workgroups of the kernel on every CU)."""
    rp.judge_launch_shapes(lambda GA, GB: indefinite_ritz(GA, GB, hip_lib), _family_in_one_launch(hip_lib))


def test_through_the_modules(hip_lib):
    # A..E at their refined points: C (37 unknowns) is answered on the host, the rest on the device, in input order
    all_keys = ("A", "B", "C", "D", "E")
    out = hessian_spectrum_batch([at(k)[0] for k in all_keys], [at(k)[1] for k in all_keys], k=4, rel_tol=REL_TOL, max_iters=MAX_ITERS,
                                 shift=SHIFT, lib_path=hip_lib)
    assert [info["engine"] for _, info in out] == ["device", "device", "python", "device", "device"]
    for key, (cur, info) in zip(all_keys, out):
        ref = at(key)[2]
        print(key, info)
        assert cur.kind == "minimum" and cur.negative() == [] and info["group"] == 0 and info["unconverged"] == 0
        assert info["shift"] == SHIFT * info["h_max"] and cur.vectors.shape == (ref.n, 4)
        check_pairs(ref, 4, cur.values, cur.vectors, REL_TOL, f"{key} of A..E")
    assert all(info["rounds"] == out[0][1]["rounds"] > 0 for _, info in out)
    # a saddle found by the group call, left with escape, refined: both members are minima and the cost has fallen
    (fg_l, res_l, ref_l), (fg_r, res_r, _) = at("line"), at("2x20_refined")
    (cur_l, _), (cur_r, _) = hessian_spectrum_batch([fg_l, fg_r], [res_l, res_r], k=4, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT,
                                                    lib_path=hip_lib)
    assert cur_l.kind == "saddle" and cur_r.kind == "minimum"
    cost_before = float(ref_l.prob.cost(ref_l.point))
    refined, rinfo = refine_estimate(fg_l, escape(fg_l, res_l, cur_l), engine="native", lib_path=hip_lib)
    (cur_l2, _), (cur_r2, _) = hessian_spectrum_batch([fg_l, fg_r], [refined, res_r], k=4, rel_tol=REL_TOL, max_iters=MAX_ITERS,
                                                      shift=SHIFT, lib_path=hip_lib)
    print("line: cost", cost_before, "->", rinfo["cost_final"], "values", cur_l.values[:2], "->", cur_l2.values[:2])
    assert cur_l2.kind == "minimum" and cur_r2.kind == "minimum" and rinfo["cost_final"] < cost_before
    # the keyword of refine_estimate_batch: the check on the handle that refined
    fgs, starts = group(("B", "E"))
    refined = refine_estimate_batch(fgs, starts, lib_path=hip_lib, curvature=4)
    assert all("curvature" not in info for _, info in refine_estimate_batch(fgs, starts, lib_path=hip_lib))
    separate = hessian_spectrum_batch(fgs, [res for res, _ in refined], k=4, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT, lib_path=hip_lib)
    for fg, (res, info), (cur2, info2) in zip(fgs, refined, separate):
        cur, cinfo = info["curvature"]
        assert cinfo["engine"] == "device" and cinfo["group"] == info["group"] and cinfo["rounds"] > 0 and cur.kind == cur2.kind
        prob, point = _problem_and_point(fg, res, None, None)
        E = sparse_hessian(prob, point)
        rho = np.linalg.norm(E @ cur.vectors - cur.vectors * cur.values, axis=0)
        rho2 = np.linalg.norm(E @ cur2.vectors - cur2.vectors * cur2.values, axis=0)
        assert np.all(np.abs(cur.values - cur2.values) <= rho + rho2), (cur.values - cur2.values, rho, rho2)


def test_contract(hip_lib):
    header = open(os.path.join(ROOT, "include", "score_curvature_batch.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = re.findall(r"\b(score_[a-z_0-9]+)\s*\(", header)
    assert sorted(declared) == sorted(CURVATURE_BATCH) == sorted(CURVATURE_BATCH_SYMBOLS)
    lib = ctypes.CDLL(hip_lib)
    for sym in CURVATURE_BATCH_SYMBOLS:
        assert hasattr(lib, sym), sym
