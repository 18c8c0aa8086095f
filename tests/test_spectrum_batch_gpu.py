"""Batched weakest modes on the device (score_refine_batch_spectrum, csrc/score_spectrum_batch.hpp) and the device
Rayleigh-Ritz kernel alone (score_spectrum_ritz).

Every member of a group is judged by the checks A-D of tests/spectrum_helpers.py against its own ``SpectrumReference`` at its
own point: every bound is computed on the spot from the reference, the pair's residual recomputed on the host, and the number
format -- no tolerance is chosen.  REL_TOL = 1e-9, SHIFT = 1e-8, MAX_ITERS = 200 (a condition, not a measurement).

The points are ``twin_alone(key)[0]``, the host-refined estimates of tests/refine_batch_helpers.py.  Unknowns per member:
A 363, B 151, C 37, D 839, E 197, 3D0 / 3D1 303.  In the group (A, B, D, E) D has the only long row (158 > 128) and sits
between short-row members; 151 = 4 x 32 + 23 and 197 = 6 x 32 + 5 give tail tiles of the Gram pass that end at a member
boundary; and the members finish rounds apart, which is what exercises the per-member modes."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import ritz_pencils as rp
from conftest import ROOT
from refine_batch_helpers import group, member, rough_start, twin_alone
from ritz_pencils import _deflated
from spectrum_helpers import EPS, MAX_ITERS, REL_TOL, SHIFT, SpectrumReference, check_modes, reference
from score_amd.marginals import _problem_and_point
from score_amd.refine_batch import RefineBatchHandle, _problem_of
from score_amd.spectrum import covariance_bracket
from score_amd.spectrum_batch import (RITZ_BREAKDOWN, RITZ_NO_P, RITZ_OK, SPECTRUM_BATCH_SYMBOLS, _bind, device_ritz,
                                      information_spectrum_batch)

pytestmark = pytest.mark.gpu

KEYS = ("A", "B", "D", "E")


@functools.lru_cache(maxsize=None)
def ref_of(key):
    """The host reference of a member at its host-refined point."""
    return SpectrumReference(member(key)[0], twin_alone(key)[0])


def _problems(keys):
    return zip(*[_problem_and_point(member(k)[0], twin_alone(k)[0], None, None) for k in keys])


_cache = {}


def raw_group(hip_lib, keys, k, max_iters=MAX_ITERS):
    """One ``RefineBatchHandle.spectrum`` call on the group ``keys`` at the members' points: (rc, per member, info); once."""
    at = (hip_lib, keys, k, max_iters)
    if at not in _cache:
        probs, points = _problems(keys)
        with RefineBatchHandle(probs, hip_lib) as h:
            _cache[at] = h.spectrum(list(points), k, REL_TOL, max_iters, SHIFT)
        print(keys, "k =", k, _cache[at][2], "iterations", [m[3] for m in _cache[at][1]])
    return _cache[at]


def _check_member(label, ref, k, values, Vt, res, h_max, subspace=True):
    """A member's raw outputs under the checks A-D, its reported residuals and h_max under ``_device``'s bounds of
    tests/test_spectrum_gpu.py."""
    assert abs(h_max - ref.h_max) <= (ref.n + 1) * EPS * ref.h_max
    figures, rho = check_modes(ref, k, values, np.ascontiguousarray(Vt.T), REL_TOL, label, subspace=subspace)
    # the reported residuals are those of the device's H: an entry of it differs from the host's by (longest row + 1) eps h_max
    # at most, a row of the product by sqrt(longest row) times that for a unit vector -- gather and product, both sides
    delta = (ref.longest_row + 1) * EPS * ref.h_max
    assert np.all(np.abs(res - rho) <= 4 * delta * np.sqrt(ref.n * ref.longest_row)), (res, rho)
    return figures


def test_group_of_four(hip_lib):
    rc, per, info = raw_group(hip_lib, KEYS, 8)
    assert rc == 0 and info["unconverged"] == 0 and info["members"] == 4 and info["modes"] == 8 and info["block"] == 16
    for key, (values, Vt, res, its, converged, h_max) in zip(KEYS, per):
        assert converged and 1 <= its <= MAX_ITERS
        _check_member(f"{key} in (A, B, D, E), k = 8", ref_of(key), 8, values, Vt, res, h_max)
    assert [ref_of(k).n for k in KEYS] == [363, 151, 839, 197]
    assert ref_of("D").longest_row > 128 and all(ref_of(k).longest_row <= 128 for k in "BE")
    its = [m[3] for m in per]
    assert len(set(its)) > 1, f"the members' iteration counts are all equal ({its}): the gating went untested"
    assert info["rounds"] > max(its)  # (every member takes at least one verifying round)
    assert info["max_residual"] == max(float(np.max(m[2])) for m in per)


@pytest.mark.parametrize("k", [1, 16])
def test_one_and_sixteen_modes(hip_lib, k):
    keys = ("B", "E")
    rc, per, info = raw_group(hip_lib, keys, k)
    assert rc == 0 and info["unconverged"] == 0
    for key, (values, Vt, res, its, converged, h_max) in zip(keys, per):
        assert converged and values.shape == (k,) and Vt.shape == (k, ref_of(key).n)
        _check_member(f"{key} in (B, E), k = {k}", ref_of(key), k, values, Vt, res, h_max)


def test_3d_group(hip_lib):
    keys = ("3D0", "3D1")
    fgs, pts = [member(k)[0] for k in keys], [twin_alone(k)[0] for k in keys]
    out = information_spectrum_batch(fgs, pts, k=8, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT, lib_path=hip_lib)
    for key, (modes, info) in zip(keys, out):
        ref = ref_of(key)
        print(key, info)
        assert ref.n == 303 and info["engine"] == "device" and info["unconverged"] == 0 and info["group"] == 0
        assert 1 <= info["iterations"] <= MAX_ITERS and info["rounds"] > info["iterations"]
        assert info["shift"] == SHIFT * info["h_max"]
        _check_member(key, ref, 8, modes.values, modes.vectors.T, modes.residuals, info["h_max"])
        assert modes.block("L0").shape == (3, 8)


def test_segmented_chain_inside_a_union(hip_lib):
    """One chain of 1100 poses (the second level of score_join.hpp, applied to all 16 vectors) beside B."""
    fg, results, ref = reference("c")
    assert ref.H is None and ref.n == 3301  # the reference is eigsh
    out = information_spectrum_batch([fg, member("B")[0]], [results, twin_alone("B")[0]], k=4, rel_tol=REL_TOL, max_iters=MAX_ITERS,
                                     shift=SHIFT, lib_path=hip_lib)
    for label, r, (modes, info) in (("1100 poses", ref, out[0]), ("B beside it", ref_of("B"), out[1])):
        print(label, info)
        assert info["engine"] == "device" and info["shift"] == SHIFT * info["h_max"]
        _check_member(label, r, 4, modes.values, modes.vectors.T, modes.residuals, info["h_max"])


def test_degenerate_member(hip_lib):
    fg_d, res_d, ref_d = reference("degenerate")
    fg_o, res_o, ref_o = reference("2x20")
    assert ref_d.n == 123 and ref_o.n == 121
    out = information_spectrum_batch([fg_d, fg_o], [res_d, res_o], k=8, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT, lib_path=hip_lib)
    (modes, info), (other, info_o) = out
    print("degenerate", info, modes.values[:3])
    assert modes.values[0] <= REL_TOL * info["h_max"]
    und = modes.undetermined()
    assert [j for j, _ in und] == [0] and und[0][1][0][0] == "L2" and und[0][1][0][1] >= 0.99
    rho = ref_d.residuals(modes.values, modes.vectors)
    assert np.all(rho <= 2 * REL_TOL * ref_d.h_max)
    assert abs(modes.values[1] - ref_d.values[1]) <= rho[1] + ref_d.rho[1]  # B for lambda_1
    with pytest.raises(RuntimeError, match="L2"):
        covariance_bracket(modes)
    assert list(covariance_bracket(other)) and other.undetermined() == []
    _check_member("2x20 beside the degenerate member", ref_o, 8, other.values, other.vectors.T, other.residuals, info_o["h_max"])
    # ... and the other member is what it is in a group of its own, bit for bit
    (alone, info_a), = information_spectrum_batch([fg_o], [res_o], k=8, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT, lib_path=hip_lib)
    for f in ("values", "vectors", "residuals"):
        np.testing.assert_array_equal(getattr(other, f), getattr(alone, f))
    assert info_o["iterations"] == info_a["iterations"] and info_o["h_max"] == info_a["h_max"]


def test_a_member_does_not_depend_on_its_group(hip_lib):
    _, per, _ = raw_group(hip_lib, KEYS, 8)
    _, alone, info = raw_group(hip_lib, ("B",), 8)
    assert info["members"] == 1
    in_group, by_itself = per[KEYS.index("B")], alone[0]
    for a, b in zip(in_group[:3], by_itself[:3]):  # values, vectors, residuals
        np.testing.assert_array_equal(a, b)
    assert in_group[3:] == by_itself[3:]  # iterations, converged, h_max


def test_two_calls_give_the_same_bits(hip_lib):
    keys = ("B", "E")
    probs, points = _problems(keys)
    with RefineBatchHandle(probs, hip_lib) as h:
        first = h.spectrum(list(points), 8, REL_TOL, MAX_ITERS, SHIFT)
        second = h.spectrum(list(points), 8, REL_TOL, MAX_ITERS, SHIFT)
    assert first[0] == second[0] == 0 and first[2]["rounds"] == second[2]["rounds"]
    for a, b in zip(first[1], second[1]):
        for x, y in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(x, y)
        assert a[3:] == b[3:]


def test_iteration_cap(hip_lib):
    keys = ("B", "E")
    rc, per, info = raw_group(hip_lib, keys, 16, max_iters=2)
    assert rc == 1 and info["unconverged"] == 2
    for values, Vt, res, its, converged, h_max in per:
        assert not converged and its == 2  # (reported as -(2 + 1), decoded by batch_spectrum)
        assert np.all(np.isfinite(values)) and np.all(np.isfinite(Vt)) and np.all(np.isfinite(res))
    probs, points = _problems(keys)
    with RefineBatchHandle(probs, hip_lib) as h:  # the raw words
        lib = _bind(h.lib)
        from score_amd.refine_robust import _point_arrays
        arrays = [_point_arrays(p, x) for p, x in zip(probs, points)]
        poses = np.ascontiguousarray(np.concatenate([a[0].ravel() for a in arrays]))
        lms = np.ascontiguousarray(np.concatenate([a[1].ravel() for a in arrays]))
        its = np.zeros(2, dtype=np.int32)
        f64, i32 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        rc = lib.score_refine_batch_spectrum(h.h, poses.ctypes.data_as(f64), lms.ctypes.data_as(f64), 16, REL_TOL, 2, SHIFT,
                                             None, None, None, its.ctypes.data_as(i32), None, None)
        assert rc == 1 and list(its) == [-3, -3]
    with pytest.raises(RuntimeError, match=r"graph 0: .*did not reach"):
        information_spectrum_batch([member(k)[0] for k in keys], [twin_alone(k)[0] for k in keys], k=16, max_iters=2, lib_path=hip_lib)


def test_handle_state_survives_the_spectrum(hip_lib):
    """run, spectrum at the refined points, run from other starts: the second run equals a fresh handle's bit for bit."""
    keys = ("B", "E")
    fgs, starts = group(keys)
    probs, first = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, starts)])
    second = [_problem_of(fg, rough_start(k), None, None)[1] for k, fg in zip(keys, fgs)]
    with RefineBatchHandle(probs, hip_lib) as h:
        refined, _ = h.run(list(first))
        rc, per, _ = h.spectrum(refined, 8, REL_TOL, MAX_ITERS, SHIFT)
        assert rc == 0
        pts, infos = h.run(second)
    with RefineBatchHandle(probs, hip_lib) as h:
        fresh, finfos = h.run(second)
    for k, a, b, ia, ib in zip(keys, pts, fresh, infos, finfos):
        print(k, "run after the spectrum: iterations", ia["iterations"], "solves", ia["linear_solves"], "pcg", ia["pcg_iters"])
        assert np.array_equal(a, b)
        for f in ("iterations", "linear_solves", "pcg_iters", "cost_initial", "cost_final", "grad_inf"):
            assert ia[f] == ib[f]


def test_errors_are_reported_not_faults(hip_lib):
    keys = ("A", "B", "C")
    probs, points = _problems(keys)
    with RefineBatchHandle(probs, hip_lib) as h:
        with pytest.raises(RuntimeError, match=r"member 2: 37 unknowns"):
            h.spectrum(list(points), 8, REL_TOL, MAX_ITERS, SHIFT)
    keys = ("B", "E")
    probs, points = _problems(keys)
    with RefineBatchHandle(probs, hip_lib) as h:
        for what, args in (("k must be", (0, REL_TOL, MAX_ITERS, SHIFT)), ("k must be", (17, REL_TOL, MAX_ITERS, SHIFT)),
                           ("rel_tol", (8, 0.0, MAX_ITERS, SHIFT)), ("shift_rel", (8, REL_TOL, MAX_ITERS, 0.0)),
                           ("max_iters", (8, REL_TOL, 0, SHIFT))):
            with pytest.raises(RuntimeError, match=what):
                h.spectrum(list(points), *args)
        assert _bind(h.lib).score_refine_batch_spectrum(None, None, None, 8, REL_TOL, MAX_ITERS, SHIFT, None, None, None, None, None, None) < 0
        # the handle answers a good call afterwards
        rc, per, info = h.spectrum(list(points), 4, REL_TOL, MAX_ITERS, SHIFT)
        assert rc == 0 and info["unconverged"] == 0
        for key, (values, Vt, res, its, converged, h_max) in zip(keys, per):
            _check_member(f"{key} after the refusals", ref_of(key), 4, values, Vt, res, h_max)
    # A..E through the module: C (37 unknowns) is answered on the host, the rest on the device, in input order
    all_keys = ("A", "B", "C", "D", "E")
    out = information_spectrum_batch([member(k)[0] for k in all_keys], [twin_alone(k)[0] for k in all_keys], k=4, rel_tol=REL_TOL,
                                     max_iters=MAX_ITERS, shift=SHIFT, lib_path=hip_lib)
    assert [info["engine"] for _, info in out] == ["device", "device", "python", "device", "device"]
    for key, (modes, info) in zip(all_keys, out):
        ref = SpectrumReference(member(key)[0], twin_alone(key)[0]) if key == "C" else ref_of(key)
        assert modes.vectors.shape == (ref.n, 4) and info["group"] == 0
        check_modes(ref, 4, modes.values, modes.vectors, REL_TOL, f"{key} of A..E")


def test_device_rayleigh_ritz_alone(hip_lib):
    """score_spectrum_ritz on the three pencils of test_spectrum_host.py::test_rayleigh_ritz_under_sanitizers (full rank; S'S of
    rank 40; an empty P), one with a NaN entry and one with S'AS negated, in ONE launch; theta against scipy.linalg.eigh of the
    deflated pencil under that test's bound 48 eps |A|_2 cond(G), |C'BC - I| under its bound."""
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
    theta, coef, status, kept = device_ritz(np.array([p[0] for p in pencils]), np.array([p[1] for p in pencils]), hip_lib)
    print("status", status, "kept", kept)
    assert list(status) == [RITZ_OK, RITZ_OK, RITZ_OK, RITZ_BREAKDOWN, RITZ_BREAKDOWN]
    assert list(kept[:3]) == [48, 40, 32]
    for p, ((A, B), kept_want) in enumerate(zip(good, (48, 40, 32))):
        T, G, kept_ref = _deflated(A, B, 1e-10)
        assert kept_ref == kept_want
        want = sla.eigh(T, G, eigvals_only=True)[:nb]
        bound = 48 * EPS * np.linalg.norm(0.5 * (A + A.T), 2) * np.linalg.cond(G)
        print("pencil", p, "kept", kept[p], "worst |theta - eigh| / bound:", float(np.max(np.abs(theta[p] - want)) / bound))
        assert np.all(np.abs(theta[p] - want) <= bound), (p, theta[p] - want, bound)
        Bsym = 0.5 * (B + B.T)
        ortho = float(np.max(np.abs(coef[p].T @ Bsym @ coef[p] - np.eye(nb))))
        print("pencil", p, "|C'BC - I| / bound:", ortho / (48 * EPS * np.linalg.cond(G) * 48))
        assert ortho <= 48 * EPS * np.linalg.cond(G) * 48
        if p == 2:
            assert not coef[p][32:].any()
    # a broken pencil leaves its neighbours alone: the launch without the broken ones gives the same bits
    theta3, coef3, status3, kept3 = device_ritz(np.array([p[0] for p in good]), np.array([p[1] for p in good]), hip_lib)
    np.testing.assert_array_equal(theta[:3], theta3)
    np.testing.assert_array_equal(coef[:3], coef3)
    assert list(status3) == [RITZ_OK] * 3 and list(kept3) == [48, 40, 32]
    # ... and twice the same launch, the same bits (the rotation order is fixed)
    again = device_ritz(np.array([p[0] for p in good]), np.array([p[1] for p in good]), hip_lib)
    np.testing.assert_array_equal(again[0], theta3)
    np.testing.assert_array_equal(again[1], coef3)


@functools.lru_cache(maxsize=None)
def _family_in_one_launch(hip_lib):
    return rp.judge_launch(lambda GA, GB: device_ritz(GA, GB, hip_lib), False)


def test_device_rayleigh_ritz_on_the_family(hip_lib):
    """score_spectrum_ritz on the family of tests/ritz_pencils.py in ONE launch, under the assertions the host routine passes in
    test_spectrum_host.py::test_rayleigh_ritz_under_sanitizers: status and kept as stated there (odd first and second
    decompositions, kept == nb, kept < nb, ma < nb, scattered index maps, excluded diagonals, ties, exact zeros, graded, tiny
    and huge scales), the three bounds, theta as the Rayleigh quotient of its vector, zero rows of the directions not in use,
    the wrapper's NaN where the step broke down, and
    the retry: a pencil whose P block is non-finite or negative ends without P, with the bits of the pencil whose P rows and
    columns are zero.  profiles/ritz_pencils.md holds the measured ratios."""
    per = _family_in_one_launch(hip_lib)
    by = dict(zip([p.label for p in rp.family()], per))
    assert [by[label][2:] for label in ("nanP", "infP", "negP", "shift3")] == [(RITZ_NO_P, 32)] * 4
    assert [by[label][2:] for label in ("rank16", "rank15", "few", "negated")] == [(RITZ_OK, 16), (RITZ_BREAKDOWN, 15), (RITZ_BREAKDOWN, 0),
                                                                                   (RITZ_BREAKDOWN, 32)]


def test_device_rayleigh_ritz_whatever_the_launch(hip_lib):
    """A pencil's bits are those of the one launch of the family: in the family reversed, alone in a launch, and among 600
    pencils (two resident workgroups of the kernel on every CU)."""
    rp.judge_launch_shapes(lambda GA, GB: device_ritz(GA, GB, hip_lib), _family_in_one_launch(hip_lib))


def test_contract(hip_lib):
    header = open(os.path.join(ROOT, "include", "score_spectrum_batch.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = re.findall(r"\b(score_[a-z_0-9]+)\s*\(", header)
    assert sorted(declared) == sorted(SPECTRUM_BATCH_SYMBOLS)
    lib = ctypes.CDLL(hip_lib)
    for sym in SPECTRUM_BATCH_SYMBOLS:
        assert hasattr(lib, sym), sym
