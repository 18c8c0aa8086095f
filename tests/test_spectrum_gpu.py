"""The lowest eigenpairs of the information matrix on the device (score_refine_spectrum, csrc/score_spectrum.hpp) against
the host reference, under the checks A-D of tests/spectrum_helpers.py: every bound is computed from the reference, the
pair's own residual recomputed on the host, and the number format.  max_iters = 200 throughout: a condition."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from marginals_helpers import landmark_names, pose_names
from spectrum_helpers import (EPS, MAX_ITERS, REL_TOL, SHIFT, SpectrumReference, beacon_off_weights, bracket_margins, check_modes,
                              reference)
from score_amd.marginals import _select, marginal_covariances
from score_amd.spectrum import SPECTRUM_SYMBOLS, SpectrumHandle, covariance_bracket, device_spectrum, information_spectrum

pytestmark = pytest.mark.gpu


def _device(key, k, **kw):
    fg, results, ref = reference(key)
    modes, info = information_spectrum(fg, results, k=k, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT, **kw)
    print(key, "k =", k, info)
    assert info["engine"] == "device" and info["unconverged"] == 0 and 1 <= info["iterations"] <= MAX_ITERS  # A: the return code
    assert abs(info["h_max"] - ref.h_max) <= (ref.n + 1) * EPS * ref.h_max and info["shift"] == SHIFT * info["h_max"]
    figures, rho = check_modes(ref, k, modes.values, modes.vectors, REL_TOL, f"{key}, k = {k}")
    # the reported residuals are those of the device's H: an entry of it differs from the host's by (longest row + 1) eps h_max
    # at most, a row of the product by sqrt(longest row) times that for a unit vector -- gather and product, both sides
    delta = (ref.longest_row + 1) * EPS * ref.h_max
    assert np.all(np.abs(modes.residuals - rho) <= 4 * delta * np.sqrt(ref.n * ref.longest_row)), (modes.residuals, rho)
    return fg, results, ref, modes, info


@pytest.mark.parametrize("k", [1, 8, 16])
def test_short_rows_and_the_tail_tile(hip_lib, k):
    fg, results, ref, modes, info = _device("2x20", k)
    assert ref.n == 121  # 121 = 3 * 32 + 25: a tail tile of the Gram pass, one row block of the others
    total = sum(modes.participation.values())
    assert np.all(np.abs(total - 1.0) <= 4 * EPS * len(modes.names))


def test_beacon_rows_beyond_the_long_row_limit(hip_lib):
    fg, results, ref, *_ = _device("long_rows", 8)
    assert int(np.max(np.diff(ref.Hs.tocsr().indptr))) > 128  # kMvLongRow


def test_loop_closures_and_a_landmark_prior(hip_lib):
    _device("a", 8)


def test_chain_beyond_the_second_level(hip_lib):
    fg, results, ref, *_ = _device("c", 4)  # 1100 poses: the chain is segmented, the preconditioner applied to 16 vectors at once
    assert ref.H is None and ref.n == 3301  # the reference is eigsh


def test_3d_graph(hip_lib):
    fg, results, ref, modes, _ = _device("d", 8)
    assert modes.block(pose_names(fg)[1][-1]).shape == (6, 8) and modes.block("L0").shape == (3, 8)


def test_degenerate_beacon_on_the_device(hip_lib):
    fg, results, ref = reference("degenerate")
    modes, info = information_spectrum(fg, results, k=8, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT)
    print("degenerate", info, modes.values[:3])
    assert modes.values[0] <= REL_TOL * info["h_max"]
    und = modes.undetermined()
    assert [j for j, _ in und] == [0] and und[0][1][0][0] == "L2" and und[0][1][0][1] >= 0.99
    rho = ref.residuals(modes.values, modes.vectors)
    assert np.all(rho <= 2 * REL_TOL * ref.h_max)
    assert abs(modes.values[1] - ref.values[1]) <= rho[1] + ref.rho[1]  # B for lambda_1
    with pytest.raises(RuntimeError, match="L2"):
        covariance_bracket(modes)
    # every range of L1 off: two more directions without information
    w = beacon_off_weights(fg, "L1")
    assert 0 < np.count_nonzero(w == 0) < len(w)
    modes_w, info_w = information_spectrum(fg, results, k=8, range_weights=w, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT)
    print("degenerate, L1 off", info_w, modes_w.values[:4])
    und = modes_w.undetermined()
    assert [j for j, _ in und] == [0, 1, 2]
    on = np.array([sum(s for nm, s in shares if nm in ("L1", "L2")) for _, shares in und])
    assert np.all(on >= 0.99)
    L1 = sum(float(modes_w.participation["L1"][j]) for j in range(3))
    L2 = sum(float(modes_w.participation["L2"][j]) for j in range(3))
    assert abs(L1 - 2.0) <= 0.02 and abs(L2 - 1.0) <= 0.02  # two on L1, one on L2 (a zero eigenvalue of multiplicity 3 mixes them)
    ref_w = SpectrumReference(fg, results, range_weights=w)
    rho_w = ref_w.residuals(modes_w.values, modes_w.vectors)
    assert np.all(rho_w <= 2 * REL_TOL * ref_w.h_max)
    assert np.all(np.abs(modes_w.values - ref_w.values[:8])[3:] <= (rho_w + ref_w.rho[:8])[3:])  # B for the determined modes


def test_bracket_on_the_device(hip_lib):
    fg, results, ref = reference("2x20")
    k = 8
    modes, info = information_spectrum(fg, results, k=k, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT)
    bracket = covariance_bracket(modes)
    cov, _ = marginal_covariances(fg, results, engine="python")
    assert list(bracket) == list(cov)
    rho = ref.residuals(modes.values, modes.vectors)
    gaps = ref.gaps(k)
    lam = ref.values[:k]
    cond = ref.all_values[-1] / ref.all_values[0]
    spectral = float(np.sum((2 * rho / gaps + rho / lam) / lam))
    for nm in cov:
        lower, slack = bracket[nm]
        S = cov[nm]
        norm = float(np.linalg.norm(S, 2))
        tau = spectral + ref.n * EPS * cond * norm
        lo = float(np.linalg.eigvalsh(S - lower)[0])
        hi = float(np.linalg.eigvalsh(lower + slack * np.eye(len(S)) - S)[0])
        print(nm, "Sigma - lower:", lo, "upper - Sigma:", hi, "tau:", tau)
        assert lo >= -tau and hi >= -tau, (nm, lo, hi, tau)


def test_two_calls_give_the_same_bits(hip_lib):
    fg, results, ref = reference("a")
    with SpectrumHandle(ref.prob) as h:
        first = h.spectrum(ref.point, 8, REL_TOL, MAX_ITERS, SHIFT)
        second = h.spectrum(ref.point, 8, REL_TOL, MAX_ITERS, SHIFT)
    assert first[0] == second[0] == 0 and first[4]["iterations"] == second[4]["iterations"]
    np.testing.assert_array_equal(first[1], second[1])
    np.testing.assert_array_equal(first[2], second[2])


def test_contract(hip_lib):
    header = open(os.path.join(ROOT, "include", "score_spectrum.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = re.findall(r"\b(score_[a-z_0-9]+)\s*\(", header)
    assert sorted(declared) == sorted(SPECTRUM_SYMBOLS)
    lib = ctypes.CDLL(hip_lib)
    for sym in SPECTRUM_SYMBOLS:
        assert hasattr(lib, sym), sym
    fg, results, ref = reference("2x20")
    with SpectrumHandle(ref.prob) as h:
        rc, values, vectors, res, info = h.spectrum(ref.point, 16, REL_TOL, 2, SHIFT)
        assert rc == 1 and info["unconverged"] > 0 and info["iterations"] == 2
        assert values.shape == (16,) and vectors.shape == (16, ref.n)
        assert np.all(np.isfinite(values)) and np.all(np.isfinite(vectors)) and np.all(np.isfinite(res))
        with pytest.raises(RuntimeError, match="did not reach"):
            information_spectrum(fg, results, k=16, max_iters=2)
        with pytest.raises(RuntimeError, match="k must be"):
            h.spectrum(ref.point, 0, REL_TOL, MAX_ITERS, SHIFT)
        # the handle goes on after the refusals
        rc, *_ = h.spectrum(ref.point, 4, REL_TOL, MAX_ITERS, SHIFT)
        assert rc == 0
    fg_c, results_c, ref_c = reference("c")
    with pytest.raises(RuntimeError, match="chain_split"):
        device_spectrum(ref_c.prob, ref_c.point, 4, solver_settings=dict(chain_split=1))
