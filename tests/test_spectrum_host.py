"""The spectrum module without a GPU (score_amd/spectrum.py, engine="python") and the host Rayleigh-Ritz of the device
solver (score_amd/csrc/score_spectrum_rr.hpp) as a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

from conftest import ROOT
from marginals_helpers import landmark_names, pose_names
from spectrum_helpers import EPS, REL_TOL, bracket_margins, reference
from score_amd.marginals import _select
from score_amd.spectrum import covariance_bracket, information_spectrum


def test_python_engine_against_the_definition():
    fg, results, ref = reference("2x20")
    k = 16
    modes, info = information_spectrum(fg, results, k=k, engine="python")
    assert info["engine"] == "python" and info["h_max"] == ref.h_max
    assert modes.values.shape == (k,) and modes.vectors.shape == (ref.n, k) and modes.residuals.shape == (k,)
    assert np.all(np.diff(modes.values) >= 0)
    # H V = V diag(values) to the dense solver's own residual: n eps |H|_2 per pair (a backward-stable symmetric solver)
    rho = np.linalg.norm(ref.H @ modes.vectors - modes.vectors * modes.values, axis=0)
    assert np.all(rho <= ref.n * EPS * np.linalg.norm(ref.H, 2)), rho
    np.testing.assert_array_equal(modes.residuals, rho)
    np.testing.assert_allclose(modes.values, ref.values[:k], rtol=0, atol=ref.n * EPS * np.linalg.norm(ref.H, 2))
    total = sum(modes.participation.values())
    assert total.shape == (k,) and np.all(np.abs(total - 1.0) <= 4 * EPS * len(modes.names))
    everything = [nm for ch in pose_names(fg) for nm in ch][1:] + landmark_names(fg)
    assert modes.names == everything
    for nm in ("L0", "A1", "B19"):
        _, _, _, cols = _select(ref.prob, [nm])
        np.testing.assert_array_equal(modes.block(nm), modes.vectors[cols])
    assert modes.undetermined() == []
    with pytest.raises(ValueError):
        modes.block("A0")


def test_degenerate_beacon():
    fg, results, ref = reference("degenerate")
    modes, info = information_spectrum(fg, results, k=8, engine="python")
    und = modes.undetermined()
    print("lambda_0, lambda_1 =", modes.values[0], modes.values[1], "threshold", REL_TOL * info["h_max"])
    assert [j for j, _ in und] == [0]
    name, share = und[0][1][0]
    assert name == "L2" and share >= 0.99
    with pytest.raises(RuntimeError, match="L2"):
        covariance_bracket(modes)


def test_bracket_holds_with_exact_pairs():
    fg, results, ref = reference("2x20")
    modes, _ = information_spectrum(fg, results, k=8, engine="python")
    bracket = covariance_bracket(modes)
    want = landmark_names(fg) + [ch[-1] for ch in pose_names(fg)]
    assert list(bracket) == want
    Sigma = np.linalg.inv(ref.H)
    cond = ref.all_values[-1] / ref.all_values[0]
    cols = {nm: _select(ref.prob, [nm])[3] for nm in want}
    for nm, (lo, hi, norm) in bracket_margins(bracket, Sigma, ref, cols).items():
        tau = ref.n * EPS * cond * norm  # the rounding of the dense inverse; nothing else enters with exact eigenpairs
        print(nm, "Sigma - lower:", lo, "upper - Sigma:", hi, "tau:", tau)
        assert lo >= -tau and hi >= -tau, (nm, lo, hi, tau)
    # named variables, and a single mode: no lower part, the slack alone
    one, _ = information_spectrum(fg, results, k=1, engine="python")
    lower, slack = covariance_bracket(one, ["B5"])["B5"]
    assert lower.shape == (3, 3) and not lower.any() and slack == 1.0 / one.values[0]


def _deflated(A, B, drop):
    """The pencil restricted as score_spectrum_rr.hpp does it: directions with a positive Gram diagonal, scaled to a unit
    diagonal, the eigen-directions of the scaled Gram matrix above drop * largest."""
    A, B = 0.5 * (A + A.T), 0.5 * (B + B.T)
    use = np.nonzero(np.diag(B) > 0)[0]
    d = 1.0 / np.sqrt(np.diag(B)[use])
    As, Bs = A[np.ix_(use, use)] * np.outer(d, d), B[np.ix_(use, use)] * np.outer(d, d)
    lam, Q = np.linalg.eigh(Bs)
    keep = lam > drop * lam[-1]
    Y = Q[:, keep]
    return Y.T @ As @ Y, Y.T @ Bs @ Y, int(keep.sum())


def test_rayleigh_ritz_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / "spectrum_rr_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "score_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "spectrum_rr_check.cpp")], check=True)
    rng = np.random.default_rng(5)
    m, nb, rows = 48, 16, 400
    Aop = rng.normal(size=(rows, rows))
    Aop = Aop @ Aop.T / rows + 0.1 * np.eye(rows)  # SPD operator
    S1 = rng.normal(size=(rows, m))
    S2 = S1.copy()
    S2[:, 40:] = S2[:, :8] + 1e-14 * rng.normal(size=(rows, 8))  # S'S of rank 40
    S3 = S1.copy()
    S3[:, 32:] = 0.0  # an empty P
    pencils = [(S.T @ Aop @ S, S.T @ S) for S in (S1, S2, S3)]
    with open(tmp_path / "in.txt", "w") as f:
        f.write(f"{len(pencils)}\n")
        for A, B in pencils:
            f.write(f"{m} {nb}\n")
            for M in (A, B):
                f.write("\n".join(repr(float(v)) for v in M.ravel()) + "\n")
    run = subprocess.run([exe, str(tmp_path / "in.txt"), str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    tokens = open(tmp_path / "out.txt").read().split()
    per = 2 + nb + m * nb
    assert len(tokens) == per * len(pencils)
    for p, ((A, B), kept_want) in enumerate(zip(pencils, (48, 40, 32))):
        tok = tokens[p * per:(p + 1) * per]
        status, kept = int(tok[0]), int(tok[1])
        theta = np.array([float(t) for t in tok[2:2 + nb]])
        Cf = np.array([float(t) for t in tok[2 + nb:]]).reshape(m, nb)
        T, G, kept_ref = _deflated(A, B, 1e-10)
        assert status == 0 and kept == kept_ref == kept_want
        want = sla.eigh(T, G, eigvals_only=True)[:nb]
        bound = 48 * EPS * np.linalg.norm(0.5 * (A + A.T), 2) * np.linalg.cond(G)
        print("pencil", p, "kept", kept, "worst |theta - eigh| / bound:", float(np.max(np.abs(theta - want)) / bound))
        assert np.all(np.abs(theta - want) <= bound), (p, theta - want, bound)
        # the coefficients form B-orthonormal Ritz vectors; unused directions get none
        Bsym = 0.5 * (B + B.T)
        assert np.max(np.abs(Cf.T @ Bsym @ Cf - np.eye(nb))) <= 48 * EPS * np.linalg.cond(G) * 48
        if p == 2:
            assert not Cf[32:].any()


def test_argument_errors():
    fg, results, _ = reference("2x20")
    for kw in (dict(k=0), dict(k=17), dict(k=2.5), dict(rel_tol=0.0), dict(rel_tol=-1e-9), dict(max_iters=0), dict(shift=0.0),
               dict(shift=-1e-8), dict(engine="eager")):
        with pytest.raises(ValueError):
            information_spectrum(fg, results, **{"engine": "python", **kw})
