"""The spectrum module without a GPU (score_amd/spectrum.py, engine="python") and the host Rayleigh-Ritz of the device
solver (score_amd/csrc/score_spectrum_rr.hpp) as a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

import ritz_pencils as rp
from conftest import ROOT
from marginals_helpers import landmark_names, pose_names
from ritz_pencils import _deflated
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


def build_rr_check(where, include=os.path.join(ROOT, "score_amd", "csrc")):
    """tests/tools/spectrum_rr_check.cpp as a program of its own under the host sanitizers."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(where / "spectrum_rr_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", include, "-o", exe, os.path.join(ROOT, "tests", "tools", "spectrum_rr_check.cpp")], check=True)
    return exe


def run_rr_check(exe, where, pencils, indefinite):
    """The program on ``pencils`` under a rule, as a child process: per pencil (theta, coef, status, kept)."""
    m, nb = rp.M, rp.NB
    inp, outp = str(where / "in.txt"), str(where / f"out{int(indefinite)}.txt")
    if not os.path.exists(inp):
        with open(inp, "w") as f:
            f.write(f"{len(pencils)}\n")
            for p in pencils:
                f.write(f"{m} {nb}\n")
                for mat in (p.A, p.B):
                    f.write("\n".join(repr(float(v)) for v in mat.ravel()) + "\n")
    run = subprocess.run([exe, inp, outp] + (["indefinite"] if indefinite else []), capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    tokens = open(outp).read().split()
    per = 2 + nb + m * nb
    assert len(tokens) == per * len(pencils)
    out = []
    for i in range(len(pencils)):
        tok = tokens[i * per:(i + 1) * per]
        out.append((np.array([float(t) for t in tok[2:2 + nb]]), np.array([float(t) for t in tok[2 + nb:]]).reshape(m, nb),
                    int(tok[0]), int(tok[1])))
    return out


def check_host_family(exe, where, say=print):
    """The whole family of tests/ritz_pencils.py under both rules; returns {(label, indefinite): (status, kept, ratios)} and the
    raw results per rule."""
    pencils = rp.checked_family()
    labels = [p.label for p in pencils]
    table, results = {}, {}
    for indefinite in rp.RULES:
        results[indefinite] = run_rr_check(exe, where, pencils, indefinite)
        for p, (theta, coef, status, kept) in zip(pencils, results[indefinite]):
            ratios = rp.judge(p, indefinite, theta, coef, status, kept)
            table[(p.label, indefinite)] = (status, kept, ratios)
            say(f"{p.label:14s} {'indefinite' if indefinite else 'definite  '} status {status} kept {kept:2d} ratios to the bounds "
                f"(theta, C'BC, C'AC, quotient): {ratios}")
            # a quarter of a bound is the most the host routine may use: beyond it the pencil or the routine is at fault
            assert ratios is None or max(ratios) <= 0.25, (p.label, indefinite, ratios)
        # a retry repeats the arithmetic of the pencil whose P rows and columns are zero: the same bits
        for label, twin in rp.same_bits_pairs(indefinite):
            got, want = results[indefinite][labels.index(label)], results[indefinite][labels.index(twin)]
            assert got[2] == rp.RITZ_NO_P and want[2] == rp.RITZ_OK and got[3] == want[3], (label, twin)
            np.testing.assert_array_equal(got[0], want[0], err_msg=f"theta of {label} against {twin}")
            np.testing.assert_array_equal(got[1], want[1], err_msg=f"coef of {label} against {twin}")
    # the rule is read by the sign test alone: where no value is negative both rules give the same bits
    for label in rp.positive_labels():
        a, b = results[False][labels.index(label)], results[True][labels.index(label)]
        assert a[2:] == b[2:]
        if a[2] != rp.RITZ_BREAKDOWN:
            np.testing.assert_array_equal(a[0], b[0], err_msg=label)
            np.testing.assert_array_equal(a[1], b[1], err_msg=label)
    return table, results


def test_rayleigh_ritz_under_sanitizers(tmp_path):
    """sp_rayleigh_ritz on the family of tests/ritz_pencils.py under both rules (status, kept, the three bounds,
    theta as the Rayleigh quotient of its vector, zero rows of the directions not in use, the bit-equalities of the retry, the
    statuses that depend on the rule), and the first three pencils under the assertions they have always had.
    profiles/ritz_pencils.md holds the measured ratios."""
    exe = build_rr_check(tmp_path)
    table, results = check_host_family(exe, tmp_path)
    assert [table[(label, False)][:2] for label in ("negP", "shift3", "negated")] == [(1, 32), (1, 32), (2, 32)]
    assert [table[(label, True)][:2] for label in ("negP", "shift3", "negated")] == [(0, 48), (0, 48), (0, 48)]
    nb = rp.NB
    first = rp.family()[:3]
    assert [p.label for p in first] == ["full", "dep8", "emptyP"]
    for p, (pen, kept_want) in enumerate(zip(first, (48, 40, 32))):
        A, B = pen.A, pen.B
        theta, Cf, status, kept = results[False][p]
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


def test_the_reference_of_the_pencils_against_mpmath():
    """scipy.linalg.eigh of the deflated pencil (T, G) is what every Rayleigh-Ritz result is judged against: its own distance
    from the values at 40 digits (mpmath), on the five pencils with the largest cond(G), stays inside a quarter of the bound on
    theta it serves (what is judged against it keeps the rest)."""
    cases = []
    for p in rp.checked_family():
        for status in sorted({s for s, _ in p.expect.values()} - {rp.RITZ_BREAKDOWN}):
            cases.append((rp.reference(p, status)["cond"], p.label, status))
    cases.sort(reverse=True)
    seen, hardest = set(), []
    for cond, label, status in cases:  # (a retried pencil is its zeroed twin: one of them)
        if round(cond, 6) not in seen:
            seen.add(round(cond, 6))
            hardest.append((cond, label, status))
    for cond, label, status in hardest[:5]:
        ratio = rp.mpmath_distance(rp.by_label()[label], status)
        print(f"{label} (status {status}): cond(G) = {cond:.3g}, |eigh - mpmath| / theta bound = {ratio:.3g}")
        assert ratio <= 0.25, (label, ratio)


def test_argument_errors():
    fg, results, _ = reference("2x20")
    for kw in (dict(k=0), dict(k=17), dict(k=2.5), dict(rel_tol=0.0), dict(rel_tol=-1e-9), dict(max_iters=0), dict(shift=0.0),
               dict(shift=-1e-8), dict(engine="eager")):
        with pytest.raises(ValueError):
            information_spectrum(fg, results, **{"engine": "python", **kw})
