"""Predicted relative poses on the host: ``relative_jacobians`` against central differences of the definitions, rp_pair_jac of
csrc/score_relative.hpp as a stand-alone program (plain and under the host sanitizers) against ``relative_jacobians``, the
Python engine and the gate on graph a, and the binding table.  The bounds are derived in tests/relative_helpers.py.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import relative_helpers as rh
from marginals_helpers import EPS, reference
from score_amd.bindings import LATER_TABLES, RELATIVE, TABLES, TABLES_AFTER, TABLES_LATEST, TABLES_SINCE, bind
from score_amd.marginals import marginal_covariances
from score_amd.refine import _point_arrays, so3_exp, unknown_sizes
from score_amd.relative import (RELATIVE_SYMBOLS, PredictedRelativePoses, RelativeHandle, _rotations_and_translations,
                                measurement_noise, predicted_relative_poses, relative_jacobians, so3_log, wrap_angle)
from test_binding_tables_host import SCALARS, _declarations, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs(prob):
    """(0, k), (k, 0), the two neighbours of one chain (both orders), two poses of different robots, and ten of the list."""
    Np = prob.Np
    fixed = [(0, 7), (7, 0), (11, 12), (12, 11), (5, Np // 2 + 9), (Np - 1, 3), (0, Np // 2), (1, 0)]
    return np.concatenate([np.asarray(fixed, dtype=np.int32), rh.pair_list(prob, 10)])


@pytest.mark.parametrize("key", ["a", "d"])
def test_jacobians_against_central_differences(key):
    """The test that decides the formulas of include/score_relative.h."""
    _, _, ref = reference(key)
    prob = ref.prob
    d, dp = unknown_sizes(prob)
    ids = _pairs(prob)
    G, Rab, tab = relative_jacobians(prob, ref.point, ids)
    fd, bound, defect = rh.finite_difference_jacobians(prob, ref.point, ids)
    err = np.abs(G - fd)
    print(f"{key}: {len(ids)} pairs, h = {rh.FD_STEP:.3e}, worst |G - differences| = {err.max():.3e}, worst / bound = "
          f"{float(np.max(err / bound)):.3e}, bounds {bound.min():.3e} .. {bound.max():.3e}, |t_ab| up to "
          f"{np.linalg.norm(tab, axis=1).max():.2f}, orthogonality defect {defect:.2e}")
    assert G.shape == (prob.n, len(ids) * dp) and np.all(err <= bound)
    assert bound.max() < 1e-8  # (the bound decides: an entry of G that matters is of order 1 or |t_ab|)
    # every pair has dp independent gradients; a pair on pose 0 has them on its other end alone
    for c, (a, b) in enumerate(ids):
        g = G[:, c * dp:(c + 1) * dp]
        assert np.linalg.matrix_rank(g) == dp
        rows = np.flatnonzero(np.any(g != 0, axis=1))
        allowed = np.concatenate([np.arange(dp * (v - 1), dp * v) for v in (a, b) if v >= 1])
        assert set(rows) <= set(allowed) and (min(a, b) >= 1 or len(rows) <= dp)
    # and the definitions themselves: the prediction composes
    R, t = _rotations_and_translations(prob, ref.point)
    for c, (a, b) in enumerate(ids):
        np.testing.assert_allclose(R[a] @ Rab[c], R[b], atol=16 * EPS)
        np.testing.assert_allclose(t[a] + R[a] @ tab[c], t[b], atol=16 * EPS * (1 + np.abs(t[[a, b]]).max()))


def _program(tmp_path, name, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / name)
    subprocess.run([gxx, "-std=c++17", *flags, "-I", os.path.join(ROOT, "score_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "relative_jac_check.cpp")], check=True)
    return exe


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitizers"])
def test_device_text_on_the_host_against_numpy(tmp_path, flags):
    """tests/tools/relative_jac_check.cpp: rp_pair_jac as g++ compiles it, entry by entry against ``relative_jacobians``
    within JAC_ULPS eps of the entry's sum |terms| -- structural zeros and the constants +-1 exactly."""
    exe = _program(tmp_path, "relative_jac_check", flags)
    for key in ("a", "d"):
        _, _, ref = reference(key)
        prob = ref.prob
        d, dp = unknown_sizes(prob)
        ids = _pairs(prob)
        poses, _ = _point_arrays(prob, ref.point)
        path = tmp_path / f"points_{key}.txt"
        with open(path, "w") as f:
            f.write(f"{d} {prob.Np} {len(ids)}\n")
            f.write("\n".join(" ".join(float(x).hex() for x in row) for row in poses) + "\n")
            f.write("\n".join(f"{a} {b}" for a, b in ids) + "\n")
        run = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        lines = run.stdout.strip().splitlines()
        assert len(lines) == len(ids)
        G, Rab, tab = relative_jacobians(prob, ref.point, ids)
        R, t = _rotations_and_translations(prob, ref.point)
        keep = rh.structure(d)
        worst = 0.0
        for c, (ln, (a, b)) in enumerate(zip(lines, ids)):
            words = ln.split()
            assert words[:3] == ["pair", str(a), str(b)]
            v = np.array([float.fromhex(w) for w in words[3:]])
            assert len(v) == d * d + d + 2 * dp * dp
            R_t, t_t, G_t = v[:d * d].reshape(d, d), v[d * d:d * d + d], v[d * d + d:].reshape(dp, 2 * dp)
            B, BR, Bt = rh.jacobian_scale(R[a], t[a], R[b], t[b])
            assert np.all(G_t[~keep] == 0.0) and np.all(B[~keep] == 0.0)
            assert np.all(np.abs(R_t - Rab[c]) <= rh.JAC_ULPS * EPS * BR) and np.all(np.abs(t_t - tab[c]) <= rh.JAC_ULPS * EPS * Bt)
            for v_id, first in ((a, 0), (b, dp)):  # (pose 0 has no columns in NumPy's G: the program's are not compared)
                if v_id < 1:
                    continue
                mine = G[dp * (v_id - 1):dp * v_id, c * dp:(c + 1) * dp].T
                gap, room = np.abs(G_t[:, first:first + dp] - mine), rh.JAC_ULPS * EPS * B[:, first:first + dp]
                assert np.all(gap <= room), (key, a, b)
                worst = max(worst, float(np.max(gap[room > 0] / room[room > 0])))
                ones = np.abs(mine) == 1.0
                assert np.array_equal(G_t[:, first:first + dp][ones & (room == 0)], mine[ones & (room == 0)])
        print(f"{key} {flags[0]}: {len(ids)} pairs, worst |program - NumPy| / ({rh.JAC_ULPS} eps sum|terms|) = {worst:.3e}")


def test_python_engine_and_the_gate():
    fg, results, ref = reference("a")
    prob = ref.prob
    names = list(prob.a["pose_names"])
    pairs = [("A10", "B7"), ("A0", "B20"), ("B3", "A0"), ("A11", "A12"), ("B24", "A1")]
    pred, info = predicted_relative_poses(fg, results, pairs, engine="python")
    assert isinstance(pred, PredictedRelativePoses) and info["engine"] == "python" and pred.pairs == pairs and pred.dof == 3
    assert pred.covariance.shape == (5, 3, 3) and pred.rotation.shape == (5, 2, 2) and pred.angle.shape == (5,)
    assert np.all(np.abs(pred.angle) <= np.pi) and info["residuals"].shape == (5, 3) and info["asymmetry"] < 1e-9
    # P = G'Sigma G with Sigma the joint marginal of the two ends
    ids = np.array([[names.index(a), names.index(b)] for a, b in pairs])
    G, Rab, tab = relative_jacobians(prob, ref.point, ids)
    np.testing.assert_array_equal(pred.rotation, Rab)
    np.testing.assert_array_equal(pred.translation, tab)
    for c, (a, b) in enumerate(pairs):
        ends = [nm for nm in (a, b) if nm != names[0]]
        _, minfo = marginal_covariances(fg, results, variables=ends, joint=True, engine="python")
        rows = np.concatenate([np.arange(3 * (names.index(nm) - 1), 3 * names.index(nm)) for nm in ends])
        g = G[rows, 3 * c:3 * c + 3]
        want = g.T @ minfo["joint"] @ g
        # both sides: a dense solve of the same H (condition kappa = |H| / lambda_min), then 6-term products
        room = 64 * EPS * np.linalg.norm(ref.H, 2) / ref.lambda_min * np.abs(want).max()
        assert np.all(np.abs(pred.covariance[c] - want) <= room), (a, b)
        assert np.all(np.linalg.eigvalsh(pred.covariance[c]) > 0)
    # the gate: the prediction's own relative pose has d2 = 0; an innovation e has e'(P + N)^-1 e
    kappa, tau = 4.0, 9.0
    d2, dof = pred.gate([(R, t) for R, t in zip(pred.rotation, pred.translation)], kappa, tau)
    assert dof == 3 and np.all(d2 == 0.0)
    e = np.array([[0.05, 0.3, -0.2], [-0.4, 1.0, 2.0], [3.1, 0.0, 0.0], [0.0, -0.01, 0.02], [-2.0, 5.0, 5.0]])
    meas = []
    for c in range(5):
        th = pred.angle[c] + e[c, 0]
        meas.append((np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]), pred.translation[c] + e[c, 1:]))
    inn = pred.innovation(meas)
    np.testing.assert_allclose(inn, e, atol=64 * EPS * (1 + np.abs(pred.translation).max()))
    d2, _ = pred.gate(meas, kappa, tau)
    N = np.diag([1 / (2 * tau), 1 / kappa, 1 / kappa])
    for c in range(5):
        want = inn[c] @ np.linalg.inv(pred.covariance[c] + N) @ inn[c]
        assert d2[c] == pytest.approx(want, rel=1e-12) and d2[c] > 0
    np.testing.assert_array_equal(measurement_noise(2, kappa, tau, 1)[0], N)
    # objects with the loop closures' attributes work like tuples
    lc = fg.loop_closure_measurements[0]
    one = PredictedRelativePoses(pairs[:1], pred.rotation[:1], pred.translation[:1], pred.covariance[:1])
    np.testing.assert_array_equal(one.innovation([lc]), one.innovation([(lc.rotation_matrix, lc.translation_vector)]))
    # wrap: theta_m - theta_ab across the cut
    assert wrap_angle(np.pi) == np.pi and wrap_angle(-np.pi) == np.pi and abs(wrap_angle(3.0 + 3.5 - 2 * np.pi) - 0.21681469) < 1e-8
    # the information gain is positive and grows with the precisions
    g1, g2, g3 = pred.information_gain(kappa, tau), pred.information_gain(2 * kappa, tau), pred.information_gain(kappa, 2 * tau)
    assert np.all(g1 > 0) and np.all(g2 > g1) and np.all(g3 > g1)
    for c in range(5):
        want = 0.5 * np.linalg.slogdet(np.eye(3) + np.linalg.inv(N) @ pred.covariance[c])[1]
        assert g1[c] == pytest.approx(want, rel=1e-12)
    # refusals before any call
    for bad, words in (([("A3", "L0")], "is a landmark"), ([("A3", "A3")], "to itself"), ([("A3", "Z9")], "unknown variable"), ([], "no pairs")):
        with pytest.raises(ValueError, match=words):
            predicted_relative_poses(fg, results, bad, engine="python")
    with pytest.raises(ValueError, match="engine"):
        predicted_relative_poses(fg, results, pairs, engine="numpy")
    with pytest.raises(ValueError, match="block_width"):
        predicted_relative_poses(fg, results, pairs, block_width=17, engine="python")
    with pytest.raises(ValueError, match="positive"):
        pred.gate(meas, 0.0, tau)


def test_python_engine_in_3d():
    fg, results, ref = reference("d")
    pairs = [("A4", "B9"), ("A0", "B2"), ("B5", "A0")]
    pred, info = predicted_relative_poses(fg, results, pairs, engine="python")
    assert pred.dof == 6 and pred.angle is None and pred.covariance.shape == (3, 6, 6)
    names = list(ref.prob.a["pose_names"])
    ids = np.array([[names.index(a), names.index(b)] for a, b in pairs])
    want, _, _ = rh.dense_covariances(ref, ids)
    np.testing.assert_array_equal(pred.covariance, 0.5 * (want + np.swapaxes(want, 1, 2)))  # (the same H, G and Cholesky solve)
    assert np.all(np.linalg.eigvalsh(pred.covariance) > 0)
    assert info["asymmetry"] == np.abs(want - np.swapaxes(want, 1, 2)).max()
    w = np.array([[0.2, -0.1, 0.3], [1.0, 2.0, -0.5], [0.0, 0.0, 1e-3]])
    np.testing.assert_allclose(so3_log(so3_exp(w)), w, atol=64 * EPS)
    e = np.concatenate([w, [[0.1, 0.2, 0.3], [-1.0, 0.5, 2.0], [0.0, 0.0, 0.0]]], axis=1)
    meas = [(pred.rotation[c] @ so3_exp(e[c, :3]), pred.translation[c] + e[c, 3:]) for c in range(3)]
    np.testing.assert_allclose(pred.innovation(meas), e, atol=256 * EPS * (1 + np.abs(pred.translation).max()))
    zero, dof = pred.gate(list(zip(pred.rotation, pred.translation)), 4.0, 9.0)
    assert dof == 6 and np.all(zero <= (64 * EPS) ** 2 * 6 * 18.0)  # (Log of R_ab'R_ab: the defect of a stored rotation, squared, times |N^-1|)
    d2, _ = pred.gate(meas, 4.0, 9.0)
    N = np.diag([1 / 18.0] * 3 + [1 / 4.0] * 3)
    inn = pred.innovation(meas)
    for c in range(3):
        assert d2[c] == pytest.approx(inn[c] @ np.linalg.inv(pred.covariance[c] + N) @ inn[c], rel=1e-12)
    assert np.all(pred.information_gain(4.0, 9.0) > 0)


def test_table_matches_header():
    table = RELATIVE
    assert TABLES_LATEST == (RELATIVE,) and table.name == "relative"
    assert all(table not in group for group in (TABLES, LATER_TABLES, TABLES_SINCE, TABLES_AFTER))
    assert RELATIVE in RelativeHandle.headers
    declared = _declarations(table.name)
    assert sorted(declared) == sorted(table) == sorted(RELATIVE_SYMBOLS) == ["score_refine_relative_covariances"]
    lib = bind(_Stub(), table)
    assert bind(lib, table) is lib  # (bound once)
    for sym, params in declared.items():
        argtypes, restype = table[sym]
        assert restype is C.c_int and lib.__dict__[sym].argtypes == argtypes and len(argtypes) == len(params) == 16, sym
        for param, typ in zip(params, argtypes):
            is_pointer = typ is C.c_void_p or hasattr(typ, "contents")
            assert ("*" in param) == is_pointer, (sym, param, typ)
            if not is_pointer:
                assert SCALARS[param.split()[-2]] is typ, (sym, param, typ)


def test_missing_symbol():
    sym = list(RELATIVE)[-1]
    with pytest.raises(RuntimeError, match=re.escape(f"{sym} is missing from the library: rebuild it "
                                                     "(the CPU twin has no relative-pose covariances: engine='python' runs there)")):
        bind(_Stub(lacks=sym), RELATIVE)
