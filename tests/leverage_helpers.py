"""What the leverage tests share: the thinned-beacon graph, the pairs, the expected sums of score_refine_leverage and the derived
bounds.  The graphs, points and dense references are those of tests/marginals_helpers.py / tests/samples_helpers.py.

Sums.  The device forms, per measurement m and converged draw s, y_q = sum_e J[q, e] d_e over the measurement's local unknowns
(k terms: 2 dp of a relative pose, 2 d of a range, 1 of a prior), o_q = z_q - y_q, t = sum_q y_q^2, v = sum_q o_q^2, and adds
t, t^2, v, v^2 over the draws in ascending s.  The expectation is computed from the DEVICE's own steps d (every variable
selected: the steps are the block's solutions bit for bit), NumPy's J and NumPy's noise, in np.longdouble, so that what is
left is the device's rounding and the two inputs it does not share with NumPy:

* z: the project's tolerance for device normals against the host restatement, NOISE_ATOL = 1e-12 per component;
* J: both sides compute it in double from the same point through their own libm (sin / cos of a 2-D heading), sqrt of the
  precisions and sums of up to 3 x 3 products that can cancel (d(R_i tm)/dtheta, R_i [e_c]x Rm); per entry that is at most
  J_ULPS eps times the largest entry of the measurement's block (which is >= sqrt(kappa) and >= sqrt(tau) / sqrt(3): an
  entry that cancelled is small against it).  J_ULPS = 64 covers two nested 3-term sums on both sides (2 x (3 + 3 + 2) eps
  of terms <= 3 sqrt(tau), against sqrt(tau) / sqrt(3)); structural zeros are exact zeros on both sides.

With A = |J| |d| per row and B = max|J_m| sum_e |d_e| over the row's pattern:

    ey_q = (k + 1) eps A_q + J_ULPS eps B_q                       (a k-term product sum in any order; the entries of J)
    eo_q = NOISE_ATOL + ey_q + eps |o_q|                          (z, y, the subtraction)
    et   = sum_q (2 |y_q| ey_q + ey_q^2) + (R + 1) eps t          (the squares, their products' rounding and R additions)
    ev   = the same with o, eo
    |lev_sum - sum_s t|   <= sum_s et + (S + 1) eps sum_s t        (S + 1 additions, the zero included)
    |lev_sq - sum_s t^2|  <= sum_s (2 t et + et^2) + (S + 2) eps sum_s t^2
and the same for red_sum / red_sq with v, ev.  A pair's g = (u, -u) is a range's Jacobian at precision 1: the same formulas
with k = 2 d and one row.  Every term is computed from NumPy's values; no tolerance is chosen.

Range variances.  x_ref is the Cholesky solve of the dense H with NumPy's g, rho_ref its residual in np.longdouble, rounding
the rounding of a residual in double (marginals_helpers), dg = G_ULPS eps |g| the difference of the two g.  Each side forms
u_k = dv_k / rho with w = eps / 2 per operation: dv_k = a_k - b_k (w), its square (2 w + w), the sum of d <= 3 squares
((d - 1) w more: (d + 2) w on rho^2), the root (half of that, + w), the quotient (w of dv, rho's, + w):
(3 + (d + 2) / 2) w <= 5.5 w = 2.75 eps per side, 5.5 eps for the two, so G_ULPS = 8 (a fused multiply-add only drops
roundings).  From H (x - x_ref) = (g_np - H x_ref) - (g_dev - H x) + (g_dev - g_np):

    |x - x_ref|_2 <= (residual + rounding + rho_ref + dg) / lambda_min
    |variance - g'x_ref| <= |g| |x - x_ref|_2 + dg |x_ref|_2 + (2 d + 1) eps |g|' |x_ref|       (the last: the dot itself).

The entry point's `solutions` output gives x itself, so the reported residual is held from both sides against
|g_np - H x|_2 recomputed in np.longdouble with the dense H: what is left is the device's own rounding -- of its product
(`rounding`, with |x| for |x_ref|), of its sum of n squares ((n + 1) eps relative) -- and dg; and the reported variance
against g_np'x within dg |x|_2 + (2 d + 1) eps |g|'|x|.
"""
import functools

import numpy as np
import scipy.linalg as sla

from marginals_helpers import EPS, Reference, noisy_truth
from samples_helpers import NOISE_ATOL, Twin
from score_amd.leverage import _row_groups, measurement_counts, pair_gradients
from score_amd.manhattan import make_manhattan
from score_amd.refine import _Problem3D

J_ULPS = 64
G_ULPS = 8
SUMS = ("lev_sum", "lev_sq", "red_sum", "red_sq")


def thinned_graph():
    """One robot, two beacons, every pose ranged to both; the ranges to the last beacon thinned to its 2nd and 9th.  Two ranges
    are the least that fix a 2-D landmark: nothing else controls them, their leverage is 1 (indices 2 and 10 of the remaining
    range list), every other range has h in 0.087 .. 0.541."""
    fg = make_manhattan(n_robots=1, n_poses=12, n_beacons=2, seed=5, p_range=1.0)
    last = fg.landmark_variables[-1].name
    keep, seen = [], 0
    for r in fg.range_measurements:
        if last in r.association:
            seen += 1
            if seen not in (2, 9):
                continue
        keep.append(r)
    fg.range_measurements = keep
    return fg


THINNED = [2, 10]


@functools.lru_cache(maxsize=None)
def thinned_twin():
    fg = thinned_graph()
    results = noisy_truth(fg)
    return Twin(fg, results, Reference(fg, results))


def pair_list(prob, count, on_first_landmark=False):
    """`count` pairs of variable ids: pose - landmark, the fixed first pose - pose, pose - pose half the poses apart (across
    the robots where there are two), landmark - pose, in turn; on_first_landmark: every pair ends at landmark 0."""
    Np, Nl = prob.Np, prob.Nl
    out = []
    for k in range(count):
        p = 1 + (7 * k + 3) % (Np - 1)
        if on_first_landmark:
            out.append((p, Np) if k % 2 == 0 else (Np, p))
        elif k % 4 == 0:
            out.append((p, Np + k % Nl))
        elif k % 4 == 1:
            out.append((0, p))
        elif k % 4 == 2:
            out.append((p, 1 + (p + Np // 2) % (Np - 1)))
        else:
            out.append((Np + k % Nl, p))
    ids = np.asarray(out, dtype=np.int32).reshape(-1, 2)
    assert np.all(ids[:, 0] != ids[:, 1])
    return ids


def _terms(prob):
    """Per measurement the terms of a row's product sum on the device: its local unknowns."""
    d = 3 if isinstance(prob, _Problem3D) else 2
    n_rel, n_rng, n_pri = measurement_counts(prob)
    return np.concatenate([np.full(n_rel, 4 * d if d == 3 else 6), np.full(n_rng, 2 * d), np.ones(n_pri)]).astype(np.int64)


def _fold(t, et, S):
    """(sum, bound of the sum, sum of squares, bound of it) of per-draw values t (S x M, np.longdouble) with errors et."""
    t64 = t.astype(np.float64)
    s1, s2 = np.sum(t, axis=0).astype(np.float64), np.sum(t * t, axis=0).astype(np.float64)
    b1 = np.sum(et, axis=0) + (S + 1) * EPS * s1
    b2 = np.sum(2 * t64 * et + et * et, axis=0) + (S + 2) * EPS * s2
    return s1, b1, s2, b2


def expected_sums(tw, delta, z, ids=None):
    """(sums, bounds) of the module's docstring for the draws delta (S x n: the device's steps of the CONVERGED draws) and
    their noise z (S x rows, NumPy's): dicts over SUMS and, with ids, "pair_sum" / "pair_sq"."""
    prob = tw.ref.prob
    S = len(delta)
    first, rows = _row_groups(prob)
    J = np.asarray(tw.J.todense(), dtype=np.float64)
    absJ, pattern = np.abs(J), (J != 0).astype(np.float64)
    m_of_row = np.repeat(np.arange(len(rows)), rows)
    jmax = np.maximum.reduceat(np.max(absJ, axis=1), first)[m_of_row] if len(rows) else np.zeros(0)
    k = _terms(prob)[m_of_row]
    ld = np.longdouble
    Y = delta.astype(ld) @ J.T.astype(ld)
    O = z.astype(ld) - Y
    absd = np.abs(delta)
    ey = (k + 1) * EPS * (absd @ absJ.T) + J_ULPS * EPS * jmax * (absd @ pattern.T)
    eo = NOISE_ATOL + ey + EPS * np.abs(O).astype(np.float64)

    def per_measurement(V, eV):
        t = np.add.reduceat(V * V, first, axis=1)
        et = np.add.reduceat(2 * np.abs(V).astype(np.float64) * eV + eV * eV, first, axis=1) + (rows + 1) * EPS * t.astype(np.float64)
        return _fold(t, et, S)

    sums, bounds = {}, {}
    sums["lev_sum"], bounds["lev_sum"], sums["lev_sq"], bounds["lev_sq"] = per_measurement(Y, ey)
    sums["red_sum"], bounds["red_sum"], sums["red_sq"], bounds["red_sq"] = per_measurement(O, eo)
    if ids is not None:
        G, _ = pair_gradients(prob, tw.ref.point, ids)
        d = 3 if isinstance(prob, _Problem3D) else 2
        y = delta.astype(ld) @ G.astype(ld)
        ey = (2 * d + 1) * EPS * (absd @ np.abs(G)) + J_ULPS * EPS * (absd @ (G != 0).astype(np.float64))  # (max |u| <= 1)
        t = y * y
        et = 2 * np.abs(y).astype(np.float64) * ey + ey * ey + 2 * EPS * t.astype(np.float64)
        sums["pair_sum"], bounds["pair_sum"], sums["pair_sq"], bounds["pair_sq"] = _fold(t, et, S)
    return sums, bounds


def check_sums(tw, out, delta, z, ids, label, keys=None):
    """The device's sums against expected_sums; prints and returns the worst |device - expected| / bound."""
    want, bound = expected_sums(tw, delta, z, ids)
    worst = 0.0
    for key in (keys or tuple(want)):
        diff = np.abs(out[key] - want[key])
        assert out[key].shape == want[key].shape, key
        ratio = float(np.max(diff / np.where(bound[key] > 0, bound[key], 1.0))) if diff.size else 0.0
        worst = max(worst, ratio)
        bad = np.flatnonzero(diff > bound[key])
        assert bad.size == 0, f"{label}, {key}: entry {bad[:5]}: |device - expected| {diff[bad[:5]]} > bound {bound[key][bad[:5]]}"
    print(f"{label}: sums, worst |device - expected| / bound = {worst:.3e}")
    return worst, want, bound


def check_range_variances(tw, ids, out, label):
    """The bounds of the module's docstring for every pair: the variance against g'Sigma g, and -- `out` holds the call's
    `solutions` -- the reported residual and variance against |g - H x|_2 and g'x recomputed from x itself.  Prints the worst
    ratios."""
    ref = tw.ref
    prob = ref.prob
    d = 3 if isinstance(prob, _Problem3D) else 2
    G, dist = pair_gradients(prob, ref.point, ids)
    X = sla.cho_solve(ref.chol, G)
    Hl, Xl = ref.H.astype(np.longdouble), X.astype(np.longdouble)
    R = G.astype(np.longdouble) - Hl @ Xl
    rho_ref = np.sqrt(np.sum(R * R, axis=0)).astype(np.float64)
    rounding = (ref.longest_row + 1) * EPS * np.linalg.norm(ref.absH @ np.abs(X), axis=0)
    gnorm = np.linalg.norm(G, axis=0)
    dg = G_ULPS * EPS * gnorm
    want = np.einsum("ic,ic->c", G, X)
    bound = (gnorm * (out["residuals"] + rounding + rho_ref + dg) / ref.lambda_min + dg * np.linalg.norm(X, axis=0)
             + (2 * d + 1) * EPS * np.einsum("ic,ic->c", np.abs(G), np.abs(X)))
    err = np.abs(out["variances"] - want)
    print(f"{label}: {len(ids)} pairs, worst |variance - g'Sigma g| / bound = {float(np.max(err / bound)):.3e}, "
          f"worst relative error {float(np.max(err / want)):.3e}, worst residual {float(np.max(out['residuals'])):.3e}")
    assert out["rc"] == 0 and np.all(out["converged"]), f"{label}: {out['iterations']}"
    assert np.all(want > 0) and np.all(err <= bound), f"{label}: pair {int(np.argmax(err - bound))}"
    assert np.all(np.abs(out["distances"] - dist) <= 4 * EPS * dist)
    if out.get("solutions") is None:  # (the public function does not ask for them)
        return
    x = out["solutions"].T  # (n x C, as X)
    assert x.shape == X.shape
    Rx = G.astype(np.longdouble) - Hl @ x.astype(np.longdouble)
    mine = np.sqrt(np.sum(Rx * Rx, axis=0)).astype(np.float64)
    slack = (ref.longest_row + 1) * EPS * np.linalg.norm(ref.absH @ np.abs(x), axis=0) + (ref.n + 1) * EPS * mine + dg
    off = np.abs(out["residuals"] - mine)
    dot = np.einsum("ic,ic->c", G, x)
    dot_slack = dg * np.linalg.norm(x, axis=0) + (2 * d + 1) * EPS * np.einsum("ic,ic->c", np.abs(G), np.abs(x))
    print(f"{label}: worst |reported - recomputed residual| / slack = {float(np.max(off / slack)):.3e} (recomputed up to "
          f"{float(np.max(mine)):.3e}), worst |variance - g'x| / slack = {float(np.max(np.abs(out['variances'] - dot) / dot_slack)):.3e}")
    assert np.all(mine > 0) and np.all(off <= slack), f"{label}: pair {int(np.argmax(off - slack))}: {out['residuals']} against {mine}"
    assert np.all(np.abs(out["variances"] - dot) <= dot_slack)
    assert np.all(np.linalg.norm(x - X, axis=0) <= (out["residuals"] + rounding + rho_ref + dg) / ref.lambda_min)
