"""What the posterior-sample tests share: the graphs and dense references of tests/marginals_helpers.py, the Jacobian in the
library's (m, q) row order, and the derived bounds.

Right-hand side.  b = J'z sums, per unknown, one product per non-zero of its column of J.  The device's z differs from the
NumPy restatement's by at most 1e-12 per component (the project's tolerance for device normals against a host restatement,
tests/test_generate.py), which reaches b through |J|; a sum of k products in any order carries at most (k + 1) eps times
the sum of their absolute values.  Entrywise:

    |b_dev - J' z_py|  <=  |J|' (1e-12 * 1)  +  (longest column of J + 1) eps |J|' |z_py|.

Solve.  delta_ref is the Cholesky solve of the dense H with b_py, rho_ref its residual in np.longdouble, and
delta_rounding = (longest row + 1) eps || |H| |delta_ref| ||_2 the rounding of a residual computed in double.  From
H (delta_dev - delta_ref) = (b_py - H delta_ref) - (b_dev - H delta_dev) + (b_dev - b_py):

    || delta_dev - delta_ref ||_2  <=  (rho_s + delta_rounding + rho_ref + || b_dev - b_py ||_2) / lambda_min(H).

Every term is computed here; no tolerance is chosen."""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.stats

from marginals_helpers import EPS, Reference, landmark_names, pose_names, reference
from score_amd.marginals import _select
from score_amd.refine import _Problem3D
from score_amd.samples import SamplesHandle, noise_block, ordered_jacobian

NOISE_ATOL = 1e-12


def everything(fg):
    """Every variable with unknowns, in the order of the unknowns."""
    return [nm for ch in pose_names(fg) for nm in ch][1:] + landmark_names(fg)


class Twin:
    """The python side of one graph at the test's point: the marginals' Reference, J in the (m, q) order and what the
    bounds need of it.  Computed once and left unchanged."""

    def __init__(self, fg, results, ref):
        self.fg, self.results, self.ref = fg, results, ref
        self.J = ordered_jacobian(ref.prob, ref.point).tocsr()
        self.absJ = abs(self.J)
        self.longest_column = int(np.max(np.diff(self.J.tocsc().indptr)))
        self.names = everything(fg)
        self.ids = _select(ref.prob, self.names)[1]

    def noise(self, seed, first_sample, n_samples):
        return noise_block(self.ref.prob, seed, first_sample, n_samples)

    def rhs(self, z):
        return (self.J.T @ z.T).T

    def rhs_bound(self, z):
        ones = np.ones(self.J.shape[0])
        return (self.absJ.T @ (NOISE_ATOL * ones))[None, :] + (self.longest_column + 1) * EPS * (self.absJ.T @ np.abs(z).T).T

    def solve(self, b):
        """delta_ref (S x n), rho_ref (S, from np.longdouble), delta_rounding (S)."""
        ref = self.ref
        X = sla.cho_solve(ref.chol, b.T)
        R = b.T.astype(np.longdouble) - ref.H.astype(np.longdouble) @ X.astype(np.longdouble)
        rho_ref = np.sqrt(np.sum(R * R, axis=0)).astype(np.float64)
        rounding = (ref.longest_row + 1) * EPS * np.linalg.norm(ref.absH @ np.abs(X), axis=0)
        return X.T, rho_ref, rounding


@functools.lru_cache(maxsize=None)
def twin(key):
    fg, results, ref = reference(key)
    return Twin(fg, results, ref)


def weighted_twin(fg, results, range_weights):
    return Twin(fg, results, Reference(fg, results, range_weights))


def device_draws(tw, hip_lib, n_samples, **kw):
    """One ``score_refine_samples`` call with every variable selected and the diagnostics asked for."""
    with SamplesHandle(tw.ref.prob, hip_lib) as h:
        return h.draw(tw.ref.point, tw.ids, n_samples, with_rhs=True, with_noise=True, **kw)


def check_noise(tw, out, seed, first_sample, label):
    z = tw.noise(seed, first_sample, out["noise"].shape[0])
    worst = float(np.max(np.abs(out["noise"] - z)))
    print(f"{label}: noise, worst |device - numpy| = {worst:.3e}")
    assert out["noise"].shape == z.shape and worst <= NOISE_ATOL
    return z


def check_rhs(tw, out, z, label):
    b_py, bound = tw.rhs(z), tw.rhs_bound(z)
    diff = np.abs(out["rhs"] - b_py)
    print(f"{label}: right-hand side, worst |b_dev - J'z| / bound = {float(np.max(diff / bound)):.3e} "
          f"(longest column {tw.longest_column})")
    assert np.all(bound > 0) and np.all(diff <= bound)
    return b_py


def check_solve(tw, out, b_py, label):
    ref = tw.ref
    assert out["rc"] == 0 and np.all(out["converged"]), f"{label}: {out['iterations']}"
    X, rho_ref, rounding = tw.solve(b_py)
    delta = out["steps"]  # (every variable is selected: the steps are the full solutions)
    assert delta.shape == X.shape
    db = np.linalg.norm(out["rhs"] - b_py, axis=1)
    err = np.linalg.norm(delta - X, axis=1)
    bound = (out["residuals"] + rounding + rho_ref + db) / ref.lambda_min
    # the reported residual against one recomputed with the dense H (in np.longdouble: what is left is the device's own
    # rounding -- of its product, `rounding`, and of its sum of n squares, (n + 1) eps relative)
    R = out["rhs"].T.astype(np.longdouble) - ref.H.astype(np.longdouble) @ delta.T.astype(np.longdouble)
    mine = np.sqrt(np.sum(R * R, axis=0)).astype(np.float64)
    print(f"{label}: solve, worst error / bound = {float(np.max(err / bound)):.3e}, worst residual {float(np.max(out['residuals'])):.3e}, "
          f"worst |reported - recomputed| / rounding = {float(np.max(np.abs(out['residuals'] - mine) / rounding)):.3e}")
    assert np.all(np.abs(out["residuals"] - mine) <= rounding + (ref.n + 1) * EPS * mine)
    assert np.all(err <= bound), f"{label}: draw {int(np.argmax(err - bound))}"


def fixed_order_moments(prob_dims, delta):
    """(moments, means, sum of absolute terms of each) from full steps, draws added in ascending order."""
    Np, Nl, dp, d = prob_dims
    npu = dp * (Np - 1)
    Mp, Ml, Ap, Al = np.zeros((Np - 1, dp, dp)), np.zeros((Nl, d, d)), np.zeros((Np - 1, dp, dp)), np.zeros((Nl, d, d))
    mean, amean = np.zeros(delta.shape[1]), np.zeros(delta.shape[1])
    for row in delta:
        P, L = row[:npu].reshape(-1, dp), row[npu:].reshape(-1, d)
        tp, tl = P[:, :, None] * P[:, None, :], L[:, :, None] * L[:, None, :]
        Mp += tp; Ml += tl; Ap += np.abs(tp); Al += np.abs(tl)
        mean += row; amean += np.abs(row)
    return (np.concatenate([Mp.ravel(), Ml.ravel()]), mean, np.concatenate([Ap.ravel(), Al.ravel()]), amean)


def dims(prob):
    d = 3 if isinstance(prob, _Problem3D) else 2
    return prob.Np, prob.Nl, (6 if d == 3 else 3), d


def check_distribution(tw, delta, covariance, label):
    """T = sum_s delta_s' H delta_s ~ chi^2(n S), and per variable and diagonal entry S M_v[a, a] / Sigma_v[a, a] ~ chi^2(S):
    both inside the 1e-6 quantiles (the second shared over the n entries tested).  delta: S x n full steps; covariance:
    name -> M_v / S."""
    ref = tw.ref
    S, n = delta.shape
    T = float(np.einsum("si,ij,sj->", delta, ref.H, delta))
    lo, hi = scipy.stats.chi2.ppf(1e-6, n * S), scipy.stats.chi2.isf(1e-6, n * S)
    print(f"{label}: T = {T:.1f} in chi^2({n * S}) quantiles [{lo:.1f}, {hi:.1f}]")
    assert lo <= T <= hi
    Sigma = np.linalg.inv(ref.H)
    names, cols = ref.columns(tw.names)
    ratio = np.empty(n)
    at = 0
    for nm in names:
        M = covariance(nm)
        k = M.shape[0]
        ratio[at:at + k] = S * np.diag(M) / np.diag(Sigma)[cols[at:at + k]]
        at += k
    assert at == n
    lo, hi = scipy.stats.chi2.ppf(1e-6 / n, S), scipy.stats.chi2.isf(1e-6 / n, S)
    print(f"{label}: S M/Sigma in [{ratio.min():.2f}, {ratio.max():.2f}], chi^2({S}) quantiles [{lo:.2f}, {hi:.2f}] over {n} entries")
    assert np.all(ratio >= lo) and np.all(ratio <= hi)

