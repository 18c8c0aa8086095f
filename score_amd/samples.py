"""Draws from the Gaussian posterior of a refined estimate (include/score_samples.h): perturb-and-solve.

At the maximum-likelihood estimate the cost ``refine_estimate`` minimises is |r(x)|^2 with the whitened residual r and its
Jacobian J; H = J'J is the information matrix in the refinement's own unknowns -- (theta, x, y) per 2-D pose, (omega, v) of
the retraction R Exp(omega), t + v per 3-D pose, the coordinates of a landmark; the first pose of the first chain is fixed.
For z ~ N(0, I) the solution of H delta = J'z has covariance H^-1 J'J H^-1 = H^-1 exactly, so a draw of N(x_hat, H^-1) costs
one solve against H and needs no factor of it.  ``posterior_samples`` draws on the device (``score_refine_samples``: noise
and J'z of up to 16 draws in one pass over the measurements, the lock-step chain-preconditioned PCG of the marginals, and
the reduction of the draws to per-variable second moments without the draws leaving the device) and returns

* every variable's covariance block to a relative standard error of sqrt(2 / S) (``Samples.covariance``),
* the tangent steps of the selected variables draw by draw (``Samples.steps``) and the same retracted onto the estimate
  (``Samples.results``): error ellipses along a trajectory, the spread of any derived quantity, plausible worlds.

The noise is counter based (``ps_noise``: Philox4x32-10 keyed by the seed, counter = (13, measurement, draw, row pair),
Box-Muller): draw s is the same whatever the call it is part of.  A singular H does not stop a draw's solve (J'z lies in
the range of J'J), so the device call first solves one probe column H x = xi, xi random: where it fails, every draw is
reported as not converged and ``posterior_samples`` raises.  ``engine="python"`` is the dense twin for small graphs and
the tests: the same noise stream from NumPy, J from the host Jacobian, a dense Cholesky solve.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import SAMPLES, ScoreSamplesInfo, bind, ptr, steps_and_converged
from .marginals import MAX_BLOCK_WIDTH, MarginalsHandle, _problem_and_point, _select, n_columns
from .refine import _point_arrays, so3_exp, unknown_sizes
from .solver import _i32p
from .spectrum import _layout

# the symbols include/score_samples.h declares
SAMPLES_SYMBOLS = list(SAMPLES)
GEN_SAMPLE = 13  # the Philox purpose of the posterior noise (csrc/score_samples.hpp)

_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(key, c0, c1, c2, c3):
    """Philox4x32-10 (Salmon et al., SC'11) over arrays of counters: four uint64 arrays holding the 32-bit outputs."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64(key >> 32)
    x0, x1, x2, x3 = (np.asarray(c, dtype=np.uint64) & _MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = _M0 * x0, _M1 * x2  # (32 x 32 bits: no overflow in 64)
        x0, x1, x2, x3 = (p1 >> _S32) ^ x1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ x3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return x0, x1, x2, x3


def _u01(hi, lo):
    return (((hi << _S32) | lo) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def ps_noise(seed, m, s, q):
    """Component q of measurement m's noise in draw s (arrays broadcast): component q & 1 of the Box-Muller pair of
    Philox4x32-10(seed, (GEN_SAMPLE, m, s, q >> 1)) -- the stream of ``score_refine_samples``."""
    m, s, q = np.broadcast_arrays(np.asarray(m, dtype=np.int64), np.asarray(s, dtype=np.int64), np.asarray(q, dtype=np.int64))
    p = philox4x32_10(seed, np.full(m.shape, GEN_SAMPLE, dtype=np.uint64), m.astype(np.uint64), s.astype(np.uint64),
                      (q >> 1).astype(np.uint64))
    u, v = 1.0 - _u01(p[0], p[1]), _u01(p[2], p[3])
    r, a = np.sqrt(-2.0 * np.log(u)), 2.0 * np.pi * v
    return np.where(q & 1, r * np.sin(a), r * np.cos(a))


def measurement_rows(prob):
    """The residual rows in the library's (m, q) order: (perm, m, q) with row k of that order being row perm[k] of
    ``prob.residuals`` (which lists all translation rows, then all rotation rows, then ranges, then priors)."""
    d, _ = unknown_sizes(prob)
    n_rel, n_rng, n_pri = len(prob.bi), len(prob.ra), len(prob.pl)
    nr = d + d * d
    e = np.repeat(np.arange(n_rel, dtype=np.int64), nr)
    q = np.tile(np.arange(nr, dtype=np.int64), n_rel)
    rel = np.where(q < d, d * e + q, d * n_rel + d * d * e + (q - d))
    base = nr * n_rel
    perm = np.concatenate([rel, base + np.arange(n_rng, dtype=np.int64), base + n_rng + np.arange(d * n_pri, dtype=np.int64)])
    m = np.concatenate([e, n_rel + np.arange(n_rng, dtype=np.int64), n_rel + n_rng + np.repeat(np.arange(n_pri, dtype=np.int64), d)])
    qq = np.concatenate([q, np.zeros(n_rng, dtype=np.int64), np.tile(np.arange(d, dtype=np.int64), n_pri)])
    return perm, m, qq


def ordered_jacobian(prob, point):
    """The whitened Jacobian at the point as a sparse matrix with its rows in the (m, q) order."""
    _, J = prob.residuals(point, jac=True)
    return J.tocsr()[measurement_rows(prob)[0]]


def noise_block(prob, seed, first_sample, n_samples) -> np.ndarray:
    """z of the draws first_sample .. first_sample + n_samples - 1: (n_samples, rows) in the (m, q) order."""
    _, m, q = measurement_rows(prob)
    s = first_sample + np.arange(n_samples, dtype=np.int64)
    return ps_noise(seed, m[None, :], s[:, None], q[None, :])


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, SAMPLES)


def _moment_sizes(prob):
    d, dp = unknown_sizes(prob)
    return d, dp, dp * dp * (prob.Np - 1) + d * d * prob.Nl


def _n_rows(prob):
    d, _ = unknown_sizes(prob)
    return (d + d * d) * len(prob.bi) + len(prob.ra) + d * len(prob.pl)


class SamplesHandle(MarginalsHandle):
    """A refinement handle kept for several ``score_refine_samples`` calls on one graph."""

    headers = MarginalsHandle.headers + (SAMPLES,)

    def draw(self, point, ids, n_samples, seed=0, first_sample=0, rel_tol=1e-10, max_iters=4000, block_width=MAX_BLOCK_WIDTH,
             with_rhs=False, with_noise=False) -> dict:
        """``score_refine_samples`` as it is.  Returns a dict: ``rc``, ``moments`` and ``means`` (packed sums, as the header
        lays them out), ``steps`` (n_samples x C), ``rhs`` / ``noise`` (asked for: else None), ``residuals``, ``iterations``,
        ``converged`` and ``info`` (the call's record)."""
        prob = self.prob
        poses, lms = _point_arrays(prob, point)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        ncol = n_columns(prob, ids)
        S = max(int(n_samples), 0)
        moments = np.zeros(_moment_sizes(prob)[2])
        means = np.zeros(prob.n)
        steps = np.zeros((S, ncol))
        rhs = np.zeros((S, prob.n)) if with_rhs else None
        noise = np.zeros((S, _n_rows(prob))) if with_noise else None
        res = np.zeros(S)
        its = np.zeros(S, dtype=np.int32)
        info = ScoreSamplesInfo()
        rc = self.lib.score_refine_samples(self.h, ptr(poses), ptr(lms), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                           int(first_sample), int(n_samples), ptr(ids, _i32p), len(ids), float(rel_tol),
                                           int(max_iters), int(block_width), ptr(moments), ptr(means), ptr(steps), ptr(rhs),
                                           ptr(noise), ptr(res), ptr(its, _i32p), C.byref(info))
        if rc < 0:
            raise RuntimeError(f"score_refine_samples failed: {self.lib.score_last_error().decode()}")
        iterations, converged = steps_and_converged(its)
        return {"rc": rc, "moments": moments, "means": means, "steps": steps, "rhs": rhs, "noise": noise, "residuals": res,
                "iterations": iterations, "converged": converged, "info": info.as_dict()}


def accumulate_moments(prob, delta):
    """The packed sums of ``score_refine_samples`` from full steps delta (S x n): per variable the outer products added
    in ascending s, and the sums of delta."""
    d, dp, size = _moment_sizes(prob)
    npu = dp * (prob.Np - 1)
    Mp, Ml = np.zeros((prob.Np - 1, dp, dp)), np.zeros((prob.Nl, d, d))
    mean = np.zeros(prob.n)
    for row in np.asarray(delta, dtype=np.float64).reshape(-1, prob.n):
        P, L = row[:npu].reshape(-1, dp), row[npu:].reshape(-1, d)
        Mp += P[:, :, None] * P[:, None, :]
        Ml += L[:, :, None] * L[:, None, :]
        mean += row
    return np.concatenate([Mp.ravel(), Ml.ravel()]), mean


class Samples:
    """S draws of the posterior's tangent step.  ``count`` (S: the draws that entered), ``names`` (every variable with
    unknowns), ``order`` (the selected variables), ``steps`` (name -> (S, k) for the selected ones), ``mean(name)``,
    ``covariance(name)`` (any variable), ``standard_error``, ``results(s)``."""

    def __init__(self, prob, results, moments, means, count, order, sizes, steps, first_sample):
        names, first, size = _layout(prob)
        d, dp, _ = _moment_sizes(prob)
        self.names = names
        self.count = int(count)
        self.first_sample = int(first_sample)
        self.order = list(order)
        self._rows = {nm: (f, s) for nm, f, s in zip(names, first, size)}
        off = np.concatenate([[0], np.cumsum([s * s for s in size])])
        self._moment = {nm: (int(off[k]), s) for k, (nm, s) in enumerate(zip(names, size))}
        self._moments, self._means = np.asarray(moments, dtype=np.float64), np.asarray(means, dtype=np.float64)
        col = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64) if len(sizes) else np.zeros(1, dtype=np.int64)
        self.steps = {nm: steps[:, col[k]:col[k + 1]] for k, nm in enumerate(self.order)}
        self._dim = d
        self._estimate = {}
        poses = {str(nm) for nm in prob.a["pose_names"]}
        for nm in self.order:
            self._estimate[nm] = np.array((results.poses if nm in poses else results.landmarks)[nm], dtype=np.float64)

    @property
    def standard_error(self) -> float:
        """Relative standard error of a diagonal entry of ``covariance``: S M[a, a] / Sigma[a, a] ~ chi^2(S)."""
        return float(np.sqrt(2.0 / self.count))

    def _known(self, name):
        if str(name) not in self._rows:
            raise ValueError(f"posterior_samples: unknown variable {name} (the fixed first pose has no unknowns)")
        return str(name)

    def covariance(self, name) -> np.ndarray:
        """The k x k second moment M_v / S of the variable (not centred: the mean of a draw is zero)."""
        o, k = self._moment[self._known(name)]
        return self._moments[o:o + k * k].reshape(k, k) / self.count

    def mean(self, name) -> np.ndarray:
        f, k = self._rows[self._known(name)]
        return self._means[f:f + k] / self.count

    def results(self, s: int) -> dict:
        """Draw s (0-based within the call) of the selected variables retracted onto the estimate: name -> homogeneous
        matrix of a pose (theta + dtheta, t + v in 2-D; R Exp(omega), t + v in 3-D), name -> coordinates of a landmark."""
        out = {}
        for nm in self.order:
            step, est = self.steps[nm][s], self._estimate[nm]
            if est.ndim == 1:
                out[nm] = est + step
            elif self._dim == 2:
                th = np.arctan2(est[1, 0], est[0, 0]) + step[0]
                T = np.eye(3)
                T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
                T[:2, 2] = est[:2, 2] + step[1:]
                out[nm] = T
            else:
                T = np.eye(4)
                T[:3, :3] = est[:3, :3] @ so3_exp(step[:3])
                T[:3, 3] = est[:3, 3] + step[3:]
                out[nm] = T
        return out


def _python_draws(prob, point, seed, first_sample, n_samples):
    """The dense twin: (delta (S x n), b (S x n), z (S x rows), residuals)."""
    import scipy.linalg as sla

    J = np.asarray(ordered_jacobian(prob, point).todense(), dtype=np.float64)
    z = noise_block(prob, seed, first_sample, n_samples)
    b = z @ J
    H = J.T @ J
    try:
        delta = sla.cho_solve(sla.cho_factor(H, lower=True), b.T).T
    except np.linalg.LinAlgError:
        return None, b, z, np.full(n_samples, np.inf)
    return delta, b, z, np.linalg.norm(b - delta @ H, axis=1)


def _singular(failed, total, max_iters):
    return RuntimeError(f"posterior_samples: {failed} of {total} draws did not converge (max_iters = {max_iters}): J'J is singular or "
                        "nearly so -- information_spectrum(...).undetermined() names the variables the measurements do not determine")


def posterior_samples(data, results, n_samples: int = 64, seed: int = 0, first_sample: int = 0, variables=None,
                      range_weights=None, loop_closure_weights=None, rel_tol: float = 1e-10, max_iters: int = 4000,
                      block_width: int = MAX_BLOCK_WIDTH, engine: str = "device", lib_path: Optional[str] = None,
                      solver_settings: Optional[dict] = None):
    """``n_samples`` draws of N(x_hat, H^-1) at the estimate ``results`` -- normally what ``refine_estimate`` returned, with
    the same ``range_weights`` / ``loop_closure_weights``.  The draws are numbers ``first_sample`` .. of the stream of
    ``seed``: a draw does not depend on the call it is part of.  ``variables`` (pose or landmark names; None: every
    landmark and the last pose of every chain) are the ones whose steps come back; the covariance blocks cover every
    variable.  Returns ``(Samples, info)``; ``info``: ``order``, ``residuals`` (|b_s - H delta_s|_2), ``iterations``,
    ``pcg_iters``, ``batches``, ``setup_ms``, ``rhs_ms``, ``solve_ms``, ``engine`` and, from the python engine, ``noise``
    (z, S x rows in the library's (m, q) order) and ``rhs`` (J'z).  Draws that do not converge raise RuntimeError:
    usually a variable the measurements do not determine."""
    if engine not in ("device", "python"):
        raise ValueError("engine must be 'device' or 'python'")
    if int(n_samples) != n_samples or n_samples < 1:
        raise ValueError("n_samples must be an integer >= 1")
    if int(block_width) != block_width or not 1 <= int(block_width) <= MAX_BLOCK_WIDTH:
        raise ValueError(f"block_width must be an integer in 1..{MAX_BLOCK_WIDTH}")
    if int(first_sample) != first_sample or first_sample < 0 or first_sample + n_samples > 2 ** 32:
        raise ValueError("first_sample .. first_sample + n_samples must lie in 0 .. 2^32")
    if not rel_tol > 0 or max_iters < 1:
        raise ValueError("rel_tol must be positive and max_iters at least 1")
    prob, point = _problem_and_point(data, results, range_weights, loop_closure_weights)
    try:
        names, ids, size, cols = _select(prob, variables)
    except ValueError as e:
        raise ValueError(str(e).replace("marginal_covariances", "posterior_samples")) from None
    S = int(n_samples)
    if engine == "python":
        delta, b, z, res = _python_draws(prob, point, seed, int(first_sample), S)
        if delta is None:
            raise _singular(S, S, max_iters)
        moments, means = accumulate_moments(prob, delta)
        steps = np.ascontiguousarray(delta[:, cols])
        info = {"pcg_iters": 0, "batches": 0, "setup_ms": 0.0, "rhs_ms": 0.0, "solve_ms": 0.0, "iterations": np.zeros(S, dtype=np.int64),
                "noise": z, "rhs": b}
    else:
        with SamplesHandle(prob, lib_path, solver_settings) as h:
            out = h.draw(point, ids, S, seed, int(first_sample), rel_tol, max_iters, int(block_width))
        failed = int(np.count_nonzero(~out["converged"]))
        if failed:
            raise _singular(failed, S, max_iters)
        moments, means, steps, res = out["moments"], out["means"], out["steps"], out["residuals"]
        rec = out["info"]
        info = {"pcg_iters": int(rec["pcg_iters"]), "batches": int(rec["batches"]), "setup_ms": float(rec["setup_ms"]),
                "rhs_ms": float(rec["rhs_ms"]), "solve_ms": float(rec["solve_ms"]), "iterations": out["iterations"]}
    info.update({"order": names, "residuals": res, "engine": engine})
    return Samples(prob, results, moments, means, S, names, size, steps, first_sample), info


__all__ = ["posterior_samples", "Samples", "SamplesHandle", "ps_noise", "philox4x32_10", "measurement_rows", "ordered_jacobian",
           "noise_block", "accumulate_moments", "SAMPLES_SYMBOLS", "GEN_SAMPLE"]
