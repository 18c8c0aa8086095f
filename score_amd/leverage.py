"""Leverage of the range measurements and predicted range variances at a refined estimate (include/score_leverage.h).

Marginals, weakest modes and posterior samples speak about variables; this module speaks about measurements.  With J the
whitened Jacobian at the estimate and H = J'J, the hat matrix P = J H^-1 J' projects the measurement space onto the range of
J.  The leverage of measurement m is h_m = trace(J_m H^-1 J_m') over its rows and rows_m - h_m its redundancy (for a range,
one row: 1 - h_m, the redundancy number of network adjustment).  The residual of a measurement shows only the share 1 - h_m
of an error in it: a range with redundancy near 0 absorbs any outlier into the estimate and shows a residual of zero, so no
residual test -- GNC-TLS included -- can flag it.  The identities

    sum_m h_m = n (the unknowns),        sum_m (rows_m - h_m) = rows - n

hold exactly.  ``range_leverage`` estimates both from posterior draws on the device (``score_refine_leverage``): with
delta = H^-1 J'z, J delta = P z, so E|J_m delta|^2 = h_m and E|z_m - J_m delta|^2 = rows_m - h_m -- one small kernel per block
of 16 draws on top of ``posterior_samples``' own work.  The first sum has relative error sqrt(2 / S) on the leverage, the
second on the redundancy: a range nothing else controls gets a redundancy of rounding size from the second, while its
leverage estimate still wanders by sqrt(2 / S) around 1.  ``Leverage.studentized`` is residual / sqrt(redundancy), the
statistic a threshold such as ``inlier_threshold=3.0`` refers to.

``predicted_range_variances`` gives the exact variance g'H^-1 g of a hypothetical range between two named variables (g: the
gradient of |p_a - p_b|): one column per pair of the marginals' block PCG (``score_refine_range_variances``) where
``marginal_covariances(joint=True)`` needs 5-12 -- what active ranging, beacon placement and the gate of an incoming range
ask for.  ``engine="python"`` restates both in NumPy (the draws of ``samples.py``, a dense solve): small graphs, the tests.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import LEVERAGE, ScoreMarginalsInfo, ScoreSamplesInfo, bind, ptr, steps_and_converged
from .marginals import MAX_BLOCK_WIDTH, _problem_and_point, check_block_solve
from .refine import _point_arrays, _Problem3D, unknown_sizes
from .samples import SamplesHandle, _python_draws, measurement_rows, ordered_jacobian
from .solver import _i32p

# the symbols include/score_leverage.h declares
LEVERAGE_SYMBOLS = list(LEVERAGE)
KINDS = ("relative_pose", "range", "prior")


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, LEVERAGE)


def measurement_counts(prob):
    """(n_rel, n_rng, n_pri): the measurements in the library's numbering -- relative poses, then ranges, then priors."""
    return len(prob.bi), len(prob.ra), len(prob.pl)


def _row_groups(prob):
    """(first row, rows) of every measurement in the (m, q) order."""
    d, _ = unknown_sizes(prob)
    n_rel, n_rng, n_pri = measurement_counts(prob)
    rows = np.concatenate([np.full(n_rel, d + d * d), np.ones(n_rng), np.full(n_pri, d)]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int64), rows


class LeverageHandle(SamplesHandle):
    """A refinement handle kept for ``score_refine_leverage`` / ``score_refine_range_variances`` calls on one graph (and,
    being a ``SamplesHandle``, for ``score_refine_samples`` calls with the same draws)."""

    headers = SamplesHandle.headers + (LEVERAGE,)

    def leverage(self, point, pair_ids, n_samples, seed=0, first_sample=0, rel_tol=1e-10, max_iters=4000,
                 block_width=MAX_BLOCK_WIDTH) -> dict:
        """``score_refine_leverage`` as it is.  ``pair_ids``: (C, 2) variable ids or None.  Returns a dict: ``rc``, the six
        sums (``lev_sum``, ``lev_sq``, ``red_sum``, ``red_sq`` over all measurements, ``pair_sum``, ``pair_sq``),
        ``residuals``, ``iterations``, ``converged`` and ``info`` (the call's record)."""
        prob = self.prob
        poses, lms = _point_arrays(prob, point)
        pairs = np.zeros((0, 2), dtype=np.int32) if pair_ids is None else np.asarray(pair_ids, dtype=np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        M, S = sum(measurement_counts(prob)), max(int(n_samples), 0)
        sums = {k: np.zeros(M) for k in ("lev_sum", "lev_sq", "red_sum", "red_sq")}
        psum, psq = np.zeros(len(pa)), np.zeros(len(pa))
        res, its = np.zeros(S), np.zeros(S, dtype=np.int32)
        info = ScoreSamplesInfo()
        rc = self.lib.score_refine_leverage(self.h, ptr(poses), ptr(lms), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                            int(first_sample), int(n_samples), ptr(pa, _i32p), ptr(pb, _i32p), len(pa),
                                            float(rel_tol), int(max_iters), int(block_width), ptr(sums["lev_sum"]),
                                            ptr(sums["lev_sq"]), ptr(sums["red_sum"]), ptr(sums["red_sq"]), ptr(psum), ptr(psq),
                                            ptr(res), ptr(its, _i32p), C.byref(info))
        if rc < 0:
            raise RuntimeError(f"score_refine_leverage failed: {self.lib.score_last_error().decode()}")
        iterations, converged = steps_and_converged(its)
        out = {"rc": rc, "pair_sum": psum, "pair_sq": psq, "residuals": res, "iterations": iterations, "converged": converged,
               "info": info.as_dict()}
        out.update(sums)
        return out

    def range_variances(self, point, pair_ids, rel_tol=1e-10, max_iters=4000, block_width=MAX_BLOCK_WIDTH,
                        with_solutions=False) -> dict:
        """``score_refine_range_variances`` as it is: ``rc``, ``variances``, ``distances``, ``residuals``, ``iterations``,
        ``converged`` per pair, ``solutions`` (asked for: C x n, x_c as computed; else None) and ``info``."""
        poses, lms = _point_arrays(self.prob, point)
        pairs = np.asarray(pair_ids, dtype=np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        var, dist, res = np.zeros(len(pa)), np.zeros(len(pa)), np.zeros(len(pa))
        its = np.zeros(len(pa), dtype=np.int32)
        sol = np.zeros((len(pa), self.prob.n)) if with_solutions else None
        info = ScoreMarginalsInfo()
        rc = self.lib.score_refine_range_variances(self.h, ptr(poses), ptr(lms), ptr(pa, _i32p), ptr(pb, _i32p), len(pa),
                                                   float(rel_tol), int(max_iters), int(block_width), ptr(var), ptr(dist), ptr(res),
                                                   ptr(its, _i32p), ptr(sol), C.byref(info))
        if rc < 0:
            raise RuntimeError(f"score_refine_range_variances failed: {self.lib.score_last_error().decode()}")
        iterations, converged = steps_and_converged(its)
        return {"rc": rc, "variances": var, "distances": dist, "residuals": res, "iterations": iterations, "converged": converged,
                "solutions": sol, "info": info.as_dict()}


def pair_ids(prob, pairs, who: str) -> np.ndarray:
    """Pairs of names -> (C, 2) variable ids as in the graph's range endpoints (poses 0..Np-1, then the landmarks).  The fixed
    first pose is a legitimate end: it has a position and no unknowns."""
    ids = {str(nm): i for i, nm in enumerate(prob.a["pose_names"])}
    ids.update({str(nm): prob.Np + i for i, nm in enumerate(prob.a["landmark_names"])})
    out = np.zeros((len(pairs), 2), dtype=np.int32)
    for c, pair in enumerate(pairs):
        if len(pair) != 2:
            raise ValueError(f"{who}: a pair is two names, got {pair!r}")
        for k, nm in enumerate(pair):
            if str(nm) not in ids:
                raise ValueError(f"{who}: unknown variable {nm}")
            out[c, k] = ids[str(nm)]
        if out[c, 0] == out[c, 1]:
            raise ValueError(f"{who}: the pair ({pair[0]}, {pair[1]}) joins a variable to itself")
    return out


def _positions(prob, point):
    if isinstance(prob, _Problem3D):
        return point[1], point[2]
    _, t, lm = prob.split(point)
    return t, lm


def pair_gradients(prob, point, ids):
    """(G, distance): column c of G (n x C) is the gradient of |p_a - p_b| of pair c in the refinement's unknowns -- +u on the
    translation unknowns of a, -u on those of b, u the unit vector of p_a - p_b (zero where the distance is <= 1e-12, the
    rule of a range's Jacobian); the fixed first pose has no unknowns."""
    d, dp = unknown_sizes(prob)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1, 2)
    t, lm = _positions(prob, point)
    pa, pb = prob._point(ids[:, 0], t, lm), prob._point(ids[:, 1], t, lm)
    dv = pa - pb
    rho = np.sqrt(np.einsum("ij,ij->i", dv, dv))
    u = dv / np.where(rho > 1e-12, rho, 1.0)[:, None]
    u[rho <= 1e-12] = 0.0
    G = np.zeros((prob.n, len(ids)))
    for c, (a, b) in enumerate(ids):
        for v, sign in ((a, 1.0), (b, -1.0)):
            if v >= prob.Np:
                first = dp * (prob.Np - 1) + d * (v - prob.Np)
            elif v >= 1:
                first = dp * (v - 1) + (dp - d)
            else:
                continue
            G[first:first + d, c] = sign * u[c]
    return G, rho


def dense_leverage(prob, point) -> np.ndarray:
    """The exact leverage h_m = trace(J_m H^-1 J_m') of every measurement (M, in the library's numbering) from the dense H:
    small graphs and the tests."""
    import scipy.linalg as sla

    J = np.asarray(ordered_jacobian(prob, point).todense(), dtype=np.float64)
    X = sla.cho_solve(sla.cho_factor(J.T @ J, lower=True), J.T)
    per_row = np.einsum("ij,ji->i", J, X)
    return np.bincount(measurement_rows(prob)[1], weights=per_row, minlength=sum(measurement_counts(prob)))


def measurement_sums(prob, J, z, delta, G=None) -> dict:
    """The six sums of ``score_refine_leverage`` from full steps delta (S x n), the noise z (S x rows) and the dense J in the
    (m, q) order: per draw t = sum_q y_q^2 and v = sum_q (z_q - y_q)^2 with y = J_m delta, the rows added in ascending q and
    the draws in ascending s -- the library's order."""
    first, rows = _row_groups(prob)
    Y = delta @ J.T
    t, v = np.zeros((len(delta), len(rows))), np.zeros((len(delta), len(rows)))
    for q in range(int(rows.max()) if len(rows) else 0):
        has = rows > q
        y, o = Y[:, first[has] + q], z[:, first[has] + q] - Y[:, first[has] + q]
        t[:, has] += y * y
        v[:, has] += o * o
    p = (delta @ G) ** 2 if G is not None else np.zeros((len(delta), 0))
    out = {k: np.zeros(len(rows)) for k in ("lev_sum", "lev_sq", "red_sum", "red_sq")}
    out["pair_sum"], out["pair_sq"] = np.zeros(p.shape[1]), np.zeros(p.shape[1])
    for s in range(len(delta)):
        out["lev_sum"] += t[s]; out["lev_sq"] += t[s] * t[s]
        out["red_sum"] += v[s]; out["red_sq"] += v[s] * v[s]
        out["pair_sum"] += p[s]; out["pair_sq"] += p[s] * p[s]
    return out


def _mean_and_error(s1, s2, count):
    """The mean of `count` terms with sum s1 and sum of squares s2, and its standard error (infinite from one term)."""
    mean = s1 / count
    if count < 2:
        return mean, np.full_like(mean, np.inf)
    var = np.maximum(s2 / count - mean * mean, 0.0) * (count / (count - 1.0))
    return mean, np.sqrt(var / count)


class Leverage:
    """Leverage and redundancy of the measurements from ``count`` posterior draws.

    Over the graph's range list: ``leverage`` (the estimate of h_m, relative error sqrt(2 / count)), ``leverage_error`` (its
    standard error from the draws), ``redundancy`` (the estimate of 1 - h_m from the second sum, relative error sqrt(2 / count)
    on the REDUNDANCY: rounding size where nothing else controls the range), ``redundancy_error``, ``residuals`` (the
    whitened range residuals at the point) and ``studentized`` (residuals / sqrt(redundancy); inf where the redundancy is 0).
    ``by_kind``: "relative_pose" | "range" | "prior" -> (leverage, redundancy) per measurement, summed over its rows (6 | 12
    of a relative pose, d of a prior).  ``total_leverage`` and ``total_redundancy`` estimate the identities
    sum h = ``unknowns`` (n) and sum (rows_m - h_m) = ``rows`` - n.  ``pair_variance`` / ``pair_variance_error``: the
    estimate of g'H^-1 g for the pairs given (None without pairs)."""

    def __init__(self, prob, point, sums, count, pairs):
        n_rel, n_rng, n_pri = measurement_counts(prob)
        self.count = int(count)
        lev, lev_err = _mean_and_error(sums["lev_sum"], sums["lev_sq"], self.count)
        red, red_err = _mean_and_error(sums["red_sum"], sums["red_sq"], self.count)
        cut = {"relative_pose": slice(0, n_rel), "range": slice(n_rel, n_rel + n_rng), "prior": slice(n_rel + n_rng, n_rel + n_rng + n_pri)}
        self.by_kind = {k: (lev[s], red[s]) for k, s in cut.items()}
        rng = cut["range"]
        self.leverage, self.leverage_error = lev[rng], lev_err[rng]
        self.redundancy, self.redundancy_error = red[rng], red_err[rng]
        perm = measurement_rows(prob)[0]
        first, _ = _row_groups(prob)
        self.residuals = np.asarray(prob.residuals(point))[perm][first[rng]]
        with np.errstate(divide="ignore", invalid="ignore"):
            self.studentized = np.where(self.redundancy > 0, self.residuals / np.sqrt(self.redundancy), np.inf)
        self.total_leverage, self.total_redundancy = float(np.sum(lev)), float(np.sum(red))
        self.unknowns, self.rows = int(prob.n), int(np.sum(_row_groups(prob)[1]))
        self.pairs = list(pairs) if pairs is not None else None
        if pairs is not None:
            self.pair_variance, self.pair_variance_error = _mean_and_error(sums["pair_sum"], sums["pair_sq"], self.count)
        else:
            self.pair_variance = self.pair_variance_error = None

    def uncontrolled(self, min_redundancy: float = 0.1) -> np.ndarray:
        """Indices (into the range list) of the ranges whose redundancy estimate is at most ``min_redundancy``: an error in
        such a range goes into the estimate, not into its residual."""
        return np.flatnonzero(self.redundancy <= min_redundancy)


class PredictedRanges:
    """Hypothetical ranges between pairs of variables at the estimate: ``pairs``, ``distance`` (|p_a - p_b|) and ``variance``
    (g'H^-1 g, metres^2: the variance of the distance the estimate predicts)."""

    def __init__(self, pairs, distance, variance):
        self.pairs = list(pairs)
        self.distance, self.variance = np.asarray(distance, dtype=np.float64), np.asarray(variance, dtype=np.float64)

    def information_gain(self, precision):
        """1/2 log(1 + precision * variance): what a range of that precision would add, in nats."""
        return 0.5 * np.log1p(np.asarray(precision, dtype=np.float64) * self.variance)

    def gate(self, measured, precision):
        """(measured - distance)^2 / (1 / precision + variance): chi^2(1) for a range that fits the estimate."""
        measured, precision = np.asarray(measured, dtype=np.float64), np.asarray(precision, dtype=np.float64)
        return (measured - self.distance) ** 2 / (1.0 / precision + self.variance)


def _check_block(block_width, rel_tol, max_iters, engine):
    if engine not in ("device", "python"):
        raise ValueError("engine must be 'device' or 'python'")
    check_block_solve(block_width, rel_tol, max_iters)


def _singular(who, failed, total, what, max_iters):
    return RuntimeError(f"{who}: {failed} of {total} {what} did not converge (max_iters = {max_iters}): J'J is singular or nearly "
                        "so -- information_spectrum(...).undetermined() names the variables the measurements do not determine")


def range_leverage(data, results, n_samples: int = 256, seed: int = 0, first_sample: int = 0, pairs=None, range_weights=None,
                   loop_closure_weights=None, rel_tol: float = 1e-10, max_iters: int = 4000, block_width: int = MAX_BLOCK_WIDTH,
                   engine: str = "device", lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
    """Leverage and redundancy of every measurement at the estimate ``results`` -- normally what ``refine_estimate`` returned,
    with the same ``range_weights`` / ``loop_closure_weights`` -- from ``n_samples`` posterior draws (numbers ``first_sample``
    .. of the stream of ``seed``: the draws of ``posterior_samples``).  ``pairs``: hypothetical ranges as pairs of names, whose
    variance the same draws estimate (``predicted_range_variances`` gives it exactly).  Returns ``(Leverage, info)``;
    ``info``: ``residuals`` (|b_s - H delta_s|_2 per draw), ``iterations``, ``pcg_iters``, ``batches``, ``setup_ms``,
    ``rhs_ms``, ``solve_ms``, ``engine``.  Draws that do not converge raise RuntimeError: usually a variable the
    measurements do not determine."""
    _check_block(block_width, rel_tol, max_iters, engine)
    if int(n_samples) != n_samples or n_samples < 1:
        raise ValueError("n_samples must be an integer >= 1")
    if int(first_sample) != first_sample or first_sample < 0 or first_sample + n_samples > 2 ** 32:
        raise ValueError("first_sample .. first_sample + n_samples must lie in 0 .. 2^32")
    prob, point = _problem_and_point(data, results, range_weights, loop_closure_weights)
    ids = pair_ids(prob, pairs, "range_leverage") if pairs is not None else None
    S = int(n_samples)
    if engine == "python":
        delta, _, z, res = _python_draws(prob, point, seed, int(first_sample), S)
        if delta is None:
            raise _singular("range_leverage", S, S, "draws", max_iters)
        J = np.asarray(ordered_jacobian(prob, point).todense(), dtype=np.float64)
        sums = measurement_sums(prob, J, z, delta, pair_gradients(prob, point, ids)[0] if ids is not None else None)
        info = {"pcg_iters": 0, "batches": 0, "setup_ms": 0.0, "rhs_ms": 0.0, "solve_ms": 0.0, "iterations": np.zeros(S, dtype=np.int64)}
    else:
        with LeverageHandle(prob, lib_path, solver_settings) as h:
            sums = h.leverage(point, ids, S, seed, int(first_sample), rel_tol, max_iters, int(block_width))
        failed = int(np.count_nonzero(~sums["converged"]))
        if failed:
            raise _singular("range_leverage", failed, S, "draws", max_iters)
        rec, res = sums["info"], sums["residuals"]
        info = {"pcg_iters": int(rec["pcg_iters"]), "batches": int(rec["batches"]), "setup_ms": float(rec["setup_ms"]),
                "rhs_ms": float(rec["rhs_ms"]), "solve_ms": float(rec["solve_ms"]), "iterations": sums["iterations"]}
    info.update({"residuals": res, "engine": engine})
    return Leverage(prob, point, sums, S, pairs), info


def predicted_range_variances(data, results, pairs, range_weights=None, loop_closure_weights=None, rel_tol: float = 1e-10,
                              max_iters: int = 4000, block_width: int = MAX_BLOCK_WIDTH, engine: str = "device",
                              lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
    """The distance and its variance g'H^-1 g for hypothetical ranges between ``pairs`` of names, e.g.
    ``[("A10", "L1"), ("A10", "B10")]``, at the estimate ``results``: one column H x = g per pair, up to ``block_width``
    pairs per block of the marginals' PCG.  Returns ``(PredictedRanges, info)``; ``info``: ``residuals`` (|g_c - H x_c|_2),
    ``iterations``, ``pcg_iters``, ``batches``, ``setup_ms``, ``solve_ms``, ``engine``.  A column that does not converge raises
    RuntimeError."""
    _check_block(block_width, rel_tol, max_iters, engine)
    prob, point = _problem_and_point(data, results, range_weights, loop_closure_weights)
    pairs = [tuple(p) for p in pairs]
    if not pairs:
        raise ValueError("predicted_range_variances: no pairs")
    ids = pair_ids(prob, pairs, "predicted_range_variances")
    if engine == "python":
        from .marginals import dense_information

        G, dist = pair_gradients(prob, point, ids)
        H = dense_information(prob, point)
        try:
            X = np.linalg.solve(H, G)
        except np.linalg.LinAlgError:
            raise _singular("predicted_range_variances", len(pairs), len(pairs), "columns", max_iters) from None
        var, res = np.einsum("ic,ic->c", G, X), np.linalg.norm(G - H @ X, axis=0)
        info = {"pcg_iters": 0, "batches": 0, "setup_ms": 0.0, "solve_ms": 0.0, "iterations": np.zeros(len(pairs), dtype=np.int64)}
    else:
        with LeverageHandle(prob, lib_path, solver_settings) as h:
            out = h.range_variances(point, ids, rel_tol, max_iters, int(block_width))
        failed = int(np.count_nonzero(~out["converged"]))
        if failed:
            raise _singular("predicted_range_variances", failed, len(pairs), "columns", max_iters)
        var, dist, res, rec = out["variances"], out["distances"], out["residuals"], out["info"]
        info = {"pcg_iters": int(rec["pcg_iters"]), "batches": int(rec["batches"]), "setup_ms": float(rec["setup_ms"]),
                "solve_ms": float(rec["solve_ms"]), "iterations": out["iterations"]}
    info.update({"residuals": res, "engine": engine})
    return PredictedRanges(pairs, dist, var), info


__all__ = ["range_leverage", "predicted_range_variances", "Leverage", "PredictedRanges", "LeverageHandle", "dense_leverage",
           "measurement_sums", "pair_gradients", "pair_ids", "measurement_counts", "LEVERAGE_SYMBOLS"]
