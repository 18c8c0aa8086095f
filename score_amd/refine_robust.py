"""Outlier-robust local refinement: GNC-TLS re-weighting of the ranges and / or the loop closures on the residuals of the
maximum-likelihood cost (include/score_refine_robust.h states the loop in full).

``solve_score_robust`` weighs a range by its term in the RELAXED objective, ``sqrt(prec) max(0, |t_a - t_b| - dist)``: a range
measured too long costs nothing there and keeps weight 1.  The refinement's range term ``w (|p_a - p_b| - dist)^2`` is
two-sided, so a long outlier drags the refined estimate; so does a false loop closure that lands where the relaxation is
free.  ``refine_estimate_robust`` runs the GNC-TLS loop around the Levenberg-Marquardt step of ``refine_estimate``:

    solve 1 as refine_estimate;  r = sqrt(prec) | |p_a - p_b| - dist |,  r = sqrt(kappa |t_j - t_i - R_i t~|^2 + tau |R_j - R_i R~|_F^2)
    with the MEASURED precisions;  stop (first solve, no 2 max r_f^2 > c_f^2 | a later solve on binary weights | max_outer |
    non-finite);  mu0 = min_f c_f^2 / (2 max r_f^2 - c_f^2), then mu <- mu_step mu;  w = gnc_tls_weight(r, mu, c_f);  next
    precisions prec max(w, min_weight);  solves 2.. are at most inner_iters LM iterations from the current point;  one last run
    with the final weights to max_iters / tol.

``engine="native"`` runs the whole loop behind the C ABI on one refinement handle (``score_refine_robust_run``: two streaming
kernels per outer iteration at the point on the device, csrc/score_gn_robust.hpp); ``engine="python"`` is the readable twin --
the same schedule (``_Stage``; the library's is ``GncState`` and ``gnc_*`` of csrc/score_refine_rule.hpp) around
``refine._lm_loop`` with NumPy residuals in the device's operation order -- which the tests compare with.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import REFINE_ROBUST, ScoreRefineRobustInfo, ScoreRefineRobustSettings, bind, ptr
from .refine import (RefineHandle, _as_results, _DeviceNormalEquations, _lm_loop, _Member, _native_info, _point_arrays, _point_from,
                     _point_outputs, _problem_and_point, _Problem3D)
from .robust import BINARY_TOL, _robust_info, gnc_tls_weight, initial_mu, n_loop_closures_of

# the symbols include/score_refine_robust.h declares
REFINE_ROBUST_SYMBOLS = list(REFINE_ROBUST)

FAMILY_RANGES, FAMILY_LOOP_CLOSURES = 1, 2


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, REFINE_ROBUST)


# ---------------------------------------------------------------------------------------------------------------------
# the residuals (the device's are csrc/score_gn.hpp: gn_robust_residual<DIM> -- same operations, same order)
# ---------------------------------------------------------------------------------------------------------------------
def _translations(prob, point):
    if isinstance(prob, _Problem3D):
        _, t, lm = point
    else:
        _, t, lm = prob.split(point)
    return t, lm


def range_residuals(prob, point, prec) -> np.ndarray:
    """r = sqrt(prec) | |p_a - p_b| - dist | of every range at ``point`` (the packed unknowns in 2-D, (R, t, lm) in 3-D) -- the
    square root of the range's own term in the refinement's cost, two-sided."""
    t, lm = _translations(prob, point)
    pa, pb = prob._point(prob.ra, t, lm), prob._point(prob.rb, t, lm)
    nn = np.zeros(len(prob.ra))
    for k in range(pa.shape[1]):
        dl = pa[:, k] - pb[:, k]
        nn = nn + dl * dl
    r = np.sqrt(np.asarray(prec, dtype=np.float64)) * (np.sqrt(nn) - prob.dist)
    return np.sqrt(r * r)


def loop_closure_residuals(prob, point, kappa, tau) -> np.ndarray:
    """r = sqrt(kappa |t_j - t_i - R_i t~|^2 + tau |R_j - R_i R~|_F^2) of every loop closure (the trailing relative-pose
    entries; ``kappa``, ``tau``: one per loop closure) at ``point`` -- the square root of its term in the refinement's cost."""
    n_lc = len(kappa)
    sl = slice(len(prob.bi) - n_lc, len(prob.bi))
    bi, tj = prob.bi[sl], prob.tj[sl]
    sk, st = np.sqrt(np.asarray(kappa, dtype=np.float64)), np.sqrt(np.asarray(tau, dtype=np.float64))
    rows = []
    if isinstance(prob, _Problem3D):
        R, t, _ = point
        tm, Rm = np.asarray(prob.tm).reshape(-1, 3)[sl], np.asarray(prob.Rm).reshape(-1, 3, 3)[sl]
        Ri, Rj, ti, tjv = R[bi], R[tj], t[bi], t[tj]
        for a in range(3):
            rt = np.zeros(n_lc)
            for k in range(3):
                rt = rt + Ri[:, a, k] * tm[:, k]
            rows.append(sk * (tjv[:, a] - ti[:, a] - rt))
        for a in range(3):
            for b in range(3):
                rr = np.zeros(n_lc)
                for k in range(3):
                    rr = rr + Ri[:, a, k] * Rm[:, k, b]
                rows.append(st * (Rj[:, a, b] - rr))
    else:
        th, t, _ = prob.split(point)
        tm, Rm = np.asarray(prob.tm).reshape(-1, 2)[sl], np.asarray(prob.Rm).reshape(-1, 4)[sl]
        ci, si, cj, sj = np.cos(th[bi]), np.sin(th[bi]), np.cos(th[tj]), np.sin(th[tj])
        rows.append(sk * (t[tj, 0] - t[bi, 0] - (ci * tm[:, 0] - si * tm[:, 1])))
        rows.append(sk * (t[tj, 1] - t[bi, 1] - (si * tm[:, 0] + ci * tm[:, 1])))
        rows.append(st * (cj - (ci * Rm[:, 0] - si * Rm[:, 2])))
        rows.append(st * (-sj - (ci * Rm[:, 1] - si * Rm[:, 3])))
        rows.append(st * (sj - (si * Rm[:, 0] + ci * Rm[:, 2])))
        rows.append(st * (cj - (si * Rm[:, 1] + ci * Rm[:, 3])))
    cost = np.zeros(n_lc)
    for r in rows:
        cost = cost + r * r
    return np.sqrt(cost)


# ---------------------------------------------------------------------------------------------------------------------
# the stop rule (the library's is csrc/score_refine_rule.hpp: robust_decide)
# ---------------------------------------------------------------------------------------------------------------------
def _nonbinary(w) -> int:
    w = np.asarray(w, dtype=np.float64)
    return int(np.count_nonzero(~((np.abs(w) <= BINARY_TOL) | (np.abs(1.0 - w) <= BINARY_TOL))))


def decide(k: int, max_outer: int, seen) -> str:
    """What follows outer solve ``k``: "go", "converged", "max_outer" or "non_finite".  ``seen``: one
    ``(items, max r^2, c, non-binary weights of this solve)`` per enabled family."""
    if not all(np.isfinite(r2) for _, r2, _, _ in seen):
        return "non_finite"
    outliers = any(n > 0 and 2.0 * r2 > c * c for n, r2, c, _ in seen)
    nonbinary = sum(nb for _, _, _, nb in seen)
    if (not outliers) if k == 1 else (nonbinary == 0):
        return "converged"
    return "max_outer" if k >= max_outer else "go"


def first_mu(seen) -> float:
    """mu after the first solve: the smallest c_f^2 / (2 max r_f^2 - c_f^2) of the families with outliers."""
    return min(initial_mu(r2, c) for n, r2, c, _ in seen if n > 0 and 2.0 * r2 > c * c)


class RobustRefineHandle(RefineHandle):
    """A refinement handle (``score_refine_create``) with the calls of include/score_refine_robust.h (and ``score_refine_run``)
    as they are: points go in and come out in the problem's own form (``_Problem``: packed unknowns; ``_Problem3D``: (R, t, lm))."""

    headers = RefineHandle.headers + (REFINE_ROBUST,)

    def __init__(self, prob, lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
        super().__init__(prob, lib_path, solver_settings)
        self.n_rng, self.n_lc = len(prob.ra), n_loop_closures_of(prob.a)

    def default_settings(self) -> ScoreRefineRobustSettings:
        rs = ScoreRefineRobustSettings()
        self.lib.score_refine_robust_default_settings(C.byref(rs))
        return rs

    def _outputs(self):
        return [np.ones(max(1, n)) for n in (self.n_rng, self.n_rng, self.n_lc, self.n_lc)]

    def robust_run(self, point, rs: ScoreRefineRobustSettings):
        """``score_refine_robust_run``: returns (point, weights, residuals, loop-closure weights, residuals, info dict)."""
        poses_in, lms_in = _point_arrays(self.prob, point)
        poses_out, lms_out = _point_outputs(poses_in, lms_in)
        w, r, wl, rl = self._outputs()
        info = ScoreRefineRobustInfo()
        rc = self.lib.score_refine_robust_run(self.h, C.byref(rs), ptr(poses_in), ptr(lms_in), ptr(poses_out), ptr(lms_out), ptr(w),
                                              ptr(r), ptr(wl), ptr(rl), C.byref(info))
        if rc != 0:
            raise RuntimeError(f"score_refine_robust_run failed: {self.lib.score_last_error().decode()}")
        return (_point_from(self.prob, poses_out, lms_out), w[: self.n_rng], r[: self.n_rng], wl[: self.n_lc], rl[: self.n_lc],
                info.as_dict())

    def residuals(self, point, mu: float = 0.0, c: float = 3.0, c_rel: float = 3.0):
        """``score_refine_residuals``: (residuals, loop-closure residuals, weights, loop-closure weights) at ``point``."""
        poses_in, lms_in = _point_arrays(self.prob, point)
        w, r, wl, rl = self._outputs()
        rc = self.lib.score_refine_residuals(self.h, ptr(poses_in), ptr(lms_in), float(mu), float(c), float(c_rel), ptr(r), ptr(rl),
                                             ptr(w), ptr(wl))
        if rc != 0:
            raise RuntimeError(f"score_refine_residuals failed: {self.lib.score_last_error().decode()}")
        return r[: self.n_rng], rl[: self.n_lc], w[: self.n_rng], wl[: self.n_lc]


# ---------------------------------------------------------------------------------------------------------------------
# engine="python": the readable twin
# ---------------------------------------------------------------------------------------------------------------------
FIRST, INNER, LAST, DONE = "first", "inner", "last", "done"


class _Stage:
    """One graph's place in the schedule (first run, inner runs, last run), and what it does when one of its runs stops.
    ``s``: families, c, c_rel, max_outer, inner_iters, min_weight, mu_step, max_iters, tol."""

    def __init__(self, prob, s: dict):
        self.prob, self.s = prob, s
        self.f_rng, self.f_rel = bool(s["families"] & FAMILY_RANGES), bool(s["families"] & FAMILY_LOOP_CLOSURES)
        self.n_lc = n_loop_closures_of(prob.a)
        self.first = len(prob.bi) - self.n_lc
        self.prec0 = np.array(prob.a["rng_prec"], dtype=np.float64)
        self.kappa0 = np.array(prob.a["rel_kappa"], dtype=np.float64)[self.first:]
        self.tau0 = np.array(prob.a["rel_tau"], dtype=np.float64)[self.first:]
        self.w, self.wl = np.ones(len(self.prec0)), np.ones(self.n_lc)
        self.sk_all, self.st_all = prob.sk.copy(), prob.st.copy()
        self.stage, self.k, self.mu, self.what = FIRST, 1, 0.0, "go"
        self.lm = self.linear_solves = 0
        self.cost_initial = 0.0

    def cap(self) -> int:
        """The iteration cap of the run the graph stands in."""
        return self.s["inner_iters"] if self.stage == INNER else self.s["max_iters"]

    def weigh(self, floor: Optional[float]) -> None:
        """The precisions the cost reads: prec max(w, floor) in the enabled families (floor None: prec w)."""
        prob = self.prob
        fl = (lambda w: np.maximum(w, floor)) if floor is not None else (lambda w: w)
        if self.f_rng:
            prob.sw = np.sqrt(self.prec0 * fl(self.w))
        if self.f_rel and self.n_lc:
            f = fl(self.wl)
            self.sk_all[self.first:], self.st_all[self.first:] = np.sqrt(self.kappa0 * f), np.sqrt(self.tau0 * f)
            prob.sk, prob.st = self.sk_all, self.st_all

    def run_stopped(self, u, member: _Member) -> bool:
        """A run has stopped at ``u``: True when another run follows."""
        s = self.s
        if self.stage == FIRST:
            self.cost_initial = member.cost_initial
        self.lm += member.iterations
        self.linear_solves += member.linear_solves
        if self.stage == LAST:
            self.stage = DONE
            return False
        seen = []
        if self.f_rng:
            r = range_residuals(self.prob, u, self.prec0)
            seen.append((len(r), float(np.max(r * r)) if len(r) else 0.0, s["c"], _nonbinary(self.w)))
        if self.f_rel:
            rl = loop_closure_residuals(self.prob, u, self.kappa0, self.tau0)
            seen.append((len(rl), float(np.max(rl * rl)) if len(rl) else 0.0, s["c_rel"], _nonbinary(self.wl)))
        self.what = decide(self.k, s["max_outer"], seen)
        if self.what == "go":
            self.mu = first_mu(seen) if self.k == 1 else self.mu * s["mu_step"]
            if self.f_rng:
                self.w = gnc_tls_weight(r, self.mu, s["c"])
            if self.f_rel:
                self.wl = gnc_tls_weight(rl, self.mu, s["c_rel"])
            self.weigh(s["min_weight"])
            self.k += 1
            self.stage = INNER
            return True
        if self.k > 1 and self.what != "non_finite":  # the final weights, to max_iters / tol
            self.stage = LAST
            return True
        self.stage = DONE
        return False


def _python_loop(prob, u, s: dict, linear_solver, lib_path, solver_settings, pcg_rel_tol=1e-9):
    """The runs of one ``_Stage`` (settings ``s``) from ``u``, one after the other."""
    stage, dev = _Stage(prob, s), None
    try:
        while True:
            res, J = prob.residuals(u, jac=True)
            if dev is None and linear_solver == "device" and prob.n > 0:
                dev = _DeviceNormalEquations(prob, J, lib_path, solver_settings)
            u, m = _lm_loop(prob, u, res, J, float(res @ res), stage.cap(), s["tol"], False, dev, pcg_rel_tol)
            if not stage.run_stopped(u, m):
                break
        pcg = (dev.pcg_iters, dev.solves) if dev else (0, 0)
    finally:
        if dev:
            dev.close()
    r = range_residuals(prob, u, stage.prec0)
    rl = loop_closure_residuals(prob, u, stage.kappa0, stage.tau0)
    info = {"cost_initial": stage.cost_initial, "cost_final": m.f, "iterations": stage.lm, "grad_inf": m.gnorm,
            "linear_solver": linear_solver, "engine": "python", "pcg_iters": pcg[0], "linear_solves": pcg[1]}
    return u, info, (stage.w, r, stage.wl, rl, stage.k, stage.mu, stage.what == "converged")


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
def _check(inlier_threshold, c_rel, max_outer, inner_iters, min_weight, mu_step, engine, linear_solver, f_rng, f_rel) -> None:
    if not f_rng and not f_rel:
        raise ValueError("refine_estimate_robust: robust_ranges and robust_loop_closures are both off: nothing to re-weight")
    if not (np.isfinite(inlier_threshold) and inlier_threshold > 0):
        raise ValueError(f"inlier_threshold must be positive and finite, not {inlier_threshold}")
    if not (np.isfinite(c_rel) and c_rel > 0):
        raise ValueError(f"loop_closure_threshold must be positive and finite, not {c_rel}")
    if int(max_outer) < 1:
        raise ValueError(f"max_outer must be >= 1, not {max_outer}")
    if int(inner_iters) < 1:
        raise ValueError(f"inner_iters must be >= 1, not {inner_iters}")
    if not (0.0 < min_weight <= 1.0):
        raise ValueError(f"min_weight must lie in (0, 1], not {min_weight}")
    if not (np.isfinite(mu_step) and mu_step > 1.0):
        raise ValueError(f"mu_step must be finite and > 1, not {mu_step}")
    if engine not in ("native", "python"):
        raise ValueError("engine must be 'native' or 'python'")
    if linear_solver not in ("device", "scipy"):
        raise ValueError("linear_solver must be 'device' or 'scipy'")
    if engine == "native" and linear_solver != "device":
        raise ValueError("engine='native' solves on the device: linear_solver='scipy' goes with engine='python'")


def _check_precisions(prob, f_rng: bool, f_rel: bool, who: str) -> None:
    """The measured precisions of the enabled families; ``who``: the prefix of the message."""
    n_lc = n_loop_closures_of(prob.a)
    if f_rng and len(prob.ra) and not (np.all(np.isfinite(prob.a["rng_prec"])) and np.all(np.asarray(prob.a["rng_prec"]) > 0)):
        raise ValueError(f"{who}every range precision must be positive and finite")
    if f_rel:
        if n_lc < 0:
            raise ValueError(f"{who}fewer relative-pose entries than odometry steps")
        for key in ("rel_kappa", "rel_tau"):
            v = np.asarray(prob.a[key], dtype=np.float64)[len(prob.bi) - n_lc:]
            if v.size and not (np.all(np.isfinite(v)) and np.all(v > 0)):
                raise ValueError(f"{who}every loop closure's precision ({key}) must be positive and finite")


def _prior(weights, floor: float, enabled: bool):
    """Prior weights as the precisions take them: those of a re-weighted family are floored like the loop's own weights (a
    measurement the relaxation took out, weight 0, stays a term of precision prec * min_weight)."""
    if weights is None or not enabled:
        return weights
    w = np.asarray(weights, dtype=np.float64)
    return np.where(w < floor, floor, w) if np.all(np.isfinite(w)) and np.all(w >= 0) else w


def refine_estimate_robust(data, results, inlier_threshold: float = 3.0, robust_ranges: bool = True, robust_loop_closures: bool = False,
                           loop_closure_threshold: Optional[float] = None, max_outer: int = 50, inner_iters: int = 5,
                           min_weight: float = 1e-6, mu_step: float = 1.4, max_iters: int = 50, tol: float = 1e-10,
                           engine: str = "native", linear_solver: str = "device", range_weights=None, loop_closure_weights=None,
                           lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
    """``refine_estimate`` with GNC-TLS re-weighting of the ranges (``robust_ranges``) and / or the loop closures
    (``robust_loop_closures``; threshold ``loop_closure_threshold``, None: ``inlier_threshold``) on the residuals of the
    maximum-likelihood cost.  Returns ``(refined SolverResults, info)``: the keys of ``refine_estimate``'s info (``iterations``:
    the Levenberg-Marquardt iterations of all solves) and ``info["robust"]`` with the keys of ``solve_score_robust``'s --
    ``weights``, ``residuals`` (at the final estimate), ``outliers``, ``outer_iterations``, ``mu``, ``converged`` and, with the
    loop closures on, ``loop_closure_weights`` / ``_residuals`` / ``_outliers``.  A graph without outliers takes one solve, and
    its result is ``refine_estimate``'s.

    ``range_weights`` / ``loop_closure_weights`` are prior weights (the relaxation's, say): they scale the measured precisions
    before the loop as in ``refine_estimate`` -- a prior weight below ``min_weight`` in a re-weighted family counts as
    ``min_weight`` there, so every precision stays positive -- and the returned weights are prior x GNC: they go straight into
    ``marginal_covariances(..., range_weights=...)``.  ``engine="python"`` takes ``linear_solver="scipy"`` or ``"device"``;
    ``engine="native"`` raises without the HIP library."""
    f_rng, f_rel = bool(robust_ranges), bool(robust_loop_closures)
    c = float(inlier_threshold)
    c_rel = c if loop_closure_threshold is None else float(loop_closure_threshold)
    _check(c, c_rel, max_outer, inner_iters, min_weight, mu_step, engine, linear_solver, f_rng, f_rel)
    families = (FAMILY_RANGES if f_rng else 0) | (FAMILY_LOOP_CLOSURES if f_rel else 0)
    pw, pwl = _prior(range_weights, float(min_weight), f_rng), _prior(loop_closure_weights, float(min_weight), f_rel)
    prob, u = _problem_and_point(data, results, pw, pwl)
    _check_precisions(prob, f_rng, f_rel, "refine_estimate_robust: ")
    if engine == "native":
        with RobustRefineHandle(prob, lib_path, solver_settings) as h:
            rs = h.default_settings()
            rs.inlier_threshold, rs.rel_threshold, rs.mu_step, rs.min_weight = c, c_rel, float(mu_step), float(min_weight)
            rs.families, rs.max_outer, rs.inner_iters = families, int(max_outer), int(inner_iters)
            rs.max_iters, rs.tol = int(max_iters), float(tol)
            u, w, r, wl, rl, ni = h.robust_run(u, rs)
        info = _native_info(ni, "lm_iterations")
        k, mu, conv = ni["outer_iterations"], ni["mu"], bool(ni["converged"])
    else:
        s = dict(families=families, c=c, c_rel=c_rel, max_outer=int(max_outer), inner_iters=int(inner_iters), min_weight=float(min_weight),
                 mu_step=float(mu_step), max_iters=int(max_iters), tol=float(tol))
        u, info, (w, r, wl, rl, k, mu, conv) = _python_loop(prob, u, s, linear_solver, lib_path, solver_settings)
    if range_weights is not None:  # prior x GNC
        w = w * np.asarray(range_weights, dtype=np.float64)
    if loop_closure_weights is not None:
        wl = wl * np.asarray(loop_closure_weights, dtype=np.float64)
    info["robust"] = _robust_info(w, r, k, mu, conv, wl if f_rel else None, rl if f_rel else None)
    return _as_results(prob, u, results, info["cost_final"]), info


__all__ = ["refine_estimate_robust", "RobustRefineHandle", "range_residuals", "loop_closure_residuals", "decide", "first_mu",
           "REFINE_ROBUST_SYMBOLS"]
