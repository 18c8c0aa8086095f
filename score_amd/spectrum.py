"""The weakest modes of a refined estimate (include/score_spectrum.h).

The lowest eigenpairs (lambda_j, v_j) of the information matrix H = J'J at the estimate -- in the unknowns of
``marginal_covariances``: (theta, x, y) per 2-D pose, (omega, v) per 3-D pose, the coordinates of a landmark, the first
pose fixed -- answer two questions the marginals cannot.  Which variable do the measurements not determine: a mode with
lambda_j at zero, and the variables that carry it (``Modes.undetermined``).  How uncertain is everything at once: with the
lowest k pairs, for every variable v,

    lower_v = sum_{j < k-1} v_j[v] v_j[v]' / lambda_j,      lower_v <= Sigma_vv <= lower_v + I / lambda_{k-1}

(``covariance_bracket``), at the cost of about one block of marginal columns instead of one column per unknown.
``information_spectrum`` runs LOBPCG with a block of 16 vectors on the device (``score_refine_spectrum``);
``engine="python"`` is the dense ``eigh`` of J'J from the host Jacobian: for small graphs, the tests, and libraries without
the symbol (the CPU twin).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import SPECTRUM, ScoreSpectrumInfo, bind, ptr
from .marginals import MarginalsHandle, _problem_and_point, _select, dense_information
from .refine import _point_arrays, unknown_sizes

# the symbols include/score_spectrum.h declares
SPECTRUM_SYMBOLS = list(SPECTRUM)
MAX_MODES = 16
MIN_DEVICE_UNKNOWNS = 48


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, SPECTRUM)


def _layout(prob):
    """Every variable with unknowns, in the order of the unknowns: (names, first unknown of each, size of each)."""
    poses, lms = list(prob.a["pose_names"]), list(prob.a["landmark_names"])
    d, dp = unknown_sizes(prob)
    names = [str(nm) for nm in poses[1:]] + [str(nm) for nm in lms]
    first = [dp * p for p in range(prob.Np - 1)] + [dp * (prob.Np - 1) + d * l for l in range(len(lms))]
    size = [dp] * (prob.Np - 1) + [d] * len(lms)
    return names, first, size


class Modes:
    """The k lowest eigenpairs of H.  ``values`` (k, ascending), ``vectors`` (n x k, unit columns), ``residuals``
    (|H v_j - lambda_j v_j|_2), ``names`` (every variable with unknowns, in the order of the rows), ``participation``
    (name -> (k,): the share of |v_j|^2 on that variable's rows; over all names it sums to 1 per mode)."""

    def __init__(self, values, vectors, residuals, names, first, size, h_max, rel_tol, default_variables):
        self.values = np.asarray(values, dtype=np.float64)
        self.vectors = np.asarray(vectors, dtype=np.float64)
        self.residuals = np.asarray(residuals, dtype=np.float64)
        self.names = list(names)
        self.h_max = float(h_max)
        self.rel_tol = float(rel_tol)
        self._rows = {nm: (f, s) for nm, f, s in zip(names, first, size)}
        self._default_variables = list(default_variables)
        sq = self.vectors ** 2
        total = sq.sum(axis=0)
        self.participation = {nm: sq[f:f + s].sum(axis=0) / total for nm, (f, s) in self._rows.items()}

    def block(self, name) -> np.ndarray:
        """The rows of ``vectors`` that belong to the variable: (3 | 6 | 2 | 3) x k."""
        if str(name) not in self._rows:
            raise ValueError(f"information_spectrum: unknown variable {name} (the fixed first pose has no rows)")
        f, s = self._rows[str(name)]
        return self.vectors[f:f + s]

    def undetermined(self):
        """[(j, [(name, share), ...] by descending share)] for every mode with lambda_j <= rel_tol * h_max: not
        distinguishable from zero at the accuracy asked for."""
        out = []
        for j in np.nonzero(self.values <= self.rel_tol * self.h_max)[0]:
            shares = sorted(((nm, float(p[j])) for nm, p in self.participation.items()), key=lambda e: -e[1])
            out.append((int(j), shares))
        return out


class SpectrumHandle(MarginalsHandle):
    """A refinement handle kept for several ``score_refine_spectrum`` calls on one graph."""

    headers = MarginalsHandle.headers + (SPECTRUM,)

    def spectrum(self, point, k, rel_tol=1e-9, max_iters=200, shift=1e-8):
        """``score_refine_spectrum`` as it is: (return code, values (k), vectors (k x n), residuals (k), info record)."""
        prob = self.prob
        poses, lms = _point_arrays(prob, point)
        kk = max(0, min(int(k), MAX_MODES))
        values = np.full(kk, np.nan)
        vectors = np.full((kk, prob.n), np.nan)
        res = np.full(kk, np.nan)
        info = ScoreSpectrumInfo()
        rc = self.lib.score_refine_spectrum(self.h, ptr(poses), ptr(lms), int(k), float(rel_tol), int(max_iters), float(shift),
                                            ptr(values), ptr(vectors), ptr(res), C.byref(info))
        if rc < 0:
            raise RuntimeError(f"score_refine_spectrum failed: {self.lib.score_last_error().decode()}")
        return rc, values, vectors, res, info.as_dict()


def device_spectrum(prob, point, k, rel_tol=1e-9, max_iters=200, shift=1e-8, lib_path=None, solver_settings=None):
    """One ``SpectrumHandle.spectrum`` call on a handle of its own."""
    with SpectrumHandle(prob, lib_path, solver_settings) as h:
        return h.spectrum(point, k, rel_tol, max_iters, shift)


def _python_spectrum(prob, point, k):
    H = dense_information(prob, point)
    w, V = np.linalg.eigh(H)
    w, V = w[:k], V[:, :k]
    res = np.linalg.norm(H @ V - V * w, axis=0)
    return w, V, res, float(np.max(np.diag(H)))


def information_spectrum(data, results, k: int = 8, range_weights=None, loop_closure_weights=None, rel_tol: float = 1e-9,
                         max_iters: int = 200, shift: float = 1e-8, engine: str = "device", lib_path: Optional[str] = None,
                         solver_settings: Optional[dict] = None):
    """The ``k`` (1..16) lowest eigenpairs of the information matrix at the estimate ``results`` -- normally what
    ``refine_estimate`` returned, with the same weights.  Returns ``(Modes, info)``; ``info``: ``h_max`` (max diag H),
    ``shift`` (sigma = shift * h_max: the iteration runs on H + sigma I, which exists for a singular H), ``iterations``,
    ``unconverged``, ``setup_ms``, ``solve_ms``, ``engine``.  A pair counts as converged at
    |H v - lambda v|_2 <= rel_tol * h_max; one that is not raises RuntimeError naming the mode and its residual."""
    if engine not in ("device", "python"):
        raise ValueError("engine must be 'device' or 'python'")
    if int(k) != k or not 1 <= int(k) <= MAX_MODES:
        raise ValueError(f"k must be an integer in 1..{MAX_MODES}")
    if not rel_tol > 0 or not np.isfinite(rel_tol):
        raise ValueError("rel_tol must be positive")
    if int(max_iters) != max_iters or max_iters < 1:
        raise ValueError("max_iters must be at least 1")
    if not shift > 0 or not np.isfinite(shift):
        raise ValueError("shift must be positive")
    k = int(k)
    prob, point = _problem_and_point(data, results, range_weights, loop_closure_weights)
    if k > prob.n:
        raise ValueError(f"k = {k} modes of a graph with {prob.n} unknowns")
    names, first, size = _layout(prob)
    if engine == "python":
        values, V, res, h_max = _python_spectrum(prob, point, k)
        rec = {"h_max": h_max, "shift": shift * h_max, "iterations": 0, "unconverged": 0, "setup_ms": 0.0, "solve_ms": 0.0}
    else:
        if prob.n < MIN_DEVICE_UNKNOWNS:
            raise ValueError(f"information_spectrum: {prob.n} unknowns are fewer than the {MIN_DEVICE_UNKNOWNS} the device solver's "
                             "basis holds: use engine=\"python\"")
        rc, values, Vt, res, rec = device_spectrum(prob, point, k, rel_tol, int(max_iters), shift, lib_path, solver_settings)
        V = np.ascontiguousarray(Vt.T)
        if rc != 0:
            bad = [j for j in range(k) if not res[j] <= rel_tol * rec["h_max"]]
            raise RuntimeError("information_spectrum: " + ", ".join(f"mode {j} (residual {res[j]:.3e})" for j in bad)
                               + f" did not reach {rel_tol:g} * h_max = {rel_tol * rec['h_max']:.3e} in {max_iters} iterations")
    try:
        default_variables = _select(prob, None)[0]
    except ValueError:  # (a graph without landmarks whose only chain is the fixed pose)
        default_variables = []
    modes = Modes(values, V, res, names, first, size, rec["h_max"], rel_tol, default_variables)
    info = {"h_max": float(rec["h_max"]), "shift": float(rec["shift"]), "iterations": int(rec["iterations"]),
            "unconverged": int(rec["unconverged"]), "setup_ms": float(rec["setup_ms"]), "solve_ms": float(rec["solve_ms"]),
            "engine": engine}
    return modes, info


def covariance_bracket(modes: Modes, variables=None):
    """name -> (lower, slack) with lower <= Sigma_vv <= lower + slack I: ``lower`` from the first k-1 modes, ``slack`` =
    1 / lambda_{k-1}.  ``variables``: names; None: those ``marginal_covariances`` defaults to (every landmark, the last pose
    of every chain).  Raises where a mode in use is undetermined: the covariance does not exist then."""
    zero = modes.undetermined()
    if zero:
        j, shares = zero[0]
        raise RuntimeError(f"covariance_bracket: mode {j} (lambda = {modes.values[j]:.3e}) is not determined by the measurements "
                           f"(mostly {shares[0][0]}): the covariance does not exist")
    names = modes._default_variables if variables is None else [str(v) for v in variables]
    if not names:
        raise ValueError("covariance_bracket: no variables")
    k = len(modes.values)
    slack = 1.0 / float(modes.values[k - 1])
    out = {}
    for nm in names:
        B = modes.block(nm)[:, :k - 1]
        out[nm] = ((B / modes.values[:k - 1]) @ B.T, slack)
    return out


__all__ = ["information_spectrum", "covariance_bracket", "Modes", "SpectrumHandle", "device_spectrum", "SPECTRUM_SYMBOLS", "MAX_MODES"]
