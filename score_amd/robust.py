"""Outlier-robust range measurements and loop closures: graduated non-convexity with a truncated-least-squares loss
(GNC-TLS; Yang, Antonante, Tzoumas, Carlone, RA-L 2020) around the SCORE relaxation.

Every range costs ``w * max(0, |t_a - t_b| - dist)^2`` in the relaxation: a range measured too SHORT pulls
its two ends together, one measured too long costs nothing.  Multipath and wrong associations of acoustic ranging produce
the first kind; a handful of them can spoil an estimate.  The loop below re-weights the ranges between outer solves
(include/score_robust.h states it in full):

    solve with precisions prec * max(w, min_weight);  r = sqrt(prec) * max(0, |t_a - t_b| - dist)  (relaxed translations);
    stop (first solve, 2 max r^2 <= c^2 | a later solve on binary weights | max_outer);  mu0 = c^2 / (2 max r^2 - c^2), then
    mu <- mu_step * mu;  w = gnc_tls_weight(r, mu, c).

Loop closures are the second family (``robust_loop_closures=True``): a false place recognition is a relative-pose term of
odometry-grade precision that bends a whole chain.  Its residual is the square root of its own term in the relaxed objective,
``relaxed_loop_closure_residuals``; its weight scales both precisions, kappa and tau; a graph keeps one mu for both families
(the smallest of the families' mu0 after the first solve).  Odometry and landmark priors keep weight 1.

``engine="device"`` runs the whole loop behind the C ABI (``score_robust_solve_rel``: the graphs go up once, weights and
control records are computed on the device, csrc/score_robust.hpp);
``engine="python"`` is the readable twin -- a host loop over ``solve_score_batch`` on re-weighted ``ArrayGraph`` s -- that
also runs on the oracle's CPU twin (``lib_path``).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import compat
from .assemble import QCQP_RELAXATION, SOCP_RELAXATION, check_valid_relaxation
from .bindings import ROBUST, ScoreRobustInfo, ScoreRobustSettings, bind, ptr
from .solver import ScoreInfo, _i32p, load_library, make_settings

# the symbols include/score_robust.h declares (include/score_hip.h's list, solver.ABI_SYMBOLS, stays that header's)
ROBUST_SYMBOLS = list(ROBUST)

BINARY_TOL = 1e-6  # a weight within this of 0 or 1 counts as decided


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, ROBUST)


# ---------------------------------------------------------------------------------------------------------------------
# the rule (the device's is csrc/score_robust.hpp: gnc_tls_weight -- same operations, same order)
# ---------------------------------------------------------------------------------------------------------------------
def gnc_tls_weight(r, mu: float, c: float) -> np.ndarray:
    """GNC-TLS weights of residuals ``r`` (sigma units) at parameter ``mu`` and inlier threshold ``c``:
    1 for r^2 <= mu / (mu + 1) c^2, 0 for r^2 >= (mu + 1) / mu c^2, c / |r| sqrt(mu (mu + 1)) - mu in between."""
    r = np.abs(np.asarray(r, dtype=np.float64))
    r2, c2 = r * r, c * c
    lo, hi = mu / (mu + 1.0) * c2, (mu + 1.0) / mu * c2
    w = np.zeros_like(r)
    mid = (r2 > lo) & (r2 < hi)
    w[mid] = c / r[mid] * np.sqrt(mu * (mu + 1.0)) - mu
    w[r2 <= lo] = 1.0
    return w


def initial_mu(r2max: float, c: float) -> float:
    """mu0 = c^2 / (2 max r^2 - c^2) after the first solve (only defined when 2 max r^2 > c^2: there are outliers)."""
    return c * c / (2.0 * r2max - c * c)


def relaxed_range_residuals(arrays: dict, relaxed_poses: np.ndarray, landmarks: np.ndarray) -> np.ndarray:
    """r = sqrt(prec) * max(0, |t_a - t_b| - dist) from the relaxation's translations (``relaxed_poses``: (Np, d, d+1)
    blocks [R | t]; ``landmarks``: (Nl, d)) -- the square root of each range's own term in the relaxed objective."""
    d = int(arrays["dim"])
    tr = np.asarray(relaxed_poses, dtype=np.float64)[:, :, d]
    if len(landmarks):
        tr = np.concatenate([tr, np.asarray(landmarks, dtype=np.float64).reshape(-1, d)])
    delta = tr[arrays["rng_a"]] - tr[arrays["rng_b"]]
    nn = np.zeros(len(delta))
    for k in range(d):  # (the device's order: sum over k, no fused multiply-add)
        nn = nn + delta[:, k] * delta[:, k]
    return np.sqrt(arrays["rng_prec"]) * np.maximum(0.0, np.sqrt(nn) - arrays["rng_dist"])


def n_loop_closures_of(arrays: dict) -> int:
    """Loop closures of a graph's arrays: its trailing ``n_rel - sum(chain_len - 1)`` relative-pose entries (odometry, then
    loop closures: include/score_hip.h)."""
    return int(len(arrays["rel_base"]) - int(np.sum(np.asarray(arrays["chain_len"], dtype=np.int64) - 1)))


def relaxed_loop_closure_residuals(arrays: dict, relaxed_poses: np.ndarray) -> np.ndarray:
    """r = sqrt(kappa |t_j - t_i - R_i t~|^2 + tau |R_j - R_i R~|_F^2) of every loop closure (the trailing relative-pose entries
    of ``arrays``) from the relaxation's blocks (``relaxed_poses``: (Np, d, d+1) blocks [R | t]; the pinned pose is [I | 0]) and
    the measured precisions -- the square root of each loop closure's own term in the relaxed objective."""
    d = int(arrays["dim"])
    n_lc = n_loop_closures_of(arrays)
    X = np.asarray(relaxed_poses, dtype=np.float64)
    sl = slice(len(arrays["rel_base"]) - n_lc, len(arrays["rel_base"]))
    Xi, Xj = X[np.asarray(arrays["rel_base"])[sl]], X[np.asarray(arrays["rel_to"])[sl]]
    tm = np.asarray(arrays["rel_t"], dtype=np.float64).reshape(-1, d)[sl]
    Rm = np.asarray(arrays["rel_R"], dtype=np.float64).reshape(-1, d, d)[sl]
    st, sR = np.zeros(n_lc), np.zeros(n_lc)
    for k in range(d):  # (the device's order: rows k, columns c, sums over the inner index, no fused multiply-add)
        s = np.zeros(n_lc)
        for c in range(d):
            s = s + Xi[:, k, c] * tm[:, c]
        dl = Xj[:, k, d] - Xi[:, k, d] - s
        st = st + dl * dl
        for c in range(d):
            u = np.zeros(n_lc)
            for j in range(d):
                u = u + Xi[:, k, j] * Rm[:, j, c]
            dr = Xj[:, k, c] - u
            sR = sR + dr * dr
    return np.sqrt(np.asarray(arrays["rel_kappa"], dtype=np.float64)[sl] * st + np.asarray(arrays["rel_tau"], dtype=np.float64)[sl] * sR)


def _check_families(robust_ranges, robust_loop_closures, inlier_threshold, loop_closure_threshold) -> float:
    """The loop closures' threshold (None: the ranges')."""
    if not robust_ranges and not robust_loop_closures:
        raise ValueError("solve_score_robust: robust_ranges and robust_loop_closures are both off: nothing to re-weight")
    c_rel = inlier_threshold if loop_closure_threshold is None else loop_closure_threshold
    if not (np.isfinite(c_rel) and c_rel > 0):
        raise ValueError(f"loop_closure_threshold must be positive and finite, not {c_rel}")
    return float(c_rel)


def _check_args(relaxation_type, qcqp_mode, inlier_threshold, max_outer, min_weight, mu_step, engine) -> None:
    check_valid_relaxation(relaxation_type)
    if relaxation_type == QCQP_RELAXATION and qcqp_mode != "via_socp":
        raise ValueError(f"solve_score_robust: the QCQP relaxation is solved through the SOCP (qcqp_mode='via_socp'), not {qcqp_mode!r}")
    if not (np.isfinite(inlier_threshold) and inlier_threshold > 0):
        raise ValueError(f"inlier_threshold must be positive and finite, not {inlier_threshold}")
    if int(max_outer) < 1:
        raise ValueError(f"max_outer must be >= 1, not {max_outer}")
    if not (0.0 < min_weight <= 1.0):
        raise ValueError(f"min_weight must lie in (0, 1], not {min_weight}")
    if not (np.isfinite(mu_step) and mu_step > 1.0):
        raise ValueError(f"mu_step must be finite and > 1, not {mu_step}")
    if engine not in ("device", "python"):
        raise ValueError(f"engine must be 'device' or 'python', not {engine!r}")


def _arrays_of(data, loop_closures: bool = False) -> dict:
    from .native import ArrayGraph, cached_graph_arrays, unconnected_variable_names

    a = data.arrays if isinstance(data, ArrayGraph) else cached_graph_arrays(data)
    unconnected_variables = unconnected_variable_names(a)  # score/solve_score.py:28-32
    assert len(unconnected_variables) == 0, f"Found {unconnected_variables} unconnected variables. "
    prec = np.asarray(a["rng_prec"], dtype=np.float64)
    if prec.size and not (np.all(np.isfinite(prec)) and np.all(prec > 0)):
        raise ValueError("solve_score_robust: every range precision must be positive and finite")
    if loop_closures:
        n_lc = n_loop_closures_of(a)
        if n_lc < 0:
            raise ValueError("solve_score_robust: fewer relative-pose entries than odometry steps")
        for key in ("rel_kappa", "rel_tau"):
            v = np.asarray(a[key], dtype=np.float64)[len(a["rel_base"]) - n_lc:]
            if v.size and not (np.all(np.isfinite(v)) and np.all(v > 0)):
                raise ValueError(f"solve_score_robust: every loop closure's precision ({key}) must be positive and finite")
    return a


def _weighted(a: dict, w: np.ndarray, min_weight: float, w_rel: Optional[np.ndarray] = None) -> dict:
    """The graph's arrays with range precisions prec * max(w, min_weight) and, with ``w_rel``, the loop closures' kappa and tau
    times max(w_rel, min_weight) (a graph of the generator's batch included: the copy is an ordinary graph, uploaded as it is)."""
    out = {k: v for k, v in a.items() if k not in ("_owner", "_index", "_cstruct")}
    out["rng_prec"] = np.ascontiguousarray(np.asarray(a["rng_prec"], dtype=np.float64) * np.maximum(w, min_weight))
    if w_rel is not None and len(w_rel):
        f = np.maximum(w_rel, min_weight)
        for key in ("rel_kappa", "rel_tau"):
            v = np.array(a[key], dtype=np.float64)
            v[len(v) - len(f):] *= f
            out[key] = v
    return out


def _settings(datas, relaxation_type: str, solver_settings: Optional[dict], lib_path: Optional[str]) -> dict:
    """What solve_score_batch hands to the library for these graphs (the same defaults, the same loop-closure rule)."""
    from .native import ArrayGraph
    from .solve_score import DEFAULT_SOLVER_SETTINGS, _loop_closure_settings

    settings = dict(DEFAULT_SOLVER_SETTINGS)
    settings.update(solver_settings or {})
    lc = any((d.n_loop_closures if isinstance(d, ArrayGraph) else len(d.loop_closure_measurements)) for d in datas)
    _loop_closure_settings(settings, solver_settings, lc, lib_path)
    return settings


def _robust_info(w, r, k, mu, converged, w_rel=None, r_rel=None) -> dict:
    w = np.asarray(w, dtype=np.float64)
    info = dict(weights=w, residuals=np.asarray(r, dtype=np.float64), outliers=np.nonzero(w < 0.5)[0],
                outer_iterations=int(k), mu=float(mu), converged=bool(converged))
    if w_rel is not None:  # (the loop closures' family is on)
        w_rel = np.asarray(w_rel, dtype=np.float64)
        info.update(loop_closure_weights=w_rel, loop_closure_residuals=np.asarray(r_rel, dtype=np.float64),
                    loop_closure_outliers=np.nonzero(w_rel < 0.5)[0])
    return info


# ---------------------------------------------------------------------------------------------------------------------
# engine="python": the readable twin
# ---------------------------------------------------------------------------------------------------------------------
def _binary(w: np.ndarray) -> bool:
    return bool(np.all((np.abs(w) <= BINARY_TOL) | (np.abs(1.0 - w) <= BINARY_TOL)))


def _python_loop(datas, arrays, relaxation_type, c, max_outer, min_weight, mu_step, solver_settings, lib_path,
                 f_rng: bool = True, f_rel: bool = False, c_rel: float = 0.0) -> list:
    from .native import ArrayGraph
    from .solve_score import solve_score_batch

    n = len(arrays)
    w = [np.ones(len(a["rng_a"])) for a in arrays]
    w_rel = [np.ones(n_loop_closures_of(a)) if f_rel else None for a in arrays]
    mu = [0.0] * n
    out = [None] * n
    active = list(range(n))
    for k in range(1, int(max_outer) + 1):
        graphs = [ArrayGraph(_weighted(arrays[m], w[m], min_weight, w_rel[m])) for m in active]
        results = solve_score_batch(graphs, relaxation_type=relaxation_type, solver_settings=solver_settings, lib_path=lib_path)
        keep = []
        for m, res in zip(active, results):
            a = arrays[m]
            r = relaxed_range_residuals(a, res.relaxed_poses.array, res.landmarks.array)
            r_rel = relaxed_loop_closure_residuals(a, res.relaxed_poses.array) if f_rel else None
            # the enabled families: (largest r^2, threshold, weights of this solve)
            fams = []
            if f_rng:
                fams.append((float(np.max(r * r)) if len(r) else 0.0, c, w[m]))
            if f_rel:
                fams.append((float(np.max(r_rel * r_rel)) if len(r_rel) else 0.0, c_rel, w_rel[m]))
            with_outliers = [(r2, cf) for r2, cf, _ in fams if 2.0 * r2 > cf * cf]
            if not all(np.isfinite(r2) for r2, _, _ in fams):
                stop, conv = True, False
            elif k == 1 and not with_outliers:
                stop, conv = True, True
            elif k > 1 and all(_binary(wf) for _, _, wf in fams):
                stop, conv = True, True
            else:
                stop, conv = k >= int(max_outer), False
            if stop:
                res.info["robust"] = _robust_info(w[m], r, k, mu[m], conv, w_rel[m], r_rel)
                out[m] = res
                continue
            mu[m] = min(initial_mu(r2, cf) for r2, cf in with_outliers) if k == 1 else mu[m] * mu_step
            if f_rng:
                w[m] = gnc_tls_weight(r, mu[m], c)
            if f_rel:
                w_rel[m] = gnc_tls_weight(r_rel, mu[m], c_rel)
            keep.append(m)
        active = keep
        if not active:
            break
    return out


# ---------------------------------------------------------------------------------------------------------------------
# engine="device": score_robust_solve
# ---------------------------------------------------------------------------------------------------------------------
def _device_group(datas, arrays, relaxation_type, c, max_outer, min_weight, mu_step, settings, lib_path,
                  f_rng: bool = True, f_rel: bool = False, c_rel: float = 0.0) -> list:
    from .native import ScoreGraph, graph_model, score_graph_struct
    from .rounding import finish_device_poses

    lib = _bind(load_library(lib_path))
    count = len(arrays)
    d = int(arrays[0]["dim"])
    qdirs = relaxation_type == QCQP_RELAXATION
    st = make_settings(lib, settings)
    rs = ScoreRobustSettings()
    lib.score_robust_default_settings(C.byref(rs))
    rs.inlier_threshold, rs.mu_step, rs.min_weight = float(c), float(mu_step), float(min_weight)
    rs.max_outer, rs.qcqp_directions = int(max_outer), 1 if qdirs else 0
    gs = (ScoreGraph * count)()
    for i, a in enumerate(arrays):
        C.memmove(C.byref(gs[i]), C.byref(score_graph_struct(a, 0)), C.sizeof(ScoreGraph))
    Np = [len(a["pose_names"]) for a in arrays]
    Nl = [len(a["landmark_names"]) for a in arrays]
    Nr = [len(a["rng_a"]) for a in arrays]
    Nc = [n_loop_closures_of(a) if f_rel else 0 for a in arrays]
    rw = d if qdirs else 1
    W, Rr = np.empty(max(1, sum(Nr))), np.empty(max(1, sum(Nr)))
    Wc, Rc = np.ones(max(1, sum(Nc))), np.zeros(max(1, sum(Nc)))
    T, B = np.empty((sum(Np), d + 1, d + 1)), np.empty((sum(Np), d, d + 1))
    Lm, Rg = np.empty((max(1, sum(Nl)), d)), np.empty((max(1, sum(Nr)), rw))
    F = np.empty(sum(Np), dtype=np.int32)
    infos, rinfos = (ScoreInfo * count)(), (ScoreRobustInfo * count)()
    rc = lib.score_robust_solve_rel(gs, count, C.byref(st), C.byref(rs), (1 if f_rng else 0) | (2 if f_rel else 0), float(c_rel),
                                    ptr(W), ptr(Rr), ptr(Wc), ptr(Rc), ptr(T), ptr(B), ptr(Lm), ptr(Rg), ptr(F, _i32p), infos, rinfos)
    if rc != 0:
        raise ValueError(f"score_robust_solve failed: {lib.score_last_error().decode()}")
    backend = lib.score_backend().decode()
    out, po, lo, ro, co = [], 0, 0, 0, 0
    for i, (data, a) in enumerate(zip(datas, arrays)):
        model = graph_model(a, SOCP_RELAXATION)
        sl_p, sl_l, sl_r = slice(po, po + Np[i]), slice(lo, lo + Nl[i]), slice(ro, ro + Nr[i])
        sl_c = slice(co, co + Nc[i])
        po += Np[i]; lo += Nl[i]; ro += Nr[i]; co += Nc[i]
        info = dict(infos[i].as_dict(), backend=backend)
        ri = rinfos[i]
        info["robust"] = _robust_info(W[sl_r].copy(), Rr[sl_r].copy(), ri.outer_iterations, ri.mu, ri.converged,
                                      Wc[sl_c].copy() if f_rel else None, Rc[sl_c].copy() if f_rel else None)
        info["robust"].update(setup_ms=float(ri.setup_ms), solve_ms=float(ri.solve_ms), total_ms=float(ri.total_ms))
        solved = info["status"] == 1
        Ti = finish_device_poses(T[sl_p].copy(), B[sl_p].copy(), F[sl_p].copy())
        values = compat.VariableValues(d, compat.ArrayDict(model.pose_names, Ti), compat.ArrayDict(model.landmark_names, Lm[sl_l].copy()),
                                       compat.ArrayDict(model.range_keys, Rg[sl_r].copy()))
        out.append(compat.SolverResults(
            variables=values, total_time=(ri.setup_ms + ri.solve_ms) * 1e-3, solved=solved,
            pose_chain_names=model.pose_chain_names if model.pose_chain_names is not None else data.get_pose_chain_names(),
            solver_cost=info.get("pobj"), info=info, relaxed_poses=compat.ArrayDict(model.pose_names, B[sl_p].copy()),
        ))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
def solve_score_robust(
    data, relaxation_type: str = QCQP_RELAXATION, inlier_threshold: float = 3.0, max_outer: int = 50, min_weight: float = 1e-6,
    mu_step: float = 1.4, engine: str = "device", solver_settings: Optional[dict] = None, lib_path: Optional[str] = None,
    qcqp_mode: str = "via_socp", robust_loop_closures: bool = False, loop_closure_threshold: Optional[float] = None,
    robust_ranges: bool = True,
) -> compat.SolverResults:
    """``solve_score`` with GNC-TLS re-weighting of the range measurements.  ``info["robust"]`` holds ``weights`` and
    ``residuals`` (in the order of the graph's range list: ``graph_arrays``' ``rng_*``), ``outliers`` (indices of the ranges
    whose final weight is below 1/2), ``outer_iterations``, ``mu`` and ``converged``.  A graph without outliers takes one
    solve, and its result is ``solve_score``'s.  Relaxations: "SOCP", and "QCQP" through the SOCP.

    ``robust_loop_closures=True`` re-weights the loop closures too (threshold ``loop_closure_threshold``; None:
    ``inlier_threshold``), ``robust_ranges=False`` leaves the ranges at weight 1 (their ``weights`` are ones, their
    ``residuals`` still those of the last solve).  With the loop closures on, ``info["robust"]`` also holds
    ``loop_closure_weights``, ``loop_closure_residuals`` and ``loop_closure_outliers`` (indices into
    ``data.loop_closure_measurements`` with final weight below 1/2)."""
    return solve_score_robust_batch([data], relaxation_type, inlier_threshold, max_outer, min_weight, mu_step, engine,
                                    solver_settings, lib_path, qcqp_mode=qcqp_mode, robust_loop_closures=robust_loop_closures,
                                    loop_closure_threshold=loop_closure_threshold, robust_ranges=robust_ranges)[0]


def solve_score_robust_batch(
    datas: Sequence, relaxation_type: str = QCQP_RELAXATION, inlier_threshold: float = 3.0, max_outer: int = 50,
    min_weight: float = 1e-6, mu_step: float = 1.4, engine: str = "device", solver_settings: Optional[dict] = None,
    lib_path: Optional[str] = None, qcqp_mode: str = "via_socp", workers: int = 4, group_size: Optional[int] = None,
    robust_loop_closures: bool = False, loop_closure_threshold: Optional[float] = None, robust_ranges: bool = True,
) -> List[compat.SolverResults]:
    """``solve_score_robust`` for many graphs.  ``engine="device"``: lock-step groups as in ``solve_score_batch`` (one dimension per
    group, graphs of similar size together, at most 16 per group, one group per worker thread); within a group every graph
    keeps its own mu and its own stopping point, and a graph that stops leaves the group's next handle."""
    _check_args(relaxation_type, qcqp_mode, inlier_threshold, max_outer, min_weight, mu_step, engine)
    f_rng, f_rel = bool(robust_ranges), bool(robust_loop_closures)
    c_rel = _check_families(f_rng, f_rel, inlier_threshold, loop_closure_threshold)
    if len(datas) == 0:
        return []
    arrays = [_arrays_of(d_, f_rel) for d_ in datas]
    settings = _settings(datas, relaxation_type, solver_settings, lib_path)
    c = float(inlier_threshold)
    if engine == "python":
        return _python_loop(datas, arrays, relaxation_type, c, max_outer, float(min_weight), float(mu_step), solver_settings, lib_path,
                            f_rng, f_rel, c_rel)
    group = max(1, min(16, -(-len(datas) // max(1, workers)))) if group_size is None else max(1, int(group_size))
    chunks = []
    for dim in sorted({int(a["dim"]) for a in arrays}):
        sub = sorted([i for i, a in enumerate(arrays) if int(a["dim"]) == dim], key=lambda i: len(arrays[i]["pose_names"]) + len(arrays[i]["rng_a"]))
        chunks += [sub[i : i + group] for i in range(0, len(sub), group)]

    def one(idx):
        return _device_group([datas[i] for i in idx], [arrays[i] for i in idx], relaxation_type, c, max_outer, float(min_weight),
                             float(mu_step), settings, lib_path, f_rng, f_rel, c_rel)

    if workers <= 1 or len(chunks) == 1:
        parts = [one(ch) for ch in chunks]
    else:
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=min(workers, len(chunks))) as pool:
            parts = list(pool.map(one, chunks))
    out = [None] * len(datas)
    for idx, rs in zip(chunks, parts):
        for i, r in zip(idx, rs):
            out[i] = r
    return out


def corrupt_ranges(data, fraction: float, low: float = 0.3, high: float = 0.6, seed: int = 0):
    """A copy of ``data`` (a FactorGraphData or an ``ArrayGraph``) as an ``ArrayGraph`` with about ``fraction`` of its ranges
    measured SHORT -- the measured distance times U(low, high): the outliers that pull the relaxation -- and the indices of the
    corrupted ranges.  For tests and measurements."""
    from .native import ArrayGraph

    a = _arrays_of(data)
    rng = np.random.default_rng(seed)
    nr = len(a["rng_a"])
    bad = np.sort(rng.choice(nr, size=int(round(fraction * nr)), replace=False)) if nr else np.zeros(0, np.int64)
    out = {k: v for k, v in a.items() if k not in ("_owner", "_index", "_cstruct")}
    dist = np.array(a["rng_dist"], dtype=np.float64)
    dist[bad] *= rng.uniform(low, high, size=len(bad))
    out["rng_dist"] = dist
    return ArrayGraph(out), bad


def corrupt_loop_closures(data, count: int, spread: float = 8.0, seed: int = 0):
    """A copy of ``data`` as an ``ArrayGraph`` with ``count`` of its loop closures replaced by false place recognitions -- a
    translation drawn from U(-spread, spread)^d and a rotation drawn uniformly in the angle (2-D) or the rotation vector (3-D),
    the precisions kept -- and the indices of the corrupted loop closures (into ``data.loop_closure_measurements``).  For tests
    and measurements."""
    from .manhattan import _rotvec
    from .native import ArrayGraph

    a = _arrays_of(data)
    d = int(a["dim"])
    n_lc = n_loop_closures_of(a)
    rng = np.random.default_rng(seed)
    bad = np.sort(rng.choice(n_lc, size=count, replace=False))
    out = {k: v for k, v in a.items() if k not in ("_owner", "_index", "_cstruct")}
    rel_t = np.array(a["rel_t"], dtype=np.float64).reshape(-1, d)
    rel_R = np.array(a["rel_R"], dtype=np.float64).reshape(-1, d, d)
    first = len(a["rel_base"]) - n_lc
    for k in bad:
        rel_t[first + k] = rng.uniform(-spread, spread, size=d)
        if d == 2:
            th = rng.uniform(-np.pi, np.pi)
            rel_R[first + k] = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        else:
            rel_R[first + k] = _rotvec(rng.uniform(-np.pi, np.pi, size=3))
    out["rel_t"], out["rel_R"] = np.ascontiguousarray(rel_t.reshape(np.shape(a["rel_t"]))), np.ascontiguousarray(rel_R.reshape(np.shape(a["rel_R"])))
    return ArrayGraph(out), bad


__all__ = ["solve_score_robust", "solve_score_robust_batch", "gnc_tls_weight", "initial_mu", "relaxed_range_residuals",
           "relaxed_loop_closure_residuals", "corrupt_ranges", "corrupt_loop_closures", "ROBUST_SYMBOLS"]
