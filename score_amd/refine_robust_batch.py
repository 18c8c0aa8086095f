"""Outlier-robust local refinement of many graphs in lock-step (include/score_refine_robust_batch.h,
csrc/score_gn_robust_batch.hpp): the GNC-TLS loop of ``refine_estimate_robust``, one per member, on the group handles of
``refine_estimate_batch``.

Every member has its own ``mu``, its own count of outer solves and its own place in the schedule (first run, inner runs, last
run).  When a member's Levenberg-Marquardt run stops it gets its residuals, the stop rule, ``mu`` and its weights, and is solved
again in the next round while others are mid-run or finished; members whose runs stop in the same round share the launches.
Members never influence one another: member by member the result is ``refine_estimate_robust``'s.

``engine="python"`` is the same controller in Python with SciPy's sparse LU (a ``refine_robust._Stage`` per member over the
rounds of ``refine_batch._LockStep``): it only reorders independent work, so member by member it EQUALS
``refine_estimate_robust(engine="python", linear_solver="scipy")``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import REFINE_ROBUST_BATCH, ScoreRefineRobustSettings, bind
from .groups import follow, grouped, paired, per_graph, run_chunks
from .refine import STOPPED, _as_results, _native_info
from .refine_batch import _LockStep, _problem_of
from .refine_robust import (DONE, FAMILY_LOOP_CLOSURES, FAMILY_RANGES, _check, _check_precisions, _prior, _Stage,
                            loop_closure_residuals, range_residuals, refine_estimate_robust)
from .robust import _robust_info

# the symbols include/score_refine_robust_batch.h declares
REFINE_ROBUST_BATCH_SYMBOLS = list(REFINE_ROBUST_BATCH)


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, REFINE_ROBUST_BATCH)


# ---------------------------------------------------------------------------------------------------------------------
# engine="python": the lock-step twin
# ---------------------------------------------------------------------------------------------------------------------
def _python_robust_lock_step(probs, points, settings):
    """``refine_batch._python_lock_step`` with a stage per member.  Returns (points, last-run members, stages, rounds, the
    passes in which some member changed stage)."""
    G = len(probs)
    R = [_Stage(prob, s) for prob, s in zip(probs, settings)]
    L = _LockStep(probs, points)
    tol, cap = (lambda g: settings[g]["tol"]), (lambda g: R[g].cap())
    for g in range(G):
        L.start(g, tol(g), cap(g))
    rounds = stage_rounds = 0
    while True:
        ended = [g for g in range(G) if R[g].stage != DONE and L.S[g].phase == STOPPED]
        if ended:
            stage_rounds += 1
            for g in ended:
                if R[g].run_stopped(L.u[g], L.S[g]):
                    L.start(g, tol(g), cap(g))
            continue  # (a run may stop where it starts)
        if not L.round(tol, cap):
            break
        rounds += 1
    return L.u, L.S, R, rounds, stage_rounds


# ---------------------------------------------------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------------------------------------------------
def refine_estimate_robust_batch(datas, results, inlier_threshold=3.0, robust_ranges: bool = True, robust_loop_closures: bool = False,
                                 loop_closure_threshold=None, max_outer: int = 50, inner_iters: int = 5, min_weight: float = 1e-6,
                                 mu_step: float = 1.4, max_iters: int = 50, tol: float = 1e-10, engine: str = "native",
                                 range_weights=None, loop_closure_weights=None, lib_path: Optional[str] = None,
                                 solver_settings: Optional[dict] = None, max_group: int = 64, marginals=None):
    """``refine_estimate_robust`` for many graphs at once.  ``inlier_threshold`` and ``loop_closure_threshold`` take a scalar or
    a sequence with one entry per graph (``loop_closure_threshold`` None: the graph's ``inlier_threshold``); ``range_weights`` /
    ``loop_closure_weights`` are lists with one entry per graph (prior weights as ``refine_estimate_robust`` takes them: floored
    at ``min_weight`` in a re-weighted family, and the returned weights are prior x GNC).  The graphs are grouped by dimension,
    in chunks of at most ``max_group`` (the rule of ``score_amd/groups.py``): each group is one device handle and one
    ``score_refine_batch_robust_run`` (``engine="native"``) or one lock-step loop in Python with SciPy's sparse LU
    (``engine="python"``).  Graphs without unknowns are answered on the host.  Returns ``[(refined SolverResults, info), ...]``
    in input order, ``info`` as ``refine_estimate_robust`` builds it (``info["robust"]`` included) plus ``group``, ``rounds``
    (lock-step rounds of the group) and ``stage_rounds`` (the passes in which some member of the group changed stage).

    ``marginals``: True, or a list with one entry per graph as ``marginal_covariances_batch`` takes ``variables`` -- the group's
    handle then keeps the final weights (``keep_weights=1``: precisions prec x w, the plain weight) and computes the marginal
    covariances at the refined points before it is closed; ``info["marginals"]`` is the ``(cov, marginals_info)`` of
    ``marginal_covariances_batch`` for that graph with the returned weights (None for a graph without unknowns).  Where a prior
    weight lies below ``min_weight`` in a re-weighted family, the kept precisions carry the floor (prec x min_weight x w), not
    the prior weight itself.  Errors about one graph are raised with ``graph i:`` in front."""
    from .marginals_batch import marginals_follow_up

    f_rng, f_rel = bool(robust_ranges), bool(robust_loop_closures)
    datas, results = paired(datas, results, max_group)
    N = len(datas)
    cs = per_graph(inlier_threshold, N, "inlier_threshold", scalar=True)
    crs = per_graph(loop_closure_threshold, N, "loop_closure_threshold", scalar=True)
    cs = [float(c) for c in cs]
    crs = [c if cr is None else float(cr) for c, cr in zip(cs, crs)]
    linear_solver = "scipy" if engine == "python" else "device"
    _check(1.0, 1.0, max_outer, inner_iters, min_weight, mu_step, engine, linear_solver, f_rng, f_rel)  # what every graph shares
    for i in range(N):
        try:
            _check(cs[i], crs[i], max_outer, inner_iters, min_weight, mu_step, engine, linear_solver, f_rng, f_rel)
        except ValueError as e:
            raise ValueError(f"graph {i}: {e}") from None
    families = (FAMILY_RANGES if f_rng else 0) | (FAMILY_LOOP_CLOSURES if f_rel else 0)
    rws = per_graph(range_weights, N, "range_weights")
    lws = per_graph(loop_closure_weights, N, "loop_closure_weights")
    with_marginals = marginals is not None and marginals is not False
    follow_ups = [marginals_follow_up(marginals, N)] if with_marginals else []
    common = dict(max_outer=int(max_outer), inner_iters=int(inner_iters), min_weight=float(min_weight), mu_step=float(mu_step),
                  max_iters=int(max_iters), tol=float(tol), families=families)
    out: list = [None] * N

    def member(i, data, res):
        prob, point = _problem_of(data, res, _prior(rws[i], float(min_weight), f_rng), _prior(lws[i], float(min_weight), f_rel))
        _check_precisions(prob, f_rng, f_rel, f"graph {i}: ")
        if prob.n == 0:  # nothing to refine: the host's answer, as refine_estimate_robust gives it
            out[i] = refine_estimate_robust(data, res, inlier_threshold=cs[i], robust_ranges=f_rng, robust_loop_closures=f_rel,
                                            loop_closure_threshold=crs[i], max_outer=max_outer, inner_iters=inner_iters,
                                            min_weight=min_weight, mu_step=mu_step, max_iters=max_iters, tol=tol, engine="python",
                                            linear_solver="scipy", range_weights=rws[i], loop_closure_weights=lws[i])
            out[i][1].update({f.key: None for f in follow_ups})
            return None
        for f in follow_ups:  # (the selection's errors before any work)
            f.keep(i, prob)
        return prob, point

    def body(handle, number, idx, probs, points, extras):
        if handle is None:
            settings = [dict(common, c=cs[i], c_rel=crs[i]) for i in idx]
            pts, S, R, rounds, stage_rounds = _python_robust_lock_step(probs, points, settings)
            per, infos, loops = [], [], []
            for prob, pt, s, st in zip(probs, pts, S, R):
                per.append((st.w, range_residuals(prob, pt, st.prec0), st.wl, loop_closure_residuals(prob, pt, st.kappa0, st.tau0)))
                infos.append({"cost_initial": st.cost_initial, "cost_final": s.f, "iterations": st.lm, "grad_inf": s.gnorm,
                              "linear_solver": "scipy", "engine": "python", "pcg_iters": 0, "linear_solves": st.linear_solves})
                loops.append((st.k, st.mu, st.what == "converged"))
            if with_marginals:
                for st in R:
                    st.weigh(None)  # the kept precisions: prec w
            extra = follow(follow_ups, None, number, idx, probs, pts, [info["cost_final"] for info in infos])
        else:
            recs = []
            for i in idx:
                rs = ScoreRefineRobustSettings()
                rs.inlier_threshold, rs.rel_threshold, rs.mu_step, rs.min_weight = cs[i], crs[i], float(mu_step), float(min_weight)
                rs.families, rs.max_outer, rs.inner_iters = families, int(max_outer), int(inner_iters)
                rs.max_iters, rs.tol = int(max_iters), float(tol)
                recs.append(rs)
            pts, per, raw = handle.robust_run(points, recs, keep_weights=with_marginals)
            extra = follow(follow_ups, handle, number, idx, probs, pts, [r["cost_final"] for r in raw])
            rounds, stage_rounds = handle.robust_rounds()
            infos = [_native_info(r, "lm_iterations") for r in raw]
            loops = [(r["outer_iterations"], r["mu"], bool(r["converged"])) for r in raw]
        got = []
        for i, prob, pt, info, (w, r, wl, rl), (outer, mu, conv), more in zip(idx, probs, pts, infos, per, loops, extra):
            if rws[i] is not None:  # prior x GNC
                w = w * np.asarray(rws[i], dtype=np.float64)
            if lws[i] is not None:
                wl = wl * np.asarray(lws[i], dtype=np.float64)
            info["robust"] = _robust_info(w, r, outer, mu, conv, wl if f_rel else None, rl if f_rel else None)
            info["group"], info["rounds"], info["stage_rounds"] = number, rounds, stage_rounds
            info.update(more)
            got.append((_as_results(prob, pt, results[i], info["cost_final"]), info))
        return got

    return run_chunks(grouped(datas, results, member, named=False), max_group, out, body, engine != "python", lib_path, solver_settings)


__all__ = ["refine_estimate_robust_batch", "REFINE_ROBUST_BATCH_SYMBOLS"]
