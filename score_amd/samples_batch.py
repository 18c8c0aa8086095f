"""Posterior samples of many graphs at once (include/score_samples_batch.h, csrc/score_samples_batch.hpp).

``posterior_samples`` takes one graph, builds one refinement handle and runs a block PCG whose launches are latency-bound on
a small world.  ``posterior_samples_batch`` hands the graphs to the device as groups, by the rule of ``score_amd/groups.py``:
the group handle's union matrix H = J'J is block diagonal, so one union vector carries one draw of every member, and a block
of up to 16 union vectors advances 16 draws of all members per pass over the union matrix (``score_refine_batch_samples``).
Every (member, draw) pair has its own alpha, beta, stopping gate and verdict, every member its own noise stream and its own
probe column: graph i's draws are those ``posterior_samples(..., seed=seed_i)`` forms on it alone, up to the rounding of the
two iterations (the noise is the same stream, the right-hand sides the same sums).

``RefineBatchHandle.samples`` is the raw call on a kept group handle, so a study refines and draws with one create;
``refine_estimate_batch(..., samples=S)`` does exactly that.  ``engine="python"`` is the dense twin
``samples._python_draws`` graph by graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import SAMPLES_BATCH, Cutter, ScoreSamplesBatchInfo, _u64p, bind, ptr, steps_and_converged
from .groups import grouped, paired, per_graph, run_chunks
from .marginals import MAX_BLOCK_WIDTH, _problem_and_point, _select, check_block_solve, n_columns
from .marginals_batch import _flat_ids
from .samples import Samples, _moment_sizes, _n_rows, _python_draws, accumulate_moments
from .solver import _i32p

# the symbols include/score_samples_batch.h declares
SAMPLES_BATCH_SYMBOLS = list(SAMPLES_BATCH)


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, SAMPLES_BATCH)


def batch_draws(handle, points, ids_per_member, n_samples, seeds, first_sample=0, rel_tol=1e-10, max_iters=4000,
                block_width=MAX_BLOCK_WIDTH, with_rhs=False, with_noise=False):
    """``score_refine_batch_samples`` as it is, on a ``RefineBatchHandle``: ``points`` in the problems' own form,
    ``ids_per_member`` the member-local variable ids of every member (an empty list: no steps), ``n_samples`` and ``seeds`` an
    integer or one per member (a member with 0 draws takes no part).  Returns (return code, one dict per member, the call's
    info record).  A member's dict has the keys ``SamplesHandle.draw`` returns -- ``rc`` is 0 iff all ITS draws converged,
    ``info`` the call's record with the member's own ``samples`` and ``batches`` -- plus ``determined`` (1: its probe passed,
    0: it failed, -1: no draws)."""
    probs = handle.probs
    G = len(probs)
    if len(points) != G or len(ids_per_member) != G:
        raise ValueError("one point and one list of variables per member expected")
    counts = [int(s) for s in per_graph(n_samples, G, "n_samples", none=False, scalar=True)]
    keys = [int(s) & 0xFFFFFFFFFFFFFFFF for s in per_graph(seeds, G, "seeds", none=False, scalar=True)]
    lib = _bind(handle.lib)
    _, poses, lms = handle._flat_points(points)
    ids, var_ptr, flat = _flat_ids(ids_per_member)
    ncol = [n_columns(prob, v) for prob, v in zip(probs, ids)]
    on = [max(s, 0) for s in counts]  # (a negative count is the library's error to report)
    n_mom = [_moment_sizes(p)[2] if s else 0 for p, s in zip(probs, on)]
    n_mean = [p.n if s else 0 for p, s in zip(probs, on)]
    total = sum(on)
    moments, means = np.zeros(max(1, sum(n_mom))), np.zeros(max(1, sum(n_mean)))
    steps = np.zeros(max(1, sum(s * c for s, c in zip(on, ncol))))
    rhs = np.zeros(max(1, sum(s * p.n for s, p in zip(on, probs)))) if with_rhs else None
    noise = np.zeros(max(1, sum(s * _n_rows(p) for s, p in zip(on, probs)))) if with_noise else None
    res, its = np.zeros(max(1, total)), np.zeros(max(1, total), dtype=np.int32)
    det = np.zeros(G, dtype=np.int32)
    n_arr = np.ascontiguousarray(counts, dtype=np.int32)
    seed_arr = np.ascontiguousarray(keys, dtype=np.uint64)
    info = ScoreSamplesBatchInfo()
    rc = lib.score_refine_batch_samples(handle.h, ptr(poses), ptr(lms), ptr(seed_arr, _u64p), int(first_sample), ptr(n_arr, _i32p),
                                        ptr(var_ptr, _i32p), ptr(flat, _i32p), float(rel_tol), int(max_iters), int(block_width),
                                        ptr(moments), ptr(means), ptr(steps), ptr(rhs), ptr(noise), ptr(res), ptr(its, _i32p),
                                        ptr(det, _i32p), C.byref(info))
    if rc < 0:
        raise RuntimeError(f"score_refine_batch_samples failed: {lib.score_last_error().decode()}")
    rec, cut, out = info.as_dict(), Cutter(), []
    for g, prob in enumerate(probs):
        S, c, rows = on[g], ncol[g], _n_rows(prob)
        iterations, converged = steps_and_converged(cut(its, S))
        out.append({
            "moments": cut(moments, n_mom[g]) if S else np.zeros(_moment_sizes(prob)[2]),
            "means": cut(means, n_mean[g]) if S else np.zeros(prob.n),
            "steps": cut(steps, S * c, (S, c)), "rhs": cut(rhs, S * prob.n, (S, prob.n)), "noise": cut(noise, S * rows, (S, rows)),
            "residuals": cut(res, S), "iterations": iterations, "converged": converged, "determined": int(det[g]),
            "rc": 0 if np.all(converged) else 1, "info": dict(rec, samples=S, batches=-(-S // int(block_width))),
        })
    return rc, out, rec


def _failed(i, failed, total, max_iters):
    return RuntimeError(f"posterior_samples_batch: graph {i}: {failed} of {total} draws did not converge (max_iters = {max_iters}): "
                        "J'J is singular or nearly so -- information_spectrum(...).undetermined() names the variables the "
                        "measurements do not determine")


def draw_info(rec, member, number, engine, draws=True) -> dict:
    """A graph's ``info`` of a group's block solve: ``rec`` the call's record, ``member`` the graph's dict of the raw call,
    ``number`` the group's.  ``draws``: the call drew samples (``rhs_ms`` and the probe's ``determined``)."""
    info = {"pcg_iters": int(rec["pcg_iters"]), "batches": int(member["info"]["batches"]), "setup_ms": float(rec["setup_ms"]),
            "solve_ms": float(rec["solve_ms"]), "iterations": member["iterations"], "residuals": member["residuals"], "engine": engine,
            "group": number, "passes": int(rec["passes"])}
    if draws:
        info["rhs_ms"], info["determined"] = float(rec["rhs_ms"]), member["determined"]
    return info


HOST_RECORD = {"pcg_iters": 0, "passes": 0, "setup_ms": 0.0, "rhs_ms": 0.0, "solve_ms": 0.0}  # of a call that met no device


def group_samples(handle, probs, points, estimates, selections, indices, number, counts, seeds, first_sample=0, rel_tol=1e-10,
                  max_iters=4000, block_width=MAX_BLOCK_WIDTH, engine="device"):
    """The draws of one group: ``selections[k]`` is ``marginals._select`` of member k, ``estimates[k]`` the SolverResults its
    draws are retracted onto, ``indices[k]`` its graph's number in the caller's list (for messages), ``handle`` the group's
    ``RefineBatchHandle`` (None with ``engine="python"``).  Returns ``(Samples, info)`` per member."""
    out = []
    if engine == "python":
        for prob, point, est, (names, _, size, cols), i, S, seed in zip(probs, points, estimates, selections, indices, counts, seeds):
            delta, b, z, res = _python_draws(prob, point, seed, int(first_sample), S)
            if delta is None:
                raise _failed(i, S, S, max_iters)
            moments, means = accumulate_moments(prob, delta)
            m = {"info": {"batches": 0}, "iterations": np.zeros(S, dtype=np.int64), "residuals": res, "determined": 1}
            info = dict(draw_info(HOST_RECORD, m, number, engine), noise=z, rhs=b, order=names)
            out.append((Samples(prob, est, moments, means, S, names, size, np.ascontiguousarray(delta[:, cols]), first_sample), info))
        return out
    _, members, rec = handle.samples(points, [sel[1] for sel in selections], counts, seeds, first_sample, rel_tol, max_iters, block_width)
    for prob, est, (names, _, size, _), i, S, m in zip(probs, estimates, selections, indices, counts, members):
        failed = int(np.count_nonzero(~m["converged"]))
        if failed:
            raise _failed(i, failed, S, max_iters)
        out.append((Samples(prob, est, m["moments"], m["means"], S, names, size, m["steps"], first_sample),
                    dict(draw_info(rec, m, number, engine), order=names)))
    return out


def _check_draw_arguments(counts, first_sample, block_width, rel_tol, max_iters):
    for S in counts:
        if int(S) != S or S < 1:
            raise ValueError("n_samples must be an integer >= 1 (for every graph)")
    check_block_solve(block_width, rel_tol, max_iters, first_sample, max(counts))


def _seeds_of(seed, count: int) -> list:
    """An integer: graph i draws from the stream of seed + i.  A list: one seed per graph."""
    if np.ndim(seed) == 0:
        return [int(seed) + i for i in range(count)]
    return [int(s) for s in per_graph(seed, count, "seed", none=False)]


def posterior_samples_batch(datas, results, n_samples=64, seed=0, first_sample: int = 0, variables=None, range_weights=None,
                            loop_closure_weights=None, rel_tol: float = 1e-10, max_iters: int = 4000,
                            block_width: int = MAX_BLOCK_WIDTH, engine: str = "device", lib_path: Optional[str] = None,
                            solver_settings: Optional[dict] = None, max_group: int = 64):
    """``posterior_samples`` for many graphs at once: ``datas`` and ``results`` graph by graph, ``variables`` None or a list
    with one entry per graph (None: that graph's default, every landmark and the last pose of every chain; else a list of
    names), ``range_weights`` / ``loop_closure_weights`` lists with one entry per graph.  ``n_samples``: an integer or one per
    graph.  ``seed``: a list with one seed per graph, or an integer -- graph i then draws from the stream of ``seed + i``, so
    that graph i's draws are those of ``posterior_samples(..., seed=seed + i)``; ``first_sample`` is shared.  The graphs are
    grouped by dimension, in chunks of at most ``max_group`` (the rule of ``score_amd/groups.py``); each group is one device
    handle and one ``score_refine_batch_samples`` call (``engine="device"``) or the dense twin graph by graph
    (``engine="python"``).  Returns a list of ``(Samples, info)`` in input order: per graph what ``posterior_samples`` returns,
    plus ``group`` (the group's number), ``passes`` (passes of the group's call; ``batches`` counts those in which the graph
    itself had draws; ``pcg_iters``, ``setup_ms``, ``rhs_ms`` and ``solve_ms`` are the group's) and ``determined`` (the graph's
    own probe).  The single call's ValueErrors are raised with ``graph i:`` in front; draws that do not converge raise
    RuntimeError naming the first such graph."""
    if engine not in ("device", "python"):
        raise ValueError("engine must be 'device' or 'python'")
    datas, results = paired(datas, results, max_group)
    counts = per_graph(n_samples, len(datas), "n_samples", none=False, scalar=True)
    if datas:
        _check_draw_arguments(counts, first_sample, block_width, rel_tol, max_iters)
    counts = [int(s) for s in counts]
    seeds = _seeds_of(seed, len(datas))
    rws = per_graph(range_weights, len(datas), "range_weights")
    lws = per_graph(loop_closure_weights, len(datas), "loop_closure_weights")
    wanted = per_graph(variables, len(datas), "variables")

    def member(i, data, res):
        prob, point = _problem_and_point(data, res, rws[i], lws[i])
        sel = _select(prob, wanted[i])
        if prob.n == 0:
            raise ValueError("the graph has no unknowns")
        return prob, point, sel

    def body(handle, number, idx, probs, points, extras):
        return group_samples(handle, probs, points, [results[i] for i in idx], extras[0], idx, number, [counts[i] for i in idx],
                             [seeds[i] for i in idx], int(first_sample), rel_tol, max_iters, int(block_width), engine)

    groups = grouped(datas, results, member, who="posterior_samples")
    return run_chunks(groups, max_group, [None] * len(datas), body, engine == "device", lib_path, solver_settings)


__all__ = ["posterior_samples_batch", "batch_draws", "group_samples", "SAMPLES_BATCH_SYMBOLS", "ScoreSamplesBatchInfo"]
