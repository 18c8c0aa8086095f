"""Range leverage and predicted range variances of many graphs at once (include/score_leverage_batch.h,
csrc/score_leverage_batch.hpp).

``range_leverage`` / ``predicted_range_variances`` take one graph, build one refinement handle and run block solves whose
launches are latency-bound on a small world.  The questions they answer are study questions -- over 64 generated worlds,
which share of the ranges is uncontrolled?  what variance does a candidate beacon-pose range have in each world? -- so
``range_leverage_batch`` and ``predicted_range_variances_batch`` hand the graphs to the device as groups, by the rule of
``score_amd/groups.py``: one union vector carries one draw (one pair's column) of every member.  Graph i's draws
are those of ``range_leverage(..., seed=seed + i)`` on it alone (the same noise stream, the same right-hand sides), its sums
those of that call up to the rounding of the two iterations.

``RefineBatchHandle.leverage`` / ``.range_variances`` are the raw calls on a kept group handle, so a study refines and
analyses with one create; ``refine_estimate_batch(..., leverage=S)`` does exactly that.  ``engine="python"`` is the single
functions' python engine graph by graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import LEVERAGE_BATCH, Cutter, ScoreMarginalsBatchInfo, ScoreSamplesBatchInfo, _u64p, bind, ptr, steps_and_converged
from .groups import group_size, grouped, paired, per_graph, run_chunks
from .leverage import (Leverage, PredictedRanges, _check_block, _singular, measurement_counts, pair_ids, predicted_range_variances,
                       range_leverage)
from .marginals import MAX_BLOCK_WIDTH, _problem_and_point
from .samples_batch import _check_draw_arguments, _seeds_of, draw_info
from .solver import _i32p

# the symbols include/score_leverage_batch.h declares
LEVERAGE_BATCH_SYMBOLS = list(LEVERAGE_BATCH)
SUMS = ("lev_sum", "lev_sq", "red_sum", "red_sq")


def _flat_pairs(pairs_per_member, count: int):
    """(per member (C_g, 2) int32 ids, pair_ptr, pair_a, pair_b) of one list of id pairs (or None) per member."""
    if len(pairs_per_member) != count:
        raise ValueError(f"one list of pairs per member expected ({count}), got {len(pairs_per_member)}")
    ids = [np.zeros((0, 2), dtype=np.int32) if p is None else np.asarray(p, dtype=np.int32).reshape(-1, 2) for p in pairs_per_member]
    pair_ptr = np.concatenate([[0], np.cumsum([len(p) for p in ids])]).astype(np.int32)
    flat = np.concatenate(ids) if ids else np.zeros((0, 2), dtype=np.int32)
    return ids, pair_ptr, np.ascontiguousarray(flat[:, 0]), np.ascontiguousarray(flat[:, 1])


def batch_leverage(handle, points, pairs_per_member, n_samples, seeds, first_sample=0, rel_tol=1e-10, max_iters=4000,
                   block_width=MAX_BLOCK_WIDTH):
    """``score_refine_batch_leverage`` as it is, on a ``RefineBatchHandle``: ``points`` in the problems' own form,
    ``pairs_per_member`` the member-local variable id pairs of every member (None or an empty list: none), ``n_samples`` and
    ``seeds`` an integer or one per member (a member with 0 draws takes no part).  Returns (return code, one dict per member,
    the call's info record).  A member's dict has the keys ``LeverageHandle.leverage`` returns -- ``rc`` is 0 iff all ITS
    draws converged, ``info`` the call's record with the member's own ``samples`` and ``batches`` -- plus ``determined``."""
    probs = handle.probs
    G = len(probs)
    if len(points) != G:
        raise ValueError("one point per member expected")
    counts = [int(s) for s in per_graph(n_samples, G, "n_samples", none=False, scalar=True)]
    keys = [int(s) & 0xFFFFFFFFFFFFFFFF for s in per_graph(seeds, G, "seeds", none=False, scalar=True)]
    lib = bind(handle.lib, LEVERAGE_BATCH)
    _, poses, lms = handle._flat_points(points)
    ids, pair_ptr, pa, pb = _flat_pairs(pairs_per_member, G)
    on = [max(s, 0) for s in counts]  # (a negative count is the library's error to report)
    n_meas = [sum(measurement_counts(p)) for p in probs]
    room = sum(m for m, s in zip(n_meas, on) if s)
    sums = {k: np.zeros(max(1, room)) for k in SUMS}
    psum, psq = np.zeros(max(1, len(pa))), np.zeros(max(1, len(pa)))
    total = sum(on)
    res, its = np.zeros(max(1, total)), np.zeros(max(1, total), dtype=np.int32)
    det = np.zeros(G, dtype=np.int32)
    n_arr = np.ascontiguousarray(counts, dtype=np.int32)
    seed_arr = np.ascontiguousarray(keys, dtype=np.uint64)
    info = ScoreSamplesBatchInfo()
    rc = lib.score_refine_batch_leverage(handle.h, ptr(poses), ptr(lms), ptr(seed_arr, _u64p), int(first_sample), ptr(n_arr, _i32p),
                                         pair_ptr.ctypes.data_as(_i32p), ptr(pa, _i32p), ptr(pb, _i32p), float(rel_tol), int(max_iters),
                                         int(block_width), ptr(sums["lev_sum"]), ptr(sums["lev_sq"]), ptr(sums["red_sum"]),
                                         ptr(sums["red_sq"]), ptr(psum), ptr(psq), ptr(res), ptr(its, _i32p), ptr(det, _i32p),
                                         C.byref(info))
    if rc < 0:
        raise RuntimeError(f"score_refine_batch_leverage failed: {lib.score_last_error().decode()}")
    rec, cut, out = info.as_dict(), Cutter(), []
    for g in range(G):
        S, M, n_pairs = on[g], n_meas[g], len(ids[g])
        iterations, converged = steps_and_converged(cut(its, S))
        member = {k: (cut(sums[k], M) if S else np.zeros(M)) for k in SUMS}
        member.update({
            "pair_sum": cut(psum, n_pairs), "pair_sq": cut(psq, n_pairs), "residuals": cut(res, S), "iterations": iterations,
            "converged": converged, "determined": int(det[g]), "rc": 0 if np.all(converged) else 1,
            "info": dict(rec, samples=S, batches=-(-S // int(block_width))),
        })
        out.append(member)
    return rc, out, rec


def batch_range_variances(handle, points, pairs_per_member, rel_tol=1e-10, max_iters=4000, block_width=MAX_BLOCK_WIDTH):
    """``score_refine_batch_range_variances`` as it is, on a ``RefineBatchHandle``.  Returns (return code, one dict per
    member with the keys of ``LeverageHandle.range_variances`` except ``solutions`` -- ``rc`` is 0 iff all ITS columns
    converged, ``info`` the call's record with the member's own ``columns`` --, the call's info record)."""
    probs = handle.probs
    G = len(probs)
    if len(points) != G:
        raise ValueError("one point per member expected")
    lib = bind(handle.lib, LEVERAGE_BATCH)
    _, poses, lms = handle._flat_points(points)
    ids, pair_ptr, pa, pb = _flat_pairs(pairs_per_member, G)
    n = max(1, len(pa))
    var, dist, res, its = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    info = ScoreMarginalsBatchInfo()
    rc = lib.score_refine_batch_range_variances(handle.h, ptr(poses), ptr(lms), pair_ptr.ctypes.data_as(_i32p), ptr(pa, _i32p),
                                                ptr(pb, _i32p), float(rel_tol), int(max_iters), int(block_width), ptr(var), ptr(dist),
                                                ptr(res), ptr(its, _i32p), C.byref(info))
    if rc < 0:
        raise RuntimeError(f"score_refine_batch_range_variances failed: {lib.score_last_error().decode()}")
    rec, cut, out = info.as_dict(), Cutter(), []
    for n_pairs in map(len, ids):
        iterations, converged = steps_and_converged(cut(its, n_pairs))
        out.append({"rc": 0 if np.all(converged) else 1, "variances": cut(var, n_pairs), "distances": cut(dist, n_pairs),
                    "residuals": cut(res, n_pairs), "iterations": iterations, "converged": converged, "info": dict(rec, columns=n_pairs)})
    return rc, out, rec


def _failed(who, i, failed, total, what, max_iters):
    return _singular(f"{who}: graph {i}", failed, total, what, max_iters)


def group_leverage(handle, probs, points, names, indices, number, counts, seeds, first_sample=0, rel_tol=1e-10, max_iters=4000,
                   block_width=MAX_BLOCK_WIDTH):
    """The leverages of one group on its ``RefineBatchHandle``: ``names[k]`` the name pairs of member k (or None),
    ``indices[k]`` its graph's number in the caller's list (for messages).  Returns ``(Leverage, info)`` per member."""
    ids = [pair_ids(p, nm, f"range_leverage_batch: graph {i}") if nm is not None else None for p, nm, i in zip(probs, names, indices)]
    _, members, rec = handle.leverage(points, ids, counts, seeds, first_sample, rel_tol, max_iters, block_width)
    out = []
    for prob, point, nm, i, S, m in zip(probs, points, names, indices, counts, members):
        failed = int(np.count_nonzero(~m["converged"]))
        if failed:
            raise _failed("range_leverage_batch", i, failed, S, "draws", max_iters)
        out.append((Leverage(prob, point, m, S, nm), draw_info(rec, m, number, "device")))
    return out


def _members(datas, results, range_weights, loop_closure_weights, who):
    """(graphs, estimates, range weights, loop-closure weights, ``groups.grouped`` of (graph number, problem, point))."""
    datas, results = paired(datas, results)
    rws = per_graph(range_weights, len(datas), "range_weights")
    lws = per_graph(loop_closure_weights, len(datas), "loop_closure_weights")

    def member(i, data, res):
        prob, point = _problem_and_point(data, res, rws[i], lws[i])
        if prob.n == 0:
            raise ValueError("the graph has no unknowns")
        return prob, point

    return datas, results, rws, lws, grouped(datas, results, member, who=who)


def _ids_of(groups, names, who) -> dict:
    """{graph number: (C, 2) variable ids or None} of the graphs' name pairs; a bad pair raises with ``graph i:`` in front."""
    return {i: pair_ids(prob, names[i], f"{who}: graph {i}") if names[i] is not None else None
            for members in groups.values() for i, prob, _ in members}


def range_leverage_batch(datas, results, n_samples=256, seed=0, first_sample: int = 0, pairs=None, range_weights=None,
                         loop_closure_weights=None, rel_tol: float = 1e-10, max_iters: int = 4000,
                         block_width: int = MAX_BLOCK_WIDTH, engine: str = "device", lib_path: Optional[str] = None,
                         solver_settings: Optional[dict] = None, max_group: int = 64):
    """``range_leverage`` for many graphs at once: ``datas`` and ``results`` graph by graph, ``pairs`` None or a list with one
    entry per graph (None or a list of name pairs), ``range_weights`` / ``loop_closure_weights`` lists with one entry per
    graph.  ``n_samples``: an integer or one per graph.  ``seed``: a list with one seed per graph, or an integer -- graph i then
    draws from the stream of ``seed + i`` (``posterior_samples_batch``'s rule), so its draws are those of
    ``range_leverage(..., seed=seed + i)``.  The graphs are grouped by dimension, in chunks of at most ``max_group`` (the
    rule of ``score_amd/groups.py``); each group is one device handle and one ``score_refine_batch_leverage`` call
    (``engine="device"``) or ``range_leverage(engine="python")`` graph by graph.  Returns a list of ``(Leverage, info)`` in input
    order: per graph what ``range_leverage`` returns, plus ``group``, ``passes`` and ``determined`` on the device.  Draws that do
    not converge raise RuntimeError naming the first such graph."""
    _check_block(block_width, rel_tol, max_iters, engine)
    group_size(max_group)
    datas, results = list(datas), list(results)
    counts = per_graph(n_samples, len(datas), "n_samples", none=False, scalar=True)
    if datas:
        _check_draw_arguments(counts, first_sample, block_width, rel_tol, max_iters)
    counts = [int(s) for s in counts]
    seeds = _seeds_of(seed, len(datas))
    names = per_graph(pairs, len(datas), "pairs")
    datas, results, rws, lws, groups = _members(datas, results, range_weights, loop_closure_weights, "range_leverage")
    _ids_of(groups, names, "range_leverage_batch")  # (the pairs' errors before any work)
    out: list = [None] * len(datas)
    if engine == "python":
        for i, (data, res) in enumerate(zip(datas, results)):
            try:
                out[i] = range_leverage(data, res, counts[i], seeds[i], int(first_sample), names[i], rws[i], lws[i], rel_tol, max_iters,
                                        int(block_width), engine="python")
            except RuntimeError as e:
                raise RuntimeError(str(e).replace("range_leverage:", f"range_leverage_batch: graph {i}:")) from None
        return out

    def body(handle, number, idx, probs, points, extras):
        return group_leverage(handle, probs, points, [names[i] for i in idx], idx, number, [counts[i] for i in idx],
                              [seeds[i] for i in idx], int(first_sample), rel_tol, max_iters, int(block_width))

    return run_chunks(groups, max_group, out, body, True, lib_path, solver_settings)


def predicted_range_variances_batch(datas, results, pairs, range_weights=None, loop_closure_weights=None, rel_tol: float = 1e-10,
                                    max_iters: int = 4000, block_width: int = MAX_BLOCK_WIDTH, engine: str = "device",
                                    lib_path: Optional[str] = None, solver_settings: Optional[dict] = None, max_group: int = 64):
    """``predicted_range_variances`` for many graphs at once: ``pairs`` is one list of name pairs per graph; a graph may list
    none (its ``PredictedRanges`` is empty).  Grouped as ``range_leverage_batch``; each group is one device handle and one
    ``score_refine_batch_range_variances`` call (``engine="device"``) or the dense solve graph by graph (``engine="python"``).
    Returns a list of ``(PredictedRanges, info)`` in input order: per graph what ``predicted_range_variances`` returns, plus
    ``group`` and ``passes`` on the device.  A column that does not converge raises RuntimeError naming the first such
    graph."""
    _check_block(block_width, rel_tol, max_iters, engine)
    group_size(max_group)
    datas = list(datas)
    names = [[tuple(p) for p in nm] if nm is not None else [] for nm in per_graph(pairs, len(datas), "pairs")]
    datas, results, rws, lws, groups = _members(datas, results, range_weights, loop_closure_weights, "predicted_range_variances")
    ids_of = _ids_of(groups, names, "predicted_range_variances_batch")  # (the pairs' errors before any work)
    out: list = [None] * len(datas)

    def empty():
        return (PredictedRanges([], np.zeros(0), np.zeros(0)),
                {"pcg_iters": 0, "batches": 0, "setup_ms": 0.0, "solve_ms": 0.0, "iterations": np.zeros(0, dtype=np.int64),
                 "residuals": np.zeros(0), "engine": engine})

    if engine == "python":
        for i, (data, res) in enumerate(zip(datas, results)):
            if not names[i]:
                out[i] = empty()
                continue
            try:
                out[i] = predicted_range_variances(data, res, names[i], rws[i], lws[i], rel_tol, max_iters, int(block_width), engine="python")
            except RuntimeError as e:
                raise RuntimeError(str(e).replace("predicted_range_variances:", f"predicted_range_variances_batch: graph {i}:")) from None
        return out

    def body(handle, number, idx, probs, points, extras):
        _, members, rec = handle.range_variances(points, [ids_of[i] for i in idx], rel_tol, max_iters, int(block_width))
        got = []
        for i, m in zip(idx, members):
            failed = int(np.count_nonzero(~m["converged"]))
            if failed:
                raise _failed("predicted_range_variances_batch", i, failed, len(names[i]), "columns", max_iters)
            mine = dict(m, info={"batches": -(-len(names[i]) // int(block_width))})  # (the passes in which the graph had columns)
            got.append((PredictedRanges(names[i], m["distances"], m["variances"]), draw_info(rec, mine, number, engine, draws=False)))
        return got

    return run_chunks(groups, max_group, out, body, True, lib_path, solver_settings)


__all__ = ["range_leverage_batch", "predicted_range_variances_batch", "batch_leverage", "batch_range_variances", "group_leverage",
           "LEVERAGE_BATCH_SYMBOLS"]
