"""Greedy selection of candidate ranges for many graphs at once (include/score_select_batch.h, csrc/score_select_batch.hpp).

``select_ranges`` takes one graph, builds one refinement handle, runs ceil(C / 16) latency-bound block solves and one
factorisation in a single workgroup.  "k more ranges out of these C candidates -- which k?" is what a study asks of EVERY
world, so ``select_ranges_batch`` hands the graphs to the device as groups, by the rule of ``score_amd/groups.py``: one union
vector carries one candidate's column of every member, one launch forms the cross terms of a pass for all members, one launch
symmetrises all matrices and one runs the members' factorisations side by side, a workgroup each.

``RefineBatchHandle.select_ranges`` is the raw call on a kept group handle, so a study refines and selects with one create;
``refine_estimate_batch(..., select=...)`` does exactly that.  ``engine="python"`` is ``select_ranges``' python engine graph by
graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import SELECT_BATCH, Cutter, ScoreSelectBatchInfo, bind, ptr, steps_and_converged
from .groups import group_size, per_graph, run_chunks
from .leverage import _check_block
from .leverage_batch import _flat_pairs, _ids_of, _members
from .marginals import MAX_BLOCK_WIDTH
from .selection import Selection, _check_selection, select_ranges
from .solver import _i32p

# the symbols include/score_select_batch.h declares
SELECT_BATCH_SYMBOLS = list(SELECT_BATCH)


def batch_select_ranges(handle, points, pairs_per_member, precisions_per_member, k, min_gain=0.0, rel_tol=1e-10, max_iters=4000,
                        block_width=MAX_BLOCK_WIDTH, with_matrix=False):
    """``score_refine_batch_select_ranges`` as it is, on a ``RefineBatchHandle``: ``points`` in the problems' own form,
    ``pairs_per_member`` the member-local variable id pairs of every member (None or an empty list: none),
    ``precisions_per_member`` one array per member (None where it lists none), ``k`` one integer per member (0 where it lists
    none) or one for all that list any.  Returns (return code, one dict per member, the call's info record).  A member's dict
    has the keys ``SelectionHandle.select_ranges`` returns -- ``rc`` is 0 iff all ITS columns converged, ``matrix`` its own
    C_g x C_g block, ``info`` the call's record with the member's own ``candidates``, ``picked``, ``excluded``, ``total_gain``
    and ``solve["columns"]`` -- plus ``picked`` and ``total_gain``."""
    probs = handle.probs
    G = len(probs)
    if len(points) != G:
        raise ValueError("one point per member expected")
    lib = bind(handle.lib, SELECT_BATCH)
    _, poses, lms = handle._flat_points(points)
    ids, pair_ptr, pa, pb = _flat_pairs(pairs_per_member, G)
    counts = [len(i) for i in ids]
    if len(precisions_per_member) != G:
        raise ValueError(f"one array of precisions per member expected ({G}), got {len(precisions_per_member)}")
    w = np.ascontiguousarray(np.concatenate([np.zeros(0) if p is None else np.asarray(p, dtype=np.float64).ravel()
                                             for p in precisions_per_member] + [np.zeros(0)]))
    if len(w) != len(pa):
        raise ValueError(f"one precision per listed pair expected ({len(pa)}), got {len(w)}")
    # (one k for all: a member without candidates has 0; a list goes to the library as it is)
    ks = [int(v) if (c or np.ndim(k)) else 0 for v, c in zip(per_graph(k, G, "k", none=False, scalar=True), counts)]
    k_arr = np.ascontiguousarray(ks, dtype=np.int32)
    room = [max(v, 0) for v in ks]  # (a negative k is the library's error to report)
    n, picks = max(1, len(pa)), max(1, sum(room))
    order = np.full(picks, -7, dtype=np.int32)
    gains, pick = np.zeros(picks), np.zeros(picks)
    picked, totals = np.zeros(G, dtype=np.int32), np.zeros(G)
    var, dist, rem, res, its = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    mat = np.zeros(max(1, sum(c * c for c in counts))) if with_matrix else None
    info = ScoreSelectBatchInfo()
    rc = lib.score_refine_batch_select_ranges(handle.h, ptr(poses), ptr(lms), pair_ptr.ctypes.data_as(_i32p), ptr(pa, _i32p),
                                              ptr(pb, _i32p), ptr(w), k_arr.ctypes.data_as(_i32p), float(min_gain), float(rel_tol),
                                              int(max_iters), int(block_width), ptr(order, _i32p), ptr(gains), ptr(pick),
                                              ptr(picked, _i32p), ptr(totals), ptr(var), ptr(dist), ptr(rem), ptr(res),
                                              ptr(its, _i32p), ptr(mat), C.byref(info))
    if rc < 0:
        raise RuntimeError(f"score_refine_batch_select_ranges failed: {lib.score_last_error().decode()}")
    rec, cut, out = info.as_dict(), Cutter(), []
    for g, (c, kk) in enumerate(zip(counts, room)):
        iterations, converged = steps_and_converged(cut(its, c))
        mine = dict(rec, candidates=c, picked=int(picked[g]), excluded=int(np.count_nonzero(~converged)), total_gain=float(totals[g]),
                    solve=dict(rec["solve"], columns=c))
        out.append({"rc": 0 if np.all(converged) else 1, "order": cut(order, kk), "gains": cut(gains, kk), "pick_variances": cut(pick, kk),
                    "variances": cut(var, c), "distances": cut(dist, c), "remaining": cut(rem, c), "residuals": cut(res, c),
                    "iterations": iterations, "converged": converged, "matrix": cut(mat, c * c, (c, c)), "picked": int(picked[g]),
                    "total_gain": float(totals[g]), "info": mine})
    return rc, out, rec


def _empty(engine):
    """What a graph without candidates gets (``select_ranges`` itself refuses an empty list)."""
    none = np.zeros(0)
    return (Selection([], np.zeros(0, dtype=np.int64), none, none, none, none, none, np.zeros(0, dtype=np.int64)),
            {"pcg_iters": 0, "batches": 0, "setup_ms": 0.0, "solve_ms": 0.0, "cross_ms": 0.0, "greedy_ms": 0.0,
             "iterations": np.zeros(0, dtype=np.int64), "residuals": none, "asymmetry": 0.0, "engine": engine})


def selection_arguments(names, k, precision, min_gain, who):
    """(k per graph, precisions per graph) of ``select_ranges_batch``'s arguments, checked: ``k`` one value or one per graph,
    ``precision`` one value, or one entry per graph that is one value or one per candidate.  A graph without candidates keeps
    k = 0 and no precisions.  Errors carry ``graph i:`` in front."""
    count = len(names)
    ks = per_graph(k, count, "k", none=False, scalar=True)
    one = isinstance(precision, (int, float, np.number)) or (isinstance(precision, np.ndarray) and precision.ndim == 0)
    ws = [precision] * count if one else per_graph(list(precision), count, "precision", none=False)  # (the entries may differ in shape)
    out_k, out_w = [], []
    for i, nm in enumerate(names):
        if not nm:
            out_k.append(0)
            out_w.append(None)
            continue
        w = np.asarray(ws[i], dtype=np.float64)
        w = np.full(len(nm), float(w)) if w.ndim == 0 else w.copy()
        _check_selection(len(nm), ks[i], min_gain, w, f"{who}: graph {i}")
        out_k.append(int(ks[i]))
        out_w.append(w)
    if not min_gain >= 0:
        raise ValueError(f"{who}: min_gain must be >= 0")
    return out_k, out_w


def group_selection(handle, points, names, ids, precisions, ks, number, min_gain=0.0, rel_tol=1e-10, max_iters=4000,
                    block_width=MAX_BLOCK_WIDTH):
    """The selections of one group on its ``RefineBatchHandle``: ``names[m]`` the name pairs of member m, ``ids[m]`` their
    variable ids, ``precisions[m]`` and ``ks[m]`` as ``selection_arguments`` returns them.  Returns ``(Selection, info)`` per
    member; a member that lists none gets an empty one.  ``info`` is ``select_ranges``' plus ``group`` and ``passes``;
    ``asymmetry``, the times and ``pcg_iters`` are the group call's."""
    _, members, rec = handle.select_ranges(points, ids, precisions, ks, min_gain, rel_tol, max_iters, int(block_width))
    out = []
    for nm, m in zip(names, members):
        if not nm:
            out.append(_empty("device"))
            out[-1][1].update(group=number, passes=int(rec["solve"]["passes"]))
            continue
        info = {"pcg_iters": int(rec["solve"]["pcg_iters"]), "batches": -(-len(nm) // int(block_width)),
                "setup_ms": float(rec["solve"]["setup_ms"]), "solve_ms": float(rec["solve"]["solve_ms"]),
                "cross_ms": float(rec["cross_ms"]), "greedy_ms": float(rec["greedy_ms"]), "iterations": m["iterations"],
                "residuals": m["residuals"], "asymmetry": float(rec["asymmetry"]), "engine": "device", "group": number,
                "passes": int(rec["solve"]["passes"])}
        p = m["picked"]
        out.append((Selection(nm, m["order"][:p], m["gains"][:p], m["pick_variances"][:p], m["variances"], m["distances"],
                              m["remaining"], np.flatnonzero(~m["converged"])), info))
    return out


def _python_selection(data, res, names, k, w, min_gain, rw, lw, i, who):
    if not names:
        return _empty("python")
    try:
        return select_ranges(data, res, names, k, precision=w, min_gain=min_gain, range_weights=rw, loop_closure_weights=lw, engine="python")
    except RuntimeError as e:
        raise RuntimeError(str(e).replace("select_ranges:", f"{who}: graph {i}:")) from None


def select_ranges_batch(datas, results, pairs, k, precision=1.0, min_gain: float = 0.0, range_weights=None, loop_closure_weights=None,
                        rel_tol: float = 1e-10, max_iters: int = 4000, block_width: int = MAX_BLOCK_WIDTH, engine: str = "device",
                        lib_path: Optional[str] = None, solver_settings: Optional[dict] = None, max_group: int = 64):
    """``select_ranges`` for many graphs at once: ``pairs`` is one list of name pairs per graph; a graph may list none (its
    ``Selection`` is empty).  ``k``: one value or one per graph; ``precision``: one value, or one entry per graph, each one value
    or one per candidate of that graph; ``min_gain`` holds for all.  Grouped as ``predicted_range_variances_batch``; each group
    is one device handle and one ``score_refine_batch_select_ranges`` call (``engine="device"``) or
    ``select_ranges(engine="python")`` graph by graph.  Returns a list of ``(Selection, info)`` in input order: per graph what
    ``select_ranges`` returns, plus ``group`` and ``passes`` on the device (``asymmetry``, ``pcg_iters`` and the times are the
    group call's).  A column that does not converge excludes its candidate in its graph.  Argument errors carry ``graph i:``
    in front and come before any device work."""
    who = "select_ranges_batch"
    _check_block(block_width, rel_tol, max_iters, engine)
    group_size(max_group)
    datas = list(datas)
    names = [[tuple(p) for p in nm] if nm is not None else [] for nm in per_graph(pairs, len(datas), "pairs")]
    datas, results, rws, lws, groups = _members(datas, results, range_weights, loop_closure_weights, "select_ranges")
    ids_of = _ids_of(groups, names, who)  # (the pairs' errors before any work)
    ks, ws = selection_arguments(names, k, precision, min_gain, who)
    out: list = [None] * len(datas)
    if engine == "python":
        for i, (data, res) in enumerate(zip(datas, results)):
            out[i] = _python_selection(data, res, names[i], ks[i], ws[i], float(min_gain), rws[i], lws[i], i, who)
        return out

    def body(handle, number, idx, probs, points, extras):
        return group_selection(handle, points, [names[i] for i in idx], [ids_of[i] for i in idx], [ws[i] for i in idx],
                               [ks[i] for i in idx], number, float(min_gain), rel_tol, max_iters, int(block_width))

    return run_chunks(groups, max_group, out, body, True, lib_path, solver_settings)


__all__ = ["select_ranges_batch", "batch_select_ranges", "group_selection", "selection_arguments", "SELECT_BATCH_SYMBOLS"]
