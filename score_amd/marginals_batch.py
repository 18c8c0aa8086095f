"""Marginal covariances of many graphs at once (include/score_marginals_batch.h, csrc/score_marginals_batch.hpp).

``marginal_covariances`` takes one graph, builds one refinement handle and runs a block PCG whose launches are latency-bound
on a small world.  ``marginal_covariances_batch`` hands the graphs to the device as groups, by the rule of
``score_amd/groups.py``: the group handle's union matrix H = J'J is block diagonal, so one union vector carries one unit
column of every member, and a block of up to 16 union vectors advances 16 columns of all members per pass over the union
matrix (``score_refine_batch_marginals``).  Every (member, column) pair has its own alpha, beta, stopping gate and verdict: a
member's result is what ``marginal_covariances`` computes on it alone, up to the rounding of the two iterations.

``RefineBatchHandle.marginals`` is the raw call on a kept group handle, so a study refines and takes covariances with one
create; ``refine_estimate_batch(..., marginals=True)`` does exactly that.  ``engine="python"`` is the dense inverse of
``marginals._python_columns`` member by member.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import MARGINALS_BATCH, Cutter, ScoreMarginalsBatchInfo, bind, ptr, steps_and_converged
from .groups import FollowUp, grouped, naming, paired, per_graph, run_chunks
from .marginals import MAX_BLOCK_WIDTH, _member_result, _problem_and_point, _python_columns, _select, check_block_solve, n_columns
from .solver import _i32p

# the symbols include/score_marginals_batch.h declares
MARGINALS_BATCH_SYMBOLS = list(MARGINALS_BATCH)


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, MARGINALS_BATCH)


def _flat_ids(ids_per_member):
    """The members' variable ids as the group calls take them: (ids per member, var_ptr, all ids in a row)."""
    ids = [np.asarray(v, dtype=np.int32).ravel() for v in ids_per_member]
    var_ptr = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(v) for v in ids])]), dtype=np.int32)
    return ids, var_ptr, np.ascontiguousarray(np.concatenate(ids + [np.zeros(0, np.int32)]), dtype=np.int32)


def batch_columns(handle, points, ids_per_member, rel_tol=1e-10, max_iters=4000, block_width=MAX_BLOCK_WIDTH):
    """``score_refine_batch_marginals`` as it is, on a ``RefineBatchHandle``: ``points`` in the problems' own form,
    ``ids_per_member`` the member-local variable ids of every member (an empty list: none).  Returns (return code, per member
    ``(A, residuals, steps, converged)`` -- A is C_g x C_g, column c is x_c on the selected rows, not symmetrised --, the
    call's info record)."""
    probs = handle.probs
    if len(points) != len(probs) or len(ids_per_member) != len(probs):
        raise ValueError("one point and one list of variables per member expected")
    lib = _bind(handle.lib)
    _, poses, lms = handle._flat_points(points)
    ids, var_ptr, flat = _flat_ids(ids_per_member)
    ncol = [n_columns(prob, v) for prob, v in zip(probs, ids)]
    joint = np.zeros(max(1, sum(c * c for c in ncol)))
    res = np.zeros(max(1, sum(ncol)))
    its = np.zeros(max(1, sum(ncol)), dtype=np.int32)
    info = ScoreMarginalsBatchInfo()
    rc = lib.score_refine_batch_marginals(handle.h, ptr(poses), ptr(lms), ptr(var_ptr, _i32p), ptr(flat, _i32p), float(rel_tol),
                                          int(max_iters), int(block_width), ptr(joint), ptr(res), ptr(its, _i32p), C.byref(info))
    if rc < 0:
        raise RuntimeError(f"score_refine_batch_marginals failed: {lib.score_last_error().decode()}")
    cut, out = Cutter(), []
    for c in ncol:
        steps, converged = steps_and_converged(cut(its, c))
        out.append((cut(joint, c * c, (c, c)), cut(res, c), steps, converged))
    return rc, out, info.as_dict()


def group_marginals(handle, probs, points, selections, indices, number, rel_tol=1e-10, max_iters=4000,
                    block_width=MAX_BLOCK_WIDTH, engine="device", joint=False):
    """The covariances of one group: ``selections[k]`` is ``marginals._select`` of member k, ``indices[k]`` its graph's number
    in the caller's list (for messages), ``handle`` the group's ``RefineBatchHandle`` (None with ``engine="python"``).
    Returns ``(cov, info)`` per member."""
    if engine == "python":
        cols = []
        for prob, point, (_, _, _, c) in zip(probs, points, selections):
            A, res = _python_columns(prob, point, c)
            cols.append((A, res, np.zeros(len(c), dtype=np.int64), np.isfinite(res)))
        rec = {"pcg_iters": 0, "passes": 0, "setup_ms": 0.0, "solve_ms": 0.0}
    else:
        _, cols, rec = handle.marginals(points, [sel[1] for sel in selections], rel_tol, max_iters, block_width)
    out = []
    for (names, _, size, c), (A, res, steps, converged), i in zip(selections, cols, indices):
        mine = dict(rec, batches=0 if engine == "python" else -(-len(c) // int(block_width)))
        cov, info = _member_result("marginal_covariances_batch", f"graph {i}", names, size, A, res, steps, converged, mine, engine,
                                   joint, max_iters)
        info["group"], info["passes"] = number, int(rec["passes"])
        out.append((cov, info))
    return out


def marginals_follow_up(marginals, count: int) -> FollowUp:
    """The ``marginals=`` keyword of the two refine front ends (True, or ``variables`` as ``marginal_covariances_batch`` takes
    them): ``info["marginals"]`` is that call's ``(cov, info)`` at the refined points, on the group's handle."""
    wanted = per_graph(None if marginals is True else marginals, count, "variables")

    def prepare(i, prob):
        with naming(i):
            return _select(prob, wanted[i])

    def run(handle, number, idx, probs, points, costs, selections):
        return group_marginals(handle, probs, points, selections, idx, number, engine="python" if handle is None else "device")

    return FollowUp("marginals", run, prepare)


def marginal_covariances_batch(datas, results, variables=None, joint: bool = False, range_weights=None, loop_closure_weights=None,
                               rel_tol: float = 1e-10, max_iters: int = 4000, block_width: int = MAX_BLOCK_WIDTH,
                               engine: str = "device", lib_path: Optional[str] = None, solver_settings: Optional[dict] = None,
                               max_group: int = 64):
    """``marginal_covariances`` for many graphs at once: ``datas`` and ``results`` graph by graph, ``variables`` None or a list
    with one entry per graph (None: that graph's default, every landmark and the last pose of every chain; else a list of
    names), ``range_weights`` / ``loop_closure_weights`` lists with one entry per graph.  The graphs are grouped by dimension,
    in chunks of at most ``max_group`` (the rule of ``score_amd/groups.py``); each group is one device handle and one
    ``score_refine_batch_marginals`` call (``engine="device"``) or the dense inverse graph by graph (``engine="python"``).
    Returns a list of ``(dict name -> k x k ndarray, info)`` in input order: per graph what ``marginal_covariances`` returns,
    plus ``group`` (the group's number) and ``passes`` (passes of the group's call; ``batches`` counts those in which the
    graph itself had columns; ``pcg_iters``, ``setup_ms`` and ``solve_ms`` are the group's).
    ``block_width``: 1..16 columns of every member advance together.  The single call's ValueErrors are raised with
    ``graph i:`` in front; a column that does not converge raises RuntimeError naming the graph and the variable."""
    if engine not in ("device", "python"):
        raise ValueError("engine must be 'device' or 'python'")
    check_block_solve(block_width, rel_tol, max_iters)
    datas, results = paired(datas, results, max_group)
    rws = per_graph(range_weights, len(datas), "range_weights")
    lws = per_graph(loop_closure_weights, len(datas), "loop_closure_weights")
    wanted = per_graph(variables, len(datas), "variables")

    def member(i, data, res):
        prob, point = _problem_and_point(data, res, rws[i], lws[i])
        return prob, point, _select(prob, wanted[i])

    def body(handle, number, idx, probs, points, extras):
        return group_marginals(handle, probs, points, extras[0], idx, number, rel_tol, max_iters, int(block_width), engine, joint)

    return run_chunks(grouped(datas, results, member), max_group, [None] * len(datas), body, engine == "device", lib_path, solver_settings)


__all__ = ["marginal_covariances_batch", "batch_columns", "group_marginals", "MARGINALS_BATCH_SYMBOLS"]
