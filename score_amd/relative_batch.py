"""Predicted relative poses and their covariances for many graphs at once (include/score_relative_batch.h,
csrc/score_relative_batch.hpp): the Mahalanobis gates of a whole study.

``predicted_relative_poses`` takes one graph, builds one refinement handle and runs block solves whose launches are
latency-bound on a small world.  The question it answers is a study question -- across 64 generated worlds, which
place-recognition candidates pass the gate, and how well does it separate planted false matches from true ones? -- so
``predicted_relative_poses_batch`` hands the graphs to the device as groups, by the rule of ``score_amd/groups.py``: one
union vector carries one column of every member, dp columns per listed pair.

``RefineBatchHandle.relative_covariances`` is the raw call on a kept group handle, so a study refines and gates with one
create; ``refine_estimate_batch(..., relative=pairs_per_graph)`` does exactly that.  ``engine="python"`` is
``predicted_relative_poses``' python engine graph by graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import RELATIVE_BATCH, Cutter, ScoreMarginalsBatchInfo, bind, ptr, steps_and_converged
from .groups import group_size, per_graph, run_chunks
from .leverage import _check_block
from .leverage_batch import _failed, _flat_pairs, _members
from .marginals import MAX_BLOCK_WIDTH
from .refine import unknown_sizes
from .relative import PredictedRelativePoses, _pose_pair_ids, predicted_relative_poses
from .samples_batch import draw_info
from .solver import _i32p

# the symbols include/score_relative_batch.h declares
RELATIVE_BATCH_SYMBOLS = list(RELATIVE_BATCH)


def batch_relative_covariances(handle, points, pairs_per_member, rel_tol=1e-10, max_iters=4000, block_width=MAX_BLOCK_WIDTH):
    """``score_refine_batch_relative_covariances`` as it is, on a ``RefineBatchHandle``: ``points`` in the problems' own form,
    ``pairs_per_member`` the member-local pose id pairs of every member (None or an empty list: none).  Returns (return code,
    one dict per member with the keys of ``RelativeHandle.relative_covariances`` except ``solutions`` -- ``rc`` is 0 iff all
    ITS columns converged, ``info`` the call's record with the member's own ``columns`` --, the call's info record)."""
    probs = handle.probs
    G = len(probs)
    if len(points) != G:
        raise ValueError("one point per member expected")
    lib = bind(handle.lib, RELATIVE_BATCH)
    _, poses, lms = handle._flat_points(points)
    ids, pair_ptr, pa, pb = _flat_pairs(pairs_per_member, G)
    d, dp = unknown_sizes(probs[0])
    n = max(1, len(pa))
    rot, trans, cov = np.zeros(n * d * d), np.zeros(n * d), np.zeros(n * dp * dp)
    res, its = np.zeros(n * dp), np.zeros(n * dp, dtype=np.int32)
    info = ScoreMarginalsBatchInfo()
    rc = lib.score_refine_batch_relative_covariances(handle.h, ptr(poses), ptr(lms), pair_ptr.ctypes.data_as(_i32p), ptr(pa, _i32p),
                                                     ptr(pb, _i32p), float(rel_tol), int(max_iters), int(block_width), ptr(rot),
                                                     ptr(trans), ptr(cov), ptr(res), ptr(its, _i32p), C.byref(info))
    if rc < 0:
        raise RuntimeError(f"score_refine_batch_relative_covariances failed: {lib.score_last_error().decode()}")
    rec, cut, out = info.as_dict(), Cutter(), []
    for c in map(len, ids):
        iterations, converged = steps_and_converged(cut(its, c * dp, (c, dp)))
        out.append({"rc": 0 if np.all(converged) else 1, "rotations": cut(rot, c * d * d, (c, d, d)),
                    "translations": cut(trans, c * d, (c, d)), "covariances": cut(cov, c * dp * dp, (c, dp, dp)),
                    "residuals": cut(res, c * dp, (c, dp)), "iterations": iterations, "converged": converged,
                    "info": dict(rec, columns=c * dp)})
    return rc, out, rec


def group_relative(handle, points, names, ids, indices, number, rel_tol=1e-10, max_iters=4000, block_width=MAX_BLOCK_WIDTH):
    """The predictions of one group on its ``RefineBatchHandle``: ``names[k]`` the name pairs of member k, ``ids[k]`` their
    pose ids, ``indices[k]`` its graph's number in the caller's list (for messages).  Returns ``(PredictedRelativePoses,
    info)`` per member; a member that lists none gets an empty one."""
    dp = unknown_sizes(handle.probs[0])[1]
    _, members, rec = handle.relative_covariances(points, ids, rel_tol, max_iters, int(block_width))
    out = []
    for i, nm, m in zip(indices, names, members):
        failed = int(np.count_nonzero(~m["converged"]))
        if failed:
            raise _failed("predicted_relative_poses_batch", i, failed, len(nm) * dp, "columns", max_iters)
        mine = dict(m, info={"batches": -(-len(nm) * dp // int(block_width))})  # (the passes in which the graph had columns)
        info = draw_info(rec, mine, number, "device", draws=False)
        cov = m["covariances"]
        covT = np.swapaxes(cov, 1, 2)
        info["asymmetry"] = float(np.max(np.abs(cov - covT))) if len(nm) else 0.0
        out.append((PredictedRelativePoses(nm, m["rotations"], m["translations"], 0.5 * (cov + covT)), info))
    return out


def _empty(d, dp, engine):
    """What a graph without pairs gets (``predicted_relative_poses`` itself refuses an empty list)."""
    return (PredictedRelativePoses([], np.zeros((0, d, d)), np.zeros((0, d)), np.zeros((0, dp, dp))),
            {"pcg_iters": 0, "batches": 0, "setup_ms": 0.0, "solve_ms": 0.0, "iterations": np.zeros((0, dp), dtype=np.int64),
             "residuals": np.zeros((0, dp)), "asymmetry": 0.0, "engine": engine})


def predicted_relative_poses_batch(datas, results, pairs, range_weights=None, loop_closure_weights=None, rel_tol: float = 1e-10,
                                   max_iters: int = 4000, block_width: int = MAX_BLOCK_WIDTH, engine: str = "device",
                                   lib_path: Optional[str] = None, solver_settings: Optional[dict] = None, max_group: int = 64):
    """``predicted_relative_poses`` for many graphs at once: ``pairs`` is one list of pose name pairs per graph; a graph may
    list none (its ``PredictedRelativePoses`` is empty).  Grouped as ``predicted_range_variances_batch``; each group is one
    device handle and one ``score_refine_batch_relative_covariances`` call (``engine="device"``) or the dense solve graph by
    graph (``engine="python"``).  Returns a list of ``(PredictedRelativePoses, info)`` in input order: per graph what
    ``predicted_relative_poses`` returns (the covariance symmetrised, ``asymmetry``, ``residuals``, ``iterations``,
    ``batches``, ``engine``), plus ``group`` and ``passes`` on the device.  A column that does not converge raises
    RuntimeError naming the first such graph."""
    _check_block(block_width, rel_tol, max_iters, engine)
    group_size(max_group)
    datas = list(datas)
    names = [[tuple(p) for p in nm] if nm is not None else [] for nm in per_graph(pairs, len(datas), "pairs")]
    datas, results, rws, lws, groups = _members(datas, results, range_weights, loop_closure_weights, "predicted_relative_poses")
    # (the pairs' errors before any work)
    ids_of = {i: _pose_pair_ids(prob, names[i], f"predicted_relative_poses_batch: graph {i}")
              for members in groups.values() for i, prob, _ in members}
    out: list = [None] * len(datas)
    if engine == "python":
        for i, (data, res) in enumerate(zip(datas, results)):
            if not names[i]:
                out[i] = _empty(data.dimension, 3 if data.dimension == 2 else 6, engine)
                continue
            try:
                out[i] = predicted_relative_poses(data, res, names[i], rws[i], lws[i], rel_tol, max_iters, int(block_width), engine="python")
            except RuntimeError as e:
                raise RuntimeError(str(e).replace("predicted_relative_poses:", f"predicted_relative_poses_batch: graph {i}:")) from None
        return out

    def body(handle, number, idx, probs, points, extras):
        return group_relative(handle, points, [names[i] for i in idx], [ids_of[i] for i in idx], idx, number, rel_tol, max_iters,
                              int(block_width))

    return run_chunks(groups, max_group, out, body, True, lib_path, solver_settings)


__all__ = ["predicted_relative_poses_batch", "batch_relative_covariances", "group_relative", "RELATIVE_BATCH_SYMBOLS"]
