"""Local refinement of many graphs in lock-step (include/score_refine_batch.h, csrc/score_gn_batch.hpp).

``refine_estimate`` takes one graph, builds one handle and meets the device four or five times per Levenberg-Marquardt
iteration.  A Monte-Carlo study refines dozens of small worlds; ``refine_estimate_batch`` hands them to the device as groups:
one union problem per group (block-diagonal J'J on one linear-mode pattern), one gather / factorisation / conjugate-gradient
solve / trial / cost per ROUND for every member that needs one, and a controller that keeps one state per member.  Members
never influence one another: every member takes exactly the decisions ``refine._lm_loop`` takes on it alone.

``engine="python"`` is the same lock-step controller in Python around ``refine._Problem`` / ``_Problem3D`` with SciPy's sparse
LU: the step rule is ``refine._Member``'s, the one ``refine._lm_loop`` drives (the library's: ``LmState`` and ``lm_*`` of
csrc/score_refine_rule.hpp under ``gb_start`` / ``gb_round``).  It is the twin the tests compare with: it only reorders
independent work, so its results equal ``refine_estimate(engine="python", linear_solver="scipy")`` member by member, bit for bit.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from .bindings import CURVATURE_BATCH, LEVERAGE_BATCH, REFINE_BATCH, REFINE_ROBUST_BATCH, ScoreRefineRobustInfo, ScoreRefineRobustSettings, bind, ptr
from .groups import FollowUp, follow, grouped, paired, per_graph, run_chunks
from .native import ScoreGraph, score_graph_struct
from .refine import (GRADIENT, SOLVE, _as_results, _attempt, _gradient, _Handle, _Member, _native_info, _point_arrays, _point_from,
                     _problem_and_point as _problem_of, refine_estimate)
from .robust import n_loop_closures_of
from .solver import ScoreRefineInfo

# the symbols include/score_refine_batch.h declares
REFINE_BATCH_SYMBOLS = list(REFINE_BATCH)


class _LockStep:
    """The members' points, runs (``_Member``) and normal equations.  ``tol`` / ``cap``: the limits of a member's run."""

    def __init__(self, probs, points):
        self.probs, self.u = probs, list(points)
        self.S, self.lin, self.grad, self.H = ([None] * len(probs) for _ in range(4))

    def _gradient(self, g: int, tol: float, cap: int) -> None:
        res, J = self.lin[g]  # of the current point
        self.grad[g], gnorm = _gradient(res, J)
        self.S[g].after_gradient(gnorm, tol, cap)
        self.H[g] = (J.T @ J).tocsc() if self.S[g].phase == SOLVE else None

    def start(self, g: int, tol: float, cap: int) -> None:
        """Member ``g`` enters a run at its current point, under the precisions as they stand."""
        self.lin[g] = self.probs[g].residuals(self.u[g], jac=True)
        res = self.lin[g][0]
        self.S[g] = _Member(float(res @ res), cap)
        if self.S[g].phase == GRADIENT:
            self._gradient(g, tol, cap)

    def round(self, tol, cap) -> bool:
        """Every member in phase SOLVE gets one damped solve, one trial point and one cost (limits ``tol(g)``, ``cap(g)``); then
        each decides for itself.  False: no member is in phase SOLVE (nothing was done)."""
        live = [g for g, s in enumerate(self.S) if s.phase == SOLVE]
        for g in live:
            ok, un, fn = _attempt(self.probs[g], self.u[g], self.H[g], self.grad[g], self.S[g].lam)
            if self.S[g].after_solve(ok, 0, fn, cap(g)):
                self.u[g] = un
                if self.S[g].phase == GRADIENT:
                    self.lin[g] = self.probs[g].residuals(un, jac=True)
                    self._gradient(g, tol(g), cap(g))
        return bool(live)


def _python_lock_step(probs, points, max_iters: int, tol: float):
    """The lock-step controller over ``probs`` from ``points``: returns (points, members, rounds)."""
    L = _LockStep(probs, points)
    for g in range(len(probs)):
        L.start(g, tol, max_iters)
    rounds = 0
    while L.round(lambda g: tol, lambda g: max_iters):
        rounds += 1
    return L.u, L.S, rounds


def _bind(lib):
    return bind(lib, REFINE_BATCH)


def member_counts(probs):
    """(ranges, loop closures) of every member."""
    return [len(p.ra) for p in probs], [n_loop_closures_of(p.a) for p in probs]


class RefineBatchHandle(_Handle):
    """A group handle (``score_refine_batch_create``) over ``probs`` (all of one dimension, every one with unknowns); ``run``
    takes and returns points in the problems' own form (``_Problem``: packed unknowns; ``_Problem3D``: (R, t, lm))."""

    headers = (REFINE_BATCH, LEVERAGE_BATCH, CURVATURE_BATCH)
    destroy = "score_refine_batch_destroy"

    def __init__(self, probs: Sequence, lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
        self.probs = list(probs)
        super().__init__(lib_path, solver_settings)

    def _create(self, st) -> None:
        graphs = (ScoreGraph * len(self.probs))(*[score_graph_struct(p.a) for p in self.probs])
        if self.lib.score_refine_batch_create(graphs, len(self.probs), C.byref(st), C.byref(self.h)) != 0:
            raise RuntimeError(f"score_refine_batch_create failed: {self.lib.score_last_error().decode()}")

    def _flat_points(self, points):
        """The members' points as the group calls take them: (the C arrays member by member, all poses, all landmarks)."""
        if len(points) != len(self.probs):
            raise ValueError("one point per member expected")
        arrays = [_point_arrays(prob, x) for prob, x in zip(self.probs, points)]
        poses = np.ascontiguousarray(np.concatenate([a[0].ravel() for a in arrays]))
        lms = np.ascontiguousarray(np.concatenate([a[1].ravel() for a in arrays]))
        return arrays, poses, lms

    def _points_from(self, arrays, poses, lms):
        """The way back: the members' points out of flat arrays laid out as ``_flat_points`` lays out ``arrays``."""
        out, p0, l0 = [], 0, 0
        for prob, (pa, la) in zip(self.probs, arrays):
            out.append(_point_from(prob, poses[p0 : p0 + pa.size].reshape(pa.shape), lms[l0 : l0 + la.size].reshape(la.shape)))
            p0 += pa.size
            l0 += la.size
        return out

    def _per_member(self, flat, counts):
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return [flat[offs[g] : offs[g + 1]].copy() for g in range(len(counts))]

    def run(self, points, max_iters: int = 50, tol: float = 1e-10):
        """``score_refine_batch_run``: (points, info dicts), member by member."""
        arrays, poses_in, lms_in = self._flat_points(points)
        poses_out, lms_out = np.empty_like(poses_in), np.empty(max(1, lms_in.size))
        infos = (ScoreRefineInfo * len(self.probs))()
        rc = self.lib.score_refine_batch_run(self.h, ptr(poses_in), ptr(lms_in), int(max_iters), float(tol), ptr(poses_out),
                                             ptr(lms_out), infos)
        if rc != 0:
            raise RuntimeError(f"score_refine_batch_run failed: {self.lib.score_last_error().decode()}")
        return self._points_from(arrays, poses_out, lms_out), [infos[i].as_dict() for i in range(len(self.probs))]

    def marginals(self, points, ids_per_member, rel_tol: float = 1e-10, max_iters: int = 4000, block_width: int = 16):
        """``score_refine_batch_marginals`` at ``points`` (include/score_marginals_batch.h): ``ids_per_member`` lists the
        member-local variable ids of every member (an empty list: none).  Returns (return code, per member
        ``(A, residuals, steps, converged)``, the call's info record); the handle is left as it was found."""
        from .marginals_batch import batch_columns

        return batch_columns(self, points, ids_per_member, rel_tol, max_iters, block_width)

    def spectrum(self, points, k, rel_tol: float = 1e-9, max_iters: int = 200, shift: float = 1e-8):
        """``score_refine_batch_spectrum`` at ``points`` (include/score_spectrum_batch.h): the ``k`` lowest eigenpairs of
        every member's H = J'J.  Returns (return code, per member ``(values, vectors k x n_g, residuals, iterations,
        converged, h_max)``, the call's info record); the handle is left as it was found."""
        from .spectrum_batch import batch_spectrum

        return batch_spectrum(self, points, k, rel_tol, max_iters, shift)

    def curvature(self, points, k, rel_tol: float = 1e-9, max_iters: int = 200, shift: float = 1e-8):
        """``score_refine_batch_curvature`` at ``points`` (include/score_curvature_batch.h): the ``k`` lowest eigenpairs of
        every member's E, half the Hessian of its cost.  Returns (return code, per member ``(values, vectors k x n_g,
        residuals, v'(J'J)v, iterations, converged, h_max, c_max)``, the call's info record); the handle is left as it was
        found."""
        from .curvature_batch import batch_curvature

        return batch_curvature(self, points, k, rel_tol, max_iters, shift)

    def hessian_product(self, points, V_per_member, exact: bool = True):
        """``score_refine_batch_hessian_product`` at ``points``: per member A_g V_g with A = E (``exact``) or J'J;
        ``V_per_member``: one n_g x c array per member (or a vector each), the same c in 1..16 for all.  Returns the products in
        the shapes of the inputs; the handle is left as it was found."""
        from .curvature_batch import batch_hessian_product

        return batch_hessian_product(self, points, V_per_member, exact)

    def samples(self, points, ids_per_member, n_samples, seeds, first_sample: int = 0, rel_tol: float = 1e-10, max_iters: int = 4000,
                block_width: int = 16, with_rhs: bool = False, with_noise: bool = False):
        """``score_refine_batch_samples`` at ``points`` (include/score_samples_batch.h): ``n_samples`` draws of every member
        (an integer or one per member; 0: the member takes no part) from the streams of ``seeds``, the steps of the
        member-local variables ``ids_per_member``.  Returns (return code, per member the dict of ``SamplesHandle.draw`` plus
        ``determined``, the call's info record); the handle is left as it was found."""
        from .samples_batch import batch_draws

        return batch_draws(self, points, ids_per_member, n_samples, seeds, first_sample, rel_tol, max_iters, block_width, with_rhs,
                           with_noise)

    def leverage(self, points, pairs_per_member, n_samples, seeds, first_sample: int = 0, rel_tol: float = 1e-10,
                 max_iters: int = 4000, block_width: int = 16):
        """``score_refine_batch_leverage`` at ``points`` (include/score_leverage_batch.h): the leverage and redundancy sums of
        every member's measurements over ``n_samples`` draws (an integer or one per member; 0: the member takes no part) from
        the streams of ``seeds``, and of the member-local variable id pairs ``pairs_per_member`` (None or empty: none).
        Returns (return code, per member the dict of ``LeverageHandle.leverage`` plus ``determined``, the call's info
        record); the handle is left as it was found."""
        from .leverage_batch import batch_leverage

        return batch_leverage(self, points, pairs_per_member, n_samples, seeds, first_sample, rel_tol, max_iters, block_width)

    def range_variances(self, points, pairs_per_member, rel_tol: float = 1e-10, max_iters: int = 4000, block_width: int = 16):
        """``score_refine_batch_range_variances`` at ``points``: the exact variance g'H^-1 g of every listed pair of every
        member.  Returns (return code, per member the dict of ``LeverageHandle.range_variances`` without ``solutions``, the
        call's info record); the handle is left as it was found."""
        from .leverage_batch import batch_range_variances

        return batch_range_variances(self, points, pairs_per_member, rel_tol, max_iters, block_width)

    def relative_covariances(self, points, pairs_per_member, rel_tol: float = 1e-10, max_iters: int = 4000, block_width: int = 16):
        """``score_refine_batch_relative_covariances`` at ``points`` (include/score_relative_batch.h): the predicted relative
        pose of every listed pair of member-local pose ids of every member and its covariance G H^-1 G'.  Returns (return
        code, per member the dict of ``RelativeHandle.relative_covariances`` without ``solutions``, the call's info record);
        the handle is left as it was found."""
        from .relative_batch import batch_relative_covariances

        return batch_relative_covariances(self, points, pairs_per_member, rel_tol, max_iters, block_width)

    def select_ranges(self, points, pairs_per_member, precisions_per_member, k, min_gain: float = 0.0, rel_tol: float = 1e-10,
                      max_iters: int = 4000, block_width: int = 16, with_matrix: bool = False):
        """``score_refine_batch_select_ranges`` at ``points`` (include/score_select_batch.h): of every member's candidate
        ranges ``pairs_per_member`` (member-local variable id pairs; None or empty: none) with ``precisions_per_member`` the
        ``k`` (one integer, or one per member) the greedy rule picks.  Returns (return code, per member the dict of
        ``SelectionHandle.select_ranges`` plus ``picked`` and ``total_gain``, the call's info record); the handle is left as it
        was found."""
        from .selection_batch import batch_select_ranges

        return batch_select_ranges(self, points, pairs_per_member, precisions_per_member, k, min_gain, rel_tol, max_iters, block_width,
                                   with_matrix)

    def _robust(self):
        """The library with the calls of include/score_refine_robust_batch.h bound."""
        return bind(self.lib, REFINE_ROBUST_BATCH)

    def _robust_outputs(self):
        """(ranges per member, loop closures per member, [weights, residuals, loop-closure weights, loop-closure residuals])."""
        n_rng, n_lc = member_counts(self.probs)
        return n_rng, n_lc, [np.ones(max(1, int(sum(n)))) for n in (n_rng, n_rng, n_lc, n_lc)]

    def robust_run(self, points, settings, keep_weights: bool = False):
        """``score_refine_batch_robust_run`` (include/score_refine_robust_batch.h): ``settings`` is one
        ``ScoreRefineRobustSettings`` (shared) or a sequence with one per member.  Returns (points, per member
        ``(weights, residuals, loop-closure weights, loop-closure residuals)``, info dicts)."""
        lib = self._robust()
        G = len(self.probs)
        recs = [settings] if isinstance(settings, ScoreRefineRobustSettings) else list(settings)
        rs = (ScoreRefineRobustSettings * max(1, len(recs)))(*recs)
        arrays, poses_in, lms_in = self._flat_points(points)
        poses_out, lms_out = np.empty_like(poses_in), np.empty(max(1, lms_in.size))
        n_rng, n_lc, (w, r, wl, rl) = self._robust_outputs()
        infos = (ScoreRefineRobustInfo * G)()
        rc = lib.score_refine_batch_robust_run(self.h, rs, len(recs), ptr(poses_in), ptr(lms_in), ptr(poses_out), ptr(lms_out), ptr(w),
                                               ptr(r), ptr(wl), ptr(rl), 1 if keep_weights else 0, infos)
        if rc != 0:
            raise RuntimeError(f"score_refine_batch_robust_run failed: {self.lib.score_last_error().decode()}")
        per = list(zip(self._per_member(w, n_rng), self._per_member(r, n_rng), self._per_member(wl, n_lc), self._per_member(rl, n_lc)))
        return self._points_from(arrays, poses_out, lms_out), per, [infos[i].as_dict() for i in range(G)]

    def residuals(self, points, mu=0.0, c=3.0, c_rel=3.0):
        """``score_refine_batch_residuals`` at ``points``: ``mu``, ``c``, ``c_rel`` a scalar or one entry per member.  Returns
        per member ``(residuals, loop-closure residuals, weights, loop-closure weights)``."""
        lib = self._robust()
        G = len(self.probs)
        mu, c, c_rel = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (G,))) for v in (mu, c, c_rel))
        _, poses, lms = self._flat_points(points)
        n_rng, n_lc, (w, r, wl, rl) = self._robust_outputs()
        rc = lib.score_refine_batch_residuals(self.h, ptr(poses), ptr(lms), ptr(mu), ptr(c), ptr(c_rel), ptr(r), ptr(rl), ptr(w), ptr(wl))
        if rc != 0:
            raise RuntimeError(f"score_refine_batch_residuals failed: {self.lib.score_last_error().decode()}")
        return list(zip(self._per_member(r, n_rng), self._per_member(rl, n_lc), self._per_member(w, n_rng), self._per_member(wl, n_lc)))

    def robust_rounds(self):
        """``score_refine_batch_robust_rounds``: (lock-step rounds, passes in which some member changed stage) of the last
        ``robust_run``."""
        rounds, stages = C.c_int32(0), C.c_int32(0)
        if self._robust().score_refine_batch_robust_rounds(self.h, C.byref(rounds), C.byref(stages)) != 0:
            raise RuntimeError(f"score_refine_batch_robust_rounds failed: {self.lib.score_last_error().decode()}")
        return int(rounds.value), int(stages.value)

    def restore(self) -> None:
        """``score_refine_batch_restore``: the handle's cost reads the measured precisions again (after ``keep_weights``)."""
        if self._robust().score_refine_batch_restore(self.h) != 0:
            raise RuntimeError(f"score_refine_batch_restore failed: {self.lib.score_last_error().decode()}")


def refine_estimate_batch(datas, results, max_iters: int = 50, tol: float = 1e-10, range_weights=None, loop_closure_weights=None,
                          engine: str = "native", lib_path: Optional[str] = None, solver_settings: Optional[dict] = None,
                          max_group: int = 64, marginals=None, samples=None, samples_seed: int = 0, leverage=None,
                          leverage_seed: int = 0, curvature=None, relative=None, select=None):
    """``refine_estimate`` for many graphs at once: ``datas`` and ``results`` member by member, ``range_weights`` /
    ``loop_closure_weights`` lists with one entry (an array as ``refine_estimate`` takes it, or None) per member -- they only
    scale precisions.  The members are grouped by dimension, in chunks of at most ``max_group`` (the rule of
    ``score_amd/groups.py``), each group one device handle (``engine="native"``) or one lock-step loop in Python with SciPy's
    sparse LU (``engine="python"``).  Members without unknowns are answered on the host.  Returns a list of ``(refined
    SolverResults, info)`` in input order; ``info`` as ``refine_estimate`` reports it, plus ``group`` (the group's number) and
    ``rounds`` (lock-step rounds of the group).
    ``marginals``: True, or a list with one entry per graph as ``marginal_covariances_batch`` takes ``variables`` -- every
    group's handle then also computes the marginal covariances at the refined points before it is closed (one create for
    both), and ``info["marginals"]`` is the ``(cov, marginals_info)`` of ``marginal_covariances_batch`` for that graph (None
    for a graph without unknowns).
    ``samples``: a number of draws S -- every group's handle then also draws S posterior samples of every member at the refined
    points (``posterior_samples_batch``'s call on the same handle: default variables, graph i from the stream of
    ``samples_seed + i``), and ``info["samples"]`` is that graph's ``(Samples, samples_info)`` (None for a graph without
    unknowns).  Without the keyword nothing changes.
    ``leverage``: a number of draws S -- every group's handle then also forms the leverage and redundancy of every member's
    measurements at the refined points (``range_leverage_batch``'s call on the same handle: no pairs, graph i from the stream
    of ``leverage_seed + i``; ``engine="python"``: ``range_leverage``'s python engine), and ``info["leverage"]`` is that
    graph's ``(Leverage, leverage_info)`` (None for a graph without unknowns).  Without the keyword nothing changes.
    ``curvature``: a number of modes k -- every group's handle then also runs the second-order check at the refined points
    (``hessian_spectrum_batch``'s call on the same handle, after the other analyses: the k lowest eigenpairs of E, half the
    Hessian of the cost, at its default tolerances; ``engine="python"``: the dense path), and ``info["curvature"]`` is that
    graph's ``(Curvature, curvature_info)`` (None for a graph without unknowns).  A member with fewer than 48 unknowns is
    answered by the dense path; the other members of its group then run on a handle of their own.  Without the keyword nothing
    changes.
    ``relative``: a list with one entry per graph, None or a list of pose name pairs as ``predicted_relative_poses_batch`` takes
    ``pairs`` -- every group's handle then also predicts the relative poses of the listed pairs at the refined points with
    their covariances (``predicted_relative_poses_batch``'s call on the same handle, after the other analyses;
    ``engine="python"``: the dense path), and ``info["relative"]`` is that graph's ``(PredictedRelativePoses, info)`` (empty
    for a graph that lists none, None for a graph without unknowns).  Without the keyword nothing changes.
    ``select``: a dict ``{"pairs": ..., "k": ..., "precision": 1.0, "min_gain": 0.0}`` with the arguments of those names of
    ``select_ranges_batch`` (``pairs``: one entry per graph, None or a list of name pairs) -- every group's handle then also
    picks k of each graph's candidate ranges at the refined points (``select_ranges_batch``'s call on the same handle, after
    the other analyses; ``engine="python"``: the dense path), and ``info["selection"]`` is that graph's ``(Selection, info)``
    (empty for a graph that lists none, None for a graph without unknowns).  Without the keyword nothing changes."""
    from .leverage import range_leverage
    from .leverage_batch import group_leverage
    from .marginals import _select
    from .marginals_batch import marginals_follow_up
    from .curvature_batch import _check_arguments as _check_curvature_arguments, follow_up_curvature
    from .samples_batch import _check_draw_arguments, group_samples

    if engine not in ("native", "python"):
        raise ValueError("engine must be 'native' or 'python'")
    datas, results = paired(datas, results, max_group)
    rws = per_graph(range_weights, len(datas), "range_weights")
    lws = per_graph(loop_closure_weights, len(datas), "loop_closure_weights")
    follow_ups = []  # (on a group's handle in this order)
    if marginals is not None and marginals is not False:
        follow_ups.append(marginals_follow_up(marginals, len(datas)))
    if samples is not None and samples is not False:
        _check_draw_arguments([samples], 0, 16, 1e-10, 4000)

        def draws(handle, number, idx, probs, pts, costs, selections):
            """(Samples, info) per member at the refined points, retracted onto the refined estimates"""
            ests = [_as_results(p, pt, results[i], f) for p, pt, i, f in zip(probs, pts, idx, costs)]
            return group_samples(handle, probs, pts, ests, selections, idx, number, [int(samples)] * len(idx),
                                 [int(samples_seed) + i for i in idx], engine="python" if handle is None else "device")

        follow_ups.append(FollowUp("samples", draws, lambda i, prob: _select(prob, None)))
    if leverage is not None and leverage is not False:
        _check_draw_arguments([leverage], 0, 16, 1e-10, 4000)

        def leverages(handle, number, idx, probs, pts, costs, kept):
            """(Leverage, info) per member at the refined points"""
            if handle is None:
                return [range_leverage(datas[i], _as_results(p, pt, results[i], f), int(leverage), int(leverage_seed) + i,
                                       range_weights=rws[i], loop_closure_weights=lws[i], engine="python")
                        for p, pt, i, f in zip(probs, pts, idx, costs)]
            return group_leverage(handle, probs, pts, [None] * len(idx), idx, number, [int(leverage)] * len(idx),
                                  [int(leverage_seed) + i for i in idx])

        follow_ups.append(FollowUp("leverage", leverages))
    if curvature is not None and curvature is not False:
        _check_curvature_arguments(curvature, 1e-9, 200, 1e-8)

        def curvatures(handle, number, idx, probs, pts, costs, kept):
            """(Curvature, info) per member at the refined points"""
            return follow_up_curvature(handle, number, idx, probs, pts, int(curvature), lib_path, solver_settings)

        def enough_unknowns(i, prob):
            if int(curvature) > prob.n:
                raise ValueError(f"graph {i}: k = {int(curvature)} modes of a graph with {prob.n} unknowns")

        follow_ups.append(FollowUp("curvature", curvatures, enough_unknowns))
    if relative is not None and relative is not False:
        from .relative import _pose_pair_ids, predicted_relative_poses
        from .relative_batch import _empty, group_relative

        pair_names = [[tuple(p) for p in nm] if nm is not None else [] for nm in per_graph(relative, len(datas), "relative", none=False)]

        def relatives(handle, number, idx, probs, pts, costs, kept):
            """(PredictedRelativePoses, info) per member at the refined points"""
            if handle is None:
                return [predicted_relative_poses(datas[i], _as_results(p, pt, results[i], f), pair_names[i], rws[i], lws[i], engine="python")
                        if pair_names[i] else _empty(datas[i].dimension, 3 if datas[i].dimension == 2 else 6, "python")
                        for p, pt, i, f in zip(probs, pts, idx, costs)]
            return group_relative(handle, pts, [pair_names[i] for i in idx], kept, idx, number)

        follow_ups.append(FollowUp("relative", relatives,
                                   lambda i, prob: _pose_pair_ids(prob, pair_names[i], f"refine_estimate_batch: graph {i}")))
    if select is not None and select is not False:
        from .leverage import pair_ids
        from .selection_batch import _python_selection, group_selection, selection_arguments

        unknown = set(select) - {"pairs", "k", "precision", "min_gain"}
        if unknown or "pairs" not in select or "k" not in select:
            raise ValueError("select: a dict with 'pairs' and 'k', and optionally 'precision' and 'min_gain'")
        sel_gain = float(select.get("min_gain", 0.0))
        sel_names = [[tuple(p) for p in nm] if nm is not None else []
                     for nm in per_graph(select["pairs"], len(datas), "select['pairs']", none=False)]
        sel_k, sel_w = selection_arguments(sel_names, select["k"], select.get("precision", 1.0), sel_gain, "refine_estimate_batch")

        def selections(handle, number, idx, probs, pts, costs, kept):
            """(Selection, info) per member at the refined points"""
            if handle is None:
                return [_python_selection(datas[i], _as_results(p, pt, results[i], f), sel_names[i], sel_k[i], sel_w[i], sel_gain, rws[i],
                                          lws[i], i, "refine_estimate_batch")
                        for p, pt, i, f in zip(probs, pts, idx, costs)]
            return group_selection(handle, pts, [sel_names[i] for i in idx], kept, [sel_w[i] for i in idx], [sel_k[i] for i in idx],
                                   number, sel_gain)

        follow_ups.append(FollowUp("selection", selections,
                                   lambda i, prob: pair_ids(prob, sel_names[i], f"refine_estimate_batch: graph {i}")))
    out: list = [None] * len(datas)

    def member(i, data, res):
        prob, point = _problem_of(data, res, rws[i], lws[i])
        if prob.n == 0:  # nothing to refine: the host's answer, as refine_estimate gives it
            out[i] = refine_estimate(data, res, max_iters=max_iters, tol=tol, linear_solver="scipy", engine="python",
                                     range_weights=rws[i], loop_closure_weights=lws[i])
            out[i][1].update({f.key: None for f in follow_ups})
            return None
        for f in follow_ups:  # (the selections' errors before any work)
            f.keep(i, prob)
        return prob, point

    def body(handle, number, idx, probs, points, extras):
        if handle is None:
            pts, S, rounds = _python_lock_step(probs, points, max_iters, tol)
            infos = [{"cost_initial": s.cost_initial, "cost_final": s.f, "iterations": s.iterations, "grad_inf": s.gnorm,
                      "linear_solver": "scipy", "engine": "python", "pcg_iters": 0, "linear_solves": s.linear_solves} for s in S]
        else:
            pts, raw = handle.run(points, max_iters, tol)
            rounds = max(r["linear_solves"] for r in raw)
            infos = [_native_info(r) for r in raw]
        extra = follow(follow_ups, handle, number, idx, probs, pts, [info["cost_final"] for info in infos])
        for info, more in zip(infos, extra):
            info["group"], info["rounds"] = number, rounds
            info.update(more)
        return [(_as_results(prob, pt, results[i], info["cost_final"]), info) for i, prob, pt, info in zip(idx, probs, pts, infos)]

    return run_chunks(grouped(datas, results, member, named=False), max_group, out, body, engine == "native", lib_path, solver_settings)
