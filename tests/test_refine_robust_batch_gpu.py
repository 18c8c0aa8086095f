"""Batched outlier-robust refinement on the device (include/score_refine_robust_batch.h, csrc/score_gn_robust_batch.hpp).

Tolerances.  The kernels, entry by entry, to the bounds of tests/test_refine_robust_gpu.py: residuals rtol 1e-11 against the NumPy
twins (both fp64 with the same operations); a weight strictly between the thresholds |w - w_ref| <= 1e-11 (w_ref + mu) plus the
rounding of the subtraction, and exactly 0 or 1 beyond them.  The loop against the single handle (the two differ in the rounding
of their conjugate-gradient implementations only): outer counts, outlier sets and weights equal, mu rel 1e-9, cost rel 1e-7, poses
and landmarks atol 1e-7 in 2-D and 1e-5 in 3-D (the figure tests/test_refine_batch_gpu.py holds there); poses 1e-5 against SciPy's
LU.  A member that stops after solve 1 is the plain batch's member, bit for bit.  The marginal covariances under the kept weights
are judged by the derived bound of tests/marginals_helpers.py."""
import ctypes as C

import numpy as np
import pytest

from marginals_helpers import Reference, check_columns
from refine_robust_batch_helpers import (CLEAN3, SCHEDULE, THRESHOLD, batch, graph, landmarks_of, pinned_member, poses_of, second_start,
                                         single, sparse_members, wide_member)
from refine_robust_helpers import point_of
from score_amd.marginals import _problem_and_point, _select, dense_information
from score_amd.marginals_batch import marginal_covariances_batch
from score_amd.refine_batch import RefineBatchHandle, refine_estimate_batch
from score_amd.refine_robust import (ScoreRefineRobustInfo, ScoreRefineRobustSettings, loop_closure_residuals, range_residuals)
from score_amd.refine_robust_batch import _bind
from score_amd.robust import gnc_tls_weight, n_loop_closures_of
from score_amd.solver import _f64p, load_library

pytestmark = pytest.mark.gpu

RTOL = 1e-11
VACUOUS = 1e-3  # tests/test_marginals_batch_gpu.py: worst bound / largest covariance entry beyond which the bound says nothing
MUS = (0.0, 1e-3, 1.0, 1e3)


def _settings(c=3.0, c_rel=None, families=3, **kw):
    rs = ScoreRefineRobustSettings()
    rs.inlier_threshold, rs.rel_threshold, rs.mu_step, rs.min_weight = c, c if c_rel is None else c_rel, 1.4, 1e-6
    rs.families, rs.max_outer, rs.inner_iters, rs.max_iters, rs.tol = families, 50, 5, 50, 1e-10
    for k, v in kw.items():
        setattr(rs, k, v)
    return rs


def _members(pairs):
    got = [point_of(fg, start) for fg, start in pairs]
    return [g[0] for g in got], [g[1] for g in got]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels, entry by entry
# ---------------------------------------------------------------------------------------------------------------------
def _check_group(pairs, hip_lib, c=(3.0, 2.0, 4.0), c_rel=(2.5, 3.5, 1.5)):
    """score_refine_batch_residuals at the members' start points against the NumPy twins: every mu on every member, mixed across
    the members within one call.  Returns per member (ranges, loop closures, classes of the weight rule its ranges met)."""
    probs, points = _members(pairs)
    G = len(probs)
    cs, crs = [c[g % len(c)] for g in range(G)], [c_rel[g % len(c_rel)] for g in range(G)]
    refs = []
    for prob, point in zip(probs, points):
        n_lc, ne = n_loop_closures_of(prob.a), len(prob.bi)
        refs.append((range_residuals(prob, point, prob.a["rng_prec"]),
                     loop_closure_residuals(prob, point, prob.a["rel_kappa"][ne - n_lc:], prob.a["rel_tau"][ne - n_lc:])))
    classes = [set() for _ in range(G)]
    with RefineBatchHandle(probs, hip_lib) as h:
        for shift in range(len(MUS)):
            mus = [MUS[(g + shift) % len(MUS)] for g in range(G)]
            got = h.residuals(points, mus, cs, crs)
            for g, (r, rl, w, wl) in enumerate(got):
                mu = mus[g]
                for name, got_r, got_w, want_r, cf in (("ranges", r, w, refs[g][0], cs[g]), ("loop closures", rl, wl, refs[g][1], crs[g])):
                    assert got_r.shape == want_r.shape == got_w.shape, (g, name)
                    if len(want_r):
                        print("member", g, name, "mu", mu, "worst relative residual difference",
                              float(np.max(np.abs(got_r - want_r) / np.maximum(want_r, 1e-300))))
                    np.testing.assert_allclose(got_r, want_r, rtol=RTOL, atol=0)
                    if mu == 0.0:
                        assert np.all(got_w == 1.0)
                        continue
                    want_w = gnc_tls_weight(want_r, mu, cf)
                    r2, lo, hi = want_r * want_r, mu / (mu + 1.0) * cf * cf, (mu + 1.0) / mu * cf * cf
                    margin = 4.0 * RTOL  # on r^2: twice the residual's tolerance, twice over
                    inl, out = r2 <= lo * (1.0 - margin), r2 >= hi * (1.0 + margin)
                    mid = (r2 >= lo * (1.0 + margin)) & (r2 <= hi * (1.0 - margin))
                    assert np.all(got_w[inl] == 1.0) and np.all(got_w[out] == 0.0)
                    assert np.all(np.abs(got_w[mid] - want_w[mid]) <= RTOL * (want_w[mid] + mu) + 4 * np.finfo(float).eps * (1.0 + mu))
                    assert np.all((got_w >= 0.0) & (got_w <= 1.0))
                    if name == "ranges":
                        classes[g] |= {k for k, m in (("in", inl), ("mid", mid), ("out", out)) if np.any(m)}
    return [(len(a), len(b), cl) for (a, b), cl in zip(refs, classes)]


def test_kernels_entry_by_entry_2d(hip_lib):
    got = _check_group([graph(k)[:2] for k in ("G1", "G2", "G4")], hip_lib)
    assert [(a, b) for a, b, _ in got] == [(185, 4), (68, 3), (185, 4)]
    assert got[0][2] == {"in", "mid", "out"}  # every branch of the weight rule was taken


def test_kernels_entry_by_entry_3d(hip_lib):
    got = _check_group([graph(k)[:2] for k in ("G3", CLEAN3)], hip_lib)
    assert got[0][:2] == (78, 3) and got[0][2] == {"in", "mid", "out"}


def test_kernels_at_the_pinned_pose(hip_lib):
    fg, start = pinned_member()
    prob, _ = point_of(fg, start)
    assert prob.ra[0] == 0 and prob.bi[len(prob.bi) - 2] == 0
    _check_group([graph("G1")[:2], (fg, start)], hip_lib)


def test_a_member_over_two_workgroups(hip_lib):
    """The middle member has more than 256 lanes: it spans two workgroups, and the next member starts on a fresh one."""
    got = _check_group([graph("G2")[:2], wide_member(), graph("G4")[:2]], hip_lib)
    print(got)
    assert 256 < got[1][0] + got[1][1] <= 512


def test_members_with_an_empty_family(hip_lib):
    got = _check_group(sparse_members() + [graph("G2")[:2]], hip_lib)
    assert got[0][1] == 0 and got[0][0] > 0 and got[1][0] == 0 and got[1][1] == 2 and got[2][:2] == (0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the loop against the single handle
# ---------------------------------------------------------------------------------------------------------------------
_runs = {}


def _batch(keys, hip_lib, **kw):
    at = (tuple(keys), hip_lib, tuple(sorted(kw.items())))
    if at not in _runs:
        _runs[at] = batch(list(keys), engine="native", lib_path=hip_lib, **kw)
    return _runs[at]


def _assert_member(key, got, hip_lib, atol):
    fg, _, bad, _, lc_bad = graph(key)
    (res, info), (res_1, info_1), (res_s, info_s) = got, single(key, "native", hip_lib), single(key)
    rb, r1, rs = info["robust"], info_1["robust"], info_s["robust"]
    print(key, "outer", rb["outer_iterations"], r1["outer_iterations"], rs["outer_iterations"], "iterations", info["iterations"],
          info_1["iterations"], "mu", rb["mu"], r1["mu"], "cost", info["cost_final"], info_1["cost_final"],
          "worst pose difference", float(np.max(np.abs(poses_of(fg, res) - poses_of(fg, res_1)))),
          "against SciPy's LU", float(np.max(np.abs(poses_of(fg, res) - poses_of(fg, res_s)))))
    assert rb["outer_iterations"] == r1["outer_iterations"] and rb["converged"] == r1["converged"]
    for name in ("outliers", "loop_closure_outliers", "weights", "loop_closure_weights"):
        np.testing.assert_array_equal(rb[name], r1[name], err_msg=f"{key}: {name}")
    assert rb["mu"] == pytest.approx(r1["mu"], rel=1e-9, abs=0)
    assert info["cost_final"] == pytest.approx(info_1["cost_final"], rel=1e-7, abs=0)
    np.testing.assert_allclose(poses_of(fg, res), poses_of(fg, res_1), rtol=0, atol=atol)
    np.testing.assert_allclose(landmarks_of(fg, res), landmarks_of(fg, res_1), rtol=0, atol=atol)
    # SciPy's LU: the same sets
    np.testing.assert_array_equal(rb["outliers"], rs["outliers"])
    np.testing.assert_array_equal(rb["loop_closure_outliers"], rs["loop_closure_outliers"])
    np.testing.assert_allclose(poses_of(fg, res), poses_of(fg, res_s), rtol=0, atol=1e-5)
    # the planted sets
    np.testing.assert_array_equal(rb["outliers"], bad)
    np.testing.assert_array_equal(rb["loop_closure_outliers"], lc_bad)
    assert rb["converged"]
    # the reported residuals are those of the final estimate
    prob, point = point_of(fg, res)
    n_lc, ne = n_loop_closures_of(prob.a), len(prob.bi)
    np.testing.assert_allclose(rb["residuals"], range_residuals(prob, point, prob.a["rng_prec"]), rtol=1e-9, atol=0)
    np.testing.assert_allclose(rb["loop_closure_residuals"],
                               loop_closure_residuals(prob, point, prob.a["rel_kappa"][ne - n_lc:], prob.a["rel_tau"][ne - n_lc:]),
                               rtol=1e-9, atol=0)


def test_the_loop_matches_the_single_handle_2d(hip_lib):
    keys = ("G1", "G4", "G2")
    out = _batch(keys, hip_lib)
    for key, got in zip(keys, out):
        _assert_member(key, got, hip_lib, 1e-7)
    outer = [info["robust"]["outer_iterations"] for _, info in out]
    assert outer[1] == 1 and outer[0] > outer[2] > 1  # the members leave the schedule at different times
    assert out[0][1]["rounds"] == max(info["linear_solves"] for _, info in out)
    assert out[0][1]["stage_rounds"] >= outer[0]


def test_the_loop_matches_the_single_handle_3d(hip_lib):
    keys = ("G3", CLEAN3)
    out = _batch(keys, hip_lib)
    for key, got in zip(keys, out):
        _assert_member(key, got, hip_lib, 1e-5)
        R = poses_of(graph(key)[0], got[0])[:, :3, :3]
        assert np.max(np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3))) <= 1e-12
    assert [info["robust"]["outer_iterations"] for _, info in out][1] == 1


# ---------------------------------------------------------------------------------------------------------------------
# 3. clean members are the plain batch, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _points_equal(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def test_clean_members_are_the_plain_batch_bit_for_bit(hip_lib):
    fg = graph("G4")[0]
    probs, points = _members([(fg, graph("G4")[1]), (fg, second_start("G4"))])
    with RefineBatchHandle(probs, hip_lib) as h:
        pts, per, infos = h.robust_run(points, _settings(c=5.0))
    with RefineBatchHandle(probs, hip_lib) as h:
        pts_p, infos_p = h.run(points)
    _points_equal(pts, pts_p)
    for (w, r, wl, rl), info, plain in zip(per, infos, infos_p):
        assert np.all(w == 1.0) and np.all(wl == 1.0) and len(w) == 185 and len(wl) == 4
        assert info["mu"] == 0.0 and info["outer_iterations"] == 1 and info["converged"] == 1
        assert info["outliers"] == 0 and info["rel_outliers"] == 0
        for name in ("cost_initial", "cost_final", "grad_inf", "linear_solves", "pcg_iters"):
            assert info[name] == plain[name], name
        assert info["lm_iterations"] == plain["iterations"]


def test_the_clean_member_of_a_mixed_group_is_the_plain_batch_member(hip_lib):
    keys = ("G1", "G4", "G2")
    (res, info) = _batch(keys, hip_lib)[1]
    plain = refine_estimate_batch([graph(k)[0] for k in keys], [graph(k)[1] for k in keys], lib_path=hip_lib)[1]
    fg = graph("G4")[0]
    np.testing.assert_array_equal(poses_of(fg, res), poses_of(fg, plain[0]))
    np.testing.assert_array_equal(landmarks_of(fg, res), landmarks_of(fg, plain[0]))
    for name in ("cost_initial", "cost_final", "grad_inf", "iterations", "linear_solves", "pcg_iters"):
        assert info[name] == plain[1][name], name


# ---------------------------------------------------------------------------------------------------------------------
# 4. shared and per-member settings
# ---------------------------------------------------------------------------------------------------------------------
def test_shared_settings_equal_identical_records(hip_lib):
    probs, points = _members([graph(k)[:2] for k in ("G2", "G4", "G2")])
    with RefineBatchHandle(probs, hip_lib) as h:
        one = h.robust_run(points, _settings(c=3.0))
    with RefineBatchHandle(probs, hip_lib) as h:
        many = h.robust_run(points, [_settings(c=3.0) for _ in probs])
        with pytest.raises(RuntimeError, match="n_settings must be 1 or the number of members"):
            h.robust_run(points, [_settings(), _settings()])
    _points_equal(one[0], many[0])
    for a, b in zip(one[1], many[1]):
        _points_equal(a, b)
    drop = ("setup_ms", "solve_ms")
    assert [{k: v for k, v in i.items() if k not in drop} for i in one[2]] == [{k: v for k, v in i.items() if k not in drop} for i in many[2]]


def test_families_per_member(hip_lib):
    """Member 0 re-weights its ranges only, member 1 both families: member 0's false loop closure keeps weight 1, and its
    loop-closure residuals are reported all the same."""
    probs, points = _members([graph("G2")[:2], graph("G2")[:2]])
    with RefineBatchHandle(probs, hip_lib) as h:
        pts, per, infos = h.robust_run(points, [_settings(families=1), _settings(families=3)])
    (w0, r0, wl0, rl0), (w1, r1, wl1, rl1) = per
    assert np.all(wl0 == 1.0) and infos[0]["rel_outliers"] == 0
    assert infos[1]["rel_outliers"] == 1 and np.count_nonzero(wl1 == 0.0) == 1
    prob = probs[0]
    n_lc, ne = n_loop_closures_of(prob.a), len(prob.bi)
    want = loop_closure_residuals(prob, pts[0], prob.a["rel_kappa"][ne - n_lc:], prob.a["rel_tau"][ne - n_lc:])
    np.testing.assert_allclose(rl0, want, rtol=1e-9, atol=0)
    assert np.max(rl0) > 3.0 and infos[0]["outliers"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. the handle afterwards
# ---------------------------------------------------------------------------------------------------------------------
def test_the_handle_afterwards(hip_lib):
    probs, points = _members([graph("G2")[:2], graph("G4")[:2]])
    with RefineBatchHandle(probs, hip_lib) as h:
        fresh_plain = h.run(points)
    drop = ("setup_ms", "solve_ms")
    strip = lambda infos: [{k: v for k, v in i.items() if k not in drop} for i in infos]  # noqa: E731
    with RefineBatchHandle(probs, hip_lib) as h:
        first = h.robust_run(points, [_settings(c=3.0), _settings(c=5.0)])
        assert first[2][0]["outer_iterations"] > 1
        after = h.run(points)  # keep_weights = 0: the measured precisions are back
        _points_equal(after[0], fresh_plain[0])
        assert strip(after[1]) == strip(fresh_plain[1])
        with pytest.raises(RuntimeError, match=r"member 1: max_outer must be >= 1"):
            h.robust_run(points, [_settings(), _settings(max_outer=0)])
        after = h.run(points)
        _points_equal(after[0], fresh_plain[0])
        assert strip(after[1]) == strip(fresh_plain[1])
        second = h.robust_run(points, [_settings(c=3.0), _settings(c=5.0)])
    _points_equal(second[0], first[0])
    for a, b in zip(second[1], first[1]):
        _points_equal(a, b)
    assert strip(second[2]) == strip(first[2])


# ---------------------------------------------------------------------------------------------------------------------
# 6. keep_weights = 1
# ---------------------------------------------------------------------------------------------------------------------
class WeightedReference(Reference):
    """tests/marginals_helpers.py's dense reference, with weights on both families."""

    def __init__(self, fg, results, range_weights=None, loop_closure_weights=None):
        import scipy.linalg as sla

        self.prob, self.point = _problem_and_point(fg, results, range_weights, loop_closure_weights)
        self.H = dense_information(self.prob, self.point)
        self.H.setflags(write=False)
        self.n = self.prob.n
        self.chol = sla.cho_factor(self.H, lower=True)
        self.lambda_min = float(sla.eigvalsh(self.H, subset_by_index=[0, 0])[0])
        assert self.lambda_min > 0
        self.longest_row = int(np.max(np.count_nonzero(self.H, axis=1)))
        self.absH = np.abs(self.H)


def _check_marginals(label, ref, cols, column):
    A, rho, _, converged = column
    assert np.all(converged)
    figures, bound, _ = check_columns(ref, cols, A, rho, label)
    assert figures["worst_bound_over_max_sigma"] < VACUOUS, f"{label}: the bound is vacuous"
    return A, bound


def test_kept_weights_serve_the_marginals(hip_lib):
    keys = ("G1", "G2")
    fgs = [graph(k)[0] for k in keys]
    out = _batch(keys, hip_lib, marginals=True)
    refined = [res for res, _ in out]
    ws = [info["robust"]["weights"] for _, info in out]
    wls = [info["robust"]["loop_closure_weights"] for _, info in out]
    assert all(np.any(w == 0.0) for w in ws) and all(np.any(w == 0.0) for w in wls)
    weighted = [WeightedReference(fg, res, w, wl) for fg, res, w, wl in zip(fgs, refined, ws, wls)]
    plain = [WeightedReference(fg, res) for fg, res in zip(fgs, refined)]
    assert all(np.max(np.abs(a.H - b.H)) > 1e-3 for a, b in zip(weighted, plain))  # the weights matter
    probs, points = _members([graph(k)[:2] for k in keys])
    sels = [_select(prob, None) for prob in probs]
    with RefineBatchHandle(probs, hip_lib) as h:
        pts, per, infos = h.robust_run(points, _settings(c=3.0), keep_weights=True)
        for g, key in enumerate(keys):  # (the same run as the one above)
            np.testing.assert_array_equal(per[g][0], ws[g])
            np.testing.assert_array_equal(per[g][2], wls[g])
        rc, cols, _ = h.marginals(pts, [sel[1] for sel in sels])
        assert rc == 0
        kept = [_check_marginals(f"{key}, kept weights", weighted[g], sels[g][3], cols[g]) for g, key in enumerate(keys)]
        h.restore()
        rc, cols, _ = h.marginals(pts, [sel[1] for sel in sels])
        assert rc == 0
        for g, key in enumerate(keys):
            _check_marginals(f"{key}, restored", plain[g], sels[g][3], cols[g])
    # the high-level call: the covariances of marginal_covariances_batch with the returned weights -- both lie within their own
    # bounds of the same dense reference
    again = marginal_covariances_batch(fgs, refined, range_weights=ws, loop_closure_weights=wls, lib_path=hip_lib)
    for g, key in enumerate(keys):
        ref, (names, _, size, cols) = weighted[g], sels[g]
        X, rho_ref, delta = ref.solve(cols)
        want = 0.5 * (X[cols, :] + X[cols, :].T)
        off = np.concatenate([[0], np.cumsum(size)])
        worst_bound = []
        for label, (cov, minfo) in (("refine_estimate_robust_batch", out[g][1]["marginals"]), ("marginal_covariances_batch", again[g])):
            assert list(cov) == minfo["order"] == names
            bound = (np.asarray(minfo["residuals"]) + delta + rho_ref) / ref.lambda_min
            assert np.max(bound) / np.max(np.abs(want)) < VACUOUS
            worst_bound.append(bound)
            for k, nm in enumerate(names):
                sl = slice(off[k], off[k + 1])
                worst = float(np.max(np.abs(cov[nm] - want[sl, sl])))
                assert worst <= np.max(bound[sl]), (key, label, nm, worst)
        # ... and so the two agree with each other to the sum of their bounds
        (cov_a, _), (cov_b, _) = out[g][1]["marginals"], again[g]
        for k, nm in enumerate(names):
            sl = slice(off[k], off[k + 1])
            allowed = float(np.max(worst_bound[0][sl]) + np.max(worst_bound[1][sl]))
            print(key, nm, "difference", float(np.max(np.abs(cov_a[nm] - cov_b[nm]))), "allowed", allowed)
            np.testing.assert_allclose(cov_a[nm], cov_b[nm], rtol=0, atol=allowed)


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors are reported, not faults
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_are_reported(hip_lib):
    lib = _bind(load_library(hip_lib))
    probs, points = _members([graph("G2")[:2], graph("G4")[:2]])
    rs = _settings()
    err = lambda: lib.score_last_error().decode()  # noqa: E731
    with RefineBatchHandle(probs, hip_lib) as h:
        _, poses, lms = h._flat_points(points)
        p = lambda x: x.ctypes.data_as(_f64p)  # noqa: E731
        out_p, out_l = np.empty_like(poses), np.empty_like(lms)
        infos = (ScoreRefineRobustInfo * 2)()
        call = lambda handle, s, pi, li: lib.score_refine_batch_robust_run(handle, C.byref(s) if s is not None else None, 1, pi, li,  # noqa: E731
                                                                            p(out_p), p(out_l), None, None, None, None, 0, infos)
        assert call(None, rs, p(poses), p(lms)) != 0 and "null handle" in err()
        assert call(h.h, rs, None, p(lms)) != 0 and "points are missing" in err()
        assert call(h.h, rs, p(poses), None) != 0 and "points are missing" in err()
        assert call(h.h, None, p(poses), p(lms)) != 0 and "settings are missing" in err()
        assert call(h.h, _settings(families=0), p(poses), p(lms)) != 0 and "member 0: families must be" in err()
        assert call(h.h, _settings(max_outer=0), p(poses), p(lms)) != 0 and "member 0: max_outer must be >= 1" in err()
        assert lib.score_refine_batch_residuals(None, p(poses), p(lms), None, None, None, None, None, None, None) != 0 and "null handle" in err()
        assert lib.score_refine_batch_residuals(h.h, p(poses), p(lms), None, None, None, None, None, None, None) != 0 and "one entry per member" in err()
        assert lib.score_refine_batch_restore(None) != 0 and "null handle" in err()
        # the handle stays usable
        assert call(h.h, _settings(c=5.0, max_outer=2), p(poses), p(lms)) == 0
        assert infos[1].outer_iterations == 1 and infos[0].outer_iterations == 2 and infos[0].converged == 0
        assert h.robust_rounds()[0] > 0
