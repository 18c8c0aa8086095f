"""Batched marginal covariances (score_amd/marginals_batch.py) and the NEES (score_amd/consistency.py): what runs without a
GPU -- the dense engine member by member, the grouping, the argument errors, the binding of
include/score_marginals_batch.h.  The device path is tests/test_marginals_batch_gpu.py."""
import os
import re

import numpy as np
import pytest

from marginals_helpers import landmark_names, pose_names
from refine_batch_helpers import member
from score_amd.consistency import nees, pose_error
from score_amd.marginals import marginal_covariances
from score_amd.marginals_batch import MARGINALS_BATCH_SYMBOLS, marginal_covariances_batch
from score_amd.refine import so3_exp
from score_amd.solver import load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want):
    (cov, info), (cov1, info1) = got, want
    assert list(cov) == list(cov1) and info["order"] == info1["order"]
    for nm in cov1:
        np.testing.assert_array_equal(cov[nm], cov1[nm])
    for f in ("residuals", "iterations", "joint", "joint_raw"):
        np.testing.assert_array_equal(info[f], info1[f])
    for f in ("asymmetry", "pcg_iters", "batches", "engine"):
        assert info[f] == info1[f]


def test_python_engine_equals_the_single_call_member_by_member():
    """Mixed dimensions, groups of at most two, per-graph variables and weights: every graph comes back at its own place
    with exactly what marginal_covariances(engine="python") gives on it alone."""
    keys = ("B", "3D0", "C", "E", "3D1")
    fgs, starts = [member(k)[0] for k in keys], [member(k)[1] for k in keys]
    w = np.ones(len(fgs[0].range_measurements))
    w[[1, 5, 9]] = 0.0
    poses_e = pose_names(fgs[3])
    variables = [None, None, None, [poses_e[1][7], landmark_names(fgs[3])[0], poses_e[0][3]], None]
    weights = [w, None, None, None, None]
    out = marginal_covariances_batch(fgs, starts, variables, joint=True, range_weights=weights, engine="python", max_group=2)
    assert len(out) == len(keys)
    # 2-D first (B, C | E), then 3-D (3D0, 3D1): the group numbers follow refine_estimate_batch's grouping
    assert [info["group"] for _, info in out] == [0, 2, 0, 1, 2]
    for fg, st, v, rw, got in zip(fgs, starts, variables, weights, out):
        _same(got, marginal_covariances(fg, st, v, joint=True, range_weights=rw, engine="python"))
        assert got[1]["passes"] == 0
    assert out[3][1]["order"] == variables[3]
    plain = marginal_covariances(fgs[0], starts[0], engine="python")[0]
    assert max(np.max(np.abs(plain[nm] - out[0][0][nm])) for nm in plain) > 0  # the weights reached graph 0


def test_validation_errors_carry_the_graph_index():
    fgs, starts = [member(k)[0] for k in ("C", "B")], [member(k)[1] for k in ("C", "B")]
    first = fgs[1].pose_variables[0][0].name
    other = fgs[1].pose_variables[1][3].name
    kw = dict(engine="python")
    with pytest.raises(ValueError, match=r"graph 1: .*fixed first pose"):
        marginal_covariances_batch(fgs, starts, [None, [first]], **kw)
    with pytest.raises(ValueError, match=r"graph 1: .*unknown variable"):
        marginal_covariances_batch(fgs, starts, [None, ["no_such_variable"]], **kw)
    with pytest.raises(ValueError, match=r"graph 1: .*twice"):
        marginal_covariances_batch(fgs, starts, [None, [other, other]], **kw)
    with pytest.raises(ValueError, match=r"graph 0: .*no variables"):
        marginal_covariances_batch(fgs, starts, [[], None], **kw)
    with pytest.raises(ValueError, match=r"graph 1: .*range_weights"):
        marginal_covariances_batch(fgs, starts, range_weights=[None, np.ones(len(fgs[1].range_measurements) + 1)], **kw)
    with pytest.raises(ValueError, match="one entry per graph"):
        marginal_covariances_batch(fgs, starts, [None], **kw)
    with pytest.raises(ValueError, match="one estimate per graph"):
        marginal_covariances_batch(fgs, starts[:1], **kw)
    with pytest.raises(ValueError, match="engine"):
        marginal_covariances_batch(fgs, starts, engine="host")
    with pytest.raises(ValueError, match="max_group"):
        marginal_covariances_batch(fgs, starts, max_group=0, **kw)
    with pytest.raises(ValueError, match="rel_tol"):
        marginal_covariances_batch(fgs, starts, rel_tol=0.0, **kw)


@pytest.mark.parametrize("width", [0, -1, 17, 2.5])
def test_block_width_outside_1_to_16_is_refused(width):
    fg, start = member("C")
    with pytest.raises(ValueError, match="block_width"):
        marginal_covariances_batch([fg], [start], block_width=width, engine="python")


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "score_marginals_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(score_[a-z_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert _declared_symbols() == sorted(MARGINALS_BATCH_SYMBOLS)


def test_hip_library_exports_the_declared_symbols(hip_lib):
    lib = load_library(hip_lib)
    for sym in _declared_symbols():
        assert hasattr(lib, sym), sym


def test_nees_is_the_quadratic_form_by_hand():
    fg, est = member("C")  # the noisy start is the "estimate", the graph's own true values the truth
    truth = _truth_2d(fg)
    cov, info = marginal_covariances(fg, est, engine="python")
    got = nees(truth, est, cov)
    assert list(got) == info["order"]
    for nm in info["order"]:
        if nm in est.landmarks:
            e = np.asarray(truth.landmarks[nm]) - np.asarray(est.landmarks[nm])
        else:
            Tt, Te = truth.poses[nm], est.poses[nm]
            dth = np.arctan2(Tt[1, 0], Tt[0, 0]) - np.arctan2(Te[1, 0], Te[0, 0])
            e = np.array([(dth + np.pi) % (2 * np.pi) - np.pi, Tt[0, 2] - Te[0, 2], Tt[1, 2] - Te[1, 2]])
        want = float(e @ np.linalg.inv(cov[nm]) @ e)
        assert got[nm][1] == e.size == cov[nm].shape[0]
        assert got[nm][0] > 0 and abs(got[nm][0] - want) <= 1e-10 * want
    # order: a subset, in the caller's order; zero error gives 0
    some = list(reversed(info["order"][:2]))
    assert list(nees(truth, est, cov, order=some)) == some
    assert all(v == (0.0, cov[nm].shape[0]) for nm, v in nees(est, est, cov).items())
    with pytest.raises(ValueError, match="no covariance"):
        nees(truth, est, cov, order=[fg.pose_variables[0][1].name])


def _truth_2d(fg):
    from refine_batch_helpers import noisy_truth

    return noisy_truth(fg, 0, 0.0, 0.0)


def test_nees_3d_error_is_in_the_retraction_of_the_estimate():
    rng = np.random.default_rng(7)
    for angle in (1e-9, 0.03, 1.0, 3.0, np.pi - 1e-9):
        w = rng.normal(size=3)
        w *= angle / np.linalg.norm(w)
        Te, Tt = np.eye(4), np.eye(4)
        Te[:3, :3] = so3_exp(rng.normal(size=3))
        Te[:3, 3] = rng.normal(size=3)
        Tt[:3, :3] = Te[:3, :3] @ so3_exp(w)
        Tt[:3, 3] = Te[:3, 3] + np.array([0.3, -0.2, 0.1])
        e = pose_error(Tt, Te)
        assert np.max(np.abs(Te[:3, :3] @ so3_exp(e[:3]) - Tt[:3, :3])) <= 1e-12
        np.testing.assert_array_equal(e[3:], Tt[:3, 3] - Te[:3, 3])
    fg, est = member("3D0")
    truth = member("3D1")[1]  # (the same graph from another point: any two results of one graph will do)
    cov, info = marginal_covariances(fg, est, engine="python")
    got = nees(truth, est, cov)
    for nm in info["order"]:
        if nm in est.poses:
            e = pose_error(truth.poses[nm], est.poses[nm])
            assert np.max(np.abs(est.poses[nm][:3, :3] @ so3_exp(e[:3]) - truth.poses[nm][:3, :3])) <= 1e-12
            assert got[nm][1] == 6 and abs(got[nm][0] - float(e @ np.linalg.solve(cov[nm], e))) <= 1e-10 * got[nm][0]
        else:
            assert got[nm][1] == 3
    assert all(v[0] == 0.0 for v in nees(est, est, cov).values())
