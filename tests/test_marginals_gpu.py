"""Marginal covariances on the device (score_refine_marginals, csrc/score_marginals.hpp) against the dense Cholesky
reference, under the bound derived in tests/marginals_helpers.py: every term of it is computed from the reference, the
library's own reported residual and the number format -- no tolerance is chosen."""
import numpy as np
import pytest

from marginals_helpers import (check_columns, check_iteration_caps, graph_a, landmark_names, noisy_truth, pose_names, reference,
                               two_pose_graph, undetermined_graph, Reference)
from refine_batch_helpers import member, twin_alone
from score_amd.marginals import MarginalsHandle, _problem_and_point, _select, device_columns, marginal_covariances

pytestmark = pytest.mark.gpu


def _device(label, fg, results, ref, variables, **kw):
    """The library's columns for `variables` (names) checked against the reference; returns what the checks need."""
    cov, info = marginal_covariances(fg, results, variables, joint=True, **kw)
    names, cols = ref.columns(variables)
    assert info["order"] == names
    A = info["joint_raw"]
    assert A.shape == (len(cols), len(cols))
    figures, bound, delta = check_columns(ref, cols, A, info["residuals"], label)
    return cov, info, cols, A, bound, delta


def test_analytic_two_pose_graph_on_the_device(hip_lib):
    kappa, tau = 7.0, 3.0
    fg = two_pose_graph(kappa, tau)
    results = noisy_truth(fg)
    ref = Reference(fg, results)
    # n = 3: one block of 3 columns padded to the width
    cov, info, cols, A, bound, _ = _device("two poses", fg, results, ref, None)
    assert info["batches"] == 1 and len(cols) == 3 and list(cov) == ["A1"]
    # ... and the reference is the analytic covariance (H is diagonal: 2 tau, kappa, kappa)
    expect = np.diag([1.0 / (2.0 * tau), 1.0 / kappa, 1.0 / kappa])
    np.testing.assert_allclose(ref.solve(cols)[0], expect, rtol=1e-12, atol=1e-12 * expect.max())


def test_all_variables_of_graph_a(hip_lib):
    fg, results, ref = reference("a")
    everything = [nm for ch in pose_names(fg) for nm in ch][1:] + landmark_names(fg)
    cov, info, cols, A, bound, delta = _device("a", fg, results, ref, everything)
    assert len(cols) == ref.n == 151 and info["batches"] == 10  # the last block holds 7 live columns
    # all rows are selected: the reported residual is |e_c - H x_c|_2 of the dense H, to the rounding of that product
    mine = np.linalg.norm(np.eye(ref.n)[:, cols] - ref.H[:, cols] @ A, axis=0)
    print("residual recomputation: worst |reported - recomputed| / delta =", float(np.max(np.abs(info["residuals"] - mine) / delta)))
    assert np.all(np.abs(info["residuals"] - mine) <= delta)
    # H^-1 is symmetric: what is left of A - A' is the two columns' errors
    asym = np.abs(A - A.T)
    assert np.all(asym <= bound[:, None] + bound[None, :])
    assert info["asymmetry"] == float(asym.max())
    # narrower blocks and the sequential single-right-hand-side path obey the same rule
    for width in (4, 0):
        cov_w, info_w, _, A_w, _, _ = _device(f"a, width {width}", fg, results, ref, everything, block_width=width)
        assert info_w["batches"] == (38 if width == 4 else 151)
        for nm in cov:
            assert cov_w[nm].shape == cov[nm].shape


def test_split_long_row(hip_lib):
    fg, results, ref = reference("b")
    assert ref.longest_row == 600  # the beacon's rows: beyond kMvLongRow, one workgroup per row
    poses = pose_names(fg)[0]
    cov, info, cols, *_ = _device("b", fg, results, ref, landmark_names(fg) + [poses[1], poses[150], poses[299]])
    assert len(cols) == 11 and info["batches"] == 1


def test_chain_beyond_the_second_level(hip_lib):
    fg, results, ref = reference("c")  # 1100 poses: the chain is segmented (score_join.hpp), applied to 16 vectors at once
    poses = pose_names(fg)[0]
    cov, info, cols, *_ = _device("c", fg, results, ref, landmark_names(fg) + [poses[550], poses[1099]])
    assert len(cols) == 10


def test_3d_graph_and_joint(hip_lib):
    fg, results, ref = reference("d")
    cov, info, cols, A, *_ = _device("d", fg, results, ref, None)
    want = landmark_names(fg) + [ch[-1] for ch in pose_names(fg)]
    assert info["order"] == want
    assert [cov[nm].shape for nm in want] == [(3, 3)] * 3 + [(6, 6)] * 2
    off = np.concatenate([[0], np.cumsum([cov[nm].shape[0] for nm in want])])
    for k, nm in enumerate(want):
        np.testing.assert_array_equal(info["joint"][off[k]:off[k + 1], off[k]:off[k + 1]], cov[nm])


def test_range_weights(hip_lib):
    fg = graph_a()
    results = noisy_truth(fg)
    w = np.ones(len(fg.range_measurements))
    w[[1, 5, 9]] = 0.0
    ref = Reference(fg, results, range_weights=w)
    plain = reference("a")[2]
    assert np.max(np.abs(ref.H - plain.H)) > 1e-3  # the three ranges matter
    _device("a, three ranges off", fg, results, ref, None, range_weights=w)


def test_iteration_cap_at_the_chunk_boundaries(hip_lib):
    """Member A of tests/refine_batch_helpers.py at width 4 under max_iters at and around the boundaries of the queued
    chunks: see check_iteration_caps."""
    prob, point = _problem_and_point(member("A")[0], twin_alone("A")[0], None, None)
    ids = _select(prob, None)[1]

    def run(cap):
        rc, A, res, steps, converged, _ = h.columns(point, ids, max_iters=cap, block_width=4)
        return rc, [(A, res, steps, converged)]

    with MarginalsHandle(prob, hip_lib) as h:
        check_iteration_caps(run, "A, width 4")


def test_undetermined_variable_is_a_verdict(hip_lib):
    fg = undetermined_graph()  # one range fixes the landmark's distance only: H is singular
    results = noisy_truth(fg)
    lm = landmark_names(fg)[0]
    with pytest.raises(RuntimeError, match=lm):
        marginal_covariances(fg, results, max_iters=50)
    prob, point = _problem_and_point(fg, results, None, None)
    _, ids, _, _ = _select(prob, None)
    rc, A, res, steps, converged, info = device_columns(prob, point, ids, max_iters=50)
    assert rc == 1 and info["unconverged"] > 0 and not np.all(converged) and np.all(steps <= 50)
    # the process goes on: a well-posed call on the same library
    fg2, results2, ref2 = reference("a")
    _device("a, after the singular call", fg2, results2, ref2, None)
