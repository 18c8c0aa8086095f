"""Marginal covariances (score_amd/marginals.py): what runs without a GPU -- the dense engine on the analytic two-pose
graph, the selection of variables and the argument errors.  The device path is tests/test_marginals_gpu.py."""
import numpy as np
import pytest

from marginals_helpers import graph_a, noisy_truth, two_pose_graph
from score_amd.marginals import marginal_covariances


def test_analytic_two_pose_covariance():
    kappa, tau = 7.0, 3.0
    fg = two_pose_graph(kappa, tau)
    cov, info = marginal_covariances(fg, noisy_truth(fg), engine="python")
    assert info["order"] == ["A1"] and list(cov) == ["A1"]
    expect = np.diag([1.0 / (2.0 * tau), 1.0 / kappa, 1.0 / kappa])
    np.testing.assert_allclose(cov["A1"], expect, rtol=1e-12, atol=1e-12 * expect.max())


def test_argument_errors():
    fg = graph_a()
    res = noisy_truth(fg)
    first = fg.pose_variables[0][0].name
    other = fg.pose_variables[1][3].name
    with pytest.raises(ValueError, match="fixed first pose"):
        marginal_covariances(fg, res, [first], engine="python")
    with pytest.raises(ValueError, match="unknown variable"):
        marginal_covariances(fg, res, ["no_such_variable"], engine="python")
    with pytest.raises(ValueError, match="twice"):
        marginal_covariances(fg, res, [other, other], engine="python")
    with pytest.raises(ValueError, match="range_weights"):
        marginal_covariances(fg, res, [other], range_weights=np.ones(len(fg.range_measurements) + 1), engine="python")
    with pytest.raises(ValueError, match="engine"):
        marginal_covariances(fg, res, [other], engine="host")


@pytest.mark.parametrize("width", [-1, 17, 2.5])
def test_block_width_outside_0_to_16_is_refused(width):
    fg = two_pose_graph()
    with pytest.raises(ValueError, match="block_width"):
        marginal_covariances(fg, noisy_truth(fg), block_width=width, engine="python")


def test_default_variables_and_joint():
    fg = graph_a()
    res = noisy_truth(fg)
    cov, info = marginal_covariances(fg, res, joint=True, engine="python")
    want = [l.name for l in fg.landmark_variables] + [ch[-1].name for ch in fg.pose_variables]
    assert info["order"] == want and list(cov) == want
    sizes = [cov[nm].shape[0] for nm in want]
    assert sizes == [2, 2, 3, 3]
    J = info["joint"]
    assert J.shape == (sum(sizes), sum(sizes))
    np.testing.assert_array_equal(J, J.T)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for k, nm in enumerate(want):
        np.testing.assert_array_equal(J[off[k]:off[k + 1], off[k]:off[k + 1]], cov[nm])
        assert np.all(np.linalg.eigvalsh(cov[nm]) > 0)
    # a marginal does not depend on what else is selected
    alone, _ = marginal_covariances(fg, res, [want[2]], engine="python")
    np.testing.assert_allclose(alone[want[2]], cov[want[2]], rtol=1e-12)
