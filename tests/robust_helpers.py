"""Comparisons the GNC-TLS GPU tests share (test_robust_gpu.py, test_robust_loop_closures_gpu.py)."""
import numpy as np


def _poses_close(a, b, rel):
    scale = max(1.0, max(float(np.max(np.abs(T[:-1, -1]))) for T in b.poses.values()))
    worst = max(float(np.max(np.abs(a.poses[k] - b.poses[k]))) for k in b.poses) / scale
    assert worst <= rel, worst


def _bit_equal(a, b):
    for k in b.poses:
        np.testing.assert_array_equal(a.poses[k], b.poses[k])
    for k in b.landmarks:
        np.testing.assert_array_equal(a.landmarks[k], b.landmarks[k])
    np.testing.assert_array_equal(a.relaxed_poses.array, b.relaxed_poses.array)
