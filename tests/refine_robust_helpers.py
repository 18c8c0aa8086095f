"""What the robust-refinement tests share: the graphs with their planted outliers, the start points, the Python twin's runs
(computed once per graph and linear solver, and left unchanged)."""
import functools

import numpy as np

from score_amd import compat
from score_amd.manhattan import make_manhattan, make_manhattan_3d
from score_amd.refine import so3_exp


def noisy_truth(fg, seed=0):
    rng = np.random.default_rng(seed)
    names = [p.name for ch in fg.pose_variables for p in ch]
    T = np.tile(np.eye(3), (len(names), 1, 1))
    i = 0
    for ch in fg.pose_variables:
        for p in ch:
            th = p.true_theta + 0.02 * rng.normal()
            T[i, :2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
            T[i, :2, 2] = np.asarray(p.true_position) + 0.1 * rng.normal(size=2)
            i += 1
    lms = np.array([np.asarray(l.true_position) + 0.1 * rng.normal(size=2) for l in fg.landmark_variables]).reshape(-1, 2)
    vals = compat.VariableValues(2, compat.ArrayDict(names, T), compat.ArrayDict([l.name for l in fg.landmark_variables], lms), None)
    return compat.SolverResults(variables=vals, total_time=0.0, solved=True, pose_chain_names=fg.get_pose_chain_names(),
                                solver_cost=0.0, info={})


def noisy_truth3(fg, seed=0):
    rng = np.random.default_rng(seed)
    names = [p.name for ch in fg.pose_variables for p in ch]
    T = np.tile(np.eye(4), (len(names), 1, 1))
    for i, p in enumerate(q for ch in fg.pose_variables for q in ch):
        T[i, :3, :3] = p.rotation_matrix @ so3_exp(0.03 * rng.normal(size=3))
        T[i, :3, 3] = np.asarray(p.true_position) + 0.1 * rng.normal(size=3)
    lms = np.array([np.asarray(l.true_position) + 0.1 * rng.normal(size=3) for l in fg.landmark_variables]).reshape(-1, 3)
    vals = compat.VariableValues(3, compat.ArrayDict(names, T), compat.ArrayDict([l.name for l in fg.landmark_variables], lms), None)
    return compat.SolverResults(variables=vals, total_time=0.0, solved=True, pose_chain_names=fg.get_pose_chain_names(),
                                solver_cost=0.0, info={})


def start_of(fg):
    return noisy_truth3(fg) if fg.dimension == 3 else noisy_truth(fg)


def corrupt(fg, seed, lc_bad=()):
    """About 10 % of the ranges of ``fg`` become outliers, in place: every second one (and every one of 8 m or less) is
    measured LONG, + U(8, 15) m, the others SHORT, x U(0.3, 0.5); the listed (2-D) loop closures become false place
    recognitions.  Returns (indices of the corrupted ranges, mask of the long ones among them)."""
    rng = np.random.default_rng(seed + 1)
    n = len(fg.range_measurements)
    bad = np.sort(rng.choice(n, size=max(2, n // 10), replace=False))
    long_ = np.zeros(len(bad), dtype=bool)
    for j, i in enumerate(bad):
        m = fg.range_measurements[i]
        if j % 2 == 0 or m.dist <= 8:
            m.dist = float(m.dist + rng.uniform(8, 15))
            long_[j] = True
        else:
            m.dist = float(m.dist * rng.uniform(0.3, 0.5))
    for k in lc_bad:
        m = fg.loop_closure_measurements[k]
        m.x, m.y = float(rng.uniform(-8, 8)), float(rng.uniform(-8, 8))
        m.theta = float(rng.uniform(-np.pi, np.pi))
    return bad, long_


def _g1():
    fg = make_manhattan(seed=5, n_robots=3, n_poses=40, n_beacons=3, p_range=0.4, n_loop_closures=4)
    bad, long_ = corrupt(fg, 5, (1,))
    return fg, bad, long_, np.array([1])


def _g2():
    fg = make_manhattan(seed=9, n_robots=2, n_poses=25, n_beacons=2, p_range=0.5, n_loop_closures=3)
    bad, long_ = corrupt(fg, 9, (0,))
    return fg, bad, long_, np.array([0])


def _g3():
    fg = make_manhattan_3d(seed=41, n_robots=2, n_poses=25, n_beacons=3, p_range=0.5, n_loop_closures=3)
    bad, long_ = corrupt(fg, 41)
    return fg, bad, long_, np.zeros(0, dtype=np.int64)


def _g4():  # no outliers: noisier ranges, a wider threshold
    fg = make_manhattan(seed=5, n_robots=3, n_poses=40, n_beacons=3, p_range=0.4, n_loop_closures=4, sigma_range=0.5)
    return fg, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int64)


_GRAPHS = {"G1": _g1, "G2": _g2, "G3": _g3, "G4": _g4}
THRESHOLD = {"G1": 3.0, "G2": 3.0, "G3": 3.0, "G4": 5.0}


@functools.lru_cache(maxsize=None)
def graph(key):
    """(fg, start, planted ranges, which of them are long, planted loop closures); nothing in it is modified afterwards."""
    fg, bad, long_, lc_bad = _GRAPHS[key]()
    return fg, start_of(fg), bad, long_, lc_bad


_twin_cache = {}


def twin(key, linear_solver="scipy", lib_path=None, **schedule):
    """The Python engine on graph ``key`` with both families on (computed once per solver, library and schedule)."""
    from score_amd.refine_robust import refine_estimate_robust

    at = (key, linear_solver, lib_path, tuple(sorted(schedule.items())))
    if at not in _twin_cache:
        fg, start, *_ = graph(key)
        _twin_cache[at] = refine_estimate_robust(fg, start, inlier_threshold=THRESHOLD[key], robust_loop_closures=True, engine="python",
                                                 linear_solver=linear_solver, lib_path=lib_path, **schedule)
    return _twin_cache[at]


def rmse_all_poses(fg, results):
    """Root mean square position error over all poses, in the frame the fixed first pose defines."""
    d = fg.dimension
    err = [np.asarray(results.poses[p.name])[:d, d] - np.asarray(p.true_position) for ch in fg.pose_variables for p in ch]
    return float(np.sqrt(np.mean(np.sum(np.square(err), axis=1))))


def point_of(fg, results, range_weights=None, loop_closure_weights=None):
    """(problem, point) of the refinement at ``results``."""
    from score_amd.marginals import _problem_and_point

    return _problem_and_point(fg, results, range_weights, loop_closure_weights)
