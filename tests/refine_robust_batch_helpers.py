"""What the batched robust-refinement tests share: the graphs of tests/refine_robust_helpers.py plus one clean 3-D graph, the
schedules they were checked with, and the single-graph runs of the Python engine (computed once, and left unchanged)."""
import functools

import numpy as np

from refine_robust_helpers import THRESHOLD as _THRESHOLD, graph as _graph, start_of
from score_amd.manhattan import make_manhattan, make_manhattan_3d

CLEAN3 = "S43"  # the clean 3-D graph
THRESHOLD = dict(_THRESHOLD, **{CLEAN3: 5.0})
SCHEDULE = {"G1": {}, "G2": {}, "G4": {}, "G3": dict(max_iters=3, inner_iters=3), CLEAN3: dict(max_iters=3, inner_iters=3)}
# outer solves / LM iterations of the Python engine with SciPy's LU, both families on
OUTER = {"G1": 33, "G2": 26, "G3": 17, "G4": 1, CLEAN3: 1}
LM_ITERATIONS = {"G1": 211, "G2": 168, "G3": 54}


@functools.lru_cache(maxsize=None)
def graph(key):
    """(fg, start, planted ranges, which of them are long, planted loop closures); nothing in it is modified afterwards."""
    if key != CLEAN3:
        return _graph(key)
    fg = make_manhattan_3d(seed=43, n_robots=2, n_poses=20, n_beacons=3, p_range=0.5, n_loop_closures=2)
    return fg, start_of(fg), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def second_start(key):
    """Another start point of a 2-D graph."""
    from refine_robust_helpers import noisy_truth

    return noisy_truth(graph(key)[0], seed=1)


@functools.lru_cache(maxsize=None)
def wide_member():
    """A member with more than 256 ranges + loop closures: two workgroups of the robust kernels."""
    fg = make_manhattan(seed=3, n_robots=3, n_poses=60, n_beacons=3, p_range=0.6, n_loop_closures=4)
    return fg, start_of(fg)


_single = {}


def single(key, engine="python", lib_path=None, **kw):
    """``refine_estimate_robust`` on graph ``key`` alone, both families on, at the graph's threshold and schedule."""
    from score_amd.refine_robust import refine_estimate_robust

    at = (key, engine, lib_path, tuple(sorted(kw.items())))
    if at not in _single:
        fg, start, *_ = graph(key)
        args = dict(inlier_threshold=THRESHOLD[key], robust_loop_closures=True, engine=engine, lib_path=lib_path,
                    linear_solver="scipy" if engine == "python" else "device", **SCHEDULE[key])
        args.update(kw)
        _single[at] = refine_estimate_robust(fg, start, **args)
    return _single[at]


def batch(keys, engine="python", lib_path=None, **kw):
    from score_amd.refine_robust_batch import refine_estimate_robust_batch

    schedule = SCHEDULE[keys[0]]
    assert all(SCHEDULE[k] == schedule for k in keys if graph(k)[0].dimension == graph(keys[0])[0].dimension)
    args = dict(inlier_threshold=[THRESHOLD[k] for k in keys], robust_loop_closures=True, engine=engine, lib_path=lib_path, **schedule)
    args.update(kw)
    return refine_estimate_robust_batch([graph(k)[0] for k in keys], [graph(k)[1] for k in keys], **args)


def poses_of(fg, res):
    return np.array([np.asarray(res.poses[p.name]) for ch in fg.pose_variables for p in ch])


def landmarks_of(fg, res):
    return np.array([np.asarray(res.landmarks[l.name]) for l in fg.landmark_variables]).reshape(len(fg.landmark_variables), -1)


@functools.lru_cache(maxsize=None)
def pinned_member():
    """G2's graph with range 0 and loop closure 1 re-attached to pose 0, the pinned pose."""
    from refine_robust_helpers import corrupt

    fg = make_manhattan(seed=9, n_robots=2, n_poses=25, n_beacons=2, p_range=0.5, n_loop_closures=3)
    corrupt(fg, 9, (0,))
    first = fg.pose_variables[0][0].name
    m = fg.range_measurements[0]
    m.association = (first, m.association[1])
    fg.loop_closure_measurements[1].base_pose = first
    return fg, start_of(fg)


@functools.lru_cache(maxsize=None)
def sparse_members():
    """Members without loop closures, without ranges, and with neither."""
    fgs = [make_manhattan(seed=2, n_robots=2, n_poses=15, n_beacons=2, p_range=0.5, n_loop_closures=0),
           make_manhattan(seed=2, n_robots=2, n_poses=15, n_beacons=0, p_range=0.0, n_loop_closures=2),
           make_manhattan(seed=4, n_robots=2, n_poses=12, n_beacons=0, p_range=0.0, n_loop_closures=0)]
    return [(fg, start_of(fg)) for fg in fgs]
