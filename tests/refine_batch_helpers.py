"""What the batched-refinement tests share: the group, its start points, the single-graph reference runs (computed once and left
unchanged), and the properties of the fixture the tests rely on -- asserted from those single-graph runs and from the patterns,
never from the batch code.

The 2-D group is small but meets every boundary of the device code: members of different sizes whose boundaries fall inside a
64-row product tile of the unpadded layout, a member smaller than one tile (C), a member with a landmark row beyond the
128-entry long-row limit (D) beside members without one, members that reject steps (linear_solves > iterations) and members
that stop after different numbers of iterations."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from score_amd import compat
from score_amd.manhattan import make_manhattan, make_manhattan_3d
from score_amd.refine import _initial_point, _Problem, _Problem3D, refine_estimate, so3_exp

MILD = (0.02, 0.1)    # sigma_theta, sigma_t of the start point around the truth
ROUGH = (0.6, 1.5)
TILE_ROWS, LONG_ROW = 64, 128  # of the product's tiles (csrc/score_marginals.hpp: kMvRows, kMvLongRow; mv_tiles cuts a member's too)

SPECS_2D = {
    "A": dict(seed=5, n_robots=3, n_poses=40, n_beacons=3, p_range=0.4, n_loop_closures=4),
    "B": dict(seed=9, n_robots=2, n_poses=25, n_beacons=2, p_range=0.5, n_loop_closures=3),
    "C": dict(seed=11, n_robots=1, n_poses=12, n_beacons=2, p_range=0.6),
    "D": dict(seed=13, n_robots=4, n_poses=70, n_beacons=1, p_range=0.3),
    "E": dict(seed=17, n_robots=2, n_poses=33, n_beacons=1, p_range=0.5, n_loop_closures=2),
}
KEYS_2D = tuple(SPECS_2D)
NOISE_2D = {k: (MILD if i % 2 == 0 else ROUGH) for i, k in enumerate(KEYS_2D)}  # the members alternate
SPEC_3D = dict(seed=41, n_robots=2, n_poses=25, n_beacons=3, p_range=0.5, n_loop_closures=3)
SEEDS_3D = (0, 1)


def noisy_truth(fg, seed, sigma_theta, sigma_t):
    """refine_robust_helpers.noisy_truth with the noise levels as arguments."""
    rng = np.random.default_rng(seed)
    names = [p.name for ch in fg.pose_variables for p in ch]
    T = np.tile(np.eye(3), (len(names), 1, 1))
    i = 0
    for ch in fg.pose_variables:
        for p in ch:
            th = p.true_theta + sigma_theta * rng.normal()
            T[i, :2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
            T[i, :2, 2] = np.asarray(p.true_position) + sigma_t * rng.normal(size=2)
            i += 1
    lms = np.array([np.asarray(l.true_position) + sigma_t * rng.normal(size=2) for l in fg.landmark_variables]).reshape(-1, 2)
    vals = compat.VariableValues(2, compat.ArrayDict(names, T), compat.ArrayDict([l.name for l in fg.landmark_variables], lms), None)
    return compat.SolverResults(variables=vals, total_time=0.0, solved=True, pose_chain_names=fg.get_pose_chain_names(),
                                solver_cost=0.0, info={})


def noisy_truth3(fg, seed):
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


@functools.lru_cache(maxsize=None)
def member(key):
    """(graph, start) of a member: "A".."E" (2-D), "3D0" / "3D1" (the 3-D graph from two start points)."""
    if key.startswith("3D"):
        fg = make_manhattan_3d(**SPEC_3D)
        return fg, noisy_truth3(fg, SEEDS_3D[int(key[2:])])
    fg = make_manhattan(**SPECS_2D[key])
    return fg, noisy_truth(fg, SPECS_2D[key]["seed"], *NOISE_2D[key])


def group(keys):
    return [member(k)[0] for k in keys], [member(k)[1] for k in keys]


def rough_start(key):
    """A second start point of a 2-D member, at the rough level (handle reuse, the group around a member at its optimum)."""
    fg = member(key)[0]
    return noisy_truth(fg, 1000 + SPECS_2D[key]["seed"], *ROUGH)


@functools.lru_cache(maxsize=None)
def twin_alone(key):
    """``refine_estimate(engine="python", linear_solver="scipy")`` on the member alone: (results, info, sparse-LU solves)."""
    fg, start = member(key)
    solves = [0]
    real = spla.splu

    def counted(*a, **k):
        solves[0] += 1
        return real(*a, **k)

    spla.splu = counted  # (refine.py calls spla.splu: the module attribute, looked up at every call)
    try:
        res, info = refine_estimate(fg, start, engine="python", linear_solver="scipy")
    finally:
        spla.splu = real
    return res, info, solves[0]


_native_cache = {}


def native_alone(key, lib_path):
    """``refine_estimate(engine="native")`` (one handle, one graph) on the member: (results, info); computed once."""
    if (key, lib_path) not in _native_cache:
        fg, start = member(key)
        _native_cache[(key, lib_path)] = refine_estimate(fg, start, engine="native", lib_path=lib_path)
    return _native_cache[(key, lib_path)]


@functools.lru_cache(maxsize=None)
def row_lengths(key):
    """Entries per row of the pattern of J'J (diagonal included) of a member."""
    fg, start = member(key)
    if fg.dimension == 3:
        prob = _Problem3D(fg)
        point = prob.initial_state(start)
    else:
        prob = _Problem(fg)
        point = _initial_point(prob, start)
    _, J = prob.residuals(point, jac=True)
    ones = J.copy()
    ones.data[:] = 1.0
    pat = (ones.T @ ones + sp.identity(prob.n, format="csr")).tocsr()
    return np.diff(pat.indptr)


@functools.lru_cache(maxsize=None)
def check_fixture():
    """The properties the tests rely on; returns the figures (printed by the tests that use them)."""
    runs = {k: twin_alone(k) for k in KEYS_2D}
    its = {k: runs[k][1]["iterations"] for k in KEYS_2D}
    solves = {k: runs[k][2] for k in KEYS_2D}
    for k in KEYS_2D:
        assert its[k] < 50, f"{k}: the reference run meets max_iters"
        assert runs[k][1]["cost_final"] <= runs[k][1]["cost_initial"]
    assert len(set(its.values())) > 1, f"iteration counts do not differ between members: {its}"
    assert any(solves[k] > its[k] for k in KEYS_2D), f"no member rejects a step: solves {solves}, iterations {its}"
    longest = {k: int(row_lengths(k).max()) for k in KEYS_2D}
    assert any(v > LONG_ROW for v in longest.values()) and any(v <= LONG_ROW for v in longest.values()), longest
    assert longest["D"] > LONG_ROW, longest
    sizes = [len(row_lengths(k)) for k in KEYS_2D]
    assert sizes[KEYS_2D.index("C")] < TILE_ROWS
    bounds = np.cumsum(sizes)[:-1]
    assert np.all(bounds % TILE_ROWS != 0), f"a member boundary falls on a tile boundary: {bounds}"
    return {"iterations": its, "solves": solves, "longest_row": longest, "unknowns": dict(zip(KEYS_2D, sizes))}


def arrays_of(fg, res):
    """(poses stacked, landmarks stacked) of a SolverResults in the graph's own order."""
    P = np.array([np.asarray(res.poses[p.name]) for ch in fg.pose_variables for p in ch])
    d = fg.dimension
    L = np.array([np.asarray(res.landmarks[l.name]) for l in fg.landmark_variables]).reshape(-1, d)
    return P, L
