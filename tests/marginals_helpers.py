"""What the marginal-covariance tests share: the graphs, the points, the dense reference and the derived bound.

For a column c the library gives x_c on the rows of S and its residual rho_c = |e_c - H x_c|_2.  The reference is the
Cholesky solve x_ref of the dense H = J'J from the Python Jacobian at the same point, with its own residual rho_ref
(computed in np.longdouble).  A residual computed in double carries the rounding
delta_c = (longest row + 1) eps || |H| |x_ref| ||_2, so H (x_c - x_ref) = (e_c - H x_ref) - (e_c - H x_c) gives

    || (x_c - x_ref)[S] ||_2  <=  || x_c - x_ref ||_2  <=  (rho_c + delta_c + rho_ref) / lambda_min(H).

Every term is computed here; no tolerance is chosen."""
import functools

import numpy as np
import scipy.linalg as sla

from score_amd import compat
from score_amd.manhattan import make_manhattan, make_manhattan_3d
from score_amd.marginals import _problem_and_point, _select, dense_information
from score_amd.refine import so3_exp

EPS = np.finfo(np.float64).eps


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


def two_pose_graph(kappa=7.0, tau=3.0):
    """One chain of two poses, odometry only: the covariance of pose 1 in (theta, x, y) is diag(1/(2 tau), 1/kappa, 1/kappa)
    (|dR/dtheta|_F^2 = 2, and the translation residual does not depend on theta_1)."""
    fg = compat.FactorGraphData(dimension=2)
    fg.pose_variables = [[compat.PoseVariable2D("A0", (0.0, 0.0), 0.0), compat.PoseVariable2D("A1", (1.0, 0.5), 0.3)]]
    fg.odom_measurements = [[compat.PoseMeasurement2D("A0", "A1", 1.0, 0.5, 0.3, kappa, tau)]]
    return fg


def pose_names(fg):
    return [[p.name for p in ch] for ch in fg.pose_variables]


def landmark_names(fg):
    return [l.name for l in fg.landmark_variables]


def graph_a():
    fg = make_manhattan(n_robots=2, n_poses=25, n_beacons=2, seed=9, p_range=0.5, n_loop_closures=3)
    lm = fg.landmark_variables[0]
    fg.landmark_priors = [compat.LandmarkPrior2D(lm.name, (lm.true_position[0] + 0.2, lm.true_position[1] - 0.1), 2.0)]
    return fg


def graph_b():
    return make_manhattan(n_robots=1, n_poses=300, n_beacons=1, seed=3, p_range=1.0)


def graph_c():
    return make_manhattan(n_robots=1, n_poses=1100, n_beacons=2, seed=4, p_range=0.3)


def graph_d():
    fg = make_manhattan_3d(n_robots=2, n_poses=25, n_beacons=3, seed=41, p_range=0.5, sigma_t=0.05, sigma_theta=0.02)
    fg.landmark_priors = [compat.LandmarkPrior3D(fg.landmark_variables[1].name, (1.0, 2.0, -1.0), 0.5)]
    return fg


def undetermined_graph():
    return make_manhattan(n_robots=1, n_poses=1, n_beacons=1, seed=3, p_range=1.0)


GRAPHS = {"a": graph_a, "b": graph_b, "c": graph_c, "d": graph_d}


class Reference:
    """The dense H at the test's point, its Cholesky factor, lambda_min and the longest row: computed once per graph (and
    weight vector) and left unchanged."""

    def __init__(self, fg, results, range_weights=None):
        self.prob, self.point = _problem_and_point(fg, results, range_weights, None)
        self.H = dense_information(self.prob, self.point)
        self.H.setflags(write=False)
        self.n = self.prob.n
        self.chol = sla.cho_factor(self.H, lower=True)
        self.lambda_min = float(sla.eigvalsh(self.H, subset_by_index=[0, 0])[0])
        assert self.lambda_min > 0
        self.longest_row = int(np.max(np.count_nonzero(self.H, axis=1)))
        self.absH = np.abs(self.H)

    def columns(self, variables):
        """(names, unknowns of the variables) in the library's order."""
        names, _, _, cols = _select(self.prob, variables)
        return names, cols

    def solve(self, cols):
        """x_ref (n x C), rho_ref (C, from np.longdouble), delta (C)."""
        E = np.zeros((self.n, len(cols)))
        E[cols, np.arange(len(cols))] = 1.0
        X = sla.cho_solve(self.chol, E)
        R = E.astype(np.longdouble) - self.H.astype(np.longdouble) @ X.astype(np.longdouble)
        rho_ref = np.sqrt(np.sum(R * R, axis=0)).astype(np.float64)
        delta = (self.longest_row + 1) * EPS * np.linalg.norm(self.absH @ np.abs(X), axis=0)
        return X, rho_ref, delta


@functools.lru_cache(maxsize=None)
def reference(key):
    fg = GRAPHS[key]()
    results = noisy_truth3(fg) if fg.dimension == 3 else noisy_truth(fg)
    return fg, results, Reference(fg, results)


def check_columns(ref, cols, A, rho, label):
    """The bound of the module's docstring for every column of A (C x C: column c is the library's x_c on the rows `cols`).
    Prints and returns the figures profiles/r11_marginals.json records."""
    X, rho_ref, delta = ref.solve(cols)
    err = np.linalg.norm(A - X[cols, :], axis=0)
    bound = (np.asarray(rho) + delta + rho_ref) / ref.lambda_min
    sigma_max = float(np.max(np.abs(X[cols, :])))
    diag_ref = np.diag(X[cols, :])
    figures = {
        "graph": label, "n": int(ref.n), "columns": int(len(cols)), "lambda_min": ref.lambda_min, "longest_row": ref.longest_row,
        "worst_bound_over_max_sigma": float(np.max(bound) / sigma_max),
        "worst_error_over_max_sigma": float(np.max(err) / sigma_max),
        "worst_diag_rel_error": float(np.max(np.abs(np.diag(A) - diag_ref) / np.abs(diag_ref))),
        "worst_residual": float(np.max(rho)),
    }
    print(figures)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"{label}: column {worst}: error {err[worst]:.3e} > bound {bound[worst]:.3e}"
    return figures, bound, delta


def check_iteration_caps(run, label):
    """The chunk boundaries of the queued iteration (16 iterations, then 32 at a time, never beyond max_iters).
    ``run(max_iters)`` -> (return code, [(A, residuals, steps, converged), ...]) on ONE handle.  The full run converges
    everywhere with step counts s; under a cap below max(s) -- max(s) - 1, and 16 and 17 where they are below max(s) -- a
    column with s_c <= cap is the full run's bit for bit, one beyond it reports -(cap + 1) and the call returns 1."""
    rc, full = run(4000)
    assert rc == 0 and all(np.all(conv) for *_, conv in full), f"{label}: the full run did not converge"
    top = max(int(steps.max()) for _, _, steps, _ in full)
    caps = sorted({top - 1} | {c for c in (16, 17) if c < top})
    print(f"{label}: max(s) = {top}, caps {caps}, steps {[steps.tolist() for _, _, steps, _ in full]}")
    assert caps[0] >= 1
    for cap in caps:
        rc_c, capped = run(cap)
        assert rc_c == 1, f"{label}, cap {cap}: return code {rc_c}"
        for (A, res, steps, _), (A_c, res_c, steps_c, conv_c) in zip(full, capped):
            reported = np.where(conv_c, steps_c, -(steps_c + 1))  # (what the C entry point wrote)
            within = steps <= cap
            assert np.array_equal(reported[within], steps[within]), f"{label}, cap {cap}: {reported} against {steps}"
            assert np.all(reported[~within] == -(cap + 1)), f"{label}, cap {cap}: {reported} against {steps}"
            assert np.array_equal(A_c[:, within], A[:, within]) and np.array_equal(res_c[within], res[within])
    return top
