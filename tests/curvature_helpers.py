"""What the curvature tests share: the graphs and points, an independent reference for E = half the Hessian of the cost, the
entrywise bound, and the checks A-D of the device tests restated for an indefinite matrix.

Reference.  The cost F is written again here from ``graph_arrays`` alone, in torch float64, as a function of a step x around
the point: 2-D (theta, x, y) + x, 3-D R matrix_exp(hat(omega)), t + v, a landmark + its step; the first pose has no step.
``E_ref = torch.autograd.functional.hessian(F, 0) / 2``, dense, for n <= DENSE_LIMIT.  Nothing of score_amd's Jacobians or
curvature formulas is used.  Beyond DENSE_LIMIT the reference eigenpairs are ``eigsh`` of ``sparse_hessian``, shift-inverted
below a Gershgorin bound of its spectrum.

Bound.  Every entry of E is a sum of per-measurement contributions sum_q J_qa J_qb + sum_q r_q (grad^2 r_q)_ab.  With the
residual rows' own first and second derivatives (torch again, per measurement in its local unknowns)
    B_ab = sum over measurements of ( sum_q |J_qa| |J_qb| + sum_q |r_q| |(grad^2 r_q)_ab| ),
``count_ab`` = the measurements that contribute to the entry, and c = max count + 128 (the sums inside one contribution are
at most 12 products long, the trigonometric and square-root evaluations a few ulps each), two evaluations of E in double
differ by at most c eps B entrywise.  Everything is computed on the spot; no tolerance is chosen.
"""
import functools

import numpy as np
import scipy.sparse.linalg as spla
import torch

from marginals_helpers import noisy_truth, noisy_truth3
from spectrum_helpers import DENSE_LIMIT, EPS, GRAPHS as SPECTRUM_GRAPHS, MAX_ITERS, REL_TOL, SHIFT  # noqa: F401
from score_amd import compat
from score_amd.curvature import sparse_hessian
from score_amd.marginals import _problem_and_point
from score_amd.native import graph_arrays
from score_amd.refine import _Problem3D, _point_arrays, refine_estimate

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# graphs and points
# ---------------------------------------------------------------------------------------------------------------------
def graph_line():
    """One robot, 20 poses at (i, 0) heading 0, exact odometry (1, 0, 0) with precisions 1e4 / 2.5e5, one landmark L0 at
    (7.3, 3.0), one range per pose with noise 0.3 rng.normal() (default_rng(0), in pose order) and precision 1."""
    rng = np.random.default_rng(0)
    fg = compat.FactorGraphData(dimension=2)
    fg.pose_variables = [[compat.PoseVariable2D(f"A{i}", (float(i), 0.0), 0.0) for i in range(20)]]
    fg.odom_measurements = [[compat.PoseMeasurement2D(f"A{i}", f"A{i + 1}", 1.0, 0.0, 0.0, 1e4, 2.5e5) for i in range(19)]]
    fg.landmark_variables = [compat.LandmarkVariable2D("L0", (7.3, 3.0))]
    fg.range_measurements = [compat.FGRangeMeasurement((f"A{i}", "L0"), float(np.hypot(i - 7.3, 3.0) + 0.3 * rng.normal()), 1.0)
                             for i in range(20)]
    return fg


def line_start(fg):
    """The true poses with L0 at (7.0, 0.0): on the line of the poses, where the reflection y -> -y maps the problem to itself."""
    names = [p.name for p in fg.pose_variables[0]]
    T = np.tile(np.eye(3), (len(names), 1, 1))
    T[:, 0, 2] = np.arange(len(names), dtype=np.float64)
    vals = compat.VariableValues(2, compat.ArrayDict(names, T), compat.ArrayDict(["L0"], np.array([[7.0, 0.0]])), None)
    return compat.SolverResults(variables=vals, total_time=0.0, solved=True, pose_chain_names=fg.get_pose_chain_names(),
                                solver_cost=0.0, info={})


def host_refined(fg, results):
    return refine_estimate(fg, results, engine="python", linear_solver="scipy")


def noise_free(fg):
    """(fg, results): the graph with every measurement replaced by what its true poses and landmarks give (the precisions
    stay), and the truth as the point: every residual is zero there, to rounding."""
    d = fg.dimension
    poses = {p.name: p for ch in fg.pose_variables for p in ch}
    names = list(poses)
    T = np.tile(np.eye(d + 1), (len(names), 1, 1))
    for i, p in enumerate(poses.values()):
        th = getattr(p, "true_theta", None)
        T[i, :d, :d] = p.rotation_matrix if d == 3 else [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
        T[i, :d, d] = np.asarray(p.true_position, dtype=np.float64)
    frame = dict(zip(names, T))
    where = {nm: M[:d, d] for nm, M in frame.items()}
    where.update({l.name: np.asarray(l.true_position, dtype=np.float64) for l in fg.landmark_variables})
    for m in [m for ch in fg.odom_measurements for m in ch] + list(fg.loop_closure_measurements):
        rel = np.linalg.inv(frame[m.base_pose]) @ frame[m.to_pose]
        if d == 2:
            m.x, m.y, m.theta = float(rel[0, 2]), float(rel[1, 2]), float(np.arctan2(rel[1, 0], rel[0, 0]))
        else:
            m.translation, m.rotation = rel[:3, 3].copy(), rel[:3, :3].copy()
    for m in fg.range_measurements:
        m.dist = float(np.linalg.norm(where[m.association[0]] - where[m.association[1]]))
    for pr in fg.landmark_priors:
        pr.position = tuple(float(v) for v in where[pr.name])
    lms = np.array([where[l.name] for l in fg.landmark_variables]).reshape(-1, d)
    vals = compat.VariableValues(d, compat.ArrayDict(names, T), compat.ArrayDict([l.name for l in fg.landmark_variables], lms), None)
    return fg, compat.SolverResults(variables=vals, total_time=0.0, solved=True, pose_chain_names=fg.get_pose_chain_names(),
                                    solver_cost=0.0, info={})


@functools.lru_cache(maxsize=None)
def case(key):
    """(fg, results) of a named case: a graph of spectrum_helpers at noisy_truth, "2x20_refined", "line" (the symmetric
    stationary point the host solver stops at) and "line_escaped" is made by the tests themselves."""
    if key == "line":
        fg = graph_line()
        results, info = host_refined(fg, line_start(fg))
        return fg, results
    if key == "2x20_refined":
        fg = SPECTRUM_GRAPHS["2x20"]()
        results, info = host_refined(fg, noisy_truth(fg))
        return fg, results
    fg = SPECTRUM_GRAPHS[key]()
    return fg, (noisy_truth3(fg) if fg.dimension == 3 else noisy_truth(fg))


NOISY = ("2x20", "long_rows", "a", "d")             # at noisy_truth / noisy_truth3
DENSE_CASES = NOISY + ("2x20_refined", "line")      # every case with a dense reference
ALL_CASES = DENSE_CASES + ("c",)


# ---------------------------------------------------------------------------------------------------------------------
# the cost again, in torch
# ---------------------------------------------------------------------------------------------------------------------
def _hat(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


class TorchCost:
    """The residual rows of every measurement kind as functions of the LOCAL steps of the measurement's variables (a batch
    over the measurements of the kind), and F of the global step."""

    def __init__(self, fg, results, range_weights=None):
        prob, point = _problem_and_point(fg, results, range_weights, None)
        a = prob.a
        self.d = d = fg.dimension
        self.dp = dp = 3 if d == 2 else 6
        self.Np, self.Nl = len(a["pose_names"]), len(a["landmark_names"])
        self.n = dp * (self.Np - 1) + d * self.Nl
        poses, lms = _point_arrays(prob, point)  # the C layout: [theta, x, y] or [R | t] per pose
        t = lambda x, dt=F64: torch.as_tensor(np.ascontiguousarray(x), dtype=dt)  # noqa: E731
        self.poses, self.lms = t(poses), t(lms).reshape(-1, d)
        self.bi, self.tj = t(a["rel_base"], torch.long), t(a["rel_to"], torch.long)
        self.tm, self.Rm = t(a["rel_t"]).reshape(-1, d), t(a["rel_R"]).reshape(-1, d, d)
        self.sk, self.st = torch.sqrt(t(a["rel_kappa"])), torch.sqrt(t(a["rel_tau"]))
        self.ra, self.rb = t(a["rng_a"], torch.long), t(a["rng_b"], torch.long)
        self.dist, self.sw = t(a["rng_dist"]), torch.sqrt(t(prob.a["rng_prec"]))
        self.pl, self.pt = t(a["lprior_lm"], torch.long), t(a["lprior_t"]).reshape(-1, d)
        self.spw = torch.sqrt(t(a["lprior_prec"]))
        # local -> global columns; self.n marks "no unknown" (the fixed pose): it reads the zero appended to the step
        pose_cols = lambda p: torch.where(p[:, None] > 0, dp * (p[:, None] - 1) + torch.arange(dp)[None], self.n)  # noqa: E731
        self.rel_cols = torch.cat([pose_cols(self.bi), pose_cols(self.tj)], 1)

        def point_cols(v):
            first = torch.where(v < self.Np, dp * (v - 1) + (dp - d), dp * (self.Np - 1) + d * (v - self.Np))
            cols = first[:, None] + torch.arange(d)[None]
            return torch.where((v == 0)[:, None], self.n, cols)

        self.rng_cols = torch.cat([point_cols(self.ra), point_cols(self.rb)], 1)
        self.pri_cols = dp * (self.Np - 1) + d * self.pl[:, None] + torch.arange(d)[None]

    def _pose(self, idx, step):
        """(rotation (e, d, d), translation (e, d)) of the poses idx moved by their local steps (e, dp)."""
        P = self.poses[idx]
        if self.d == 2:
            th = P[:, 0] + step[:, 0]
            c, s = torch.cos(th), torch.sin(th)
            return torch.stack([torch.stack([c, -s], -1), torch.stack([s, c], -1)], -2), P[:, 1:3] + step[:, 1:3]
        return P[:, :9].reshape(-1, 3, 3) @ torch.matrix_exp(_hat(step[:, :3])), P[:, 9:12] + step[:, 3:6]

    def _point(self, idx):
        out = torch.empty((len(idx), self.d), dtype=F64)
        pose = idx < self.Np
        out[pose] = self.poses[idx[pose]][:, 1:3] if self.d == 2 else self.poses[idx[pose]][:, 9:12]
        out[~pose] = self.lms[idx[~pose] - self.Np]
        return out

    def rel(self, X):    # X (e, 2 dp) -> r (e, d + d d)
        Ri, ti = self._pose(self.bi, X[:, :self.dp])
        Rj, tj = self._pose(self.tj, X[:, self.dp:])
        rt = self.sk[:, None] * (tj - ti - torch.einsum("eij,ej->ei", Ri, self.tm))
        rR = self.st[:, None] * (Rj - Ri @ self.Rm).reshape(len(X), -1)
        return torch.cat([rt, rR], 1)

    def rng(self, X):    # X (e, 2 d) -> r (e, 1)
        dv = (self._point(self.ra) + X[:, :self.d]) - (self._point(self.rb) + X[:, self.d:])
        return (self.sw * (torch.sqrt((dv * dv).sum(1)) - self.dist))[:, None]

    def pri(self, X):    # X (e, d) -> r (e, d)
        return self.spw[:, None] * (self.lms[self.pl] + X - self.pt)

    def kinds(self):
        return [(self.rel, self.rel_cols), (self.rng, self.rng_cols), (self.pri, self.pri_cols)]

    def F(self, x):
        xx = torch.cat([x, torch.zeros(1, dtype=F64)])
        return sum((f(xx[cols]) ** 2).sum() for f, cols in self.kinds() if len(cols))

    def hessian(self):
        x0 = torch.zeros(self.n, dtype=F64)
        H = torch.autograd.functional.hessian(self.F, x0)
        return 0.5 * H.numpy()

    def parts(self):
        """(J'J, |J|'|J| + sum |r| |grad^2 r|, contributions per entry, longest row) as dense n x n arrays, from the per-row
        first and second derivatives of every measurement in its local unknowns."""
        n = self.n
        JtJ, B, count = np.zeros((n + 1, n + 1)), np.zeros((n + 1, n + 1)), np.zeros((n + 1, n + 1), dtype=np.int64)
        for f, cols in self.kinds():
            if not len(cols):
                continue
            e, L = cols.shape
            X = torch.zeros((e, L), dtype=F64, requires_grad=True)
            r = f(X)
            Q = r.shape[1]
            J = torch.zeros((e, Q, L), dtype=F64)
            Hs = torch.zeros((e, Q, L, L), dtype=F64)
            for q in range(Q):
                (g,) = torch.autograd.grad(r[:, q].sum(), X, create_graph=True)
                J[:, q] = g.detach()
                for a in range(L):
                    if g[:, a].requires_grad:
                        (h,) = torch.autograd.grad(g[:, a].sum(), X, retain_graph=True, allow_unused=True)
                        if h is not None:
                            Hs[:, q, a] = h
            Jn, Hn, rn, cn = J.numpy(), Hs.numpy(), r.detach().numpy(), cols.numpy()
            jj = np.einsum("eqa,eqb->eab", Jn, Jn)
            bb = np.einsum("eqa,eqb->eab", np.abs(Jn), np.abs(Jn)) + np.einsum("eq,eqab->eab", np.abs(rn), np.abs(Hn))
            rows, cc = np.repeat(cn, L, axis=1).ravel(), np.tile(cn, (1, L)).ravel()
            np.add.at(JtJ, (rows, cc), jj.ravel())
            np.add.at(B, (rows, cc), bb.ravel())
            np.add.at(count, (rows, cc), (bb.ravel() != 0).astype(np.int64))
        return JtJ[:n, :n], B[:n, :n], count[:n, :n]


class CurvatureReference:
    """E_ref, J'J, B and c of a case, its lowest eigenpairs and their residuals: computed once and left unchanged."""

    def __init__(self, fg, results, pairs=17):
        self.prob, self.point = _problem_and_point(fg, results, None, None)
        self.n = self.prob.n
        self.Es = sparse_hessian(self.prob, self.point).tocsc()      # (the product of the residual checks, and n > DENSE_LIMIT)
        _, J = self.prob.residuals(self.point, jac=True)
        self.Hs = (J.T @ J).tocsc()
        self.h_max = float(self.Hs.diagonal().max())
        self.longest_row = int(np.max(np.diff(self.Es.indptr)))
        if self.n <= DENSE_LIMIT:
            tc = TorchCost(fg, results)
            assert tc.n == self.n
            self.E = tc.hessian()
            self.JtJ, self.B, count = tc.parts()
            self.c = int(count.max()) + 128
            for a in (self.E, self.JtJ, self.B):
                a.setflags(write=False)
            w, V = np.linalg.eigh(0.5 * (self.E + self.E.T))
            self.values, self.vectors = w[:pairs].copy(), V[:, :pairs].copy()
            self.rho = np.linalg.norm(self.E @ self.vectors - self.vectors * self.values, axis=0)
        else:
            self.E = self.JtJ = self.B = None
            A = abs(self.Es)
            d = self.Es.diagonal()
            lower = float(np.min(d - (np.asarray(A.sum(axis=1)).ravel() - np.abs(d))))  # Gershgorin: no eigenvalue below
            w, V = spla.eigsh(self.Es, k=pairs, sigma=lower - SHIFT * self.h_max, which="LM", tol=0)
            o = np.argsort(w)
            self.values, self.vectors = w[o], V[:, o]
            self.rho = np.linalg.norm(self.Es @ self.vectors - self.vectors * self.values, axis=0)
        for a in (self.values, self.vectors, self.rho):
            a.setflags(write=False)

    def residuals(self, values, V):
        """|E v_j - lambda_j v_j|_2 with the reference's E (the dense one where it exists)."""
        E = self.E if self.E is not None else self.Es
        return np.linalg.norm(E @ V - V * values, axis=0)


@functools.lru_cache(maxsize=None)
def reference(key):
    fg, results = case(key)
    return fg, results, CurvatureReference(fg, results)


def check_input_conditions(key, ref):
    """The conditions on the fixtures: a wrong fixture cannot hide a failure."""
    if ref.E is not None and key in NOISY:
        assert np.max(np.abs(ref.E - ref.JtJ)) >= 1e-3 * np.max(np.abs(ref.JtJ)), key
    if key in ("2x20", "long_rows", "line"):
        assert ref.values[0] < -1.0, (key, ref.values[:3])
    if key == "2x20_refined":
        assert ref.values[0] > 0.15, ref.values[:3]
    if key == "line":
        assert np.linalg.eigvalsh(ref.JtJ)[0] <= 1e-9 * ref.h_max


def check_pairs(ref, k, values, V, rel_tol, label):
    """A-D of spectrum_helpers.check_modes for E: A residuals <= 2 rel_tol h_max; B Weyl, index by index; C unit norms and
    |V'V - I|_max <= 16 * 2 * rel_tol; D Davis-Kahan for the first m modes, m where the ABSOLUTE gap lambda_m - lambda_{m-1} of
    the reference is largest among the first k (the values may be negative: a relative gap has no meaning)."""
    values, V = np.asarray(values), np.asarray(V)
    assert values.shape == (k,) and V.shape == (ref.n, k)
    assert np.all(np.isfinite(values)) and np.all(np.isfinite(V))
    assert np.all(np.diff(values) >= 0), f"{label}: the values do not ascend"
    rho = ref.residuals(values, V)
    lam_ref, rho_ref = ref.values[:k], ref.rho[:k]
    err = np.abs(values - lam_ref)
    norms = np.linalg.norm(V, axis=0)
    ortho = float(np.max(np.abs(V.T @ V - np.eye(k))))
    w = ref.values
    gaps = [w[m] - w[m - 1] for m in range(1, k + 1)]
    m = 1 + int(np.argmax(gaps))
    gap = float(w[m] - w[m - 1])
    Vr, Vm = ref.vectors[:, :m], V[:, :m]
    angle = float(np.linalg.norm(Vm - Vr @ (Vr.T @ Vm), 2))
    dk = float(np.max(rho[:m]) / gap) if gap > 0 else np.inf
    figures = {"case": label, "n": int(ref.n), "k": int(k), "h_max": ref.h_max, "lowest": float(values[0]),
               "worst_rho_over_tol": float(np.max(rho) / (rel_tol * ref.h_max)),
               "worst_value_error_over_bound": float(np.max(err / (rho + rho_ref))), "ortho": ortho, "m": m, "gap": gap,
               "subspace_angle": angle, "davis_kahan": dk}
    print(figures)
    assert np.all(rho <= 2 * rel_tol * ref.h_max), f"{label}: A: residuals {rho} above {2 * rel_tol * ref.h_max:.3e}"
    worst = int(np.argmax(err - (rho + rho_ref)))
    assert np.all(err <= rho + rho_ref), f"{label}: B: mode {worst}: |{values[worst]!r} - {lam_ref[worst]!r}| > {rho[worst] + rho_ref[worst]:.3e}"
    assert np.all(np.abs(norms - 1.0) <= (ref.n + 2) * EPS), f"{label}: C: norms {norms}"
    assert ortho <= 16 * 2 * rel_tol, f"{label}: C: |V'V - I|_max = {ortho:.3e}"
    assert angle <= dk, f"{label}: D: first {m} modes: {angle:.3e} > {dk:.3e}"
    return figures, rho
