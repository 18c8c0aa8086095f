"""What the spectrum tests share: the graphs, the points, the reference eigenpairs (computed once per graph and left
unchanged) and the checks A-D of the device tests.

Reference: the dense ``eigh`` of the Python twin's H = J'J up to n = 1500, ``eigsh(H, sigma=-shift * h_max)`` beyond.
For a returned pair (lambda_j, v_j) the test recomputes rho_j = |H_host v_j - lambda_j v_j|_2, and rho_ref_j the same way for
the reference's pairs.  Then
  A  rho_j <= 2 rel_tol h_max
  B  |lambda_j - lambda_ref_j| <= rho_j + rho_ref_j                          (Weyl, index by index)
  C  | |v_j| - 1 | <= (n + 2) eps   (a unit vector rounded entry by entry, its norm summed in double: n eps at worst) and
     |V'V - I|_max <= 16 * 2 * rel_tol
  D  |(I - V_ref V_ref') V_m|_2 <= max_j rho_j / gap, the first m modes, m where the reference's relative gap
     (lambda_m - lambda_{m-1}) / lambda_m is largest, gap = lambda_m - lambda_{m-1} of the reference   (Davis-Kahan)
Every term is computed on the spot; no tolerance is chosen."""
import functools

import numpy as np
import scipy.sparse.linalg as spla

from marginals_helpers import graph_a, graph_c, graph_d, noisy_truth, noisy_truth3
from score_amd import compat
from score_amd.manhattan import make_manhattan
from score_amd.marginals import _problem_and_point

EPS = np.finfo(np.float64).eps
REL_TOL = 1e-9
SHIFT = 1e-8
MAX_ITERS = 200      # a condition of the issue, not a measurement
DENSE_LIMIT = 1500


def graph_2x20():
    return make_manhattan(n_robots=2, n_poses=20, n_beacons=2, seed=0, side=6, p_range=0.5)


def graph_degenerate():
    """2 x 20 plus a beacon L2 at (3, 4) heard once, from pose B7: its tangential direction is not determined."""
    fg = graph_2x20()
    fg.landmark_variables.append(compat.LandmarkVariable2D("L2", (3.0, 4.0)))
    b7 = next(p for ch in fg.pose_variables for p in ch if p.name == "B7")
    dist = float(np.linalg.norm(np.asarray(b7.true_position, dtype=np.float64) - np.array([3.0, 4.0])))
    fg.range_measurements.append(compat.FGRangeMeasurement(("B7", "L2"), dist + 0.05, 1.0))
    return fg


def graph_long_rows():
    return make_manhattan(n_robots=1, n_poses=150, n_beacons=2, seed=2, side=10, p_range=0.6)


GRAPHS = {"2x20": graph_2x20, "degenerate": graph_degenerate, "long_rows": graph_long_rows, "a": graph_a, "c": graph_c, "d": graph_d}


def beacon_off_weights(fg, name):
    """range_weights that zero every range of the landmark `name`."""
    return np.array([0.0 if name in (m.association[0], m.association[1]) else 1.0 for m in fg.range_measurements])


class SpectrumReference:
    def __init__(self, fg, results, range_weights=None, pairs=17):
        self.prob, self.point = _problem_and_point(fg, results, range_weights, None)
        _, J = self.prob.residuals(self.point, jac=True)
        self.Hs = (J.T @ J).tocsc()
        self.n = self.prob.n
        self.h_max = float(self.Hs.diagonal().max())
        self.longest_row = int(np.max(np.diff(self.Hs.indptr)))
        if self.n <= DENSE_LIMIT:
            self.H = np.asarray(self.Hs.todense(), dtype=np.float64)
            self.H.setflags(write=False)
            w, V = np.linalg.eigh(self.H)
            self.all_values = w
            self.values, self.vectors = w[:pairs].copy(), V[:, :pairs].copy()
        else:
            self.H = None
            self.all_values = None
            w, V = spla.eigsh(self.Hs, k=pairs, sigma=-SHIFT * self.h_max, which="LM", tol=0)
            o = np.argsort(w)
            self.values, self.vectors = w[o], V[:, o]
        self.rho = self.residuals(self.values, self.vectors)
        for a in (self.values, self.vectors, self.rho):
            a.setflags(write=False)

    def residuals(self, values, V):
        """|H v_j - lambda_j v_j|_2 with the host's H."""
        return np.linalg.norm(self.Hs @ V - V * values, axis=0)

    def gaps(self, k):
        """Distance of each of the first k reference values to the nearest other one."""
        w = self.values
        return np.array([min(abs(w[j] - w[i]) for i in range(len(w)) if i != j) for j in range(k)])


@functools.lru_cache(maxsize=None)
def reference(key):
    fg = GRAPHS[key]()
    results = noisy_truth3(fg) if fg.dimension == 3 else noisy_truth(fg)
    return fg, results, SpectrumReference(fg, results)


def check_modes(ref, k, values, V, rel_tol, label, subspace=True):
    """A (the residual part), B, C and D for the pairs (values (k), V (n x k)); prints and returns the figures."""
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
    rel_gap = [(w[m] - w[m - 1]) / w[m] if w[m] > 0 else -np.inf for m in range(1, k + 1)]
    m = 1 + int(np.argmax(rel_gap))
    gap = float(w[m] - w[m - 1])
    Vr = ref.vectors[:, :m]
    Vm = V[:, :m]
    angle = float(np.linalg.norm(Vm - Vr @ (Vr.T @ Vm), 2))
    dk = float(np.max(rho[:m]) / gap) if gap > 0 else np.inf
    figures = {
        "graph": label, "n": int(ref.n), "k": int(k), "h_max": ref.h_max,
        "worst_rho_over_tol": float(np.max(rho) / (rel_tol * ref.h_max)),
        "worst_value_error_over_bound": float(np.max(err / (rho + rho_ref))),
        "worst_value_error_over_rho": float(np.max(err / np.maximum(rho, np.finfo(float).tiny))),
        "ortho": ortho, "m": m, "gap": gap, "subspace_angle": angle, "davis_kahan": dk,
    }
    print(figures)
    assert np.all(rho <= 2 * rel_tol * ref.h_max), f"{label}: A: residuals {rho} above {2 * rel_tol * ref.h_max:.3e}"
    worst = int(np.argmax(err - (rho + rho_ref)))
    assert np.all(err <= rho + rho_ref), f"{label}: B: mode {worst}: |{values[worst]!r} - {lam_ref[worst]!r}| > {rho[worst] + rho_ref[worst]:.3e}"
    assert np.all(np.abs(norms - 1.0) <= (ref.n + 2) * EPS), f"{label}: C: norms {norms}"
    assert ortho <= 16 * 2 * rel_tol, f"{label}: C: |V'V - I|_max = {ortho:.3e}"
    if subspace:
        assert angle <= dk, f"{label}: D: first {m} modes: {angle:.3e} > {dk:.3e}"
    return figures, rho


def bracket_margins(bracket, Sigma, ref, names_cols):
    """For every variable the smallest eigenvalue of Sigma_vv - lower and of lower + slack I - Sigma_vv, and |Sigma_vv|_2."""
    out = {}
    for nm, cols in names_cols.items():
        lower, slack = bracket[nm]
        S = Sigma[np.ix_(cols, cols)]
        S = 0.5 * (S + S.T)
        lo = float(np.linalg.eigvalsh(S - lower)[0])
        hi = float(np.linalg.eigvalsh(lower + slack * np.eye(len(cols)) - S)[0])
        out[nm] = (lo, hi, float(np.linalg.norm(S, 2)))
    return out
