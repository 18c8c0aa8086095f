"""What the relative-pose tests share: the pairs, the finite-difference model of the definitions, and the derived bounds.  The
graphs, points and dense references are those of tests/marginals_helpers.py.  eps = 2^-52; d = 2 or 3, dp = 3 or 6.

The Jacobian, entry by entry.  R_ab = R_a'R_b and t_ab = R_a'(t_b - t_a) are d-term sums of products; G's entries are copies
of entries of R_ab, R_a and t_ab, the constants 0 and +-1.  Two evaluations in double (NumPy's, g++'s, the device's) share the
point and differ by: the factors -- in 2-D cos / sin of a heading through each side's libm, each within 2 ulp of the exact
value, so within 4 eps of one another (in 3-D the rotations are data: 0) -- 8 eps for a product of two; the product's
rounding, eps / 2 per side: 1 eps; the d - 1 additions per side (a fused multiply-add only drops roundings): 2 eps.  That is
11 eps of sum |terms|; JAC_ULPS = 16.  The subtraction t_b - t_a is one operation on the same inputs: the same on all sides.
``jacobian_scale`` gives sum |terms| per entry (B): 0 for a structural zero and for the constants, which therefore agree
exactly.

The finite differences.  xi(step) is the definition's error coordinate of the relative pose after the refinement's own
retraction: 2-D ((theta_b + s_b) - (theta_a + s_a) - theta_ab, R(theta_a + s_a)'(t_b - t_a + ...) - t_ab), 3-D
(Log(R_ab'R_ab(step)), t_ab(step) - t_ab), in np.longdouble.  Along one unknown at a time: the rotation part is LINEAR (2-D
by definition; 3-D Log(R_ab' Exp(-s e_k) R_ab) = -s R_ab'e_k and Log(Exp(s e_k)) = s e_k), the translation part is linear in
(x, y) / v and, along the heading / omega_a,k, t_ab(s) = Exp(-s e_k) t_ab, whose third derivative has norm <= |t_ab|.  The
central difference with step h is therefore off by at most h^2 / 6 (1 + |t_ab|) (the 1: slack for nothing), plus the rounding
of the two evaluations, LD_OPS eps_ld (1 + |t_a| + |t_b|) / h with LD_OPS = 64 (four nested d-term sums and Rodrigues'
formula: < 16 roundings per entry and evaluation, relative to magnitudes <= 1 + |t_a| + |t_b|, two evaluations, and the Log's
theta / sin theta), plus the double Jacobian's own JAC_ULPS eps B, plus the point's defect: a 3-D rotation of the point is
orthogonal to `defect` = max |R'R - I| only, which enters R_ab'R_ab(step) and so xi to first order: 8 defect (1 + |t_ab|).
With h = 2^-17 the bound is of order 1e-11 (1 + |t_ab|); a wrong sign or a transposed block is off by the entry itself.

The covariances.  Column j = c dp + q solves H x_j = g_q, g_q = G_c'e_q.  x_ref is the Cholesky solve of the dense H with
NumPy's g_q, rho_ref its residual in np.longdouble, `rounding` the rounding of a residual in double (marginals_helpers),
dg_q = JAC_ULPS eps B_q entry by entry the difference of the two g_q.  As in leverage_helpers,

    |x_j - x_ref|_2 <= ex := (residual_j + rounding + rho_ref + |dg_q|_2) / lambda_min,
    |P[q', q] - g_q'' x_ref| <= |g_q'|_2 ex + dg_q''(|x_ref|) + |dg_q'|_2 ex + (2 dp + 1) eps (|g_q'|'|x_ref| + |g_q'|_2 ex):

the solution's error through g_q', the two sides' g_q' on |x_j| <= |x_ref| + |x_j - x_ref|, and the dot itself (2 dp products
added to a zero).  With the call's `solutions` (x_j itself) the reported residual is held against |g_q - H x_j|_2 recomputed
in np.longdouble within rounding(|x_j|) + (n + 1) eps of it + |dg_q|_2, and P[q', q] against g_q''x_j within
dg_q''|x_j| + (2 dp + 1) eps |g_q'|'|x_j|.  R_ab and t_ab are held within JAC_ULPS eps B.  Every term is computed from NumPy's
values; no tolerance is chosen.
"""
import numpy as np
import scipy.linalg as sla

from marginals_helpers import EPS, Reference
from score_amd.marginals import _problem_and_point, dense_information
from score_amd.refine import _hat, unknown_sizes
from score_amd.relative import _rotations_and_translations, relative_jacobians

JAC_ULPS = 16
LD_OPS = 64
FD_STEP = 2.0 ** -17
LD = np.longdouble
EPS_LD = float(np.finfo(np.longdouble).eps)


def pair_list(prob, count):
    """`count` pairs of pose ids, in turn: (0, k), (k, 0), two neighbours of one chain, two poses of different robots (half the
    poses apart; on a single chain: far apart), then two poses a few steps apart."""
    Np = prob.Np
    out = []
    for k in range(count):
        p = 1 + (7 * k + 3) % (Np - 2)  # 1 .. Np - 2
        kind = k % 5
        if kind == 0:
            out.append((0, p))
        elif kind == 1:
            out.append((p, 0))
        elif kind == 2:
            out.append((p + 1, p) if (p + 1) % (Np // 2) else (p, p - 1))
        elif kind == 3:
            out.append((p, 1 + (p - 1 + Np // 2) % (Np - 1)))
        else:
            out.append((p, 1 + (p + 4) % (Np - 1)))
    ids = np.asarray(out, dtype=np.int32).reshape(-1, 2)
    assert np.all(ids[:, 0] != ids[:, 1]) and ids.min() >= 0 and ids.max() < Np
    return ids


class WeightedReference(Reference):
    """marginals_helpers.Reference under range AND loop-closure weights."""

    def __init__(self, fg, results, range_weights, loop_closure_weights):
        self.prob, self.point = _problem_and_point(fg, results, range_weights, loop_closure_weights)
        self.H = dense_information(self.prob, self.point)
        self.H.setflags(write=False)
        self.n = self.prob.n
        self.chol = sla.cho_factor(self.H, lower=True)
        self.lambda_min = float(sla.eigvalsh(self.H, subset_by_index=[0, 0])[0])
        assert self.lambda_min > 0
        self.longest_row = int(np.max(np.count_nonzero(self.H, axis=1)))
        self.absH = np.abs(self.H)


# ---------------------------------------------------------------------------------------------------------------------
# the Jacobian's scale and structure
# ---------------------------------------------------------------------------------------------------------------------
def jacobian_scale(Ra, ta, Rb, tb):
    """(B_G (dp x 2 dp), B_R (d x d), B_t (d)): sum |terms| of every entry of G, R_ab and t_ab -- 0 for the structural zeros
    and the constants."""
    d = len(ta)
    dp = 3 if d == 2 else 6
    ro = dp - d
    BR, Bt = np.abs(Ra).T @ np.abs(Rb), np.abs(Ra).T @ np.abs(tb - ta)
    B = np.zeros((dp, 2 * dp))
    if d == 2:
        B[1, 0], B[2, 0] = Bt[1], Bt[0]
    else:
        B[:3, :3] = BR.T
        B[3:, :3] = np.abs(_hat(Bt))
    B[ro:, ro:dp] = np.abs(Ra).T
    B[ro:, dp + ro:] = np.abs(Ra).T
    return B, BR, Bt


def structure(d):
    """The entries of G (dp x 2 dp) that are not structural zeros."""
    dp = 3 if d == 2 else 6
    M = np.zeros((dp, 2 * dp), dtype=bool)
    if d == 2:
        M[0, 0] = M[0, 3] = True
        M[1:, 0] = True
        M[1:, 1:3] = M[1:, 4:6] = True
    else:
        M[:3, :3] = True
        M[:3, 6:9] = np.eye(3, dtype=bool)
        M[3:, :3] = ~np.eye(3, dtype=bool)
        M[3:, 3:6] = M[3:, 9:12] = True
    return M


def scales(prob, point, ids):
    """(B (n x C dp, laid out as relative_jacobians' G), B_R (C x d x d), B_t (C x d)) for the pairs."""
    d, dp = unknown_sizes(prob)
    R, t = _rotations_and_translations(prob, point)
    B = np.zeros((prob.n, len(ids) * dp))
    BR, Bt = np.zeros((len(ids), d, d)), np.zeros((len(ids), d))
    for c, (a, b) in enumerate(np.asarray(ids, dtype=np.int64)):
        g, BR[c], Bt[c] = jacobian_scale(R[a], t[a], R[b], t[b])
        for v, first in ((a, 0), (b, dp)):
            if v >= 1:
                B[dp * (v - 1):dp * v, c * dp:(c + 1) * dp] = g[:, first:first + dp].T
    return B, BR, Bt


# ---------------------------------------------------------------------------------------------------------------------
# central differences of the definitions in np.longdouble
# ---------------------------------------------------------------------------------------------------------------------
def _hat_ld(w):
    K = np.zeros((3, 3), dtype=LD)
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
    return K


def _exp_ld(w):
    th2 = w @ w
    th = np.sqrt(th2)
    K = _hat_ld(w)
    if th < LD(1e-10):
        A, Bc = LD(1) - th2 / 6, LD(0.5) - th2 / 24
    else:
        A, Bc = np.sin(th) / th, (LD(1) - np.cos(th)) / th2
    return np.eye(3, dtype=LD) + A * K + Bc * (K @ K)


def _log_ld(M):
    w = LD(0.5) * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]], dtype=LD)
    s = np.sqrt(w @ w)
    c = LD(0.5) * (M[0, 0] + M[1, 1] + M[2, 2] - LD(1))
    th = np.arctan2(s, c)
    return w * (LD(1) + th * th / 6 if s < LD(1e-10) else th / s)


def _relative_ld(dim, pa, pb):
    """(rotation part, t_ab) of T_a^-1 T_b from the ends (2-D: (theta, t); 3-D: (R, t)) in np.longdouble."""
    if dim == 2:
        c, s = np.cos(pa[0]), np.sin(pa[0])
        Ra = np.array([[c, -s], [s, c]], dtype=LD)
        return pb[0] - pa[0], Ra.T @ (pb[1] - pa[1])
    return pa[0].T @ pb[0], pa[0].T @ (pb[1] - pa[1])


def _retract_ld(dim, pose, step):
    """The refinement's retraction of one pose by its dp unknowns."""
    if dim == 2:
        return pose[0] + step[0], pose[1] + step[1:]
    return pose[0] @ _exp_ld(step[:3]), pose[1] + step[3:]


def finite_difference_jacobians(prob, point, ids, h=FD_STEP):
    """(G_fd (n x C dp, as relative_jacobians' G), bound (the same shape), defect): central differences of the definitions
    through the retraction, and the module docstring's bound per entry."""
    d, dp = unknown_sizes(prob)
    R, t = _rotations_and_translations(prob, point)
    if d == 2:
        th = prob.split(point)[0]
        pose = [(LD(th[p]), t[p].astype(LD)) for p in range(prob.Np)]
        defect = 0.0
    else:
        pose = [(R[p].astype(LD), t[p].astype(LD)) for p in range(prob.Np)]
        defect = float(np.max(np.abs(np.einsum("pki,pkj->pij", R, R) - np.eye(3))))
    ids = np.asarray(ids, dtype=np.int64)
    Gnp, _, tab = relative_jacobians(prob, point, ids)
    B, _, _ = scales(prob, point, ids)
    G = np.zeros_like(Gnp)
    bound = np.zeros_like(Gnp)
    hl = LD(h)

    def xi(pa, pb, rot0, t0):
        rot, tt = _relative_ld(d, pa, pb)
        r = np.array([rot - rot0], dtype=LD) if d == 2 else _log_ld(rot0.T @ rot)
        return np.concatenate([r, tt - t0])

    for c, (a, b) in enumerate(ids):
        rot0, t0 = _relative_ld(d, pose[a], pose[b])
        size = 1.0 + float(np.linalg.norm(tab[c]))
        reach = 1.0 + float(np.linalg.norm(t[a])) + float(np.linalg.norm(t[b]))
        for v, moves_a in ((a, True), (b, False)):
            if v < 1:
                continue
            for k in range(dp):
                step = np.zeros(dp, dtype=LD)
                step[k] = hl
                plus, minus = _retract_ld(d, pose[v], step), _retract_ld(d, pose[v], -step)
                if moves_a:
                    up, dn = xi(plus, pose[b], rot0, t0), xi(minus, pose[b], rot0, t0)
                else:
                    up, dn = xi(pose[a], plus, rot0, t0), xi(pose[a], minus, rot0, t0)
                G[dp * (v - 1) + k, c * dp:(c + 1) * dp] = ((up - dn) / (2 * hl)).astype(np.float64)
        bound[:, c * dp:(c + 1) * dp] = (h * h / 6.0 * size + LD_OPS * EPS_LD * reach / h + 8.0 * defect * size
                                         + JAC_ULPS * EPS * B[:, c * dp:(c + 1) * dp])
    return G, bound, defect


# ---------------------------------------------------------------------------------------------------------------------
# the device's outputs against the dense reference
# ---------------------------------------------------------------------------------------------------------------------
def dense_covariances(ref, ids):
    """(P (C x dp x dp) = G_c'Sigma G_c from the dense Cholesky, G, X = Sigma G)."""
    _, dp = unknown_sizes(ref.prob)
    G, _, _ = relative_jacobians(ref.prob, ref.point, ids)
    X = sla.cho_solve(ref.chol, G)
    P = np.stack([G[:, c * dp:(c + 1) * dp].T @ X[:, c * dp:(c + 1) * dp] for c in range(len(ids))])
    return P, G, X


def check_relative(ref, ids, out, label, need_converged=True):
    """The bounds of the module's docstring for every CONVERGED column of the call's outputs `out` (RelativeHandle's dict, or
    one put together from the public function's results): prints the worst ratios, returns (want, bound) of P."""
    prob = ref.prob
    d, dp = unknown_sizes(prob)
    C = len(ids)
    want, G, X = dense_covariances(ref, ids)
    B, BR, Bt = scales(prob, ref.point, ids)
    _, Rab, tab = relative_jacobians(prob, ref.point, ids)
    Hl = ref.H.astype(LD)
    Rr = G.astype(LD) - Hl @ X.astype(LD)
    rho_ref = np.sqrt(np.sum(Rr * Rr, axis=0)).astype(np.float64)
    rounding = (ref.longest_row + 1) * EPS * np.linalg.norm(ref.absH @ np.abs(X), axis=0)
    DG = JAC_ULPS * EPS * B
    gnorm, dgnorm = np.linalg.norm(G, axis=0), np.linalg.norm(DG, axis=0)
    res = np.asarray(out["residuals"]).reshape(C * dp)
    conv = np.asarray(out["converged"]).reshape(C * dp)
    if need_converged:
        assert out["rc"] == 0 and np.all(conv), f"{label}: {out['iterations']}"
    ex = (res + rounding + rho_ref + dgnorm) / ref.lambda_min  # per column j
    absX = np.abs(X)
    bound = np.zeros((C, dp, dp))
    for c in range(C):
        cols = slice(c * dp, (c + 1) * dp)
        g, dg = G[:, cols], DG[:, cols]
        for q in range(dp):
            j = c * dp + q
            bound[c, :, q] = (gnorm[cols] * ex[j] + dg.T @ absX[:, j] + dgnorm[cols] * ex[j]
                              + (2 * dp + 1) * EPS * (np.abs(g).T @ absX[:, j] + gnorm[cols] * ex[j]))
    err = np.abs(out["covariances"] - want)
    live = np.broadcast_to(conv.reshape(C, 1, dp), err.shape)  # (column q of P_c is column j's)
    worst = float(np.max(np.where(live, err / bound, 0.0)))
    scale = np.abs(want).max(axis=(1, 2), keepdims=True)
    print(f"{label}: {C} pairs, worst |P - G'Sigma G| / bound = {worst:.3e}, worst error over the block's largest entry "
          f"{float(np.max(np.where(live, err / scale, 0.0))):.3e}, worst residual {float(np.max(res[conv])) if conv.any() else 0.0:.3e}")
    assert np.all(np.diagonal(want, axis1=1, axis2=2) > 0)
    assert np.all(err[live] <= bound[live]), f"{label}: pair {int(np.argmax(np.where(live, err - bound, -np.inf)) // (dp * dp))}"
    rot_err, tr_err = np.abs(out["rotations"] - Rab), np.abs(out["translations"] - tab)
    print(f"{label}: worst |R_ab - NumPy's| / eps = {float(rot_err.max()) / EPS:.2f}, |t_ab - NumPy's| / (eps |t_ab|) = "
          f"{float(np.max(tr_err / np.maximum(np.abs(tab), 1e-300))) / EPS:.2f}")
    assert np.all(rot_err <= JAC_ULPS * EPS * BR) and np.all(tr_err <= JAC_ULPS * EPS * Bt)
    if out.get("solutions") is None:  # (the public function does not ask for them)
        return want, bound
    x = out["solutions"].T  # (n x C dp, as X)
    assert x.shape == X.shape
    Rx = G.astype(LD) - Hl @ x.astype(LD)
    mine = np.sqrt(np.sum(Rx * Rx, axis=0)).astype(np.float64)
    slack = (ref.longest_row + 1) * EPS * np.linalg.norm(ref.absH @ np.abs(x), axis=0) + (ref.n + 1) * EPS * mine + dgnorm
    off = np.abs(res - mine)
    absx = np.abs(x)
    worst_dot = 0.0
    for c in range(C):
        cols = slice(c * dp, (c + 1) * dp)
        g, dg = G[:, cols], DG[:, cols]
        for q in range(dp):
            j = c * dp + q
            dot = (g.astype(LD).T @ x[:, j].astype(LD)).astype(np.float64)
            dot_slack = dg.T @ absx[:, j] + (2 * dp + 1) * EPS * (np.abs(g).T @ absx[:, j])
            gap = np.abs(out["covariances"][c, :, q] - dot)
            worst_dot = max(worst_dot, float(np.max(gap / dot_slack)))
            assert np.all(gap <= dot_slack), f"{label}: column {j}: P against G x"
    print(f"{label}: worst |reported - recomputed residual| / slack = {float(np.max(off / slack)):.3e} (recomputed up to "
          f"{float(np.max(mine)):.3e}), worst |P - G x| / slack = {worst_dot:.3e}")
    assert np.all(mine > 0) and np.all(off <= slack), f"{label}: column {int(np.argmax(off - slack))}: {res} against {mine}"
    assert np.all((np.linalg.norm(x - X, axis=0) <= ex)[conv])
    return want, bound
