"""What the selection tests share: the candidate lists on the graphs of tests/marginals_helpers.py, the dense checks of the
greedy rule, the random matrices of the kernel tests and the derived bounds.

Dense checks (host).  With G the candidates' gradients and H the dense information, the gain of the picks S is
1/2 [logdet(H + G_S W_S G_S') - logdet H]; gains[j] is held to the difference of two such slogdet values within 1e-9: measured
at most 9e-12 on gains of 0.03 .. 2.8, and the margin covers slogdet's own rounding at n = 899 (graph b: an LU factorisation of
899 rows, about n eps = 2e-13 relative on a logdet of some thousands, i.e. up to ~1e-9 absolute in a difference of two).

The variances of the python engine (g'H^-1 g, the pick and remaining variances) are held to dense solves with H + G_S W_S G_S'
within dense_rtol = n eps cond_2(H) relative: both sides are backward-stable dense solves in double (an LU or Cholesky
factorisation of n rows perturbs the matrix by about n eps relative, which moves a quadratic form g'M^-1 g by at most
cond_2(M) times that), and cond_2(H + G_S W_S G_S') exceeds cond_2(H) by at most 1 + 2 sum w / lambda_max(H) (|g|^2 <= 2),
which the factor is multiplied by.  Computed per graph from the Reference's lambda_min; no number is chosen.

Kernel bounds (GPU).  The device and `bounded_reference` run the SAME rule on the SAME matrix P; the reference runs in
np.longdouble (its own rounding is 2^-11 of a double's and counted as one more rounding per operation below), so what is
left is the rounding of the kernels' double operations, u = eps / 2 each, a fused multiply-add only dropping one.  With
gamma_m = m u / (1 - m u), and E_x a bound on |x_device - x_reference| carried from step to step:

    A_rc = [1 +] (sqrt w_lo * (1/2 (P_rc + P_cr))) * sqrt w_hi     one addition, two roots, two products, the 1 on the diagonal:
        E_A = gamma_6 |v| (+ u |A_cc| on the diagonal)             (the halving is exact)
    d_c = A_cc at the start:   E_d = E_A
    step j, pivot p (the same on both sides: see the precondition):
    acc_c = A_cp - sum_{i<j} L_ci L_pi      j products and j subtractions in ascending i:
        E_acc = E_A[c, p] + sum_i (E_L[c, i] (|L_pi| + E_L[p, i]) + |L_ci| E_L[p, i])
                + gamma_{j+2} (|A_cp| + sum_i (|L_ci| + E_L[c, i]) (|L_pi| + E_L[p, i]))
    root = sqrt(d_p):   E_root = E_d[p] / sqrt(d_p) + 2 u sqrt(d_p)        (sqrt a - sqrt b = (a - b) / (sqrt a + sqrt b))
    l_c = acc_c / root: E_l = (E_acc + |l_c| E_root) / (root - E_root) + 2 u (|l_c| + E_l')      (E_l' the first term)
    d_c -= l_c^2:       E_d[c] += 2 |l_c| E_l + E_l^2 + 2 u (|l_c| + E_l)^2 + 2 u (|d_c| + E_d[c])
    gains[j] = 1/2 log d_p:   E = 1/2 E_d[p] / (d_p - E_d[p]) + (LOG_ULPS + 1) eps |gain|     (the device's log: 1 ulp as
                              documented for the HIP math library; one more for the reference's conversion to double)
    pick_variances[j] = (d_p - 1) / w_p:   E = (E_d[p] + 2 u |d_p - 1|) / w_p + 2 u |value|;   remaining[c] alike.

Every Schur diagonal is thus a j-term sum whose bound follows from the operation count; no number is chosen.

Precondition on the pivot gap.  Near-ties are in the data (7e-6 relative between the two best pivots on graph b), so an order
is compared only with the order of the rule on the SAME matrix, and only where the reference's smallest relative gap between
the two best eligible pivots is at least MIN_GAP = 1e-6 -- asserted here, never skipped: the seeds below were chosen on the CPU
for it -- and where, besides, the bound E_d of both pivots stays below half that gap."""
import functools

import numpy as np

from leverage_helpers import G_ULPS, pair_list
from marginals_helpers import EPS, reference
from samples_helpers import twin
from score_amd.leverage import pair_gradients
from score_amd.refine import _Problem3D
from score_amd.selection import greedy_reference, selection_matrix

U = EPS / 2
LOG_ULPS = 1
MIN_GAP = 1e-6
# graph -> (candidates, k)
CASES = {"a": (37, 12), "b": (70, 16), "d": (37, 12)}
BASE_PRECISIONS = (4.0, 400.0)
# the kernel tests: the tile edges of the 32 x 32 transpose, a wavefront, one lane past the workgroup; k = C (capped at 256)
# and k = 3; one seed per C, chosen on the CPU for the gap precondition
SIZES = (1, 2, 31, 32, 33, 64, 65, 257)
SHAPES = [(c, kk) for c in SIZES for kk in sorted({min(c, 256), min(c, 3)})]
SEEDS = {c: 100 + c for c in SIZES}
# the ownership slots of k_sel_greedy (lane t owns the candidates t + 256 m, m < 16) and both caps: two full slots (16 tiles a
# side), the first lane with three candidates at k = 256 (row_p full), slot 4 in one lane, slot 8 in a coupled sweep, one short of
# the cap with a ragged last tile, and C = 4096 with k = 256 (d and state full, every slot live, L of 2^20 entries, 8256
# workgroups of k_sel_sym).  Seeds 100 + C as above, checked on the CPU for the gap precondition (tests/test_selection_host.py)
SLOT_SHAPES = [(512, 3), (513, 256), (1025, 3), (2049, 40), (4095, 3), (4096, 256)]
SEEDS.update({c: 100 + c for c, _ in SLOT_SHAPES})
# graph -> (candidates, k) of the long list on a handle: k_sel_cross with three workgroups a column, 41 solved blocks
LONG_CASES = {"b": (650, 40)}
CAP, CAP_PICKS = 4096, 256


def candidates(key):
    """(ids, count, k) of the graph's candidate list: pair_list's pose - landmark, first pose - pose, pose - pose and landmark -
    pose pairs in turn."""
    count, k = CASES[key]
    return pair_list(reference(key)[2].prob, count), count, k


def long_candidates(key):
    """(ids, count, k) of the graph's long candidate list (LONG_CASES): pair_list again.  On graph b its 650 ordered pairs are
    all different, and 88 of them join two variables that another pair lists in the other direction; the two directions
    carry different precisions (1 + 1/2 cos c), so no two leading pivots tie exactly and the list stays as pair_list gives it:
    the gap precondition on the dense P is asserted in tests/test_selection_host.py."""
    count, k = LONG_CASES[key]
    return pair_list(reference(key)[2].prob, count), count, k


def precisions(count, base):
    """`base` scaled by 1 + 1/2 cos c: no two candidates weigh the same."""
    return base * (1.0 + 0.5 * np.cos(np.arange(count)))


def gamma(m):
    return m * U / (1.0 - m * U)


@functools.lru_cache(maxsize=None)
def dense_candidates(key):
    """(G, dist, P_dense) of the graph's candidates from the dense Cholesky factor; computed once and left unchanged."""
    import scipy.linalg as sla

    ref = reference(key)[2]
    ids, _, _ = candidates(key)
    G, dist = pair_gradients(ref.prob, ref.point, ids)
    X = sla.cho_solve(ref.chol, G)
    P = G.T @ X
    for a in (G, dist, P, X):
        a.setflags(write=False)
    return G, dist, P, X


@functools.lru_cache(maxsize=None)
def dense_long_matrix(key):
    """P_dense of the graph's long candidate list from the dense Cholesky factor; computed once and left unchanged."""
    import scipy.linalg as sla

    ref = reference(key)[2]
    G, _ = pair_gradients(ref.prob, ref.point, long_candidates(key)[0])
    P = G.T @ sla.cho_solve(ref.chol, G)
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def _lambda_max(key):
    import scipy.linalg as sla

    ref = reference(key)[2]
    return float(sla.eigvalsh(ref.H, subset_by_index=[ref.n - 1, ref.n - 1])[0])


def dense_rtol(key, w):
    """n eps cond_2(H) (1 + 2 sum w / lambda_max(H)): the relative error a dense solve leaves in g'M^-1 g (module docstring)."""
    ref = reference(key)[2]
    lmax = _lambda_max(key)
    return ref.n * EPS * (lmax / ref.lambda_min) * (1.0 + 2.0 * float(np.sum(w)) / lmax)


def slogdet_gains(H, G, w, order):
    """The increments of 1/2 logdet(H + sum w g g') along `order`."""
    out, M = [], H.copy()
    last = np.linalg.slogdet(M)[1]
    for c in order:
        M = M + w[c] * np.outer(G[:, c], G[:, c])
        now = np.linalg.slogdet(M)[1]
        out.append(0.5 * (now - last))
        last = now
    return np.asarray(out)


def random_matrix(n, seed):
    """(P, w): P = B B'/m with m = 2 n columns (full rank: no Schur diagonal runs into 1) plus an antisymmetric part of 1e-9,
    and precisions graded over two decades."""
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(n, 2 * n))
    R = rng.normal(size=(n, n))
    P = B @ B.T / (2 * n) + 1e-9 * (R - R.T)
    w = 0.5 * 100.0 ** (rng.permutation(n) / max(n - 1, 1))
    return P, w


@functools.lru_cache(maxsize=1)
def slot_matrix(n):
    """random_matrix(n, SEEDS[n]) of a slot shape, read-only; the last one asked for is kept (134 MB at the cap)."""
    P, w = random_matrix(n, SEEDS[n])
    P.setflags(write=False)
    w.setflags(write=False)
    return P, w


@functools.lru_cache(maxsize=None)
def slot_reference(n, k):
    """bounded_reference of a slot shape: computed once a session (11 s of host time at the caps) and left unchanged."""
    ref = bounded_reference(*slot_matrix(n), k)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def graded(count, modulus):
    """pi(c) = (1001 c) mod `modulus`, c < count <= modulus: 1001 is odd and the modulus a power of two, so pi is a bijection
    of range(modulus) and takes `count` distinct values on range(count).  The diagonal 1 + pi / 4096 is exact in double, and
    under precisions of 4 (sqrt 4 is exact) so is every pivot 5 + pi / 1024: the order of the picks is argsort(-pi)."""
    assert count <= modulus <= 4096 and modulus & (modulus - 1) == 0
    pi = (1001 * np.arange(count)) % modulus
    assert len(set(pi.tolist())) == count
    return pi, 1.0 + pi / 4096.0


def bounded_reference(P, w, k, min_gain=0.0, excluded=None):
    """The rule in np.longdouble on P (greedy_reference) with the bounds of the module's docstring: a dict with the
    reference's outputs in double and `gain_bound`, `pick_bound` (k), `remaining_bound` (C), `min_gap`.  Asserts the
    precondition on the pivot gap."""
    ld = np.longdouble
    ref = greedy_reference(P, w, k, min_gain, excluded, dtype=ld)
    m, n = ref["picked"], len(w)
    assert m == 0 or ref["min_gap"] >= MIN_GAP, f"the reference's smallest pivot gap is {ref['min_gap']:.3e}: choose another seed"
    Pl, wl = np.asarray(P, dtype=ld), np.asarray(w, dtype=ld)
    A = selection_matrix(Pl, wl)
    V = np.abs(A - np.eye(n, dtype=ld)).astype(np.float64)
    absA = np.abs(A).astype(np.float64)
    E_A = gamma(6) * V + np.diag(U * np.diag(absA))
    d = np.diag(A).copy()
    E_d = np.diag(E_A).copy()
    L, E_L = np.zeros((n, max(k, 1)), dtype=ld), np.zeros((n, max(k, 1)))
    gain_bound, pick_bound = np.zeros(k), np.zeros(k)
    w64 = np.asarray(w, dtype=np.float64)
    for j in range(m):
        p = int(ref["order"][j])
        dp, Edp = float(d[p]), float(E_d[p])
        gain = 0.5 * np.log(dp)
        assert Edp < 0.5 * MIN_GAP * dp
        gain_bound[j] = 0.5 * Edp / (dp - Edp) + (LOG_ULPS + 1) * EPS * abs(gain)
        pick_bound[j] = (Edp + 2 * U * abs(dp - 1)) / w64[p] + 2 * U * abs(dp - 1) / w64[p]
        absL, Lp, ELp = np.abs(L[:, :j]).astype(np.float64), np.abs(L[p, :j]).astype(np.float64), E_L[p, :j]
        E_acc = (E_A[:, p] + E_L[:, :j] @ (Lp + ELp) + absL @ ELp
                 + gamma(j + 2) * (absA[:, p] + (absL + E_L[:, :j]) @ (Lp + ELp)))
        acc = A[p, :].copy()
        for i in range(j):
            acc -= L[:, i] * L[p, i]
        root = np.sqrt(d[p])
        E_root = Edp / float(root) + 2 * U * float(root)
        l = acc / root
        absl = np.abs(l).astype(np.float64)
        first = (E_acc + absl * E_root) / (float(root) - E_root)
        E_l = first + 2 * U * (absl + first)
        L[:, j], E_L[:, j] = l, E_l
        d = d - l * l
        E_d = E_d + 2 * absl * E_l + E_l * E_l + 2 * U * (absl + E_l) ** 2 + 2 * U * (np.abs(d).astype(np.float64) + E_d)
    val = np.abs(d - 1).astype(np.float64)
    remaining_bound = (E_d + 2 * U * val) / w64 + 2 * U * val / w64
    picked = ref["order"][:m]
    remaining_bound[picked] = pick_bound[:m]
    out = {k_: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype == ld else v) for k_, v in ref.items()}
    out.update(gain_bound=gain_bound, pick_bound=pick_bound, remaining_bound=remaining_bound)
    return out


def check_against_reference(out, ref, label):
    """A device selection `out` (greedy_from_matrix / SelectionHandle.select_ranges) against bounded_reference on the same
    matrix: the order exactly, the three value arrays within their bounds.  Prints the worst ratios."""
    m = ref["picked"]
    np.testing.assert_array_equal(out["order"], ref["order"], err_msg=label)
    worst = {}
    for key, bound in (("gains", "gain_bound"), ("pick_variances", "pick_bound"), ("remaining", "remaining_bound")):
        err = np.abs(out[key] - ref[key])
        keep = np.isfinite(ref[key])
        worst[key] = float(np.max(err[keep] / np.where(ref[bound][keep] > 0, ref[bound][keep], 1.0))) if np.any(keep) else 0.0
        bad = np.flatnonzero(keep & ~(err <= ref[bound]))
        assert bad.size == 0, f"{label}, {key}: entry {bad[:5]}: |device - reference| {err[bad[:5]]} > bound {ref[bound][bad[:5]]}"
    assert np.all(out["order"][m:] == -1) and np.all(out["gains"][m:] == 0) and np.all(out["pick_variances"][m:] == 0)
    print(f"{label}: {m} picks, min pivot gap {ref['min_gap']:.3e}, worst |device - reference| / bound: "
          + ", ".join(f"{k_} {v:.3e}" for k_, v in worst.items()))


def matrix_bound(tw, ids, out):
    """The bound of leverage_helpers.check_range_variances extended to g_c'x_d, entry by entry (C x C, entry [c, d]):
    |g_c| |x_d - x_ref,d| + dg_c |x_ref,d| + (2 d + 1) eps |g_c|'|x_ref,d|, with |x_d - x_ref,d| <= (residual_d + rounding_d +
    rho_ref,d + dg_d) / lambda_min.  Returns (P_ref, bound)."""
    import scipy.linalg as sla

    ref = tw.ref
    dim = 3 if isinstance(ref.prob, _Problem3D) else 2
    G, _ = pair_gradients(ref.prob, ref.point, ids)
    X = sla.cho_solve(ref.chol, G)
    R = G.astype(np.longdouble) - ref.H.astype(np.longdouble) @ X.astype(np.longdouble)
    rho_ref = np.sqrt(np.sum(R * R, axis=0)).astype(np.float64)
    rounding = (ref.longest_row + 1) * EPS * np.linalg.norm(ref.absH @ np.abs(X), axis=0)
    gnorm = np.linalg.norm(G, axis=0)
    dg = G_ULPS * EPS * gnorm
    dx = (out["residuals"] + rounding + rho_ref + dg) / ref.lambda_min
    bound = (gnorm[:, None] * dx[None, :] + dg[:, None] * np.linalg.norm(X, axis=0)[None, :]
             + (2 * dim + 1) * EPS * (np.abs(G).T @ np.abs(X)))
    return G.T @ X, bound


def total_gain_bound(P_ref, bound, w, order):
    """What an entrywise error `bound` of P implies for the gain 1/2 logdet(I + D_S P_SS D_S) of the set `order`: with
    M = I + D_S sym(P_SS) D_S (eigenvalues >= 1 for the exact P) and E the perturbation, |E|_2 <= |D_S bound_SS D_S|_F = e, and
    |logdet(M + E) - logdet M| <= m e / (1 - e) for m picks (each eigenvalue moves by at most e, log is 1-Lipschitz above 1 - e).
    Returns (the dense reference's gain of that set, the bound)."""
    S = np.asarray(order, dtype=np.int64)
    sw = np.sqrt(w[S])
    M = np.eye(len(S)) + sw[:, None] * (0.5 * (P_ref + P_ref.T))[np.ix_(S, S)] * sw[None, :]
    e = float(np.linalg.norm(sw[:, None] * bound[np.ix_(S, S)] * sw[None, :]))
    assert e < 0.5
    return 0.5 * float(np.linalg.slogdet(M)[1]), 0.5 * len(S) * e / (1.0 - e)


__all__ = ["CASES", "BASE_PRECISIONS", "MIN_GAP", "SIZES", "SHAPES", "SEEDS", "candidates", "precisions", "dense_candidates", "dense_rtol", "slogdet_gains", "random_matrix",
           "bounded_reference", "check_against_reference", "matrix_bound", "total_gain_bound", "twin", "reference", "SLOT_SHAPES",
           "LONG_CASES", "CAP", "CAP_PICKS", "long_candidates", "dense_long_matrix", "slot_matrix", "slot_reference", "graded"]
