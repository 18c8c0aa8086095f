"""What the tests of the selection of loop closures share: the candidate lists on the graphs of tests/marginals_helpers.py,
the dense checks of the block rule, the random matrices of the kernel tests and the derived bounds.  It extends the docstring of
tests/selection_helpers.py (left as it is) from a scalar pivot d_c to a dp x dp block B_c; eps = 2^-52, u = eps / 2,
gamma_m = m u / (1 - m u), d = 2 or 3, dp = 3 or 6, column r = c dp + q of candidate c, N = C dp.

Dense checks (host).  With G_c (n x dp) the candidates' Jacobians transposed, H the dense information and W_c = N_c^-1 =
diag(w_r) the candidate's precisions, the gain of the picks S is 1/2 [logdet(H + sum_S G_c W_c G_c') - logdet H]; gains[j] is
held to the difference of two such slogdet values within 1e-9, the margin of selection_helpers.slogdet_gains restated for
blocks: a pick now adds a rank-dp term, which changes nothing in the argument -- each slogdet is one LU factorisation of n
rows (n <= 899: about n eps = 2e-13 relative on a logdet of some thousands, up to ~1e-9 absolute in a difference of two), and
the rule's own gains carry the rounding of a dp x dp Cholesky factorisation on numbers of order one, far below that.

Kernel bounds (GPU).  The device and `bounded_block_reference` run the SAME rule on the SAME matrix P; the reference runs in
np.longdouble (its own rounding is 2^-11 of a double's and counted as one more rounding per operation below), so what is left
is the rounding of the kernels' double operations.  E_x bounds |x_device - x_reference| and is carried from step to step:

    A_rs as in selection_helpers: E_A = gamma_6 |v| (+ u |A_rr| on the diagonal)
    B_c = the diagonal block of A at the start:   E_B[c] = E_A's block, ENTRYWISE (this replaces the scalar E_d)
    step j, pivot p (the same on both sides: see the precondition), sub-step q, J = j dp + q, r = p dp + q:
    acc_i = A_ri - sum_{m<J} L_im L_rm      J products and J subtractions in ascending m:
        E_acc = E_A[i, r] + sum_m (E_L[i, m] (|L_rm| + E_L[r, m]) + |L_im| E_L[r, m])
                + gamma_{J+2} (|A_ir| + sum_m (|L_im| + E_L[i, m]) (|L_rm| + E_L[r, m]))
    root = sqrt(B_p[q, q]):   E_root = E_B[p][q, q] / root + 2 u root
    l_i = acc_i / root:       E_l = (E_acc + |l_i| E_root) / (root - E_root) + 2 u (|l_i| + E_l')     (E_l' the first term)
    B_c[a, b] -= l_a l_b (l_a = l_{c dp + a}):
        E_B[c][a, b] += |l_a| E_l_b + |l_b| E_l_a + E_l_a E_l_b + 2 u (|l_a| + E_l_a) (|l_b| + E_l_b) + 2 u (|B_c[a, b]| + E_B[c][a, b])
    gain(B): the device factorises B + dB, |dB| <= E_B, by an unpivoted Cholesky factorisation of dp rows, whose computed factor
        is the exact factor of B + dB + dB2 with |dB2| <= gamma_{dp+1} |L||L'| (Higham, Accuracy and Stability, Thm 10.3; |L||L'|
        from the reference's factor, gamma_{dp+2} covering the difference of the two factors).  With E = E_B + gamma_{dp+2} |L||L'|
        and e = |E|_F, the `total_gain_bound` argument of selection_helpers on B >= I (every eigenvalue of a Schur block of
        A = I + PSD is >= 1, each moves by at most e, log is 1 / (1 - e)-Lipschitz above 1 - e) gives
        |logdet(B + dB + dB2) - logdet B| <= dp e / (1 - e).  The pivot pi_q the logarithm sees is the squared diagonal of that
        factor up to 2 u relative (the root and its square): 2 u per pivot.  The device's log is within LOG_ULPS ulp, the dp - 1
        additions round gamma_{dp-1} sum |log pi_q|, the halving is exact, and the reference's conversion to double is eps |gain|:
            E_gain = 1/2 [dp e / (1 - e) + 2 dp u + (LOG_ULPS eps + gamma_{dp-1}) sum_q |log pi_q|] + eps |gain|.
    pick_covariances[j][a, b] = (B_p[a, b] - [a == b]) / (sqrt w_a * sqrt w_b): one subtraction, two roots, a product, a division:
        E = E_B[p][a, b] / (sqrt w_a sqrt w_b) (1 + gamma_4) + gamma_6 |value|;     remaining[c] alike.

No number is chosen.

Precondition on the gap.  An order is compared only with the order of the rule on the SAME matrix, and only where the
reference's smallest relative gap (gain_p - gain_next) / gain_p is at least MIN_GAP = 1e-6 -- asserted, never skipped -- and
where, besides, E_gain of the two best candidates of every step stays below half their gap.  The seeds below were checked on
the CPU (tests/test_selection_poses_host.py does it again): the smallest gap of the kernel shapes is printed there."""
import functools

import numpy as np

from marginals_helpers import EPS, reference
from relative_helpers import JAC_ULPS, LD, pair_list, scales
from samples_helpers import twin
from score_amd.refine import unknown_sizes
from score_amd.relative import relative_jacobians
from score_amd.selection import selection_matrix
from score_amd.selection_poses import _block_gains, _scaled, block_greedy_reference, column_precisions

U = EPS / 2
LOG_ULPS = 1
MIN_GAP = 1e-6
# graph -> (candidates, k)
CASES = {"a": (23, 8), "b": (30, 10), "d": (12, 5)}
BASE_PRECISIONS = (4.0, 400.0)
# the kernel tests: N = 63 / 66 around a wavefront and the 32-tiles, one candidate past k's cap (85, 42), one past the workgroup
SIZES = {2: (1, 2, 21, 22, 64, 65, 86, 257), 3: (1, 2, 10, 11, 43, 65)}
SHAPES = [(dim, c, kk) for dim in (2, 3) for c in SIZES[dim] for kk in sorted({min(c, 256 // (3 if dim == 2 else 6)), min(c, 3)})]
# the ownership slots of k_selp_greedy (lane t owns the candidates t + 256 m; m < 3 in 3-D, m < 6 in 2-D) and the caps: in 3-D
# the first lane with two candidates at k's cap, the third (last) slot, one short of the cap and the caps (N = 4092, K = 252);
# in 2-D the third slot at k's cap, one short of the cap and the caps (N = 4095, K = 255, the sixth slot).  random_block_matrix's
# seed 100 + C, checked on the CPU for the gap precondition (tests/test_selection_poses_host.py)
SLOT_SHAPES = [(3, 257, 42), (3, 513, 3), (3, 681, 3), (3, 682, 42), (2, 513, 85), (2, 1364, 3), (2, 1365, 85)]
CAPS = {2: (1365, 85), 3: (682, 42)}
# graph -> (candidates, k) of the long list on a handle: N = 960 columns, two workgroups of k_selp_cross a column slot
LONG_CASES = {"b": (320, 12)}


def dof(dim):
    return 3 if dim == 2 else 6


def gamma(m):
    return m * U / (1.0 - m * U)


def candidates(key):
    """(ids, count, k) of the graph's candidate list: relative_helpers.pair_list."""
    count, k = CASES[key]
    return pair_list(reference(key)[2].prob, count), count, k


def precisions(count, base):
    """(kappa, tau): base (1 + 1/2 cos c) and 2.5 base (1 + 1/2 sin c): no two candidates weigh the same."""
    c = np.arange(count)
    return base * (1.0 + 0.5 * np.cos(c)), 2.5 * base * (1.0 + 0.5 * np.sin(c))


@functools.lru_cache(maxsize=None)
def dense_candidates(key):
    """(G (n x C dp), X = H^-1 G, P = G'X) of the graph's candidates from the dense Cholesky factor; computed once and left
    unchanged."""
    import scipy.linalg as sla

    ref = reference(key)[2]
    ids, _, _ = candidates(key)
    G, _, _ = relative_jacobians(ref.prob, ref.point, ids)
    X = sla.cho_solve(ref.chol, G)
    P = G.T @ X
    for a in (G, X, P):
        a.setflags(write=False)
    return G, X, P


def slogdet_block_gains(H, G, w, dp, order):
    """The increments of 1/2 logdet(H + sum G_c W_c G_c') along `order` (selection_helpers.slogdet_gains for blocks)."""
    out, M = [], H.copy()
    last = np.linalg.slogdet(M)[1]
    for c in order:
        Gc = G[:, c * dp:(c + 1) * dp]
        M = M + (Gc * w[c * dp:(c + 1) * dp]) @ Gc.T
        now = np.linalg.slogdet(M)[1]
        out.append(0.5 * (now - last))
        last = now
    return np.asarray(out)


@functools.lru_cache(maxsize=None)
def random_block_matrix(count, dim):
    """(P, kappa, tau): P = B B'/m + 1e-9 (R - R') with N = count dp rows and m = 2 N columns (full rank: no Schur block runs
    into I), kappa and tau each graded over two decades by an independent permutation; seed 100 + count.  Left unchanged."""
    n = count * dof(dim)
    rng = np.random.default_rng(100 + count)
    B = rng.normal(size=(n, 2 * n))
    R = rng.normal(size=(n, n))
    P = B @ B.T / (2 * n) + 1e-9 * (R - R.T)
    kappa = 0.5 * 100.0 ** (rng.permutation(count) / max(count - 1, 1))
    tau = 0.5 * 100.0 ** (rng.permutation(count) / max(count - 1, 1))
    for a in (P, kappa, tau):
        a.setflags(write=False)
    return P, kappa, tau


@functools.lru_cache(maxsize=1)
def slot_block_matrix(count, dim):
    """random_block_matrix(count, dim) of a slot shape without that function's unbounded cache: the last one asked for is kept
    (134 MB at the caps)."""
    return random_block_matrix.__wrapped__(count, dim)


@functools.lru_cache(maxsize=None)
def slot_block_reference(dim, count, k):
    """bounded_block_reference of a slot shape: computed once a session (10 s of host time at the caps) and left unchanged."""
    ref = bounded_block_reference(*slot_block_matrix(count, dim), dim, k)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def graded_blocks(count, dim):
    """(pi, P): selection_helpers.graded with the modulus 2048 (1001 is odd: (1001 c) mod 2048 is a bijection of range(2048),
    so it takes `count` <= 1365 distinct values on range(count)), and P = diag(1 + pi(c) / 4096 on all dp coordinates of c)."""
    from selection_helpers import graded

    pi, value = graded(count, 2048)
    return pi, np.diag(np.repeat(value, dof(dim)))


def long_candidates(key):
    """(ids, count, k) of the graph's long candidate list (LONG_CASES): relative_helpers.pair_list again, whose first 320
    pairs on graph b are 320 different unordered pairs -- no reversed duplicate, no exact tie."""
    count, k = LONG_CASES[key]
    return pair_list(reference(key)[2].prob, count), count, k


@functools.lru_cache(maxsize=None)
def dense_long_matrix(key):
    """P = G'H^-1 G of the graph's long candidate list from the dense Cholesky factor; computed once and left unchanged."""
    import scipy.linalg as sla

    ref = reference(key)[2]
    G, _, _ = relative_jacobians(ref.prob, ref.point, long_candidates(key)[0])
    P = G.T @ sla.cho_solve(ref.chol, G)
    P.setflags(write=False)
    return P


def _gain_bound(B, E_B, dp):
    """E_gain of the module's docstring for the reference block B (long double) with the entrywise bound E_B."""
    Lc = np.linalg.cholesky(np.asarray(B, dtype=np.float64))
    T = np.abs(Lc) @ np.abs(Lc).T
    e = float(np.linalg.norm(E_B + gamma(dp + 2) * T))
    assert e < 0.5
    logs = float(np.sum(np.abs(np.log(np.diag(Lc) ** 2))))
    gain = 0.5 * float(np.linalg.slogdet(np.asarray(B, dtype=np.float64))[1])
    return 0.5 * (dp * e / (1.0 - e) + 2 * dp * U + (LOG_ULPS * EPS + gamma(dp - 1)) * logs) + EPS * abs(gain)


def _scaled_bound(B, E_B, w):
    sw = np.sqrt(np.asarray(w, dtype=np.float64))
    scale = sw[..., :, None] * sw[..., None, :]
    value = np.abs(np.asarray(_scaled(B, np.asarray(w, dtype=B.dtype)), dtype=np.float64))
    return E_B / scale * (1.0 + gamma(4)) + gamma(6) * value


def bounded_block_reference(P, kappa, tau, dim, k, min_gain=0.0, excluded=None):
    """The rule in np.longdouble on P (block_greedy_reference) with the bounds of the module's docstring: a dict with the
    reference's outputs in double and `gain_bound` (k), `pick_bound` (k x dp x dp), `remaining_bound` (C x dp x dp), `min_gap`.
    Asserts the precondition on the gap."""
    dp = dof(dim)
    n = len(kappa)
    N = n * dp
    w64 = column_precisions(dim, np.asarray(kappa, dtype=np.float64), np.asarray(tau, dtype=np.float64), n)
    wl = w64.astype(LD)
    ref = block_greedy_reference(P, wl, dp, k, min_gain, excluded, dtype=LD)
    m = ref["picked"]
    assert m == 0 or ref["min_gap"] >= MIN_GAP, f"the reference's smallest gap is {ref['min_gap']:.3e}: choose another seed"
    Pl = np.asarray(P, dtype=LD)
    A = selection_matrix(Pl, wl)
    V = np.abs(A - np.eye(N, dtype=LD)).astype(np.float64)
    absA = np.abs(A).astype(np.float64)
    E_A = gamma(6) * V + np.diag(U * np.diag(absA))
    blocks = lambda M: np.stack([M[c * dp:(c + 1) * dp, c * dp:(c + 1) * dp] for c in range(n)]).copy()
    B, E_B = blocks(A), blocks(E_A)
    state = np.ones(n, dtype=np.int64)
    if excluded is not None:
        state[np.asarray(excluded) != 0] = 0
    K = max(k, 1) * dp
    L, E_L = np.zeros((N, K), dtype=LD), np.zeros((N, K))
    gain_bound, pick_bound = np.zeros(k), np.zeros((k, dp, dp))
    wb = w64.reshape(n, dp)
    for j in range(m):
        p = int(ref["order"][j])
        gain_bound[j] = _gain_bound(B[p], E_B[p], dp)
        eligible = np.flatnonzero(state == 1)
        if eligible.size > 1:  # the two best of the step: the bound of both below half their gap
            g = _block_gains(B[eligible])
            g[eligible == p] = -1
            s = int(eligible[int(np.argmax(g))])
            gap = float(_block_gains(B[[p]])[0] - np.max(g))
            worst = max(gain_bound[j], _gain_bound(B[s], E_B[s], dp))
            assert worst < 0.5 * gap, f"step {j}: the bound {worst:.3e} of the two best gains against half their gap {0.5 * gap:.3e}"
        pick_bound[j] = _scaled_bound(B[p], E_B[p], wb[p])
        state[p] = 2
        for q in range(dp):
            J, r = j * dp + q, p * dp + q
            absL, Lr, ELr = np.abs(L[:, :J]).astype(np.float64), np.abs(L[r, :J]).astype(np.float64), E_L[r, :J]
            E_acc = (E_A[:, r] + E_L[:, :J] @ (Lr + ELr) + absL @ ELr
                     + gamma(J + 2) * (absA[:, r] + (absL + E_L[:, :J]) @ (Lr + ELr)))
            acc = A[r, :].copy()
            for i in range(J):
                acc -= L[:, i] * L[r, i]
            root = np.sqrt(B[p, q, q])
            E_root = E_B[p, q, q] / float(root) + 2 * U * float(root)
            l = acc / root
            absl = np.abs(l).astype(np.float64)
            first = (E_acc + absl * E_root) / (float(root) - E_root)
            E_l = first + 2 * U * (absl + first)
            L[:, J], E_L[:, J] = l, E_l
            lb, la, El = l.reshape(n, dp), absl.reshape(n, dp), E_l.reshape(n, dp)
            B = B - lb[:, :, None] * lb[:, None, :]
            E_B = (E_B + la[:, :, None] * El[:, None, :] + la[:, None, :] * El[:, :, None] + El[:, :, None] * El[:, None, :]
                   + 2 * U * (la + El)[:, :, None] * (la + El)[:, None, :] + 2 * U * (np.abs(B).astype(np.float64) + E_B))
    remaining_bound = _scaled_bound(B, E_B, wb)
    picked = ref["order"][:m]
    remaining_bound[picked] = pick_bound[:m]
    out = {k_: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) and v.dtype == LD else v) for k_, v in ref.items()}
    out.update(gain_bound=gain_bound, pick_bound=pick_bound, remaining_bound=remaining_bound)
    return out


def check_against_reference(out, ref, label):
    """A device selection `out` (block_greedy_from_matrix / PoseSelectionHandle.select_relative_poses) against
    bounded_block_reference on the same matrix: the order exactly, the three value arrays within their bounds.  Prints the
    worst ratios."""
    m = ref["picked"]
    np.testing.assert_array_equal(out["order"], ref["order"], err_msg=label)
    worst = {}
    for key, bound in (("gains", "gain_bound"), ("pick_covariances", "pick_bound"), ("remaining", "remaining_bound")):
        err = np.abs(out[key] - ref[key])
        worst[key] = float(np.max(err / np.where(ref[bound] > 0, ref[bound], 1.0))) if err.size else 0.0
        bad = np.argwhere(~(err <= ref[bound]))
        assert bad.size == 0, f"{label}, {key}: entry {bad[:3].tolist()}: |device - reference| {err[tuple(bad[0])]} > bound {ref[bound][tuple(bad[0])]}"
    assert np.all(out["order"][m:] == -1) and np.all(out["gains"][m:] == 0) and np.all(out["pick_covariances"][m:] == 0)
    print(f"{label}: {m} picks, min gap {ref['min_gap']:.3e}, worst |device - reference| / bound: "
          + ", ".join(f"{k_} {v:.3e}" for k_, v in worst.items()))


def matrix_bound(tw, ids, out):
    """The entrywise bound of relative_helpers.check_relative extended to the cross terms g_r'x_j (N x N, entry [r, j], the
    matrix_bound pattern of selection_helpers): |g_r| ex_j + dg_r'|x_ref,j| + |dg_r| ex_j + (2 dp + 1) eps (|g_r|'|x_ref,j| +
    |g_r| ex_j), with ex_j = (residual_j + rounding_j + rho_ref,j + |dg_j|) / lambda_min.  Returns (P_ref, bound)."""
    import scipy.linalg as sla

    ref = tw.ref
    _, dp = unknown_sizes(ref.prob)
    G, _, _ = relative_jacobians(ref.prob, ref.point, ids)
    B, _, _ = scales(ref.prob, ref.point, ids)
    X = sla.cho_solve(ref.chol, G)
    R = G.astype(LD) - ref.H.astype(LD) @ X.astype(LD)
    rho_ref = np.sqrt(np.sum(R * R, axis=0)).astype(np.float64)
    rounding = (ref.longest_row + 1) * EPS * np.linalg.norm(ref.absH @ np.abs(X), axis=0)
    DG = JAC_ULPS * EPS * B
    gnorm, dgnorm = np.linalg.norm(G, axis=0), np.linalg.norm(DG, axis=0)
    ex = (np.asarray(out["residuals"]).reshape(-1) + rounding + rho_ref + dgnorm) / ref.lambda_min
    absX = np.abs(X)
    bound = (gnorm[:, None] * ex[None, :] + DG.T @ absX + dgnorm[:, None] * ex[None, :]
             + (2 * dp + 1) * EPS * (np.abs(G).T @ absX + gnorm[:, None] * ex[None, :]))
    return G.T @ X, bound


def total_gain_bound(P_ref, bound, w, dp, order):
    """selection_helpers.total_gain_bound for blocks: what an entrywise error `bound` of P implies for the gain
    1/2 logdet(I + D_S P_SS D_S) of the columns of the candidates `order`: |logdet(M + E) - logdet M| <= m e / (1 - e) for the
    m = picks dp columns, e = |D_S bound_SS D_S|_F.  Returns (the dense reference's gain of that set, the bound)."""
    S = (np.asarray(order, dtype=np.int64)[:, None] * dp + np.arange(dp)[None, :]).reshape(-1)
    sw = np.sqrt(w[S])
    M = np.eye(len(S)) + sw[:, None] * (0.5 * (P_ref + P_ref.T))[np.ix_(S, S)] * sw[None, :]
    e = float(np.linalg.norm(sw[:, None] * bound[np.ix_(S, S)] * sw[None, :]))
    assert e < 0.5
    return 0.5 * float(np.linalg.slogdet(M)[1]), 0.5 * len(S) * e / (1.0 - e)


__all__ = ["CASES", "BASE_PRECISIONS", "MIN_GAP", "SIZES", "SHAPES", "dof", "candidates", "precisions", "dense_candidates",
           "slogdet_block_gains", "random_block_matrix", "bounded_block_reference", "check_against_reference", "matrix_bound",
           "total_gain_bound", "twin", "reference", "SLOT_SHAPES", "CAPS", "LONG_CASES", "slot_block_matrix", "slot_block_reference",
           "graded_blocks", "long_candidates", "dense_long_matrix"]
