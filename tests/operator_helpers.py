"""What the operator-identity tests share: the graphs, references built from the problem data alone, and the figures.

The two operators of every solve -- the KKT product w = K p and the chain preconditioner z = M^-1 r -- are checked through
identities that hold for the vectors a handle reads back after an ADMM iteration, against matrices SciPy builds from the
problem (P, A, the chain hint) and the handle's scales D, E.  No product or twin host code is used; every product that enters
a figure is accumulated in np.longdouble.

    K  = D P D + sigma I + rho (E A D)'(E A D)                       (reference_K)
    T  = the entries of K inside a chain at node distance <= 1
         + the blocks of K between the linked node pairs             (preconditioned_matrix)
    M^-1 r = T^-1 r on the chain columns, r / diag(K) elsewhere

The float-storage model (model_solve) is the reference for the float-factor figures: every chain's banded Cholesky factor of
T (scipy.linalg.cholesky_banded, a sequential elimination from the first node to the last) rounded to float32, T32 = C32'C32
rebuilt, the link blocks added in double, and the sparse system solved by SuperLU.  It is not a restatement of the kernels:
they eliminate in a nested-dissection order, join segments through a second level and solve a capacitance system."""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from score_amd.assemble import assemble
from score_amd.manhattan import make_manhattan, make_manhattan_3d
from score_amd.solver import ConicSolver

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
RHO, SIGMA = 0.37, 1e-6
ADMM_SETTINGS = dict(rho=RHO, sigma=SIGMA, adaptive_rho=0, adaptive_cg=0, polish=0, check_interval=5)
ADMM_VECS = ("xt", "kx", "p", "w", "r", "z")


# ---------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------
SYNTH_B = dict(n_robots=3, n_poses=50, n_beacons=3, seed=12, n_loop_closures=4)  # the synth_b fixture of conftest.SYNTH

GRAPHS = {
    "A": lambda: make_manhattan(n_robots=2, n_poses=60, n_beacons=3, seed=21),
    "B": lambda: make_manhattan(**SYNTH_B),
    "C255": lambda: make_manhattan(n_robots=2, n_poses=255, n_beacons=3, seed=21),
    "C1023": lambda: make_manhattan(n_robots=2, n_poses=1023, n_beacons=3, seed=21),
    "C1024": lambda: make_manhattan(n_robots=2, n_poses=1024, n_beacons=3, seed=21),
    "D300": lambda: make_manhattan(n_robots=3, n_poses=300, n_beacons=3, seed=21),
    "D1023": lambda: make_manhattan(n_robots=3, n_poses=1023, n_beacons=3, seed=21),
    "E40": lambda: make_manhattan_3d(n_robots=2, n_poses=40, n_beacons=3, seed=32, p_range=0.3),
    "E60": lambda: make_manhattan_3d(n_robots=2, n_poses=60, n_beacons=3, seed=32, p_range=0.3, n_loop_closures=2),
    "E1100": lambda: make_manhattan_3d(n_robots=1, n_poses=1100, n_beacons=3, seed=32, p_range=0.3),
    "F": lambda: make_manhattan(n_robots=4, n_poses=700, n_beacons=2, seed=60, p_range=0.3),
    "S150": lambda: make_manhattan(n_robots=1, n_poses=150, n_beacons=2, seed=2, p_range=0.6),
    "H": lambda: make_manhattan(n_robots=2, n_poses=1100, n_beacons=3, seed=21, n_loop_closures=3),
}
# a case: the graphs of one handle (G: a lock-step batch whose tiles straddle problems)
CASE_GRAPHS = {k: (k,) for k in GRAPHS if k != "S150"}
CASE_GRAPHS["G"] = ("A", "B", "S150")


@functools.lru_cache(maxsize=None)
def model_of(name):
    """(graph, assembled model) of a named graph; shared by every test of a session and never changed."""
    fg = GRAPHS[name]()
    return fg, assemble(fg, "SOCP")


def case_models(case):
    return [model_of(g) for g in CASE_GRAPHS[case]]


# ---------------------------------------------------------------------------------------------------------------------
# long-double products
# ---------------------------------------------------------------------------------------------------------------------
def ld_matvec(M, v, absolute=False):
    """M v (or |M| |v|) with every row accumulated in np.longdouble."""
    M = M.tocsr()
    data, vec = M.data.astype(LD), np.asarray(v).astype(LD)
    if absolute:
        data, vec = np.abs(data), np.abs(vec)
    prod = data * vec[M.indices]
    out = np.zeros(M.shape[0], dtype=LD)
    full = np.diff(M.indptr) > 0
    if prod.size:
        out[full] = np.add.reduceat(prod, M.indptr[:-1][full])
    return out


def norm_inf_matrix(M):
    M = M.tocsr()
    return float(ld_matvec(M, np.ones(M.shape[1]), absolute=True).max()) if M.nnz else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def reference_K(qp, D, E, rho=RHO, sigma=SIGMA):
    """K = D P D + sigma I + rho (E A D)'(E A D) from the problem data and the handle's scales (which
    test_device_setup_against_scipy pins), all d replicas and the tail: the full matrix the problem defines."""
    n = qp.n
    Ps = sp.diags(D) @ qp.P @ sp.diags(D)
    As = sp.diags(E) @ qp.A @ sp.diags(D)
    K = (Ps + sigma * sp.identity(n) + rho * (As.T @ As)).tocsr()
    K.sum_duplicates()
    K.sort_indices()
    return K


def chain_nodes_of_problem(qp):
    """Per column: (chain, node within the chain) from the chain hint of the problem, -1 off the chains."""
    n, bs = qp.n, int(qp.block_size)
    chain, node = -np.ones(n, dtype=np.int64), -np.ones(n, dtype=np.int64)
    cols = np.asarray(qp.node_cols, dtype=np.int64).reshape(-1, bs)
    cp = np.asarray(qp.chain_ptr, dtype=np.int64)
    for c in range(len(cp) - 1):
        for j in range(cp[c], cp[c + 1]):
            chain[cols[j]] = c
            node[cols[j]] = j - cp[c]
    return chain, node


def chain_nodes_of_ids(chain_id, bs):
    """The same from a per-column chain id whose chains own consecutive columns (score_debug_get "chain_id_of_col")."""
    chain = np.asarray(chain_id).astype(np.int64)
    n = chain.size
    first = np.full(chain.max() + 2, n, dtype=np.int64)
    np.minimum.at(first, chain[chain >= 0], np.nonzero(chain >= 0)[0])
    node = np.where(chain >= 0, (np.arange(n) - first[np.maximum(chain, 0)]) // bs, -1)
    return chain, node


def loop_closure_pairs(fg, mdl):
    """First columns (one pair per matrix row k of the pose blocks) of the node pairs the graph's loop closures couple
    outside the chains: both ends free poses, not neighbours in a chain, every pair once.  From the graph and the
    assembler's column maps only."""
    d, qp = mdl.dim, mdl.qp
    D1, PB = d + 1, d * (d + 1)
    new_of_model = -np.ones(mdl.n_model, dtype=np.int64)
    new_of_model[mdl.free_cols] = np.arange(qp.n)
    idx = {nm: i for i, nm in enumerate(mdl.pose_names)}
    chain, node = chain_nodes_of_problem(qp)
    out = set()
    for meas in fg.loop_closure_measurements:
        i, j = idx[meas.base_pose], idx[meas.to_pose]
        if i == j:
            continue
        for k in range(d):
            ca, cb = int(new_of_model[i * PB + k * D1]), int(new_of_model[j * PB + k * D1])
            if ca < 0 or cb < 0:
                continue  # the pinned pose is a constant
            assert chain[ca] >= 0 and chain[cb] >= 0
            if chain[ca] == chain[cb] and abs(node[ca] - node[cb]) == 1:
                continue  # a second odometry edge: inside the chain
            out.add((min(ca, cb), max(ca, cb)))
    return sorted(out)


def preconditioned_matrix(M, chain, node, bs, pairs):
    """The matrix whose exact inverse the chain preconditioner applies on the chain columns: the entries of M whose
    columns lie in the same chain at node distance <= 1, plus the blocks of M between the linked node pairs (first
    columns).  Returns (T, chain-column mask)."""
    n = M.shape[0]
    coo = M.tocoo()
    keep = (chain[coo.row] >= 0) & (chain[coo.row] == chain[coo.col]) & (np.abs(node[coo.row] - node[coo.col]) <= 1)
    for ca, cb in pairs:
        ra, rb = (coo.row >= ca) & (coo.row < ca + bs), (coo.row >= cb) & (coo.row < cb + bs)
        keep |= (ra & (coo.col >= cb) & (coo.col < cb + bs)) | (rb & (coo.col >= ca) & (coo.col < ca + bs))
    T = sp.csr_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=(n, n))
    return T, chain >= 0


def model_solve(T, qp, rhs, float_factors):
    """Reference 3.  Every chain's banded Cholesky factor C of its block-tridiagonal part of T (upper form), kept as it is or
    rounded to float32 and back; the chains' C'C and the double-precision blocks of T outside the chains' bands (the link
    blocks) as one sparse matrix on the chain columns; SuperLU solves it for rhs.  Returns z on all columns (0 off the chains)."""
    bs = int(qp.block_size)
    cols_all = np.asarray(qp.node_cols, dtype=np.int64)
    cp = np.asarray(qp.chain_ptr, dtype=np.int64) * bs
    chain, node = chain_nodes_of_problem(qp)
    n = T.shape[0]
    u = 2 * bs - 1
    Tc = T.tocsr()
    coo = Tc.tocoo()
    band = (chain[coo.row] >= 0) & (chain[coo.row] == chain[coo.col]) & (np.abs(node[coo.row] - node[coo.col]) <= 1)
    rows, cls, vals = [coo.row[~band]], [coo.col[~band]], [coo.data[~band]]  # the link blocks, in double
    for c in range(len(cp) - 1):
        cols = cols_all[cp[c] : cp[c + 1]]
        m = cols.size
        sub = Tc[cols][:, cols].tocoo()
        ab = np.zeros((u + 1, m))
        up = (sub.col >= sub.row) & (sub.col // bs - sub.row // bs <= 1)  # (a loop closure inside the chain is a link block)
        ab[u + sub.row[up] - sub.col[up], sub.col[up]] = sub.data[up]
        cb = sla.cholesky_banded(ab, lower=False)
        if float_factors:
            cb = cb.astype(np.float32).astype(np.float64)
        # C as a sparse upper-triangular matrix: C[i, j] = cb[u + i - j, j]
        jj = np.tile(np.arange(m), (u + 1, 1))
        ii = jj - u + np.arange(u + 1)[:, None]
        ok = ii >= 0
        C = sp.csr_matrix((cb[ok], (ii[ok], jj[ok])), shape=(m, m))
        Tm = (C.T @ C).tocoo()
        rows.append(cols[Tm.row]); cls.append(cols[Tm.col]); vals.append(Tm.data)
    full = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cls))), shape=(n, n))
    on = np.nonzero(chain >= 0)[0]
    z = np.zeros(n)
    if on.size:
        z[on] = spla.splu(full[on][:, on].tocsc()).solve(np.asarray(rhs, dtype=np.float64)[on])
    return z


# ---------------------------------------------------------------------------------------------------------------------
# the figures
# ---------------------------------------------------------------------------------------------------------------------
def i1_figures(K, p, w, z, cg_iters):
    """I1, w = K p, row by row.  With one PCG iteration the last product of a solve is w = K p itself; with more it is
    w = K z + beta w_old with p = z + beta p_old (the KPB launch: one gather per nonzero), where w_old = K p_old up to its
    own error.  A row of L terms summed in any order carries (L - 1 + 1) eps (|K| |v|)_i; the update adds two more roundings,
    so one product contributes at most (L + 4) eps (|K| (|z| + |beta p_old|))_i, and beta p_old = p - z gives
    |z| + |beta p_old| <= |p| + 2 |z|.  Each of the cg_iters products of the solve adds such a term through the recurrence:

        |w - K p|_i  <=  cg_iters (L + 4) eps (|K| (|p| + 2 |z|))_i,        L = the longest row of K.

    (z is the vector read back, the preconditioned residual of the launch that ends the iteration.)  Rows whose scale is 0
    are left out of the ratio and must be equal exactly.  Returns (worst ratio to the bound, every zero-scale row exact)."""
    L = int(np.diff(K.indptr).max())
    err = np.abs(np.asarray(w).astype(LD) - ld_matvec(K, p))
    scale = ld_matvec(K, np.abs(np.asarray(p)).astype(LD) + 2 * np.abs(np.asarray(z)).astype(LD), absolute=True)
    bound = cg_iters * (L + 4) * LD(EPS) * scale
    live = scale > 0
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    return ratio, bool(np.all(err[~live] == 0))


def i2_figure(K, xt, kx):
    """I2: e = |kx - K xt|_inf / (|K|_inf |xt|_inf), the relative error of the carried product."""
    den = norm_inf_matrix(K) * float(np.abs(xt).max())
    return float(np.abs(np.asarray(kx).astype(LD) - ld_matvec(K, xt)).max()) / den if den > 0 else 0.0


def i2_bound(K, e_twin):
    return 8.0 * max(e_twin, (int(np.diff(K.indptr).max()) + 4) * EPS)


def eta_figure(T, on, z, rhs):
    """Normwise backward error of T z = rhs over the chain columns `on`: |T z - rhs|_inf / (|T|_inf |z|_inf + |rhs|_inf)."""
    if not on.any():
        return 0.0
    res = np.abs(ld_matvec(T, z) - np.asarray(rhs).astype(LD))[on]
    den = norm_inf_matrix(T) * float(np.abs(np.asarray(z)[on]).max()) + float(np.abs(np.asarray(rhs)[on]).max())
    return float(res.max()) / den if den > 0 else float(res.max())


def eta_bound(T, qp, on, rhs, float_factors):
    """The bound of I3 / I4: 4 * max(eta of the double model, 4 eps) with double factors, 4 * eta of the float-storage model
    with float factors.  The factor 4 covers what the model leaves out on purpose: the nested-dissection order, the join
    level and the capacitance solve against one sequential Cholesky.  Returns (bound, eta of the model)."""
    eta_m = eta_figure(T, on, model_solve(T, qp, rhs, float_factors), rhs)
    return (4.0 * eta_m if float_factors else 4.0 * max(eta_m, 4 * EPS)), eta_m


def jacobi_ok(M, on, z, rhs):
    """Off the chains the preconditioner is Jacobi: z = rhs / diag(M) to 4 eps."""
    off = ~on
    return bool(np.allclose(np.asarray(z)[off], (np.asarray(rhs)[off] / M.diagonal()[off]), rtol=4 * EPS, atol=0.0))


# ---------------------------------------------------------------------------------------------------------------------
# a handle's problems
# ---------------------------------------------------------------------------------------------------------------------
class ProblemView:
    """One problem of a handle: its slice of the handle's vectors and its references."""

    def __init__(self, fg, mdl, xoff, roff, D, E, link_pairs):
        qp = mdl.qp
        self.fg, self.mdl, self.qp, self.x0, self.x1 = fg, mdl, qp, xoff, xoff + qp.n
        self.K = reference_K(qp, D[xoff : xoff + qp.n], E[roff : roff + qp.m])
        self.chain, self.node = chain_nodes_of_problem(qp)
        self.pairs = [(a - xoff, b - xoff) for a, b in link_pairs if xoff <= a < xoff + qp.n]
        self.expected_pairs = loop_closure_pairs(fg, mdl)
        self.T, self.on = preconditioned_matrix(self.K, self.chain, self.node, int(qp.block_size), self.expected_pairs)

    def cut(self, v):
        return np.asarray(v)[self.x0 : self.x1]


def problem_views(sol, models):
    """The views of every problem of a handle created from `models` (list of (graph, model))."""
    D, E = sol.debug_get("D"), sol.debug_get("E")
    lp = sol.debug_get("link_pairs").astype(np.int64).reshape(-1, 2)
    pairs = sorted((int(min(a, b)), int(max(a, b))) for a, b in lp)
    out, xo, ro = [], 0, 0
    for fg, mdl in models:
        out.append(ProblemView(fg, mdl, xo, ro, D, E, pairs))
        xo += mdl.qp.n
        ro += mdl.qp.m
    return out


def admm_snapshots(models, settings, lib_path):
    """reset(), then steps(5) twice with the fixed settings: both end in a measured iteration (the last launch applies the
    preconditioner to the final residual, so z = M^-1 r for the r read back).  Returns (views, [vectors after 5, after 10])."""
    sol = ConicSolver([m.qp for _, m in models], dict(ADMM_SETTINGS, **settings), lib_path=lib_path)
    try:
        views = problem_views(sol, models)
        sol.reset()
        snaps = []
        for _ in range(2):
            sol.steps(5)
            snaps.append({v: sol.debug_get(v) for v in ADMM_VECS})
    finally:
        sol.close()
    return views, snaps


def admm_figures(view, vec, cg_iters, float_factors):
    """Every figure of I1-I3 for one problem and one snapshot, as a dict."""
    p, w, r, z, xt, kx = (view.cut(vec[k]) for k in ("p", "w", "r", "z", "xt", "kx"))
    ratio, exact = i1_figures(view.K, p, w, z, cg_iters)
    bound, eta_m = eta_bound(view.T, view.qp, view.on, r, float_factors)
    return dict(i1=ratio, i1_exact=exact, i2=i2_figure(view.K, xt, kx), i3=eta_figure(view.T, view.on, z, r),
                i3_bound=bound, i3_model=eta_m, jacobi=jacobi_ok(view.K, view.on, z, r), pairs_ok=view.pairs == view.expected_pairs)


def newton_snapshot(model, settings, lib_path=None):
    """I4: 15 ADMM iterations, then the Newton set assembled and factored at that iterate (what the first Newton iteration
    does) and z = M^-1 (-g) from PREC_INIT on it.  Returns (H as the device assembled it, g, z, link pairs of the handle)."""
    qp = model.qp
    sol = ConicSolver(qp, settings, lib_path=lib_path)
    try:
        sol.reset()
        sol.steps(15)
        assert sol.debug_get("polish_assemble_at_x").size == 1
        n = qp.n
        H = sp.csr_matrix((sol.debug_get("Hval"), sol.debug_get("Hcol").astype(np.int64), sol.debug_get("Hptr").astype(np.int64)), shape=(n, n))
        g, z = sol.debug_get("polish_g"), sol.debug_get("polish_prec_of_negg")
        lp = sol.debug_get("link_pairs").astype(np.int64).reshape(-1, 2)
    finally:
        sol.close()
    return H, g, z, sorted((int(min(a, b)), int(max(a, b))) for a, b in lp)


def newton_figures(fg, model, H, g, z, pairs, float_factors):
    """The figures of I4 for one problem: T_H z = -g on the chain columns, Jacobi elsewhere."""
    qp = model.qp
    chain, node = chain_nodes_of_problem(qp)
    expected = loop_closure_pairs(fg, model)
    T, on = preconditioned_matrix(H, chain, node, int(qp.block_size), expected)
    bound, eta_m = eta_bound(T, qp, on, -g, float_factors)
    return dict(i4=eta_figure(T, on, z, -g), i4_bound=bound, i4_model=eta_m, jacobi=jacobi_ok(H, on, z, -g), pairs_ok=pairs == expected)
