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
they eliminate in a nested-dissection order, join segments through a second level and solve a capacitance system.

The second half of the file runs the loop as the benchmark drives it (penalty_update_run, changing_cg_run,
replay_and_single_steps: 16-iteration blocks replayed from a captured graph, a penalty update at every check, a PCG count that
changes between blocks) and models one iteration in np.longdouble (iteration_model: the right-hand side, the relaxation, the
cone projections and the dual update, with forward-error bounds counted operation by operation).  K and T are built at each
problem's own penalty, read back from the handle (score_debug_get "rho").

LINK_GRAPHS / LINK_PLANS put the loop-closure link plan (score_link.hpp) at its caps and one step beyond each; a view then takes
"the pairs expected inside the preconditioner" (case_inside): every loop closure of the graph, or none beyond a cap, where T
is the chain part alone (test_link_caps_gpu.py, test_link_caps_host.py)."""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from score_amd import compat
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


def lc(fg, rng, a, i, b, j):
    """A loop closure from pose i of robot a to pose j of robot b, as test_loop_closure_edge_cases_in_the_link_correction
    builds it: the true relative pose plus noise of 0.01 / 0.01 / 0.002 (2-D: x, y, theta; 3-D: 0.01 on the translation, the
    true rotation) from `rng`, kappa = 1e4, tau = 2.5e5."""
    A, B = fg.pose_variables[a][i], fg.pose_variables[b][j]
    rel = np.linalg.inv(A.transformation_matrix) @ B.transformation_matrix
    if fg.dimension == 3:
        return compat.PoseMeasurement3D(A.name, B.name, rel[:3, 3] + 0.01 * rng.standard_normal(3), rel[:3, :3].copy(), 1e4, 2.5e5)
    return compat.PoseMeasurement2D(A.name, B.name, float(rel[0, 2] + 0.01 * rng.standard_normal()), float(rel[1, 2] + 0.01 * rng.standard_normal()),
                                    float(np.arctan2(rel[1, 0], rel[0, 0]) + 0.002 * rng.standard_normal()), 1e4, 2.5e5)


def with_loop_closures(fg, ends):
    """`fg` with the loop closures lc(a, i, b, j) of `ends`, the noise drawn in list order from np.random.default_rng(5)."""
    rng = np.random.default_rng(5)
    fg.loop_closure_measurements = [lc(fg, rng, *e) for e in ends]
    return fg


# The link plan at its caps (score_link.hpp: 96 unknowns in a group, 48 rounds on a chain, 256 linked nodes in a problem), one
# step beyond each of them (the all-or-nothing fallbacks of make_link_plan: L97, R3over, N260) and the kernel variants below
# the caps that the generators' own loop closures never reach: LINK_PLANS lists what each graph must give.
_PAIRED = lambda n_pairs, per_pair: [(2 * pr, 2 + 2 * k, 2 * pr + 1, 33 - 2 * k) for pr in range(n_pairs) for k in range(per_pair)]
_RING = [e for k in range(6) for e in ((0, 2 + 2 * k, 1, 3 + 2 * k), (1, 20 + 2 * k, 2, 3 + 2 * k), (2, 20 + 2 * k, 0, 21 + 2 * k))]
LINK_GRAPHS = {
    "L96": lambda: with_loop_closures(make_manhattan(n_robots=2, n_poses=40, n_beacons=3, seed=77, p_range=0.3), [(0, 2 + 2 * k, 1, 37 - 2 * k) for k in range(16)]),
    "L97": lambda: with_loop_closures(make_manhattan(n_robots=2, n_poses=40, n_beacons=3, seed=77, p_range=0.3), [(0, 2 + 2 * k, 1, 37 - 2 * k) for k in range(17)]),
    "HUB15": lambda: with_loop_closures(make_manhattan(n_robots=1, n_poses=60, n_beacons=3, seed=80, p_range=0.4), [(0, 5, 0, 12 + 3 * k) for k in range(15)]),
    "HUB10": lambda: with_loop_closures(make_manhattan(n_robots=1, n_poses=60, n_beacons=3, seed=78, p_range=0.4), [(0, 5, 0, 12 + 3 * k) for k in range(10)]),
    "HUB93": lambda: with_loop_closures(make_manhattan(n_robots=3, n_poses=40, n_beacons=3, seed=82, p_range=0.3),
                                        [(0, 5, 1, 3 + 3 * k) for k in range(10)] + [(0, 8 + 3 * k, 2, 37 - 3 * k) for k in range(10)]),
    "R3": lambda: with_loop_closures(make_manhattan(n_robots=3, n_poses=40, n_beacons=3, seed=79, p_range=0.3), _RING[:15]),
    "R3over": lambda: with_loop_closures(make_manhattan(n_robots=3, n_poses=40, n_beacons=3, seed=79, p_range=0.3), _RING[:17]),
    "E96": lambda: with_loop_closures(make_manhattan_3d(n_robots=2, n_poses=40, n_beacons=3, seed=32, p_range=0.3), [(0, 2 + 3 * k, 1, 37 - 3 * k) for k in range(12)]),
    "N256": lambda: with_loop_closures(make_manhattan(n_robots=8, n_poses=36, n_beacons=3, seed=80, p_range=0.2), _PAIRED(4, 16)),
    "N260": lambda: with_loop_closures(make_manhattan(n_robots=10, n_poses=36, n_beacons=3, seed=80, p_range=0.2), _PAIRED(4, 16) + [(8, 10, 9, 20)]),
    "LS96": lambda: with_loop_closures(make_manhattan(n_robots=2, n_poses=1100, n_beacons=3, seed=21), [(0, 30 + 64 * k, 1, 1070 - 64 * k) for k in range(16)]),
}
GRAPHS.update(LINK_GRAPHS)
# the twin's "links" read-out: [pairs, inside the preconditioner, unknowns, chains, rounds, singular, groups, largest group, most
# chains of a group] (the HIP handle reports the first six)
LINK_PLANS = {
    "L96": [32, 32, 192, 4, 48, 0, 2, 96, 2],      # a group at the cap of 96 unknowns, 48 rounds on each of its two chains
    "L97": [34, 0, 0, 0, 0, 0, 0, 0, 0],           # 51 rounds on a chain: the chain preconditioner alone
    "HUB15": [30, 30, 96, 2, 48, 0, 2, 48, 1],     # one pose with 15 partners: rows of G with 45 nonzeros, 48 rounds on ONE chain
    "HUB93": [40, 40, 186, 6, 33, 0, 2, 93, 3],    # a hub between robots: 93 unknowns, three chains to a group
    "R3": [30, 30, 180, 6, 30, 0, 2, 90, 3],       # a ring of three robots: 90 unknowns, three chains to a group
    "R3over": [34, 0, 0, 0, 0, 0, 0, 0, 0],        # a group of 102 unknowns (36 rounds a chain are fine): none
    "E96": [36, 36, 288, 6, 48, 0, 3, 96, 2],      # 3-D: blocks of 4, three groups of 96
    "N256": [128, 128, 768, 16, 48, 0, 8, 96, 2],  # exactly 256 linked nodes: eight groups of 96
    "N260": [130, 0, 0, 0, 0, 0, 0, 0, 0],         # 258 linked nodes: none
    "LS96": [32, 32, 192, 4, 48, 0, 2, 96, 2],     # L96 on chains cut into segments: items per segment, the join level
    "HUB10": [20, 20, 66, 2, 33, 0, 2, 33, 1],
}
# The HIP backend cuts a chain beyond 1023 poses into segments (score_join.hpp) and lists an affected chain per segment (a
# LinkItem each); the twin solves whole chains.  LS96: 2 robots x 2 matrix rows x 2 segments -- the one figure of the six in
# which the two handles differ.
LINK_CHAINS_ON_DEVICE = {"LS96": 8}
LINK_FALLBACKS = ("L97", "R3over", "N260")  # no pair inside the preconditioner: T is the chain part alone
LINK_CASES = ["L96", "L97", "HUB15", "HUB93", "R3", "R3over", "E96", "N256", "N260", "LS96", "GL"]

# a case: the graphs of one handle (G, GL: a lock-step batch whose tiles straddle problems)
CASE_GRAPHS = {k: (k,) for k in GRAPHS if k not in ("S150", "HUB10")}
CASE_GRAPHS["G"] = ("A", "B", "S150")
CASE_GRAPHS["GL"] = ("L96", "A", "HUB10")  # groups of 96, none and 33 unknowns in one launch


@functools.lru_cache(maxsize=None)
def model_of(name):
    """(graph, assembled model) of a named graph; shared by every test of a session and never changed."""
    fg = GRAPHS[name]()
    return fg, assemble(fg, "SOCP")


def case_models(case):
    return [model_of(g) for g in CASE_GRAPHS[case]]


def case_inside(case):
    """Per graph of a case, the pairs expected inside the preconditioner: None = every loop closure of the graph
    (loop_closure_pairs), [] for the graphs beyond a cap of the link plan."""
    return [[] if g in LINK_FALLBACKS else None for g in CASE_GRAPHS[case]]


def case_link_plan(case):
    """The twin's "links" read-out a case must give: the members' figures added up, rounds / largest group / most chains of a
    group the largest of them."""
    plans = np.array([LINK_PLANS.get(g, [0] * 9) for g in CASE_GRAPHS[case]])
    return [int(plans[:, k].max() if k in (4, 7, 8) else plans[:, k].sum()) for k in range(9)]


def device_link_plan(case):
    """The six "links" figures the HIP handle of a case must report: the twin's first six, the chains counted per segment."""
    plan = case_link_plan(case)[:6]
    plan[3] += sum(LINK_CHAINS_ON_DEVICE[g] - LINK_PLANS[g][3] for g in CASE_GRAPHS[case] if g in LINK_CHAINS_ON_DEVICE)
    return plan


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


def link_cap_bound(eta_model, eta_twin, float_factors):
    """The bound of I3 and I4 for the DEVICE on the cases of LINK_CASES: 4 * max(eta of the model, eta of the twin), plus the 4 eps
    floor with double factors.  The model is SuperLU on the assembled matrix and never forms y - Z t; the twin does form it (a
    host restatement of the same Woodbury correction on the same plan), so with a link plan at its caps -- a pose with 15
    partners, 96 unknowns on top of the join level -- the twin's own figure is the yardstick of that cancellation, as it is of
    the carried product in I2.  The twin itself stays under eta_bound."""
    return 4.0 * max(eta_model, eta_twin, 0.0 if float_factors else 4 * EPS)


def jacobi_ok(M, on, z, rhs):
    """Off the chains the preconditioner is Jacobi: z = rhs / diag(M) to 4 eps."""
    off = ~on
    return bool(np.allclose(np.asarray(z)[off], (np.asarray(rhs)[off] / M.diagonal()[off]), rtol=4 * EPS, atol=0.0))


# ---------------------------------------------------------------------------------------------------------------------
# a handle's problems
# ---------------------------------------------------------------------------------------------------------------------
class ProblemView:
    """One problem of a handle: its slice of the handle's vectors and its references."""

    def __init__(self, fg, mdl, xoff, roff, D, E, link_pairs, rho=RHO, sigma=SIGMA, inside=None):
        qp = mdl.qp
        self.fg, self.mdl, self.qp, self.x0, self.x1 = fg, mdl, qp, xoff, xoff + qp.n
        self.r0, self.r1, self.rho, self.sigma = roff, roff + qp.m, float(rho), float(sigma)
        self.D, self.E = np.asarray(D[xoff : xoff + qp.n]), np.asarray(E[roff : roff + qp.m])
        self.K = reference_K(qp, self.D, self.E, rho=self.rho, sigma=self.sigma)
        self.pairs = [(a - xoff, b - xoff) for a, b in link_pairs if xoff <= a < xoff + qp.n]
        if fg is None:  # a general conic program: no chains, no graph
            self.chain = self.node = -np.ones(qp.n, dtype=np.int64)
            self.expected_pairs = []
        else:
            self.chain, self.node = chain_nodes_of_problem(qp)
            self.expected_pairs = loop_closure_pairs(fg, mdl) if inside is None else list(inside)
        self.T, self.on = preconditioned_matrix(self.K, self.chain, self.node, int(qp.block_size), self.expected_pairs)

    def cut(self, v):
        return np.asarray(v)[self.x0 : self.x1]

    def cut_rows(self, v):
        return np.asarray(v)[self.r0 : self.r1]


def problem_views(sol, models, rho=None, inside=None):
    """The views of every problem of a handle created from `models` (list of (graph, model)); `rho`: the penalty of every
    problem (default: RHO for all of them); `inside`: per problem, the pairs expected inside the preconditioner (case_inside;
    default: every loop closure of the graph)."""
    D, E = sol.debug_get("D"), sol.debug_get("E")
    lp = sol.debug_get("link_pairs").astype(np.int64).reshape(-1, 2)
    pairs = sorted((int(min(a, b)), int(max(a, b))) for a, b in lp)
    out, xo, ro = [], 0, 0
    for k, (fg, mdl) in enumerate(models):
        out.append(ProblemView(fg, mdl, xo, ro, D, E, pairs, rho=RHO if rho is None else float(rho[k]), inside=None if inside is None else inside[k]))
        xo += mdl.qp.n
        ro += mdl.qp.m
    return out


def links_of(sol):
    """The handle's "links" read-out as integers (six figures from the HIP library, nine from the twin)."""
    return [int(v) for v in sol.debug_get("links")]


def admm_snapshots(models, settings, lib_path, counters=None, inside=None):
    """reset(), then steps(check_interval) twice with the fixed settings (5 iterations each unless `settings` says otherwise;
    16 or more are replayed from a captured graph when use_graph = 1): both end in a measured iteration (the last launch
    applies the preconditioner to the final residual, so z = M^-1 r for the r read back).  Returns (views, [vectors after
    the first block, after the second]); `counters`, when given, receives the handle's "graph_launches", its "links" before the first
    and after the last iteration and its "link_pairs"."""
    st = dict(ADMM_SETTINGS, **settings)
    sol = ConicSolver([m.qp for _, m in models], st, lib_path=lib_path)
    try:
        views = problem_views(sol, models, inside=inside)
        if counters is not None:
            counters["links"], counters["link_pairs"] = links_of(sol), sol.debug_get("link_pairs")
        sol.reset()
        snaps = []
        for _ in range(2):
            sol.steps(st["check_interval"])
            snaps.append({v: sol.debug_get(v) for v in ADMM_VECS})
        if counters is not None:
            counters["graph_launches"] = int(sol.debug_get("graph_launches")[0])
            counters["links_after"] = links_of(sol)
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


def newton_snapshot(model, settings, lib_path=None, counters=None):
    """I4: 15 ADMM iterations, then the Newton set assembled and factored at that iterate (what the first Newton iteration
    does) and z = M^-1 (-g) from PREC_INIT on it.  Returns (H as the device assembled it, g, z, link pairs of the handle);
    `counters`, when given, receives the handle's "links" read after it."""
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
        if counters is not None:
            counters["links"] = links_of(sol)  # (after the Newton set's first refresh: both sets' singular systems counted)
    finally:
        sol.close()
    return H, g, z, sorted((int(min(a, b)), int(max(a, b))) for a, b in lp)


def newton_figures(fg, model, H, g, z, pairs, float_factors, inside=None):
    """The figures of I4 for one problem: T_H z = -g on the chain columns, Jacobi elsewhere; `inside`: the pairs expected inside
    the preconditioner (default: every loop closure of the graph)."""
    qp = model.qp
    chain, node = chain_nodes_of_problem(qp)
    expected = loop_closure_pairs(fg, model) if inside is None else list(inside)
    T, on = preconditioned_matrix(H, chain, node, int(qp.block_size), expected)
    bound, eta_m = eta_bound(T, qp, on, -g, float_factors)
    return dict(i4=eta_figure(T, on, z, -g), i4_bound=bound, i4_model=eta_m, jacobi=jacobi_ok(H, on, z, -g), pairs_ok=pairs == expected)


def newton_twin_figures(fg, model, H, g, float_factors, twin_lib, inside=None):
    """The twin as second yardstick of I4.  The twin has no Newton polish, but its linear mode (score_linear_create /
    score_linear_solve: the host restatement of chain factors, float rounding, link plan and Woodbury correction) takes any
    SPD matrix on a chain hint: handed the H the device assembled and the problem's chains, it factors H along them, finds the
    link pairs in H's pattern and applies M^-1.  A linear solve takes at least one PCG step, so the pair read back is
    (r, z = M^-1 r) with r the residual after one step from -g -- another vector of the same Krylov sequence, the same T_H, the
    same factors and the same capacitance systems.  Returns the figures of newton_figures for it (against the model on ITS
    r), its "links" and whether its pairs are the expected ones."""
    from score_amd.solver import _f64p, _ptr, LinearSolver

    qp = model.qp
    bs = int(qp.block_size)
    Hs = sp.csr_matrix(H, copy=True)
    Hs.sum_duplicates()
    Hs.sort_indices()
    ls = LinearSolver(Hs, qp.chain_ptr, np.asarray(qp.node_cols)[::bs], bs, dict(fac_fp32=1 if float_factors else 0), lib_path=twin_lib)

    def read(name):
        size = ls.lib.score_debug_get(ls._h, name.encode(), None, 0)
        out = np.empty(size)
        ls.lib.score_debug_get(ls._h, name.encode(), _ptr(out, _f64p), size)
        return out

    try:
        ls.solve(Hs.data, -np.asarray(g), rel_tol=1e-30, max_iters=1)
        r, z, links = read("r"), read("z"), [int(v) for v in read("links")]
        lp = read("link_pairs").astype(np.int64).reshape(-1, 2)
    finally:
        ls.close()
    pairs = sorted((int(min(a, b)), int(max(a, b))) for a, b in lp)
    f = newton_figures(fg, model, H, -r, z, pairs, float_factors, inside=inside)
    return dict(f, links=links, r_max=float(np.abs(r).max()))


# ---------------------------------------------------------------------------------------------------------------------
# the loop as the benchmark drives it: penalty updates, a changing PCG count, replayed graphs
# ---------------------------------------------------------------------------------------------------------------------
BLOCK = 16  # iterations per block: the shortest one HipBackend::run replays from a captured graph
RHO_SETTINGS = dict(ADMM_SETTINGS, adaptive_rho=1, adaptive_rho_interval=BLOCK, adaptive_rho_tol=1.0, check_interval=BLOCK, use_graph=1,
                    max_iters=3 * BLOCK, eps_abs=1e-30, eps_rel=1e-30, polish=0, adaptive_cg=0, cg_iters=2)
CG_SETTINGS = dict(RHO_SETTINGS, adaptive_rho=0, adaptive_cg=1, cg_iters=2, max_cg_iters=6, cg_target=1e-12)
ALPHA = 1.8  # score_default_settings


def scaled_data(view):
    """As = E A D, bs = E b, qs = D q of a problem in np.longdouble (entries of As on the pattern of A, duplicates summed).
    Returns (A pattern as CSR with double values, the np.longdouble values of As in that order, bs, qs)."""
    qp = view.qp
    A = sp.csr_matrix(qp.A, copy=True)
    A.sum_duplicates()
    A.sort_indices()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    vals = view.E.astype(LD)[rows] * A.data.astype(LD) * view.D.astype(LD)[A.indices]
    return A, vals, view.E.astype(LD) * np.asarray(qp.b).astype(LD), view.D.astype(LD) * np.asarray(qp.q).astype(LD)


def _ld_rows(A, vals, v, absolute=False):
    """(A with np.longdouble values `vals`) v, row by row in np.longdouble."""
    vec = np.asarray(v).astype(LD)
    data = vals
    if absolute:
        data, vec = np.abs(data), np.abs(vec)
    prod = data * vec[A.indices]
    out = np.zeros(A.shape[0], dtype=LD)
    full = np.diff(A.indptr) > 0
    if prod.size:
        out[full] = np.add.reduceat(prod, A.indptr[:-1][full])
    return out


def _ld_cols(A, vals, v, absolute=False):
    """(A with np.longdouble values `vals`)' v in np.longdouble."""
    vec = np.asarray(v).astype(LD)
    data = vals
    if absolute:
        data, vec = np.abs(data), np.abs(vec)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    order = np.argsort(A.indices, kind="stable")
    prod = (data * vec[rows])[order]
    cols = A.indices[order]
    out = np.zeros(A.shape[1], dtype=LD)
    if prod.size:
        first = np.nonzero(np.r_[True, cols[1:] != cols[:-1]])[0]
        out[cols[first]] = np.add.reduceat(prod, first)
    return out


def _sum_by_key(keys, *vals):
    """Entries with equal keys added up (np.longdouble); returns (sorted unique keys, sums ..., counts)."""
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    first = np.nonzero(np.r_[True, keys[1:] != keys[:-1]])[0] if keys.size else np.zeros(0, dtype=np.int64)
    sums = [np.add.reduceat(v[order], first) if keys.size else np.zeros(0, dtype=LD) for v in vals]
    counts = np.diff(np.r_[first, keys.size])
    return (keys[first], *sums, counts)


def _lookup(keys, vals, query):
    pos = np.minimum(np.searchsorted(keys, query), max(keys.size - 1, 0))
    hit = (keys[pos] == query) if keys.size else np.zeros(query.shape, dtype=bool)
    return np.where(hit, vals[pos] if keys.size else 0, 0).astype(vals.dtype), hit


def reference_K_parts(view):
    """K0 = D P D + sigma I and K1 = As'As of a problem, entry by entry in np.longdouble from the problem data and D, E:
    (keys i * n + j, K0), (keys, K1, sum of |terms| of K1, number of terms of K1)."""
    qp, n = view.qp, view.qp.n
    P = sp.coo_matrix(qp.P)
    Dl = view.D.astype(LD)
    k0_keys = np.r_[P.row.astype(np.int64) * n + P.col, np.arange(n, dtype=np.int64) * (n + 1)]
    k0_vals = np.r_[Dl[P.row] * P.data.astype(LD) * Dl[P.col], np.full(n, LD(view.sigma))]
    k0k, k0v, _ = _sum_by_key(k0_keys, k0_vals)
    A, vals, _, _ = scaled_data(view)
    lens = np.diff(A.indptr)
    keys, terms = [], []
    for r in np.unique(lens[lens > 0]):
        rows = np.nonzero(lens == r)[0]
        at = A.indptr[rows][:, None] + np.arange(r)[None, :]
        idx, val = A.indices[at].astype(np.int64), vals[at]
        keys.append((idx[:, :, None] * n + idx[:, None, :]).ravel())
        terms.append((val[:, :, None] * val[:, None, :]).ravel())
    keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
    terms = np.concatenate(terms) if terms else np.zeros(0, dtype=LD)
    k1k, k1v, k1a, k1c = _sum_by_key(keys, terms, np.abs(terms))
    return (k0k, k0v), (k1k, k1v, k1a, k1c)


def stored_rows(view, rep):
    """The rows of a problem the stored K holds: all of them, or -- a problem run with `rep` replicas -- replica 0's and
    the tail's."""
    n, nr = view.qp.n, int(getattr(view.qp, "rep_n", 0))
    local = np.arange(n)
    return np.ones(n, dtype=bool) if rep <= 1 else ((local < nr) | (local >= rep * nr))


def kval_figures(view, rho, Kptr, Kcol, Kval, rep):
    """Step 2a: the stored values of K = K0 + rho K1 of one problem against K0, K1 from the problem data, entry by entry on
    the CSR pattern of the handle (score_debug_get "Kptr" / "Kcol": a replicated K holds replica 0's rows and the tail's, with
    the columns of the full matrix).  Where the product streams a band view instead (case F), the copy k_band_pack makes of
    these values is not read here: it is held through the fresh kx = K xt of the same step and through I1.

    k_kval computes K0[k] + rho * K1[k]: one product and one sum (or one fused operation) on the stored K0, K1.  Were those
    the correctly rounded values of the exact ones, the entry would carry 1/2 eps each from K0 and K1, 1/2 eps from the
    product and 1/2 eps from the sum: |Kval - K|  <=  3 eps (|K0| + rho |K1|) with room to spare -- the bound of the test.
    The stored K0 = fl(fl(P D_j) D_i) (+ sigma on the diagonal) and K1 = the double sum of t products of twice-rounded
    entries of As are not correctly rounded; operation by operation they give (eps/2) (5 |K0| + rho (t + 6) sum|terms|),
    returned as the second ratio (t = the terms of the entry; the test prints it beside the first).

    Returns dict(ratio: worst |Kval - K_ref| / bound over the entries with a positive bound, exact: the others equal their
    reference exactly, complete: every nonzero of the reference on a stored row is on the pattern and no other row holds
    an entry, ratio_ops: the worst ratio to the operation count's bound, worst: (row, column) of `ratio`)."""
    n = view.qp.n
    (k0k, k0v), (k1k, k1v, k1a, k1c) = reference_K_parts(view)
    ptr = np.asarray(Kptr).astype(np.int64)[view.x0 : view.x1 + 1]
    col = np.asarray(Kcol).astype(np.int64)[ptr[0] : ptr[-1]] - view.x0
    val = np.asarray(Kval)[ptr[0] : ptr[-1]].astype(LD)
    row = np.repeat(np.arange(n), np.diff(ptr))
    stored = stored_rows(view, rep)
    in_range = bool(np.all((col >= 0) & (col < n)))
    keys = row * n + col
    k0, _ = _lookup(k0k, k0v, keys)
    k1, _ = _lookup(k1k, k1v, keys)
    k1abs, _ = _lookup(k1k, k1a, keys)
    t, _ = _lookup(k1k, k1c.astype(np.int64), keys)
    r = LD(rho)
    err = np.abs(val - (k0 + r * k1))
    bound = 3 * LD(EPS) * (np.abs(k0) + r * np.abs(k1))
    ops = LD(EPS) / 2 * (5 * np.abs(k0) + r * (t + 6) * k1abs)
    live = bound > 0
    ratios = np.where(live, err / np.where(live, bound, 1), 0)
    worst = int(np.argmax(ratios)) if ratios.size else 0
    # every nonzero of the reference on a stored row must be on the pattern
    ref_keys = np.union1d(k0k[k0v != 0], k1k[k1v != 0])
    ref_keys = ref_keys[stored[ref_keys // n]]
    complete = in_range and bool(np.all(np.isin(ref_keys, keys))) and bool(np.all(stored[row]))
    return dict(ratio=float(ratios.max()) if ratios.size else 0.0, exact=bool(np.all(err[~live] == 0)), complete=complete,
                ratio_ops=float((err[ops > 0] / ops[ops > 0]).max()) if np.any(ops > 0) else 0.0,
                worst=(int(row[worst]), int(col[worst])) if ratios.size else (0, 0), terms=int(t.max()) if t.size else 0)


def u_refresh_figures(view, rho, u, y, s):
    """Step 2a, k_refresh_u: u = rho (bs - s) - y row by row.  The kernel rounds three times (difference, product,
    difference) and reads bs = fl(E b): |u - u_ref|_i <= 3 eps (rho (|bs| + |s|) + |y|)_i.  Returns (worst ratio, rows with a
    zero bound equal exactly)."""
    _, _, bs, _ = scaled_data(view)
    r, sl, yl = LD(rho), view.cut_rows(s).astype(LD), view.cut_rows(y).astype(LD)
    err = np.abs(view.cut_rows(u).astype(LD) - (r * (bs - sl) - yl))
    bound = 3 * LD(EPS) * (r * (np.abs(bs) + np.abs(sl)) + np.abs(yl))
    live = bound > 0
    return (float((err[live] / bound[live]).max()) if live.any() else 0.0), bool(np.all(err[~live] == 0))


def fresh_product_figures(K, xt, kx):
    """Step 2a: kx = K xt as ONE fresh product (HipBackend::upload_rho recomputes it after K changed) -- the cg_iters = 1
    form of I1 without a direction update: |kx - K xt|_i <= (L + 4) eps (|K| |xt|)_i.  Returns (worst ratio, zero rows exact)."""
    L = int(np.diff(K.indptr).max())
    err = np.abs(np.asarray(kx).astype(LD) - ld_matvec(K, xt))
    bound = (L + 4) * LD(EPS) * ld_matvec(K, xt, absolute=True)
    live = bound > 0
    return (float((err[live] / bound[live]).max()) if live.any() else 0.0), bool(np.all(err[~live] == 0))


def penalty_update_run(models, settings, lib_path, iteration_after=False, through_reset=True, inside=None):
    """The sequence of part 2 on one handle: solve() with RHO_SETTINGS (three blocks of 16 iterations, a penalty update after
    each, none latched), the read-outs of step a, steps(16) (step b: one replay under the new penalties), optionally one
    more iteration for the long-double model (iteration_capture), and -- unless through_reset is off -- reset() and
    steps(16) twice (step c).  Returns a dict; every view is built from the problem data, D, E and the penalties read back."""
    st = dict(RHO_SETTINGS, **settings)
    sol = ConicSolver([m.qp for _, m in models], st, lib_path=lib_path)
    out = dict(settings=st)
    try:
        out["infos"] = [o.info for o in sol.solve()]
        out["rho"] = sol.debug_get("rho")
        out["a"] = {k: sol.debug_get(k) for k in ("Kval", "Kptr", "Kcol", "u", "y", "s", "xt", "kx")}
        out["rep"] = int(sol.debug_get("rep")[0])
        out["views"] = problem_views(sol, models, rho=out["rho"], inside=inside)
        out["links"] = links_of(sol)
        sol.steps(BLOCK)
        out["b"] = {v: sol.debug_get(v) for v in ADMM_VECS}
        if iteration_after:
            out["iteration"] = iteration_capture(sol)
        if not through_reset:
            return out
        sol.reset()
        out["rho_reset"] = sol.debug_get("rho")
        out["views_reset"] = problem_views(sol, models, inside=inside)
        out["c"] = []
        for _ in range(2):
            sol.steps(BLOCK)
            out["c"].append({v: sol.debug_get(v) for v in ADMM_VECS})
        out["graph_launches"] = int(sol.debug_get("graph_launches")[0])
    finally:
        sol.close()
    return out


def cg_rule(cg_now, worst, st):
    """The PCG count the driver chooses after a check: one more below 4, half as many again from 4 on, up to max_cg_iters,
    when the worst measured reduction exceeds cg_target; fewer when it is far below.  A restatement of the rule in
    Driver::check (score_driver.hpp, adaptive_cg) that must follow it: changing_cg_checks infers every check's verdict from
    the counts this rule predicts, and would infer nothing if the two drifted apart (its "sequence" check pins 2, 3, 4, 6)."""
    if worst > st["cg_target"]:
        return min(st["max_cg_iters"], cg_now + 1 if cg_now < 4 else cg_now + cg_now // 2)
    if worst < 0.01 * st["cg_target"] and cg_now > st["cg_iters"]:
        return max(st["cg_iters"], cg_now - max(1, cg_now // 4))
    return cg_now


# ---------------------------------------------------------------------------------------------------------------------
# one iteration against a long-double model
# ---------------------------------------------------------------------------------------------------------------------
ITER_VECS = ("x", "y", "s", "u", "xt", "r")


def iteration_capture(sol):
    """x0, y0, s0 as the handle holds them, then steps(1) -- a single measuring iteration, nothing deferred -- and
    x1, y1, s1, u1, xt1, r1 (all in the solver's scaled variables)."""
    before = {k + "0": sol.debug_get(k) for k in ("x", "y", "s")}
    sol.steps(1)
    return dict(before, **{k + "1": sol.debug_get(k) for k in ITER_VECS})


def cone_layout(qp):
    """(first row of every cone, its rows, SOC or zero) -- the z zero rows one cone each, then the second-order cones."""
    dims = np.r_[np.ones(int(qp.z), dtype=np.int64), np.asarray(qp.soc_dims, dtype=np.int64)]
    return np.r_[0, np.cumsum(dims)[:-1]].astype(np.int64), dims, np.r_[np.zeros(int(qp.z), dtype=bool), np.ones(len(qp.soc_dims), dtype=bool)]


def iteration_model(view, cap, alpha=ALPHA):
    """One ADMM iteration of a problem in np.longdouble from its data (As = E A D, bs, qs), alpha, sigma and its penalty rho,
    given x0, y0, s0 and the xt1 the PCG produced:

        v = alpha (bs - As xt1) + (1 - alpha) s0          w = v - y0 / rho           s_ref = Proj_K(w), zero cones -> 0
        y_ref = y0 + rho (s_ref - v)                      u_ref = rho (bs - s_ref) - y_ref
        x_ref = alpha xt1 + (1 - alpha) x0                rhs_ref = sigma x0 - qs + As'(rho (bs - s0) - y0)   (= r1 + K xt1)

    and the forward-error bounds of the kernels' arithmetic, every rounding counted with eps = 2^-52 (twice the unit
    roundoff: the margin over first order).  L_i = entries of row i of As (at most 2 in a SCORE model).

      v   k_cone / k_cone_wave: the row product sums L_i products of entries rounded twice at setup (L_i + 2 roundings on
          |As||xt1|), bs = fl(E b) (1), the difference (1), the product with alpha (1), fl(1 - alpha) and its product with s0
          (2), the sum (1):                     e_v = eps (|alpha| (4 |bs| + (L_i + 5) |As||xt1|) + 3 |1 - alpha| |s0|)
      w   fl(1 / rho), its product with y0, the difference (on |w| <= |v| + |y0| / rho):
                                                e_w = eps (|alpha| (5 |bs| + (L_i + 6) |As||xt1|) + 4 |1 - alpha| |s0| + 3 |y0| / rho)
      s   per cone, in the 2-norm: the projection is 1-Lipschitz, so the error of w passes at most unchanged; soc_scales rounds
          the squared tail norm (dim - 1 roundings, halved by the root, + 1), the mean (1), the quotient (1) and the scaled tail
          (1) -- at most (dim + 5) roundings on |w|_2 (a branch taken the other way at a boundary moves s by less, the
          projection being continuous):         B_s = |e_w|_2 + (dim + 5) eps |w|_2          (zero cones: s = 0 exactly)
      y   row by row: rho (B_s + e_v) from s and v, the difference, the product, the sum:
                                                B_y = rho (B_s + e_v) + eps (3 rho (|s_ref| + |v|) + |y0|)
      u   the same three operations on bs (rounded), s and y:
                                                B_u = rho (eps |bs| + B_s) + B_y + eps (3 rho (|bs| + |s_ref|) + |y_ref|)
      x   k_xupdate: two products, fl(1 - alpha), one sum:   B_x = 3 eps (|alpha| |xt1| + |1 - alpha| |x0|)

    No bound holds a free constant; rows and cones whose bound is 0 must be equal exactly.  The right-hand-side identity
    carries the PCG recurrence's error (r1 + kx1 telescopes exactly, kx1 = K xt1 only up to I2), so its figure is normwise with
    the twin's own as yardstick (rhs_figure).  Returns a dict of the references, the bounds and `branch` per cone:
    0 zero cone, 1 inside (kept), 2 polar (-> 0), 3 outside (projected onto the boundary)."""
    qp = view.qp
    A, vals, bs, qs = scaled_data(view)
    rho, al, sig, eps = LD(view.rho), LD(alpha), LD(view.sigma), LD(EPS)
    x0, y0, s0, xt1 = (view.cut(cap["x0"]).astype(LD), view.cut_rows(cap["y0"]).astype(LD), view.cut_rows(cap["s0"]).astype(LD),
                       view.cut(cap["xt1"]).astype(LD))
    Lr = np.diff(A.indptr).astype(LD)
    axt, axt_abs = _ld_rows(A, vals, xt1), _ld_rows(A, vals, xt1, absolute=True)
    v = al * (bs - axt) + (1 - al) * s0
    w = v - y0 / rho
    first, dims, soc = cone_layout(qp)
    head = np.zeros(qp.m, dtype=bool)
    head[first] = True
    cone_of_row = np.repeat(np.arange(first.size), dims)
    t0 = w[first]
    nz = np.sqrt(np.add.reduceat(np.where(head, 0, w * w), first))
    branch = np.where(~soc, 0, np.where(nz <= t0, 1, np.where(nz <= -t0, 2, 3)))
    mean = (t0 + nz) / 2
    head_val = np.where(branch == 1, t0, np.where(branch == 3, mean, 0))
    tail_fac = np.where(branch == 1, 1, np.where(branch == 3, mean / np.where(nz > 0, nz, 1), 0))
    s_ref = np.where(head, head_val[cone_of_row], tail_fac[cone_of_row] * w)
    y_ref = y0 + rho * (s_ref - v)
    u_ref = rho * (bs - s_ref) - y_ref
    x_ref = al * xt1 + (1 - al) * x0
    u0 = rho * (bs - s0) - y0
    rhs_ref = sig * x0 - qs + _ld_cols(A, vals, u0)
    rhs_scale = sig * np.abs(x0) + np.abs(qs) + _ld_cols(A, vals, rho * (np.abs(bs) + np.abs(s0)) + np.abs(y0), absolute=True)
    a1, a2 = np.abs(al), np.abs(1 - al)
    e_v = eps * (a1 * (4 * np.abs(bs) + (Lr + 5) * axt_abs) + 3 * a2 * np.abs(s0))
    e_w = eps * (a1 * (5 * np.abs(bs) + (Lr + 6) * axt_abs) + 4 * a2 * np.abs(s0) + 3 * np.abs(y0) / rho)
    B_s = np.where(soc, np.sqrt(np.add.reduceat(e_w * e_w, first)) + (dims + 5) * eps * np.sqrt(np.add.reduceat(w * w, first)), 0)
    B_y = rho * (B_s[cone_of_row] + e_v) + eps * (3 * rho * (np.abs(s_ref) + np.abs(v)) + np.abs(y0))
    B_u = rho * (eps * np.abs(bs) + B_s[cone_of_row]) + B_y + eps * (3 * rho * (np.abs(bs) + np.abs(s_ref)) + np.abs(y_ref))
    B_x = 3 * eps * (a1 * np.abs(xt1) + a2 * np.abs(x0))
    return dict(v=v, w=w, s=s_ref, y=y_ref, u=u_ref, x=x_ref, rhs=rhs_ref, rhs_scale=rhs_scale, branch=branch, first=first, dims=dims,
                B_s=B_s, B_y=B_y, B_u=B_u, B_x=B_x)


def _worst(err, bound):
    live = bound > 0
    return (float((err[live] / bound[live]).max()) if live.any() else 0.0), bool(np.all(err[~live] == 0))


def rhs_figure(view, model, cap):
    """e = |r1 + K xt1 - rhs_ref|_inf / (|K|_inf |xt1|_inf + |rhs scale|_inf): the right-hand side k_spmv<MODE_RHS> formed, as
    the residual and the iterate it led to show it."""
    xt1 = view.cut(cap["xt1"])
    lhs = view.cut(cap["r1"]).astype(LD) + ld_matvec(view.K, xt1)
    den = norm_inf_matrix(view.K) * float(np.abs(xt1).max()) + float(model["rhs_scale"].max())
    return float(np.abs(lhs - model["rhs"]).max()) / den if den > 0 else 0.0


def rhs_bound(view, e_twin):
    """8 max(e_twin, (L + 4) eps), L = the longest row of K plus the longest column of As plus the two other terms: the
    margin and the floor of I2 (i2_bound), for the same reason."""
    A = sp.csc_matrix(view.qp.A)
    L = int(np.diff(view.K.indptr).max()) + (int(np.diff(A.indptr).max()) if A.nnz else 0) + 2
    return 8.0 * max(e_twin, (L + 4) * EPS)


def iteration_figures(view, model, cap):
    """The ratios of what one iteration left (x1, s1, y1, u1) to the bounds of iteration_model: dict of (worst ratio, zero-bound
    entries exact) for x, y, u row by row and s cone by cone (2-norm), and the figure of the right-hand-side identity."""
    x1, y1, s1, u1 = (view.cut(cap["x1"]).astype(LD), view.cut_rows(cap["y1"]).astype(LD), view.cut_rows(cap["s1"]).astype(LD),
                      view.cut_rows(cap["u1"]).astype(LD))
    ds = s1 - model["s"]
    return dict(x=_worst(np.abs(x1 - model["x"]), model["B_x"]), s=_worst(np.sqrt(np.add.reduceat(ds * ds, model["first"])), model["B_s"]),
                y=_worst(np.abs(y1 - model["y"]), model["B_y"]), u=_worst(np.abs(u1 - model["u"]), model["B_u"]),
                rhs=rhs_figure(view, model, cap))


def iteration_ok(f):
    return all(f[k][0] <= 1.0 and f[k][1] for k in ("x", "s", "y", "u"))


def general_conic_program(dims, seed=0):
    """minimise 1/2 |x - c|^2 over a product of second-order cones (P = I, A = -I, b = 0, no chains): a program whose cones are
    not SCORE's.  Of the cones with more than one row, c lies outside the first (projected onto its boundary), inside the second
    and in the polar cone of the third, and so on in turn.  Returns (None, model-like with .qp)."""
    import types

    from score_amd.assemble import ConicQP

    rng = np.random.default_rng(seed + int(sum(dims)))
    n = int(sum(dims))
    c = rng.normal(size=n)
    off, kind = 0, 0
    for dm in dims:
        blk = c[off : off + dm]
        if dm > 1:
            nt = np.linalg.norm(blk[1:])
            blk[0] = (0.3 * nt, 2.0 * nt + 0.1, -2.0 * nt - 0.1)[kind % 3]
            kind += 1
        off += dm
    qp = ConicQP(P=sp.identity(n, format="csr"), q=-c, c0=0.5 * float(c @ c), A=(-sp.identity(n, format="csr")), b=np.zeros(n), z=0,
                 soc_dims=np.asarray(dims, dtype=np.int32))
    return None, types.SimpleNamespace(qp=qp)


GENERAL_DIMS = {"Q": (3, 130, 1, 70),      # k_cone's register path (3 rows outside, 1 row); k_cone_wave inside (130) and polar (70)
                "Q32": (20, 1, 7, 32),     # k_cone's general path: 5 to 32 rows, one lane per cone, in all three branches
                "QW": (130, 70, 1, 100)}   # k_cone_wave (more than 32 rows, lanes striding by 64) outside, inside and polar


def iteration_models(case):
    """The (graph, model) list of a case of the iteration tests: a case of CASE_GRAPHS or a general conic program."""
    return [general_conic_program(GENERAL_DIMS[case])] if case in GENERAL_DIMS else case_models(case)


def iteration_at_start(models, settings, lib_path):
    """reset(), steps(3), then one captured iteration at rho = settings.rho.  Returns (views, capture)."""
    sol = ConicSolver([m.qp for _, m in models], dict(ADMM_SETTINGS, **settings), lib_path=lib_path)
    try:
        views = problem_views(sol, models)
        sol.reset()
        sol.steps(3)
        cap = iteration_capture(sol)
    finally:
        sol.close()
    return views, cap


def replay_and_single_steps(models, settings, lib_path):
    """Part 5: two handles from the same models -- reset(), steps(16) (one replay, 15 deferred updates) against use_graph = 0,
    reset() and steps(1) sixteen times (nothing deferred).  Returns (vectors of the first, of the second, graph launches of
    each)."""
    st = dict(ADMM_SETTINGS, check_interval=BLOCK, **settings)
    vecs = ("x", "y", "s", "xt", "kx")
    out = []
    for use_graph, blocks in ((1, (BLOCK,)), (0, (1,) * BLOCK)):
        sol = ConicSolver([m.qp for _, m in models], dict(st, use_graph=use_graph), lib_path=lib_path)
        try:
            sol.reset()
            for k in blocks:
                sol.steps(k)
            out.append(({v: sol.debug_get(v) for v in vecs}, int(sol.debug_get("graph_launches")[0])))
        finally:
            sol.close()
    return out[0][0], out[1][0], (out[0][1], out[1][1])


# ---------------------------------------------------------------------------------------------------------------------
# the checks the GPU tests and the twin's tests share
# ---------------------------------------------------------------------------------------------------------------------
def identity_checks(view, vec, cg_iters, float_factors, label, yard=None, link_caps=False):
    """I1-I3 of one problem and one snapshot as {name: passed} and the OPID line; `yard`: (view, vectors) of the twin's run of
    the same sequence, the yardstick of I2 (None: the floor of the bound alone, what the twin itself is held to); `link_caps`:
    I3 under link_cap_bound, with the twin's figure of `yard` beside the model's."""
    f = admm_figures(view, vec, cg_iters, float_factors)
    e_yard = 0.0 if yard is None else i2_figure(yard[0].K, yard[0].cut(yard[1]["xt"]), yard[0].cut(yard[1]["kx"]))
    b2 = i2_bound(view.K, e_yard)
    b3 = f["i3_bound"]
    if link_caps and yard is not None:
        b3 = link_cap_bound(f["i3_model"], eta_figure(yard[0].T, yard[0].on, yard[0].cut(yard[1]["z"]), yard[0].cut(yard[1]["r"])), float_factors)
    line = (f"OPID {label} n={view.qp.n} rho={view.rho:.6g} | I1 {f['i1']:.4f} | I2 {f['i2']:.3e} bound {b2:.3e} | "
            f"I3 {f['i3']:.3e} bound {b3:.3e}")
    return {"link pairs": f["pairs_ok"], "I1": f["i1"] <= 1.0 and f["i1_exact"], "I2": f["i2"] <= b2,
            "I3": f["i3"] <= b3, "I3 Jacobi": f["jacobi"]}, line


def penalty_update_checks(run, float_factors, label, yard=None, expect_launches=None, link_caps=False):
    """Every assertion of part 2 on the result of penalty_update_run, as (failures, OPID lines); `yard`: the twin's run
    (I2's yardstick in steps b and c; with `link_caps` the second yardstick of I3 as well: identity_checks)."""
    st, views, rho = run["settings"], run["views"], run["rho"]
    cg, fails, lines = st["cg_iters"], [], []

    def note(lab, checks):
        fails.extend((lab, nm) for nm, ok in checks.items() if not ok)

    a = run["a"]
    note(label, {"three updates": all(i["rho_updates"] == 3 for i in run["infos"]),
                 "rho read back == info": all(float(rho[k]) == i["rho"] for k, i in enumerate(run["infos"])),
                 "penalties differ": len(set(float(r) for r in rho)) == len(rho),
                 "rho after reset": bool(np.all(run["rho_reset"] == st["rho"])),
                 "graph launches": expect_launches is None or run["graph_launches"] == expect_launches})
    for k, v in enumerate(views):
        lab = f"{label}[{k}]"
        kv = kval_figures(v, rho[k], a["Kptr"], a["Kcol"], a["Kval"], run["rep"])
        uf = u_refresh_figures(v, rho[k], a["u"], a["y"], a["s"])
        kf = fresh_product_figures(v.K, v.cut(a["xt"]), v.cut(a["kx"]))
        lines.append(f"OPID {lab} update rho={float(rho[k]):.6g} | Kval {kv['ratio']:.4f} of 3 eps (|K0| + rho |K1|) (terms <= {kv['terms']}: "
                     f"{kv['ratio_ops']:.4f} of the operation count) | u {uf[0]:.4f} | kx {kf[0]:.4f}")
        note(lab + " a", {"Kval": kv["ratio"] <= 1.0 and kv["exact"], "Kval pattern": kv["complete"], "u": uf[0] <= 1.0 and uf[1],
                          "kx": kf[0] <= 1.0 and kf[1]})
        yb = None if yard is None else (yard["views"][k], yard["b"])
        checks, line = identity_checks(v, run["b"], cg, float_factors, lab + " b", yb, link_caps)
        lines.append(line)
        note(lab + " b", checks)
        for s, vec in enumerate(run["c"]):
            yc = None if yard is None else (yard["views_reset"][k], yard["c"][s])
            checks, line = identity_checks(run["views_reset"][k], vec, cg, float_factors, f"{lab} c{s + 1}", yc, link_caps)
            lines.append(line)
            note(f"{lab} c{s + 1}", checks)
    return fails, lines


def iteration_checks(views, cap, label, yard=None, alpha=ALPHA):
    """The figures of one captured iteration for every problem of a handle, as (failures, OPID lines, models); `yard`:
    (views, capture) of the twin's run, the yardstick of the right-hand-side identity (None: its floor alone)."""
    fails, lines, models = [], [], []
    for k, v in enumerate(views):
        m = iteration_model(v, cap, alpha)
        f = iteration_figures(v, m, cap)
        e_yard = 0.0 if yard is None else rhs_figure(yard[0][k], iteration_model(yard[0][k], yard[1], alpha), yard[1])
        b = rhs_bound(v, e_yard)
        lines.append(f"OPID {label}[{k}] iteration rho={v.rho:.6g} cones in/polar/out {[int((m['branch'] == c).sum()) for c in (1, 2, 3)]} | "
                     f"x {f['x'][0]:.4f} | s {f['s'][0]:.4f} | y {f['y'][0]:.4f} | u {f['u'][0]:.4f} | rhs {f['rhs']:.3e} bound {b:.3e}")
        fails += [(f"{label}[{k}]", nm) for nm in ("x", "s", "y", "u") if not (f[nm][0] <= 1.0 and f[nm][1])]
        if not f["rhs"] <= b:
            fails.append((f"{label}[{k}]", "rhs"))
        models.append(m)
    return fails, lines, models


def iteration_after_updates(models, settings, lib_path):
    """The part 2 sequence up to its step b, then one captured iteration at the updated per-problem penalties.
    Returns (views, capture)."""
    run = penalty_update_run(models, settings, lib_path, iteration_after=True, through_reset=False)
    return run["views"], run["iteration"]


def changing_cg_run(models, settings, lib_path):
    """Part 3 on one handle: solve() with CG_SETTINGS (three blocks of 16 iterations, the PCG count re-chosen after each),
    then steps(16) under the last count and the vectors it leaves."""
    st = dict(CG_SETTINGS, **settings)
    sol = ConicSolver([m.qp for _, m in models], st, lib_path=lib_path)
    try:
        infos = [o.info for o in sol.solve()]
        after = [o.info for o in sol.steps(BLOCK)]
        out = dict(settings=st, infos=infos, after=after, views=problem_views(sol, models), snap={v: sol.debug_get(v) for v in ADMM_VECS},
                   graph_launches=int(sol.debug_get("graph_launches")[0]))
    finally:
        sol.close()
    return out


def changing_cg_checks(run, float_factors, label, yard=None, expect_launches=None):
    """The assertions of part 3, as (failures, OPID lines).  The count after a check is a function of the count before it
    and of the check's verdict (cg_rule: above the target, between, far below); the PCG iterations of the three blocks and
    of the block after them are reported (info.cg_iters), and of the 27 verdict sequences only `above` three times gives
    both figures -- so they show that the measured reduction exceeded the target at every check."""
    import itertools

    st, fails, lines = run["settings"], [], []
    verdicts = dict(above=1.0, between=0.5 * st["cg_target"], below=0.0)
    outcomes = {}
    for names in itertools.product(verdicts, repeat=3):
        seq = [st["cg_iters"]]
        for nm in names:
            seq.append(cg_rule(seq[-1], verdicts[nm], st))
        outcomes.setdefault((BLOCK * sum(seq[:3]), seq[3]), []).append((names, seq))
    (want_total, want_last), = [k for k, v in outcomes.items() if any(n == ("above",) * 3 for n, _ in v)]
    seq = outcomes[(want_total, want_last)][0][1]
    checks = {"sequence": seq == [2, 3, 4, 6] and want_total == BLOCK * (2 + 3 + 4),
              "verdicts pinned": len(outcomes[(want_total, want_last)]) == 1,
              "cg_iters of solve": all(i["cg_iters"] == want_total for i in run["infos"]),
              "cg_iters of the block after": all(i["cg_iters"] - want_total == BLOCK * want_last for i in run["after"]),
              "graph launches": expect_launches is None or run["graph_launches"] == expect_launches}
    fails += [(label, nm) for nm, ok in checks.items() if not ok]
    for k, v in enumerate(run["views"]):
        y = None if yard is None else (yard["views"][k], yard["snap"])
        c, line = identity_checks(v, run["snap"], want_last, float_factors, f"{label}[{k}] cg={seq}", y)
        lines.append(line)
        fails += [(f"{label}[{k}]", nm) for nm, ok in c.items() if not ok]
    return fails, lines
