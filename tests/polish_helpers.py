"""What the tests of the semismooth-Newton polish share: a np.longdouble model of the function the polish minimises, with a
forward-error bound beside every quantity, a float64 restatement of it, and the checkers that hold a set of arrays (the
device's read-outs, or the restatement's) to the model.

The model follows the head comment of score_polish_host.hpp, in the equilibrated variables (As = E A D, bs = E b, qs = D q,
Ps = D P D, built from the problem data and the handle's D and E alone).  Every cone k is a second-order cone whose head
variable h is private (one entry a < 0 of As in the head row, b_head = 0, P_hh > 0 on the diagonal only); with the heads
minimised out in closed form (they stay 0 in u)

    F(u)  = 1/2 u'Ps u + qs'u + sum_k 1/2 c_k max(0, |t_k| - theta_k)^2          t_k = bs_tail - As_tail u
    c_k   = P_hh / a^2              theta_k = |a| (-q_h / P_hh)                  rho_k = |t_k|,  tau = t / rho,  ex = rho - theta
    nu_k  = -c_k ex tau             on active cones (rho > theta, rho > 0), 0 otherwise
    B_k   = c_k [(1 - theta / rho)(I - tau tau') + tau tau']   on active cones, 0 otherwise
    g     = Ps u + qs + As_tail' nu                            on the non-head rows, 0 on the heads
    H     = Ps + As_tail' B As_tail + 1e-9 I                   on the non-head rows, unit rows on the heads
    stopping measure  max_i |g_i| / D_i

and what the finish derives from u: heads max(x*, rho / |a|) with x* = -q_h / P_hh, s_tail = t, s_head = |a| x_head,
y_tail = nu, y_head = |y_tail|_2.

THE BOUNDS.  Every quantity is carried as a pair (value, bound) of np.longdouble arrays (class VB) and every operation of
the kernels' arithmetic is counted where it happens, with eps = 2^-52 (twice the unit roundoff: the margin over first order,
as in operator_helpers.iteration_model); x^ is what the kernel holds, |x^ - x| <= e_x:

    z = x + y    e_z = (e_x + e_y)(1 + eps) + r(z)                      z = x y    e_z = (|x| e_y + |y| e_x + e_x e_y)(1 + eps) + r(z)
    z = x / y    e_z = (e_x + |z| e_y) / (|y| - e_y) (1 + eps) + r(z)   z = sqrt x e_z = max(sqrt(x + e_x) - z, z - sqrt(max(x - e_x, 0)))(1 + eps) + r(z)
    a sum of k terms t_j (+ a first value p) in ANY order -- serial, tiled, strided, a tree:
                 e   = (e_p + sum e_j) + ops eps (|p| + sum |t_j| + e_p + sum e_j),    ops = the adds on the longest path
    max(x, y), max(0, x), |x|: 1-Lipschitz, the bounds pass unchanged (the larger of the two for max)

r(z) is one rounding, eps |z| -- or 0 where the operands carry no error and z is a double: an IEEE operation on exact operands
whose exact result is representable returns it (the np.longdouble value has 64 bits; where it fits 53 it is what the double
operation returns).  A fused multiply-add rounds once where the count has two roundings: it stays under the count.  So the
bounds are absolute (1 - theta / rho cancels as rho -> theta and its bound does not), there is no free constant, and an
entry whose bound is 0 must be equal exactly: the heads of g, nu and B of the inactive cones, the entries of H that only
inactive cones touch where the P part is exact, and everything in a program whose data are powers of two.  The data:
As = fl(fl(E A) D) and Ps = fl(fl(P D_j) D_i) carry two roundings, bs = fl(E b), qs = fl(D q) and 1 / D one (none where
the scale is a power of two).

A cone is UNDECIDED when |rho - theta| <= e_rho + e_theta (with a positive bound) or rho <= e_rho: the kernel may take
either branch.  nu and F are continuous across the boundary and their bounds cover both branches; B is not, so the model
takes the branch it is told for those cones (`branch`: the act bits of the device) and its own otherwise.

The sums: t_k is b - a_1 u_1 - a_2 u_2 ... in the row's order (k adds for k entries); (Ps u)_i and (As'nu)_i are tiled
sums (L - 1 adds in some order); g adds qs and the two sums (2); F adds the n - heads row terms u_i (1/2 (Ps u)_i + qs_i) and
the cones' terms inside blocks of 256 (a tree of 8 levels) and then one partial per block on the host (device_sum_ops; the
block counts are read from the handle, polish_blocks), and g'delta likewise over the row blocks of H; an entry of H with k contributions is P + c_1 B_1 + ... in
turn (k adds) up to kLongContrib = 64 contributions and, above that, 256 strided lane sums (ceil(k / 256) - 1 adds), a tree
over the lanes (8) and the P part (1).  A contribution that is exactly 0 (an inactive cone) adds nothing."""
# (operator_helpers.scaled_data and reference_K_parts return the np.longdouble values of As and of K alone; here every entry
#  needs its bound beside it, so scaled_of_view restates the scaling in VB arithmetic -- the same products, E A D and D P D,
#  with their roundings counted.  _sum_by_key, _lookup, cone_layout, ld_matvec and the figures of the refresh and the fresh
#  product are used as they are.)
import numpy as np
import scipy.sparse as sp

import operator_helpers as oh
from operator_helpers import EPS, LD

REG = 1e-9          # kPolishDiagReg
LONG_CONTRIB = 64   # kLongContrib
LANES = 256         # kThreads: the lanes of a long entry's workgroup
_E = LD(EPS)


# ---------------------------------------------------------------------------------------------------------------------
# values with bounds
# ---------------------------------------------------------------------------------------------------------------------
def _is_double(v):
    return v.astype(np.float64).astype(LD) == v


class VB:
    """np.longdouble values with forward-error bounds; the rules of the module's docstring."""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.zeros(self.v.shape, dtype=LD) if e is None else np.broadcast_to(np.asarray(e, dtype=LD), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, VB) else VB(np.asarray(x, dtype=LD))

    def _rounded(self, v, e_in):
        exact = (e_in == 0) & _is_double(v)
        return VB(v, e_in * (1 + _E) + np.where(exact, 0, _E * np.abs(v)))

    def __getitem__(self, k):
        return VB(self.v[k], self.e[k])

    def __neg__(self):
        return VB(-self.v, self.e)

    def __add__(self, o):
        o = VB.of(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = VB.of(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return VB.of(o) - self

    def __mul__(self, o):
        o = VB.of(o)
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = VB.of(o)
        ok = np.abs(o.v) > o.e
        den = np.where(ok, np.abs(o.v) - o.e, 1)
        v = self.v / np.where(o.v != 0, o.v, 1)
        return self._rounded(v, np.where(ok, (self.e + np.abs(v) * o.e) / den, np.inf))

    def __rtruediv__(self, o):
        return VB.of(o) / self

    def sqrt(self):
        v = np.sqrt(np.maximum(self.v, 0))
        lo, hi = np.sqrt(np.maximum(self.v - self.e, 0)), np.sqrt(np.maximum(self.v + self.e, 0))
        return self._rounded(v, np.maximum(hi - v, v - lo))

    def abs(self):
        return VB(np.abs(self.v), self.e)

    def where(self, mask, other=0):
        o = VB.of(other)
        return VB(np.where(mask, self.v, o.v), np.where(mask, self.e, o.e))

    def live(self):
        """Terms that are not exactly 0: the ones whose addition can round."""
        return (self.v != 0) | (self.e != 0)


def vb_max(a, b):
    a, b = VB.of(a), VB.of(b)
    return VB(np.maximum(a.v, b.v), np.maximum(a.e, b.e))


def vb_sum(terms, first, ops, start=None):
    """Sums of the groups of `terms` that begin at `first` (np.add.reduceat), added to `start` (one value per group): any
    order, `ops` adds on the longest path.  Returns (VB, sum of |terms| + |start|)."""
    n = first.size
    if terms.v.size:
        sv, sa, se = (np.add.reduceat(x, first) for x in (terms.v, np.abs(terms.v), terms.e))
        empty = np.r_[first[1:], terms.v.size] == first
        sv, sa, se = (np.where(empty, 0, x) for x in (sv, sa, se))
    else:
        sv = sa = se = np.zeros(n, dtype=LD)
    if start is not None:
        sv, sa, se = sv + start.v, sa + np.abs(start.v), se + start.e
    return VB(sv, se + np.asarray(ops, dtype=LD) * _E * (sa + se)), sa


def _count_live(mask, first):
    if not mask.size:
        return np.zeros(first.size, dtype=np.int64)
    c = np.add.reduceat(mask.astype(np.int64), first)
    return np.where(np.r_[first[1:], mask.size] == first, 0, c)


# ---------------------------------------------------------------------------------------------------------------------
# the problem in the equilibrated variables
# ---------------------------------------------------------------------------------------------------------------------
class Scaled:
    """As, bs, qs, Ps of one problem with their bounds, and its cones."""

    def __init__(self, n, m, A, As, bs, qs, Prow, Pcol, Ps, D, first, T):
        self.n, self.m, self.A, self.As, self.bs, self.qs, self.D, self.first, self.T = n, m, A, As, bs, qs, D, first, T
        order = np.lexsort((Pcol, Prow))
        self.Prow, self.Pcol, self.Ps = Prow[order], Pcol[order], Ps[order]
        self.P = sp.csr_matrix((np.ones(order.size), (self.Prow, self.Pcol)), shape=(n, n))
        self.P.sort_indices()
        ptr = A.indptr
        assert np.all(np.diff(ptr)[first] == 1), "a head row holds the head column alone"
        self.head_col = A.indices[ptr[first]].astype(np.int64)
        self.is_head = np.zeros(n, dtype=bool)
        self.is_head[self.head_col] = True
        self.a = As[ptr[first]]
        diag = self.Prow == self.Pcol
        pos = -np.ones(n, dtype=np.int64)
        pos[self.Prow[diag]] = np.nonzero(diag)[0]
        assert np.all(pos[self.head_col] >= 0) and np.all(self.a.v < 0)
        self.phh = self.Ps[pos[self.head_col]]
        self.tail_rows = (first[:, None] + 1 + np.arange(T)[None, :]).ravel()


def scaled_of_view(view):
    """From the problem data and the handle's D and E: two roundings on the entries of As and Ps, one on bs and qs."""
    qp = view.qp
    assert int(qp.z) == 0 and len(qp.soc_dims) and np.all(np.asarray(qp.soc_dims) == qp.soc_dims[0])
    A = sp.csr_matrix(qp.A, copy=True)
    A.sum_duplicates(); A.sort_indices()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    D, E = VB(view.D), VB(view.E)
    As = (E[rows] * VB(A.data)) * D[A.indices]
    P = sp.coo_matrix(qp.P)
    P.sum_duplicates()
    Ps = (VB(P.data) * D[P.col]) * D[P.row]
    first, dims, _ = oh.cone_layout(qp)
    return Scaled(qp.n, qp.m, A, As, E * VB(qp.b), D * VB(qp.q), P.row.astype(np.int64), P.col.astype(np.int64), Ps, np.asarray(view.D, dtype=np.float64),
                  first, int(dims[0]) - 1)


HANDLE_ARRAYS = ("Aval", "Aptr", "Acol", "G2val", "G2ptr", "G2col", "G2split", "qs", "bs", "D")


def scaled_of_handle(arr, n, m, x0, r0, first, T, D):
    """From the handle's own scaled arrays (Aval / Aptr / Acol, G2val / G2ptr / G2col / G2split, qs, bs: the setup tests pin
    them), cut to the problem whose columns start at x0 and rows at r0: the data carry no error.  For a program the handle
    transforms before it scales (the head form of a QCQP model)."""
    ap = arr["Aptr"].astype(np.int64)[r0 : r0 + m + 1]
    A = sp.csr_matrix((arr["Aval"][ap[0] : ap[-1]], arr["Acol"].astype(np.int64)[ap[0] : ap[-1]] - x0, ap - ap[0]), shape=(m, n))
    gp, split = arr["G2ptr"].astype(np.int64)[x0 : x0 + n + 1], arr["G2split"].astype(np.int64)[x0 : x0 + n]
    take = np.concatenate([np.arange(gp[i], split[i]) for i in range(n)]) if n else np.zeros(0, dtype=np.int64)
    Prow = np.repeat(np.arange(n), split - gp[:-1])
    Pcol = arr["G2col"].astype(np.int64)[take] - x0
    return Scaled(n, m, A, VB(A.data), VB(arr["bs"][r0 : r0 + m]), VB(arr["qs"][x0 : x0 + n]), Prow, Pcol, VB(arr["G2val"][take]),
                  np.asarray(D, dtype=np.float64), np.asarray(first, dtype=np.int64), T)


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
INACTIVE, ACTIVE = 0, 1


def _tail_entries(S):
    """Padded entry positions of the tail rows: (cones, T, Lmax) positions into As and their validity."""
    ptr = S.A.indptr
    rows = S.tail_rows.reshape(-1, S.T)
    lens = ptr[rows + 1] - ptr[rows]
    Lmax = int(lens.max()) if lens.size else 0
    pos = ptr[rows][:, :, None] + np.arange(Lmax)[None, None, :]
    ok = np.arange(Lmax)[None, None, :] < lens[:, :, None]
    return np.where(ok, pos, 0), ok


def polish_model(view, u, branch=None, scaled=None, f_ops=None):
    """The model at the point u (the problem's slice of the equilibrated iterate, heads 0), every quantity a VB.  `branch`:
    per cone, the activity the model takes where the cone is undecided (None: its own).  Returns a dict:

      F, gn (the stopping measure), g (n), nu (m; 0 on the head rows), B (cones, T, T), cls (cones: INACTIVE / ACTIVE),
      undecided (cones), t (cones, T), rho, theta, ck, keys / H / H_terms / H_live / H_ops (the entries of H on the model's
      pattern, key = row * n + column, with the number of contributions of each, of those that are not exactly 0, and the adds
      counted for it), Hmat (float64 CSR of H),
      xhead, s (m), y (m): what the finish derives from u, and `S`, the scaled problem.

    `f_ops`: the adds on the longest path of the sum that forms F (device_sum_ops for the kernels, numpy_sum_ops for the
    restatement; None: terms_ops, which covers both).  The derivations are the module's docstring; nothing here but the
    formulas in VB arithmetic."""
    S = scaled_of_view(view) if scaled is None else scaled
    n, m, T, nc = S.n, S.m, S.T, S.first.size
    uv = VB(np.asarray(u, dtype=np.float64))
    assert np.all(uv.v[S.is_head] == 0), "the heads stay 0 in u"
    A, As = S.A, S.As
    rowptr = A.indptr
    nnz_row = np.repeat(np.arange(m), np.diff(rowptr))
    # ---- cones: c, theta, x*, t, rho ----
    a_abs = -S.a
    ck = S.phh / (S.a * S.a)
    xstar = (-S.qs[S.head_col]) / S.phh
    theta = a_abs * xstar
    prod = As * uv[A.indices]
    full = np.nonzero(np.diff(rowptr) > 0)[0]
    tsum = VB(np.zeros(m, dtype=LD))
    part, _ = vb_sum(-prod, rowptr[:-1][full], _count_live(prod.live(), rowptr[:-1][full]), start=S.bs[full])
    tsum.v[full], tsum.e[full] = part.v, part.e
    empty = np.diff(rowptr) == 0
    tsum.v[empty], tsum.e[empty] = S.bs.v[empty], S.bs.e[empty]
    t = tsum[S.tail_rows.reshape(nc, T)]
    rho2 = t[:, 0] * t[:, 0]
    for c in range(1, T):
        rho2 = rho2 + t[:, c] * t[:, c]
    rho = rho2.sqrt()
    gap = rho - theta
    slack = rho.e + theta.e
    undecided = ((np.abs(rho.v - theta.v) <= slack) & (slack > 0)) | ((rho.v <= rho.e) & (rho.e > 0) & (rho.v > theta.v))
    own = (rho.v > theta.v) & (rho.v > 0)
    on = own if branch is None else np.where(undecided, np.asarray(branch).astype(bool), own)
    decided_off = ~undecided & ~own
    ex = VB(np.maximum(gap.v, 0), np.where(decided_off, 0, gap.e))
    phi = ((ck * 0.5) * ex) * ex
    # ---- multipliers and blocks ----
    ir = (1.0 / rho.where(on, 1.0)).where(on, 0.0)
    cex = (-ck) * ex
    nu = VB(np.zeros(m, dtype=LD))
    tau = []
    for c in range(T):
        val = ((cex * t[:, c]) * ir).where(on, 0.0)
        nu.v[S.first + 1 + c], nu.e[S.first + 1 + c] = val.v, val.e
        tau.append(t[:, c] * ir)
    w1 = (ck * (1.0 - theta * ir)).where(on, 0.0)
    w2 = ((ck * theta) * ir).where(on, 0.0)
    B = VB(np.zeros((nc, T, T), dtype=LD))
    for c in range(T):
        for d in range(T):
            val = (w2 * tau[c]) * tau[d]
            if c == d:
                val = w1 + val
            val = val.where(on, 0.0)
            B.v[:, c, d], B.e[:, c, d] = val.v, val.e
    # ---- gradient, F, stopping measure ----
    nonhead = ~S.is_head
    pu_terms = S.Ps * uv[S.Pcol]
    pfirst = S.P.indptr[:-1]
    prow_full = np.nonzero(np.diff(S.P.indptr) > 0)[0]
    pu = VB(np.zeros(n, dtype=LD))
    part, _ = vb_sum(pu_terms, pfirst[prow_full], np.maximum(_count_live(pu_terms.live(), pfirst[prow_full]) - 1, 0))
    pu.v[prow_full], pu.e[prow_full] = part.v, part.e
    order = np.argsort(A.indices, kind="stable")
    cols = A.indices[order]
    at_terms = (As * nu[nnz_row])[order]
    cfirst = np.nonzero(np.r_[True, cols[1:] != cols[:-1]])[0] if cols.size else np.zeros(0, dtype=np.int64)
    atnu = VB(np.zeros(n, dtype=LD))
    part, _ = vb_sum(at_terms, cfirst, np.maximum(_count_live(at_terms.live(), cfirst) - 1, 0))
    atnu.v[cols[cfirst]], atnu.e[cols[cfirst]] = part.v, part.e
    g = ((pu + S.qs) + atnu).where(nonhead, 0.0)
    rowterm = (uv * (pu * 0.5 + S.qs)).where(nonhead, 0.0)
    allterms = VB(np.r_[rowterm.v, phi.v], np.r_[rowterm.e, phi.e])
    Fsum, _ = vb_sum(allterms, np.zeros(1, dtype=np.int64), min(max(int(allterms.live().sum()) - 1, 0), terms_ops(allterms.v.size) if f_ops is None else int(f_ops)))
    measure = g.abs() * (1.0 / VB(S.D))
    worst = int(np.argmax(measure.v)) if n else 0
    gn = VB(measure.v[worst : worst + 1].max(initial=0), measure.e.max(initial=0))
    # ---- H entry by entry ----
    pos, ok = _tail_entries(S)
    Lmax = pos.shape[2]
    keys, tv, te = [], [], []
    for a_ in range(T):
        for b_ in range(T):
            for e_ in range(Lmax):
                for f_ in range(Lmax):
                    sel = ok[:, a_, e_] & ok[:, b_, f_]
                    if not sel.any():
                        continue
                    pe, pf = pos[sel, a_, e_], pos[sel, b_, f_]
                    term = (As[pe] * As[pf]) * B[sel, a_, b_]
                    keys.append(A.indices[pe].astype(np.int64) * n + A.indices[pf])
                    tv.append(term.v); te.append(term.e)
    keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
    tv = np.concatenate(tv) if tv else np.zeros(0, dtype=LD)
    te = np.concatenate(te) if te else np.zeros(0, dtype=LD)
    live = ((tv != 0) | (te != 0)).astype(LD)
    ck_, cv, ca, ce, cl, cnt = oh._sum_by_key(keys, tv, np.abs(tv), te, live)
    # the P part: Ps on the non-head rows, + 1e-9 on their diagonal (a diagonal P does not hold is 1e-9 alone); unit rows on the heads
    nh_ent = nonhead[S.Prow]
    pk = S.Prow[nh_ent] * n + S.Pcol[nh_ent]
    nhi = np.nonzero(nonhead)[0].astype(np.int64)
    dk = nhi * (n + 1)
    order_p = np.argsort(pk, kind="stable")
    pk_s, pv_s, pe_s = pk[order_p], S.Ps.v[nh_ent][order_p], S.Ps.e[nh_ent][order_p]
    hit = np.zeros(dk.size, dtype=bool)
    if pk_s.size:
        at = np.minimum(np.searchsorted(pk_s, dk), pk_s.size - 1)
        hit = pk_s[at] == dk
        dsum = VB(pv_s[at[hit]], pe_s[at[hit]]) + REG
        pv_s, pe_s = pv_s.copy(), pe_s.copy()
        pv_s[at[hit]], pe_s[at[hit]] = dsum.v, dsum.e
    extra = dk[~hit]
    hk = S.head_col.astype(np.int64) * (n + 1)
    all_keys = np.r_[pk_s, extra, hk]
    all_v = np.r_[pv_s, np.full(extra.size, LD(REG)), np.ones(hk.size, dtype=LD)]
    all_e = np.r_[pe_s, np.zeros(extra.size + hk.size, dtype=LD)]
    ukeys = np.union1d(all_keys, ck_)
    Pv, _ = oh._lookup(*_sorted(all_keys, all_v), ukeys)
    Pe, _ = oh._lookup(*_sorted(all_keys, all_e), ukeys)
    Cv, _ = oh._lookup(ck_, cv, ukeys)
    Ca, _ = oh._lookup(ck_, ca, ukeys)
    Ce, _ = oh._lookup(ck_, ce, ukeys)
    Cl, _ = oh._lookup(ck_, cl, ukeys)
    Cn, _ = oh._lookup(ck_, cnt.astype(np.int64), ukeys)
    long_ops = -(-Cn // LANES) - 1 + 8 + 1
    ops = np.where(Cn > LONG_CONTRIB, np.minimum(Cl.astype(np.int64), long_ops), Cl.astype(np.int64))
    H = VB(Pv + Cv, Pe + Ce + ops.astype(LD) * _E * (np.abs(Pv) + Ca + Pe + Ce))
    Hmat = sp.csr_matrix((H.v.astype(np.float64), (ukeys // n, ukeys % n)), shape=(n, n))
    # ---- what the finish derives from u ----
    xhead = vb_max(xstar, rho / a_abs)
    s = VB(np.zeros(m, dtype=LD))
    y = VB(np.zeros(m, dtype=LD))
    sh = a_abs * xhead
    s.v[S.first], s.e[S.first] = sh.v, sh.e
    tr = S.tail_rows
    s.v[tr], s.e[tr] = t.v.ravel(), t.e.ravel()
    y.v[tr], y.e[tr] = nu.v[tr], nu.e[tr]
    y2 = nu[S.first + 1] * nu[S.first + 1]
    for c in range(1, T):
        y2 = y2 + nu[S.first + 1 + c] * nu[S.first + 1 + c]
    yh = y2.sqrt()
    y.v[S.first], y.e[S.first] = yh.v, yh.e
    return dict(S=S, F=Fsum[0], gn=gn, g=g, nu=nu, B=B, cls=np.where(on, ACTIVE, INACTIVE), undecided=undecided, t=t, rho=rho, theta=theta, ck=ck,
                keys=ukeys, H=H, H_terms=Cn, H_live=Cl.astype(np.int64), H_ops=ops, Hmat=Hmat, xhead=xhead, s=s, y=y, phi=phi)


def _sorted(keys, vals):
    o = np.argsort(keys, kind="stable")
    return keys[o], vals[o]


# ---------------------------------------------------------------------------------------------------------------------
# a float64 restatement: what a correct double-precision implementation returns
# ---------------------------------------------------------------------------------------------------------------------
def polish_float64(view, u, scaled=None):
    """The same function in plain float64 NumPy from data scaled in float64 (fl(fl(E A) D), ...): F, gn, g, nu, B, act (bit 1:
    active), the entries of H on the model's pattern (keys, Hval) with the contributions of every entry (contrib: key -> list of
    values, for the planted errors), and the finish (xhead, s, y).  Every sum runs in NumPy's own order."""
    S = scaled_of_view(view) if scaled is None else scaled
    f8 = np.float64
    n, m, T, nc = S.n, S.m, S.T, S.first.size
    A = S.A
    if scaled is None:
        qp = view.qp
        A0 = sp.csr_matrix(qp.A, copy=True); A0.sum_duplicates(); A0.sort_indices()
        rows = np.repeat(np.arange(m), np.diff(A0.indptr))
        D, E = np.asarray(view.D, f8), np.asarray(view.E, f8)
        Av = (E[rows] * A0.data) * D[A0.indices]
        P = sp.coo_matrix(qp.P); P.sum_duplicates()
        order = np.lexsort((P.col, P.row))
        Pv = ((P.data * D[P.col]) * D[P.row])[order]
        bs, qs = E * np.asarray(qp.b, f8), D * np.asarray(qp.q, f8)
    else:
        Av, Pv, bs, qs = S.As.v.astype(f8), S.Ps.v.astype(f8), S.bs.v.astype(f8), S.qs.v.astype(f8)
    u = np.asarray(u, f8)
    ptr = A.indptr
    a = Av[ptr[S.first]]
    diag = np.nonzero(S.Prow == S.Pcol)[0]
    dpos = -np.ones(n, dtype=np.int64); dpos[S.Prow[diag]] = diag
    phh = Pv[dpos[S.head_col]]
    ck, xstar = phh / (a * a), -qs[S.head_col] / phh
    theta = -a * xstar
    tall = bs.copy()
    nnz_row = np.repeat(np.arange(m), np.diff(ptr))
    np.subtract.at(tall, nnz_row, Av * u[A.indices])
    t = tall[S.tail_rows.reshape(nc, T)]
    rho = np.sqrt((t * t).sum(axis=1))
    ex = np.where(rho > theta, rho - theta, 0.0)
    on = (ex > 0) & (rho > 0)
    ir = np.where(on, 1.0 / np.where(on, rho, 1.0), 0.0)
    nu = np.zeros(m)
    nu[S.tail_rows] = np.where(on[:, None], -ck[:, None] * ex[:, None] * t * ir[:, None], 0.0).ravel()
    w1, w2 = np.where(on, ck * (1.0 - theta * ir), 0.0), np.where(on, ck * theta * ir, 0.0)
    tau = t * ir[:, None]
    B = np.where(on[:, None, None], w1[:, None, None] * np.eye(T)[None] + w2[:, None, None] * tau[:, :, None] * tau[:, None, :], 0.0)
    pu = np.zeros(n); np.add.at(pu, S.Prow, Pv * u[S.Pcol])
    atnu = np.zeros(n); np.add.at(atnu, A.indices, Av * nu[nnz_row])
    nonhead = ~S.is_head
    g = np.where(nonhead, pu + qs + atnu, 0.0)
    phi = 0.5 * ck * ex * ex
    F = float(np.where(nonhead, u * (0.5 * pu + qs), 0.0).sum() + phi.sum())
    gn = float((np.abs(g) * (1.0 / S.D)).max())
    # H
    pos, ok = _tail_entries(S)
    keys, vals = [], []
    for a_ in range(T):
        for b_ in range(T):
            for e_ in range(pos.shape[2]):
                for f_ in range(pos.shape[2]):
                    sel = ok[:, a_, e_] & ok[:, b_, f_]
                    if sel.any():
                        pe, pf = pos[sel, a_, e_], pos[sel, b_, f_]
                        keys.append(A.indices[pe].astype(np.int64) * n + A.indices[pf]); vals.append((Av[pe] * Av[pf]) * B[sel, a_, b_])
    keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
    vals = np.concatenate(vals) if vals else np.zeros(0)
    nh = nonhead[S.Prow]
    pk, pv = S.Prow[nh] * n + S.Pcol[nh], Pv[nh].copy()
    dk = np.nonzero(nonhead)[0].astype(np.int64) * (n + 1)
    Hd = {}
    for k_, v_ in zip(pk.tolist(), pv.tolist()):
        Hd[k_] = v_
    for k_ in dk.tolist():
        Hd[k_] = Hd.get(k_, 0.0) + REG
    for h in S.head_col.tolist():
        Hd[h * (n + 1)] = 1.0
    order = np.argsort(keys, kind="stable")
    ks, vs = keys[order], vals[order]
    starts = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0] if ks.size else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], ks.size]
    contrib = {}
    for s0, s1 in zip(starts.tolist(), ends.tolist()):
        k_ = int(ks[s0])
        acc = Hd.get(k_, 0.0)
        for v_ in vs[s0:s1].tolist():
            acc += v_
        Hd[k_] = acc
        contrib[k_] = (s0, s1)
    hkeys = np.array(sorted(Hd), dtype=np.int64)
    Hval = np.array([Hd[k_] for k_ in hkeys.tolist()])
    xhead = np.maximum(xstar, rho / -a)
    s, y = np.zeros(m), np.zeros(m)
    s[S.first], s[S.tail_rows] = -a * xhead, t.ravel()
    y[S.tail_rows] = nu[S.tail_rows]
    y[S.first] = np.sqrt((nu[S.tail_rows].reshape(nc, T) ** 2).sum(axis=1))
    return dict(F=F, gn=gn, g=g, nu=nu, B=B, act=np.where(on, 2, 0), keys=hkeys, Hval=Hval, contrib=contrib, contrib_vals=vs, xhead=xhead, s=s, y=y,
                phi=phi, S=S)


# ---------------------------------------------------------------------------------------------------------------------
# the checkers
# ---------------------------------------------------------------------------------------------------------------------
def _ratio(got, ref):
    """(worst |got - ref.v| / ref.e over the entries with a positive bound, the others equal exactly)."""
    err = np.abs(np.asarray(got).astype(LD) - ref.v)
    live = ref.e > 0
    return (float((err[live] / ref.e[live]).max()) if live.any() else 0.0), bool(np.all(err[~live] == 0))


def evaluation_figures(mdl, got):
    """E: F, the stopping measure, g, nu and B of `got` (a dict of arrays of one problem) against the model, each as (worst
    ratio to the bound, zero-bound entries exact); `act`: bit 1 of the act words equals the model's class off the undecided
    cones; `heads`: the head entries of g are exactly 0."""
    S = mdl["S"]
    out = dict(F=_ratio(np.asarray([got["F"]]), VB(mdl["F"].v.reshape(1), mdl["F"].e.reshape(1))),
               gn=_ratio(np.asarray([got["gn"]]), VB(mdl["gn"].v.reshape(1), mdl["gn"].e.reshape(1))),
               g=_ratio(got["g"], mdl["g"]), nu=_ratio(got["nu"], mdl["nu"]),
               B=_ratio(np.asarray(got["B"]).reshape(mdl["B"].v.shape), mdl["B"]))
    bit = (np.asarray(got["act"]).astype(np.int64) >> 1) & 1
    dec = ~mdl["undecided"]
    out["act"] = bool(np.all(bit[dec] == mdl["cls"][dec]))
    out["heads"] = bool(np.all(np.asarray(got["g"])[S.is_head] == 0))
    return out


def evaluation_ok(f):
    return all(f[k][0] <= 1.0 and f[k][1] for k in ("F", "gn", "g", "nu", "B")) and f["act"] and f["heads"]


def hessian_figures(mdl, keys, vals, pon=None):
    """H: the stored entries (key = row * n + column, any order) against the model's: `ratio` (worst ratio, zero-bound entries
    exact) over the entries on the model's pattern, `superset`: every entry of the model is stored, `off`: the stored entries
    off the model's pattern are exactly 0, `long`: the same ratio over the entries with more than kLongContrib contributions
    alone and their number.  `pon` (the stored P part of every entry, where there is one to read): `p_part`: the entries all of
    whose contributions are exactly 0 -- only inactive cones touch them -- equal their P part bit for bit, and their number."""
    keys, vals = np.asarray(keys, dtype=np.int64), np.asarray(vals)
    order = np.argsort(keys, kind="stable")
    ks, vs = keys[order], vals[order]
    p_part = (True, 0)
    if pon is not None:
        live_terms, on_pattern = oh._lookup(mdl["keys"], mdl["H_live"], ks)
        quiet = on_pattern & (live_terms == 0)
        p_part = (bool(np.all(vs[quiet] == np.asarray(pon)[order][quiet])), int(quiet.sum()))
    got, hit = oh._lookup(ks, vs.astype(LD), mdl["keys"])
    ref = mdl["H"]
    err = np.abs(got - ref.v)
    live = ref.e > 0
    ratios = np.where(live, err / np.where(live, ref.e, 1), 0)
    exact = bool(np.all(err[~live] == 0))
    on_model = np.isin(ks, mdl["keys"])
    lg = mdl["H_terms"] > LONG_CONTRIB
    worst = int(np.argmax(ratios)) if ratios.size else 0
    return dict(ratio=(float(ratios.max()) if ratios.size else 0.0, exact), superset=bool(np.all(hit)), off=bool(np.all(vs[~on_model] == 0)),
                long=(float(ratios[lg].max()) if lg.any() else 0.0, int(lg.sum())), worst=int(mdl["keys"][worst]) if ratios.size else -1, p_part=p_part)


def hessian_ok(f):
    return f["ratio"][0] <= 1.0 and f["ratio"][1] and f["superset"] and f["off"] and f["p_part"][0]


def step_figures(S, u0, delta, step, u1):
    """S(b): u1 = u0 + step delta entrywise to one rounding -- the step is a power of two, so step delta is exact and the sum
    rounds once: |u1 - ref| <= eps / 2 |ref| (+ 2^-63 |ref|, the rounding of the np.longdouble reference itself); the heads
    stay exactly 0.  Returns (worst ratio, heads exact)."""
    ref = np.asarray(u0).astype(LD) + LD(step) * np.asarray(delta).astype(LD)
    nh = ~S.is_head
    err = np.abs(np.asarray(u1).astype(LD) - ref)[nh]
    bound = (_E / 2 + LD(2.0) ** -63) * np.abs(ref[nh])
    live = bound > 0
    ok0 = bool(np.all(err[~live] == 0))
    return (float((err[live] / bound[live]).max()) if live.any() else 0.0), ok0 and bool(np.all(np.asarray(u1)[S.is_head] == 0))


def finish_figures(mdl, x, s, y):
    """F: what the finish wrote (the problem's slices of x, s, y in the equilibrated variables) against the model at the
    returned u: heads, s, y entry by entry under the bounds; s and y in the cone up to the bound of the head entry."""
    S = mdl["S"]
    out = dict(heads=_ratio(np.asarray(x)[S.head_col], mdl["xhead"]), s=_ratio(s, mdl["s"]), y=_ratio(y, mdl["y"]))
    nc, T = S.first.size, S.T
    for nm, v in (("s", np.asarray(s)), ("y", np.asarray(y))):
        tail = np.sqrt((v[S.tail_rows].astype(LD).reshape(nc, T) ** 2).sum(axis=1))
        slack = mdl[nm].e[S.first] + np.sqrt((mdl[nm].e[S.tail_rows].reshape(nc, T) ** 2).sum(axis=1)) + (T + 1) * _E * tail
        out[nm + "_cone"] = bool(np.all(tail <= v[S.first].astype(LD) + slack))
    return out


def finish_ok(f):
    return all(f[k][0] <= 1.0 and f[k][1] for k in ("heads", "s", "y")) and f["s_cone"] and f["y_cone"]


def armijo_model(view, u0, delta, F0, gd, scaled=None, max_trials=40, f_ops=None):
    """S(c): the trial steps 1, 1/2, ... the model takes from u0 along delta with the rule of polish_lockstep,
    F(u0 + step delta) <= F0 + 1e-4 step gd, where F0 and gd are the model's own (VB).  Returns (trials taken, accepted step,
    separated, the model at the accepted point): `separated` is False when the bounds cannot tell a decision -- the margin F0 + 1e-4 step gd - F_trial lies
    within e_F0 + 1e-4 step e_gd + e_Ftrial -- which is a failure of the choice of point."""
    step, separated = 1.0, True
    S = scaled
    for k in range(max_trials):
        ut = np.asarray(u0, dtype=np.float64) + step * np.asarray(delta, dtype=np.float64)
        m = polish_model(view, ut, scaled=S, f_ops=f_ops)
        S = m["S"]
        margin = (F0.v + LD(1e-4) * LD(step) * gd.v) - m["F"].v
        slack = F0.e + LD(1e-4) * LD(step) * gd.e + m["F"].e + _E * (np.abs(F0.v) + np.abs(m["F"].v))
        if np.abs(margin) <= slack:
            separated = False
        if margin >= 0:
            return k + 1, step, separated, m
        step *= 0.5
    return max_trials, 0.0, separated, None


def directional_derivative(mdl, delta, ops=None):
    """g'delta of the model as a VB: n products summed in blocks and then block by block on the host; `ops`: the adds on the
    longest path (device_sum_ops with the row blocks of H; None: terms_ops)."""
    terms = mdl["g"] * VB(np.asarray(delta, dtype=np.float64))
    tot, _ = vb_sum(terms, np.zeros(1, dtype=np.int64), min(max(int(terms.live().sum()) - 1, 0), terms_ops(terms.v.size) if ops is None else int(ops)))
    return tot[0]


def device_sum_ops(*blocks):
    """Adds on the longest path of a sum the kernels leave as one partial per block and the host finishes: inside a block of
    256 lanes a wave reduction (6 levels) and (r0 + r1) + (r2 + r3) over the four waves (2), then the host adds the blocks'
    partials one after the other, those of every kind of block in turn (`blocks`: their numbers)."""
    return 8 + int(sum(blocks))


def numpy_sum_ops(n):
    """The same for np.sum over n float64 values (pairwise summation: halves down to runs of at most 128, eight accumulators
    over a run -- 16 adds each, 7 more for a ragged end --, three levels to join them, one level per halving)."""
    return min(max(n - 1, 0), 16 + 7 + 3 + max(0, int(np.ceil(np.log2(max(n, 1) / 128.0)))))


def terms_ops(n):
    """A count that covers both orders for n terms: blocks of 256 with one partial each (device_sum_ops with ceil(n / 256)
    blocks of each of two kinds) or NumPy's pairwise sum."""
    return max(device_sum_ops(2 * -(-n // 256)), numpy_sum_ops(n) + 1)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
NEWTON_SETTINGS = dict(rho=oh.RHO, sigma=oh.SIGMA, adaptive_rho=0, adaptive_cg=0, check_interval=5)  # (operator_helpers.ADMM_SETTINGS with the polish on)
STEPS = 15  # ADMM iterations before the point of a graph case: active and inactive cones both non-empty (asserted)
STEPS_3D = 5  # ... of a 3-D case (after 15 iterations the ranges of E40 and of the one-beacon graphs are all slack)


def case_steps(case):
    """ADMM iterations from reset() to the point of a case; the hand-made programs are evaluated at x = 0."""
    return 0 if case.startswith("PH") else (STEPS_3D if case in ("E40", "E60", "L64-3d", "L65-3d") else STEPS)


def case_settings(case, **extra):
    return dict(NEWTON_SETTINGS, **(dict(scale_iters=0) if case.startswith("PH") else {}), **extra)


def _long_entry_graph(n_poses, three_d):
    """One robot, one beacon, every pose ranged to it: the beacon's entries of H collect exactly n_poses contributions -- 64
    and 65 stand on either side of kLongContrib."""
    from score_amd.manhattan import make_manhattan, make_manhattan_3d

    return (make_manhattan_3d if three_d else make_manhattan)(n_robots=1, n_poses=n_poses, n_beacons=1, p_range=1.0)


def _prior_graph():
    """The prior2d graph of conftest.graph_by_name: two robots, three beacons, 2-D landmark priors on two of them."""
    from score_amd import compat
    from score_amd.manhattan import make_manhattan

    fg = make_manhattan(n_robots=2, n_poses=60, n_beacons=3, seed=15, p_range=0.4)
    lm = fg.landmark_variables
    fg.landmark_priors = [compat.LandmarkPrior2D(lm[0].name, (lm[0].true_position[0] + 0.3, lm[0].true_position[1] - 0.2), 4.0),
                          compat.LandmarkPrior2D(lm[2].name, (lm[2].true_position[0] - 0.1, lm[2].true_position[1] + 0.4), 0.25)]
    return fg


EXTRA_GRAPHS = {"L64": lambda: _long_entry_graph(64, False), "L65": lambda: _long_entry_graph(65, False),
                "L64-3d": lambda: _long_entry_graph(64, True), "L65-3d": lambda: _long_entry_graph(65, True), "prior2d": _prior_graph}
_extra = {}


def case_models(case):
    """The (graph, model) list of a case: a case of operator_helpers.CASE_GRAPHS, one of EXTRA_GRAPHS, or a hand-made
    private-head program PH<T> / PH<T>-nohint."""
    if case in EXTRA_GRAPHS:
        if case not in _extra:
            from score_amd.assemble import assemble

            fg = EXTRA_GRAPHS[case]()
            _extra[case] = (fg, assemble(fg, "SOCP"))
        return [_extra[case]]
    if case.startswith("PH"):
        return [private_head_program(int(case[2]), hint=not case.endswith("-nohint"))]
    return oh.case_models(case)


PH_CONES = 266  # 38 rounds of the seven kinds: the cones, and with them the pattern of H, cross a cone block of 256
PH_KINDS = ("inside", "boundary", "one ulp", "outside", "t=0 theta>0", "t=0 theta=0", "theta=0")


def private_head_program(T, hint=True):
    """A hand-made program of the private-head form, cones of T + 1 rows: non-head variables v_0 .. v_{cones T - 1} with a
    tridiagonal P (4 on the diagonal, -1 beside it: SPD) and q = 1/2; cone k has the tail rows b - A v with A = -1 on v_{kT + c}
    and 1/2 on the next variable, its head variable alone in the head row with a = -2, P_hh = 4 (so c_k = 1) and
    q_h = -2 theta_k (so theta_k comes out exactly).  Everything but the `one ulp` thresholds is a power of two or a small
    integer, and with scale_iters = 0 the scales are 1.  At x = 0, t = b_tail, and the cones cycle through PH_KINDS:

        inside        |t| = N, theta = 2 N                      inactive
        boundary      |t| = theta = N exactly                   nu = 0 and B = 0 exactly
        one ulp       theta = the double below N                active: 1 - theta / rho cancels
        outside       theta = N / 8                             active
        t=0 theta>0   t = 0, theta = 2                          inactive
        t=0 theta=0   t = 0, theta = 0                          inactive (rho = 0)
        theta=0       |t| = N, theta = 0                        B = c I

    with t = (5), (3, 4), (2, 3, 6) and N = 5, 5, 7.  `hint`: one chain of block size T over the non-head variables.
    Returns (None, model-like with .qp), as operator_helpers.general_conic_program does."""
    import types

    from score_amd.assemble import ConicQP

    nc, nv = PH_CONES, PH_CONES * T
    tvec = {1: (5.0,), 2: (3.0, 4.0), 3: (2.0, 3.0, 6.0)}[T]
    N = {1: 5.0, 2: 5.0, 3: 7.0}[T]
    n, m = nv + nc, nc * (T + 1)
    P = sp.diags([np.r_[np.full(nv, 4.0), np.full(nc, 4.0)], np.r_[np.full(nv - 1, -1.0), np.zeros(nc)], np.r_[np.full(nv - 1, -1.0), np.zeros(nc)]],
                 [0, 1, -1], shape=(n, n), format="csr")
    P.eliminate_zeros()
    q, b = np.r_[np.full(nv, 0.5), np.zeros(nc)], np.zeros(m)
    rows, cols, vals = [], [], []
    for k in range(nc):
        kind = PH_KINDS[k % len(PH_KINDS)]
        theta = dict([("inside", 2 * N), ("boundary", N), ("one ulp", float(np.nextafter(N, 0.0))), ("outside", N / 8), ("t=0 theta>0", 2.0),
                      ("t=0 theta=0", 0.0), ("theta=0", 0.0)])[kind]
        r0 = k * (T + 1)
        rows.append(r0); cols.append(nv + k); vals.append(-2.0)
        q[nv + k] = -2.0 * theta
        for c in range(T):
            j = k * T + c
            rows += [r0 + 1 + c]; cols += [j]; vals += [-1.0]
            if j + 1 < nv:
                rows += [r0 + 1 + c]; cols += [j + 1]; vals += [0.5]
            b[r0 + 1 + c] = 0.0 if kind.startswith("t=0") else tvec[c]
    A = sp.csr_matrix((vals, (rows, cols)), shape=(m, n))
    extra = dict(chain_ptr=np.array([0, nc], dtype=np.int32), node_cols=np.arange(nv, dtype=np.int32), block_size=T) if hint else {}
    qp = ConicQP(P=P, q=q, c0=0.0, A=A, b=b, z=0, soc_dims=np.full(nc, T + 1, dtype=np.int32), **extra)
    return None, types.SimpleNamespace(qp=qp)


def ph_expected(T):
    """Per cone of a PH program at x = 0: (kind, active)."""
    kinds = [PH_KINDS[k % len(PH_KINDS)] for k in range(PH_CONES)]
    return kinds, np.array([k in ("one ulp", "outside", "theta=0") for k in kinds])


def assert_ph_expected(S, cls, undecided, nu, B):
    """The table of private_head_program on the arrays of an evaluation at x = 0: the class of every cone, none undecided,
    nu = 0 and B = 0 exactly on every inactive cone (the boundary cones among them), B = c I = I where theta = 0."""
    kinds, active = ph_expected(S.T)
    assert not undecided.any()
    assert np.array_equal(np.asarray(cls).astype(bool), active)
    B = np.asarray(B).reshape(-1, S.T, S.T)
    nu_t = np.asarray(nu)[S.tail_rows].reshape(-1, S.T)
    assert np.all(B[~active] == 0) and np.all(nu_t[~active] == 0)
    for k, kind in enumerate(kinds):
        if kind == "theta=0":
            assert np.array_equal(B[k], np.eye(S.T)), (k, B[k])


# ---------------------------------------------------------------------------------------------------------------------
# a handle's read-outs, problem by problem
# ---------------------------------------------------------------------------------------------------------------------
def device_state(sol, views):
    """The read-outs of the last evaluation and the stored H (score_debug_get polish_eval / polish_u / polish_g / polish_nu /
    polish_B / polish_act / Hval and polish_Pon on Hptr, Hcol), cut to every problem of the handle: a list of dicts."""
    ev = sol.debug_get("polish_eval").reshape(-1, 3)
    u, g, nu, B, act = (sol.debug_get(k) for k in ("polish_u", "polish_g", "polish_nu", "polish_B", "polish_act"))
    Hptr, Hcol, Hval, Pon = sol.debug_get("Hptr").astype(np.int64), sol.debug_get("Hcol").astype(np.int64), sol.debug_get("Hval"), sol.debug_get("polish_Pon")
    blocks = sol.debug_get("polish_blocks")
    long_pos = blocks[3 * len(views) :].astype(np.int64)
    out, c0 = [], 0
    for k, v in enumerate(views):
        nc, T, n = len(v.qp.soc_dims), int(v.qp.soc_dims[0]) - 1, v.qp.n
        ptr = Hptr[v.x0 : v.x1 + 1]
        cols = Hcol[ptr[0] : ptr[-1]] - v.x0
        rows = np.repeat(np.arange(n), np.diff(ptr))
        out.append(dict(F=float(ev[k, 0]), gn=float(ev[k, 1]), flips=float(ev[k, 2]), u=v.cut(u).copy(), g=v.cut(g).copy(), nu=v.cut_rows(nu).copy(),
                        B=B[c0 * T * T : (c0 + nc) * T * T].copy(), act=act[c0 : c0 + nc].astype(np.int64), keys=rows * n + cols,
                        Hval=Hval[ptr[0] : ptr[-1]].copy(), Pon=Pon[ptr[0] : ptr[-1]].copy(), cols_in_range=bool(np.all((cols >= 0) & (cols < n))),
                        Hcsr=sp.csr_matrix((Hval[ptr[0] : ptr[-1]], cols, ptr - ptr[0]), shape=(n, n)),
                        f_ops=device_sum_ops(blocks[3 * k], blocks[3 * k + 1]), gd_ops=device_sum_ops(blocks[3 * k + 2]),
                        long_keys=np.sort((rows * n + cols)[long_pos[(long_pos >= ptr[0]) & (long_pos < ptr[-1])] - ptr[0]])))
        c0 += nc
    return out


class HandleView:
    """One problem of a single-problem handle seen through the handle's own scaled arrays, for a program the handle transforms
    before it scales (the head form of a QCQP model): what ProblemView offers the polish tests -- the cuts, the scaled problem
    `S` (scaled_of_handle), K = Ps + sigma I + rho As'As, and the chains (score_debug_get "chain_id_of_col")."""

    def __init__(self, sol, qp, rho=oh.RHO, sigma=oh.SIGMA):
        import types

        arr = {k: sol.debug_get(k) for k in HANDLE_ARRAYS}
        n, m = arr["qs"].size, arr["bs"].size
        first, dims, _ = oh.cone_layout(qp)
        assert m == qp.m and n < qp.n, "the head form keeps the rows and drops the range directions"
        self.S = scaled_of_handle(arr, n, m, 0, 0, first, int(dims[0]) - 1, arr["D"])
        self.x0, self.x1, self.r0, self.r1, self.rho, self.sigma = 0, n, 0, m, float(rho), float(sigma)
        self.qp = types.SimpleNamespace(n=n, m=m, soc_dims=qp.soc_dims, block_size=int(qp.block_size))
        S = self.S
        As = sp.csr_matrix((S.As.v.astype(np.float64), S.A.indices, S.A.indptr), shape=(m, n))
        Ps = sp.csr_matrix((S.Ps.v.astype(np.float64), (S.Prow, S.Pcol)), shape=(n, n))
        self.K = (Ps + sigma * sp.identity(n) + rho * (As.T @ As)).tocsr()
        self.K.sum_duplicates(); self.K.sort_indices()
        self.chain, self.node = oh.chain_nodes_of_ids(sol.debug_get("chain_id_of_col"), int(qp.block_size))
        self.pairs = self.expected_pairs = []
        assert sol.debug_get("link_pairs").size == 0

    def cut(self, v):
        return np.asarray(v)[self.x0 : self.x1]

    def cut_rows(self, v):
        return np.asarray(v)[self.r0 : self.r1]


def u_figures(S, rho, u, y, s):
    """operator_helpers.u_refresh_figures on a scaled problem: u = rho (bs - s) - y row by row, three roundings,
    |u - u_ref|_i <= 3 eps (rho (|bs| + |s|) + |y|)_i.  Returns (worst ratio, rows with a zero bound equal exactly)."""
    r, sl, yl = LD(rho), np.asarray(s).astype(LD), np.asarray(y).astype(LD)
    err = np.abs(np.asarray(u).astype(LD) - (r * (S.bs.v - sl) - yl))
    bound = 3 * _E * (r * (np.abs(S.bs.v) + np.abs(sl)) + np.abs(yl)) + r * S.bs.e
    live = bound > 0
    return (float((err[live] / bound[live]).max()) if live.any() else 0.0), bool(np.all(err[~live] == 0))


def with_chains(view):
    """A view made without a graph (a hand-made program) with the chains of the program's own hint, for the model
    preconditioner."""
    if int(view.qp.block_size):
        view.chain, view.node = oh.chain_nodes_of_problem(view.qp)
        view.T, view.on = oh.preconditioned_matrix(view.K, view.chain, view.node, int(view.qp.block_size), [])
    return view


def model_at(view, st, scaled=None):
    """The model at the point of a device state, the undecided cones on the branch the device took, F summed as the handle's
    blocks sum it."""
    return polish_model(view, st["u"], branch=(st["act"] >> 1) & 1, scaled=scaled, f_ops=st.get("f_ops"))


# ---------------------------------------------------------------------------------------------------------------------
# S(e): the step solves what it was asked to solve
# ---------------------------------------------------------------------------------------------------------------------
def model_preconditioner(view, H):
    """M of I4 on the matrix H: the chain part and the link blocks of H (operator_helpers.preconditioned_matrix) solved exactly
    on the chain columns (SuperLU), the reciprocal diagonal elsewhere.  Returns v -> M^-1 v."""
    import scipy.sparse.linalg as spla

    T, on = oh.preconditioned_matrix(H, view.chain, view.node, int(view.qp.block_size), view.expected_pairs)
    idx = np.nonzero(on)[0]
    lu = spla.splu(T[idx][:, idx].tocsc()) if idx.size else None
    d = H.diagonal()

    def apply(v):
        v = np.asarray(v, dtype=np.float64)
        z = v / d
        if lu is not None:
            z[idx] = lu.solve(v[idx])
        return z

    return apply


def pcg_reference(H, b, Minv, eta, cap=400):
    """PCG on H x = b from x = 0 with np.longdouble products and recurrences, stopped by the gate of pcg_gate: the first step
    sets the threshold eta^2 r0'z0, every later step is taken only while the r'z it is about to use exceeds it.  Returns
    (x, steps taken)."""
    b = np.asarray(b).astype(LD)
    x, r = np.zeros(b.size, dtype=LD), b.copy()
    z = Minv(r).astype(LD)
    p, rz = z.copy(), r @ z
    w = oh.ld_matvec(H, p)
    ref, used = LD(eta) * LD(eta) * rz, 0
    while used < cap:
        if not (rz > ref if used else rz > 0):
            break
        alpha = rz / (p @ w)
        x, r = x + alpha * p, r - alpha * w
        used += 1
        z = Minv(r).astype(LD)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        w = oh.ld_matvec(H, p)
        rz = rz_new
    return x, used


def step_quality(H, g0, delta, Minv):
    """phi = sqrt(rho'M^-1 rho / g0'M^-1 g0) with rho = -g0 - H delta in np.longdouble."""
    g0 = np.asarray(g0).astype(LD)
    res = -g0 - oh.ld_matvec(H, delta)
    return float(np.sqrt((res @ Minv(res).astype(LD)) / (g0 @ Minv(g0).astype(LD))))
