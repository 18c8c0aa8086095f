"""One family of 48 x 48 pencils (nb = 16) for the Rayleigh-Ritz step, stated once: the host routine
(score_amd/csrc/score_spectrum_rr.hpp, tests/test_spectrum_host.py) and the device kernel k_gsp_ritz
(score_amd/csrc/score_spectrum_batch.hpp, tests/test_spectrum_batch_gpu.py, tests/test_curvature_batch_gpu.py) are held to the
same pencils, the same expectations and the same bounds.  No test lives here.

Every pencil is built from NumPy alone, from the ingredients of the first tests of the step: ``default_rng(5)``, an SPD operator
``Aop`` on 400 rows, ``S1 = rng.normal(size=(400, 48))`` and the pencil ``(S' Aop S, S'S)`` of a basis S = [X | W | P].  Each
carries the branch of the kernel it is there for (``why``) and what the step must answer under both rules (``expect``:
indefinite -> (status, kept)).  ``family()`` asserts, before any library is called, that no expectation hangs on a coin toss:

  * every eigenvalue of the scaled Gram matrix of every attempt that runs is a factor 100 away from kSpRrDrop * largest;
  * the expected ``kept`` is the count of ``deflated``;
  * where the definite rule answers, the lowest value of the deflated pencil exceeds the bound on theta;
  * where negative values are expected, every value is further from zero than that bound and their count is as stated.

Reference and bounds (``reference``, ``judge``): ``scipy.linalg.eigh`` of the deflated pencil (T, G); for a result without P
(status RITZ_NO_P) the P block is zeroed first.  With As = D sym(A) D on the directions in use (D = diag(B)^-1/2: theta does
not change under column scaling, and the unscaled norm would make the bound vacuous for graded, tiny and huge columns):

    |theta - want|               <= 48 eps |As|_2 cond(G)
    |C'BC - I|                   <= 48 48 eps cond(G)
    |C' sym(A) C - diag(theta)|  <= 48 48 eps |As|_2 cond(G)

and theta_j is the Rayleigh quotient of the vector its column of C forms, to the rounding of that quotient alone (``judge``).
The third pins the span of C: with the values equal to the lowest ones, C'AC diagonal and C'BC = I, C spans the lowest
invariant subspace of the deflated pencil, which the values alone do not show.  The five pencils of the first tests
(``legacy``) also keep the bound they were written with, 48 eps |sym(A)|_2 cond(G) of the unscaled matrix."""
import functools
from dataclasses import dataclass, field

import numpy as np
import scipy.linalg as sla

from score_amd.spectrum_batch import BASIS, BLOCK, RITZ_BREAKDOWN, RITZ_NO_P, RITZ_OK

EPS = float(np.finfo(np.float64).eps)
M, NB, ROWS = BASIS, BLOCK, 400
DROP = 1e-10  # kSpRrDrop of score_spectrum_rr.hpp
MARGIN = 100.0  # no eigenvalue of a scaled Gram matrix within this factor of DROP * largest
RULES = (False, True)  # indefinite?


@dataclass
class Pencil:
    label: str
    A: np.ndarray
    B: np.ndarray
    why: str                     # the branch of the kernel (and of the host routine) the pencil is there for
    expect: dict                 # indefinite -> (status, kept)
    negatives: int = 0           # negative values of the deflated pencil the indefinite rule answers
    bits_of: dict = field(default_factory=dict)  # indefinite -> label of the status-OK pencil whose theta and coef it repeats
    exact_theta: np.ndarray = None               # where the values are exact
    legacy: bool = False         # one of the five pencils of the first tests: their bound holds as well


def sym(X):
    return 0.5 * (X + X.T)


def in_use(B, no_p=False):
    """The directions of step 1: a finite, positive Gram diagonal; without the P block where the step retried."""
    b = np.diag(B)[:2 * NB if no_p else M]
    with np.errstate(invalid="ignore"):
        return np.nonzero(np.isfinite(b) & (b > 0))[0]


def scaled_gram_values(B, no_p=False):
    use = in_use(B, no_p)
    if len(use) < NB:
        return None
    d = 1.0 / np.sqrt(np.diag(B)[use])
    return np.linalg.eigvalsh(sym(B)[np.ix_(use, use)] * np.outer(d, d))


def deflated(A, B, drop=DROP, no_p=False):
    """The pencil restricted as score_spectrum_rr.hpp does it: directions with a finite positive Gram diagonal (without the P
    block: those of X and W), scaled to a unit diagonal, the eigen-directions of the scaled Gram matrix above drop * largest.
    Returns (T, G, kept, use, As); fewer than nb directions in use: (None, None, 0, use, None)."""
    use = in_use(B, no_p)
    if len(use) < NB:
        return None, None, 0, use, None
    A, B = sym(A), sym(B)
    d = 1.0 / np.sqrt(np.diag(B)[use])
    As, Bs = A[np.ix_(use, use)] * np.outer(d, d), B[np.ix_(use, use)] * np.outer(d, d)
    lam, Q = np.linalg.eigh(Bs)
    keep = lam > drop * lam[-1]
    Y = Q[:, keep]
    return Y.T @ As @ Y, Y.T @ Bs @ Y, int(keep.sum()), use, As


def _deflated(A, B, drop):
    """``deflated`` in the form the first tests of the step call it."""
    return deflated(A, B, drop)[:3]


def without_p(X):
    Z = X.copy()
    Z[2 * NB:, :] = 0.0
    Z[:, 2 * NB:] = 0.0
    return Z


@functools.lru_cache(maxsize=None)
def _reference(label, no_p):
    p = by_label()[label]
    A, B = (without_p(p.A), without_p(p.B)) if no_p else (p.A, p.B)
    T, G, kept, use, As = deflated(A, B, DROP, no_p)
    cond, norm = float(np.linalg.cond(G)), float(np.linalg.norm(As, 2))
    ref = dict(T=T, G=G, kept=kept, use=use, cond=cond, norm=norm, want=sla.eigh(T, G, eigvals_only=True),
               theta_bound=48 * EPS * norm * cond, ortho_bound=48 * 48 * EPS * cond, ritz_bound=48 * 48 * EPS * norm * cond,
               A=sym(A), B=sym(B))
    ref["want"].setflags(write=False)
    return ref


def reference(p, status):
    """What a result of ``status`` (RITZ_OK or RITZ_NO_P) is judged against; computed once and left unchanged."""
    assert status in (RITZ_OK, RITZ_NO_P)
    return _reference(p.label, status == RITZ_NO_P)


def judge(p, indefinite, theta, coef, status, kept, breakdown_is_nan=False):
    """The assertions on one result, the same for the host routine and the device.  Returns the ratios to their bounds (theta,
    C'BC, C'AC, the Rayleigh quotient), or None for a breakdown."""
    tag = f"{p.label} ({'indefinite' if indefinite else 'definite'} rule)"
    want_status, want_kept = p.expect[indefinite]
    assert (int(status), int(kept)) == (want_status, want_kept), (tag, int(status), int(kept), "expected", want_status, want_kept)
    if status == RITZ_BREAKDOWN:
        if breakdown_is_nan:  # (the wrapper's NaN: the kernel writes neither)
            assert np.all(np.isnan(theta)) and np.all(np.isnan(coef)), tag
        return None
    assert theta.shape == (NB,) and coef.shape == (M, NB) and np.all(np.isfinite(theta)) and np.all(np.isfinite(coef)), tag
    ref = reference(p, status)
    want = ref["want"][:NB]
    r_theta = float(np.max(np.abs(theta - want)) / ref["theta_bound"])
    assert np.all(np.abs(theta - want) <= ref["theta_bound"]), (tag, theta - want, ref["theta_bound"])
    unused = np.setdiff1d(np.arange(M), ref["use"])
    assert not coef[unused].any(), (tag, "coefficients on directions not in use", unused)
    use = ref["use"]  # (the rows not in use are zero: the products run over the others, a bad Gram diagonal is not read)
    Cu, Au, Bu = coef[use], ref["A"][np.ix_(use, use)], ref["B"][np.ix_(use, use)]
    ortho = float(np.max(np.abs(Cu.T @ Bu @ Cu - np.eye(NB))))
    assert ortho <= ref["ortho_bound"], (tag, ortho, ref["ortho_bound"])
    ritz = float(np.max(np.abs(Cu.T @ Au @ Cu - np.diag(theta))))
    assert ritz <= ref["ritz_bound"], (tag, ritz, ref["ritz_bound"])
    # theta_j is the Rayleigh quotient of the vector the coefficients form, recomputed from the unscaled matrices (step 4), not
    # the value of the reduced problem: it is held to the rounding of that evaluation alone, whatever cond(G) is.  With u = eps / 2
    # and n directions in use: two nested dot products of length n give c'Ac and c'Bc to 2 (n + 1) u |c|'|A||c| each, the
    # symmetrisation, the division and the last scaling of c add 4 u: (2 n + 6) u <= (n + 6) eps.  Evaluated here in long double.
    Cl, Al, Bl = Cu.astype(np.longdouble), Au.astype(np.longdouble), Bu.astype(np.longdouble)
    cac, cbc = np.sum(Cl * (Al @ Cl), axis=0), np.sum(Cl * (Bl @ Cl), axis=0)
    room = (len(use) + 6) * EPS * (np.sum(np.abs(Cl) * (np.abs(Al) @ np.abs(Cl)), axis=0)
                                   + np.abs(theta) * np.sum(np.abs(Cl) * (np.abs(Bl) @ np.abs(Cl)), axis=0))
    r_quotient = float(np.max(np.abs(cac - theta * cbc) / room)) if np.all(room > 0) else 0.0
    assert np.all(np.abs(cac - theta * cbc) <= room), (tag, "theta is not the Rayleigh quotient of its vector", r_quotient)
    if p.legacy:  # the first tests' bound, of the unscaled matrix
        assert np.all(np.abs(theta - want) <= 48 * EPS * np.linalg.norm(Au, 2) * ref["cond"]), tag
    if p.exact_theta is not None:
        np.testing.assert_array_equal(theta, p.exact_theta, err_msg=tag)
    negative = int(np.sum(theta < 0.0))
    assert negative == (min(p.negatives, NB) if indefinite else 0), (tag, "negative values", negative)
    return r_theta, ortho / ref["ortho_bound"], ritz / ref["ritz_bound"], r_quotient


def same_bits_pairs(indefinite):
    """(label, label of the status-OK pencil whose theta and coef it must repeat bit for bit) under a rule."""
    return [(p.label, p.bits_of[indefinite]) for p in family() if indefinite in p.bits_of]


def positive_labels():
    """The pencils whose answer does not depend on the rule: the indefinite rule gives the definite rule's bits."""
    return [p.label for p in family() if p.expect[False] == p.expect[True] and p.negatives == 0]


def stacked(pencils):
    return np.array([p.A for p in pencils]), np.array([p.B for p in pencils])


def same_bits(a, b):
    """Two results (theta, coef, status, kept) of one pencil, bit for bit (a NaN the wrapper left equals itself, -0 is not 0)."""
    return (all(np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)) for x, y in zip(a[:2], b[:2]))
            and int(a[2]) == int(b[2]) and int(a[3]) == int(b[3]))


def judge_launch(run, indefinite, say=print):
    """``run(GA, GB) -> (theta, coef, status, kept)`` (one launch of k_gsp_ritz under a rule) on the whole family at once: every
    pencil under ``judge``, the bit-equalities of the retry.  Returns the per-pencil results in the family's order."""
    pencils = checked_family()
    labels = [p.label for p in pencils]
    theta, coef, status, kept = run(*stacked(pencils))
    per = [(theta[i], coef[i], int(status[i]), int(kept[i])) for i in range(len(pencils))]
    for p, r in zip(pencils, per):
        ratios = judge(p, indefinite, *r, breakdown_is_nan=True)
        say(f"{p.label:14s} {'indefinite' if indefinite else 'definite  '} status {r[2]} kept {r[3]:2d} ratios to the bounds "
            f"(theta, C'BC, C'AC, quotient): {ratios}")
    for label, twin in same_bits_pairs(indefinite):
        got, want = per[labels.index(label)], per[labels.index(twin)]
        assert got[2] == RITZ_NO_P and want[2] == RITZ_OK and got[3] == want[3], (label, twin)
        assert same_bits(got[:2] + (0, 0), want[:2] + (0, 0)), f"{label} does not repeat the bits of {twin}"
    return per


def judge_launch_shapes(run, per, tiled=600):
    """The bits of ``per`` (the family in one launch) do not depend on the launch: the family reversed, every pencil alone, and
    the family tiled to ``tiled`` pencils -- more workgroups than the chip holds at once, two resident per CU."""
    pencils = family()
    n = len(pencils)
    GA, GB = stacked(pencils)
    back = run(GA[::-1], GB[::-1])
    for i, p in enumerate(pencils):
        assert same_bits([x[n - 1 - i] for x in back], per[i]), f"{p.label}: the reversed launch gives other bits"
    for i, p in enumerate(pencils):
        alone = run(GA[i:i + 1], GB[i:i + 1])
        assert same_bits([x[0] for x in alone], per[i]), f"{p.label}: alone in a launch it gives other bits"
    order = np.arange(tiled) % n
    many = run(GA[order], GB[order])
    for j, i in enumerate(order):
        assert same_bits([x[j] for x in many], per[i]), f"{pencils[i].label}: copy {j} of {tiled} gives other bits"


def _check(p):
    """The conditions of the head of the file, from NumPy alone."""
    retried = any(p.expect[r][0] != RITZ_OK for r in RULES)
    for no_p in ((False, True) if retried else (False,)):
        lam = scaled_gram_values(p.B, no_p)
        if lam is None:
            continue
        edge = DROP * lam[-1]
        assert np.all((lam >= MARGIN * edge) | (lam <= edge / MARGIN)), (p.label, no_p, "a Gram value near the drop threshold", lam / edge)
    for indefinite in RULES:
        status, kept = p.expect[indefinite]
        no_p = status != RITZ_OK
        T, G, kept_ref, use, As = deflated(p.A, p.B, DROP, no_p)
        assert kept == kept_ref, (p.label, indefinite, kept, kept_ref)
        if status == RITZ_BREAKDOWN:
            continue
        ref = reference(p, status)
        w = ref["want"]
        assert np.all(np.abs(w) > ref["theta_bound"]), (p.label, indefinite, "a value within the bound of zero")
        if indefinite:
            assert int(np.sum(w < 0)) == p.negatives, (p.label, int(np.sum(w < 0)), p.negatives)
        else:
            assert w[0] > ref["theta_bound"], (p.label, w[0], ref["theta_bound"])
    if p.expect[False] != p.expect[True]:  # only the sign test separates the rules
        assert p.negatives > 0 and p.expect[True][0] == RITZ_OK, p.label


@functools.lru_cache(maxsize=None)
def family():
    """The pencils, in a fixed order; built and checked once."""
    rng = np.random.default_rng(5)
    Aop = rng.normal(size=(ROWS, ROWS))
    Aop = Aop @ Aop.T / ROWS + 0.1 * np.eye(ROWS)  # SPD operator
    S1 = rng.normal(size=(ROWS, M))
    S2 = S1.copy()
    S2[:, 40:] = S2[:, :8] + 1e-14 * rng.normal(size=(ROWS, 8))  # S'S of rank 40
    S3 = S1.copy()
    S3[:, 32:] = 0.0  # an empty P

    def of(S):
        return S.T @ Aop @ S, S.T @ S

    ok = lambda kept: {False: (RITZ_OK, kept), True: (RITZ_OK, kept)}
    broken = lambda kept: {False: (RITZ_BREAKDOWN, kept), True: (RITZ_BREAKDOWN, kept)}
    no_p = lambda kept: {False: (RITZ_NO_P, kept), True: (RITZ_NO_P, kept)}
    out = []

    def add(label, AB, why, expect, **kw):
        out.append(Pencil(label, np.ascontiguousarray(AB[0], dtype=np.float64), np.ascontiguousarray(AB[1], dtype=np.float64), why,
                          expect, **kw))

    # --- the five pencils of the first tests, with the values asserted there
    A1, B1 = of(S1)
    add("full", (A1, B1), "full rank: both decompositions of size 48", ok(48), legacy=True)
    add("dep8", of(S2), "S'S of rank 40: the second decomposition of size 40", ok(40), legacy=True)
    add("emptyP", of(S3), "an empty P (the first iteration): one decomposition size, 32; a prefix index map", ok(32), legacy=True)
    with_nan = A1.copy()
    with_nan[3, 7] = np.nan
    add("nanX", (with_nan, B1), "a NaN in the X block: both attempts fail in the second decomposition", broken(32), legacy=True)
    add("negated", (-A1, B1), "S'AS negated: the sign test alone separates the rules",
        {False: (RITZ_BREAKDOWN, 32), True: (RITZ_OK, 48)}, negatives=48, legacy=True)

    # --- sizes and parity
    for k in (1, 7, 15):
        S = S1.copy()
        S[:, M - k:] = S[:, :k] + 1e-14 * rng.normal(size=(ROWS, k))
        add(f"dep{k}", of(S), f"the last {k} columns repeat the first: ODD SECOND decomposition ({M - k})", ok(M - k))
    S = S1.copy()
    S[:, M - 3:] = S[:, :3] + 5e-4 * rng.normal(size=(ROWS, 3))
    add("soft3", of(S), "the last 3 columns repeat the first up to 5e-4: Gram values 1e-7 of the largest are KEPT (cond(G) of 1e7)", ok(48))
    X = S1[:, :NB]
    for label, kept in (("rank17", 17), ("rank16", 16), ("rank15", 15)):
        S = np.empty((ROWS, M))
        S[:, :NB] = X
        if kept == 15:
            S[:, 5] = S[:, 2] + 1e-14 * rng.normal(size=ROWS)  # one X column depends on another
        S[:, NB:] = S[:, :NB] @ rng.normal(size=(NB, 2 * NB)) + 1e-14 * rng.normal(size=(ROWS, 2 * NB))
        if kept == 17:
            S[:, NB] = S1[:, NB]  # one independent column of W
        why = {17: "W and P in the span of X but for one column: kept == nb + 1, odd second decomposition (17)",
               16: "W and P in the span of X: kept == nb exactly",
               15: "W and P in the span of X, and X of rank 15: kept == nb - 1 in both attempts"}[kept]
        add(label, of(S), why, broken(15) if kept == 15 else ok(kept))
    S = S1.copy()
    S[:, NB + 3] = 0.0
    add("odd47", of(S), "one W column is zero: ma = 47, ODD FIRST decomposition; an index map with a hole", ok(47))
    S = S1.copy()
    S[:, 2 * NB:] = 0.0
    S[:, NB + 9] = 0.0
    add("odd31", of(S), "P and one W column are zero: ma = 31, both decompositions odd", ok(31))
    S = S1.copy()
    for c in (1, 4, 5, 11):
        S[:, NB + c] = S[:, 2 * NB + c] = 0.0
    add("done4", of(S), "done columns 1, 4, 5, 11 (W_c = P_c = 0): ma = 40, SCATTERED index map", ok(40))
    S = S1.copy()
    S[:, NB + 1:2 * NB] = 0.0
    S[:, 2 * NB + 1:] = 0.0
    add("one_live", of(S), "done columns 1..15: ma = 18, kept just above nb, scattered index map", ok(18))
    S = S1.copy()
    S[:, 15:] = 0.0
    add("few", of(S), "15 positive Gram diagonals: ma < nb in both attempts, kept stays 0", broken(0))
    Bbad = B1.copy()
    Bbad[5, 5], Bbad[20, 20], Bbad[40, 40] = 0.0, -1.0, np.inf
    add("baddiag", (A1, Bbad), "Gram diagonals 0, -1 and inf beside good ones: EXCLUDED directions in X, W and P, odd sizes (45)", ok(45))

    # --- structure
    add("identity", (np.eye(M), np.eye(M)), "(I, I): off == 0 before the first sweep, all values TIED (ranking by index)", ok(48),
        exact_theta=np.ones(NB))
    add("diag", (np.diag(np.arange(48.0, 0.0, -1.0)), np.eye(M)), "(diag(48..1), I): off == 0, the ranking reverses the order; exact values",
        ok(48), exact_theta=np.arange(1.0, NB + 1.0))
    Ab, Bb = A1.copy(), B1.copy()
    for Z in (Ab, Bb):
        Z[:24, 24:] = 0.0
        Z[24:, :24] = 0.0
    add("blockdiag", (Ab, Bb), "two 24 x 24 blocks: EXACT ZEROS, the apq == 0 path without a rotation", ok(48))
    K = rng.normal(size=(M, M))
    K = K - K.T
    add("skew", (A1 + K, B1 + K), "a skew-symmetric matrix added to both: the symmetrisation of step 1", ok(48))

    # --- scales
    add("graded", of(S1 * 10.0 ** rng.uniform(-12.0, 0.0, size=M)), "columns GRADED over twelve orders of magnitude: step 2", ok(48))
    S = S1.copy()
    S[:, NB:2 * NB] *= 1e-9
    S[:, 2 * NB:] *= 1e-4
    add("lobpcg_scales", of(S), "W at 1e-9, P at 1e-4 beside a unit X: the scales of a late iteration", ok(48))
    w, V = np.linalg.eigh(Aop)
    S = np.empty((ROWS, M))
    S[:, :NB] = V[:, :NB] + 1e-6 * rng.normal(size=(ROWS, NB))
    Xl = S[:, :NB]
    S[:, NB:2 * NB] = Aop @ Xl - Xl * (np.sum(Xl * (Aop @ Xl), axis=0) / np.sum(Xl * Xl, axis=0))
    S[:, 2 * NB:] = 1e-5 * rng.normal(size=(ROWS, NB))
    add("lobpcg", of(S), "X near the 16 lowest eigenvectors, W their residuals, a small P: a late iteration as it is", ok(48))
    add("tiny", of(S1 * 1e-150), "columns of 1e-150: Gram entries of 1e-298 beside the absolute 1e-300 test", ok(48))
    add("huge", of(S1 * 1e140), "columns of 1e140: Gram entries of 1e282 beside the finiteness test", ok(48))
    # the same late iteration on a stiff operator (eigenvalues over eight orders of magnitude): the value of the reduced problem
    # and the Rayleigh quotient of the vector part ways by far more than the quotient's rounding -- what step 4 recomputes
    Qs, _ = np.linalg.qr(rng.normal(size=(ROWS, ROWS)))
    stiff = (Qs * 10.0 ** np.sort(rng.uniform(0.0, 8.0, size=ROWS))) @ Qs.T
    stiff = 0.5 * (stiff + stiff.T)
    S = np.empty((ROWS, M))
    S[:, :NB] = Qs[:, :NB] + 1e-6 * rng.normal(size=(ROWS, NB))
    Xl = S[:, :NB]
    S[:, NB:2 * NB] = stiff @ Xl - Xl * (np.sum(Xl * (stiff @ Xl), axis=0) / np.sum(Xl * Xl, axis=0))
    S[:, 2 * NB:] = 1e-5 * rng.normal(size=(ROWS, NB))
    add("lobpcg_stiff", (S.T @ stiff @ S, S.T @ S), "a late iteration on a stiff operator: theta is the RAYLEIGH QUOTIENT of its vector", ok(48))

    # --- retry and the two rules
    add("zeroP", (without_p(A1), without_p(B1)), "the full pencil with the P rows and columns zeroed: what a retry must repeat", ok(32))
    An = A1.copy()
    An[37, 5] = np.nan
    add("nanP", (An, B1), "a NaN in the P rows of S'AS: RETRY taken, on the LDS state the first attempt left", no_p(32),
        bits_of={False: "zeroP", True: "zeroP"})
    Ai = A1.copy()
    Ai[35, 40] = np.inf
    add("infP", (Ai, B1), "an inf in the P-P block of S'AS: retry taken", no_p(32), bits_of={False: "zeroP", True: "zeroP"})
    Ag = A1.copy()
    Ag[2 * NB:, 2 * NB:] *= -1.0
    Ag[:2 * NB, 2 * NB:] = 0.0
    Ag[2 * NB:, :2 * NB] = 0.0
    add("negP", (Ag, B1), "P-P block negated, cross blocks zero: the retry SEPARATES THE RULES (definite: P dropped; indefinite: kept)",
        {False: (RITZ_NO_P, 32), True: (RITZ_OK, 48)}, negatives=16, bits_of={False: "zeroP"})
    vals = sla.eigh(A1, B1, eigvals_only=True)
    sigma = 0.5 * (vals[2] + vals[3])
    add("shift3", (A1 - sigma * B1, B1), "(A - sigma B, B), sigma between the 3rd and 4th value: A FEW NEGATIVE values among positive ones",
        {False: (RITZ_NO_P, 32), True: (RITZ_OK, 48)}, negatives=3)

    assert len({p.label for p in out}) == len(out)
    for p in out:
        p.A.setflags(write=False)
        p.B.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def by_label():
    return {p.label: p for p in family()}


@functools.lru_cache(maxsize=None)
def checked_family():
    """``family()`` after the conditions of the head of the file have passed on every pencil."""
    for p in family():
        _check(p)
    return family()


def mpmath_distance(p, status, digits=40):
    """The reference's own error on (T, G): max |scipy.linalg.eigh - mpmath at ``digits`` digits| over the nb lowest values, in
    units of the bound on theta."""
    import mpmath as mp
    ref = reference(p, status)
    with mp.workdps(digits):
        T, G = mp.matrix(ref["T"].tolist()), mp.matrix(ref["G"].tolist())
        T, G = (T + T.T) / 2, (G + G.T) / 2
        Li = mp.inverse(mp.cholesky(G))
        C = Li * T * Li.T
        exact = sorted(mp.eigsy((C + C.T) / 2, eigvals_only=True))[:NB]
        return float(max(abs(mp.mpf(float(a)) - b) for a, b in zip(ref["want"][:NB], exact)) / mp.mpf(ref["theta_bound"]))
