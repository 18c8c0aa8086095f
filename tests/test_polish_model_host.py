"""The long-double model of the Newton polish (polish_helpers.py) tested on itself, without a GPU: a float64 restatement of
the model stays under every bound on every shape the GPU tests use (the bounds are not too tight), its gradient is the
derivative of its F, and the checkers catch planted errors in the restatement (they are not too loose).  The points are
the CPU twin's ADMM iterates (the twin has no polish: it supplies D, E and x only).  The HIP kernels:
test_polish_model_gpu.py."""
import numpy as np
import pytest

import operator_helpers as oh
import polish_helpers as ph

CASES = ["A", "B", "E40", "E60", "C1024", "F", "G", "L64", "L65", "L64-3d", "L65-3d", "prior2d", "A-qcqp", "PH1", "PH2", "PH3", "PH1-nohint",
         "PH2-nohint", "PH3-nohint"]
_points = {}


def points(case, twin_lib):
    """(view, scaled problem, u) of every problem of a case at the case's point, computed once and never changed."""
    if case not in _points and case == "A-qcqp":
        _points[case] = [_qcqp_point(twin_lib)]
    if case not in _points:
        from score_amd.solver import ConicSolver

        models = ph.case_models(case)
        sol = ConicSolver([m.qp for _, m in models], ph.case_settings(case), lib_path=twin_lib)
        try:
            views = oh.problem_views(sol, models)
            sol.reset()
            if ph.case_steps(case):
                sol.steps(ph.case_steps(case))
            x = sol.debug_get("x")
        finally:
            sol.close()
        out = []
        for v in views:
            S = ph.scaled_of_view(v)
            u = v.cut(x).copy()
            u[S.is_head] = 0.0
            u.setflags(write=False)
            out.append((v, S, u))
        _points[case] = out
    return _points[case]


def _qcqp_point(twin_lib):
    """Graph A as the QCQP relaxation, which a handle rewrites into the head form before it scales: the scaled problem is read
    from the twin's own arrays (polish_helpers.scaled_of_handle: data without error, so most bounds are those of the
    arithmetic alone) after 15 ADMM iterations.  There is no view: (None, scaled problem, u)."""
    from score_amd.assemble import assemble
    from score_amd.solver import ConicSolver

    qp = assemble(oh.model_of("A")[0], "QCQP").qp
    sol = ConicSolver(qp, dict(ph.NEWTON_SETTINGS), lib_path=twin_lib)
    try:
        sol.reset()
        sol.steps(ph.STEPS)
        arr = {k: sol.debug_get(k) for k in ph.HANDLE_ARRAYS + ("x",)}
    finally:
        sol.close()
    n, m = arr["qs"].size, arr["bs"].size
    first, dims, _ = oh.cone_layout(qp)
    assert m == qp.m and n < qp.n
    S = ph.scaled_of_handle(arr, n, m, 0, 0, first, int(dims[0]) - 1, arr["D"])
    u = np.where(S.is_head, 0.0, arr["x"][:n])
    u.setflags(write=False)
    return None, S, u


def _model(v, S, u):
    """The model with F summed as NumPy sums it in polish_float64: the row terms and the cone terms pairwise, one add."""
    return ph.polish_model(v, u, scaled=S, f_ops=max(ph.numpy_sum_ops(S.n), ph.numpy_sum_ops(S.first.size)) + 1)


def _restatement(v, S, u):
    return ph.polish_float64(v, u, scaled=S if v is None else None)


def _as_state(r):
    return dict(F=r["F"], gn=r["gn"], g=r["g"], nu=r["nu"], B=r["B"], act=r["act"])


@pytest.mark.parametrize("case", CASES)
def test_a_float64_restatement_stays_under_every_bound(case, twin_lib):
    """polish_float64 -- the model's formulas in plain float64 NumPy, sums in NumPy's order -- against polish_model at the
    case's point: F, the stopping measure, g, nu, B, every entry of H and the finish under the bounds, zero-bound entries
    equal, the classes equal; A-qcqp runs the path that builds the model from a handle's own arrays.  The graph cases hold active and inactive cones both; PH: the expected class of every cone,
    none undecided, nu = 0 and B = 0 exactly on the boundary cones, B = c I where theta = 0."""
    for k, (v, S, u) in enumerate(points(case, twin_lib)):
        m = _model(v, S, u)
        r = _restatement(v, S, u)
        fe, fh = ph.evaluation_figures(m, _as_state(r)), ph.hessian_figures(m, r["keys"], r["Hval"])
        x = u.copy()
        x[S.head_col] = r["xhead"]
        ff = ph.finish_figures(m, x, r["s"], r["y"])
        print(f"POLISH host {case}[{k}] n={S.n} cones={S.first.size} active={int(m['cls'].sum())} undecided={int(m['undecided'].sum())} "
              f"terms<={int(m['H_terms'].max())} | F {fe['F'][0]:.4f} gn {fe['gn'][0]:.4f} g {fe['g'][0]:.4f} nu {fe['nu'][0]:.4f} B {fe['B'][0]:.4f} "
              f"H {fh['ratio'][0]:.4f} long {fh['long'][0]:.4f} ({fh['long'][1]}) | heads {ff['heads'][0]:.4f} s {ff['s'][0]:.4f} y {ff['y'][0]:.4f}")
        assert ph.evaluation_ok(fe), (case, k, fe)
        assert ph.hessian_ok(fh), (case, k, fh)
        assert ph.finish_ok(ff), (case, k, ff)
        if case.startswith("PH"):
            ph.assert_ph_expected(S, m["cls"], m["undecided"], r["nu"], r["B"])
        else:
            assert 0 < int(m["cls"].sum()) < S.first.size, (case, k)
    if case in ("L64", "L64-3d"):
        assert int(m["H_terms"].max()) == ph.LONG_CONTRIB and fh["long"][1] == 0
    if case in ("L65", "L65-3d"):
        assert int(m["H_terms"].max()) == ph.LONG_CONTRIB + 1 and fh["long"][1] == S.T * S.T
    if case == "F":
        assert int(m["H_terms"].max()) == 833


def test_the_gradient_is_the_derivative_of_F(twin_lib):
    """On graph A: g'd of the model against central differences of the model's F in np.longdouble along three random
    directions on the non-head entries, c(h) = (F(u + h d) - F(u - h d)) / 2 h with h = 1e-5 |u|_inf / |d|_inf, extrapolated
    once, (4 c(h / 2) - c(h)) / 3 (F is smooth between the cones' boundaries, not quadratic: |t| is a norm; the extrapolation
    leaves O(h^4) and the rounding of F in np.longdouble, 1e-19 |F| / h): relative 1e-9."""
    v, S, u = points("A", twin_lib)[0]
    m = ph.polish_model(v, u, scaled=S)
    rng = np.random.default_rng(3)
    for _ in range(3):
        d = np.where(S.is_head, 0.0, rng.normal(size=S.n))
        h = 1e-5 * np.abs(u).max() / np.abs(d).max()

        def central(step):
            fp, fm = ph.polish_model(v, u + step * d, scaled=S)["F"], ph.polish_model(v, u - step * d, scaled=S)["F"]
            return (fp.v - fm.v) / (2 * oh.LD(step))

        fd = (4 * central(h / 2) - central(h)) / 3
        gd = ph.directional_derivative(m, d)
        print(f"POLISH host gradient check g'd {float(gd.v):.12e} difference {float(fd):.12e} relative {abs(float(fd - gd.v)) / abs(float(gd.v)):.2e}")
        assert abs(float(fd - gd.v)) <= 1e-9 * abs(float(gd.v)), (float(fd), float(gd.v))


# ---------------------------------------------------------------------------------------------------------------------
# planted errors
# ---------------------------------------------------------------------------------------------------------------------
def _clean(case, twin_lib, k=0):
    v, S, u = points(case, twin_lib)[k]
    m, r = _model(v, S, u), _restatement(v, S, u)
    assert ph.evaluation_ok(ph.evaluation_figures(m, _as_state(r))) and ph.hessian_ok(ph.hessian_figures(m, r["keys"], r["Hval"]))
    return v, S, u, m, r


def test_a_dropped_contribution_of_a_long_entry_is_caught(twin_lib):
    """L65: one of the 65 contributions of a beacon entry of H left out (the largest of an entry with more than kLongContrib):
    H fails, on a long entry."""
    v, S, u, m, r = _clean("L65", twin_lib)
    lg = m["keys"][m["H_terms"] > ph.LONG_CONTRIB]
    key = int(lg[0])
    s0, s1 = r["contrib"][key]
    vals = r["contrib_vals"][s0:s1]
    assert s1 - s0 == 65 and np.abs(vals).max() > 0
    Hval = r["Hval"].copy()
    Hval[np.searchsorted(r["keys"], key)] -= vals[np.argmax(np.abs(vals))]
    f = ph.hessian_figures(m, r["keys"], Hval)
    assert not ph.hessian_ok(f) and f["long"][0] > 1.0 and f["worst"] == key


def test_a_neighbouring_cones_block_is_caught(twin_lib):
    v, S, u, m, r = _clean("A", twin_lib)
    k = int(np.nonzero(m["cls"] == ph.ACTIVE)[0][0])
    B = r["B"].copy()
    B[k] = r["B"][k + 1 if k + 1 < len(B) else k - 1]
    f = ph.evaluation_figures(m, dict(_as_state(r), B=B))
    assert not ph.evaluation_ok(f) and f["B"][0] > 1.0 and all(f[q][0] <= 1.0 for q in ("F", "gn", "g", "nu"))


def test_a_wrong_sign_of_nu_is_caught(twin_lib):
    v, S, u, m, r = _clean("E40", twin_lib)
    row = int(np.argmax(np.abs(r["nu"])))
    nu = r["nu"].copy()
    nu[row] = -nu[row]
    f = ph.evaluation_figures(m, dict(_as_state(r), nu=nu))
    assert not ph.evaluation_ok(f) and f["nu"][0] > 1.0


def test_a_boundary_cone_classed_active_is_caught(twin_lib):
    """PH2: a cone with rho = theta exactly classed active with the active branch's block c tau tau': the class and B fail
    (its bounds are 0: the block must be 0 exactly)."""
    v, S, u, m, r = _clean("PH2", twin_lib)
    kinds, _ = ph.ph_expected(S.T)
    k = kinds.index("boundary")
    act, B = r["act"].copy(), r["B"].copy()
    tau = np.array([3.0, 4.0]) / 5.0
    act[k], B[k] = 2, np.outer(tau, tau)
    f = ph.evaluation_figures(m, dict(_as_state(r), act=act, B=B))
    assert not f["act"] and not f["B"][1]


def test_a_missing_regularisation_is_caught(twin_lib):
    v, S, u, m, r = _clean("A", twin_lib)
    Hval = r["Hval"].copy()
    diag = (r["keys"] // S.n == r["keys"] % S.n) & ~S.is_head[r["keys"] // S.n]
    Hval[diag] -= ph.REG
    f = ph.hessian_figures(m, r["keys"], Hval)
    assert not ph.hessian_ok(f) and f["ratio"][0] > 1.0


def test_F_without_one_cone_block_is_caught(twin_lib):
    """F: the cone terms of one block of 256 cones left out of F (the block with the largest sum)."""
    v, S, u, m, r = _clean("F", twin_lib)
    blocks = [r["phi"][b : b + 256].sum() for b in range(0, r["phi"].size, 256)]
    assert max(blocks) > 0
    f = ph.evaluation_figures(m, dict(_as_state(r), F=r["F"] - max(blocks)))
    assert not ph.evaluation_ok(f) and f["F"][0] > 1.0 and f["g"][0] <= 1.0


def test_a_step_of_another_members_length_is_caught(twin_lib):
    """u1 = u0 + 1/2 delta where the member's accepted step is 1 (a batch mate's length): the step check fails; the right step
    passes to one rounding."""
    v, S, u, m, r = _clean("A", twin_lib)
    delta = np.where(S.is_head, 0.0, -r["g"] / np.abs(r["g"]).max())
    good, bad = u + 1.0 * delta, u + 0.5 * delta
    assert ph.step_figures(S, u, delta, 1.0, good) == (ph.step_figures(S, u, delta, 1.0, good)[0], True) and ph.step_figures(S, u, delta, 1.0, good)[0] <= 1.0
    assert ph.step_figures(S, u, delta, 1.0, bad)[0] > 1.0


def test_y_head_without_the_root_is_caught(twin_lib):
    v, S, u, m, r = _clean("A", twin_lib)
    x = u.copy()
    x[S.head_col] = r["xhead"]
    assert ph.finish_ok(ph.finish_figures(m, x, r["s"], r["y"]))
    y = r["y"].copy()
    y[S.first] = y[S.first] ** 2
    f = ph.finish_figures(m, x, r["s"], y)
    assert not ph.finish_ok(f) and f["y"][0] > 1.0 and f["s"][0] <= 1.0
