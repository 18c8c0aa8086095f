"""The semismooth-Newton polish on the device -- k_newton_cone_b, k_spmv<MODE_GRAD>, k_hassemble (short and long entries),
the Newton PCG on H, k_newton_trial_b, k_copy_segments, k_polish_finish_b and the host rule around them
(HipBackend::polish_lockstep) -- against the np.longdouble model of polish_helpers.py, entry by entry under forward-error
bounds counted operation by operation (the derivations: the docstring of polish_helpers).  The points are ADMM iterates
(reset(), steps(k)), for the hand-made programs x = 0.  Run with -m gpu on an MI355X; profiles/polish_model.md records the
measured figures beside their bounds."""
import numpy as np
import pytest

import operator_helpers as oh
import polish_helpers as ph

pytestmark = pytest.mark.gpu

LINK_PAIRS = {"B": 8, "E60": 6, "G": 8}  # (as in test_operator_identities_gpu.py)


def _hip_only(hip_lib):
    import ctypes

    lib = ctypes.CDLL(hip_lib)
    lib.score_backend.restype = ctypes.c_char_p
    assert lib.score_backend().decode() == "hip-gfx950"


FAC = [(0, "double"), (None, "default"), (2, "float")]


def _handle(case, hip_lib, fac_fp32=None):
    from score_amd.solver import ConicSolver

    extra = {} if fac_fp32 is None else dict(fac_fp32=fac_fp32)
    if case == "A-qcqp":  # graph A as the QCQP relaxation: the handle rewrites it into the head form, the view reads the handle's arrays
        from score_amd.assemble import assemble

        qp = assemble(oh.model_of("A")[0], "QCQP").qp
        sol = ConicSolver(qp, ph.case_settings(case, **extra), lib_path=hip_lib)
        return sol, [ph.HandleView(sol, qp)]
    models = ph.case_models(case)
    sol = ConicSolver([m.qp for _, m in models], ph.case_settings(case, **extra), lib_path=hip_lib)
    views = oh.problem_views(sol, models)
    return sol, [ph.with_chains(v) for v in views] if case.startswith("PH") else views


def _scaled(v):
    return getattr(v, "S", None)


def _u_figures(v, fin):
    if _scaled(v) is not None:
        return ph.u_figures(v.S, v.rho, v.cut_rows(fin["u"]), v.cut_rows(fin["y"]), v.cut_rows(fin["s"]))
    return oh.u_refresh_figures(v, v.rho, fin["u"], fin["y"], fin["s"])


def _to_the_point(sol, case):
    sol.reset()
    if ph.case_steps(case):
        sol.steps(ph.case_steps(case))
    assert sol.debug_get("polish_assemble_at_x").size == 1


# (id, what the shape reaches)
EVAL_CASES = [
    "A",           # base
    "B",           # loop closures
    "E40",         # 3-D: T = 3
    "E60",         # ... with loop closures
    "C1024",       # join level: 703 cones, three cone blocks
    "F",           # entries of 833 contributions: the long-entry path of k_hassemble, the split long rows of MODE_GRAD
    "G",           # lock-step batch: cone blocks and row blocks straddle problems
    "L64", "L65",  # the beacon's entries collect 64 and 65 contributions: either side of kLongContrib
    "L64-3d", "L65-3d",
    "prior2d",     # landmark priors
    "PH1", "PH2", "PH3",  # hand-made private-head programs, a chain hint of block size T
    "PH1-nohint", "PH2-nohint", "PH3-nohint",  # ... and none
]


@pytest.mark.parametrize("case", EVAL_CASES)
def test_evaluation_and_hessian_against_the_model(case, hip_lib):
    """E and H.  polish_assemble_at_x at the case's point, then for every problem of the handle:

    E  F and the stopping measure max |g_i| / D_i (polish_eval), g row by row, nu row by row, B block by block, all under the
       model's bounds, zero-bound entries equal; bit 1 of every act word is the model's class (off the undecided cones); the
       head entries of g are exactly 0; on a fresh handle the flips counted are the active cones (the reference bits are 0).
    H  every stored entry of Hval under its bound; the pattern holds every entry of the model, and what it holds beyond them
       is exactly 0; entries that only inactive cones touch equal the stored P part (polish_Pon) bit for bit, and that
       P part lies under its own bound (two roundings of D P D, one of the regularisation; 0 where it is exact).
       The entries with more than kLongContrib contributions are reported on their own (F, G, C1024, L65).
       The entries the handle sends down the long path (polish_blocks) are exactly the model's entries with more than
       kLongContrib contributions: none on L64, the T^2 entries of the beacon on L65.
    The graph cases hold active and inactive cones both; L64 / L65 collect exactly 64 / 65 contributions; the PH programs
    show the table of polish_helpers.private_head_program."""
    _hip_only(hip_lib)
    sol, views = _handle(case, hip_lib)
    try:
        _to_the_point(sol, case)
        states = ph.device_state(sol, views)
        x = sol.debug_get("x")
    finally:
        sol.close()
    for k, (v, st) in enumerate(zip(views, states)):
        m = ph.model_at(v, st)
        S = m["S"]
        assert np.array_equal(st["u"], np.where(S.is_head, 0.0, v.cut(x))), "the point evaluated is x with the heads at 0"
        fe, fh = ph.evaluation_figures(m, st), ph.hessian_figures(m, st["keys"], st["Hval"], st["Pon"])
        decided_active = int(((m["cls"] == ph.ACTIVE) & ~m["undecided"]).sum())
        print(f"POLISH {case}[{k}] n={S.n} cones={S.first.size} active={int(m['cls'].sum())} undecided={int(m['undecided'].sum())} "
              f"terms<={int(m['H_terms'].max())} | F {fe['F'][0]:.4f} gn {fe['gn'][0]:.4f} g {fe['g'][0]:.4f} nu {fe['nu'][0]:.4f} B {fe['B'][0]:.4f} | "
              f"H {fh['ratio'][0]:.4f} long {fh['long'][0]:.4f} ({fh['long'][1]} entries) stored {st['keys'].size} model {m['keys'].size} P part alone {fh['p_part'][1]}")
        assert ph.evaluation_ok(fe), (case, k, fe)
        assert st["cols_in_range"] and ph.hessian_ok(fh) and fh["p_part"][1] > 0, (case, k, fh)
        assert decided_active <= st["flips"] <= decided_active + int(m["undecided"].sum()), (st["flips"], decided_active)
        assert np.array_equal(st["long_keys"], m["keys"][m["H_terms"] > ph.LONG_CONTRIB]), "the entries the handle gives the long path of k_hassemble"
        if case.startswith("PH"):
            ph.assert_ph_expected(S, (st["act"] >> 1) & 1, m["undecided"], st["nu"], st["B"])
        else:
            assert 0 < int(m["cls"].sum()) < S.first.size, (case, k)
        if case.startswith("L64"):
            assert int(m["H_terms"].max()) == ph.LONG_CONTRIB and fh["long"][1] == 0
        if case.startswith("L65"):
            assert int(m["H_terms"].max()) == ph.LONG_CONTRIB + 1 and fh["long"][1] == S.T * S.T
        if case == "F":
            assert int(m["H_terms"].max()) == 833 and fh["long"][1] > 0


def test_evaluation_and_hessian_of_a_qcqp_model_through_its_head_form(hip_lib):
    """E and H for graph A assembled as the QCQP relaxation, which the handle rewrites into the head form before it scales
    (score_headform.hpp: the rows and cones stay, the range directions leave the unknowns): the model is built from the
    handle's own scaled arrays (Aval / Aptr / Acol, G2val / G2ptr / G2col / G2split, qs, bs, D: the setup tests pin them),
    which then carry no error of their own."""
    _hip_only(hip_lib)
    import types

    from score_amd.assemble import assemble
    from score_amd.solver import ConicSolver

    fg, _ = oh.model_of("A")
    qp = assemble(fg, "QCQP").qp
    sol = ConicSolver(qp, dict(ph.NEWTON_SETTINGS), lib_path=hip_lib)
    try:
        sol.reset()
        sol.steps(ph.STEPS)
        assert sol.debug_get("polish_assemble_at_x").size == 1
        arr = {k: sol.debug_get(k) for k in ("Aval", "Aptr", "Acol", "G2val", "G2ptr", "G2col", "G2split", "qs", "bs", "D")}
        n, m = arr["qs"].size, arr["bs"].size
        first, dims, _ = oh.cone_layout(qp)
        view = types.SimpleNamespace(x0=0, x1=n, r0=0, r1=m, qp=types.SimpleNamespace(n=n, soc_dims=qp.soc_dims), cut=lambda a: np.asarray(a)[:n],
                                     cut_rows=lambda a: np.asarray(a)[:m])
        st = ph.device_state(sol, [view])[0]
    finally:
        sol.close()
    assert m == qp.m and n < qp.n, "the head form keeps the rows and drops the range directions"
    S = ph.scaled_of_handle(arr, n, m, 0, 0, first, int(dims[0]) - 1, arr["D"])
    mdl = ph.model_at(None, st, scaled=S)
    fe, fh = ph.evaluation_figures(mdl, st), ph.hessian_figures(mdl, st["keys"], st["Hval"], st["Pon"])
    print(f"POLISH A-qcqp[0] n={n} cones={first.size} active={int(mdl['cls'].sum())} undecided={int(mdl['undecided'].sum())} | F {fe['F'][0]:.4f} "
          f"gn {fe['gn'][0]:.4f} g {fe['g'][0]:.4f} nu {fe['nu'][0]:.4f} B {fe['B'][0]:.4f} | H {fh['ratio'][0]:.4f}")
    assert 0 < int(mdl["cls"].sum()) < first.size
    assert ph.evaluation_ok(fe), fe
    assert st["cols_in_range"] and ph.hessian_ok(fh), fh


# ---------------------------------------------------------------------------------------------------------------------
# one Newton iteration
# ---------------------------------------------------------------------------------------------------------------------
STEP_CASES = ["A", "B", "E40", "E60", "C1024", "F", "G", "L64", "L65", "L64-3d", "L65-3d", "prior2d", "A-qcqp", "PH1", "PH2", "PH3",
              "PH1-nohint", "PH2-nohint", "PH3-nohint"]
TRACE = dict(live=0, reref=1, eta=2, pcg_used=3, fired=4, F=5, gn=6, gd=7, trials=8, step=9, F_new=10, gn_new=11, stalled=12, tol=13)


def _one_ratio(got, ref):
    return ph._ratio(np.asarray([got]), ph.VB(ref.v.reshape(1), ref.e.reshape(1)))


@pytest.mark.parametrize("fac_fp32,fac", FAC, ids=[f for _, f in FAC])
@pytest.mark.parametrize("case", STEP_CASES)
def test_one_newton_iteration_against_the_model(case, fac_fp32, fac, hip_lib):
    """P, S and F(k = 1).  From the point of E (u0: the read-outs after polish_assemble_at_x), newton_steps(1); per problem:

    S(a) the trace's F, gn equal the evaluation's and lie under the model's bounds at u0, gd = g0'delta under the bound of the
         model's g0'delta (n products summed in blocks), F_new and gn_new under the model's bounds at u1;
    S(b) u1 = u0 + step delta entrywise to one rounding, heads 0 (polish_helpers.step_figures);
    S(c) the trial steps taken and the accepted step are the ones the model's Armijo rule takes on its own F, and the bounds
         separate every decision;
    S(d) the one iteration refactors (reref: it == 0), the problem is live and not stalled; the tolerance pcg_gate read for the
         problem (polish_gate) is the square of the trace's eta, bit for bit -- every member of a batch its own;
    S(e) phi = sqrt(rho'M^-1 rho / g0'M^-1 g0), rho = -g0 - H0 delta in np.longdouble with the model's g0 and H0 and M the model
         preconditioner of I4 on H0: phi <= 2 max(phi_ref, eta) with phi_ref of polish_helpers.pcg_reference stopped by the same
         gate at the trace's eta, and |pcg_used - k_ref| <= max(2, k_ref / 10);
    P    w = H p row by row for the last product of the Newton PCG (polish_p, w, z) in the form of I1 with pcg_used + 1
         products, on the H the device holds (which test H holds to the model);
    The shapes are those of E: the graphs on either side of kLongContrib, the landmark priors, graph A through the QCQP head form
    (its view reads the handle's own arrays: polish_helpers.HandleView) and the hand-made programs from x = 0, whose finish
    meets cones with rho = theta exactly and with theta = 0.
    F    x, s, y after the call against the model at u1: heads max(x*, rho / |a|), s_tail = t, s_head = |a| x_head,
         y_tail = nu, y_head = |y_tail|, s and y in the cone; kx = K xt as one fresh product and u = rho (bs - s) - y
         (operator_helpers.fresh_product_figures / u_refresh_figures)."""
    _hip_only(hip_lib)
    sol, views = _handle(case, hip_lib, fac_fp32)
    try:
        _to_the_point(sol, case)
        st0 = ph.device_state(sol, views)
        sol.newton_steps(1)
        trace = sol.debug_get("polish_trace").reshape(-1, len(views), len(TRACE))
        st1 = ph.device_state(sol, views)
        delta, p, w, z = (sol.debug_get(k) for k in ("polish_delta", "polish_p", "w", "z"))
        pcg = sol.debug_get("polish_pcg").reshape(2, -1)
        gate = sol.debug_get("polish_gate").reshape(2, -1)
        fin = {k: sol.debug_get(k) for k in ("x", "s", "y", "xt", "kx", "u")}
        pairs = sol.debug_get("link_pairs").size // 2
    finally:
        sol.close()
    assert trace.shape[0] == 1 and pairs == LINK_PAIRS.get(case, 0)
    fails = []
    for k, v in enumerate(views):
        tr = {nm: float(trace[0, k, i]) for nm, i in TRACE.items()}
        m0 = ph.model_at(v, st0[k], scaled=_scaled(v))
        S = m0["S"]
        m1 = ph.model_at(v, st1[k], scaled=S)
        d = v.cut(delta)
        gd = ph.directional_derivative(m0, np.where(S.is_head, 0.0, d), ops=st0[k]["gd_ops"])
        a = dict(F=_one_ratio(tr["F"], m0["F"]), gn=_one_ratio(tr["gn"], m0["gn"]), gd=_one_ratio(tr["gd"], gd),
                 F_new=_one_ratio(tr["F_new"], m1["F"]), gn_new=_one_ratio(tr["gn_new"], m1["gn"]))
        b = ph.step_figures(S, st0[k]["u"], d, tr["step"], st1[k]["u"])
        trials, step, separated, _ = ph.armijo_model(v, st0[k]["u"], np.where(S.is_head, 0.0, d), m0["F"], gd, scaled=S, f_ops=st0[k]["f_ops"])
        Minv = ph.model_preconditioner(v, m0["Hmat"])
        g0 = m0["g"].v
        phi = ph.step_quality(m0["Hmat"], g0, np.where(S.is_head, 0.0, d), Minv)
        x_ref, k_ref = ph.pcg_reference(m0["Hmat"], -g0, Minv, tr["eta"])
        phi_ref = ph.step_quality(m0["Hmat"], g0, x_ref, Minv)
        used = int(tr["pcg_used"])
        i1, i1_exact = oh.i1_figures(st0[k]["Hcsr"], v.cut(p), v.cut(w), v.cut(z), used + 1)
        ff = ph.finish_figures(m1, v.cut(fin["x"]), v.cut_rows(fin["s"]), v.cut_rows(fin["y"]))
        kx = oh.fresh_product_figures(v.K, v.cut(fin["xt"]), v.cut(fin["kx"]))
        uu = _u_figures(v, fin)
        print(f"POLISH {case}[{k}] fac={fac} step | F {a['F'][0]:.4f} gn {a['gn'][0]:.4f} gd {a['gd'][0]:.4f} F_new {a['F_new'][0]:.4f} gn_new {a['gn_new'][0]:.4f} | "
              f"u1 {b[0]:.4f} | trials {int(tr['trials'])}/{trials} step {tr['step']}/{step} | eta {tr['eta']:.3e} phi {phi:.3e} phi_ref {phi_ref:.3e} "
              f"pcg {used}/{k_ref} | w=Hp {i1:.4f} | heads {ff['heads'][0]:.4f} s {ff['s'][0]:.4f} y {ff['y'][0]:.4f} kx {kx[0]:.4f} u {uu[0]:.4f}")
        checks = {
            "a": all(r <= 1.0 and ex for r, ex in a.values()) and tr["F"] == st0[k]["F"] and tr["gn"] == st0[k]["gn"]
                 and tr["F_new"] == st1[k]["F"] and tr["gn_new"] == st1[k]["gn"],
            "b": b[0] <= 1.0 and b[1],
            "c": separated and int(tr["trials"]) == trials and tr["step"] == step,
            "d": tr["live"] == 1 and tr["reref"] == 1 and tr["stalled"] == 0 and tr["fired"] == 1,
            "e": phi <= 2 * max(phi_ref, tr["eta"]) and abs(used - k_ref) <= max(2, k_ref / 10),
            "pcg words": int(pcg[1, k]) == used and int(pcg[0, k]) == 1,
            "gate tolerance": gate[0, k] == tr["eta"] * tr["eta"] and gate[1, k] > 0,
            "P": i1 <= 1.0 and i1_exact,
            "F": ph.finish_ok(ff) and kx[0] <= 1.0 and kx[1] and uu[0] <= 1.0 and uu[1],
            "point": np.array_equal(v.cut(fin["x"])[~S.is_head], st1[k]["u"][~S.is_head]),
        }
        fails += [(f"{case}[{k}]", nm) for nm, ok in checks.items() if not ok]
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------
# I4 on a batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fac_fp32,fac", FAC, ids=[f for _, f in FAC])
def test_newton_preconditioner_identities_on_a_batch(fac_fp32, fac, hip_lib):
    """I4 of test_operator_identities_gpu.py for the batch G (A, B and S150 in one handle: the work items of k_factor and of
    the chain kernel straddle problems): after 15 ADMM iterations the Newton set is assembled and factored for all three
    and z = M^-1 (-g) comes from PREC_INIT; per problem T_H z = -g on the chain columns under the bounds of I3, Jacobi
    elsewhere, the link pairs those of the graph."""
    _hip_only(hip_lib)
    from score_amd.solver import ConicSolver

    models = oh.case_models("G")
    sol = ConicSolver([m.qp for _, m in models], {} if fac_fp32 is None else dict(fac_fp32=fac_fp32), lib_path=hip_lib)
    try:
        views = oh.problem_views(sol, models)
        sol.reset()
        sol.steps(15)
        assert sol.debug_get("polish_assemble_at_x").size == 1
        states = ph.device_state(sol, views)
        z = sol.debug_get("polish_prec_of_negg")
    finally:
        sol.close()
    assert sum(len(v.pairs) for v in views) == LINK_PAIRS["G"]
    for k, ((fg, model), v, st) in enumerate(zip(models, views, states)):
        f = oh.newton_figures(fg, model, st["Hcsr"], st["g"], v.cut(z), v.pairs, fac_fp32 != 0)
        print(f"POLISH G[{k}] newton fac={fac} n={model.qp.n} | I4 dev {f['i4']:.3e} model {f['i4_model']:.3e} bound {f['i4_bound']:.3e}")
        assert f["pairs_ok"] and np.abs(st["g"]).max() > 0
        assert f["i4"] <= f["i4_bound"] and f["jacobi"], (k, f)


# ---------------------------------------------------------------------------------------------------------------------
# to convergence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fac_fp32,fac", FAC, ids=[f for _, f in FAC])
@pytest.mark.parametrize("case", ["A", "E40", "G"])
def test_newton_to_convergence_and_the_finish(case, fac_fp32, fac, hip_lib):
    """newton_steps(50) from the case's point, every problem to its tolerance.  From the returned point (x with the heads at
    0), in the three factor modes (stale factors are what the refactor rule is about): the finish under the model's bounds
    (heads, s, y, the cones; kx = K xt as one fresh product and u = rho (bs - s) - y for every member, those that finished
    early and were skipped by the later iterations included); the model's stopping measure there is at most the
    trace's tolerance (plus its bound); every iteration's record is consistent -- F and gn of an iteration are F_new and
    gn_new of the problem's last live one, a problem is live exactly while its gn exceeds the tolerance and it has not
    stalled.  S(d) over the whole run: the points u_0, u_1, ... are read from the same sequence stopped after 0, 1, ...
    iterations, and reref of every iteration equals `it == 0 or the model's active set at u_it differs from the one at the
    last factorisation point`; the tolerance pcg_gate read for a problem in an iteration (polish_gate of the sequence stopped
    there, whose trace must repeat the first run's bit for bit) is the square of that problem's eta.  A member that finishes before the others comes back unchanged: its x, s, y equal bit for
    bit those of the sequence stopped at the member's last live iteration (G)."""
    _hip_only(hip_lib)
    sol, views = _handle(case, hip_lib, fac_fp32)
    try:
        _to_the_point(sol, case)
        infos = [o.info for o in sol.newton_steps(50)]
        trace = sol.debug_get("polish_trace").reshape(-1, len(views), len(TRACE))
        fin = {k: sol.debug_get(k) for k in ("x", "s", "y", "xt", "kx", "u")}
        last_live = [int(np.nonzero(trace[:, k, TRACE["live"]])[0].max()) + 1 for k in range(len(views))]
        early = {}  # the handle's x, s, y after 0, 1, ... iterations: the same sequence stopped earlier
        for it in range(trace.shape[0]):
            _to_the_point(sol, case)
            if it:
                sol.newton_steps(it)
            early[it] = {k: sol.debug_get(k) for k in ("x", "s", "y")}
            if it:  # the tolerances pcg_gate read in iteration it - 1, every member its own
                early[it]["tol2"] = sol.debug_get("polish_gate")[: len(views)]
                assert np.array_equal(sol.debug_get("polish_trace").reshape(-1, len(views), len(TRACE))[:it], trace[:it]), "the same sequence"
    finally:
        sol.close()
    assert all(i["newton_iters"] == trace.shape[0] for i in infos)
    if case == "G":
        assert len(set(last_live)) > 1, last_live
    for k, v in enumerate(views):
        S = ph.scaled_of_view(v)
        u = np.where(S.is_head, 0.0, v.cut(fin["x"]))
        m = ph.polish_model(v, u, scaled=S)
        ff = ph.finish_figures(m, v.cut(fin["x"]), v.cut_rows(fin["s"]), v.cut_rows(fin["y"]))
        tol = float(trace[0, k, TRACE["tol"]])
        kx = oh.fresh_product_figures(v.K, v.cut(fin["xt"]), v.cut(fin["kx"]))
        uu = _u_figures(v, fin)
        print(f"POLISH {case}[{k}] fac={fac} converged after {last_live[k]} of {trace.shape[0]} iterations | measure {float(m['gn'].v):.3e} tol {tol:.3e} | "
              f"heads {ff['heads'][0]:.4f} s {ff['s'][0]:.4f} y {ff['y'][0]:.4f} kx {kx[0]:.4f} u {uu[0]:.4f}")
        assert ph.finish_ok(ff), (k, ff)
        assert kx[0] <= 1.0 and kx[1] and uu[0] <= 1.0 and uu[1], (k, kx, uu)
        assert np.array_equal(v.cut(fin["xt"]), v.cut(fin["x"])), "xt is the returned point"
        assert float(m["gn"].v) <= tol + float(m["gn"].e), (float(m["gn"].v), tol)
        F, gn, stalled = None, None, False
        ref_cls = ref_und = None
        for it in range(trace.shape[0]):
            tr = {nm: float(trace[it, k, i]) for nm, i in TRACE.items()}
            # S(d): the factors are recomputed at the first iteration and whenever the model's active set at the iteration's
            # point differs from the one at the last factorisation point (cones undecided at either point may count or not)
            mi = ph.polish_model(v, np.where(S.is_head, 0.0, v.cut(early[it]["x"])), scaled=S)
            if it == 0:
                lo = hi = True
            else:
                diff, unsure = mi["cls"] != ref_cls, mi["undecided"] | ref_und
                lo, hi = bool(np.any(diff & ~unsure)), bool(np.any(diff & ~unsure) or np.any(unsure))
            if it + 1 < trace.shape[0]:
                assert early[it + 1]["tol2"][k] == tr["eta"] * tr["eta"], (it, k, early[it + 1]["tol2"], tr["eta"])
            if tr["live"]:
                assert lo <= bool(tr["reref"]) <= hi, (it, tr, lo, hi)
                if tr["reref"]:
                    ref_cls, ref_und = mi["cls"], mi["undecided"]
            else:
                assert tr["reref"] == 0
            if it > 0:
                assert tr["F"] == F and tr["gn"] == gn, (it, tr)
            assert tr["live"] == float(tr["gn"] > tr["tol"] and not stalled), (it, tr)
            if tr["live"]:
                stalled = bool(tr["stalled"])
                if not stalled:
                    F, gn = tr["F_new"], tr["gn_new"]
            else:
                F, gn = tr["F"], tr["gn"]
        if last_live[k] < trace.shape[0]:
            for nm in ("x", "s", "y"):
                cut = v.cut if nm == "x" else v.cut_rows
                assert np.array_equal(cut(fin[nm]), cut(early[last_live[k]][nm])), (k, nm)


@pytest.mark.parametrize("case", ["A", "G"])
def test_a_default_solve_ends_under_the_traces_tolerance(case, hip_lib):
    """solve() with the default settings: every problem solved; info.newton_iters is the length of the trace of the polish
    that ended the solve; the model's stopping measure at the returned point (the handle's x with the heads at 0) is at
    most the trace's tolerance for the problem, plus its bound."""
    _hip_only(hip_lib)
    from score_amd.solver import ConicSolver

    models = ph.case_models(case)
    sol = ConicSolver([m.qp for _, m in models], {}, lib_path=hip_lib)
    try:
        views = oh.problem_views(sol, models)
        infos = [o.info for o in sol.solve()]
        trace = sol.debug_get("polish_trace").reshape(-1, len(views), len(TRACE))
        x = sol.debug_get("x")
    finally:
        sol.close()
    for k, v in enumerate(views):
        S = ph.scaled_of_view(v)
        m = ph.polish_model(v, np.where(S.is_head, 0.0, v.cut(x)), scaled=S)
        tol = float(trace[0, k, TRACE["tol"]])
        print(f"POLISH {case}[{k}] solve: newton_iters {infos[k]['newton_iters']} trace {trace.shape[0]} | measure {float(m['gn'].v):.3e} tol {tol:.3e}")
        assert infos[k]["status"] == 1 and infos[k]["newton_iters"] == trace.shape[0], infos[k]
        assert float(m["gn"].v) <= tol + float(m["gn"].e)
