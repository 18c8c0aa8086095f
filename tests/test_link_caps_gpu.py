"""The loop-closure link correction of both chain preconditioners (csrc/score_link.hpp: k_link_cap, k_link_solve, k_link_apply,
k_link_group, the 48-vector launch of the chain kernel behind them) at the caps of its plan and one step beyond each, held to
the identities of test_operator_identities_gpu.py.  The generators' own loop closures reach groups of 24 unknowns on two
chains; the graphs of operator_helpers.LINK_GRAPHS reach

    case     largest group / most chains of a group     what runs
    L96      96 / 2    k_link_cap<false> (four wavefronts), listed nonzeros, k_link_group; 48 rounds on a chain
    HUB15    48 / 1    k_link_cap<true>, the plain walk (rows of G with 45 nonzeros), k_link_group; 48 rounds on ONE chain
    HUB93    93 / 3    k_link_cap<false>, the plain walk (hub rows: 30 nonzeros), k_link_solve + k_link_apply
    R3       90 / 3    k_link_cap<false>, listed nonzeros, k_link_solve + k_link_apply
    E96      96 / 2    3-D (blocks of 4, three groups): k_link_cap<false>, listed nonzeros, k_link_group
    N256     96 / 2    exactly 256 linked nodes, eight groups: k_link_cap<false>, listed nonzeros, k_link_group
    LS96     96 / 2    L96 on chains cut into segments: a link item per segment (8 chains, the twin counts 4 whole ones), the
                       join level inside the 48-vector launch; k_link_cap<false>, listed nonzeros, and -- four items to a group
                       -- k_link_solve + k_link_apply with the separators' columns
    GL       96, none, 33 in one lock-step batch: k_link_cap<false> on groups of two sizes, the plain walk in HUB10's
    L97, R3over, N260  beyond 48 rounds / 96 unknowns / 256 nodes: no pair inside, the chain preconditioner alone

The device's I3 and I4 are held to operator_helpers.link_cap_bound = 4 max(eta_model, eta_twin) (+ the 4 eps floor with double
factors), the twin's to operator_helpers.eta_bound except on LS96 with double factors (printed only: test_link_caps_host.py);
profiles/operator_identities.md records the measured figures beside their bounds.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import operator_helpers as oh
from oracle import score_oracle as so
from score_amd.solver import ConicSolver

pytestmark = pytest.mark.gpu
CG = 2


def _hip_only(hip_lib):
    import ctypes

    lib = ctypes.CDLL(hip_lib)
    lib.score_backend.restype = ctypes.c_char_p
    assert lib.score_backend().decode() == "hip-gfx950"


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("case", oh.LINK_CASES)
def test_link_correction_at_its_caps_against_scipy_identities(case, fp32, hip_lib, twin_lib):
    """I1, I2, I3 and Jacobi of test_admm_operators_against_scipy_identities for every problem of the handle after 5 and after
    10 iterations (cg_iters = 2), on the device and on the twin; T = chain part + the blocks of the pairs expected inside the
    preconditioner -- every loop closure of the graph, or none beyond a cap.  The device handle's six "links" figures equal
    the twin's first six, the twin's nine equal operator_helpers.LINK_PLANS, and no capacitance system was singular, before
    the first and after the last iteration."""
    _hip_only(hip_lib)
    models, inside = oh.case_models(case), oh.case_inside(case)
    settings = dict(cg_iters=CG, fac_fp32=fp32)
    dc, tc = {}, {}
    dev_views, dev = oh.admm_snapshots(models, settings, hip_lib, dc, inside=inside)
    twin_views, twin = oh.admm_snapshots(models, settings, twin_lib, tc, inside=inside)
    print(f"LINKCAP {case} fp32={fp32} links dev {dc['links']} twin {tc['links']}")
    assert tc["links"] == oh.case_link_plan(case)
    # (equal to the twin's first six; LS96 alone counts its chains per segment: operator_helpers.LINK_CHAINS_ON_DEVICE)
    assert dc["links"] == oh.device_link_plan(case) and dc["links_after"] == dc["links"] and dc["links"][5] == 0
    assert [v for k, v in enumerate(dc["links"]) if k != 3 or case != "LS96"] == [v for k, v in enumerate(tc["links"][:6]) if k != 3 or case != "LS96"]
    assert np.array_equal(dc["link_pairs"], tc["link_pairs"])
    failures = []
    for k, (dv, tv) in enumerate(zip(dev_views, twin_views)):
        for s in range(2):
            fd, ft = oh.admm_figures(dv, dev[s], CG, bool(fp32)), oh.admm_figures(tv, twin[s], CG, bool(fp32))
            b2 = oh.i2_bound(dv.K, ft["i2"])
            b3 = oh.link_cap_bound(fd["i3_model"], ft["i3"], bool(fp32))
            label = f"{case}[{k}] fp32={fp32} it={5 * (s + 1)}"
            print(f"LINKCAP {label} n={dv.qp.n} | I1 dev {fd['i1']:.4f} twin {ft['i1']:.4f} | I2 dev {fd['i2']:.3e} twin {ft['i2']:.3e} "
                  f"bound {b2:.3e} | I3 dev {fd['i3']:.3e} model {fd['i3_model']:.3e} bound {b3:.3e} twin {ft['i3']:.3e} bound {ft['i3_bound']:.3e}")
            checks = {
                "link pairs": fd["pairs_ok"] and ft["pairs_ok"],
                "I1": fd["i1"] <= 1.0 and fd["i1_exact"], "I1 twin": ft["i1"] <= 1.0 and ft["i1_exact"],
                "I2": fd["i2"] <= b2,
                "I3": fd["i3"] <= b3, "I3 Jacobi": fd["jacobi"], "I3 Jacobi twin": ft["jacobi"],
                "I3 twin": ft["i3"] <= ft["i3_bound"] or (case == "LS96" and not fp32),
            }
            failures += [(label, nm, fd, ft) for nm, ok in checks.items() if not ok]
    assert not failures, failures


NEWTON_CASES = ["L96", "HUB15", "HUB93", "R3", "E96", "LS96", "L97"]


@pytest.mark.parametrize("fac_fp32", [0, None, 2], ids=["double", "default", "float"])
@pytest.mark.parametrize("case", NEWTON_CASES)
def test_newton_link_correction_at_its_caps(case, fac_fp32, hip_lib, twin_lib):
    """I4 of test_newton_preconditioner_against_scipy_identities on the Newton set: T_H z = -g with T_H = chain part + link
    blocks of the H the device assembled (L97: the chain part alone), Jacobi off the chains, no singular capacitance system in
    either set.  The device is held to operator_helpers.link_cap_bound, as in I3.  The twin's figure comes from its linear mode
    on the same H and the same chains (operator_helpers.newton_twin_figures: z = M^-1 r for the residual r after one PCG step
    from -g); the twin must find the plan of operator_helpers.LINK_PLANS in H's pattern and is itself held to
    operator_helpers.eta_bound, except on LS96 with double factors (printed only, as in I3).

    Against the model alone three cases would miss (profiles/operator_identities.md): L97 float 1.269e-08 against
    4 x 1.379e-09, HUB93 float 3.755e-08 against 4 x 5.877e-09, LS96 double 1.060e-14 against 16 eps.  The model eliminates
    every chain from its first node to its last; eliminated from the last to the first it gives 1.267e-08 on L97's system, the
    device's own figure, and on the twin's right-hand side 1.136e-08 -- it moves by 9 x where the twin, which eliminates in the
    device's order, stands within 2.2 x of the device in all three."""
    _hip_only(hip_lib)
    fg, model = oh.model_of(case)
    (inside,) = oh.case_inside(case)
    counters = {}
    H, g, z, pairs = oh.newton_snapshot(model, {} if fac_fp32 is None else dict(fac_fp32=fac_fp32), hip_lib, counters)
    floats = fac_fp32 != 0
    f = oh.newton_figures(fg, model, H, g, z, pairs, floats, inside=inside)
    ft = oh.newton_twin_figures(fg, model, H, g, floats, twin_lib, inside=inside)
    bound = oh.link_cap_bound(f["i4_model"], ft["i4"], floats)
    print(f"LINKCAP {case} newton fac_fp32={fac_fp32} n={model.qp.n} links {counters['links']} | I4 dev {f['i4']:.3e} model {f['i4_model']:.3e} "
          f"bound {bound:.3e} | twin {ft['i4']:.3e} model {ft['i4_model']:.3e} bound {ft['i4_bound']:.3e}")
    assert counters["links"] == oh.device_link_plan(case) and ft["links"] == oh.LINK_PLANS[case]
    assert len(pairs) == oh.LINK_PLANS[case][1]
    assert f["pairs_ok"] and ft["pairs_ok"], pairs
    assert np.abs(g).max() > 0 and ft["r_max"] > 0
    assert ft["i4"] <= ft["i4_bound"] or (case == "LS96" and fac_fp32 == 0), ft
    assert ft["jacobi"], ft
    assert f["i4"] <= bound, (f, ft)
    assert f["jacobi"], f


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("case", ["L96", "HUB93"])
def test_link_correction_at_its_caps_after_penalty_updates(case, fp32, hip_lib, twin_lib):
    """The sequence of test_identities_after_penalty_updates: the correction is derived again after every k_kval (the rounds,
    k_link_cap at 96 and 93 unknowns), then I1-I3 after one replayed block under the updated penalty and after reset();
    the device's I3 under operator_helpers.link_cap_bound, the twin under today's rule."""
    _hip_only(hip_lib)
    models = oh.case_models(case)
    settings = dict(adaptive_rho=1, use_graph=1, fac_fp32=fp32)
    dev = oh.penalty_update_run(models, settings, hip_lib)
    twin = oh.penalty_update_run(models, settings, twin_lib)
    fails, lines = oh.penalty_update_checks(dev, bool(fp32), f"{case} fp32={fp32}", yard=twin, expect_launches=6, link_caps=True)
    tfails, tlines = oh.penalty_update_checks(twin, bool(fp32), f"twin {case} fp32={fp32}", expect_launches=0)
    print("\n".join(lines + tlines))
    assert dev["links"] == oh.device_link_plan(case) and twin["links"] == oh.LINK_PLANS[case]
    assert not fails and not tfails, (fails, tfails)


def _solve(qp, hip_lib):
    sol = ConicSolver([qp], {}, lib_path=hip_lib)
    try:
        before = oh.links_of(sol)
        out = sol.solve()[0]
        return out, before, oh.links_of(sol), sol.debug_get("link_pairs")
    finally:
        sol.close()


@pytest.mark.parametrize("case", ["L96", "HUB93"])
def test_graph_path_finds_the_same_link_plan_at_its_caps(case, hip_lib):
    """The handle made from the graph (ConicSolver.from_graphs: links from the measurement list) against the one made from the
    arrays (links from P's pattern): the same "links" figures and bit-equal link pairs."""
    from score_amd.native import graph_arrays

    _hip_only(hip_lib)
    fg, model = oh.model_of(case)
    out = []
    for make in (lambda: ConicSolver.from_graphs([graph_arrays(fg)], 0, {}, lib_path=hip_lib), lambda: ConicSolver([model.qp], {}, lib_path=hip_lib)):
        sol = make()
        try:
            out.append((oh.links_of(sol), sol.debug_get("link_pairs")))
        finally:
            sol.close()
    (g_links, g_pairs), (a_links, a_pairs) = out
    assert g_links == a_links == oh.device_link_plan(case)
    assert g_pairs.size == 2 * a_links[1] and np.array_equal(g_pairs, a_pairs)


@pytest.mark.parametrize("case", ["L96", "R3", "E96"])
def test_default_solve_with_a_link_plan_at_its_caps(case, hip_lib, monkeypatch):
    """The default solve (ADMM loop + Newton polish, both preconditioners with the correction) against SCORE_NO_LINKS=1: both
    solved, the same objective to 1e-7, the KKT certificate of test_loop_closures_inside_the_newton_preconditioner, the
    oracle's Newton objective to 1e-6, and no more Newton PCG iterations with the links than without (both counts printed: the
    ratio has not been measured at these sizes, none is asserted)."""
    _hip_only(hip_lib)
    fg, model = oh.model_of(case)
    qp = model.qp
    monkeypatch.delenv("SCORE_NO_LINKS", raising=False)
    a, ia, ia_after, pa = _solve(qp, hip_lib)
    monkeypatch.setenv("SCORE_NO_LINKS", "1")
    b, ib, _, _ = _solve(qp, hip_lib)
    monkeypatch.delenv("SCORE_NO_LINKS", raising=False)
    print(f"LINKCAP {case} solve | links {ia} | pobj {a.info['pobj']:.12g} plain {b.info['pobj']:.12g} | iters {a.info['iters']} plain {b.info['iters']} | "
          f"newton_cg_iters {a.info['newton_cg_iters']} plain {b.info['newton_cg_iters']}")
    assert ia == oh.device_link_plan(case) and ia_after == ia and ib[1] == 0 and ib[3] == 0, (ia, ia_after, ib)
    assert pa.size == 2 * ia[1]
    assert a.solved and b.solved, (a.info, b.info)
    assert a.info["pobj"] == pytest.approx(b.info["pobj"], rel=1e-7, abs=1e-7)
    cert = so.kkt_certificate(qp.P, qp.q, qp.A, qp.b, 0, qp.soc_dims, a.x, a.y, a.s)
    assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, cert
    rp, u, info = so.newton_solve(fg, tol=1e-12)
    assert a.info["pobj"] == pytest.approx(info["objective"], rel=1e-6, abs=1e-7)
    assert a.info["newton_cg_iters"] <= b.info["newton_cg_iters"], (a.info["newton_cg_iters"], b.info["newton_cg_iters"])


@pytest.mark.parametrize("case", oh.LINK_FALLBACKS)
def test_default_solve_beyond_a_cap_of_the_link_plan(case, hip_lib, monkeypatch):
    """One step beyond a cap (51 rounds on a chain, a group of 102 unknowns, 258 linked nodes) the problem keeps the chain
    preconditioner alone: no pair inside, no affected chain, solved, and the objective of the run under SCORE_NO_LINKS=1 to 1e-7."""
    _hip_only(hip_lib)
    qp = oh.model_of(case)[1].qp
    monkeypatch.delenv("SCORE_NO_LINKS", raising=False)
    a, ia, ia_after, pa = _solve(qp, hip_lib)
    monkeypatch.setenv("SCORE_NO_LINKS", "1")
    b, ib, _, _ = _solve(qp, hip_lib)
    monkeypatch.delenv("SCORE_NO_LINKS", raising=False)
    print(f"LINKCAP {case} solve | links {ia} | pobj {a.info['pobj']:.12g} plain {b.info['pobj']:.12g} | iters {a.info['iters']} plain {b.info['iters']}")
    assert ia == oh.device_link_plan(case) and ia_after == ia and ia[0] > 0 and ia[1] == 0 and ia[3] == 0 and pa.size == 0, (ia, pa)
    assert a.solved and b.solved, (a.info, b.info)
    assert a.info["pobj"] == pytest.approx(b.info["pobj"], rel=1e-7, abs=1e-7)
