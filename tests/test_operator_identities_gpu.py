"""The HIP kernels that dominate every solve -- the KKT product (k_spmv / k_spmv_band, modes KP and KPB) and the chain
preconditioner (k_prec_pre / k_prec / k_prec_wave, the join level, the link correction, k_factor behind them) -- against
SciPy identities built from the problem data alone (operator_helpers.py), in double- and in float-factor mode (the default).
The second half drives the ADMM loop the way bench.py does -- blocks replayed from a captured graph, penalty updates
(k_kval, k_band_pack, the re-factorisation, k_refresh_u), a PCG count that changes between blocks -- and holds the kernels
between the two operators (k_spmv<MODE_RHS>, k_xupdate, k_cone, k_cone_wave) to a long-double model of one iteration.
Run with -m gpu on an MI355X; profiles/operator_identities.md records the measured figures beside their bounds."""
import numpy as np
import pytest

import operator_helpers as oh

pytestmark = pytest.mark.gpu

# (id, case, settings, environment): the smallest shapes that reach each code path
CONFIGS = [
    ("A-graph0", "A", dict(use_graph=0), {}),                 # base case, launches queued one by one
    ("A-graph1", "A", dict(use_graph=1, check_interval=oh.BLOCK), {}),  # ... two blocks of 16, each replayed from a captured graph
    ("A-norep", "A", {}, dict(SCORE_NO_REPLICATION="1")),     # the general kernels on the full K
    ("B", "B", {}, {}),                                       # loop closures: the link correction
    ("C255", "C255", {}, {}),                                 # LDS-resident chain kernel
    ("C255-radix2", "C255", dict(chain_radix=2), {}),         # streaming chain kernel
    ("C1023", "C1023", {}, {}),                               # the longest chain the LDS kernel holds
    ("C1024", "C1024", {}, {}),                               # segments + join level
    ("D300", "D300", dict(chain_split=1), {}),                # k_prec_wave, 2 parts
    ("D1023", "D1023", dict(chain_split=1), {}),              # k_prec_wave, 4 parts
    ("E40", "E40", {}, {}),                                   # 3-D: block size 4, three replicas
    ("E60-links", "E60", {}, {}),                             # links in 3-D (6 pairs)
    ("E1100", "E1100", {}, {}),                               # 3-D segments
    ("F", "F", {}, {}),                                       # split long rows (L = 834) through the band view
    ("F-noband", "F", {}, dict(SCORE_NO_BAND="1")),           # ... through the CSR stream
    ("G-batch", "G", {}, {}),                                 # lock-step batch; tiles straddle problems
    ("G-graph1", "G", dict(use_graph=1, check_interval=oh.BLOCK), {}),  # ... two blocks of 16, replayed
    ("H-links-join", "H", {}, {}),                            # links on top of the join level
]
LINK_PAIRS = {"B": 8, "E60": 6, "G": 8, "H": 6}


def _hip_only(hip_lib):
    import ctypes

    lib = ctypes.CDLL(hip_lib)
    lib.score_backend.restype = ctypes.c_char_p
    assert lib.score_backend().decode() == "hip-gfx950"


@pytest.mark.parametrize("cg_iters", [1, 2, 4])
@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("config", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_admm_operators_against_scipy_identities(config, fp32, cg_iters, hip_lib, twin_lib, monkeypatch):
    """For every problem of the handle, after 5 and after 10 ADMM iterations (rho = 0.37, sigma = 1e-6, fixed PCG count;
    both end in a measured iteration, so z = M^-1 r for the r read back; the -graph1 configurations: after 16 and after 32,
    each block replayed from a captured graph -- the handle must count two graph launches, every other configuration none):

    I1  w = K p row by row: |w - K p|_i <= cg_iters (L + 4) eps (|K| (|p| + 2|z|))_i (derivation: operator_helpers.i1_figures);
        cg_iters = 1 runs KP alone, 2 and 4 run KPB as well.
    I2  the carried product kx = K xt, e = |kx - K xt|_inf / (|K|_inf |xt|_inf): e_dev <= 8 max(e_twin, (L + 4) eps).  The error
        accumulates over `a w` updates whose scales are gone afterwards, so the twin's own figure on the same problem is the
        yardstick.  The margin 8: the two sides add a row in different orders (band view, split segments, replicas), so their
        roundings differ by small multiples of one another, never by orders; (L + 4) eps is the floor one product alone may
        reach; a wrong or missing entry of K gives 1e-6 or worse, eight orders above either.
    I3  T z = r on the chain columns, eta = |T z - r|_inf / (|T|_inf |z|_inf + |r|_inf), T = chain part of K + link blocks:
        double factors eta <= 4 max(eta_model64, 4 eps), float factors (the default) eta <= 4 eta_model32, the model being the
        banded Cholesky factor (rounded to float32) + SuperLU of operator_helpers.model_solve; off the chains
        z = r / diag(K) to 4 eps.  The twin's figure is asserted under the same bound: a check of the checker.
    The handle's link pairs must be the loop closures of the graph itself.

    (Before k_link_cap set the eliminated entries of a pivot column to exactly 0, I3 with double factors on synth_b -- B and
    problem 1 of the batch G -- stood at 6.8e-15 .. 3.2e-14 against 3.55e-15: profiles/operator_identities.md.)"""
    _hip_only(hip_lib)
    name, case, extra, env = config
    models = oh.case_models(case)
    settings = dict(cg_iters=cg_iters, fac_fp32=fp32, **extra)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    counters = {}
    dev_views, dev = oh.admm_snapshots(models, settings, hip_lib, counters)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    twin_views, twin = oh.admm_snapshots(models, settings, twin_lib)
    assert sum(len(v.pairs) for v in dev_views) == LINK_PAIRS.get(case, 0)
    block = settings.get("check_interval", oh.ADMM_SETTINGS["check_interval"])
    assert counters["graph_launches"] == (2 if name.endswith("-graph1") else 0)
    failures = []
    for k, (dv, tv) in enumerate(zip(dev_views, twin_views)):
        for s in range(2):
            fd, ft = oh.admm_figures(dv, dev[s], cg_iters, bool(fp32)), oh.admm_figures(tv, twin[s], cg_iters, bool(fp32))
            b2 = oh.i2_bound(dv.K, ft["i2"])
            label = f"{name}[{k}] fp32={fp32} cg={cg_iters} it={block * (s + 1)}"
            print(f"OPID {label} n={dv.qp.n} L={int(np.diff(dv.K.indptr).max())} | I1 dev {fd['i1']:.4f} twin {ft['i1']:.4f} | "
                  f"I2 dev {fd['i2']:.3e} twin {ft['i2']:.3e} bound {b2:.3e} | I3 dev {fd['i3']:.3e} bound {fd['i3_bound']:.3e} "
                  f"twin {ft['i3']:.3e} bound {ft['i3_bound']:.3e}")
            checks = {
                "link pairs": fd["pairs_ok"] and ft["pairs_ok"],
                "I1": fd["i1"] <= 1.0 and fd["i1_exact"], "I1 twin": ft["i1"] <= 1.0 and ft["i1_exact"],
                "I2": fd["i2"] <= b2,
                "I3": fd["i3"] <= fd["i3_bound"], "I3 Jacobi": fd["jacobi"],
                "I3 twin": ft["i3"] <= ft["i3_bound"] and ft["jacobi"],
            }
            failures += [(label, nm, fd, ft) for nm, ok in checks.items() if not ok]
    assert not failures, failures


NEWTON_CASES = ["A", "B", "C1023", "C1024", "E40", "E60", "E1100", "H"]


@pytest.mark.parametrize("fac_fp32", [0, None, 2], ids=["double", "default", "float"])
@pytest.mark.parametrize("case", NEWTON_CASES)
def test_newton_preconditioner_against_scipy_identities(case, fac_fp32, hip_lib):
    """I4: after 15 ADMM iterations the Newton set is assembled and factored at the iterate (k_hassemble, k_factor) and
    z = M^-1 (-g) comes from PREC_INIT on it: T_H z = -g on the chain columns with T_H = chain part + link blocks of the H the
    device assembled, the same eta and bounds as I3, Jacobi off the chains to 4 eps, and the link pairs checked against the graph.
    fac_fp32 = 0 keeps the Newton factors in double (the double bound), fac_fp32 = 2 in float (the float bound).  The default
    settings (fac_fp32 = 1) keep them in double only for 2-D chains shorter than 256 poses and stream float copies otherwise
    (HipBackend::init), so the default run is held to the float bound; the double bound is what the first run asserts."""
    _hip_only(hip_lib)
    fg, model = oh.model_of(case)
    H, g, z, pairs = oh.newton_snapshot(model, {} if fac_fp32 is None else dict(fac_fp32=fac_fp32), hip_lib)
    f = oh.newton_figures(fg, model, H, g, z, pairs, fac_fp32 != 0)
    print(f"OPID {case} newton fac_fp32={fac_fp32} n={model.qp.n} | I4 dev {f['i4']:.3e} model {f['i4_model']:.3e} bound {f['i4_bound']:.3e}")
    assert len(pairs) == LINK_PAIRS.get(case, 0)
    assert f["pairs_ok"], pairs
    assert np.abs(g).max() > 0
    assert f["i4"] <= f["i4_bound"], f
    assert f["jacobi"], f


# ---------------------------------------------------------------------------------------------------------------------
# the loop as bench.py drives it: replayed graphs, penalty updates, a changing PCG count
# ---------------------------------------------------------------------------------------------------------------------
UPDATE_CASES = [
    ("A", {}),                          # base
    ("B", {}),                          # the link correction re-derived
    ("C1024", {}),                      # join level
    ("D300", dict(chain_split=1)),      # k_prec_wave
    ("E60", {}),                        # 3-D with links
    ("F", {}),                          # band view: k_band_pack after k_kval, split long rows
    ("G", {}),                          # batch, tiles straddle problems, one penalty per member
]


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("case,extra", UPDATE_CASES, ids=[c for c, _ in UPDATE_CASES])
def test_identities_after_penalty_updates(case, extra, fp32, hip_lib, twin_lib):
    """adaptive_rho=1 with an update at every check (operator_helpers.RHO_SETTINGS: adaptive_rho_interval = check_interval = 16,
    adaptive_rho_tol = 1, max_iters = 48, eps = 1e-30 so that no member is latched, use_graph = 1, cg_iters = 2).

    a  after solve() -- the third update has just run (k_kval, k_band_pack, launch_factor, the float rounding, kx = K xt,
       k_refresh_u: HipBackend::upload_rho) and no iteration has followed it: rho_updates == 3 for every problem; the
       penalties the kernels read (score_debug_get "rho") equal info.rho bit for bit and differ between the members of a
       batch; Kval against K0 + rho K1 from the problem data on the pattern the device streams, entry by entry,
       |Kval - K| <= 3 eps (|K0| + rho |K1|) (operator_helpers.kval_figures; no entry of the reference missing); u against
       rho (bs - s) - y to 3 eps (rho (|bs| + |s|) + |y|); kx against K xt to (L + 4) eps (|K||xt|), row by row.
    b  after steps(16), one replay under the new penalties: I1-I3 of test_admm_operators_against_scipy_identities with K and T
       built at each problem's own penalty; the twin's run of the same sequence is the yardstick of I2 (each side at its
       own penalties, which differ by rounding) and is held to the same bounds.
    c  after reset() on the same handle: the kernels read settings.rho again, and I1-I3 hold at it after steps(16) twice --
       no factor, band value or float copy left over from the updates.
    The handle replays six graphs in all (three in solve(), one in b, two in c)."""
    _hip_only(hip_lib)
    models = oh.case_models(case)
    # (adaptive_rho=1 and use_graph=1 repeat operator_helpers.RHO_SETTINGS: restated only so that this file names its configuration)
    settings = dict(adaptive_rho=1, use_graph=1, fac_fp32=fp32, **extra)
    dev = oh.penalty_update_run(models, settings, hip_lib)
    twin = oh.penalty_update_run(models, settings, twin_lib)
    fails, lines = oh.penalty_update_checks(dev, bool(fp32), f"{case} fp32={fp32}", yard=twin, expect_launches=6)
    tfails, tlines = oh.penalty_update_checks(twin, bool(fp32), f"twin {case} fp32={fp32}", expect_launches=0)
    print("\n".join(lines + tlines))
    assert sum(len(v.pairs) for v in dev["views"]) == LINK_PAIRS.get(case, 0)
    assert not fails and not tfails, (fails, tfails)


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("case", ["A", "G"])
def test_identities_under_a_changing_pcg_count(case, fp32, hip_lib, twin_lib):
    """adaptive_cg=1 with cg_iters = 2, max_cg_iters = 6 and a target (1e-12) the measured reduction exceeds at every check:
    the count goes 2, 3, 4, 6 by the rule of Driver::check, every change destroys the captured graph and the next block
    captures a new one.  After solve(): info.cg_iters == 16 (2 + 3 + 4), which together with the 16 * 6 of the next block
    pins the verdict of every check (operator_helpers.changing_cg_checks).  After steps(16): I1-I3 with cg_iters = 6 in the
    bound of I1, the twin's run as yardstick of I2, and four graph launches -- the replays went on after every re-capture."""
    _hip_only(hip_lib)
    models = oh.case_models(case)
    # (adaptive_cg=1 and use_graph=1 repeat operator_helpers.CG_SETTINGS: restated only so that this file names its configuration)
    settings = dict(adaptive_cg=1, use_graph=1, fac_fp32=fp32)
    dev = oh.changing_cg_run(models, settings, hip_lib)
    twin = oh.changing_cg_run(models, settings, twin_lib)
    fails, lines = oh.changing_cg_checks(dev, bool(fp32), f"{case} fp32={fp32}", yard=twin, expect_launches=4)
    tfails, tlines = oh.changing_cg_checks(twin, bool(fp32), f"twin {case} fp32={fp32}", expect_launches=0)
    print("\n".join(lines + tlines))
    assert not fails and not tfails, (fails, tfails)


ITERATION_CASES = ["A", "E40", "F", "G", "Q", "Q32", "QW"]


@pytest.mark.parametrize("case", ITERATION_CASES)
def test_one_iteration_against_the_long_double_model(case, hip_lib, twin_lib):
    """The kernels between the two operators -- k_spmv<MODE_RHS>, k_xupdate, k_cone, k_cone_wave -- against
    operator_helpers.iteration_model: x0, y0, s0 read, one measuring iteration run (steps(1), nothing deferred), and
    x1, s1, y1, u1 compared with the model's np.longdouble values under the operation counts of its docstring (x, y, u row by
    row, s cone by cone in the 2-norm; zero cones exactly); the right-hand side through r1 + K xt1 with the twin's figure as
    yardstick.  At the start (reset(), steps(3), rho = 0.37) and after the penalty updates of
    test_identities_after_penalty_updates, at each problem's own penalty.  A: base; E40: 4-row cones, three replicas; F:
    long rows; G: cone blocks straddle problems, one penalty per member; Q: a general conic program with cones of 3, 130, 1
    and 70 rows (P = I, A = -I, no chains: k_cone's register path, a 1-row cone, k_cone_wave); Q32: cones of 20, 1, 7 and
    32 rows (k_cone's general path, one lane per cone); QW: cones of 130, 70, 1 and 100 rows.  In each of the three the
    cones with more than one row are, in order, outside the cone (projected onto its boundary: the mean and the scaled
    tail of soc_scales), inside it and in its polar cone at the iteration checked, asserted from w of the model -- so
    k_cone_wave, which takes the cones of more than 32 rows, projects inside and polar cones in Q and all three kinds in QW
    (its 130- and 100-row cones make the lanes stride twice), and k_cone's general path all three in Q32."""
    _hip_only(hip_lib)
    models = oh.iteration_models(case)
    for where, run in (("start", oh.iteration_at_start), ("updated", oh.iteration_after_updates)):
        views, cap = run(models, {}, hip_lib)
        tviews, tcap = run(models, {}, twin_lib)
        fails, lines, ms = oh.iteration_checks(views, cap, f"{case} {where}", yard=(tviews, tcap))
        tfails, tlines, _ = oh.iteration_checks(tviews, tcap, f"twin {case} {where}")
        print("\n".join(lines + tlines))
        assert not fails and not tfails, (fails, tfails)
        if case in oh.GENERAL_DIMS:
            assert [int(b) for b, d in zip(ms[0]["branch"], ms[0]["dims"]) if d > 1] == [3, 1, 2], (where, ms[0]["branch"])
            if case == "QW":  # every one of them is k_cone_wave's
                assert [int(d) for d in ms[0]["dims"] if d > 32] == [130, 70, 100]


@pytest.mark.parametrize("case", ["A", "G"])
def test_a_replayed_block_against_single_steps(case, hip_lib):
    """Two device handles from the same models, double factors: reset(), steps(16) -- one replay, the end-of-PCG update
    deferred 15 times (applied by the next right-hand-side launch and on the fly by k_cone) -- against use_graph = 0,
    reset() and steps(1) sixteen times, every update applied by its own iteration.  The two differ only in the order in
    which r'z and p'w are reduced: x, y, s, xt, kx agree within the double-factor tolerance of
    test_gpu_parity.py::test_iterates_match_cpu_twin, 1e-9 max(1, |v|_inf)."""
    _hip_only(hip_lib)
    replayed, single, launches = oh.replay_and_single_steps(oh.case_models(case), dict(fac_fp32=0, cg_iters=2), hip_lib)
    assert launches == (1, 0)
    worst = {}
    for v in replayed:
        scale = max(1.0, float(np.abs(single[v]).max()))
        worst[v] = float(np.abs(replayed[v] - single[v]).max()) / scale
    print(f"OPID {case} replay against single steps | " + " ".join(f"{v} {worst[v]:.3e}" for v in worst) + " | bound 1.000e-09")
    assert all(w <= 1e-9 for w in worst.values()), worst
