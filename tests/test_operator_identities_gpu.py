"""The HIP kernels that dominate every solve -- the KKT product (k_spmv / k_spmv_band, modes KP and KPB) and the chain
preconditioner (k_prec_pre / k_prec / k_prec_wave, the join level, the link correction, k_factor behind them) -- against
SciPy identities built from the problem data alone (operator_helpers.py), in double- and in float-factor mode (the default).
Run with -m gpu on an MI355X; profiles/operator_identities.md records the measured figures beside their bounds."""
import numpy as np
import pytest

import operator_helpers as oh

pytestmark = pytest.mark.gpu

# (id, case, settings, environment): the smallest shapes that reach each code path
CONFIGS = [
    ("A-graph0", "A", dict(use_graph=0), {}),                 # base case, launches queued one by one
    ("A-graph1", "A", dict(use_graph=1), {}),                 # ... replayed from a captured graph
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
    both end in a measured iteration, so z = M^-1 r for the r read back):

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
    dev_views, dev = oh.admm_snapshots(models, settings, hip_lib)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    twin_views, twin = oh.admm_snapshots(models, settings, twin_lib)
    assert sum(len(v.pairs) for v in dev_views) == LINK_PAIRS.get(case, 0)
    failures = []
    for k, (dv, tv) in enumerate(zip(dev_views, twin_views)):
        for s in range(2):
            fd, ft = oh.admm_figures(dv, dev[s], cg_iters, bool(fp32)), oh.admm_figures(tv, twin[s], cg_iters, bool(fp32))
            b2 = oh.i2_bound(dv.K, ft["i2"])
            label = f"{name}[{k}] fp32={fp32} cg={cg_iters} it={5 * (s + 1)}"
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
