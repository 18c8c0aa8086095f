"""The operator identities of operator_helpers.py on the CPU twin, and the checker tested on itself: a planted value error in
the vectors must fail exactly the identity it belongs to.  (The HIP kernels: test_operator_identities_gpu.py.)"""
import numpy as np
import pytest

import operator_helpers as oh

CASES = ["A", "B", "E40", "G"]


def _assert_identities(view, vec, cg_iters, float_factors, label):
    f = oh.admm_figures(view, vec, cg_iters, float_factors)
    floor = oh.i2_bound(view.K, 0.0)
    print(f"OPID twin {label} n={view.qp.n} I1 ratio {f['i1']:.3f} | I2 e {f['i2']:.2e} floor {floor:.2e} | "
          f"I3 eta {f['i3']:.2e} model {f['i3_model']:.2e} bound {f['i3_bound']:.2e} ratio {f['i3'] / f['i3_bound']:.2f}")
    assert f["pairs_ok"], (label, view.pairs, view.expected_pairs)
    assert f["i1"] <= 1.0 and f["i1_exact"], (label, f)
    assert f["i2"] <= floor, (label, f)
    assert f["i3"] <= f["i3_bound"] and f["jacobi"], (label, f)
    return f


@pytest.mark.parametrize("cg_iters", [1, 2, 4])
@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_operator_identities_on_the_twin(case, fp32, cg_iters, twin_lib):
    """I1 (w = K p, row by row: operator_helpers.i1_figures), I2 (the carried product kx = K xt: on the twin alone under the
    floor 8 (L + 4) eps of the device's bound) and I3 (T z = r: normwise backward error under 4 * max(model, 4 eps) with double
    factors, 4 * the float-storage model with float factors; Jacobi off the chains to 4 eps) for every problem of the handle,
    after 5 and after 10 ADMM iterations.  The link pairs of the handle must be the graph's loop closures.
    A: 2 x 60 poses; B: loop closures (8 link pairs); E40: 3-D, block size 4; G: a batch of three."""
    views, snaps = oh.admm_snapshots(oh.case_models(case), dict(cg_iters=cg_iters, fac_fp32=fp32), twin_lib)
    assert sum(len(v.pairs) for v in views) == (8 if case in ("B", "G") else 0)
    for k, view in enumerate(views):
        for s, vec in enumerate(snaps):
            _assert_identities(view, vec, cg_iters, bool(fp32), f"{case}[{k}] fp32={fp32} cg={cg_iters} it={5 * (s + 1)}")


def _verdicts(view, vec, cg_iters, float_factors, e_clean):
    """Which identities hold for these vectors (I2 against the bound a clean run of the same problem sets)."""
    f = oh.admm_figures(view, vec, cg_iters, float_factors)
    return dict(i1=f["i1"] <= 1.0 and f["i1_exact"], i2=f["i2"] <= oh.i2_bound(view.K, e_clean), i3=f["i3"] <= f["i3_bound"] and f["jacobi"])


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("where", ["chain", "link"])
def test_the_checker_catches_a_scaled_entry_of_z(where, fp32, twin_lib):
    """One entry of z scaled by 1 + 1e-6 -- on a chain column of A, on a column of a linked node of B: I3 fails, I1 and I2
    still hold.  The entry is the one with the largest |T_ii z_i| among the candidates (a relative change of 1e-6 must show
    above the float-factor bound of about 1e-7 of the system's scale)."""
    cg = 2
    views, snaps = oh.admm_snapshots(oh.case_models("B" if where == "link" else "A"), dict(cg_iters=cg, fac_fp32=fp32), twin_lib)
    view, vec = views[0], {k: v.copy() for k, v in snaps[1].items()}
    e_clean = oh.i2_figure(view.K, vec["xt"], vec["kx"])
    assert _verdicts(view, vec, cg, bool(fp32), e_clean) == dict(i1=True, i2=True, i3=True)
    bs = int(view.qp.block_size)
    cand = np.nonzero(view.on)[0] if where == "chain" else np.concatenate([np.arange(c, c + bs) for pr in view.pairs for c in pr])
    i = cand[np.argmax(np.abs(view.T.diagonal()[cand] * vec["z"][cand]))]
    vec["z"][i] *= 1.0 + 1e-6
    assert _verdicts(view, vec, cg, bool(fp32), e_clean) == dict(i1=True, i2=True, i3=False)


@pytest.mark.parametrize("cg_iters", [1, 2])
def test_the_checker_catches_a_dropped_entry_of_a_row(cg_iters, twin_lib):
    """One entry of w replaced by its row's sum without the row's last nonzero (what an off-by-one row end computes): I1
    fails, I2 and I3 still hold."""
    views, snaps = oh.admm_snapshots(oh.case_models("A"), dict(cg_iters=cg_iters, fac_fp32=1), twin_lib)
    view, vec = views[0], {k: v.copy() for k, v in snaps[1].items()}
    e_clean = oh.i2_figure(view.K, vec["xt"], vec["kx"])
    assert _verdicts(view, vec, cg_iters, True, e_clean) == dict(i1=True, i2=True, i3=True)
    K = view.K
    last = K.indptr[1:] - 1
    lost = np.abs(K.data[last] * vec["p"][K.indices[last]])
    i = int(np.argmax(lost / np.maximum(np.abs(vec["w"]), 1e-300)))
    assert lost[i] > 0
    row = slice(K.indptr[i], K.indptr[i + 1] - 1)
    vec["w"][i] = float(np.sum(K.data[row].astype(oh.LD) * vec["p"][K.indices[row]].astype(oh.LD)))
    assert _verdicts(view, vec, cg_iters, True, e_clean) == dict(i1=False, i2=True, i3=True)


def test_the_checker_catches_a_dropped_update_of_the_carried_product(twin_lib):
    """kx with one `a w` update dropped on one row: I2 fails, I1 and I3 still hold.  With one PCG iteration per ADMM iteration
    the step length a of the last update is read off xt: xt(10) - xt(9) = a p."""
    from score_amd.solver import ConicSolver

    models = oh.case_models("A")
    views, snaps = oh.admm_snapshots(models, dict(cg_iters=1, fac_fp32=1), twin_lib)
    view, vec = views[0], {k: v.copy() for k, v in snaps[1].items()}
    sol = ConicSolver([m.qp for _, m in models], dict(oh.ADMM_SETTINGS, cg_iters=1, fac_fp32=1), lib_path=twin_lib)
    sol.reset()
    sol.steps(5); sol.steps(4)
    xt9 = sol.debug_get("xt")
    sol.steps(1)
    assert np.array_equal(sol.debug_get("xt"), vec["xt"])  # the same trajectory as the snapshots
    sol.close()
    j = int(np.argmax(np.abs(vec["p"])))
    a = (vec["xt"][j] - xt9[j]) / vec["p"][j]
    np.testing.assert_allclose(vec["xt"] - xt9, a * vec["p"], rtol=0, atol=1e-9 * abs(a) * np.abs(vec["p"]).max())
    e_clean = oh.i2_figure(view.K, vec["xt"], vec["kx"])
    assert _verdicts(view, vec, 1, True, e_clean) == dict(i1=True, i2=True, i3=True)
    i = int(np.argmax(np.abs(vec["w"])))
    vec["kx"][i] -= a * vec["w"][i]
    assert _verdicts(view, vec, 1, True, e_clean) == dict(i1=True, i2=False, i3=True)
