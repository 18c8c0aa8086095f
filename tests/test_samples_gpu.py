"""Posterior samples on the device (score_refine_samples, csrc/score_samples.hpp) against the python engine's noise stream,
J'z from the host Jacobian and the dense Cholesky solve, under the bounds derived in tests/samples_helpers.py: every term is
computed from the reference, the library's own reported residual and the number format.

Shapes: graph a (two chains, loop closures, a prior), b (one beacon ranged from 300 poses: the long contribution list and
the long-row tile), c (1100 poses: the join level), d (3-D); 1, 16 or 17 draws (17: two blocks, the second with one live
column)."""
import functools

import numpy as np
import pytest

from marginals_helpers import check_iteration_caps, graph_a, noisy_truth, undetermined_graph
from samples_helpers import (EPS, check_distribution, check_noise, check_rhs, check_solve, device_draws, dims, fixed_order_moments,
                             twin, weighted_twin)
from score_amd.marginals import _problem_and_point, _select
from score_amd.samples import Samples, SamplesHandle, posterior_samples

pytestmark = pytest.mark.gpu

SEED = 7
CASES = [("a", 1), ("a", 16), ("a", 17), ("b", 1), ("b", 16), ("b", 17), ("c", 16), ("d", 1), ("d", 16), ("d", 17)]
OUTPUTS = ("moments", "means", "steps", "rhs", "noise", "residuals", "iterations")


@functools.lru_cache(maxsize=None)
def _draws(key, n_samples, hip_lib):
    """One call per case, shared by the tests below and left unchanged."""
    return device_draws(twin(key), hip_lib, n_samples, seed=SEED)


@pytest.mark.parametrize("key,n_samples", CASES)
def test_noise_rhs_and_solve(hip_lib, key, n_samples):
    tw, out, label = twin(key), _draws(key, n_samples, hip_lib), f"{key}, {n_samples} draws"
    assert out["info"]["samples"] == n_samples and out["info"]["batches"] == (n_samples + 15) // 16
    z = check_noise(tw, out, SEED, 0, label)
    b_py = check_rhs(tw, out, z, label)
    check_solve(tw, out, b_py, label)
    if key == "b":
        assert tw.longest_column > 128  # the beacon's contribution list: one workgroup per unknown


@pytest.mark.parametrize("key,n_samples", [("a", 17), ("b", 17), ("d", 17), ("d", 1)])
def test_moments_are_the_sums_of_the_steps(hip_lib, key, n_samples):
    tw, out = twin(key), _draws(key, n_samples, hip_lib)
    M, mean, absM, absmean = fixed_order_moments(dims(tw.ref.prob), out["steps"])
    S = n_samples
    print(f"{key}: worst |moments - sums| / ((S + 1) eps sum |terms|) = "
          f"{float(np.max(np.abs(out['moments'] - M) / ((S + 1) * EPS * absM + np.finfo(np.float64).tiny))):.3e}")
    assert out["moments"].shape == M.shape and np.all(np.abs(out["moments"] - M) <= (S + 1) * EPS * absM)
    assert np.all(np.abs(out["means"] - mean) <= (S + 1) * EPS * absmean)
    assert np.any(out["moments"] != 0)


def test_grouping_and_prefix(hip_lib):
    tw = twin("a")
    full = _draws("a", 17, hip_lib)
    with SamplesHandle(tw.ref.prob, hip_lib) as h:
        def run(n, **kw):
            return h.draw(tw.ref.point, tw.ids, n, seed=SEED, with_rhs=True, with_noise=True, **kw)

        narrow, five, last, again = run(17, block_width=4), run(5), run(1, first_sample=16), run(17)
    assert narrow["info"]["batches"] == 5 and full["info"]["batches"] == 2
    np.testing.assert_array_equal(narrow["rhs"], full["rhs"])
    np.testing.assert_array_equal(five["rhs"], full["rhs"][:5])
    np.testing.assert_array_equal(last["rhs"][0], full["rhs"][16])
    np.testing.assert_array_equal(last["noise"][0], full["noise"][16])
    for k in OUTPUTS:
        np.testing.assert_array_equal(again[k], full[k], err_msg=k)
    assert again["rc"] == full["rc"] == 0


@pytest.mark.parametrize("key", ["a", "d"])
def test_distribution(hip_lib, key):
    tw = twin(key)
    smp, info = posterior_samples(tw.fg, tw.results, n_samples=64, seed=0, variables=tw.names, lib_path=hip_lib)
    delta = np.concatenate([smp.steps[nm] for nm in tw.names], axis=1)
    assert info["batches"] == 4 and info["engine"] == "device" and delta.shape == (64, tw.ref.n)
    check_distribution(tw, delta, smp.covariance, f"{key}, device")


def test_range_weights(hip_lib):
    fg = graph_a()
    results = noisy_truth(fg)
    w = np.ones(len(fg.range_measurements))
    w[::3] = 0.0
    tw = weighted_twin(fg, results, w)
    assert np.max(np.abs(tw.ref.H - twin("a").ref.H)) > 1e-3  # the ranges matter
    out = device_draws(tw, hip_lib, 16, seed=SEED)
    z = check_noise(tw, out, SEED, 0, "a, a third of the ranges off")
    b_py = check_rhs(tw, out, z, "a, a third of the ranges off")
    check_solve(tw, out, b_py, "a, a third of the ranges off")


def test_draws_beyond_max_iters_raise(hip_lib):
    tw = twin("a")
    with pytest.raises(RuntimeError, match=r"of 5 draws did not converge.*information_spectrum\(\.\.\.\)\.undetermined\(\)"):
        posterior_samples(tw.fg, tw.results, n_samples=5, seed=SEED, max_iters=2, lib_path=hip_lib)
    # the process goes on: a well-posed call on the same library
    smp, info = posterior_samples(tw.fg, tw.results, n_samples=2, seed=SEED, lib_path=hip_lib)
    assert isinstance(smp, Samples) and smp.count == 2 and np.all(info["residuals"] < 1e-6)


def test_iteration_cap(hip_lib):
    """check_iteration_caps of tests/marginals_helpers.py with draws for columns: under max_iters = max(steps) - 1 (and 16, 17
    where they are below it) the draws within the cap are the full run's bit for bit, the others report -(cap + 1); a draw
    that did not converge is left out of the moments."""
    tw = twin("a")
    kept = {}

    def run(cap):
        out = h.draw(tw.ref.point, tw.ids, 6, seed=SEED, max_iters=cap, block_width=4)
        kept[cap] = out
        return out["rc"], [(out["steps"].T, out["residuals"], out["iterations"], out["converged"])]

    with SamplesHandle(tw.ref.prob, hip_lib) as h:
        top = check_iteration_caps(run, "a, 6 draws, width 4")
    out = kept[top - 1]
    assert out["info"]["unconverged"] == int(np.count_nonzero(~out["converged"])) > 0
    M, mean, absM, absmean = fixed_order_moments(dims(tw.ref.prob), out["steps"][out["converged"]])
    assert np.all(np.abs(out["moments"] - M) <= (6 + 1) * EPS * absM) and np.all(np.abs(out["means"] - mean) <= (6 + 1) * EPS * absmean)


def test_singular_information_is_a_verdict(hip_lib):
    """On undetermined_graph() the call returns 1 with every draw reported as not converged, and posterior_samples raises.
    The draws' own solves cannot say so: b = J'z lies in the range of J'J, the singular system is consistent and its PCG
    converges (measured without the probe: return code 0, 1 iteration per draw, residuals of 1e-18).  The verdict comes
    from the call's probe column H x = xi, xi random, whose iteration does not converge on a singular H."""
    fg = undetermined_graph()  # one range fixes the landmark's distance only: H is singular
    results = noisy_truth(fg)
    prob, point = _problem_and_point(fg, results, None, None)
    ids = _select(prob, None)[1]
    with SamplesHandle(prob, hip_lib) as h:
        out = h.draw(point, ids, 3, seed=SEED, max_iters=64)
    print("singular H:", out["rc"], out["iterations"], out["converged"], out["residuals"], out["info"])
    assert out["rc"] == 1 and not np.any(out["converged"]) and out["info"]["unconverged"] == 3
    with pytest.raises(RuntimeError, match=r"3 of 3 draws.*undetermined\(\)"):
        posterior_samples(fg, results, n_samples=3, seed=SEED, max_iters=64, lib_path=hip_lib)
