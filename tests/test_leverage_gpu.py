"""Range leverage and predicted range variances on the device (score_refine_leverage, score_refine_range_variances,
csrc/score_leverage.hpp) against NumPy's J and noise and the dense Cholesky solve, under the bounds derived in
tests/leverage_helpers.py.

Shapes: graph a (120 measurements: one workgroup, loop closures and a prior), b (599 measurements over three workgroups, 300
lanes on one beacon), d (3-D, 12-row relative poses); 1, 16 or 17 draws (17: a second block with one live draw); 5 pairs with
every call, so that the pairs' lanes follow the measurements' in the last workgroup."""
import functools

import numpy as np
import pytest

from leverage_helpers import SUMS, THINNED, check_range_variances, check_sums, expected_sums, pair_list, thinned_twin
from marginals_helpers import graph_a, noisy_truth, undetermined_graph
from samples_helpers import NOISE_ATOL, twin, weighted_twin
from score_amd.leverage import Leverage, LeverageHandle, measurement_counts, pair_ids, predicted_range_variances, range_leverage

pytestmark = pytest.mark.gpu

SEED = 7
CASES = [("a", 1), ("a", 16), ("a", 17), ("b", 16), ("b", 17), ("d", 1), ("d", 17)]
ALL = SUMS + ("pair_sum", "pair_sq")


@functools.lru_cache(maxsize=None)
def _runs(key, n_samples, hip_lib):
    """One score_refine_leverage call with 5 pairs and the score_refine_samples call of the same draws (every variable
    selected) on one handle: shared by the tests below and left unchanged."""
    tw = twin(key)
    ids = pair_list(tw.ref.prob, 5)
    with LeverageHandle(tw.ref.prob, hip_lib) as h:
        lev = h.leverage(tw.ref.point, ids, n_samples, seed=SEED)
        smp = h.draw(tw.ref.point, tw.ids, n_samples, seed=SEED)
    return ids, lev, smp


@pytest.mark.parametrize("key,n_samples", CASES)
def test_same_draws_as_the_samples(hip_lib, key, n_samples):
    _, lev, smp = _runs(key, n_samples, hip_lib)
    assert lev["rc"] == smp["rc"] == 0 and lev["info"]["batches"] == smp["info"]["batches"] == (n_samples + 15) // 16
    np.testing.assert_array_equal(lev["residuals"], smp["residuals"])
    np.testing.assert_array_equal(lev["iterations"], smp["iterations"])
    np.testing.assert_array_equal(lev["converged"], smp["converged"])
    assert lev["info"]["pcg_iters"] == smp["info"]["pcg_iters"]


@pytest.mark.parametrize("key,n_samples", CASES)
def test_sums(hip_lib, key, n_samples):
    tw = twin(key)
    ids, lev, smp = _runs(key, n_samples, hip_lib)
    z = tw.noise(SEED, 0, n_samples)
    _, want, bound = check_sums(tw, lev, smp["steps"], z, ids, f"{key}, {n_samples} draws")
    assert all(np.any(lev[k] != 0) for k in ALL)
    n_rel, n_rng, n_pri = measurement_counts(tw.ref.prob)
    assert lev["lev_sum"].shape == (n_rel + n_rng + n_pri,) and lev["pair_sum"].shape == (5,)
    if key == "a":  # the prior's entry and a loop closure's, by index
        for m in (n_rel + n_rng, n_rel - 1):
            for k in SUMS:
                assert lev[k][m] > 0 and abs(lev[k][m] - want[k][m]) <= bound[k][m], (k, m)
        assert n_pri == 1 and n_rel - 1 >= 48  # (two chains of 25: 48 odometry steps, then the loop closures)


def test_pairs_across_a_workgroup_edge(hip_lib):
    """b has 599 measurements: 175 pairs put the last six of them into a fourth workgroup of 256 lanes, the rest behind the
    measurements in the third."""
    tw = twin("b")
    ids = pair_list(tw.ref.prob, 175)
    assert sum(measurement_counts(tw.ref.prob)) == 599
    with LeverageHandle(tw.ref.prob, hip_lib) as h:
        lev = h.leverage(tw.ref.point, ids, 3, seed=SEED)
        smp = h.draw(tw.ref.point, tw.ids, 3, seed=SEED)
    check_sums(tw, lev, smp["steps"], tw.noise(SEED, 0, 3), ids, "b, 3 draws, 175 pairs")
    assert np.all(lev["pair_sum"] > 0)
    _, five, _ = _runs("b", 16, hip_lib)
    assert not np.array_equal(lev["pair_sum"][:5], five["pair_sum"])  # (3 draws against 16)


def test_grouping_prefix_and_two_calls(hip_lib):
    tw = twin("a")
    ids, full, _ = _runs("a", 17, hip_lib)
    _, sixteen, _ = _runs("a", 16, hip_lib)
    with LeverageHandle(tw.ref.prob, hip_lib) as h:
        narrow = h.leverage(tw.ref.point, ids, 17, seed=SEED, block_width=4)
        last = h.leverage(tw.ref.point, ids, 1, seed=SEED, first_sample=16)
        again = h.leverage(tw.ref.point, ids, 17, seed=SEED)
    assert narrow["info"]["batches"] == 5 and full["info"]["batches"] == 2
    for k in SUMS:
        np.testing.assert_array_equal(narrow[k], full[k], err_msg=k)
    for k in ALL + ("residuals", "iterations"):
        np.testing.assert_array_equal(again[k], full[k], err_msg=k)
    # draw 16 alone against what the 17-draw and the 16-draw runs imply, within the bound of the 17-draw sums
    z = tw.noise(SEED, 0, 17)
    _, smp = _runs("a", 17, hip_lib)[1:]
    _, bound = expected_sums(tw, smp["steps"], z, ids)
    for k in ALL:
        assert np.all(np.abs((full[k] - sixteen[k]) - last[k]) <= bound[k]), k
    assert np.any(last["lev_sum"] != 0)


def test_unconverged_draws_stay_out_of_the_sums(hip_lib):
    """check_iteration_caps' pattern: under max_iters = max(steps) - 1 the draws beyond the cap report -(cap + 1), the call
    returns 1, and the sums hold the converged draws only."""
    tw = twin("a")
    ids = pair_list(tw.ref.prob, 5)
    with LeverageHandle(tw.ref.prob, hip_lib) as h:
        steps = h.leverage(tw.ref.point, ids, 6, seed=SEED, block_width=4)["iterations"]
        cap = int(steps.max()) - 1
        lev = h.leverage(tw.ref.point, ids, 6, seed=SEED, block_width=4, max_iters=cap)
        smp = h.draw(tw.ref.point, tw.ids, 6, seed=SEED, block_width=4, max_iters=cap)
    keep = lev["converged"]
    print(f"a, 6 draws, cap {cap}: steps {steps.tolist()}, converged {keep.tolist()}")
    assert lev["rc"] == 1 and 0 < np.count_nonzero(keep) < 6 and lev["info"]["unconverged"] == int(np.count_nonzero(~keep))
    np.testing.assert_array_equal(keep, steps <= cap)
    np.testing.assert_array_equal(keep, smp["converged"])
    z = tw.noise(SEED, 0, 6)
    check_sums(tw, lev, smp["steps"][keep], z[keep], ids, f"a, cap {cap}")


@pytest.mark.parametrize("key", ["a", "b", "d"])
def test_range_variances(hip_lib, key):
    tw = twin(key)
    prob = tw.ref.prob
    with LeverageHandle(prob, hip_lib) as h:
        for count in (1, 16, 17):
            ids = pair_list(prob, count)
            out = h.range_variances(tw.ref.point, ids, with_solutions=True)
            assert out["info"]["columns"] == count and out["info"]["batches"] == (count + 15) // 16
            check_range_variances(tw, ids, out, f"{key}, {count} pairs")
            assert np.any(ids == 0) or count == 1  # one end at the fixed first pose
        if key == "b":
            ids = pair_list(prob, 16, on_first_landmark=True)
            check_range_variances(tw, ids, h.range_variances(tw.ref.point, ids, with_solutions=True), "b, 16 pairs on the one beacon")
            narrow = h.range_variances(tw.ref.point, ids, block_width=3, with_solutions=True)
            assert narrow["info"]["batches"] == 6
            check_range_variances(tw, ids, narrow, "b, 16 pairs on the one beacon, width 3")


def test_the_library_refuses_bad_pairs(hip_lib):
    """The entry points' own argument errors (the Python functions catch the same cases before the call): raw ids through the
    handle.  Each comes back as an error with its message, and the handle goes on."""
    tw = twin("a")
    prob = tw.ref.prob
    top = prob.Np + prob.Nl
    bad = [([(3, 3)], "joins a variable to itself"), ([(3, top)], "out of range"), ([(-1, 4)], "out of range")]
    with LeverageHandle(prob, hip_lib) as h:
        for ids, words in bad:
            with pytest.raises(RuntimeError, match="score_refine_leverage: .*" + words):
                h.leverage(tw.ref.point, ids, 2, seed=SEED)
            with pytest.raises(RuntimeError, match="score_refine_range_variances: .*" + words):
                h.range_variances(tw.ref.point, ids)
        with pytest.raises(RuntimeError, match="block_width must be 1..16"):
            h.range_variances(tw.ref.point, [(3, 4)], block_width=17)
        with pytest.raises(RuntimeError, match="n_samples must be >= 1"):
            h.leverage(tw.ref.point, [(3, 4)], 0, seed=SEED)
        none = h.range_variances(tw.ref.point, np.zeros((0, 2), dtype=np.int32))  # (no pairs: nothing to do, no error)
        assert none["rc"] == 0 and none["info"]["columns"] == 0 and none["info"]["batches"] == 0
        ids = pair_list(prob, 3)
        check_range_variances(tw, ids, h.range_variances(tw.ref.point, ids, with_solutions=True), "a, after the refusals")


def test_end_to_end_on_the_thinned_graph(hip_lib):
    tw = thinned_twin()
    lev, info = range_leverage(tw.fg, tw.results, n_samples=16, seed=SEED, lib_path=hip_lib)
    others = np.delete(lev.redundancy, THINNED)
    print(f"thinned, device: redundancy of the two {lev.redundancy[THINNED]}, the others >= {others.min():.3f}, "
          f"worst draw residual {float(np.max(info['residuals'])):.3e}")
    assert isinstance(lev, Leverage) and info["engine"] == "device" and lev.count == 16
    assert lev.uncontrolled().tolist() == THINNED and np.all(lev.redundancy[THINNED] < 1e-6)
    keep = np.ones(len(lev.redundancy), dtype=bool)
    keep[THINNED] = False
    assert np.all(np.isfinite(lev.studentized[keep]))
    pairs = [("A10", "L1"), ("A10", "A3"), ("A0", "L0")]
    pred, pinfo = predicted_range_variances(tw.fg, tw.results, pairs, lib_path=hip_lib)
    assert pred.pairs == pairs and pinfo["engine"] == "device" and pinfo["batches"] == 1
    out = {"rc": 0, "converged": np.ones(3, dtype=bool), "variances": pred.variance, "distances": pred.distance,
           "residuals": pinfo["residuals"], "iterations": pinfo["iterations"]}
    check_range_variances(tw, pair_ids(tw.ref.prob, pairs, "test"), out, "thinned, by name")


def test_singular_information_raises_and_the_library_goes_on(hip_lib):
    fg = undetermined_graph()
    results = noisy_truth(fg)
    with pytest.raises(RuntimeError, match=r"3 of 3 draws did not converge.*information_spectrum\(\.\.\.\)\.undetermined\(\)"):
        range_leverage(fg, results, n_samples=3, seed=SEED, max_iters=64, lib_path=hip_lib)
    tw = twin("a")
    lev, info = range_leverage(tw.fg, tw.results, n_samples=2, seed=SEED, lib_path=hip_lib)
    assert lev.count == 2 and np.all(info["residuals"] < 1e-6)


def test_range_weights(hip_lib):
    fg = graph_a()
    results = noisy_truth(fg)
    w = np.ones(len(fg.range_measurements))
    w[::3] = 0.0
    tw = weighted_twin(fg, results, w)
    prob = tw.ref.prob
    ids = pair_list(prob, 5)
    with LeverageHandle(prob, hip_lib) as h:
        lev = h.leverage(tw.ref.point, ids, 16, seed=SEED)
        smp = h.draw(tw.ref.point, tw.ids, 16, seed=SEED)
    z = tw.noise(SEED, 0, 16)
    _, want, bound = check_sums(tw, lev, smp["steps"], z, ids, "a, a third of the ranges off")
    n_rel, n_rng, _ = measurement_counts(prob)
    off = n_rel + np.flatnonzero(w == 0)
    # J_m = 0: y is an exact zero, so the leverage sums are zeros and the redundancy sums those of z^2 -- the bound left for
    # them is the noise tolerance's alone
    assert np.all(lev["lev_sum"][off] == 0) and np.all(lev["lev_sq"][off] == 0) and np.all(bound["lev_sum"][off] == 0)
    first_row = tw.J.shape[0] - n_rng - 2  # (the ranges' rows: one each, before the prior's two)
    z2 = np.sum(z[:, first_row + np.flatnonzero(w == 0)] ** 2, axis=0)
    assert np.all(np.abs(lev["red_sum"][off] - z2) <= bound["red_sum"][off])
    # (16 draws of 2 |z| NOISE_ATOL with |z| < 8.6, the most Box-Muller gives from 53 bits, and a few eps of z^2)
    assert np.all(bound["red_sum"][off] <= 1.05 * 16 * 2 * 8.6 * NOISE_ATOL)
