"""Range leverage and predicted range variances, the python engine (score_amd/leverage.py): the exact identities of the hat
matrix from the dense H, the sums against a plain restatement from the python draws, the share of ranges inside three
standard errors, the uncontrolled ranges of the thinned-beacon graph, the exact pair variances against the marginals'
reference, the argument errors and the header's symbols."""
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from leverage_helpers import THINNED, thinned_twin
from marginals_helpers import graph_a, landmark_names, noisy_truth, pose_names
from samples_helpers import twin
from score_amd.leverage import (LEVERAGE_SYMBOLS, Leverage, dense_leverage, measurement_counts, pair_gradients, pair_ids,
                                predicted_range_variances, range_leverage)
from score_amd.samples import _python_draws, measurement_rows, ordered_jacobian

SEED = 7


def _ranges(prob):
    n_rel, n_rng, _ = measurement_counts(prob)
    return slice(n_rel, n_rel + n_rng)


@pytest.mark.parametrize("key", ["a", "b", "d"])
def test_exact_identities(key):
    tw = twin(key)
    prob = tw.ref.prob
    h = dense_leverage(prob, tw.ref.point)
    rows = np.bincount(measurement_rows(prob)[1])
    n = prob.n
    print(f"{key}: |sum h - n| = {abs(h.sum() - n):.3e}, n = {n}, rows = {rows.sum()}")
    assert h.shape == rows.shape == (sum(measurement_counts(prob)),)
    assert abs(h.sum() - n) <= 1e-9 * n
    assert abs(np.sum(rows - h) - (rows.sum() - n)) <= 1e-9 * n
    assert np.all(h > -1e-12) and np.all(h < rows + 1e-12)


def test_thinned_ranges_have_leverage_one():
    tw = thinned_twin()
    prob = tw.ref.prob
    h = dense_leverage(prob, tw.ref.point)[_ranges(prob)]
    others = np.delete(h, THINNED)
    print(f"thinned: h = {h[THINNED]}, the others in {others.min():.3f} .. {others.max():.3f}, n = {prob.n}")
    assert prob.n == 37 and np.all(np.abs(h[THINNED] - 1.0) <= 1e-9)
    assert others.max() < 0.6


@pytest.mark.parametrize("key", ["a", "d"])
def test_python_sums_restated(key):
    tw = twin(key)
    prob, point = tw.ref.prob, tw.ref.point
    S = 256
    lev, _ = range_leverage(tw.fg, tw.results, n_samples=S, seed=SEED, engine="python")
    delta, _, z, _ = _python_draws(prob, point, SEED, 0, S)
    J = np.asarray(ordered_jacobian(prob, point).todense())
    m = measurement_rows(prob)[1]
    M = sum(measurement_counts(prob))
    Y = delta @ J.T
    t = np.stack([np.bincount(m, weights=Y[s] ** 2, minlength=M) for s in range(S)])
    v = np.stack([np.bincount(m, weights=(z[s] - Y[s]) ** 2, minlength=M) for s in range(S)])
    kinds = np.concatenate([lev.by_kind[k][0] for k in ("relative_pose", "range", "prior")])
    kinds_red = np.concatenate([lev.by_kind[k][1] for k in ("relative_pose", "range", "prior")])
    np.testing.assert_allclose(kinds, t.sum(axis=0) / S, rtol=1e-12, atol=0)
    np.testing.assert_allclose(kinds_red, v.sum(axis=0) / S, rtol=1e-12, atol=0)
    r = _ranges(prob)
    np.testing.assert_array_equal(lev.leverage, kinds[r])
    np.testing.assert_array_equal(lev.redundancy, kinds_red[r])
    # the standard errors are those of the mean of the per-draw terms
    np.testing.assert_allclose(lev.leverage_error, t[:, r].std(axis=0, ddof=1) / np.sqrt(S), rtol=1e-9)
    np.testing.assert_allclose(lev.redundancy_error, v[:, r].std(axis=0, ddof=1) / np.sqrt(S), rtol=1e-9)
    n, rows = prob.n, J.shape[0]
    assert (lev.unknowns, lev.rows, lev.count) == (n, rows, S)
    dev_l, dev_r = (lev.total_leverage - n) / np.sqrt(2.0 * n / S), (lev.total_redundancy - (rows - n)) / np.sqrt(2.0 * (rows - n) / S)
    print(f"{key}: sum lev / S = {lev.total_leverage:.3f} (n = {n}, {dev_l:+.2f} sd), sum red / S = {lev.total_redundancy:.3f} "
          f"(rows - n = {rows - n}, {dev_r:+.2f} sd)")
    assert abs(dev_l) <= 4 and abs(dev_r) <= 4
    # P z and (I - P) z are orthogonal: per draw |y|^2 + |z - y|^2 = |z|^2 over all rows, so the two totals add up to sum |z|^2 / S
    assert abs(lev.total_leverage + lev.total_redundancy - np.sum(z * z) / S) <= 1e-9 * rows


@pytest.mark.parametrize("key", ["a", "b", "d"])
def test_share_of_ranges_inside_three_standard_errors(key):
    tw = twin(key)
    prob = tw.ref.prob
    lev, _ = range_leverage(tw.fg, tw.results, n_samples=256, seed=SEED, engine="python")
    h = dense_leverage(prob, tw.ref.point)[_ranges(prob)]
    inside = np.abs(lev.leverage - h) <= 3 * lev.leverage_error
    inside_r = np.abs(lev.redundancy - (1 - h)) <= 3 * lev.redundancy_error
    print(f"{key}: {inside.mean():.3%} of {len(h)} leverages and {inside_r.mean():.3%} of the redundancies inside 3 standard errors")
    assert inside.mean() >= 0.95 and inside_r.mean() >= 0.95


@pytest.mark.parametrize("seed", [0, 7])
def test_uncontrolled_ranges_of_the_thinned_graph(seed):
    tw = thinned_twin()
    lev, _ = range_leverage(tw.fg, tw.results, n_samples=16, seed=seed, engine="python")
    others = np.delete(lev.redundancy, THINNED)
    print(f"seed {seed}: redundancy of the two {lev.redundancy[THINNED]}, the others >= {others.min():.3f}; their leverage "
          f"estimates {lev.leverage[THINNED]}")
    assert lev.uncontrolled().tolist() == THINNED
    assert np.all(lev.redundancy[THINNED] <= 1e-20) and others.min() > 0.1
    assert isinstance(lev, Leverage) and lev.residuals.shape == lev.studentized.shape == lev.leverage.shape
    keep = np.ones(len(lev.residuals), dtype=bool)
    keep[THINNED] = False
    assert np.all(np.isfinite(lev.studentized[keep]))
    np.testing.assert_array_equal(lev.studentized[keep], lev.residuals[keep] / np.sqrt(lev.redundancy[keep]))


@pytest.mark.parametrize("key", ["a", "d"])
def test_pair_gradient_and_residuals_against_the_ranges_themselves(key):
    """A pair that coincides with a measured range has that range's row of the Jacobian, divided by sqrt(precision), as its
    gradient -- the layout of g from a source that does not know pair_gradients -- and `Leverage.residuals` are
    sqrt(precision) (|p_a - p_b| - measured) restated from the graph's own measurements and the estimate."""
    tw = twin(key)
    prob, point, fg = tw.ref.prob, tw.ref.point, tw.fg
    n_rel, n_rng, _ = measurement_counts(prob)
    d = fg.dimension
    first_row = (d + d * d) * n_rel
    J = np.asarray(tw.J.todense())[first_row:first_row + n_rng]
    names = [str(nm) for nm in prob.a["pose_names"]] + [str(nm) for nm in prob.a["landmark_names"]]
    pairs = [tuple(r.association) for r in fg.range_measurements]
    ids = pair_ids(prob, pairs, "test")
    np.testing.assert_array_equal(ids[:, 0], prob.ra)
    np.testing.assert_array_equal(ids[:, 1], prob.rb)
    assert [names[v] for v in ids[:, 0]] == [p[0] for p in pairs]
    G, dist = pair_gradients(prob, point, ids)
    eps = np.finfo(float).eps
    np.testing.assert_allclose(G.T, J / prob.sw[:, None], rtol=4 * eps, atol=0)
    assert np.array_equal(G.T != 0, J != 0)

    def position(nm):
        v = np.asarray((tw.results.poses if nm in tw.results.poses else tw.results.landmarks)[nm], dtype=float)
        return v[:d, d] if v.ndim == 2 else v

    want = np.array([np.sqrt(r.precision) * (np.linalg.norm(position(a) - position(b)) - r.dist)
                     for r, (a, b) in zip(fg.range_measurements, pairs)])
    lev, _ = range_leverage(fg, tw.results, n_samples=2, seed=SEED, engine="python")
    # (the two distances differ by a few eps of themselves, and the difference with the measured one is scaled by sqrt(precision))
    tol = 8 * eps * np.sqrt([r.precision for r in fg.range_measurements]) * np.maximum(dist, [r.dist for r in fg.range_measurements])
    print(f"{key}: worst |residuals - restated| / tolerance = {float(np.max(np.abs(lev.residuals - want) / tol)):.3e}")
    assert np.any(np.abs(want) > 0.01) and np.all(np.abs(lev.residuals - want) <= tol)
    np.testing.assert_allclose(dist, [np.linalg.norm(position(a) - position(b)) for a, b in pairs], rtol=4 * eps)


def _pairs(fg):
    chains, lms = pose_names(fg), landmark_names(fg)
    pairs = [(chains[0][10], lms[-1]), (chains[0][0], chains[0][7]), (lms[0], chains[0][0]), (chains[0][3], chains[0][20])]
    if len(chains) > 1:
        pairs += [(chains[0][10], chains[1][10]), (chains[1][4], lms[0])]
    return pairs


@pytest.mark.parametrize("key", ["a", "d"])
def test_predicted_range_variances_python(key):
    tw = twin(key)
    ref = tw.ref
    pairs = _pairs(tw.fg)
    assert any(pose_names(tw.fg)[0][0] in p for p in pairs)  # one end at the fixed first pose
    pred, info = predicted_range_variances(tw.fg, tw.results, pairs, engine="python")
    ids = pair_ids(ref.prob, pairs, "test")
    G, dist = pair_gradients(ref.prob, ref.point, ids)
    for c, (a, b) in enumerate(pairs):
        ends = [nm for nm in (a, b) if nm != pose_names(tw.fg)[0][0]]
        _, cols = ref.columns(ends)
        X, _, _ = ref.solve(cols)           # the columns of Sigma over the endpoints' unknowns
        Sigma = X[cols, :]
        g = G[cols, c]
        assert np.count_nonzero(G[:, c]) == np.count_nonzero(g) > 0
        want = g @ Sigma @ g
        assert abs(pred.variance[c] - want) <= 1e-9 * want, (a, b)
        pa = np.asarray((tw.results.poses if a in tw.results.poses else tw.results.landmarks)[a], dtype=float)
        pb = np.asarray((tw.results.poses if b in tw.results.poses else tw.results.landmarks)[b], dtype=float)
        d = tw.fg.dimension
        xa, xb = (pa[:d, d] if pa.ndim == 2 else pa), (pb[:d, d] if pb.ndim == 2 else pb)
        assert abs(pred.distance[c] - np.linalg.norm(xa - xb)) <= 4 * np.finfo(float).eps * pred.distance[c]
    assert pred.pairs == pairs and info["engine"] == "python" and np.all(info["residuals"] < 1e-9)
    prec, measured = 4.0, pred.distance + 0.3
    # (the plain formula rounds 1 + x: an absolute error of eps / 2 (1 + x) under a logarithm of slope <= 1)
    eps = np.finfo(float).eps
    np.testing.assert_allclose(pred.information_gain(prec), 0.5 * np.log(1 + prec * pred.variance), rtol=4 * eps, atol=eps)
    np.testing.assert_allclose(pred.gate(measured, prec), 0.3 ** 2 / (1 / prec + pred.variance), rtol=1e-12)
    # the draws estimate the same variances
    lev, _ = range_leverage(tw.fg, tw.results, n_samples=256, seed=SEED, pairs=pairs, engine="python")
    assert np.all(np.abs(lev.pair_variance - pred.variance) <= 5 * lev.pair_variance_error)


def test_argument_errors_and_symbols():
    fg = graph_a()
    results = noisy_truth(fg)
    some, other = pose_names(fg)[0][3], landmark_names(fg)[0]
    bad = [
        (dict(n_samples=0), "n_samples"), (dict(block_width=0), "block_width"), (dict(block_width=17), "block_width"),
        (dict(engine="cuda"), "engine"), (dict(pairs=[(some, some)]), "to itself"), (dict(pairs=[(some, "nobody")]), "unknown variable"),
        (dict(range_weights=np.ones(len(fg.range_measurements) + 1)), "range_weights"),
    ]
    for kw, words in bad:
        args = dict(engine="python")
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            range_leverage(fg, results, **args)
    bad = [
        (dict(pairs=[(some, some)]), "to itself"), (dict(pairs=[("nobody", other)]), "unknown variable"), (dict(pairs=[]), "no pairs"),
        (dict(block_width=0), "block_width"), (dict(block_width=17), "block_width"),
        (dict(range_weights=np.ones(len(fg.range_measurements) + 1)), "range_weights"),
    ]
    for kw, words in bad:
        args = dict(pairs=[(some, other)], engine="python")
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            predicted_range_variances(fg, results, **args)
    header = open(os.path.join(ROOT, "include", "score_leverage.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(re.findall(r"\b(score_[a-z_0-9]+)\s*\(", header)) == sorted(LEVERAGE_SYMBOLS)


def test_the_samples_header_is_untouched():
    """The leverage entry points came with a header of their own: include/score_samples.h still has the bytes it had before
    them (their SHA-256, so that the test needs no history to compare with).  The digest belongs to the change that added
    score_leverage.h: a later change that edits score_samples.h on purpose updates it here, or removes this test."""
    mine = open(os.path.join(ROOT, "include", "score_samples.h"), "rb").read()
    assert hashlib.sha256(mine).hexdigest() == "f68a37a6856bba0c2f055b2077d18bb70d7cb3444a82091436e129d8bcebc06a"
