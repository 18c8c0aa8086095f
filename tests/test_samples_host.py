"""Posterior samples, the python engine (score_amd/samples.py): the noise stream against the oracle's Philox, the analytic
two-pose case, the independence of a draw from the call it is part of, the distribution of the draws (chi^2 quantiles at
seed 0: no seed is searched for), the moments and the retraction, the argument errors and the header's symbols."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from marginals_helpers import graph_a, landmark_names, noisy_truth, pose_names, two_pose_graph
from oracle import generate_oracle as go
from samples_helpers import check_distribution, dims, everything, fixed_order_moments, twin
from score_amd.samples import GEN_SAMPLE, SAMPLES_SYMBOLS, philox4x32_10, posterior_samples, ps_noise


def test_noise_stream_against_the_oracle():
    rng = np.random.default_rng(5)
    seed = 0x1234_5678_9ABC_DEF1
    m = np.concatenate([rng.integers(0, 5000, 150), [0, 1, 2 ** 20 + 3]])
    s = np.concatenate([rng.integers(0, 300, 100), rng.integers(2 ** 16, 2 ** 31, 50), [0, 2 ** 16, 2 ** 32 - 1]])
    q = np.concatenate([rng.integers(0, 12, 150), [0, 1, 11]])
    assert GEN_SAMPLE not in (go.START, go.TURN, go.ODOM_A, go.ODOM_B, go.BEACON, go.HIT_RB, go.NOISE_RB, go.HIT_RR, go.NOISE_RR)
    assert GEN_SAMPLE > 12  # (the generator's purposes end at 12: csrc/score_generate.hpp)
    assert np.any(q & 1) and np.any(~(q & 1).astype(bool)) and np.any(s >= 2 ** 16)
    ints = philox4x32_10(seed, np.full(len(m), GEN_SAMPLE), m, s, q >> 1)
    mine = ps_noise(seed, m, s, q)
    for k in range(len(m)):
        p = go.philox4x32_10(seed, GEN_SAMPLE, int(m[k]), int(s[k]), int(q[k]) >> 1)
        assert tuple(int(w[k]) for w in ints) == p  # bit for bit
        want = go.normal2(p)[int(q[k]) & 1]
        # the same expressions on the same bits: what differs is the last place of log, sqrt and cos / sin in the two
        # libraries -- r (1 + 3 eps) (c + eps) with r <= sqrt(2 * 53 log 2) < 8.6 and |c| <= 1
        assert abs(mine[k] - want) <= 8.6 * 4 * np.finfo(np.float64).eps
    assert ps_noise(seed, 3, 4, 5).shape == ()


def test_analytic_two_pose_graph():
    kappa, tau = 7.0, 3.0
    fg = two_pose_graph(kappa, tau)
    results = noisy_truth(fg)
    smp, info = posterior_samples(fg, results, n_samples=9, seed=3, engine="python")
    z, steps = info["noise"], smp.steps["A1"]
    assert z.shape == (9, 6) and steps.shape == (9, 3) and smp.order == ["A1"]
    # H = diag(2 tau, kappa, kappa); J'z by hand: the translation rows reach (x, y) with sqrt(kappa), the four rotation rows
    # reach theta with sqrt(tau) d(R(theta))/dtheta = sqrt(tau) (-s, -c, c, -s)
    T = np.asarray(results.poses["A1"])
    th = np.arctan2(T[1, 0], T[0, 0])
    c, s = np.cos(th), np.sin(th)
    b_th = np.sqrt(tau) * (-s * z[:, 2] - c * z[:, 3] + c * z[:, 4] - s * z[:, 5])
    want = np.column_stack([b_th / (2 * tau), np.sqrt(kappa) * z[:, 0] / kappa, np.sqrt(kappa) * z[:, 1] / kappa])
    np.testing.assert_allclose(steps, want, rtol=1e-13, atol=0)


def test_prefix_and_grouping():
    tw = twin("a")
    few, _ = posterior_samples(tw.fg, tw.results, n_samples=5, seed=11, variables=tw.names, engine="python")
    many, _ = posterior_samples(tw.fg, tw.results, n_samples=17, seed=11, variables=tw.names, engine="python")
    two, _ = posterior_samples(tw.fg, tw.results, n_samples=2, first_sample=3, seed=11, variables=tw.names, engine="python")
    narrow, _ = posterior_samples(tw.fg, tw.results, n_samples=5, seed=11, variables=tw.names, engine="python", block_width=3)
    for nm in tw.names:
        np.testing.assert_array_equal(few.steps[nm], many.steps[nm][:5])
        np.testing.assert_array_equal(two.steps[nm], many.steps[nm][3:5])
        np.testing.assert_array_equal(narrow.steps[nm], few.steps[nm])
    other, _ = posterior_samples(tw.fg, tw.results, n_samples=5, seed=12, variables=tw.names, engine="python")
    assert not np.array_equal(other.steps[tw.names[0]], few.steps[tw.names[0]])


@pytest.mark.parametrize("key", ["a", "d"])
def test_distribution(key):
    tw = twin(key)
    smp, info = posterior_samples(tw.fg, tw.results, n_samples=64, seed=0, variables=tw.names, engine="python")
    delta = np.concatenate([smp.steps[nm] for nm in tw.names], axis=1)
    assert delta.shape == (64, tw.ref.n) and smp.standard_error == np.sqrt(2.0 / 64)
    check_distribution(tw, delta, smp.covariance, f"{key}, python engine")


@pytest.mark.parametrize("key", ["a", "d"])
def test_moments_are_the_sums_of_the_steps(key):
    tw = twin(key)
    smp, _ = posterior_samples(tw.fg, tw.results, n_samples=7, seed=2, variables=tw.names, engine="python")
    delta = np.concatenate([smp.steps[nm] for nm in tw.names], axis=1)
    M, mean, _, _ = fixed_order_moments(dims(tw.ref.prob), delta)
    at = 0
    for nm in tw.names:
        k = smp.steps[nm].shape[1]
        np.testing.assert_array_equal(smp.covariance(nm), M[at:at + k * k].reshape(k, k) / 7)
        at += k * k
    assert at == len(M)
    np.testing.assert_array_equal(np.concatenate([smp.mean(nm) for nm in tw.names]), mean / 7)
    # a variable that is not selected has its covariance too
    only, _ = posterior_samples(tw.fg, tw.results, n_samples=7, seed=2, variables=[tw.names[-1]], engine="python")
    assert list(only.steps) == [tw.names[-1]]
    np.testing.assert_array_equal(only.covariance(tw.names[0]), smp.covariance(tw.names[0]))


def test_results_retract_as_the_refinement_does():
    tw = twin("d")
    prob = tw.ref.prob
    smp, _ = posterior_samples(tw.fg, tw.results, n_samples=3, seed=4, variables=tw.names, engine="python")
    poses = [nm for ch in pose_names(tw.fg) for nm in ch]
    for s in range(3):
        step = np.concatenate([smp.steps[nm][s] for nm in tw.names])
        R, t, lm = prob.retract(tw.ref.point, step)
        got = smp.results(s)
        assert sorted(got) == sorted(tw.names)
        for p, nm in enumerate(poses[1:], start=1):
            assert got[nm].shape == (4, 4)
            np.testing.assert_allclose(got[nm][:3, :3], R[p], rtol=0, atol=4 * np.finfo(np.float64).eps)
            np.testing.assert_array_equal(got[nm][:3, 3], t[p])
            np.testing.assert_array_equal(got[nm][3], [0, 0, 0, 1])
        for l, nm in enumerate(landmark_names(tw.fg)):
            np.testing.assert_array_equal(got[nm], lm[l])
    # 2-D: theta + dtheta, t + v
    ta = twin("a")
    smp2, _ = posterior_samples(ta.fg, ta.results, n_samples=1, seed=4, variables=[ta.names[0]], engine="python")
    T0, T1, st = np.asarray(ta.results.poses[ta.names[0]]), smp2.results(0)[ta.names[0]], smp2.steps[ta.names[0]][0]
    th = np.arctan2(T0[1, 0], T0[0, 0]) + st[0]
    np.testing.assert_allclose(T1, [[np.cos(th), -np.sin(th), T0[0, 2] + st[1]], [np.sin(th), np.cos(th), T0[1, 2] + st[2]], [0, 0, 1]],
                               rtol=0, atol=1e-15)


def test_argument_errors_and_symbols():
    fg = graph_a()
    results = noisy_truth(fg)
    first = pose_names(fg)[0][0]
    some = pose_names(fg)[0][3]
    bad = [
        (dict(n_samples=0), "n_samples"), (dict(block_width=0), "block_width"), (dict(block_width=17), "block_width"),
        (dict(engine="cuda"), "engine"), (dict(variables=[first]), "fixed first pose"), (dict(variables=[some, some]), "twice"),
        (dict(variables=["nobody"]), "unknown variable"), (dict(range_weights=np.ones(len(fg.range_measurements) + 1)), "range_weights"),
    ]
    for kw, words in bad:
        args = dict(engine="python")
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            posterior_samples(fg, results, **args)
    header = open(os.path.join(ROOT, "include", "score_samples.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(re.findall(r"\b(score_[a-z_0-9]+)\s*\(", header)) == sorted(SAMPLES_SYMBOLS)
    assert everything(fg)[0] == pose_names(fg)[0][1]
