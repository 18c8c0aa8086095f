"""Greedy selection of candidate loop closures (score_refine_select_relative_poses, score_select_block_greedy): what the
selection adds to the relative covariances it is built on, and what the one-workgroup block factorisation costs at its 2-D caps.

  python profiles/scripts/selection_poses.py [--out profiles/selection_poses.json] [--rounds 5]
      20 x 1000 poses (seed 3000) and 4 x 1000 poses (seed 2000), 4 beacons, at refine_estimate's point, one kept handle per
      world: score_refine_select_relative_poses (C = 85 pose - pose candidates = 255 columns, k = 16, kappa = 4 (1 + 1/2 cos c),
      tau = 10 (1 + 1/2 sin c), width 16) against score_refine_relative_covariances over the same pairs, alternating, medians
      of `rounds` calls after a warm-up, the host clock around calls that end in a device synchronise; cross_ms and greedy_ms
      as the call reports them; the joint gain beside the sum of the k best single gains.  Then score_select_block_greedy alone
      at C = 1365, k = 85 in 2-D (N = 4095 columns, K = 255 columns of L) on P = B B'/m (m = 2 N) with precisions graded over
      two decades: medians of `rounds` calls after a warm-up (the host clock: the upload of the 134 MB matrix is inside it,
      and reported apart from a call with k = 1).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from score_amd.manhattan import make_manhattan  # noqa: E402
from score_amd.marginals import _problem_and_point  # noqa: E402
from score_amd.refine import refine_estimate  # noqa: E402
from score_amd.selection_poses import PoseSelectionHandle, block_greedy_from_matrix, column_precisions  # noqa: E402
from score_amd.solve_score import solve_score  # noqa: E402

WORLDS = {"20x1000": dict(n_robots=20, n_poses=1000, n_beacons=4, seed=3000),
          "4x1000": dict(n_robots=4, n_poses=1000, n_beacons=4, seed=2000)}
CANDIDATES, PICKS = 85, 16


def pairs_of(prob, count):
    """Pose - pose pairs spread over the graph: in turn 37 poses on (the same robot, mostly), half the graph away (another
    robot), and two steps on (nearly redundant with the chain)."""
    Np = prob.Np
    c = np.arange(count)
    p = 1 + (c * ((Np - 1) // count) + 11) % (Np - 1)
    step = np.choose(c % 3, [36, Np // 2, 1])
    other = 1 + (p + step) % (Np - 1)
    assert np.all(other != p)
    return np.column_stack([p, other]).astype(np.int32)


def world(name, rounds):
    fg = make_manhattan(**WORLDS[name])
    refined, _ = refine_estimate(fg, solve_score(fg, "SOCP"))
    prob, point = _problem_and_point(fg, refined, None, None)
    pid = pairs_of(prob, CANDIDATES)
    c = np.arange(CANDIDATES)
    kappa, tau = 4.0 * (1.0 + 0.5 * np.cos(c)), 10.0 * (1.0 + 0.5 * np.sin(c))
    ts, tv = [], []
    with PoseSelectionHandle(prob) as h:
        for rnd in range(rounds + 1):  # round 0 warms up
            t = time.perf_counter()
            s = h.select_relative_poses(point, pid, kappa, tau, PICKS)
            ds = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            v = h.relative_covariances(point, pid)
            dv = (time.perf_counter() - t) * 1e3
            assert s["rc"] == 0 and v["rc"] == 0 and np.array_equal(s["covariances"], v["covariances"])
            if rnd:
                ts.append((ds, s["info"])); tv.append((dv, v["info"]))
            print(f"{name} round {rnd}: select_relative_poses {ds:8.2f} ms (cross {s['info']['cross_ms']:.3f}, greedy "
                  f"{s['info']['greedy_ms']:.3f}), relative_covariances {dv:8.2f} ms", flush=True)
    med = lambda xs: float(np.median(xs))  # noqa: E731
    sw = np.sqrt(column_precisions(2, kappa, tau, CANDIDATES)).reshape(CANDIDATES, 3)
    cov = 0.5 * (s["covariances"] + np.swapaxes(s["covariances"], 1, 2))
    single = 0.5 * np.linalg.slogdet(np.eye(3)[None] + sw[:, :, None] * cov * sw[:, None, :])[1]
    return {
        "graph": f"make_manhattan({WORLDS[name]}) at refine_estimate's point", "n": int(prob.n), "rounds": rounds,
        "candidates": CANDIDATES, "columns": 3 * CANDIDATES, "k": PICKS, "block_width": 16,
        "select_relative_poses_ms_median": med([x[0] for x in ts]), "select_relative_poses_ms_all": [float(x[0]) for x in ts],
        "relative_covariances_ms_median": med([x[0] for x in tv]), "relative_covariances_ms_all": [float(x[0]) for x in tv],
        "difference_ms": med([x[0] for x in ts]) - med([x[0] for x in tv]),
        "cross_ms_median": med([x[1]["cross_ms"] for x in ts]), "greedy_ms_median": med([x[1]["greedy_ms"] for x in ts]),
        "solve_ms_median": med([x[1]["solve"]["solve_ms"] for x in ts]), "batches": int(ts[-1][1]["solve"]["batches"]),
        "pcg_iters": int(ts[-1][1]["solve"]["pcg_iters"]),
        "ms_per_block": med([x[1]["solve"]["solve_ms"] for x in ts]) / int(ts[-1][1]["solve"]["batches"]),
        "total_gain": float(s["info"]["total_gain"]), "asymmetry": float(s["info"]["asymmetry"]),
        "sum_of_the_k_largest_single_gains": float(np.sum(np.sort(single)[-PICKS:])),
        "picks_shared_with_the_k_largest_single_gains": int(len(set(s["order"].tolist()) & set(np.argsort(single)[-PICKS:].tolist()))),
    }


def greedy_alone(rounds, n=1365, k=85):
    N = 3 * n
    rng = np.random.default_rng(5)
    B = rng.normal(size=(N, 2 * N))
    P = B @ B.T / (2 * N)
    kappa = 0.5 * 100.0 ** (rng.permutation(n) / (n - 1))
    tau = 0.5 * 100.0 ** (rng.permutation(n) / (n - 1))
    full, one = [], []
    for rnd in range(rounds + 1):
        t = time.perf_counter()
        out = block_greedy_from_matrix(P, kappa, tau, 2, k)
        df = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        block_greedy_from_matrix(P, kappa, tau, 2, 1)
        d1 = (time.perf_counter() - t) * 1e3
        assert out["picked"] == k
        if rnd:
            full.append(df); one.append(d1)
        print(f"block greedy alone round {rnd}: k = {k} {df:8.2f} ms, k = 1 {d1:8.2f} ms", flush=True)
    return {"candidates": n, "columns": N, "k": k, "columns_of_L": 3 * k, "call_ms_median": float(np.median(full)), "call_ms_all": full,
            "call_k1_ms_median": float(np.median(one)), "call_k1_ms_all": one,
            "factorisation_ms": float(np.median(full) - np.median(one)), "total_gain": float(np.sum(out["gains"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selection_poses.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worlds", default=",".join(WORLDS))
    args = ap.parse_args()
    doc = {}
    for name in args.worlds.split(","):
        doc[name] = world(name, args.rounds)
    doc["block_greedy_alone"] = greedy_alone(args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
