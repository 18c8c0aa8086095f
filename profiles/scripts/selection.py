"""Greedy selection of candidate ranges (score_refine_select_ranges, score_select_greedy): what the selection adds to the
range variances it is built on, and what the one-workgroup factorisation costs at its caps.

  python profiles/scripts/selection.py [--out profiles/selection.json] [--rounds 5]
      20 x 1000 poses (seed 3000) and 4 x 1000 poses (seed 2000), 4 beacons, at refine_estimate's point, one kept handle per
      world: score_refine_select_ranges (C = 256 pose - beacon and pose - pose candidates, k = 32, precision 4 graded by
      1 + 1/2 cos c, width 16) against score_refine_range_variances over the same pairs, alternating, medians of `rounds`
      calls after a warm-up, the host clock around calls that end in a device synchronise; cross_ms and greedy_ms as the
      call reports them.  Then score_select_greedy alone at C = 4096, k = 256 on P = B B'/m (m = 2 C) with precisions graded
      over two decades: medians of `rounds` calls after a warm-up (the host clock: the upload of the 134 MB matrix is inside
      it, and reported apart from a call with k = 1).
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
from score_amd.selection import SelectionHandle, greedy_from_matrix  # noqa: E402
from score_amd.solve_score import solve_score  # noqa: E402

WORLDS = {"20x1000": dict(n_robots=20, n_poses=1000, n_beacons=4, seed=3000),
          "4x1000": dict(n_robots=4, n_poses=1000, n_beacons=4, seed=2000)}
CANDIDATES, PICKS = 256, 32


def pairs_of(prob, count):
    """Half pose - beacon (the beacons in turn), half pose - pose 37 on (profiles/scripts/leverage.py's pairs)."""
    Np, Nl = prob.Np, prob.Nl
    p = 1 + (np.arange(count) * ((Np - 1) // count) + 11) % (Np - 1)
    other = np.where(np.arange(count) % 2 == 0, Np + (np.arange(count) // 2) % Nl, 1 + (p + 36) % (Np - 1))
    return np.column_stack([p, other]).astype(np.int32)


def world(name, rounds):
    fg = make_manhattan(**WORLDS[name])
    refined, _ = refine_estimate(fg, solve_score(fg, "SOCP"))
    prob, point = _problem_and_point(fg, refined, None, None)
    pid = pairs_of(prob, CANDIDATES)
    w = 4.0 * (1.0 + 0.5 * np.cos(np.arange(CANDIDATES)))
    ts, tv = [], []
    with SelectionHandle(prob) as h:
        for rnd in range(rounds + 1):  # round 0 warms up
            t = time.perf_counter()
            s = h.select_ranges(point, pid, w, PICKS)
            ds = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            v = h.range_variances(point, pid)
            dv = (time.perf_counter() - t) * 1e3
            assert s["rc"] == 0 and v["rc"] == 0 and np.array_equal(s["variances"], v["variances"])
            if rnd:
                ts.append((ds, s["info"])); tv.append((dv, v["info"]))
            print(f"{name} round {rnd}: select_ranges {ds:8.2f} ms (cross {s['info']['cross_ms']:.3f}, greedy {s['info']['greedy_ms']:.3f}), "
                  f"range_variances {dv:8.2f} ms", flush=True)
    med = lambda xs: float(np.median(xs))  # noqa: E731
    single = 0.5 * np.log1p(w * s["variances"])
    return {
        "graph": f"make_manhattan({WORLDS[name]}) at refine_estimate's point", "n": int(prob.n), "rounds": rounds,
        "candidates": CANDIDATES, "k": PICKS, "block_width": 16,
        "select_ranges_ms_median": med([x[0] for x in ts]), "select_ranges_ms_all": [float(x[0]) for x in ts],
        "range_variances_ms_median": med([x[0] for x in tv]), "range_variances_ms_all": [float(x[0]) for x in tv],
        "difference_ms": med([x[0] for x in ts]) - med([x[0] for x in tv]),
        "cross_ms_median": med([x[1]["cross_ms"] for x in ts]), "greedy_ms_median": med([x[1]["greedy_ms"] for x in ts]),
        "solve_ms_median": med([x[1]["solve"]["solve_ms"] for x in ts]), "batches": int(ts[-1][1]["solve"]["batches"]),
        "pcg_iters": int(ts[-1][1]["solve"]["pcg_iters"]),
        "ms_per_block": med([x[1]["solve"]["solve_ms"] for x in ts]) / int(ts[-1][1]["solve"]["batches"]),
        "total_gain": float(s["info"]["total_gain"]), "asymmetry": float(s["info"]["asymmetry"]),
        "sum_of_the_k_largest_single_gains": float(np.sum(np.sort(single)[-PICKS:])),
        "picks_shared_with_the_k_largest_single_gains": int(len(set(s["order"].tolist()) & set(np.argsort(single)[-PICKS:].tolist()))),
    }


def greedy_alone(rounds, n=4096, k=256):
    rng = np.random.default_rng(5)
    B = rng.normal(size=(n, 2 * n))
    P = B @ B.T / (2 * n)
    w = 0.5 * 100.0 ** (rng.permutation(n) / (n - 1))
    full, one = [], []
    for rnd in range(rounds + 1):
        t = time.perf_counter()
        out = greedy_from_matrix(P, w, k)
        df = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        greedy_from_matrix(P, w, 1)
        d1 = (time.perf_counter() - t) * 1e3
        assert out["picked"] == k
        if rnd:
            full.append(df); one.append(d1)
        print(f"greedy alone round {rnd}: k = {k} {df:8.2f} ms, k = 1 {d1:8.2f} ms", flush=True)
    return {"candidates": n, "k": k, "call_ms_median": float(np.median(full)), "call_ms_all": full,
            "call_k1_ms_median": float(np.median(one)), "call_k1_ms_all": one,
            "factorisation_ms": float(np.median(full) - np.median(one)), "total_gain": float(np.sum(out["gains"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selection.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worlds", default=",".join(WORLDS))
    args = ap.parse_args()
    doc = {}
    for name in args.worlds.split(","):
        doc[name] = world(name, args.rounds)
    doc["greedy_alone"] = greedy_alone(args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
