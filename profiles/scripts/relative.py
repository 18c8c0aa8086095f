"""Predicted relative-pose covariances (score_refine_relative_covariances): what a call costs on the headline graph and on a
4 x 1000 world, against the route through the joint marginals.

  python profiles/scripts/relative.py [--out profiles/relative.json] [--rounds 5]
      20 x 1000 poses (seed 3000) and 4 x 1000 poses (seed 2000), 4 beacons, at refine_estimate's point, one kept handle per
      world: score_refine_relative_covariances for 16 and 64 pose - pose pairs (3 columns per pair) against
      score_refine_marginals over the same endpoints (6 columns per pair: what marginal_covariances(joint=True) runs)
      followed by G' Sigma G in NumPy (pair_jacobian's 3 x 6 G on the pair's 6 x 6 part of the joint), alternating, medians
      of `rounds` calls after a warm-up, the host clock around calls that end in a device synchronise; the agreement of P
      between the two routes.
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
from score_amd.marginals import _problem_and_point, _select  # noqa: E402
from score_amd.refine import refine_estimate  # noqa: E402
from score_amd.relative import RelativeHandle, _rotations_and_translations, pair_jacobian  # noqa: E402
from score_amd.solve_score import solve_score  # noqa: E402

WORLDS = {"20x1000": dict(n_robots=20, n_poses=1000, n_beacons=4, seed=3000),
          "4x1000": dict(n_robots=4, n_poses=1000, n_beacons=4, seed=2000)}
PAIRS = (16, 64)


def pairs_of(prob, count):
    """pose - pose: poses spread over the graph against ones 37 on (profiles/scripts/leverage.py's pose - pose pairs)."""
    Np = prob.Np
    p = 1 + (np.arange(count) * ((Np - 1) // count) + 11) % (Np - 1)
    return np.column_stack([p, 1 + (p + 36) % (Np - 1)]).astype(np.int32)


def world(name, rounds):
    fg = make_manhattan(**WORLDS[name])
    refined, _ = refine_estimate(fg, solve_score(fg, "SOCP"))
    prob, point = _problem_and_point(fg, refined, None, None)
    names = list(prob.a["pose_names"])
    out = {"graph": f"make_manhattan({WORLDS[name]}) at refine_estimate's point", "n": int(prob.n), "rounds": rounds, "pairs": {}}
    with RelativeHandle(prob) as h:
        for count in PAIRS:
            pid = pairs_of(prob, count)
            ends = sorted({int(v) for v in pid.ravel()})
            end_ids = np.asarray(ends, dtype=np.int32)
            at = {v: k for k, v in enumerate(ends)}  # where an endpoint's three columns stand in the joint
            cols = _select(prob, [names[v] for v in ends])[3]
            ta, tb = [], []
            for rnd in range(rounds + 1):  # round 0 warms up
                t = time.perf_counter()
                o = h.relative_covariances(point, pid)
                dt = (time.perf_counter() - t) * 1e3
                assert o["rc"] == 0, o["info"]
                t = time.perf_counter()
                rc, A, _, _, _, minfo = h.columns(point, end_ids, block_width=16)
                S_ = 0.5 * (A + A.T)
                R, tr = _rotations_and_translations(prob, point)
                P = np.zeros((count, 3, 3))
                for c, (a, b) in enumerate(pid):  # the pair's 6 x 6 part of the joint and its 3 x 6 Jacobian
                    g = pair_jacobian(R[a], tr[a], R[b], tr[b])[0]
                    rows = np.concatenate([np.arange(3 * at[a], 3 * at[a] + 3), np.arange(3 * at[b], 3 * at[b] + 3)])
                    P[c] = g @ S_[np.ix_(rows, rows)] @ g.T
                dm = (time.perf_counter() - t) * 1e3
                assert rc == 0
                if rnd:
                    ta.append((dt, o["info"])); tb.append((dm, minfo))
                print(f"{name} round {rnd} {count} pairs: relative_covariances {dt:8.2f} ms, marginals + G'SG {dm:8.2f} ms", flush=True)
            mine = 0.5 * (o["covariances"] + np.swapaxes(o["covariances"], 1, 2))
            scale = np.abs(P).max(axis=(1, 2), keepdims=True)
            out["pairs"][str(count)] = {
                "relative_covariances_ms_median": float(np.median([x[0] for x in ta])), "relative_covariances_ms_all": [float(x[0]) for x in ta],
                "solve_ms_median": float(np.median([x[1]["solve_ms"] for x in ta])), "setup_ms_median": float(np.median([x[1]["setup_ms"] for x in ta])),
                "columns": int(ta[-1][1]["columns"]), "batches": ta[-1][1]["batches"], "pcg_iters": ta[-1][1]["pcg_iters"],
                "marginals_ms_median": float(np.median([x[0] for x in tb])), "marginals_ms_all": [float(x[0]) for x in tb],
                "marginals_columns": int(len(cols)), "marginals_batches": tb[-1][1]["batches"], "marginals_pcg_iters": tb[-1][1]["pcg_iters"],
                "max_difference_over_largest_entry_of_the_block": float(np.max(np.abs(mine - P) / scale)),
                "max_asymmetry_over_largest_entry": float(np.max(np.abs(o["covariances"] - np.swapaxes(o["covariances"], 1, 2)) / scale)),
                "trace_min_max": [float(np.trace(mine, axis1=1, axis2=2).min()), float(np.trace(mine, axis1=1, axis2=2).max())],
                "max_residual": float(o["residuals"].max()),
            }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relative.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worlds", default=",".join(WORLDS))
    args = ap.parse_args()
    doc = {}
    for name in args.worlds.split(","):
        doc[name] = world(name, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
