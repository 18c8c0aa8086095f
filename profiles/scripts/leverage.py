"""Range leverage and predicted range variances (score_refine_leverage, score_refine_range_variances): what a call costs on
the headline graph and on a 4 x 1000 world.

  python profiles/scripts/leverage.py [--out profiles/leverage.json] [--rounds 5]
      20 x 1000 poses (seed 3000) and 4 x 1000 poses (seed 2000), 4 beacons, at refine_estimate's point, one handle per world:
      score_refine_leverage at 64 / 256 draws against score_refine_samples with the same draws (default variables) on the
        same handle, alternating, medians of `rounds` calls after a warm-up; the difference is what k_lv_measure costs beyond
        the moments and the step selection it replaces; the kernel's bytes per launch from shapes;
      score_refine_range_variances for 16 and 64 pairs (pose - beacon, pose - pose) against score_refine_marginals over the
        same endpoints (what marginal_covariances(joint=True) runs) followed by g' Sigma g in NumPy;
      the worst |device - expected| / bound of the sums on the tests' cases (tests/leverage_helpers.py).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from score_amd.leverage import LeverageHandle, measurement_counts, pair_gradients  # noqa: E402
from score_amd.manhattan import make_manhattan  # noqa: E402
from score_amd.marginals import _problem_and_point, _select  # noqa: E402
from score_amd.refine import refine_estimate  # noqa: E402
from score_amd.solve_score import solve_score  # noqa: E402

WORLDS = {"20x1000": dict(n_robots=20, n_poses=1000, n_beacons=4, seed=3000),
          "4x1000": dict(n_robots=4, n_poses=1000, n_beacons=4, seed=2000)}
COUNTS = (64, 256)
PAIRS = (16, 64)


def launch_bytes(prob):
    """Bytes one launch of k_lv_measure<2> moves for a block of 16 converged draws, from shapes: the graph's arrays as
    k_ps_blocks reads them, delta at every measurement's local unknowns (per lane; a wave on one beacon reads its two doubles
    once -- `unique` counts every unknown once per draw and measurement kind), the four sums in and out."""
    n_rel, n_rng, n_pri = measurement_counts(prob)
    M = n_rel + n_rng + n_pri
    graph = n_rel * (2 * 4 + (2 + 4 + 2) * 8 + 2 * 3 * 8) + n_rng * (2 * 4 + 2 * 8 + 2 * 2 * 8) + n_pri * (4 + 3 * 8 + 2 * 8)
    per_lane = 16 * 8 * (6 * n_rel + 4 * n_rng + 2 * n_pri)
    pose_ends = int(np.count_nonzero(prob.ra < prob.Np) + np.count_nonzero(prob.rb < prob.Np))
    unique = 16 * 8 * (6 * n_rel + 2 * pose_ends + 2 * prob.Nl + 2 * n_pri)
    sums = 2 * 4 * M * 8
    return {"measurements": int(M), "graph": int(graph), "delta_per_lane": int(per_lane), "delta_unique": int(unique), "sums": int(sums),
            "k_lv_measure_per_lane": int(graph + per_lane + sums), "k_lv_measure_unique": int(graph + unique + sums)}


def pairs_of(prob, count, kind):
    """pose - beacon (every fifth-ish pose against the beacons in turn) or pose - pose (the same poses against ones 37 on)."""
    Np, Nl = prob.Np, prob.Nl
    p = 1 + (np.arange(count) * ((Np - 1) // count) + 11) % (Np - 1)
    other = Np + np.arange(count) % Nl if kind == "pose-beacon" else 1 + (p + 36) % (Np - 1)
    return np.column_stack([p, other]).astype(np.int32)


def world(name, rounds):
    fg = make_manhattan(**WORLDS[name])
    refined, _ = refine_estimate(fg, solve_score(fg, "SOCP"))
    prob, point = _problem_and_point(fg, refined, None, None)
    ids = _select(prob, None)[1]
    names = list(prob.a["pose_names"]) + list(prob.a["landmark_names"])
    out = {"graph": f"make_manhattan({WORLDS[name]}) at refine_estimate's point", "n": int(prob.n), "rounds": rounds,
           "bytes_per_launch_16_draws": launch_bytes(prob), "n_samples": {}, "pairs": {}}
    with LeverageHandle(prob) as h:
        rec = {(S, who): [] for S in COUNTS for who in ("leverage", "samples")}
        for rnd in range(rounds + 1):  # round 0 warms up
            for S in COUNTS:
                for who in ("leverage", "samples"):
                    t = time.perf_counter()
                    o = h.leverage(point, None, S, seed=0) if who == "leverage" else h.draw(point, ids, S, seed=0)
                    dt = (time.perf_counter() - t) * 1e3
                    assert o["rc"] == 0, o["info"]
                    if rnd:
                        rec[(S, who)].append((dt, o["info"]))
                    print(f"{name} round {rnd} {S:3d} draws {who:8s}: {dt:9.2f} ms {o['info']}", flush=True)
        for S in COUNTS:
            doc = {}
            for who in ("leverage", "samples"):
                r = rec[(S, who)]
                doc[who] = {"call_ms_median": float(np.median([x[0] for x in r])), "call_ms_all": [float(x[0]) for x in r],
                            "solve_ms_median": float(np.median([x[1]["solve_ms"] for x in r])), "batches": r[-1][1]["batches"],
                            "pcg_iters": r[-1][1]["pcg_iters"]}
            doc["call_ms_difference"] = doc["leverage"]["call_ms_median"] - doc["samples"]["call_ms_median"]
            doc["solve_ms_difference_per_block"] = (doc["leverage"]["solve_ms_median"] - doc["samples"]["solve_ms_median"]) / doc["leverage"]["batches"]
            out["n_samples"][str(S)] = doc
        lev = h.leverage(point, None, 256, seed=0)
        n_rel, n_rng, _ = measurement_counts(prob)
        red = lev["red_sum"][n_rel:n_rel + n_rng] / 256
        out["redundancy_of_the_ranges_256_draws"] = {"min": float(red.min()), "median": float(np.median(red)), "max": float(red.max()),
                                                     "total_leverage": float(lev["lev_sum"].sum() / 256), "unknowns": int(prob.n)}
        for count in PAIRS:
            for kind in ("pose-beacon", "pose-pose"):
                pid = pairs_of(prob, count, kind)
                ends = sorted({int(v) for v in pid.ravel()})
                end_ids = np.asarray(ends, dtype=np.int32)
                cols = _select(prob, [names[v] for v in ends])[3]
                G, _ = pair_gradients(prob, point, pid)
                ta, tb = [], []
                for rnd in range(rounds + 1):
                    t = time.perf_counter()
                    o = h.range_variances(point, pid)
                    dt = (time.perf_counter() - t) * 1e3
                    assert o["rc"] == 0, o["info"]
                    t = time.perf_counter()
                    rc, A, _, _, _, minfo = h.columns(point, end_ids, block_width=16)
                    S_ = 0.5 * (A + A.T)
                    var = np.einsum("ic,ij,jc->c", G[cols], S_, G[cols])
                    dm = (time.perf_counter() - t) * 1e3
                    assert rc == 0
                    if rnd:
                        ta.append((dt, o["info"])); tb.append((dm, minfo))
                    print(f"{name} round {rnd} {count} {kind} pairs: range_variances {dt:8.2f} ms, marginals + g'Sg {dm:8.2f} ms", flush=True)
                out["pairs"][f"{count} {kind}"] = {
                    "range_variances_ms_median": float(np.median([x[0] for x in ta])), "range_variances_ms_all": [float(x[0]) for x in ta],
                    "columns": int(count), "batches": ta[-1][1]["batches"], "pcg_iters": ta[-1][1]["pcg_iters"],
                    "marginals_ms_median": float(np.median([x[0] for x in tb])), "marginals_ms_all": [float(x[0]) for x in tb],
                    "marginals_columns": int(len(cols)), "marginals_batches": tb[-1][1]["batches"], "marginals_pcg_iters": tb[-1][1]["pcg_iters"],
                    "max_relative_difference": float(np.max(np.abs(o["variances"] - var) / var)),
                    "variance_min_max": [float(o["variances"].min()), float(o["variances"].max())],
                }
    return out


def sums_on_the_tests_cases():
    from leverage_helpers import check_sums, pair_list
    from samples_helpers import twin

    doc = {}
    for key, S in [("a", 1), ("a", 16), ("a", 17), ("b", 16), ("b", 17), ("d", 1), ("d", 17)]:
        tw = twin(key)
        pid = pair_list(tw.ref.prob, 5)
        with LeverageHandle(tw.ref.prob) as h:
            lev = h.leverage(tw.ref.point, pid, S, seed=7)
            smp = h.draw(tw.ref.point, tw.ids, S, seed=7)
        doc[f"{key}, {S} draws"] = check_sums(tw, lev, smp["steps"], tw.noise(7, 0, S), pid, f"{key}, {S} draws")[0]
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leverage.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worlds", default=",".join(WORLDS))
    args = ap.parse_args()
    doc = {"sums_worst_error_over_bound": sums_on_the_tests_cases()}
    for name in args.worlds.split(","):
        doc[name] = world(name, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
