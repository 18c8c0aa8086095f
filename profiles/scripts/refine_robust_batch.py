"""Batched robust refinement against a loop of refine_estimate_robust over the same worlds (profiles/r15_refine_robust_batch.json).

  python profiles/scripts/refine_robust_batch.py OUT.json [--lib PATH] [--runs 5] [--worlds 64] [--robots 4] [--poses 1000]

The workload: `worlds` generated Manhattan worlds (generate_manhattan: 4 robots x 1000 poses, the study's shape), 5 % of every
world's ranges corrupted as in profiles/scripts/robust_refine.py -- every second one and every one of 8 m or less measured
long, + U(8, 15) m, the others short, x U(0.3, 0.5) --, relaxed in lock-step (solve_score_robust_batch); every world is refined
from the relaxation's estimate with its weights as prior weights.  Legs, alternating, `runs` times each after one warm-up of each:
  batch  refine_estimate_robust_batch(engine="native", max_group=worlds): one group handle, the lock-step loop with a stage per
         member
  loop   [refine_estimate_robust(engine="native") for every world]: one handle create and one serial loop per world -- the
         existing code
Wall times are host clocks around calls that end with the estimates read back (a device synchronise); medians of the runs, with
minimum and maximum.  Recorded beside them: the group's rounds and the passes in which some member changed stage, outer solves
and LM iterations per world (min / median / max), the group's setup_ms / solve_ms against the sums of the single handles', the
worst difference between the two legs' estimates, and how many planted ranges each leg flagged."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from score_amd.generate import GeneratedBatch  # noqa: E402
from score_amd.native import ArrayGraph  # noqa: E402
from score_amd.refine_robust import refine_estimate_robust  # noqa: E402
from score_amd.refine_robust_batch import refine_estimate_robust_batch  # noqa: E402
from score_amd.robust import solve_score_robust_batch  # noqa: E402


def corrupt(graph, fraction, seed):
    """A copy of ``graph`` with ``fraction`` of its ranges corrupted; (copy, indices, which of them are long)."""
    a = graph.arrays
    rng = np.random.default_rng(seed)
    n = len(a["rng_a"])
    bad = np.sort(rng.choice(n, size=max(2, int(fraction * n)), replace=False))
    long_ = np.zeros(len(bad), dtype=bool)
    dist = np.array(a["rng_dist"], dtype=np.float64)
    for j, i in enumerate(bad):
        if j % 2 == 0 or dist[i] <= 8:
            dist[i] = dist[i] + rng.uniform(8, 15)
            long_[j] = True
        else:
            dist[i] = dist[i] * rng.uniform(0.3, 0.5)
    out = {k: v for k, v in a.items() if k not in ("_owner", "_index", "_cstruct")}
    out["rng_dist"] = dist
    return ArrayGraph(out), bad, long_


def spread(values):
    v = np.asarray(values)
    return dict(min=int(v.min()), median=float(np.median(v)), max=int(v.max()), sum=int(v.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--poses", type=int, default=1000)
    args = ap.parse_args()
    batch = GeneratedBatch(args.worlds, seed=7, n_robots=args.robots, n_poses=args.poses, lib_path=args.lib)
    made = [corrupt(g, 0.05, seed=1000 + i) for i, g in enumerate(batch.graphs())]
    graphs, planted = [m[0] for m in made], [m[1] for m in made]
    t0 = time.perf_counter()
    relaxed = solve_score_robust_batch(graphs, "SOCP", lib_path=args.lib)
    relax_ms = 1e3 * (time.perf_counter() - t0)
    priors = [r.info["robust"]["weights"] for r in relaxed]

    def record(out, wall):
        infos = [i for _, i in out]
        return dict(wall_ms=wall, outer=[i["robust"]["outer_iterations"] for i in infos], lm_iterations=[i["iterations"] for i in infos],
                    linear_solves=[i["linear_solves"] for i in infos], pcg_iters=[i["pcg_iters"] for i in infos],
                    converged=int(sum(i["robust"]["converged"] for i in infos)),
                    planted_flagged=int(sum(np.count_nonzero(i["robust"]["weights"][bad] < 0.5) for i, bad in zip(infos, planted))),
                    flagged=int(sum(len(i["robust"]["outliers"]) for i in infos)))

    def batch_leg():
        t0 = time.perf_counter()
        out = refine_estimate_robust_batch(graphs, relaxed, range_weights=priors, lib_path=args.lib, max_group=args.worlds)
        rec = record(out, 1e3 * (time.perf_counter() - t0))
        info = out[0][1]
        rec.update(setup_ms=info["setup_ms"], solve_ms=info["solve_ms"], rounds=info["rounds"], stage_rounds=info["stage_rounds"])
        return out, rec

    def loop_leg():
        t0 = time.perf_counter()
        out = [refine_estimate_robust(g, r, range_weights=w, engine="native", lib_path=args.lib) for g, r, w in zip(graphs, relaxed, priors)]
        rec = record(out, 1e3 * (time.perf_counter() - t0))
        rec.update(setup_ms_sum=float(sum(i["setup_ms"] for _, i in out)), solve_ms_sum=float(sum(i["solve_ms"] for _, i in out)))
        return out, rec

    b_runs, l_runs = [], []
    for i in range(args.runs + 1):  # (the first of each warms up)
        out_b, rec_b = batch_leg()
        out_l, rec_l = loop_leg()
        if i:
            b_runs.append(rec_b)
            l_runs.append(rec_l)
    worst = 0.0
    for (rb, _), (rl, _) in zip(out_b, out_l):
        worst = max(worst, float(np.max(np.abs(np.asarray(rb.poses.array) - np.asarray(rl.poses.array)))),
                    float(np.max(np.abs(np.asarray(rb.landmarks.array) - np.asarray(rl.landmarks.array)))))
    same_sets = int(sum(np.array_equal(ib["robust"]["outliers"], il["robust"]["outliers"]) for (_, ib), (_, il) in zip(out_b, out_l)))
    med = lambda runs, k: float(np.median([r[k] for r in runs]))  # noqa: E731
    rng_ = lambda runs, k: [float(min(r[k] for r in runs)), float(max(r[k] for r in runs))]  # noqa: E731
    per_world = {}
    for name, runs in (("batch", b_runs), ("loop", l_runs)):  # the per-world lists are the same in every run: kept as spreads of the last
        last = runs[-1]
        per_world[name] = {k: spread(last[k]) for k in ("outer", "lm_iterations", "linear_solves", "pcg_iters")}
        for r in runs:
            for k in ("outer", "lm_iterations", "linear_solves", "pcg_iters"):
                r[k + "_sum"] = int(sum(r.pop(k)))
    last_b = b_runs[-1]
    rec = dict(
        workload=dict(worlds=args.worlds, robots=args.robots, poses=args.poses, seed=7, corrupted_fraction=0.05,
                      planted=int(sum(len(b) for b in planted)), planted_long=int(sum(int(m[2].sum()) for m in made)),
                      ranges=int(sum(len(g.arrays["rng_a"]) for g in graphs)), relaxation="SOCP, solve_score_robust_batch",
                      relaxation_wall_ms=relax_ms, relaxation_flagged=int(sum(len(r.info["robust"]["outliers"]) for r in relaxed))),
        batch=dict(runs=b_runs, wall_ms_median=med(b_runs, "wall_ms"), wall_ms_min_max=rng_(b_runs, "wall_ms"),
                   setup_ms_median=med(b_runs, "setup_ms"), solve_ms_median=med(b_runs, "solve_ms"),
                   solve_ms_min_max=rng_(b_runs, "solve_ms"), rounds=last_b["rounds"], stage_rounds=last_b["stage_rounds"],
                   solve_ms_per_round=med(b_runs, "solve_ms") / max(1, last_b["rounds"]), per_world=per_world["batch"],
                   worlds_per_s=1e3 * args.worlds / med(b_runs, "wall_ms")),
        loop=dict(runs=l_runs, wall_ms_median=med(l_runs, "wall_ms"), wall_ms_min_max=rng_(l_runs, "wall_ms"),
                  setup_ms_sum_median=med(l_runs, "setup_ms_sum"), solve_ms_sum_median=med(l_runs, "solve_ms_sum"),
                  solve_ms_sum_min_max=rng_(l_runs, "solve_ms_sum"), per_world=per_world["loop"],
                  worlds_per_s=1e3 * args.worlds / med(l_runs, "wall_ms")),
        loop_over_batch=med(l_runs, "wall_ms") / med(b_runs, "wall_ms"),
        loop_solve_sum_over_batch_solve=med(l_runs, "solve_ms_sum") / med(b_runs, "solve_ms"),
        worst_difference_batch_vs_loop=worst, worlds_with_equal_outlier_sets=same_sets,
        planted_flagged=dict(batch=last_b["planted_flagged"], loop=l_runs[-1]["planted_flagged"]),
    )
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "runs"} if isinstance(v, dict) else v) for k, v in rec.items()}))


if __name__ == "__main__":
    main()
