"""Batched refinement against a loop of refine_estimate over the same worlds (profiles/r13_refine_batch.json).

  python profiles/scripts/refine_batch.py OUT.json [--lib PATH] [--runs 5] [--worlds 64] [--robots 4] [--poses 1000]

The workload: `worlds` generated Manhattan worlds (generate_manhattan: 4 robots x 1000 poses, the study's shape), relaxed in
lock-step (solve_score_batch), each refined from its relaxation's estimate.  Legs, alternating, `runs` times each after one
warm-up of each:
  batch  refine_estimate_batch(engine="native", max_group=worlds): one group handle, the lock-step loop
  loop   [refine_estimate(engine="native") for every world]: one handle create and one LM loop per world -- the existing code
Wall times are host clocks around calls that end with the estimates read back (a device synchronise); medians of the runs,
with minimum and maximum.  Recorded beside them: LM rounds of the group, per-world iterations, linear solves and PCG iterations
of both legs, the group's setup_ms / solve_ms, and the worst difference between the two legs' estimates."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from score_amd.generate import GeneratedBatch  # noqa: E402
from score_amd.refine import refine_estimate  # noqa: E402
from score_amd.refine_batch import refine_estimate_batch  # noqa: E402
from score_amd.solve_score import solve_score_batch  # noqa: E402


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
    graphs = batch.graphs()
    t0 = time.perf_counter()
    relaxed = solve_score_batch(graphs, "SOCP", lib_path=args.lib)
    relax_ms = 1e3 * (time.perf_counter() - t0)

    def batch_leg():
        t0 = time.perf_counter()
        out = refine_estimate_batch(graphs, relaxed, lib_path=args.lib, max_group=args.worlds)
        wall = 1e3 * (time.perf_counter() - t0)
        infos = [i for _, i in out]
        return out, dict(wall_ms=wall, setup_ms=infos[0]["setup_ms"], solve_ms=infos[0]["solve_ms"], rounds=infos[0]["rounds"],
                         iterations=[i["iterations"] for i in infos], linear_solves=[i["linear_solves"] for i in infos],
                         pcg_iters=[i["pcg_iters"] for i in infos])

    def loop_leg():
        t0 = time.perf_counter()
        out = [refine_estimate(g, r, engine="native", lib_path=args.lib) for g, r in zip(graphs, relaxed)]
        wall = 1e3 * (time.perf_counter() - t0)
        infos = [i for _, i in out]
        return out, dict(wall_ms=wall, setup_ms_sum=float(sum(i["setup_ms"] for i in infos)), solve_ms_sum=float(sum(i["solve_ms"] for i in infos)),
                         iterations=[i["iterations"] for i in infos], linear_solves=[i["linear_solves"] for i in infos],
                         pcg_iters=[i["pcg_iters"] for i in infos])

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
    grad = [i["grad_inf"] / max(1.0, i["cost_final"]) for _, i in out_b]
    med = lambda runs, k: float(np.median([r[k] for r in runs]))  # noqa: E731
    rng_ = lambda runs, k: [float(min(r[k] for r in runs)), float(max(r[k] for r in runs))]  # noqa: E731
    last_b, last_l = b_runs[-1], l_runs[-1]
    for runs in (b_runs, l_runs):  # sums per run; the per-world lists are the same in every run: kept with the last
        for j, r in enumerate(runs):
            for k in ("iterations", "linear_solves", "pcg_iters"):
                r[k + "_sum"] = int(sum(r[k]))
                if j + 1 < len(runs):
                    del r[k]
    rec = dict(
        workload=dict(worlds=args.worlds, robots=args.robots, poses=args.poses, seed=7, relaxation="SOCP, solve_score_batch",
                      relaxation_wall_ms=relax_ms, unknowns_per_world=3 * (args.robots * args.poses - 1) + 2 * len(graphs[0].arrays["landmark_names"])),
        batch=dict(runs=b_runs, wall_ms_median=med(b_runs, "wall_ms"), wall_ms_min_max=rng_(b_runs, "wall_ms"),
                   setup_ms_median=med(b_runs, "setup_ms"), solve_ms_median=med(b_runs, "solve_ms"), rounds=last_b["rounds"],
                   worlds_per_s=1e3 * args.worlds / med(b_runs, "wall_ms")),
        loop=dict(runs=l_runs, wall_ms_median=med(l_runs, "wall_ms"), wall_ms_min_max=rng_(l_runs, "wall_ms"),
                  setup_ms_sum_median=med(l_runs, "setup_ms_sum"), solve_ms_sum_median=med(l_runs, "solve_ms_sum"),
                  worlds_per_s=1e3 * args.worlds / med(l_runs, "wall_ms")),
        loop_over_batch=med(l_runs, "wall_ms") / med(b_runs, "wall_ms"),
        worst_difference_batch_vs_loop=worst, worst_grad_inf_over_max_1_cost=float(max(grad)),
    )
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    short = {k: ({kk: vv for kk, vv in v.items() if kk != "runs"} if isinstance(v, dict) else v) for k, v in rec.items()}
    print(json.dumps(short))
    print("batch: solve_ms / (rounds) =", med(b_runs, "solve_ms") / max(1, last_b["rounds"]), "ms per round;",
          "PCG iterations summed over worlds:", last_b["pcg_iters_sum"], "(loop:", last_l["pcg_iters_sum"], ")")


if __name__ == "__main__":
    main()
