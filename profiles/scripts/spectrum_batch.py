"""Batched weakest modes against the single-graph call over the same worlds (profiles/spectrum_batch.json).

  python profiles/scripts/spectrum_batch.py OUT.json [--lib PATH] [--runs 5] [--worlds 64] [--robots 4] [--poses 1000]
                                                     [--kernel-stats STATS.csv]
  python profiles/scripts/spectrum_batch.py --profile-only
      a few group calls and nothing else: the run to put under rocprofv3 --kernel-trace --stats (no counters); its
      kernel-stats CSV goes to the measuring run as --kernel-stats (k_gsp_ritz's and k_gsp_gram's time per launch beside
      their bytes from shapes).

The workload is the README's study: `worlds` generated Manhattan worlds (4 robots x 1000 poses), relaxed in lock-step
(solve_score_batch), refined by refine_estimate_batch; the k = 8 and k = 16 lowest eigenpairs of every world's H at its
refined point.  Legs, alternating in one process, `runs` times each after one warm-up of each; medians with minimum and
maximum:
  a  the group call (RefineBatchHandle.spectrum) on a kept group handle: host clock around it (setup_ms + solve_ms beside it)
  b  SpectrumHandle.spectrum over `worlds` kept single handles, creates excluded: host clock around the loop of calls --
     the way to the same answer without the group call
The creates of both sides are timed once and reported.  Recorded beside them: rounds, iterations per world (min / median /
max), time per round, and the largest |lambda_group - lambda_single| / (rho + rho') over all worlds and modes, rho and rho'
the two calls' own reported residuals."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from score_amd.generate import GeneratedBatch  # noqa: E402
from score_amd.marginals import _problem_and_point  # noqa: E402
from score_amd.refine_batch import RefineBatchHandle, refine_estimate_batch  # noqa: E402
from score_amd.solve_score import solve_score_batch  # noqa: E402
from score_amd.spectrum import SpectrumHandle  # noqa: E402

REL_TOL, MAX_ITERS, SHIFT = 1e-9, 200, 1e-8


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), all=[float(x) for x in xs])


def kernel_time_us(path, needle):
    """Average time of the kernel whose name contains `needle` in a rocprofv3 kernel-stats CSV."""
    with open(path) as f:
        for row in csv.DictReader(f):
            if needle in row.get("Name", ""):
                return dict(name=row["Name"], calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3,
                            min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "spectrum_batch.json"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()
    batch = GeneratedBatch(args.worlds, seed=7, n_robots=args.robots, n_poses=args.poses, lib_path=args.lib)
    graphs = batch.graphs()
    relaxed = solve_score_batch(graphs, "SOCP", lib_path=args.lib)
    refined = [r for r, _ in refine_estimate_batch(graphs, relaxed, lib_path=args.lib, max_group=args.worlds)]
    probs, points = zip(*[_problem_and_point(g, r, None, None) for g, r in zip(graphs, refined)])
    points = list(points)
    if args.profile_only:
        with RefineBatchHandle(probs, args.lib) as h:
            for k in (8, 8, 16):
                rc, _, info = h.spectrum(points, k, REL_TOL, MAX_ITERS, SHIFT)
                print(rc, info, flush=True)
        return

    t0 = time.perf_counter()
    group = RefineBatchHandle(probs, args.lib)
    create_a = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    singles = [SpectrumHandle(p, args.lib) for p in probs]
    create_b = 1e3 * (time.perf_counter() - t0)
    n = int(sum(p.n for p in probs))
    rec = dict(workload=dict(worlds=args.worlds, robots=args.robots, poses=args.poses, seed=7, unknowns_per_world=int(probs[0].n),
                             union_unknowns=n, runs=args.runs, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT),
               creates_ms=dict(group_handle=create_a, single_handles=create_b))
    try:
        for k in (8, 16):
            a_wall, a_own, b_wall = [], [], []
            for i in range(args.runs + 1):  # (the first of each warms up)
                t0 = time.perf_counter()
                rc_a, per_a, info_a = group.spectrum(points, k, REL_TOL, MAX_ITERS, SHIFT)
                wall_a = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                per_b = [h.spectrum(x, k, REL_TOL, MAX_ITERS, SHIFT) for h, x in zip(singles, points)]
                wall_b = 1e3 * (time.perf_counter() - t0)
                print(f"k = {k}, round {i}: a {wall_a:.1f} ms (setup + solve {info_a['setup_ms'] + info_a['solve_ms']:.1f}), rc {rc_a}, "
                      f"rounds {info_a['rounds']} | b {wall_b:.1f} ms, rc {max(r[0] for r in per_b)}", flush=True)
                if i:
                    a_wall.append(wall_a); a_own.append(info_a["setup_ms"] + info_a["solve_ms"]); b_wall.append(wall_b)
            its_a = np.array([m[3] for m in per_a])
            its_b = np.array([r[4]["iterations"] for r in per_b])
            worst = max(float(np.max(np.abs(ma[0] - rb[1]) / (ma[2] + rb[3]))) for ma, rb in zip(per_a, per_b))
            rec[f"k{k}"] = dict(
                a_group_call=dict(wall_ms=stats(a_wall), setup_plus_solve_ms=stats(a_own), setup_ms_last=info_a["setup_ms"],
                                  solve_ms_last=info_a["solve_ms"], rc=int(rc_a), rounds=int(info_a["rounds"]),
                                  ms_per_round=float(info_a["solve_ms"] / info_a["rounds"]), unconverged=int(info_a["unconverged"]),
                                  max_residual=float(info_a["max_residual"]),
                                  iterations_of_a_world=dict(min=int(its_a.min()), median=float(np.median(its_a)), max=int(its_a.max()))),
                b_kept_single_handles=dict(wall_ms=stats(b_wall), ms_per_world=float(np.median(b_wall) / args.worlds),
                                           rc_max=int(max(r[0] for r in per_b)),
                                           iterations_of_a_world=dict(min=int(its_b.min()), median=float(np.median(its_b)), max=int(its_b.max()))),
                b_over_a=float(np.median(b_wall) / np.median(a_wall)),
                ranges_do_not_overlap=bool(np.max(a_wall) < np.min(b_wall)),
                worst_value_difference_over_rho_plus_rho=worst)
    finally:
        group.close()
        for h in singles:
            h.close()
    # bytes of one launch from shapes, every world iterating with all columns live
    wgs = int(sum(-(-(-(-p.n // 32)) // 16) for p in probs))
    rec["bytes_per_launch"] = dict(
        k_gsp_gram=int(6 * 16 * n * 8 + wgs * 2 * 48 * 48 * 8), k_gsp_gram_workgroups=wgs,
        k_gsp_ritz=int(args.worlds * (2 * 48 * 48 * 8 + (16 + 48 * 16) * 8 + 8)))
    if args.kernel_stats:
        for name in ("k_gsp_ritz", "k_gsp_gram", "k_gsp_gram_sum", "k_gsp_combine", "k_gsp_product", "k_gsp_residual", "k_gsp_done",
                     "k_prec"):
            rec.setdefault("kernel_trace", {})[name] = (kernel_time_us(args.kernel_stats, name + "E") or kernel_time_us(args.kernel_stats, name + "(")
                                                        or kernel_time_us(args.kernel_stats, name))
        g = rec["kernel_trace"].get("k_gsp_gram")
        if g:
            g["bytes"] = rec["bytes_per_launch"]["k_gsp_gram"]
            g["TB_per_s_at_max_us"] = g["bytes"] / (g["max_us"] * 1e-6) / 1e12
            g["note"] = ("`bytes` is a launch with every world iterating and all columns live; later launches read fewer columns "
                         "and serve fewer worlds, so the rate belongs to the slowest launch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k not in ("workload",)}))


if __name__ == "__main__":
    main()
