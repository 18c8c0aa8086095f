"""Batched marginal covariances against the single-graph call over the same worlds (profiles/r14_marginals_batch.json).

  python profiles/scripts/marginals_batch.py OUT.json [--lib PATH] [--runs 5] [--worlds 64] [--robots 4] [--poses 1000]
                                                      [--kernel-stats STATS.csv]
  python profiles/scripts/marginals_batch.py --profile-only
      a few group calls and nothing else: the run to put under rocprofv3 --kernel-trace --stats; its kernel-stats CSV goes
      to the measuring run as --kernel-stats (k_gbm_product<16>'s time over its algorithmic bytes).

The workload is the README's study: `worlds` generated Manhattan worlds (4 robots x 1000 poses), relaxed in lock-step
(solve_score_batch), refined by refine_estimate_batch; the default variables of every world (the generator's 6 beacons + 4
last poses = 24 columns: one pass of 16 slots, one of 8).  Legs, alternating in one process, `runs` times each after one
warm-up of each; medians with minimum and maximum:
  a  the group call (RefineBatchHandle.marginals) on a kept group handle: setup_ms + solve_ms, and the host clock around it
  b  MarginalsHandle.columns over `worlds` kept single handles, creates excluded: host clock around the loop of calls
  c  [marginal_covariances(...) for every world], end to end: what a user runs without the group call
  d  refine_estimate_batch(marginals=True) end to end, against refine_estimate_batch followed by c
Recorded beside them: passes and iterations, the largest relative difference of a diagonal entry of H^-1 between a and b --
next to the same figure between block_width 16 and 0 on one single handle --, and the mean NEES of the beacons and last poses
over the worlds beside their degrees of freedom (reported, not gated: range noise is clamped at 0, so it is not exactly
Gaussian)."""
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
from score_amd.marginals import MarginalsHandle, _problem_and_point, _select, marginal_covariances  # noqa: E402
from score_amd.refine_batch import RefineBatchHandle, refine_estimate_batch  # noqa: E402
from score_amd.solve_score import solve_score_batch  # noqa: E402


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
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "r14_marginals_batch.json"))
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
    sels = [_select(p, None) for p in probs]
    ids = [s[1] for s in sels]
    if args.profile_only:
        with RefineBatchHandle(probs, args.lib) as h:
            for _ in range(3):
                rc, _, info = h.marginals(list(points), ids)
                print(rc, info, flush=True)
        return

    def leg_c():
        t0 = time.perf_counter()
        out = [marginal_covariances(g, r, lib_path=args.lib) for g, r in zip(graphs, refined)]
        return 1e3 * (time.perf_counter() - t0), out

    a_runs, a_wall, b_runs, c_runs, d_runs, d_two = [], [], [], [], [], []
    with RefineBatchHandle(probs, args.lib) as group:
        singles = [MarginalsHandle(p, args.lib) for p in probs]
        try:
            for i in range(args.runs + 1):  # (the first of each warms up)
                t0 = time.perf_counter()
                rc_a, cols_a, info_a = group.marginals(list(points), ids)
                wall_a = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                cols_b = [h.columns(x, v) for h, x, v in zip(singles, points, ids)]
                wall_b = 1e3 * (time.perf_counter() - t0)
                wall_c, out_c = leg_c()
                t0 = time.perf_counter()
                out_d = refine_estimate_batch(graphs, relaxed, lib_path=args.lib, max_group=args.worlds, marginals=True)
                wall_d = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                two = refine_estimate_batch(graphs, relaxed, lib_path=args.lib, max_group=args.worlds)
                _ = [marginal_covariances(g, r, lib_path=args.lib) for g, (r, _) in zip(graphs, two)]
                wall_two = 1e3 * (time.perf_counter() - t0)
                assert rc_a == 0 and all(c[0] == 0 for c in cols_b)
                print(f"round {i}: a {info_a['setup_ms'] + info_a['solve_ms']:.1f} ms (wall {wall_a:.1f}) | b {wall_b:.1f} | c {wall_c:.1f} | "
                      f"d {wall_d:.1f} vs {wall_two:.1f}", flush=True)
                if i:
                    a_runs.append(info_a["setup_ms"] + info_a["solve_ms"]); a_wall.append(wall_a); b_runs.append(wall_b)
                    c_runs.append(wall_c); d_runs.append(wall_d); d_two.append(wall_two)
            # one single handle: block_width 16 against the single-right-hand-side PCG per column
            w16, w0 = singles[0].columns(points[0], ids[0]), singles[0].columns(points[0], ids[0], block_width=0)
        finally:
            for h in singles:
                h.close()
    rel = lambda A, B: float(np.max(np.abs(np.diag(A) - np.diag(B)) / np.abs(np.diag(B))))  # noqa: E731
    diag_ab = max(rel(ca[0], cb[1]) for ca, cb in zip(cols_a, cols_b))
    steps_a = np.concatenate([c[2] for c in cols_a])
    steps_b = np.concatenate([c[3] for c in cols_b])
    # NEES over the worlds, from leg d's estimates and covariances
    nees = {"beacons": [], "last_poses": []}
    for i, (res, info) in enumerate(out_d):
        for nm, (val, dof) in batch.nees(i, res, info["marginals"][0]).items():
            nees["beacons" if dof == 2 else "last_poses"].append(val)
    n, nnz = int(sum(p.n for p in probs)), None
    try:
        nnz = int(sum((lambda J: (J.T @ J).nnz)(p.residuals(x, jac=True)[1]) for p, x in zip(probs, points)))
    except Exception as e:  # (shapes only: the bytes below are left out without them)
        print("nnz not available:", e)
    b_spread = float(np.max(b_runs) - np.min(b_runs))
    rec = dict(
        workload=dict(worlds=args.worlds, robots=args.robots, poses=args.poses, seed=7, unknowns_per_world=int(probs[0].n),
                      columns_per_world=int(len(sels[0][3])), union_unknowns=n, union_nnz=nnz, runs=args.runs),
        a_group_call=dict(setup_plus_solve_ms=stats(a_runs), wall_ms=stats(a_wall), setup_ms_last=info_a["setup_ms"],
                          solve_ms_last=info_a["solve_ms"], passes=info_a["passes"], pcg_iters=info_a["pcg_iters"],
                          columns=info_a["columns"], max_residual=info_a["max_residual"],
                          steps_of_a_column=dict(min=int(steps_a.min()), median=float(np.median(steps_a)), max=int(steps_a.max()))),
        b_kept_single_handles=dict(wall_ms=stats(b_runs), pcg_iters_sum=int(sum(c[5]["pcg_iters"] for c in cols_b)),
                                   batches_sum=int(sum(c[5]["batches"] for c in cols_b)),
                                   steps_of_a_column=dict(min=int(steps_b.min()), median=float(np.median(steps_b)), max=int(steps_b.max()))),
        c_marginal_covariances_loop=dict(wall_ms=stats(c_runs)),
        d_refine_with_marginals=dict(wall_ms=stats(d_runs), refine_then_loop_wall_ms=stats(d_two),
                                     two_step_over_one=float(np.median(d_two) / np.median(d_runs))),
        b_over_a=float(np.median(b_runs) / np.median(a_runs)), c_over_a=float(np.median(c_runs) / np.median(a_runs)),
        speed_condition=dict(statement="a (setup + solve) is not slower than b; the margin is the spread of b over its runs",
                             a_median_ms=float(np.median(a_runs)), b_median_ms=float(np.median(b_runs)), b_spread_ms=b_spread,
                             met=bool(np.median(a_runs) <= np.median(b_runs) + b_spread)),
        worst_relative_difference_of_a_diagonal_entry=dict(group_vs_single_handles=diag_ab, width_16_vs_0_on_one_single_handle=rel(w16[1], w0[1])),
        nees={k: dict(mean=float(np.mean(v)), count=len(v), degrees_of_freedom=2 if k == "beacons" else 3) for k, v in nees.items()},
    )
    if nnz is not None:  # one launch from shapes: the matrix once (values, columns, row pointers) + NV operands read + NV products written
        rec["k_gbm_product_bytes"] = {str(nv): int(nnz * 12 + (n + 1) * 4 + 2 * nv * n * 8) for nv in (16, 4)}
    if args.kernel_stats:
        k = kernel_time_us(args.kernel_stats, "k_gbm_productILi16E") or kernel_time_us(args.kernel_stats, "k_gbm_product<16>")
        if k and nnz is not None:
            k["bytes"] = rec["k_gbm_product_bytes"]["16"]
            k["TB_per_s_at_average"] = k["bytes"] / (k["average_us"] * 1e-6) / 1e12
            k["TB_per_s_at_max_us"] = k["bytes"] / (k["max_us"] * 1e-6) / 1e12
            k["note"] = ("`bytes` is a launch with all 16 slots of every world live.  Slots that have converged cost no traffic, so "
                         "late launches move fewer bytes and the rate at the average time overstates; the slowest launch is one "
                         "with every slot live, and the rate at max_us is the kernel's")
        rec["k_gbm_product_16_trace"] = k
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k not in ("workload",)}))


if __name__ == "__main__":
    main()
