"""Batched range leverage and predicted range variances against the single-graph calls over the same worlds
(profiles/leverage_batch.json).

  python profiles/scripts/leverage_batch.py OUT.json [--lib PATH] [--runs 5] [--e2e-runs 3] [--worlds 64] [--robots 4] [--poses 1000]

The workload is that of profiles/samples_batch.json: `worlds` generated Manhattan worlds (4 robots x 1000 poses), relaxed in
lock-step (solve_score_batch), refined by refine_estimate_batch; world i from the stream of seed i.  The parent process never
touches the device: it runs every step below as a child of its own (`--step NAME`) under that step's time limit and stops at
the first one that fails.  Every child builds the workload again.  Legs alternate in one process, `runs` times each after
one warm-up of each; medians with minimum and maximum of the host clock around the calls, creates excluded:
  leverage   (A) RefineBatchHandle.leverage at 16 and 64 draws on a kept group handle, (S) RefineBatchHandle.samples with
             the same draws on the same handle (what k_gbl_measure costs beside the moments it replaces), (B)
             LeverageHandle.leverage over `worlds` kept single handles; the largest difference of a redundancy
             (red_sum / S over the ranges) between A and B; bytes per launch of k_gbl_measure from shapes
  variances  RefineBatchHandle.range_variances with 16 pose-beacon pairs per world against a loop of
             LeverageHandle.range_variances over kept single handles; the largest relative difference of a variance
  e2e        range_leverage_batch(...) at 16 draws against [range_leverage(...) for every world] (`e2e-runs` times each)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

COUNTS = (16, 64)
STEPS = (("leverage", 900), ("variances", 600), ("e2e", 900))  # (name, seconds)


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), all=[float(x) for x in xs])


def measure_bytes(probs):
    """Bytes one launch of k_gbl_measure moves for a pass of 16 taken draws of every world, from shapes (2-D): the graph (ids,
    measured values, precisions, the two poses or points), the four sums in and out, and per draw the measurement's local
    unknowns (6 per relative pose, 4 per range, 2 per prior; z is regenerated, not read)."""
    total = 0
    for prob in probs:
        n_rel, n_rng, n_pri = len(prob.bi), len(prob.ra), len(prob.pl)
        graph = n_rel * (2 * 4 + (2 + 4 + 2) * 8 + 2 * 3 * 8) + n_rng * (2 * 4 + 2 * 8 + 2 * 2 * 8) + n_pri * (4 + 3 * 8 + 2 * 8)
        sums = 2 * 4 * 8 * (n_rel + n_rng + n_pri)
        total += graph + sums + 16 * 8 * (6 * n_rel + 4 * n_rng + 2 * n_pri)
    return int(total)


def workload(args):
    from score_amd.generate import GeneratedBatch
    from score_amd.marginals import _problem_and_point, _select
    from score_amd.refine_batch import refine_estimate_batch
    from score_amd.solve_score import solve_score_batch

    batch = GeneratedBatch(args.worlds, seed=7, n_robots=args.robots, n_poses=args.poses, lib_path=args.lib)
    graphs = batch.graphs()
    relaxed = solve_score_batch(graphs, "SOCP", lib_path=args.lib)
    refined = [r for r, _ in refine_estimate_batch(graphs, relaxed, lib_path=args.lib, max_group=args.worlds)]
    probs, points = zip(*[_problem_and_point(g, r, None, None) for g, r in zip(graphs, refined)])
    ids = [_select(p, None)[1] for p in probs]
    print("worlds ready", flush=True)
    return graphs, refined, list(probs), list(points), ids


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def step_leverage(args):
    from score_amd.leverage import LeverageHandle, measurement_counts
    from score_amd.refine_batch import RefineBatchHandle

    _, _, probs, points, ids = workload(args)
    seeds = list(range(args.worlds))
    rec = dict(workload=dict(worlds=args.worlds, robots=args.robots, poses=args.poses, seed=7, unknowns_per_world=int(probs[0].n),
                             measurements=int(sum(sum(measurement_counts(p)) for p in probs)), runs=args.runs),
               bytes_per_launch_k_gbl_measure_16_draws=measure_bytes(probs), n_samples={})
    group, create = clock(lambda: RefineBatchHandle(probs, args.lib))
    rec["create_ms"] = dict(group_handle=create)
    singles = []
    try:
        singles, create = clock(lambda: [LeverageHandle(p, args.lib) for p in probs])
        rec["create_ms"]["single_handles_sum"] = create
        for S in COUNTS:
            a, s, b = [], [], []
            for i in range(args.runs + 1):  # (the first of each warms up)
                (rc_a, out_a, info_a), wall_a = clock(lambda: group.leverage(points, [None] * len(probs), S, seeds))
                (rc_s, _, info_s), wall_s = clock(lambda: group.samples(points, ids, S, seeds))
                out_b, wall_b = clock(lambda: [h.leverage(x, None, S, seed=k) for h, x, k in zip(singles, points, seeds)])
                assert rc_a == 0 and rc_s == 0 and all(o["rc"] == 0 for o in out_b)
                print(f"{S} draws, round {i}: A {wall_a:.1f} ms | samples {wall_s:.1f} ms | B {wall_b:.1f} ms", flush=True)
                if i:
                    a.append(wall_a); s.append(wall_s); b.append(wall_b)
            worst = 0.0
            for p, ga, gb in zip(probs, out_a, out_b):
                n_rel, n_rng, _ = measurement_counts(p)
                cut = slice(n_rel, n_rel + n_rng)
                worst = max(worst, float(np.max(np.abs(ga["red_sum"][cut] - gb["red_sum"][cut]))) / S)
            rec["n_samples"][str(S)] = dict(
                a_group_leverage_wall_ms=stats(a), group_samples_wall_ms=stats(s), b_kept_single_handles_wall_ms=stats(b),
                b_over_a=float(np.median(b) / np.median(a)), a_over_samples=float(np.median(a) / np.median(s)),
                a_last=dict(setup_ms=info_a["setup_ms"], rhs_ms=info_a["rhs_ms"], solve_ms=info_a["solve_ms"], passes=info_a["passes"],
                            pcg_iters=info_a["pcg_iters"], max_residual=info_a["max_residual"]),
                samples_last=dict(setup_ms=info_s["setup_ms"], rhs_ms=info_s["rhs_ms"], solve_ms=info_s["solve_ms"]),
                largest_redundancy_difference_a_vs_b=worst)
    finally:
        for h in singles:
            h.close()
        group.close()
    return rec


def step_variances(args):
    from score_amd.leverage import LeverageHandle
    from score_amd.refine_batch import RefineBatchHandle

    _, _, probs, points, _ = workload(args)
    # 16 pose - beacon pairs per world: poses spread over the world, the beacons in turn
    pairs = [np.asarray([(1 + (k * (p.Np - 1)) // 16, p.Np + k % p.Nl) for k in range(16)], dtype=np.int32) for p in probs]
    group = RefineBatchHandle(probs, args.lib)
    singles = []
    try:
        singles = [LeverageHandle(p, args.lib) for p in probs]
        a, b = [], []
        for i in range(args.runs + 1):
            (rc_a, out_a, info_a), wall_a = clock(lambda: group.range_variances(points, pairs))
            out_b, wall_b = clock(lambda: [h.range_variances(x, c) for h, x, c in zip(singles, points, pairs)])
            assert rc_a == 0 and all(o["rc"] == 0 for o in out_b)
            print(f"range variances, round {i}: group {wall_a:.1f} ms | loop {wall_b:.1f} ms", flush=True)
            if i:
                a.append(wall_a); b.append(wall_b)
        worst = max(float(np.max(np.abs(ga["variances"] - gb["variances"]) / gb["variances"])) for ga, gb in zip(out_a, out_b))
        return dict(pairs_per_world=16, group_wall_ms=stats(a), kept_single_handles_wall_ms=stats(b), loop_over_group=float(np.median(b) / np.median(a)),
                    group_last=dict(setup_ms=info_a["setup_ms"], solve_ms=info_a["solve_ms"], passes=info_a["passes"], pcg_iters=info_a["pcg_iters"],
                                    max_residual=info_a["max_residual"]),
                    largest_relative_variance_difference=worst)
    finally:
        for h in singles:
            h.close()
        group.close()


def step_e2e(args):
    from score_amd.leverage import range_leverage
    from score_amd.leverage_batch import range_leverage_batch

    graphs, refined, _, _, _ = workload(args)
    one, loop = [], []
    for i in range(args.e2e_runs + 1):
        _, wall_one = clock(lambda: range_leverage_batch(graphs, refined, n_samples=16, seed=0, lib_path=args.lib, max_group=args.worlds))
        _, wall_loop = clock(lambda: [range_leverage(g, r, n_samples=16, seed=k, lib_path=args.lib) for k, (g, r) in enumerate(zip(graphs, refined))])
        print(f"16 draws, end to end, round {i}: batch {wall_one:.1f} ms | loop {wall_loop:.1f} ms", flush=True)
        if i:
            one.append(wall_one); loop.append(wall_loop)
    return dict(n_samples=16, range_leverage_batch_wall_ms=stats(one), range_leverage_loop_wall_ms=stats(loop),
                loop_over_batch=float(np.median(loop) / np.median(one)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "leverage_batch.json"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--e2e-runs", type=int, default=3)
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    ap.add_argument("--only", default=None, help="comma-separated steps to run (default: all)")
    args = ap.parse_args()
    if args.step:  # a child: one step, its record to `out`
        rec = dict(leverage=step_leverage, variances=step_variances, e2e=step_e2e)[args.step](args)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = {}
    wanted = args.only.split(",") if args.only else [s for s, _ in STEPS]
    for name, limit in STEPS:
        if name not in wanted:
            continue
        part = f"{args.out}.{name}.part"
        cmd = [sys.executable, os.path.abspath(__file__), part, "--step", name, "--runs", str(args.runs), "--e2e-runs", str(args.e2e_runs),
               "--worlds", str(args.worlds), "--robots", str(args.robots), "--poses", str(args.poses)] + (["--lib", args.lib] if args.lib else [])
        try:
            done = subprocess.run(cmd, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {name}: no result within {limit} s; stopping", flush=True)
            sys.exit(124)
        if done.returncode != 0:
            print(f"step {name}: exit status {done.returncode}; stopping", flush=True)
            sys.exit(done.returncode if done.returncode > 0 else 1)
        with open(part) as f:
            rec[name] = json.load(f)
        os.remove(part)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
