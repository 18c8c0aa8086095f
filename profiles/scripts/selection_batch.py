"""Batched greedy selection of candidate ranges against the single-graph call over the same worlds
(profiles/selection_batch.json).

  python profiles/scripts/selection_batch.py OUT.json [--lib PATH] [--runs 5] [--e2e-runs 3] [--worlds 64] [--robots 4] [--poses 1000]

The workload is that of profiles/leverage_batch.json: `worlds` generated Manhattan worlds (4 robots x 1000 poses), relaxed in
lock-step (solve_score_batch), refined by refine_estimate_batch; world i from the stream of seed i.  Every world lists
C = 256 candidates (profiles/scripts/selection.py's pairs: half pose - beacon, half pose - pose) with precision 4 graded by
1 + 1/2 cos c, k = 32, width 16.  The parent process never touches the device: it runs every step below as a child of its own
(`--step NAME`) under that step's time limit and stops at the first one that fails.  Every child builds the workload again.
Legs alternate in one process, `runs` times each after one warm-up of each; medians with minimum and maximum of the host clock
around calls that end in a device synchronise, creates excluded:
  group  (a) RefineBatchHandle.select_ranges against RefineBatchHandle.range_variances over the same pairs on the same kept
         group handle: the feature's own cost, with the call's cross_ms and greedy_ms;
         (b) the same group call against a loop of SelectionHandle.select_ranges over `worlds` kept single handles; beside it
         contract 3 on every world: order, gains, pick variances and remaining of the group call equal to score_select_greedy
         on that world's returned matrix, np.array_equal
  e2e    (c) select_ranges_batch(...) against [select_ranges(...) for every world]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CANDIDATES, PICKS = 256, 32
STEPS = (("group", 1000), ("e2e", 1000))  # (name, seconds)


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), all=[float(x) for x in xs])


def workload(args):
    from score_amd.generate import GeneratedBatch
    from score_amd.marginals import _problem_and_point
    from score_amd.refine_batch import refine_estimate_batch
    from score_amd.solve_score import solve_score_batch

    batch = GeneratedBatch(args.worlds, seed=7, n_robots=args.robots, n_poses=args.poses, lib_path=args.lib)
    graphs = batch.graphs()
    relaxed = solve_score_batch(graphs, "SOCP", lib_path=args.lib)
    refined = [r for r, _ in refine_estimate_batch(graphs, relaxed, lib_path=args.lib, max_group=args.worlds)]
    probs, points = zip(*[_problem_and_point(g, r, None, None) for g, r in zip(graphs, refined)])
    print("worlds ready", flush=True)
    return graphs, refined, list(probs), list(points)


def pairs_of(prob, count):
    """Half pose - beacon (the beacons in turn), half pose - pose 37 on (profiles/scripts/selection.py's pairs)."""
    Np, Nl = prob.Np, prob.Nl
    p = 1 + (np.arange(count) * ((Np - 1) // count) + 11) % (Np - 1)
    other = np.where(np.arange(count) % 2 == 0, Np + (np.arange(count) // 2) % Nl, 1 + (p + 36) % (Np - 1))
    return np.column_stack([p, other]).astype(np.int32)


def weights():
    return 4.0 * (1.0 + 0.5 * np.cos(np.arange(CANDIDATES)))


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


VALUES = ("order", "gains", "pick_variances", "remaining")


def step_group(args):
    from score_amd.refine_batch import RefineBatchHandle
    from score_amd.selection import SelectionHandle, greedy_from_matrix

    _, _, probs, points = workload(args)
    G = len(probs)
    pairs, ws, w = [pairs_of(p, CANDIDATES) for p in probs], [weights()] * G, weights()
    rec = dict(workload=dict(worlds=args.worlds, robots=args.robots, poses=args.poses, seed=7, unknowns_per_world=int(probs[0].n),
                             candidates_per_world=CANDIDATES, k=PICKS, block_width=16, runs=args.runs))
    group, create = clock(lambda: RefineBatchHandle(probs, args.lib))
    rec["create_ms"] = dict(group_handle=create)
    singles = []
    try:
        singles, create = clock(lambda: [SelectionHandle(p, args.lib) for p in probs])
        rec["create_ms"]["single_handles_sum"] = create
        a, v, b, infos = [], [], [], []
        for i in range(args.runs + 1):  # (the first of each warms up)
            (rc_a, out_a, info_a), wall_a = clock(lambda: group.select_ranges(points, pairs, ws, PICKS))
            (rc_v, out_v, info_v), wall_v = clock(lambda: group.range_variances(points, pairs))
            out_b, wall_b = clock(lambda: [h.select_ranges(x, c, w, PICKS) for h, x, c in zip(singles, points, pairs)])
            assert rc_a == 0 and rc_v == 0 and all(o["rc"] == 0 for o in out_b)
            print(f"round {i}: group select_ranges {wall_a:.1f} ms (cross {info_a['cross_ms']:.2f}, greedy {info_a['greedy_ms']:.2f}) | "
                  f"group range_variances {wall_v:.1f} ms | loop of single select_ranges {wall_b:.1f} ms", flush=True)
            if i:
                a.append(wall_a); v.append(wall_v); b.append(wall_b); infos.append(info_a)
        same_columns = all(np.array_equal(x[f], y[f]) for x, y in zip(out_a, out_v) for f in ("variances", "residuals", "iterations"))
        same_order = sum(bool(np.array_equal(x["order"], y["order"])) for x, y in zip(out_a, out_b))
        gain_gap = max(abs(x["total_gain"] - y["info"]["total_gain"]) / y["info"]["total_gain"] for x, y in zip(out_a, out_b))
        # contract 3 on every world: the group call's member against score_select_greedy on its returned matrix
        _, with_matrix, _ = group.select_ranges(points, pairs, ws, PICKS, with_matrix=True)
        equal = 0
        for m, plain in zip(with_matrix, out_a):
            alone = greedy_from_matrix(m["matrix"], w, PICKS, lib_path=args.lib)
            equal += all(np.array_equal(m[f], alone[f]) and np.array_equal(m[f], plain[f]) for f in VALUES)
        single_infos = [o["info"] for o in out_b]
        med = lambda xs: float(np.median(xs))  # noqa: E731
        rec.update(group_select_wall_ms=stats(a), group_range_variances_wall_ms=stats(v), kept_single_handles_wall_ms=stats(b),
                   selection_cost_ms=med(a) - med(v), loop_over_group=med(b) / med(a),
                   cross_ms=stats([x["cross_ms"] for x in infos]), greedy_ms=stats([x["greedy_ms"] for x in infos]),
                   group_last=dict(setup_ms=info_a["solve"]["setup_ms"], solve_ms=info_a["solve"]["solve_ms"], passes=info_a["solve"]["passes"],
                                   pcg_iters=info_a["solve"]["pcg_iters"], max_residual=info_a["solve"]["max_residual"],
                                   picked=info_a["picked"], total_gain=info_a["total_gain"], asymmetry=info_a["asymmetry"]),
                   singles_last=dict(solve_ms_sum=float(sum(s["solve"]["solve_ms"] for s in single_infos)),
                                     cross_ms_sum=float(sum(s["cross_ms"] for s in single_infos)),
                                     greedy_ms_sum=float(sum(s["greedy_ms"] for s in single_infos)),
                                     batches_each=int(single_infos[0]["solve"]["batches"])),
                   columns_equal_the_group_range_variances=bool(same_columns),
                   worlds_whose_selection_equals_score_select_greedy_on_their_matrix=int(equal),
                   worlds_with_the_single_handles_order=int(same_order), largest_relative_total_gain_difference_to_single=float(gain_gap),
                   derived=dict(P_bytes=8 * G * CANDIDATES ** 2, L_bytes=8 * G * CANDIDATES * PICKS,
                                cross_bytes_written_per_launch=8 * G * CANDIDATES * 16,
                                note="from shapes; per-launch kernel times were not traced"))
    finally:
        for h in singles:
            h.close()
        group.close()
    return rec


def step_e2e(args):
    from score_amd.selection import select_ranges
    from score_amd.selection_batch import select_ranges_batch

    graphs, refined, probs, _ = workload(args)
    names = []
    for p in probs:
        nm = [str(x) for x in p.a["pose_names"]] + [str(x) for x in p.a["landmark_names"]]
        names.append([(nm[a], nm[b]) for a, b in pairs_of(p, CANDIDATES)])
    w = weights()
    one, loop = [], []
    for i in range(args.e2e_runs + 1):
        got, wall_one = clock(lambda: select_ranges_batch(graphs, refined, names, PICKS, precision=[w] * len(graphs), lib_path=args.lib,
                                                          max_group=args.worlds))
        ref, wall_loop = clock(lambda: [select_ranges(g, r, nm, PICKS, precision=w, lib_path=args.lib)
                                        for g, r, nm in zip(graphs, refined, names)])
        print(f"end to end, round {i}: batch {wall_one:.1f} ms | loop {wall_loop:.1f} ms", flush=True)
        if i:
            one.append(wall_one); loop.append(wall_loop)
    same = sum(bool(np.array_equal(a.order, b.order)) for (a, _), (b, _) in zip(got, ref))
    return dict(candidates_per_world=CANDIDATES, k=PICKS, runs=args.e2e_runs, select_ranges_batch_wall_ms=stats(one),
                select_ranges_loop_wall_ms=stats(loop), loop_over_batch=float(np.median(loop) / np.median(one)),
                worlds_with_equal_orders=int(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "selection_batch.json"))
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
        rec = dict(group=step_group, e2e=step_e2e)[args.step](args)
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
               "--worlds", str(args.worlds), "--robots", str(args.robots), "--poses", str(args.poses)]
        cmd += ["--lib", args.lib] if args.lib else []
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
