"""Batched predicted relative poses against the single-graph call over the same worlds (profiles/relative_batch.json).

  python profiles/scripts/relative_batch.py OUT.json [--lib PATH] [--parent-lib PATH] [--runs 5] [--e2e-runs 5] [--worlds 64]
                                                     [--robots 4] [--poses 1000]

The workload is that of profiles/leverage_batch.json: `worlds` generated Manhattan worlds (4 robots x 1000 poses), relaxed in
lock-step (solve_score_batch), refined by refine_estimate_batch; world i from the stream of seed i.  The parent process never
touches the device: it runs every step below as a child of its own (`--step NAME`) under that step's time limit and stops at
the first one that fails.  Every child builds the workload again.  Legs alternate in one process, `runs` times each after
one warm-up of each; medians with minimum and maximum of the host clock around the calls, creates excluded:
  group  RefineBatchHandle.relative_covariances with 16 pose-pose pairs per world (48 columns, width 16) on a kept group
         handle against a loop of RelativeHandle.relative_covariances over `worlds` kept single handles; the largest
         difference of the two P over a block's largest entry; the group call's setup_ms / solve_ms, passes and iterations
  e2e    predicted_relative_poses_batch(...) against [predicted_relative_poses(...) for every world]
  bits   (with --parent-lib: a library built from the parent commit) score_refine_relative_covariances on the tests' graphs a
         and d at widths 16 and 5 under both libraries: every output compared with np.array_equal"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

PAIRS = 16
STEPS = (("group", 900), ("e2e", 900), ("bits", 300))  # (name, seconds)


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


def pose_pairs(prob):
    """16 pose - pose pairs of a world: poses spread over the world, each with the pose half the poses on (another robot's);
    the first from the fixed pose 0."""
    Np = prob.Np
    out = [(0, Np // 2)]
    for k in range(1, PAIRS):
        p = 1 + (k * (Np - 1)) // PAIRS
        out.append((p, 1 + (p - 1 + Np // 2) % (Np - 1)))
    return np.asarray(out, dtype=np.int32)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def step_group(args):
    from score_amd.refine_batch import RefineBatchHandle
    from score_amd.relative import RelativeHandle

    _, _, probs, points = workload(args)
    pairs = [pose_pairs(p) for p in probs]
    rec = dict(workload=dict(worlds=args.worlds, robots=args.robots, poses=args.poses, seed=7, unknowns_per_world=int(probs[0].n),
                             pairs_per_world=PAIRS, columns_per_world=3 * PAIRS, block_width=16, runs=args.runs))
    group, create = clock(lambda: RefineBatchHandle(probs, args.lib))
    rec["create_ms"] = dict(group_handle=create)
    singles = []
    try:
        singles, create = clock(lambda: [RelativeHandle(p, args.lib) for p in probs])
        rec["create_ms"]["single_handles_sum"] = create
        a, b = [], []
        for i in range(args.runs + 1):  # (the first of each warms up)
            (rc_a, out_a, info_a), wall_a = clock(lambda: group.relative_covariances(points, pairs))
            out_b, wall_b = clock(lambda: [h.relative_covariances(x, c) for h, x, c in zip(singles, points, pairs)])
            assert rc_a == 0 and all(o["rc"] == 0 for o in out_b)
            print(f"relative covariances, round {i}: group {wall_a:.1f} ms | loop {wall_b:.1f} ms", flush=True)
            if i:
                a.append(wall_a); b.append(wall_b)
        worst = max(float(np.max(np.abs(ga["covariances"] - gb["covariances"]) / np.abs(gb["covariances"]).max(axis=(1, 2), keepdims=True)))
                    for ga, gb in zip(out_a, out_b))
        single_infos = [o["info"] for o in out_b]
        rec.update(group_wall_ms=stats(a), kept_single_handles_wall_ms=stats(b), loop_over_group=float(np.median(b) / np.median(a)),
                   group_last=dict(setup_ms=info_a["setup_ms"], solve_ms=info_a["solve_ms"], passes=info_a["passes"],
                                   pcg_iters=info_a["pcg_iters"], max_residual=info_a["max_residual"]),
                   singles_last=dict(setup_ms_sum=float(sum(s["setup_ms"] for s in single_infos)),
                                     solve_ms_sum=float(sum(s["solve_ms"] for s in single_infos)),
                                     batches_each=int(single_infos[0]["batches"]),
                                     pcg_iters_median=float(np.median([s["pcg_iters"] for s in single_infos])),
                                     pcg_iters_max=int(max(s["pcg_iters"] for s in single_infos))),
                   largest_difference_over_a_blocks_largest_entry=worst)
    finally:
        for h in singles:
            h.close()
        group.close()
    return rec


def step_e2e(args):
    from score_amd.relative import predicted_relative_poses
    from score_amd.relative_batch import predicted_relative_poses_batch

    graphs, refined, probs, _ = workload(args)
    names = []
    for p in probs:
        nm = [str(x) for x in p.a["pose_names"]]
        names.append([(nm[a], nm[b]) for a, b in pose_pairs(p)])
    one, loop = [], []
    for i in range(args.e2e_runs + 1):
        got, wall_one = clock(lambda: predicted_relative_poses_batch(graphs, refined, names, lib_path=args.lib, max_group=args.worlds))
        ref, wall_loop = clock(lambda: [predicted_relative_poses(g, r, nm, engine="device", lib_path=args.lib)
                                        for g, r, nm in zip(graphs, refined, names)])
        print(f"16 pairs, end to end, round {i}: batch {wall_one:.1f} ms | loop {wall_loop:.1f} ms", flush=True)
        if i:
            one.append(wall_one); loop.append(wall_loop)
    worst = max(float(np.max(np.abs(a.covariance - b.covariance) / np.abs(b.covariance).max(axis=(1, 2), keepdims=True)))
                for (a, _), (b, _) in zip(got, ref))
    return dict(pairs_per_world=PAIRS, runs=args.e2e_runs, predicted_relative_poses_batch_wall_ms=stats(one),
                predicted_relative_poses_loop_wall_ms=stats(loop), loop_over_batch=float(np.median(loop) / np.median(one)),
                largest_difference_over_a_blocks_largest_entry=worst)


def step_bits(args):
    """score_refine_relative_covariances under the parent commit's library and this one: equal bits, output by output."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import relative_helpers as rh
    from marginals_helpers import reference
    from score_amd.relative import RelativeHandle

    rec = {}
    for key, count in (("a", 6), ("d", 3)):
        _, _, ref = reference(key)
        ids = rh.pair_list(ref.prob, count)
        for width in (16, 5):
            outs = []
            for lib in (args.parent_lib, args.lib):
                with RelativeHandle(ref.prob, lib) as h:
                    outs.append(h.relative_covariances(ref.point, ids, block_width=width, with_solutions=True))
            old, new = outs
            same = {k: bool(np.array_equal(old[k], new[k]))
                    for k in ("rotations", "translations", "covariances", "residuals", "iterations", "converged", "solutions")}
            same["rc"] = old["rc"] == new["rc"] == 0
            same["pcg_iters"] = old["info"]["pcg_iters"] == new["info"]["pcg_iters"]
            print(f"graph {key}, {count} pairs, width {width}: {same}", flush=True)
            rec[f"{key}_width_{width}"] = dict(pairs=count, columns=int(new["info"]["columns"]), equal=same, all_equal=all(same.values()))
    rec["no_differing_entry"] = all(v["all_equal"] for v in rec.values())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "relative_batch.json"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    ap.add_argument("--only", default=None, help="comma-separated steps to run (default: all; bits needs --parent-lib)")
    args = ap.parse_args()
    if args.step:  # a child: one step, its record to `out`
        rec = dict(group=step_group, e2e=step_e2e, bits=step_bits)[args.step](args)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rec = {}
    wanted = args.only.split(",") if args.only else [s for s, _ in STEPS if s != "bits" or args.parent_lib]
    for name, limit in STEPS:
        if name not in wanted:
            continue
        part = f"{args.out}.{name}.part"
        cmd = [sys.executable, os.path.abspath(__file__), part, "--step", name, "--runs", str(args.runs), "--e2e-runs", str(args.e2e_runs),
               "--worlds", str(args.worlds), "--robots", str(args.robots), "--poses", str(args.poses)]
        cmd += (["--lib", args.lib] if args.lib else []) + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
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
