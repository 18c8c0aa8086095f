"""Batched posterior samples against the single-graph call over the same worlds (profiles/samples_batch.json).

  python profiles/scripts/samples_batch.py OUT.json [--lib PATH] [--runs 5] [--e2e-runs 3] [--worlds 64] [--robots 4] [--poses 1000]

The workload is the README's study: `worlds` generated Manhattan worlds (4 robots x 1000 poses), relaxed in lock-step
(solve_score_batch), refined by refine_estimate_batch; 16 and 64 draws per world, the default variables of every world (the
generator's beacons and last poses), world i from the stream of seed i.  Legs, alternating in one process, `runs` times each
after one warm-up of each; medians with minimum and maximum:
  a  the group call (RefineBatchHandle.samples) on a kept group handle: setup_ms + rhs_ms + solve_ms, and the host clock
  b  SamplesHandle.draw over `worlds` kept single handles, creates excluded: host clock around the loop of calls
  c  posterior_samples_batch(...) end to end against [posterior_samples(...) for every world] (`e2e-runs` times each)
The creates of both kinds of handle are timed once and reported beside the legs.  Recorded with them: passes and iterations
per pass, rhs_ms / solve_ms, the largest difference between the steps of a and b, what one launch of k_gbs_blocks /
k_gbs_gather / k_gbs_moments moves for a full pass (from shapes), and the mean sampled NEES of the beacons and last poses
over the worlds from Samples.covariance at 64 draws (reported, not gated: the range noise is clamped at 0, and a sampled
covariance of 64 draws carries a relative standard error of sqrt(2 / 64) per entry)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from score_amd.generate import GeneratedBatch  # noqa: E402
from score_amd.marginals import _problem_and_point, _select  # noqa: E402
from score_amd.refine_batch import RefineBatchHandle, refine_estimate_batch  # noqa: E402
from score_amd.samples import SamplesHandle, _moment_sizes, posterior_samples  # noqa: E402
from score_amd.samples_batch import posterior_samples_batch  # noqa: E402
from score_amd.solve_score import solve_score_batch  # noqa: E402

COUNTS = (16, 64)


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), all=[float(x) for x in xs])


def launch_bytes(probs):
    """Bytes one launch moves for a pass of 16 draws of every world, from shapes (2-D: 6 local unknowns per relative pose, 4
    per range, 2 per prior): the single kernels' figures (profiles/scripts/posterior_samples.py) summed over the members."""
    blocks = gather = moments = 0
    for prob in probs:
        n_rel, n_rng, n_pri, n = len(prob.bi), len(prob.ra), len(prob.pl), int(prob.n)
        gsz = 6 * n_rel + 4 * n_rng + 2 * n_pri
        contributions = gsz - 3 * int(np.count_nonzero(prob.bi == 0)) - 3 * int(np.count_nonzero(prob.tj == 0)) \
            - 2 * int(np.count_nonzero(prob.ra == 0)) - 2 * int(np.count_nonzero(prob.rb == 0))
        graph = n_rel * (2 * 4 + (2 + 4 + 2) * 8 + 2 * 3 * 8) + n_rng * (2 * 4 + 2 * 8 + 2 * 2 * 8) + n_pri * (4 + 3 * 8 + 2 * 8)
        blocks += graph + 16 * gsz * 8
        gather += (n + 1) * 4 + contributions * 4 + 16 * contributions * 8 + 16 * n * 8
        moments += 16 * n * 8 + 2 * (_moment_sizes(prob)[2] + n) * 8
    return dict(k_gbs_blocks=int(blocks), k_gbs_gather=int(gather), k_gbs_moments=int(moments))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "samples_batch.json"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--e2e-runs", type=int, default=3)
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--poses", type=int, default=1000)
    args = ap.parse_args()
    batch = GeneratedBatch(args.worlds, seed=7, n_robots=args.robots, n_poses=args.poses, lib_path=args.lib)
    graphs = batch.graphs()
    relaxed = solve_score_batch(graphs, "SOCP", lib_path=args.lib)
    refined = [r for r, _ in refine_estimate_batch(graphs, relaxed, lib_path=args.lib, max_group=args.worlds)]
    probs, points = zip(*[_problem_and_point(g, r, None, None) for g, r in zip(graphs, refined)])
    sels = [_select(p, None) for p in probs]
    ids = [s[1] for s in sels]
    seeds = list(range(args.worlds))
    print("worlds ready", flush=True)
    rec = dict(workload=dict(worlds=args.worlds, robots=args.robots, poses=args.poses, seed=7, unknowns_per_world=int(probs[0].n),
                             selected_unknowns_per_world=int(len(sels[0][3])), union_unknowns=int(sum(p.n for p in probs)),
                             runs=args.runs, e2e_runs=args.e2e_runs),
               bytes_per_launch_16_draws=launch_bytes(probs), n_samples={})
    t0 = time.perf_counter()
    group = RefineBatchHandle(probs, args.lib)
    rec["create_ms"] = dict(group_handle=1e3 * (time.perf_counter() - t0))
    singles = []
    try:
        t0 = time.perf_counter()
        singles = [SamplesHandle(p, args.lib) for p in probs]
        rec["create_ms"]["single_handles_sum"] = 1e3 * (time.perf_counter() - t0)
        for S in COUNTS:
            a_runs, a_wall, b_runs = [], [], []
            for i in range(args.runs + 1):  # (the first of each warms up)
                t0 = time.perf_counter()
                rc_a, out_a, info_a = group.samples(list(points), ids, S, seeds)
                wall_a = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                out_b = [h.draw(x, v, S, seed=s) for h, x, v, s in zip(singles, points, ids, seeds)]
                wall_b = 1e3 * (time.perf_counter() - t0)
                assert rc_a == 0 and all(o["rc"] == 0 for o in out_b)
                own = info_a["setup_ms"] + info_a["rhs_ms"] + info_a["solve_ms"]
                print(f"{S} draws, round {i}: a {own:.1f} ms (wall {wall_a:.1f}) | b {wall_b:.1f}", flush=True)
                if i:
                    a_runs.append(own); a_wall.append(wall_a); b_runs.append(wall_b)
            diff = max(float(np.max(np.abs(a["steps"] - b["steps"]))) for a, b in zip(out_a, out_b))
            scale = max(float(np.max(np.abs(b["steps"]))) for b in out_b)
            its_a = np.concatenate([m["iterations"] for m in out_a])
            its_b = np.concatenate([o["iterations"] for o in out_b])
            rec["n_samples"][str(S)] = dict(
                a_group_call=dict(own_ms=stats(a_runs), wall_ms=stats(a_wall), setup_ms_last=info_a["setup_ms"], rhs_ms_last=info_a["rhs_ms"],
                                  solve_ms_last=info_a["solve_ms"], passes=info_a["passes"], pcg_iters=info_a["pcg_iters"],
                                  iterations_per_pass=info_a["pcg_iters"] / info_a["passes"], max_residual=info_a["max_residual"],
                                  steps_of_a_draw=dict(min=int(its_a.min()), median=float(np.median(its_a)), max=int(its_a.max()))),
                b_kept_single_handles=dict(wall_ms=stats(b_runs), pcg_iters_sum=int(sum(o["info"]["pcg_iters"] for o in out_b)),
                                           batches_sum=int(sum(o["info"]["batches"] for o in out_b)),
                                           own_ms_sum_last=float(sum(o["info"]["setup_ms"] + o["info"]["rhs_ms"] + o["info"]["solve_ms"] for o in out_b)),
                                           steps_of_a_draw=dict(min=int(its_b.min()), median=float(np.median(its_b)), max=int(its_b.max()))),
                b_over_a=float(np.median(b_runs) / np.median(a_wall)),
                worst_step_difference_a_vs_b=dict(absolute=diff, largest_step=scale))
    finally:
        for h in singles:
            h.close()
        group.close()
    for S in COUNTS:
        one, loop = [], []
        for i in range(args.e2e_runs + 1):
            t0 = time.perf_counter()
            out_c = posterior_samples_batch(graphs, refined, n_samples=S, seed=0, lib_path=args.lib, max_group=args.worlds)
            wall_one = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            _ = [posterior_samples(g, r, n_samples=S, seed=k, lib_path=args.lib) for k, (g, r) in enumerate(zip(graphs, refined))]
            wall_loop = 1e3 * (time.perf_counter() - t0)
            print(f"{S} draws, end to end, round {i}: batch {wall_one:.1f} ms | loop {wall_loop:.1f} ms", flush=True)
            if i:
                one.append(wall_one); loop.append(wall_loop)
        rec["n_samples"][str(S)]["c_end_to_end"] = dict(posterior_samples_batch_wall_ms=stats(one), posterior_samples_loop_wall_ms=stats(loop),
                                                        loop_over_batch=float(np.median(loop) / np.median(one)))
    # sampled NEES over the worlds, from the last end-to-end call (64 draws): Samples.covariance of the default variables
    nees = {"beacons": [], "last_poses": []}
    for i, (smp, _) in enumerate(out_c):
        cov = {nm: smp.covariance(nm) for nm in smp.order}
        for nm, (val, dof) in batch.nees(i, refined[i], cov).items():
            nees["beacons" if dof == 2 else "last_poses"].append(val)
    rec["sampled_nees_64_draws"] = {k: dict(mean=float(np.mean(v)), count=len(v), degrees_of_freedom=2 if k == "beacons" else 3)
                                    for k, v in nees.items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k != "workload"}))


if __name__ == "__main__":
    main()
