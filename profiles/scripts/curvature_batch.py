"""The batched second-order check against the single-graph call over the same worlds (profiles/curvature_batch.json).

  python profiles/scripts/curvature_batch.py OUT.json [--lib PATH] [--runs 5] [--worlds 64] [--robots 4] [--poses 1000]

The workload is that of profiles/scripts/spectrum_batch.py: `worlds` generated Manhattan worlds (4 robots x 1000 poses),
relaxed in lock-step (solve_score_batch), refined by refine_estimate_batch; the k = 8 lowest eigenpairs of every world's E,
half the Hessian of its cost, at its refined point, rel_tol = 1e-9.  Legs, alternating in one process, `runs` times each
after one warm-up of each; medians with minimum and maximum, host clock around the calls:
  a  the group call (RefineBatchHandle.curvature) on a kept group handle
  b  CurvatureHandle.curvature over `worlds` kept single handles, creates excluded -- the way to the same answer without the
     group call
  c  RefineBatchHandle.spectrum on the same group handle: the sibling whose setup (a)'s is compared with
Recorded beside them: rounds, iterations per world (min / median / max), how many worlds are minima, the largest difference
of the lowest value between (a) and (b) in units of the two calls' reported residuals' sum, the setup of (a) beside the setup
of (c), and the bytes of one k_gbc_blocks and one k_gbc_gather launch from shapes (no kernel trace is taken here)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from score_amd.curvature import CurvatureHandle  # noqa: E402
from score_amd.generate import GeneratedBatch  # noqa: E402
from score_amd.marginals import _problem_and_point  # noqa: E402
from score_amd.refine_batch import RefineBatchHandle, refine_estimate_batch  # noqa: E402
from score_amd.solve_score import solve_score_batch  # noqa: E402

REL_TOL, MAX_ITERS, SHIFT, K = 1e-9, 200, 1e-8, 8


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), all=[float(x) for x in xs])


def launch_bytes(probs, points):
    """Bytes of one k_gbc_blocks and one k_gbc_gather launch, from shapes.  Blocks: what a lane reads of its measurement and
    its variables, and the block and J'r slots it writes (2-D: 36 + 6 doubles per relative pose, 16 + 4 per range, 4 + 2 per
    prior; 3-D: 144 + 12, 36 + 6, 9 + 3).  Gather: per entry its list bounds, the diagonal word and the value written; per
    slot its index and the J'J and the exact block entry.  The slots are counted as every block entry (those of the fixed
    poses have none: an upper bound), the entries as the non-zeros of |J|'|J|."""
    blocks = gather_slots = entries = 0
    for p, x in zip(probs, points):
        d = 3 if "3D" in type(p).__name__ else 2
        ps, nr, ng = (3, 6, 4) if d == 2 else (12, 12, 6)
        n_rel, n_rng, n_pri = len(p.a["rel_base"]), len(p.a["rng_a"]), len(p.a["lprior_lm"])
        blocks += n_rel * (8 * (2 * ps + d + d * d + 2) + 8 + 8 * (nr * nr + nr))
        blocks += n_rng * (8 * (2 * d + 2) + 8 + 8 * (ng * ng + ng))
        blocks += n_pri * (8 * (2 * d + 1) + 4 + 8 * (d * d + d))
        gather_slots += n_rel * nr * nr + n_rng * ng * ng + n_pri * d * d
        _, J = p.residuals(x, jac=True)
        entries += int((abs(J).T @ abs(J)).nnz)
    return dict(k_gbc_blocks=int(blocks), k_gbc_gather=int(gather_slots * (4 + 8 + 8) + entries * (4 + 4 + 8)),
                pattern_entries=int(entries), block_slots_upper_bound=int(gather_slots))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "curvature_batch.json"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--robots", type=int, default=4)
    ap.add_argument("--poses", type=int, default=1000)
    args = ap.parse_args()
    batch = GeneratedBatch(args.worlds, seed=7, n_robots=args.robots, n_poses=args.poses, lib_path=args.lib)
    graphs = batch.graphs()
    relaxed = solve_score_batch(graphs, "SOCP", lib_path=args.lib)
    refined = [r for r, _ in refine_estimate_batch(graphs, relaxed, lib_path=args.lib, max_group=args.worlds)]
    probs, points = zip(*[_problem_and_point(g, r, None, None) for g, r in zip(graphs, refined)])
    points = list(points)

    t0 = time.perf_counter()
    group = RefineBatchHandle(probs, args.lib)
    create_a = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    singles = [CurvatureHandle(p, args.lib) for p in probs]
    create_b = 1e3 * (time.perf_counter() - t0)
    n = int(sum(p.n for p in probs))
    rec = dict(workload=dict(worlds=args.worlds, robots=args.robots, poses=args.poses, seed=7, unknowns_per_world=int(probs[0].n),
                             union_unknowns=n, k=K, runs=args.runs, rel_tol=REL_TOL, max_iters=MAX_ITERS, shift=SHIFT),
               creates_ms=dict(group_handle=create_a, single_handles=create_b))
    try:
        a_wall, a_setup, a_solve, b_wall, c_wall, c_setup, c_solve = [], [], [], [], [], [], []
        for i in range(args.runs + 1):  # (the first of each warms up)
            t0 = time.perf_counter()
            rc_a, per_a, info_a = group.curvature(points, K, REL_TOL, MAX_ITERS, SHIFT)
            wall_a = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            per_b = [h.curvature(x, K, REL_TOL, MAX_ITERS, SHIFT) for h, x in zip(singles, points)]
            wall_b = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            rc_c, per_c, info_c = group.spectrum(points, K, REL_TOL, MAX_ITERS, SHIFT)
            wall_c = 1e3 * (time.perf_counter() - t0)
            print(f"round {i}: a {wall_a:.1f} ms (setup {info_a['setup_ms']:.1f}, solve {info_a['solve_ms']:.1f}), rc {rc_a}, rounds "
                  f"{info_a['rounds']} | b {wall_b:.1f} ms, rc {max(r[0] for r in per_b)} | c {wall_c:.1f} ms (setup "
                  f"{info_c['setup_ms']:.1f}), rc {rc_c}, rounds {info_c['rounds']}", flush=True)
            if i:
                a_wall.append(wall_a); a_setup.append(info_a["setup_ms"]); a_solve.append(info_a["solve_ms"])
                b_wall.append(wall_b)
                c_wall.append(wall_c); c_setup.append(info_c["setup_ms"]); c_solve.append(info_c["solve_ms"])
        its_a = np.array([m[4] for m in per_a])
        its_b = np.array([r[5]["iterations"] for r in per_b])
        minima = int(sum(1 for m in per_a if m[0][0] > REL_TOL * m[6]))
        saddles = int(sum(1 for m in per_a if np.any(m[0] < -REL_TOL * m[6])))
        worst = max(float(abs(ma[0][0] - rb[1][0]) / (ma[2][0] + rb[3][0])) for ma, rb in zip(per_a, per_b))
        rec["k8"] = dict(
            a_group_call=dict(wall_ms=stats(a_wall), setup_ms=stats(a_setup), solve_ms=stats(a_solve), rc=int(rc_a),
                              rounds=int(info_a["rounds"]), ms_per_round=float(info_a["solve_ms"] / info_a["rounds"]),
                              unconverged=int(info_a["unconverged"]), saddles_reported=int(info_a["saddles"]),
                              max_residual=float(info_a["max_residual"]),
                              iterations_of_a_world=dict(min=int(its_a.min()), median=float(np.median(its_a)), max=int(its_a.max()))),
            b_kept_single_handles=dict(wall_ms=stats(b_wall), ms_per_world=float(np.median(b_wall) / args.worlds),
                                       rc_max=int(max(r[0] for r in per_b)),
                                       iterations_of_a_world=dict(min=int(its_b.min()), median=float(np.median(its_b)), max=int(its_b.max()))),
            c_group_spectrum=dict(wall_ms=stats(c_wall), setup_ms=stats(c_setup), solve_ms=stats(c_solve), rc=int(rc_c),
                                  rounds=int(info_c["rounds"])),
            b_over_a=float(np.median(b_wall) / np.median(a_wall)),
            ranges_do_not_overlap=bool(np.max(a_wall) < np.min(b_wall)),
            a_over_c=float(np.median(a_wall) / np.median(c_wall)),
            setup_a_minus_setup_c_ms=float(np.median(a_setup) - np.median(c_setup)),
            worlds_at_a_minimum=minima, worlds_at_a_saddle=saddles,
            largest_c_max=float(max(m[7] for m in per_a)),
            worst_lowest_value_difference_over_rho_plus_rho=worst)
    finally:
        group.close()
        for h in singles:
            h.close()
    rec["bytes_per_launch"] = launch_bytes(probs, points)
    rec["bytes_per_launch"]["note"] = "from shapes; no kernel trace was taken: the per-launch kernel times are not recorded"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k not in ("workload",)}))


if __name__ == "__main__":
    main()
