"""The GNC-TLS refinement loop on the device against the same loop written around refine_estimate (profiles/r12_robust_refine.json).

  python profiles/scripts/robust_refine.py OUT.json [--lib PATH] [--runs 5] [--robots 20] [--poses 1000] [--engine native]

The graph: 20 x 1000 poses, 4 beacons (the headline graph), 5 % of the ranges corrupted -- every second one and every one of
8 m or less measured long, + U(8, 15) m, the others short, x U(0.3, 0.5).  The start is the robust relaxation's estimate
(solve_score_robust) and its weights are the prior weights.  Legs, alternating, `runs` times each after one warm-up of each:
  device    refine_estimate_robust(engine="native"): one handle, the whole loop behind score_refine_robust_run
  baseline  the same schedule in Python around refine_estimate(engine="native", range_weights=...): one handle create
            (pattern of J'J, contribution lists, linear-mode handle, uploads) per outer solve, residuals and weights in NumPy
Wall times are host clocks around calls that end with the estimate read back (a device synchronise).
reweigh_call_ms: one score_refine_residuals call at the final estimate (upload of the point, both kernels, all four arrays
read back): an upper bound of what an outer iteration of the device loop costs beyond its LM iterations (in the loop the point
is already on the device and only the per-block partials are read).
--engine python (with --lib pointing at a CPU build of the C ABI) rehearses the script without a GPU; it measures nothing."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from score_amd.manhattan import make_manhattan  # noqa: E402
from score_amd.refine import _initial_point, _Problem, refine_estimate  # noqa: E402
from score_amd.refine_robust import (RobustRefineHandle, _nonbinary, decide, first_mu, range_residuals,  # noqa: E402
                                     refine_estimate_robust)
from score_amd.robust import gnc_tls_weight, solve_score_robust  # noqa: E402

C_IN, MIN_W, MU_STEP, MAX_OUTER, INNER, MAX_ITERS = 3.0, 1e-6, 1.4, 50, 5, 50


def corrupt(fg, fraction, seed):
    rng = np.random.default_rng(seed)
    n = len(fg.range_measurements)
    bad = np.sort(rng.choice(n, size=max(2, int(fraction * n)), replace=False))
    long_ = np.zeros(len(bad), dtype=bool)
    for j, i in enumerate(bad):
        m = fg.range_measurements[i]
        if j % 2 == 0 or m.dist <= 8:
            m.dist = float(m.dist + rng.uniform(8, 15))
            long_[j] = True
        else:
            m.dist = float(m.dist * rng.uniform(0.3, 0.5))
    return bad, long_


def baseline(fg, start, prior, kw):
    """The loop of include/score_refine_robust.h around refine_estimate: what a user could write before the device loop."""
    floor = np.where(prior < MIN_W, MIN_W, prior)
    prob = _Problem(fg, floor)  # (for the residuals only)
    prec0 = np.asarray(prob.a["rng_prec"], dtype=np.float64)
    w = np.ones(len(prec0))
    est, info = refine_estimate(fg, start, max_iters=MAX_ITERS, range_weights=floor, **kw)
    lm, k, mu = info["iterations"], 1, 0.0
    while True:
        r = range_residuals(prob, _initial_point(prob, est), prec0)
        seen = [(len(r), float(np.max(r * r)), C_IN, _nonbinary(w))]
        what = decide(k, MAX_OUTER, seen)
        if what != "go":
            break
        mu = first_mu(seen) if k == 1 else mu * MU_STEP
        w = gnc_tls_weight(r, mu, C_IN)
        k += 1
        est, info = refine_estimate(fg, est, max_iters=INNER, range_weights=floor * np.maximum(w, MIN_W), **kw)
        lm += info["iterations"]
    if k > 1 and what != "non_finite":
        est, info = refine_estimate(fg, est, max_iters=MAX_ITERS, range_weights=floor * np.maximum(w, MIN_W), **kw)
        lm += info["iterations"]
    return est, dict(outer=k, lm_iterations=lm, converged=what == "converged", flagged=int(np.count_nonzero(w < 0.5)), weights=w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--robots", type=int, default=20)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--engine", default="native", choices=["native", "python"])
    args = ap.parse_args()
    native = args.engine == "native"
    fg = make_manhattan(n_robots=args.robots, n_poses=args.poses, n_beacons=4, seed=3000)
    bad, long_ = corrupt(fg, 0.05, seed=1)
    relaxed = solve_score_robust(fg, "SOCP", engine="device" if native else "python", lib_path=args.lib)
    prior = relaxed.info["robust"]["weights"]
    kw = dict(engine=args.engine, linear_solver="device", lib_path=args.lib)

    def device_leg():
        t0 = time.perf_counter()
        est, info = refine_estimate_robust(fg, relaxed, range_weights=prior, **kw)
        wall = 1e3 * (time.perf_counter() - t0)
        rb = info["robust"]
        return est, dict(wall_ms=wall, setup_ms=info.get("setup_ms"), solve_ms=info.get("solve_ms"), outer=rb["outer_iterations"],
                         lm_iterations=info["iterations"], pcg_iters=info["pcg_iters"], converged=rb["converged"],
                         flagged=len(rb["outliers"])), rb["weights"]

    def baseline_leg():
        t0 = time.perf_counter()
        est, rec = baseline(fg, relaxed, prior, kw)
        rec["wall_ms"] = 1e3 * (time.perf_counter() - t0)
        return est, rec, rec.pop("weights") * prior

    dev_runs, base_runs = [], []
    for i in range(args.runs + 1):  # (the first of each warms up)
        est_d, rec_d, w_d = device_leg()
        est_b, rec_b, w_b = baseline_leg()
        if i:
            dev_runs.append(rec_d)
            base_runs.append(rec_b)
    planted_found = dict(device=int(np.count_nonzero(w_d[bad] < 0.5)), baseline=int(np.count_nonzero(w_b[bad] < 0.5)))
    worst = max(float(np.max(np.abs(np.asarray(est_d.poses[nm]) - np.asarray(est_b.poses[nm])))) for nm in est_d.poses)
    reweigh = []
    if native:
        prob = _Problem(fg, np.where(prior < MIN_W, MIN_W, prior))
        point = _initial_point(prob, est_d)
        with RobustRefineHandle(prob, args.lib) as h:
            for i in range(args.runs + 2):
                t0 = time.perf_counter()
                h.residuals(point, 1.0, C_IN, C_IN)
                if i > 1:  # (the first call brings the buffers)
                    reweigh.append(1e3 * (time.perf_counter() - t0))
    med = lambda runs, k: float(np.median([r[k] for r in runs]))  # noqa: E731
    rng_ = lambda runs, k: [float(min(r[k] for r in runs)), float(max(r[k] for r in runs))]  # noqa: E731
    rec = dict(
        graph=dict(robots=args.robots, poses=args.poses, beacons=4, seed=3000, ranges=len(fg.range_measurements), planted=len(bad),
                   planted_long=int(long_.sum()), relaxation_flagged=len(relaxed.info["robust"]["outliers"]),
                   relaxation_outer=relaxed.info["robust"]["outer_iterations"]),
        engine=args.engine, schedule=dict(c=C_IN, min_weight=MIN_W, mu_step=MU_STEP, max_outer=MAX_OUTER, inner_iters=INNER, max_iters=MAX_ITERS),
        device=dict(runs=dev_runs, wall_ms_median=med(dev_runs, "wall_ms"), wall_ms_min_max=rng_(dev_runs, "wall_ms")),
        baseline=dict(runs=base_runs, wall_ms_median=med(base_runs, "wall_ms"), wall_ms_min_max=rng_(base_runs, "wall_ms")),
        baseline_over_device=med(base_runs, "wall_ms") / med(dev_runs, "wall_ms"),
        planted_flagged=planted_found, worst_pose_difference_device_vs_baseline=worst,
        reweigh_call_ms=dict(runs=reweigh, median=float(np.median(reweigh)) if reweigh else None),
    )
    if native:
        rec["device"]["solve_ms_per_lm_iteration_median"] = float(np.median([r["solve_ms"] / r["lm_iterations"] for r in dev_runs]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "runs"} if isinstance(v, dict) else v) for k, v in rec.items()}))


if __name__ == "__main__":
    main()
