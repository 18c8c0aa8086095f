"""Marginal covariances (score_refine_marginals): accuracy on the test graphs and time on the headline graph.

  python profiles/scripts/r11_marginals.py [--out profiles/r11_marginals.json] [--rounds 5]
      accuracy: the graphs of tests/test_marginals_gpu.py against the dense Cholesky reference (the bound of
                tests/marginals_helpers.py relative to max |Sigma|, the worst relative error of a diagonal entry);
      speed:    20 x 1000 poses, 4 beacons at the refined estimate, the default request (4 beacons + 20 last poses = 68
                columns) with block_width 16, 8, 4 and 0 (the single-right-hand-side PCG per column), the variants
                alternating on one handle after a warm-up round, host clock around the (synchronous) call.
  python profiles/scripts/r11_marginals.py --profile-only 16
      a few calls at one width and nothing else: the run to put under rocprofv3 --kernel-trace --stats for k_mv_product.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from score_amd.manhattan import make_manhattan  # noqa: E402
from score_amd.marginals import MarginalsHandle, _problem_and_point, _select, marginal_covariances  # noqa: E402
from score_amd.refine import refine_estimate  # noqa: E402
from score_amd.solve_score import solve_score  # noqa: E402


def accuracy():
    from marginals_helpers import check_columns, landmark_names, pose_names, reference

    out = []
    for key in "abcd":
        fg, results, ref = reference(key)
        poses = pose_names(fg)
        if key == "a":
            variables = [nm for ch in poses for nm in ch][1:] + landmark_names(fg)
        elif key == "b":
            variables = landmark_names(fg) + [poses[0][1], poses[0][150], poses[0][299]]
        elif key == "c":
            variables = landmark_names(fg) + [poses[0][550], poses[0][1099]]
        else:
            variables = None
        for width in ((16, 4, 0) if key == "a" else (16,)):
            _, info = marginal_covariances(fg, results, variables, joint=True, block_width=width)
            _, cols = ref.columns(variables)
            fig, _, _ = check_columns(ref, cols, info["joint_raw"], info["residuals"], f"({key}) width {width}")
            fig.update(block_width=width, pcg_iters=info["pcg_iters"], batches=info["batches"], solve_ms=info["solve_ms"])
            out.append(fig)
    return out


def headline():
    fg = make_manhattan(n_robots=20, n_poses=1000, n_beacons=4, seed=3000)
    res = solve_score(fg, "SOCP")
    refined, rinfo = refine_estimate(fg, res)
    prob, point = _problem_and_point(fg, refined, None, None)
    _, ids, size, cols = _select(prob, None)
    _, J = prob.residuals(point, jac=True)
    nnz = int((J.T @ J).nnz)
    return prob, point, ids, len(cols), nnz, rinfo


def speed(rounds):
    prob, point, ids, ncol, nnz, rinfo = headline()
    widths = [16, 8, 4, 0]
    times = {w: [] for w in widths}
    last = {}
    with MarginalsHandle(prob) as h:
        for rnd in range(rounds + 1):  # round 0 warms up
            for w in widths:
                t = time.perf_counter()
                rc, A, res, steps, conv, info = h.columns(point, ids, block_width=w)
                dt = (time.perf_counter() - t) * 1e3
                assert rc == 0, (w, info)
                if rnd:
                    times[w].append(dt)
                last[w] = dict(info, max_steps=int(steps.max()), asymmetry=float(np.max(np.abs(A - A.T))))
                print(f"round {rnd} width {w:2d}: {dt:9.2f} ms  (setup {info['setup_ms']:.2f}, solve {info['solve_ms']:.2f}) "
                      f"pcg_iters {info['pcg_iters']} batches {info['batches']} max residual {info['max_residual']:.2e}", flush=True)
    seq = float(np.median(times[0]))
    out = {"graph": "make_manhattan(n_robots=20, n_poses=1000, n_beacons=4, seed=3000) at refine_estimate's point",
           "n": int(prob.n), "nnz": nnz, "columns": ncol, "rounds": rounds, "refine": {k: rinfo[k] for k in ("iterations", "pcg_iters", "cost_final")},
           "widths": {}}
    for w in widths:
        med = float(np.median(times[w]))
        out["widths"][str(w)] = {"call_ms_median": med, "call_ms_min": float(np.min(times[w])), "call_ms_all": [float(x) for x in times[w]],
                                 "solve_ms_last": last[w]["solve_ms"], "setup_ms_last": last[w]["setup_ms"], "pcg_iters": last[w]["pcg_iters"],
                                 "batches": last[w]["batches"], "max_steps_of_a_column": last[w]["max_steps"],
                                 "max_residual": last[w]["max_residual"], "sequential_over_this": seq / med}
    # what one k_mv_product launch moves, from shapes: the matrix once (values, columns, row pointers) + W operand vectors
    # read + W product vectors written
    out["k_mv_product_bytes"] = {str(w): int(nnz * 12 + (prob.n + 1) * 4 + 2 * w * prob.n * 8) for w in (16, 8, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_marginals.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile-only", type=int, default=None, metavar="WIDTH")
    ap.add_argument("--skip-accuracy", action="store_true")
    args = ap.parse_args()
    if args.profile_only is not None:
        prob, point, ids, ncol, nnz, _ = headline()
        with MarginalsHandle(prob) as h:
            for _ in range(3):
                rc, *_rest, info = h.columns(point, ids, block_width=args.profile_only)
                print(rc, info, flush=True)
        return
    doc = {}
    if not args.skip_accuracy:
        doc["accuracy"] = accuracy()
    doc["speed"] = speed(args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
