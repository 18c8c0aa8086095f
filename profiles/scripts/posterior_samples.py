"""Posterior samples (score_refine_samples): what a call costs on the headline graph and on a 4 x 1000 world.

  python profiles/scripts/posterior_samples.py [--out profiles/posterior_samples.json] [--rounds 5]
      20 x 1000 poses (seed 3000) and 4 x 1000 poses (seed 2000), 4 beacons, at refine_estimate's point, one handle per world:
      n_samples = 16, 64 and 256 (default variables): the call's rhs_ms / solve_ms / setup_ms and the host clock around it,
      the iterations per block, medians of `rounds` calls after a warm-up;
      what one launch of k_ps_blocks / k_ps_gather / k_ps_moments moves for a full block, from shapes;
      one block of 16 marginal columns on the same handle (the same iteration on unit columns);
      scipy.sparse.linalg.splu(H) and 64 solves with the device's right-hand sides on the host.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.sparse.linalg as spla  # noqa: E402

from score_amd.manhattan import make_manhattan  # noqa: E402
from score_amd.marginals import _problem_and_point, _select  # noqa: E402
from score_amd.refine import refine_estimate  # noqa: E402
from score_amd.samples import SamplesHandle, _moment_sizes, _n_rows  # noqa: E402
from score_amd.solve_score import solve_score  # noqa: E402

WORLDS = {"20x1000": dict(n_robots=20, n_poses=1000, n_beacons=4, seed=3000),
          "4x1000": dict(n_robots=4, n_poses=1000, n_beacons=4, seed=2000)}
COUNTS = (16, 64, 256)


def launch_bytes(prob):
    """Bytes one launch moves for a block of 16 draws, from shapes (2-D: 6 local unknowns per relative pose, 4 per range)."""
    n_rel, n_rng, n_pri, n = len(prob.bi), len(prob.ra), len(prob.pl), int(prob.n)
    gsz = 6 * n_rel + 4 * n_rng + 2 * n_pri
    contributions = gsz - 3 * int(np.count_nonzero(prob.bi == 0)) - 3 * int(np.count_nonzero(prob.tj == 0)) \
        - 2 * int(np.count_nonzero(prob.ra == 0)) - 2 * int(np.count_nonzero(prob.rb == 0))
    graph = n_rel * (2 * 4 + (2 + 4 + 2) * 8 + 2 * 3 * 8) + n_rng * (2 * 4 + 2 * 8 + 2 * 2 * 8) + n_pri * (4 + 3 * 8 + 2 * 8)
    return {
        "gblk_doubles_per_draw": gsz, "noise_rows": _n_rows(prob),
        "k_ps_blocks": int(graph + 16 * gsz * 8),
        "k_ps_gather": int((n + 1) * 4 + contributions * 4 + 16 * contributions * 8 + 16 * n * 8),
        "k_ps_moments": int(16 * n * 8 + 2 * (_moment_sizes(prob)[2] + n) * 8),
    }


def world(name, rounds):
    fg = make_manhattan(**WORLDS[name])
    refined, rinfo = refine_estimate(fg, solve_score(fg, "SOCP"))
    prob, point = _problem_and_point(fg, refined, None, None)
    _, J = prob.residuals(point, jac=True)
    H = (J.T @ J).tocsc()
    names, ids, size, cols = _select(prob, None)
    poses, lms = list(prob.a["pose_names"]), list(prob.a["landmark_names"])
    block_ids = _select(prob, lms[:2] + [poses[len(poses) // 5 * i + 7] for i in range(1, 5)])[1]  # 2 x 2 + 4 x 3 = 16 columns
    out = {"graph": f"make_manhattan({WORLDS[name]}) at refine_estimate's point", "n": int(prob.n), "nnz": int(H.nnz),
           "selected_unknowns": int(len(cols)), "rounds": rounds, "bytes_per_launch_16_draws": launch_bytes(prob), "n_samples": {}}
    rec = {S: [] for S in COUNTS}
    rec["block"] = []
    with SamplesHandle(prob) as h:
        for rnd in range(rounds + 1):  # round 0 warms up
            for S in COUNTS:
                t = time.perf_counter()
                o = h.draw(point, ids, S, seed=0)
                dt = (time.perf_counter() - t) * 1e3
                assert o["rc"] == 0, o["info"]
                if rnd:
                    rec[S].append((dt, o["info"]))
                print(f"{name} round {rnd} {S:3d} draws: {dt:9.2f} ms {o['info']}", flush=True)
            t = time.perf_counter()
            rc, A, bres, steps, conv, binfo = h.columns(point, block_ids, block_width=16)
            dt = (time.perf_counter() - t) * 1e3
            if rnd:
                rec["block"].append((dt, binfo))
            print(f"{name} round {rnd} one block of 16 marginal columns: {dt:9.2f} ms {binfo}", flush=True)
        rhs64 = h.draw(point, ids, 64, seed=0, with_rhs=True)
    for S in COUNTS:
        info = rec[S][-1][1]
        med = {k: float(np.median([r[1][k] for r in rec[S]])) for k in ("setup_ms", "rhs_ms", "solve_ms")}
        out["n_samples"][str(S)] = {
            "call_ms_median": float(np.median([r[0] for r in rec[S]])), "call_ms_all": [float(r[0]) for r in rec[S]],
            **{k + "_median": v for k, v in med.items()}, "batches": info["batches"], "pcg_iters": info["pcg_iters"],
            "iterations_per_block": info["pcg_iters"] / info["batches"], "max_residual": info["max_residual"],
            "rhs_ms_per_block": med["rhs_ms"] / info["batches"], "solve_ms_per_block": med["solve_ms"] / info["batches"],
            "solve_ms_per_iteration": med["solve_ms"] / info["pcg_iters"],
        }
    binfo = rec["block"][-1][1]
    bsolve = float(np.median([r[1]["solve_ms"] for r in rec["block"]]))
    out["one_block_of_16_marginal_columns"] = {"call_ms_median": float(np.median([r[0] for r in rec["block"]])), "solve_ms_median": bsolve,
                                               "pcg_iters": binfo["pcg_iters"], "solve_ms_per_iteration": bsolve / binfo["pcg_iters"]}
    t = time.perf_counter()
    lu = spla.splu(H)
    t_factor = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    X = lu.solve(np.ascontiguousarray(rhs64["rhs"].T))
    t_solve = (time.perf_counter() - t) * 1e3
    out["host_splu"] = {"factor_ms": t_factor, "solve_64_ms": t_solve,
                        "max_abs_difference_to_device_on_selected_unknowns": float(np.max(np.abs(X[cols].T - rhs64["steps"])))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_samples.json"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    doc = {name: world(name, args.rounds) for name in WORLDS}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
