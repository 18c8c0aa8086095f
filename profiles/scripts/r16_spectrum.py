"""Lowest eigenpairs of the information matrix (score_refine_spectrum): iterations on the test graphs, time on the headline
graph and on a 4 x 1000 world.

  python profiles/scripts/r16_spectrum.py [--out profiles/r16_spectrum.json] [--rounds 5]
      shapes:  the graphs of tests/test_spectrum_gpu.py: iterations and the figures of the checks A-D;
      speed:   20 x 1000 poses (seed 3000) and 4 x 1000 poses (seed 2000), 4 beacons, at refine_estimate's point:
               information_spectrum's device call for k = 8 and 16 on one handle, medians of `rounds` calls after a warm-up,
               host clock around the (synchronous) call; one block of 16 marginal columns on the same handle as the yardstick;
               scipy.sparse.linalg.eigsh(H, k, sigma=-shift * h_max) on the host for the same H (the only baseline there is);
      trace:   on the 4 x 1000 world, the share of trace(Sigma) that the bracket's lower part reaches, over a sample of
               poses whose covariances come from score_refine_marginals.
  python profiles/scripts/r16_spectrum.py --profile-only 16
      a few calls on the headline graph and nothing else: the run to put under rocprofv3 --kernel-trace --stats for
      k_sp_gram and k_sp_combine.
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
import scipy.sparse.linalg as spla  # noqa: E402

from score_amd.manhattan import make_manhattan  # noqa: E402
from score_amd.marginals import _problem_and_point, _select  # noqa: E402
from score_amd.refine import refine_estimate  # noqa: E402
from score_amd.solve_score import solve_score  # noqa: E402
from score_amd.spectrum import Modes, SpectrumHandle, _layout, covariance_bracket  # noqa: E402

REL_TOL, SHIFT, MAX_ITERS = 1e-9, 1e-8, 200
WORLDS = {"20x1000": dict(n_robots=20, n_poses=1000, n_beacons=4, seed=3000),
          "4x1000": dict(n_robots=4, n_poses=1000, n_beacons=4, seed=2000)}


def shapes():
    from spectrum_helpers import check_modes, reference

    out = []
    for key, ks in (("2x20", (1, 8, 16)), ("long_rows", (8,)), ("a", (8,)), ("c", (4,)), ("d", (8,)), ("degenerate", (8,))):
        fg, results, ref = reference(key)
        with SpectrumHandle(ref.prob) as h:
            for k in ks:
                rc, values, Vt, res, info = h.spectrum(ref.point, k, REL_TOL, MAX_ITERS, SHIFT)
                fig = {"graph": key, "n": int(ref.n), "k": k}
                if key != "degenerate":
                    fig, _ = check_modes(ref, k, values, Vt.T, REL_TOL, key)
                fig.update(rc=rc, iterations=info["iterations"], solve_ms=info["solve_ms"], lambda_0=float(values[0]))
                out.append(fig)
    return out


def world(name):
    fg = make_manhattan(**WORLDS[name])
    res = solve_score(fg, "SOCP")
    refined, rinfo = refine_estimate(fg, res)
    prob, point = _problem_and_point(fg, refined, None, None)
    _, J = prob.residuals(point, jac=True)
    H = (J.T @ J).tocsc()
    return fg, prob, point, H, rinfo


def speed(name, rounds):
    fg, prob, point, H, rinfo = world(name)
    n, nnz = int(prob.n), int(H.nnz)
    h_max = float(H.diagonal().max())
    out = {"graph": f"make_manhattan({WORLDS[name]}) at refine_estimate's point", "n": n, "nnz": nnz, "h_max": h_max,
           "rounds": rounds, "refine": {k: rinfo[k] for k in ("iterations", "pcg_iters", "cost_final")}, "k": {}}
    poses, lms = list(prob.a["pose_names"]), list(prob.a["landmark_names"])
    block_vars = lms[:2] + [poses[len(poses) // 5 * i + 7] for i in range(1, 5)]  # 2 x 2 + 4 x 3 = 16 columns
    _, block_ids, _, block_cols = _select(prob, block_vars)
    assert len(block_cols) == 16
    times = {8: [], 16: [], "block": []}
    last = {}
    with SpectrumHandle(prob) as h:
        for rnd in range(rounds + 1):  # round 0 warms up
            for k in (8, 16):
                t = time.perf_counter()
                rc, values, Vt, res, info = h.spectrum(point, k, REL_TOL, MAX_ITERS, SHIFT)
                dt = (time.perf_counter() - t) * 1e3
                if rnd:
                    times[k].append(dt)
                last[k] = (rc, values, Vt, res, info)
                print(f"{name} round {rnd} k {k:2d}: {dt:9.2f} ms rc {rc} {info}", flush=True)
            t = time.perf_counter()
            rc, A, bres, steps, conv, binfo = h.columns(point, block_ids, block_width=16)
            dt = (time.perf_counter() - t) * 1e3
            if rnd:
                times["block"].append(dt)
            print(f"{name} round {rnd} one block of 16 marginal columns: {dt:9.2f} ms {binfo}", flush=True)
        for k in (8, 16):
            rc, values, Vt, res, info = last[k]
            t = time.perf_counter()
            w = spla.eigsh(H, k=k, sigma=-SHIFT * h_max, which="LM", return_eigenvectors=True)[0]
            host_ms = (time.perf_counter() - t) * 1e3
            w = np.sort(w)
            out["k"][str(k)] = {
                "rc": rc, "iterations": info["iterations"], "unconverged": info["unconverged"],
                "call_ms_median": float(np.median(times[k])), "call_ms_all": [float(x) for x in times[k]],
                "setup_ms_last": info["setup_ms"], "solve_ms_last": info["solve_ms"], "max_residual_over_tol": float(np.max(res) / (REL_TOL * h_max)),
                "values": [float(v) for v in values], "eigsh_host_ms": host_ms, "max_abs_value_difference_to_eigsh": float(np.max(np.abs(values - w))),
            }
        out["one_block_of_16_marginal_columns"] = {"call_ms_median": float(np.median(times["block"])), "pcg_iters": binfo["pcg_iters"],
                                                   "solve_ms_last": binfo["solve_ms"], "setup_ms_last": binfo["setup_ms"]}
        # what one launch moves, from shapes: Gram reads the six blocks (and writes its partial matrices), combine reads six
        # and writes four
        wgs = min((n + 31) // 32, 128)
        out["k_sp_gram_bytes"] = int(96 * n * 8 + wgs * 2 * 48 * 48 * 8)
        out["k_sp_combine_bytes"] = int(160 * n * 8 + 2 * ((n + 255) // 256) * 48 * 16 * 8)
        if name == "4x1000":  # the share of trace(Sigma) the lower part of the bracket reaches, over a sample of poses
            names, first, size = _layout(prob)
            sample = [poses[i] for i in range(37, len(poses), 97) if i % 1000 != 0]
            _, ids, _, cols = _select(prob, sample)
            share = {}
            rc, A, cres, steps, conv, cinfo = h.columns(point, ids, block_width=16)
            assert rc == 0
            off = np.concatenate([[0], np.cumsum([3] * len(sample))])
            total = float(sum(np.trace(A[off[i]:off[i + 1], off[i]:off[i + 1]]) for i in range(len(sample))))
            for k in (8, 16):
                rc, values, Vt, res, info = last[k]
                modes = Modes(values, Vt.T, res, names, first, size, info["h_max"], REL_TOL, [])
                for m in sorted({4, 8, k}):
                    if m + 1 > k:
                        continue
                    sub = Modes(values[:m + 1], Vt.T[:, :m + 1], res[:m + 1], names, first, size, info["h_max"], REL_TOL, [])
                    br = covariance_bracket(sub, sample)
                    share[f"{m} modes"] = float(sum(np.trace(br[nm][0]) for nm in sample)) / total
                br = covariance_bracket(modes, sample)
                share[f"{k - 1} modes"] = float(sum(np.trace(br[nm][0]) for nm in sample)) / total
            out["trace_share"] = {"sampled_poses": len(sample), "trace_sigma_of_sample": total, "columns_ms": cinfo["solve_ms"], "lower_part_share": share}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_spectrum.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile-only", type=int, default=None, metavar="K")
    ap.add_argument("--skip-shapes", action="store_true")
    args = ap.parse_args()
    if args.profile_only is not None:
        fg, prob, point, H, _ = world("20x1000")
        with SpectrumHandle(prob) as h:
            for _ in range(3):
                rc, *_rest, info = h.spectrum(point, args.profile_only, REL_TOL, MAX_ITERS, SHIFT)
                print(rc, info, flush=True)
        return
    doc = {}
    if not args.skip_shapes:
        doc["shapes"] = shapes()
    doc["speed"] = {name: speed(name, args.rounds) for name in WORLDS}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
