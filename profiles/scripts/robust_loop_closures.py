"""The GNC-TLS device loop with and without the loop closures' family (profiles/robust_loop_closures.json).

  python profiles/scripts/robust_loop_closures.py OUT.json [--lib PATH] [--runs 5] [--legs ranges,both]

ranges: score_robust_solve (the old entry point: also what a library built from an earlier commit exports) on the 20 x 1000
        headline graph with 5 % of the ranges shortened -- the ranges-only loop's overhead per outer iteration,
        (loop wall - creates - solves) / outer iterations, `runs` times after a warm-up;
both:   4 x 1000 poses with 20 loop closures, 4 of them corrupted, plus 5 % shortened ranges: the ranges alone and both
        families through solve_score_robust (needs score_robust_solve_rel).
Run it once per library (a fresh process each) to compare two builds in one session."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from score_amd.manhattan import make_manhattan  # noqa: E402
from score_amd.native import ScoreGraph, score_graph_struct  # noqa: E402
from score_amd.robust import ScoreRobustInfo, ScoreRobustSettings, corrupt_ranges  # noqa: E402
from score_amd.solver import ScoreInfo, ScoreSettings, _f64p, load_library  # noqa: E402


def ranges_only_abi(lib, arrays, runs):
    """score_robust_solve through ctypes, default settings (loop closures: none in this graph)."""
    lib.score_robust_default_settings.argtypes = [C.POINTER(ScoreRobustSettings)]
    lib.score_robust_default_settings.restype = None
    lib.score_robust_solve.argtypes = [C.POINTER(ScoreGraph), C.c_int32, C.POINTER(ScoreSettings), C.POINTER(ScoreRobustSettings)] + \
        [_f64p] * 6 + [C.POINTER(C.c_int32), C.POINTER(ScoreInfo), C.POINTER(ScoreRobustInfo)]
    lib.score_robust_solve.restype = C.c_int
    st, rs = ScoreSettings(), ScoreRobustSettings()
    lib.score_default_settings(C.byref(st))
    lib.score_robust_default_settings(C.byref(rs))
    gs = (ScoreGraph * 1)()
    C.memmove(C.byref(gs[0]), C.byref(score_graph_struct(arrays, 0)), C.sizeof(ScoreGraph))
    nr = len(arrays["rng_a"])
    W, R = np.empty(nr), np.empty(nr)
    infos, rinfos = (ScoreInfo * 1)(), (ScoreRobustInfo * 1)()
    out = []
    for i in range(runs + 1):
        t0 = time.perf_counter()
        rc = lib.score_robust_solve(gs, 1, C.byref(st), C.byref(rs), W.ctypes.data_as(_f64p), R.ctypes.data_as(_f64p),
                                    None, None, None, None, None, infos, rinfos)
        wall = 1e3 * (time.perf_counter() - t0)
        if rc != 0:
            raise RuntimeError(lib.score_last_error().decode())
        ri = rinfos[0]
        if i:  # (the first call warms up)
            out.append(dict(wall_ms=wall, outer=ri.outer_iterations, converged=bool(ri.converged), total_ms=ri.total_ms,
                            setup_ms=ri.setup_ms, solve_ms=ri.solve_ms, flagged=int(np.count_nonzero(W < 0.5)),
                            overhead_ms_per_outer=(ri.total_ms - ri.setup_ms - ri.solve_ms) / ri.outer_iterations))
    return out


def through_python(g, runs, lib_path, **kw):
    from score_amd.robust import solve_score_robust

    out = []
    for i in range(runs + 1):
        t0 = time.perf_counter()
        res = solve_score_robust(g, "SOCP", lib_path=lib_path, **kw)
        wall = 1e3 * (time.perf_counter() - t0)
        ri = res.info["robust"]
        if i:
            out.append(dict(wall_ms=wall, outer=ri["outer_iterations"], converged=ri["converged"], total_ms=ri["total_ms"],
                            setup_ms=ri["setup_ms"], solve_ms=ri["solve_ms"], flagged=len(ri["outliers"]),
                            flagged_loop_closures=ri.get("loop_closure_outliers", np.zeros(0)).tolist(),
                            overhead_ms_per_outer=(ri["total_ms"] - ri["setup_ms"] - ri["solve_ms"]) / ri["outer_iterations"]))
    return out


def spread(runs):
    v = [r["overhead_ms_per_outer"] for r in runs]
    return [min(v), max(v)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--legs", default="ranges,both")
    args = ap.parse_args()
    legs = args.legs.split(",")
    lib = load_library(args.lib)
    rec = {"library": "default" if args.lib is None else os.path.relpath(os.path.abspath(args.lib), ROOT)}
    if "ranges" in legs:
        fg = make_manhattan(n_robots=20, n_poses=1000, n_beacons=4, seed=3000)
        g, bad = corrupt_ranges(fg, 0.05, seed=0)
        runs = ranges_only_abi(lib, g.arrays, args.runs)
        rec["headline_20x1000_5pct_ranges_only"] = dict(ranges=len(g.arrays["rng_a"]), injected=len(bad), runs=runs,
                                                        overhead_ms_per_outer_min_max=spread(runs))
    if "both" in legs:
        from score_amd.robust import corrupt_loop_closures

        fg = make_manhattan(n_robots=4, n_poses=1000, n_beacons=4, seed=3000, n_loop_closures=20)
        g1, bad_lc = corrupt_loop_closures(fg, 4, seed=0)
        g, bad = corrupt_ranges(g1, 0.05, seed=0)
        a = through_python(g, args.runs, args.lib)
        b = through_python(g, args.runs, args.lib, robust_loop_closures=True)
        rec["4x1000_20lc_4bad_5pct"] = dict(
            ranges=len(g.arrays["rng_a"]), injected_ranges=len(bad), injected_loop_closures=bad_lc.tolist(),
            ranges_only=dict(runs=a, overhead_ms_per_outer_min_max=spread(a)),
            both_families=dict(runs=b, overhead_ms_per_outer_min_max=spread(b)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: (v if isinstance(v, str) else {kk: vv for kk, vv in v.items() if "runs" != kk}) for k, v in rec.items()}, default=str)[:3000])


if __name__ == "__main__":
    main()
