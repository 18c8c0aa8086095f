"""Everything score_robust_solve_rel returns, as one file of raw bytes, for comparing two builds of the library bit for bit
(profiles/r10_robust_family_ab.txt).

  python profiles/scripts/robust_family_dump.py OUT.bin [--lib PATH]

Run it once per library, a fresh process each; `cmp` the files.  Per case: weights, residuals, rel_weights, rel_residuals, poses,
relaxed, landmarks, ranges, degenerate, and the fields of score_robust_info and score_info that are not timings.  The cases are
those of tests/test_robust_gpu.py and tests/test_robust_loop_closures_gpu.py that reach every path of the loop."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from score_amd import compat  # noqa: E402
from score_amd.manhattan import make_manhattan, make_manhattan_3d  # noqa: E402
from score_amd.native import ArrayGraph, ScoreGraph, graph_arrays, score_graph_struct  # noqa: E402
from score_amd.robust import (ScoreRobustInfo, ScoreRobustSettings, _bind, corrupt_loop_closures, corrupt_ranges,  # noqa: E402
                              n_loop_closures_of)
from score_amd.solver import ScoreInfo, ScoreSettings, _f64p, _i32p, load_library  # noqa: E402

G2 = dict(n_robots=1, n_poses=80, n_beacons=3, p_range=0.5, sigma_range=0.1, n_loop_closures=10)
G3 = dict(n_robots=1, n_poses=40, n_beacons=3, p_range=0.5, sigma_range=0.1, n_loop_closures=6)
TIMINGS = ("setup_ms", "solve_ms", "total_ms")


def arrays_of(g):
    return g.arrays if isinstance(g, ArrayGraph) else graph_arrays(g)


def indexing_graph(n_lc, seed):
    fg = make_manhattan(n_robots=2, n_poses=40, n_beacons=3, p_range=0.5, sigma_range=0.1, seed=seed, n_loop_closures=n_lc)
    Ti = fg.pose_variables[0][0].transformation_matrix
    Tj = fg.pose_variables[1][7].transformation_matrix
    rel = np.linalg.inv(Ti) @ Tj
    fg.loop_closure_measurements.append(compat.PoseMeasurement2D(
        "A0", "B7", float(rel[0, 2]), float(rel[1, 2]), float(np.arctan2(rel[1, 0], rel[0, 0])), 1e4, 2.5e5))
    return corrupt_loop_closures(fg, 3, seed=seed)[0]


def cases():
    """(name, graphs, families or None for score_robust_solve, environment)"""
    from conftest import graph_3d

    g5 = corrupt_ranges(corrupt_loop_closures(make_manhattan(seed=5, **G2), 2, seed=5)[0], 0.05, seed=5)[0]
    g3 = corrupt_loop_closures(make_manhattan(seed=3, **G2), 2, seed=3)[0]
    r60 = corrupt_ranges(make_manhattan(n_robots=2, n_poses=60, n_beacons=3, p_range=0.5, sigma_range=0.1, seed=2), 0.08, seed=2)[0]
    yield "indexing_71_6_131", [indexing_graph(n, 40 + i) for i, n in enumerate((70, 5, 130))], 2, {}
    yield "g2_seed5_both", [g5], 3, {}
    yield "g3_seed2_closures", [corrupt_loop_closures(make_manhattan_3d(seed=2, **G3), 1, seed=2)[0]], 2, {}
    yield "graph3d_both", [graph_3d(n=40)], 3, {}
    yield "ranges_2x60_old_entry", [r60], None, {}
    yield "ranges_2x60_families_1", [r60], 1, {}
    yield "lockstep_16", [corrupt_loop_closures(make_manhattan(seed=500 + s, **G2), 2 if s % 2 else 0, seed=s)[0] for s in range(16)], 2, {}
    yield "g2_seed3_host_assemble", [g3], 2, {"SCORE_HOST_ASSEMBLE": "1"}
    yield "g2_seed3_host_setup", [g3], 2, {"SCORE_HOST_SETUP": "1"}
    yield "ranges_2x60_both_no_closures", [r60], 3, {}


def run(lib, graphs, families):
    arrays = [arrays_of(g) for g in graphs]
    count, d = len(arrays), int(arrays[0]["dim"])
    st, rs = ScoreSettings(), ScoreRobustSettings()
    lib.score_default_settings(C.byref(st))
    lib.score_robust_default_settings(C.byref(rs))
    gs = (ScoreGraph * count)()
    for i, a in enumerate(arrays):
        C.memmove(C.byref(gs[i]), C.byref(score_graph_struct(a, 0)), C.sizeof(ScoreGraph))
    Np = sum(len(a["pose_names"]) for a in arrays)
    Nl = sum(len(a["landmark_names"]) for a in arrays)
    Nr = sum(len(a["rng_a"]) for a in arrays)
    Nc = sum(n_loop_closures_of(a) for a in arrays) if families and families & 2 else 0
    out = dict(weights=np.zeros(max(1, Nr)), residuals=np.zeros(max(1, Nr)), rel_weights=np.zeros(max(1, Nc)),
               rel_residuals=np.zeros(max(1, Nc)), poses=np.zeros((Np, d + 1, d + 1)), relaxed=np.zeros((Np, d, d + 1)),
               landmarks=np.zeros((max(1, Nl), d)), ranges=np.zeros((max(1, Nr), 1)))
    F = np.zeros(Np, dtype=np.int32)
    infos, rinfos = (ScoreInfo * count)(), (ScoreRobustInfo * count)()
    p = lambda x: x.ctypes.data_as(_f64p)  # noqa: E731
    head = (gs, count, C.byref(st), C.byref(rs))
    tail = (p(out["poses"]), p(out["relaxed"]), p(out["landmarks"]), p(out["ranges"]), F.ctypes.data_as(_i32p), infos, rinfos)
    if families is None:
        rc = lib.score_robust_solve(*head, p(out["weights"]), p(out["residuals"]), *tail)
    else:
        rc = lib.score_robust_solve_rel(*head, families, 3.0, p(out["weights"]), p(out["residuals"]), p(out["rel_weights"]),
                                        p(out["rel_residuals"]), *tail)
    if rc != 0:
        raise RuntimeError(lib.score_last_error().decode())
    out["degenerate"] = F
    for rec, cls in ((rinfos, ScoreRobustInfo), (infos, ScoreInfo)):
        for key, _ in cls._fields_:
            if key not in TIMINGS:
                out[cls.__name__ + "." + key] = np.array([getattr(r, key) for r in rec])
    return out, [r.outer_iterations for r in rinfos]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    lib = _bind(load_library(args.lib))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "wb") as f:
        for name, graphs, families, env in cases():
            os.environ.update(env)
            try:
                out, outer = run(lib, graphs, families)
            finally:
                for k in env:
                    del os.environ[k]
            for key, v in out.items():
                f.write(f"{name}/{key} {v.dtype} {v.shape}\n".encode())
                f.write(np.ascontiguousarray(v).tobytes())
            print(name, "outer iterations", outer, flush=True)


if __name__ == "__main__":
    main()
