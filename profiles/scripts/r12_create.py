"""The create path of one library, for comparing two builds (profiles/r12_create_ab.txt).  A fresh process per library:

  python profiles/scripts/r12_create.py dump OUT.txt --lib LIB     every setup array and the default solve's outputs of ten cases, as
                                                                   one line of sha256 per array (timings left out): two builds
                                                                   must write byte-identical files
  python profiles/scripts/r12_create.py creates --lib LIB --case headline|trials16 --source device|derived|uploaded [--reps N]
                                                                   creates only (the workload of a kernel / memory-copy trace)
  python profiles/scripts/r12_create.py time --lib LIB [--reps N]  wall time of the headline create and of the 16-trial create, ms
"""
import argparse, hashlib, os, sys, time
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from score_amd.manhattan import make_manhattan
from score_amd.native import assemble_native, graph_arrays
from score_amd.solver import ConicSolver

SETUP = ("Aptr", "Acol", "G1ptr", "G1col", "G2ptr", "G2split", "G2col", "Kptr", "Kcol", "Kptr_dev", "Kcol_dev", "Hptr", "Hcol",
         "D", "E", "invD", "invE", "qs", "bs", "Aval", "G1val", "G2val", "K0", "K1", "Kval", "setup_scalars")
ENV = {"device": {}, "derived": {"SCORE_HOST_SETUP": "1"}, "uploaded": {"SCORE_HOST_SETUP": "1", "SCORE_NO_DEVICE_RUIZ": "1"}}


def with_env(env, make):
    for k in ("SCORE_HOST_SETUP", "SCORE_NO_DEVICE_RUIZ"):
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return make()
    finally:
        for k in env:
            os.environ.pop(k, None)


def headline():
    return make_manhattan(n_robots=20, n_poses=1000, n_beacons=4, seed=3000)


def trials16():
    return [make_manhattan(n_robots=4, n_poses=1000, n_beacons=4, seed=3000 + t) for t in range(16)]


def dump(args):
    from conftest import graph_by_name, load_fixtures
    fx = load_fixtures()
    qp = lambda g: assemble_native(g, "SOCP", lib_path=args.lib).qp
    batch = [make_manhattan(n_robots=2, n_poses=40, n_beacons=2, seed=121), make_manhattan(n_robots=3, n_poses=70, n_beacons=2, seed=122)]
    long2 = make_manhattan(n_robots=2, n_poses=1500, n_beacons=2, seed=123)
    cases = []
    for nm in ("synth_a", "graph3d"):
        cases += [(f"{nm}/{src}", [qp(graph_by_name(nm, fx))], {}, ENV[src]) for src in ("device", "derived", "uploaded")]
    cases += [("batch/device", [qp(g) for g in batch], {}, {}), ("batch/host_setup", [qp(g) for g in batch], {}, ENV["derived"])]  # (a batch under SCORE_HOST_SETUP: uploaded)
    cases.append(("goats/device", [qp(graph_by_name("goats", fx))], {}, {}))
    cases.append(("2x1500/device", [qp(long2)], {}, {}))
    cases.append(("manhattan/chain_split", [qp(graph_by_name("manhattan", fx))], dict(chain_split=1), {}))
    hq = [qp(headline())]
    cases += [(f"headline/{src}", hq, {}, ENV[src]) for src in ("device", "derived", "uploaded")]
    with open(args.out, "w") as out:
        for name, qps, st, env in cases:
            sv = with_env(env, lambda: ConicSolver(qps, st, lib_path=args.lib))
            try:
                src = int(sv.debug_get("matrix_source")[0])
            except KeyError:  # (a build from before the key)
                src = -1
            print(f"{name}: matrix_source {src}", flush=True)
            for nm in SETUP:
                try:
                    a = np.ascontiguousarray(sv.debug_get(nm))
                except KeyError:
                    out.write(f"{name} {nm} absent\n")
                    continue
                out.write(f"{name} {nm} {a.shape[0]} {hashlib.sha256(a.tobytes()).hexdigest()}\n")
            for p, r in enumerate(sv.solve()):
                for nm, a in (("x", r.x), ("y", r.y), ("s", r.s)):
                    out.write(f"{name} solve{p}.{nm} {a.shape[0]} {hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()}\n")
                out.write(f"{name} solve{p} solved={int(r.solved)} iters={r.info['iters']} newton_iters={r.info['newton_iters']} pobj={float(r.info['pobj']).hex()}\n")
            sv.close()


def maker(case, lib, source):
    graphs = [headline()] if case == "headline" else trials16()
    if source == "device":  # the default create builds the model on the device too (score_create_from_graphs)
        arr = [graph_arrays(g) for g in graphs]
        return lambda: ConicSolver.from_graphs(arr, 0, {}, lib_path=lib)
    qps = [assemble_native(g, "SOCP", lib_path=lib).qp for g in graphs]  # (the host sources start from the program)
    return lambda: with_env(ENV[source], lambda: ConicSolver(qps, {}, lib_path=lib))


def creates(args):
    make = maker(args.case, args.lib, args.source)
    for _ in range(args.reps):
        make().close()


def timed(args):
    for case in ("headline", "trials16"):
        make = maker(case, args.lib, "device")
        make().close()
        ms, setup = [], []
        for _ in range(args.reps):
            t = time.perf_counter(); sv = make(); ms.append(1e3 * (time.perf_counter() - t))
            if case == "headline":  # (setup_ms: the library's own figure, reported with a solve)
                setup.append(float(sv.solve()[0].info["setup_ms"]))
            sv.close()
        if setup:
            print(f"{case} setup_ms median {sorted(setup)[len(setup) // 2]:.3f} min {min(setup):.3f} max {max(setup):.3f} all " + " ".join(f"{v:.2f}" for v in setup), flush=True)
        print(f"{case} create_ms median {sorted(ms)[len(ms) // 2]:.3f} min {min(ms):.3f} max {max(ms):.3f} all " + " ".join(f"{v:.2f}" for v in ms), flush=True)


ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("dump", "creates", "time"))
ap.add_argument("out", nargs="?")
ap.add_argument("--lib", required=True)
ap.add_argument("--case", choices=("headline", "trials16"), default="headline")
ap.add_argument("--source", choices=tuple(ENV), default="device")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
{"dump": dump, "creates": creates, "time": timed}[args.mode](args)
