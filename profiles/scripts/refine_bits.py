"""Every array and counter the refinement, marginals and spectrum entry points return on the tests' small fixtures, for a
bit-for-bit comparison of two builds of the library (a refactor of their kernels or drivers must not move one bit).

  python profiles/scripts/refine_bits.py OUT.npz [--lib PATH]        record
  python profiles/scripts/refine_bits.py OUT.npz --engine python     record the refinement runs only, with engine="python" and
                                                                      SciPy's sparse LU: needs no library and no device
  python profiles/scripts/refine_bits.py --compare A.npz B.npz        compare two records with array_equal (NaNs equal); exit 1
                                                                      if any entry differs or is missing

Runs, each on a fresh handle: refine_estimate on the 2-D members A..E and the 3-D members of tests/refine_batch_helpers.py,
refine_estimate_batch on the 2-D group and on the 3-D group, refine_estimate_robust (both families) on G1..G4 and the clean 3-D
graph of tests/refine_robust_batch_helpers.py, refine_estimate_robust_batch on (G1, G2, G4) and on (G3, clean 3-D).  Recorded per
run: poses and landmarks in the graph's order and every numeric entry of the info record, nested ones included (iteration
counters, costs, gradient norm, mu, weights, residuals, outlier sets); timings (*_ms) are left out.

Then, at the host-refined points of tests/refine_batch_helpers.py (twin_alone): marginal_covariances on A and 3D0 at block
widths 0, 4 and 16, marginal_covariances_batch on the 2-D group and on the 3-D group at widths 4 and 16, information_spectrum
(k = 4) on A.  Recorded per run: the matrices (joint and as computed), residuals, per-column step counts and the numeric info
fields; for the spectrum the values, vectors and residuals.  At the same points: information_spectrum_batch (k = 4) on the
2-D group and on the 3-D group (values, vectors, residuals, iterations, h_max); score_refine_samples on A and 3D0, 5 draws at
block width 4 (right-hand sides, noise, steps, moments, means, residuals, step counts); score_refine_batch_samples at width 4
on the 2-D group with 5, 2, 0, 7, 1 draws and on the 3-D group with 5, 2 and with 0, 5.  And marginal_covariances on the
long-row graph "b" of tests/marginals_helpers.py."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def flatten(prefix, value, out):
    if isinstance(value, dict):
        for k, v in value.items():
            if not str(k).endswith("_ms"):
                flatten(f"{prefix}/{k}", v, out)
    elif isinstance(value, (bool, int, float, np.integer, np.floating, np.bool_)):
        out[prefix] = np.asarray(value)
    elif isinstance(value, np.ndarray) and value.dtype.kind in "fiub":
        out[prefix] = value
    elif isinstance(value, (list, tuple)) and value and all(isinstance(v, (int, float, np.integer, np.floating)) for v in value):
        out[prefix] = np.asarray(value)


def record(lib, engine="native"):
    from refine_batch_helpers import KEYS_2D, arrays_of, group, member
    from refine_robust_batch_helpers import CLEAN3, SCHEDULE, THRESHOLD, graph
    from score_amd.refine import refine_estimate
    from score_amd.refine_batch import refine_estimate_batch
    from score_amd.refine_robust import refine_estimate_robust
    from score_amd.refine_robust_batch import refine_estimate_robust_batch

    out = {}
    single = dict(engine=engine, lib_path=lib, **({"linear_solver": "scipy"} if engine == "python" else {}))
    batch = dict(engine=engine, lib_path=lib)

    def keep(name, fg, res, info):
        poses, lms = arrays_of(fg, res)
        out[f"{name}/poses"], out[f"{name}/landmarks"] = poses, lms
        flatten(f"{name}/info", info, out)

    for k in KEYS_2D + ("3D0", "3D1"):
        fg, start = member(k)
        keep(f"refine_estimate/{k}", fg, *refine_estimate(fg, start, **single))
    for keys in (KEYS_2D, ("3D0", "3D1")):
        fgs, starts = group(keys)
        for k, fg, (res, info) in zip(keys, fgs, refine_estimate_batch(fgs, starts, **batch)):
            keep(f"refine_estimate_batch/{'+'.join(keys)}/{k}", fg, res, info)
    for k in ("G1", "G2", "G3", "G4", CLEAN3):
        fg, start = graph(k)[:2]
        keep(f"refine_estimate_robust/{k}", fg, *refine_estimate_robust(fg, start, inlier_threshold=THRESHOLD[k], robust_loop_closures=True,
                                                                        **single, **SCHEDULE[k]))
    for keys in (("G1", "G2", "G4"), ("G3", CLEAN3)):
        fgs, starts = [graph(k)[0] for k in keys], [graph(k)[1] for k in keys]
        got = refine_estimate_robust_batch(fgs, starts, inlier_threshold=[THRESHOLD[k] for k in keys], robust_loop_closures=True,
                                           **batch, **SCHEDULE[keys[0]])
        for k, fg, (res, info) in zip(keys, fgs, got):
            keep(f"refine_estimate_robust_batch/{'+'.join(keys)}/{k}", fg, res, info)
    if engine == "python":  # (the marginals and the spectrum are the library's)
        return out
    from refine_batch_helpers import twin_alone
    from score_amd.marginals import marginal_covariances
    from score_amd.marginals_batch import marginal_covariances_batch
    from score_amd.spectrum import information_spectrum

    for k in ("A", "3D0"):
        for width in (0, 4, 16):
            _, info = marginal_covariances(member(k)[0], twin_alone(k)[0], joint=True, block_width=width, lib_path=lib)
            flatten(f"marginal_covariances/{k}/width{width}", info, out)
    for keys in (KEYS_2D, ("3D0", "3D1")):
        for width in (4, 16):
            got = marginal_covariances_batch([member(k)[0] for k in keys], [twin_alone(k)[0] for k in keys], joint=True,
                                             block_width=width, lib_path=lib)
            for k, (_, info) in zip(keys, got):
                flatten(f"marginal_covariances_batch/{'+'.join(keys)}/width{width}/{k}", info, out)
    modes, info = information_spectrum(member("A")[0], twin_alone("A")[0], k=4, lib_path=lib)
    for what in ("values", "vectors", "residuals"):
        out[f"information_spectrum/A/{what}"] = getattr(modes, what)
    flatten("information_spectrum/A/info", info, out)

    from marginals_helpers import landmark_names, pose_names, reference
    from score_amd.marginals import _problem_and_point, _select
    from score_amd.refine_batch import RefineBatchHandle
    from score_amd.samples import SamplesHandle
    from score_amd.samples_batch import batch_draws
    from score_amd.spectrum_batch import information_spectrum_batch

    fg, results, _ = reference("b")  # the beacon's rows hold 600 entries: one product tile each
    poses = pose_names(fg)[0]
    _, info = marginal_covariances(fg, results, landmark_names(fg) + [poses[1], poses[150], poses[299]], joint=True, lib_path=lib)
    flatten("marginal_covariances/long_row", info, out)

    drawn = ("rhs", "noise", "steps", "moments", "means", "residuals", "iterations", "converged")

    def at_twin(k):
        prob, point = _problem_and_point(member(k)[0], twin_alone(k)[0], None, None)
        return prob, point, _select(prob, None)[1]

    for k in ("A", "3D0"):  # 5 draws at width 4: the last block is partial, and the probe runs
        prob, point, ids = at_twin(k)
        with SamplesHandle(prob, lib) as h:
            got = h.draw(point, ids, 5, seed=11, block_width=4, with_rhs=True, with_noise=True)
        for what in drawn:
            out[f"posterior_samples/{k}/{what}"] = np.asarray(got[what])
        flatten(f"posterior_samples/{k}/info", got["info"], out)
    # unequal counts at width 4, a member without draws among them: two passes, members drop out after the first
    for keys, counts in ((KEYS_2D, [5, 2, 0, 7, 1]), (("3D0", "3D1"), [5, 2]), (("3D0", "3D1"), [0, 5])):
        probs, points, ids = zip(*[at_twin(k) for k in keys])
        with RefineBatchHandle(list(probs), lib) as h:
            rc, per, rec = batch_draws(h, list(points), list(ids), counts, [11 + i for i in range(len(keys))], block_width=4,
                                       with_rhs=True, with_noise=True)
        name = f"posterior_samples_batch/{'+'.join(keys)}/{'-'.join(map(str, counts))}"
        out[f"{name}/rc"] = np.asarray(rc)
        flatten(f"{name}/info", rec, out)
        for k, got in zip(keys, per):
            for what in drawn + ("determined",):
                out[f"{name}/{k}/{what}"] = np.asarray(got[what])
    for keys in (KEYS_2D, ("3D0", "3D1")):
        got = information_spectrum_batch([member(k)[0] for k in keys], [twin_alone(k)[0] for k in keys], k=4, lib_path=lib)
        for k, (modes, info) in zip(keys, got):
            for what in ("values", "vectors", "residuals"):
                out[f"information_spectrum_batch/{'+'.join(keys)}/{k}/{what}"] = getattr(modes, what)
            flatten(f"information_spectrum_batch/{'+'.join(keys)}/{k}/info", info, out)  # (iterations, h_max, rounds)
    return out


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("only in one record:", k)
    for k in sorted(set(a.files) & set(b.files)):
        if not (a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")):
            worst = float(np.max(np.abs(a[k].astype(float) - b[k].astype(float)))) if a[k].shape == b[k].shape and a[k].size else float("nan")
            print("differs:", k, a[k].shape, b[k].shape, "worst difference", worst)
            bad.append(k)
    print(f"{len(a.files)} entries in {path_a}, {len(b.files)} in {path_b}: {len(bad)} differ or are missing")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--engine", default="native", choices=("native", "python"))
    ap.add_argument("--compare", action="store_true")
    args = ap.parse_args()
    if args.compare:
        if len(args.paths) != 2:
            ap.error("--compare takes two records")
        sys.exit(compare(*args.paths))
    out = record(args.lib, args.engine)
    os.makedirs(os.path.dirname(os.path.abspath(args.paths[0])), exist_ok=True)
    np.savez(args.paths[0], **out)
    print(len(out), "entries ->", args.paths[0])


if __name__ == "__main__":
    main()
