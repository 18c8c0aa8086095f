"""Every output of score_refine_batch_samples, score_refine_leverage and score_refine_range_variances on the tests' small
fixtures, for a bit-for-bit comparison of two builds of the library: the three calls share their lane bodies and their draws
with the group forms of include/score_leverage_batch.h, and a refactor for those must not move one bit of them.

  python profiles/scripts/leverage_bits.py OUT.npz [--lib PATH]     record
  python profiles/scripts/leverage_bits.py --compare A.npz B.npz    compare two records (profiles/scripts/refine_bits.py's rule)

Recorded, at the points of tests/samples_batch_helpers.py (member_twin) with the seeds of seed_of:
  score_refine_batch_samples on A..E, 17 draws at width 16 and the counts [17, 5, 0, 16, 1] at width 4, every variable
    selected, right-hand sides and noise asked for; on (A, C), 6 draws at width 4 under max_iters = (the most steps of the
    full run) - 1, so that some draws stay out of the moments;
  score_refine_leverage on a, b, d of tests/marginals_helpers.py: 17 draws with 5 pairs, and a capped run of 6 at width 4;
  score_refine_range_variances on a, b, d: 17 pairs at widths 16 and 3, with the solutions.
The handles bind only the headers both builds have."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from refine_bits import compare, flatten  # noqa: E402


def record(lib):
    from leverage_helpers import pair_list
    from refine_batch_helpers import KEYS_2D
    from samples_batch_helpers import member_twin, seed_of
    from samples_helpers import twin
    from score_amd.bindings import REFINE_BATCH
    from score_amd.leverage import LeverageHandle
    from score_amd.refine_batch import RefineBatchHandle
    from score_amd.samples_batch import batch_draws

    class GroupHandle(RefineBatchHandle):
        headers = (REFINE_BATCH,)

    out = {}

    def keep(name, got):
        for k, v in got.items():
            if k == "info":
                flatten(f"{name}/info", v, out)
            elif v is not None:
                out[f"{name}/{k}"] = np.asarray(v)

    def group_call(name, h, keys, counts, **kw):
        tws = [member_twin(k) for k in keys]
        rc, per, rec = batch_draws(h, [t.ref.point for t in tws], [t.ids for t in tws], counts, [seed_of(k) for k in keys],
                                   with_rhs=True, with_noise=True, **kw)
        out[f"{name}/rc"] = np.asarray(rc)
        flatten(f"{name}/info", rec, out)
        for k, got in zip(keys, per):
            keep(f"{name}/{k}", got)
        return per

    with GroupHandle([member_twin(k).ref.prob for k in KEYS_2D], lib) as h:
        group_call("batch_samples/A-E/17", h, KEYS_2D, 17)
        group_call("batch_samples/A-E/17-5-0-16-1/width4", h, KEYS_2D, [17, 5, 0, 16, 1], block_width=4)
    keys = ("A", "C")
    with GroupHandle([member_twin(k).ref.prob for k in keys], lib) as h:
        full = group_call("batch_samples/A+C/6/width4", h, keys, 6, block_width=4)
        cap = max(int(m["iterations"].max()) for m in full) - 1
        capped = group_call("batch_samples/A+C/6/width4/capped", h, keys, 6, block_width=4, max_iters=cap)
        assert any(not np.all(m["converged"]) for m in capped)
    for k in ("a", "b", "d"):
        tw = twin(k)
        prob, point = tw.ref.prob, tw.ref.point
        with LeverageHandle(prob, lib) as h:
            got = h.leverage(point, pair_list(prob, 5), 17, seed=5)
            keep(f"leverage/{k}/17", got)
            steps = h.leverage(point, pair_list(prob, 5), 6, seed=5, block_width=4)["iterations"]
            keep(f"leverage/{k}/6/width4/capped", h.leverage(point, pair_list(prob, 5), 6, seed=5, block_width=4, max_iters=int(steps.max()) - 1))
            for width in (16, 3):
                keep(f"range_variances/{k}/17/width{width}", h.range_variances(point, pair_list(prob, 17), block_width=width, with_solutions=True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--compare", action="store_true")
    args = ap.parse_args()
    if args.compare:
        if len(args.paths) != 2:
            ap.error("--compare takes two records")
        sys.exit(compare(*args.paths))
    out = record(args.lib)
    os.makedirs(os.path.dirname(os.path.abspath(args.paths[0])), exist_ok=True)
    np.savez(args.paths[0], **out)
    print(len(out), "entries ->", args.paths[0])


if __name__ == "__main__":
    main()
