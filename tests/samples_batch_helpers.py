"""What the batched posterior-sample tests share: one ``samples_helpers.Twin`` per member, computed once and left unchanged.

Members A..E, 3D0 and 3D1 are those of tests/refine_batch_helpers.py at their host-refined points (``twin_alone``), where every
member's H is positive definite; "b" and "c" are the graphs of tests/marginals_helpers.py at their own test points (b: one
beacon ranged from 300 poses, the long contribution list; c: one chain of 1100 poses, the join level).  Every bound a test
applies is the derived one of tests/samples_helpers.py -- no tolerance is chosen here."""
import functools

import numpy as np

from marginals_helpers import Reference
from refine_batch_helpers import member, twin_alone
from samples_helpers import Twin, twin

OUTPUTS = ("moments", "means", "steps", "rhs", "noise", "residuals", "iterations", "converged", "determined", "rc")
DISTRIBUTION_SEED = 0  # graph i draws from the stream of DISTRIBUTION_SEED + i: the host test holds the python engine to it


@functools.lru_cache(maxsize=None)
def member_twin(key):
    if key in ("b", "c"):
        return twin(key)
    fg, pt = member(key)[0], twin_alone(key)[0]
    return Twin(fg, pt, Reference(fg, pt))


def seed_of(key):
    """A distinct noise stream per member."""
    return 100 + 7 * sum(ord(ch) for ch in key)


def group_draws(handle, keys, n_samples, seeds=None, **kw):
    """One ``score_refine_batch_samples`` call on a handle over ``keys``: every variable of every member selected, the
    diagnostics asked for.  Returns (rc, per-member dicts, info)."""
    tws = [member_twin(k) for k in keys]
    seeds = [seed_of(k) for k in keys] if seeds is None else seeds
    return handle.samples([t.ref.point for t in tws], [t.ids for t in tws], n_samples, seeds, with_rhs=True, with_noise=True, **kw)


def solve_bound(tw, out, b_py):
    """The per-draw bound ``samples_helpers.check_solve`` holds || delta_dev - delta_ref ||_2 to (its module docstring), for
    comparing two device results through the reference they share."""
    _, rho_ref, rounding = tw.solve(b_py)
    db = np.linalg.norm(out["rhs"] - b_py, axis=1)
    return (out["residuals"] + rounding + rho_ref + db) / tw.ref.lambda_min


def same_bits(a, b, label, keys=OUTPUTS):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{label}: {k}")
