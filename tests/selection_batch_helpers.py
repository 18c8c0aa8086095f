"""What the batched selection tests share: the candidate lists of the groups of tests/refine_batch_helpers.py (at the
host-refined points of tests/samples_batch_helpers.member_twin) and their dense matrices.

The group A..E lists [37, 0, 9, 260, 1] candidates with k = [12, 0, 9, 32, 1]: B takes no part, D's 260 candidates leave a partly
filled ninth tile and its lanes run past one 256-lane workgroup, and the pair kernel's first workgroup spans A, C and D.  The
group (3D0, 3D1) lists [20, 7] with k = [8, 7]; the group (D, B, C, A) lists [600, 37, 0, 513] with k = [40, 12, 0, 3].  PRECONDITION holds every (member, candidates, k) whose pivot gap the host test
asserts on the dense P -- the GPU lists, and the smaller lists of B and D the issue's table names.  No bound is chosen here:
every one is tests/selection_helpers.py's or tests/leverage_helpers.py's."""
import functools

import numpy as np

from leverage_helpers import pair_list
from refine_batch_helpers import KEYS_2D
from samples_batch_helpers import member_twin
from score_amd.leverage import pair_gradients
from selection_helpers import BASE_PRECISIONS, precisions

KEYS_3D = ("3D0", "3D1")
COUNTS_2D, KS_2D = [37, 0, 9, 260, 1], [12, 0, 9, 32, 1]
COUNTS_3D, KS_3D = [20, 7], [8, 7]
# unequal members that straddle the ownership slots of sel_greedy_workgroup (lane t owns t + 256 m): D's 600 candidates reach the
# third slot in 88 lanes under a coupled sweep of 40 steps, A's 513 reach it in one lane, B stays in the first, C takes no part;
# the pair kernel runs five workgroups (1150 pairs), the first two inside D, the third across D, B and A.  Every member that
# lists candidates is in PRECONDITION below, so every member's order is held to the reference
KEYS_SLOTS, COUNTS_SLOTS, KS_SLOTS = ("D", "B", "C", "A"), [600, 37, 0, 513], [40, 12, 0, 3]
PRECONDITION = [("A", 37, 12), ("B", 5, 5), ("C", 9, 9), ("D", 70, 16), ("D", 260, 32), ("E", 1, 1), ("3D0", 20, 8), ("3D1", 7, 7),
                ("D", 600, 40), ("B", 37, 12), ("A", 513, 3)]


def candidates(key, count):
    """(count, 2) variable ids of the member's candidate list (leverage_helpers.pair_list), or None for none."""
    return np.asarray(pair_list(member_twin(key).ref.prob, count), dtype=np.int32) if count else None


@functools.lru_cache(maxsize=None)
def dense_matrix(key, count):
    """P = G'H^-1 G of the member's candidates from the dense Cholesky factor; computed once and left unchanged."""
    import scipy.linalg as sla

    ref = member_twin(key).ref
    G, _ = pair_gradients(ref.prob, ref.point, candidates(key, count))
    P = G.T @ sla.cho_solve(ref.chol, G)
    P.setflags(write=False)
    return P


def names_of(key, ids):
    prob = member_twin(key).ref.prob
    names = [str(nm) for nm in prob.a["pose_names"]] + [str(nm) for nm in prob.a["landmark_names"]]
    return [(names[a], names[b]) for a, b in ids] if ids is not None else []


__all__ = ["KEYS_2D", "KEYS_3D", "COUNTS_2D", "KS_2D", "COUNTS_3D", "KS_3D", "KEYS_SLOTS", "COUNTS_SLOTS", "KS_SLOTS", "PRECONDITION", "BASE_PRECISIONS", "candidates",
           "dense_matrix", "names_of", "precisions", "member_twin"]
