"""The end of a PCG sweep of the ADMM loop on a single-problem handle (run with -m gpu on an MI355X).

The update of an iteration's last PCG step -- xt += a p, kx += a w, x relaxed -- rides on helper workgroups: kx and x on
the iteration's cone launch, xt on the next iteration's INIT launch (which therefore writes its new direction into the
other of the two direction buffers whenever the pending one is its default target), and a measuring iteration relaxes x
on the helpers of its extra STEP launch instead of a launch of its own.  What is computed does not change; these tests
hold the new homes of the update to that on the two shapes at which they can go wrong: one ragged helper item and fewer
cones than one cone workgroup, and several helper items with a ragged last one beside several cone workgroups."""
import functools

import numpy as np
import pytest

from score_amd.assemble import assemble
from score_amd.manhattan import make_manhattan
from score_amd.solver import ConicSolver

BLOCK = 16
SETTINGS = dict(adaptive_rho=0, adaptive_cg=0, check_interval=BLOCK, polish=0)
SHAPES = {
    "1x40": dict(n_robots=1, n_poses=40, n_beacons=2, seed=3, p_range=0.5),
    "2x300": dict(n_robots=2, n_poses=300, n_beacons=2, seed=3, p_range=0.5),
}
ITERATES = ("x", "xt", "kx", "s", "y", "u")
VECS = ITERATES + ("r", "p")
CGS = (1, 2, 3, 4)
HELP_ENTRIES = 3072  # vector entries per helper item of a chain launch
CONE_HELP_ENTRIES = 1536  # ... and per helper workgroup of the cone launch
CONES_PER_WORKGROUP = 128  # of the loop's cone launch on a single-problem handle


@functools.lru_cache(maxsize=None)
def _qp(shape):
    return assemble(make_manhattan(**SHAPES[shape]), "SOCP").qp


def _cones(qp):
    return int(qp.z) + len(qp.soc_dims)


def _vectors(sol, names=VECS):
    return {v: sol.debug_get(v) for v in names}


def _two_blocks(sol):
    sol.reset()
    sol.steps(BLOCK)
    sol.steps(BLOCK)
    return _vectors(sol)


@functools.lru_cache(maxsize=None)
def _twin_blocks(shape, cg, twin_lib):
    """The CPU twin's iterates (double factors) after one and after two blocks of 16: computed once per shape and PCG count."""
    cpu = ConicSolver(_qp(shape), dict(SETTINGS, cg_iters=cg, fac_fp32=0), lib_path=twin_lib)
    try:
        cpu.reset()
        out = []
        for _ in range(2):
            cpu.steps(BLOCK)
            out.append(_vectors(cpu, ITERATES))
        return out
    finally:
        cpu.close()


def _close_to(got, ref, tol, what):
    for v in ref:
        scale = max(1.0, float(np.abs(ref[v]).max()))
        err = float(np.abs(got[v] - ref[v]).max())
        assert err <= tol * scale, (what, v, err, scale)


def test_shapes_reach_every_path():
    small, large = _qp("1x40"), _qp("2x300")
    assert small.n < HELP_ENTRIES and 0 < _cones(small) < CONES_PER_WORKGROUP  # one ragged helper item, less than one cone workgroup
    assert large.n > HELP_ENTRIES and large.n % HELP_ENTRIES != 0             # at least two helper items, the last one ragged
    assert _cones(large) > 2 * CONES_PER_WORKGROUP and _cones(large) % CONES_PER_WORKGROUP != 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_helper_layout_of_a_single_problem_handle(shape, hip_lib):
    qp = _qp(shape)
    sol = ConicSolver(qp, dict(SETTINGS, cg_iters=2), lib_path=hip_lib)
    try:
        assert sol.backend == "hip-gfx950"
        on, n_help, entries, cones_per_wg, cone_helpers = (int(v) for v in sol.debug_get("sweep_help"))
        assert on == 1 and entries == HELP_ENTRIES and cones_per_wg == CONES_PER_WORKGROUP
        assert n_help == -(-qp.n // HELP_ENTRIES) and cone_helpers == -(-qp.n // CONE_HELP_ENTRIES)
    finally:
        sol.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cg", CGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_blocks_repeat_bit_for_bit(shape, cg, hip_lib):
    """reset(), steps(16), steps(16): twice on one handle, once on a second, launched directly and replayed from a captured
    graph.  Every run leaves the same bits in x, xt, kx, s, y, u, r and p -- a helper that read a direction buffer while the
    chains of its launch wrote it would differ from run to run --, and the replayed blocks the same bits as the direct ones."""
    qp = _qp(shape)
    runs = {}
    for use_graph in (0, 1):
        st = dict(SETTINGS, cg_iters=cg, use_graph=use_graph)
        one, two = ConicSolver(qp, st, lib_path=hip_lib), ConicSolver(qp, st, lib_path=hip_lib)
        try:
            assert int(one.debug_get("sweep_help")[0]) == 1
            first, again, other = _two_blocks(one), _two_blocks(one), _two_blocks(two)
            launches = int(one.debug_get("graph_launches")[0])
            assert launches >= 1 if use_graph else launches == 0, (use_graph, launches)
        finally:
            one.close(); two.close()
        for v in VECS:
            assert np.array_equal(first[v], again[v]), (v, use_graph, "second run of the same handle")
            assert np.array_equal(first[v], other[v]), (v, use_graph, "second handle")
        runs[use_graph] = first
    for v in VECS:
        assert np.array_equal(runs[0][v], runs[1][v]), (v, "direct launches against the replayed graph")


@pytest.mark.gpu
@pytest.mark.parametrize("cg", CGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_blocks_match_cpu_twin(shape, cg, hip_lib, twin_lib):
    """Double factors: the iterates after one and after two blocks of 16 against the CPU twin, to the 1e-9 max(1, |v|_inf) of
    test_gpu_parity.py::test_iterates_match_cpu_twin (pure floating-point reassociation)."""
    ref = _twin_blocks(shape, cg, twin_lib)
    for use_graph in (0, 1):
        gpu = ConicSolver(_qp(shape), dict(SETTINGS, cg_iters=cg, fac_fp32=0, use_graph=use_graph), lib_path=hip_lib)
        try:
            assert int(gpu.debug_get("sweep_help")[0]) == 1
            gpu.reset()
            for k in range(2):
                gpu.steps(BLOCK)
                _close_to(_vectors(gpu, ITERATES), ref[k], 1e-9, (use_graph, k))
        finally:
            gpu.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cg", CGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_block_against_single_steps(shape, cg, hip_lib):
    """One block of 16 iterations (15 updates finished by the helpers of the cone and INIT launches) against sixteen
    steps(1) calls (measuring iterations only: every update finished by its own extra STEP), double factors.  The two form
    the step length from differently shaped reductions, so they agree to the tolerance of
    test_operator_identities_gpu.py::test_a_replayed_block_against_single_steps, 1e-9 max(1, |v|_inf), not bit for bit."""
    out = []
    for blocks in ((BLOCK,), (1,) * BLOCK):
        sol = ConicSolver(_qp(shape), dict(SETTINGS, cg_iters=cg, fac_fp32=0, use_graph=0), lib_path=hip_lib)
        try:
            sol.reset()
            for k in blocks:
                sol.steps(k)
            out.append(_vectors(sol, ("x", "y", "s", "xt", "kx")))
        finally:
            sol.close()
    _close_to(out[0], out[1], 1e-9, "block against single steps")


@pytest.mark.gpu
@pytest.mark.parametrize("cg", (1, 2, 3))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_iteration_measuring(shape, cg, hip_lib, twin_lib):
    """check_interval = 1: every iteration is a measuring one, whose extra STEP launch relaxes x on its helper items.  x
    (and xt, kx, which the same items write) equal the twin's to 1e-9 max(1, |v|_inf) after 1 and after 8 more iterations."""
    st = dict(SETTINGS, check_interval=1, cg_iters=cg, fac_fp32=0)
    gpu, cpu = ConicSolver(_qp(shape), dict(st, use_graph=0), lib_path=hip_lib), ConicSolver(_qp(shape), st, lib_path=twin_lib)
    try:
        assert int(gpu.debug_get("sweep_help")[0]) == 1
        gpu.reset(); cpu.reset()
        for k in (1, 8):
            a, b = gpu.steps(k)[0], cpu.steps(k)[0]
            _close_to(_vectors(gpu, ("x", "xt", "kx")), _vectors(cpu, ("x", "xt", "kx")), 1e-9, k)
            np.testing.assert_allclose(a.x, b.x, rtol=0, atol=1e-9 * max(1.0, float(np.abs(b.x).max())))
    finally:
        gpu.close(); cpu.close()


@pytest.mark.gpu
def test_a_handle_of_two_problems_matches_two_single_handles(hip_lib):
    """The lock-step path keeps the deferred update in the right-hand-side kernel and k_xupdate: a handle of both shapes
    reports no sweep helpers, and its solutions after two blocks are those of the two single handles up to the order in
    which the partial sums of r'z and p'w are added (double factors: 1e-9 max(1, |v|_inf))."""
    st = dict(SETTINGS, cg_iters=2, fac_fp32=0)
    qps = [_qp("1x40"), _qp("2x300")]
    both = ConicSolver(qps, st, lib_path=hip_lib)
    try:
        assert int(both.debug_get("sweep_help")[0]) == 0
        both.reset()
        both.steps(BLOCK)
        batch = both.steps(BLOCK)
    finally:
        both.close()
    for qp, got in zip(qps, batch):
        sol = ConicSolver(qp, st, lib_path=hip_lib)
        try:
            sol.reset()
            sol.steps(BLOCK)
            ref = sol.steps(BLOCK)[0]
        finally:
            sol.close()
        _close_to({"x": got.x, "y": got.y, "s": got.s}, {"x": ref.x, "y": ref.y, "s": ref.s}, 1e-9, "batch against single")
