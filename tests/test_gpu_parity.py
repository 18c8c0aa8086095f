"""GPU parity tests (run with -m gpu on an MI355X).  Everything goes through the
C ABI of include/score_hip.h into the HIP library; the oracle (CPU twin, Newton
solve, golden fixtures, KKT certificate) is only the checker."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN_NAMES, compare_residuals_with_golden, compare_with_golden, graph_by_name, load_golden
from oracle import score_oracle as so
from score_amd.assemble import assemble
from score_amd.manhattan import make_config, make_manhattan
from score_amd.solve_score import (
    solve_problem_with_intermediate_iterates,
    solve_score,
    solve_score_batch,
)
from score_amd.solver import ConicSolver

pytestmark = pytest.mark.gpu

VECS = ["x", "xt", "s", "y", "u", "r", "z", "p", "w", "kx"]


def _hip_only(hip_lib):
    import ctypes

    lib = ctypes.CDLL(hip_lib)
    lib.score_backend.restype = ctypes.c_char_p
    assert lib.score_backend().decode() == "hip-gfx950"


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("radix,cg", [(4, 2), (2, 1), (4, 3), (3, 4)])
@pytest.mark.parametrize("name", ["manhattan", "synth_b"])
def test_iterates_match_cpu_twin(name, radix, cg, fp32, fixtures, hip_lib, twin_lib):
    """Kernel-level parity: after k ADMM iterations every internal vector of the
    HIP solver equals the CPU twin's (same algorithm, loops instead of kernels).
    fac_fp32 = 0 (chain factors in double): differences are pure floating-point reassociation, 1e-9.
    fac_fp32 = 1 (the default: factors kept to float precision on both sides, the LDS-resident chain
    kernel streams the 4-byte copies): host and device factorisations round a few entries to
    neighbouring floats, so the iterates agree to float eps times the conditioning of the chain blocks:
    2e-5 on the iterates (x itself to 1e-6), 1e-4 on the PCG internals.
    synth_b has loop closures: its preconditioner carries the link correction (score_link.hpp), restated
    independently in the twin (dense capacitance matrix, LU) -- with double factors the two agree to the same
    1e-9; with float factors the correction y - Z t cancels leading digits of two float-accurate terms, so the
    preconditioned directions (and with a fixed PCG count the iterates) agree to 1e-3 only.
    check_interval = 16 keeps every steps(k) one block: steps(9) is one run of 9 iterations with 8 deferred end-of-PCG
    updates (it was 5 + 4 under check_interval = 5), and the last block, 16 iterations, is long enough to be replayed from
    a captured graph (HipBackend::graph_min_iters): with use_graph = 1 the handle must report the launch, with
    use_graph = 0 none.
    After that block (31 iterations in all) the iterates x, xt, s, y, u and kx are held to the tolerances above.  The PCG
    internals r, z, p, w have by then decayed -- synth_b: |p|_inf from 608 to 0.22, |r|_inf from 1.8 to 1.9e-4 -- while the
    terms they cancel from (|kx|_inf = 4e2) have not, so their rounding no longer shrinks with them and the tolerance
    relative to max(1, |v|_inf) of the vector itself asks for more than the twin defines: on synth_b with radix 4, cg 2
    and double factors four builds of the twin (-march=native on two processors, without fused multiply-adds, generic)
    differ from one another by 6e-10 .. 1.0e-9 in p, and the device differs from them by 9.2e-10 .. 1.54e-9 (use_graph 0
    and 1 bit-identical) -- against 1e-9 the case passes or fails with the machine the twin was compiled on.  For this
    block these four vectors are therefore measured against the largest |v|_inf the vector has had in the run (the scale
    it had before it cancelled; same factors 1e-9 / 1e-4 / 1e-2), so that the absolute tolerance of the block does not fall
    below that of the blocks before it; the blocks of 1, 5 and 9 iterations keep the vector's own scale."""
    _hip_only(hip_lib)
    qp = assemble(graph_by_name(name, fixtures), "SOCP").qp
    st = dict(chain_radix=radix, cg_iters=cg, adaptive_cg=0, adaptive_rho=0, check_interval=16, fac_fp32=fp32)
    links = name == "synth_b"
    tol = (1e-3 if links else 2e-5) if fp32 else 1e-9
    xtol = (1e-3 if links else 1e-6) if fp32 else 1e-9
    for use_graph in (0, 1):
        gpu = ConicSolver(qp, dict(use_graph=use_graph, **st), lib_path=hip_lib)
        cpu = ConicSolver(qp, st, lib_path=twin_lib)
        assert gpu.backend == "hip-gfx950" and cpu.backend == "cpu-twin"
        # the product runs the problem row-replicated (K_row streamed once for both rows of the pose matrices);
        # the twin applies the full K the problem defines
        assert gpu.debug_get("rep")[0] == 2 and cpu.debug_get("rep")[0] == 1
        gpu.reset(); cpu.reset()
        peak = {v: 0.0 for v in VECS}  # largest |v|_inf of the twin's vector over the blocks run so far
        for k in (1, 5, 9, 16):
            a, b = gpu.steps(k)[0], cpu.steps(k)[0]
            for v in VECS:
                ga, gb = gpu.debug_get(v), cpu.debug_get(v)
                peak[v] = max(peak[v], float(np.abs(gb).max()))
                scale = max(1.0, peak[v] if (k == 16 and v in ("r", "z", "p", "w")) else np.abs(gb).max())
                # (fp32 factors: the PCG internals r, z, p, w are small differences of large terms -- 1e-4)
                vtol = (1e-2 if links else 1e-4) if (fp32 and v in ("r", "z", "p", "w")) else tol
                assert np.abs(ga - gb).max() <= vtol * scale, (v, k, use_graph, np.abs(ga - gb).max(), scale)
            np.testing.assert_allclose(a.x, b.x, rtol=0, atol=xtol * max(1.0, np.abs(b.x).max()))
            assert a.info["res_pri"] == pytest.approx(b.info["res_pri"], rel=1e-2 if fp32 else 1e-6, abs=1e-12)
            assert a.info["res_dual"] == pytest.approx(b.info["res_dual"], rel=1e-2 if fp32 else 1e-6, abs=1e-2 if fp32 else 1e-9)
            assert a.info["pobj"] == pytest.approx(b.info["pobj"], rel=tol, abs=tol)
        launches = int(gpu.debug_get("graph_launches")[0])
        assert launches >= 1 if use_graph else launches == 0, (use_graph, launches)
        gpu.close(); cpu.close()


def test_band_view_and_split_long_rows_against_the_csr_stream(fixtures, hip_lib, monkeypatch):
    """K through its band view (score_band.hpp: chain rows as value-slot pairs without column indices, remainder
    entries, diagonal tiles) and long rows in segments (the last segment to arrive adds the segment sums in segment
    order) against the plain CSR-stream kernels (SCORE_NO_BAND; the long rows are split there too): the same products up to the order
    of a row's additions -- iterates of a lock-step batch of 2-D graphs (a landmark seen by > 512 ranges: split rows) and
    of a 3-D graph (three replicas, 4 x 4 blocks: six slot pairs) to 1e-10; repeated runs of one handle are bit-identical
    (the combine order of the segments does not depend on who arrives last)."""
    _hip_only(hip_lib)
    qps2 = [assemble(make_manhattan(n_robots=4, n_poses=1500 + 200 * k, n_beacons=2, seed=60 + k, p_range=0.3), "SOCP").qp for k in range(2)]
    qp3 = assemble(graph_by_name("graph3d", fixtures), "SOCP").qp
    st = dict(adaptive_cg=0, check_interval=5, polish=0)
    for qps in (qps2, [qp3]):
        monkeypatch.delenv("SCORE_NO_BAND", raising=False)
        new = ConicSolver(qps, st, lib_path=hip_lib)
        again = ConicSolver(qps, st, lib_path=hip_lib)
        monkeypatch.setenv("SCORE_NO_BAND", "1")
        old = ConicSolver(qps, st, lib_path=hip_lib)
        monkeypatch.delenv("SCORE_NO_BAND", raising=False)
        for sv in (new, again, old):
            sv.reset()
        for k in (1, 6):
            a, r, b = new.steps(k), again.steps(k), old.steps(k)
            for v in VECS:
                va, vr, vb = new.debug_get(v), again.debug_get(v), old.debug_get(v)
                assert np.array_equal(va, vr), (v, k)
                tol = 1e-10 if v in ("x", "xt", "s", "y", "u") else 1e-7
                assert np.allclose(va, vb, rtol=0.0, atol=tol * max(1.0, float(np.abs(vb).max()))), (v, k, float(np.abs(va - vb).max()))
        for sv in (new, again, old):
            sv.close()


def test_device_derived_a_g1_g2_equal_the_host_arrays(fixtures, hip_lib, monkeypatch):
    """A single problem whose equilibration ran on the device gets its equilibrated A, G1 = A' and G2 = [P | A'] DERIVED there
    (k_derive_a / k_derive_g: from the raw matrices, the A' map and the scales the passes left on the device) instead of filled
    on the host and uploaded: bit-equal to the host arrays -- 2-D and 3-D, replicated (native assembler: replicas bit-equal) and
    not (SCORE_NO_REPLICATION), BASELINE configs[3]; a batch keeps the uploads."""
    _hip_only(hip_lib)
    from score_amd.manhattan import make_config
    from score_amd.native import assemble_native

    monkeypatch.setenv("SCORE_HOST_SETUP", "1")  # (the host-side setup and its device-derived pieces: the default builds everything on the device)
    cases = [assemble_native(graph_by_name(nm, fixtures), "SOCP", lib_path=hip_lib).qp for nm in ("synth_a", "synth_b", "graph3d", "prior2d")]
    cases.append(assemble_native(make_config(3), "SOCP", lib_path=hip_lib).qp)
    for k, qp in enumerate(cases):
        for norep in (False, True):
            if norep:
                monkeypatch.setenv("SCORE_NO_REPLICATION", "1")
            dev = ConicSolver([qp], {}, lib_path=hip_lib)
            c = dev.debug_get("ag_device_check")
            assert c[0] == 1.0, "A, G1, G2 were not derived on the device"
            assert not c[1:].any(), c
            sd = dev.solve()[0]
            dev.close()
            monkeypatch.delenv("SCORE_NO_REPLICATION", raising=False)
            assert sd.solved
            if k < 4 and norep:
                break
    batch = ConicSolver(cases[:2], {}, lib_path=hip_lib)
    cb = batch.debug_get("ag_device_check")
    assert cb[0] == 0.0 and not cb[1:].any()
    batch.close()


def test_device_built_newton_matrix_equals_the_host_build(fixtures, hip_lib, monkeypatch):
    """score_create builds the Newton matrix's pattern, P on it, the contribution lists, the chain / Jacobi positions and the
    long entries ON THE DEVICE (score_polish_device.hpp: records, stable radix sort, scan, scatter).  Entry by entry and
    contribution by contribution it is what the host loop (score_polish_host.hpp, kept for the twin and as the fallback)
    builds -- no mismatch, coefficients bit-equal -- on 2-D and 3-D goldens, a graph with loop closures and landmark priors, a
    lock-step batch of different sizes and a graph whose landmark is seen by thousands of ranges (long entries); and the
    default solves through either build agree to the last bit."""
    _hip_only(hip_lib)
    cases = [[assemble(graph_by_name(nm, fixtures), "SOCP").qp] for nm in ("synth_a", "synth_b", "graph3d", "prior2d")]
    cases.append([assemble(make_manhattan(n_robots=2 + k, n_poses=300 + 170 * k, n_beacons=2, seed=90 + k), "SOCP").qp for k in range(3)])
    cases.append([assemble(make_manhattan(n_robots=4, n_poses=1500, n_beacons=1, seed=61, p_range=0.4), "SOCP").qp])
    from score_amd.manhattan import make_config
    from score_amd.native import assemble_native

    cases.append([assemble_native(make_config(3), "SOCP", lib_path=hip_lib).qp])  # BASELINE configs[3]: 20 x 1000 poses, landmark rows of thousands of entries
    monkeypatch.setenv("SCORE_HOST_SETUP", "1")  # (polish_build_check compares with the host loop, which reads the host-side matrices)
    for qps in cases:
        monkeypatch.delenv("SCORE_HOST_POLISH_BUILD", raising=False)
        dev = ConicSolver(qps, {}, lib_path=hip_lib)
        c = dev.debug_get("polish_build_check")
        assert c[0] == 1.0, "the Newton matrix was not built on the device"
        assert c[1] == c[2] and c[1] > 0, c
        assert not c[3:].any(), c
        sd = dev.solve()
        dev.close()
        monkeypatch.setenv("SCORE_HOST_POLISH_BUILD", "1")
        host = ConicSolver(qps, {}, lib_path=hip_lib)
        assert host.debug_get("polish_build_check")[0] == 0.0
        sh = host.solve()
        host.close()
        monkeypatch.delenv("SCORE_HOST_POLISH_BUILD", raising=False)
        for a, b in zip(sd, sh):
            assert a.solved and b.solved
            assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y) and a.info["newton_iters"] == b.info["newton_iters"]


_SETUP_INT = ("Aptr", "Acol", "G1ptr", "G1col", "G2ptr", "G2split", "G2col", "Kptr", "Kcol", "Kptr_dev", "Kcol_dev", "Hptr", "Hcol")
_SETUP_VAL = ("D", "E", "invD", "invE", "qs", "bs", "Aval", "G1val", "G2val", "K0", "K1", "Kval", "setup_scalars")


def test_device_setup_equals_the_host_setup(fixtures, hip_lib, monkeypatch):
    """f2: score_create builds every matrix of a handle ON THE DEVICE from the raw program (score_setup_device.hpp): the A' map
    (a stable sort of the columns), the equilibration over the block-diagonal batch, the equilibrated A, G1 = A', G2 = [P | A'],
    q, b, and K = P + sigma I + rho A'A as K0 + rho K1 (records in the host loop's order, stable radix sort, an entry adds its
    records in order).  Against the host setup (build_system, SCORE_HOST_SETUP=1; its equilibration on the device too, so that
    both sides start from the same scales): every pattern equal entry by entry, every value array equal BIT FOR BIT -- 2-D, 3-D,
    loop closures, priors, the direct QCQP form, general (non-replicated) problems, a lock-step batch of different sizes, a
    landmark seen by thousands of ranges, BASELINE configs[3] -- and the default solves agree to the last bit."""
    _hip_only(hip_lib)
    from score_amd.manhattan import make_config
    from score_amd.native import assemble_native

    cases = [([assemble_native(graph_by_name(nm, fixtures), "SOCP", lib_path=hip_lib).qp], {}) for nm in ("synth_a", "synth_b", "graph3d", "prior2d", "goats")]
    cases.append(([assemble_native(graph_by_name("synth_d", fixtures), "QCQP", lib_path=hip_lib).qp], dict(cg_iters=8, adaptive_rho=0)))
    cases.append(([assemble(graph_by_name("synth_c", fixtures), "SOCP").qp], {}))
    cases.append(([assemble_native(make_manhattan(n_robots=2 + k, n_poses=300 + 170 * k, n_beacons=2, seed=90 + k), "SOCP", lib_path=hip_lib).qp for k in range(3)], {}))
    cases.append(([assemble_native(make_manhattan(n_robots=4, n_poses=1500, n_beacons=1, seed=61, p_range=0.4), "SOCP", lib_path=hip_lib).qp], {}))
    cases.append(([assemble_native(make_config(3), "SOCP", lib_path=hip_lib).qp], {}))
    for k, (qps, st) in enumerate(cases):
        for norep in (False, True):
            if norep:
                monkeypatch.setenv("SCORE_NO_REPLICATION", "1")
            monkeypatch.delenv("SCORE_HOST_SETUP", raising=False)
            dev = ConicSolver(qps, st, lib_path=hip_lib)
            assert dev.debug_get("device_setup")[0] == 1.0, "the matrices were not built on the device"
            monkeypatch.setenv("SCORE_HOST_SETUP", "1")
            host = ConicSolver(qps, st, lib_path=hip_lib)
            assert host.debug_get("device_setup")[0] == 0.0
            monkeypatch.delenv("SCORE_HOST_SETUP", raising=False)
            for nm in _SETUP_INT + _SETUP_VAL:
                if nm in ("Hptr", "Hcol") and st:  # (the direct QCQP form has no Newton matrix)
                    continue
                a, b = dev.debug_get(nm), host.debug_get(nm)
                assert a.shape == b.shape and a.size > 0, (k, norep, nm, a.shape, b.shape)
                bad = np.nonzero(a != b)[0]
                assert bad.size == 0, (k, norep, nm, bad[:5], a[bad[:5]], b[bad[:5]])
            sd, sh = dev.solve(), host.solve()
            dev.close(); host.close()
            for x, y in zip(sd, sh):
                assert x.solved and y.solved
                assert np.array_equal(x.x, y.x) and np.array_equal(x.y, y.y) and np.array_equal(x.s, y.s)
                assert x.info["newton_iters"] == y.info["newton_iters"] and x.info["pobj"] == y.info["pobj"]
            monkeypatch.delenv("SCORE_NO_REPLICATION", raising=False)
            if k not in (0, 2, 7):
                break  # (the general kernels on the full K: a 2-D graph, the 3-D one, the batch)


_SOURCE_DEVICE, _SOURCE_DERIVED, _SOURCE_UPLOADED = 0.0, 1.0, 2.0  # score_debug_get "matrix_source" (HipBackend::MatrixSource)


@pytest.mark.parametrize("case", ["synth_a", "graph3d", "batch"])
def test_the_three_matrix_sources_give_the_same_handle(case, fixtures, hip_lib, monkeypatch):
    """A create takes its matrices from one of three sources, decided once (HipBackend::matrix_source): built on the device from
    the raw program (the default), the host's build_system with the equilibrated A, G1, G2 derived on the device (SCORE_HOST_SETUP=1,
    a single problem), or the host's build_system with everything uploaded (SCORE_HOST_SETUP=1 for a batch -- the derivation
    needs count == 1 --, or with SCORE_NO_DEVICE_RUIZ=1 as well).  Each handle reports the source it took.  With the equilibration
    on the device on both sides every setup array is equal bit for bit and so are the default solves (the comparisons of
    test_device_setup_equals_the_host_setup); the host's equilibration loop against the device's as
    test_device_equilibration_equals_the_host_loop compares them: the same formulas, D and E equal to 1e-12, K to 1e-11.
    synth_a: one robot x 60 poses; graph3d: 40 poses, 4 x 4 blocks, a loop closure and a prior; a lock-step batch of two
    Manhattan graphs of different sizes (2 x 40 and 3 x 70 poses)."""
    _hip_only(hip_lib)
    from score_amd.native import assemble_native

    if case == "batch":
        graphs = [make_manhattan(n_robots=2, n_poses=40, n_beacons=2, seed=121), make_manhattan(n_robots=3, n_poses=70, n_beacons=2, seed=122)]
    else:
        graphs = [graph_by_name(case, fixtures)]
    qps = [assemble_native(g, "SOCP", lib_path=hip_lib).qp for g in graphs]
    single = len(qps) == 1

    def create(expected, **env):
        for k in ("SCORE_HOST_SETUP", "SCORE_NO_DEVICE_RUIZ"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        sv = ConicSolver(qps, {}, lib_path=hip_lib)
        for k in env:
            monkeypatch.delenv(k, raising=False)
        assert sv.debug_get("matrix_source")[0] == expected, (case, env, sv.debug_get("matrix_source"))
        assert sv.debug_get("device_setup")[0] == (1.0 if expected == _SOURCE_DEVICE else 0.0)
        return sv

    dev = create(_SOURCE_DEVICE)
    host = create(_SOURCE_DERIVED if single else _SOURCE_UPLOADED, SCORE_HOST_SETUP="1")
    for nm in _SETUP_INT + _SETUP_VAL:
        a, b = dev.debug_get(nm), host.debug_get(nm)
        assert a.shape == b.shape and a.size > 0, (case, nm, a.shape, b.shape)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (case, nm, bad[:5], a[bad[:5]], b[bad[:5]])
    for x, y in zip(dev.solve(), host.solve()):
        assert x.solved and y.solved
        assert np.array_equal(x.x, y.x) and np.array_equal(x.y, y.y) and np.array_equal(x.s, y.s)
        assert x.info["newton_iters"] == y.info["newton_iters"] and x.info["pobj"] == y.info["pobj"]
    if single:  # the host's equilibration loop, everything uploaded, against the derived handle (scales from the device's passes)
        up = create(_SOURCE_UPLOADED, SCORE_HOST_SETUP="1", SCORE_NO_DEVICE_RUIZ="1")
        for v in ("D", "E"):
            a, b = host.debug_get(v), up.debug_get(v)
            assert a.min() > 0
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
        np.testing.assert_allclose(host.debug_get("Kval"), up.debug_get("Kval"), rtol=1e-11, atol=1e-300)
        up.close()
    dev.close(); host.close()


def test_device_assembler_equals_the_host_assembler(fixtures, hip_lib, monkeypatch):
    """f2: score_create_from_graphs builds the MODEL on the device (k_ga_*: every relative-pose measurement, range and prior
    writes the records score_assemble's filling pass adds, in that order; a stable sort and an in-order merge turn them into P
    and q; A and b are written in place) -- replaces initialize_model, /root/reference/score/utils/gurobi_utils.py:173-187,
    :233-352, :358-526.  Against a handle made from the host assembler's program (score_assemble -> score_create, both with the
    device setup): every setup array -- A, G1, G2, K0, K1, q, b, the scales -- bit-equal, i.e. P, q, A, b are the host
    assembler's to the last bit; the default solves identical including the objective (c0).  2-D, 3-D, loop closures, priors,
    the pinned pose in ranges and loop closures, the direct QCQP form, a batch, BASELINE configs[3]."""
    _hip_only(hip_lib)
    from score_amd.manhattan import make_config
    from score_amd.native import assemble_native, graph_arrays

    def graphs_of(names):
        return [graph_by_name(nm, fixtures) for nm in names]

    cases = [([g], "SOCP", {}) for g in graphs_of(("synth_a", "synth_b", "synth_c", "graph3d", "prior2d", "goats", "manhattan"))]
    cases.append((graphs_of(("synth_d",)), "QCQP", dict(cg_iters=8, adaptive_rho=0)))
    cases.append((graphs_of(("graph3d",)), "QCQP", dict(cg_iters=8, adaptive_rho=0)))
    cases.append(([make_manhattan(n_robots=2 + k, n_poses=300 + 170 * k, n_beacons=2, seed=90 + k) for k in range(3)], "SOCP", {}))
    cases.append(([make_config(3)], "SOCP", {}))
    # round 6, the per-row sort of the records (k_row_rank_sort): a pose tied to sixty others by loop closures -- its rows of P hold
    # more records than a lane ranks (the listed long rows: segmented radix sort) --, beside a two-pose graph
    hub = make_manhattan(n_robots=1, n_poses=80, n_beacons=2, seed=97, p_range=0.5)
    from score_amd import compat
    T = [pv.transformation_matrix for pv in hub.pose_variables[0]]
    for j in range(12, 72):
        rel = np.linalg.inv(T[5]) @ T[j]
        hub.loop_closure_measurements.append(compat.PoseMeasurement2D("A5", f"A{j}", float(rel[0, 2]), float(rel[1, 2]),
                                                                      float(np.arctan2(rel[1, 0], rel[0, 0])), 1e4, 2.5e5))
    cases.append(([hub, make_manhattan(n_robots=1, n_poses=2, n_beacons=1, seed=98, p_range=1.0)], "SOCP", {}))
    cases.append(([hub], "QCQP", dict(cg_iters=8, adaptive_rho=0)))
    for k, (graphs, relax, st) in enumerate(cases):
        arrays = [graph_arrays(g) for g in graphs]
        if relax == "QCQP":
            # the device assembler's own QCQP program (SCORE_QCQP_PLAIN: without the library's rewrite into private-head cones,
            # csrc/score_headform.hpp -- with it a QCQP graph handle builds the SOCP program; compared below)
            monkeypatch.setenv("SCORE_QCQP_PLAIN", "1")
        else:
            monkeypatch.delenv("SCORE_QCQP_PLAIN", raising=False)
        dev = ConicSolver.from_graphs(arrays, 0 if relax == "SOCP" else 1, st, lib_path=hip_lib)
        assert dev.debug_get("device_setup")[0] == 1.0
        host = ConicSolver([assemble_native(g, relax, lib_path=hip_lib, arrays=a).qp for g, a in zip(graphs, arrays)], st, lib_path=hip_lib)
        assert host.debug_get("device_setup")[0] == 1.0
        for nm in _SETUP_INT + _SETUP_VAL:
            if nm in ("Hptr", "Hcol") and st:
                continue
            a, b = dev.debug_get(nm), host.debug_get(nm)
            assert a.shape == b.shape and a.size > 0, (k, nm, a.shape, b.shape)
            bad = np.nonzero(a != b)[0]
            assert bad.size == 0, (k, nm, bad[:5], a[bad[:5]], b[bad[:5]])
        sd, sh = dev.solve(), host.solve()
        dev.close(); host.close()
        for x, y in zip(sd, sh):
            assert x.solved and y.solved
            assert np.array_equal(x.x, y.x) and np.array_equal(x.y, y.y) and np.array_equal(x.s, y.s)
            assert x.info["newton_iters"] == y.info["newton_iters"] and x.info["pobj"] == y.info["pobj"]
        if relax == "QCQP":
            # by default: the graph handle solves the graph's SOCP program and maps back (headform_from_graph), the array handle
            # rewrites the QCQP program it is given (headform_reduce) -- the same optimum, x / y / s of the QCQP program from both
            monkeypatch.delenv("SCORE_QCQP_PLAIN", raising=False)
            dev = ConicSolver.from_graphs(arrays, 1, {}, lib_path=hip_lib)
            host = ConicSolver([assemble_native(g, relax, lib_path=hip_lib, arrays=a).qp for g, a in zip(graphs, arrays)], {}, lib_path=hip_lib)
            assert (dev.n_total, dev.m_total) == (host.n_total, host.m_total)
            sd, sh = dev.solve(), host.solve()
            dev.close(); host.close()
            for x, y, g in zip(sd, sh, graphs):
                assert x.solved and y.solved and x.info["newton_iters"] > 0 and y.info["newton_iters"] > 0
                assert x.info["pobj"] == pytest.approx(y.info["pobj"], rel=1e-7, abs=1e-8)
                T = g.dimension
                # the cones' duals (zero where a cone is slack; the slacks (1, r) of slack cones follow undetermined landmarks)
                U, V = x.y.reshape(-1, T + 1), y.y.reshape(-1, T + 1)
                np.testing.assert_allclose(U, V, atol=1e-5 * max(1.0, np.abs(V).max()))
                assert np.all(x.s.reshape(-1, T + 1)[:, 0] == 1.0) and np.all(y.s.reshape(-1, T + 1)[:, 0] == 1.0)
    monkeypatch.delenv("SCORE_QCQP_PLAIN", raising=False)
    # the switch back to the host assembler, and what solve_score makes of either
    fg = graph_by_name("manhattan", fixtures)
    r_dev = solve_score(fg, "SOCP", lib_path=hip_lib)
    monkeypatch.setenv("SCORE_HOST_ASSEMBLE", "1")
    r_host = solve_score(fg, "SOCP", lib_path=hip_lib)
    monkeypatch.delenv("SCORE_HOST_ASSEMBLE", raising=False)
    r_nat = solve_score(fg, "SOCP", lib_path=hip_lib, assembler="native")
    for r in (r_host, r_nat):
        assert r.solved and r_dev.solved
        assert np.array_equal(r.poses.array, r_dev.poses.array) and np.array_equal(r.landmarks.array, r_dev.landmarks.array)
    # errors of the graph checks travel as ValueError
    arr = dict(graph_arrays(graph_by_name("synth_a", fixtures)))
    arr["rng_a"] = arr["rng_a"].copy(); arr["rng_a"][0] = 10 ** 6
    with pytest.raises(ValueError, match="range endpoint out of range"):
        ConicSolver.from_graphs([arr], 0, {}, lib_path=hip_lib)


@pytest.mark.parametrize("name,relax", [("manhattan", "SOCP"), ("graph3d", "SOCP"), ("synth_d", "QCQP"), ("synth_b", "SOCP"), ("prior2d", "SOCP")])
def test_device_setup_against_scipy(name, relax, fixtures, hip_lib, monkeypatch):
    """The setup the kernels run on, checked without any of the product's (or the twin's) host code: the scales D, E
    and the stored KKT operator come back from the handle; SciPy rebuilds K = D P D + sigma I + rho (E A D)'(E A D)
    from the problem data alone.  The stored rows (replica 0 of every pose row / landmark coordinate + the tail)
    must hold exactly SciPy's rows, and SciPy's K must be I_d (x) K_row + tail -- the structure the replicated
    kernels rely on (gurobi_utils.py:504-526: the cost couples one row of [R | t] at a time; :345-352: only the
    cones couple rows, and K sees them through A'A, which is per coordinate)."""
    _hip_only(hip_lib)
    monkeypatch.setenv("SCORE_QCQP_PLAIN", "1")  # (the QCQP program as given, not its head form: csrc/score_headform.hpp)
    qp = assemble(graph_by_name(name, fixtures), relax).qp
    rho, sigma = 0.37, 1e-6
    sol = ConicSolver(qp, dict(rho=rho, sigma=sigma, adaptive_rho=0), lib_path=hip_lib)
    D, E = sol.debug_get("D"), sol.debug_get("E")
    Kval, Kcol, Kptr = sol.debug_get("Kval"), sol.debug_get("Kcol").astype(np.int64), sol.debug_get("Kptr").astype(np.int64)
    rep, nr = int(sol.debug_get("rep")[0]), int(qp.rep_n)
    sol.close()
    assert rep == qp.rep_d and D.min() > 0 and E.min() > 0
    n = qp.n
    Ps = sp.diags(D) @ qp.P @ sp.diags(D)
    As = sp.diags(E) @ qp.A @ sp.diags(D)
    K = (Ps + sigma * sp.identity(n) + rho * (As.T @ As)).tocsr()
    stored = sp.csr_matrix((Kval[: Kptr[-1]], Kcol[: Kptr[-1]], Kptr), shape=(n, n))
    scale = abs(K).max()
    # rows the handle stores: replica 0 and the tail; the other replicas' rows are empty there
    rows = np.r_[np.arange(nr), np.arange(rep * nr, n)]
    assert abs(stored[rows] - K[rows]).max() <= 1e-12 * scale
    others = np.arange(nr, rep * nr)
    assert stored[others].nnz == 0
    # ... and what they would hold is replica 0's block again
    Krow = K[:nr, :nr]
    for k in range(1, rep):
        blk = K[k * nr : (k + 1) * nr]
        assert abs(blk[:, k * nr : (k + 1) * nr] - Krow).max() <= 1e-12 * scale
        off = blk.copy().tolil()
        off[:, k * nr : (k + 1) * nr] = 0
        assert abs(off.tocsr()).max() == 0.0
    assert abs(K[:nr, nr:]).max() == 0.0



@pytest.mark.parametrize("name,relax,rep", [("manhattan", "SOCP", 2), ("graph3d", "SOCP", 3), ("synth_d", "QCQP", 2), ("synth_b", "SOCP", 2)])
def test_replicated_kernels_match_the_general_ones(name, relax, rep, fixtures, hip_lib, twin_lib, monkeypatch):
    """K = I_d (x) K_row (+ tail) for every SCORE model (the cost couples one row of the pose matrices at a time,
    gurobi_utils.py:504-526; only the cones couple rows, :345-352).  The product streams K_row once and applies it to
    the d right-hand sides (k_spmv<MODE, NR>), factors one set of chains per robot and lets the d chains of a robot
    share it.  Against the same library with the structure switched off (SCORE_NO_REPLICATION: the general kernels on
    the full K) and against the CPU twin: every internal vector after k ADMM iterations, in 2-D, 3-D (three
    replicas), for the direct QCQP form (no tail unknowns) and with loop closures."""
    _hip_only(hip_lib)
    monkeypatch.setenv("SCORE_QCQP_PLAIN", "1")  # (the QCQP program as given -- replicas without a tail --, not its head form)
    qp = assemble(graph_by_name(name, fixtures), relax).qp
    st = dict(adaptive_cg=0, adaptive_rho=0, check_interval=5, fac_fp32=0, polish=0)
    monkeypatch.delenv("SCORE_NO_REPLICATION", raising=False)
    fast = ConicSolver(qp, st, lib_path=hip_lib)
    monkeypatch.setenv("SCORE_NO_REPLICATION", "1")
    plain = ConicSolver(qp, st, lib_path=hip_lib)
    monkeypatch.delenv("SCORE_NO_REPLICATION", raising=False)
    cpu = ConicSolver(qp, st, lib_path=twin_lib)
    ri, rp = fast.debug_get("rep"), plain.debug_get("rep")
    assert ri[0] == rep and rp[0] == 1 and cpu.debug_get("rep")[0] == 1
    n_tail = qp.n - rep * qp.rep_n
    assert ri[1] * rep - (rep - 1) * n_tail == rp[1]  # stored K: replica 0's rows + the (diagonal) tail rows
    for s_ in (fast, plain, cpu):
        s_.reset()
    for k in (1, 6, 13):
        outs = [s_.steps(k)[0] for s_ in (fast, plain, cpu)]
        for v in VECS:
            ga, gb, gc = fast.debug_get(v), plain.debug_get(v), cpu.debug_get(v)
            scale = max(1.0, np.abs(gc).max())
            # (loop closures: the capacitance solve of the link correction amplifies the reassociation a little)
            assert np.abs(ga - gb).max() <= (1e-9 if name == "synth_b" else 1e-10) * scale, (v, k, np.abs(ga - gb).max(), scale)
            assert np.abs(ga - gc).max() <= 1e-9 * scale, (v, k, np.abs(ga - gc).max(), scale)
        assert outs[0].info["res_dual"] == pytest.approx(outs[1].info["res_dual"], rel=1e-6, abs=1e-9)
    # a penalty change re-derives K_row, its factors and the carried product K xt on the device
    a = ConicSolver(qp, dict(polish=0, fac_fp32=0, rho=300.0, max_iters=3000), lib_path=hip_lib).solve()[0]
    monkeypatch.setenv("SCORE_NO_REPLICATION", "1")
    b = ConicSolver(qp, dict(polish=0, fac_fp32=0, rho=300.0, max_iters=3000), lib_path=hip_lib).solve()[0]
    # (the adaptive penalty / PCG count decisions amplify rounding differences: the two runs may take different paths)
    assert a.info["status"] == b.info["status"] and (a.info["status"] == 1 or relax == "QCQP"), (a.info, b.info)
    assert a.info["rho_updates"] > 0 and b.info["rho_updates"] > 0 or name != "manhattan"
    assert a.info["pobj"] == pytest.approx(b.info["pobj"], rel=1e-5, abs=1e-6)  # (the optimiser itself need not be unique)
    for s_ in (fast, plain, cpu):
        s_.close()


@pytest.mark.parametrize("relax", ["SOCP", "QCQP"])
@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_solve_score_matches_golden(name, relax, fixtures, hip_lib):
    """Product default path against the oracle-only goldens (2-D fixtures of the reference, four
    synthetic graphs, one 3-D graph): objective, every pose / landmark the optimum determines, and --
    where robots keep gauge freedom -- the residuals and range excesses every optimum shares."""
    _hip_only(hip_lib)
    fg = graph_by_name(name, fixtures)
    res = solve_score(fg, relax)  # default library = HIP
    gold = load_golden(name)
    assert res.solved, res.info
    assert res.info["pobj"] == pytest.approx(float(gold["objective"]), rel=1e-5, abs=1e-6)
    compare_with_golden(res, gold, pose_tol=1e-4)  # north_star: 1e-4 relative
    compare_residuals_with_golden(res, fg, gold, tol=1e-4)


def test_newton_control_queued_ahead_is_bit_equal(fixtures, hip_lib, monkeypatch):
    """The polish queues the next Newton iteration's control fetch and Hessian assembly before the host waits for the
    evaluation (k_fetch_wait: released by the host's words; HipBackend::prequeue_control).  Against the launch after the
    decision (SCORE_NO_PREQUEUE=1): same Newton iterations, x, y, s to the last bit -- single problems (2-D fixture, GOATS with
    its step-length searches, 3-D), a lock-step batch whose members finish at different iterations, and a handle solved twice."""
    _hip_only(hip_lib)
    from score_amd.native import assemble_native

    cases = [[assemble_native(graph_by_name(nm, fixtures), "SOCP", lib_path=hip_lib).qp] for nm in ("manhattan", "goats", "graph3d", "synth_b")]
    cases.append([assemble_native(make_manhattan(n_robots=2 + k, n_poses=120 + 90 * k, n_beacons=3, seed=70 + k, p_range=0.2 + 0.1 * k), "SOCP", lib_path=hip_lib).qp
                  for k in range(4)])
    for qps in cases:
        runs = {}
        for off in (False, True):
            if off:
                monkeypatch.setenv("SCORE_NO_PREQUEUE", "1")
            else:
                monkeypatch.delenv("SCORE_NO_PREQUEUE", raising=False)
            sv = ConicSolver(qps, {}, lib_path=hip_lib)
            first = sv.solve()
            runs[off] = (first, sv.solve())
            sv.close()
        monkeypatch.delenv("SCORE_NO_PREQUEUE", raising=False)
        for a_run, b_run in zip(runs[False], runs[True]):
            for a, b in zip(a_run, b_run):
                assert a.solved and b.solved and a.info["newton_iters"] == b.info["newton_iters"] > 0
                assert a.info["newton_cg_iters"] == b.info["newton_cg_iters"]
                assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y) and np.array_equal(a.s, b.s)


@pytest.mark.parametrize("name", ["manhattan", "graph3d"])
def test_solve_score_without_replication(name, fixtures, hip_lib, monkeypatch):
    """The experiment switch SCORE_NO_REPLICATION through the product entry point: the graph assembler on the device writes one
    replica's rows, so a handle that is not to be replicated must take the host assembler (device_setup_ok_graphs) -- same golden
    optimum, polish included."""
    _hip_only(hip_lib)
    fg = graph_by_name(name, fixtures)
    monkeypatch.setenv("SCORE_NO_REPLICATION", "1")
    res = solve_score(fg, "SOCP")
    monkeypatch.delenv("SCORE_NO_REPLICATION", raising=False)
    assert res.solved and res.info["newton_iters"] > 0, res.info
    gold = load_golden(name)
    assert res.info["pobj"] == pytest.approx(float(gold["objective"]), rel=1e-5, abs=1e-6)
    compare_with_golden(res, gold, pose_tol=1e-4)


def test_qcqp_direct_on_gpu(fixtures, hip_lib, monkeypatch):
    """The reference's default relaxation handed over as it is (gurobi_utils.py:341-344, :488-496): the library rewrites the
    constant-head unit-ball cones into private-head cones (csrc/score_headform.hpp), so the direct form takes the same
    ADMM warm-up + semismooth-Newton polish as the SOCP form -- same optimum as via the SOCP and as the golden file to 1e-6,
    in comparable time; the directions r_ij come back in closed form.  SCORE_QCQP_PLAIN=1: the plain loop of rounds 1-4."""
    fg = fixtures["manhattan"]
    gold = load_golden("manhattan")
    monkeypatch.delenv("SCORE_QCQP_PLAIN", raising=False)
    solve_score(fg, "QCQP"); solve_score(fg, "QCQP", qcqp_mode="direct")  # (warm: first handles of a process pay for the runtime)
    a = solve_score(fg, "QCQP")
    b = solve_score(fg, "QCQP", qcqp_mode="direct")
    assert a.solved and b.solved
    assert b.info["newton_iters"] > 0 and b.info["iters"] == a.info["iters"]
    assert b.total_time <= 2.0 * a.total_time
    assert a.info["pobj"] == pytest.approx(b.info["pobj"], rel=1e-6)
    assert b.info["pobj"] == pytest.approx(float(gold["objective"]), rel=1e-6)
    compare_with_golden(a, gold, pose_tol=1e-6)
    compare_with_golden(b, gold, pose_tol=1e-6)
    for m in fg.range_measurements:  # r_ij agree wherever the measured distance is not zero
        if m.dist > 1e-6:
            k = (m.first_key, m.second_key)
            np.testing.assert_allclose(a.distances[k], b.distances[k], atol=1e-6)
            assert np.linalg.norm(b.distances[k]) <= 1.0 + 1e-12
    # the same through the array API (score_create with the QCQP program as given): x, y, s of THAT program
    from score_amd.assemble import assemble
    from score_amd.solver import ConicSolver

    qp = assemble(fg, "QCQP").qp
    sv = ConicSolver([qp], {})
    sol = sv.solve()[0]
    assert (sv.n_total, sv.m_total) == (qp.n, qp.m)
    sv.close()
    assert sol.solved and sol.info["newton_iters"] > 0
    scale = max(1.0, np.abs(sol.y).max())
    assert np.abs(qp.A @ sol.x + sol.s - qp.b).max() <= 1e-12
    assert np.abs(qp.P @ sol.x + qp.q + qp.A.T @ sol.y).max() <= 1e-6 * scale
    assert qp.objective(sol.x) == pytest.approx(float(gold["objective"]), rel=1e-6)
    monkeypatch.setenv("SCORE_QCQP_PLAIN", "1")
    c = solve_score(fg, "QCQP", qcqp_mode="direct")
    assert c.solved and c.info["newton_iters"] == 0 and c.info["iters"] > 10 * b.info["iters"]
    assert c.info["pobj"] == pytest.approx(b.info["pobj"], rel=1e-5)


def test_deterministic_and_batch(hip_lib):
    graphs = [make_manhattan(n_robots=3, n_poses=40 + 10 * (s % 4), n_beacons=4, seed=s, p_range=0.4) for s in (300, 303, 305, 307)]
    b1 = solve_score_batch(graphs, "SOCP", lockstep=True, solver_settings=dict(polish=0))
    b2 = solve_score_batch(graphs, "SOCP", lockstep=True, solver_settings=dict(polish=0))
    for g, r1, r2 in zip(graphs, b1, b2):
        ri = solve_score(g, "SOCP", solver_settings=dict(polish=0))  # ADMM alone: lock-step == one by one
        assert r1.solved and ri.solved and r1.info["iters"] == ri.info["iters"]
        for nm in ri.poses:
            assert np.array_equal(r1.poses[nm], r2.poses[nm])  # bitwise reproducible
            np.testing.assert_allclose(r1.poses[nm], ri.poses[nm], atol=1e-9)


def test_edge_cases_on_gpu(hip_lib):
    fg = make_manhattan(n_robots=1, n_poses=30, n_beacons=0, seed=2)  # m = 0: no cones
    res = solve_score(fg, "SOCP")
    assert res.solved and res.info["pobj"] == pytest.approx(0.0, abs=1e-6)
    fg = make_manhattan(n_robots=1, n_poses=2, n_beacons=1, seed=3, p_range=1.0)  # tiny
    assert solve_score(fg, "SOCP").solved
    res = solve_score(fg, "SOCP", solver_settings=dict(max_iters=25, eps_abs=1e-15, eps_rel=1e-15, polish=0))
    assert res.solved is False and res.info["status"] == 2  # not an exception


def test_long_chain_and_3d_blocks(hip_lib, twin_lib):
    """A 3000-pose single chain (multi-level partition with > 256 runs per level)
    and block size 4 (3-D poses) against the CPU twin."""
    from test_oracle_and_assembly import _graph_3d

    fg = make_manhattan(n_robots=1, n_poses=3000, n_beacons=3, seed=8)
    a = solve_score(fg, "SOCP", solver_settings=dict(polish=0))
    b = solve_score(fg, "SOCP", lib_path=twin_lib)
    # the two runs may straddle a convergence check by one launch graph (float reassociation)
    assert a.solved and b.solved and abs(a.info["iters"] - b.info["iters"]) <= 25
    for nm in ("A1", "A1500", "A2999"):
        np.testing.assert_allclose(a.poses[nm], b.poses[nm], atol=5e-6)
    fg3 = _graph_3d(n=40)
    a = solve_score(fg3, "SOCP")
    b = solve_score(fg3, "SOCP", lib_path=twin_lib)
    assert a.solved and b.solved
    for nm in a.poses:
        np.testing.assert_allclose(a.poses[nm], b.poses[nm], atol=5e-6)
    rp, u, _ = so.newton_solve(fg3, tol=1e-12)
    assert a.info["pobj"] == pytest.approx(so.LiteralModel(fg3, "SOCP").direct_cost(so.reduced_to_values(rp, u, "SOCP")), rel=1e-5, abs=1e-6)


@pytest.mark.parametrize("n_poses", [255, 1023, 1024])
def test_both_chain_kernels_match_the_twin(n_poses, hip_lib, twin_lib):
    """Chains of up to 1023 poses run the register/LDS-resident chain kernel (k_prec_pre); longer ones are cut into
    segments for it and joined by a second level (score_join.hpp; 1024 poses: robot B's 1024 free nodes), radix != 4 takes
    the streaming kernel (k_prec): same preconditioner, same iterates.  A fixed number of ADMM iterations is compared with
    the CPU twin on both sides of the boundary, and the kernels with each other on the same chain (radix 2 forces the
    streaming kernel).  With float factors (the default) a segmented chain's operator is the exact inverse of a matrix
    rounded differently from the twin's whole-chain factors: compared with double factors there."""
    fg = make_manhattan(n_robots=2, n_poses=n_poses, n_beacons=3, seed=21)
    qp = assemble(fg, "SOCP").qp
    outs = {}
    f32 = dict(fac_fp32=0) if n_poses > 1023 else {}
    for name, lib, extra in (("hip", None, f32), ("twin", twin_lib, f32), ("hip_r2", None, dict(chain_radix=2)),
                             ("twin_r2", twin_lib, dict(chain_radix=2))):
        sol = ConicSolver(qp, dict(polish=0, adaptive_rho=0, adaptive_cg=0, **extra), lib_path=lib)
        outs[name] = sol.steps(50)[0]
        sol.close()
    for a, b in (("hip", "twin"), ("hip_r2", "twin_r2")):
        scale = np.abs(outs[b].x).max()
        np.testing.assert_allclose(outs[a].x, outs[b].x, atol=1e-7 * scale)
        assert outs[a].info["pobj"] == pytest.approx(outs[b].info["pobj"], rel=1e-8)


@pytest.mark.parametrize("case", ["2d", "3d", "batch"])
def test_segmented_long_chains_equal_the_streaming_solve(case, hip_lib, twin_lib, monkeypatch):
    """Chains of more than 1023 poses (score_host.hpp: JoinChain; score_join.hpp): segments for the LDS-resident chain
    kernel + separators' Schur system + spike correction = the exact solve with the whole chain's block-tridiagonal matrix.
    With double factors the ADMM iterates equal the twin's (whole chains, streaming solve) and the streaming kernel's
    (SCORE_NO_SEGMENTS=1) to rounding; the default solver (float factors, Newton polish with its own segmented factors)
    takes the same Newton iterations and ends at the same point; 2-D, 3-D (4 x 4 blocks) and a lock-step batch."""
    from score_amd.manhattan import make_manhattan_3d

    if case == "2d":
        graphs = [make_manhattan(n_robots=2, n_poses=2500, n_beacons=3, seed=31)]  # 3 segments per chain
    elif case == "3d":
        graphs = [make_manhattan_3d(n_robots=2, n_poses=1300, n_beacons=3, seed=32, p_range=0.3)]
    else:
        graphs = [make_manhattan(n_robots=1, n_poses=1100, n_beacons=2, seed=33), make_manhattan(n_robots=2, n_poses=700, n_beacons=3, seed=34),
                  make_manhattan(n_robots=2, n_poses=2100, n_beacons=3, seed=35)]
    qps = [assemble(g, "SOCP").qp for g in graphs]
    fixed = dict(polish=0, adaptive_rho=0, adaptive_cg=0, fac_fp32=0)
    outs = {}
    for name, lib, env in (("seg", None, None), ("stream", None, "1"), ("twin", twin_lib, None)):
        if env:
            monkeypatch.setenv("SCORE_NO_SEGMENTS", env)
        else:
            monkeypatch.delenv("SCORE_NO_SEGMENTS", raising=False)
        sol = ConicSolver(qps, fixed, lib_path=lib)
        outs[name] = sol.steps(40)
        sol.close()
    for k in range(len(qps)):
        scale = max(1.0, np.abs(outs["twin"][k].x).max())
        np.testing.assert_allclose(outs["seg"][k].x, outs["twin"][k].x, atol=1e-9 * scale)
        np.testing.assert_allclose(outs["seg"][k].x, outs["stream"][k].x, atol=1e-9 * scale)
    full = {}
    for name, env in (("seg", None), ("stream", "1")):
        if env:
            monkeypatch.setenv("SCORE_NO_SEGMENTS", env)
        else:
            monkeypatch.delenv("SCORE_NO_SEGMENTS", raising=False)
        sol = ConicSolver(qps, {})
        full[name] = sol.solve()
        sol.close()
    monkeypatch.delenv("SCORE_NO_SEGMENTS", raising=False)
    for k, qp in enumerate(qps):
        a, b = full["seg"][k], full["stream"][k]
        assert a.solved and b.solved and a.info["newton_iters"] > 0
        assert a.info["newton_iters"] == b.info["newton_iters"] and a.info["iters"] == b.info["iters"]
        scale = max(1.0, np.abs(b.x).max())
        np.testing.assert_allclose(a.x, b.x, atol=1e-7 * scale)
        assert a.info["pobj"] == pytest.approx(b.info["pobj"], rel=1e-8, abs=1e-8)
        cert = so.kkt_certificate(qp.P, qp.q, qp.A, qp.b, 0, qp.soc_dims, a.x, a.y, a.s)
        assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, cert
    if case == "2d":
        # the linear mode (Gauss-Newton / LM refinement after SCORE: score_linear_solve on the pose chains) takes the same path
        from score_amd.refine import refine_estimate

        res = solve_score(graphs[0], "SOCP")
        ref = {}
        for name, env in (("seg", None), ("stream", "1")):
            if env:
                monkeypatch.setenv("SCORE_NO_SEGMENTS", env)
            else:
                monkeypatch.delenv("SCORE_NO_SEGMENTS", raising=False)
            ref[name] = refine_estimate(graphs[0], res)
        monkeypatch.delenv("SCORE_NO_SEGMENTS", raising=False)
        (ra, ia), (rb, ib) = ref["seg"], ref["stream"]
        assert ia["iterations"] == ib["iterations"] and ia["cost_final"] == pytest.approx(ib["cost_final"], rel=1e-10)
        assert max(np.abs(ra.poses[k] - rb.poses[k]).max() for k in ra.poses) < 1e-9


def test_a_chain_of_more_than_65_segments(hip_lib):
    """Advisor finding (round 5): a chain of more than 65 segments of 1023 nodes (> 66.6 k poses) failed at score_create
    ("chain too long: more than 65 segments").  The second level now holds 128 separators per chain (132 k poses; the
    streaming kernel, which a longer chain falls back to, keeps its coarse levels in LDS and ends at ~18 k: it never reached
    this size).  One robot x 67 000 poses (66 segments): created, solved, KKT certificate of the program as given."""
    fg = make_manhattan(n_robots=1, n_poses=67000, n_beacons=2, seed=5, p_range=0.02)
    qp = assemble(fg, "SOCP").qp
    sol = ConicSolver([qp], {})
    out = sol.solve()[0]
    sol.close()
    assert out.solved, out.info
    cert = so.kkt_certificate(qp.P, qp.q, qp.A, qp.b, 0, qp.soc_dims, out.x, out.y, out.s)
    assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, cert


@pytest.mark.parametrize("index", [1, 2, 3])
def test_full_size_configs_are_certified(index, hip_lib):
    """BASELINE.json's full sizes (1x500, 4x1000, 20x1000 poses): the solver-
    independent KKT certificate of the conic program, the reference's objective
    evaluated literally on the returned estimate, cone feasibility, the pinned
    pose -- and the oracle's optimum pose by pose: computed on the spot up to
    4 x 1000 poses, from the committed golden file (oracle alone, offline) at
    the headline size 20 x 1000."""
    fg = make_config(index)
    mdl = assemble(fg, "SOCP")
    sol = ConicSolver(mdl.qp, dict(eps_abs=1e-7, eps_rel=1e-7))
    out = sol.solve()[0]
    sol.close()
    assert out.solved, out.info
    cert = so.kkt_certificate(mdl.qp.P, mdl.qp.q, mdl.qp.A, mdl.qp.b, 0, mdl.qp.soc_dims, out.x, out.y, out.s)
    assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, cert
    assert cert["s_cone_dist"] < 1e-9 and cert["y_cone_dist"] < 1e-9, cert
    assert cert["gap"] < 1e-4 * max(1.0, abs(out.info["pobj"])), cert
    assert cert["primal_res_inf"] == pytest.approx(out.info["res_pri"], rel=1e-6, abs=1e-12)
    assert cert["dual_res_inf"] == pytest.approx(out.info["res_dual"], rel=1e-6, abs=1e-8)
    xm = mdl.expand(out.x)
    d = 2
    vals = {
        "poses": {nm: mdl.pose_blocks(xm)[i] for i, nm in enumerate(mdl.pose_names)},
        "landmarks": {nm: mdl.landmark_block(xm)[i] for i, nm in enumerate(mdl.landmark_names)},
        "dists": {k: mdl.range_block(xm)[i] for i, k in enumerate(mdl.range_keys)},
    }
    lit = so.LiteralModel(fg, "SOCP")
    assert lit.pin_violation(vals) == 0.0
    assert lit.cone_violation(vals) < 1e-5
    assert lit.direct_cost(vals) == pytest.approx(out.info["pobj"], rel=1e-6, abs=1e-6)
    if index <= 2:  # the Newton oracle finishes in seconds at these sizes
        rp, u, info = so.newton_solve(fg, tol=1e-12)
        assert out.info["pobj"] == pytest.approx(info["objective"], rel=1e-5)
        ref = so.reduced_to_values(rp, u, "SOCP")
        scale = max(np.abs(v[:, 2]).max() for v in ref["poses"].values())
        worst = max(np.abs(vals["poses"][n] - ref["poses"][n]).max() for n in ref["poses"])
        assert worst / scale < 1e-4
    else:
        # the headline size: the oracle's optimum was computed offline in the build container
        # (tests/golden/make_config_golden.py) -- all 20 000 pose blocks, pose by pose, to the 1e-4 relative
        # north_star states for what solve_score returns (/root/reference/score/solve_score.py:54-86)
        gold = load_golden(f"config{index}")
        assert bool(gold["pose_determined"].all()) and bool(gold["landmark_determined"].all())
        assert out.info["pobj"] == pytest.approx(float(gold["objective"]), rel=1e-6)
        P = mdl.pose_blocks(xm)
        scale = float(np.abs(gold["poses"][:, :, d]).max())
        assert np.abs(P - gold["poses"]).max() / scale < 1e-4
        assert np.abs(mdl.landmark_block(xm) - gold["landmarks"]).max() / scale < 1e-4
        res = solve_score(fg, "SOCP")  # the drop-in API on the same graph: rounded poses, landmarks, shared residuals
        assert res.solved
        wt, wr = compare_with_golden(res, gold, pose_tol=1e-4)
        compare_residuals_with_golden(res, fg, gold, tol=1e-4)
        rq = solve_score(fg, "QCQP")  # the reference's default relaxation shares the optimum
        assert rq.solved
        compare_with_golden(rq, gold, pose_tol=1e-4)


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_newton_polish_matches_golden(name, fixtures, hip_lib):
    """Full solver (ADMM warm-up + semismooth-Newton polish on the GPU): tighter
    than ADMM alone -- objective to 1e-8 relative, poses to 1e-6, primal residual
    exactly feasible, and far fewer ADMM iterations."""
    _hip_only(hip_lib)
    fg = graph_by_name(name, fixtures)
    gold = load_golden(name)
    res = solve_score(fg, "SOCP", solver_settings=dict(polish=1))
    plain = solve_score(fg, "SOCP", solver_settings=dict(polish=0))
    assert res.solved and plain.solved, (res.info, plain.info)
    assert res.info["newton_iters"] > 0 and plain.info["newton_iters"] == 0
    assert res.info["iters"] < plain.info["iters"]
    assert res.info["pobj"] == pytest.approx(float(gold["objective"]), rel=1e-8, abs=1e-8)
    assert res.info["res_pri"] <= 1e-9
    compare_with_golden(res, gold, pose_tol=1e-6)
    # the other factor precisions (0: double throughout; 2: float stream for the Newton factors too) end at the same optimum
    for mode in (0, 2):
        alt = solve_score(fg, "SOCP", solver_settings=dict(fac_fp32=mode))
        assert alt.solved and alt.info["pobj"] == pytest.approx(float(gold["objective"]), rel=1e-8, abs=1e-8), (mode, alt.info)
        compare_with_golden(alt, gold, pose_tol=1e-6)
    compare_residuals_with_golden(res, fg, gold, tol=1e-6)
    rq = solve_score(fg, "QCQP", solver_settings=dict(polish=1))  # QCQP answered through the polished SOCP
    assert rq.solved
    compare_with_golden(rq, gold, pose_tol=1e-6)


def test_newton_polish_on_degenerate_and_unsupported_cases(hip_lib):
    # a small graph on which plain ADMM needs > 10^4 iterations
    fg = make_manhattan(n_robots=3, n_poses=60, n_beacons=4, seed=302, p_range=0.4)
    res = solve_score(fg, "SOCP", solver_settings=dict(max_iters=5000))
    assert res.solved and res.info["newton_iters"] > 0, res.info
    rp, u, info = so.newton_solve(fg, tol=1e-13)
    assert res.info["pobj"] == pytest.approx(info["objective"], rel=1e-7, abs=1e-9)
    # batches are polished in lock-step or one after another
    graphs = [make_manhattan(n_robots=3, n_poses=40 + 10 * (s % 4), n_beacons=4, seed=s, p_range=0.4) for s in (300, 303)]
    lock = solve_score_batch(graphs, "SOCP", lockstep=True)
    pool = solve_score_batch(graphs, "SOCP", lockstep=False)
    for a, b in zip(lock, pool):
        assert a.solved and b.solved and a.info["newton_iters"] > 0 and b.info["newton_iters"] > 0
        assert a.info["pobj"] == pytest.approx(b.info["pobj"], rel=1e-8, abs=1e-9)
    rd = solve_score(graphs[0], "QCQP", qcqp_mode="direct")  # (round 5: rewritten into its head form and polished)
    assert rd.solved and rd.info["newton_iters"] > 0
    assert rd.info["pobj"] == pytest.approx(lock[0].info["pobj"], rel=1e-7, abs=1e-9)


def test_random_graphs_against_the_oracle(hip_lib):
    """Randomised sweep: 24 small graphs of varying shape (1-4 robots, with and
    without beacons / loop closures, sparse and dense ranging).  The full GPU solver
    must reproduce the oracle's optimum: objective to 1e-7 relative, the pinned
    robot's trajectory to 1e-5 relative."""
    rng = np.random.default_rng(2024)
    worst_obj, worst_pose = 0.0, 0.0
    for trial in range(24):
        kw = dict(
            n_robots=int(rng.integers(1, 5)), n_poses=int(rng.integers(20, 90)), n_beacons=int(rng.integers(0, 5)),
            seed=1000 + trial, p_range=float(rng.choice([0.1, 0.2, 0.4])), n_loop_closures=int(rng.choice([0, 0, 3])),
        )
        fg = make_manhattan(**kw)
        if fg.unconnected_variable_names:
            continue
        res = solve_score(fg, "SOCP")
        assert res.solved, (kw, res.info)
        rp, u, info = so.newton_solve(fg, tol=1e-13, max_iter=300)
        ref = so.reduced_to_values(rp, u, "SOCP")
        obj = so.LiteralModel(fg, "SOCP").direct_cost(ref)
        worst_obj = max(worst_obj, abs(res.info["pobj"] - obj) / max(1.0, abs(obj)))
        scale = max(1.0, max(np.abs(X[:, 2]).max() for X in ref["poses"].values()))
        for p in fg.pose_variables[0]:
            worst_pose = max(worst_pose, float(np.abs(res.poses[p.name][:2, 2] - ref["poses"][p.name][:, 2]).max()) / scale)
    assert worst_obj < 1e-7, worst_obj
    assert worst_pose < 1e-5, worst_pose


def test_handles_from_a_thread_pool_and_empty_tiles(hip_lib):
    """Regression: (1) several host threads drive their own handles while others capture launch
    graphs; (2) a problem without any cone (empty A, empty trailing tiles) solved after other
    handles were freed -- the clamped unconditional loads must stay inside padded arrays."""
    graphs = [make_manhattan(n_robots=3, n_poses=40 + 10 * (s % 4), n_beacons=4, seed=s, p_range=0.4) for s in (300, 303, 305, 307, 309, 310)]
    seq = solve_score_batch(graphs, "SOCP", workers=1)
    par = solve_score_batch(graphs, "SOCP", workers=6)
    for a, b in zip(seq, par):
        assert a.solved and b.solved
        for nm in a.poses:
            assert np.array_equal(a.poses[nm], b.poses[nm])
    for seed in range(3):
        fg = make_manhattan(n_robots=1, n_poses=50 + 17 * seed, n_beacons=0, seed=seed, p_range=0.0)
        assert solve_score(fg, "SOCP").solved


def test_polish_warmup_and_in_loop_timing_probe(hip_lib):
    """polish_warmup sets the length of the first ADMM block; score_time_iteration returns a
    positive device-clock duration for each of the six kernels of the iteration and leaves the
    handle usable."""
    qp = assemble(make_manhattan(n_robots=3, n_poses=200, n_beacons=3, seed=6), "SOCP").qp
    for warm, expect in ((15, 15), (0, 25), (40, 25)):
        sol = ConicSolver(qp, dict(polish_warmup=warm))
        out = sol.solve()[0]
        sol.close()
        assert out.solved and out.info["newton_iters"] > 0 and out.info["iters"] == expect, out.info
    sol = ConicSolver(qp, dict(polish=0))
    ref = sol.solve()[0]
    us, disp = sol.time_iteration(warmup=5, iters=20, dispatch=True)
    assert list(us) == list(disp) == ["rhs", "prec_init", "kp", "prec_step", "kpb", "cone"]
    assert all(0.5 < v < 500.0 for v in us.values()), us
    # begin-to-end of a dispatch (start/stop events bound to the launch) contains the interval
    # first workgroup in -> last workgroup out
    assert all(0.5 < disp[k] < 500.0 and disp[k] > 0.8 * us[k] for k in us), (us, disp)
    again = sol.solve()[0]  # solve() resets the iterates: the probe leaves no trace
    np.testing.assert_array_equal(ref.x, again.x)
    sol.close()


def test_chain_length_sweep_against_the_twin(hip_lib, twin_lib, monkeypatch):
    """Chain lengths around every structural boundary of the chain kernels (last-level runs of
    1..3 nodes, one/two/three levels, 64/256 runs per level, the k_prec_pre / k_prec switch), with
    random robot / beacon / loop-closure counts: 40 ADMM iterations must reproduce the CPU twin's
    iterates, and the full solver must return a certified optimum.  Graphs with loop closures are compared
    twice: the float-factor chain kernels with the link correction off (the correction on float factors agrees
    to 1e-3 only, test_iterates_match_cpu_twin), and the correction itself on double factors."""
    rng = np.random.default_rng(123)
    for trial, n_poses in enumerate([2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257]):
        nrob, nb = int(rng.integers(1, 4)), int(rng.integers(0, 4))
        nlc = int(rng.integers(0, 3)) if n_poses > 8 else 0
        if nrob == 1 and nb == 0:
            nb = 1
        fg = make_manhattan(n_robots=nrob, n_poses=n_poses, n_beacons=nb, seed=1000 + trial, n_loop_closures=nlc,
                            p_range=float(rng.uniform(0.05, 0.6)))
        qp = assemble(fg, "SOCP").qp
        for no_links, fp32 in ([("1", 1), (None, 0)] if nlc else [(None, 1)]):
            if no_links:
                monkeypatch.setenv("SCORE_NO_LINKS", no_links)
            outs = []
            for lib in (None, twin_lib):
                sol = ConicSolver(qp, dict(polish=0, adaptive_rho=0, adaptive_cg=0, fac_fp32=fp32), lib_path=lib)
                outs.append(sol.steps(40)[0])
                sol.close()
            monkeypatch.delenv("SCORE_NO_LINKS", raising=False)
            scale = max(1.0, np.abs(outs[1].x).max())
            np.testing.assert_allclose(outs[0].x, outs[1].x, atol=1e-7 * scale, err_msg=f"n_poses={n_poses} fp32={fp32}")
        sol = ConicSolver(qp, {})
        full = sol.solve()[0]
        sol.close()
        assert full.solved, (n_poses, full.info)
        cert = so.kkt_certificate(qp.P, qp.q, qp.A, qp.b, 0, qp.soc_dims, full.x, full.y, full.s)
        assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, (n_poses, cert)


def test_live_handles_of_different_sizes(hip_lib):
    """The dynamic-LDS ceiling of the chain kernels is a per-function attribute shared by every
    handle of the process: creating a smaller handle must not lower it under a larger live one."""
    qps = [assemble(make_manhattan(n_robots=2, n_poses=n, n_beacons=3, seed=n), "SOCP").qp for n in (1000, 500, 120)]
    sols = [ConicSolver(qp, {}) for qp in qps]  # largest first
    ref = [s.solve()[0] for s in sols]
    for _ in range(2):
        for s, r in zip(sols, ref):
            out = s.solve()[0]
            assert out.solved and out.info["pobj"] == r.info["pobj"]
    for s in sols:
        s.close()


def test_lockstep_batch_polish_matches_individual_solves(hip_lib):
    """A batch handle advances all its problems through the same launches, ADMM warm-up and Newton
    polish alike (per-problem step lengths, line searches and PCG tolerances): every problem must
    end where its own single-problem solve ends, whatever its neighbours in the batch need."""
    specs = [(2, 150, 3, 1), (1, 400, 2, 2), (3, 80, 3, 3), (4, 1000, 4, 4), (2, 37, 0, 5), (1, 12, 1, 6), (1, 30, 0, 7),
             (3, 300, 2, 8)]
    qps = [assemble(make_manhattan(n_robots=r, n_poses=n, n_beacons=b, seed=s), "SOCP").qp for r, n, b, s in specs]
    single = []
    for qp in qps:
        sol = ConicSolver(qp, {})
        single.append(sol.solve()[0])
        sol.close()
    sol = ConicSolver(qps, {})
    batch = sol.solve()
    again = sol.solve()
    sol.close()
    assert any(o.info["newton_iters"] > 0 for o in batch)
    for qp, a, b, c in zip(qps, single, batch, again):
        assert a.solved and b.solved, (a.info, b.info)
        assert b.info["pobj"] == pytest.approx(a.info["pobj"], rel=1e-7, abs=1e-8)
        cert = so.kkt_certificate(qp.P, qp.q, qp.A, qp.b, 0, qp.soc_dims, b.x, b.y, b.s)
        assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, cert
        np.testing.assert_array_equal(b.x, c.x)  # deterministic


@pytest.mark.parametrize("name", ["manhattan", "graph3d"])
def test_newton_kernels_against_the_oracle(name, fixtures, hip_lib):
    """Kernel-level parity of the semismooth-Newton polish: the gradient (k_newton_cone_b + k_spmv<GRAD>), the
    generalised Hessian the device assembles (k_hassemble on the host-built pattern) and the chain
    factorisation (k_factor, applied through the chain kernel) are compared, entry by entry, with the
    oracle's ReducedProblem.grad_hess at the same point -- an ADMM iterate, far from the optimum, with a
    mixed set of active and slack cones."""
    import scipy.sparse as sp

    fg = graph_by_name(name, fixtures)
    mdl = assemble(fg, "SOCP")
    d = mdl.dim
    sol = ConicSolver(mdl.qp, dict(adaptive_rho=0, fac_fp32=0))  # factors in double: the chain solve is exact
    sol.reset()
    sol.steps(15)
    assert sol.debug_get("polish_assemble_at_x").size == 1
    D = sol.debug_get("D")
    xhat = sol.debug_get("x")
    n = mdl.qp.n
    Hm = sp.csr_matrix((sol.debug_get("Hval"), sol.debug_get("Hcol").astype(np.int64), sol.debug_get("Hptr").astype(np.int64)), shape=(n, n))
    g = sol.debug_get("polish_g")
    head = sol.debug_get("is_head") > 0
    # the same point in the oracle's variables
    rp = so.ReducedProblem(fg)
    xm = mdl.expand(xhat * D)
    u = np.zeros(rp.n)
    omap = -np.ones(mdl.n_model, dtype=np.int64)  # model column -> oracle column
    PB = d * (d + 1)
    for i, nm in enumerate(mdl.pose_names):
        if nm != rp.first_pose:
            omap[i * PB : (i + 1) * PB] = rp.col[nm] + np.arange(PB)
    for i, nm in enumerate(mdl.landmark_names):
        omap[mdl.lm_base + i * d : mdl.lm_base + (i + 1) * d] = rp.col[nm] + np.arange(d)
    sel = omap >= 0
    u[omap[sel]] = xm[sel]
    go, Ho = rp.grad_hess(u)
    dl = rp.deltas(u)
    n_active = int((np.linalg.norm(dl, axis=1) > rp.dist).sum())
    assert 0 < n_active < rp.nr  # a genuinely mixed active set
    oc = omap[mdl.free_cols]  # solver column -> oracle column (-1: range variable = eliminated head)
    assert np.array_equal(oc < 0, head)
    nh = np.nonzero(~head)[0]
    # gradient: g_product = D g_oracle
    np.testing.assert_allclose(g[nh], D[nh] * go[oc[nh]], rtol=0, atol=1e-9 * np.abs(go).max() * D.max())
    assert np.all(g[head] == 0.0)
    # Hessian: H_product = D H_oracle D (+ the 1e-9 diagonal regularisation) on the non-head block
    Hd = Hm[nh][:, nh].toarray() if len(nh) <= 4000 else None
    Ho_perm = Ho.tocsr()[oc[nh]][:, oc[nh]]
    ref = sp.diags(D[nh]) @ Ho_perm @ sp.diags(D[nh])
    diff = (Hm[nh][:, nh] - ref - 1e-9 * sp.identity(len(nh))).tocsr()
    scale = abs(ref).max()
    assert abs(diff).max() <= 1e-10 * scale, (abs(diff).max(), scale)
    del Hd
    # head rows are decoupled unit rows
    Hh = Hm[np.nonzero(head)[0]]
    assert Hh.nnz == int(head.sum()) and np.all(Hh.data == 1.0)
    # chain factorisation: z = M^-1 (-g) must solve the block-tridiagonal chain part T of the SAME H exactly,
    # and be the Jacobi quotient on the other columns
    from operator_helpers import chain_nodes_of_ids, preconditioned_matrix

    z = sol.debug_get("polish_prec_of_negg")
    bs = mdl.qp.block_size
    chain, node = chain_nodes_of_ids(sol.debug_get("chain_id_of_col"), bs)
    # ... plus the loop-closure blocks (round 6, csrc/score_link.hpp: the Woodbury correction makes the preconditioner the exact
    # inverse of chains + the blocks between linked nodes; graph3d has one loop closure)
    pairs = sol.debug_get("link_pairs").astype(np.int64).reshape(-1, 2)
    assert len(pairs) == (3 if name == "graph3d" else 0)
    T, inchain = preconditioned_matrix(Hm, chain, node, bs, pairs)
    resid = (T @ z + g)[inchain]
    assert np.abs(resid).max() <= 1e-9 * max(1.0, np.abs(g).max()), np.abs(resid).max()
    other = ~inchain
    np.testing.assert_allclose(z[other], -g[other] / Hm.diagonal()[other], rtol=1e-12, atol=1e-300)
    sol.close()
    # fac_fp32 = 2 (Newton factors kept to float precision too, 4-byte factor stream in the chain kernel): the same
    # solve to float eps times the conditioning of the chain blocks
    sol = ConicSolver(mdl.qp, dict(adaptive_rho=0, fac_fp32=2))
    sol.reset()
    sol.steps(15)
    assert sol.debug_get("polish_assemble_at_x").size == 1
    z32, g32 = sol.debug_get("polish_prec_of_negg"), sol.debug_get("polish_g")
    sol.close()
    zs = np.abs(z[inchain]).max()
    assert np.abs(z32 - z)[inchain].max() <= 1e-3 * zs, (np.abs(z32 - z)[inchain].max(), zs)
    assert np.abs((T @ z32 + g32)[inchain]).max() <= 1e-4 * max(1.0, np.abs(g32).max())


@pytest.mark.parametrize("name", ["manhattan", "synth_a"])
def test_intermediate_iterates_on_the_default_trajectory(name, fixtures, hip_lib, twin_lib):
    """score/solve_score.py:89-116 on the GPU: ONE run of the product's default solver, paused every 3
    ADMM iterations of the warm-up (6 by default) and after every Newton iteration of the polish.  Every ADMM snapshot
    equals the CPU twin's iterate at the same iteration count; along the Newton phase the objective
    gap shrinks and the snapshots are exactly primal-feasible; `solved` is the solver's own status;
    the last snapshot is the golden optimum."""
    fg = graph_by_name(name, fixtures)
    gold = load_golden(name)
    its = solve_problem_with_intermediate_iterates(fg, "SOCP", every=3)
    admm = [r for r in its if r.info["newton_iters"] == 0]
    newton = [r for r in its if r.info["newton_iters"] > 0]
    assert [r.info["iters"] for r in admm] == [3, 6] and len(newton) >= 2
    assert [r.info["newton_iters"] for r in newton] == list(range(1, len(newton) + 1))
    assert all(r.info["iters"] == 6 for r in newton)
    assert [r.solved for r in its[:-1]] == [False] * (len(its) - 1) and its[-1].solved
    # ADMM snapshots against the twin, iterate by iterate
    qp = assemble(fg, "SOCP").qp
    cpu = ConicSolver(qp, {}, lib_path=twin_lib)
    cpu.reset()
    for r in admm:
        b = cpu.steps(3)[0]
        assert b.info["iters"] == r.info["iters"]
        # (default settings: chain factors kept to float precision on both sides -> float-eps agreement)
        assert r.info["pobj"] == pytest.approx(b.info["pobj"], rel=1e-6, abs=1e-6)
        assert r.info["res_pri"] == pytest.approx(b.info["res_pri"], rel=1e-3, abs=1e-9)
    cpu.close()
    # Newton snapshots: exactly feasible points whose objective decreases to the optimum
    obj = [r.info["pobj"] for r in newton]
    assert all(r.info["res_pri"] <= 1e-9 for r in newton)
    assert all(obj[i + 1] <= obj[i] + 1e-9 * max(1.0, abs(obj[i])) for i in range(len(obj) - 1))
    assert obj[-1] == pytest.approx(float(gold["objective"]), rel=1e-8, abs=1e-8)
    compare_with_golden(its[-1], gold, pose_tol=1e-6)
    full = solve_score(fg, "SOCP")
    assert abs(full.info["newton_iters"] - len(newton)) <= 1  # the paused run is the run solve_score makes


def test_goats_example_script_runs_on_the_pickle(hip_lib, tmp_path):
    """BASELINE configs[0]: the (corrected) example script on the reference's own pickle, HIP library."""
    import subprocess
    import sys

    from conftest import GOLDEN, ROOT
    from score_amd.io import load_tum

    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "solve_goats_example_score.py"),
                          os.path.join(GOLDEN, "goats_14_6_2002_15_20.pkl")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "solved=True" in out.stdout and "objective=330.48" in out.stdout, out.stdout
    est = load_tum("/tmp/goats_score_A.tum")
    assert est.shape == load_tum(os.path.join(GOLDEN, "gt_traj_A.tum")).shape
    # ... followed by the local refinement on the same GPU, which can only lower the maximum-likelihood cost
    line = [l for l in out.stdout.splitlines() if l.startswith("refined: cost")]
    assert line, out.stdout
    c0, c1 = (float(x) for x in line[0].split("cost")[1].split("in")[0].split("->"))
    assert c1 <= c0
    assert load_tum("/tmp/goats_refined_A.tum").shape == est.shape


@pytest.mark.parametrize("n_poses", [255, 300, 640, 1000, 1023])
def test_split_chain_kernel_matches_the_twin(n_poses, hip_lib, twin_lib):
    """chain_split=1: every chain of >= 256 poses is cut at the nodes of its last nested-dissection level
    into 2-4 parts, each solved by its own workgroup (k_prec_wave) with one in-kernel exchange; shorter
    chains run the same kernel as a single part.  Same factor, same operator: 40 ADMM iterations must
    reproduce the CPU twin's iterates, the default (unsplit) kernel's, and the full solver must agree."""
    fg = make_manhattan(n_robots=3, n_poses=n_poses, n_beacons=3, seed=31 + n_poses)
    qp = assemble(fg, "SOCP").qp
    outs = {}
    for name, lib, extra in (("split", None, dict(chain_split=1)), ("plain", None, dict(chain_split=0)), ("twin", twin_lib, {})):
        sol = ConicSolver(qp, dict(polish=0, adaptive_rho=0, adaptive_cg=0, **extra), lib_path=lib)
        outs[name] = sol.steps(40)[0]
        sol.close()
    scale = np.abs(outs["twin"].x).max()
    np.testing.assert_allclose(outs["split"].x, outs["twin"].x, atol=1e-7 * scale)
    np.testing.assert_allclose(outs["split"].x, outs["plain"].x, atol=1e-9 * scale)
    a = ConicSolver(qp, dict(chain_split=1)); ra = a.solve()[0]; a.close()
    b = ConicSolver(qp, dict(chain_split=0)); rb = b.solve()[0]; b.close()
    assert ra.solved and rb.solved and ra.info["pobj"] == pytest.approx(rb.info["pobj"], rel=1e-9)
    cert = so.kkt_certificate(qp.P, qp.q, qp.A, qp.b, 0, qp.soc_dims, ra.x, ra.y, ra.s)
    assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, cert


def test_config5_all_64_trials_are_certified(hip_lib):
    """BASELINE configs[4] at its full size: 64 four-robot x 1000-pose Monte-Carlo trials, solved
    the way bench.py solves them (lock-step handles of 16, product default solver).  EVERY trial
    must carry a solver-independent KKT certificate, and four of them are compared pose by pose
    with the oracle's Newton solve (north_star: 1e-4 relative)."""
    import bench

    args = bench.parse_args([])
    mc = bench.MonteCarlo(args, range(64), 0, None)
    assert mc.group_sizes == [16, 16, 16, 16]
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=4) as pool:
        sols = mc.sweep(pool)
    mc.close()
    assert len(sols) == 64 and all(o.solved for o in sols)
    for t, (mdl, out) in enumerate(zip(mc.models, sols)):
        qp = mdl.qp
        cert = so.kkt_certificate(qp.P, qp.q, qp.A, qp.b, 0, qp.soc_dims, out.x, out.y, out.s)
        assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, (t, cert)
        assert cert["s_cone_dist"] < 1e-9 and cert["y_cone_dist"] < 1e-9, (t, cert)
        assert cert["gap"] < 1e-4 * max(1.0, abs(out.info["pobj"])), (t, cert)
    for t in (0, 21, 42, 63):
        fg = make_manhattan(n_robots=4, n_poses=1000, n_beacons=4, seed=bench.MC_SEED0 + t)
        rp, u, info = so.newton_solve(fg, tol=1e-12)
        assert sols[t].info["pobj"] == pytest.approx(info["objective"], rel=1e-6)
        ref = so.reduced_to_values(rp, u, "SOCP")
        mdl = mc.models[t]
        blocks = mdl.pose_blocks(mdl.expand(sols[t].x))
        scale = max(np.abs(v[:, 2]).max() for v in ref["poses"].values())
        worst = max(np.abs(blocks[i] - ref["poses"][nm]).max() for i, nm in enumerate(mdl.pose_names))
        assert worst / scale < 1e-4, (t, worst / scale)


def test_bench_montecarlo_mode_reports_a_contract_line(hip_lib):
    """bench.py --montecarlo (BASELINE config 5): lock-step groups, one JSON line with the contract keys."""
    import json
    import subprocess
    import sys

    from conftest import ROOT

    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "montecarlo", "--montecarlo", "4", "--mc-batch", "2",
         "--mc-threads", "2", "--steps", "1", "--warmup", "1"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in rec
    assert rec["metric"] == "problems_per_sec" and rec["value"] > 0 and rec["legs"]["problems_solved_last_sweep"] == 4
    assert len(out.stdout.strip().splitlines()[-1]) <= 4096


@pytest.mark.parametrize("d", [2, 3])
def test_device_rounding_matches_reference_vectors_and_the_twin(d, hip_lib, twin_lib):
    """k_round_so through score_round_to_so: the reference-generated golden vectors, then a 50 000-block
    stack against the CPU twin's loop over the same per-block function (fp64: reassociation only) and,
    on the well-conditioned blocks, against the oracle's SVD restatement."""
    from conftest import GOLDEN
    from score_amd.rounding import round_to_special_orthogonal
    from score_amd.solver import load_library

    _hip_only(hip_lib)
    hip, twin = load_library(hip_lib), load_library(twin_lib)
    z = np.load(os.path.join(GOLDEN, "rounding_golden.npz"))
    M, R = z[f"in_{d}d"], z[f"out_{d}d"]
    full_rank = np.abs(z[f"det_{d}d"]) > 1e-6
    got = round_to_special_orthogonal(M, lib=hip)
    np.testing.assert_allclose(got[full_rank], R[full_rank], atol=1e-10)
    rng = np.random.default_rng(40 + d)
    big = rng.normal(size=(50000, d, d))
    q, _ = np.linalg.qr(rng.normal(size=(20000, d, d)))
    big[:20000] = q + 1e-3 * rng.normal(size=(20000, d, d))
    big[20000:22000] *= 10.0 ** rng.uniform(-6, 6, size=(2000, 1, 1))
    g_hip, g_twin = round_to_special_orthogonal(big, lib=hip), round_to_special_orthogonal(big, lib=twin)
    sv = np.linalg.svd(big, compute_uv=False)
    det = np.linalg.det(big)
    margin = np.where(det > 0, sv[:, -1] + sv[:, -2], sv[:, -2] - sv[:, -1]) / sv[:, 0]
    ok = margin > 1e-3
    np.testing.assert_allclose(g_hip[ok], g_twin[ok], atol=1e-11)
    np.testing.assert_allclose(g_hip @ np.swapaxes(g_hip, 1, 2), np.tile(np.eye(d), (len(big), 1, 1)), atol=1e-9)
    idx = np.flatnonzero(ok)[:3000]
    ref = np.stack([so.round_to_special_orthogonal(m) for m in big[idx]])
    np.testing.assert_allclose(g_hip[idx], ref, atol=1e-9)
    with pytest.raises(ValueError, match="Could not round"):
        round_to_special_orthogonal(np.full((3, d, d), np.nan), lib=hip)


def test_linear_mode_and_refinement_on_the_gpu(hip_lib, twin_lib):
    """f4: the damped Gauss-Newton normal equations of the local refinement, solved by k_factor +
    k_prec_pre + k_spmv through score_linear_solve.  (1) same PCG as the CPU twin's loop (same solution; the
    iteration counts within 10 % -- the graph has loop closures, and the link correction of the preconditioner on
    float factors agrees between the two to 1e-3 only), equal to SciPy's direct solve; (2) refinement through the HIP library reaches the
    cost of the sparse-LU variant; (3) at 20 robots x 1000 poses the solve meets its residual bound."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    from score_amd.refine import _DeviceNormalEquations, _initial_point, _Problem, refine_estimate

    _hip_only(hip_lib)
    fg = make_manhattan(n_robots=4, n_poses=300, n_beacons=3, seed=21, p_range=0.3, n_loop_closures=6, sigma_t=0.05, sigma_theta=0.02)
    res = solve_score(fg, "SOCP", lib_path=hip_lib)
    assert res.solved
    prob = _Problem(fg)
    u = _initial_point(prob, res)
    r, J = prob.residuals(u, jac=True)
    H, g = (J.T @ J).tocsr(), J.T @ r
    out = {}
    for name, lib in (("hip", hip_lib), ("twin", twin_lib)):
        dev = _DeviceNormalEquations(prob, J, lib, None)
        x, info = dev.solver.solve(dev.values(H) + 0.0, -g, rel_tol=1e-11, max_iters=2000, residual=True)
        v = dev.values(H); v[dev.diag] += 1e-4
        x2, info2 = dev.solver.solve(v, -g, rel_tol=1e-11, max_iters=2000, residual=True)
        out[name] = (x, info, x2, info2)
        dev.close()
    for k in (1, 3):
        assert out["hip"][k]["converged"] and abs(out["hip"][k]["iters"] - out["twin"][k]["iters"]) <= max(1, out["twin"][k]["iters"] // 10)
    scale = np.abs(out["twin"][2]).max()
    np.testing.assert_allclose(out["hip"][2], out["twin"][2], atol=1e-8 * scale)
    ref = spla.spsolve((H + 1e-4 * sp.identity(prob.n)).tocsc(), -g)
    np.testing.assert_allclose(out["hip"][2], ref, atol=1e-7 * max(1.0, np.abs(ref).max()))
    refined, info = refine_estimate(fg, res, lib_path=hip_lib)  # whole loop on the device (score_refine_run)
    by_twin, info_twin = refine_estimate(fg, res, lib_path=twin_lib)  # the same loop, kernels as CPU loops
    by_py, info_py = refine_estimate(fg, res, lib_path=hip_lib, engine="python")  # host Jacobians, device solves
    by_lu, info_lu = refine_estimate(fg, res, linear_solver="scipy")
    assert info["engine"] == "native" and info["pcg_iters"] > 0
    assert info["iterations"] == info_twin["iterations"] == info_py["iterations"]
    assert info["cost_initial"] == pytest.approx(info_twin["cost_initial"], rel=1e-13)
    for other in (info_twin, info_py, info_lu):
        assert info["cost_final"] == pytest.approx(other["cost_final"], rel=1e-8)
    for nm in refined.poses:
        np.testing.assert_allclose(refined.poses[nm], by_twin.poses[nm], atol=1e-6)
        np.testing.assert_allclose(refined.poses[nm], by_lu.poses[nm], atol=1e-4)
    assert info["cost_final"] <= info["cost_initial"]
    # BASELINE size (configs[3]): residual bound of one damped solve
    big = make_config(3) if False else make_manhattan(n_robots=20, n_poses=1000, n_beacons=4, seed=3000)
    rb = solve_score(big, "SOCP", lib_path=hip_lib)
    pb = _Problem(big)
    ub = _initial_point(pb, rb)
    r, J = pb.residuals(ub, jac=True)
    dev = _DeviceNormalEquations(pb, J, hip_lib, None)
    v = dev.values((J.T @ J).tocsr()); v[dev.diag] += 1e-6
    x, info = dev.solver.solve(v, -(J.T @ r), rel_tol=1e-8, max_iters=4000, residual=True)
    dev.close()
    assert info["converged"] and info["rel_residual"] < 1e-5 and np.all(np.isfinite(x))


def test_long_pcg_verdict_on_the_gpu(hip_lib):
    from test_refine import check_long_pcg_verdict

    _hip_only(hip_lib)
    check_long_pcg_verdict(hip_lib)


def test_refinement_edge_cases_on_the_gpu(hip_lib):
    from test_refine import check_refinement_edge_cases

    _hip_only(hip_lib)
    check_refinement_edge_cases(hip_lib)


def test_random_3d_graphs_are_certified(hip_lib):
    """3-D graphs (block size 4: the streaming chain kernel, SO(3) rounding on the device) of several lengths and
    seeds: the product default solver returns an optimum the oracle certifies, and its objective equals the oracle's
    Newton solve on the smaller ones."""
    from conftest import graph_3d

    _hip_only(hip_lib)
    for seed, n, n_lm in ((1, 12, 3), (2, 25, 3), (3, 64, 5), (4, 130, 3), (5, 300, 5)):
        fg = graph_3d(seed=seed, n=n, n_lm=n_lm)
        mdl = assemble(fg, "SOCP")
        qp = mdl.qp
        sol = ConicSolver(qp, {})
        out = sol.solve()[0]
        sol.close()
        assert out.solved, (seed, n, out.info)
        cert = so.kkt_certificate(qp.P, qp.q, qp.A, qp.b, 0, qp.soc_dims, out.x, out.y, out.s)
        assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, (seed, n, cert)
        res = solve_score(fg, "SOCP")
        for T in res.poses.values():
            R = T[:3, :3]
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-9) and np.linalg.det(R) == pytest.approx(1.0, abs=1e-9)
        if n <= 64:
            rp, u, info = so.newton_solve(fg, tol=1e-12)
            assert out.info["pobj"] == pytest.approx(info["objective"], rel=1e-6, abs=1e-8)


@pytest.mark.parametrize("dims", [(64, 3, 4), (200,), (3, 130, 1, 70)])
def test_large_cones_through_the_abi(dims, hip_lib, twin_lib):
    """The C ABI takes any product of second-order cones, not only SCORE's 3- and 4-row ones (gurobi_utils.py:341-352):
    cones with more than four rows take k_cone's general path (one lane walks the rows of its cone).  Known answer:
    the Euclidean projection of a point c onto the product cone, minimise 1/2 |x - c|^2 s.t. x in K, equals the
    oracle's proj_soc cone by cone -- interior, exterior (-> 0) and boundary cases -- on the GPU and on the twin."""
    import scipy.sparse as sp

    from score_amd.assemble import ConicQP

    rng = np.random.default_rng(sum(dims))
    n = int(sum(dims))
    c = rng.normal(size=n)
    off, expect = 0, np.zeros(n)
    for i, dm in enumerate(dims):
        blk = c[off : off + dm]
        if dm > 1:
            if i % 3 == 0:
                blk[0] = 0.3 * np.linalg.norm(blk[1:])        # outside: projected onto the boundary
            elif i % 3 == 1:
                blk[0] = 2.0 * np.linalg.norm(blk[1:]) + 0.1  # inside: unchanged
            else:
                blk[0] = -2.0 * np.linalg.norm(blk[1:]) - 0.1  # in the polar cone: projected to 0
        expect[off : off + dm] = so.proj_soc(blk)
        off += dm
    qp = ConicQP(P=sp.identity(n, format="csr"), q=-c, c0=0.5 * float(c @ c), A=(-sp.identity(n, format="csr")), b=np.zeros(n), z=0,
                 soc_dims=np.asarray(dims, dtype=np.int32))
    for lib in (hip_lib, twin_lib):
        sol = ConicSolver(qp, dict(eps_abs=1e-9, eps_rel=1e-9, max_iters=5000), lib_path=lib)
        out = sol.solve()[0]
        sol.close()
        assert out.solved, out.info
        np.testing.assert_allclose(out.x, expect, atol=1e-6)
        np.testing.assert_allclose(out.s, expect, atol=1e-6)  # s = b - A x = x
        assert out.info["pobj"] == pytest.approx(0.5 * float((expect - c) @ (expect - c)), abs=1e-6)


@pytest.mark.parametrize("n_poses", [40, 333, 1000])
def test_3d_chain_kernels_match_the_twin(n_poses, hip_lib, twin_lib):
    """3-D problems (gurobi_utils.py:37-50: dimension 3 -> 3 x 4 pose matrices, chains of 4 x 4 blocks, three replicas):
    with the 4-byte factor stream (the default) the LDS-resident chain kernel k_prec_pre<4, ., float> runs -- level-0
    tile and coarse-level factors kept as floats, converted where used -- with double factors the streaming kernel
    k_prec<4>.  Both against the CPU twin after k ADMM iterations, and the full default solve against the oracle."""
    from score_amd.manhattan import make_manhattan_3d

    _hip_only(hip_lib)
    fg = make_manhattan_3d(n_robots=2, n_poses=n_poses, n_beacons=3, seed=31, p_range=0.3)
    qp = assemble(fg, "SOCP").qp
    assert qp.block_size == 4 and qp.rep_d == 3
    for fp32, tol in ((0, 1e-9), (1, 2e-5)):
        st = dict(adaptive_cg=0, adaptive_rho=0, check_interval=5, fac_fp32=fp32, polish=0)
        gpu = ConicSolver(qp, st, lib_path=hip_lib)
        cpu = ConicSolver(qp, st, lib_path=twin_lib)
        assert gpu.debug_get("rep")[0] == 3
        gpu.reset(); cpu.reset()
        for k in (1, 7):
            a, b = gpu.steps(k)[0], cpu.steps(k)[0]
            for v in VECS:
                ga, gb = gpu.debug_get(v), cpu.debug_get(v)
                scale = max(1.0, np.abs(gb).max())
                vtol = 1e-4 if (fp32 and v in ("r", "z", "p", "w")) else tol
                assert np.abs(ga - gb).max() <= vtol * scale, (v, k, fp32, np.abs(ga - gb).max(), scale)
        gpu.close(); cpu.close()
    if n_poses <= 333:
        res = solve_score(fg, "SOCP")
        rp, u, info = so.newton_solve(fg, tol=1e-12, max_iter=300)
        assert res.solved and res.info["newton_iters"] > 0
        assert res.info["pobj"] == pytest.approx(info["objective"], rel=1e-7, abs=1e-8)


def test_3d_refinement_on_the_gpu(hip_lib, twin_lib):
    """f4 in 3-D: SE(3) Gauss-Newton / LM behind score_refine_run on the device (k_gn_blocks<3>: 12 x 12 relative-pose
    blocks; k_gn_trial<3>: the retraction R Exp(omega), t + v; normal equations through the chain-preconditioned PCG
    with the omega and v chains of every robot) -- against SciPy's least_squares / sparse LU (check_3d_refinement) and
    against the CPU twin of the same loop; then on a larger graph: same LM iterations as the twin."""
    from test_refine import _graph3, _noisy_truth3, check_3d_refinement

    from score_amd.manhattan import make_manhattan_3d
    from score_amd.refine import refine_estimate

    _hip_only(hip_lib)
    check_3d_refinement(hip_lib)
    fg = _graph3()
    res = _noisy_truth3(fg)
    a, ia = refine_estimate(fg, res, lib_path=hip_lib)
    b, ib = refine_estimate(fg, res, lib_path=twin_lib)
    assert (ia["iterations"], ia["linear_solves"]) == (ib["iterations"], ib["linear_solves"])
    assert ia["cost_final"] == pytest.approx(ib["cost_final"], rel=1e-8)
    for nm in a.poses:
        np.testing.assert_allclose(a.poses[nm], b.poses[nm], atol=1e-6)
    fg = make_manhattan_3d(n_robots=3, n_poses=400, n_beacons=4, seed=47, p_range=0.2, sigma_t=0.05, sigma_theta=0.02)
    res = _noisy_truth3(fg, seed=3)
    a, ia = refine_estimate(fg, res, lib_path=hip_lib)
    b, ib = refine_estimate(fg, res, lib_path=twin_lib)
    assert ia["iterations"] == ib["iterations"] and ia["cost_final"] == pytest.approx(ib["cost_final"], rel=1e-7)
    assert ia["cost_final"] < 0.05 * ia["cost_initial"] and ia["grad_inf"] < 1e-5 * max(1.0, ia["cost_final"])


@pytest.mark.parametrize("name,relax", [("manhattan", "SOCP"), ("graph3d", "SOCP"), ("synth_d", "QCQP"), ("goats", "SOCP")])
def test_device_equilibration_equals_the_host_loop(name, relax, fixtures, hip_lib, twin_lib, monkeypatch):
    """f2: the passes of the Ruiz equilibration run on the device for a single problem (k_ruiz_cols: a wavefront per
    column of [[P, A'], [A, 0]]; k_ruiz_groups: one scale per cone; k_ruiz_apply) -- the scales D, E must be the ones
    the host loop computes (ruiz_scale, which the twin runs): same formulas, so equal to rounding; replicated problems
    (2 and 3 replicas), the direct QCQP form, and the switch back to the host loop (SCORE_NO_DEVICE_RUIZ)."""
    _hip_only(hip_lib)
    qp = assemble(graph_by_name(name, fixtures), relax).qp
    monkeypatch.delenv("SCORE_NO_DEVICE_RUIZ", raising=False)
    dev = ConicSolver(qp, dict(polish=0), lib_path=hip_lib)
    monkeypatch.setenv("SCORE_NO_DEVICE_RUIZ", "1")
    host = ConicSolver(qp, dict(polish=0), lib_path=hip_lib)
    monkeypatch.delenv("SCORE_NO_DEVICE_RUIZ", raising=False)
    twin = ConicSolver(qp, dict(polish=0), lib_path=twin_lib)
    for v in ("D", "E"):
        a, b, c = dev.debug_get(v), host.debug_get(v), twin.debug_get(v)
        assert a.min() > 0
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
        np.testing.assert_allclose(a, c, rtol=1e-12, atol=0)
    np.testing.assert_allclose(dev.debug_get("Kval"), host.debug_get("Kval"), rtol=1e-11, atol=1e-300)
    for s_ in (dev, host, twin):
        s_.close()


# Every environment switch the library still reads (conftest.SURVIVING_SWITCHES) must still compute the golden optimum.  One child
# process per switch: several are read once per process.
from conftest import SURVIVING_SWITCHES  # noqa: E402

_SWITCH_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
from conftest import compare_with_golden, graph_by_name, load_golden, load_fixtures
from score_amd.solve_score import solve_score
fx = load_fixtures()
for name, relax, mode in (("manhattan", "SOCP", "via_socp"), ("synth_b", "SOCP", "via_socp"), ("graph3d", "QCQP", "via_socp"), ("synth_d", "QCQP", "direct")):
    res = solve_score(graph_by_name(name, fx), relax, qcqp_mode=mode)
    gold = load_golden(name)
    assert res.solved and res.info["backend"] == "hip-gfx950", res.info
    assert abs(res.info["pobj"] - float(gold["objective"])) <= 1e-5 * max(1.0, abs(float(gold["objective"]))), (name, res.info["pobj"], float(gold["objective"]))
    compare_with_golden(res, gold, pose_tol=1e-4)
print("SWITCH_OK")
"""


@pytest.mark.parametrize("switch,value", SURVIVING_SWITCHES)
def test_every_surviving_switch_still_reaches_the_golden_optimum(switch, value, hip_lib):
    import subprocess
    import sys as _sys

    from conftest import ROOT

    _hip_only(hip_lib)
    code = _SWITCH_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([_sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, **{switch: value}))
    assert out.returncode == 0 and "SWITCH_OK" in out.stdout, (switch, out.stdout[-800:], out.stderr[-2500:])


def _links_info(sol):
    v = sol.debug_get("links")
    return dict(pairs=int(v[0]), used=int(v[1]), unknowns=int(v[2]), chains=int(v[3]), rounds=int(v[4]), singular=int(v[5]))


@pytest.mark.parametrize("case", ["2d", "3d", "segments", "batch"])
def test_loop_closures_inside_the_newton_preconditioner(case, fixtures, hip_lib, monkeypatch):
    """Round 6 (csrc/score_link.hpp): a loop closure (gurobi_utils.py:407-430) is a relative-pose term between poses that are no
    neighbours in a chain -- as stiff as odometry, and outside the block-tridiagonal chain preconditioner: 30-60 PCG iterations per
    Newton step.  The Newton set's chain solve now carries the Woodbury correction for those blocks (exact inverse of chains +
    loop-closure blocks).  Against SCORE_NO_LINKS=1 (the chain preconditioner alone): the same optimum -- objective, x, KKT
    certificate of the program as given, the oracle's objective -- in at most HALF the PCG iterations; through the array path
    (links found in P's pattern) and the graph path (links from the measurement list); 2-D, 3-D (4 x 4 blocks), chains cut into
    segments (second level + links), and a lock-step batch in which one graph has no loop closure."""
    from score_amd.manhattan import make_manhattan_3d
    from score_amd.native import assemble_native, graph_arrays

    _hip_only(hip_lib)
    if case == "2d":
        graphs = [make_manhattan(n_robots=2, n_poses=397, n_beacons=3, seed=1008, p_range=0.115, n_loop_closures=2)]
    elif case == "3d":
        graphs = [make_manhattan_3d(n_robots=2, n_poses=300, n_beacons=3, seed=32, p_range=0.2, n_loop_closures=2)]
    elif case == "segments":
        graphs = [make_manhattan(n_robots=2, n_poses=2570, n_beacons=2, seed=1002, p_range=0.08, n_loop_closures=3)]
    else:
        graphs = [make_manhattan(n_robots=2, n_poses=200, n_beacons=3, seed=71, n_loop_closures=2), make_manhattan(n_robots=2, n_poses=260, n_beacons=3, seed=72),
                  make_manhattan(n_robots=3, n_poses=150, n_beacons=2, seed=73, n_loop_closures=3)]
    qps = [assemble_native(g, "SOCP", lib_path=hip_lib).qp for g in graphs]  # (the host assembler: bit-equal to the device's)
    outs = {}
    for name, env in (("links", None), ("plain", "1")):
        if env:
            monkeypatch.setenv("SCORE_NO_LINKS", env)
        else:
            monkeypatch.delenv("SCORE_NO_LINKS", raising=False)
        sol = ConicSolver(qps, {}, lib_path=hip_lib)
        info = _links_info(sol)
        outs[name] = (sol.solve(), info)
        assert _links_info(sol)["singular"] == 0
        sol.close()
    monkeypatch.delenv("SCORE_NO_LINKS", raising=False)
    (a, ia), (b, ib) = outs["links"], outs["plain"]
    n_lc = sum(len(g.loop_closure_measurements) for g in graphs)
    assert 0 < ia["used"] <= n_lc * graphs[0].dimension and ia["unknowns"] > 0 and ia["rounds"] >= graphs[0].dimension + 1, ia
    assert ib["used"] == 0 and ib["chains"] == 0, ib
    for k, qp in enumerate(qps):
        assert a[k].solved and b[k].solved, (a[k].info, b[k].info)
        assert a[k].info["pobj"] == pytest.approx(b[k].info["pobj"], rel=1e-7, abs=1e-7)
        scale = max(1.0, np.abs(b[k].x).max())
        np.testing.assert_allclose(a[k].x, b[k].x, atol=2e-5 * scale)
        cert = so.kkt_certificate(qp.P, qp.q, qp.A, qp.b, 0, qp.soc_dims, a[k].x, a[k].y, a[k].s)
        assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, cert
    with_lc = [k for k, g in enumerate(graphs) if len(g.loop_closure_measurements)]
    pcg_a = sum(a[k].info["newton_cg_iters"] for k in with_lc) if case != "batch" else a[0].info["newton_cg_iters"]
    pcg_b = sum(b[k].info["newton_cg_iters"] for k in with_lc) if case != "batch" else b[0].info["newton_cg_iters"]
    assert 2 * pcg_a <= pcg_b, (pcg_a, pcg_b)
    if case in ("2d", "3d"):
        rp, u, info = so.newton_solve(graphs[0], tol=1e-12)
        assert a[0].info["pobj"] == pytest.approx(info["objective"], rel=1e-6, abs=1e-7)
    # the graph path (score_create_from_graphs: links from the measurement list) finds the same links: the same handle, bit for bit
    gsol = ConicSolver.from_graphs([graph_arrays(g) for g in graphs], 0, {}, lib_path=hip_lib)
    assert _links_info(gsol) == ia
    gi, _ = gsol.solve_estimates()
    gsol.close()
    for k, info in enumerate(gi):
        assert info["status"] == 1 and info["newton_cg_iters"] == a[k].info["newton_cg_iters"] and info["pobj"] == a[k].info["pobj"], (k, info, a[k].info)
    # ... and through solve_score_batch (which starts loop-closure graphs with more ADMM PCG iterations: another warm-up point)
    res = solve_score_batch(graphs, "SOCP", lockstep=True, solver_settings=dict(device=0))
    for k, r in enumerate(res):
        assert r.solved and r.info["pobj"] == pytest.approx(a[k].info["pobj"], rel=1e-7, abs=1e-7)
    assert 2 * sum(res[k].info["newton_cg_iters"] for k in with_lc) <= sum(b[k].info["newton_cg_iters"] for k in with_lc)


def test_loop_closure_edge_cases_in_the_link_correction(hip_lib, monkeypatch):
    """Loop closures the generators never draw: BETWEEN robots (what a multi-session data set has), onto the pinned pose (a
    constant, no unknown), between chain neighbours (a second odometry edge: inside the chain already), the same pair twice.
    Array path and graph path must find the same links (bit-equal handles), the optimum must be the one without the correction
    and the oracle's."""
    from score_amd import compat
    from score_amd.native import assemble_native, graph_arrays

    _hip_only(hip_lib)
    fg = make_manhattan(n_robots=3, n_poses=150, n_beacons=3, seed=77, p_range=0.15)
    rng = np.random.default_rng(5)

    def lc(a, i, b, j):
        Ta, Tb = fg.pose_variables[a][i].transformation_matrix, fg.pose_variables[b][j].transformation_matrix
        rel = np.linalg.inv(Ta) @ Tb
        return compat.PoseMeasurement2D(fg.pose_variables[a][i].name, fg.pose_variables[b][j].name, float(rel[0, 2] + 0.01 * rng.standard_normal()),
                                        float(rel[1, 2] + 0.01 * rng.standard_normal()), float(np.arctan2(rel[1, 0], rel[0, 0]) + 0.002 * rng.standard_normal()), 1e4, 2.5e5)

    fg.loop_closure_measurements = [lc(0, 40, 1, 90), lc(2, 10, 1, 30), lc(0, 0, 2, 120), lc(1, 70, 1, 71), lc(0, 100, 0, 20), lc(0, 20, 0, 100), lc(2, 140, 0, 60)]
    qp = assemble_native(fg, "SOCP", lib_path=hip_lib).qp
    outs = {}
    for name, env in (("links", None), ("plain", "1")):
        if env:
            monkeypatch.setenv("SCORE_NO_LINKS", env)
        else:
            monkeypatch.delenv("SCORE_NO_LINKS", raising=False)
        sol = ConicSolver([qp], {}, lib_path=hip_lib)
        outs[name] = (sol.solve()[0], _links_info(sol), sol.debug_get("link_pairs"))
        sol.close()
    monkeypatch.delenv("SCORE_NO_LINKS", raising=False)
    (a, ia, pa), (b, ib, _) = outs["links"], outs["plain"]
    # four real links (A40-B90, C10-B30, A100-A20 once, C140-A60), two rows each: the pinned pose, the neighbours and the
    # repeated pair add none
    assert ia["pairs"] == ia["used"] == 8 and ia["singular"] == 0 and ib["used"] == 0, (ia, ib)
    assert a.solved and b.solved and a.info["pobj"] == pytest.approx(b.info["pobj"], rel=1e-7, abs=1e-7)
    assert 2 * a.info["newton_cg_iters"] <= b.info["newton_cg_iters"], (a.info["newton_cg_iters"], b.info["newton_cg_iters"])
    rp, u, info = so.newton_solve(fg, tol=1e-12)
    assert a.info["pobj"] == pytest.approx(info["objective"], rel=1e-6, abs=1e-7)
    cert = so.kkt_certificate(qp.P, qp.q, qp.A, qp.b, 0, qp.soc_dims, a.x, a.y, a.s)
    assert cert["primal_res_inf"] < 1e-5 and cert["dual_res_inf"] < 1e-4, cert
    g = ConicSolver.from_graphs([graph_arrays(fg)], 0, {}, lib_path=hip_lib)
    assert _links_info(g) == ia and np.array_equal(g.debug_get("link_pairs"), pa)
    gi, _ = g.solve_estimates()
    g.close()
    assert gi[0]["status"] == 1 and gi[0]["newton_cg_iters"] == a.info["newton_cg_iters"] and gi[0]["pobj"] == a.info["pobj"]
