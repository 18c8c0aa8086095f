"""The batched second-order check (score_amd/curvature_batch.py): what runs without a GPU -- the binding table of
include/score_curvature_batch.h, the dense engine member by member, the grouping, the argument errors and the ``curvature``
keyword of ``refine_estimate_batch`` on the python engine.  The device path is tests/test_curvature_batch_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from marginals_helpers import noisy_truth, two_pose_graph
from refine_batch_helpers import member
from score_amd.bindings import CURVATURE_BATCH, LATER_TABLES, TABLES, TABLES_SINCE, ScoreCurvatureBatchInfo, bind
from score_amd.curvature import Curvature, dense_hessian, hessian_spectrum
from score_amd.marginals import _problem_and_point
from score_amd.curvature_batch import CURVATURE_BATCH_SYMBOLS, hessian_spectrum_batch
from score_amd.refine_batch import RefineBatchHandle, refine_estimate_batch
from test_binding_tables_host import SCALARS, _declarations, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_matches_header():
    table = CURVATURE_BATCH
    assert table not in TABLES and table not in LATER_TABLES and table not in TABLES_SINCE and table.name == "curvature_batch"
    assert CURVATURE_BATCH in RefineBatchHandle.headers
    declared = _declarations(table.name)
    assert sorted(declared) == sorted(table) == sorted(CURVATURE_BATCH_SYMBOLS)
    assert sorted(declared) == ["score_curvature_ritz", "score_refine_batch_curvature", "score_refine_batch_hessian_product"]
    lib = bind(_Stub(), table)
    assert bind(lib, table) is lib  # (bound once)
    for sym, params in declared.items():
        argtypes, restype = table[sym]
        assert restype is C.c_int and lib.__dict__[sym].argtypes == argtypes and len(argtypes) == len(params), sym
        for param, typ in zip(params, argtypes):
            is_pointer = typ is C.c_void_p or hasattr(typ, "contents")
            assert ("*" in param) == is_pointer, (sym, param, typ)
            if not is_pointer:
                assert SCALARS[param.split()[-2]] is typ, (sym, param, typ)
    # the info record is the header's, field by field: six int32, three doubles
    with open(os.path.join(ROOT, "include", "score_curvature_batch.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"typedef struct score_curvature_batch_info \{(.*?)\}", text, flags=re.S).group(1)
    fields = [(nm.strip(), SCALARS[typ]) for typ, names in re.findall(r"(int32_t|double)\s+([^;]+);", body) for nm in names.split(",")]
    assert [(nm, typ) for nm, typ in ScoreCurvatureBatchInfo._fields_] == fields
    assert [nm for nm, _ in fields] == ["members", "modes", "block", "rounds", "unconverged", "saddles", "max_residual", "setup_ms", "solve_ms"]
    assert C.sizeof(ScoreCurvatureBatchInfo) == 48


def test_missing_symbol():
    sym = list(CURVATURE_BATCH)[-1]
    with pytest.raises(RuntimeError, match=re.escape(f"{sym} is missing from the library: rebuild it "
                                                     "(the oracle's CPU twin has no eigensolver: engine='python' runs there)")):
        bind(_Stub(lacks=sym), CURVATURE_BATCH)


def test_python_engine_equals_the_single_call_member_by_member():
    """Mixed dimensions, groups of at most two, weights for one graph: every graph comes back at its own place with exactly
    what hessian_spectrum(engine="python") gives on it alone."""
    keys = ("B", "3D0", "C", "E", "3D1")
    fgs, starts = [member(k)[0] for k in keys], [member(k)[1] for k in keys]
    w = np.ones(len(fgs[0].range_measurements))
    w[[1, 5, 9]] = 0.0
    weights = [w, None, None, None, None]
    out = hessian_spectrum_batch(fgs, starts, k=5, range_weights=weights, engine="python", max_group=2)
    assert len(out) == len(keys)
    # 2-D first (B, C | E), then 3-D (3D0, 3D1): the group numbers follow refine_estimate_batch's grouping
    assert [info["group"] for _, info in out] == [0, 2, 0, 1, 2]
    for fg, st, rw, (cur, info) in zip(fgs, starts, weights, out):
        alone, info1 = hessian_spectrum(fg, st, k=5, range_weights=rw, engine="python")
        assert isinstance(cur, Curvature)
        for f in ("values", "vectors", "residuals", "gauss_newton"):
            np.testing.assert_array_equal(getattr(cur, f), getattr(alone, f))
        assert cur.names == alone.names and cur.h_max == alone.h_max and cur.rel_tol == alone.rel_tol and cur.kind == alone.kind
        for nm in alone.names:
            np.testing.assert_array_equal(cur.participation[nm], alone.participation[nm])
        assert {f: info[f] for f in info1} == info1 and info["rounds"] == 0
        assert cur.negative() == alone.negative()
    plain, _ = hessian_spectrum(fgs[0], starts[0], k=5, engine="python")
    assert np.max(np.abs(plain.values - out[0][0].values)) > 0  # the weights reached graph 0


def test_argument_errors_carry_the_graph_index():
    fgs, starts = [member(k)[0] for k in ("C", "B")], [member(k)[1] for k in ("C", "B")]
    kw = dict(engine="python")
    with pytest.raises(ValueError, match=r"graph 1: .*range_weights"):
        hessian_spectrum_batch(fgs, starts, range_weights=[None, np.ones(len(fgs[1].range_measurements) + 1)], **kw)
    with pytest.raises(ValueError, match=r"one entry per graph"):
        hessian_spectrum_batch(fgs, starts, range_weights=[None], **kw)
    with pytest.raises(ValueError, match="one estimate per graph"):
        hessian_spectrum_batch(fgs, starts[:1], **kw)
    with pytest.raises(ValueError, match="engine"):
        hessian_spectrum_batch(fgs, starts, engine="host")
    with pytest.raises(ValueError, match="max_group"):
        hessian_spectrum_batch(fgs, starts, max_group=0, **kw)
    for bad in (dict(k=0), dict(k=17), dict(k=2.5), dict(rel_tol=0.0), dict(rel_tol=-1e-9), dict(max_iters=0), dict(shift=0.0),
                dict(shift=-1e-8)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            hessian_spectrum_batch(fgs, starts, **{**kw, **bad})
    small = two_pose_graph()
    with pytest.raises(ValueError, match=r"graph 1: k = 16 modes of a graph with 3 unknowns"):
        hessian_spectrum_batch([fgs[0], small], [starts[0], noisy_truth(small)], k=16, **kw)


def test_refine_keyword_fills_the_curvature_from_the_dense_path():
    keys = ("C", "B")
    fgs, starts = [member(k)[0] for k in keys], [member(k)[1] for k in keys]
    plain = refine_estimate_batch(fgs, starts, engine="python")
    out = refine_estimate_batch(fgs, starts, engine="python", curvature=4)
    assert all("curvature" not in info for _, info in plain)
    for fg, (res0, info0), (res, info) in zip(fgs, plain, out):
        assert info["cost_final"] == info0["cost_final"] and info["iterations"] == info0["iterations"]  # (the run is the same run)
        cur, cinfo = info["curvature"]
        # the follow-up reads the refined point itself, the single call the point as SolverResults hold it (an angle as a
        # rotation matrix and back): the pairs agree as two sets of approximate eigenpairs of one E do -- Weyl, index by index,
        # with both residuals recomputed against E at the results
        alone, ainfo = hessian_spectrum(fg, res, k=4, engine="python")
        prob, point = _problem_and_point(fg, res, None, None)
        E = dense_hessian(prob, point)
        rho = np.linalg.norm(E @ cur.vectors - cur.vectors * cur.values, axis=0)
        rho_alone = np.linalg.norm(E @ alone.vectors - alone.vectors * alone.values, axis=0)
        assert isinstance(cur, Curvature) and cur.vectors.shape == (prob.n, 4) and cur.gauss_newton.shape == (4,)
        assert np.all(np.abs(cur.values - alone.values) <= rho + rho_alone), (cur.values - alone.values, rho, rho_alone)
        assert np.all(rho <= 2 * cur.rel_tol * cur.h_max)
        assert cinfo["engine"] == "python" and cinfo["group"] == info["group"] and cinfo["rounds"] == 0 and cinfo["iterations"] == 0
        assert cur.kind == alone.kind
    with pytest.raises(ValueError, match="k must be"):
        refine_estimate_batch(fgs, starts, engine="python", curvature=17)
