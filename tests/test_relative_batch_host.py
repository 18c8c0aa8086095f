"""Batched predicted relative poses (score_amd/relative_batch.py): what runs without a GPU -- the plan of
csrc/score_relative_batch_plan.hpp as a stand-alone program (plain and under the host sanitizers), the python engine graph by
graph, the argument errors, and the binding table of include/score_relative_batch.h.  The device path is
tests/test_relative_batch_gpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from refine_batch_helpers import member
from score_amd import bindings
from score_amd.bindings import (LATER_TABLES, RELATIVE_BATCH, TABLES, TABLES_AFTER, TABLES_GROUP_PAIRS, TABLES_LATEST, TABLES_SINCE,
                                ScoreMarginalsBatchInfo, bind)
from score_amd.refine_batch import RefineBatchHandle, refine_estimate_batch
from score_amd.relative import PredictedRelativePoses, predicted_relative_poses
from score_amd.relative_batch import RELATIVE_BATCH_SYMBOLS, predicted_relative_poses_batch
from test_binding_tables_host import SCALARS, _declarations, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitizers"])
def test_plan_program(tmp_path, flags):
    """tests/tools/relative_batch_plan_check.cpp: the plan against tables written by hand for both DP -- a straddling pair, a
    member without pairs, members that drop out mid-way, widths 16, 5 and 1, every argument error."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / "relative_batch_plan_check")
    subprocess.run([gxx, "-std=c++17", *flags, "-I", os.path.join(ROOT, "score_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "relative_batch_plan_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "every branch reached" and run.stderr == ""


def _pose(fg, k, chain=0):
    return fg.pose_variables[chain][k].name


def _same(a, b, info_a, info_b):
    assert isinstance(a, PredictedRelativePoses) and a.pairs == b.pairs and a.dof == b.dof
    for f in ("rotation", "translation", "covariance"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    assert (a.angle is None) == (b.angle is None)
    for f in ("residuals", "iterations"):
        np.testing.assert_array_equal(info_a[f], info_b[f], err_msg=f)
    assert info_a["asymmetry"] == info_b["asymmetry"] and info_a["engine"] == info_b["engine"] == "python"


def test_python_engine_equals_the_single_call_graph_by_graph():
    """A 2-D and a 3-D list, mixed in one call, weights for one graph, a graph that lists none: every graph comes back at its
    own place with exactly what predicted_relative_poses(engine="python") gives on it alone."""
    keys = ("B", "3D0", "C", "3D1", "E")
    fgs, starts = [member(k)[0] for k in keys], [member(k)[1] for k in keys]
    w = np.ones(len(fgs[0].range_measurements))
    w[[1, 5, 9]], w[2] = 0.0, 0.25
    rws = [w, None, None, None, None]
    lws = [np.array([1.0, 0.5, 1.0]), None, None, None, None]
    assert len(fgs[0].loop_closure_measurements) == 3
    pairs = [[(_pose(fgs[0], 0), _pose(fgs[0], 7, 1)), (_pose(fgs[0], 3), _pose(fgs[0], 2))],
             [(_pose(fgs[1], 4), _pose(fgs[1], 9, 1)), (_pose(fgs[1], 5, 1), _pose(fgs[1], 0))],
             [], [(_pose(fgs[3], 2), _pose(fgs[3], 3))], None]
    out = predicted_relative_poses_batch(fgs, starts, pairs, range_weights=rws, loop_closure_weights=lws, engine="python", max_group=2)
    assert len(out) == 5
    for fg, st, rw, lw, nm, (pred, info) in zip(fgs, starts, rws, lws, pairs, out):
        if not nm:
            dp = 3 if fg.dimension == 2 else 6
            assert pred.pairs == [] and pred.covariance.shape == (0, dp, dp) and pred.rotation.shape == (0, fg.dimension, fg.dimension)
            assert info["engine"] == "python" and info["residuals"].shape == (0, dp) and info["asymmetry"] == 0.0
            continue
        alone, info1 = predicted_relative_poses(fg, st, nm, range_weights=rw, loop_closure_weights=lw, engine="python")
        _same(pred, alone, info, info1)
    assert out[0][0].dof == 3 and out[1][0].dof == 6 and out[3][0].covariance.shape == (1, 6, 6)
    for of in (slice(0, None, 2), slice(1, None, 2)):  # a 2-D list, then a 3-D list, a call each
        got = predicted_relative_poses_batch(fgs[of], starts[of], pairs[of], range_weights=rws[of], loop_closure_weights=lws[of],
                                             engine="python")
        assert len({fg.dimension for fg in fgs[of]}) == 1
        for (a, ia), (b, ib) in zip(got, out[of]):
            _same(a, b, ia, ib)
    assert predicted_relative_poses_batch([], [], [], engine="python") == []


def test_argument_errors_carry_the_graph_index():
    fgs, starts = [member(k)[0] for k in ("C", "B")], [member(k)[1] for k in ("C", "B")]
    some = [(_pose(fgs[1], 3), _pose(fgs[1], 4))]
    landmark = fgs[1].landmark_variables[0].name
    for engine in ("python", "device"):  # (the pairs' errors come before any work: no library is opened)
        kw = dict(engine=engine, lib_path="/nonexistent/libscore_hip.so")
        with pytest.raises(ValueError, match=rf"predicted_relative_poses_batch: graph 1: {landmark} is a landmark: a relative pose joins two poses"):
            predicted_relative_poses_batch(fgs, starts, [[], [(_pose(fgs[1], 3), landmark)]], **kw)
        with pytest.raises(ValueError, match="predicted_relative_poses_batch: graph 1: unknown variable Z9"):
            predicted_relative_poses_batch(fgs, starts, [[], [(_pose(fgs[1], 3), "Z9")]], **kw)
        with pytest.raises(ValueError, match="predicted_relative_poses_batch: graph 0: the pair .* joins a variable to itself"):
            predicted_relative_poses_batch(fgs, starts, [[(_pose(fgs[0], 3), _pose(fgs[0], 3))], some], **kw)
        with pytest.raises(ValueError, match="predicted_relative_poses_batch: graph 1: a pair is two names"):
            predicted_relative_poses_batch(fgs, starts, [[], [(_pose(fgs[1], 3),)]], **kw)
        with pytest.raises(ValueError, match=r"pairs: one entry per graph expected \(2\), got 1"):
            predicted_relative_poses_batch(fgs, starts, [some], **kw)
        with pytest.raises(ValueError, match="block_width"):
            predicted_relative_poses_batch(fgs, starts, [[], some], block_width=17, **kw)
        with pytest.raises(ValueError, match="max_group"):
            predicted_relative_poses_batch(fgs, starts, [[], some], max_group=0, **kw)
    with pytest.raises(ValueError, match="engine must be 'device' or 'python'"):
        predicted_relative_poses_batch(fgs, starts, [[], some], engine="numpy")
    with pytest.raises(ValueError, match=rf"refine_estimate_batch: graph 1: {landmark} is a landmark"):
        refine_estimate_batch(fgs, starts, engine="python", relative=[None, [(_pose(fgs[1], 3), landmark)]])


def test_refine_estimate_batch_python_engine_with_relative():
    """The follow-up on the python engine is predicted_relative_poses(engine="python") at the refined estimates; without the
    keyword nothing changes."""
    fgs, starts = [member(k)[0] for k in ("C", "B")], [member(k)[1] for k in ("C", "B")]
    pairs = [None, [(_pose(fgs[1], 3), _pose(fgs[1], 4, 1)), (_pose(fgs[1], 6, 1), _pose(fgs[1], 0))]]
    out = refine_estimate_batch(fgs, starts, engine="python", relative=pairs)
    plain = refine_estimate_batch(fgs, starts, engine="python")
    for fg, nm, (res, info), (res_p, info_p) in zip(fgs, pairs, out, plain):
        pred, pinfo = info["relative"]
        assert "relative" not in info_p and info["cost_final"] == info_p["cost_final"]
        for name in res_p.poses:
            np.testing.assert_array_equal(res.poses[name], res_p.poses[name])
        if nm is None:
            assert pred.pairs == [] and pred.covariance.shape == (0, 3, 3)
            continue
        alone, info1 = predicted_relative_poses(fg, res_p, nm, engine="python")
        _same(pred, alone, pinfo, info1)


def test_table_matches_header():
    table = RELATIVE_BATCH
    assert TABLES_GROUP_PAIRS == (RELATIVE_BATCH,) and table.name == "relative_batch"
    assert all(table not in group for group in (TABLES, LATER_TABLES, TABLES_SINCE, TABLES_AFTER, TABLES_LATEST))
    assert hasattr(RefineBatchHandle, "relative_covariances")
    declared = _declarations(table.name)
    assert sorted(declared) == sorted(table) == sorted(RELATIVE_BATCH_SYMBOLS) == ["score_refine_batch_relative_covariances"]
    lib = bind(_Stub(), table)
    assert bind(lib, table) is lib  # (bound once)
    for sym, params in declared.items():
        argtypes, restype = table[sym]
        assert restype is C.c_int and lib.__dict__[sym].argtypes == argtypes and len(argtypes) == len(params) == 15, sym
        assert argtypes[-1]._type_ is ScoreMarginalsBatchInfo
        for param, typ in zip(params, argtypes):
            is_pointer = typ is C.c_void_p or hasattr(typ, "contents")
            assert ("*" in param) == is_pointer, (sym, param, typ)
            if not is_pointer:
                assert SCALARS[param.split()[-2]] is typ, (sym, param, typ)
    # the tuple after TABLES_LATEST in the module's text: the earlier tuples are pinned by their tests
    with open(bindings.__file__) as f:
        text = f.read()
    assert text.index("TABLES_LATEST = ") < text.index("TABLES_GROUP_PAIRS = ")


def test_missing_symbol():
    sym = list(RELATIVE_BATCH)[-1]
    with pytest.raises(RuntimeError, match=re.escape(f"{sym} is missing from the library: rebuild it "
                                                     "(the CPU twin has no relative-pose covariances: engine='python' runs there)")):
        bind(_Stub(lacks=sym), RELATIVE_BATCH)
