"""The second-order check on the host: ``dense_hessian`` against an independent torch reference, the block functions of
csrc/score_gn.hpp against differences of the existing gradient, ``Curvature`` / ``escape`` on a true saddle, and the binding
table.  No GPU."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import curvature_helpers as ch
from score_amd.bindings import CURVATURE, LATER_TABLES, TABLES, TABLES_SINCE, bind
from score_amd.curvature import CURVATURE_SYMBOLS, CurvatureHandle, dense_hessian, escape, hessian_spectrum
from score_amd.marginals import _problem_and_point, dense_information
from score_amd.refine import refine_estimate
from test_binding_tables_host import SCALARS, _declarations, _Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = ch.EPS


def _entrywise(label, got, want, B, c):
    """|got - want| <= c eps B entry by entry; an entry without contributions is zero in both."""
    err = np.abs(got - want)
    bound = c * EPS * B
    ratio = float(np.max(err[B > 0] / bound[B > 0]))
    print(f"{label}: n = {got.shape[0]}, c = {c}, worst |difference| / (c eps B) = {ratio:.3e}")
    assert np.all(err <= bound), f"{label}: worst entry at {ratio:.3e} of its bound"
    return ratio


@pytest.mark.parametrize("key", ch.DENSE_CASES)
def test_dense_hessian_against_autograd(key):
    fg, results, ref = ch.reference(key)
    ch.check_input_conditions(key, ref)
    E = dense_hessian(ref.prob, ref.point)
    _entrywise(key, E, ref.E, ref.B, ref.c)
    _entrywise(key + " (J'J)", dense_information(ref.prob, ref.point), ref.JtJ, ref.B, ref.c)


@pytest.mark.parametrize("key", ["a", "d"])
def test_curvature_term_vanishes_without_noise(key):
    fg, results = ch.noise_free(ch.SPECTRUM_GRAPHS[key]())
    prob, point = _problem_and_point(fg, results, None, None)
    tc = ch.TorchCost(fg, results)
    _, B, count = tc.parts()
    E, H = dense_hessian(prob, point), dense_information(prob, point)
    assert np.max(np.abs(H)) > 1.0
    c = int(count.max()) + 128
    _entrywise(key + " noise-free", E, H, B, c)
    assert np.all(np.abs((E - H) - (E - H).T) <= c * EPS * B)
    # and at a noisy point the term is symmetric to the rounding of its own sums
    fg2, results2, ref = ch.reference(key)
    T = dense_hessian(ref.prob, ref.point) - dense_information(ref.prob, ref.point)
    assert np.all(np.abs(T - T.T) <= ref.c * EPS * ref.B)
    assert np.max(np.abs(T)) >= 1e-3 * np.max(np.abs(ref.JtJ))


def _blocks_program(tmp_path, name, flags):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / name)
    subprocess.run([gxx, "-std=c++17", *flags, "-I", os.path.join(ROOT, "score_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "curvature_blocks_check.cpp")], check=True)
    return exe


def _blocks_figures(out):
    rows = [ln.split() for ln in out.strip().splitlines()]
    assert [r[0] for r in rows] == ["rel2", "range2", "rel3", "range3"]
    return {r[0]: (float(r[1]), float(r[2])) for r in rows}


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitizers"])
def test_exact_blocks_against_differences_of_the_gradient(tmp_path, flags):
    """tests/tools/curvature_blocks_check.cpp: the four block kinds at 64 points each.  The bound is 100 x the largest relative
    discrepancy measured when the feature was written (profiles/curvature.json), and may not exceed 1e-6 of the block's
    largest entry; a formula error is of order 1e-2 or more (the program checks the curvature part's share first)."""
    with open(os.path.join(ROOT, "profiles", "curvature.json")) as f:
        rec = json.load(f)["blocks_check"]
    bound = rec["bound"]
    assert abs(bound - 100.0 * rec["largest_relative_discrepancy"]) <= 4 * EPS * bound and 0.0 < bound <= 1e-6
    assert rec["largest_relative_discrepancy"] == max(k["largest_relative_discrepancy"] for k in rec["per_kind"].values())
    exe = _blocks_program(tmp_path, "curvature_blocks_check", flags)
    run = subprocess.run([exe, repr(bound)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    figures = _blocks_figures(run.stdout)
    assert all(d <= bound and share >= 1e-2 for d, share in figures.values())


def test_saddle_kind_negative_escape():
    fg, results, ref = ch.reference("line")
    ch.check_input_conditions("line", ref)
    cur, info = hessian_spectrum(fg, results, k=3, engine="python")
    assert info["engine"] == "python" and info["c_max"] > 1.0
    print("line:", cur.values, cur.gauss_newton, info)
    assert cur.kind == "saddle"
    assert abs(cur.values[0] - (-16.43)) < 0.005 and abs(cur.values[1] - 19.65) < 0.005
    neg = cur.negative()
    assert len(neg) == 1 and neg[0][0] == 0 and neg[0][1] == cur.values[0]
    assert neg[0][2][0][0] == "L0" and neg[0][2][0][1] > 0.99
    assert cur.gauss_newton[0] >= 0.0 and cur.gauss_newton[0] - cur.values[0] > 16.0  # J'J sees nothing wrong along v_0
    # the Gauss-Newton matrix calls the same direction undetermined
    assert np.linalg.eigvalsh(ref.JtJ)[0] <= 1e-9 * ref.h_max
    moved = escape(fg, results, cur)
    assert moved.solver_cost < 31.3077 - 1.0
    refined, rinfo = refine_estimate(fg, moved, engine="python", linear_solver="scipy")
    assert rinfo["cost_final"] < 2.0, rinfo
    cur2, _ = hessian_spectrum(fg, refined, k=3, engine="python")
    print("line, escaped and refined:", cur2.values, rinfo["cost_final"])
    assert cur2.kind == "minimum" and cur2.negative() == []
    with pytest.raises(ValueError, match="no negative mode"):
        escape(fg, refined, cur2)


def test_kind_flat_and_escape_without_descent():
    fg, results, ref = ch.reference("line")
    cur, _ = hessian_spectrum(fg, results, k=2, engine="python")
    first, size = [f for f, _ in cur._rows.values()], [s for _, s in cur._rows.values()]
    flat = type(cur)(np.array([0.0, 1.0]), cur.vectors, cur.residuals, cur.gauss_newton, cur.names, first, size, cur.h_max, cur.rel_tol, [])
    assert flat.kind == "flat" and flat.negative() == []
    with pytest.raises(RuntimeError, match="lowers the cost"):
        escape(fg, results, cur, steps=(1e3,))  # (a kilometre along v_0: every range residual grows)
    with pytest.raises(ValueError, match="engine"):
        hessian_spectrum(fg, results, engine="numpy")
    with pytest.raises(ValueError, match="k must be"):
        hessian_spectrum(fg, results, k=17, engine="python")
    with pytest.raises(ValueError, match="rel_tol"):
        hessian_spectrum(fg, results, rel_tol=0.0, engine="python")
    with pytest.raises(ValueError, match="shift"):
        hessian_spectrum(fg, results, shift=-1.0, engine="python")


def test_table_matches_header():
    table = CURVATURE
    assert TABLES_SINCE == (CURVATURE,) and table not in TABLES and table not in LATER_TABLES and table.name == "curvature"
    assert CURVATURE in CurvatureHandle.headers
    declared = _declarations(table.name)
    assert sorted(declared) == sorted(table) == sorted(CURVATURE_SYMBOLS)
    assert sorted(declared) == ["score_refine_curvature", "score_refine_hessian_product"]
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
    # the info record is the header's, field by field
    with open(os.path.join(ROOT, "include", "score_curvature.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    body = re.search(r"typedef struct score_curvature_info \{(.*?)\}", text, flags=re.S).group(1)
    fields = [(nm.strip(), SCALARS[typ]) for typ, names in re.findall(r"(int32_t|double)\s+([^;]+);", body) for nm in names.split(",")]
    from score_amd.bindings import ScoreCurvatureInfo
    assert [(nm, typ) for nm, typ in ScoreCurvatureInfo._fields_] == fields


def test_missing_symbol():
    sym = list(CURVATURE)[-1]
    with pytest.raises(RuntimeError, match=re.escape(f"{sym} is missing from the library: rebuild it "
                                                     "(the oracle's CPU twin has no eigensolver: engine='python' runs there)")):
        bind(_Stub(lacks=sym), CURVATURE)
