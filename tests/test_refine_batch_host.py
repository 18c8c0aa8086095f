"""The lock-step controller of the batched refinement (score_amd/refine_batch.py, engine="python") against
``refine_estimate(engine="python", linear_solver="scipy")`` member by member.  The controller only reorders independent work --
every member sees the operations of the single loop on the same numbers -- so iterations, costs, poses and landmarks are EQUAL,
not close."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from refine_batch_helpers import KEYS_2D, arrays_of, check_fixture, group, member, twin_alone
from score_amd import compat
from score_amd.manhattan import make_manhattan
from score_amd.refine import refine_estimate
from score_amd.refine_batch import _Member, refine_estimate_batch


def _same(fg, got, want):
    for a, b in zip(arrays_of(fg, got), arrays_of(fg, want)):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_fixture_properties():
    print(check_fixture())


def test_python_engine_equals_the_single_loop_member_by_member():
    figures = check_fixture()
    keys = KEYS_2D + ("3D0", "3D1")
    fgs, starts = group(keys)
    out = refine_estimate_batch(fgs, starts, engine="python")
    assert len(out) == len(keys)
    for k, fg, (res, info) in zip(keys, fgs, out):
        want, winfo, solves = twin_alone(k)
        print(k, "iterations", info["iterations"], "solves", info["linear_solves"], "cost", info["cost_final"], "grad", info["grad_inf"])
        assert info["iterations"] == winfo["iterations"] and info["linear_solves"] == solves
        assert info["cost_initial"] == winfo["cost_initial"] and info["cost_final"] == winfo["cost_final"]
        assert info["grad_inf"] == winfo["grad_inf"]
        assert info["engine"] == "python"
        _same(fg, res, want)
    # the 2-D members are one group, the 3-D members another
    assert [info["group"] for _, info in out] == [0] * len(KEYS_2D) + [1, 1]
    assert out[0][1]["rounds"] == max(figures["solves"].values())


def test_grouping_by_dimension_and_max_group_keeps_the_input_order():
    keys = ("3D0", "C", "B", "3D1", "E")
    fgs, starts = group(keys)
    out = refine_estimate_batch(fgs, starts, engine="python", max_group=2)
    assert [info["group"] for _, info in out] == [2, 0, 0, 2, 1]  # 2-D: (C, B), (E); then 3-D: (3D0, 3D1)
    for k, fg, (res, info) in zip(keys, fgs, out):
        want, winfo, _ = twin_alone(k)
        assert info["iterations"] == winfo["iterations"]
        _same(fg, res, want)
        assert list(res.poses.keys()) == [p.name for ch in fg.pose_variables for p in ch]


def test_member_without_unknowns_is_answered_on_the_host():
    lone = compat.FactorGraphData(dimension=2)
    lone.pose_variables = [[compat.PoseVariable2D("A0", (0.5, -0.25), 0.3)]]
    lone.odom_measurements = [[]]
    T = np.eye(3)
    T[:2, 2] = (0.5, -0.25)
    vals = compat.VariableValues(2, compat.ArrayDict(["A0"], T[None]), compat.ArrayDict([], np.zeros((0, 2))), None)
    start = compat.SolverResults(variables=vals, total_time=0.0, solved=True, pose_chain_names=[["A0"]], solver_cost=0.0, info={})
    fg, st = member("C")
    out = refine_estimate_batch([lone, fg, lone], [start, st, start], engine="python")
    want, winfo = refine_estimate(lone, start, engine="python", linear_solver="scipy")
    for i in (0, 2):
        assert out[i][1]["iterations"] == winfo["iterations"] and out[i][1]["cost_final"] == winfo["cost_final"] == 0.0
        assert np.array_equal(np.asarray(out[i][0].poses["A0"]), np.asarray(want.poses["A0"]))
    _same(fg, out[1][0], twin_alone("C")[0])
    # a native call made of such members alone needs no library at all
    out = refine_estimate_batch([lone], [start], engine="native", lib_path="/nonexistent/libscore_hip.so")
    assert out[0][1]["cost_final"] == 0.0


def test_per_member_weights_only_scale_precisions():
    keys = ("B", "E")
    fgs, starts = group(keys)
    rng = np.random.default_rng(3)
    rw = [rng.uniform(0.0, 1.0, size=len(fgs[0].range_measurements)), None]
    lw = [None, np.array([0.0, 0.5])]
    out = refine_estimate_batch(fgs, starts, engine="python", range_weights=rw, loop_closure_weights=lw)
    for i, fg in enumerate(fgs):
        want, winfo = refine_estimate(fg, starts[i], engine="python", linear_solver="scipy", range_weights=rw[i], loop_closure_weights=lw[i])
        assert out[i][1]["iterations"] == winfo["iterations"] and out[i][1]["cost_final"] == winfo["cost_final"]
        _same(fg, out[i][0], want)
    # the weights changed something
    assert out[0][1]["cost_final"] != twin_alone("B")[1]["cost_final"]
    assert out[1][1]["cost_final"] != twin_alone("E")[1]["cost_final"]


def test_argument_errors():
    fgs, starts = group(("B", "C"))
    with pytest.raises(ValueError, match="engine"):
        refine_estimate_batch(fgs, starts, engine="cuda")
    with pytest.raises(ValueError, match="one estimate per graph"):
        refine_estimate_batch(fgs, starts[:1], engine="python")
    with pytest.raises(ValueError, match="max_group"):
        refine_estimate_batch(fgs, starts, engine="python", max_group=0)
    with pytest.raises(ValueError, match="range_weights"):
        refine_estimate_batch(fgs, starts, engine="python", range_weights=[None])
    with pytest.raises(ValueError, match="loop_closure_weights"):
        refine_estimate_batch(fgs, starts, engine="python", loop_closure_weights=[None, None, None])
    with pytest.raises(ValueError, match="weights expected"):
        refine_estimate_batch(fgs, starts, engine="python", range_weights=[np.ones(1), None])
    assert refine_estimate_batch([], [], engine="python") == []


def test_member_transitions_follow_the_single_loop():
    """The state machine on a scripted member: rejected attempts raise lambda tenfold and stop at twelve; an accepted step
    lowers it and opens the next iteration; max_iters closes it."""
    m = _Member(10.0, 50)
    m.after_gradient(1.0, 1e-10, 50)
    assert m.phase == "solve"
    for k in range(11):
        assert not m.after_solve(k % 2 == 0, 3, 11.0, 50)  # failed solves and worse costs alike
        assert m.phase == "solve" and m.lam == pytest.approx(1e-6 * 10.0 ** (k + 1))
    assert not m.after_solve(True, 3, float("nan"), 50)
    assert m.phase == "stopped" and m.iterations == 1 and m.linear_solves == 12 and m.pcg_iters == 36 and m.f == 10.0
    m = _Member(10.0, 2)
    m.after_gradient(1.0, 1e-10, 2)
    assert m.after_solve(True, 0, 9.0, 2) and m.phase == "gradient" and m.it == 2 and m.lam == pytest.approx(1e-7)
    m.after_gradient(0.5, 1e-10, 2)
    assert m.after_solve(True, 0, 8.0, 2) and m.phase == "stopped" and m.iterations == 2 and m.gnorm == 0.5
    m = _Member(10.0, 50)
    m.after_gradient(1e-9, 1e-10, 50)  # |g| <= tol max(1, f)
    assert m.phase == "stopped" and m.iterations == 1
    m = _Member(10.0, 50)
    m.after_gradient(1.0, 1e-10, 50)
    assert m.after_solve(True, 0, 10.0 - 1e-14, 50) and m.phase == "stopped"  # the decrease is below 1e-14 max(1, f)
    assert _Member(10.0, 0).phase == "stopped"


def test_rule_and_drivers_on_scripted_runs_under_sanitizers(tmp_path):
    """tests/tools/refine_rule_check.cpp: the step rule and the GNC-TLS schedule of csrc/score_refine_rule.hpp under their four
    drivers, on scripted backends, against lambdas, mus and final states written by hand there; it exits non-zero unless the
    scripts reach every exit of the rules."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / "refine_rule_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(root, "score_amd", "csrc"), "-o", exe,
                    os.path.join(root, "tests", "tools", "refine_rule_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "every exit reached" in run.stdout


def test_a_members_view_equals_the_view_of_a_handle_on_it_alone_under_sanitizers(tmp_path):
    """tests/tools/refine_view_check.cpp: the group's measurement table advanced to a member (gn_meas_from of csrc/score_gn.hpp,
    what gb_view hands a workgroup) against gn_build of that member alone, every integer and double compared with ==; a 2-D and
    a 3-D group of three: one member with landmarks, ranges and priors, one without landmarks, one with ranges and no priors."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / "refine_view_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(root, "score_amd", "csrc"), "-o", exe,
                    os.path.join(root, "tests", "tools", "refine_view_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "every member's view equals its own" in run.stdout
