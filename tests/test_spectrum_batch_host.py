"""Batched weakest modes (score_amd/spectrum_batch.py): what runs without a GPU -- the dense engine member by member, the
grouping, the argument errors, the binding of include/score_spectrum_batch.h, and the mode rule of
csrc/score_spectrum_batch_rule.hpp as a stand-alone program under the host sanitizers.  The device path is
tests/test_spectrum_batch_gpu.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from refine_batch_helpers import member
from score_amd.spectrum import covariance_bracket, information_spectrum
from score_amd.spectrum_batch import SPECTRUM_BATCH_SYMBOLS, ScoreSpectrumBatchInfo, information_spectrum_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_engine_equals_the_single_call_member_by_member():
    """Mixed dimensions, groups of at most two, weights for one graph: every graph comes back at its own place with exactly
    what information_spectrum(engine="python") gives on it alone."""
    keys = ("B", "3D0", "C", "E", "3D1")
    fgs, starts = [member(k)[0] for k in keys], [member(k)[1] for k in keys]
    w = np.ones(len(fgs[0].range_measurements))
    w[[1, 5, 9]] = 0.0
    weights = [w, None, None, None, None]
    out = information_spectrum_batch(fgs, starts, k=5, range_weights=weights, engine="python", max_group=2)
    assert len(out) == len(keys)
    # 2-D first (B, C | E), then 3-D (3D0, 3D1): the group numbers follow refine_estimate_batch's grouping
    assert [info["group"] for _, info in out] == [0, 2, 0, 1, 2]
    for fg, st, rw, (modes, info) in zip(fgs, starts, weights, out):
        alone, info1 = information_spectrum(fg, st, k=5, range_weights=rw, engine="python")
        for f in ("values", "vectors", "residuals"):
            np.testing.assert_array_equal(getattr(modes, f), getattr(alone, f))
        assert modes.names == alone.names and modes.h_max == alone.h_max and modes.rel_tol == alone.rel_tol
        for nm in alone.names:
            np.testing.assert_array_equal(modes.participation[nm], alone.participation[nm])
        assert {f: info[f] for f in info1} == info1 and info["rounds"] == 0
        assert list(covariance_bracket(modes)) == list(covariance_bracket(alone))
        assert modes.undetermined() == alone.undetermined()
    plain, _ = information_spectrum(fgs[0], starts[0], k=5, engine="python")
    assert np.max(np.abs(plain.values - out[0][0].values)) > 0  # the weights reached graph 0


def test_argument_errors_carry_the_graph_index():
    fgs, starts = [member(k)[0] for k in ("C", "B")], [member(k)[1] for k in ("C", "B")]
    kw = dict(engine="python")
    with pytest.raises(ValueError, match=r"graph 1: .*range_weights"):
        information_spectrum_batch(fgs, starts, range_weights=[None, np.ones(len(fgs[1].range_measurements) + 1)], **kw)
    with pytest.raises(ValueError, match=r"one entry per graph"):
        information_spectrum_batch(fgs, starts, range_weights=[None], **kw)
    with pytest.raises(ValueError, match="one estimate per graph"):
        information_spectrum_batch(fgs, starts[:1], **kw)
    with pytest.raises(ValueError, match="engine"):
        information_spectrum_batch(fgs, starts, engine="host")
    with pytest.raises(ValueError, match="max_group"):
        information_spectrum_batch(fgs, starts, max_group=0, **kw)
    for bad in (dict(k=0), dict(k=17), dict(k=2.5), dict(rel_tol=0.0), dict(rel_tol=-1e-9), dict(max_iters=0), dict(shift=0.0),
                dict(shift=-1e-8)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            information_spectrum_batch(fgs, starts, **{**kw, **bad})


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "score_spectrum_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(score_[a-z_0-9]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert _declared_symbols() == sorted(SPECTRUM_BATCH_SYMBOLS)
    # the info record as the header lays it out: five int32, padding to 8, three doubles
    text = open(os.path.join(ROOT, "include", "score_spectrum_batch.h")).read()
    body = re.search(r"typedef struct score_spectrum_batch_info \{(.*?)\}", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int32_t|double)\s+([a-z_]+)\s*;", body)
    want = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(nm, want[ty]) for ty, nm in fields] == list(ScoreSpectrumBatchInfo._fields_)
    assert ctypes.sizeof(ScoreSpectrumBatchInfo) == 48


def test_mode_rule_on_scripted_runs_under_sanitizers(tmp_path):
    """tests/tools/spectrum_batch_rule_check.cpp: the rule of csrc/score_spectrum_batch_rule.hpp on scripted norm sequences
    against states written by hand there -- done by the recurrence but not by the product, the cap (also reached while
    verifying), breakdown, a member finished while others go on; it exits non-zero unless the scripts reach every exit."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / "spectrum_batch_rule_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "score_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "spectrum_batch_rule_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "every exit reached" in run.stdout
