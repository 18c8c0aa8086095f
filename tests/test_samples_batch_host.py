"""Batched posterior samples (score_amd/samples_batch.py): what runs without a GPU -- the binding of
include/score_samples_batch.h, the dense engine graph by graph, the grouping, the argument errors, and the plan of
csrc/score_samples_batch_plan.hpp as a stand-alone program under the host sanitizers.  The device path is
tests/test_samples_batch_gpu.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from refine_batch_helpers import member
from samples_batch_helpers import DISTRIBUTION_SEED, member_twin
from samples_helpers import check_distribution
from score_amd.samples import posterior_samples
from score_amd.samples_batch import SAMPLES_BATCH_SYMBOLS, ScoreSamplesBatchInfo, posterior_samples_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "score_samples_batch.h")


def test_header_and_binding_agree():
    text = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(score_[a-z_0-9]+)\s*\(", plain))) == sorted(SAMPLES_BATCH_SYMBOLS)
    # the info record as the header lays it out: six int32, four doubles
    body = re.search(r"typedef struct score_samples_batch_info \{(.*?)\}", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int32_t|double)\s+([a-z_]+)\s*;", body)
    want = {"int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(nm, want[ty]) for ty, nm in fields] == list(ScoreSamplesBatchInfo._fields_)
    assert [nm for _, nm in fields] == ["members", "samples", "passes", "pcg_iters", "unconverged", "singular", "max_residual",
                                        "setup_ms", "rhs_ms", "solve_ms"]
    assert ctypes.sizeof(ScoreSamplesBatchInfo) == 56
    # score_samples.h stays as it is beside the new header
    single = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "score_samples.h")).read(), flags=re.S)
    assert "score_refine_batch_samples" not in single


def test_python_engine_equals_the_single_call_graph_by_graph():
    """Mixed dimensions, groups of at most two, weights for one graph, a count per graph: every graph comes back at its own
    place with exactly what posterior_samples(engine="python", seed=seed + i) gives on it alone."""
    keys = ("B", "3D0", "C", "E", "3D1")
    fgs, starts = [member(k)[0] for k in keys], [member(k)[1] for k in keys]
    w = np.ones(len(fgs[0].range_measurements))
    w[[1, 5, 9]] = 0.0
    weights = [w, None, None, None, None]
    counts = [5, 3, 4, 6, 2]
    out = posterior_samples_batch(fgs, starts, n_samples=counts, seed=40, first_sample=2, range_weights=weights, engine="python",
                                  max_group=2)
    assert len(out) == len(keys)
    # 2-D first (B, C | E), then 3-D (3D0, 3D1): the group numbers follow refine_estimate_batch's grouping
    assert [info["group"] for _, info in out] == [0, 2, 0, 1, 2]
    for i, (fg, st, rw, S, (smp, info)) in enumerate(zip(fgs, starts, weights, counts, out)):
        alone, info1 = posterior_samples(fg, st, n_samples=S, seed=40 + i, first_sample=2, range_weights=rw, engine="python")
        assert smp.order == alone.order and smp.names == alone.names and smp.count == alone.count == S
        assert smp.first_sample == alone.first_sample == 2
        for nm in alone.order:
            np.testing.assert_array_equal(smp.steps[nm], alone.steps[nm])
        for nm in alone.names:
            np.testing.assert_array_equal(smp.covariance(nm), alone.covariance(nm))
            np.testing.assert_array_equal(smp.mean(nm), alone.mean(nm))
        for f in info1:
            np.testing.assert_array_equal(info[f], info1[f], err_msg=f)
        assert info["passes"] == 0 and info["determined"] == 1 and info["engine"] == "python"
        for s in range(S):
            got, want = smp.results(s), alone.results(s)
            for nm in alone.order:
                np.testing.assert_array_equal(got[nm], want[nm])
    # a list of seeds, an integer count: the same draws
    again = posterior_samples_batch(fgs[:2], starts[:2], n_samples=3, seed=[40, 41], first_sample=2, range_weights=weights[:2], engine="python")
    for (a, _), (b, _) in zip(again, out[:2]):
        for nm in a.order:
            np.testing.assert_array_equal(a.steps[nm], b.steps[nm][:3])
    plain, _ = posterior_samples(fgs[0], starts[0], n_samples=5, seed=40, first_sample=2, engine="python")
    assert not np.array_equal(plain.steps[plain.order[0]], out[0][0].steps[plain.order[0]])  # the weights reached graph 0


@pytest.mark.parametrize("keys", [("B", "E"), ("3D0",)])
def test_distribution_of_the_python_engine_at_the_gpu_tests_seeds(keys):
    tws = [member_twin(k) for k in keys]
    out = posterior_samples_batch([t.fg for t in tws], [t.results for t in tws], n_samples=64, seed=DISTRIBUTION_SEED,
                                  variables=[t.names for t in tws], engine="python")
    for k, tw, (smp, info) in zip(keys, tws, out):
        delta = np.concatenate([smp.steps[nm] for nm in tw.names], axis=1)
        assert delta.shape == (64, tw.ref.n)
        check_distribution(tw, delta, smp.covariance, f"{k}, python engine")


def test_argument_errors_carry_the_graph_index():
    fgs, starts = [member(k)[0] for k in ("C", "B")], [member(k)[1] for k in ("C", "B")]
    kw = dict(engine="python", n_samples=2)
    first = fgs[1].pose_variables[0][0].name
    some = fgs[1].pose_variables[0][3].name
    with pytest.raises(ValueError, match=r"graph 1: .*range_weights"):
        posterior_samples_batch(fgs, starts, range_weights=[None, np.ones(len(fgs[1].range_measurements) + 1)], **kw)
    with pytest.raises(ValueError, match=r"graph 1: .*fixed first pose"):
        posterior_samples_batch(fgs, starts, variables=[None, [first]], **kw)
    with pytest.raises(ValueError, match=r"graph 1: .*twice"):
        posterior_samples_batch(fgs, starts, variables=[None, [some, some]], **kw)
    with pytest.raises(ValueError, match=r"graph 0: .*unknown variable"):
        posterior_samples_batch(fgs, starts, variables=[["nobody"], None], **kw)
    for what in ("range_weights", "loop_closure_weights", "variables"):
        with pytest.raises(ValueError, match=rf"{what}: one entry per graph"):
            posterior_samples_batch(fgs, starts, **{**kw, what: [None]})
    with pytest.raises(ValueError, match="n_samples: one entry per graph"):
        posterior_samples_batch(fgs, starts, engine="python", n_samples=[2, 2, 2])
    with pytest.raises(ValueError, match="seed: one entry per graph"):
        posterior_samples_batch(fgs, starts, seed=[1], **kw)
    with pytest.raises(ValueError, match="one estimate per graph"):
        posterior_samples_batch(fgs, starts[:1], **kw)
    with pytest.raises(ValueError, match="engine"):
        posterior_samples_batch(fgs, starts, engine="host")
    with pytest.raises(ValueError, match="max_group"):
        posterior_samples_batch(fgs, starts, max_group=0, **kw)
    for bad, words in ((dict(n_samples=0), "n_samples"), (dict(n_samples=2.5), "n_samples"), (dict(n_samples=[2, 0]), "n_samples"),
                       (dict(block_width=0), "block_width"), (dict(block_width=17), "block_width"), (dict(block_width=2.5), "block_width"),
                       (dict(first_sample=-1), "first_sample"), (dict(first_sample=2 ** 32 - 1), "first_sample"),
                       (dict(first_sample=0.5), "first_sample"), (dict(rel_tol=0.0), "rel_tol"), (dict(max_iters=0), "max_iters")):
        with pytest.raises(ValueError, match=words):
            posterior_samples_batch(fgs, starts, **{**kw, **bad})


def test_refine_estimate_batch_draws_at_the_refined_points():
    """refine_estimate_batch(samples=S) on the python engine: the refinement is what it is without the keyword, and graph i's
    draws are those of the stream samples_seed + i at the refined point (from the point itself: no trip through matrices)."""
    from score_amd.refine_batch import _problem_of, _python_lock_step, refine_estimate_batch
    from score_amd.samples import _python_draws

    keys = ("C", "B")
    fgs, starts = [member(k)[0] for k in keys], [member(k)[1] for k in keys]
    out = refine_estimate_batch(fgs, starts, engine="python", samples=4, samples_seed=9)
    plain = refine_estimate_batch(fgs, starts, engine="python")
    probs, first = zip(*[_problem_of(fg, st, None, None) for fg, st in zip(fgs, starts)])
    pts, _, _ = _python_lock_step(list(probs), list(first), 50, 1e-10)
    for i, ((res, info), (res_p, info_p)) in enumerate(zip(out, plain)):
        smp, si = info["samples"]
        assert "samples" not in info_p and info["cost_final"] == info_p["cost_final"] and info["iterations"] == info_p["iterations"]
        for nm in res_p.poses:
            np.testing.assert_array_equal(res.poses[nm], res_p.poses[nm])
        delta, _, _, _ = _python_draws(probs[i], pts[i], 9 + i, 0, 4)
        assert smp.count == 4 and si["engine"] == "python" and si["group"] == 0
        np.testing.assert_array_equal(np.concatenate([smp.steps[nm] for nm in smp.order], axis=1),
                                      delta[:, _select_cols(probs[i])])
    with pytest.raises(ValueError, match="n_samples"):
        refine_estimate_batch(fgs, starts, engine="python", samples=0)


def _select_cols(prob):
    from score_amd.marginals import _select

    return _select(prob, None)[3]


def test_plan_on_hand_written_cases_under_sanitizers(tmp_path):
    """tests/tools/samples_batch_plan_check.cpp: the plan of csrc/score_samples_batch_plan.hpp -- output offsets, passes, NV
    per pass, the draw of every (member, slot, pass) -- against tables written by hand there, for the counts [17, 5, 0, 16, 1]
    at widths 1, 4 and 16, single members and every argument error; it exits non-zero unless every branch is reached."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path / "samples_batch_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "score_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "tools", "samples_batch_plan_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    assert "every branch reached" in run.stdout
