"""ctypes bindings of the refinement family's headers (include/score_robust.h, score_refine_robust.h, score_refine_batch.h,
score_refine_robust_batch.h, score_marginals.h, score_spectrum.h, score_samples.h, score_leverage.h, score_curvature.h, the
``*_batch.h`` analyses, score_relative.h, score_relative_batch.h, score_select.h, score_select_batch.h and score_select_poses.h): their records, one ``Table`` per header -- ``{symbol: (argtypes, restype)}``, so the list of a
header's symbols and their argument types are one text -- and the one ``bind`` that applies a table to a library.
include/score_hip.h's own binding is ``solver.load_library``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .native import ScoreGraph
from .solver import InfoRecord, ScoreInfo, ScoreRefineInfo, ScoreSettings, _f64p, _i32p

_u64p = C.POINTER(C.c_uint64)
_handle = C.c_void_p  # score_refine* / score_refine_batch*


# ---------------------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------------------
class ScoreRobustSettings(C.Structure):
    _fields_ = [
        ("inlier_threshold", C.c_double), ("mu_step", C.c_double), ("min_weight", C.c_double),
        ("max_outer", C.c_int32), ("qcqp_directions", C.c_int32),
    ]


class ScoreRobustInfo(C.Structure):
    _fields_ = [
        ("outer_iterations", C.c_int32), ("converged", C.c_int32), ("outliers", C.c_int32), ("rel_outliers", C.c_int32),
        ("mu", C.c_double), ("setup_ms", C.c_double), ("solve_ms", C.c_double), ("total_ms", C.c_double),
    ]


class ScoreRefineRobustSettings(C.Structure):
    _fields_ = [
        ("inlier_threshold", C.c_double), ("rel_threshold", C.c_double), ("mu_step", C.c_double), ("min_weight", C.c_double),
        ("families", C.c_int32), ("max_outer", C.c_int32), ("inner_iters", C.c_int32), ("max_iters", C.c_int32),
        ("tol", C.c_double),
    ]


class ScoreRefineRobustInfo(InfoRecord):
    _fields_ = [
        ("outer_iterations", C.c_int32), ("converged", C.c_int32), ("outliers", C.c_int32), ("rel_outliers", C.c_int32),
        ("mu", C.c_double), ("lm_iterations", C.c_int32), ("linear_solves", C.c_int32), ("pcg_iters", C.c_int32),
        ("cost_initial", C.c_double), ("cost_final", C.c_double), ("grad_inf", C.c_double),
        ("setup_ms", C.c_double), ("solve_ms", C.c_double),
    ]


class ScoreMarginalsInfo(InfoRecord):
    _fields_ = [
        ("columns", C.c_int32), ("batches", C.c_int32), ("pcg_iters", C.c_int32), ("unconverged", C.c_int32),
        ("max_residual", C.c_double), ("setup_ms", C.c_double), ("solve_ms", C.c_double),
    ]


class ScoreMarginalsBatchInfo(InfoRecord):
    _fields_ = [
        ("columns", C.c_int32), ("passes", C.c_int32), ("pcg_iters", C.c_int32), ("unconverged", C.c_int32),
        ("max_residual", C.c_double), ("setup_ms", C.c_double), ("solve_ms", C.c_double),
    ]


class ScoreSpectrumInfo(InfoRecord):
    _fields_ = [
        ("modes", C.c_int32), ("block", C.c_int32), ("iterations", C.c_int32), ("unconverged", C.c_int32),
        ("h_max", C.c_double), ("shift", C.c_double), ("max_residual", C.c_double),
        ("setup_ms", C.c_double), ("solve_ms", C.c_double),
    ]


class ScoreCurvatureInfo(InfoRecord):
    _fields_ = [
        ("modes", C.c_int32), ("block", C.c_int32), ("iterations", C.c_int32), ("unconverged", C.c_int32),
        ("h_max", C.c_double), ("shift", C.c_double), ("c_max", C.c_double), ("max_residual", C.c_double),
        ("setup_ms", C.c_double), ("solve_ms", C.c_double),
    ]


class ScoreSpectrumBatchInfo(InfoRecord):
    _fields_ = [
        ("members", C.c_int32), ("modes", C.c_int32), ("block", C.c_int32), ("rounds", C.c_int32), ("unconverged", C.c_int32),
        ("max_residual", C.c_double), ("setup_ms", C.c_double), ("solve_ms", C.c_double),
    ]


class ScoreCurvatureBatchInfo(InfoRecord):
    _fields_ = [
        ("members", C.c_int32), ("modes", C.c_int32), ("block", C.c_int32), ("rounds", C.c_int32), ("unconverged", C.c_int32),
        ("saddles", C.c_int32),
        ("max_residual", C.c_double), ("setup_ms", C.c_double), ("solve_ms", C.c_double),
    ]


class ScoreSamplesInfo(InfoRecord):
    _fields_ = [
        ("samples", C.c_int32), ("batches", C.c_int32), ("pcg_iters", C.c_int32), ("unconverged", C.c_int32),
        ("max_residual", C.c_double), ("setup_ms", C.c_double), ("rhs_ms", C.c_double), ("solve_ms", C.c_double),
    ]


class ScoreSamplesBatchInfo(InfoRecord):
    _fields_ = [
        ("members", C.c_int32), ("samples", C.c_int32), ("passes", C.c_int32), ("pcg_iters", C.c_int32), ("unconverged", C.c_int32),
        ("singular", C.c_int32),
        ("max_residual", C.c_double), ("setup_ms", C.c_double), ("rhs_ms", C.c_double), ("solve_ms", C.c_double),
    ]


class ScoreSelectInfo(InfoRecord):
    _fields_ = [
        ("solve", ScoreMarginalsInfo),
        ("candidates", C.c_int32), ("picked", C.c_int32), ("excluded", C.c_int32),
        ("total_gain", C.c_double), ("asymmetry", C.c_double), ("cross_ms", C.c_double), ("greedy_ms", C.c_double),
    ]

    def as_dict(self) -> dict:
        out = super().as_dict()
        out["solve"] = self.solve.as_dict()
        return out


class ScoreSelectPosesInfo(InfoRecord):
    _fields_ = [
        ("solve", ScoreMarginalsInfo),
        ("candidates", C.c_int32), ("picked", C.c_int32), ("excluded", C.c_int32),
        ("total_gain", C.c_double), ("asymmetry", C.c_double), ("cross_ms", C.c_double), ("greedy_ms", C.c_double),
    ]

    def as_dict(self) -> dict:
        out = super().as_dict()
        out["solve"] = self.solve.as_dict()
        return out


class ScoreSelectBatchInfo(InfoRecord):
    _fields_ = [
        ("solve", ScoreMarginalsBatchInfo),
        ("members", C.c_int32), ("candidates", C.c_int32), ("picked", C.c_int32), ("excluded", C.c_int32),
        ("total_gain", C.c_double), ("asymmetry", C.c_double), ("cross_ms", C.c_double), ("greedy_ms", C.c_double),
    ]

    def as_dict(self) -> dict:
        out = super().as_dict()
        out["solve"] = self.solve.as_dict()
        return out


# ---------------------------------------------------------------------------------------------------------------------
# one table per header
# ---------------------------------------------------------------------------------------------------------------------
class Table(dict):
    """``{symbol: (argtypes, restype)}`` of the header include/score_<name>.h.  ``missing``: what the error about a symbol
    the library lacks says after "rebuild it" (None: no check of its own, ctypes' AttributeError names the symbol)."""

    def __init__(self, name: str, missing, functions: dict):
        super().__init__(functions)
        self.name, self.missing = name, missing


def bind(lib, table: Table):
    """``lib`` with the argument and result types of ``table``'s symbols set (once per library and table)."""
    flag = f"_score_{table.name}_bound"
    if getattr(lib, flag, False):
        return lib
    if table.missing is not None:
        for sym in table:
            if not hasattr(lib, sym):
                raise RuntimeError(f"{sym} is missing from the library: rebuild it {table.missing}")
    for sym, (argtypes, restype) in table.items():
        fn = getattr(lib, sym)
        fn.argtypes, fn.restype = argtypes, restype
    setattr(lib, flag, True)
    return lib


_NO_ROBUST_LOOP = "(the oracle's CPU twin has no robust loop: engine='python' runs there)"
_NO_ROBUST_REFINEMENT = "(the CPU twin of the tests has no robust refinement: engine='python' runs there)"
_NO_MARGINALS = "(the oracle's CPU twin has no marginals: engine='python' runs there)"
_NO_EIGENSOLVER = "(the oracle's CPU twin has no eigensolver: engine='python' runs there)"
_NO_SAMPLES = "(the CPU twin has no posterior samples: engine='python' runs there)"
_NO_LEVERAGES = "(the CPU twin has no leverages: engine='python' runs there)"

ROBUST = Table("robust", _NO_ROBUST_LOOP, {
    "score_robust_default_settings": ([C.POINTER(ScoreRobustSettings)], None),
    "score_robust_solve": ([C.POINTER(ScoreGraph), C.c_int32, C.POINTER(ScoreSettings), C.POINTER(ScoreRobustSettings),
                            _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, C.POINTER(ScoreInfo), C.POINTER(ScoreRobustInfo)], C.c_int),
    "score_robust_solve_rel": ([C.POINTER(ScoreGraph), C.c_int32, C.POINTER(ScoreSettings), C.POINTER(ScoreRobustSettings),
                                C.c_int32, C.c_double, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p,
                                C.POINTER(ScoreInfo), C.POINTER(ScoreRobustInfo)], C.c_int),
})

REFINE_ROBUST = Table("refine_robust", _NO_ROBUST_REFINEMENT, {
    "score_refine_robust_default_settings": ([C.POINTER(ScoreRefineRobustSettings)], None),
    "score_refine_robust_run": ([_handle, C.POINTER(ScoreRefineRobustSettings)] + [_f64p] * 8 + [C.POINTER(ScoreRefineRobustInfo)],
                                C.c_int),
    "score_refine_residuals": ([_handle, _f64p, _f64p, C.c_double, C.c_double, C.c_double, _f64p, _f64p, _f64p, _f64p], C.c_int),
})

REFINE_BATCH = Table("refine_batch", None, {
    "score_refine_batch_create": ([C.POINTER(ScoreGraph), C.c_int32, C.POINTER(ScoreSettings), C.POINTER(_handle)], C.c_int),
    "score_refine_batch_run": ([_handle, _f64p, _f64p, C.c_int32, C.c_double, _f64p, _f64p, C.POINTER(ScoreRefineInfo)], C.c_int),
    "score_refine_batch_destroy": ([_handle], None),
})

REFINE_ROBUST_BATCH = Table("refine_robust_batch", _NO_ROBUST_REFINEMENT, {
    "score_refine_batch_robust_run": ([_handle, C.POINTER(ScoreRefineRobustSettings), C.c_int32] + [_f64p] * 8
                                      + [C.c_int32, C.POINTER(ScoreRefineRobustInfo)], C.c_int),
    "score_refine_batch_residuals": ([_handle] + [_f64p] * 9, C.c_int),
    "score_refine_batch_restore": ([_handle], C.c_int),
    "score_refine_batch_robust_rounds": ([_handle, _i32p, _i32p], C.c_int),
})

MARGINALS = Table("marginals", _NO_MARGINALS, {
    "score_refine_marginals": ([_handle, _f64p, _f64p, _i32p, C.c_int32, C.c_double, C.c_int32, C.c_int32, _f64p, _f64p, _i32p,
                                C.POINTER(ScoreMarginalsInfo)], C.c_int),
})

MARGINALS_BATCH = Table("marginals_batch", _NO_MARGINALS, {
    "score_refine_batch_marginals": ([_handle, _f64p, _f64p, _i32p, _i32p, C.c_double, C.c_int32, C.c_int32, _f64p, _f64p, _i32p,
                                      C.POINTER(ScoreMarginalsBatchInfo)], C.c_int),
})

SPECTRUM = Table("spectrum", _NO_EIGENSOLVER, {
    "score_refine_spectrum": ([_handle, _f64p, _f64p, C.c_int32, C.c_double, C.c_int32, C.c_double, _f64p, _f64p, _f64p,
                               C.POINTER(ScoreSpectrumInfo)], C.c_int),
})

SPECTRUM_BATCH = Table("spectrum_batch", _NO_EIGENSOLVER, {
    "score_refine_batch_spectrum": ([_handle, _f64p, _f64p, C.c_int32, C.c_double, C.c_int32, C.c_double, _f64p, _f64p, _f64p, _i32p,
                                     _f64p, C.POINTER(ScoreSpectrumBatchInfo)], C.c_int),
    "score_spectrum_ritz": ([C.c_int32, _f64p, _f64p, _f64p, _f64p, _i32p, _i32p], C.c_int),
})

SAMPLES = Table("samples", _NO_SAMPLES, {
    "score_refine_samples": ([_handle, _f64p, _f64p, C.c_uint64, C.c_int64, C.c_int32, _i32p, C.c_int32, C.c_double, C.c_int32,
                              C.c_int32, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, C.POINTER(ScoreSamplesInfo)], C.c_int),
})

SAMPLES_BATCH = Table("samples_batch", _NO_SAMPLES, {
    "score_refine_batch_samples": ([_handle, _f64p, _f64p, _u64p, C.c_int64, _i32p, _i32p, _i32p, C.c_double, C.c_int32, C.c_int32,
                                    _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, _i32p, C.POINTER(ScoreSamplesBatchInfo)],
                                   C.c_int),
})

LEVERAGE = Table("leverage", _NO_LEVERAGES, {
    "score_refine_leverage": ([_handle, _f64p, _f64p, C.c_uint64, C.c_int64, C.c_int32, _i32p, _i32p, C.c_int32, C.c_double,
                               C.c_int32, C.c_int32, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p,
                               C.POINTER(ScoreSamplesInfo)], C.c_int),
    "score_refine_range_variances": ([_handle, _f64p, _f64p, _i32p, _i32p, C.c_int32, C.c_double, C.c_int32, C.c_int32, _f64p, _f64p,
                                      _f64p, _i32p, _f64p, C.POINTER(ScoreMarginalsInfo)], C.c_int),
})

LEVERAGE_BATCH = Table("leverage_batch", _NO_LEVERAGES, {
    "score_refine_batch_leverage": ([_handle, _f64p, _f64p, _u64p, C.c_int64, _i32p, _i32p, _i32p, _i32p, C.c_double, C.c_int32,
                                     C.c_int32, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, _i32p,
                                     C.POINTER(ScoreSamplesBatchInfo)], C.c_int),
    "score_refine_batch_range_variances": ([_handle, _f64p, _f64p, _i32p, _i32p, _i32p, C.c_double, C.c_int32, C.c_int32, _f64p, _f64p,
                                            _f64p, _i32p, C.POINTER(ScoreMarginalsBatchInfo)], C.c_int),
})

TABLES = (ROBUST, REFINE_ROBUST, REFINE_BATCH, REFINE_ROBUST_BATCH, MARGINALS, MARGINALS_BATCH, SPECTRUM, SPECTRUM_BATCH,
          SAMPLES, SAMPLES_BATCH, LEVERAGE)
# the headers that came after those (TABLES itself is pinned by its test)
LATER_TABLES = (LEVERAGE_BATCH,)

CURVATURE = Table("curvature", _NO_EIGENSOLVER, {
    "score_refine_hessian_product": ([_handle, _f64p, _f64p, C.c_int32, _f64p, C.c_int32, _f64p], C.c_int),
    "score_refine_curvature": ([_handle, _f64p, _f64p, C.c_int32, C.c_double, C.c_int32, C.c_double, _f64p, _f64p, _f64p, _f64p,
                                C.POINTER(ScoreCurvatureInfo)], C.c_int),
})
# and those after them (LATER_TABLES is pinned too)
TABLES_SINCE = (CURVATURE,)

CURVATURE_BATCH = Table("curvature_batch", _NO_EIGENSOLVER, {
    "score_refine_batch_hessian_product": ([_handle, _f64p, _f64p, C.c_int32, _f64p, C.c_int32, _f64p], C.c_int),
    "score_refine_batch_curvature": ([_handle, _f64p, _f64p, C.c_int32, C.c_double, C.c_int32, C.c_double, _f64p, _f64p, _f64p, _f64p,
                                      _i32p, _f64p, _f64p, C.POINTER(ScoreCurvatureBatchInfo)], C.c_int),
    "score_curvature_ritz": ([C.c_int32, _f64p, _f64p, _f64p, _f64p, _i32p, _i32p], C.c_int),
})
# and the group forms that followed (TABLES_SINCE is pinned as well)
TABLES_AFTER = (CURVATURE_BATCH,)

RELATIVE = Table("relative", "(the CPU twin has no relative-pose covariances: engine='python' runs there)", {
    "score_refine_relative_covariances": ([_handle, _f64p, _f64p, _i32p, _i32p, C.c_int32, C.c_double, C.c_int32, C.c_int32, _f64p,
                                           _f64p, _f64p, _f64p, _i32p, _f64p, C.POINTER(ScoreMarginalsInfo)], C.c_int),
})
# and the analyses of pairs of poses (TABLES_AFTER is pinned like the others)
TABLES_LATEST = (RELATIVE,)

RELATIVE_BATCH = Table("relative_batch", "(the CPU twin has no relative-pose covariances: engine='python' runs there)", {
    "score_refine_batch_relative_covariances": ([_handle, _f64p, _f64p, _i32p, _i32p, _i32p, C.c_double, C.c_int32, C.c_int32, _f64p,
                                                 _f64p, _f64p, _f64p, _i32p, C.POINTER(ScoreMarginalsBatchInfo)], C.c_int),
})
# and their group form (TABLES_LATEST is pinned in its turn)
TABLES_GROUP_PAIRS = (RELATIVE_BATCH,)

SELECT = Table("select", "(the CPU twin has no selection of ranges: engine='python' runs there)", {
    "score_refine_select_ranges": ([_handle, _f64p, _f64p, _i32p, _i32p, _f64p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                    C.c_int32, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, _f64p,
                                    C.POINTER(ScoreSelectInfo)], C.c_int),
    "score_select_greedy": ([_f64p, _f64p, _i32p, C.c_int32, C.c_int32, C.c_double, _i32p, _f64p, _f64p, _f64p, _i32p, _f64p], C.c_int),
})
# and the analyses of SETS of candidates (TABLES_GROUP_PAIRS is pinned as the others are)
TABLES_SELECTION = (SELECT,)

SELECT_BATCH = Table("select_batch", "(the CPU twin has no selection of ranges: engine='python' runs there)", {
    "score_refine_batch_select_ranges": ([_handle, _f64p, _f64p, _i32p, _i32p, _i32p, _f64p, _i32p, C.c_double, C.c_double, C.c_int32,
                                          C.c_int32, _i32p, _f64p, _f64p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, _f64p,
                                          C.POINTER(ScoreSelectBatchInfo)], C.c_int),
})
# and their group form (TABLES_SELECTION is pinned in its turn)
TABLES_GROUP_SELECTION = (SELECT_BATCH,)

SELECT_POSES = Table("select_poses", "(the CPU twin has no selection of loop closures: engine='python' runs there)", {
    "score_refine_select_relative_poses": ([_handle, _f64p, _f64p, _i32p, _i32p, _f64p, _f64p, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                            C.c_int32, C.c_int32, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, _f64p,
                                            C.POINTER(ScoreSelectPosesInfo)], C.c_int),
    "score_select_block_greedy": ([_f64p, _f64p, _f64p, _i32p, C.c_int32, C.c_int32, C.c_int32, C.c_double, _i32p, _f64p, _f64p, _f64p,
                                   _i32p, _f64p], C.c_int),
})
# and the selection of BLOCK candidates, the relative poses (TABLES_GROUP_SELECTION is pinned like the rest)
TABLES_POSE_SELECTION = (SELECT_POSES,)


# ---------------------------------------------------------------------------------------------------------------------
# three conventions of the calls
# ---------------------------------------------------------------------------------------------------------------------
def ptr(a, kind=_f64p):
    """The array's data as ``kind``; null for None or an empty array."""
    return a.ctypes.data_as(kind) if a is not None and a.size else None


def steps_and_converged(its):
    """(steps, converged) from the ``iters`` a call wrote: a column (a draw, a member) that did not converge reports
    -(steps + 1)."""
    converged = its >= 0
    return np.where(converged, its, -its - 1), converged


class Cutter:
    """The members' consecutive pieces of a group call's flat outputs: ``cut(a, size, shape)`` is a copy of the next ``size``
    entries of ``a`` (None stays None), every array counted for itself.  A member that took no room in ``a`` is not cut."""

    def __init__(self):
        self.at = {}

    def __call__(self, flat, size, shape=None):
        if flat is None:
            return None
        at = self.at.get(id(flat), 0)
        self.at[id(flat)] = at + size
        return flat[at : at + size].reshape((size,) if shape is None else shape).copy()
