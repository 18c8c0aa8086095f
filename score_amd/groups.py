"""How the batch front ends hand many graphs to ``score_refine_batch`` handles, stated once.

``refine_estimate_batch``, ``refine_estimate_robust_batch``, ``marginal_covariances_batch``, ``information_spectrum_batch``,
``posterior_samples_batch``, ``range_leverage_batch``, ``predicted_range_variances_batch``, ``predicted_relative_poses_batch`` and
``select_ranges_batch`` all read: check the own arguments,
``grouped`` with a callback that builds what is kept per graph, ``run_chunks`` with a body that answers one chunk.  THE RULE: the
graphs are grouped by dimension, dimensions ascending; every dimension is cut into chunks of at most ``max_group`` graphs in input
order; the chunks are numbered from 0 across the dimensions; a chunk is one group handle, created for it and destroyed after it;
every graph's result goes to its place in the input order.

Nothing here knows the library: the handle class is imported when the first device chunk opens.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Callable, Optional

import numpy as np


def per_graph(value, count: int, what: str, none: bool = True, scalar: bool = False) -> list:
    """``value`` as a list with one entry per graph.  ``none``: None stands for None everywhere; ``scalar``: so does anything
    of no dimension for itself.  (Only an argument that takes both says so in its error.)"""
    if (none and value is None) or (scalar and np.ndim(value) == 0):
        return [value] * count
    value = list(value)
    if len(value) != count:
        entries = "a scalar or one entry" if none and scalar else "one entry"
        raise ValueError(f"{what}: {entries} per graph expected ({count}), got {len(value)}")
    return value


def group_size(max_group) -> int:
    if int(max_group) < 1:
        raise ValueError("max_group must be at least 1")
    return int(max_group)


def paired(datas, results, max_group=None):
    """(graphs, estimates) as lists of one length; ``max_group`` is checked after them when given."""
    datas, results = list(datas), list(results)
    if len(datas) != len(results):
        raise ValueError(f"one estimate per graph expected: {len(datas)} graphs, {len(results)} estimates")
    if max_group is not None:
        group_size(max_group)
    return datas, results


@contextmanager
def naming(i: int, who: Optional[str] = None):
    """A ValueError raised inside gets ``graph i:`` in front (``who``: the single call's name in it, ``marginal_covariances``
    -- whose checks every analysis borrows --, becomes the caller's)."""
    try:
        yield
    except ValueError as e:
        text = str(e).replace("marginal_covariances", who) if who else str(e)
        raise ValueError(f"graph {i}: {text}") from None


def grouped(datas, results, member: Callable, named: bool = True, who: Optional[str] = None) -> dict:
    """{dimension: [(i, problem, point, ...)]} of the graphs in input order.  ``member(i, data, res)`` returns what the front
    end keeps of graph i -- (problem, point) and anything more, a selection or pair ids -- or None for a graph it has answered
    itself: that graph is in no group.  ``named``: the callback's ValueErrors are raised under ``naming(i, who)``."""
    groups: dict = {}
    for i, (data, res) in enumerate(zip(datas, results)):
        if data.dimension not in (2, 3):
            raise ValueError(f"graph {i}: dimension must be 2 or 3")
        if named:
            with naming(i, who):
                kept = member(i, data, res)
        else:
            kept = member(i, data, res)
        if kept is not None:
            groups.setdefault(data.dimension, []).append((i, *kept))
    return groups


def chunks(groups: dict, max_group):
    """(number, chunk) of THE RULE: a chunk is a list of the members ``grouped`` made."""
    number = 0
    for dim in sorted(groups):
        members = groups[dim]
        for c0 in range(0, len(members), int(max_group)):
            yield number, members[c0 : c0 + int(max_group)]
            number += 1


def columns(chunk) -> tuple:
    """(graph numbers, problems, points, [whatever else the members keep, a list each]) of a chunk."""
    idx, probs, points, *extras = (list(col) for col in zip(*chunk))
    return idx, probs, points, extras


def run_chunks(groups: dict, max_group, out: list, body: Callable, device: bool, lib_path: Optional[str] = None,
               solver_settings: Optional[dict] = None, handle=None) -> list:
    """Every chunk's ``body(handle, number, idx, probs, points, extras)`` -- one result per member, in the chunk's order --
    into ``out`` at the members' places.  ``device``: the body runs inside ``with RefineBatchHandle(probs, lib_path,
    solver_settings)`` (one create and one destroy per chunk); else its handle is None."""
    for number, chunk in chunks(groups, max_group):
        idx, probs, points, extras = columns(chunk)
        if device:
            if handle is None:
                from .refine_batch import RefineBatchHandle as handle
            with handle(probs, lib_path, solver_settings) as h:
                got = body(h, number, idx, probs, points, extras)
        else:
            got = body(None, number, idx, probs, points, extras)
        for i, g in zip(idx, got):
            out[i] = g
    return out


class FollowUp:
    """An analysis a refine front end runs on a group's handle at the refined points before the handle is closed:
    ``info[key]`` of every graph.  ``prepare(i, problem)``: what is kept of graph i before any work (its errors come before
    any handle); ``run(handle, number, idx, probs, points, costs, kept)``: one entry per member, ``handle`` None on the python
    engine.  A graph without unknowns gets None."""

    def __init__(self, key: str, run: Callable, prepare: Optional[Callable] = None):
        self.key, self.run, self.prepare, self.kept = key, run, prepare, {}

    def keep(self, i: int, prob) -> None:
        if self.prepare is not None:
            self.kept[i] = self.prepare(i, prob)

    def __call__(self, handle, number, idx, probs, points, costs) -> list:
        return self.run(handle, number, idx, probs, points, costs, [self.kept.get(i) for i in idx])


def follow(follow_ups, handle, number, idx, probs, points, costs) -> list:
    """Per member {key: entry} of every follow-up, run in the order of the list."""
    extra = [{} for _ in idx]
    for f in follow_ups:
        for mine, got in zip(extra, f(handle, number, idx, probs, points, costs)):
            mine[f.key] = got
    return extra


__all__ = ["per_graph", "group_size", "paired", "naming", "grouped", "chunks", "columns", "run_chunks", "FollowUp", "follow"]
