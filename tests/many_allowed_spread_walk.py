"""The untried children of a stopped allowed walk, on the host (a helper module of the solve_many_allowed resume and spread
tests, no test itself).  many_walk_allowed and the oracle are its only sources.

A stopped many_walk_allowed.Walk is a list of frames (node, variable, next value).  Its untried children in WALK ORDER are
the ALLOWED values >= next of the current node's variable, ascending, then those of the frame below it, down to the oldest
frame; child (frame, value) as a root row is the frame's node with the variable set to the value.  A forbidden value is no
child: the walk neither tries nor counts it.  The contribution of a child walked as a root row of its own is
many_spread_walk.contribution(), the same formula as on the width walk."""
import numpy as np

import many_spread_walk
import many_walk_allowed
from many_spread_walk import COUNTERS, contribution, fold  # noqa: F401


def untried(walk):
    """[(node, variable, [allowed values >= next, ascending])], the current node first, the oldest frame last"""
    return [(node, v, [c for c in many_walk_allowed.allowed(walk.rel, node, v) if c >= nv])
            for node, v, nv in reversed(walk.frames())]


def count_children(walk):
    return sum(len(values) for _, _, values in untried(walk))


def width_count(walk):
    """what the width walk's formula counts on the same frames: every value of [next, hi]"""
    return many_spread_walk.count_children(walk)


def children_of(walk):
    """-> int32 [children, n, 2]: the root rows of the untried children of a stopped allowed walk, in walk order"""
    rows = []
    for node, v, values in untried(walk):
        for value in values:
            row = node.copy()
            row[v] = (value, value)
            rows.append(row)
    return np.stack(rows).astype(np.int32)


def folded(text, walk, part):
    """the record of a stopped walk (`part`) plus the fold of every child walked to its end as a root row of its own ->
    dict of COUNTERS"""
    subs = [many_walk_allowed.Walk(text, row).run(1 << 62) for row in children_of(walk)]
    return fold(subs, [0] * len(subs), [{f: part[f] for f in COUNTERS}])[0]
