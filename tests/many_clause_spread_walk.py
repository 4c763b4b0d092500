"""What Model.solve_many_clauses_spread and the kernels under it are specified to compute, on the host (a helper module of
test_solve_many_clauses_spread_host.py and test_gpu_solve_many_clauses_spread.py, no test itself): the driver of
many_spread_walk.spread_many over many_walk_objective.Walk(text, row, "ALL") in place of many_walk.Walk.

The frames of a stopped clause walk, their children in walk order, a child's contribution to its owner and the fold are
many_spread_walk's (count_children, children_of, contribution, fold): a clause walk stops as "try value nv of variable v on
the node cur" over a stack of (node, variable, next value) frames like any other.  Under ALL there is no incumbent and
"<obj>", if the model has one, is an ordinary variable, so a child walked as a root row of its own is the subtree the one
walk would have walked.

props are the oracle's, which treats a child as an event-driven node and a root row as a full pass: they need not follow
the identity and are compared on no set (many_walk_objective.FIELDS has no props).  On the device the identity holds for
props as well, and the GPU tests compare them with the one call of the kernel itself."""
import bisect

import numpy as np

import many_walk_objective as W
from many_spread_walk import BIG, COUNTERS, children_of, contribution, count_children, fold  # noqa: F401
from many_walk_objective import DONE, LIMIT

FIELDS = W.FIELDS  # status, nodes, cuts, solutions


def stopped_walk(text, row, budget):
    """-> (the ALL walk of `row` after `budget` nodes, its record)"""
    walk = W.Walk(text, row, "ALL")
    return walk, walk.run(budget)


def spread_many(text, roots, budgets, max_rounds=1 << 30):
    """-> (per-owner dicts: FIELDS, root_props, props and first, info).  info = dict(rounds, sub_instances, per_round,
    replaced_later: owners whose `first` candidate was replaced by a solution of a later round, one_child_frames: walks
    fanned out with a frame before its variable's last value, depth0: checkpoints fanned out that held the current node
    only, dead_rows: sub-rows inconsistent as roots (the +1 cut), solution_rows: sub-rows that are themselves the one
    solution (0 nodes, 1 solution))"""
    def budget(rnd):
        return budgets[min(rnd, len(budgets) - 1)]

    K = len(roots)
    batch, records = map(list, zip(*(stopped_walk(text, row, budget(0)) for row in roots)))
    owners = [{f: r[f] for f in FIELDS + ("root_props", "props")} for r in records]
    first = [r["first"] for r in records]
    pos = [0 if r["solutions"] > 0 else BIG for r in records]
    owner = list(range(K))
    info = dict(rounds=1, sub_instances=0, per_round=[], replaced_later=0, one_child_frames=0, depth0=0, dead_rows=0,
                solution_rows=0)
    level = 0

    def leave():
        for t, r in enumerate(records):
            if r["status"] == LIMIT:
                owners[owner[t]]["status"] = LIMIT
        if level == 0:
            return
        fold(records, owner, owners)
        for t, r in enumerate(records):  # ascending: the lowest row of an owner comes first
            info["dead_rows"] += r["status"] == DONE and r["nodes"] == 0 and r["solutions"] == 0
            info["solution_rows"] += r["status"] == DONE and r["nodes"] == 0 and r["solutions"] == 1
            if r["solutions"] > 0 and t < pos[owner[t]]:
                info["replaced_later"] += first[owner[t]] is not None
                first[owner[t]] = r["first"]
                pos[owner[t]] = t

    while info["rounds"] < max_rounds:
        index = [t for t, r in enumerate(records) if r["status"] == LIMIT]
        if not index:
            break
        counts = [count_children(batch[t]) for t in index]
        rows = np.concatenate([children_of(batch[t]) for t in index])
        came_from = np.repeat(np.arange(len(index)), counts)
        for t in index:
            info["one_child_frames"] += int(batch[t].has_last_value_frame())
            info["depth0"] += len(batch[t].frames()) == 1
            owners[owner[t]]["status"] = DONE  # it goes on in its children
        offsets = np.concatenate([[0], np.cumsum(counts)])
        for r in records:  # the stopped rows are left for their children
            if r["status"] == LIMIT:
                r["status"] = -1
        leave()
        pos = [int(offsets[bisect.bisect_left(index, p)]) for p in pos]
        owner = [owner[index[c]] for c in came_from]
        batch, records = map(list, zip(*(stopped_walk(text, row, budget(info["rounds"])) for row in rows)))
        level += 1
        info["rounds"] += 1
        info["sub_instances"] += len(batch)
        info["per_round"].append(len(batch))
    leave()
    out = []
    for o, f in zip(owners, first):
        o = dict(o)
        o["first"] = f
        out.append(o)
    return out, info
