"""What Model.solve_many_spread and the kernels under it are specified to compute, on the host (a helper module of
test_solve_many_spread_host.py and test_gpu_solve_many_spread.py, no test itself).  many_walk and the oracle are its only
sources.

A stopped many_walk.Walk is a list of frames (node, variable, next value).  Its untried children in WALK ORDER are the
values next .. hi of the current node, ascending, then those of the frame below it, down to the oldest frame; child (frame,
value) as a root row is the frame's node with the variable set to the value.  children_of() lists those rows.

A child walked as a root row of its own gives its owner (contribution()):
    nodes 1 + sub.nodes; cuts sub.cuts, plus 1 if the row was inconsistent as a root (DONE, no node, no solution);
    props sub.root_props + sub.props; solutions sub.solutions

spread_many() is the driver in these terms: round 0 walks every root row with budgets[0]; every later round lists the
children of all stopped walks of the batch, one after the other in the order of the batch, and walks them as a fresh batch
with that round's budget (the last budget repeats).  A batch is folded once, when it is left.  `first`: an owner that had a
solution when round 0 stopped keeps it; otherwise the lowest row of a batch with a solution holds it, and a solution of a
later batch comes before that candidate exactly when its row lies below the start of the children of the first stopped
row at or after the candidate's -- one bisection per round (`pos`)."""
import bisect

import numpy as np

import many_walk
from many_walk import DONE, LIMIT

BIG = 1 << 62
COUNTERS = ("nodes", "cuts", "props", "solutions")


def count_children(walk):
    """untried children of a stopped walk"""
    return sum(int(node[v, 1]) - nv + 1 for node, v, nv in walk.frames())


def children_of(walk):
    """-> int32 [children, n, 2]: the root rows of the untried children of a stopped walk, in walk order"""
    rows = []
    for node, v, nv in reversed(walk.frames()):
        for value in range(nv, int(node[v, 1]) + 1):
            row = node.copy()
            row[v] = (value, value)
            rows.append(row)
    return np.stack(rows).astype(np.int32)


def contribution(sub):
    """what the record of a child walked as a root row adds to its owner"""
    dead = sub["status"] == DONE and sub["nodes"] == 0 and sub["solutions"] == 0
    return dict(nodes=1 + sub["nodes"], cuts=sub["cuts"] + int(dead), props=sub["root_props"] + sub["props"],
                solutions=sub["solutions"])


def fold(records, owner, results):
    """add every record's contribution to results[owner[t]] (dicts with COUNTERS), in place"""
    for sub, o in zip(records, owner):
        for f, x in contribution(sub).items():
            results[o][f] += x
    return results


def fan_out(walks, results):
    """the stopped walks of a batch, fanned out -> (index of the stopped ones, their child counts, rows [total, n, 2],
    came_from [total]: the position in `index` a row came from)"""
    index = [t for t, r in enumerate(results) if r["status"] == LIMIT]
    counts = [count_children(walks[t]) for t in index]
    rows = np.concatenate([children_of(walks[t]) for t in index]) if index else None
    came_from = np.repeat(np.arange(len(index)), counts)
    return index, counts, rows, came_from


def spread_many(text, roots, budgets, max_rounds=1 << 30):
    """-> (per-owner dicts in many_walk.dive()'s form, info): info = dict(rounds, sub_instances, per_round: sub-instances of
    every round after round 0, replaced_later: owners whose `first` candidate was replaced by a solution of a later round,
    one_child_frames: walks fanned out with a frame before its variable's last value (one child), depth0: checkpoints fanned out that held the
    current node only)"""
    def budget(rnd):
        return budgets[min(rnd, len(budgets) - 1)]

    K = len(roots)
    batch = [many_walk.Walk(text, row) for row in roots]
    records = [w.run(budget(0)) for w in batch]
    owners = [{f: r[f] for f in many_walk.FIELDS} for r in records]
    first = [r["rows"][0] if r["rows"] else None for r in records]
    pos = [0 if r["solutions"] > 0 else BIG for r in records]
    owner = list(range(K))
    info = dict(rounds=1, sub_instances=0, per_round=[], replaced_later=0, one_child_frames=0, depth0=0)
    level = 0

    def leave():
        for t, r in enumerate(records):
            if r["status"] == LIMIT:
                owners[owner[t]]["status"] = LIMIT
        if level == 0:
            return
        fold(records, owner, owners)
        for t, r in enumerate(records):  # ascending: the lowest row of an owner comes first
            if r["solutions"] > 0 and t < pos[owner[t]]:
                info["replaced_later"] += first[owner[t]] is not None
                first[owner[t]] = r["rows"][0]
                pos[owner[t]] = t

    while info["rounds"] < max_rounds:
        index, counts, rows, came_from = fan_out(batch, records)
        if not index:
            break
        for t in index:
            frames = batch[t].frames()
            info["one_child_frames"] += int(batch[t].has_last_value_frame())
            info["depth0"] += len(frames) == 1
            owners[owner[t]]["status"] = DONE  # it goes on in its children
        offsets = np.concatenate([[0], np.cumsum(counts)])
        for r in records:  # the stopped rows are left for their children
            if r["status"] == LIMIT:
                r["status"] = -1
        leave()
        pos = [int(offsets[bisect.bisect_left(index, p)]) for p in pos]
        owner = [owner[index[c]] for c in came_from]
        batch = [many_walk.Walk(text, row) for row in rows]
        records = [w.run(budget(info["rounds"])) for w in batch]
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
