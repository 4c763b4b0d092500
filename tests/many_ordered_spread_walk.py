"""What the spread of Model.solve_many_clauses_ordered and the kernels under it are specified to compute
(include/csolve_gpu.h), on the host (a helper module of test_solve_many_clauses_ordered_spread_host.py and the two GPU
test files of the ordered spread, no test itself).  many_walk_ordered.Walk, many_clause_from_walk and many_spread_walk are
its only sources.

A stopped many_walk_ordered.Walk is a list of frames (node, variable, next): its `stack`, then the current node (`cur`,
`v`, `nv`).  With lo, hi = node[variable] and mid = (lo + hi) >> 1, the children of a frame are the walk's own:

  enumerating (hi - lo + 1 <= split_width)   the rows variable = [x, x] for x = next .. hi
  halving, next == mid + 1                   one child, variable = [mid + 1, hi]
  halving, next == lo (current node only)    two children, [lo, mid] then [mid + 1, hi]

In the third case the walk has not yet counted the parent in `halvings` (it does when the first half is tried): the
instance owes one halving that no record holds, unsplit_of() == 1.  Walk order: the current node's children, then those of
the frame below it, down to the oldest.  A child's contribution to its owner is many_spread_walk.contribution, and an
owner's `halvings` is its own count, plus the unsplit of each of its fanned walks, plus the counts of its sub-instances.

FromOrdered(text, row, objective, order, split_width, start) is many_walk_ordered.Walk with a start incumbent under the
rules of many_clause_from_walk.From.  spread_all() and spread_minmax() are the drivers of
many_clause_spread_walk.spread_many and many_clause_from_walk.spread_minmax over these walks, with the `halvings` fold.
props are not compared on the host, for the reason given in many_clause_spread_walk."""
import bisect

import numpy as np

import many_walk_objective as W
import many_walk_ordered as O
from many_clause_from_walk import better, bound
from many_spread_walk import BIG, contribution
from many_walk_ordered import BAD_ROOT, DONE, LIMIT  # noqa: F401

FIELDS = W.FIELDS + ("halvings",)  # status, nodes, cuts, solutions, halvings


def frames_of(walk):
    """the frames of a stopped ordered walk, the oldest first, the current node last: [(node, variable, next)]"""
    assert walk.open
    return walk.stack + [(walk.cur, walk.v, walk.nv)]


def frame_kind(node, v, nv, split, current):
    """-> "enumerating", "second" (a halving frame with its second half left) or "unsplit" (neither half tried)"""
    lo, hi = int(node[v, 0]), int(node[v, 1])
    if hi - lo + 1 > split:
        mid = (lo + hi) >> 1
        if nv == mid + 1:
            return "second"
        assert current and nv == lo, "a halving frame stands at mid + 1 or, the current node only, at lo"
        return "unsplit"
    assert lo <= nv <= hi
    return "enumerating"


def frame_children(node, v, nv, split, current):
    """the bounds [a, b] the frame's variable takes in each of its children, in walk order"""
    lo, hi = int(node[v, 0]), int(node[v, 1])
    kind = frame_kind(node, v, nv, split, current)
    if kind == "enumerating":
        return [(x, x) for x in range(nv, hi + 1)]
    mid = (lo + hi) >> 1
    return [(mid + 1, hi)] if kind == "second" else [(lo, mid), (mid + 1, hi)]


def _frames_with_children(walk):
    frames = frames_of(walk)
    return [(node, v, frame_children(node, v, nv, walk.split, d == len(frames) - 1)) for d, (node, v, nv) in enumerate(frames)]


def count_children(walk):
    """untried children of a stopped ordered walk"""
    return sum(len(kids) for _, _, kids in _frames_with_children(walk))


def children_of(walk):
    """-> int32 [children, n, 2]: the root rows of the untried children of a stopped ordered walk, in walk order"""
    rows = []
    for node, v, kids in reversed(_frames_with_children(walk)):
        for a, b in kids:
            row = node.copy()
            row[v] = (a, b)
            rows.append(row)
    return np.stack(rows).astype(np.int32)


def unsplit_of(walk):
    """1 if the current node of a stopped ordered walk is a halving one with neither half tried, else 0"""
    return int(frame_kind(walk.cur, walk.v, walk.nv, walk.split, True) == "unsplit")


def kinds_of(walk):
    """-> dict: how many frames of each kind a stopped walk holds -- pushed_halving (a pushed frame that halves), unsplit,
    between (the current node between its halves), several (an enumerating frame with more than one value left)"""
    frames = frames_of(walk)
    out = dict(pushed_halving=0, unsplit=0, between=0, several=0)
    for d, (node, v, nv) in enumerate(frames):
        current = d == len(frames) - 1
        kind = frame_kind(node, v, nv, walk.split, current)
        out["pushed_halving"] += kind == "second" and not current
        out["between"] += kind == "second" and current
        out["unsplit"] += kind == "unsplit"
        out["several"] += kind == "enumerating" and int(node[v, 1]) - nv + 1 > 1
    return out


class FromOrdered(O.Walk):
    """many_walk_ordered.Walk whose instance starts with an incumbent it did not find itself (`start`: a value or None),
    as many_clause_from_walk.From is many_walk_objective.Walk with one"""

    def __init__(self, text, root_row, objective, order="smallest-domain", split_width=256, start=None):
        assert objective in ("MIN", "MAX")
        row = np.array(root_row, dtype=np.int32)
        self.start = None if start is None else int(start)
        self.emptied = False  # the start bound emptied dom[obj] of the root row
        _, dom = W.oracle_for(text)
        good = not ((row[:, 0] > row[:, 1]).any() or (row[:, 0] < dom[:, 0]).any() or (row[:, 1] > dom[:, 1]).any())
        if self.start is not None and good:
            ov = W.model_of(text).view.obj_var
            lo, hi = bound(W.SENSE[objective], int(row[ov, 0]), int(row[ov, 1]), self.start)
            if lo > hi:  # an inconsistent root node: DONE, no node, the oracle is not asked
                self.emptied = True
                self.order, self.split, self.halvings, self.deepest = order, split_width, 0, 0
                self.objective, self.sense, self.ov = objective, W.SENSE[objective], ov
                self.best, self.row = self.start, None
                self.orc = W.oracle_for(text)[0]
                self.out = dict(status=DONE, root_props=0, nodes=0, cuts=0, props=0, solutions=0)
                self.rows, self.stack, self.cur, self.v, self.nv, self.open = [], [], None, -1, 0, False
                return
            row[ov] = (lo, hi)
        super().__init__(text, row, objective, order, split_width)
        if self.best is None:  # (a root node that is the one solution is the instance's own)
            self.best = self.start

    @property
    def incumbent(self):
        """what a checkpoint's header holds: the own best, else the start, else None"""
        return self.best

    def result(self):
        out = super().result()
        if out["solutions"] == 0:
            out["best"], out["first"] = None, None
        return out


def walk_from(text, row, objective, order, split_width, start=None, max_nodes=1 << 62):
    return FromOrdered(text, row, objective, order, split_width, start).run(max_nodes)


def _new_info():
    return dict(rounds=1, sub_instances=0, per_round=[], pushed_halving=0, unsplit=0, between=0, several=0, dead_rows=0,
                emptied=0, replaced_later=0, improved_later=0, tightened=0)


def _note_kinds(info, walk):
    for k, x in kinds_of(walk).items():
        info[k] += x


def spread_all(text, roots, order, split_width, budgets, max_rounds=1 << 30):
    """the ALL spread -> (per-owner dicts: FIELDS, root_props, props, first; info).  info counts, over the fanned
    checkpoints, the frames of every kind (kinds_of), and dead_rows: sub-rows inconsistent as roots (the +1 cut)"""
    def budget(rnd):
        return budgets[min(rnd, len(budgets) - 1)]

    def stopped(row, rnd):
        walk = O.Walk(text, row, "ALL", order, split_width)
        return walk, walk.run(budget(rnd))

    K = len(roots)
    batch, records = map(list, zip(*(stopped(row, 0) for row in roots)))
    owners = [{f: r[f] for f in FIELDS + ("root_props", "props")} for r in records]
    first = [r["first"] for r in records]
    pos = [0 if r["solutions"] > 0 else BIG for r in records]
    owner = list(range(K))
    info = _new_info()
    level = 0

    def leave():
        for t, r in enumerate(records):
            if r["status"] == LIMIT:
                owners[owner[t]]["status"] = LIMIT
        if level == 0:
            return
        for t, (r, o) in enumerate(zip(records, owner)):  # ascending: the lowest row of an owner comes first
            for f, x in contribution(r).items():
                owners[o][f] += x
            owners[o]["halvings"] += r["halvings"]
            info["dead_rows"] += r["status"] == DONE and r["nodes"] == 0 and r["solutions"] == 0
            if r["solutions"] > 0 and t < pos[o]:
                info["replaced_later"] += first[o] is not None
                first[o] = r["first"]
                pos[o] = t

    while info["rounds"] < max_rounds:
        index = [t for t, r in enumerate(records) if r["status"] == LIMIT]
        if not index:
            break
        counts = [count_children(batch[t]) for t in index]
        rows = np.concatenate([children_of(batch[t]) for t in index])
        came_from = np.repeat(np.arange(len(index)), counts)
        for t in index:
            _note_kinds(info, batch[t])
            owners[owner[t]]["status"] = DONE  # it goes on in its children
        offsets = np.concatenate([[0], np.cumsum(counts)])
        for r in records:  # the stopped rows are left for their children
            if r["status"] == LIMIT:
                r["status"] = -1
        leave()
        for t in index:  # the halving a fanned walk owes, once
            owners[owner[t]]["halvings"] += unsplit_of(batch[t])
        pos = [int(offsets[bisect.bisect_left(index, p)]) for p in pos]
        owner = [owner[index[c]] for c in came_from]
        batch, records = map(list, zip(*(stopped(row, info["rounds"]) for row in rows)))
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


def spread_minmax(text, roots, objective, order, split_width, budgets, max_rounds=1 << 30):
    """the MIN / MAX spread -> (per-owner dicts: FIELDS, root_props, props, best, first; info).  info as spread_all's,
    and emptied: sub-rows whose start bound empties dom[obj], improved_later, tightened (many_clause_from_walk)"""
    sense = W.SENSE[objective]

    def budget(rnd):
        return budgets[min(rnd, len(budgets) - 1)]

    K = len(roots)
    batch = [FromOrdered(text, row, objective, order, split_width) for row in roots]
    records = [w.run(budget(0)) for w in batch]
    owners = [{f: r[f] for f in FIELDS + ("root_props", "props", "best", "first")} for r in records]
    owner = list(range(K))
    info = _new_info()
    level = 0

    def leave():
        for t, r in enumerate(records):
            if r["status"] == LIMIT:
                owners[owner[t]]["status"] = LIMIT
        if level == 0:
            return
        found = {}
        for t, (r, o) in enumerate(zip(records, owner)):  # ascending: the lowest row of a value comes first
            for f, x in contribution(r).items():
                owners[o][f] += x
            owners[o]["halvings"] += r["halvings"]
            info["dead_rows"] += r["status"] == DONE and r["nodes"] == 0 and r["solutions"] == 0
            info["emptied"] += batch[t].emptied
            if r["solutions"] > 0 and (o not in found or better(sense, r["best"], records[found[o]]["best"])):
                found[o] = t
        for o, t in found.items():
            if better(sense, records[t]["best"], owners[o]["best"]):
                info["improved_later"] += owners[o]["best"] is not None
                owners[o]["best"], owners[o]["first"] = records[t]["best"], records[t]["first"]

    while info["rounds"] < max_rounds:
        index = [t for t, r in enumerate(records) if r["status"] == LIMIT]
        if not index:
            break
        for t in index:
            owners[owner[t]]["status"] = DONE  # it goes on in its children
        for r in records:  # the stopped rows are left for their children
            if r["status"] == LIMIT:
                r["status"] = -1
        leave()
        rows, starts, new_owner = [], [], []
        for t in index:
            _note_kinds(info, batch[t])
            owners[owner[t]]["halvings"] += unsplit_of(batch[t])
            kids = children_of(batch[t])
            assert len(kids) == count_children(batch[t])
            start, mine = batch[t].incumbent, owners[owner[t]]["best"]
            if mine is not None and better(sense, mine, start):
                start = mine
                info["tightened"] += len(kids)
            rows.extend(kids)
            starts.extend([start] * len(kids))
            new_owner.extend([owner[t]] * len(kids))
        owner = new_owner
        batch = [FromOrdered(text, row, objective, order, split_width, s) for row, s in zip(rows, starts)]
        records = [w.run(budget(info["rounds"])) for w in batch]
        level += 1
        info["rounds"] += 1
        info["sub_instances"] += len(batch)
        info["per_round"].append(len(batch))
    leave()
    return [dict(o) for o in owners], info


# ---- the row sets of the ordered-spread tests (the project's own; each finishes within 2^15 nodes per row) ----
import functools  # noqa: E402

import many_clause_sets as sets  # noqa: E402
import order_walk  # noqa: E402


def _recorded(name):
    text = order_walk.text_of(name)
    return text, O.root_row(text)


# (set, objective, order, split_width, budgets)
ALL_CASES = [("wcet_max", "ALL", "largest-value", 4, (8, 64)),
             ("wide2_mid", "ALL", "none", 16, (8, 64)),
             ("wide2_mid", "ALL", "smallest-domain", 16, (8, 64)),
             ("wide3_plain", "ALL", "smallest-domain", 16, (8, 64))]
MINMAX_CASES = [("schedule5_open_min", "MIN", "none", 4, (4, 16)),
                ("schedule5_open_min", "MIN", "smallest-domain", 4, (4, 16)),
                ("schedule6_min_budget", "MIN", "smallest-value", 4, (16, 64)),
                ("wcet_max", "MAX", "none", 4, (8, 32))]
FINISH = 1 << 15  # nodes per row within which every set above finishes


@functools.lru_cache(maxsize=None)
def rows_of(name):
    """-> (text, roots [K, n, 2] int32, read-only)"""
    if name in ("wide2_mid", "wide3_plain"):
        text, roots = _recorded(name)
    elif name in O.SETS:
        text, roots = O.build(name)[:2]
    else:
        text, roots = sets.build(name)[:2]
    roots = np.ascontiguousarray(roots, dtype=np.int32)
    roots.setflags(write=False)
    return text, roots


@functools.lru_cache(maxsize=None)
def one_walk(name, objective, order, split_width):
    """the one host walk of every row of a set, to the end (computed once, shared, not to be changed)"""
    text, roots = rows_of(name)
    res = O.walk_many(text, roots, objective, FINISH, order, split_width)
    for a in res.values():
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def spread_of(name, objective, order, split_width, budgets, max_rounds=1 << 30):
    """the host spread of a set (computed once, shared, not to be changed) -> (per-owner dicts, info)"""
    text, roots = rows_of(name)
    if objective == "ALL":
        return spread_all(text, roots, order, split_width, budgets, max_rounds)
    return spread_minmax(text, roots, objective, order, split_width, budgets, max_rounds)


@functools.lru_cache(maxsize=None)
def stopped_walks(name, objective, order, split_width, budget):
    """the walks of a set after `budget` nodes -> [(walk, record)]; MIN / MAX walks are FromOrdered without a start"""
    text, roots = rows_of(name)
    out = []
    for row in roots:
        walk = O.Walk(text, row, "ALL", order, split_width) if objective == "ALL" else \
            FromOrdered(text, row, objective, order, split_width)
        out.append((walk, walk.run(budget)))
    return out
