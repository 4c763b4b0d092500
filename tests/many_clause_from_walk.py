"""What csgpu_solve_many_clauses_from and Model.solve_many_clauses_spread under MIN / MAX are specified to compute
(include/csolve_gpu.h), on the host (a helper module of test_solve_many_clauses_from_host.py and
test_gpu_solve_many_clauses_from.py, no test itself).  many_walk_objective, many_spread_walk and the oracle are its sources.

From(text, row, objective, start) is many_walk_objective.Walk whose instance starts with an incumbent it did not find
itself (`start`: a value or None):
  - the incumbent of the walk is `start` until the instance has a solution of its own: it bounds every child as the
    private incumbent does, and dom[obj] of the ROOT ROW takes the bound before the root node's fixpoint.  A bound that
    empties dom[obj] makes the root node inconsistent: DONE, 0 nodes, 0 solutions (the oracle is not asked)
  - result()["best"] and ["first"] are those of own solutions only: None for an instance that proves that nothing beats
    its start.  `incumbent` is what a checkpoint's header holds: the own best, else the start, else None
start = None is many_walk_objective.Walk, field for field.

spread_minmax(text, roots, objective, budgets, max_rounds) is the driver of many_clause_spread_walk.spread_many for a MIN /
MAX walk: round 0 walks every root row with budgets[0] and no start; every later round lists the children of all stopped
walks of the batch (many_spread_walk.children_of, in the order of the batch) and walks them as From rows with that
round's budget.  A batch is folded once, when it is left: the counters by many_spread_walk.contribution; an owner's best /
first are replaced only by a STRICTLY better value, and take the lowest row of the batch that holds the batch's best.  A
child starts from the strictly better of its checkpoint's incumbent and its owner's best after that fold.  An owner is
DONE when all its sub-instances are, else LIMIT with the best folded so far (best None, solutions 0 if nothing was found).
-> (per-owner dicts: FIELDS, best, first; info)."""
import numpy as np

import many_walk
import many_walk_objective as W
from many_spread_walk import children_of, contribution, count_children
from many_walk_objective import BAD_ROOT, DONE, LIMIT  # noqa: F401

FIELDS = W.FIELDS  # status, nodes, cuts, solutions


def better(sense, a, b):
    """is the value a strictly better than b (b None: anything is)?"""
    return b is None or (a < b if sense == 1 else a > b)


def bound(sense, lo, hi, best):
    """dom[obj] = [lo, hi] under the incumbent `best`"""
    return (lo, min(hi, best - 1)) if sense == 1 else (max(lo, best + 1), hi)


class From(W.Walk):
    def __init__(self, text, root_row, objective, start=None):
        assert objective in ("MIN", "MAX")
        row = np.array(root_row, dtype=np.int32)
        self.start = None if start is None else int(start)
        _, dom = W.oracle_for(text)
        good = not ((row[:, 0] > row[:, 1]).any() or (row[:, 0] < dom[:, 0]).any() or (row[:, 1] > dom[:, 1]).any())
        if self.start is not None and good:
            ov = W.model_of(text).view.obj_var
            lo, hi = bound(W.SENSE[objective], int(row[ov, 0]), int(row[ov, 1]), self.start)
            if lo > hi:  # the bound empties dom[obj]: an inconsistent root node
                self.objective, self.sense, self.ov = objective, W.SENSE[objective], ov
                self.best, self.row = self.start, None
                self.orc = W.oracle_for(text)[0]
                self.out = dict(status=DONE, root_props=0, nodes=0, cuts=0, props=0, solutions=0)
                self.rows, self.stack, self.cur, self.v, self.nv, self.open = [], [], None, -1, 0, False
                return
            row[ov] = (lo, hi)
        super().__init__(text, row, objective)
        if self.best is None:  # (a root node that is the one solution is the instance's own)
            self.best = self.start

    @property
    def incumbent(self):
        return self.best

    def result(self):
        out = super().result()
        if out["solutions"] == 0:
            out["best"], out["first"] = None, None
        return out


def walk_from(text, row, objective, start=None, max_nodes=1 << 62):
    return From(text, row, objective, start).run(max_nodes)


def spread_minmax(text, roots, objective, budgets, max_rounds=1 << 30):
    """-> (per-owner dicts, info).  info = dict(rounds, sub_instances, per_round, ties: (owner, batch) pairs whose best
    value of the batch is held by more than one row, dead: sub-rows inconsistent as roots (the +1 cut), the start bound
    among the reasons, nosol_done: sub-instances that walked nodes and ended DONE without a solution of their own,
    improved_later: replacements of an owner's best by a strictly better one, tightened: children that start from their
    owner's best because it beats their checkpoint's incumbent)"""
    sense = W.SENSE[objective]

    def budget(rnd):
        return budgets[min(rnd, len(budgets) - 1)]

    K = len(roots)
    batch = [From(text, row, objective) for row in roots]
    records = [w.run(budget(0)) for w in batch]
    owners = [{f: r[f] for f in FIELDS + ("root_props", "props", "best", "first")} for r in records]
    owner = list(range(K))
    info = dict(rounds=1, sub_instances=0, per_round=[], ties=0, dead=0, nosol_done=0, improved_later=0, tightened=0)
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
            info["dead"] += r["status"] == DONE and r["nodes"] == 0 and r["solutions"] == 0
            info["nosol_done"] += r["status"] == DONE and r["nodes"] > 0 and r["solutions"] == 0
            if r["solutions"] > 0:
                if o not in found or better(sense, r["best"], records[found[o][0]]["best"]):
                    found[o] = [t, 1]
                elif r["best"] == records[found[o][0]]["best"]:
                    found[o][1] += 1
        for o, (t, holders) in found.items():
            info["ties"] += holders > 1
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
        batch = [From(text, row, objective, s) for row, s in zip(rows, starts)]
        records = [w.run(budget(info["rounds"])) for w in batch]
        level += 1
        info["rounds"] += 1
        info["sub_instances"] += len(batch)
        info["per_round"].append(len(batch))
    leave()
    return [dict(o) for o in owners], info


def gather(results, n):
    """per-owner dicts -> arrays shaped like the spread's answer: FIELDS int64 [K], has bool [K], best int64 [K], first [K, n]"""
    res = many_walk.gather([dict(r, root_props=r.get("root_props", 0), props=r.get("props", 0)) for r in results], n)
    res["has"] = np.array([r["best"] is not None for r in results])
    res["best"] = np.array([0 if r["best"] is None else r["best"] for r in results], dtype=np.int64)
    return res
