"""What Model.solve_many_clauses_ordered is specified to compute (include/csolve_gpu.h), on the host with the oracle for
every node (a helper module of the ordered-walk tests, no test itself): many_walk_objective.Walk with two changes.

  branching variable   the open variable with the smallest order_walk.branch_key(order, False, lo, hi, 0, index): the
                       reference's five orders, ties to the lowest index
  children             a node whose branching variable has more than `split_width` values (hi - lo + 1, a Python
                       integer) has two: [lo, mid], then [mid + 1, hi], mid = (lo + hi) >> 1 (a floor); any other node
                       its values in ascending order.  Whether a node halves, and its mid, come from the node as it was
                       entered, before any incumbent bound, so a frame popped later makes the same children.  A half is
                       "narrow the variable, then the fixpoint": a node in `nodes`, a cut if the fixpoint fails or the
                       incumbent's bound empties dom[obj].  A halving parent is counted once, in `halvings`, when its
                       first half is tried

Everything else is many_walk_objective.Walk's: the root node, the counters, the budget compared before a child is tried,
a child entered at once and its parent pushed only while it has children left, ANY / ALL / MIN / MAX and the incumbent.
A frame is (node, variable, next): next is a value, or mid + 1 for the second half of a halving node -- the kind is read
back from the node, as the kernel reads it from the frame's row.  result() adds `halvings` and `deepest`, the most
frames the stack ever held (the current node not counted).

frames(domains, split_width) is the frame bound of csgpu_many_clauses_ordered_frames as plain integers.  The row sets of
the ordered tests are here as well (SETS, build, walked).  Nothing here calls the product's library."""
import functools

import numpy as np

import many_clause_sets as sets
import many_walk
import many_walk_objective as W
import order_walk
import search_sets
from csolve_amd import problems
from many_walk import BAD_ROOT, DONE, LIMIT  # noqa: F401

ORDERS = order_walk.ORDERS
FIELDS = many_walk.FIELDS + ("halvings", "deepest")
_INDEX = (1 << 32) - 1


class Walk(W.Walk):
    def __init__(self, text, root_row, objective="ANY", order="smallest-domain", split_width=256):
        assert order in ORDERS and split_width >= 1
        self.order, self.split = order, split_width
        self.halvings, self.deepest = 0, 0
        super().__init__(text, root_row, objective)

    def _branch(self, state):
        keys = [order_walk.branch_key(self.order, False, lo, hi, 0, i) for i, (lo, hi) in enumerate(state.tolist()) if lo != hi]
        v = min(keys) & _INDEX
        return v, int(state[v, 0])

    def _child(self, cur, v, a, b):
        """the child `v in [a, b]` of the node `cur` under the incumbent -> (status, state)"""
        if self.sense and self.best is not None:
            row = cur.copy()
            row[v] = (a, b)
            lo, hi = int(row[self.ov, 0]), int(row[self.ov, 1])
            if self.sense == 1:
                hi = min(hi, self.best - 1)
            else:
                lo = max(lo, self.best + 1)
            if lo > hi:
                return -1, None
            if (lo, hi) != (int(row[self.ov, 0]), int(row[self.ov, 1])):
                row[self.ov] = (lo, hi)
                return self.orc.instance(row, -1, 0, 0)
        return self.orc.instance(cur, v, a, b)

    def result(self):
        out = super().result()
        out["halvings"], out["deepest"] = self.halvings, self.deepest
        return out

    def run(self, budget):
        assert budget > 0
        out = self.out
        if not self.open:
            return self.result()
        out["status"] = DONE
        tried = 0
        while True:
            if tried >= budget:
                out["status"] = LIMIT
                return self.result()
            cur, v = self.cur, self.v
            lo, hi = int(cur[v, 0]), int(cur[v, 1])
            if hi - lo + 1 > self.split:  # the node as it was entered decides, and fixes mid
                mid = (lo + hi) >> 1
                first = self.nv == lo
                a, b = (lo, mid) if first else (self.nv, hi)
                assert first or self.nv == mid + 1
                last, then = not first, mid + 1
                self.halvings += first
            else:
                a = b = self.nv
                last, then = self.nv == hi, self.nv + 1
            status, child = self._child(cur, v, a, b)
            out["nodes"] += 1
            tried += 1
            descend = False
            if status < 0:
                out["cuts"] += 1
            else:
                out["props"] += status
                if (child[:, 0] == child[:, 1]).all():
                    out["solutions"] += 1
                    self._solution(child[:, 0])
                    if self.objective == "ANY":
                        break
                else:
                    descend = True
            if descend:
                if not last:
                    self.stack.append((cur, v, then))
                    self.deepest = max(self.deepest, len(self.stack))
                self.cur = child
                self.v, self.nv = self._branch(child)
            elif last:
                if not self.stack:
                    break
                self.cur, self.v, self.nv = self.stack.pop()
            else:
                self.nv = then
        self.open = False
        return self.result()


def walk(text, root_row, objective="ANY", max_nodes=1 << 62, order="smallest-domain", split_width=256):
    return Walk(text, root_row, objective, order, split_width).run(max_nodes)


def walk_many(text, roots, objective="ANY", max_nodes=1 << 62, order="smallest-domain", split_width=256):
    """walk() of every row -> dict of arrays shaped like Model.solve_many_clauses_ordered's answer: many_walk_objective's
    and halvings, deepest int64 [K]; equal rows are walked once"""
    results = many_walk.walk_each(roots, lambda row, _: walk(text, row, objective, max_nodes, order, split_width))
    res = many_walk.gather(results, np.shape(roots)[1], FIELDS)
    res["best"] = np.array([0 if d["best"] is None else d["best"] for d in results], dtype=np.int64)
    return res


def frames(domains, split_width):
    """the frames a wave needs: n + sum of h(v), h(v) the smallest h for which the root width of v, halved h times with
    ceiling, is at most split_width.  A pushed frame either values a variable (at most n - 1 of those and the current
    node) or is a halving parent with its second half left, and along a path a variable is halved at most h(v) times:
    rows lie inside the root domains and intervals only shrink."""
    total = len(domains)
    for lo, hi in np.asarray(domains).tolist():
        w = hi - lo + 1
        while w > split_width:
            w = (w + 1) >> 1
            total += 1
    return total


def root_row(text):
    """the root-domain row of `text` as many_walk_objective.oracle_for normalises the model: [1, n, 2] int32"""
    return np.ascontiguousarray(W.oracle_for(text)[1][None], dtype=np.int32)


# the sets whose recorded ALL trees (order_walk.RECORDED) the walk reproduces from the root-domain row, under every
# recorded order
RECORDED_SETS = ["narrow_sums7", "narrow_plain7", "infeasible6", "wide2_cut", "wide2_straddle", "wide2_mid", "wide3_sums",
                 "wide3_plain", "planted30", "planted80", "queens7", "queens8", "offsets6x5"]
RECORDED_PAIRS = [(name, order) for name in RECORDED_SETS for order in order_walk.orders_of(name)]
WIDE = ["wide2_cut", "wide2_straddle", "wide2_mid", "wide3_sums", "wide3_plain"]


def _open_end():
    """schedule(5, 1) with windows for the start times only: `end` and "<obj>" keep their root width of 2,147,483,639
    values, which the plain walk enumerates until its budget and this one halves"""
    text = problems.schedule(5, 1)
    return text, sets.windows(text, 8, 4, 30, select=lambda name: name.endswith("_start"))


def _of(name):
    return lambda: sets.build(name)[:2]


def _wide2_mid_any():
    text = search_sets.text_of("wide2_mid", "ANY")
    return text, root_row(text)


BUDGET = 1 << 15
# name -> (builder of (text, roots), objective, max_nodes, [(order, split_width)], whole)
SETS = {
    "schedule5_open_min": (_open_end, "MIN", BUDGET, [(o, s) for o in ORDERS for s in (256, 4)], True),
    "wcet_max": (_of("wcet_max"), "MAX", BUDGET, [("largest-value", 256), ("none", 4)], True),
    "linear12_any": (_of("linear12_any"), "ANY", 4096, [("largest-domain", 256), ("smallest-value", 2)], True),
    "wide2_mid_any": (_wide2_mid_any, "ANY", BUDGET, [("none", 256), ("largest-value", 16)], True),
    "schedule6_min_budget": (_of("schedule6_min_budget"), "MIN", 256, [("smallest-domain", 4), ("smallest-value", 4)], False),
}
CASES = [(name, order, split) for name, s in SETS.items() for order, split in s[3]]


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (text, roots [K, n, 2] int32, objective, max_nodes)"""
    make, objective, budget, _, _ = SETS[name]
    text, roots = make()
    roots = np.ascontiguousarray(roots, dtype=np.int32)
    roots.setflags(write=False)
    return text, roots, objective, budget


@functools.lru_cache(maxsize=None)
def walked(name, order, split_width):
    """the host walk of every instance of a set at its budget (computed once, shared by the tests, not to be changed)"""
    text, roots, objective, budget = build(name)
    res = walk_many(text, roots, objective, budget, order, split_width)
    for a in res.values():
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def recorded_walk(name, order):
    """the ALL walk of a recorded set from its root-domain row, once per process"""
    text = order_walk.text_of(name)
    return walk(text, root_row(text)[0], "ALL", order_walk.CAP + 1, order, order_walk.SPLIT_WIDTH)
