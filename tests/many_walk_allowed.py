"""What Model.solve_many(branching="allowed") and solve_many_upto(branching="allowed") are specified to compute, on the
host (a helper module of the solve_many_allowed tests, no test itself).

The walk is many_walk.Walk's except for the branching (include/csolve_gpu.h, "Branching on the allowed values"): at a
node, a value c of an open variable w is FORBIDDEN when some valued variable u and some clause w != u + d of the model
has c == value(u) + d; the other values of [lo, hi] are allowed.  The walk branches on the open variable with the fewest
allowed values, ties to the lowest index, and tries only those, ascending.  A forbidden value is no node.  A frame stays
(node, variable, value + 1): coming back to it the walk goes on at the first allowed value >= that.

The != relation comes from the model's TEXT, not from the product: relation(text) parses the `A + a != B + b` and
all_different(...) lines that problems.queens / sudoku / offsets / sparse_ne write, keyed by the oracle's variable
numbers (Model.names()).  test_solve_many_allowed_host.py pins it against the oracle's own shaving."""
import re

import numpy as np

import many_walk
from many_walk import DONE, LIMIT, BAD_ROOT, FIELDS, first_of, gather, walk_each  # noqa: F401

_relations = {}
_TERM = re.compile(r"^\s*([A-Za-z_]\w*)\s*(?:([+-])\s*(\d+))?\s*$")


def _term(s):
    m = _TERM.match(s)
    assert m, f"not a `variable +- constant` term: {s!r}"
    return m.group(1), (int(m.group(3)) if m.group(3) else 0) * (-1 if m.group(2) == "-" else 1)


def relation(text):
    """-> [n] lists of (u, d): variable w != variable u + d, both directions of every clause, duplicates removed"""
    if text in _relations:
        return _relations[text]
    many_walk.oracle_for(text)
    index = {name: i for i, name in enumerate(many_walk._models[text][2].names())}
    rel = [set() for _ in index]

    def differ(a, b):  # a = (name, const), b likewise: name_a + const_a != name_b + const_b
        if a[0] == b[0]:
            return
        w, u = index[a[0]], index[b[0]]
        rel[w].add((u, b[1] - a[1]))
        rel[u].add((w, a[1] - b[1]))

    for line in text.split("\n"):
        line = line.split("#", 1)[0]
        for stmt in line.split(";"):
            stmt = stmt.strip()
            if stmt.startswith("all_different("):
                terms = [_term(t) for t in stmt[len("all_different("):stmt.rindex(")")].split(",")]
                for i in range(len(terms)):
                    for j in range(i + 1, len(terms)):
                        differ(terms[i], terms[j])
            elif "!=" in stmt:
                a, b = stmt.split("!=")
                differ(_term(a), _term(b))
    _relations[text] = [sorted(s) for s in rel]
    return _relations[text]


def allowed(rel, state, w):
    """the allowed values of the open variable w in the node `state`, ascending"""
    lo, hi = int(state[w, 0]), int(state[w, 1])
    forbidden = {int(state[u, 0]) + d for u, d in rel[w] if state[u, 0] == state[u, 1]}
    return [c for c in range(lo, hi + 1) if c not in forbidden]


class Walk(many_walk.Walk):
    """many_walk.Walk branching on the fewest allowed values and trying only those"""

    def __init__(self, text, root_row):
        self.rel = relation(text)
        self.check = None  # a callable(state, w, allowed values) for every open variable of every entered node
        super().__init__(text, root_row)

    def _branch(self, state):
        best, best_v = None, -1
        for w in np.nonzero(state[:, 0] != state[:, 1])[0]:
            a = allowed(self.rel, state, int(w))
            if self.check is not None:
                self.check(state, int(w), a)
            if best is None or len(a) < best:
                best, best_v = len(a), int(w)
        return best_v, int(state[best_v, 0])

    def _from(self, state, v, value):
        """the first allowed value >= value of variable v (at a fixpoint the upper bound is allowed)"""
        return next(c for c in allowed(self.rel, state, v) if c >= value)

    def run(self, budget, stop_at=None):
        """many_walk.Walk.run with the step to the next value replaced"""
        assert budget > 0 and (stop_at is None or stop_at >= 1)
        out = self.out
        if not self.open:
            return self.result()
        out["status"] = DONE
        if stop_at is not None and out["solutions"] >= stop_at:
            self.open = False
            return self.result()
        tried = 0
        while True:
            if tried >= budget:
                out["status"] = LIMIT
                return self.result()
            cur, v = self.cur, self.v
            value, last = self.nv, self.nv == cur[v, 1]
            status, child = self.orc.instance(cur, v, value, value)
            out["nodes"] += 1
            tried += 1
            descend = False
            if status < 0:
                out["cuts"] += 1
            else:
                out["props"] += status
                if (child[:, 0] == child[:, 1]).all():
                    out["solutions"] += 1
                    self.rows.append(child[:, 0].copy())
                    if stop_at is not None and out["solutions"] >= stop_at:
                        break
                else:
                    descend = True
            if descend:
                if not last:
                    self.stack.append((cur, v, value + 1))
                self.cur = child
                self.v, self.nv = self._branch(child)
            elif last:
                if not self.stack:
                    break
                self.cur, self.v, nv = self.stack.pop()
                self.nv = self._from(self.cur, self.v, nv)
            else:
                self.nv = self._from(cur, v, value + 1)
        self.open = False
        return self.result()


def dive(text, root_row, objective="ANY", max_nodes=1 << 62):
    """many_walk.dive on the allowed-values walk"""
    assert objective in ("ANY", "ALL") and max_nodes > 0
    return first_of(Walk(text, root_row).run(max_nodes, 1 if objective == "ANY" else None))


def upto(text, root_row, k, max_nodes=1 << 62):
    """-> the counters and `rows`, at most k solutions in walk order"""
    return Walk(text, root_row).run(max_nodes, k)


def dive_many(text, roots, objective="ANY", max_nodes=1 << 62):
    return gather(walk_each(roots, lambda row, _: dive(text, row, objective, max_nodes)), np.shape(roots)[1])


def upto_many(text, roots, k, max_nodes=1 << 62):
    return gather(walk_each(roots, lambda row, _: upto(text, row, k, max_nodes)), np.shape(roots)[1], width=k)
