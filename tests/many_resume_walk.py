"""The walk of tests/many_walk.py as an object that can stop and go on (a helper module of test_many_resume_host.py and
test_gpu_many_resume.py, no test itself): what a checkpointed Model.solve_many followed by Model.resume_many is specified
to compute, and what Model.checkpoint_states is specified to list.

Walk(text, root_row, objective).run(budget) tries at most `budget` more children and returns the counters so far, in
many_walk.dive()'s form; the budget is checked before a child is tried, as there.  A stopped walk is "try value nv of
variable v on the node cur" over a stack of (node, variable, next value) frames; open_subtrees() lists them as states,
the oldest frame first and the current node last: the node with the variable narrowed to [next value, its upper bound].
Such a state is not at the fixpoint yet (the next value has not been pushed)."""
import numpy as np

import many_walk
from many_walk import BAD_ROOT, DONE, LIMIT


class Walk:
    def __init__(self, text, root_row, objective="ANY"):
        assert objective in ("ANY", "ALL")
        self.text, self.objective = text, objective
        self.orc, dom = many_walk.oracle_for(text)
        row = np.ascontiguousarray(root_row, dtype=np.int32)
        self.out = dict(status=DONE, root_props=0, nodes=0, cuts=0, props=0, solutions=0, first=None)
        self.stack, self.cur, self.v, self.nv = [], None, -1, 0
        self.open = False  # work left: the walk stands before a child
        if (row[:, 0] > row[:, 1]).any() or (row[:, 0] < dom[:, 0]).any() or (row[:, 1] > dom[:, 1]).any():
            self.out["status"] = BAD_ROOT
            return
        status, cur = self.orc.instance(row, -1, 0, 0)
        if status < 0:
            return
        self.out["root_props"] = status
        if (cur[:, 0] == cur[:, 1]).all():
            self.out["solutions"] = 1
            self.out["first"] = cur[:, 0].copy()
            return
        self.cur = cur
        self.v, self.nv = self._branch(cur)
        self.open = True

    @staticmethod
    def _branch(state):
        width = (state[:, 1] - state[:, 0]).astype(np.int64)
        width[width == 0] = 1 << 40
        v = int(np.argmin(width))
        return v, int(state[v, 0])

    def result(self):
        out = dict(self.out)
        if out["first"] is not None:
            out["first"] = out["first"].copy()
        return out

    def run(self, budget):
        """at most `budget` more children -> the counters so far (status LIMIT: stopped with work left)"""
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
                    if out["first"] is None:
                        out["first"] = child[:, 0].copy()
                    if self.objective == "ANY":
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
                self.cur, self.v, self.nv = self.stack.pop()
            else:
                self.nv = value + 1
        self.open = False
        return self.result()

    def frames(self):
        """the frames of a stopped walk, the oldest first, the current node last: [(node [n, 2], variable, next value)]"""
        assert self.open
        return self.stack + [(self.cur, self.v, self.nv)]

    def open_subtrees(self):
        """-> int32 [depth + 1, n, 2]: every frame's node with its variable narrowed to the values not tried yet"""
        rows = []
        for node, v, nv in self.frames():
            row = node.copy()
            row[v, 0] = nv
            rows.append(row)
        return np.stack(rows).astype(np.int32)

    def has_last_value_frame(self):
        """does some frame stand before the LAST value of its variable (its state has a new valued variable)?"""
        return any(nv == node[v, 1] for node, v, nv in self.frames())


def solutions_below(text, states):
    """solutions of the ALL trees below `states`: each propagated as a root row, then walked; a state that is a solution
    after propagation counts one (dive() does exactly this with a root row)"""
    return sum(many_walk.dive(text, s, "ALL")["solutions"] for s in states)
