"""What Model.solve_many_upto is specified to compute, on the host with the oracle for every node (a helper module of
test_solve_many_upto_host.py and test_gpu_solve_many_upto.py, no test itself).

dive_upto(text, root_row, k, max_nodes) is many_walk.dive's walk -- the same root node, branching rule, value order,
counters and budget test -- with the stop moved: the instance leaves right after accepting its k-th solution (ANY leaves
after the first, ALL never), and every solution is kept, in walk order.  A root row that is a solution already is the
one solution, row 0.  WalkUpto is the same walk as an object that stops and goes on, in the manner of
many_resume_walk.Walk: run(budget, k) tries at most `budget` more children with the k of THIS slice; a walk that already
holds k solutions when it is continued ends DONE before it tries a node, its counters as they were."""
import numpy as np

import many_walk
from many_walk import BAD_ROOT, DONE, LIMIT

FIELDS = ("status", "root_props", "nodes", "cuts", "props", "solutions")


class WalkUpto:
    def __init__(self, text, root_row):
        self.orc, dom = many_walk.oracle_for(text)
        row = np.ascontiguousarray(root_row, dtype=np.int32)
        self.out = dict(status=DONE, root_props=0, nodes=0, cuts=0, props=0, solutions=0)
        self.rows = []  # the solutions in walk order
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
            self.rows.append(cur[:, 0].copy())
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
        out["rows"] = [r.copy() for r in self.rows]
        return out

    def run(self, budget, k):
        """at most `budget` more children, leaving at the k-th solution -> the counters so far and the solutions in order
        (status LIMIT: stopped at the budget with work left)"""
        assert budget > 0 and k >= 1
        out = self.out
        if not self.open:
            return self.result()
        out["status"] = DONE
        if out["solutions"] >= k:  # a smaller k than the slice before: nothing is tried
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
                    if out["solutions"] >= k:
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

    def open_subtrees(self):
        """as many_resume_walk.Walk.open_subtrees: every frame's node, its variable narrowed to the values not tried yet"""
        assert self.open
        rows = []
        for node, v, nv in self.stack + [(self.cur, self.v, self.nv)]:
            row = node.copy()
            row[v, 0] = nv
            rows.append(row)
        return np.stack(rows).astype(np.int32)


def dive_upto(text, root_row, k, max_nodes=1 << 62):
    """-> dict(status, root_props, nodes, cuts, props, solutions, rows): rows = the solutions found, in walk order (a list
    of int32 [n], at most k)"""
    return WalkUpto(text, root_row).run(max_nodes, k)


def dive_sliced(text, root_row, slices):
    """the walk in slices [(budget, k), ...] -> the result after the last one"""
    w = WalkUpto(text, root_row)
    out = w.result()
    for budget, k in slices:
        out = w.run(budget, k)
    return out


def _gather(results, K, n, k):
    res = {f: np.zeros(K, dtype=np.int64) for f in FIELDS}
    res["rows"] = np.zeros((K, k, n), dtype=np.int32)
    for i, d in enumerate(results):
        for f in FIELDS:
            res[f][i] = d[f]
        for j, row in enumerate(d["rows"][:k]):
            res["rows"][i, j] = row
    return res


def dive_many_upto(text, roots, k, max_nodes=1 << 62, slices=None):
    """dive_upto() of every row -> dict of arrays shaped like Model.solve_many_upto's answer (rows [K, k, n]: zeros where
    there is none); slices=[(budget, k), ...] walks every row in those slices instead (rows [K, max k, n]).  Equal rows
    are walked once."""
    roots = np.ascontiguousarray(roots, dtype=np.int32)
    seen, results = {}, []
    for row in roots:
        key = row.tobytes()
        if key not in seen:
            seen[key] = dive_upto(text, row, k, max_nodes) if slices is None else dive_sliced(text, row, slices)
        results.append(seen[key])
    width = k if slices is None else max(kk for _, kk in slices)
    if width > 1 << 20:  # "no k" on the host (e.g. 2**40): as many rows as the richest instance has
        width = max([len(d["rows"]) for d in results] + [1])
    return _gather(results, roots.shape[0], roots.shape[1], width)
