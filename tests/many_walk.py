"""What Model.solve_many and its family are specified to compute, on the host with the oracle for every node (a helper
module of the solve_many tests, no test itself).

Walk(text, root_row): the instance `root_row` of the model `text` -- the root node through the oracle
(Oracle.instance(row, -1, 0, 0): the full root fixpoint), then depth-first: branching variable = the open variable with
the smallest interval, ties to the lowest index; values in ascending order; every child through Oracle.instance; a
consistent child with open variables is entered at once and its parent comes back for its next value afterwards.
Counters as the engine defines them: nodes = children tried, cuts = inconsistent children, props = the oracle's PROPS of
the consistent children, solutions; root_props = the narrowings of the root node (0 when it is inconsistent).  A root
row that is a solution already is the one solution, row 0.

run(budget, stop_at) tries at most `budget` more children and leaves right after solution number `stop_at` (1 is ANY,
None is ALL, k is "up to k"); every solution is kept, in walk order.  The budget is checked before a child is tried: a
walk that would need one more node stops with LIMIT.  A stopped walk is "try value nv of variable v on the node cur"
over a stack of (node, variable, next value) frames, and run() goes on from there; a walk that already holds `stop_at`
solutions when it is continued ends DONE before it tries a node, its counters as they were.  open_subtrees() lists the
frames as states, the oldest first and the current node last: the node with the variable narrowed to [next value, its
upper bound].  Such a state is not at the fixpoint yet (the next value has not been pushed).

dive() is one run() with a single budget, in Model.solve_many's terms (ANY / ALL, the first solution)."""
import numpy as np

DONE, LIMIT, BAD_ROOT = 0, 1, 2
FIELDS = ("status", "root_props", "nodes", "cuts", "props", "solutions")

_models = {}


def oracle_for(text):
    """(oracle on the model with its root domains, those domains): the model as solve_root leaves it"""
    if text not in _models:
        from oracle.cs_oracle import Model as OModel, Oracle
        om = OModel.parse(text)
        orc = Oracle(om)
        orc.set_root_phase(True)
        assert orc.propagate(om.root, om.n_vars) >= 0, "infeasible model"
        dom = orc.domains()
        om.set_domains(dom)
        om.index()
        _models[text] = (Oracle(om), dom, om)
    return _models[text][:2]


class Walk:
    def __init__(self, text, root_row):
        self.orc, dom = oracle_for(text)
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

    def run(self, budget, stop_at=None):
        """at most `budget` more children, leaving at solution number `stop_at` -> the counters so far and the solutions
        in order (status LIMIT: stopped at the budget with work left)"""
        assert budget > 0 and (stop_at is None or stop_at >= 1)
        out = self.out
        if not self.open:
            return self.result()
        out["status"] = DONE
        if stop_at is not None and out["solutions"] >= stop_at:  # a smaller stop than the slice before: nothing is tried
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


def first_of(result):
    """a Walk result in dive()'s form: `first` (the first solution, or None) in place of `rows`"""
    rows = result.pop("rows")
    result["first"] = rows[0] if rows else None
    return result


def dive(text, root_row, objective="ANY", max_nodes=1 << 62):
    """-> dict(status, root_props, nodes, cuts, props, solutions, first): first = the first solution found (int32 [n]) or
    None"""
    assert objective in ("ANY", "ALL") and max_nodes > 0
    return first_of(Walk(text, root_row).run(max_nodes, 1 if objective == "ANY" else None))


def walk_each(roots, walk, tags=None):
    """[walk(row, tag) of every row of int32 `roots` [K, n, 2]], tag = tags[i] (None without tags); equal (row, tag)
    pairs are walked once"""
    seen, results = {}, []
    for i, row in enumerate(np.ascontiguousarray(roots, dtype=np.int32)):
        tag = None if tags is None else tags[i]
        if (row.tobytes(), tag) not in seen:
            seen[row.tobytes(), tag] = walk(row, tag)
        results.append(seen[row.tobytes(), tag])
    return results


def gather(results, n, fields=FIELDS, width=None):
    """per-instance result dicts -> dict of arrays shaped like the answers of the solve_many family: `fields` int64 [K];
    `first` int32 [K, n] (width None) or `rows` int32 [K, width, n], zeros where there is none"""
    K = len(results)
    res = {f: np.zeros(K, dtype=np.int64) for f in fields}
    res["first" if width is None else "rows"] = np.zeros((K, n) if width is None else (K, width, n), dtype=np.int32)
    for i, d in enumerate(results):
        for f in fields:
            res[f][i] = d[f]
        if width is not None:
            for j, row in enumerate(d["rows"][:width]):
                res["rows"][i, j] = row
        elif d["first"] is not None:
            res["first"][i] = d["first"]
    return res


def dive_many(text, roots, objective="ANY", max_nodes=1 << 62):
    """dive() of every row -> dict of arrays shaped like Model.solve_many's answer (first: zeros where there is none);
    equal rows are walked once"""
    return gather(walk_each(roots, lambda row, _: dive(text, row, objective, max_nodes)), np.shape(roots)[1])
