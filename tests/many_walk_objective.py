"""What Model.solve_many_clauses is specified to compute (include/csolve_gpu.h), on the host with the oracle for every
node (a helper module of the solve_many_clauses tests, no test itself): many_walk.Walk with an objective.

oracle_for(text) is many_walk.oracle_for for clause models: the root phase the product runs (root fixpoint, the
normaliser, root fixpoint again: solver.solve_root), so that a tree clause is the tree the device tables hold.  It fills
many_walk's own cache, so many_walk.Walk and many_walk.dive see the same model.

Walk(text, root_row, objective) adds to many_walk.Walk
  - the private incumbent of MIN / MAX: none at the start; before a child's fixpoint, once the instance has a solution,
    dom[obj] becomes the objective bound under `best`.  Kernel 6 revises every clause of a node, so the bound is
    propagated like the assignment: where it narrows dom[obj], the child is the oracle's full fixpoint (a `var < 0` node)
    of the parent with the assignment and the bound written in; where it does not, the child is Oracle.instance as in
    many_walk.  A bound that empties dom[obj] is a node and a cut, and the oracle is not asked.  A solution sets `best`
    to the value of "<obj>" and replaces the stored row; the walk goes on to the end of the tree
  - under ANY / ALL the model's "<obj>", if it has one, is an ordinary variable, and the stored row is the first solution
  - run(budget) as many_walk.Walk.run: at most `budget` more children, compared before a child is tried; a stopped walk
    goes on with the next run().  ANY leaves at the first solution.
result(): status, root_props, nodes, cuts, props, solutions, best (None without a solution or under ANY / ALL), first
(the stored row or None).  props are the oracle's, which kernel 6 does not promise (its order of narrowings differs): the
GPU tests compare props with kernel 6 itself, node by node."""
import numpy as np

import many_walk
from many_walk import BAD_ROOT, DONE, LIMIT  # noqa: F401

FIELDS = ("status", "nodes", "cuts", "solutions")
SENSE = {"ANY": 0, "ALL": 0, "MIN": 1, "MAX": 2}
CODE = {"ANY": 0, "ALL": 1, "MIN": 2, "MAX": 3}


def oracle_for(text):
    """(oracle on the model with its root domains, those domains), the model normalised as the product's tables are"""
    if text not in many_walk._models:
        from oracle.cs_oracle import Model as OModel, Oracle
        om = OModel.parse(text)
        for normalise in (True, False):  # root fixpoint, the normaliser, root fixpoint again
            orc = Oracle(om)
            orc.set_root_phase(True)
            assert orc.propagate(om.root, 1 << 20) >= 0, "infeasible model"
            om.set_domains(orc.domains())
            if normalise:
                om.normalize()
        om.index()
        many_walk._models[text] = (Oracle(om), om.domains(), om)
    return many_walk._models[text][:2]


def model_of(text):
    """the oracle's model behind oracle_for(text)"""
    oracle_for(text)
    return many_walk._models[text][2]


class Walk(many_walk.Walk):
    def __init__(self, text, root_row, objective="ANY"):
        om = model_of(text)
        self.objective, self.sense = objective, SENSE[objective]
        self.ov = om.view.obj_var
        if self.sense:
            assert self.ov >= 0 and om.view.objective == CODE[objective], "MIN / MAX: the model's own sense"
        self.best, self.row = None, None
        super().__init__(text, root_row)
        if self.rows:  # the root node was the one solution
            self._solution(self.rows[0])

    def _solution(self, row):
        if self.sense:
            self.best = int(row[self.ov])
        if self.sense or self.row is None:
            self.row = row.copy()

    def _child(self, cur, v, value):
        """the child `v = value` of the node `cur` under the incumbent -> (status, state)"""
        if self.sense and self.best is not None:
            row = cur.copy()
            row[v] = (value, value)
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
        return self.orc.instance(cur, v, value, value)

    def result(self):
        out = dict(self.out)
        out["best"] = self.best
        out["first"] = None if self.row is None else self.row.copy()
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
            value, last = self.nv, self.nv == cur[v, 1]
            status, child = self._child(cur, v, value)
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


def walk(text, root_row, objective="ANY", max_nodes=1 << 62):
    return Walk(text, root_row, objective).run(max_nodes)


def walk_many(text, roots, objective="ANY", max_nodes=1 << 62):
    """walk() of every row -> dict of arrays shaped like Model.solve_many_clauses's answer: status, root_props, nodes,
    cuts, props, solutions int64 [K], best int64 [K] (0 where there is none), first int32 [K, n] (zeros where there is
    none); equal rows are walked once"""
    results = many_walk.walk_each(roots, lambda row, _: walk(text, row, objective, max_nodes))
    res = many_walk.gather(results, np.shape(roots)[1])
    res["best"] = np.array([0 if d["best"] is None else d["best"] for d in results], dtype=np.int64)
    return res
