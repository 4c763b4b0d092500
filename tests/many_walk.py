"""What Model.solve_many is specified to compute, on the host with the oracle for every node (a helper module of
test_solve_many_host.py and test_gpu_solve_many.py, no test itself).

dive(text, root_row, objective, max_nodes): the instance `root_row` of the model `text` -- the root node through the
oracle (Oracle.instance(row, -1, 0, 0): the full root fixpoint), then depth-first: branching variable = the open variable
with the smallest interval, ties to the lowest index; values in ascending order; every child through Oracle.instance;
a consistent child with open variables is entered at once and its parent comes back for its next value afterwards.
Counters as the engine defines them: nodes = children tried, cuts = inconsistent children, props = the oracle's PROPS of
the consistent children, solutions; root_props = the narrowings of the root node (0 when it is inconsistent).  The
budget is checked before a child is tried: an instance that would need one more node stops with nodes == max_nodes."""
import numpy as np

DONE, LIMIT, BAD_ROOT = 0, 1, 2

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


def dive(text, root_row, objective="ANY", max_nodes=1 << 62):
    """-> dict(status, root_props, nodes, cuts, props, solutions, first): first = the first solution found (int32 [n]) or
    None"""
    assert objective in ("ANY", "ALL") and max_nodes > 0
    orc, dom = oracle_for(text)
    row = np.ascontiguousarray(root_row, dtype=np.int32)
    out = dict(status=DONE, root_props=0, nodes=0, cuts=0, props=0, solutions=0, first=None)
    if (row[:, 0] > row[:, 1]).any() or (row[:, 0] < dom[:, 0]).any() or (row[:, 1] > dom[:, 1]).any():
        out["status"] = BAD_ROOT
        return out
    status, cur = orc.instance(row, -1, 0, 0)
    if status < 0:
        return out
    out["root_props"] = status
    if (cur[:, 0] == cur[:, 1]).all():
        out["solutions"] = 1
        out["first"] = cur[:, 0].copy()
        return out

    def branch(state):
        width = (state[:, 1] - state[:, 0]).astype(np.int64)
        width[width == 0] = 1 << 40
        v = int(np.argmin(width))
        return v, int(state[v, 0])

    stack = []  # (state, variable, next value) of the nodes that come back
    v, nv = branch(cur)
    while True:
        if out["nodes"] >= max_nodes:
            out["status"] = LIMIT
            break
        value, last = nv, nv == cur[v, 1]
        status, child = orc.instance(cur, v, value, value)
        out["nodes"] += 1
        descend = False
        if status < 0:
            out["cuts"] += 1
        else:
            out["props"] += status
            if (child[:, 0] == child[:, 1]).all():
                out["solutions"] += 1
                if out["first"] is None:
                    out["first"] = child[:, 0].copy()
                if objective == "ANY":
                    break
            else:
                descend = True
        if descend:
            if not last:
                stack.append((cur, v, value + 1))
            cur = child
            v, nv = branch(cur)
        elif last:
            if not stack:
                break
            cur, v, nv = stack.pop()
        else:
            nv = value + 1
    return out


def dive_many(text, roots, objective="ANY", max_nodes=1 << 62):
    """dive() of every row -> dict of arrays shaped like Model.solve_many's answer (first: zeros where there is none);
    equal rows are walked once"""
    roots = np.ascontiguousarray(roots, dtype=np.int32)
    K, n = roots.shape[0], roots.shape[1]
    res = {k: np.zeros(K, dtype=np.int64) for k in ("status", "root_props", "nodes", "cuts", "props", "solutions")}
    res["first"] = np.zeros((K, n), dtype=np.int32)
    seen = {}
    for i in range(K):
        key = roots[i].tobytes()
        if key not in seen:
            seen[key] = dive(text, roots[i], objective, max_nodes)
        d = seen[key]
        for k in ("status", "root_props", "nodes", "cuts", "props", "solutions"):
            res[k][i] = d[k]
        if d["first"] is not None:
            res["first"][i] = d["first"]
    return res
