"""What Model.solve_many_clauses_restarts is specified to compute, on the host with the oracle for every node (a helper
module of test_solve_many_clauses_restarts_host.py and test_gpu_solve_many_clauses_restarts.py, no test itself).  Written
from the definition in include/csolve_gpu.h; the value function and the Luby step are many_walk_restarts's restatements.

The walk is many_walk_objective.walk under ANY -- the clause model as the product's tables hold it, "<obj>" an ordinary
variable, no incumbent -- with the two changes of many_walk_restarts.dive_restarts.  A node that branches on variable v
with [lo, hi] tries value(seed, run, v, lo, hi, j) for j = 0 .. hi - lo; a frame holds (node, v, next j); `last` is
j == hi - lo of the node as it was entered.  After a failed child, unless it was the last value of a node with no frame
pushed (the tree is exhausted: DONE, proven), and when restart_base > 0: fails += 1, and fails > threshold x restart_base
starts the walk again from the root node's fixpoint with run + 1, the next Luby threshold and fails = 0.  A restart costs
no node and no rounds; root_props is counted once; nodes / cuts / props and the budget run over all runs; the budget is
compared before a child is tried.

props are the oracle's, which kernel 6 does not promise: step(orc=...) takes another source of nodes, and the GPU tests
pass kernel 6 itself."""
import numpy as np

import many_walk
import many_walk_objective as W
from many_walk import BAD_ROOT, DONE, FIELDS, LIMIT  # noqa: F401
from many_walk_restarts import ROTATE_FIRST, luby_next, value

M32 = 0xffffffff
M64 = 0xffffffffffffffff


def _branch(state):
    width = (state[:, 1] - state[:, 0]).astype(np.int64)
    width[width == 0] = 1 << 40
    return int(np.argmin(width))


def walk_restarts(text, row, restart_base, seed, rotate_first=False, max_nodes=1 << 62, orc=None):
    """-> dict(status, root_props, nodes, cuts, props, solutions, restarts, first); orc: another source of nodes than the
    oracle (anything with Oracle.instance's signature)"""
    assert restart_base >= 0 and max_nodes > 0
    oracle, dom = W.oracle_for(text)
    orc = oracle if orc is None else orc
    row = np.ascontiguousarray(row, dtype=np.int32)
    flags = ROTATE_FIRST if rotate_first else 0
    out = dict(status=DONE, root_props=0, nodes=0, cuts=0, props=0, solutions=0, restarts=0, first=None)
    if (row[:, 0] > row[:, 1]).any() or (row[:, 0] < dom[:, 0]).any() or (row[:, 1] > dom[:, 1]).any():
        out["status"] = BAD_ROOT
        return out
    status, root = orc.instance(row, -1, 0, 0)
    if status < 0:
        return out  # an inconsistent root: DONE, no node
    out["root_props"] = status
    if (root[:, 0] == root[:, 1]).all():
        out["solutions"] = 1
        out["first"] = root[:, 0].copy()
        return out
    run, fails, threshold, counter = 0, 0, 1, 1
    cur, stack = root, []  # stack: (node, variable, next j) of the nodes that come back
    v, j = _branch(cur), 0
    while True:
        if out["nodes"] >= max_nodes:
            out["status"] = LIMIT
            break
        lo, hi = int(cur[v, 0]), int(cur[v, 1])
        last = j == hi - lo
        val = value(seed & M32, run, v, lo, hi, j, flags)
        status, child = orc.instance(cur, v, val, val)
        out["nodes"] += 1
        if status >= 0:
            out["props"] += status
            if (child[:, 0] == child[:, 1]).all():
                out["solutions"] = 1
                out["first"] = child[:, 0].copy()
                break
            if not last:
                stack.append((cur, v, j + 1))
            cur = child
            v, j = _branch(cur), 0
            continue
        out["cuts"] += 1
        if last and not stack:
            break  # this run has walked the whole tree: proven
        if restart_base > 0:
            fails += 1
            if fails > ((threshold * restart_base) & M64):
                fails = 0
                threshold, counter = luby_next(threshold, counter)
                run += 1
                out["restarts"] += 1
                cur, stack = root, []
                v, j = _branch(cur), 0
                continue
        if last:
            cur, v, j = stack.pop()
        else:
            j += 1
    return out


def walk_many_restarts(text, roots, restart_base, seed=0, seeds=None, rotate_first=False, max_nodes=1 << 62):
    """walk_restarts() of every row (seeds[i], or `seed` for all) -> dict of arrays shaped like
    Model.solve_many_clauses_restarts's answer (first: zeros where there is none); equal (row, seed) pairs are walked once"""
    tags = [int(seeds[i]) & M32 if seeds is not None else int(seed) & M32 for i in range(len(roots))]
    results = many_walk.walk_each(roots, lambda r, s: walk_restarts(text, r, restart_base, s, rotate_first, max_nodes), tags)
    return many_walk.gather(results, np.shape(roots)[1], FIELDS + ("restarts",))
