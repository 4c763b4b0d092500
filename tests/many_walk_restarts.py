"""What Model.solve_many_restarts is specified to compute, on the host with the oracle for every node (a helper module of
test_solve_many_restarts_host.py and test_gpu_solve_many_restarts.py, no test itself).  Written from the definition in
include/csolve_gpu.h; the value function is restated here and not taken from the library, which is compared with it.

The walk is many_walk.dive under ANY with two changes.  A node that branches on variable v with [lo, hi] tries
value(j) = lo + ((start + j) mod width), j = 0 .. width - 1, with start = 0 in run 0 (unless rotate_first) and else the
high word of key x width, key = fmix32(seed ^ fmix32(run x 0x9E3779B1 + v + 1)) in wrapping 32 bits; a frame holds
(node, v, next j).  After a failed child, unless it was the last value of a node with no frame left (the tree is
exhausted: DONE, proven), and when restart_base > 0: fails += 1, and fails > threshold x restart_base starts the walk
again from the root node's fixpoint with run + 1, the next Luby threshold and fails = 0.  A restart costs no node;
nodes / cuts / props and the budget run over all runs; the budget is compared before a child is tried."""
import numpy as np

import many_walk
from many_walk import BAD_ROOT, DONE, FIELDS, LIMIT  # noqa: F401

M32 = 0xffffffff
ROTATE_FIRST = 1


def fmix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def start_of(seed, run, var, width, flags=0):
    if run == 0 and not flags & ROTATE_FIRST:
        return 0
    key = fmix32((seed & M32) ^ fmix32((run * 0x9E3779B1 + var + 1) & M32))
    return (key * width) >> 32


def value(seed, run, var, lo, hi, j, flags=0):
    """the value a node that branches on `var` with [lo, hi] tries j-th"""
    width = hi - lo + 1
    return lo + (start_of(seed, run, var, width, flags) + j) % width


def luby_next(threshold, counter):
    """fail_threshold_next of the reference: 1 1 2 1 1 2 4 ..."""
    if counter & -counter == threshold:
        return 1, counter + 1
    return threshold << 1, counter


def dive_restarts(text, row, restart_base, seed, rotate_first=False, max_nodes=1 << 62):
    """-> dict(status, root_props, nodes, cuts, props, solutions, restarts, first)"""
    assert restart_base >= 0 and max_nodes > 0
    orc, dom = many_walk.oracle_for(text)
    row = np.ascontiguousarray(row, dtype=np.int32)
    flags = ROTATE_FIRST if rotate_first else 0
    out = dict(status=DONE, root_props=0, nodes=0, cuts=0, props=0, solutions=0, restarts=0, first=None)
    if (row[:, 0] > row[:, 1]).any() or (row[:, 0] < dom[:, 0]).any() or (row[:, 1] > dom[:, 1]).any():
        out["status"] = BAD_ROOT
        return out
    status, root = orc.instance(row, -1, 0, 0)
    if status < 0:
        return out
    out["root_props"] = status
    if (root[:, 0] == root[:, 1]).all():
        out["solutions"] = 1
        out["first"] = root[:, 0].copy()
        return out

    def branch(state):
        width = (state[:, 1] - state[:, 0]).astype(np.int64)
        width[width == 0] = 1 << 40
        return int(np.argmin(width))

    run, fails, threshold, counter = 0, 0, 1, 1
    cur, stack = root, []  # stack: (node, variable, next j) of the nodes that come back
    v, j = branch(cur), 0
    while True:
        if out["nodes"] >= max_nodes:
            out["status"] = LIMIT
            break
        lo, hi = int(cur[v, 0]), int(cur[v, 1])
        last = j == hi - lo
        val = value(seed, run, v, lo, hi, j, flags)
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
            v, j = branch(cur), 0
            continue
        out["cuts"] += 1
        if last and not stack:
            break  # this run has walked the whole tree
        if restart_base > 0:
            fails += 1
            if fails > ((threshold * restart_base) & 0xffffffffffffffff):
                fails = 0
                threshold, counter = luby_next(threshold, counter)
                run += 1
                out["restarts"] += 1
                cur, stack = root, []
                v, j = branch(cur), 0
                continue
        if last:
            cur, v, j = stack.pop()
        else:
            j += 1
    return out


def dive_many_restarts(text, roots, restart_base, seed=0, seeds=None, rotate_first=False, max_nodes=1 << 62):
    """dive_restarts() of every row (seeds[i], or `seed` for all) -> dict of arrays shaped like
    Model.solve_many_restarts's answer (first: zeros where there is none); equal (row, seed) pairs are walked once"""
    tags = [int(seeds[i]) & M32 if seeds is not None else int(seed) & M32 for i in range(len(roots))]
    results = many_walk.walk_each(roots, lambda row, s: dive_restarts(text, row, restart_base, s, rotate_first, max_nodes), tags)
    return many_walk.gather(results, np.shape(roots)[1], FIELDS + ("restarts",))
