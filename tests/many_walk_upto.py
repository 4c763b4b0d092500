"""What Model.solve_many_upto is specified to compute, on the host with the oracle for every node (a helper module of
test_solve_many_upto_host.py and test_gpu_solve_many_upto.py, no test itself).

dive_upto(text, root_row, k, max_nodes) is many_walk.Walk leaving right after its k-th solution, every solution kept in
walk order (`rows`).  WalkUpto is that walk as an object that stops and goes on: run(budget, k) tries at most `budget`
more children with the k of THIS slice; a walk that already holds k solutions when it is continued ends DONE before it
tries a node, its counters as they were."""
import numpy as np

import many_walk
from many_walk import BAD_ROOT, DONE, FIELDS, LIMIT  # noqa: F401


class WalkUpto(many_walk.Walk):
    def run(self, budget, k):
        assert k >= 1
        return super().run(budget, k)


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


def dive_many_upto(text, roots, k, max_nodes=1 << 62, slices=None):
    """dive_upto() of every row -> dict of arrays shaped like Model.solve_many_upto's answer (rows [K, k, n]: zeros where
    there is none); slices=[(budget, k), ...] walks every row in those slices instead (rows [K, max k, n]).  Equal rows
    are walked once."""
    results = many_walk.walk_each(
        roots, lambda row, _: dive_upto(text, row, k, max_nodes) if slices is None else dive_sliced(text, row, slices))
    width = k if slices is None else max(kk for _, kk in slices)
    if width > 1 << 20:  # "no k" on the host (e.g. 2**40): as many rows as the richest instance has
        width = max([len(d["rows"]) for d in results] + [1])
    return many_walk.gather(results, np.shape(roots)[1], width=width)
