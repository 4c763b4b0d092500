"""What Model.solve_many_clauses_upto is specified to compute (include/csolve_gpu.h), on the host with the oracle for every
node (a helper module of test_solve_many_clauses_upto_host.py and test_gpu_solve_many_clauses_upto.py, no test itself).

Walk(text, root_row) is many_walk_objective.Walk built under "ALL" -- the clause model normalised as the product's tables
are, "<obj>" an ordinary variable, no incumbent -- with many_walk.Walk's run(budget, stop_at) and result(): the walk
leaves right after solution number `stop_at` and keeps every solution in walk order (`rows`; the objective walk's own
result() drops them).  A walk that already holds `stop_at` solutions when it is continued ends DONE before it tries a
node, its counters as they were.  props are the oracle's, which kernel 6 does not promise: the GPU tests compare props
with kernel 6 itself, node by node."""
import numpy as np

import many_walk
import many_walk_objective as W
from many_walk import BAD_ROOT, DONE, LIMIT  # noqa: F401

FIELDS = W.FIELDS  # status, nodes, cuts, solutions: what the device must equal


class Walk(W.Walk):
    def __init__(self, text, root_row):
        super().__init__(text, root_row, "ALL")

    run = many_walk.Walk.run
    result = many_walk.Walk.result


def walk_upto(text, root_row, k, max_nodes=1 << 62):
    """-> dict(status, root_props, nodes, cuts, props, solutions, rows): rows = the solutions found, in walk order (a list
    of int32 [n], at most k)"""
    assert k >= 1
    return Walk(text, root_row).run(max_nodes, k)


def walk_sliced(text, root_row, slices):
    """the walk in slices [(budget, k), ...] -> the result after the last one"""
    w = Walk(text, root_row)
    out = w.result()
    for budget, k in slices:
        out = w.run(budget, k)
    return out


def walk_many_upto(text, roots, k, max_nodes=1 << 62, slices=None):
    """walk_upto() of every row -> dict of arrays shaped like Model.solve_many_clauses_upto's answer (rows [K, k, n]: zeros
    where there is none); slices=[(budget, k), ...] walks every row in those slices instead (rows [K, max k, n]).  Equal
    rows are walked once."""
    results = many_walk.walk_each(
        roots, lambda row, _: walk_upto(text, row, k, max_nodes) if slices is None else walk_sliced(text, row, slices))
    width = k if slices is None else max(kk for _, kk in slices)
    return many_walk.gather(results, np.shape(roots)[1], fields=many_walk.FIELDS, width=width)
