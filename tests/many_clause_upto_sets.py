"""The instance sets of the solve_many_clauses_upto tests (a helper module, no test itself): the rows, the k values, the
budget the tests pass and the cs_walk_upto instantiation the model plans.  Rows come from many_clause_sets (build,
windows, _starts), unchanged.

  the eight     the rows of one existing clause set per instantiation, CPL 1 / 2 / 4 / 8 with and without a tree clause,
                walked with k in (2, 5) at budget 4,096.  Every instance ends DONE within 296 nodes but instance 2 of
                schedule22_min_budget, which ends LIMIT at 4,096 nodes with 0 solutions: the "undecided" case.
                tree20_all holds two instances with exactly one solution (9, after 5 nodes; 19, the root node itself);
                at k = 5 wcet_max, tree20_all and mixed40_any hold instances with 1 to 4 solutions, which end as ALL
  schedule5_classes   32 windows anywhere in the root domains of schedule(5, 1), deadlines of at most 12, k = 2: 29 rows
                infeasible at the root, row 13 proven infeasible by search (52 nodes), row 19 unique, row 2 several
  schedule5_slices    the rows of schedule5_min, k = 5, budgets (8, 32, 512): 29 of 32 at LIMIT after the first, 4 after
                the second, none after the third; the largest walk has 296 nodes

All figures were measured on the host walk (many_walk_clauses_upto); test_solve_many_clauses_upto_host.py re-checks them."""
import functools

import many_clause_sets as sets
import many_walk_clauses_upto as U
from csolve_amd import problems

BUDGET = 4096
EIGHT = ("linear12_any", "linear20_all", "linear40_all", "schedule22_min_budget",
         "wcet_max", "tree20_all", "mixed40_any", "mixed120_any")
UNDECIDED = ("schedule22_min_budget", 2)
SLICES = (8, 32, 512)


def _kernel(name):
    return sets.SETS[name][3].replace("cs_walk_clauses", "cs_walk_upto")


def _classes():
    text = problems.schedule(5, 1)
    return text, sets.windows(text, 32, 21, 30, sets._starts(12), anywhere=True)


# name -> (builder of (text, roots), the k values, max_nodes, kernel)
SETS = {name: ((lambda name=name: sets.build(name)[:2]), (2, 5), BUDGET, _kernel(name)) for name in EIGHT}
SETS["schedule5_classes"] = (_classes, (2,), BUDGET, "cs_walk_upto<1, false>")
SETS["schedule5_slices"] = ((lambda: sets.build("schedule5_min")[:2]), (5,), sum(SLICES), "cs_walk_upto<1, false>")


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (text, roots [K, n, 2] int32)"""
    import numpy as np
    text, roots = SETS[name][0]()
    roots = np.ascontiguousarray(roots, dtype=np.int32)
    roots.setflags(write=False)
    return text, roots


@functools.lru_cache(maxsize=None)
def walk(name, k, max_nodes=None):
    """the host walk of every row of a set up to k, at the set's budget unless told another (computed once, shared by the
    tests, not to be changed)"""
    text, roots = build(name)
    res = U.walk_many_upto(text, roots, k, SETS[name][2] if max_nodes is None else max_nodes)
    for a in res.values():
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def sliced(budgets=SLICES, k=5):
    """schedule5_slices walked in slices, stop and go: the answers after each budget (rows [K, k, n]) and, per budget,
    {instance: open subtrees} of the instances that stand at LIMIT"""
    import many_walk
    text, roots = build("schedule5_slices")
    walks = [U.Walk(text, row) for row in roots]
    after, stopped = [], []
    for b in budgets:
        results = [w.run(b, k) for w in walks]
        after.append(many_walk.gather(results, roots.shape[1], fields=many_walk.FIELDS, width=k))
        stopped.append({i: w.open_subtrees() for i, w in enumerate(walks) if results[i]["status"] == U.LIMIT})
        for a in after[-1].values():
            a.setflags(write=False)
    return after, stopped
