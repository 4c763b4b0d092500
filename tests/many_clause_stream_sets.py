"""The instance sets of the solve_many_clauses_stream tests (a helper module, no test itself): the rows, the
cs_walk_stream instantiation the model plans and the figures of the ALL walk of every row.  Rows come from
many_clause_sets / many_clause_upto_sets, unchanged; a set is cut to the rows whose ALL walk ends within 16,000 nodes.

  set                     rows                            kernel       solutions   largest walk
  linear12_any            5 7 10 12 13 15 18 23 31        <1, false>      55,422   12,186 nodes
  linear20_all            all 24                          <2, false>      19,693   10,209
  linear40_all            all 16                          <4, false>       9,824   12,286
  schedule22_min_budget   0 1 2 3 5 6                     <8, false>       7,220    8,496
  wcet_max                all 24                          <1, true>        3,414    1,561
  tree20_all              all 24                          <2, true>          205       70
  mixed40_any             all 16                          <4, true>          163       63
  mixed120_any            0 2 5 6                         <8, true>        8,704   15,900
  schedule5_classes       all 32                          <1, false>           7       81

In tree20_all instance 19 is a solution at its root node and instance 9 has exactly one; in schedule5_classes 30 rows
have no solution.  All figures were measured on the host walk (many_walk_clauses_upto.Walk(text, row).run(budget, None));
test_solve_many_clauses_stream_host.py re-checks them."""
import functools

import numpy as np

import many_clause_sets as sets
import many_clause_upto_sets as upto_sets
import many_walk_clauses_upto as U

BUDGET = 16000  # every row of every set finishes its ALL walk within it

# name -> (the rows of the set in use, None: all; solutions of all of them; nodes of the largest walk)
TABLE = {
    "linear12_any": ((5, 7, 10, 12, 13, 15, 18, 23, 31), 55422, 12186),
    "linear20_all": (None, 19693, 10209),
    "linear40_all": (None, 9824, 12286),
    "schedule22_min_budget": ((0, 1, 2, 3, 5, 6), 7220, 8496),
    "wcet_max": (None, 3414, 1561),
    "tree20_all": (None, 205, 70),
    "mixed40_any": (None, 163, 63),
    "mixed120_any": ((0, 2, 5, 6), 8704, 15900),
    "schedule5_classes": (None, 7, 81),
}
ROWS = {"linear12_any": 9, "linear20_all": 24, "linear40_all": 16, "schedule22_min_budget": 6, "wcet_max": 24,
        "tree20_all": 24, "mixed40_any": 16, "mixed120_any": 4, "schedule5_classes": 32}
ROOT_SOLUTION = ("tree20_all", 19)  # the root node itself is the one solution
UNIQUE = ("tree20_all", 9)


def kernel(name):
    """the cs_walk_stream instantiation the set's model plans: the set's cs_walk_clauses name, the family replaced"""
    source = upto_sets.SETS[name][3] if name == "schedule5_classes" else sets.SETS[name][3]
    return source.replace("cs_walk_clauses", "cs_walk_stream").replace("cs_walk_upto", "cs_walk_stream")


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (text, roots [K, n, 2] int32): the rows of the set that the table names"""
    text, roots = upto_sets.build(name) if name == "schedule5_classes" else sets.build(name)[:2]
    picked = TABLE[name][0]
    roots = np.ascontiguousarray(roots if picked is None else roots[list(picked)], dtype=np.int32)
    roots.setflags(write=False)
    return text, roots


@functools.lru_cache(maxsize=None)
def walk(name):
    """the unbounded ALL walk of every row of the set on the host: a tuple of result dicts with `rows`, the solutions in
    walk order (computed once, shared by the tests, not to be changed)"""
    text, roots = build(name)
    return tuple(U.Walk(text, row).run(1 << 62, None) for row in roots)
