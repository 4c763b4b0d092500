"""The instance sets of the solve_many_clauses_restarts tests (a helper module, no test itself): one model text, its root
rows, the restart bases the tests pass, the seed (or one seed per instance), the budget, the cs_walk_restart instantiation
the model plans and, per base, what the host walk of many_walk_clauses_restarts gives: the largest walk of the set (nodes
over all runs) and the number of instances that restart.

Conditions, which test_solve_many_clauses_restarts_host.py re-checks on these very rows: at most 64 rows per set; every
budget is at most 8,192 and lies above the largest host walk, so no instance ends LIMIT; every one of the eight
instantiations has a set with at least 4 restarting instances.

Five sets are the rows of many_clause_sets walked under ANY.  Its linear, wcet and tree20 rows never fail a child, so
they cannot restart; the other instantiations have rows of their own here: wider windows around the first solution.
schedule5_unsat is proven unsatisfiable only through restarts: the schedule5_min rows with the upper bound of `end` set
to the row's optimum minus 1 (the optimum of many_walk_objective.walk under MIN).  None of its 32 rows has a solution: 5
are BAD_ROOT (the optimum was the lower bound), 10 fail at the root node, 16 restart; at base 1 the largest walk is 4,020
nodes with 510 restarts, at base 2 3,002 nodes with 254.  walk(name, base) is computed once and shared; nothing writes
to it."""
import functools

import numpy as np

import many_clause_sets as sets
import many_walk_clauses_restarts as R
import many_walk_objective as W
import tree_sets
from csolve_amd import problems

SEED = 12345


def _rows_of(name):
    return sets.build(name)[:2]


def _unsat():
    text, roots = _rows_of("schedule5_min")
    end = W.model_of(text).names().index("end")
    rows = np.array(roots)
    for i, row in enumerate(roots):
        best = W.walk(text, row, "MIN")["best"]
        assert best is not None
        rows[i, end, 1] = best - 1
    return text, rows


def _schedule(tasks, count, width, deadline):
    text = problems.schedule(tasks, 1)
    return text, sets.windows(text, count, 11, width, sets._starts(deadline))


# name -> (builder of (text, roots), bases, seeds (None: SEED for every instance), max_nodes, kernel,
#          {base: (largest walk, restarted instances)})
SETS = {
    "schedule5": (lambda: _rows_of("schedule5_min"), (1, 2), None, 256, "cs_walk_restart<1, false>", {1: (44, 10), 2: (57, 9)}),
    "schedule6": (lambda: _rows_of("schedule6_min_budget"), (1,), None, 1024, "cs_walk_restart<1, false>", {1: (345, 13)}),
    "schedule5_unsat": (_unsat, (1, 2), None, 8192, "cs_walk_restart<1, false>", {1: (4020, 16), 2: (3002, 16)}),
    "schedule12": (lambda: _schedule(12, 16, 20, 40), (2,), None, 1024, "cs_walk_restart<2, false>", {2: (360, 6)}),
    "schedule16": (lambda: _schedule(16, 16, 20, 40), (1,), None, 2048, "cs_walk_restart<4, false>", {1: (623, 9)}),
    "schedule22": (lambda: _rows_of("schedule22_min_budget"), (2,), None, 4096, "cs_walk_restart<8, false>", {2: (1870, 8)}),
    "wcet": (lambda: (sets._wcet(), sets.windows(sets._wcet(), 48, 5, 40)), (1,), None, 1024, "cs_walk_restart<1, true>", {1: (140, 6)}),
    "tree20": (lambda: sets._tree_set("ALL", 24, 6, 16, n=20, seed=14, shapes=tree_sets.FAMILIES, clauses=40, plain=40, slack=3),
               (1, 2), None, 1024, "cs_walk_restart<2, true>", {1: (105, 20), 2: (65, 13)}),
    "mixed40": (lambda: _rows_of("mixed40_any"), (1, 2), None, 1024, "cs_walk_restart<4, true>", {1: (95, 8), 2: (25, 4)}),
    "mixed120": (lambda: _rows_of("mixed120_any"), (1,), None, 1024, "cs_walk_restart<8, true>", {1: (191, 7)}),
}

# The tail the restarts are for (CPU only): 48 rows of three schedule models, windows of `width` values around the first
# solution and at most `deadline` values for `end`, rows seed 11, walk seed 7, no rotate_first, 20,000 nodes per instance.
# name -> (tasks, width, deadline, {base: (nodes in all, deepest walk, instances at the budget)}); base 0 is the ascending
# walk, today's ANY
TAIL_BUDGET, TAIL_SEED, TAIL_BASES = 20000, 7, (1, 2, 4, 8, 16, 32)
TAIL = {
    "schedule8": (8, 30, 40, {0: (26530, 7824, 0), 1: (2481, 477, 0), 2: (2554, 685, 0), 4: (2390, 610, 0), 8: (3217, 1072, 0),
                              16: (4133, 1955, 0), 32: (3689, 1549, 0)}),
    "schedule10": (10, 30, 40, {0: (45183, 20000, 1), 1: (1980, 366, 0), 2: (1279, 168, 0), 4: (1372, 277, 0), 8: (1443, 171, 0),
                                16: (1858, 299, 0), 32: (2368, 542, 0)}),
    "schedule12": (12, 40, 60, {0: (299771, 20000, 11), 1: (14178, 3960, 0), 2: (16353, 5951, 0), 4: (23231, 9862, 0),
                                8: (35828, 17715, 0), 16: (49963, 20000, 1), 32: (60124, 20000, 2)}),
}
DEFAULT_BASE = 1  # the base with the fewest nodes in all over the three: 18,639 (2: 20,186, 4: 26,993, ... 32: 66,181)


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (text, roots [K, n, 2] int32, seeds uint32 [K] or None)"""
    text, roots = SETS[name][0]()
    roots = np.ascontiguousarray(roots, dtype=np.int32)
    roots.setflags(write=False)
    return text, roots, None if SETS[name][2] is None else np.array(SETS[name][2], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def walk(name, base, max_nodes=None, rotate_first=False):
    """the host walk of the whole set under `base` (and the set's budget unless another is given), computed once"""
    text, roots, seeds = build(name)
    res = R.walk_many_restarts(text, roots, base, seed=SEED, seeds=seeds, rotate_first=rotate_first,
                               max_nodes=SETS[name][3] if max_nodes is None else max_nodes)
    for a in res.values():
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def tail_rows(name):
    tasks, width, deadline, _ = TAIL[name]
    text = problems.schedule(tasks, 1)
    return text, sets.windows(text, 48, 11, width, sets._starts(deadline))


@functools.lru_cache(maxsize=None)
def tail_walk(name, base):
    text, roots = tail_rows(name)
    return R.walk_many_restarts(text, roots, base, seed=TAIL_SEED, max_nodes=TAIL_BUDGET)


def planned(text):
    """the cs_walk_restart instantiation the tables of `text` plan (host only)"""
    return sets.planned(text).replace("cs_walk_clauses", "cs_walk_restart")
