"""The instance sets of the solve_many_clauses_wide tests past 512 clauses (a helper module, no test itself): a model
text, its root rows, the objective and the budget.  Kernel 6 cannot run these models, so the expected values are the
host walk's (tests/many_walk_objective.py, the specification), computed once per (set, objective) and shared.

  sudoku_less    problems.sudoku_less(3, 5, 24): 81 variables, 1,159 clauses.  Twelve rows that reveal 15 to 40 % of the
                 grid, three of them with one given moved to another value of its root domain.  ANY and ALL, 400 nodes:
                 the rows of 15 and 20 % reach the budget under ANY, a moved given makes a row inconsistent at its root
  schedule32     problems.schedule(32, 1): 98 variables, 657 clauses, MIN, 200 nodes.  Row 0 is the root domains (LIMIT
                 with one solution, makespan 114); the others fix most starts to that solution's and give `end` a
                 deadline a few values above 114 -- without one every value above the incumbent is one more cut child --
                 so that they prove their optimum inside the budget
  tree630        a tests/tree_sets.py model of 150 variables and 631 clauses, expression trees among them, eight windows of
                 at most three values around the planted point: ALL, and the model's own MAX of a sum of four variables,
                 100 nodes (some rows finish, some do not)

The rows, the shares and the budgets were chosen on the host with many_walk_objective alone;
test_solve_many_clauses_wide_host.py re-checks every outcome class the sets are chosen for."""
import functools

import numpy as np

import many_clause_sets as sets
import many_walk_objective as W
import tree_sets
from csolve_amd import problems

SUDOKU = (3, 5, 24)  # box, seed of the grid, inequalities
# the share of the grid a row reveals (row k's cells are its own seeded choice, so the order is free): the 15 % rows are
# the ones whose ANY walk is longer than the budget
SHARES = (0.40, 0.35, 0.30, 0.25, 0.20, 0.15, 0.15, 0.20, 0.25, 0.30, 0.35, 0.15)
MOVED = (0, 3, 9)    # rows with one given moved
TREE_OBJECTIVE = "MAX C1 + C2 + C4 + C6"


@functools.lru_cache(maxsize=None)
def sudoku_less():
    """-> (text, rows [12, 81, 2] int32 inside the root domains)"""
    box, seed, pairs = SUDOKU
    text = problems.sudoku_less(box, seed, pairs)
    _, dom = W.oracle_for(text)
    _, rows = problems.sudoku_less_roots(box, seed, pairs, SHARES, dom=dom)
    grid = np.array(problems.sudoku_solution(box, seed)).reshape(-1)
    assert ((grid >= dom[:, 0]) & (grid <= dom[:, 1])).all()  # the grid is a solution of the model
    for k in MOVED:
        given = [v for v in range(len(grid)) if rows[k, v, 0] == rows[k, v, 1] and dom[v, 0] != dom[v, 1]]
        rng = problems.LCG(77 + k)
        v = given[rng.below(len(given))]
        others = [x for x in range(dom[v, 0], dom[v, 1] + 1) if x != grid[v]]
        rows[k, v] = others[rng.below(len(others))]
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    rows.setflags(write=False)
    return text, rows


@functools.lru_cache(maxsize=None)
def schedule32():
    """-> (text, rows [10, 98, 2] int32)"""
    text = problems.schedule(32, 1)
    _, dom = W.oracle_for(text)
    names = W.model_of(text).names()
    found = W.walk(text, dom, "MIN", 200)
    assert found["solutions"] == 1 and found["best"] == 114
    starts = [v for v, s in enumerate(names) if s.endswith("_start")]
    end = names.index("end")
    rows = [dom.copy()]
    for k, keep in enumerate((28, 29, 30, 26, 27, 24, 31, 20, 12)):
        order = problems.LCG(1000 + k).shuffle(list(starts))
        row = dom.copy()
        row[end, 1] = min(int(dom[end, 1]), 114 + 6 + k)
        for v in order[:keep]:
            row[v] = found["first"][v]
        rows.append(row)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    rows.setflags(write=False)
    return text, rows


@functools.lru_cache(maxsize=None)
def tree630(objective):
    """-> (text, rows [8, n, 2] int32); objective: "ALL" or TREE_OBJECTIVE (one more variable, "<obj>")"""
    text, preds, _ = tree_sets.generate(n=150, seed=13, shapes=tree_sets.FAMILIES, clauses=330, plain=45, slack=3,
                                        objective=objective)
    rows = np.ascontiguousarray(sets.tree_windows(text, preds.planted, 8, 9, 3), dtype=np.int32)
    rows.setflags(write=False)
    return text, rows


# name -> (builder of (text, rows), the objective the walk runs under, max_nodes)
CASES = {
    "sudoku_less_any": (sudoku_less, "ANY", 400),
    "sudoku_less_all": (sudoku_less, "ALL", 400),
    "schedule32_min": (schedule32, "MIN", 200),
    "tree630_all": (lambda: tree630("ALL"), "ALL", 100),
    "tree630_max": (lambda: tree630(TREE_OBJECTIVE), "MAX", 100),
}


def build(name):
    """-> (text, rows, objective, max_nodes)"""
    make, objective, budget = CASES[name]
    text, rows = make()
    return text, rows, objective, budget


@functools.lru_cache(maxsize=None)
def walked(name):
    """the host walk of every row of a case at its budget (computed once, shared by the tests, not to be changed)"""
    text, rows, objective, budget = build(name)
    res = W.walk_many(text, rows, objective, budget)
    for a in res.values():
        a.setflags(write=False)
    return res


def host_model(text):
    """the product's model of `text` with its host tables built from the oracle's root domains (no device call)"""
    from csolve_amd.solver import Model
    m = Model.from_text(text)
    m.set_domains(W.oracle_for(text)[1])
    return m.normalize().build_tables()
