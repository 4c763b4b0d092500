"""The instance sets of the solve_many_clauses tests (a helper module, no test itself): one model text, its root rows, the
objective, the budget the tests pass, the cs_walk_clauses instantiation the model plans and whether the set is "whole".

Rows are windows around one solution of the model: the first solution of the ANY walk from the root domains (the planted
point of a tree_sets model), and for every selected open variable a seeded interval of at most `width` values that holds
the solution's value, cut to the root domain.  Every row therefore has a solution and a tree whose size the width sets.
Widths, seeds and budgets were chosen on the host with many_walk_objective alone:

  whole sets    every instance ends DONE below the budget, the largest tree has at most 20,000 nodes, at most 64 rows
  budget sets   MIN with a budget of at most 4,096 that some instances reach: they are compared AT the budget, with the
                best found so far and its row

test_solve_many_clauses_host.py re-checks these conditions; together the sets plan all eight instantiations, CPL 1 / 2 /
4 / 8 with and without a tree clause (the clause count of the tables is the model's: the objective's constant and the
bound clauses count)."""
import functools
import os

import numpy as np

import many_walk_objective as W
import tree_sets
from csolve_amd import problems

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "problems")


def windows(text, count, seed, width, select=None, centre=None, anywhere=False):
    """`count` rows inside the root domains of `text`: every open variable whose name `select` accepts (default: all but
    the objective variable) is cut to a seeded window of 1 .. width values around `centre` (default: the first solution
    of the ANY walk from the root domains); where select(name) is a number above 1, that is the variable's width.
    anywhere: the windows lie anywhere in the root domains instead (such a row need not have a solution), and a numbered
    variable keeps its lower bound: the number is then an upper bound on its width, e.g. a deadline"""
    _, dom = W.oracle_for(text)
    om = W.model_of(text)
    names = om.names()
    if centre is None and not anywhere:
        first = W.walk(text, dom, "ANY", 1 << 20)
        assert first["solutions"] == 1, "no solution within 2^20 nodes"
        centre = first["first"]
    rng = problems.LCG(seed * 2654435761 + count)
    rows = np.repeat(dom[None], count, 0).astype(np.int32)
    for k in range(count):
        for v in range(dom.shape[0]):
            if dom[v, 0] == dom[v, 1] or (v == om.view.obj_var if select is None else not select(names[v])):
                continue
            own = select(names[v]) if select is not None else True
            w = 1 + rng.below(width if own is True else int(own))
            if anywhere:
                full = int(dom[v, 1]) - int(dom[v, 0]) + 1
                w = int(own) if own is not True else min(w, full)
                lo = int(dom[v, 0]) + (0 if own is not True else rng.below(full - w + 1))
            else:
                lo = max(int(dom[v, 0]), int(centre[v]) - rng.below(w))
            rows[k, v] = (lo, min(int(dom[v, 1]), lo + w - 1))
    return rows


def _tree(objective, **kw):
    """a tree_sets model and its planted point in the model's variable order"""
    text, preds, _ = tree_sets.generate(objective=objective, **kw)
    return text, preds.planted


def tree_windows(text, planted, count, seed, width):
    import search_sets
    om = W.model_of(text)
    centre = np.zeros(om.n_vars, dtype=np.int64)
    for i, c in enumerate(search_sets.columns(om.names())):
        centre[c] = planted[i]
    return windows(text, count, seed, width, centre=centre)


def _starts(deadline):
    """windows for the start times of a schedule() model and at most `deadline` values for `end`, its objective variable
    (another deadline per row; without an upper bound of its own every value above the incumbent is one more cut child)"""
    return lambda name: name.endswith("_start") or (deadline if name == "end" else False)


def _wcet():
    return open(os.path.join(GOLDEN, "ref_wcet.txt")).read()


def _mixed(name, objective):
    return tree_sets.generate_set(name, objective)[0], tree_sets.generate_set(name, objective)[1].planted


def _tree_set(objective, count, rows_seed, width, name=None, **kw):
    text, planted = _mixed(name, objective) if name else _tree(objective, **kw)
    return text, tree_windows(text, planted, count, rows_seed, width)


# name -> (builder of (text, roots), objective, max_nodes, kernel, whole)
SETS = {
    "linear12_any": (lambda: (problems.linear(12, 1, "ANY"), windows(problems.linear(12, 1, "ANY"), 32, 1, 12)), "ANY", 4096,
                     "cs_walk_clauses<1, false>", True),
    "linear20_all": (lambda: (problems.linear(20, 3, "ALL"), windows(problems.linear(20, 3, "ALL"), 24, 2, 3)), "ALL", 1 << 15,
                     "cs_walk_clauses<2, false>", True),
    "linear40_all": (lambda: (problems.linear(40, 2, "ALL"), windows(problems.linear(40, 2, "ALL"), 16, 3, 2)), "ALL", 1 << 15,
                     "cs_walk_clauses<4, false>", True),
    "schedule5_min": (lambda: (problems.schedule(5, 1), windows(problems.schedule(5, 1), 32, 4, 30, _starts(40))), "MIN", 1 << 15,
                      "cs_walk_clauses<1, false>", True),
    "wcet_max": (lambda: (_wcet(), windows(_wcet(), 24, 5, 8)), "MAX", 1 << 15, "cs_walk_clauses<1, true>", True),
    "tree20_all": (lambda: _tree_set("ALL", 24, 6, 3, n=20, seed=14, shapes=tree_sets.FAMILIES, clauses=40, plain=40, slack=3),
                   "ALL", 1 << 15, "cs_walk_clauses<2, true>", True),
    "mixed40_any": (lambda: _tree_set("ANY", 16, 7, 4, name="mixed40"), "ANY", 1 << 15, "cs_walk_clauses<4, true>", True),
    "mixed120_any": (lambda: _tree_set("ANY", 8, 8, 3, name="mixed120"), "ANY", 1 << 15, "cs_walk_clauses<8, true>", True),
    "schedule6_min_budget": (lambda: (problems.schedule(6, 1), windows(problems.schedule(6, 1), 24, 4, 30, _starts(40))), "MIN",
                             256, "cs_walk_clauses<1, false>", False),
    "schedule22_min_budget": (lambda: (problems.schedule(22, 1), windows(problems.schedule(22, 1), 8, 4, 12, _starts(60))), "MIN",
                              100, "cs_walk_clauses<8, false>", False),
}
WHOLE = [k for k, s in SETS.items() if s[4]]
BUDGET = [k for k, s in SETS.items() if not s[4]]


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (text, roots [K, n, 2] int32, objective, max_nodes)"""
    make, objective, budget, _, _ = SETS[name]
    text, roots = make()
    roots = np.ascontiguousarray(roots, dtype=np.int32)
    roots.setflags(write=False)
    return text, roots, objective, budget


@functools.lru_cache(maxsize=None)
def walked(name):
    """the oracle walk of every instance of a set at its budget (computed once, shared by the tests, not to be changed)"""
    text, roots, objective, budget = build(name)
    res = W.walk_many(text, roots, objective, budget)
    for a in res.values():
        a.setflags(write=False)
    return res


def planned(text):
    """the instantiation the tables of `text` plan: clauses per lane from the model's clause count, a tree from the
    clauses the linear fast paths do not take (host only: the oracle's root domains, the normaliser,
    csgpu_model_build_tables)"""
    from csolve_amd.solver import Model
    m = Model.from_text(text)
    m.set_domains(W.oracle_for(text)[1])
    info = m.normalize().build_tables().device_info()
    per = (m.n_clauses + 63) // 64
    cpl = 1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8
    return f"cs_walk_clauses<{cpl}, {'true' if info['tree_clauses'] else 'false'}>"
