"""The stop-and-go host walk of checkpointed Model.solve_many_clauses_ordered / Model.resume_many_clauses (a helper module
of test_solve_many_clauses_ordered_resume_host.py and test_gpu_solve_many_clauses_ordered_resume.py, no test itself):
many_walk_ordered.Walk, whose run(budget) already continues a stopped walk and keeps `halvings`, over the cases of
many_walk_ordered.CASES in the slices the tests use, and over four ALL rows whose stacks grow past n_vars.

slices(name)          1, 7, 56 and the rest of the set's budget
sliced(name, o, s)    every instance of a case walked in those slices, once: the answers after each slice in walk_many's
                      form (with halvings), and per slice what every instance at LIMIT left: its open subtrees, its
                      incumbent, its frames in use (the current node counted), whether it stands between the two halves
                      of its current node, and its pushed halving parents
ALL_ROWS              (set of order_walk, order, split_width): the root-domain row of the set under ALL
all_row(name, o, s)   -> (text, roots [1, n, 2], whole walk)
stopped_all(...)      that row after a cumulative budget: (answer so far, open subtrees, frames in use)"""
import functools

import numpy as np

import many_walk
import many_walk_ordered as O
import order_walk

DONE, LIMIT = O.DONE, O.LIMIT
FIELDS = many_walk.FIELDS + ("halvings",)
ALL_ROWS = [("wide2_cut", "smallest-domain", 1), ("wide2_cut", "none", 1), ("wide2_cut", "largest-value", 16),
            ("wide3_sums", "none", 4)]
DEEP = ("wide2_cut", "smallest-domain", 1)  # the deep-stack test's row: F = 31 frames for n_vars = 5
ALL_BUDGET = 1 << 15


def slices(name):
    budget = O.SETS[name][2]
    assert budget > 64
    return (1, 7, 56, budget - 64)


def gather(results, n):
    res = many_walk.gather(results, n, FIELDS)
    res["best"] = np.array([0 if d["best"] is None else d["best"] for d in results], dtype=np.int64)
    return res


def halving_parents(walk):
    """the pushed frames of a stopped walk that wait for their second half"""
    return sum(1 for node, v, nv in walk.stack if int(node[v, 1]) - int(node[v, 0]) + 1 > walk.split)


def between_halves(walk):
    """does the stopped walk stand after the first and before the second half of its current node?"""
    lo, hi = int(walk.cur[walk.v, 0]), int(walk.cur[walk.v, 1])
    return hi - lo + 1 > walk.split and walk.nv == ((lo + hi) >> 1) + 1


def left_by(walk):
    return dict(states=walk.open_subtrees(), best=walk.best, frames=len(walk.stack) + 1, between=between_halves(walk),
                parents=halving_parents(walk))


@functools.lru_cache(maxsize=None)
def sliced(name, order, split_width):
    """(computed once, shared by the tests, not to be changed) -> (answers after each slice, per slice {instance: left_by})"""
    text, roots, objective, _ = O.build(name)
    walks = [O.Walk(text, row, objective, order, split_width) for row in roots]
    after, stopped = [], []
    for b in slices(name):
        results = [w.run(b) for w in walks]
        after.append(gather(results, roots.shape[1]))
        stopped.append({i: left_by(w) for i, w in enumerate(walks) if results[i]["status"] == LIMIT})
        for a in after[-1].values():
            a.setflags(write=False)
    return after, stopped


@functools.lru_cache(maxsize=None)
def all_row(name, order, split_width):
    text = order_walk.text_of(name)
    roots = O.root_row(text)
    roots.setflags(write=False)
    return text, roots, O.walk(text, roots[0], "ALL", ALL_BUDGET, order, split_width)


@functools.lru_cache(maxsize=None)
def stopped_all(name, order, split_width, budget):
    text, roots, _ = all_row(name, order, split_width)
    walk = O.Walk(text, roots[0], "ALL", order, split_width)
    res = walk.run(budget)
    assert res["status"] == LIMIT
    return res, walk.open_subtrees(), len(walk.stack) + 1


def solutions_below(text, states, order, split_width):
    """the ALL solutions of the open subtrees, each walked as a root row under the same order and split_width"""
    return sum(O.walk(text, s, "ALL", ALL_BUDGET, order, split_width)["solutions"] for s in states)
