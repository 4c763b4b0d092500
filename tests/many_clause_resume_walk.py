"""The stop-and-go host walk of checkpointed Model.solve_many_clauses / Model.resume_many_clauses (a helper module of
test_many_clauses_resume_host.py and test_gpu_many_clauses_resume.py, no test itself): many_walk_objective.Walk, whose
run(budget) already continues a stopped walk, over the sets of many_clause_sets.py in the slices the tests use.

slices(name)     1, 7, 56 and the rest of the set's budget
Tracked          the walk that also remembers its deepest stack (Walk.stack: the pushed frames, without the current node)
sliced(name)     every instance of a set walked in those slices, once: the answers after each slice in walk_many's form,
                 the open subtrees and the incumbent of every instance where it stood at LIMIT, the deepest stack
finished6()      schedule6_min_budget walked on to 256 + 32,768 nodes, where every instance is DONE: the proven optima"""
import functools

import numpy as np

import many_clause_sets as sets
import many_walk
import many_walk_objective as W

DONE, LIMIT = W.DONE, W.LIMIT
FINISH6 = (256, 32768)


def slices(name):
    budget = sets.SETS[name][2]
    assert budget > 64
    return (1, 7, 56, budget - 64)


class Tracked(W.Walk):
    deepest = 0

    def _branch(self, state):  # called whenever a node is entered, after its parent was pushed
        self.deepest = max(self.deepest, len(self.stack))
        return many_walk.Walk._branch(state)


def gather(results, n):
    res = many_walk.gather(results, n)
    res["best"] = np.array([0 if d["best"] is None else d["best"] for d in results], dtype=np.int64)
    return res


def _walk_in(text, roots, objective, budgets):
    """-> (answers after each budget, per budget {instance: (open subtrees, incumbent or None)} of the instances at LIMIT,
    the deepest stack of any instance)"""
    walks = [Tracked(text, row, objective) for row in roots]
    after, stopped = [], []
    for b in budgets:
        results = [w.run(b) for w in walks]
        after.append(gather(results, roots.shape[1]))
        stopped.append({i: (w.open_subtrees(), w.best) for i, w in enumerate(walks) if results[i]["status"] == LIMIT})
        for a in after[-1].values():
            a.setflags(write=False)
    return after, stopped, max(w.deepest for w in walks)


@functools.lru_cache(maxsize=None)
def sliced(name):
    """(computed once, shared by the tests, not to be changed)"""
    text, roots, objective, _ = sets.build(name)
    return _walk_in(text, roots, objective, slices(name))


@functools.lru_cache(maxsize=None)
def finished6():
    text, roots, objective, budget = sets.build("schedule6_min_budget")
    assert budget == FINISH6[0]
    return _walk_in(text, roots, objective, FINISH6)
