"""The instance sets of the solve_many(branching="allowed") tests (a helper module like many_sets.py, no test itself): one
model text, its root rows, the objective, k (None: the plain call; an int: solve_many_upto), the budget the tests pass and
the cs_dive_allowed instantiation the model plans (its cs_dive_allowed_upto one has the same arguments).  Budgets were
chosen on the host with many_walk_allowed alone: `largest` is the largest tree (nodes) of the set by that walk,
test_solve_many_allowed_host.py re-checks it, and every budget lies above it -- no instance of these sets ends in LIMIT.

The shapes are the smallest that reach every instantiation (table entries of 8 / 16 bits, 1 / 2 / 4 variables per lane,
1 / 4 set words) and every branch of the walk: three slots per pair (queens), roots that are inconsistent or valued
already (queens12_two), the three sudoku sets whose node counts the feature was proposed with, and models whose root
domains need more than one set word (33 .. 128 values)."""
import numpy as np

import many_sets
from csolve_amd import problems


def _sparse(n, width, lo_spread, seed):
    """a sparse != network of n variables, all but three given: `width` values (<= 32: one set word, more: four), lower
    bounds up to lo_spread apart (0: 8-bit table entries, 2000: 16-bit ones)"""
    text = problems.sparse_ne(n, 3, width, 1, per_pair=1, offset_spread=4, lo_spread=lo_spread, pinned=n - 3, objective="ALL")
    return text, many_sets.narrowed(text, 8, seed, 2, 8)


def _wide20(count=12, free=4, window=12):
    """20 variables of 96 values (three of the four set words in use): a row is one solution of the model with `free`
    seeded variables opened to a window of `window` values around theirs, anywhere in the 96 -- the valued neighbours
    forbid values INSIDE those windows"""
    import many_walk
    text = problems.offsets(20, 96, 1, "ALL")
    _, dom = many_walk.oracle_for(text)
    start = dom.copy()  # the first solution with variable v at least 31 (v mod 3) above its lower bound: the windows
    start[:, 0] += 31 * (np.arange(dom.shape[0]) % 3)  # then lie in, and across, the first three set words
    solution = many_walk.dive(text, start, "ANY", 1 << 20)["first"]
    rng = problems.LCG(96 * 20 + count)
    rows = np.repeat(np.stack([solution, solution], 1)[None], count, 0).astype(np.int32)
    for k in range(count):
        for v in rng.shuffle(list(range(dom.shape[0])))[:free]:
            lo = max(int(dom[v, 0]), int(solution[v]) - rng.below(window))
            rows[k, v] = (lo, min(int(dom[v, 1]), lo + window - 1))
    return text, rows


def _queens8():
    return problems.queens(8, "ALL"), np.array([[[1, 8]] * 8], dtype=np.int32)


K = "cs_dive_allowed<unsigned %s, %d, %d>"
# name -> (builder of (text, roots), objective, k, max_nodes, kernel, largest tree of the set by many_walk_allowed)
SETS = {
    "queens8_all": (_queens8, "ALL", None, 1 << 12, K % ("char", 1, 1), 662),
    "queens12_two": (many_sets.SETS["queens12_two"][0], "ALL", None, 1 << 16, K % ("char", 1, 1), 2604),
    "sudoku9_30_any": (lambda: problems.sudoku_roots(3, 0.30, list(range(1, 33))), "ANY", None, 512, K % ("char", 2, 1), 76),
    "sudoku9_40_all": (lambda: problems.sudoku_roots(3, 0.40, list(range(1, 33)), "ALL"), "ALL", None, 1 << 12,
                       K % ("char", 2, 1), 384),
    "sudoku9_25_upto2": (lambda: problems.sudoku_roots(3, 0.25, list(range(1, 17)), "ALL"), "ALL", 2, 1 << 12,
                         K % ("char", 2, 1), 3482),
    "sudoku16_any": (many_sets.SETS["sudoku16_any"][0], "ANY", None, 256, K % ("char", 4, 1), 11),
    "sparse40_e16": (many_sets.SETS["sparse40_e16"][0], "ALL", None, 1 << 17, K % ("short", 1, 4), 61034),
    "sparse100_e16": (many_sets.SETS["sparse100_e16"][0], "ALL", None, 1 << 17, K % ("short", 2, 4), 61194),
    "sparse150_e16": (many_sets.SETS["sparse150_e16"][0], "ALL", None, 1 << 17, K % ("short", 4, 4), 61192),
    "sparse40_e16_w16": (lambda: _sparse(40, 16, 2000, 11), "ALL", None, 1 << 14, K % ("short", 1, 1), 1840),
    "sparse100_e16_w16": (lambda: _sparse(100, 16, 2000, 12), "ALL", None, 1 << 14, K % ("short", 2, 1), 1851),
    "sparse150_e16_w16": (lambda: _sparse(150, 16, 2000, 13), "ALL", None, 1 << 14, K % ("short", 4, 1), 3733),
    "sparse100_e8_w40": (lambda: _sparse(100, 40, 0, 14), "ALL", None, 1 << 17, K % ("char", 2, 4), 61194),
    "sparse150_e8_w40": (lambda: _sparse(150, 40, 0, 15), "ALL", None, 1 << 17, K % ("char", 4, 4), 61192),
    "wide20_w96": (_wide20, "ALL", None, 1 << 17, K % ("char", 1, 4), 14657),
}
del K
# the ALL sets on which the SETS of solution rows are compared with the width walk's (host test)
ROW_SETS = ("queens8_all", "sudoku9_40_all")


def build(name):
    """-> (text, roots [K, n, 2] int32, objective, k, max_nodes)"""
    make, objective, k, budget, _, _ = SETS[name]
    text, roots = make()
    return text, np.ascontiguousarray(roots, dtype=np.int32), objective, k, budget


def upto_kernel(name):
    return SETS[name][4].replace("cs_dive_allowed<", "cs_dive_allowed_upto<")
