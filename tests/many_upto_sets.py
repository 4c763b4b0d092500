"""The instance sets of the solve_many_upto tests (a helper module, no test itself): one model text, its root rows, the
values of k the tests pass, the budget, the cs_dive_upto instantiation the model plans and, per k, the largest tree
(nodes) of the set by the host walk of many_walk_upto.  Every budget lies far above it: no instance of these sets may
end in LIMIT, which test_solve_many_upto_host.py asserts for these very rows.  walk(name, k) is computed once and shared
by the tests that need it; nothing writes to it."""
import numpy as np

import many_sets
import many_walk_upto
from csolve_amd import problems


def _sparse(n, seed):
    text = many_sets._sparse16(n, 3)
    return text, many_sets.narrowed(text, 12, seed, 2, 8)


# name -> (builder of (text, roots), the ks, max_nodes, kernel, {k: largest tree of the set})
SETS = {
    "sudoku9": (lambda: problems.sudoku_roots(3, 0.44, list(range(1, 65)), "ALL"), (2, 3), 1 << 12,
                "cs_dive_upto<unsigned char, 2>", {2: 18, 3: 25}),
    "queens12_two": (lambda: (problems.queens(12, "ALL"), many_sets.queens_two(12, 24, 1)), (2, 5), 1 << 14,
                     "cs_dive_upto<unsigned char, 1>", {2: 262, 5: 521}),
    "sudoku16": (lambda: problems.sudoku_roots(4, 0.55, list(range(1, 9)), "ALL"), (2,), 1 << 12,
                 "cs_dive_upto<unsigned char, 4>", {2: 37}),
    "sparse40_e16": (lambda: _sparse(40, 3), (3, 200), 1 << 14, "cs_dive_upto<unsigned short, 1>", {3: 6, 200: 219}),
    "sparse100_e16": (lambda: _sparse(100, 4), (3, 200), 1 << 14, "cs_dive_upto<unsigned short, 2>", {3: 6, 200: 219}),
    "sparse150_e16": (lambda: _sparse(150, 5), (3, 200), 1 << 14, "cs_dive_upto<unsigned short, 4>", {3: 6, 200: 219}),
}

# the set of the budget, slice and smaller-k tests: deeper trees (30 % givens), k = 4; by the host walk no instance needs
# more than 1,311 nodes, so a budget of 1 << 14 ends every one DONE
DEEP = (lambda: problems.sudoku_roots(3, 0.30, list(range(1, 33)), "ALL"), 4, 1 << 14, "cs_dive_upto<unsigned char, 2>", 1311)

_built = {}
_walks = {}


def build(name):
    """-> (text, roots [K, n, 2] int32); name "deep" is DEEP"""
    if name not in _built:
        text, roots = (DEEP[0] if name == "deep" else SETS[name][0])()
        _built[name] = (text, np.ascontiguousarray(roots, dtype=np.int32))
    return _built[name]


def walk(name, k, max_nodes=None):
    """the host walk of the whole set under k (and the set's budget unless another is given), computed once"""
    budget = max_nodes if max_nodes is not None else (DEEP[2] if name == "deep" else SETS[name][2])
    key = (name, k, budget)
    if key not in _walks:
        text, roots = build(name)
        _walks[key] = many_walk_upto.dive_many_upto(text, roots, k, budget)
    return _walks[key]
