"""The instance sets of the solve_many_restarts tests (a helper module, no test itself): one model text, its root rows,
the restart bases the tests pass, the seed (or one seed per instance), the budget, the cs_dive_restart instantiation the
model plans and, per base, what the host walk of many_walk_restarts gives: the largest walk of the set (nodes over all
runs) and the number of instances that restart.  Every budget lies above the largest walk: no instance of these sets may
end in LIMIT, which test_solve_many_restarts_host.py asserts for these very rows.  Every set has instances that restart:
a set without any would test nothing new on its instantiation.  walk(name, base) is computed once and shared by the
tests that need it; nothing writes to it.

The 16-bit sets are one root row 24 times with the seeds 1 .. 24: under base 1 every instance restarts, and the seeds
lead them to 23 or 24 different solutions.  The largest of them has 140 variables, not 150: with two constraints per
pair the dense table of 150 variables (150 x 2 slots x 256 columns x 2 bytes) is larger than the 144 KB the kernels of
solve_many take, so that model does not qualify; 140 variables is the same generator call with n = 140, still R = 4."""
import numpy as np

import many_sets
import many_walk
import many_walk_restarts
from csolve_amd import problems

SEED = 12345


def _ne16(n):
    text = problems.sparse_ne(n, 6, 6, 2, per_pair=2, offset_spread=2, lo_spread=2000, pinned=n - 30)
    return text, np.repeat(many_walk.oracle_for(text)[1][None], 24, 0)


def _first(name, count):
    text, roots, _, _ = many_sets.build(name)
    return text, roots[:count]


def queens_placed(n, count, seed, placed):
    """queens-n rows with `placed` queens placed at random (placements that attack each other included)"""
    rng = problems.LCG(seed * 40503 + n * 7 + placed)
    rows = np.empty((count, n, 2), dtype=np.int32)
    rows[:, :, 0], rows[:, :, 1] = 1, n
    for k in range(count):
        cols = list(range(n))
        rng.shuffle(cols)
        for i in cols[:placed]:
            rows[k, i] = 1 + rng.below(n)
    return rows


_SEEDS24 = tuple(range(1, 25))

# name -> (builder of (text, roots), bases, seeds (None: SEED for every instance), max_nodes, kernel,
#          {base: (largest walk, restarted instances)})
SETS = {
    "sudoku9": (lambda: _first("sudoku9_any", 64), (8, 1), None, 1 << 12, "cs_dive_restart<unsigned char, 2>",
                {8: (246, 17), 1: (610, 42)}),
    "queens12_two": (lambda: _first("queens12_two", 48), (8,), None, 1 << 12, "cs_dive_restart<unsigned char, 1>",
                     {8: (287, 25)}),
    # the 12 rows of queens12_two without a solution are inconsistent at the root node: no node, no restart.  Of these
    # 32 rows with four queens, 27 have no solution and one of them is proven so only by a search: 374 nodes, 62 restarts
    "queens12_four": (lambda: (problems.queens(12, "ALL"), queens_placed(12, 32, 1, 4)), (1,), None, 1 << 12,
                      "cs_dive_restart<unsigned char, 1>", {1: (374, 5)}),
    "sudoku16": (lambda: _first("sudoku16_any", 16), (1,), None, 1 << 12, "cs_dive_restart<unsigned char, 4>",
                 {1: (241, 6)}),
    "ne16_40": (lambda: _ne16(40), (1,), _SEEDS24, 1 << 12, "cs_dive_restart<unsigned short, 1>", {1: (376, 24)}),
    "ne16_100": (lambda: _ne16(100), (1,), _SEEDS24, 1 << 12, "cs_dive_restart<unsigned short, 2>", {1: (304, 24)}),
    "ne16_140": (lambda: _ne16(140), (1,), _SEEDS24, 1 << 12, "cs_dive_restart<unsigned short, 4>", {1: (431, 24)}),
}

# the tail the restarts are for (CPU only): 512 9x9 sudokus with 30 % givens, base 32.  By the host walks: ascending
# (today's ANY) 114,515 nodes in all and 10,838 for the largest instance; with restarts 26,579 and 944, 115 restarted
TAIL = (lambda: problems.sudoku_roots(3, 0.30, list(range(1, 513))), 32, SEED,
        {"ascending": (114515, 10838), "restarts": (26579, 944), "restarted": 115})

# ROTATE_FIRST as a sampler: the empty 9x9 row 32 times, seeds 1 .. 32, base 8: 32 distinct grids, largest walk 1,470
SAMPLER = (8, tuple(range(1, 33)), 1 << 13, 1470)

_built = {}
_walks = {}


def build(name):
    """-> (text, roots [K, n, 2] int32, seeds uint32 [K] or None); "tail" and "sampler" are the two sets above"""
    if name not in _built:
        if name == "tail":
            text, roots = TAIL[0]()
            seeds = None
        elif name == "sampler":
            text = problems.sudoku_roots(3, 0.4, [1])[0]
            roots = np.repeat(many_walk.oracle_for(text)[1][None], len(SAMPLER[1]), 0)
            seeds = np.array(SAMPLER[1], dtype=np.uint32)
        else:
            text, roots = SETS[name][0]()
            seeds = None if SETS[name][2] is None else np.array(SETS[name][2], dtype=np.uint32)
        _built[name] = (text, np.ascontiguousarray(roots, dtype=np.int32), seeds)
    return _built[name]


def walk(name, base, max_nodes=None, rotate_first=False):
    """the host walk of the whole set under `base` (and the set's budget unless another is given), computed once"""
    budget = max_nodes if max_nodes is not None else (1 << 62 if name == "tail" else SAMPLER[2] if name == "sampler" else SETS[name][3])
    key = (name, base, budget, rotate_first)
    if key not in _walks:
        text, roots, seeds = build(name)
        _walks[key] = many_walk_restarts.dive_many_restarts(text, roots, base, seed=SEED, seeds=seeds,
                                                            rotate_first=rotate_first, max_nodes=budget)
    return _walks[key]
