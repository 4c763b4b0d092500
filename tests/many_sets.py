"""The instance sets of the solve_many tests (a helper module, no test itself): one model text, its root rows, the
objective, the budget the tests pass and the cs_dive_shave instantiation the model plans.  Budgets and seeds were chosen
on the host with many_walk alone: `largest` is the largest tree (nodes) of the set by that walk, and every budget lies
above it -- no instance of these sets may end in LIMIT.  test_solve_many_host.py re-checks a sample of each set."""
import numpy as np

import many_walk
from csolve_amd import problems


def narrowed(text, count, seed, keep_one_in=4, max_width=4):
    """`count` rows inside the root domains of `text`: every open variable is, with probability 1 / keep_one_in, cut
    down to a seeded sub-interval of at most max_width values"""
    _, dom = many_walk.oracle_for(text)
    rng = problems.LCG(seed * 2654435761 + count)
    rows = np.repeat(dom[None], count, 0).astype(np.int32)
    for k in range(count):
        for v in range(dom.shape[0]):
            width = int(dom[v, 1] - dom[v, 0]) + 1
            if width > 1 and rng.below(keep_one_in) == 0:
                w = 1 + rng.below(min(max_width, width))
                lo = int(dom[v, 0]) + rng.below(width - w + 1)
                rows[k, v] = (lo, lo + w - 1)
    return rows


def queens_two(n, count, seed):
    """queens-n rows with two queens placed at random (placements that attack each other included)"""
    rng = problems.LCG(seed * 40503 + n)
    rows = np.empty((count, n, 2), dtype=np.int32)
    rows[:, :, 0], rows[:, :, 1] = 1, n
    for k in range(count):
        i = rng.below(n)
        j = (i + 1 + rng.below(n - 1)) % n
        rows[k, i] = 1 + rng.below(n)
        rows[k, j] = 1 + rng.below(n)
    return rows


def _sparse16(n, free, seed=1):
    """a sparse != network whose dense table has 16-bit entries (lower bounds 2000 apart), all but `free` variables given"""
    return problems.sparse_ne(n, 3, 40, seed, per_pair=1, offset_spread=4, lo_spread=2000, pinned=n - free, objective="ALL")


# name -> (builder of (text, roots), objective, max_nodes, kernel, largest tree of the set by many_walk)
SETS = {
    "sudoku9_any": (lambda: problems.sudoku_roots(3, 0.36, list(range(1, 257))), "ANY", 4096,
                    "cs_dive_shave<unsigned char, 2>", 615),
    "sudoku9_all": (lambda: problems.sudoku_roots(3, 0.40, list(range(1, 65)), "ALL"), "ALL", 1 << 16,
                    "cs_dive_shave<unsigned char, 2>", 1136),
    "queens12_two": (lambda: (problems.queens(12, "ALL"), queens_two(12, 48, 1)), "ALL", 1 << 16,
                     "cs_dive_shave<unsigned char, 1>", 7572),
    "offsets40": (lambda: (problems.offsets(40, 8, 1, "ALL"), narrowed(problems.offsets(40, 8, 1, "ALL"), 32, 1, 12)), "ALL",
                  1 << 16, "cs_dive_shave<unsigned char, 1>", 26134),
    "offsets64": (lambda: (problems.offsets(64, 8, 1, "ALL"), narrowed(problems.offsets(64, 8, 1, "ALL"), 32, 2, 20)), "ALL",
                  1 << 16, "cs_dive_shave<unsigned char, 1>", 17465),
    "sudoku16_any": (lambda: problems.sudoku_roots(4, 0.55, list(range(1, 17))), "ANY", 1 << 14,
                     "cs_dive_shave<unsigned char, 4>", 24),
    "sparse40_e16": (lambda: (_sparse16(40, 3), narrowed(_sparse16(40, 3), 24, 3, 2, 8)), "ALL", 1 << 17,
                     "cs_dive_shave<unsigned short, 1>", 63999),
    "sparse100_e16": (lambda: (_sparse16(100, 3), narrowed(_sparse16(100, 3), 24, 4, 2, 8)), "ALL", 1 << 17,
                      "cs_dive_shave<unsigned short, 2>", 64118),
    "sparse150_e16": (lambda: (_sparse16(150, 3), narrowed(_sparse16(150, 3), 24, 5, 2, 8)), "ALL", 1 << 17,
                      "cs_dive_shave<unsigned short, 4>", 64116),
}


def build(name):
    """-> (text, roots [K, n, 2] int32, objective, max_nodes)"""
    make, objective, budget, _, _ = SETS[name]
    text, roots = make()
    return text, np.ascontiguousarray(roots, dtype=np.int32), objective, budget
