"""Synthetic workload generators in the csolve problem-text format.

These produce the shapes BASELINE.json names: N-queens exactly as the reference's
generator writes it (reference scripts/gen_queens.sh:3-37), sudoku-shaped alldiff
networks scaled from 9x9 (reference examples/sudoku.txt:28-59) to 25x25, and
schedule-style optimisation problems after reference examples/schedule.txt.
All generators are deterministic functions of their arguments (own LCG, no `random`).
"""
from __future__ import annotations


class LCG:
    """64-bit LCG (Knuth MMIX constants); identical to the one in oracle/ref_harness.c."""

    def __init__(self, seed: int):
        self.state = seed & 0xFFFFFFFFFFFFFFFF

    def next(self) -> int:
        self.state = (self.state * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return self.state >> 33

    def below(self, n: int) -> int:
        return self.next() % n

    def shuffle(self, xs):
        for i in range(len(xs) - 1, 0, -1):
            j = self.below(i + 1)
            xs[i], xs[j] = xs[j], xs[i]
        return xs


def queens(n: int, objective: str = "ANY") -> str:
    """N-queens: three all_different lines plus 1 <= Xi <= N (gen_queens.sh:5-36)."""
    xs = [f"X{i}" for i in range(1, n + 1)]
    lines = [f"# N-queens problem for N={n}", f"{objective};"]
    lines.append("all_different(" + ", ".join(xs) + ");")
    lines.append("all_different(" + ", ".join(f"X{i}+{i}" for i in range(1, n + 1)) + ");")
    lines.append("all_different(" + ", ".join(f"X{i}-{i}" for i in range(1, n + 1)) + ");")
    for i in range(1, n + 1):
        lines.append(f"1 <= X{i}; X{i} <= {n};")
    return "\n".join(lines) + "\n"


def offsets(n: int = 20, values: int = 48, seed: int = 1, objective: str = "ANY") -> str:
    """A small binary != network with irregular shape: n variables of `values` values each, every variable
    with its own lower bound, and for most pairs one or two constraints Vi != Vj + d with seeded offsets
    (neither queens' three-per-pair regularity nor a common window: exercises the general table layout
    of the forbidden-set kernels and windows of more than 32 values on small models)."""
    rng = LCG(seed * 7919 + n * 31 + values)
    lo = [rng.below(9) - 4 for _ in range(n)]
    lines = [f"# offsets network, {n} variables x {values} values, seed {seed}", f"{objective};"]
    for i in range(n):
        for j in range(i + 1, n):
            k = rng.below(4)  # 0: unrelated, 1: one constraint, 2-3: two constraints
            ds = set()
            for _ in range(min(k, 2)):
                ds.add(rng.below(2 * values // 3 + 1) - values // 3 + lo[i] - lo[j])
            for d in sorted(ds):
                lines.append(f"V{i + 1} != V{j + 1} {'+' if d >= 0 else '-'} {abs(d)};")
    for i in range(n):
        lines.append(f"{lo[i]} <= V{i + 1}; V{i + 1} <= {lo[i] + values - 1};")
    return "\n".join(lines) + "\n"


def _cell(r: int, c: int) -> str:
    return f"C{r}_{c}"


def sudoku_solution(box: int, seed: int):
    """A valid box^2 x box^2 grid: the cyclic pattern with seeded row/column/digit shuffles."""
    n = box * box
    rng = LCG(seed)

    def banded():
        bands = rng.shuffle(list(range(box)))
        out = []
        for b in bands:
            out.extend(b * box + r for r in rng.shuffle(list(range(box))))
        return out

    rows, cols = banded(), banded()
    digits = rng.shuffle(list(range(1, n + 1)))
    return [[digits[(box * (r % box) + r // box + c) % n] for c in cols] for r in rows]


def sudoku(box: int = 3, revealed: float = 0.4, seed: int = 1, objective: str = "ANY") -> str:
    """box^2 x box^2 sudoku: givens, then rows / columns / boxes as all_different,
    then 1 <= cell <= n bounds (layout of examples/sudoku.txt, scaled)."""
    n = box * box
    grid = sudoku_solution(box, seed)
    rng = LCG(seed ^ 0x9E3779B97F4A7C15)
    cells = [(r, c) for r in range(n) for c in range(n)]
    rng.shuffle(cells)
    given = sorted(cells[: int(round(revealed * n * n))])
    lines = [f"# sudoku {n}x{n}, {len(given)} givens, seed {seed}", f"{objective};"]
    for r, c in given:
        lines.append(f"{_cell(r, c)} = {grid[r][c]};")
    for r in range(n):
        lines.append("all_different(" + ", ".join(_cell(r, c) for c in range(n)) + ");")
    for c in range(n):
        lines.append("all_different(" + ", ".join(_cell(r, c) for r in range(n)) + ");")
    for br in range(box):
        for bc in range(box):
            lines.append("all_different(" + ", ".join(_cell(br * box + r, bc * box + c)
                                                      for r in range(box) for c in range(box)) + ");")
    for r in range(n):
        lines.append(" ".join(f"1 <= {_cell(r, c)}; {_cell(r, c)} <= {n};" for c in range(n)))
    return "\n".join(lines) + "\n"


def sudoku_roots(box: int, revealed: float, seeds, objective: str = "ANY"):
    """Many sudokus as instances of ONE model (Model.solve_many): -> (text of the EMPTY box^2 x box^2 model -- the
    all_different and bound lines of sudoku(), no givens --, int32 array [len(seeds), n_cells, 2] of root rows).  Row k
    holds the givens sudoku(box, revealed, seeds[k]) writes as single values and 1 .. box^2 elsewhere; cells are
    numbered row by row, which is the order the empty model declares them in."""
    import numpy as np
    n = box * box
    text = "\n".join(line for line in sudoku(box, 0.0, 0).split("\n") if not line.startswith("#"))
    text = text.replace("ANY;", f"{objective};", 1)
    text = f"# sudoku {n}x{n}, no givens: the model of sudoku_roots\n" + text
    roots = np.empty((len(seeds), n * n, 2), dtype=np.int32)
    roots[:, :, 0] = 1
    roots[:, :, 1] = n
    for k, seed in enumerate(seeds):
        grid = sudoku_solution(box, seed)
        rng = LCG(seed ^ 0x9E3779B97F4A7C15)
        cells = [(r, c) for r in range(n) for c in range(n)]
        rng.shuffle(cells)
        for r, c in cells[: int(round(revealed * n * n))]:
            roots[k, r * n + c] = grid[r][c]
    return text, roots


def _less_pairs(box: int, seed: int, pairs: int):
    """the `pairs` horizontally adjacent cell pairs of sudoku_less(box, seed, pairs), each as (smaller cell, larger cell)
    in sudoku_solution(box, seed), sorted by position"""
    n = box * box
    grid = sudoku_solution(box, seed)
    rng = LCG(seed ^ 0xC2B2AE3D27D4EB4F)
    places = [(r, c) for r in range(n) for c in range(n - 1)]
    assert 0 <= pairs <= len(places), f"at most {len(places)} horizontally adjacent pairs"
    rng.shuffle(places)
    out = []
    for r, c in sorted(places[:pairs]):
        a, b = (r, c), (r, c + 1)
        out.append((a, b) if grid[r][c] < grid[r][c + 1] else (b, a))
    return out


def sudoku_less(box: int, seed: int, pairs: int, objective: str = "ANY") -> str:
    """A "greater-than sudoku" (futoshiki): the EMPTY box^2 x box^2 model of sudoku_roots() plus `pairs` strict
    inequalities between horizontally adjacent cells, all true in sudoku_solution(box, seed); the pairs are chosen with
    the module's LCG.  A != network plus `<` relations: no model of solve_many (kernel 7), and at box = 3 past the 512
    clauses of kernel 6.  Cells are numbered row by row as in sudoku_roots()."""
    n = box * box
    text, _ = sudoku_roots(box, 0.0, [], objective)
    lines = [line for line in text.split("\n") if line and not line.startswith("#")]
    lines.insert(0, f"# sudoku {n}x{n}, no givens, {pairs} inequalities of grid {seed}: the model of sudoku_less_roots")
    for (ra, ca), (rb, cb) in _less_pairs(box, seed, pairs):
        lines.append(f"{_cell(ra, ca)} < {_cell(rb, cb)};")
    return "\n".join(lines) + "\n"


def sudoku_less_roots(box: int, seed: int, pairs: int, revealed, dom=None, objective: str = "ANY"):
    """Instances of sudoku_less(box, seed, pairs) -> (its text, int32 array [len(revealed), n_cells, 2] of root rows).
    Row k reveals int(round(revealed[k] * n_cells)) cells of sudoku_solution(box, seed) as single values -- which cells,
    the module's LCG seeded with (seed, k) says -- and leaves the others open, so every row has that grid for a solution.
    dom: the model's root domains, int [n_cells, 2] (Model.domains() of the solved root).  The root fixpoint of the
    inequalities narrows them below 1 .. box^2 (the smaller cell of a pair cannot be box^2), and an open cell of a row
    is its root domain: a row outside the root domains is BAD_ROOT to the solve_many family.  None: 1 .. box^2."""
    import numpy as np
    n = box * box
    grid = sudoku_solution(box, seed)
    roots = np.empty((len(revealed), n * n, 2), dtype=np.int32)
    if dom is None:
        roots[:, :, 0], roots[:, :, 1] = 1, n
    else:
        roots[:] = np.asarray(dom, dtype=np.int32).reshape(1, n * n, 2)
    for k, share in enumerate(revealed):
        rng = LCG((seed * 1000003 + k) ^ 0x9E3779B97F4A7C15)
        cells = [(r, c) for r in range(n) for c in range(n)]
        rng.shuffle(cells)
        for r, c in cells[: int(round(share * n * n))]:
            roots[k, r * n + c] = grid[r][c]
    return sudoku_less(box, seed, pairs, objective), roots


def schedule(tasks: int = 16, seed: int = 1, horizon_slack: int = 3) -> str:
    """Single-machine scheduling after examples/schedule.txt: per task release, WCET and
    deadline, pairwise non-overlap disjunctions, MIN end."""
    rng = LCG(seed)
    wcet = [1 + rng.below(4) for _ in range(tasks)]
    total = sum(wcet)
    release = [rng.below(max(1, total // 2)) for _ in range(tasks)]
    lines = [f"# schedule: {tasks} tasks, seed {seed}", "MIN end;"]
    for t in range(tasks):
        dl = total * horizon_slack
        p = f"t{t + 1}"
        lines.append(f"{p}_release = {release[t]};")
        lines.append(f"{p}_release <= {p}_start;")
        lines.append(f"{p}_end = {p}_start + {wcet[t]};")
        lines.append(f"{p}_end <= {p}_release + {dl};")
    for a in range(tasks):
        for b in range(a + 1, tasks):
            pa, pb = f"t{a + 1}", f"t{b + 1}"
            lines.append(f"{pa}_start > {pb}_end | {pb}_start > {pa}_end;")
    for t in range(tasks):
        lines.append(f"end >= t{t + 1}_end;")
    return "\n".join(lines) + "\n"


def linear(n: int = 12, seed: int = 1, objective: str = "ANY") -> str:
    """A seeded mixture of the clause shapes that take the direct bound-propagation paths: `x < y + d`,
    `x <= y + d`, `x = y + d`, two-literal disjunctions of such literals, and a few `!=` (test workload for the
    linear paths of the general kernel and for the clause-resident kernel; no reference example has this mix)."""
    rng = LCG(seed * 104729 + n)
    v = [f"L{i + 1}" for i in range(n)]
    lines = [f"# linear mixture, {n} variables, seed {seed}", f"{objective};"]

    def term(i, d):
        return v[i] if d == 0 else f"{v[i]} {'+' if d > 0 else '-'} {abs(d)}"

    for _ in range(2 * n):
        a, b = rng.below(n), rng.below(n)
        if a == b:
            continue
        d = rng.below(13) - 6
        kind = rng.below(10)
        if kind < 4:
            lines.append(f"{v[a]} < {term(b, d + 8)};")
        elif kind < 6:
            lines.append(f"{v[a]} <= {term(b, d + 6)};")
        elif kind < 7:
            lines.append(f"{v[a]} != {term(b, d)};")
        else:
            c, e = rng.below(n), rng.below(n)
            if c == e:
                continue
            lines.append(f"{v[a]} > {term(b, d)} | {v[c]} > {term(e, rng.below(9) - 4)};")
    # one equality chain so that EQ clauses are present without making the model infeasible
    for i in range(0, n - 1, 5):
        lines.append(f"{v[i + 1]} = {term(i, 1 + rng.below(3))};")
    for i in range(n):
        lo = rng.below(7) - 3
        lines.append(f"{lo} <= {v[i]}; {v[i]} <= {lo + 20 + rng.below(20)};")
    return "\n".join(lines) + "\n"


def sparse_ne(n: int, degree: int = 3, width: int = 16, seed: int = 1, per_pair: int = 1, offset_spread: int = 4,
              lo_spread: int = 0, pinned: int = 0, objective: str = "ANY") -> str:
    """A seeded sparse binary != network: n variables of `width` values each, variable i's lower bound drawn from
    [0, lo_spread], about `degree` neighbours per variable and `per_pair` constraints `Vi != Vj + d` per related
    pair.  Every d lies within `offset_spread` of lo_i - lo_j, so no constraint is entailed by the root domains
    (|d - (lo_i - lo_j)| < width); the spreads set the table entry widths of the kernels (offsets and lower bounds
    far apart need wide entries).  `pinned` variables get a seeded one-value domain and no constraint (a constraint on
    a fixed variable would be folded into a unary clause, which takes the network off the != kernels); the n - pinned
    free ones are spread evenly over the index range, the last variable among them, so that they reach every register
    stride.  Pinning keeps exhaustive searches small at large n while the kernels still see all n variables."""
    assert n >= 1 and width >= 1 and per_pair >= 1 and 0 <= pinned < n
    assert per_pair <= 2 * min(offset_spread, width - 1) + 1, "not enough distinct offsets for per_pair"
    rng = LCG(seed * 1000003 + n * 8191 + width * 131 + per_pair)
    lo = [rng.below(lo_spread + 1) for _ in range(n)]
    free = sorted({n - 1 - j * n // (n - pinned) for j in range(n - pinned)})
    value = {v: lo[v] + rng.below(width) for v in sorted(set(range(n)) - set(free))}
    lines = [f"# sparse != network, {n} variables x {width} values, degree {degree}, {per_pair} per pair, seed {seed}",
             f"{objective};"]
    pairs = set()
    for k, i in enumerate(free):
        for _ in range(degree if len(free) > 1 else 0):
            j = free[(k + 1 + rng.below(len(free) - 1)) % len(free)]
            pairs.add((min(i, j), max(i, j)))
    reach = min(offset_spread, width - 1)
    for i, j in sorted(pairs):
        ds = set()
        while len(ds) < per_pair:
            ds.add(lo[i] - lo[j] + rng.below(2 * reach + 1) - reach)
        for d in sorted(ds):
            lines.append(f"V{i + 1} != V{j + 1} {'+' if d >= 0 else '-'} {abs(d)};")
    for v in range(n):
        a, b = (value[v], value[v]) if v in value else (lo[v], lo[v] + width - 1)
        lines.append(f"{a} <= V{v + 1}; V{v + 1} <= {b};")
    return "\n".join(lines) + "\n"
