"""The mixed-operator sets of the expression-tree tests (a helper module, no test itself): a seeded generator of models
whose clauses are the trees only the interpreter (cs_tree_eval / cs_tree_revise) can revise -- products of variables, a
variable twice in one tree, NEG over a subexpression, `=` and `!=` between sums, three-literal disjunctions, AND / OR / NOT
below the top of a clause, products that saturate, sums near the 256-node limit -- next to the ordinary binary
relations, and the table of named sets with what test_tree_sets_host.py derives for them on the host.

Every variable has declared finite bounds and the widths of a set add up to at most MAX_TOTAL_WIDTH values: a
propagation moves a bound by at least one, so no revision order, the device's included, narrows such a model more often
than that.  The constants are drawn around one planted point, which every clause accepts."""
import os
import sys

import numpy as np

from csolve_amd import problems

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

INT32_MAX, INT32_MIN = 2**31 - 1, -2**31
MAX_TOTAL_WIDTH = 4096
MAX_TREE_NODES = 256  # CS_MAX_TREE_NODES (cs_device.h)
LONGEST_SUM = 127     # k variables, k - 1 ADD, the constant, LT and NOT: 2 k + 2 nodes (a negative constant is NEG of one: 2 k + 3
                      # until the normaliser folds it, and the root phase builds tables before that)

# shape -> is it a tree whatever the fast paths are set to (the plain shapes are the binary relations and the
# two-literal disjunction, which the linear fast paths take)
TREE_SHAPES = {
    "mul": ("mul_le", "mul_eq", "mul_ne", "mul3_le"),
    "twice": ("twice_add", "twice_mul"),
    "neg": ("neg_sum", "neg_mul"),
    "eq": ("eq_sum", "ne_sum", "ne_2a"),
    "or3": ("or3",),
    "bool": ("and_or_not", "not_or", "ne_or_sum"),
}
PLAIN_SHAPES = ("lt", "le", "eq", "ne", "or2")
ALL_TREE_SHAPES = tuple(s for fam in TREE_SHAPES.values() for s in fam)


# ---- the reference's saturating arithmetic (reference src/arith.c:27-85) on int64 numpy values: the sentinels absorb,
# -inf wins over +inf in a sum, zero counts as not negative in a product with a sentinel

def sat_neg(a):
    a = np.asarray(a, dtype=np.int64)
    return np.where(a == INT32_MIN, INT32_MAX, np.where(a == INT32_MAX, INT32_MIN, -a))


def sat_add(a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    plain = np.clip(a + b, INT32_MIN, INT32_MAX)
    return np.where((a == INT32_MIN) | (b == INT32_MIN), INT32_MIN, np.where((a == INT32_MAX) | (b == INT32_MAX), INT32_MAX, plain))


def sat_mul(a, b):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    plain = np.clip(a * b, INT32_MIN, INT32_MAX)  # |a|, |b| <= 2^31: the product fits 64 bits
    r = np.where(b == INT32_MAX, np.where(a < 0, INT32_MIN, INT32_MAX), plain)
    r = np.where(a == INT32_MAX, np.where(b < 0, INT32_MIN, INT32_MAX), r)
    r = np.where(b == INT32_MIN, np.where(a < 0, INT32_MAX, INT32_MIN), r)
    return np.where(a == INT32_MIN, np.where(b < 0, INT32_MAX, INT32_MIN), r)


def is_sentinel(a):
    a = np.asarray(a, dtype=np.int64)
    return (a == INT32_MIN) | (a == INT32_MAX)


def _term(name, d):
    return name if d == 0 else f"{name} {'+' if d > 0 else '-'} {abs(d)}"


def _pred(fn, shape, decided=None):
    """a clause as a function of a sequence x of the n values (numpy columns work as well).  fn: does the clause hold;
    shape: the generator's name of its form; decided: is its value a truth value at x (None: always) -- a comparison
    with a saturated side evaluates to `unknown` in the reference (eval.c:47-50, 81-84) although propagation treats the
    sentinel as the number it is"""
    fn.shape = shape
    fn.tree = shape not in PLAIN_SHAPES
    fn.decided = decided
    return fn


class _Predicates(list):
    """the predicates of a model, in the order of its text; .planted: the point all of them accept (C1 .. Cn)"""
    planted = None


class _Builder:
    def __init__(self, rng, bounds, slack, low=False):
        self.rng, self.bounds, self.slack = rng, bounds, slack
        self.n = len(bounds)
        self.name = [f"C{i + 1}" for i in range(self.n)]
        self.pt = [lo + rng.below(hi - lo + 1) for lo, hi in bounds]  # the planted point
        if low:  # at the lower bounds but for every fortieth variable: a sum over many variables has little room left
            self.pt = [lo + (i % 40 == 7) for i, (lo, hi) in enumerate(bounds)]
        self.lines, self.preds = [], _Predicates()
        self.preds.planted = tuple(self.pt)

    def r(self, k=None):
        return self.rng.below((self.slack if k is None else k) + 1)

    def pick(self, k):
        """k different variables"""
        out = []
        while len(out) < k:
            v = self.rng.below(self.n)
            if v not in out:
                out.append(v)
        return out

    def off(self, a, b):
        """a nonzero offset from the planted gap: the d of a literal `a != b + d` (or of a false `a = b + d`)"""
        d = 1 + self.r(1)
        return self.pt[a] - self.pt[b] + (d if self.rng.below(2) else -d)

    def lt_lit(self, true):
        """a literal a < b + d that holds (or not) at the planted point -> (text, function of x)"""
        a, b = self.pick(2)
        gap = self.pt[a] - self.pt[b]
        d = gap + 1 + self.r() if true else gap - self.r()
        return f"{self.name[a]} < {_term(self.name[b], d)}", (lambda x, a=a, b=b, d=d: x[a] < x[b] + d)

    def eq_lit(self, true):
        a, b = self.pick(2)
        d = self.pt[a] - self.pt[b] if true else self.off(a, b)
        return f"{self.name[a]} = {_term(self.name[b], d)}", (lambda x, a=a, b=b, d=d: x[a] == x[b] + d)

    def add(self, text, fn, shape, decided=None):
        assert bool(fn(self.pt)), (text, self.pt)
        self.lines.append(text + ";")
        self.preds.append(_pred(fn, shape, decided))

    def clause(self, shape):
        N, pt, r = self.name, self.pt, self.r
        if shape == "lt":
            text, fn = self.lt_lit(True)
            self.add(text, fn, shape)
        elif shape == "le":
            a, b = self.pick(2)
            d = pt[a] - pt[b] + r()
            self.add(f"{N[a]} <= {_term(N[b], d)}", lambda x: x[a] <= x[b] + d, shape)
        elif shape == "eq":
            text, fn = self.eq_lit(True)
            self.add(text, fn, shape)
        elif shape == "ne":
            a, b = self.pick(2)
            d = self.off(a, b)
            self.add(f"{N[a]} != {_term(N[b], d)}", lambda x: x[a] != x[b] + d, shape)
        elif shape == "or2":
            first = self.rng.below(2)
            (t0, f0), (t1, f1) = self.lt_lit(first == 0), self.lt_lit(first == 1 or self.rng.below(3) == 0)
            self.add(f"{t0} | {t1}", lambda x: f0(x) | f1(x), shape)
        elif shape == "mul_le":
            a, b, c = self.pick(3)
            s = pt[a] * pt[b] - pt[c] + r()
            self.add(f"{N[a]} * {N[b]} <= {_term(N[c], s)}", lambda x: x[a] * x[b] <= x[c] + s, shape)
        elif shape == "mul_eq":
            a, b, c = self.pick(3)
            s = pt[a] * pt[b] - pt[c]
            self.add(f"{N[a]} * {N[b]} = {_term(N[c], s)}", lambda x: x[a] * x[b] == x[c] + s, shape)
        elif shape == "mul_ne":
            a, b = self.pick(2)
            k = pt[a] * pt[b] + (1 + r(2)) * (1 if self.rng.below(2) else -1)
            self.add(f"{N[a]} * {N[b]} != {k}", lambda x: x[a] * x[b] != k, shape)
        elif shape == "mul3_le":
            a, b = self.pick(2)
            q = 2 + self.rng.below(3)
            s = q * pt[a] * pt[b] + r(q)
            self.add(f"{q} * {N[a]} * {N[b]} <= {s}", lambda x: q * x[a] * x[b] <= s, shape)
        elif shape == "twice_add":
            a, b = self.pick(2)
            s = 2 * pt[a] - pt[b] + r()
            self.add(f"{N[a]} + {N[a]} <= {_term(N[b], s)}", lambda x: x[a] + x[a] <= x[b] + s, shape)
        elif shape == "twice_mul":
            a, b = self.pick(2)
            s = pt[a] * pt[a] - pt[b] + r()
            self.add(f"{N[a]} * {N[a]} <= {_term(N[b], s)}", lambda x: x[a] * x[a] <= x[b] + s, shape)
        elif shape == "neg_sum":
            a, b, c, d = self.pick(4)
            s = -(pt[a] + pt[b]) - (pt[c] - pt[d]) + 1 + r()
            self.add(f"-({N[a]} + {N[b]}) < {_term(f'{N[c]} - {N[d]}', s)}", lambda x: -(x[a] + x[b]) < x[c] - x[d] + s, shape)
        elif shape == "neg_mul":
            a, b = self.pick(2)
            s = -pt[a] * pt[b] + r()
            self.add(f"-{N[a]} * {N[b]} <= {s}", lambda x: -x[a] * x[b] <= s, shape)
        elif shape == "eq_sum":
            a, b, c, d = self.pick(4)
            s = pt[a] + pt[b] - pt[c] - pt[d]
            self.add(f"{N[a]} + {N[b]} = {_term(f'{N[c]} + {N[d]}', s)}", lambda x: x[a] + x[b] == x[c] + x[d] + s, shape)
        elif shape == "ne_sum":
            a, b, c, d = self.pick(4)
            s = pt[a] + pt[b] - pt[c] - pt[d] + (1 + r(1)) * (1 if self.rng.below(2) else -1)
            self.add(f"{N[a]} + {N[b]} != {_term(f'{N[c]} + {N[d]}', s)}", lambda x: x[a] + x[b] != x[c] + x[d] + s, shape)
        elif shape == "ne_2a":
            a, b, c = self.pick(3)
            s = 2 * pt[a] - pt[b] - pt[c] + (1 + r(1)) * (1 if self.rng.below(2) else -1)
            self.add(f"2 * {N[a]} != {_term(f'{N[b]} + {N[c]}', s)}", lambda x: 2 * x[a] != x[b] + x[c] + s, shape)
        elif shape == "or3":
            true = self.rng.below(3)
            (t0, f0), (t1, f1), (t2, f2) = self.lt_lit(true == 0), self.lt_lit(true == 1), self.eq_lit(true == 2)
            self.add(f"{t0} | {t1} | {t2}", lambda x: f0(x) | f1(x) | f2(x), shape)
        elif shape == "and_or_not":  # (a < b + d1 & c = d + d2) | !(e <= f + d3)
            left = self.rng.below(2) == 0
            (t0, f0), (t1, f1) = self.lt_lit(left or self.rng.below(2) == 0), self.eq_lit(left or self.rng.below(2) == 0)
            e, f = self.pick(2)
            d3 = pt[e] - pt[f] - 1 - r() if not left or self.rng.below(3) == 0 else pt[e] - pt[f] + r()
            self.add(f"({t0} & {t1}) | !({N[e]} <= {_term(N[f], d3)})", lambda x: (f0(x) & f1(x)) | (x[e] > x[f] + d3), shape)
        elif shape == "not_or":  # !(a = b + d1 | c < d + d2)
            (t0, f0), (t1, f1) = self.eq_lit(False), self.lt_lit(False)
            self.add(f"!({t0} | {t1})", lambda x: (f0(x) == False) & (f1(x) == False), shape)  # noqa: E712
        elif shape == "ne_or_sum":  # a != b + d1 | c + d <= e + s
            left = self.rng.below(2) == 0
            a, b = self.pick(2)
            d1 = self.off(a, b) if left or self.rng.below(2) == 0 else pt[a] - pt[b]
            c, d, e = self.pick(3)
            s = pt[c] + pt[d] - pt[e] + (r() if not left or self.rng.below(2) == 0 else -1 - r())
            self.add(f"{N[a]} != {_term(N[b], d1)} | {N[c]} + {N[d]} <= {_term(N[e], s)}",
                     lambda x: (x[a] != x[b] + d1) | (x[c] + x[d] <= x[e] + s), shape)
        else:
            raise ValueError(shape)

    def long_sum(self, variables):
        s = sum(self.pt[v] for v in variables) + self.r()
        self.add(" + ".join(self.name[v] for v in variables) + f" <= {s}", lambda x: sum(x[v] for v in variables) <= s, "long_sum")

    def text(self, title):
        lines = [f"# {title}", "ALL;"] + self.lines
        for i, (lo, hi) in enumerate(self.bounds):
            lines.append(f"{lo} <= {self.name[i]}; {self.name[i]} <= {hi};")
        return "\n".join(lines) + "\n"


def generate(n, seed, shapes, clauses, width=(3, 6), slack=1, plain=0, plain_shapes=PLAIN_SHAPES, sums=(), low=False, floor=-5,
             objective="ALL"):
    """-> (text, predicates, bounds): n variables C1 .. Cn of width[0] .. width[1] values, lower bounds floor .. floor + 8
    (on both sides of zero by default); `clauses` seeded constraints, every shape of `shapes` (families of TREE_SHAPES or single shapes) at least once
    and then drawn from them, `plain` of every hundred from the binary relations and the two-literal disjunction
    instead; for every k of `sums` one sum of the first k variables (with `low` the planted point lies at the lower bounds
    but for a few variables, so that such a sum forces the others down once one of them rises); then the bounds.  Every clause holds at one seeded
    planted point with at most `slack` to spare.  predicates: the clauses in the order of the text, each with .shape and
    .tree; bounds: [(lo, hi)]."""
    rng = problems.LCG(seed * 1000003 + n * 8191 + clauses * 131 + width[0] * 17 + width[1])
    bounds = []
    for _ in range(n):
        w = width[0] + rng.below(width[1] - width[0] + 1)
        lo = rng.below(9) + floor
        bounds.append((lo, lo + w - 1))
    b = _Builder(rng, bounds, slack, low)
    pool = [s for fam in shapes for s in TREE_SHAPES.get(fam, (fam,))]
    for k in sums:
        b.long_sum(list(range(k)))
    for i in range(clauses):
        if plain and rng.below(100) < plain:
            b.clause(plain_shapes[rng.below(len(plain_shapes))])
        else:
            b.clause(pool[i] if i < len(pool) else pool[rng.below(len(pool))])
    text = b.text(f"tree model: {n} variables, seed {seed}, {clauses} clauses of {' '.join(shapes)}")
    return text.replace("ALL;", objective + ";", 1), b.preds, bounds


# the centres of sat_prod's variables: 46341 * 46341 and 1291 ** 3 are the first products past 2^31 - 1, so a product of
# two or three variables around them saturates on a part of its domain; 50000 * 50000 always does
SAT_CENTRES = (46341, -46341, 1290, -1290, 50000, -50000, 46300, 3, -2, 1291)


def generate_sat(n, seed, clauses, width=64, plain=40, objective="ALL"):
    """-> (text, predicates, bounds): variables of up to `width` values around SAT_CENTRES; products of three variables
    and of a constant and two, compared with a variable plus a constant in the direction the planted point allows, so
    that intermediate values leave the int32 range while every variable keeps its declared bounds; `plain` of every
    hundred clauses are binary relations between variables of like centres.  The predicates compute as the reference
    does (sat_add, sat_mul), and .decided says where no compared side is a sentinel."""
    rng = problems.LCG(seed * 1000003 + n * 8191 + clauses * 131 + width)
    bounds, centre = [], []
    for i in range(n):
        c = SAT_CENTRES[i % len(SAT_CENTRES)]
        w = max(3, width - rng.below(width // 2))
        lo = c - rng.below(w)
        bounds.append((lo, lo + w - 1))
        centre.append(c)
    b = _Builder(rng, bounds, 2)
    N, pt = b.name, b.pt

    def compare(text, product, shape, factors):
        """product(x) against a variable plus a constant: <= where the planted product is low, >= where it is high, and
        = / != now and then; the right side never reaches a sentinel (the constant stays 483,647 inside the range).
        `>=` is written only where the product reaches +inf on all of the declared box or on none of it: pushing
        [r, +inf] down a product divides +inf by the other factor (propagate.c:249-286), which cuts off the points where
        the product overflows, unless the normaliser has folded a product that is +inf everywhere into a constant --
        the truth of such a clause would depend on the root phase, and no predicate could state it"""
        c = rng.below(n)
        p0 = int(product(pt))
        kind = rng.below(6)
        corners = []
        for mask in range(1 << len(factors)):
            x = list(pt)
            for j, v in enumerate(factors):
                x[v] = bounds[v][(mask >> j) & 1]
            corners.append(int(product(x)))
        if p0 > 0 and (kind < 2 or is_sentinel(p0)) and max(corners) == INT32_MAX and min(corners) != INT32_MAX:
            kind = 5
        loose = max(2, min(abs(p0), 2**30) // 64)  # a product moves by tens of thousands when a factor moves by one
        if kind < 2 or is_sentinel(p0):
            if p0 > 0:
                s = min(p0 - pt[c] - b.r(loose), 2_147_000_000 - abs(pt[c]) - 64)
                b.add(f"{text} >= {_term(N[c], s)}", lambda x: product(x) >= sat_add(x[c], s), shape + "_ge",
                      lambda x: ~is_sentinel(product(x)))
            else:
                s = max(p0 - pt[c] + b.r(loose), -2_147_000_000 + abs(pt[c]) + 64)
                b.add(f"{text} <= {_term(N[c], s)}", lambda x: product(x) <= sat_add(x[c], s), shape + "_le",
                      lambda x: ~is_sentinel(product(x)))
        elif kind < 4:
            s = p0 - pt[c] + b.r(loose)
            b.add(f"{text} <= {_term(N[c], s)}", lambda x: product(x) <= sat_add(x[c], s), shape + "_le",
                  lambda x: ~is_sentinel(product(x)))
        elif kind < 5:
            s = p0 - pt[c]
            b.add(f"{text} = {_term(N[c], s)}", lambda x: product(x) == sat_add(x[c], s), shape + "_eq",
                  lambda x: ~is_sentinel(product(x)))
        else:
            k = p0 + (1 + b.r(2)) * (1 if p0 < 0 else -1)
            b.add(f"{text} != {k}", lambda x: product(x) != k, shape + "_ne", lambda x: ~is_sentinel(product(x)))

    for i in range(clauses):
        if rng.below(100) < plain:
            a = rng.below(n)
            like = [v for v in range(n) if v != a and centre[v] == centre[a]] or [v for v in range(n) if v != a]
            c = like[rng.below(len(like))]
            kind = rng.below(3)
            if kind == 0:
                d = pt[a] - pt[c] + 1 + b.r(8)
                b.add(f"{N[a]} < {_term(N[c], d)}", lambda x, a=a, c=c, d=d: x[a] < x[c] + d, "lt")
            elif kind == 1:
                d = pt[a] - pt[c] + b.r(8)
                b.add(f"{N[a]} <= {_term(N[c], d)}", lambda x, a=a, c=c, d=d: x[a] <= x[c] + d, "le")
            else:
                d = b.off(a, c)
                b.add(f"{N[a]} != {_term(N[c], d)}", lambda x, a=a, c=c, d=d: x[a] != x[c] + d, "ne")
        elif rng.below(3) == 0:
            u, v = b.pick(2)
            q = 2 + rng.below(3)
            compare(f"{q} * {N[u]} * {N[v]}", lambda x, q=q, u=u, v=v: sat_mul(sat_mul(q, x[u]), x[v]), "sat2", (u, v))
        else:
            u, v, w = b.pick(3)
            compare(f"{N[u]} * {N[v]} * {N[w]}", lambda x, u=u, v=v, w=w: sat_mul(sat_mul(x[u], x[v]), x[w]), "sat3", (u, v, w))
    text = b.text(f"saturating products: {n} variables, seed {seed}, {clauses} clauses")
    return text.replace("ALL;", objective + ";", 1), b.preds, bounds


# name -> how it is generated.  Widths are values per variable; twice*: the repeated-variable shapes alone; sat_prod: see
# generate_sat; mixed40 / mixed120: all families, 2 to 3 clauses per variable, 181 and 501 clauses in the tables (the
# objective's constant and the 2 n bound clauses count), which kernel 6 holds at 4 and at 8 clauses per lane; bigtab: more
# adjacency than kernel 1 copies into LDS; longsum: the sums of 127 and of 63 variables; longsum_prefix: the same shape at
# a length a brute force can enumerate, for the search engine
SETS = {}


def _set(name, gen="tree", **kw):
    SETS[name] = {"gen": gen, "args": kw}


FAMILIES = tuple(TREE_SHAPES)
_set("narrow_mul", n=6, seed=11, shapes=("mul",), clauses=9, plain=25, slack=2)
_set("narrow_neg", n=6, seed=12, shapes=("neg",), clauses=9, plain=25, slack=2)
_set("narrow_eq", n=6, seed=20, shapes=("eq",), clauses=9, plain=25, slack=2)
_set("narrow_or3", n=6, seed=21, shapes=("or3",), clauses=8, plain=25, slack=2)
_set("narrow_bool", n=6, seed=6, shapes=("bool",), clauses=10, plain=25, slack=2)
_set("narrow_mixed", n=7, seed=18, shapes=FAMILIES, clauses=14, plain=10, slack=2)
_set("twice6", n=6, seed=10, shapes=("twice",), clauses=8, slack=2)
_set("twice5", n=5, seed=1, shapes=("twice",), clauses=9, width=(4, 6), slack=2)
_set("sat_prod", gen="sat", n=14, seed=1, clauses=30)
_set("mixed40", n=40, seed=9, shapes=FAMILIES, clauses=100, plain=40, slack=3)
_set("mixed120", n=120, seed=10, shapes=FAMILIES, clauses=260, plain=45, slack=3)
_set("bigtab", n=1100, seed=11, shapes=("mul_ne", "ne_sum", "ne_2a", "or3", "bool", "mul_le", "neg_sum"), clauses=2600, plain=90,
     plain_shapes=("ne", "or2", "or2"), width=(2, 4), slack=1)
_set("longsum", n=LONGEST_SUM, seed=12, shapes=("lt", "le", "ne", "or2"), clauses=160, width=(2, 3), slack=3, low=True, floor=0,
     sums=(LONGEST_SUM, LONGEST_SUM // 2))
_set("longsum_prefix", n=12, seed=12, shapes=("lt", "le", "ne", "or2"), clauses=10, width=(2, 3), slack=3, low=True, floor=0, sums=(12, 6))

NAMES = list(SETS)
NARROW = [k for k in NAMES if k.startswith("narrow_")]
TWICE = [k for k in NAMES if k.startswith("twice")]
BRUTE = NARROW + TWICE + ["longsum_prefix"]   # the cross product of the declared bounds is enumerated
SMALL = NARROW + TWICE + ["sat_prod"]         # the single-node paths run on these
SEARCHED = NARROW + TWICE + ["longsum_prefix"]
BATCHES = (1, 63, 64, 65, 2000)
SAMPLE = 200_000  # points of sat_prod's seeded sample


def generate_set(name, objective="ALL"):
    rec = SETS[name]
    return (generate_sat if rec["gen"] == "sat" else generate)(objective=objective, **rec["args"])


def text_of(name, objective="ALL"):
    return generate_set(name, objective)[0]


def oracle_of(text, domains=None, normalize=True):
    """-> (oracle model, Oracle, columns): the model from the root domains (the oracle's own root phase, or `domains`),
    normalised like the product's tables, so that clause i is clause i there, and indexed; columns[i] is the model's
    index of C<i+1>"""
    import search_sets as S
    from oracle.cs_oracle import Model as OModel, Oracle
    if domains is None:
        domains = S.oracle_model(text)[0].domains()
    om = OModel.parse(text)
    om.set_domains(domains)
    if normalize:
        om.normalize()
    om.index()
    return om, Oracle(om), S.columns(om.names())


def clause_variables(om):
    """the variables of every clause of an indexed oracle model, anywhere in its tree -> [set]"""
    lists = [set() for _ in range(om.n_clauses)]
    for v in range(om.n_vars):
        for i in range(om.view.list_off[v], om.view.list_off[v + 1]):
            lists[om.view.list[i]].add(v)
    return lists


def instances(name, domains=None, batches=BATCHES):
    """the recorded instances of a set: states of seeded oracle walks (depth up to 6) and, for every batch size, value,
    interval and var = -1 nodes on repeated parents, with the oracle's verdict, fixpoint and PROPS of every node ->
    dict(states [P, n, 2], nodes [sum(batches), 4], status, out, props, oracle, model, columns)"""
    import zlib
    from test_gpu_instantiations import _nodes, _walk_states
    om, orc, cols = oracle_of(text_of(name), domains)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    states = _walk_states(orc, om.domains(), rng)
    nodes = np.concatenate([_nodes(rng, states, B) for B in batches])
    status = np.empty(len(nodes), dtype=np.int64)
    props = np.empty(len(nodes), dtype=np.int64)
    out = np.empty((len(nodes),) + states.shape[1:], dtype=np.int32)
    for i, (v, lo, hi, p) in enumerate(nodes):
        status[i], out[i] = orc.instance(states[p], int(v), int(lo), int(hi))
        props[i] = orc.props()
    return dict(states=states, nodes=nodes, status=status, out=out, props=props, oracle=orc, model=om, columns=cols)


def below(states, nodes):
    """the intervals a node's subtree lies in: its parent with the node's interval on its variable -> [B, n, 2]"""
    dom = states[nodes[:, 3]].copy()
    rows = np.nonzero(nodes[:, 0] >= 0)[0]
    dom[rows, nodes[rows, 0], 0] = nodes[rows, 1]
    dom[rows, nodes[rows, 0], 1] = nodes[rows, 2]
    return dom


def solution_rows(name, columns):
    """the points of a set that satisfy every predicate, as rows in the model's variable order: all of them by
    search_sets.brute_force, for sat_prod those among SAMPLE seeded points of the declared bounds"""
    import search_sets as S
    _, preds, bounds = generate_set(name)
    if name == "sat_prod":
        rng = np.random.default_rng(20)
        cols = [rng.integers(lo, hi + 1, size=SAMPLE) for lo, hi in bounds]
        # half of the sample near the planted point (a uniform point of 10^22 rarely satisfies thirty clauses): every
        # coordinate keeps the planted value with probability 3 / 4
        for i, c in enumerate(cols):
            keep = rng.random(SAMPLE // 2) < 0.75
            c[: SAMPLE // 2][keep] = preds.planted[i]
        ok = np.ones(SAMPLE, dtype=bool)
        for p in preds:
            ok &= p(cols)
        pts = np.stack([c[ok] for c in cols], 1)
    else:
        pts = np.array(sorted(S.brute_force(preds, bounds)), dtype=np.int64).reshape(-1, len(bounds))
    rows = np.zeros_like(pts)
    rows[:, columns] = pts
    return rows


def contained(rows, dom):
    """which solution rows lie inside the intervals `dom` [n, 2]"""
    return ((rows >= dom[:, 0]) & (rows <= dom[:, 1])).all(1)


def check_against_solutions(rows, states, nodes, status, out):
    """a consistent node's fixpoint holds every solution below the node, a failed node has none below it -> number of
    instances that had a solution below them"""
    dom = below(states, nodes)
    with_solutions = 0
    for i in range(len(nodes)):
        under = contained(rows, dom[i])
        with_solutions += bool(under.any())
        if status[i] < 0:
            assert not under.any(), ("a failed node has a solution below it", nodes[i].tolist(), rows[under][:1].tolist())
        else:
            assert (contained(rows, out[i]) == under).all(), ("the fixpoint loses a solution", nodes[i].tolist())
    return with_solutions


def points(name, columns, count=64, seed=5, box=None):
    """complete assignments of a set, satisfying and violating: seeded points of the declared bounds (or of `box`, the
    root intervals [n, 2] in the model's order: what a device state may hold) and the solution rows nearest to hand
    -> (rows in model order [k, n], points in C1 .. Cn order [k, n])"""
    _, preds, bounds = generate_set(name)
    rng = np.random.default_rng(seed)
    if box is not None:
        bounds = [(int(box[c, 0]), int(box[c, 1])) for c in columns]
    pts = np.stack([rng.integers(lo, hi + 1, size=count) for lo, hi in bounds], 1).astype(np.int64)
    sol = solution_rows(name, columns)[:count]
    if len(sol):
        pts = np.concatenate([pts, sol[:, columns]])
    rows = np.zeros_like(pts)
    rows[:, columns] = pts
    return rows, pts


def truth(pred, x):
    """the interval the reference gives a clause at the complete assignment x: 1 or 0, or [0, 1] where a compared side
    is a sentinel"""
    if pred.decided is not None and not bool(pred.decided(x)):
        return (0, 1)
    return (1, 1) if bool(pred(x)) else (0, 0)


def check_by_sampling(name, columns, states, nodes, status, out, per=2000, seed=21):
    """the same two properties where the cross product cannot be enumerated: `per` seeded points of the box below every
    node, drawn around the planted point, those of them that satisfy every predicate -> (instances with a satisfying point, satisfying points in all)"""
    _, preds, bounds = generate_set(name)
    rng = np.random.default_rng(seed)
    dom = below(states, nodes).astype(np.int64)
    planted = np.zeros(dom.shape[1], dtype=np.int64)
    planted[columns] = preds.planted
    hit = total = 0
    for i in range(len(nodes)):
        if (dom[i, :, 0] > dom[i, :, 1]).any():
            assert status[i] < 0
            continue
        rows = rng.integers(dom[i, :, 0], dom[i, :, 1] + 1, size=(per, dom.shape[1]))
        # uniform points rarely satisfy thirty clauses: three coordinates in four take the planted value where the box
        # still holds it
        inside = (planted >= dom[i, :, 0]) & (planted <= dom[i, :, 1])
        take = (rng.random(rows.shape) < 0.75) & inside
        rows[take] = np.broadcast_to(planted, rows.shape)[take]
        ok = np.ones(per, dtype=bool)
        x = [rows[:, c] for c in columns]
        for p in preds:
            ok &= p(x)
        rows = rows[ok]
        hit += bool(len(rows))
        total += len(rows)
        if status[i] < 0:
            assert not len(rows), ("a failed node has a solution below it", nodes[i].tolist(), rows[:1].tolist())
        else:
            assert contained(rows, out[i]).all(), ("the fixpoint loses a solution", nodes[i].tolist())
    return hit, total


def host_tables(text, domains, fast_paths=True, normalize=True):
    """the product's tables for `text` from the given root domains, built on the host -> (clauses, device_info());
    normalize=False: of the trees as the front end built them, which the first sweep of the root phase runs on"""
    from csolve_amd.solver import Model, set_linear_fast_paths
    try:
        set_linear_fast_paths(fast_paths)
        m = Model.from_text(text)
        m.set_domains(domains)
        if normalize:
            m.normalize()
        m.build_tables()
    finally:
        set_linear_fast_paths(True)
    return m.n_clauses, m.device_info()


def clauses_per_lane(clauses):
    """kernel 6's instantiation for a model of so many clauses: 1, 2, 4 or 8 per lane of a wave, None beyond 512"""
    per = (clauses + 63) // 64
    return None if per > 8 else next(c for c in (1, 2, 4, 8) if per <= c)


def derive(name, inst=None):
    """everything RECORDED holds for a set, from the generator, the host tables, the oracle and the brute force"""
    import search_sets as S
    text, preds, bounds = generate_set(name)
    inst = inst or instances(name)
    om = inst["model"]
    clauses, on = host_tables(text, om.domains())
    _, off = host_tables(text, om.domains(), fast_paths=False)
    rec = {
        "vars": len(bounds), "clauses": clauses, "tree": on["tree_clauses"], "ne": on["ne_clauses"],
        "linear_or2": clauses - on["skipped_clauses"] - on["ne_clauses"] - on["tree_clauses"], "tree_off": off["tree_clauses"],
        "longest": on["max_tree"], "cpl": clauses_per_lane(clauses), "width": sum(hi - lo + 1 for lo, hi in bounds),
        "instances": len(inst["nodes"]), "failed": int((inst["status"] < 0).sum()), "props": int(inst["props"].max()),
    }
    if name in SEARCHED:
        st, found, _ = S.reference_walk(text)
        rec["search"] = (st["nodes"], st["cuts"], st["solutions"])
    return rec


# what test_tree_sets_host.py derives for every set on the host (derive(); nothing here comes from the device):
#   vars; clauses of the tables, the objective's constant and the 2 n bound clauses included; tree / ne / linear_or2: the
#   clause kinds left after the root phase under the default fast paths; tree_off: trees with the fast paths off; longest:
#   nodes of the longest tree; cpl: kernel 6's clauses per lane (None: beyond its 512 clauses); width: the sum of the
#   declared widths, which bounds the propagations of any node; instances / failed: the recorded nodes (instances()) and
#   those the oracle fails; props: the oracle's largest PROPS on them; search: nodes, cuts, solutions of the ALL tree
RECORDED = {
    "narrow_mul": {"vars": 6, "clauses": 22, "tree": 9, "ne": 0, "linear_or2": 0, "tree_off": 9, "longest": 8, "cpl": 1, "width": 23, "instances": 2193, "failed": 374, "props": 3, "search": (117, 28, 60)},
    "narrow_neg": {"vars": 6, "clauses": 22, "tree": 8, "ne": 0, "linear_or2": 0, "tree_off": 8, "longest": 11, "cpl": 1, "width": 29, "instances": 2193, "failed": 565, "props": 8, "search": (153, 21, 96)},
    "narrow_eq": {"vars": 6, "clauses": 22, "tree": 9, "ne": 0, "linear_or2": 0, "tree_off": 9, "longest": 10, "cpl": 1, "width": 33, "instances": 2193, "failed": 218, "props": 10, "search": (2662, 748, 1359)},
    "narrow_or3": {"vars": 6, "clauses": 21, "tree": 8, "ne": 0, "linear_or2": 0, "tree_off": 8, "longest": 16, "cpl": 1, "width": 27, "instances": 2193, "failed": 221, "props": 5, "search": (1830, 396, 1072)},
    "narrow_bool": {"vars": 6, "clauses": 23, "tree": 9, "ne": 0, "linear_or2": 1, "tree_off": 10, "longest": 16, "cpl": 1, "width": 27, "instances": 2193, "failed": 168, "props": 10, "search": (138, 22, 75)},
    "narrow_mixed": {"vars": 7, "clauses": 29, "tree": 12, "ne": 0, "linear_or2": 1, "tree_off": 13, "longest": 16, "cpl": 1, "width": 33, "instances": 2193, "failed": 762, "props": 9, "search": (50, 8, 28)},
    "twice6": {"vars": 6, "clauses": 21, "tree": 8, "ne": 0, "linear_or2": 0, "tree_off": 8, "longest": 7, "cpl": 1, "width": 28, "instances": 2193, "failed": 462, "props": 5, "search": (376, 58, 230)},
    "twice5": {"vars": 5, "clauses": 20, "tree": 9, "ne": 0, "linear_or2": 0, "tree_off": 9, "longest": 7, "cpl": 1, "width": 26, "instances": 2193, "failed": 764, "props": 4, "search": (212, 33, 138)},
    "sat_prod": {"vars": 14, "clauses": 59, "tree": 17, "ne": 4, "linear_or2": 8, "tree_off": 25, "longest": 10, "cpl": 1, "width": 664, "instances": 2193, "failed": 499, "props": 4},
    "mixed40": {"vars": 40, "clauses": 181, "tree": 50, "ne": 1, "linear_or2": 16, "tree_off": 66, "longest": 14, "cpl": 4, "width": 177, "instances": 2193, "failed": 864, "props": 18},
    "mixed120": {"vars": 120, "clauses": 501, "tree": 86, "ne": 17, "linear_or2": 47, "tree_off": 133, "longest": 17, "cpl": 8, "width": 548, "instances": 2193, "failed": 669, "props": 38},
    "bigtab": {"vars": 1100, "clauses": 4801, "tree": 341, "ne": 424, "linear_or2": 693, "tree_off": 1034, "longest": 17, "cpl": None, "width": 3293, "instances": 2193, "failed": 39, "props": 71},
    "longsum": {"vars": 127, "clauses": 417, "tree": 2, "ne": 26, "linear_or2": 46, "tree_off": 48, "longest": 256, "cpl": 8, "width": 320, "instances": 2193, "failed": 117, "props": 180},
    "longsum_prefix": {"vars": 12, "clauses": 37, "tree": 2, "ne": 1, "linear_or2": 6, "tree_off": 8, "longest": 26, "cpl": 1, "width": 32, "instances": 2193, "failed": 134, "props": 18, "search": (183, 8, 91)},
}
