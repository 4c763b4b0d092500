"""The learnt-conflict sets of the conflict-clause tests (a helper module, no test itself): seeded models with finite
declared bounds, twelve conflict clauses ("not all of var_i == value_i", CS_OP_CONFL) on each, the instances -- walks
ALONG a clause, which is what makes a conflict clause act -- and the STRONG reference that judges them.

The reference's propagate_confl (propagate.c:395-471) infers but never fails: with every element at its conflict value it
answers PROP_NONE, so the operator is not monotone and its fixpoint depends on the order of the revisions.  strong()
below is a monotone operator instead: alternate, until nothing moves, (1) the oracle's fixpoint of the model WITHOUT its
conflict clauses and (2) one pass over the conflict clauses in which a clause with an element at another value holds, a
clause with no open element fails the node, a clause with exactly one open element whose conflict value sits on a bound
moves that bound by one, and an emptied domain fails the node.  Its result S does not depend on any order, and for every
fair order of the weak propagators (the oracle's depth-first one, the device's rounds):

  * S consistent  ->  the result is consistent and equals S bound for bound (no state on the way can have a clause fully
    at its conflict values: S lies inside every such state and would itself fail, so weak and strong revisions coincide);
  * S failed      ->  the result is failed, or consistent with at least one conflict clause fully at its conflict values
    (a consistent state without a violated clause would be a common fixpoint inside the node, which S says is not there).

judge() asserts exactly that, for every instance; none is left out.  Every number of RECORDED comes from derive() on the
host (test_conflict_sets_host.py re-derives it); nothing here comes from a device."""
import functools
import os
import sys
import zlib

import numpy as np

from csolve_amd import problems

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import search_sets as S  # noqa: E402
import tree_sets as T  # noqa: E402

MAX_TOTAL_WIDTH = 4096
MAX_CONFLICT = T.MAX_TREE_NODES - 1  # elements of the longest clause the device takes: 1 + count == CS_MAX_TREE_NODES
CONFLICTS = 12                       # per set: three special ones and nine drawn
BATCHES = (1, 63, 64, 65)            # and the rest of a set's instances in one more batch
TARGET = 2000                        # instances per set, about
CLASSES = ("shave_lo", "shave_hi", "interior", "two_open", "stopped", "violated", "chain")
CLASS_MINIMUM = 50


# ---- the strong reference ----------------------------------------------------------------------------------------

def clause_state(dom, clause):
    """-> (kind, position): "stopped" (an element at another value), "violated" (no element open, all at their conflict
    values), "two_open", or "unit" with the position of the one open element"""
    first = -1
    opened = 0
    for k, (v, cv) in enumerate(clause):
        lo, hi = dom[v]
        if lo == hi:
            if lo != cv:
                return "stopped", k
        else:
            opened += 1
            if first < 0:
                first = k
    if opened == 0:
        return "violated", -1
    return ("unit", first) if opened == 1 else ("two_open", first)


def strong(base_oracle, clauses, row):
    """the strong reference on one row [n, 2] -> (failed, fixpoint, classes): see the module's docstring.  classes: what
    the conflict clauses did on the way (CLASSES; none of them: base_only)"""
    dom = np.array(row, dtype=np.int32)
    seen = set()
    could_act = None  # the clauses that can act before any conflict clause has: a later actor was made to by a shave
    shaved_by = set()
    while True:
        st, dom = base_oracle.instance(dom, -1, 0, 0)
        if st < 0:
            return True, dom, seen
        if could_act is None:
            could_act = set()
            for ci, c in enumerate(clauses):
                kind, k = clause_state(dom, c)
                if kind == "violated" or (kind == "unit" and c[k][1] in (int(dom[c[k][0], 0]), int(dom[c[k][0], 1]))):
                    could_act.add(ci)
        moved = False
        for ci, c in enumerate(clauses):
            kind, k = clause_state(dom, c)
            if kind != "unit":
                seen.add(kind)
                if kind == "violated":
                    if ci not in could_act and shaved_by - {ci}:
                        seen.add("chain")
                    return True, dom, seen
                continue
            v, cv = c[k]
            if dom[v, 0] == cv:
                dom[v, 0] += 1
                seen.add("shave_lo")
            elif dom[v, 1] == cv:
                dom[v, 1] -= 1
                seen.add("shave_hi")
            else:
                if dom[v, 0] < cv < dom[v, 1]:
                    seen.add("interior")
                continue
            moved = True
            if ci not in could_act and shaved_by - {ci}:
                seen.add("chain")
            shaved_by.add(ci)
            if dom[v, 0] > dom[v, 1]:
                return True, dom, seen
        if not moved:
            return False, dom, seen


def violated(dom, clauses):
    """is some conflict clause fully at its conflict values in the state `dom`"""
    return any(all(dom[v, 0] == dom[v, 1] == cv for v, cv in c) for c in clauses)


def judge(s_failed, s_out, failed, out, clauses, what=None):
    """the two facts, for one instance -> True where the result is the legitimate "S failed, consistent but violated" """
    if not s_failed:
        assert not failed, ("S is consistent, the result failed", what)
        assert (out == s_out).all(), ("S is consistent, the result differs", what, np.nonzero((out != s_out).any(1))[0][:4].tolist())
        return False
    if failed:
        return False
    assert violated(out, clauses), ("S failed, the result is consistent and violates no conflict clause", what)
    return True


# ---- the sets ----------------------------------------------------------------------------------------------------

def _plain_text(title, bounds, lines):
    out = [f"# {title}", "ALL;"] + lines
    for i, (lo, hi) in enumerate(bounds):
        out.append(f"{lo} <= C{i + 1}; C{i + 1} <= {hi};")
    return "\n".join(out) + "\n"


def _wide_negative():
    """ten variables of 280 to 320 values, below zero and straddling it, binary relations and a few trees around one
    planted point"""
    rng = problems.LCG(77003)
    bounds = []
    for i in range(10):
        w = 280 + rng.below(41)
        lo = (-150 - rng.below(40)) if i % 3 == 0 else (-700 - rng.below(300))
        bounds.append((lo, lo + w - 1))
    b = T._Builder(rng, bounds, 2)
    for shape in ("lt", "le", "ne", "or2", "twice_add", "ne_sum", "lt", "ne", "le", "or2", "ne", "neg_sum", "lt", "ne"):
        b.clause(shape)
    return b.text("wide negative: 10 variables of some 300 values below and around zero"), b.preds, bounds


def _long255():
    """256 variables of [0, 2] and a few != between them"""
    bounds = [(0, 2)] * 256
    pairs = [(1, 2, 1), (4, 9, 1), (30, 200, 2), (255, 17, 2), (128, 64, 2)]  # C<a> != C<b> + d, true at C<i> = (i - 1) % 3
    lines, preds = [], T._Predicates()
    for a, b, d in pairs:
        lines.append(f"C{a} != C{b} + {d};")
        preds.append(T._pred(lambda x, a=a, b=b, d=d: x[a - 1] != x[b - 1] + d, "ne"))
    preds.planted = tuple(i % 3 for i in range(256))
    assert all(p(preds.planted) for p in preds)
    return _plain_text("long255: 256 variables of [0, 2]", bounds, lines), preds, bounds


def _queens12():
    return problems.queens(12, "ALL"), None, None


def _oracle_model(text, domains=None):
    """the oracle's model of `text`, normalised like the product's tables and indexed, on `domains` (by default its own
    root fixpoint)"""
    from oracle.cs_oracle import Model as OModel, Oracle
    if domains is None:
        om = OModel.parse(text)
        o0 = Oracle(om)
        o0.set_root_phase(True)
        assert o0.propagate(om.root, 1 << 20) >= 0
        domains = o0.domains()
    om = OModel.parse(text)
    om.set_domains(domains)
    om.normalize()
    om.index()
    return om


# name -> how the base model is made, the kind of its drawn clauses (arbitrary: any clause the planted row does not
# violate; implied: consistent dives of the base oracle with no solution below them; long: three clauses of 255 elements
# and short ones of mixed values; learnt: the decisions of failed nodes of an oracle walk), whether the cross product of
# its bounds is enumerated, and the classes its instances cannot reach by construction.  queens12_learnt: the base model
# fails wherever all elements of a clause have their conflict values, so step (1) of the strong reference fails before
# step (2) can find the clause violated; and it has no linked pair (_linked): a two-element clause of a failed queens
# node is a pair of attacking queens, which the base model's `!=` shaves first, so such a clause never acts
# Conflict values one below or above the root domain and negative ones are drawn for the arbitrary and the long sets
# (one clause in four holds one); narrow_implied and queens12_learnt cannot hold them: their drawn clauses are decisions
# the base model's propagation accepted (or, learnt, made), which lie inside the domains, and queens has no value below 1.
# long255 never qualifies for kernel 6 (its 512 bound clauses alone are past the limit): clauses at the element limit
# run on kernel 1 only.
SETS = {
    "narrow_implied": dict(base=lambda: S.generate(n=6, seed=7, width=9, plant=True, slack=1, clauses=14), kind="implied", brute=True),
    "narrow_arbitrary": dict(base=lambda: S.generate(n=7, seed=4, width=7, plant=True, slack=2, clauses=10), kind="arbitrary", brute=True),
    "wide_negative": dict(base=_wide_negative, kind="arbitrary", interior=True),
    "mixed_trees": dict(base=lambda: T.generate(**T.SETS["narrow_mixed"]["args"]), kind="arbitrary", brute=True),
    "k6_cpl2": dict(base=lambda: T.generate(n=20, seed=7, shapes=T.FAMILIES, clauses=20, plain=40, slack=4, width=(4, 8)), kind="arbitrary"),
    "k6_cpl4": dict(base=lambda: T.generate(n=40, seed=4, shapes=T.FAMILIES, clauses=40, plain=40, slack=4, width=(4, 8)), kind="arbitrary"),
    "k6_cpl8": dict(base=lambda: T.generate(n=80, seed=5, shapes=T.FAMILIES, clauses=90, plain=40, slack=4, width=(4, 8)), kind="arbitrary"),
    "across512": dict(base=lambda: T.generate(n=100, seed=6, shapes=("lt", "le", "ne", "or2", "or3", "ne_sum"), clauses=304,
                                              width=(2, 4), slack=2), kind="arbitrary"),
    "long255": dict(base=_long255, kind="long"),
    "queens12_learnt": dict(base=_queens12, kind="learnt", unreachable=("violated", "chain")),
}
NAMES = list(SETS)
K6_CLASSES = ["k6_cpl2", "k6_cpl4", "k6_cpl8"]  # the `k6_classes` family: with narrow_* at one clause per lane
BRUTE = [k for k, v in SETS.items() if v.get("brute")]
NARROW = ["narrow_implied", "narrow_arbitrary"]
TRAILED = NARROW + ["mixed_trees"]
SEARCHED = ["narrow_implied", "queens12_learnt"]
QUEENS12_SOLUTIONS = 14200


def _value(rng, lo, hi, kind):
    """a conflict value for a variable of [lo, hi]: on a bound, inside, one outside, or negative"""
    if kind == "lo":
        return lo
    if kind == "hi":
        return hi
    if kind == "interior" and hi - lo >= 2:
        return lo + 1 + int(rng.integers(hi - lo - 1))
    if kind == "below":
        return lo - 1
    if kind == "above":
        return hi + 1
    if kind == "negative":
        return -1 - int(rng.integers(max(1, -lo + 2))) if lo < 0 else -1 - int(rng.integers(3))
    return lo + int(rng.integers(hi - lo + 1))


def _kinds(rng, count, interior):
    """value kinds of a clause's elements: bounds and interior values; one clause in four has an element off the domain"""
    pool = ("interior",) * 6 + ("lo", "hi") if interior else ("lo", "hi", "interior", "lo", "hi", "any")
    kinds = [pool[int(rng.integers(len(pool)))] for _ in range(count)]
    if rng.integers(4) == 0:
        kinds[int(rng.integers(count))] = ("below", "above", "negative")[int(rng.integers(3))]
    return kinds


def _arbitrary(rng, root, planted, interior):
    """a clause of 1 to 6 elements on different open variables which the planted row does not violate"""
    open_vars = np.nonzero(root[:, 0] < root[:, 1])[0]
    while True:
        k = 2 + int(rng.integers(min(5, len(open_vars) - 1)))
        vs = rng.choice(open_vars, size=k, replace=False)
        c = [(int(v), _value(rng, int(root[v, 0]), int(root[v, 1]), kind)) for v, kind in zip(vs, _kinds(rng, k, interior))]
        if any(planted[v] != cv for v, cv in c):
            return c


def _implied(rng, orc, root, rows):
    """a clause no solution row violates although the base model's propagation accepts the whole partial assignment: a
    seeded dive of the base oracle that stays consistent and has no solution below it (what a learnt clause is)"""
    for attempt in range(4000):
        k = 2 + int(rng.integers(4))
        dom, c = root, []
        for kind in _kinds(rng, k, False):
            open_vars = np.nonzero(dom[:, 0] < dom[:, 1])[0]
            if len(open_vars) == 0:
                break
            v = int(rng.choice(open_vars))
            cv = _value(rng, int(dom[v, 0]), int(dom[v, 1]), kind if kind in ("lo", "hi", "interior") else "any")
            st, out = orc.instance(dom, v, cv, cv)
            if st < 0:
                break
            dom = out
            c.append((v, cv))
        else:
            if len(c) >= 2 and not T.contained(rows, dom).any():
                return c
    raise AssertionError("no implied clause found")


def _linked(rng, orc, root, accept):
    """two clauses made to act one after the other: A = [(p, a), (x, c)] and B = [(x, c + 1), (q, b)] with b on a bound
    of q -- once x is down to [c, c + 1] and p is a, A shaves c off x, x is c + 1, and B shaves b off q.  accept(clause):
    may the set hold it.  The pair is tried from the root row before it is taken"""
    open_vars = np.nonzero(root[:, 0] < root[:, 1])[0]
    for attempt in range(20000):
        p, x, q = (int(v) for v in rng.choice(open_vars, size=3, replace=False))
        if root[x, 1] - root[x, 0] < 2:
            continue
        c = int(rng.integers(root[x, 0], root[x, 1]))
        a = int(rng.integers(root[p, 0], root[p, 1] + 1))
        b = int(root[q, int(rng.integers(2))])
        A, B = [(p, a), (x, c)], [(x, c + 1), (q, b)]
        if not (accept(A) and accept(B)):
            continue
        row = root.copy()
        row[x] = (c, c + 1)
        failed, row, _ = strong(orc, [A, B], row)
        if failed or tuple(row[x]) != (c, c + 1) or row[p, 0] == row[p, 1]:
            continue
        row[p] = (a, a)
        failed, row, seen = strong(orc, [A, B], row)
        if not failed and "chain" in seen:
            return A, B
    raise AssertionError("no linked pair found")


def _one_element(rng, root, allowed):
    """a one-element clause (var, value) that `allowed(var, value)` accepts: an interior value where there is one"""
    open_vars = [int(v) for v in np.nonzero(root[:, 0] < root[:, 1])[0]]
    for inner in (True, False):
        for v in rng.permutation(open_vars):
            lo, hi = int(root[v, 0]), int(root[v, 1])
            values = list(range(lo + 1, hi)) if inner else [lo, hi]
            for cv in rng.permutation(values) if values else []:
                if allowed(int(v), int(cv)):
                    return [(int(v), int(cv))]
    v = open_vars[0]
    return [(v, int(root[v, 1]) + 1)]


def _learnt(rng, orc, root, count):
    """the decisions of failed nodes of seeded walks of the base oracle, two to six of them: implied clauses"""
    out = []
    while len(out) < count:
        dom, path = root, []
        for _ in range(6):
            open_vars = np.nonzero(dom[:, 0] < dom[:, 1])[0]
            v = int(rng.choice(open_vars))
            cv = int(dom[v, 0]) if rng.integers(3) == 0 else (int(dom[v, 1]) if rng.integers(2) else int(rng.integers(dom[v, 0], dom[v, 1] + 1)))
            path.append((v, cv))
            st, nxt = orc.instance(dom, v, cv, cv)
            if st < 0:
                if len(path) >= 2 and path not in out:
                    out.append(list(path))
                break
            dom = nxt
    return out


@functools.lru_cache(maxsize=None)
def build(name):
    """everything about a set that needs no device -> dict: text, preds / bounds (C1 .. Cn order; None for queens),
    columns, plain / full (the oracle's normalised indexed models without and with the conflict clauses, both on the root
    row), plain_oracle / full_oracle, clauses [[(model variable, value)]], root (the strong reference's root row), rows
    (brute-forced sets: the base model's solutions in the model's variable order), base_clauses"""
    from oracle.cs_oracle import Model as OModel, Oracle
    rec = SETS[name]
    text, preds, bounds = rec["base"]()
    plain = _oracle_model(text)
    plain_oracle = Oracle(plain)
    cols = S.columns(plain.names()) if preds is not None else None
    root0 = plain.domains()
    rng = np.random.default_rng(zlib.crc32(("clauses of " + name).encode()))
    rows = None
    if rec.get("brute"):
        pts = np.array(sorted(S.brute_force(preds, bounds)), dtype=np.int64).reshape(-1, len(bounds))
        assert len(pts) > 0
        rows = np.zeros_like(pts)
        rows[:, cols] = pts
    # the planted row, in the model's order: what no arbitrary clause may violate
    if rows is not None:
        planted = rows[len(rows) // 2]
    elif preds is not None:
        planted = np.zeros(len(bounds), dtype=np.int64)
        planted[cols] = preds.planted
    else:
        planted = None
    interior = bool(rec.get("interior"))
    kind = rec["kind"]
    clauses, linked = [], None
    if kind == "arbitrary":
        clauses = [_arbitrary(rng, root0, planted, interior) for _ in range(CONFLICTS - 5)]
        clauses += _linked(rng, plain_oracle, root0, lambda c: any(planted[v] != cv for v, cv in c))
        one = _one_element(rng, root0, lambda v, cv: planted[v] != cv)
    elif kind == "implied":
        clauses = [_implied(rng, plain_oracle, root0, rows) for _ in range(CONFLICTS - 5)]
        clauses += _linked(rng, plain_oracle, root0, lambda c: not np.all([rows[:, v] == cv for v, cv in c], axis=0).any())
        one = _one_element(rng, root0, lambda v, cv: not (rows[:, v] == cv).any())
    elif kind == "learnt":
        clauses = _learnt(rng, plain_oracle, root0, CONFLICTS - 3)
        one = _one_element(rng, root0, lambda v, cv: plain_oracle.instance(root0, v, cv, cv)[0] < 0)
    else:  # long255: 255 elements at 0, at 2 and at 1 (the planted row has every value in each), and six short ones
        n = len(bounds)
        clauses = [[(cols[i], 0) for i in range(MAX_CONFLICT)], [(cols[i], 2) for i in range(1, n)],
                   [(cols[i], 1) for i in range(MAX_CONFLICT)]]
        # the short ones hold two different values each, so that a walk along a long clause (every variable at one
        # value) cannot violate them, and the one-element clause sits on the variable the clause "at 1" leaves out
        def mixed(c):
            return any(planted[v] != cv for v, cv in c) and len({cv for _, cv in c}) > 1
        while len(clauses) < CONFLICTS - 5:
            c = _arbitrary(rng, root0, planted, False)
            if mixed(c):
                clauses.append(c)
        clauses += _linked(rng, plain_oracle, root0, mixed)
        one = [(cols[n - 1], 1)]
    # a variable twice at one value, a variable twice at two values (such a clause always holds), one element
    # of the shortest drawn clause (what holds of it holds of both)
    if kind != "learnt":
        linked = (len(clauses) - 2, len(clauses) - 1)
    short = min((c for c in clauses[: CONFLICTS - 5] if len(c) >= 2), key=len)
    (v0, c0) = short[0]
    same = short[:5] + [(v0, c0)]
    other = int(root0[v0, 0]) if c0 != int(root0[v0, 0]) else int(root0[v0, 1])
    different = short[:2] + [(v0, other)]
    clauses = clauses + [same, different, one]
    assert len(clauses) == CONFLICTS

    def oracle_model(with_clauses, domains):
        om = OModel.parse(text)
        om.set_domains(root0)
        om.normalize()
        if with_clauses:
            for c in clauses:
                om.append_clause(om.add_confl([(om.var_node(v), cv) for v, cv in c]))
        om.set_domains(domains)
        om.index()
        return om

    failed, root, _ = strong(plain_oracle, clauses, root0)
    assert not failed, "the conflict clauses make the root inconsistent"
    plain, full = oracle_model(False, root), oracle_model(True, root)
    assert full.n_clauses == plain.n_clauses + CONFLICTS
    return dict(name=name, text=text, preds=preds, bounds=bounds, columns=cols, plain=plain, full=full, plain_oracle=Oracle(plain),
                full_oracle=Oracle(full), clauses=clauses, linked=linked, root=root, rows=rows, base_clauses=plain.n_clauses, planted=planted)


def save_models(name, directory):
    """the two models as dumps the product loads (Model.from_dump) -> (path with the clauses, path without)"""
    b = build(name)
    paths = os.path.join(directory, name + ".full.model"), os.path.join(directory, name + ".plain.model")
    b["full"].save(paths[0])
    b["plain"].save(paths[1])
    return paths


# ---- the instances -----------------------------------------------------------------------------------------------

def _deviation(rng, dom, v, cv):
    """a node that leaves the walk along a clause at element (v, cv): another value, an interval with the conflict value
    on one of its bounds, or a full re-propagation"""
    lo, hi = int(dom[v, 0]), int(dom[v, 1])
    kind = int(rng.integers(10))
    if kind < 2:
        return (-1, 0, 0)
    if kind < 8 and lo <= cv <= hi:  # the conflict value on a bound of what is left
        if cv == lo or (cv < hi and rng.integers(2)):
            return (v, cv, cv + 1 + int(rng.integers(hi - cv))) if cv < hi else (v, cv, cv)
        return (v, cv - 1 - int(rng.integers(cv - lo)), cv)
    x = lo + int(rng.integers(hi - lo + 1))
    return (v, x, x)


@functools.lru_cache(maxsize=None)
def instances(name, target=TARGET):
    """-> dict: states [P, n, 2] (the parent of a value or interval node is a consistent fixpoint of the strong
    reference; the parent of a var = -1 node is such a fixpoint with one interval narrowed and nothing propagated), nodes [B, 4] in batches of
    BATCHES and the rest, failed [B] / out [B, n, 2] / classes [B] (the strong reference), status / weak / props (the
    oracle with the clauses in its model: its verdict, its end state, its PROPS)"""
    b = build(name)
    clauses, base, full = b["clauses"], b["plain_oracle"], b["full_oracle"]
    rng = np.random.default_rng(zlib.crc32(("walks of " + name).encode()))
    states, nodes, failed, outs, classes = [b["root"]], [], [], [], []

    def node(parent, v, lo, hi):
        """record one instance -> the row of its fixpoint among the states, or -1 where it failed"""
        row = states[parent].copy()
        if v >= 0:
            row[v] = (lo, hi)
        f, out, seen = strong(base, clauses, row)
        nodes.append((v, lo, hi, parent))
        failed.append(f)
        outs.append(out)
        classes.append(frozenset(seen))
        if f:
            return -1
        states.append(out)
        return len(states) - 1

    def prefix(clause, order, keep):
        """a parent with all but the last `keep` elements of a long clause at their conflict values (not an instance)"""
        row = b["root"].copy()
        for k in order[:-keep]:
            v, cv = clause[k]
            row[v] = (cv, cv)
        f, out, _ = strong(base, clauses, row)
        if f:  # a short clause of the set is violated by so many variables at one value
            return -1
        states.append(out)
        return len(states) - 1

    def chain_walk():
        """the linked pair: a short dive on other variables, x down to the two values, then A's other element"""
        A, B = (clauses[i] for i in b["linked"])
        (p, a), (x, c) = A
        q = B[1][0]
        cur = 0
        for _ in range(int(rng.integers(3))):
            dom = states[cur]
            others = [v for v in np.nonzero(dom[:, 0] < dom[:, 1])[0] if v not in (p, x, q)]
            if not others:
                break
            v = int(rng.choice(others))
            y = int(rng.integers(dom[v, 0], dom[v, 1] + 1))
            cur = node(cur, v, y, y)
            if cur < 0:
                return
        dom = states[cur]
        if dom[x, 0] <= c and c + 1 <= dom[x, 1] and dom[x, 1] - dom[x, 0] >= 2:
            cur = node(cur, x, c, c + 1)
            if cur < 0:
                return
            dom = states[cur]
        if dom[p, 0] <= a <= dom[p, 1] and dom[p, 0] < dom[p, 1]:
            node(cur, p, a, a)

    while len(nodes) < target:
        cur = 0
        if b["linked"] is not None and rng.integers(8) == 0:
            chain_walk()
            continue
        if rng.integers(4) == 0:  # a plain dive
            for _ in range(6):
                dom = states[cur]
                open_vars = np.nonzero(dom[:, 0] < dom[:, 1])[0]
                if len(open_vars) == 0:
                    break
                v = int(rng.choice(open_vars))
                x = int(rng.integers(dom[v, 0], dom[v, 1] + 1))
                if rng.integers(6) == 0:  # unpropagated, as a row of its own: a full re-propagation
                    row = dom.copy()
                    row[v] = (x, min(int(dom[v, 1]), x + int(rng.integers(2))))
                    states.append(row)
                    node(len(states) - 1, -1, 0, 0)
                    break
                cur = node(cur, v, x, x)
                if cur < 0 or rng.integers(4) == 0:
                    break
            continue
        c = clauses[int(rng.integers(len(clauses)))]
        order = [int(k) for k in rng.permutation(len(c))]
        if len(c) > 8:
            keep = 2 + int(rng.integers(3))
            cur = prefix(c, order, keep)
            if cur < 0:
                continue
            order = order[-keep:]
        # where the walk leaves the clause: at its last element (every other one then has its conflict value), never
        # (the clause ends violated), or anywhere
        leave = (len(order) - 1, len(order) - 1, len(order), len(order), len(order), int(rng.integers(len(order) + 1)))[int(rng.integers(6))]
        for step, k in enumerate(order):
            v, cv = c[k]
            dom = states[cur]
            if dom[v, 0] == dom[v, 1]:
                if dom[v, 0] != cv:
                    break
                continue
            if step == leave:
                d = _deviation(rng, dom, v, cv)
                if d[0] < 0:  # the narrowing written into a row of its own, and that row re-propagated in full
                    while d[0] < 0:
                        d = _deviation(rng, dom, v, cv)
                    row = dom.copy()
                    row[d[0]] = d[1:]
                    states.append(row)
                    node(len(states) - 1, -1, 0, 0)
                else:
                    node(cur, *d)
                break
            if not dom[v, 0] <= cv <= dom[v, 1]:
                break
            cur = node(cur, v, cv, cv)
            if cur < 0:
                break
    nodes = np.array(nodes, dtype=np.int32)
    states = np.ascontiguousarray(np.stack(states), dtype=np.int32)
    status = np.empty(len(nodes), dtype=np.int64)
    props = np.empty(len(nodes), dtype=np.int64)
    weak = np.empty((len(nodes),) + states.shape[1:], dtype=np.int32)
    for i, (v, lo, hi, p) in enumerate(nodes):
        status[i], weak[i] = full.instance(states[p], int(v), int(lo), int(hi))
        props[i] = full.props()
    return dict(states=states, nodes=nodes, failed=np.array(failed), out=np.stack(outs).astype(np.int32), classes=classes,
                status=status, weak=weak, props=props)


def batches(count):
    """the batch sizes of a set's `count` instances: 1, 63, 64, 65 and the rest"""
    return BATCHES + (count - sum(BATCHES),)


def class_counts(classes):
    out = {k: sum(k in s for s in classes) for k in CLASSES}
    out["base_only"] = sum(not (s - {"two_open", "stopped"}) for s in classes)
    return out


def solutions_below(name, dom):
    """brute-forced sets: which solution rows of model AND clauses lie inside the intervals `dom`"""
    b = build(name)
    rows = b["rows"]
    ok = T.contained(rows, dom)
    for c in b["clauses"]:
        ok &= ~np.all([rows[:, v] == cv for v, cv in c], axis=0)
    return ok


def derive(name):
    """everything RECORDED holds for a set"""
    b, inst = build(name), instances(name)
    root = b["root"]
    viol = sum(bool(f) and st >= 0 for f, st in zip(inst["failed"], inst["status"]))
    return {"vars": int(b["plain"].n_vars), "base_clauses": int(b["base_clauses"]), "clauses": int(b["full"].n_clauses),
            "cpl_base": T.clauses_per_lane(b["base_clauses"]), "cpl": T.clauses_per_lane(b["full"].n_clauses),
            "width": int((root[:, 1].astype(np.int64) - root[:, 0] + 1).sum()), "longest_conflict": max(len(c) for c in b["clauses"]),
            "instances": len(inst["nodes"]), "failed": int(inst["failed"].sum()), "oracle_violated": int(viol),
            "props": int(inst["props"].max()), "classes": class_counts(inst["classes"])}


below = T.below


def search_walk(name):
    """the ALL trees of the oracle-backed engine of cpu_engine.py from the set's root row, with the conflict clauses in
    the model and without -> {"with": (nodes, cuts, solutions), "without": the same, "found": the same solution sets}"""
    import torch
    from cpu_engine import OracleEngine
    b = build(name)
    out, found = {}, {}
    for key in ("with", "without"):
        eng = OracleEngine(b["full" if key == "with" else "plain"], parents_per_iteration=64)
        eng.put(torch.from_numpy(b["root"]).unsqueeze(0).contiguous())
        st = eng.run(1 << 40)
        assert st["done"] == 1 and eng.complete_false == 0
        out[key] = (st["nodes"], st["cuts"], st["solutions"])
        found[key] = {tuple(int(x) for x in row) for row in eng.found}
    out["found"] = found["with"] == found["without"] and len(found["with"]) == out["with"][2]
    if b["rows"] is not None:
        out["found"] = out["found"] and found["with"] == {tuple(int(x) for x in r) for r in b["rows"]}
    return out


RECORDED = {
    "narrow_implied": {'vars': 6, 'base_clauses': 25, 'clauses': 37, 'cpl_base': 1, 'cpl': 1, 'width': 42, 'longest_conflict': 3, 'instances': 2001, 'failed': 511, 'oracle_violated': 125, 'props': 12, 'classes': {'shave_lo': 125, 'shave_hi': 393, 'interior': 1371, 'two_open': 1302, 'stopped': 1468, 'violated': 222, 'chain': 286, 'base_only': 398}},
    "narrow_arbitrary": {'vars': 7, 'base_clauses': 24, 'clauses': 36, 'cpl_base': 1, 'cpl': 1, 'width': 35, 'longest_conflict': 6, 'instances': 2000, 'failed': 117, 'oracle_violated': 98, 'props': 8, 'classes': {'shave_lo': 344, 'shave_hi': 186, 'interior': 1051, 'two_open': 1788, 'stopped': 1896, 'violated': 98, 'chain': 122, 'base_only': 493}},
    "wide_negative": {'vars': 10, 'base_clauses': 35, 'clauses': 47, 'cpl_base': 1, 'cpl': 1, 'width': 2480, 'longest_conflict': 6, 'instances': 2001, 'failed': 272, 'oracle_violated': 169, 'props': 7, 'classes': {'shave_lo': 147, 'shave_hi': 66, 'interior': 969, 'two_open': 1802, 'stopped': 1829, 'violated': 169, 'chain': 74, 'base_only': 674}},
    "mixed_trees": {'vars': 7, 'base_clauses': 29, 'clauses': 41, 'cpl_base': 1, 'cpl': 1, 'width': 29, 'longest_conflict': 6, 'instances': 2000, 'failed': 775, 'oracle_violated': 103, 'props': 10, 'classes': {'shave_lo': 175, 'shave_hi': 286, 'interior': 511, 'two_open': 1302, 'stopped': 1251, 'violated': 103, 'chain': 77, 'base_only': 1009}},
    "k6_cpl2": {'vars': 20, 'base_clauses': 61, 'clauses': 73, 'cpl_base': 1, 'cpl': 2, 'width': 111, 'longest_conflict': 6, 'instances': 2002, 'failed': 119, 'oracle_violated': 108, 'props': 7, 'classes': {'shave_lo': 271, 'shave_hi': 123, 'interior': 1732, 'two_open': 1981, 'stopped': 1745, 'violated': 108, 'chain': 102, 'base_only': 129}},
    "k6_cpl4": {'vars': 40, 'base_clauses': 121, 'clauses': 133, 'cpl_base': 2, 'cpl': 4, 'width': 204, 'longest_conflict': 6, 'instances': 2001, 'failed': 420, 'oracle_violated': 254, 'props': 15, 'classes': {'shave_lo': 192, 'shave_hi': 400, 'interior': 1582, 'two_open': 1819, 'stopped': 1267, 'violated': 254, 'chain': 115, 'base_only': 194}},
    "k6_cpl8": {'vars': 80, 'base_clauses': 251, 'clauses': 263, 'cpl_base': 4, 'cpl': 8, 'width': 421, 'longest_conflict': 5, 'instances': 2002, 'failed': 411, 'oracle_violated': 76, 'props': 11, 'classes': {'shave_lo': 150, 'shave_hi': 292, 'interior': 1547, 'two_open': 1677, 'stopped': 888, 'violated': 76, 'chain': 118, 'base_only': 351}},
    "across512": {'vars': 100, 'base_clauses': 505, 'clauses': 517, 'cpl_base': 8, 'cpl': None, 'width': 215, 'longest_conflict': 6, 'instances': 2001, 'failed': 88, 'oracle_violated': 86, 'props': 35, 'classes': {'shave_lo': 353, 'shave_hi': 257, 'interior': 1838, 'two_open': 1979, 'stopped': 1431, 'violated': 86, 'chain': 107, 'base_only': 39}},
    "long255": {'vars': 256, 'base_clauses': 518, 'clauses': 530, 'cpl_base': None, 'cpl': None, 'width': 768, 'longest_conflict': 255, 'instances': 2000, 'failed': 100, 'oracle_violated': 100, 'props': 2, 'classes': {'shave_lo': 219, 'shave_hi': 273, 'interior': 1763, 'two_open': 1775, 'stopped': 1956, 'violated': 100, 'chain': 101, 'base_only': 77}},
    "queens12_learnt": {'vars': 12, 'base_clauses': 223, 'clauses': 235, 'cpl_base': 4, 'cpl': 4, 'width': 144, 'longest_conflict': 6, 'instances': 2001, 'failed': 275, 'oracle_violated': 0, 'props': 66, 'classes': {'shave_lo': 73, 'shave_hi': 63, 'interior': 263, 'two_open': 1637, 'stopped': 1676, 'violated': 0, 'chain': 0, 'base_only': 1608}},
}
SEARCH = {
    "narrow_implied": {'with': (324, 136, 126), 'without': (330, 141, 126), 'found': True},
    "queens12_learnt": {'with': (500786, 393580, 14200), 'without': (500786, 393580, 14200), 'found': True},
}
