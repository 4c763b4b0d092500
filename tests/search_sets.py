"""The clause-model sets of the search-engine tests (a helper module, no test itself): a seeded generator of models made
of `<`, `<=`, `=`, `!=`, two-literal disjunctions and sums with constant factors -- the schedule and wcet shapes, which an
ALL search walks by branch / emit / general fixpoint kernel / classify / scatter --, the reference walk (the oracle-backed
engine of cpu_engine.py), a brute force over the declared bounds, and the table of named sets with their recorded walks.
Every recorded number comes from reference_walk() and brute_force() on the host, never from the device;
test_search_sets_host.py re-derives all of them."""
import os
import sys

import numpy as np
import torch

from csolve_amd import problems

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

EXPRESSION = (2, 0, 2)  # the wcet-style objective q * C<a+1> + C<b+1> as (q, a, b): "2*C1 + C3"


def _term(name, d):
    return name if d == 0 else f"{name} {'+' if d > 0 else '-'} {abs(d)}"


def generate(n, seed, width=6, wide=0, objective="ALL", clauses=None, sums=True, slack=0, plant=False):
    """-> (text, predicates, bounds): n variables C1 .. Cn, the first `wide` of them with 300 to 1,200 values and the
    others with width - 2 .. width, lower bounds on both sides of zero; `clauses` (2 n by default) seeded constraints of
    the shapes  a < b + d,  a <= b + d,  a = b + d,  a != b + d,  a > b + d | c > e + d2  and, with sums,
    a + b <= c + s  and  q * a + b <= s; the bounds of every variable.  The constants are drawn around the middles of
    the domains (+ slack: looser) or, with plant, so that one seeded hidden point satisfies every constraint with at
    most `slack` to spare -- what keeps a model of hundreds of constraints feasible.  objective: the text before the
    first ";" -- "ALL", "ANY", "MIN C3", "MAX 2*C1 + C3" --, which the constraints do not depend on.  predicates: the
    constraints as functions of a sequence x of the n values (numpy columns work as well), bounds: [(lo, hi)]."""
    rng = problems.LCG(seed * 1000003 + n * 8191 + width * 131 + wide * 17 + (1 if sums else 0))
    name = [f"C{i + 1}" for i in range(n)]
    bounds = []
    for i in range(n):
        if i < wide:
            w = 300 + rng.below(901)
            lo = rng.below(2 * w) - (3 * w) // 2
        else:
            w = max(2, width - rng.below(3))
            lo = rng.below(9) - 5
        bounds.append((lo, lo + w - 1))
    span = [hi - lo + 1 for lo, hi in bounds]
    # the point the constants are drawn around: the middles, or the hidden point
    mid = [lo + rng.below(hi - lo + 1) for lo, hi in bounds] if plant else [(lo + hi) // 2 for lo, hi in bounds]
    lines = [f"# clause model: {n} variables, seed {seed}, width {width}, {wide} wide", f"{objective};"]
    preds = []

    def room(gap, j):
        """the constant of `left <= right + constant`, gap = left - right at the point: about the gap, or, planted, the
        gap and at most `slack` more"""
        if plant:
            return gap + rng.below(slack + 1)
        return gap + rng.below(2 * j + 1) - j + slack

    def around(a, b):
        return room(mid[a] - mid[b], max(2, min(span[a], span[b]) // 2))

    def below_gap(a, b):
        """the d of a literal `a > b + d`: planted, one the hidden point satisfies"""
        if plant:
            return mid[a] - mid[b] - 1 - rng.below(slack + 1)
        return around(a, b) - slack

    for _ in range(2 * n if clauses is None else clauses):
        a, b = rng.below(n), rng.below(n)
        kind = rng.below(12 if sums else 10)
        if a == b:
            continue
        if kind < 3:
            d = around(a, b) + 1
            lines.append(f"{name[a]} < {_term(name[b], d)};")
            preds.append(lambda x, a=a, b=b, d=d: x[a] < x[b] + d)
        elif kind < 5:
            d = around(a, b)
            lines.append(f"{name[a]} <= {_term(name[b], d)};")
            preds.append(lambda x, a=a, b=b, d=d: x[a] <= x[b] + d)
        elif kind < 6:
            d = mid[a] - mid[b] if plant else around(a, b) - slack
            lines.append(f"{name[a]} = {_term(name[b], d)};")
            preds.append(lambda x, a=a, b=b, d=d: x[a] == x[b] + d)
        elif kind < 8:
            d = mid[a] - mid[b] + 1 + rng.below(3) if plant else around(a, b) - slack
            lines.append(f"{name[a]} != {_term(name[b], d)};")
            preds.append(lambda x, a=a, b=b, d=d: x[a] != x[b] + d)
        elif kind < 10:
            c, e = rng.below(n), rng.below(n)
            if c == e:
                continue
            d = below_gap(a, b)
            d2 = mid[c] - mid[e] + rng.below(3) - 1 if plant else around(c, e) - slack
            lines.append(f"{name[a]} > {_term(name[b], d)} | {name[c]} > {_term(name[e], d2)};")
            preds.append(lambda x, a=a, b=b, c=c, e=e, d=d, d2=d2: (x[a] > x[b] + d) | (x[c] > x[e] + d2))
        elif kind < 11:
            c = rng.below(n)
            s = room(mid[a] + mid[b] - mid[c], max(2, min(span[a], span[b], span[c]) // 2))
            lines.append(f"{name[a]} + {name[b]} <= {_term(name[c], s)};")
            preds.append(lambda x, a=a, b=b, c=c, s=s: x[a] + x[b] <= x[c] + s)
        else:
            q = 2 + rng.below(3)
            s = room(q * mid[a] + mid[b], max(2, min(q * span[a], span[b]) // 2))
            lines.append(f"{q} * {name[a]} + {name[b]} <= {s};")
            preds.append(lambda x, q=q, a=a, b=b, s=s: q * x[a] + x[b] <= s)
    for i, (lo, hi) in enumerate(bounds):
        lines.append(f"{lo} <= {name[i]}; {name[i]} <= {hi};")
    return "\n".join(lines) + "\n", preds, bounds


def brute_force(preds, bounds, chunk=1 << 18):
    """every point of the cross product of `bounds` on which all predicates hold -> set of tuples (C1 .. Cn)"""
    n = len(bounds)
    spans = [hi - lo + 1 for lo, hi in bounds]
    total = int(np.prod([float(s) for s in spans]))
    assert total <= 3_000_000, "too many points for a brute force"
    found = set()
    for start in range(0, total, chunk):
        idx = np.arange(start, min(total, start + chunk), dtype=np.int64)
        cols = []
        for i in range(n - 1, -1, -1):  # mixed radix, the last variable fastest
            cols.append(bounds[i][0] + idx % spans[i])
            idx = idx // spans[i]
        cols.reverse()
        ok = np.ones(len(cols[0]), dtype=bool)
        for p in preds:
            ok &= p(cols)
        found.update(zip(*(c[ok].tolist() for c in cols)))
    return found


def oracle_model(text):
    """the oracle's model of `text` after its root phase, indexed -> (model, columns); columns[i] is the index the
    front end gave C<i+1> (variables are numbered in the order the text names them first)"""
    from oracle.cs_oracle import Model as OModel, Oracle
    om = OModel.parse(text)
    o0 = Oracle(om)
    o0.set_root_phase(True)
    if o0.propagate(om.root, 1 << 20) < 0:
        raise ValueError("INFEASIBLE PROBLEM")
    om.set_domains(o0.domains())
    om.index()
    return om, columns(om.names())


def columns(names):
    """model variable names -> the model's index of C1, C2, ... (an expression objective adds a variable of its own)"""
    own = sorted((int(s[1:]), i) for i, s in enumerate(names) if s[0] == "C" and s[1:].isdigit())
    assert [k for k, _ in own] == list(range(1, len(own) + 1)), names
    return [i for _, i in own]


def reference_walk(text, parents_per_iteration=64, shuffle_seed=None):
    """the search of `text` by the oracle-backed engine from the oracle's root fixpoint -> (statistics, solutions as a
    set of tuples (C1 .. Cn), engine); under ALL nodes, cuts and solutions do not depend on the walking order"""
    from cpu_engine import OracleEngine
    om, cols = oracle_model(text)
    eng = OracleEngine(om, parents_per_iteration=parents_per_iteration, shuffle_seed=shuffle_seed)
    eng.put(torch.from_numpy(om.domains()).unsqueeze(0).contiguous())
    st = eng.run(1 << 40)
    assert st["done"] == 1
    return st, {tuple(int(row[c]) for c in cols) for row in eng.found}, eng


def expression_value(x):
    q, a, b = EXPRESSION
    return q * x[a] + x[b]


def expression_text():
    q, a, b = EXPRESSION
    return f"{q}*C{a + 1} + C{b + 1}"


# name -> generator arguments, objective variable (1-based: MIN / MAX C<k>) and what reference_walk() and brute_force()
# gave: the ALL tree (nodes, cuts, solutions, halvings: parents split in two), whether the model keeps expression-tree
# clauses under the default fast paths, min / max of C<k> and of expression_text() over the solution set (None:
# infeasible).  `narrow`: the cross product of the bounds is small enough for brute_force().  wide2_mid is a set whose tree
# changes (5,066 nodes) when the middle of a halved interval with a negative odd lo + hi is rounded toward zero.
SETS = {
    "narrow_sums8": {
        "args": {"n": 8, "seed": 2, "width": 6}, "obj": 3, "narrow": True,
        "nodes": 8061, "cuts": 57, "solutions": 5772, "halvings": 0, "tree": True, "var": (2, 4), "expr": (6, 16)},
    "narrow_plain7": {
        "args": {"n": 7, "seed": 24, "width": 6, "sums": False}, "obj": 3, "narrow": True,
        "nodes": 1672, "cuts": 830, "solutions": 498, "halvings": 0, "tree": False, "var": (1, 4), "expr": (3, 10)},
    "narrow_plain8": {
        "args": {"n": 8, "seed": 28, "width": 6, "sums": False}, "obj": 3, "narrow": True,
        "nodes": 1387, "cuts": 100, "solutions": 891, "halvings": 0, "tree": False, "var": (2, 6), "expr": (6, 16)},
    "narrow_sums7": {
        "args": {"n": 7, "seed": 19, "width": 6}, "obj": 3, "narrow": True,
        "nodes": 932, "cuts": 498, "solutions": 190, "halvings": 0, "tree": True, "var": (-1, 2), "expr": (3, 8)},
    "infeasible6": {
        "args": {"n": 6, "seed": 18, "width": 6, "sums": False}, "obj": 3, "narrow": True,
        "nodes": 33, "cuts": 25, "solutions": 0, "halvings": 0, "tree": False, "var": None, "expr": None},
    "wide3_sums": {
        "args": {"n": 5, "seed": 4, "width": 5, "wide": 3, "clauses": 15}, "obj": 1, "narrow": False,
        "nodes": 12514, "cuts": 1245, "solutions": 11171, "halvings": 36, "tree": True, "var": (0, 4), "expr": (-1155, -245)},
    "wide3_plain": {
        "args": {"n": 5, "seed": 17, "width": 5, "wide": 3, "clauses": 15, "sums": False}, "obj": 3, "narrow": False,
        "nodes": 6991, "cuts": 2482, "solutions": 4454, "halvings": 17, "tree": False, "var": (-607, -343), "expr": (-807, -537)},
    "wide2_straddle": {
        "args": {"n": 6, "seed": 24, "width": 5, "wide": 2, "clauses": 18, "sums": False}, "obj": 2, "narrow": False,
        "nodes": 2716, "cuts": 9, "solutions": 2670, "halvings": 10, "tree": False, "var": (-192, 76), "expr": (635, 638)},
    "wide2_mid": {
        "args": {"n": 4, "seed": 19, "width": 5, "wide": 2, "clauses": 12}, "obj": 1, "narrow": False,
        "nodes": 5060, "cuts": 1056, "solutions": 3780, "halvings": 12, "tree": True, "var": (-853, -819), "expr": (-1704, -1634)},
    "wide2_cut": {
        "args": {"n": 5, "seed": 78, "width": 5, "wide": 2, "clauses": 15}, "obj": 1, "narrow": False,
        "nodes": 345, "cuts": 37, "solutions": 260, "halvings": 3, "tree": True, "var": (625, 1148), "expr": (1252, 2299)},
    "planted20": {
        "args": {"n": 20, "seed": 2, "width": 5, "clauses": 60, "sums": False, "slack": 1, "plant": True}, "obj": 1, "narrow": False,
        "nodes": 2026, "cuts": 240, "solutions": 1268, "halvings": 0, "tree": True, "var": (1, 5), "expr": (0, 9)},
    "planted30": {
        "args": {"n": 30, "seed": 2, "width": 5, "clauses": 100, "slack": 1, "plant": True}, "obj": 8, "narrow": False,
        "nodes": 2092, "cuts": 708, "solutions": 648, "halvings": 0, "tree": True, "var": (-2, 0), "expr": (-9, -9)},
    "planted80": {
        "args": {"n": 80, "seed": 2, "width": 5, "clauses": 220, "sums": False, "plant": True}, "obj": 38, "narrow": False,
        "nodes": 13798, "cuts": 2820, "solutions": 7020, "halvings": 0, "tree": False, "var": (2, 5), "expr": (10, 12)},
    "planted150": {
        "args": {"n": 150, "seed": 2, "width": 4, "clauses": 420, "plant": True}, "obj": 123, "narrow": False,
        "nodes": 6534, "cuts": 32, "solutions": 4536, "halvings": 0, "tree": True, "var": (0, 3), "expr": (3, 3)},
}


NARROW = [k for k, v in SETS.items() if v["narrow"]]
WIDE = [k for k, v in SETS.items() if v["halvings"] > 0]
FEASIBLE = [k for k, v in SETS.items() if v["solutions"] > 0]
INFEASIBLE = [k for k, v in SETS.items() if v["solutions"] == 0]


def text_of(name, objective="ALL"):
    return generate(objective=objective, **SETS[name]["args"])[0]


def optimisations(name):
    """the four optimisations of a set -> [(objective text, recorded optimum or None, value of the objective at a point
    (C1 .. Cn))]: MIN and MAX of the set's objective variable and of expression_text()"""
    rec = SETS[name]
    k = rec["obj"]
    var, expr = rec["var"] or (None, None), rec["expr"] or (None, None)
    return [(f"MIN C{k}", var[0], lambda x: x[k - 1]), (f"MAX C{k}", var[1], lambda x: x[k - 1]),
            ("MIN " + expression_text(), expr[0], expression_value), ("MAX " + expression_text(), expr[1], expression_value)]


def host_tree_clauses(text):
    """expression-tree clauses of the product's tables for `text`, built on the host from the oracle's root domains"""
    from csolve_amd.solver import Model
    om, _ = oracle_model(text)
    m = Model.from_text(text)
    m.set_domains(om.domains())
    m.normalize()
    return m.build_tables().device_info()["tree_clauses"]
