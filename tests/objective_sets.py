"""The incumbent-bounded fixpoint and the MIN / MAX trees of the search engine (a helper module, no test itself), on the
clause-model sets of search_sets.py under their optimisations.

The fixpoint under an incumbent: before a child is propagated "<obj>" is intersected with a bound, and if the bound moved
the clauses of "<obj>" are propagated as well (csgpu_propagate_batch_obj; the reference, csolve.c:251-252).  instances()
draws nodes on parents of seeded oracle walks, each with a cut of its parent's "<obj>" interval, and states the reference
two ways -- the reference's order and what a round-based kernel computes -- which test_objective_bound_host.py holds
equal; classify() says what the bound did to every node.

The trees: TREES records, for every optimisation of every set of search_sets.SETS, the walk of cpu_engine.OracleEngine
with incumbent="iteration" -- the device engine's rule: the children of an iteration are bounded by the incumbent as it
stood when the iteration began.  Every recorded number comes from the oracle on the host, never from the device;
test_objective_bound_host.py re-derives all of them."""
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import search_sets as S  # noqa: E402

INT32_MAX, INT32_MIN = 2**31 - 1, -2**31
NO_BOUND = (INT32_MIN, INT32_MAX)
MIN_EXPR, MAX_EXPR = "MIN " + S.expression_text(), "MAX " + S.expression_text()

# (set, objective): what each brings is said in DESIGN.md 5.  planted30 and planted150 are not used with the expression:
# its root domain is a single value there
PAIRS = [
    ("narrow_sums7", "MIN C3"), ("narrow_sums7", MAX_EXPR),      # tree clauses, brute-forceable
    ("narrow_plain8", "MIN C3"), ("narrow_plain8", MAX_EXPR),    # no tree clause besides the objective's
    ("wide3_sums", "MIN C1"), ("wide3_sums", MAX_EXPR),          # "<obj>" 360 values wide, and 1,621 wide below zero
    ("wide2_straddle", "MIN C2"),                                # "<obj>" straddles zero
    ("planted20", MAX_EXPR),                                     # kernel 6 at few clauses per lane
    ("planted30", "MIN C8"),                                     # bounds below zero
    ("planted80", "MIN C38"),                                    # kernel 6's upper clause classes
    ("planted150", "MIN C123"),                                  # more than 512 clauses: kernel 1 only
]
NARROW_PAIRS = [p for p in PAIRS if p[0].startswith("narrow_")]
NARROW_FAIL_PAIR = ("wide3_sums", MAX_EXPR)  # few of its bounded children narrow another variable: most of them fail

DRAWS = 1500      # nodes on seeded parents, each with a one-sided cut
DRAWS_OF = {("wide3_sums", "MIN C1"): 2800}  # 1,500 left this pair fewer than 200 bounds that empty "<obj>"
ON_OBJECTIVE = 120  # more nodes whose variable is "<obj>" itself
BOTH, CROSSED, UNBOUNDED = 120, 60, 120  # slices with both bounds set, with obj_lo > obj_hi, with no bound
BATCHES = (1, 63, 64, 65)  # and the rest

CLASSES = ("plain_fail", "empty", "narrow_fail", "narrow_other", "narrow_obj_only", "unmoved")


def pair_id(pair):
    return f"{pair[0]}-{pair[1].replace(' ', '').replace('*', 'x')}"


def sense_of(objective):
    """cs_objective_bound's sense: 1 minimise, 2 maximise"""
    return 1 if objective.startswith("MIN") else 2


# ---- the bound, stated in Python (cs_objective_bound, cs_arith.h; the reference's objective.c:101-126) ----

def sat_add(a, b):
    """the reference's saturating sum of two int32 values (arith.c): a sentinel absorbs"""
    if a in (INT32_MIN, INT32_MAX):
        return a
    return max(INT32_MIN, min(INT32_MAX, a + b))


def objective_bound(sense, lo, hi, best):
    """"<obj>" = [lo, hi] under the incumbent `best`: below it when minimising, above it when maximising.  INT32_MAX
    under MIN and INT32_MIN under MAX are "none yet": the arithmetic saturates and the interval stays."""
    if sense == 1:
        hi = min(hi, sat_add(best, -1))
    elif sense == 2:
        lo = max(lo, sat_add(best, 1))
    return lo, hi


# ---- instances ----

def _objective_nodes(rng, states, obj, count):
    """value and interval nodes on "<obj>" itself, on parents that still have it open where there are any"""
    open_rows = np.nonzero(states[:, obj, 0] < states[:, obj, 1])[0]
    rows = open_rows if len(open_rows) else np.arange(len(states))
    parent = rows[rng.integers(len(rows), size=count)]
    lo, hi = states[parent, obj, 0].astype(np.int64), states[parent, obj, 1].astype(np.int64)
    a = lo + (rng.random(count) * (hi - lo + 1)).astype(np.int64).clip(0, hi - lo)
    b = np.where(rng.random(count) < 0.4, a + (rng.random(count) * (hi - a + 1)).astype(np.int64).clip(0, hi - a), a)
    return np.stack([np.full(count, obj), a, b, parent], 1).astype(np.int32)


def reference_order(orc, obj, parent, node, bound):
    """(a) the reference's order (csolve.c:251-252): the node, then "<obj>" intersected with the bound -- an empty
    intersection fails the node --, then, if a bound moved, the clauses of "<obj>"
    -> (status, out, unbounded status, unbounded out, did the bound move, did it empty "<obj>")"""
    v, lo, hi = node
    st0, out0 = orc.instance(parent, v, lo, hi)
    if st0 < 0:
        return -1, out0, st0, out0, False, False
    nl, nh = max(int(out0[obj, 0]), bound[0]), min(int(out0[obj, 1]), bound[1])
    if nl > nh:
        return -1, out0, st0, out0, True, True
    if (nl, nh) == (int(out0[obj, 0]), int(out0[obj, 1])):
        return st0, out0, st0, out0, False, False
    st, out = orc.instance(out0, obj, nl, nh)
    return (-1 if st < 0 else st0 + st), out, st0, out0, True, False


def rounds_order(orc, obj, parent, node, bound):
    """(b) what a round-based kernel computes: the parent row with the assignment and the bound written in, then every
    clause to the fixpoint -> (status, out)"""
    v, lo, hi = node
    row = parent.copy()
    if v >= 0:
        row[v] = (lo, hi)
    nl, nh = max(int(row[obj, 0]), bound[0]), min(int(row[obj, 1]), bound[1])
    if nl > nh:
        return -1, row
    row[obj] = (nl, nh)
    return orc.instance(row, -1, 0, 0)


def classify(obj, st, out, st0, out0, moved, emptied):
    """what the bound did to a node, against the unbounded child -> one of CLASSES"""
    if st0 < 0:
        return "plain_fail"
    if emptied:
        return "empty"
    if not moved:
        return "unmoved"
    if st < 0:
        return "narrow_fail"
    other = (out != out0).any(1)
    other[obj] = False
    return "narrow_other" if other.any() else "narrow_obj_only"


def draws_of(pair):
    return DRAWS_OF.get(pair, DRAWS)


def draw(pair):
    """the drawn instances of a pair, without the reference: parents of seeded oracle walks (every one a fixpoint); value,
    interval and var = -1 nodes on them and nodes on "<obj>" itself, each with a cut drawn from [lo - 2, hi + 2] of its
    parent's "<obj>" interval -- obj_hi under MIN, obj_lo under MAX --; then slices with both bounds set, with
    obj_lo > obj_hi and with no bound -> dict(states [P, n, 2], nodes [N, 4], bounds [N, 2], obj, sense, oracle, model,
    columns)"""
    from oracle.cs_oracle import Oracle
    from test_gpu_instantiations import _nodes, _walk_states
    name, objective = pair
    draws = draws_of(pair)
    om, cols = S.oracle_model(S.text_of(name, objective))
    orc = Oracle(om)
    obj, sense = int(om.view.obj_var), sense_of(objective)
    assert obj >= 0
    rng = np.random.default_rng(zlib.crc32(pair_id(pair).encode()))
    states = _walk_states(orc, om.domains(), rng)
    extra = BOTH + CROSSED + UNBOUNDED
    nodes = np.concatenate([_nodes(rng, states, draws), _objective_nodes(rng, states, obj, ON_OBJECTIVE),
                            _nodes(rng, states, extra)])
    N = len(nodes)
    plo, phi = states[nodes[:, 3], obj, 0].astype(np.int64), states[nodes[:, 3], obj, 1].astype(np.int64)

    def cut():
        return plo - 2 + (rng.random(N) * (phi - plo + 5)).astype(np.int64).clip(0, phi - plo + 4)

    c1, c2 = cut(), cut()
    bounds = np.empty((N, 2), dtype=np.int64)
    bounds[:, 0], bounds[:, 1] = (INT32_MIN, 0) if sense == 1 else (0, INT32_MAX)
    bounds[:, 1 if sense == 1 else 0] = c1
    at = draws + ON_OBJECTIVE
    both = slice(at, at + BOTH)
    bounds[both, 0], bounds[both, 1] = np.minimum(c1, c2)[both], np.maximum(c1, c2)[both]
    crossed = slice(at + BOTH, at + BOTH + CROSSED)
    bounds[crossed, 0], bounds[crossed, 1] = np.maximum(c1, c2)[crossed] + 1, np.minimum(c1, c2)[crossed]
    bounds[at + BOTH + CROSSED:] = NO_BOUND
    return dict(pair=pair, states=states, nodes=nodes, bounds=bounds, obj=obj, sense=sense, oracle=orc, model=om, columns=cols,
                slices={"both": both, "crossed": crossed, "unbounded": slice(at + BOTH + CROSSED, N)})


def refer(inst, bounds=None, both_ways=False):
    """the reference of every drawn node under its bound (or under `bounds` [N, 2]) -> dict(status [N] (-1 or 0),
    out [N, n, 2], klass [N]); both_ways: computed by reference_order AND by rounds_order, held equal here"""
    orc, obj, states, nodes = inst["oracle"], inst["obj"], inst["states"], inst["nodes"]
    bounds = inst["bounds"] if bounds is None else bounds
    N = len(nodes)
    status = np.empty(N, dtype=np.int64)
    out = np.empty((N,) + states.shape[1:], dtype=np.int32)
    klass = []
    for i in range(N):
        node = tuple(int(x) for x in nodes[i, :3])
        bound = (int(bounds[i, 0]), int(bounds[i, 1]))
        parent = states[nodes[i, 3]]
        st, o, st0, o0, moved, emptied = reference_order(orc, obj, parent, node, bound)
        if both_ways:
            st_b, o_b = rounds_order(orc, obj, parent, node, bound)
            assert (st < 0) == (st_b < 0), ("the two statements of the reference disagree", inst["pair"], node, bound)
            assert st < 0 or (o == o_b).all(), ("the two statements of the reference disagree", inst["pair"], node, bound)
        status[i], out[i] = (-1 if st < 0 else 0), o
        klass.append(classify(obj, st, o, st0, o0, moved, emptied))
    return dict(status=status, out=out, klass=np.array(klass))


def instances(pair):
    """draw() with the reference of every node under its own bound"""
    inst = draw(pair)
    inst.update(refer(inst))
    return inst


def groups(bounds):
    """the nodes that share a bound (one launch takes one bound) -> [((obj_lo, obj_hi), indices)]"""
    uniq, inverse = np.unique(bounds, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    return [((int(b[0]), int(b[1])), np.nonzero(inverse == k)[0]) for k, b in enumerate(uniq)]


def common_bound(inst):
    """one bound for all nodes of a pair, for the tests of the batch sizes: the median, over the consistent unbounded
    children, of the end of "<obj>" the bound works against (lo under MIN, hi under MAX) -- about half of them are
    emptied by it, and those that lie wholly on its good side are left as they are"""
    orc, obj, states, nodes = inst["oracle"], inst["obj"], inst["states"], inst["nodes"]
    side = 0 if inst["sense"] == 1 else 1
    ends = []
    for v, lo, hi, p in nodes:
        st, out = orc.instance(states[p], int(v), int(lo), int(hi))
        if st >= 0:
            ends.append(int(out[obj, side]))
    cut = int(np.median(ends))
    return (INT32_MIN, cut) if inst["sense"] == 1 else (cut, INT32_MAX)


def class_counts(inst):
    return {k: int((inst["klass"] == k).sum()) for k in CLASSES}


# ---- trees ----

def engine_tree(name, objective, parents, lag=0, incumbent="iteration"):
    """the MIN / MAX walk of `name` under `objective` by the oracle-backed engine with the device's incumbent rule ->
    ((nodes, cuts, solutions, iterations, pool_peak, best), engine)"""
    from cpu_engine import OracleEngine
    om, _ = S.oracle_model(S.text_of(name, objective))
    eng = OracleEngine(om, parents_per_iteration=parents, incumbent=incumbent, lag=lag)
    eng.put(torch.from_numpy(om.domains()).unsqueeze(0).contiguous())
    st = eng.run(1 << 40)
    assert st["done"] == 1
    return tuple(int(st[k]) for k in ("nodes", "cuts", "solutions", "iterations", "pool_peak", "best")), eng


OBJECTIVES = ("min-var", "max-var", "min-expr", "max-expr")  # the order of search_sets.optimisations()
PARENTS = (1, 64)
LAGGED_SETS = ("narrow_sums7", "wide3_sums", "wide3_plain")  # the sets the engine's drive modes are compared on


def objective_text(name, which):
    return S.optimisations(name)[OBJECTIVES.index(which)][0]


# what the draws hold, class by class (classify(); test_objective_bound_host.py derives it again)
CLASS_COUNTS = {
    ('narrow_sums7', 'MIN C3'): {'plain_fail': 602, 'empty': 512, 'narrow_fail': 14, 'narrow_other': 48, 'narrow_obj_only': 0, 'unmoved': 744},
    ('narrow_sums7', 'MAX 2*C1 + C3'): {'plain_fail': 617, 'empty': 465, 'narrow_fail': 66, 'narrow_other': 97, 'narrow_obj_only': 66, 'unmoved': 609},
    ('narrow_plain8', 'MIN C3'): {'plain_fail': 66, 'empty': 715, 'narrow_fail': 0, 'narrow_other': 90, 'narrow_obj_only': 0, 'unmoved': 1049},
    ('narrow_plain8', 'MAX 2*C1 + C3'): {'plain_fail': 122, 'empty': 650, 'narrow_fail': 12, 'narrow_other': 137, 'narrow_obj_only': 70, 'unmoved': 929},
    ('wide3_sums', 'MIN C1'): {'plain_fail': 1689, 'empty': 255, 'narrow_fail': 38, 'narrow_other': 773, 'narrow_obj_only': 0, 'unmoved': 465},
    ('wide3_sums', 'MAX 2*C1 + C3'): {'plain_fail': 971, 'empty': 271, 'narrow_fail': 209, 'narrow_other': 37, 'narrow_obj_only': 100, 'unmoved': 332},
    ('wide2_straddle', 'MIN C2'): {'plain_fail': 25, 'empty': 663, 'narrow_fail': 0, 'narrow_other': 249, 'narrow_obj_only': 0, 'unmoved': 983},
    ('planted20', 'MAX 2*C1 + C3'): {'plain_fail': 79, 'empty': 592, 'narrow_fail': 0, 'narrow_other': 250, 'narrow_obj_only': 73, 'unmoved': 926},
    ('planted30', 'MIN C8'): {'plain_fail': 301, 'empty': 620, 'narrow_fail': 0, 'narrow_other': 108, 'narrow_obj_only': 0, 'unmoved': 891},
    ('planted80', 'MIN C38'): {'plain_fail': 75, 'empty': 629, 'narrow_fail': 5, 'narrow_other': 331, 'narrow_obj_only': 0, 'unmoved': 880},
    ('planted150', 'MIN C123'): {'plain_fail': 154, 'empty': 636, 'narrow_fail': 0, 'narrow_other': 241, 'narrow_obj_only': 0, 'unmoved': 889},
}

# (set, objective, parents per iteration) -> (nodes, cuts, solutions, iterations, pool_peak, best) of engine_tree(): the
# walk every device-driven mode of the engine must make (a device-driven iteration sees every solution of the
# iterations before it)
TREES = {
    ('narrow_sums8', 'min-var', 1): (52, 33, 6, 14, 10, 2), ('narrow_sums8', 'min-var', 64): (1353, 957, 56, 9, 244, 2),
    ('narrow_sums8', 'max-var', 1): (69, 51, 1, 18, 13, 4), ('narrow_sums8', 'max-var', 64): (1521, 1121, 12, 10, 292, 4),
    ('narrow_sums8', 'min-expr', 1): (52, 33, 6, 14, 10, 6), ('narrow_sums8', 'min-expr', 64): (1353, 957, 56, 9, 244, 6),
    ('narrow_sums8', 'max-expr', 1): (69, 51, 1, 18, 13, 16), ('narrow_sums8', 'max-expr', 64): (1521, 1121, 12, 10, 292, 16),
    ('narrow_plain7', 'min-var', 1): (58, 43, 1, 15, 10, 1), ('narrow_plain7', 'min-var', 64): (1533, 1131, 92, 9, 212, 1),
    ('narrow_plain7', 'max-var', 1): (47, 31, 4, 13, 8, 4), ('narrow_plain7', 'max-var', 64): (1413, 1095, 27, 9, 193, 4),
    ('narrow_plain7', 'min-expr', 1): (58, 43, 1, 15, 10, 3), ('narrow_plain7', 'min-expr', 64): (1533, 1131, 92, 9, 212, 3),
    ('narrow_plain7', 'max-expr', 1): (47, 31, 4, 13, 8, 10), ('narrow_plain7', 'max-expr', 64): (1413, 1095, 27, 9, 193, 10),
    ('narrow_plain8', 'min-var', 1): (67, 47, 3, 18, 13, 2), ('narrow_plain8', 'min-var', 64): (865, 366, 247, 8, 130, 2),
    ('narrow_plain8', 'max-var', 1): (37, 22, 3, 13, 9, 6), ('narrow_plain8', 'max-var', 64): (745, 477, 47, 8, 130, 6),
    ('narrow_plain8', 'min-expr', 1): (78, 55, 3, 21, 15, 6), ('narrow_plain8', 'min-expr', 64): (1158, 750, 81, 9, 179, 6),
    ('narrow_plain8', 'max-expr', 1): (30, 18, 3, 10, 7, 16), ('narrow_plain8', 'max-expr', 64): (244, 144, 16, 5, 47, 16),
    ('narrow_sums7', 'min-var', 1): (63, 41, 4, 19, 9, -1), ('narrow_sums7', 'min-var', 64): (765, 531, 29, 7, 88, -1),
    ('narrow_sums7', 'max-var', 1): (43, 30, 2, 12, 8, 2), ('narrow_sums7', 'max-var', 64): (673, 474, 17, 7, 88, 2),
    ('narrow_sums7', 'min-expr', 1): (54, 35, 4, 16, 9, 3), ('narrow_sums7', 'min-expr', 64): (671, 471, 13, 7, 87, 3),
    ('narrow_sums7', 'max-expr', 1): (81, 57, 2, 23, 9, 8), ('narrow_sums7', 'max-expr', 64): (567, 396, 9, 7, 87, 8),
    ('infeasible6', 'min-var', 1): (33, 25, 0, 9, 7, 2147483647), ('infeasible6', 'min-var', 64): (33, 25, 0, 3, 4, 2147483647),
    ('infeasible6', 'max-var', 1): (33, 25, 0, 9, 4, -2147483648), ('infeasible6', 'max-var', 64): (33, 25, 0, 3, 4, -2147483648),
    ('infeasible6', 'min-expr', 1): (33, 25, 0, 9, 7, 2147483647), ('infeasible6', 'min-expr', 64): (33, 25, 0, 3, 4, 2147483647),
    ('infeasible6', 'max-expr', 1): (33, 25, 0, 9, 4, -2147483648), ('infeasible6', 'max-expr', 64): (33, 25, 0, 3, 4, -2147483648),
    ('wide3_sums', 'min-var', 1): (659, 422, 223, 15, 10, 0), ('wide3_sums', 'min-var', 64): (12514, 3506, 8910, 7, 46, 0),
    ('wide3_sums', 'max-var', 1): (645, 414, 222, 10, 5, 4), ('wide3_sums', 'max-var', 64): (12514, 3506, 8910, 7, 46, 4),
    ('wide3_sums', 'min-expr', 1): (1118, 649, 452, 18, 10, -1155), ('wide3_sums', 'min-expr', 64): (12514, 2585, 9831, 7, 46, -1155),
    ('wide3_sums', 'max-expr', 1): (1723, 1481, 222, 21, 5, -245), ('wide3_sums', 'max-expr', 64): (12514, 3506, 8910, 7, 46, -245),
    ('wide3_plain', 'min-var', 1): (439, 224, 204, 12, 9, -607), ('wide3_plain', 'min-var', 64): (6991, 2482, 4454, 4, 34, -607),
    ('wide3_plain', 'max-var', 1): (435, 368, 58, 10, 7, -343), ('wide3_plain', 'max-var', 64): (6991, 2482, 4454, 4, 34, -343),
    ('wide3_plain', 'min-expr', 1): (439, 224, 204, 12, 9, -807), ('wide3_plain', 'min-expr', 64): (6991, 2482, 4454, 4, 34, -807),
    ('wide3_plain', 'max-expr', 1): (435, 368, 58, 10, 7, -537), ('wide3_plain', 'max-expr', 64): (6991, 2482, 4454, 4, 34, -537),
    ('wide2_straddle', 'min-var', 1): (287, 145, 134, 9, 5, -192), ('wide2_straddle', 'min-var', 64): (1646, 1077, 540, 5, 12, -192),
    ('wide2_straddle', 'max-var', 1): (282, 142, 133, 8, 5, 76), ('wide2_straddle', 'max-var', 64): (1646, 1084, 533, 5, 12, 76),
    ('wide2_straddle', 'min-expr', 1): (289, 146, 134, 10, 5, 635), ('wide2_straddle', 'min-expr', 64): (2186, 1350, 801, 6, 12, 635),
    ('wide2_straddle', 'max-expr', 1): (288, 145, 133, 11, 6, 638), ('wide2_straddle', 'max-expr', 64): (2720, 1614, 1067, 7, 12, 638),
    ('wide2_mid', 'min-var', 1): (856, 813, 1, 43, 38, -853), ('wide2_mid', 'min-var', 64): (1915, 1860, 1, 5, 39, -853),
    ('wide2_mid', 'max-var', 1): (850, 775, 36, 40, 36, -819), ('wide2_mid', 'max-var', 64): (5060, 4206, 630, 8, 170, -819),
    ('wide2_mid', 'min-expr', 1): (856, 813, 1, 43, 38, -1704), ('wide2_mid', 'min-expr', 64): (1915, 1855, 6, 5, 39, -1704),
    ('wide2_mid', 'max-expr', 1): (850, 775, 36, 40, 36, -1634), ('wide2_mid', 'max-expr', 64): (5054, 4203, 630, 8, 167, -1634),
    ('wide2_cut', 'min-var', 1): (42, 28, 7, 8, 5, 625), ('wide2_cut', 'min-var', 64): (270, 202, 30, 4, 29, 625),
    ('wide2_cut', 'max-var', 1): (80, 56, 11, 14, 11, 1148), ('wide2_cut', 'max-var', 64): (338, 113, 179, 5, 29, 1148),
    ('wide2_cut', 'min-expr', 1): (31, 18, 7, 7, 4, 1252), ('wide2_cut', 'min-expr', 64): (158, 109, 27, 4, 16, 1252),
    ('wide2_cut', 'max-expr', 1): (104, 77, 12, 16, 12, 2299), ('wide2_cut', 'max-expr', 64): (348, 229, 70, 5, 27, 2299),
    ('planted20', 'min-var', 1): (61, 41, 3, 18, 12, 1), ('planted20', 'min-var', 64): (1030, 502, 266, 9, 164, 1),
    ('planted20', 'max-var', 1): (51, 27, 5, 20, 11, 5), ('planted20', 'max-var', 64): (1030, 660, 108, 9, 164, 5),
    ('planted20', 'min-expr', 1): (65, 43, 3, 20, 13, 0), ('planted20', 'min-expr', 64): (1899, 1112, 333, 12, 292, 0),
    ('planted20', 'max-expr', 1): (51, 28, 5, 19, 10, 9), ('planted20', 'max-expr', 64): (1208, 862, 48, 10, 200, 9),
    ('planted30', 'min-var', 1): (52, 32, 1, 20, 11, -2), ('planted30', 'min-var', 64): (976, 598, 30, 12, 148, -2),
    ('planted30', 'max-var', 1): (45, 24, 3, 19, 10, 0), ('planted30', 'max-var', 64): (830, 486, 42, 11, 136, 0),
    ('planted30', 'min-expr', 1): (46, 28, 1, 18, 10, -9), ('planted30', 'min-expr', 64): (730, 444, 24, 10, 122, -9),
    ('planted30', 'max-expr', 1): (45, 24, 3, 19, 10, -9), ('planted30', 'max-expr', 64): (757, 467, 19, 11, 131, -9),
    ('planted80', 'min-var', 1): (58, 33, 3, 23, 13, 2), ('planted80', 'min-var', 64): (2102, 1340, 72, 16, 372, 2),
    ('planted80', 'max-var', 1): (53, 29, 3, 22, 12, 5), ('planted80', 'max-var', 64): (2109, 1211, 144, 17, 388, 5),
    ('planted80', 'min-expr', 1): (59, 34, 3, 23, 13, 10), ('planted80', 'min-expr', 64): (2082, 1331, 60, 16, 373, 10),
    ('planted80', 'max-expr', 1): (53, 29, 3, 22, 12, 12), ('planted80', 'max-expr', 64): (2088, 1193, 144, 17, 394, 12),
    ('planted150', 'min-var', 1): (59, 35, 3, 22, 13, 0), ('planted150', 'min-var', 64): (1890, 1064, 192, 16, 400, 0),
    ('planted150', 'max-var', 1): (62, 37, 4, 22, 13, 3), ('planted150', 'max-var', 64): (2082, 1192, 256, 16, 400, 3),
    ('planted150', 'min-expr', 1): (59, 35, 3, 22, 13, 3), ('planted150', 'min-expr', 64): (1854, 1040, 192, 16, 400, 3),
    ('planted150', 'max-expr', 1): (62, 37, 4, 22, 13, 3), ('planted150', 'max-expr', 64): (2046, 1168, 256, 16, 400, 3),
}

# the same with lag = 1: the host-driven loop (CSGPU_SEARCH_BURST=0), where the solutions of iteration k bound the
# children of iteration k + 2
LAGGED_TREES = {
    ('narrow_sums7', 'min-var', 1): (69, 43, 6, 21, 9, -1), ('narrow_sums7', 'min-var', 64): (932, 572, 116, 8, 88, -1),
    ('narrow_sums7', 'max-var', 1): (49, 35, 2, 13, 8, 2), ('narrow_sums7', 'max-var', 64): (876, 574, 72, 8, 88, 2),
    ('narrow_sums7', 'min-expr', 1): (60, 37, 6, 18, 9, 3), ('narrow_sums7', 'min-expr', 64): (876, 556, 90, 8, 91, 3),
    ('narrow_sums7', 'max-expr', 1): (81, 54, 5, 23, 9, 8), ('narrow_sums7', 'max-expr', 64): (830, 560, 51, 8, 87, 8),
    ('wide3_sums', 'min-var', 1): (659, 199, 446, 15, 10, 0), ('wide3_sums', 'min-var', 64): (12514, 1245, 11171, 7, 46, 0),
    ('wide3_sums', 'max-var', 1): (645, 192, 444, 10, 5, 4), ('wide3_sums', 'max-var', 64): (12514, 1245, 11171, 7, 46, 4),
    ('wide3_sums', 'min-expr', 1): (1118, 347, 754, 18, 10, -1155), ('wide3_sums', 'min-expr', 64): (12514, 1245, 11171, 7, 46, -1155),
    ('wide3_sums', 'max-expr', 1): (1723, 1259, 444, 21, 5, -245), ('wide3_sums', 'max-expr', 64): (12514, 1245, 11171, 7, 46, -245),
    ('wide3_plain', 'min-var', 1): (439, 166, 262, 12, 9, -607), ('wide3_plain', 'min-var', 64): (6991, 2482, 4454, 4, 34, -607),
    ('wide3_plain', 'max-var', 1): (435, 164, 262, 10, 7, -343), ('wide3_plain', 'max-var', 64): (6991, 2482, 4454, 4, 34, -343),
    ('wide3_plain', 'min-expr', 1): (439, 166, 262, 12, 9, -807), ('wide3_plain', 'min-expr', 64): (6991, 2482, 4454, 4, 34, -807),
    ('wide3_plain', 'max-expr', 1): (435, 164, 262, 10, 7, -537), ('wide3_plain', 'max-expr', 64): (6991, 2482, 4454, 4, 34, -537),
}
