"""The search engine's trees under the reference's five variable orders, and its ANY restart schedule, derived on the
host (a helper module, no test itself): the branching key of strategy.c:79-121 as plain integers, a walk of the ALL tree
that branches by that key with the oracle for every child, the Luby sequence of csolve.c:76-83 in closed form, pigeonhole
models (infeasible, so that an ANY search with restarts must still walk a whole tree), and the table of recorded trees.
Nothing here calls the product's library, and every recorded number comes from all_tree() on the host, never from the
device; test_order_walk_host.py re-derives all of them."""
import functools
import os
import sys

from csolve_amd import problems

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import search_sets as S  # noqa: E402

INT32_MAX, INT32_MIN = 2**31 - 1, -2**31
ORDERS = ["none", "smallest-domain", "largest-domain", "smallest-value", "largest-value"]
NON_DEFAULT = [o for o in ORDERS if o != "smallest-domain"]
SPLIT_WIDTH = 256  # an interval of more values is halved, not enumerated
CAP = 20000  # nodes of a recorded tree: about a second of host walk

_INDEX_BITS, _PRIO_BITS, _STATE_BIAS = 32, 65, 1 << 33


def branch_key(order, prefer_failing, lo, hi, prio, index):
    """the key the open variables are ordered by, one Python integer: the variable with the smallest key is branched on
    first (the one the reference's heap would pop).  From the top: the state part of the rule -- none: nothing;
    smallest-domain: hi - lo; largest-domain: -(hi - lo); smallest-value: lo; largest-value: -hi; an interval with a
    bound on INT32_MIN / INT32_MAX (the reference's infinities) has the largest size there is --, then, with
    prefer_failing, the failure count `prio`, higher first, then the index, lower first.  key >> 32 leaves the index
    out."""
    size = 1 << 32 if lo == INT32_MIN or hi == INT32_MAX else hi - lo
    state = {"none": 0, "smallest-domain": size, "largest-domain": -size, "smallest-value": lo, "largest-value": -hi}[order]
    assert -_STATE_BIAS < state < _STATE_BIAS and -(1 << 63) <= prio < (1 << 63) and 0 <= index < (1 << _INDEX_BITS)
    failing = (1 << 63) - 1 - prio if prefer_failing else 0
    return (((state + _STATE_BIAS) << _PRIO_BITS) | failing) << _INDEX_BITS | index


def all_tree(text, order, max_nodes=None):
    """the ALL tree of `text` under `order`, from the oracle's root fixpoint (search_sets.oracle_model): at each state the
    open variable with the smallest branch_key (no failure counts) is branched on -- an interval of more than 256 values
    into [lo, mid] and [mid + 1, hi] with mid = (lo + hi) >> 1, otherwise into its values --, every child is
    Oracle.instance(state, var, a, b): inconsistent is a cut, complete and root true a solution, complete and root
    false counted apart, anything else open.  -> dict(nodes: the children made, cuts, solutions, halvings: parents split
    in two, complete_false, props: the oracle's PROPS summed over the consistent children, found: the solutions as a set
    of tuples in the order of `names`, names: C1 .. Cn of a search_sets model, else the model's variables in its own
    order).  Under ALL none of this depends on the order in which the open states are taken.  max_nodes: give up
    (AssertionError) beyond it."""
    from oracle.cs_oracle import Oracle
    om, _ = S.oracle_model(text)
    orc = Oracle(om)
    names = om.names()
    if all(s[0] == "C" and s[1:].isdigit() for s in names):
        cols = S.columns(names)
    else:
        cols = list(range(len(names)))
    out = dict(nodes=0, cuts=0, solutions=0, halvings=0, complete_false=0, props=0, found=set(),
               names=[names[c] for c in cols])
    stack = [om.domains()]
    while stack:
        state = stack.pop()
        bounds = state.tolist()
        keys = [branch_key(order, False, lo, hi, 0, i) for i, (lo, hi) in enumerate(bounds) if lo != hi]
        var = min(keys) & ((1 << _INDEX_BITS) - 1)
        lo, hi = bounds[var]
        if hi - lo + 1 > SPLIT_WIDTH:
            mid = (lo + hi) >> 1
            kids = [(lo, mid), (mid + 1, hi)]
            out["halvings"] += 1
        else:
            kids = [(x, x) for x in range(lo, hi + 1)]
        for a, b in kids:
            out["nodes"] += 1
            status, child = orc.instance(state, var, a, b)
            if status < 0:
                out["cuts"] += 1
                continue
            out["props"] += status
            if (child[:, 0] == child[:, 1]).all():
                orc.set_domains(child)
                t_lo, t_hi = orc.eval(om.root)
                if t_lo > 0 or t_hi < 0:
                    out["solutions"] += 1
                    out["found"].add(tuple(int(child[c, 0]) for c in cols))
                else:
                    out["complete_false"] += 1
            else:
                stack.append(child)
        assert max_nodes is None or out["nodes"] <= max_nodes, f"ALL tree beyond {max_nodes} nodes"
    return out


def luby(k):
    """the k-th term (k = 1, 2, ...) of 1, 1, 2, 1, 1, 2, 4, 1, 1, 2, 1, 1, 2, 4, 8, ...: 2^(i-1) where k = 2^i - 1, else
    the term at k - 2^(i-1) + 1 for the i with 2^(i-1) <= k < 2^i - 1"""
    assert k >= 1
    while True:
        i = k.bit_length()
        if k == (1 << i) - 1:
            return 1 << (i - 1)
        k -= (1 << (i - 1)) - 1


def pigeon(n, tree=False, objective="ANY"):
    """n variables X0 .. X{n-1} with the n - 1 values 1 .. n - 1, pairwise different: infeasible, and consistent until
    the search has valued all but two of them.  tree: X0 + X1 < 2 (n - 1) as well -- a clause that stays an expression
    tree, which the != network's own kernel refuses and the general kernels take (it cuts the one pair of values that
    X0 != X1 forbids already)"""
    lines = [f"# pigeonhole: {n} variables, {n - 1} values", f"{objective};"]
    for i in range(n):
        for j in range(i + 1, n):
            lines.append(f"X{i} != X{j};")
    if tree:
        lines.append(f"X0 + X1 < {2 * (n - 1)};")
    for i in range(n):
        lines.append(f"1 <= X{i}; X{i} <= {n - 1};")
    return "\n".join(lines) + "\n"


# != networks of test_gpu_search.py's tree test: name -> text under ALL
NETWORKS = {
    "queens7": lambda: problems.queens(7, "ALL"),
    "queens8": lambda: problems.queens(8, "ALL"),
    "offsets6x5": lambda: problems.offsets(6, 5, 2, "ALL"),
    "sudoku9": lambda: problems.sudoku(3, 0.35, 1, "ALL"),
    "offsets40x8": lambda: problems.offsets(40, 8, 1, "ALL"),
}
CLAUSE_SETS = ["narrow_sums7", "narrow_plain7", "infeasible6", "wide2_cut", "wide2_straddle", "wide2_mid", "wide3_sums",
               "wide3_plain", "planted30", "planted80", "planted150"]
SET_NAMES = CLAUSE_SETS + list(NETWORKS)


@functools.lru_cache(maxsize=None)
def text_of(name):
    return NETWORKS[name]() if name in NETWORKS else S.text_of(name)


@functools.lru_cache(maxsize=None)
def walk(name, order):
    """all_tree of a named set, once per process: the tests share it and leave it unchanged"""
    return all_tree(text_of(name), order, max_nodes=OVER_CAP.get((name, order), CAP))


# the one recorded pair beyond CAP, with a cap of its own: offsets40x8 under the default rule, the only network of the
# table whose default engine takes the one-wave-per-parent level kernel (three seconds of host walk; test_gpu_search.py
# walks the same tree)
OVER_CAP = {("offsets40x8", "smallest-domain"): 70000}

# (set, order) -> (nodes, cuts, solutions, halvings) of all_tree().  Every pair of SET_NAMES x ORDERS is here but for
# those whose host walk would take minutes: wide3_sums under largest-domain (105,626 nodes) and under smallest-value
# (beyond 300,000), and offsets40x8 under the four non-default orders (the default rule alone keeps that network's tree
# within reach).  Every other recorded tree has at most CAP nodes.
RECORDED = {
    ("narrow_sums7", "none"): (869, 440, 190, 0),
    ("narrow_sums7", "smallest-domain"): (932, 498, 190, 0),
    ("narrow_sums7", "largest-domain"): (485, 138, 190, 0),
    ("narrow_sums7", "smallest-value"): (460, 129, 190, 0),
    ("narrow_sums7", "largest-value"): (587, 210, 190, 0),
    ("narrow_plain7", "none"): (1828, 932, 498, 0),
    ("narrow_plain7", "smallest-domain"): (1672, 830, 498, 0),
    ("narrow_plain7", "largest-domain"): (1248, 290, 498, 0),
    ("narrow_plain7", "smallest-value"): (903, 125, 498, 0),
    ("narrow_plain7", "largest-value"): (1032, 252, 498, 0),
    ("infeasible6", "none"): (81, 61, 0, 0),
    ("infeasible6", "smallest-domain"): (33, 25, 0, 0),
    ("infeasible6", "largest-domain"): (123, 83, 0, 0),
    ("infeasible6", "smallest-value"): (41, 29, 0, 0),
    ("infeasible6", "largest-value"): (5, 5, 0, 0),
    ("wide2_cut", "none"): (355, 37, 260, 3),
    ("wide2_cut", "smallest-domain"): (345, 37, 260, 3),
    ("wide2_cut", "largest-domain"): (2875, 2451, 260, 4),
    ("wide2_cut", "smallest-value"): (493, 178, 260, 2),
    ("wide2_cut", "largest-value"): (2717, 2266, 260, 15),
    ("wide2_straddle", "none"): (2714, 7, 2670, 10),
    ("wide2_straddle", "smallest-domain"): (2716, 9, 2670, 10),
    ("wide2_straddle", "largest-domain"): (4807, 0, 2670, 1),
    ("wide2_straddle", "smallest-value"): (5073, 0, 2670, 1),
    ("wide2_straddle", "largest-value"): (3772, 8, 2670, 2),
    ("wide2_mid", "none"): (5060, 1056, 3780, 12),
    ("wide2_mid", "smallest-domain"): (5060, 1056, 3780, 12),
    ("wide2_mid", "largest-domain"): (5884, 176, 3780, 2),
    ("wide2_mid", "smallest-value"): (4267, 176, 3780, 2),
    ("wide2_mid", "largest-value"): (4267, 176, 3780, 2),
    ("wide3_sums", "none"): (11812, 545, 11171, 32),
    ("wide3_sums", "smallest-domain"): (12514, 1245, 11171, 36),
    ("wide3_sums", "largest-value"): (11460, 193, 11171, 30),
    ("wide3_plain", "none"): (6098, 584, 4454, 4),
    ("wide3_plain", "smallest-domain"): (6991, 2482, 4454, 17),
    ("wide3_plain", "largest-domain"): (6240, 463, 4454, 1),
    ("wide3_plain", "smallest-value"): (6225, 457, 4454, 1),
    ("wide3_plain", "largest-value"): (6992, 2483, 4454, 17),
    ("planted30", "none"): (2850, 998, 648, 0),
    ("planted30", "smallest-domain"): (2092, 708, 648, 0),
    ("planted30", "largest-domain"): (1710, 242, 648, 0),
    ("planted30", "smallest-value"): (1499, 194, 648, 0),
    ("planted30", "largest-value"): (1267, 82, 648, 0),
    ("planted80", "none"): (14458, 1188, 7020, 0),
    ("planted80", "smallest-domain"): (13798, 2820, 7020, 0),
    ("planted80", "largest-domain"): (14026, 10, 7020, 0),
    ("planted80", "smallest-value"): (14886, 2160, 7020, 0),
    ("planted80", "largest-value"): (13492, 92, 7020, 0),
    ("planted150", "none"): (15890, 4542, 4536, 0),
    ("planted150", "smallest-domain"): (6534, 32, 4536, 0),
    ("planted150", "largest-domain"): (17836, 4548, 4536, 0),
    ("planted150", "smallest-value"): (7370, 144, 4536, 0),
    ("planted150", "largest-value"): (9604, 876, 4536, 0),
    ("queens7", "none"): (294, 185, 40, 0),
    ("queens7", "smallest-domain"): (246, 145, 40, 0),
    ("queens7", "largest-domain"): (330, 233, 40, 0),
    ("queens7", "smallest-value"): (354, 245, 40, 0),
    ("queens7", "largest-value"): (354, 245, 40, 0),
    ("queens8", "none"): (1262, 914, 92, 0),
    ("queens8", "smallest-domain"): (982, 630, 92, 0),
    ("queens8", "largest-domain"): (1558, 1210, 92, 0),
    ("queens8", "smallest-value"): (1488, 1127, 92, 0),
    ("queens8", "largest-value"): (1488, 1127, 92, 0),
    ("offsets6x5", "none"): (1776, 453, 806, 0),
    ("offsets6x5", "smallest-domain"): (1992, 707, 806, 0),
    ("offsets6x5", "largest-domain"): (1618, 282, 806, 0),
    ("offsets6x5", "smallest-value"): (1763, 442, 806, 0),
    ("offsets6x5", "largest-value"): (1888, 541, 806, 0),
    ("sudoku9", "none"): (1581, 1160, 130, 0),
    ("sudoku9", "smallest-domain"): (1134, 647, 130, 0),
    ("sudoku9", "largest-domain"): (2093, 1644, 130, 0),
    ("sudoku9", "smallest-value"): (3140, 2468, 130, 0),
    ("sudoku9", "largest-value"): (1155, 793, 130, 0),
    ("offsets40x8", "smallest-domain"): (62648, 40108, 0, 0),
}

PAIRS = list(RECORDED)
SETS_OF_THE_TABLE = [name for name in SET_NAMES if any(k[0] == name for k in RECORDED)]


def orders_of(name):
    return [o for o in ORDERS if (name, o) in RECORDED]
