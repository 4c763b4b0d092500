"""Host tests of the mixed-operator sets of tree_sets.py: the generator is pinned and the recorded table re-derives;
every set keeps the conditions that make it safe and meaningful on a device (bounded widths, no sentinel, its trees
really trees, no tree over the node limit); the oracle itself is held against a brute force over the declared bounds,
which needs neither the oracle nor the front end; and no recorded instance takes more propagations than its set's total
width.  test_gpu_tree_sets.py compares the device with the same instances."""
import functools

import numpy as np
import pytest

import search_sets as S
import tree_sets as T

SPELLED_OUT = """# tree model: 6 variables, seed 3, 15 clauses of mul twice neg eq or3 bool
ALL;
C3 * C4 <= C1 + 2;
C3 * C4 = C1 + 1;
C6 * C1 != -2;
2 * C5 * C3 <= 6;
C4 + C4 <= C3 + 2;
C4 * C4 <= C6 + 2;
-(C5 + C4) < C2 - C1 + 5;
-C1 * C3 <= 3;
C5 + C2 = C6 + C4 - 1;
C3 + C5 != C6 + C4 - 1;
2 * C5 != C2 + C3;
C5 < C4 - 1 | C3 < C5 - 3 | C1 = C6 + 1;
(C6 < C4 + 4 & C5 = C1 - 2) | !(C2 <= C4 - 2);
!(C3 = C2 | C4 < C5 - 2);
C2 != C6 - 1 | C6 + C2 <= C1 - 1;
1 <= C1; C1 <= 6;
-5 <= C2; C2 <= 0;
-4 <= C3; C3 <= 1;
-1 <= C4; C4 <= 3;
-4 <= C5; C5 <= 1;
-2 <= C6; C6 <= 1;
"""

SPELLED_OUT_SAT = """# saturating products: 5 variables, seed 2, 6 clauses
ALL;
C5 * C3 * C4 <= C2 - 2138443013;
C5 < C4 + 51267;
C1 != C5 - 3605;
C4 != C1 - 47653;
3 * C1 * C2 <= C5 - 2133272301;
C4 <= C3 - 2605;
46328 <= C1; C1 <= 46378;
-46383 <= C2; C2 <= -46327;
1283 <= C3; C3 <= 1319;
-1314 <= C4; C4 <= -1263;
49939 <= C5; C5 <= 50002;
"""


@functools.lru_cache(maxsize=None)
def _instances(name):
    return T.instances(name)


def test_the_generator_is_a_function_of_its_arguments():
    """two calls give the same text; one short model with every tree shape and one saturating model are spelled out, so
    that a change of the generator cannot pass for the table's models; the predicates say what the text says"""
    for name in T.NAMES:
        assert T.text_of(name) == T.text_of(name)
    text, preds, bounds = T.generate(n=6, seed=3, shapes=T.FAMILIES, clauses=15, slack=2)
    assert text == SPELLED_OUT
    assert [p.shape for p in preds] == list(T.ALL_TREE_SHAPES) and all(p.tree for p in preds)
    assert bounds == [(1, 6), (-5, 0), (-4, 1), (-1, 3), (-4, 1), (-2, 1)]
    assert all(p(preds.planted) for p in preds)
    # C1 .. C6 = 2, -1, 1, 2, 0, 1: by hand, clause by clause
    x = (2, -1, 1, 2, 0, 1)
    assert [bool(p(x)) for p in preds] == [2 <= 4, 2 == 3, 2 != -2, 0 <= 6, 4 <= 3, 4 <= 3, -2 < 2, -2 <= 3, -1 == 2, 1 != 2,
                                           0 != 0, (0 < 1) or (1 < -3) or (2 == 2), (1 < 6 and 0 == 0) or not (-1 <= 0),
                                           not (1 == -1 or 2 < -2), (-1 != 0) or (0 <= 1)]
    text, preds, bounds = T.generate_sat(n=5, seed=2, clauses=6)
    assert text == SPELLED_OUT_SAT and all(p(preds.planted) for p in preds)
    # 50000 * 1300 * -1300 leaves the range: the reference's product is the sentinel, the comparison holds for
    # propagation (-inf <= anything) and is undecided for evaluation; 3 * 46340 * -46340 saturates the same way; the
    # others: 50000 < 49967, 46340 != 46395, -1300 != -1313, -1300 <= -1305
    x = (46340, -46340, 1300, -1300, 50000)
    assert [T.truth(p, x) for p in preds] == [(0, 1), (0, 0), (1, 1), (1, 1), (0, 1), (0, 0)]
    assert T.sat_mul(T.sat_mul(50000, 1300), -1300) == T.INT32_MIN and T.sat_mul(T.INT32_MAX, 0) == T.INT32_MAX
    assert T.sat_add(T.INT32_MIN, T.INT32_MAX) == T.INT32_MIN and T.sat_neg(T.INT32_MIN) == T.INT32_MAX
    assert T.sat_mul(46341, 46341) == T.INT32_MAX and T.sat_mul(46340, 46341) == 46340 * 46341


@pytest.mark.parametrize("name", T.NAMES)
def test_the_recorded_table_re_derives(name):
    assert T.derive(name, _instances(name)) == T.RECORDED[name]


@pytest.mark.parametrize("name", T.NAMES)
def test_structural_conditions(name):
    """what makes a set safe to send to a device and worth sending: the declared widths add up to at most 4,096 values
    and bound the oracle's propagations on every recorded instance (asserted here, before anything runs on a GPU), no
    bound is a sentinel, no tree has more than 256 nodes, the tables keep at least the recorded number of trees, and
    none of the tree shapes is counted as a linear or two-literal clause: the fast paths may only take clauses the
    generator wrote as binary relations or two-literal disjunctions"""
    rec = T.RECORDED[name]
    text, preds, bounds = T.generate_set(name)
    inst = _instances(name)
    om = inst["model"]
    assert rec["width"] == sum(hi - lo + 1 for lo, hi in bounds) <= T.MAX_TOTAL_WIDTH
    assert all(T.INT32_MIN + 2 ** 20 < lo <= hi < T.INT32_MAX - 2 ** 20 for lo, hi in bounds)
    root = om.domains()
    assert all(lo <= int(root[c, 0]) <= int(root[c, 1]) <= hi for c, (lo, hi) in zip(inst["columns"], bounds))
    assert 0 < rec["props"] == int(inst["props"].max()) <= rec["width"]
    clauses, on = T.host_tables(text, root)
    _, off = T.host_tables(text, root, fast_paths=False)
    assert clauses == om.n_clauses == 1 + len(preds) + 2 * len(bounds)
    assert on["tree_clauses"] >= rec["tree"] > 0 and on["max_tree"] == rec["longest"] <= T.MAX_TREE_NODES
    assert off["max_tree"] <= T.MAX_TREE_NODES
    # the root phase sweeps before it normalises: the trees as written must fit as well (a negative constant is one
    # node more there, NEG of a constant)
    assert T.host_tables(text, root, normalize=False)[1]["max_tree"] <= T.MAX_TREE_NODES
    plain = sum(not p.tree for p in preds)
    assert rec["linear_or2"] + rec["ne"] <= plain
    assert off["tree_clauses"] == rec["tree"] + rec["linear_or2"]  # the fast paths off: every clause but `!=` is a tree
    # a tree shape that survives the root phase is a tree whatever the fast paths: what is left of the tree-shaped
    # clauses cannot be fewer than the trees less the plain clauses that fell back to the interpreter
    assert rec["tree"] <= sum(p.tree for p in preds) + plain - rec["linear_or2"] - rec["ne"]
    assert 0 < rec["failed"] < rec["instances"] == len(inst["nodes"]) == sum(T.BATCHES)
    kinds = inst["nodes"][:, 0] < 0, (inst["nodes"][:, 0] >= 0) & (inst["nodes"][:, 1] < inst["nodes"][:, 2])
    assert kinds[0].sum() > 50 and kinds[1].sum() > 50, "full re-propagation and interval nodes are among the instances"


def test_the_table_holds_the_cases_the_gpu_tests_need():
    """one narrow set per operator family and a mixed one, every tree shape somewhere; the cross product of a
    brute-forced set is small; sat_prod's products leave the int32 range on some points and stay inside on others;
    mixed120 has more tree clauses than a wave has lanes; two classes of kernel 6 between mixed40 and mixed120, none for
    bigtab, whose adjacency alone is more than kernel 1 copies into LDS; the long sums are the longest the tables take"""
    R = T.RECORDED
    assert [n[7:] for n in T.NARROW] == ["mul", "neg", "eq", "or3", "bool", "mixed"] and len(T.TWICE) == 2
    seen = set()
    for name in T.NAMES:
        _, preds, bounds = T.generate_set(name)
        seen |= {p.shape for p in preds}
        if name in T.NARROW:
            assert 5 <= len(bounds) <= 7 and all(3 <= hi - lo + 1 <= 6 for lo, hi in bounds) and 8 <= len(preds) <= 14
            have = {p.shape for p in preds if p.tree}
            if name == "narrow_mixed":  # fourteen clauses, fifteen shapes: every family, most of them whole
                assert all(have & set(shapes) for shapes in T.TREE_SHAPES.values()) and len(have) >= 12
            else:
                assert have >= set(T.TREE_SHAPES[name[7:]])
        if name in T.TWICE:
            assert {p.shape for p in preds} == {"twice_add", "twice_mul"}
        if name in T.BRUTE:
            assert int(np.prod([hi - lo + 1 for lo, hi in bounds])) <= (600_000 if name == "longsum_prefix" else 200_000)
            assert R[name]["search"][2] > 0
    assert seen >= set(T.ALL_TREE_SHAPES) | set(T.PLAIN_SHAPES) | {"long_sum"}
    _, preds, bounds = T.generate_set("sat_prod")
    assert all(hi - lo + 1 <= 64 for lo, hi in bounds) and max(abs(b) for lohi in bounds for b in lohi) <= 51000
    rows, pts = T.points("sat_prod", list(range(len(bounds))), count=256)
    undecided = np.array([[p.decided is not None and not p.decided(x) for p in preds] for x in pts])
    products = [i for i, p in enumerate(preds) if p.decided is not None]
    assert len(products) >= 15 and undecided[:, products].any() and not undecided[:, products].all()
    assert any(undecided[:, i].any() and not undecided[:, i].all() for i in products), "a product saturates on a part of its domain"
    assert sum(not p.tree for p in preds) >= 5
    for name, n, cpl in (("mixed40", 40, 4), ("mixed120", 120, 8)):
        _, preds, bounds = T.generate_set(name)
        assert len(bounds) == n and 2 * n <= len(preds) <= 3 * n and 2 * sum(p.tree for p in preds) >= len(preds)
        assert R[name]["cpl"] == cpl and 2 * R[name]["tree"] >= R[name]["tree"] + R[name]["linear_or2"] + R[name]["ne"]
    assert R["mixed120"]["tree"] > 64
    assert R["bigtab"]["cpl"] is None and R["bigtab"]["tree"] >= 100
    _, on = T.host_tables(T.text_of("bigtab"), _instances("bigtab")["model"].domains())
    assert 4 * (R["bigtab"]["vars"] + 1) + 8 * on["adjacency_entries"] > 32 * 1024
    assert all(hi - lo + 1 <= 4 for lo, hi in T.generate_set("bigtab")[2])
    assert R["longsum"]["longest"] == T.MAX_TREE_NODES == 2 * T.LONGEST_SUM + 2
    print("longsum: longest tree", R["longsum"]["longest"], "nodes, the sum of", T.LONGEST_SUM // 2, "variables",
          2 * (T.LONGEST_SUM // 2) + 2)


def test_one_term_more_is_refused():
    """a sum of 128 variables is a tree of 258 nodes: building the tables fails with the limit's message"""
    from csolve_amd.solver import Model
    args = dict(T.SETS["longsum"]["args"], n=T.LONGEST_SUM + 1, sums=(T.LONGEST_SUM + 1,))
    text, _, bounds = T.generate(**args)
    m = Model.from_text(text)
    m.set_domains(S.oracle_model(text)[0].domains())
    m.normalize()
    with pytest.raises(Exception, match=r"a clause has 258 nodes, device limit is 256"):
        m.build_tables()


@pytest.mark.parametrize("name", T.BRUTE + ["sat_prod"])
def test_the_oracle_against_the_brute_force(name):
    """on every recorded instance of the sets a brute force can reach: a node the oracle calls consistent has a fixpoint
    that contains every satisfying point below the node, a node it fails has none (sat_prod: among 2,000 seeded points
    of the box below every node, and among a seeded sample of the whole box); with and without the normaliser the
    oracle answers the same, but for sat_prod's folded products"""
    inst = _instances(name)
    rows = T.solution_rows(name, inst["columns"])
    assert len(rows) > 0
    with_solutions = T.check_against_solutions(rows, inst["states"], inst["nodes"], inst["status"], inst["out"])
    if name == "sat_prod":
        hit, total = T.check_by_sampling(name, inst["columns"], inst["states"], inst["nodes"], inst["status"], inst["out"])
        print(name, "instances with a sampled solution below", hit, "sampled solutions", total)
        assert hit > 0 and total > 0
    else:
        assert with_solutions > 1000
        assert len(rows) == T.RECORDED[name]["search"][2]
    _, plain_oracle, _ = T.oracle_of(T.text_of(name), inst["model"].domains(), normalize=False)
    status, out, _ = plain_oracle.instances_nodes(inst["states"], inst["nodes"])
    ok = inst["status"] >= 0
    if name == "sat_prod":
        # a product that is +inf on all of the root box is a value to the normaliser, which folds it into a constant
        # (normalize.c:78-80 by way of eval.c:138-160); left in place, `product >= r` divides +inf by a factor
        # (propagate.c:249-286) and fails.  The reference searches the normalised model, and so does the device: the
        # plain model only ever fails more
        assert (ok | (status < 0)).all() and (ok & (status < 0)).any()
        ok = ok & (status >= 0)
    else:
        assert ((status >= 0) == ok).all()
    assert (out[ok] == inst["out"][ok]).all()


@pytest.mark.parametrize("name", T.SMALL + ["longsum_prefix"])
def test_complete_assignments(name):
    """complete assignments, satisfying and violating: the oracle finds one consistent exactly when every predicate
    holds, and clause i + 1 of the normalised model evaluates to predicate i's truth (undecided where a compared side is
    a sentinel) -- the order of the text, which the device tests rely on"""
    inst = _instances(name)
    om, orc, cols = inst["model"], inst["oracle"], inst["columns"]
    _, preds, bounds = T.generate_set(name)
    rows, pts = T.points(name, cols)
    root = om.domains()
    inside = ((rows >= root[:, 0]) & (rows <= root[:, 1])).all(1)
    good = bad = 0
    for row, x, ok in zip(rows, pts, inside):
        holds = all(bool(p(x)) for p in preds)
        state = np.stack([row, row], 1).astype(np.int32)
        st, out = orc.instance(state, -1, 0, 0)
        assert (st >= 0) == holds, (name, x.tolist())
        assert ok or not holds, "a satisfying point outside the root fixpoint"
        good, bad = good + holds, bad + (not holds)
        orc.set_domains(state)
        for i, p in enumerate(preds):
            got = orc.eval(om.view.clause_node[i + 1])
            # what the root phase decided is folded to its constant; a violated clause cannot have been
            assert got == T.truth(p, x) or (got == (1, 1) and not ok), (name, i, p.shape, x.tolist(), got)
    assert good > 0 and bad > 0


@pytest.mark.parametrize("name", T.SEARCHED)
def test_recorded_searches(name):
    """the ALL tree of the oracle-backed engine finds exactly the brute force's points, each once, and does not depend
    on the walking order"""
    st, found, eng = S.reference_walk(T.text_of(name))
    _, preds, bounds = T.generate_set(name)
    assert found == S.brute_force(preds, bounds) and len(found) == st["solutions"] and eng.complete_false == 0
    assert (st["nodes"], st["cuts"], st["solutions"]) == T.RECORDED[name]["search"]
    st1, found1, _ = S.reference_walk(T.text_of(name), 7, 99)
    assert (st1["nodes"], st1["cuts"], st1["solutions"]) == T.RECORDED[name]["search"] and found1 == found
