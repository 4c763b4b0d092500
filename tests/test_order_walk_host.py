"""Host tests of order_walk.py: the branching key against the reference's VarCmp vectors, the walk against what the
suite already records for the default rule, the table of trees under the five variable orders derived again, and that
the table can tell the rules apart.  test_gpu_order_trees.py compares the device engine with the same table."""
import json

import pytest

import order_walk as W
import search_sets as S
from conftest import golden


def test_branch_key_orders_variables_like_strategy_var_cmp():
    """the 70 comparisons of test/test_strategy.c VarCmp.*: sign(strategy_var_cmp(a, b)) = sign(key(b) - key(a)) with the
    index left out (test_host.py holds the library's csgpu_branch_key to the same vectors); ties go to the lower index,
    negative lower bounds come before positive ones, an unbounded interval is the largest"""
    cases = json.load(open(golden("ref_unit_strategy.json")))["cmp"]
    assert len(cases) == 70
    for c in cases:
        ka = W.branch_key(c["order"], c["prefer_failing"], *c["a"]["val"], c["a"]["prio"], 0) >> 32
        kb = W.branch_key(c["order"], c["prefer_failing"], *c["b"]["val"], c["b"]["prio"], 0) >> 32
        assert (kb > ka) - (kb < ka) == c["sign"], (c, ka, kb)
    assert {c["order"] for c in cases} == set(W.ORDERS)
    for order in W.ORDERS:
        for prefer in (False, True):
            assert W.branch_key(order, prefer, 1, 5, 7, 3) < W.branch_key(order, prefer, 1, 5, 7, 4)
    # the state part outranks the failure count, the failure count the index
    assert W.branch_key("smallest-domain", True, 1, 5, 0, 9) < W.branch_key("smallest-domain", True, 1, 6, 99, 0)
    assert W.branch_key("smallest-domain", True, 1, 5, 2, 9) < W.branch_key("smallest-domain", True, 1, 5, 1, 0)
    assert W.branch_key("none", False, 1, 5, 2, 1) < W.branch_key("none", False, 0, 1, 9, 2)
    assert W.branch_key("smallest-value", False, -3, 9, 0, 5) < W.branch_key("smallest-value", False, 2, 3, 0, 0)
    assert W.branch_key("largest-value", False, 0, 9, 0, 5) < W.branch_key("largest-value", False, 0, -2 + 10, 0, 0)
    assert W.branch_key("largest-value", False, -9, -2, 0, 5) < W.branch_key("largest-value", False, -9, -3, 0, 0)
    wide, unbounded = (-(2**31) + 1, 2**31 - 2), (0, W.INT32_MAX)
    assert W.branch_key("smallest-domain", False, *wide, 0, 1) < W.branch_key("smallest-domain", False, *unbounded, 0, 0)
    assert W.branch_key("largest-domain", False, *unbounded, 0, 1) < W.branch_key("largest-domain", False, *wide, 0, 0)
    assert W.branch_key("largest-domain", False, W.INT32_MIN, 0, 0, 1) < W.branch_key("largest-domain", False, *wide, 0, 0)


def test_luby_is_the_references_threshold_sequence():
    """the closed form against FailThresholdNext.Basic (test/test_csolve.c) and against its own recurrence: the sequence
    up to 2^k - 1 is the sequence up to 2^(k-1) - 1 twice, then 2^(k-1)"""
    want = json.load(open(golden("ref_unit_search.json")))["luby"]["thresholds"]
    assert [W.luby(k) for k in range(1, len(want) + 1)] == want == [1, 1, 2, 1, 1, 2, 4, 1, 1, 2, 1, 1, 2, 4, 8]
    seq = [1]
    for k in range(1, 9):
        seq = seq + seq + [1 << k]
    assert [W.luby(k) for k in range(1, len(seq) + 1)] == seq


@pytest.mark.parametrize("name", W.SET_NAMES)
def test_the_walk_under_the_default_rule_equals_the_existing_records(name):
    """all_tree(text, "smallest-domain") is the tree the suite already records: search_sets.SETS for the clause sets
    (the oracle-backed engine's walk), test_gpu_search.oracle_all_tree for the != networks, propagations included"""
    got = W.walk(name, "smallest-domain")
    if name in S.SETS:
        rec = S.SETS[name]
        assert (got["nodes"], got["cuts"], got["solutions"], got["halvings"]) == (rec["nodes"], rec["cuts"], rec["solutions"], rec["halvings"])
        assert got["found"] == S.reference_walk(S.text_of(name))[1]
    else:
        from test_gpu_search import oracle_all_tree
        om, _ = S.oracle_model(W.text_of(name))
        assert got["halvings"] == 0
        assert (got["nodes"], got["cuts"], got["solutions"], got["props"]) == oracle_all_tree(W.text_of(name), om.domains())
    assert len(got["found"]) == got["solutions"] and got["complete_false"] == 0


@pytest.mark.parametrize("name", W.SETS_OF_THE_TABLE)
def test_the_table_is_what_the_walk_derives(name):
    """every recorded (nodes, cuts, solutions, halvings) derived again, within the cap; the solution set is the same
    under every order, and no complete state evaluates false"""
    default = W.walk(name, "smallest-domain")
    for order in W.orders_of(name):
        got = W.walk(name, order)
        print(name, order, {k: got[k] for k in ("nodes", "cuts", "solutions", "halvings", "props")})
        assert (got["nodes"], got["cuts"], got["solutions"], got["halvings"]) == W.RECORDED[name, order]
        assert got["nodes"] <= W.CAP or (name, order) in W.OVER_CAP
        assert got["found"] == default["found"] and got["solutions"] == len(got["found"])
        assert got["complete_false"] == 0


def test_the_table_holds_every_pair_it_may():
    """every set under every order, but for the pairs whose trees are beyond the cap (order_walk.RECORDED's comment)"""
    left_out = {("wide3_sums", "largest-domain"), ("wide3_sums", "smallest-value")} | {("offsets40x8", o) for o in W.NON_DEFAULT}
    assert set(W.RECORDED) == {(n, o) for n in W.SET_NAMES for o in W.ORDERS} - left_out
    assert W.SETS_OF_THE_TABLE == W.SET_NAMES


@pytest.mark.parametrize("name", [n for n in W.SETS_OF_THE_TABLE if len(W.orders_of(n)) >= 3])
def test_the_table_can_tell_the_rules_apart(name):
    """at least three of a set's orders walk trees of different (nodes, cuts)"""
    trees = {W.RECORDED[name, o][:2] for o in W.orders_of(name)}
    assert len(trees) >= 3, trees


def test_only_one_set_is_recorded_under_fewer_than_three_orders():
    """offsets40x8, under the default rule alone: its other trees are beyond reach of a host walk"""
    assert [n for n in W.SETS_OF_THE_TABLE if len(W.orders_of(n)) < 3] == ["offsets40x8"]
    assert W.orders_of("offsets40x8") == ["smallest-domain"] and list(W.OVER_CAP) == [("offsets40x8", "smallest-domain")]
    assert all(len(W.orders_of(n)) == 5 for n in W.SETS_OF_THE_TABLE if n not in ("offsets40x8", "wide3_sums"))


def test_pigeonhole_models_are_infeasible_with_the_recorded_trees():
    """what the restart tests walk: no solution, the whole tree 1,936 / 1,420 nodes / cuts for seven variables and
    14,978 / 11,359 for eight; the extra sum clause of tree=True cuts nothing the pairs do not cut"""
    for n, tree, want in ((7, False, (1936, 1420)), (8, False, (14978, 11359)), (7, True, None)):
        got = W.all_tree(W.pigeon(n, tree, "ALL"), "smallest-domain")
        assert got["solutions"] == 0 and got["complete_false"] == 0 and not got["found"]
        print("pigeon", n, tree, got["nodes"], got["cuts"])
        if want is not None:
            assert (got["nodes"], got["cuts"]) == want
        assert W.pigeon(n, tree, "ALL").replace("ALL;", "ANY;", 1) == W.pigeon(n, tree)
    assert "X0 + X1 < 12;" in W.pigeon(7, True) and "+" not in W.pigeon(7)
