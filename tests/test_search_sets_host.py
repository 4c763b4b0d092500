"""Host tests of the clause-model sets of search_sets.py: the generator is pinned, and everything its table records is
derived again -- the ALL trees and the optima by the oracle-backed engine (cpu_engine.OracleEngine), the solution sets
of the narrow sets by a brute force over the cross product of the bounds, which needs neither the oracle nor the
front end.  test_gpu_search_sets.py compares the device engine with the same table."""
import functools

import pytest
import torch

import search_sets as S
from csolve_amd.parallel import INT32_MAX, INT32_MIN

NAMES = list(S.SETS)

SPELLED_OUT = """# clause model: 4 variables, seed 16, width 4, 1 wide
ALL;
C2 != C3 - 7;
C2 > C3 - 5 | C2 > C3 - 5;
C4 < C1 + 198;
3 * C4 + C1 <= -191;
C4 = C3 + 1;
C2 + C3 <= C1 + 189;
2 * C2 + C3 <= -7;
C3 <= C2 + 7;
C2 < C1 + 189;
C2 + C1 <= C2 - 195;
-365 <= C1; C1 <= -23;
-5 <= C2; C2 <= -4;
0 <= C3; C3 <= 2;
1 <= C4; C4 <= 3;
"""


@functools.lru_cache(maxsize=None)
def _walk(name, objective="ALL", parents=64, shuffle=None):
    st, found, eng = S.reference_walk(S.text_of(name, objective), parents, shuffle)
    return st, found, eng.halvings, tuple(eng.halved), eng.complete_false


def test_the_generator_is_a_function_of_its_arguments():
    """two calls give the same text; one short model is spelled out, every clause shape in it, so that a change of the
    generator cannot pass for the table's models; the predicates say what the text says"""
    for name in NAMES:
        assert S.text_of(name) == S.text_of(name)
    args = dict(n=4, seed=16, width=4, clauses=10, wide=1)
    text, preds, bounds = S.generate(**args)
    assert text == SPELLED_OUT
    assert bounds == [(-365, -23), (-5, -4), (0, 2), (1, 3)] and len(preds) == 10
    # the objective is the header only
    assert S.generate(objective="MIN C3", **args)[0] == SPELLED_OUT.replace("ALL;", "MIN C3;", 1)
    # C1 = -200, C2 = -5, C3 = 0, C4 = 1: by hand, clause by clause
    x = (-200, -5, 0, 1)
    assert [bool(p(x)) for p in preds] == [-5 != -7, -5 > -5, 1 < -2, 3 - 200 <= -191, 1 == 1, -5 <= -11, -10 <= -7, 0 <= 2,
                                           -5 < -11, -205 <= -200]
    # a planted model keeps its hidden point: feasible whatever the number of clauses
    text, preds, bounds = S.generate(n=12, seed=9, width=4, clauses=60, plant=True)
    assert S.reference_walk(text)[0]["solutions"] >= 1


@pytest.mark.parametrize("name", S.NARROW)
def test_narrow_sets_equal_a_brute_force(name):
    """the oracle walk's solutions are the points of the cross product that satisfy every predicate: the same set, the
    recorded count, the recorded extremes of both objectives"""
    rec = S.SETS[name]
    _, preds, bounds = S.generate(**rec["args"])
    want = S.brute_force(preds, bounds)
    st, found, _, _, _ = _walk(name)
    assert found == want
    assert len(want) == rec["solutions"] == st["solutions"]
    for _, optimum, value in S.optimisations(name):
        if optimum is None:
            assert not want
    if want:
        k = rec["obj"] - 1
        assert rec["var"] == (min(x[k] for x in want), max(x[k] for x in want))
        assert rec["expr"] == (min(map(S.expression_value, want)), max(map(S.expression_value, want)))


@pytest.mark.parametrize("name", NAMES)
def test_recorded_all_trees_and_optima(name):
    """the table against the oracle-backed engine: nodes, cuts, solutions and halvings of the ALL tree, no complete
    state that evaluates false, every solution a point the predicates accept, and MIN / MAX of the objective variable
    and of the expression end at the extremes over the solution set (an infeasible set at the sentinels)"""
    rec = S.SETS[name]
    st, found, halvings, _, complete_false = _walk(name)
    assert (st["nodes"], st["cuts"], st["solutions"], halvings) == (rec["nodes"], rec["cuts"], rec["solutions"], rec["halvings"])
    assert st["nodes"] <= 50000 and complete_false == 0 and len(found) == st["solutions"]
    _, preds, bounds = S.generate(**rec["args"])
    for x in found:
        assert all(lo <= v <= hi for v, (lo, hi) in zip(x, bounds)) and all(p(x) for p in preds)
    for objective, optimum, value in S.optimisations(name):
        so, fo, _, _, false_o = _walk(name, objective)
        assert so["done"] == 1 and false_o == 0
        if optimum is None:
            assert so["solutions"] == 0 and not fo
            assert so["best"] == (INT32_MAX if objective.startswith("MIN") else INT32_MIN)
        else:
            pick = min if objective.startswith("MIN") else max
            assert so["best"] == optimum == pick(value(x) for x in found)
            assert fo <= found and optimum in {value(x) for x in fo}


@pytest.mark.parametrize("name", NAMES)
def test_the_walking_order_does_not_matter(name):
    """one parent per iteration (depth first), seven, and sixty-four with the pool shuffled after every iteration: the
    same ALL tree and the same optima -- what lets the device engine, which batches as its buffers allow, be compared
    with one recorded walk"""
    base = _walk(name)
    for parents, shuffle in ((1, None), (7, None), (64, 1234)):
        st, found, halvings, halved, _ = _walk(name, "ALL", parents, shuffle)
        assert (st["nodes"], st["cuts"], st["solutions"], halvings) == (base[0]["nodes"], base[0]["cuts"], base[0]["solutions"], base[2])
        assert found == base[1] and sorted(halved) == sorted(base[3])
    for objective, optimum, _ in S.optimisations(name)[:2]:
        for parents, shuffle in ((1, None), (7, 99)):
            assert _walk(name, objective, parents, shuffle)[0]["best"] == _walk(name, objective)[0]["best"]


def test_the_table_holds_the_cases_the_gpu_tests_need():
    """narrow, halving (the sign cases among the halved intervals), infeasible, negative optimum, more solutions than
    the store keeps, with and without expression-tree clauses, a wide objective variable"""
    sets = S.SETS
    assert len(S.NARROW) >= 3 and len(S.WIDE) >= 3 and len(S.INFEASIBLE) >= 1
    for name in S.NARROW:
        _, _, bounds = S.generate(**sets[name]["args"])
        points = 1
        for lo, hi in bounds:
            points *= hi - lo + 1
        assert points <= 3_000_000
    for name in S.INFEASIBLE:  # consistent at the root: the search, not the root phase, finds it out
        assert sets[name]["nodes"] > 0 and sets[name]["cuts"] > 0
    assert any(sets[k]["var"][0] < 0 for k in S.FEASIBLE) and any(sets[k]["expr"][0] < 0 for k in S.FEASIBLE)
    assert any(sets[k]["solutions"] > 1024 for k in NAMES) and any(0 < sets[k]["solutions"] <= 1024 for k in NAMES)
    assert sum(sets[k]["tree"] for k in NAMES) >= 2 and sum(not sets[k]["tree"] for k in NAMES) >= 2
    assert any(sets[k]["tree"] for k in S.WIDE) and any(not sets[k]["tree"] for k in S.WIDE)
    halved = {name: _walk(name)[3] for name in S.WIDE}
    for name in S.WIDE:
        assert len(halved[name]) == sets[name]["halvings"] > 0
        assert all(hi - lo + 1 > 256 for lo, hi in halved[name])
    everything = [iv for ivs in halved.values() for iv in ivs]
    assert any(lo + hi < 0 for lo, hi in everything)
    # lo + hi negative AND odd: where rounding the middle toward zero instead of down gives another split
    assert any(lo + hi < 0 and (lo + hi) % 2 == 1 for lo, hi in everything)
    assert any(lo < 0 < hi and (hi - lo + 1) % 2 == 1 for lo, hi in everything)
    assert any(lo > 0 for lo, hi in everything)
    # and the rounding is visible in a recorded tree: with the middle rounded toward zero wide2_mid's walk counts other nodes
    from cpu_engine import OracleEngine

    class TowardZero(OracleEngine):
        @staticmethod
        def _middle(lo, hi):
            return int((lo + hi) / 2)

    om, _ = S.oracle_model(S.text_of("wide2_mid"))
    eng = TowardZero(om, parents_per_iteration=64)
    eng.put(torch.from_numpy(om.domains()).unsqueeze(0).contiguous())
    st = eng.run(1 << 40)
    assert st["done"] == 1 and st["solutions"] == sets["wide2_mid"]["solutions"] and st["nodes"] != sets["wide2_mid"]["nodes"]
    # an objective variable that is itself wide at the root, and halved
    wide_objective = 0
    for name in S.WIDE:
        om, cols = S.oracle_model(S.text_of(name))
        lo, hi = om.domains()[cols[sets[name]["obj"] - 1]]
        wide_objective += int(hi) - int(lo) + 1 > 256
    assert wide_objective >= 1


@pytest.mark.parametrize("name", NAMES)
def test_the_tree_clause_flag_is_the_tables(name):
    """`tree`: whether the product's tables keep expression-tree clauses for the set under the default fast paths (the
    host-only table build, from the oracle's root domains)"""
    assert (S.host_tree_clauses(S.text_of(name)) > 0) == S.SETS[name]["tree"]
