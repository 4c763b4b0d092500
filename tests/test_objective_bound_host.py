"""Host tests of objective_sets.py: the two statements of the reference of the fixpoint under an incumbent agree on every
drawn instance; the draw holds the classes the GPU tests need; the Python statement of the bound is the exported
csgpu_objective_bound; the recorded MIN / MAX trees re-derive from the oracle-backed engine, whose per-iteration incumbent
walks another tree than its immediate one; on the narrow sets the recorded optimum is the brute force's extreme.
test_gpu_objective_bound.py compares the device with the same instances and the same table."""
import functools

import numpy as np
import pytest

import objective_sets as O
import search_sets as S

INT32_MAX, INT32_MIN = O.INT32_MAX, O.INT32_MIN
PAIR_IDS = [O.pair_id(p) for p in O.PAIRS]


@functools.lru_cache(maxsize=None)
def _instances(pair):
    inst = O.draw(pair)
    inst.update(O.refer(inst, both_ways=True))
    return inst


@pytest.mark.parametrize("pair", O.PAIRS, ids=PAIR_IDS)
def test_both_statements_of_the_reference_agree_and_the_classes_are_there(pair):
    """the reference's order (the node, the bound, the clauses of "<obj>") and the round-based one (assignment and bound
    written in, every clause to the fixpoint) give the same verdict and the same fixpoint on every instance (refer()
    asserts it node by node); the draw has the recorded class counts, and they hold the conditions the GPU tests rest on:
    bounds that change nothing, bounds that empty "<obj>", bounds whose narrowing reaches another variable -- the class
    a missing mark on "<obj>" gets wrong -- or fails only in the propagation that follows, nodes on "<obj>" itself"""
    inst = _instances(pair)
    counts = O.class_counts(inst)
    print(O.pair_id(pair), counts)
    assert sum(counts.values()) == len(inst["nodes"]) == O.draws_of(pair) + O.ON_OBJECTIVE + O.BOTH + O.CROSSED + O.UNBOUNDED
    assert counts == O.CLASS_COUNTS[pair]
    assert counts["unmoved"] >= 100 and counts["empty"] >= 200
    if pair == O.NARROW_FAIL_PAIR:
        assert counts["narrow_fail"] >= 100
    else:
        assert counts["narrow_other"] >= 40
    assert int((inst["nodes"][:, 0] == inst["obj"]).sum()) >= 50
    assert int((inst["nodes"][:, 0] == -1).sum()) >= 50 and int((inst["nodes"][:, 1] < inst["nodes"][:, 2]).sum()) >= 100
    # the slices: both bounds set, crossed bounds (every consistent child of those is emptied), no bound (nothing moves)
    sl, b, k = inst["slices"], inst["bounds"], inst["klass"]
    assert (b[sl["both"], 0] > INT32_MIN).all() and (b[sl["both"], 1] < INT32_MAX).all()
    assert (b[sl["both"], 0] <= b[sl["both"], 1]).all()
    assert (b[sl["crossed"], 0] > b[sl["crossed"], 1]).all() and set(k[sl["crossed"]]) <= {"plain_fail", "empty"}
    assert (b[sl["unbounded"]] == O.NO_BOUND).all() and set(k[sl["unbounded"]]) <= {"plain_fail", "unmoved"}
    # every parent is a fixpoint: the oracle's full re-propagation leaves it alone
    for state in inst["states"]:
        st, again = inst["oracle"].instance(state, -1, 0, 0)
        assert st >= 0 and (again == state).all()


def test_the_narrow_pairs_fail_in_the_propagation_after_the_bound():
    assert sum(O.class_counts(_instances(p))["narrow_fail"] for p in O.NARROW_PAIRS) >= 20


@pytest.mark.parametrize("pair", [O.PAIRS[0], O.PAIRS[5]], ids=[PAIR_IDS[0], PAIR_IDS[5]])
def test_the_reference_under_one_bound_for_all(pair):
    """the bound the batch-size tests give every node of a pair moves some of them and leaves others"""
    inst = _instances(pair)
    bound = O.common_bound(inst)
    ref = O.refer(inst, np.tile(np.array(bound, dtype=np.int64), (len(inst["nodes"]), 1)), both_ways=True)
    kinds = set(ref["klass"])
    assert "unmoved" in kinds and "empty" in kinds and len(kinds) >= 4


def test_the_bound_in_python_is_the_exported_one():
    """objective_bound() against csgpu_objective_bound: incumbents around and at both ends of "<obj>" (an incumbent at the
    lower end under MIN, at the upper end under MAX, leaves an empty interval), the "none yet" sentinels (INT32_MAX under
    MIN, INT32_MIN under MAX: the arithmetic saturates and nothing moves), the sentinels of the other side, and ALL / ANY"""
    from csolve_amd import _lib
    L = _lib.load_library()
    code = {0: 0, 1: 2, 2: 3}  # sense -> the objective of csolve_gpu.h (0 ANY, 1 ALL, 2 MIN, 3 MAX)
    intervals = [(-5, 7), (0, 0), (-1700, -80), (3, 362), (INT32_MIN, INT32_MAX), (INT32_MIN, 4), (-4, INT32_MAX)]
    for lo, hi in intervals:
        bests = {lo - 1, lo, lo + 1, (lo + hi) // 2, hi - 1, hi, hi + 1, 0, INT32_MAX, INT32_MIN, INT32_MAX - 1, INT32_MIN + 1}
        for best in sorted(b for b in bests if INT32_MIN <= b <= INT32_MAX):
            for sense in (0, 1, 2):
                got = L.csgpu_objective_bound(code[sense], _lib.Val(lo, hi), best)
                assert (got.lo, got.hi) == O.objective_bound(sense, lo, hi, best), (sense, lo, hi, best)
    assert O.objective_bound(1, -5, 7, INT32_MAX) == (-5, 7) and O.objective_bound(2, -5, 7, INT32_MIN) == (-5, 7)
    assert O.objective_bound(1, -5, 7, -5) == (-5, -6) and O.objective_bound(2, -5, 7, 7) == (8, 7)
    assert O.objective_bound(1, *O.NO_BOUND, 12) == (INT32_MIN, 11) and O.objective_bound(2, *O.NO_BOUND, 12) == (13, INT32_MAX)
    got = L.csgpu_objective_bound(1, _lib.Val(-5, 7), 3)  # ALL: no bound
    assert (got.lo, got.hi) == (-5, 7)


def test_propagate_obj_checks_its_arguments_before_it_touches_the_device():
    """bounds outside int32 and tensors that are not on the device are refused on a model that is not even finalized"""
    import torch

    from csolve_amd.solver import Model
    model = Model.from_text(S.text_of("narrow_sums7", "MIN C3"))
    states = torch.zeros((1, model.n_vars, 2), dtype=torch.int32)
    nodes = torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(ValueError):
        model.propagate_obj(states, nodes, INT32_MIN - 1, 0)
    with pytest.raises(ValueError):
        model.propagate_obj(states, nodes, 0, INT32_MAX + 1)
    with pytest.raises(AssertionError):
        model.propagate_obj(states, nodes, *O.NO_BOUND)  # host tensors
    model.close()


@pytest.mark.parametrize("name", list(S.SETS))
def test_the_recorded_trees_rederive(name):
    """TREES against the oracle-backed engine with the per-iteration incumbent, one parent per iteration and 64: nodes,
    cuts, solutions, iterations, pool peak and optimum; the optimum is the table's of search_sets (on the narrow sets the
    brute force's extreme, test_search_sets_host.py); best_row attains it; and on the sets the drive modes are compared
    on, the tree of the host-driven loop, whose incumbent arrives one iteration later"""
    for which, (objective, optimum, value) in zip(O.OBJECTIVES, S.optimisations(name)):
        for parents in O.PARENTS:
            tree, eng = O.engine_tree(name, objective, parents)
            assert tree == O.TREES[name, which, parents], (name, which, parents, tree)
            assert tree[0] <= 50000
            if optimum is None:
                assert tree[2] == 0 and eng.best_row is None
                assert tree[5] == (INT32_MAX if objective.startswith("MIN") else INT32_MIN)
            else:
                assert tree[5] == optimum and eng.best_row is not None
                cols = S.columns(eng.m.names())
                assert value([int(eng.best_row[c]) for c in cols]) == optimum == int(eng.best_row[eng.obj_var])
            if name in O.LAGGED_SETS:
                lagged, _ = O.engine_tree(name, objective, parents, lag=1)
                assert lagged == O.LAGGED_TREES[name, which, parents], (name, which, parents, lagged)
                assert lagged[5] == tree[5] and lagged[0] >= tree[0]


def test_the_incumbent_rule_changes_the_tree():
    """the per-iteration incumbent is another walk than the immediate one (same nodes at one parent per iteration, where
    a parent's children are all that differ, but other cuts and solutions), and 64 parents another again: the GPU tests
    can tell which of them the device walks"""
    per, _ = O.engine_tree("narrow_sums7", "MIN C3", 1)
    now, _ = O.engine_tree("narrow_sums7", "MIN C3", 1, incumbent="immediate")
    assert per[:3] == (63, 41, 4) and now[:3] == (63, 43, 2)
    assert O.TREES["narrow_sums7", "min-var", 64][:3] == (765, 531, 29)
    per, _ = O.engine_tree("wide3_sums", "MIN C1", 1)
    now, _ = O.engine_tree("wide3_sums", "MIN C1", 1, incumbent="immediate")
    assert per[:3] == (659, 422, 223) and now[:3] == (659, 644, 1)
    # and the lag of the host-driven loop is visible as well
    assert any(O.LAGGED_TREES[k] != O.TREES[k] for k in O.LAGGED_TREES)


def test_the_narrow_optima_are_the_brute_forces():
    for name in S.NARROW:
        rec = S.SETS[name]
        _, preds, bounds = S.generate(**rec["args"])
        want = S.brute_force(preds, bounds)
        for which, (objective, optimum, value) in zip(O.OBJECTIVES, S.optimisations(name)):
            pick = min if objective.startswith("MIN") else max
            extreme = pick(map(value, want)) if want else (INT32_MAX if objective.startswith("MIN") else INT32_MIN)
            for parents in O.PARENTS:
                assert O.TREES[name, which, parents][5] == extreme, (name, which, parents)
