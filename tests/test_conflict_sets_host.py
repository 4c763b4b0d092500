"""Host tests of the learnt-conflict sets of conflict_sets.py: the recorded table and the class counts re-derive; on every
instance the oracle (the conflict clauses in its model, the reference's weak propagate_confl) and the strong reference
keep the two facts the GPU tests judge a device by; on the brute-forced sets the strong reference itself is held against
the enumeration; and no instance takes more propagations than 4,096, asserted here before anything reaches a device.
test_gpu_conflict_sets.py runs the same instances on the device."""
import numpy as np
import pytest

import conflict_sets as K


@pytest.mark.parametrize("name", K.NAMES)
def test_the_recorded_table_re_derives(name):
    assert K.derive(name) == K.RECORDED[name]


@pytest.mark.parametrize("name", K.NAMES)
def test_structural_conditions_and_class_minima(name):
    """finite declared bounds whose widths add up to at most 4,096; twelve clauses of 1 to 6 elements (long255: up to
    255), among them a variable twice at one value, a variable twice at two values and a one-element clause; conflict
    values on bounds, inside, off the root domain and negative; the planted row violates no clause; every class the set
    can reach holds at least 50 instances; value, interval and var = -1 nodes are among them"""
    b, inst, rec = K.build(name), K.instances(name), K.RECORDED[name]
    if b["bounds"] is not None:
        assert sum(hi - lo + 1 for lo, hi in b["bounds"]) <= K.MAX_TOTAL_WIDTH
    assert rec["width"] <= K.MAX_TOTAL_WIDTH
    clauses, root = b["clauses"], b["plain"].domains()
    assert len(clauses) == K.CONFLICTS and rec["clauses"] == rec["base_clauses"] + K.CONFLICTS
    longest = K.MAX_CONFLICT if name == "long255" else 6
    assert all(1 <= len(c) <= longest for c in clauses) and rec["longest_conflict"] == max(len(c) for c in clauses)
    assert all(0 <= v < b["plain"].n_vars for c in clauses for v, _ in c)
    twice = [c for c in clauses if len({v for v, _ in c}) < len(c)]
    assert any(len(set(c)) < len(c) for c in twice), "a variable twice at one value"
    assert any(len(set(c)) == len(c) for c in twice), "a variable twice at two values"
    assert any(len(c) == 1 for c in clauses)
    if b["planted"] is not None:
        assert not any(all(b["planted"][v] == cv for v, cv in c) for c in clauses)
    where = {"lo": 0, "hi": 0, "interior": 0, "outside": 0, "negative": 0}
    for c in clauses:
        for v, cv in c:
            lo, hi = int(root[v, 0]), int(root[v, 1])
            where["lo"] += cv == lo
            where["hi"] += cv == hi
            where["interior"] += lo < cv < hi
            where["outside"] += cv < lo or cv > hi
            where["negative"] += cv < 0
    print(name, "conflict values:", where)
    assert where["lo"] and where["hi"] and where["interior"]
    # values one off the root domain and negative ones: drawn on every set of arbitrary clauses; implied and learnt
    # clauses are consistent decisions of the base model, so their values lie inside the domains (conflict_sets.SETS)
    if K.SETS[name]["kind"] in ("arbitrary", "long"):
        assert where["outside"] and where["negative"], (name, where)
    if name == "wide_negative":
        assert 2 * where["interior"] > sum(len(c) for c in clauses)
        assert (root[:, 1] < 0).any() and ((root[:, 0] < 0) & (root[:, 1] > 0)).any()
        assert all(250 <= hi - lo + 1 <= 330 for lo, hi in b["bounds"])
    unreachable = K.SETS[name].get("unreachable", ())
    for k in K.CLASSES:
        if k in unreachable:
            assert rec["classes"][k] == 0, (name, k)
        else:
            assert rec["classes"][k] >= K.CLASS_MINIMUM, (name, k, rec["classes"][k])
    nodes = inst["nodes"]
    assert abs(len(nodes) - K.TARGET) <= 8 and 0 < rec["failed"] < len(nodes)
    assert (nodes[:, 0] < 0).sum() > 20 and ((nodes[:, 0] >= 0) & (nodes[:, 1] < nodes[:, 2])).sum() > 50
    # every node lies inside its parent, every parent is a consistent row
    st = inst["states"]
    assert (st[:, :, 0] <= st[:, :, 1]).all()
    rows = np.nonzero(nodes[:, 0] >= 0)[0]
    par = st[nodes[rows, 3], nodes[rows, 0]]
    assert (par[:, 0] <= nodes[rows, 1]).all() and (nodes[rows, 1] <= nodes[rows, 2]).all() and (nodes[rows, 2] <= par[:, 1]).all()
    assert (par[:, 0] < par[:, 1]).all(), "a node's variable is open in its parent"


def test_the_table_holds_the_shapes_the_gpu_tests_need():
    R = K.RECORDED
    for name in K.NARROW:
        bounds = K.build(name)["bounds"]
        assert 6 <= len(bounds) <= 7 and all(3 <= hi - lo + 1 <= 9 for lo, hi in bounds)
    assert [R[n]["cpl"] for n in ["narrow_implied"] + K.K6_CLASSES] == [1, 2, 4, 8]
    assert [R[n]["cpl_base"] for n in K.K6_CLASSES] == [1, 2, 4], "the twelve clauses move each model one class up"
    assert R["across512"]["base_clauses"] == 505 and R["across512"]["cpl_base"] == 8 and R["across512"]["cpl"] is None
    assert R["long255"]["vars"] == 256 and R["long255"]["longest_conflict"] == K.MAX_CONFLICT == 255
    b = K.build("long255")
    assert sorted(len(c) for c in b["clauses"])[-3:] == [255] * 3 and [b["clauses"][i][0][1] for i in range(3)] == [0, 2, 1]
    # nodes of long255 with 253, 254 and 255 elements of a long clause at their conflict values
    inst = K.instances("long255")
    fixed = {253: 0, 254: 0, 255: 0}
    for dom in K.below(inst["states"], inst["nodes"]):
        for c in b["clauses"][:3]:
            k = sum(dom[v, 0] == dom[v, 1] == cv for v, cv in c)
            if k in fixed:
                fixed[k] += 1
    print("long255: nodes that fix 253 / 254 / 255 elements of a long clause:", fixed)
    assert all(v >= 20 for v in fixed.values())
    assert R["queens12_learnt"]["vars"] == 12 and "violated" in K.SETS["queens12_learnt"]["unreachable"]


@pytest.mark.parametrize("name", K.NAMES)
def test_the_oracle_keeps_the_two_facts_on_every_instance(name):
    """the oracle with the conflict clauses in its model against the strong reference, on every instance: S consistent
    -> the oracle's end state equals S; S failed -> the oracle fails or ends in a state that violates a clause.  And the
    propagation bound: no instance takes more than the set's total width, at most 4,096"""
    b, inst, rec = K.build(name), K.instances(name), K.RECORDED[name]
    consistent_but_violated = 0
    for i in range(len(inst["nodes"])):
        consistent_but_violated += K.judge(inst["failed"][i], inst["out"][i], inst["status"][i] < 0, inst["weak"][i], b["clauses"],
                                           (name, i, inst["nodes"][i].tolist()))
    assert consistent_but_violated == rec["oracle_violated"]
    assert 0 < int(inst["props"].max()) == rec["props"] <= rec["width"] <= K.MAX_TOTAL_WIDTH
    # the strong reference's outputs are fixpoints of itself and of the oracle
    ok = np.nonzero(~inst["failed"])[0]
    for i in ok[:: max(1, len(ok) // 200)]:
        f, again, _ = K.strong(b["plain_oracle"], b["clauses"], inst["out"][i])
        st, weak = b["full_oracle"].instance(inst["out"][i], -1, 0, 0)
        assert not f and (again == inst["out"][i]).all() and st >= 0 and (weak == inst["out"][i]).all()


@pytest.mark.parametrize("name", K.BRUTE)
def test_the_strong_reference_against_the_brute_force(name):
    """every consistent S holds every solution of model and clauses below its node, a failed S has none; the implied
    clauses leave the solution set of the base model unchanged (the arbitrary ones cut some solutions off)"""
    b, inst = K.build(name), K.instances(name)
    dom = K.below(inst["states"], inst["nodes"])
    with_solutions = 0
    for i in range(len(dom)):
        under = K.solutions_below(name, dom[i])
        with_solutions += bool(under.any())
        if inst["failed"][i]:
            assert not under.any(), (name, i, "a failed node has a solution below it")
        else:
            assert (K.solutions_below(name, inst["out"][i]) == under).all(), (name, i, "the fixpoint loses a solution")
    assert with_solutions > 100
    everything = np.stack([b["rows"].min(0), b["rows"].max(0)], 1)
    kept = int(K.solutions_below(name, everything).sum())
    print(name, "solutions of the base model", len(b["rows"]), "of model and clauses", kept)
    if K.SETS[name]["kind"] == "implied":
        assert kept == len(b["rows"])
    else:
        assert 0 < kept <= len(b["rows"])


@pytest.mark.parametrize("name", K.SEARCHED)
def test_recorded_searches(name):
    """the ALL tree of the oracle-backed engine with the implied clauses in its model finds exactly the solutions of the
    base model (the brute force's; queens-12: the recorded 14,200); its nodes against the same search without the
    clauses are recorded: SEARCH holds both counts and says whether the clauses ever cost a node"""
    b = K.build(name)
    got = K.search_walk(name)
    assert got == K.SEARCH[name] and got["found"]
    # what test_gpu_conflict_sets.py may assert of a device search: the clauses never cost the oracle-backed engine a node
    assert got["with"][0] <= got["without"][0] and got["with"][1] <= got["without"][1]
    if name == "queens12_learnt":
        assert got["with"][2] == got["without"][2] == K.QUEENS12_SOLUTIONS
    else:
        assert got["with"][2] == got["without"][2] == len(b["rows"])
