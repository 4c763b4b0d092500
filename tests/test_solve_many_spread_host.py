"""CPU tests of the spread of stopped ALL walks (csgpu_many_checkpoint_children / _fanout, csgpu_many_fold,
Model.solve_many_spread): the interface is declared, exported and prototyped; the argument errors in their documented
order, without a device; and the identity the spread rests on, on the host walk of tests/many_spread_walk.py against the
one-budget walk of tests/many_walk.py: the children of a stopped walk, walked as root rows of their own and folded back
over any number of levels, give the record of the one ALL walk field for field, and its first solution."""
import ctypes as C
import re

import numpy as np
import pytest

import many_sets
import many_spread_walk
import many_walk

E_ARG = -1
FIELDS = ("status", "root_props", "nodes", "cuts", "props", "solutions")
NEW_CALLS = {"csgpu_many_checkpoint_children": 5, "csgpu_many_checkpoint_fanout": 8, "csgpu_many_fold": 5}
BUDGETS = ((16, 64), (1, 7, 56))
_spreads, _dives = {}, {}


def _dive(name, text, roots, i):
    if (name, i) not in _dives:
        _dives[name, i] = many_walk.dive(text, roots[i], "ALL")
    return _dives[name, i]


def _spread(name, budgets, rows=8):
    """(the spread of the first `rows` rows of a set, its info, text, roots), walked once"""
    if (name, budgets, rows) not in _spreads:
        text, roots, _, _ = many_sets.build(name)
        _spreads[name, budgets, rows] = many_spread_walk.spread_many(text, roots[:rows], budgets) + (text, roots)
    return _spreads[name, budgets, rows]


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = _lib.load_library()
    for name, args in NEW_CALLS.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    # plain arguments: no struct of the family changed, no plan family was added
    assert C.sizeof(_lib.ManyResult) == 40 and C.sizeof(_lib.ManyOptions) == 16 and C.sizeof(_lib.ManyUptoOptions) == 16
    assert C.sizeof(_lib.ManyRestartOptions) == 24 and C.sizeof(_lib.ManyStream) == 32
    assert len(L.csgpu_solve_many_checkpointed.argtypes) == 9 and len(L.csgpu_many_checkpoint_states.argtypes) == 6
    assert not any("dive" in f or "many" in f for f in _lib.PLAN_FAMILIES)
    for method in ("solve_many_spread", "checkpoint_children", "checkpoint_fanout", "fold_many"):
        assert callable(getattr(Model, method)), method


def test_argument_errors_come_in_their_order_before_any_device_call():
    from csolve_amd import _lib
    L = _lib.load_library()
    pool = C.create_string_buffer(64)  # stands for a pool of csgpu_many_checkpoints_create: all zero
    slots = np.full(4, -1, dtype=np.int32)
    children = np.full(4, 77, dtype=np.int64)
    offsets = np.zeros(5, dtype=np.int64)
    rows = np.full((4, 8, 2), 77, dtype=np.int32)
    owner = np.full(4, 77, dtype=np.int32)
    records = np.full((4, 5), 77, dtype=np.int64)

    def refused(rc, word):
        msg = L.csgpu_last_error().decode()
        assert rc == E_ARG and word in msg, (rc, msg)

    def count_children(ck=pool, sl=slots.ctypes.data, count=4, out=children.ctypes.data):
        return L.csgpu_many_checkpoint_children(ck, sl, count, out, None)

    def fan_out(ck=pool, sl=slots.ctypes.data, count=4, off=offsets.ctypes.data, to=rows.ctypes.data, own=owner.ctypes.data,
                total=4):
        return L.csgpu_many_checkpoint_fanout(ck, sl, count, off, to, own, total, None)

    def fold(sub=records.ctypes.data, own=owner.ctypes.data, total=4, into=records.ctypes.data):
        return L.csgpu_many_fold(sub, own, total, into, None)

    for missing in ("ck", "sl", "out"):
        refused(count_children(**{missing: None}), "null")
        refused(count_children(**{missing: None, "count": -1}), "null")  # the null pointer is named first
    refused(count_children(count=-1), "negative")
    for missing in ("ck", "sl", "off", "to"):
        refused(fan_out(**{missing: None}), "null")
        refused(fan_out(**{missing: None, "count": -1, "total": -1}), "null")
    refused(fan_out(count=-1), "negative")
    refused(fan_out(total=-1), "negative")
    refused(fan_out(count=-1, total=0), "negative")  # an empty fan-out is no way round the checks
    for missing in ("sub", "own", "into"):
        refused(fold(**{missing: None}), "null")
        refused(fold(**{missing: None, "total": -1}), "null")
    refused(fold(total=-1), "negative")
    # nothing to do: success, and nothing is launched or written
    assert count_children(count=0) == 0
    assert fan_out(count=0) == 0 and fan_out(total=0) == 0 and fan_out(total=0, own=None) == 0
    assert fold(total=0) == 0
    assert (children == 77).all() and (rows == 77).all() and (owner == 77).all() and (records == 77).all()


@pytest.mark.parametrize("budgets", BUDGETS, ids=lambda b: "-".join(map(str, b)))
@pytest.mark.parametrize("name", sorted(many_sets.SETS))
def test_the_spread_walk_is_the_one_all_walk_field_for_field(name, budgets):
    got, info, text, roots = _spread(name, budgets)
    stopped = 0
    for i, g in enumerate(got):
        want = _dive(name, text, roots, i)
        for f in FIELDS:
            assert g[f] == want[f], (name, budgets, i, f, g[f], want[f])
        assert (g["first"] is None) == (want["first"] is None), (name, i)
        assert g["first"] is None or (g["first"] == want["first"]).all(), (name, i)
        stopped += want["nodes"] > budgets[0]
    print(f"{name} {budgets}: {info}")
    assert info["sub_instances"] == sum(info["per_round"]) and info["rounds"] == 1 + len(info["per_round"])
    assert (info["sub_instances"] > 0) == (stopped > 0)


def test_the_fold_of_one_level_is_the_rest_of_the_walk():
    """one fan-out of a stopped walk, every child walked to its end: stopped record + fold = the whole walk"""
    text, roots, _, _ = many_sets.build("queens12_two")
    seen = 0
    for i in range(8):
        w = many_walk.Walk(text, roots[i])
        part = w.run(16)
        if part["status"] != many_walk.LIMIT:
            continue
        rows = many_spread_walk.children_of(w)
        assert len(rows) == many_spread_walk.count_children(w) and rows.dtype == np.int32
        open_states = w.open_subtrees()[::-1]  # the same frames as narrowed states, the current node first
        assert sum(int(s[v, 1] - s[v, 0]) + 1 for s, (_, v, _) in zip(open_states, reversed(w.frames()))) == len(rows)
        subs = [many_walk.Walk(text, row).run(1 << 62) for row in rows]
        total = many_spread_walk.fold(subs, [0] * len(subs), [{f: part[f] for f in many_spread_walk.COUNTERS}])[0]
        want = _dive("queens12_two", text, roots, i)
        for f in many_spread_walk.COUNTERS:
            assert total[f] == want[f], (i, f)
        seen += 1
    assert seen >= 4


def test_a_later_round_replaces_the_candidate_first_solution():
    """queens12_two, 10 rows, budgets (8, 24): some owner's lowest solution row of one round is preceded by a solution
    found in a later round; the rule with one bisection per round finds the walk's first all the same"""
    got, info, text, roots = _spread("queens12_two", (8, 24), rows=10)
    assert info["replaced_later"] >= 1, info
    for i, g in enumerate(got):
        want = _dive("queens12_two", text, roots, i)
        assert g["status"] == many_walk.DONE and g["solutions"] == want["solutions"]
        assert (g["first"] is None) == (want["first"] is None)
        assert g["first"] is None or (g["first"] == want["first"]).all(), i


def test_the_sets_hold_one_child_frames_and_depth_0_checkpoints():
    for name in ("queens12_two", "sudoku9_all"):
        _, info, _, _ = _spread(name, (1, 7, 56))
        assert info["one_child_frames"] >= 1, (name, info)  # a frame before its variable's last value: one child
        assert info["depth0"] >= 1, (name, info)            # a checkpoint that holds the current node only
