"""CPU tests of the spread of stopped ALL walks of clause models (csgpu_many_clause_checkpoint_children / _fanout,
Model.solve_many_clauses_spread): the interface is declared, exported and prototyped; the argument errors in their
documented order, without a device; and the identity the spread rests on, on the host model of
tests/many_clause_spread_walk.py against the one ALL walk of tests/many_walk_objective.py: the children of a stopped clause
walk, walked as root rows of their own and folded back over any number of levels, give the one walk's status, nodes, cuts,
solutions and first solution.  props are the oracle's here, which counts a root row and a child differently: they are
compared on the device only."""
import ctypes as C
import re

import pytest

import many_clause_sets
import many_clause_spread_walk as S
import many_walk_objective as W

E_ARG, E_LIMIT = -1, -4
NEW_CALLS = {"csgpu_many_clause_checkpoint_children": 5, "csgpu_many_clause_checkpoint_fanout": 8}
SETS = ("tree20_all", "mixed40_any", "wcet_max", "linear20_all", "linear40_all")  # all walked under ALL
BUDGETS = ((8, 32), (2, 1, 1, 1, 64))
_spreads, _walks = {}, {}


def _one_walk(name):
    """the one ALL walk of every row of a set, walked once"""
    if name not in _walks:
        text, roots, _, _ = many_clause_sets.build(name)
        _walks[name] = [W.walk(text, row, "ALL") for row in roots]
    return _walks[name]


def _spread(name, budgets):
    if (name, budgets) not in _spreads:
        text, roots, _, _ = many_clause_sets.build(name)
        _spreads[name, budgets] = S.spread_many(text, roots, budgets)
    return _spreads[name, budgets]


class _Pool(C.Structure):
    """csgpu_many_checkpoints as cs_capi.hip lays it out, for a pool that no device call made: only `kind` is looked at
    before the count limit (0: of csgpu_many_checkpoints_create, 1: of csgpu_many_clause_checkpoints_create)"""
    _fields_ = [("m", C.c_void_p), ("capacity", C.c_int64), ("slot_bytes", C.c_size_t), ("d_pool", C.c_void_p),
                ("d_next", C.c_void_p), ("counted", C.c_int), ("kind", C.c_int), ("d_zero", C.c_void_p)]


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = _lib.load_library()
    for name, args in NEW_CALLS.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    # the kernel-7 pair and the shared fold are what they were
    assert len(L.csgpu_many_checkpoint_children.argtypes) == 5 and len(L.csgpu_many_checkpoint_fanout.argtypes) == 8
    assert len(L.csgpu_many_fold.argtypes) == 5
    assert C.sizeof(_lib.ManyResult) == 40 and C.sizeof(_lib.ManyOptions) == 16
    for method in ("solve_many_clauses_spread", "clause_checkpoint_children", "clause_checkpoint_fanout"):
        assert callable(getattr(Model, method)), method


def test_argument_errors_come_in_their_order_before_any_device_call():
    import numpy as np
    from csolve_amd import _lib
    L = _lib.load_library()
    dive_pool, clause_pool = _Pool(kind=0), _Pool(kind=1)
    slots = np.full(4, -1, dtype=np.int32)
    children = np.full(4, 77, dtype=np.int64)
    offsets = np.zeros(5, dtype=np.int64)
    rows = np.full((4, 8, 2), 77, dtype=np.int32)
    owner = np.full(4, 77, dtype=np.int32)
    too_many = 1 << 31

    def refused(rc, word, code=E_ARG):
        msg = L.csgpu_last_error().decode()
        assert rc == code and word in msg, (rc, msg)

    def count_children(ck=dive_pool, sl=slots.ctypes.data, count=4, out=children.ctypes.data):
        return L.csgpu_many_clause_checkpoint_children(C.byref(ck) if ck is not None else None, sl, count, out, None)

    def fan_out(ck=dive_pool, sl=slots.ctypes.data, count=4, off=offsets.ctypes.data, to=rows.ctypes.data,
                own=owner.ctypes.data, total=4):
        return L.csgpu_many_clause_checkpoint_fanout(C.byref(ck) if ck is not None else None, sl, count, off, to, own,
                                                     total, None)

    # null, then a negative count, then a negative total, then the pool's kind, then the count limit
    for missing in ("ck", "sl", "out"):
        refused(count_children(**{missing: None}), "null")
        refused(count_children(**{missing: None, "count": -1}), "null")
    refused(count_children(count=-1), "negative")
    refused(count_children(), "other kind")
    refused(count_children(count=too_many), "other kind")  # the pool's kind comes before the limit
    refused(count_children(ck=clause_pool, count=too_many), "2^31", E_LIMIT)
    for missing in ("ck", "sl", "off", "to"):
        refused(fan_out(**{missing: None}), "null")
        refused(fan_out(**{missing: None, "count": -1, "total": -1}), "null")
    refused(fan_out(count=-1), "negative instance")
    refused(fan_out(count=-1, total=-1), "negative instance")
    refused(fan_out(total=-1), "negative row")
    refused(fan_out(count=-1, total=0), "negative")  # an empty fan-out is no way round the checks
    refused(fan_out(total=-1, count=too_many), "negative row")
    refused(fan_out(), "other kind")
    refused(fan_out(count=0), "other kind")
    refused(fan_out(count=too_many), "other kind")
    refused(fan_out(ck=clause_pool, count=too_many), "2^31", E_LIMIT)
    refused(fan_out(ck=clause_pool, count=too_many, total=0), "2^31", E_LIMIT)
    # nothing to do: success, and nothing is launched or written
    assert count_children(ck=clause_pool, count=0) == 0
    assert fan_out(ck=clause_pool, count=0) == 0 and fan_out(ck=clause_pool, total=0) == 0
    assert fan_out(ck=clause_pool, total=0, own=None) == 0
    assert (children == 77).all() and (rows == 77).all() and (owner == 77).all()


@pytest.mark.parametrize("budgets", BUDGETS, ids=lambda b: "-".join(map(str, b)))
@pytest.mark.parametrize("name", SETS)
def test_the_spread_walk_is_the_one_all_walk(name, budgets):
    got, info = _spread(name, budgets)
    want = _one_walk(name)
    stopped = 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert w["status"] == W.DONE
        for f in S.FIELDS:
            assert g[f] == w[f], (name, budgets, i, f, g[f], w[f])
        assert (g["first"] is None) == (w["first"] is None), (name, i)
        assert g["first"] is None or (g["first"] == w["first"]).all(), (name, i)
        stopped += w["nodes"] > budgets[0]
    print(f"{name} {budgets}: {info}")
    assert info["sub_instances"] == sum(info["per_round"]) and info["rounds"] == 1 + len(info["per_round"])
    assert stopped > 0 and info["sub_instances"] > 0, "the budget must stop instances"


@pytest.mark.parametrize("name", ("wcet_max", "linear20_all"))
def test_a_later_round_replaces_the_candidate_first_solution(name):
    """budgets (2, 1, 1, 1, 64): an owner's lowest solution row of one round is preceded by a solution found in a later
    round; the rule with one bisection per round finds the walk's first all the same"""
    got, info = _spread(name, (2, 1, 1, 1, 64))
    assert info["replaced_later"] >= 1, info
    for i, (g, w) in enumerate(zip(got, _one_walk(name))):
        assert g["status"] == W.DONE and g["solutions"] == w["solutions"]
        assert (g["first"] is None) == (w["first"] is None)
        assert g["first"] is None or (g["first"] == w["first"]).all(), (name, i)


def test_the_sets_hold_the_cases_the_fold_and_the_fan_out_must_get_right():
    infos = [_spread(name, (8, 32))[1] for name in SETS]
    print(infos)
    assert sum(i["dead_rows"] for i in infos) >= 1      # sub-rows inconsistent as roots: the +1 cut
    assert sum(i["solution_rows"] for i in infos) >= 1  # sub-rows that are themselves the one solution
    assert sum(i["depth0"] for i in infos) >= 1         # checkpoints that hold the current node only
    assert sum(i["one_child_frames"] for i in infos) >= 1  # frames with one child left
