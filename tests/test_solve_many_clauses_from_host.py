"""CPU tests of the start incumbents of csgpu_solve_many_clauses_from and of the MIN / MAX spread built on them
(csgpu_many_clause_checkpoint_children_obj / _fanout_obj, csgpu_many_fold_best, Model.solve_many_clauses_spread(roots,
"MIN" / "MAX")): the host model of tests/many_clause_from_walk.py against the one MIN / MAX walk of
tests/many_walk_objective.py -- the optimum and DONE are the one call's, `first` is a solution of that value, and the sets
hold every case the fold and the fan-out must get right --, and the product before any HIP call: the interface, every
error of the new entries that needs no finalized model, in the documented order, and the key of the best-value fold."""
import ctypes as C
import re

import numpy as np
import pytest

import many_clause_from_walk as F
import many_clause_sets
import many_walk_objective as W

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
NEW_CALLS = {"csgpu_solve_many_clauses_from": 11, "csgpu_solve_many_clauses_from_resume": 9,
             "csgpu_many_clause_checkpoint_children_obj": 6, "csgpu_many_clause_checkpoint_fanout_obj": 11,
             "csgpu_many_fold_best": 7, "csgpu_many_best_key": 3, "csgpu_many_key_decode": 4}
SPREADS = (("schedule5_min", (8, 32)), ("wcet_max", (8, 32)), ("schedule6_min_budget", (16, 64)))
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
_spreads, _walks = {}, {}


def one_walk(name):
    """the one MIN / MAX walk of every row of a set to the end of its tree, walked once"""
    if name not in _walks:
        text, roots, objective, _ = many_clause_sets.build(name)
        _walks[name] = [W.walk(text, row, objective, 1 << 22) for row in roots]
    return _walks[name]


def spread(name, budgets, max_rounds=1 << 30):
    if (name, budgets, max_rounds) not in _spreads:
        text, roots, objective, _ = many_clause_sets.build(name)
        _spreads[name, budgets, max_rounds] = F.spread_minmax(text, roots, objective, budgets, max_rounds)
    return _spreads[name, budgets, max_rounds]


def satisfies(text, row):
    """is the fully valued `row` consistent at the model's root node?"""
    orc, _ = W.oracle_for(text)
    status, out = orc.instance(np.stack([row, row], 1).astype(np.int32), -1, 0, 0)
    return status >= 0 and (out[:, 0] == row).all() and (out[:, 1] == row).all()


# ---- the host model ----

@pytest.mark.parametrize("name,budgets", SPREADS, ids=[s[0] for s in SPREADS])
def test_the_spread_proves_the_one_calls_optimum(name, budgets):
    text, roots, objective, _ = many_clause_sets.build(name)
    ov = W.model_of(text).view.obj_var
    got, info = spread(name, budgets)
    print(f"{name} {budgets}: {info}; nodes {sum(g['nodes'] for g in got)} against {sum(w['nodes'] for w in one_walk(name))}")
    for i, (g, w) in enumerate(zip(got, one_walk(name))):
        assert w["status"] == W.DONE
        assert g["status"] == W.DONE and g["best"] == w["best"], (name, i, g["best"], w["best"])
        assert (g["first"] is None) == (w["best"] is None)
        if g["first"] is not None:
            assert g["first"][ov] == g["best"] and satisfies(text, g["first"]), (name, i)
        assert g["nodes"] >= w["nodes"] and g["solutions"] >= (w["best"] is not None)
    assert info["sub_instances"] == sum(info["per_round"]) > 0 and info["rounds"] == 1 + len(info["per_round"])


def test_the_sets_hold_the_cases_the_fold_and_the_fan_out_must_get_right():
    infos = [spread(name, budgets)[1] for name, budgets in SPREADS]
    for counter in ("ties", "dead", "nosol_done", "improved_later", "tightened"):
        assert max(i[counter] for i in infos) > 0, counter


def test_the_spread_is_the_walk_that_was_measured():
    """the rounds and the rows of every round the issue's prototype made"""
    assert spread("schedule5_min", (8, 32))[1]["per_round"] == [999, 729, 4]
    assert spread("wcet_max", (8, 32))[1]["per_round"] == [114, 106, 33]
    assert spread("schedule6_min_budget", (16, 64))[1]["per_round"] == [716, 918, 168, 36]


def test_max_rounds_leaves_owners_stopped_and_one_without_a_solution():
    got, info = spread("schedule22_min_budget", (16, 32), 2)
    assert info["rounds"] == 2
    assert [g["status"] for g in got] == [0, 0, 1, 0, 0, 1, 1, 1]
    none = [g for g in got if g["best"] is None]
    assert len(none) == 1 and none[0]["status"] == W.LIMIT and none[0]["solutions"] == 0 and none[0]["first"] is None
    assert all(g["solutions"] > 0 for g in got if g["best"] is not None)


@pytest.mark.parametrize("name", ["schedule5_min", "wcet_max"])
def test_a_start_at_the_optimum_proves_it_and_one_beside_it_finds_it(name):
    text, roots, objective, _ = many_clause_sets.build(name)
    worse = 1 if objective == "MIN" else -1
    for row, w in zip(roots, one_walk(name)):
        at = F.walk_from(text, row, objective, w["best"])
        assert at["status"] == W.DONE and at["solutions"] == 0 and at["best"] is None and at["first"] is None
        assert at["nodes"] <= w["nodes"]
        near = F.walk_from(text, row, objective, w["best"] + worse)
        assert near["status"] == W.DONE and near["best"] == w["best"] and near["solutions"] >= 1
        past = F.walk_from(text, row, objective, w["best"] - worse)
        assert past["status"] == W.DONE and past["solutions"] == 0


def test_no_start_is_the_walk_itself_and_an_emptying_start_is_a_dead_root():
    text, roots, objective, _ = many_clause_sets.build("schedule5_min")
    ov = W.model_of(text).view.obj_var
    for row in roots[:8]:
        for budget in (7, 1 << 22):
            want, got = W.walk(text, row, objective, budget), F.walk_from(text, row, objective, None, budget)
            assert {k: v for k, v in got.items() if k != "first"} == {k: v for k, v in want.items() if k != "first"}
            assert (got["first"] is None) == (want["first"] is None)
            assert got["first"] is None or (got["first"] == want["first"]).all()
        dead = F.walk_from(text, row, objective, int(row[ov, 0]))  # hi < lo
        assert dead == dict(status=W.DONE, root_props=0, nodes=0, cuts=0, props=0, solutions=0, best=None, first=None)


# ---- the product, before any HIP call ----

class _Pool(C.Structure):
    """csgpu_many_checkpoints as cs_capi.hip lays it out, for a pool that no device call made: only `kind` is looked at
    before the count limit (0: of csgpu_many_checkpoints_create, 1: of csgpu_many_clause_checkpoints_create)"""
    _fields_ = [("m", C.c_void_p), ("capacity", C.c_int64), ("slot_bytes", C.c_size_t), ("d_pool", C.c_void_p),
                ("d_next", C.c_void_p), ("counted", C.c_int), ("kind", C.c_int), ("d_zero", C.c_void_p)]


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    import inspect
    raw = open(_lib.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = _lib.load_library()
    for name, args in NEW_CALLS.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
        assert re.search(r"\b(int|uint64_t)\s+%s\s*\(" % name, text), name
    assert re.search(r"typedef struct csgpu_many_start \{\s*int32_t best;[^}]*int32_t have;\s*\} csgpu_many_start;", raw)
    assert hasattr(L, "csgpu_internal_many_clauses_from_symbol") and "csgpu_internal_many_clauses_from_symbol" not in raw
    # the calls the new ones stand beside are what they were
    assert len(L.csgpu_many_clause_checkpoint_children.argtypes) == 5 and len(L.csgpu_many_clause_checkpoint_fanout.argtypes) == 8
    assert len(L.csgpu_solve_many_clauses.argtypes) == 8 and len(L.csgpu_solve_many_clauses_resume.argtypes) == 9
    assert len(L.csgpu_many_fold.argtypes) == 5
    assert callable(Model.fold_many_best)
    assert inspect.signature(Model.solve_many_clauses).parameters["start"].default is None
    assert inspect.signature(Model.resume_many_clauses).parameters["own_solutions"].default is False
    assert inspect.signature(Model.solve_many_clauses_spread).parameters["objective"].default == "ALL"
    for method in (Model.clause_checkpoint_children, Model.clause_checkpoint_fanout):
        assert inspect.signature(method).parameters["objective"].default is None
    assert "owner_start" in inspect.signature(Model.clause_checkpoint_fanout).parameters


def test_the_start_entries_keep_the_order_of_the_errors_of_solve_many_clauses():
    """everything up to "the model is not finalized" (a finalized model needs a device: what follows it -- a null d_start,
    ANY / ALL, one of the pool and the slots -- is in test_gpu_solve_many_clauses_from.py)"""
    from csolve_amd import _lib, problems
    from csolve_amd._lib import ManyOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(problems.schedule(5, 1))  # MIN; parsed, not finalized
    plain = Model.from_text(problems.linear(12, 1, "ALL"))  # no objective variable
    rows = np.zeros((2, m.n_vars, 2), dtype=np.int32)
    start = np.zeros((2, 2), dtype=np.int32)
    res = np.full((2, 5), 77, dtype=np.int64)
    pool, slots = _Pool(kind=1), np.full(2, 77, dtype=np.int32)
    ok = ManyOptions(2, 0, 100)

    def fresh(model=m._h, roots=rows.ctypes.data, st=start.ctypes.data, count=2, opt=ok, results=res.ctypes.data, ck=None, sl=None):
        return L.csgpu_solve_many_clauses_from(model, roots, st, count, C.byref(opt) if opt is not None else None, results,
                                               None, None, C.byref(ck) if ck is not None else None, sl, None)

    def resume(model=m._h, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data, roots=None, st=None):
        return L.csgpu_solve_many_clauses_from_resume(model, count, C.byref(opt) if opt is not None else None, results, None,
                                                      None, C.byref(ck) if ck is not None else None, sl, None)

    def refused(rc, code, *words):
        msg = L.csgpu_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    for call in (fresh, resume):
        refused(call(model=None), E_ARG, "null")
        refused(call(results=None), E_ARG, "null")
        refused(call(opt=None), E_ARG, "null")
        refused(call(count=-1), E_ARG, "negative")
        refused(call(opt=ManyOptions(2, 0, 0)), E_ARG, "max_nodes")
        refused(call(opt=ManyOptions(2, 0, 0), count=-1), E_ARG, "negative")
        refused(call(opt=ManyOptions(7, 0, 100)), E_ARG, "no objective")
        refused(call(opt=ManyOptions(3, 0, 100)), E_ARG, "MIN", "MAX")  # MAX on a MIN model
        refused(call(model=plain._h), E_ARG, "objective")
        refused(call(), E_STATE, "finalized")
        refused(call(count=0), E_STATE, "finalized")  # an empty batch is no way round the state check
        # what the entries add comes after the state: none of it is looked at on a model that is not finalized
        refused(call(st=None), E_STATE, "finalized")
        refused(call(opt=ManyOptions(1, 0, 100)), E_STATE, "finalized")
        refused(call(ck=pool, sl=None), E_STATE, "finalized")
    refused(fresh(roots=None), E_ARG, "null")
    assert (res == 77).all() and (slots == 77).all()


def test_the_objective_fan_out_refuses_in_its_order_before_any_device_call():
    from csolve_amd import _lib
    L = _lib.load_library()
    dive_pool, clause_pool = _Pool(kind=0), _Pool(kind=1)
    slots = np.full(4, -1, dtype=np.int32)
    children = np.full(4, 77, dtype=np.int64)
    offsets = np.zeros(5, dtype=np.int64)
    rows = np.full((4, 8, 2), 77, dtype=np.int32)
    owner = np.full(4, 77, dtype=np.int32)
    start = np.full((4, 2), 77, dtype=np.int32)
    owner_start = np.zeros((4, 2), dtype=np.int32)
    too_many = 1 << 31

    def refused(rc, word, code=E_ARG):
        msg = L.csgpu_last_error().decode()
        assert rc == code and word in msg, (rc, msg)

    def count_children(ck=dive_pool, sl=slots.ctypes.data, count=4, objective=2, out=children.ctypes.data):
        return L.csgpu_many_clause_checkpoint_children_obj(C.byref(ck) if ck is not None else None, sl, count, objective, out, None)

    def fan_out(ck=dive_pool, sl=slots.ctypes.data, count=4, objective=2, ost=owner_start.ctypes.data, off=offsets.ctypes.data,
                to=rows.ctypes.data, own=owner.ctypes.data, st=start.ctypes.data, total=4):
        return L.csgpu_many_clause_checkpoint_fanout_obj(C.byref(ck) if ck is not None else None, sl, count, objective, ost, off,
                                                         to, own, st, total, None)

    # the objective, then what the ALL calls refuse, in their order
    for objective in (0, 1, 4, 5, -1):
        refused(count_children(objective=objective), "objective")
        refused(count_children(objective=objective, ck=None, count=-1), "objective")
        refused(fan_out(objective=objective), "objective")
        refused(fan_out(objective=objective, ck=None, count=-1, total=-1), "objective")
    for objective in (2, 3):
        for missing in ("ck", "sl", "out"):
            refused(count_children(objective=objective, **{missing: None}), "null")
            refused(count_children(objective=objective, **{missing: None, "count": -1}), "null")
        refused(count_children(objective=objective, count=-1), "negative")
        refused(count_children(objective=objective), "other kind")
        refused(count_children(objective=objective, count=too_many), "other kind")
        refused(count_children(objective=objective, ck=clause_pool, count=too_many), "2^31", E_LIMIT)
        for missing in ("ck", "sl", "off", "to", "st"):
            refused(fan_out(objective=objective, **{missing: None}), "null")
            refused(fan_out(objective=objective, **{missing: None, "count": -1, "total": -1}), "null")
        refused(fan_out(objective=objective, count=-1), "negative instance")
        refused(fan_out(objective=objective, count=-1, total=-1), "negative instance")
        refused(fan_out(objective=objective, total=-1), "negative row")
        refused(fan_out(objective=objective, total=-1, count=too_many), "negative row")
        refused(fan_out(objective=objective), "other kind")
        refused(fan_out(objective=objective, count=0), "other kind")
        refused(fan_out(objective=objective, ck=clause_pool, count=too_many), "2^31", E_LIMIT)
        refused(fan_out(objective=objective, ck=clause_pool, count=too_many, total=0), "2^31", E_LIMIT)
        # nothing to do: success, and nothing is launched or written; the owners and their starts may be missing
        assert count_children(objective=objective, ck=clause_pool, count=0) == 0
        assert fan_out(objective=objective, ck=clause_pool, count=0) == 0 and fan_out(objective=objective, ck=clause_pool, total=0) == 0
        assert fan_out(objective=objective, ck=clause_pool, total=0, own=None, ost=None) == 0
    assert (children == 77).all() and (rows == 77).all() and (owner == 77).all() and (start == 77).all()


def test_the_best_fold_refuses_in_its_order_before_any_device_call():
    from csolve_amd import _lib
    L = _lib.load_library()
    sub = np.zeros((4, 5), dtype=np.int64)
    best = np.zeros(4, dtype=np.int32)
    owner = np.zeros(4, dtype=np.int32)
    key = np.full(2, 77, dtype=np.uint64)

    def fold(records=sub.ctypes.data, values=best.ctypes.data, own=owner.ctypes.data, total=4, objective=2, to=key.ctypes.data):
        return L.csgpu_many_fold_best(records, values, own, total, objective, to, None)

    def refused(rc, word, code=E_ARG):
        msg = L.csgpu_last_error().decode()
        assert rc == code and word in msg, (rc, msg)

    for missing in ("records", "values", "own", "to"):
        refused(fold(**{missing: None}), "null")
        refused(fold(**{missing: None, "total": -1, "objective": 0}), "null")
    refused(fold(total=-1), "negative")
    refused(fold(total=-1, objective=1), "negative")
    for objective in (0, 1, 4, -1):
        refused(fold(objective=objective), "objective")
        refused(fold(objective=objective, total=1 << 32), "objective")
    refused(fold(total=1 << 32), "2^32", E_LIMIT)
    refused(fold(total=1 << 40, objective=3), "2^32", E_LIMIT)
    assert fold(total=0) == 0 and fold(total=0, objective=3) == 0
    assert (key == 77).all()


def test_the_key_orders_values_and_then_rows():
    from csolve_amd import _lib
    L = _lib.load_library()
    values = [INT32_MIN, INT32_MIN + 1, -70000, -2, -1, 0, 1, 2, 45, 70000, INT32_MAX - 1, INT32_MAX]
    none = (1 << 64) - 1

    def decode(objective, key):
        best, row = C.c_int32(-7), C.c_uint32(7)
        found = L.csgpu_many_key_decode(objective, key, C.byref(best), C.byref(row))
        return found, best.value, row.value

    for objective, order in ((2, values), (3, values[::-1])):  # MIN: ascending values come first; MAX: descending
        keys = [L.csgpu_many_best_key(objective, v, 5) for v in order]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        assert all(k < none for k in keys)
        for v in values:
            for row in (0, 1, 77, (1 << 32) - 2):
                key = L.csgpu_many_best_key(objective, v, row)
                assert key & 0xFFFFFFFF == row and decode(objective, key) == (1, v, row)
            # among the rows that hold a value the lowest wins, and a better value beats every row
            assert L.csgpu_many_best_key(objective, v, 3) < L.csgpu_many_best_key(objective, v, 4)
        better, worse = order[3], order[4]
        assert L.csgpu_many_best_key(objective, better, (1 << 32) - 2) < L.csgpu_many_best_key(objective, worse, 0)
        assert decode(objective, none) == (0, -7, 7)  # all ones: nothing found, nothing written
        assert L.csgpu_many_key_decode(objective, L.csgpu_many_best_key(objective, 45, 9), None, None) == 1
    assert L.csgpu_many_best_key(2, INT32_MIN, 0) == 0 and L.csgpu_many_best_key(3, INT32_MAX, 0) == 0
    assert L.csgpu_many_best_key(2, 0, 1) == (1 << 63) | 1
