"""CPU tests of csgpu_solve_many_clauses_stream / Model.solve_many_clauses_stream (a clause model under ALL, every solution
of every instance appended to one bounded stream): the interface is declared, exported and prototyped; the argument
errors, in the documented order, with no device; the shipped cs_walk_stream instantiations beside the four older walk
families; and, on the host walk the GPU tests compare with, every figure tests/many_clause_stream_sets.py records about
its sets and the property the GPU tests lean on: however the stream's rows are handed out, a call loop ends every
instance with the record and the rows of the unbounded walk."""
import ctypes as C
import re

import numpy as np
import pytest

import many_clause_sets as sets
import many_clause_stream_sets as ssets
import many_walk_clauses_stream as S
import many_walk_clauses_upto as U
from csolve_amd import problems
from test_solve_many_stream_host import shipped_kernels

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
EIGHT = {f"cs_walk_stream<{cpl}, {tree}>" for cpl in (1, 2, 4, 8) for tree in ("true", "false")}


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import ManySolutionStream, Model
    raw = open(_lib.HEADER_PATH).read()
    L = _lib.load_library()
    assert "csgpu_solve_many_clauses_stream" in _lib.declared_symbols()
    assert hasattr(L, "csgpu_solve_many_clauses_stream") and len(L.csgpu_solve_many_clauses_stream.argtypes) == 9
    assert hasattr(L, "csgpu_internal_many_clauses_stream_symbol")
    assert len(L.csgpu_internal_many_clauses_stream_symbol.argtypes) == 3
    assert "csgpu_internal_many_clauses_stream_symbol" not in raw  # cs_internal.h only
    for method in ("solve_many_clauses_stream", "solve_many_clauses_all", "many_clauses_stream_kernel"):
        assert callable(getattr(Model, method)), method
    assert callable(ManySolutionStream.take) and callable(Model.many_stream)
    # the old entries keep their argument counts, the structs their sizes, the constants their values
    old = {"csgpu_solve_many_stream": 9, "csgpu_solve_many_clauses": 8, "csgpu_solve_many_clauses_checkpointed": 10,
           "csgpu_solve_many_clauses_resume": 9, "csgpu_solve_many_clauses_upto": 7,
           "csgpu_solve_many_clauses_upto_checkpointed": 9, "csgpu_solve_many_clauses_upto_resume": 8,
           "csgpu_solve_many_clauses_restarts": 9, "csgpu_many_clause_checkpoint_states": 8,
           "csgpu_many_clause_checkpoints_create": 3}
    for name, args in old.items():
        assert len(getattr(L, name).argtypes) == args, name
    assert C.sizeof(_lib.ManyStream) == 32 and C.sizeof(_lib.ManyResult) == 40 and C.sizeof(_lib.ManyOptions) == 16
    assert _lib.MANY_FULL == 4 and _lib.MANY_SLOT_FRESH == -2
    assert len(_lib.PLAN_FAMILIES) == 16
    assert not any("walk" in f or "many" in f or "stream" in f for f in _lib.PLAN_FAMILIES)


def test_argument_errors_come_in_the_documented_order_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyOptions, ManyStream
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(problems.schedule(5, 1))  # parsed, not finalized
    n = m.n_vars
    rows = np.zeros((2, n, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    slots = np.full(2, -2, dtype=np.int32)
    pool = C.create_string_buffer(64)  # stands for a pool: no call gets as far as looking into it
    mem = np.zeros(64, dtype=np.int64)  # stands for device memory: nothing is launched
    p = mem.ctypes.data
    ok, good = ManyOptions(1, 0, 100), ManyStream(p, p, p, 4)

    def call(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data, out=good):
        rc = L.csgpu_solve_many_clauses_stream(model, roots, count, C.byref(opt) if opt is not None else None, results, ck, sl,
                                               C.byref(out) if out is not None else None, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    # 1. null arguments, the count, the budget
    for missing in ("model", "roots", "opt", "results", "ck", "sl", "out"):
        rc, msg = call(**{missing: None})
        assert rc == E_ARG and "null" in msg, (missing, msg)
    assert call(count=-1)[0] == E_ARG and "count" in call(count=-1)[1]
    for budget in (0, -5):
        rc, msg = call(opt=ManyOptions(1, 0, budget))
        assert rc == E_ARG and "max_nodes" in msg
    assert "count" in call(count=-1, opt=ManyOptions(0, 0, 0), out=ManyStream(p, p, p, 0))[1]
    assert "max_nodes" in call(opt=ManyOptions(0, 0, 0), out=ManyStream(p, p, p, 0))[1]
    # 2. the objective: ALL alone -- MIN and MAX, which csgpu_solve_many_clauses takes, and no objective at all
    for objective in (0, 2, 3, 7, -1):
        rc, msg = call(opt=ManyOptions(objective, 0, 100), out=ManyStream(p, p, p, 0))
        assert rc == E_ARG and "ALL" in msg, (objective, msg)
    # 3. the stream
    for capacity in (0, -3):
        rc, msg = call(out=ManyStream(p, p, p, capacity))
        assert rc == E_ARG and "capacity" in msg
    for bad in (ManyStream(None, p, p, 4), ManyStream(p, None, p, 4), ManyStream(p, p, None, 4)):
        rc, msg = call(out=bad)
        assert rc == E_ARG and "null" in msg
    # 4. the model's state, after all of them; an empty batch is no way round it
    rc, msg = call()
    assert rc == E_STATE and "finalized" in msg
    assert call(count=0)[0] == E_STATE
    # nothing was touched
    assert (res == 0).all() and (slots == -2).all() and (mem == 0).all()
    # the Python methods: max_nodes is required, and a numpy batch on a model that is not finalized gets the library's error
    with pytest.raises(CsolveError) as e:
        m.many_clauses_stream_kernel()
    assert e.value.code == E_STATE


def test_the_shipped_stream_kernels_are_exactly_the_eight():
    shipped = shipped_kernels("cs_walk_stream")
    assert len(shipped) == 8
    for name in shipped:
        assert re.fullmatch(r"cs_walk_stream<[1248], (true|false)>", name), name
    assert shipped == EIGHT
    for family in ("cs_walk_clauses", "cs_walk_resume", "cs_walk_upto", "cs_walk_restart"):
        old = shipped_kernels(family)
        assert len(old) == 8, family
        assert {k.replace(family, "cs_walk_stream") for k in old} == shipped, family
    assert {ssets.kernel(name) for name in ssets.TABLE} == EIGHT  # every instantiation has a set


@pytest.mark.parametrize("name", sorted(ssets.TABLE))
def test_the_sets_plan_the_instantiations_they_name(name):
    text, roots = ssets.build(name)
    assert sets.planned(text).replace("cs_walk_clauses", "cs_walk_stream") == ssets.kernel(name)
    assert len(roots) == ssets.ROWS[name]


@pytest.mark.parametrize("name", sorted(ssets.TABLE))
def test_the_figures_of_the_table_hold_on_the_host_walk(name):
    walks = ssets.walk(name)
    _, solutions, largest = ssets.TABLE[name]
    print(f"{name}: {len(walks)} rows, {sum(w['solutions'] for w in walks)} solutions, "
          f"largest walk {max(w['nodes'] for w in walks)} nodes")
    assert all(w["status"] == U.DONE for w in walks)
    assert sum(w["solutions"] for w in walks) == solutions
    assert max(w["nodes"] for w in walks) == largest <= ssets.BUDGET
    for w in walks:
        assert len(w["rows"]) == w["solutions"] and len({r.tobytes() for r in w["rows"]}) == len(w["rows"])
    if name == "tree20_all":
        root, unique = walks[ssets.ROOT_SOLUTION[1]], walks[ssets.UNIQUE[1]]
        assert root["nodes"] == 0 and root["solutions"] == 1
        assert unique["nodes"] > 0 and unique["solutions"] == 1
        assert [i for i, w in enumerate(walks) if w["solutions"] == 1] == [9, 19]
    if name == "schedule5_classes":
        assert sum(1 for w in walks if w["solutions"] == 0) == 30
    if name == "schedule22_min_budget":  # what the GPU test of budget and stream together counts on
        text, roots = ssets.build(name)
        assert U.Walk(text, roots[0]).run(64, None)["solutions"] == 39
        assert U.Walk(text, roots[2]).run(512, None)["solutions"] == 0


def test_a_refusal_steps_back():
    """the walk of one row, refused at every second request: no counter moves at a refusal, and the walk ends as the
    unbounded one"""
    text, roots = ssets.build("tree20_all")
    want = max(ssets.walk("tree20_all"), key=lambda w: w["solutions"])
    i = ssets.walk("tree20_all").index(want)
    assert want["solutions"] >= 4
    w = S.Walk(text, roots[i])
    asked = [0]

    def room():
        asked[0] += 1
        return asked[0] % 2 == 0

    refusals = 0
    while True:
        before = dict(w.out)
        res = w.run_stream(1 << 62, room)
        if res["status"] != S.FULL:
            break
        refusals += 1
        part = U.Walk(text, roots[i]).run(res["nodes"], None) if res["nodes"] else None
        if part is not None:  # FULL at node count N is the plain walk after N nodes
            assert all(part[f] == res[f] for f in ("nodes", "cuts", "props", "solutions"))
        assert res["nodes"] >= before["nodes"] and res["solutions"] <= before["solutions"] + 1
    assert refusals == want["solutions"]
    for f in S.FIELDS:
        assert res[f] == want[f], f
    assert all((a == b).all() for a, b in zip(res["rows"], want["rows"])) and len(res["rows"]) == len(want["rows"])


@pytest.mark.parametrize("capacity", [1, 7])
def test_the_call_loop_ends_every_instance_as_the_unbounded_walk(capacity):
    """the host model of the call over tree20_all, the instances served round-robin (another one first in every call):
    every instance ends with the record and the rows of the unbounded walk, each row once and in walk order"""
    text, roots = ssets.build("tree20_all")
    want = ssets.walk("tree20_all")
    K = len(roots)
    call = S.Call(text, roots, capacity)
    per = [[] for _ in range(K)]
    calls, seen_full, seen_fresh = 0, False, False
    while call.left():
        assert calls < sum(w["solutions"] for w in want) + K + 2, "the loop does not end"
        order = [(calls * 5 + j) % K for j in range(K)]
        call.call(order, 1 << 62)
        calls += 1
        seen_full |= any(r["status"] == S.FULL and s >= 0 for r, s in zip(call.records, call.slots))
        seen_fresh |= any(r["status"] == S.FULL and s == S.FRESH and r["nodes"] == 0 for r, s in zip(call.records, call.slots))
        taken = call.drain()
        assert len(taken) <= capacity
        for o, r in taken:
            per[o].append(r)
    assert seen_full and seen_fresh and calls > 1
    for i, w in enumerate(want):
        for f in S.FIELDS:
            assert call.records[i][f] == w[f], (i, f)
        assert len(per[i]) == len(w["rows"]) and all((a == b).all() for a, b in zip(per[i], w["rows"])), i


def test_budget_and_stream_together_on_the_host():
    """a budget of 8 nodes and 2 rows per call: LIMIT and FULL both occur, and the end is the same"""
    text, roots = ssets.build("tree20_all")
    want = ssets.walk("tree20_all")
    K = len(roots)
    call = S.Call(text, roots, 2)
    per = [[] for _ in range(K)]
    statuses = set()
    for calls in range(10000):
        if not call.left():
            break
        call.call(list(range(K)), 8)
        statuses |= {r["status"] for r, s in zip(call.records, call.slots) if s >= 0}
        for o, r in call.drain():
            per[o].append(r)
    assert not call.left() and statuses == {S.LIMIT, S.FULL}
    for i, w in enumerate(want):
        assert all(call.records[i][f] == w[f] for f in S.FIELDS), i
        assert len(per[i]) == len(w["rows"]) and all((a == b).all() for a, b in zip(per[i], w["rows"])), i
