"""CPU tests of csgpu_solve_many_clauses_upto / Model.solve_many_clauses_upto (an instance of a clause model stops at its
k-th solution and keeps all k): the interface is declared, exported and prototyped; the argument errors that need no
device, in their documented order; the shipped cs_walk_upto instantiations; and, on the host walk the GPU tests compare
with (tests/many_walk_clauses_upto.py), every figure that tests/many_clause_upto_sets.py records about its sets -- so that
no GPU test passes vacuously."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import many_clause_sets as sets
import many_clause_upto_sets as usets
import many_walk
import many_walk_clauses_upto as U
import many_walk_objective as W
from csolve_amd import problems

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
NEW_CALLS = {"csgpu_solve_many_clauses_upto": 7, "csgpu_solve_many_clauses_upto_checkpointed": 9,
             "csgpu_solve_many_clauses_upto_resume": 8}
INTERNAL = {"csgpu_internal_many_clauses_upto_symbol": 3}
EIGHT = {f"cs_walk_upto<{cpl}, {tree}>" for cpl in (1, 2, 4, 8) for tree in ("true", "false")}
ALL_FIELDS = many_walk.FIELDS


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    L = _lib.load_library()
    for name, args in NEW_CALLS.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
    for name, args in INTERNAL.items():  # exported and prototyped, declared in cs_internal.h only
        assert name not in _lib.declared_symbols() and len(getattr(L, name).argtypes) == args, name
    # the calls of both families that were there are what they were
    assert len(L.csgpu_solve_many_clauses.argtypes) == 8 and len(L.csgpu_solve_many_clauses_checkpointed.argtypes) == 10
    assert len(L.csgpu_solve_many_clauses_resume.argtypes) == 9 and len(L.csgpu_solve_many_upto.argtypes) == 7
    assert C.sizeof(_lib.ManyUptoOptions) == 16 and C.sizeof(_lib.ManyResult) == 40
    for method in ("solve_many_clauses_upto", "classify_many_clauses", "many_clauses_upto_kernel", "resume_many_clauses",
                   "solve_many_clauses_sliced"):
        assert callable(getattr(Model, method)), method
    assert not any("walk" in f or "many" in f or "upto" in f for f in _lib.PLAN_FAMILIES) and len(_lib.PLAN_FAMILIES) == 16
    header = open(_lib.HEADER_PATH).read()
    assert "Not here: restarts for clause models" in header and "left at the k-th solution" in header


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyUptoOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(problems.schedule(5, 1))  # parsed, not finalized
    n = m.n_vars
    rows = np.zeros((2, n, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    slots = np.full(2, -1, dtype=np.int32)
    pool = C.create_string_buffer(64)  # stands for a pool: no call gets as far as looking into it
    ok = ManyUptoOptions(2, 0, 100)

    def plain(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data):
        rc = L.csgpu_solve_many_clauses_upto(model, roots, count, C.byref(opt) if opt is not None else None, results, None, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    def fresh(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data):
        rc = L.csgpu_solve_many_clauses_upto_checkpointed(model, roots, count, C.byref(opt) if opt is not None else None,
                                                          results, None, ck, sl, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    def resume(model=m._h, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data):
        rc = L.csgpu_solve_many_clauses_upto_resume(model, count, C.byref(opt) if opt is not None else None, results, None,
                                                    ck, sl, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    assert plain(roots=None)[0] == E_ARG and fresh(roots=None)[0] == E_ARG
    for call in (plain, fresh, resume):
        assert call(model=None)[0] == E_ARG
        assert call(results=None)[0] == E_ARG
        assert call(opt=None)[0] == E_ARG
        assert call(count=-1)[0] == E_ARG
        assert call(opt=ManyUptoOptions(2, 0, 0))[0] == E_ARG
        assert call(opt=ManyUptoOptions(2, 0, -5))[0] == E_ARG
        for k in (0, -3):
            rc, msg = call(opt=ManyUptoOptions(k, 0, 100))
            assert rc == E_ARG and "max_solutions" in msg
        # the order: the count before the budget, the budget before k, all of them before the model's state
        assert "count" in call(count=-1, opt=ManyUptoOptions(0, 0, 0))[1]
        assert "max_nodes" in call(opt=ManyUptoOptions(0, 0, 0))[1]
        rc, msg = call()
        assert rc == E_STATE and "finalized" in msg
        assert call(count=0)[0] == E_STATE  # an empty batch is no way round the state check
    for call in (fresh, resume):  # the state comes before the pool is looked at, a null one included
        for ck, sl in ((None, slots.ctypes.data), (pool, None)):
            assert call(ck=ck, sl=sl)[0] == E_STATE
            assert call(ck=ck, sl=sl, opt=ManyUptoOptions(0, 0, 100))[0] == E_ARG
    assert (res == 0).all() and (slots == -1).all()
    # the Python methods: max_nodes is required, and a numpy batch on a model that is not finalized gets the library's
    # error (nothing is uploaded for it)
    with pytest.raises(TypeError):
        m.solve_many_clauses_upto(rows, 2)
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses_upto(rows, 2, max_nodes=10)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses_upto(rows, 0, max_nodes=10)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError) as e:
        m.classify_many_clauses(rows, max_nodes=10)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.many_clauses_upto_kernel()
    assert e.value.code == E_STATE
    with pytest.raises(ValueError, match="k-th solution"):
        m.solve_many_clauses_sliced(rows, "ALL", budgets=(4,), finish="search", max_solutions=2)
    with pytest.raises(AssertionError, match="max_solutions"):
        m.resume_many_clauses({"_checkpoints": None, "_objective": 1}, max_nodes=4, max_solutions=2)


@pytest.mark.parametrize("name", ["linear20_all", "mixed120_any"])
def test_the_slot_size_is_what_it_was(name):
    """no device: (n + 1)^2 x 8 once csgpu_model_build_tables has run, 0 before and for NULL"""
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    text = sets.build(name)[0]
    m = Model.from_text(text)
    n = m.n_vars
    assert m.clause_checkpoint_bytes() == 0
    m.set_domains(W.oracle_for(text)[1])
    m.normalize()
    m.build_tables()
    assert m.clause_checkpoint_bytes() == (n + 1) * (n + 1) * 8
    assert _lib.load_library().csgpu_many_clause_checkpoint_bytes(None) == 0


def shipped_walk_upto_kernels():
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == "cs_walk_upto" and "<" in name:
                shipped.add(name)
    return shipped


def test_the_shipped_upto_kernels_are_exactly_the_eight():
    from test_many_clauses_resume_host import shipped_walk_resume_kernels
    from test_solve_many_clauses_host import shipped_walk_kernels
    shipped = shipped_walk_upto_kernels()
    for name in shipped:
        assert re.fullmatch(r"cs_walk_upto<[1248], (true|false)>", name), name
    assert shipped == EIGHT == {usets.SETS[s][3] for s in usets.EIGHT}
    assert {s[3] for s in usets.SETS.values()} == EIGHT
    assert len(shipped_walk_kernels()) == 8 and len(shipped_walk_resume_kernels()) == 8  # the old families are what they were


@pytest.mark.parametrize("name", sorted(usets.SETS))
def test_the_sets_plan_the_instantiations_they_name(name):
    text, roots = usets.build(name)
    assert sets.planned(text).replace("cs_walk_clauses", "cs_walk_upto") == usets.SETS[name][3]
    if name in usets.EIGHT:
        assert roots is sets.build(name)[1] and usets.SETS[name][1:3] == ((2, 5), 4096)


def _same(a, b, where):
    for f in ALL_FIELDS:
        assert a[f] == b[f], (where, f)
    assert len(a["rows"]) == len(b["rows"]) and all((x == y).all() for x, y in zip(a["rows"], b["rows"])), where


@pytest.mark.parametrize("name", ["tree20_all", "wcet_max"])
def test_the_helper_is_the_specified_walk_with_another_stop(name):
    """every row: k = 1 is the ANY walk, k = 4,096 the ALL walk (no instance holds that many), slices are the one call"""
    text, roots = usets.build(name)
    for i, row in enumerate(roots):
        first = W.walk(text, row, "ANY")
        every = W.walk(text, row, "ALL")
        one = U.walk_upto(text, row, 1)
        whole = U.walk_upto(text, row, 4096)
        assert every["solutions"] < 4096
        for f in ALL_FIELDS:
            assert one[f] == first[f], (name, i, f)
            assert whole[f] == every[f], (name, i, f)
        assert len(one["rows"]) == first["solutions"] and len(whole["rows"]) == every["solutions"]
        if first["first"] is not None:
            assert (one["rows"][0] == first["first"]).all() and (whole["rows"][0] == every["first"]).all()
        assert len({r.tobytes() for r in whole["rows"]}) == len(whole["rows"])
        for r in whole["rows"]:
            assert ((r >= row[:, 0]) & (r <= row[:, 1])).all(), (name, i)
        for k in (2, 5):  # in walk order: a smaller k keeps the head of what a larger k keeps
            part = U.walk_upto(text, row, k)
            assert part["status"] == U.DONE and part["solutions"] == min(k, every["solutions"]) == len(part["rows"])
            assert all((a == b).all() for a, b in zip(part["rows"], whole["rows"]))
            if every["solutions"] < k:  # the tree is exhausted below k: ALL, field for field
                assert all(part[f] == every[f] for f in ALL_FIELDS)
        _same(U.walk_sliced(text, row, [(1, 3), (7, 3), (56, 3), (1 << 40, 3)]), U.walk_upto(text, row, 3), (name, i))
        _same(U.Walk(text, row).run(8, 3), U.walk_upto(text, row, 3, 8), (name, i))
        # a slice with a smaller k ends an instance that holds it, its counters as they were
        w = U.Walk(text, row)
        part = w.run(3, 5)
        if part["status"] == U.LIMIT and part["solutions"] >= 1:
            after = w.run(1 << 40, 1)
            assert after["status"] == U.DONE and all(after[f] == part[f] for f in ALL_FIELDS[1:])


def test_the_eight_sets_end_within_296_nodes_but_for_the_undecided_instance():
    fewer = set()
    for name in usets.EIGHT:
        for k in (2, 5):
            res = usets.walk(name, k)
            limit = np.flatnonzero(res["status"] == U.LIMIT).tolist()
            done = res["status"] == U.DONE
            assert done.sum() + len(limit) == len(res["status"])
            assert res["nodes"][done].max() <= 296, (name, k)
            if name == usets.UNDECIDED[0]:
                i = usets.UNDECIDED[1]
                assert limit == [i] and res["nodes"][i] == 4096 and res["solutions"][i] == 0
            else:
                assert limit == [], (name, k)
            assert (res["solutions"] <= k).all() and (res["solutions"][done] >= 0).all()
            if k == 5 and ((res["solutions"] >= 1) & (res["solutions"] <= 4) & done).any():
                fewer.add(name)
            print(f"{name}, k = {k}: largest walk {int(res['nodes'][done].max())} nodes, solutions per instance "
                  f"{dict(zip(*map(np.ndarray.tolist, np.unique(res['solutions'], return_counts=True))))}")
    assert {"wcet_max", "tree20_all", "mixed40_any"} <= fewer
    tree = usets.walk("tree20_all", 5)
    assert np.flatnonzero(tree["solutions"] == 1).tolist() == [9, 19]
    assert tree["nodes"][9] == 5 and tree["nodes"][19] == 0 and tree["status"][19] == U.DONE
    two = usets.walk("tree20_all", 2)
    assert np.flatnonzero(two["solutions"] == 1).tolist() == [9, 19]


def test_schedule5_classes_holds_every_class():
    res = usets.walk("schedule5_classes", 2)
    assert (res["status"] == U.DONE).all() and len(res["status"]) == 32
    at_root = (res["solutions"] == 0) & (res["nodes"] == 0)
    assert int(at_root.sum()) == 29
    assert res["solutions"][13] == 0 and res["nodes"][13] == 52
    assert res["solutions"][19] == 1
    assert res["solutions"][2] == 2 and res["nodes"][2] == 29
    assert sorted(np.flatnonzero(~at_root).tolist()) == [2, 13, 19]
    # unique means unique: the ALL walk of row 19 holds one solution too
    text, roots = usets.build("schedule5_classes")
    assert W.walk(text, roots[19], "ALL")["solutions"] == 1


def test_schedule5_slices_stop_and_go():
    text, roots = usets.build("schedule5_slices")
    assert roots is sets.build("schedule5_min")[1] and usets.SLICES == (8, 32, 512)
    after, stopped = usets.sliced()
    left = [int((a["status"] == U.LIMIT).sum()) for a in after]
    assert left == [29, 4, 0] and [len(s) for s in stopped] == left
    held = after[0]["solutions"][after[0]["status"] == U.LIMIT]
    assert held.min() == 0 and held.max() == 4
    assert (after[0]["nodes"][after[0]["status"] == U.LIMIT] == 8).all()
    assert (after[2]["status"] == U.DONE).all() and after[2]["nodes"].max() == 296
    one = usets.walk("schedule5_slices", 5)
    assert usets.SETS["schedule5_slices"][2] == 552
    for f in ALL_FIELDS + ("rows",):
        assert (after[2][f] == one[f]).all(), f
    for k, b in enumerate(np.cumsum(usets.SLICES)[:2]):  # the small budgets once more, from the root row
        ref = usets.walk("schedule5_slices", 5, int(b))
        for f in ALL_FIELDS + ("rows",):
            assert (after[k][f] == ref[f]).all(), (k, f)
    # the second solution of these rows is near: what makes up-to-2 cheap beside ALL
    two = usets.walk("schedule5_slices", 2)
    assert (two["solutions"] == 2).all() and two["nodes"].min() == 3 and two["nodes"].max() == 272
