"""CPU tests of the clause checkpoints (csgpu_solve_many_clauses_checkpointed / _resume, csgpu_many_clause_checkpoint_*):
the interface is declared, exported and prototyped; the argument errors that need no device, in their documented order;
the slot size; the shipped cs_walk_resume instantiations; and, on the host walk of tests/many_walk_objective.py, that the
slices the GPU tests use (tests/many_clause_resume_walk.py) stop instances inside their trees, change incumbents after the
first slice and leave open subtrees that hold the rest of the tree -- so that no GPU test passes vacuously."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import many_clause_resume_walk as R
import many_clause_sets as sets
import many_resume_walk
import many_walk_objective as W
from csolve_amd import problems

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
NEW_CALLS = {"csgpu_many_clause_checkpoint_bytes": 1, "csgpu_many_clause_checkpoints_create": 3,
             "csgpu_solve_many_clauses_checkpointed": 10, "csgpu_solve_many_clauses_resume": 9,
             "csgpu_many_clause_checkpoint_states": 8}
INTERNAL = {"csgpu_internal_many_clauses_resume_symbol": 3}
EIGHT = {f"cs_walk_resume<{cpl}, {tree}>" for cpl in (1, 2, 4, 8) for tree in ("true", "false")}


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import ManyCheckpoints, Model
    L = _lib.load_library()
    for name, args in NEW_CALLS.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
    for name, args in INTERNAL.items():  # exported and prototyped, declared in cs_internal.h only
        assert name not in _lib.declared_symbols() and len(getattr(L, name).argtypes) == args, name
    # the two calls that serve both kinds of pool, and the old clause call, are what they were
    assert len(L.csgpu_many_checkpoints_reset.argtypes) == 2 and len(L.csgpu_many_checkpoints_free.argtypes) == 1
    assert len(L.csgpu_solve_many_clauses.argtypes) == 8 and len(L.csgpu_many_checkpoint_states.argtypes) == 6
    for method in ("clause_checkpoint_bytes", "many_clause_checkpoints", "resume_many_clauses", "clause_checkpoint_states",
                   "open_clause_subtrees", "solve_many_clauses_sliced", "many_clauses_resume_kernel"):
        assert callable(getattr(Model, method)), method
    assert callable(ManyCheckpoints.reset)
    assert not any("walk" in f or "many" in f for f in _lib.PLAN_FAMILIES)
    header = open(_lib.HEADER_PATH).read()
    for phrase in ("clause checkpoints", "{best, have_best | objective << 1}", "Not here: up to k solutions and restarts"):
        assert phrase in header, phrase
    assert "No checkpoints" not in header


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(problems.schedule(5, 1))  # MIN; parsed, not finalized
    plain = Model.from_text(problems.linear(12, 1, "ALL"))  # no objective variable
    n = m.n_vars
    rows = np.zeros((2, n, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    slots = np.full(2, -1, dtype=np.int32)
    pool = C.create_string_buffer(64)  # stands for a pool: no call gets as far as looking into it
    ok = ManyOptions(0, 0, 100)

    def fresh(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data):
        rc = L.csgpu_solve_many_clauses_checkpointed(model, roots, count, C.byref(opt) if opt is not None else None, results,
                                                     None, None, ck, sl, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    def resume(model=m._h, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data):
        rc = L.csgpu_solve_many_clauses_resume(model, count, C.byref(opt) if opt is not None else None, results, None, None,
                                               ck, sl, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    assert fresh(roots=None)[0] == E_ARG
    for call in (fresh, resume):  # csgpu_solve_many_clauses's checks, in its order, whatever the pool arguments are
        for ck, sl in ((pool, slots.ctypes.data), (None, slots.ctypes.data), (pool, None)):
            assert call(model=None, ck=ck, sl=sl)[0] == E_ARG
            assert call(results=None, ck=ck, sl=sl)[0] == E_ARG
            assert call(opt=None, ck=ck, sl=sl)[0] == E_ARG
            assert call(count=-1, ck=ck, sl=sl)[0] == E_ARG
            rc, msg = call(opt=ManyOptions(0, 0, 0), ck=ck, sl=sl)
            assert rc == E_ARG and "max_nodes" in msg
            assert call(opt=ManyOptions(2, 0, -5), ck=ck, sl=sl)[0] == E_ARG
            assert call(opt=ManyOptions(7, 0, 100), ck=ck, sl=sl)[0] == E_ARG
            assert call(opt=ManyOptions(-1, 0, 100), ck=ck, sl=sl)[0] == E_ARG
            rc, msg = call(opt=ManyOptions(3, 0, 100), ck=ck, sl=sl)  # MAX on a MIN model
            assert rc == E_ARG and "MIN" in msg and "MAX" in msg
            for objective in (2, 3):  # MIN / MAX on a model without an objective
                rc, msg = call(model=plain._h, opt=ManyOptions(objective, 0, 100), ck=ck, sl=sl)
                assert rc == E_ARG and "objective" in msg
            # well-formed otherwise: the state comes before the pool is looked at, a null one included
            for opt in (ok, ManyOptions(1, 0, 100), ManyOptions(2, 0, 100)):
                rc, msg = call(opt=opt, ck=ck, sl=sl)
                assert rc == E_STATE and "finalized" in msg
            assert call(count=0, ck=ck, sl=sl)[0] == E_STATE  # an empty batch is no way round the state check
    assert (res == 0).all() and (slots == -1).all()

    out = C.c_void_p()

    def create(model=m._h, capacity=4, to=C.byref(out)):
        rc = L.csgpu_many_clause_checkpoints_create(model, capacity, to)
        assert rc < 0 and L.csgpu_last_error().decode()
        return rc
    assert create(model=None) == E_ARG
    assert create(to=None) == E_ARG
    assert create(capacity=0) == E_ARG
    assert create(capacity=-3) == E_ARG
    assert create() == E_STATE
    assert out.value is None
    count, best, have = C.c_int64(-1), C.c_int32(-7), C.c_int32(-7)

    def states(ck=pool, to=rows.ctypes.data, cnt=C.byref(count), b=C.byref(best), h=C.byref(have)):
        return L.csgpu_many_clause_checkpoint_states(ck, 0, to, 2, cnt, b, h, None)
    assert states(ck=None) == E_ARG
    assert states(to=None) == E_ARG
    assert states(cnt=None) == E_ARG
    assert states(b=None) == E_ARG
    assert states(h=None) == E_ARG
    assert (count.value, best.value, have.value) == (-1, -7, -7)
    # the Python methods: the library's state error, nothing is uploaded
    with pytest.raises(CsolveError) as e:
        m.many_clause_checkpoints(4)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.many_clauses_resume_kernel()
    assert e.value.code == E_STATE


@pytest.mark.parametrize("name", ["schedule6_min_budget", "linear20_all", "mixed120_any"])
def test_slot_size_after_the_tables_alone(name):
    """no device: (n + 1)^2 x 8 once csgpu_model_build_tables has run, 0 before and for NULL"""
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    text = sets.build(name)[0]
    m = Model.from_text(text)
    n = m.n_vars
    assert m.clause_checkpoint_bytes() == 0  # no tables yet: nothing says that it qualifies
    m.set_domains(W.oracle_for(text)[1])
    m.normalize()
    m.build_tables()
    assert m.clause_checkpoint_bytes() == (n + 1) * (n + 1) * 8
    assert _lib.load_library().csgpu_many_clause_checkpoint_bytes(None) == 0
    if name == "schedule6_min_budget":
        assert text == problems.schedule(6, 1) and m.checkpoint_bytes() == 0  # the pools of solve_many are not for it


def test_slot_size_is_zero_beyond_512_clauses():
    from csolve_amd.solver import Model
    text = problems.schedule(32, 1)
    m = Model.from_text(text)
    m.set_domains(W.oracle_for(text)[1])
    m.normalize()
    m.build_tables()
    assert m.n_clauses > 512 and m.clause_checkpoint_bytes() == 0


def shipped_walk_resume_kernels():
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == "cs_walk_resume" and "<" in name:
                shipped.add(name)
    return shipped


def resume_kernel_of(name):
    """the cs_walk_resume instantiation of a set: its cs_walk_clauses one, CPL and HAS_TREE the same"""
    return sets.SETS[name][3].replace("cs_walk_clauses", "cs_walk_resume")


def test_the_shipped_resume_kernels_are_exactly_the_eight():
    from test_solve_many_clauses_host import shipped_walk_kernels
    shipped = shipped_walk_resume_kernels()
    for name in shipped:
        assert re.fullmatch(r"cs_walk_resume<[1248], (true|false)>", name), name
    assert shipped == EIGHT == {resume_kernel_of(s) for s in sets.SETS}
    assert len(shipped_walk_kernels()) == 8  # the old family is what it was


def _changes(after):
    """instances whose incumbent differs between the answers of two consecutive slices, summed over the later slices"""
    total = 0
    for a, b in zip(after, after[1:]):
        both = (a["solutions"] > 0) & (b["solutions"] > 0)
        total += int((both & (a["best"] != b["best"])).sum())
    return total


def test_the_slices_stop_instances_inside_their_trees():
    """what the table of the issue supports, not its exact counts: every set has stopped instances after slices 1 and 2,
    seven sets after slice 3, three sets change an incumbent in a later slice, both budget sets end with LIMIT instances
    with and without a solution; and a walk in slices is the set's one walk"""
    after3 = changing = 0
    for name in sorted(sets.SETS):
        text, roots, objective, budget = sets.build(name)
        assert sum(R.slices(name)) == budget
        after, stopped, _ = R.sliced(name)
        want = sets.walked(name)
        for f in W.FIELDS + ("props", "root_props", "best", "first"):
            assert (after[3][f] == want[f]).all(), (name, f)
        left = [int((a["status"] == W.LIMIT).sum()) for a in after]
        assert [len(s) for s in stopped] == left
        changed = _changes(after) if objective in ("MIN", "MAX") else 0
        print(f"{name}: at LIMIT after each slice {left}, incumbent changes in a later slice {changed}")
        assert left[0] > 0 and left[1] > 0, name
        after3 += left[2] > 0
        changing += changed > 0
        for k, b in enumerate(np.cumsum(R.slices(name))[:3]):  # the small budgets once more, from the root row
            ref = W.walk_many(text, roots, objective, int(b))
            for f in W.FIELDS + ("best",):
                assert (after[k][f] == ref[f]).all(), (name, k, f)
        if name in sets.BUDGET:
            limit = after[3]["status"] == W.LIMIT
            assert (limit & (after[3]["solutions"] > 0)).any() and (limit & (after[3]["solutions"] == 0)).any(), name
        else:
            assert left[3] == 0
    assert after3 >= 7 and changing >= 3


def test_the_deepest_stack_is_far_below_the_frames_of_a_slot():
    deepest = {name: R.sliced(name)[2] for name in sets.SETS}
    print(deepest)
    name = max(deepest, key=deepest.get)
    assert name == "mixed120_any" and deepest[name] == 20
    # the pushed frames and the current node's: far below the n frames a slot has for them
    assert all(0 < d + 1 < W.model_of(sets.build(k)[0]).n_vars for k, d in deepest.items())


def test_schedule6_is_proven_within_the_second_budget():
    """the instances that solve_many_clauses_sliced(..., finish="search") finishes: every one DONE within 256 + 32,768
    nodes, optima 22 or 23, and some of the stopped ones improve after node 256"""
    after, stopped, _ = R.finished6()
    first, done = after
    assert (first["status"] == sets.walked("schedule6_min_budget")["status"]).all()
    assert (done["status"] == W.DONE).all() and (done["solutions"] > 0).all()
    assert int(done["nodes"].sum()) == 10311 and int(done["nodes"].max()) == 2377
    assert set(done["best"].tolist()) == {22, 23}
    left = first["status"] == W.LIMIT
    improved = left & ((first["solutions"] == 0) | (first["best"] != done["best"]))
    assert int(left.sum()) == 13 and len(stopped[0]) == 13
    assert int(improved.sum()) == 2  # (on this set: the two that had no solution at node 256; the other 11 held the optimum)


@pytest.mark.parametrize("name", ["linear20_all", "linear40_all", "tree20_all"])
def test_the_open_subtrees_of_a_stopped_walk_hold_the_rest_of_the_tree(name):
    """the export model: the states built from Walk.stack and (cur, v, nv) after 64 nodes, each walked as a root row"""
    text, roots, objective, _ = sets.build(name)
    after, stopped, _ = R.sliced(name)
    whole = sets.walked(name)
    picked = sorted(stopped[2], key=lambda i: whole["nodes"][i])[:3]
    assert picked
    for i in picked:
        states, best = stopped[2][i]
        assert best is None and states.shape[1:] == roots.shape[1:] and 1 <= states.shape[0] < roots.shape[1]
        below = many_resume_walk.solutions_below(text, states)
        assert after[2]["solutions"][i] + below == whole["solutions"][i], (name, i)
