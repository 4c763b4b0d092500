"""CPU tests of the checkpoints of solve_many (csgpu_solve_many_checkpointed / _resume, csgpu_many_checkpoint_*): the
interface is declared, exported and prototyped; the argument errors that need no device; the slot size; the shipped
cs_dive_resume instantiations; and the stop-and-continue host walk (tests/many_resume_walk.py) that the GPU tests lean
on, against the one-budget walk of tests/many_walk.py."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import many_resume_walk
import many_sets
import many_walk
from conftest import golden
from csolve_amd import problems

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
FIELDS = ("status", "root_props", "nodes", "cuts", "props", "solutions")
NEW_CALLS = {"csgpu_many_checkpoint_bytes": 1, "csgpu_many_checkpoints_create": 3, "csgpu_many_checkpoints_reset": 2,
             "csgpu_many_checkpoints_free": 1, "csgpu_solve_many_checkpointed": 9, "csgpu_solve_many_resume": 8,
             "csgpu_many_checkpoint_states": 6}


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import ManyCheckpoints, Model
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = _lib.load_library()
    for name, args in NEW_CALLS.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
    assert re.search(r"#define\s+CSGPU_MANY_BAD_SLOT\s+3\b", text) and _lib.MANY_BAD_SLOT == 3
    assert re.search(r"typedef struct csgpu_many_checkpoints csgpu_many_checkpoints;", text)
    # the old call, its records and its options are what they were
    assert len(L.csgpu_solve_many.argtypes) == 7 and C.sizeof(_lib.ManyResult) == 40 and C.sizeof(_lib.ManyOptions) == 16
    for method in ("many_checkpoints", "resume_many", "checkpoint_states", "solve_many_sliced", "many_resume_kernel"):
        assert callable(getattr(Model, method)), method
    assert callable(ManyCheckpoints.reset)
    assert not any("dive" in f or "many" in f for f in _lib.PLAN_FAMILIES)


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import ManyOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(open(golden("problems", "queens8.txt")).read())  # parsed, not finalized
    rows = np.zeros((2, 8, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    slots = np.full(2, -1, dtype=np.int32)
    pool = C.create_string_buffer(64)  # stands for a pool: no call gets as far as looking into it
    ok = ManyOptions(0, 0, 100)

    def fresh(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data):
        rc = L.csgpu_solve_many_checkpointed(model, roots, count, C.byref(opt) if opt is not None else None, results, None,
                                             ck, sl, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    def resume(model=m._h, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data):
        rc = L.csgpu_solve_many_resume(model, count, C.byref(opt) if opt is not None else None, results, None, ck, sl, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    assert fresh(roots=None)[0] == E_ARG
    for call in (fresh, resume):
        assert call(model=None)[0] == E_ARG
        assert call(results=None)[0] == E_ARG
        assert call(opt=None)[0] == E_ARG
        assert call(ck=None)[0] == E_ARG
        assert call(sl=None)[0] == E_ARG
        assert call(count=-1)[0] == E_ARG
        assert call(opt=ManyOptions(0, 0, 0))[0] == E_ARG
        assert call(opt=ManyOptions(1, 0, -5))[0] == E_ARG
        for objective in (2, 3):  # MIN / MAX: a limit of the call, named
            rc, msg = call(opt=ManyOptions(objective, 0, 100))
            assert rc == E_LIMIT and "MIN" in msg and "MAX" in msg
        assert call(opt=ManyOptions(7, 0, 100))[0] == E_ARG
        rc, msg = call()
        assert rc == E_STATE and "finalized" in msg
        assert call(count=0)[0] == E_STATE  # an empty batch is no way round the state check
    assert (res == 0).all() and (slots == -1).all()

    out = C.c_void_p()
    def create(model=m._h, capacity=4, to=C.byref(out)):
        rc = L.csgpu_many_checkpoints_create(model, capacity, to)
        assert rc < 0 and L.csgpu_last_error().decode()
        return rc
    assert create(model=None) == E_ARG
    assert create(to=None) == E_ARG
    assert create(capacity=0) == E_ARG
    assert create(capacity=-3) == E_ARG
    assert create() == E_STATE
    assert out.value is None
    assert L.csgpu_many_checkpoints_reset(None, None) == E_ARG
    L.csgpu_many_checkpoints_free(None)  # as free(NULL)
    count = C.c_int64(-1)
    assert L.csgpu_many_checkpoint_states(None, 0, rows.ctypes.data, 2, C.byref(count), None) == E_ARG
    assert L.csgpu_many_checkpoint_states(pool, 0, None, 2, C.byref(count), None) == E_ARG
    assert L.csgpu_many_checkpoint_states(pool, 0, rows.ctypes.data, 2, None, None) == E_ARG
    assert count.value == -1
    # the Python methods: the library's state error, nothing is uploaded
    from csolve_amd._lib import CsolveError
    with pytest.raises(CsolveError) as e:
        m.many_checkpoints(4)
    assert e.value.code == E_STATE


@pytest.mark.parametrize("which,n", [("queens12", 12), ("sudoku9", 81)])
def test_slot_size_of_a_qualifying_model(which, n):
    """no device: the host tables on the root domains are all the rule depends on"""
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    text = problems.queens(12, "ALL") if which == "queens12" else problems.sudoku_roots(3, 0.4, [1])[0]
    m = Model.from_text(text)
    assert m.n_vars == n
    assert m.checkpoint_bytes() == 0  # no tables yet: nothing says that it qualifies
    m.set_domains(many_walk.oracle_for(text)[1])  # the root phase, by the oracle
    m.normalize()
    m.build_tables()
    size = m.checkpoint_bytes()
    assert size > 0 and size % 8 == 0 and size >= (n + 1) * (n + 1) * 8
    assert size == int(_lib.load_library().csgpu_many_checkpoint_bytes(m._h))
    if which == "queens12":
        assert size < 1500  # "about 1.4 KB": a pool for thousands of instances stays small


def test_slot_size_is_zero_for_a_model_outside_kernel_7():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    text = problems.schedule(6, 1)
    m = Model.from_text(text)
    m.set_domains(many_walk.oracle_for(text)[1])
    m.normalize()
    m.build_tables()
    assert m.checkpoint_bytes() == 0
    assert _lib.load_library().csgpu_many_checkpoint_bytes(None) == 0


def shipped_resume_kernels():
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == "cs_dive_resume" and "<" in name:
                shipped.add(name)
    return shipped


def resume_kernel_of(name):
    """the cs_dive_resume instantiation of a set of many_sets: its cs_dive_shave one, E and R the same"""
    return many_sets.SETS[name][3].replace("cs_dive_shave", "cs_dive_resume")


def test_shipped_resume_kernels_are_the_six_the_sets_name():
    from test_solve_many_host import shipped_dive_kernels
    shipped = shipped_resume_kernels()
    assert len(shipped) == 6
    for name in shipped:
        assert re.fullmatch(r"cs_dive_resume<unsigned (char|short), ([124])>", name), name
    assert {resume_kernel_of(s) for s in many_sets.SETS} == shipped
    assert len(shipped_dive_kernels()) == 6  # the old family is what it was


SPLITS = {"queens12_two": [(1, 7), (8, 56), (64, 300), (500, 1), (3, 100000)],
          "sudoku9_all": [(1, 7), (8, 56), (64, 300), (200, 1), (5, 100000)]}


@pytest.mark.parametrize("name", sorted(SPLITS))
def test_a_walk_in_two_parts_is_the_walk_with_the_summed_budget(name):
    text, roots, objective, _ = many_sets.build(name)
    stopped = 0
    for i in range(8):
        for b1, b2 in SPLITS[name]:
            w = many_resume_walk.Walk(text, roots[i], objective)
            part = w.run(b1)
            want1 = many_walk.dive(text, roots[i], objective, b1)
            whole = w.run(b2)
            want = many_walk.dive(text, roots[i], objective, b1 + b2)
            for got, ref in ((part, want1), (whole, want)):
                for f in FIELDS:
                    assert got[f] == ref[f], (name, i, b1, b2, f)
                assert (got["first"] is None) == (ref["first"] is None)
                assert got["first"] is None or (got["first"] == ref["first"]).all()
            stopped += part["status"] == many_walk.LIMIT
    assert stopped >= 8, "the budgets must stop instances"


@pytest.mark.parametrize("name,budget", [("queens12_two", 64), ("sudoku9_all", 64), ("sudoku9_all", 8)])
def test_the_open_subtrees_of_a_stopped_walk_hold_the_remaining_solutions(name, budget):
    text, roots, _, _ = many_sets.build(name)
    stopped = last_value = 0
    for i in range(8):
        full = many_walk.dive(text, roots[i], "ALL")
        assert full["status"] == many_walk.DONE
        w = many_resume_walk.Walk(text, roots[i], "ALL")
        part = w.run(budget)
        if part["status"] != many_walk.LIMIT:
            assert part["solutions"] == full["solutions"]
            continue
        stopped += 1
        states = w.open_subtrees()
        assert states.shape == (len(w.stack) + 1, roots.shape[1], 2)
        last_value += w.has_last_value_frame()
        assert many_resume_walk.solutions_below(text, states) == full["solutions"] - part["solutions"], (name, i)
    assert stopped >= 2, "the budget must stop instances"
    print(f"{name}, budget {budget}: {stopped} stopped, {last_value} with a frame before its variable's last value")
