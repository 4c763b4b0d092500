"""CPU tests of the ordered clause checkpoints (csgpu_solve_many_clauses_ordered_checkpointed / _resume,
csgpu_many_clause_ordered_checkpoint_bytes / _checkpoints_create): the interface is declared, exported and prototyped; the
argument errors that need no device, in their documented order; the slot size; the shipped cs_walk_order_resume
instantiations; and, on the host walk of tests/many_walk_ordered.py, that the slices the GPU tests use
(tests/many_ordered_resume_walk.py) stop instances inside their trees, between the two halves of a node, above pushed
halving parents and on stacks deeper than n_vars, change incumbents after the first slice and leave open subtrees that
hold the rest of the tree -- so that no GPU test passes vacuously."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import many_ordered_resume_walk as R
import many_walk_objective as W
import many_walk_ordered as O
import order_walk
from csolve_amd import problems

E_ARG, E_STATE = -1, -5
NEW_CALLS = {"csgpu_many_clause_ordered_checkpoint_bytes": 2, "csgpu_many_clause_ordered_checkpoints_create": 4,
             "csgpu_solve_many_clauses_ordered_checkpointed": 11, "csgpu_solve_many_clauses_ordered_resume": 10}
INTERNAL = {"csgpu_internal_many_clauses_order_resume_symbol": 3}
EIGHT = {f"cs_walk_order_resume<{cpl}, {tree}>" for cpl in (1, 2, 4, 8) for tree in ("true", "false")}
SPLITS = (1, 2, 4, 16, 256, 2**31 - 1)


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import ManyCheckpoints, Model
    L = _lib.load_library()
    for name, args in NEW_CALLS.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
    for name, args in INTERNAL.items():  # exported and prototyped, declared in cs_internal.h only
        assert name not in _lib.declared_symbols() and len(getattr(L, name).argtypes) == args, name
    # what serves every kind of pool, and the plain ordered call, are what they were
    assert len(L.csgpu_many_checkpoints_reset.argtypes) == 2 and len(L.csgpu_many_checkpoints_free.argtypes) == 1
    assert len(L.csgpu_solve_many_clauses_ordered.argtypes) == 9 and len(L.csgpu_many_clause_checkpoint_states.argtypes) == 8
    for method in ("many_clause_ordered_checkpoints", "clause_ordered_checkpoint_bytes", "many_clauses_order_resume_kernel",
                   "resume_many_clauses", "solve_many_clauses_sliced"):
        assert callable(getattr(Model, method)), method
    assert callable(ManyCheckpoints.reset)
    header = open(_lib.HEADER_PATH).read()
    for phrase in ("ordered clause checkpoints", "code = objective |", "d_halvings is required",
                   "Prefer-failing is not part of this walk", "a fan-out of halves has to account for `halvings`"):
        assert phrase in header, phrase
    not_on = header[header.index("Not on this walk: up to k"):]
    not_on = not_on[:not_on.index("*/")]
    assert "checkpoints and resume," not in header and "restarts" in not_on and "the solution stream" in not_on


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyOrderOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(problems.schedule(5, 1))  # MIN; parsed, not finalized
    plain = Model.from_text(problems.linear(12, 1, "ALL"))  # no objective variable
    n = m.n_vars
    rows = np.zeros((2, n, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    halv = np.full(2, -9, dtype=np.int64)
    slots = np.full(2, -1, dtype=np.int32)
    pool = C.create_string_buffer(64)  # stands for a pool: no call gets as far as looking into it
    ok = ManyOrderOptions(2, 1, 256, 0, 100)

    def fresh(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data, hv=halv.ctypes.data, ck=pool,
              sl=slots.ctypes.data):
        rc = L.csgpu_solve_many_clauses_ordered_checkpointed(model, roots, count, C.byref(opt) if opt is not None else None,
                                                             results, None, None, hv, ck, sl, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    def resume(model=m._h, count=2, opt=ok, results=res.ctypes.data, hv=halv.ctypes.data, ck=pool, sl=slots.ctypes.data):
        rc = L.csgpu_solve_many_clauses_ordered_resume(model, count, C.byref(opt) if opt is not None else None, results,
                                                       None, None, hv, ck, sl, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    assert fresh(roots=None)[0] == E_ARG
    for call in (fresh, resume):  # the head, then csgpu_solve_many_clauses's checks, whatever the later arguments are
        for ck, sl, hv in ((pool, slots.ctypes.data, halv.ctypes.data), (None, slots.ctypes.data, halv.ctypes.data),
                           (pool, None, halv.ctypes.data), (pool, slots.ctypes.data, None)):
            kw = dict(ck=ck, sl=sl, hv=hv)
            assert call(model=None, **kw)[0] == E_ARG
            assert call(results=None, **kw)[0] == E_ARG
            assert call(opt=None, **kw)[0] == E_ARG
            assert call(count=-1, **kw)[0] == E_ARG
            rc, msg = call(opt=ManyOrderOptions(2, 1, 256, 0, 0), **kw)
            assert rc == E_ARG and "max_nodes" in msg and "slice" in msg
            assert call(opt=ManyOrderOptions(2, 9, -1, 1, -5), **kw)[0] == E_ARG
            assert call(opt=ManyOrderOptions(7, 1, 256, 0, 100), **kw)[0] == E_ARG
            rc, msg = call(opt=ManyOrderOptions(3, 1, 256, 0, 100), **kw)  # MAX on a MIN model
            assert rc == E_ARG and "MIN" in msg and "MAX" in msg
            for objective in (2, 3):  # MIN / MAX on a model without an objective
                rc, msg = call(model=plain._h, opt=ManyOrderOptions(objective, 1, 256, 0, 100), **kw)
                assert rc == E_ARG and "objective" in msg
            # the state comes before the ordered entry's own checks, d_halvings and the pool
            for opt in (ok, ManyOrderOptions(2, 9, 256, 0, 100), ManyOrderOptions(2, 1, -1, 0, 100),
                        ManyOrderOptions(2, 1, 256, 1, 100), ManyOrderOptions(1, 0, 0, 0, 100)):
                rc, msg = call(opt=opt, **kw)
                assert rc == E_STATE and "finalized" in msg
            assert call(count=0, **kw)[0] == E_STATE  # an empty batch is no way round the state check
    assert (res == 0).all() and (slots == -1).all() and (halv == -9).all()

    out = C.c_void_p()

    def create(model=m._h, capacity=4, split=256, to=C.byref(out)):
        rc = L.csgpu_many_clause_ordered_checkpoints_create(model, capacity, split, to)
        assert rc < 0 and L.csgpu_last_error().decode()
        return rc
    assert create(model=None) == E_ARG
    assert create(to=None) == E_ARG
    assert create(capacity=0) == E_ARG
    assert create(capacity=-3) == E_ARG
    assert create(split=-1) == E_ARG
    assert create() == E_STATE
    assert create(split=0) == E_STATE
    assert out.value is None
    # the Python methods: the library's state error, nothing is uploaded
    with pytest.raises(CsolveError) as e:
        m.many_clause_ordered_checkpoints(4, 4)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.many_clauses_order_resume_kernel()
    assert e.value.code == E_STATE
    with pytest.raises(ValueError):
        m.solve_many_clauses_sliced(rows, "MIN", budgets=(8,), order="none", max_solutions=2)
    with pytest.raises(ValueError):
        m.resume_many_clauses({"_checkpoints": None, "_order": 0}, max_nodes=5, max_solutions=2)
    with pytest.raises(ValueError):
        m.resume_many_clauses({"_checkpoints": None, "_order": 0}, max_nodes=5, own_solutions=True)


def _tables(text):
    from csolve_amd.solver import Model
    m = Model.from_text(text)
    dom = W.oracle_for(text)[1]
    m.set_domains(dom)
    m.normalize()
    m.build_tables()
    return m, dom


@pytest.mark.parametrize("name", ["schedule5", "wide2_cut", "wide3_sums"])
def test_slot_size_after_the_tables_alone(name):
    """no device: (F + 1) (n + 1) 8 once csgpu_model_build_tables has run, F the frame bound of many_walk_ordered"""
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    text = problems.schedule(5, 1) if name == "schedule5" else order_walk.text_of(name)
    assert Model.from_text(text).clause_ordered_checkpoint_bytes(4) == 0  # no tables yet: nothing says that it qualifies
    m, dom = _tables(text)
    n = m.n_vars
    assert n == dom.shape[0]
    for s in SPLITS:
        assert m.clause_ordered_checkpoint_bytes(s) == (O.frames(dom, s) + 1) * (n + 1) * 8, s
    assert m.clause_ordered_checkpoint_bytes(0) == m.clause_ordered_checkpoint_bytes(256) == m.clause_ordered_checkpoint_bytes()
    assert m.clause_ordered_checkpoint_bytes(-1) == 0
    widest = int((dom[:, 1].astype(np.int64) - dom[:, 0] + 1).max())
    assert 1 < widest <= 2**31 - 1
    assert m.clause_ordered_checkpoint_bytes(widest) == m.clause_checkpoint_bytes() == (n + 1) * (n + 1) * 8
    assert m.clause_ordered_checkpoint_bytes(widest - 1) == (n + 1 + int((dom[:, 1].astype(np.int64) - dom[:, 0] + 1 == widest).sum())) * (n + 1) * 8
    assert m.clause_ordered_checkpoint_bytes(1) > m.clause_checkpoint_bytes()
    assert _lib.load_library().csgpu_many_clause_ordered_checkpoint_bytes(None, 256) == 0
    if name == "wide2_cut":
        assert n == 5 and O.frames(dom, 1) == 31


def test_slot_size_is_zero_beyond_512_clauses():
    m, _ = _tables(problems.schedule(32, 1))
    assert m.n_clauses > 512 and m.clause_ordered_checkpoint_bytes(256) == 0


def shipped(kernel):
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == kernel and "<" in name:
                names.add(name)
    return names


def order_resume_kernel_of(clauses_kernel):
    """the cs_walk_order_resume instantiation of a model: its cs_walk_clauses one, CPL and HAS_TREE the same"""
    return clauses_kernel.replace("cs_walk_clauses", "cs_walk_order_resume")


def test_the_shipped_order_resume_kernels_are_exactly_the_eight():
    import many_clause_sets as sets
    from test_many_clauses_resume_host import shipped_walk_resume_kernels
    from test_solve_many_clauses_ordered_host import shipped_order_kernels
    names = shipped("cs_walk_order_resume")
    for name in names:
        assert re.fullmatch(r"cs_walk_order_resume<[1248], (true|false)>", name), name
    assert names == EIGHT == {order_resume_kernel_of(s[3]) for s in sets.SETS.values()}
    assert len(shipped_order_kernels()) == 8 and len(shipped_walk_resume_kernels()) == 8  # the old families are what they were


def test_the_slices_stop_instances_inside_their_trees():
    """every case has stopped instances after slice 1, every MIN / MAX case after each of the first three (the two ANY sets
    are over within 8 nodes); incumbents exist and change after the first slice; and a walk in slices is the case's one
    walk, halvings included"""
    after2 = after3 = changing = 0
    for name, order, split in O.CASES:
        text, roots, objective, budget = O.build(name)
        assert sum(R.slices(name)) == budget
        after, stopped = R.sliced(name, order, split)
        want = O.walked(name, order, split)
        for f in R.FIELDS + ("props", "root_props", "best", "first"):
            assert (after[3][f] == want[f]).all(), (name, order, split, f)
        left = [int((a["status"] == O.LIMIT).sum()) for a in after]
        assert [len(s) for s in stopped] == left
        changed = 0
        if objective in ("MIN", "MAX"):
            for a, b in zip(after, after[1:]):
                changed += int(((a["solutions"] > 0) & (b["solutions"] > 0) & (a["best"] != b["best"])).sum())
        print(f"{name} {order}/{split}: at LIMIT after each slice {left}, incumbent changes in a later slice {changed}")
        assert left[0] > 0, (name, order, split)
        assert (left[1] > 0 and left[2] > 0) or objective == "ANY", (name, order, split)
        after2 += left[1] > 0
        after3 += left[2] > 0
        changing += changed > 0
        for k, b in enumerate(np.cumsum(R.slices(name))[:3]):  # the small budgets once more, from the root row
            ref = O.walk_many(text, roots, objective, int(b), order, split)
            for f in R.FIELDS + ("best",):
                assert (after[k][f] == ref[f]).all(), (name, order, split, k, f)
            limit = after[k]["status"] == O.LIMIT
            assert (after[k]["nodes"][limit] == b).all()
        assert left[3] == int((want["status"] == O.LIMIT).sum())
    bounded = sum(O.SETS[name][1] in ("MIN", "MAX") for name, _, _ in O.CASES)
    assert bounded == 14 and after2 >= bounded and after3 >= bounded and changing >= 3


def test_the_stops_are_where_only_the_ordered_walk_stands():
    """schedule5_open_min: between the two halves of the current node, above pushed halving parents, on more frames than
    n_vars, with incumbents -- the figures the issue gives"""
    name = "schedule5_open_min"
    n = O.build(name)[1].shape[1]
    assert n == 17
    after, stopped = R.sliced(name, "none", 4)
    at64 = stopped[2]
    assert len(at64) == 7
    assert sum(d["between"] for d in at64.values()) == 6
    assert sum(d["parents"] > 0 for d in at64.values()) == 6
    assert sum(d["frames"] > n for d in at64.values()) == 4
    assert int((after[2]["solutions"] > 0).sum()) == 5 and sum(d["best"] is not None for d in at64.values()) >= 4
    assert all(d["states"].shape[0] == d["frames"] for d in at64.values())
    after, stopped = R.sliced(name, "smallest-domain", 256)
    at64 = stopped[2]
    assert len(at64) == 8 and all(d["frames"] > n and d["best"] is not None and d["parents"] > 0 for d in at64.values())
    text, roots, objective, _ = O.build(name)
    walks = [O.Walk(text, row, objective, "smallest-domain", 256) for row in roots]
    assert all(w.run(256)["status"] == O.LIMIT and len(w.stack) + 1 > n and w.best is not None for w in walks)
    # every frame count is inside the slot
    for order, split in O.SETS[name][3]:
        F = O.frames(W.oracle_for(text)[1], split)
        assert all(d["frames"] <= F for st in R.sliced(name, order, split)[1] for d in st.values())


@pytest.mark.parametrize("name,order,split", R.ALL_ROWS)
def test_the_open_subtrees_of_a_stopped_walk_hold_the_rest_of_the_tree(name, order, split):
    """solutions so far plus the ALL solutions of the open subtrees, each walked as a root row, are the whole tree's"""
    text, roots, whole = R.all_row(name, order, split)
    n = roots.shape[1]
    assert whole["status"] == O.DONE and whole["halvings"] > 0
    for budget in (8, 64):
        res, states, frames = R.stopped_all(name, order, split, budget)
        assert states.shape == (frames, n, 2) and res["nodes"] == budget
        assert res["solutions"] + R.solutions_below(text, states, order, split) == whole["solutions"], budget
    assert R.stopped_all(name, order, split, 64)[2] > n  # a stack the (n + 1)^2 slot does not hold


def test_the_deep_row_is_the_one_of_the_issue():
    name, order, split = R.DEEP
    text, roots, whole = R.all_row(name, order, split)
    assert roots.shape[1] == 5 and O.frames(W.oracle_for(text)[1], split) == 31
    assert (whole["nodes"], whole["solutions"], whole["halvings"]) == (518, 260, 259)
    assert R.stopped_all(name, order, split, 8)[2] == 6 and R.stopped_all(name, order, split, 64)[2] == 7
