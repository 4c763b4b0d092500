"""CPU tests of the checkpoints, slices and spread of the allowed-values walk (csgpu_solve_many_allowed_checkpointed /
_resume, _allowed_upto_checkpointed / _upto_resume, csgpu_many_allowed_checkpoint_children / _fanout,
Model.solve_many_allowed, solve_many_sliced / solve_many_spread with branching="allowed"): the interface is declared,
exported and prototyped; the argument errors in their documented order, without a device and with the results untouched
under a sentinel; the shipped instantiations; and the identity the spread rests on, on the host walk alone: the ALLOWED
untried children of a stopped many_walk_allowed.Walk, each walked as a root row of its own and folded with the width
walk's formula, give the record of the one walk.  (The refusal of a model with more than 128 values and of a clause-kind
pool need a finalized model, which needs a device: tests/test_gpu_solve_many_allowed_resume.py.)"""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import many_allowed_sets
import many_allowed_spread_walk as spread
import many_walk
import many_walk_allowed
from conftest import golden

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
FIELDS = many_walk.FIELDS
NEW_CALLS = {"csgpu_solve_many_allowed_checkpointed": 9, "csgpu_solve_many_allowed_resume": 8,
             "csgpu_solve_many_allowed_upto_checkpointed": 9, "csgpu_solve_many_allowed_upto_resume": 8,
             "csgpu_many_allowed_checkpoint_children": 5, "csgpu_many_allowed_checkpoint_fanout": 8}
SENTINEL = 77


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    raw = open(_lib.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = _lib.load_library()
    for name, args in NEW_CALLS.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
        proto = re.search(rf"\bint {name}\((.*?)\);", text, flags=re.S)
        assert proto and len(proto.group(1).split(",")) == args, name
    for name in ("csgpu_internal_many_allowed_resume_symbol", "csgpu_internal_many_allowed_upto_resume_symbol"):
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == 3
        assert name not in raw
    # the width calls and the fold are what they were
    assert len(L.csgpu_solve_many_checkpointed.argtypes) == 9 and len(L.csgpu_solve_many_resume.argtypes) == 8
    assert len(L.csgpu_many_checkpoint_children.argtypes) == 5 and len(L.csgpu_many_fold.argtypes) == 5
    assert C.sizeof(_lib.ManyResult) == 40 and C.sizeof(_lib.ManyOptions) == 16 and C.sizeof(_lib.ManyUptoOptions) == 16
    for method in ("solve_many_sliced", "solve_many_spread", "checkpoint_children", "checkpoint_fanout", "solve_many",
                   "solve_many_upto"):
        assert inspect.signature(getattr(Model, method)).parameters["branching"].default == "width", method
    params = inspect.signature(Model.solve_many_allowed).parameters
    assert params["max_solutions"].default is None and params["checkpoints"].default is None
    for method in ("many_allowed_resume_kernel", "many_allowed_upto_resume_kernel"):
        assert callable(getattr(Model, method)), method
    # the header says what is, and what still is not, on this walk
    not_on = re.search(r"Not on this walk[^:]*:(.*?)\.", raw, flags=re.S).group(1)
    for gone in ("checkpoints", "slices", "spread"):
        assert gone not in not_on, gone
    for stays in ("restarts", "stream", "clause"):
        assert stays in not_on, stays
    assert not any("dive" in f or "many" in f or "allowed" in f for f in _lib.PLAN_FAMILIES) and len(_lib.PLAN_FAMILIES) == 16


def test_argument_errors_come_in_their_order_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import ManyOptions, ManyUptoOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(open(golden("problems", "queens8.txt")).read())  # parsed, not finalized
    rows = np.zeros((2, 8, 2), dtype=np.int32)
    res = np.full((2, 5), SENTINEL, dtype=np.int64)
    sol = np.full((2, 2, 8), SENTINEL, dtype=np.int32)
    slots = np.full(2, SENTINEL, dtype=np.int32)
    pool = C.create_string_buffer(64)  # stands for a pool: no call gets as far as looking into it
    ok, ok_k = ManyOptions(0, 0, 100), ManyUptoOptions(2, 0, 100)

    def caller(entry, with_roots):
        def call(model=m._h, roots=rows.ctypes.data, count=2, opt="default", results=res.ctypes.data, ck=pool,
                 sl=slots.ctypes.data):
            if opt == "default":
                opt = ok_k if "upto" in entry else ok
            args = [model] + ([roots] if with_roots else []) + [count, C.byref(opt) if opt is not None else None, results,
                                                                 sol.ctypes.data, ck, sl, None]
            rc = getattr(L, entry)(*args)
            msg = L.csgpu_last_error().decode()
            assert rc < 0 and msg, (entry, rc, msg)
            return rc, msg
        return call

    fresh, resume = caller("csgpu_solve_many_allowed_checkpointed", True), caller("csgpu_solve_many_allowed_resume", False)
    fresh_k = caller("csgpu_solve_many_allowed_upto_checkpointed", True)
    resume_k = caller("csgpu_solve_many_allowed_upto_resume", False)
    assert fresh(roots=None)[0] == E_ARG and fresh_k(roots=None)[0] == E_ARG
    for call, options, first in ((fresh, ManyOptions, 0), (resume, ManyOptions, 0), (fresh_k, ManyUptoOptions, 2),
                                 (resume_k, ManyUptoOptions, 2)):
        for missing in ("model", "results", "opt", "ck", "sl"):
            rc, msg = call(**{missing: None, "count": -1})  # the null pointer is named first
            assert rc == E_ARG and "null" in msg, (missing, msg)
        rc, msg = call(count=-1, opt=options(first, 0, 0))  # the count before the budget
        assert rc == E_ARG and "count" in msg
        assert call(opt=options(first, 0, 0))[0] == E_ARG
        assert "max_nodes" in call(opt=options(first, 0, -5))[1]
        rc, msg = call()
        assert rc == E_STATE and "finalized" in msg
        assert call(count=0)[0] == E_STATE  # an empty batch is no way round the state check
    for call in (fresh, resume):
        for objective in (2, 3):  # MIN / MAX: a limit of the call, named, before the model's state
            rc, msg = call(opt=ManyOptions(objective, 0, 100))
            assert rc == E_LIMIT and "MIN" in msg and "MAX" in msg
        assert call(opt=ManyOptions(7, 0, 100))[0] == E_ARG
        assert "max_nodes" in call(opt=ManyOptions(7, 0, 0))[1]  # the budget before the objective
    for call in (fresh_k, resume_k):
        for k in (0, -3):
            rc, msg = call(opt=ManyUptoOptions(k, 0, 100))
            assert rc == E_ARG and "max_solutions" in msg
        assert "max_nodes" in call(opt=ManyUptoOptions(0, 0, 0))[1]  # the budget before k
    assert (res == SENTINEL).all() and (sol == SENTINEL).all() and (slots == SENTINEL).all()


def test_fan_out_errors_are_those_of_the_width_calls():
    from csolve_amd import _lib
    L = _lib.load_library()
    pool = C.create_string_buffer(64)  # all zero: a pool of csgpu_many_checkpoints_create's kind
    slots = np.full(4, -1, dtype=np.int32)
    children = np.full(4, SENTINEL, dtype=np.int64)
    offsets = np.zeros(5, dtype=np.int64)
    rows = np.full((4, 8, 2), SENTINEL, dtype=np.int32)
    owner = np.full(4, SENTINEL, dtype=np.int32)

    def refused(pair, word):
        for rc in pair:
            msg = L.csgpu_last_error().decode()
            assert rc == E_ARG and word in msg, (rc, msg)

    def count_children(ck=pool, sl=slots.ctypes.data, count=4, out=children.ctypes.data):
        """the allowed call, then the width call: the same refusal"""
        yield L.csgpu_many_allowed_checkpoint_children(ck, sl, count, out, None)
        yield L.csgpu_many_checkpoint_children(ck, sl, count, out, None)

    def fan_out(ck=pool, sl=slots.ctypes.data, count=4, off=offsets.ctypes.data, to=rows.ctypes.data, own=owner.ctypes.data,
                total=4):
        yield L.csgpu_many_allowed_checkpoint_fanout(ck, sl, count, off, to, own, total, None)
        yield L.csgpu_many_checkpoint_fanout(ck, sl, count, off, to, own, total, None)

    for missing in ("ck", "sl", "out"):
        refused(count_children(**{missing: None}), "null")
        refused(count_children(**{missing: None, "count": -1}), "null")
    refused(count_children(count=-1), "negative")
    for missing in ("ck", "sl", "off", "to"):
        refused(fan_out(**{missing: None}), "null")
        refused(fan_out(**{missing: None, "count": -1, "total": -1}), "null")
    refused(fan_out(count=-1), "negative instance")
    refused(fan_out(total=-1), "negative row")
    refused(fan_out(count=-1, total=0), "negative")
    assert list(count_children(count=0)) == [0, 0]
    assert list(fan_out(count=0)) == [0, 0] and list(fan_out(total=0)) == [0, 0] and list(fan_out(total=0, own=None)) == [0, 0]
    assert (children == SENTINEL).all() and (rows == SENTINEL).all() and (owner == SENTINEL).all()


def test_python_refuses_an_unknown_rule_and_keeps_the_pinned_errors():
    from csolve_amd._lib import CsolveError
    from csolve_amd.solver import Model
    m = Model.from_text(open(golden("problems", "queens8.txt")).read())
    rows = np.zeros((2, 8, 2), dtype=np.int32)
    pool = object()
    with pytest.raises(ValueError, match="checkpoints"):
        m.solve_many(rows, "ANY", max_nodes=10, checkpoints=pool, branching="allowed")
    with pytest.raises(ValueError, match="checkpoints"):
        m.solve_many_upto(rows, 2, max_nodes=10, checkpoints=pool, branching="allowed")
    for use in (lambda: m.solve_many_sliced(rows, "ANY", budgets=(4, 8), branching="narrowest"),
                lambda: m.solve_many_spread(rows, budgets=(4, 8), branching="narrowest"),
                lambda: m.solve_many(rows, "ANY", max_nodes=10, branching="narrowest")):
        with pytest.raises(ValueError, match="branching"):
            use()
    # the new entry on a model that is not finalized: the library's state error, nothing is uploaded
    for use in (lambda: m.solve_many_allowed(rows, "ANY", max_nodes=10),
                lambda: m.solve_many_allowed(rows, max_nodes=10, max_solutions=2)):
        with pytest.raises(CsolveError) as e:
            use()
        assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.solve_many_allowed(rows, max_nodes=10, max_solutions=0)
    assert e.value.code == E_ARG


def test_shipped_checkpoint_kernels_are_the_twelve_of_each_family():
    """the device-free half of the coverage test: the sets of many_allowed_sets name every (E, R, NW) of both new kernels;
    the four older families are what they were"""
    from test_solve_many_allowed_host import shipped_allowed_kernels
    from test_solve_many_host import shipped_dive_kernels
    ck, ck_upto = shipped_allowed_kernels("cs_dive_allowed_resume"), shipped_allowed_kernels("cs_dive_allowed_upto_resume")
    assert len(ck) == len(ck_upto) == 12
    named = {s[4] for s in many_allowed_sets.SETS.values()}
    assert {k.replace("cs_dive_allowed<", "cs_dive_allowed_resume<") for k in named} == ck
    assert {k.replace("cs_dive_allowed<", "cs_dive_allowed_upto_resume<") for k in named} == ck_upto
    assert len(shipped_allowed_kernels("cs_dive_allowed")) == len(shipped_allowed_kernels("cs_dive_allowed_upto")) == 12
    assert len(shipped_dive_kernels()) == 6
    fans = shipped_allowed_kernels("cs_dive_allowed_children") | shipped_allowed_kernels("cs_dive_allowed_fanout")
    assert fans == {f"cs_dive_allowed_{k}<unsigned {e}>" for k in ("children", "fanout") for e in ("char", "short")}


# ---- the exactness argument, on the host walk alone ---------------------------------------------------------------------

@pytest.mark.parametrize("budget", [5, 40])
@pytest.mark.parametrize("name", ["queens8_all", "sudoku9_40_all"])
def test_the_allowed_children_folded_are_the_rest_of_the_walk(name, budget):
    """a walk stopped at `budget`, its ALLOWED untried children walked to their ends as root rows of their own: stopped
    record + fold = the one walk, counter for counter"""
    text, roots, _, _, _ = many_allowed_sets.build(name)
    stopped = fewer = 0
    for row in roots[:8]:
        whole = many_walk_allowed.Walk(text, row).run(1 << 62)
        w = many_walk_allowed.Walk(text, row)
        part = w.run(budget)
        if part["status"] != many_walk.LIMIT:
            assert all(part[f] == whole[f] for f in FIELDS)
            continue
        stopped += 1
        rows = spread.children_of(w)
        assert len(rows) == spread.count_children(w) <= spread.width_count(w) and rows.dtype == np.int32
        fewer += len(rows) < spread.width_count(w)
        assert all(len(values) >= 1 for _, _, values in spread.untried(w)), "every frame has an allowed value left"
        node, v, values = spread.untried(w)[0]
        assert values[0] == w.nv  # the current node stands before an allowed value
        total = spread.folded(text, w, part)
        for f in spread.COUNTERS:
            assert total[f] == whole[f], (name, budget, f, total[f], whole[f])
    assert stopped >= 1
    print(f"{name}, budget {budget}: {stopped} stopped, {fewer} with fewer children than the width formula counts")
    if name == "sudoku9_40_all":
        assert fewer >= 1, "the set must show the rule: a forbidden value inside [next, hi]"


def test_a_forbidden_child_row_would_be_one_cut_too_many():
    """why the fan-out lists the allowed values only: a forbidden value as a root row is inconsistent -- the width fold
    would count it a node and a cut the allowed walk never counts"""
    text, roots, _, _, _ = many_allowed_sets.build("sudoku9_40_all")
    seen = 0
    for row in roots[:8]:
        w = many_walk_allowed.Walk(text, row)
        if w.run(40)["status"] != many_walk.LIMIT:
            continue
        for node, v, values in spread.untried(w):
            nv = values[0]
            for c in range(nv, int(node[v, 1]) + 1):
                if c in values:
                    continue
                bad = node.copy()
                bad[v] = (c, c)
                sub = many_walk_allowed.Walk(text, bad).run(1 << 62)
                assert sub["status"] == many_walk.DONE and sub["nodes"] == 0 and sub["solutions"] == 0
                seen += 1
    assert seen >= 1
