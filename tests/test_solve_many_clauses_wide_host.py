"""CPU tests of csgpu_solve_many_clauses_wide / Model.solve_many_clauses_wide: the interface is declared, exported and
prototyped; qualification from the host tables (past 512 clauses: wide and not plain; past the LDS of a CU: neither); the
argument errors that need no device; the generators beside it; the instance sets of tests/many_clause_wide_sets.py hold
every outcome class the GPU tests need them for; the shipped cs_walk_wide instantiations."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import many_clause_sets as sets
import many_clause_wide_sets as wide
import many_walk_objective as W
from csolve_amd import problems

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
CU_LDS = 160 * 1024


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    L = _lib.load_library()
    for name, args in (("csgpu_model_qualifies_many_clauses_wide", 1), ("csgpu_solve_many_clauses_wide", 8),
                       ("csgpu_solve_many_clauses_wide_checkpointed", 10), ("csgpu_solve_many_clauses_wide_resume", 9),
                       ("csgpu_many_clause_wide_checkpoint_bytes", 1), ("csgpu_many_clause_wide_checkpoints_create", 3)):
        assert name in _lib.declared_symbols(), name
        assert len(getattr(L, name).argtypes) == args, name
    for name in ("csgpu_internal_many_clauses_wide_symbol", "csgpu_internal_many_clauses_wide_resume_symbol"):
        assert name not in _lib.declared_symbols() and len(getattr(L, name).argtypes) == 3, name
    for method in ("qualifies_many_clauses_wide", "many_clauses_wide_kernel", "solve_many_clauses_wide",
                   "many_clause_wide_checkpoints", "clause_wide_checkpoint_bytes", "resume_many_clauses_wide"):
        assert callable(getattr(Model, method)), method
    assert not any("walk" in f or "wide" in f for f in _lib.PLAN_FAMILIES)  # the plan dictionary stays what it is
    header = open(_lib.HEADER_PATH).read()
    for phrase in ("THE WALK IS csgpu_solve_many_clauses's", "where the records live", "which models qualify", "160 KiB"):
        assert phrase in header, phrase


@pytest.mark.parametrize("make,n_vars,n_clauses", [(lambda: problems.schedule(32, 1), 98, 657),
                                                    (lambda: problems.sudoku_less(3, 5, 24), 81, 1159)])
def test_past_512_clauses_a_model_qualifies_wide_and_not_plain(make, n_vars, n_clauses):
    m = wide.host_model(make())
    assert (m.n_vars, m.n_clauses) == (n_vars, n_clauses)
    assert m.qualifies_many_clauses_wide() and not m.qualifies_many_clauses()
    assert m.clause_wide_checkpoint_bytes() == (n_vars + 1) ** 2 * 8
    assert m.clause_checkpoint_bytes() == 0
    if n_vars == 98:
        assert m.clause_wide_checkpoint_bytes() == 78408


def test_at_most_512_clauses_qualify_for_both():
    m = wide.host_model(problems.schedule(24, 1))
    assert m.n_clauses == 397
    assert m.qualifies_many_clauses_wide() and m.clause_wide_checkpoint_bytes() == m.clause_checkpoint_bytes() == 75 * 75 * 8


def test_a_model_whose_records_do_not_fit_lds_does_not_qualify():
    text = problems.queens(96, "ALL")  # 3 x 96 x 95 / 2 `!=` and 192 bounds: 16 bytes each are more than 160 KiB
    m = wide.host_model(text)
    assert m.n_clauses > 10000 and 16 * m.n_clauses > CU_LDS
    assert not m.qualifies_many_clauses_wide() and m.clause_wide_checkpoint_bytes() == 0
    assert not m.qualifies_many_clauses() and m.clause_checkpoint_bytes() == 0
    # the same network a little smaller fits: 64 queens are 6,177 records (the model's clause count), 98,832 bytes, and four slices of 528
    m = wide.host_model(problems.queens(64, "ALL"))
    assert m.n_clauses == 6177 and m.qualifies_many_clauses_wide() and not m.qualifies_many_clauses()
    # and a model without tables says no
    from csolve_amd.solver import Model
    bare = Model.from_text(problems.schedule(32, 1))
    assert not bare.qualifies_many_clauses_wide() and bare.clause_wide_checkpoint_bytes() == 0


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(problems.schedule(32, 1))  # MIN; parsed, not finalized
    plain = Model.from_text(problems.sudoku_less(3, 5, 24))  # no objective variable
    rows = np.zeros((2, m.n_vars, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    ok = ManyOptions(0, 0, 100)

    def call(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data):
        rc = L.csgpu_solve_many_clauses_wide(model, roots, count, C.byref(opt) if opt is not None else None, results, None, None,
                                             None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    assert call(model=None)[0] == E_ARG
    assert call(roots=None)[0] == E_ARG
    assert call(results=None)[0] == E_ARG
    assert call(opt=None)[0] == E_ARG
    assert call(count=-1)[0] == E_ARG
    assert call(opt=ManyOptions(0, 0, 0))[0] == E_ARG
    assert call(opt=ManyOptions(7, 0, 100))[0] == E_ARG
    rc, msg = call(opt=ManyOptions(3, 0, 100))  # MAX on a MIN model
    assert rc == E_ARG and "MIN" in msg and "MAX" in msg
    for objective in (2, 3):
        rc, msg = call(model=plain._h, opt=ManyOptions(objective, 0, 100))
        assert rc == E_ARG and "objective" in msg
    for opt in (ok, ManyOptions(1, 0, 100), ManyOptions(2, 0, 100)):
        rc, msg = call(opt=opt)
        assert rc == E_STATE and "finalized" in msg
    assert call(count=0)[0] == E_STATE
    # the checkpointed entries: the same head, and a pool cannot be made for a model that is not finalized
    slots = np.zeros(2, dtype=np.int32)
    rc = L.csgpu_solve_many_clauses_wide_checkpointed(m._h, rows.ctypes.data, 2, C.byref(ok), res.ctypes.data, None, None, None,
                                                      slots.ctypes.data, None)
    assert rc == E_STATE
    rc = L.csgpu_solve_many_clauses_wide_resume(m._h, 2, C.byref(ManyOptions(0, 0, -1)), res.ctypes.data, None, None, None,
                                                slots.ctypes.data, None)
    assert rc == E_ARG
    pool = C.c_void_p()
    assert L.csgpu_many_clause_wide_checkpoints_create(m._h, 4, C.byref(pool)) == E_STATE
    assert L.csgpu_many_clause_wide_checkpoints_create(m._h, 0, C.byref(pool)) == E_ARG
    assert L.csgpu_many_clause_wide_checkpoint_bytes(None) == 0 and L.csgpu_model_qualifies_many_clauses_wide(None) == 0
    # the Python method: max_nodes is required; a numpy batch on a model that is not finalized gets the library's error
    with pytest.raises(TypeError):
        m.solve_many_clauses_wide(rows)
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses_wide(rows, "MIN", max_nodes=10)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses_wide(rows, "MAX", max_nodes=10)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError) as e:
        m.many_clauses_wide_kernel()
    assert e.value.code == E_STATE


def test_sudoku_less_is_the_empty_sudoku_and_true_inequalities():
    box, seed, pairs = wide.SUDOKU
    text = problems.sudoku_less(box, seed, pairs)
    empty, _ = problems.sudoku_roots(box, 0.0, [])
    body = [line for line in text.split("\n") if line and not line.startswith("#")]
    base = [line for line in empty.split("\n") if line and not line.startswith("#")]
    assert body[:len(base)] == base and len(body) == len(base) + pairs
    grid = problems.sudoku_solution(box, seed)
    seen = set()
    for line in body[len(base):]:
        a, op, b = line.rstrip(";").split()
        (ra, ca), (rb, cb) = (tuple(int(x) for x in name[1:].split("_")) for name in (a, b))
        assert op == "<" and ra == rb and abs(ca - cb) == 1 and grid[ra][ca] < grid[rb][cb]
        seen.add((ra, min(ca, cb)))
    assert len(seen) == pairs
    assert problems.sudoku_less(box, seed, pairs) == text and problems.sudoku_less(box, seed + 1, pairs) != text
    assert problems.sudoku_less(box, seed, pairs, "ALL").split("\n")[1] == "ALL;"
    # the inequalities narrow the root domains, the rows lie inside them and hold the grid
    _, dom = W.oracle_for(text)
    assert ((dom[:, 1] - dom[:, 0]) < box * box - 1).any() and dom.min() == 1 and dom.max() == box * box
    loose = problems.sudoku_less_roots(box, seed, pairs, wide.SHARES)[1]
    rows = problems.sudoku_less_roots(box, seed, pairs, wide.SHARES, dom=dom)[1]
    flat = np.array(grid).reshape(-1)
    assert rows.shape == (12, 81, 2) and rows.dtype == np.int32
    assert ((rows[:, :, 0] >= dom[:, 0]) & (rows[:, :, 1] <= dom[:, 1])).all()
    assert ((rows[:, :, 0] <= flat) & (flat <= rows[:, :, 1])).all()
    assert not ((loose[:, :, 0] >= dom[:, 0]) & (loose[:, :, 1] <= dom[:, 1])).all()  # 1 .. 9 lies outside them: BAD_ROOT
    revealed = (rows[:, :, 0] == rows[:, :, 1]).sum(1) / 81
    assert revealed.min() >= 0.14 and revealed.max() <= 0.41
    assert [int(round(s * 81)) for s in wide.SHARES] == [int(((loose[k, :, 0] == loose[k, :, 1])).sum()) for k in range(12)]


def test_the_sudoku_less_rows_hold_every_outcome_class():
    """what the GPU test relies on (if a class is lost, the rows change, not this condition): under ANY a DONE row with a
    solution, a LIMIT row and an inconsistent row without a node; under ALL a LIMIT row; LIMIT means exactly max_nodes"""
    text, rows = wide.sudoku_less()
    _, dom = W.oracle_for(text)
    assert len(rows) == 12 and W.model_of(text).n_clauses == 1159
    grid = np.array(problems.sudoku_solution(*wide.SUDOKU[:2])).reshape(-1)
    for k in range(12):  # a moved given is another value of its root domain; no other row leaves the grid
        off = [v for v in range(81) if not rows[k, v, 0] <= grid[v] <= rows[k, v, 1]]
        assert len(off) == (1 if k in wide.MOVED else 0)
        assert all(dom[v, 0] <= rows[k, v, 0] == rows[k, v, 1] <= dom[v, 1] for v in off)
    a = wide.walked("sudoku_less_any")
    done = (a["status"] == W.DONE) & (a["solutions"] == 1)
    limit = a["status"] == W.LIMIT
    dead = (a["status"] == W.DONE) & (a["solutions"] == 0) & (a["nodes"] == 0)
    assert done.any() and limit.any() and dead.any()
    assert (a["nodes"][limit] == 400).all() and (a["nodes"][~limit] < 400).all()
    assert a["nodes"][done].min() >= 1 and (a["status"] != W.BAD_ROOT).all()
    b = wide.walked("sudoku_less_all")
    limit = b["status"] == W.LIMIT
    assert limit.sum() >= 2 and (b["nodes"][limit] == 400).all()
    assert (b["solutions"][limit] > 1).any() and ((b["status"] == W.DONE) & (b["solutions"] > 1)).any()


def test_the_schedule32_rows_stop_and_finish_with_an_incumbent():
    text, rows = wide.schedule32()
    assert W.model_of(text).n_clauses == 657 and (rows[0] == W.oracle_for(text)[1]).all()
    res = wide.walked("schedule32_min")
    assert res["status"][0] == W.LIMIT and res["nodes"][0] == 200 and res["solutions"][0] == 1 and res["best"][0] == 114
    done, limit = res["status"] == W.DONE, res["status"] == W.LIMIT
    assert (done & (res["solutions"] > 0)).any() and (limit & (res["solutions"] > 0)).any()
    assert (res["best"][done] == 114).all() and (res["nodes"][done] < 200).all()


def test_the_tree_model_is_past_512_clauses_with_trees_and_its_rows_finish_and_stop():
    for name in ("tree630_all", "tree630_max"):
        text, rows, objective, budget = wide.build(name)
        m = wide.host_model(text)
        assert m.n_clauses > 512 and m.device_info()["tree_clauses"] > 0
        assert m.qualifies_many_clauses_wide() and not m.qualifies_many_clauses()
        res = wide.walked(name)
        assert len(rows) == 8 and (res["solutions"] > 0).all()
        assert (res["status"] == W.LIMIT).any() and (res["nodes"][res["status"] == W.LIMIT] == budget).all()
    res = wide.walked("tree630_max")
    assert (res["status"] == W.DONE).any() and (res["solutions"] > 1).any()  # some incumbent is improved on


def test_slices_of_the_host_walk_add_up_past_512_clauses():
    """the reference the GPU slices are held to: a walk in slices is the walk with the summed budget"""
    for name in ("sudoku_less_all", "schedule32_min"):
        text, rows, objective, budget = wide.build(name)
        for row in rows[:4]:
            w, part = W.Walk(text, row, objective), None
            for piece in (1, 7, budget - 8):
                part = w.run(piece)
            ref = W.walk(text, row, objective, budget)
            assert {k: v for k, v in part.items() if k != "first"} == {k: v for k, v in ref.items() if k != "first"}


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


def test_the_shipped_wide_kernels_are_two_each_and_the_old_ones_are_untouched():
    assert shipped("cs_walk_wide") == {"cs_walk_wide<true>", "cs_walk_wide<false>"}
    assert shipped("cs_walk_wide_resume") == {"cs_walk_wide_resume<true>", "cs_walk_wide_resume<false>"}
    assert shipped("cs_walk_clauses") == {s[3] for s in sets.SETS.values()}
