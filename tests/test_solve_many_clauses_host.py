"""CPU tests of csgpu_solve_many_clauses / Model.solve_many_clauses: the interface is declared, exported and prototyped;
the argument errors that need no device; the host walk the GPU tests compare with (tests/many_walk_objective.py) against
known optima, against many_walk on a != network and against itself in slices; the instance sets; the shipped
cs_walk_clauses instantiations."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

import many_clause_sets as sets
import many_walk
import many_walk_objective as W
from conftest import golden
from csolve_amd import problems

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
EIGHT = {f"cs_walk_clauses<{cpl}, {tree}>" for cpl in (1, 2, 4, 8) for tree in ("true", "false")}


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    for name in ("csgpu_solve_many_clauses", "csgpu_model_qualifies_many_clauses"):
        assert name in _lib.declared_symbols(), name
    L = _lib.load_library()
    assert len(L.csgpu_solve_many_clauses.argtypes) == 8
    assert len(L.csgpu_internal_many_clauses_symbol.argtypes) == 3
    for method in ("solve_many_clauses", "qualifies_many_clauses", "many_clauses_kernel"):
        assert callable(getattr(Model, method)), method
    assert not any("walk" in f or "many" in f for f in _lib.PLAN_FAMILIES)  # the plan dictionary stays what it is
    header = open(_lib.HEADER_PATH).read()
    for phrase in ("ties to the lowest index", "private incumbent", "max_nodes is compared before a child is tried"):
        assert phrase in header, phrase


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
    ok = ManyOptions(0, 0, 100)

    def call(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data):
        rc = L.csgpu_solve_many_clauses(model, roots, count, C.byref(opt) if opt is not None else None, results, None, None, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    assert call(model=None)[0] == E_ARG
    assert call(roots=None)[0] == E_ARG
    assert call(results=None)[0] == E_ARG
    assert call(opt=None)[0] == E_ARG
    assert call(count=-1)[0] == E_ARG
    assert call(opt=ManyOptions(0, 0, 0))[0] == E_ARG
    assert call(opt=ManyOptions(2, 0, -5))[0] == E_ARG
    assert call(opt=ManyOptions(7, 0, 100))[0] == E_ARG
    assert call(opt=ManyOptions(-1, 0, 100))[0] == E_ARG
    rc, msg = call(opt=ManyOptions(3, 0, 100))  # MAX on a MIN model
    assert rc == E_ARG and "MIN" in msg and "MAX" in msg
    for objective in (2, 3):  # MIN / MAX on a model without an objective
        rc, msg = call(model=plain._h, opt=ManyOptions(objective, 0, 100))
        assert rc == E_ARG and "objective" in msg
    for opt in (ok, ManyOptions(1, 0, 100), ManyOptions(2, 0, 100)):  # well-formed: the state is what is wrong
        rc, msg = call(opt=opt)
        assert rc == E_STATE and "finalized" in msg
    assert call(count=0)[0] == E_STATE  # an empty batch is no way round the state check
    assert call(model=plain._h, opt=ManyOptions(1, 0, 100))[0] == E_STATE
    # the existing entry keeps refusing MIN / MAX as a limit of the call
    rc = L.csgpu_solve_many(m._h, rows.ctypes.data, 2, C.byref(ManyOptions(2, 0, 100)), res.ctypes.data, None, None)
    assert rc == E_LIMIT
    # the Python method: max_nodes is required; a numpy batch on a model that is not finalized, or with the wrong sense,
    # gets the library's error and nothing is uploaded for it
    assert not m.qualifies_many_clauses()
    with pytest.raises(TypeError):
        m.solve_many_clauses(rows)
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses(rows, "MIN", max_nodes=10)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses(rows, "MAX", max_nodes=10)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError) as e:
        m.many_clauses_kernel()
    assert e.value.code == E_STATE


def _deadline(text, slack):
    """the root domains with an upper bound on the objective's variables: at most `slack` values above their lower bounds
    (the walk tries every value of "<obj>" above the incumbent as one more cut child, so an instance states a deadline)"""
    _, dom = W.oracle_for(text)
    row = dom.copy()
    wide = (row[:, 1].astype(np.int64) - row[:, 0]) > 1 << 20
    assert wide.any()
    row[wide, 1] = row[wide, 0] + slack
    return row


@pytest.mark.parametrize("name,make,optimum", [
    ("schedule6_s1", lambda: problems.schedule(6, 1), 22),
    ("ref_schedule", lambda: open(golden("problems", "ref_schedule.txt")).read(), 11)])
def test_the_min_walk_proves_the_known_optimum(name, make, optimum):
    """on the instance "the root domains, finished by a deadline 45 above the lower bound of the makespan" the walk ends
    DONE with the optimum the reference reports for the model (tests/golden/solve_stats.json) and the oracle's own search
    finds on that instance; the stored row has that makespan"""
    from oracle.cs_oracle import Model as OModel, Oracle
    text = make()
    recorded = [r["best"] for r in json.load(open(golden("solve_stats.json"))) if r["problem"] == name and r["solutions"] > 0]
    assert recorded and set(recorded) == {optimum}
    row = _deadline(text, 45)
    out = W.walk(text, row, "MIN", 1 << 20)
    om = OModel.parse(text)
    om.set_domains(row)
    om.index()
    assert Oracle(om).solve()["best"] == optimum
    assert out["status"] == W.DONE and out["best"] == optimum and out["solutions"] >= 1
    assert out["first"][W.model_of(text).view.obj_var] == optimum
    assert 0 < out["cuts"] < out["nodes"] < 20000
    # every budget below the tree's size stops there, with an incumbent no better than the optimum
    for budget in (1, 50, out["nodes"] - 1):
        part = W.walk(text, row, "MIN", budget)
        assert part["status"] == W.LIMIT and part["nodes"] == budget
        assert part["best"] is None or part["best"] >= optimum
    assert W.walk(text, row, "MIN", out["nodes"])["status"] == W.DONE


@pytest.mark.parametrize("objective", ["ANY", "ALL"])
def test_any_and_all_are_the_walk_of_solve_many(objective):
    """on a kernel-7 network the walk is many_walk.dive, field for field and row for row"""
    import many_sets
    text = problems.queens(8, "ALL")
    _, dom = many_walk.oracle_for(text)
    rows = np.concatenate([dom[None], many_sets.queens_two(8, 6, 3)])
    for row in rows:
        for budget in (5, 1 << 40):
            want = many_walk.dive(text, row, objective, budget)
            got = W.walk(text, row, objective, budget)
            assert got["best"] is None
            for f in many_walk.FIELDS:
                assert got[f] == want[f], (f, budget)
            assert (got["first"] is None) == (want["first"] is None)
            assert got["first"] is None or (got["first"] == want["first"]).all()


@pytest.mark.parametrize("name", ["schedule5_min", "wcet_max", "linear20_all"])
def test_budget_slices_add_up(name):
    """a walk in slices is the walk with the summed budget: every counter, the incumbent and the stored row"""
    text, roots, objective, _ = sets.build(name)
    for row in roots[:6]:
        whole = W.walk(text, row, objective, 1 << 40)
        w, spent = W.Walk(text, row, objective), 0
        for budget in (1, 2, 7, 30, 1 << 40):
            part = w.run(budget)
            spent += budget
            ref = W.walk(text, row, objective, spent)
            assert {k: v for k, v in part.items() if k != "first"} == {k: v for k, v in ref.items() if k != "first"}
            assert (part["first"] is None) == (ref["first"] is None) and (part["first"] is None or (part["first"] == ref["first"]).all())
        assert part["status"] == W.DONE and part["nodes"] == whole["nodes"]


def test_the_sets_cover_every_objective_and_the_family():
    assert {sets.SETS[k][1] for k in sets.WHOLE} == {"ANY", "ALL", "MIN", "MAX"}
    assert {s[3] for s in sets.SETS.values()} == EIGHT
    assert [sets.SETS[k][1] for k in sets.BUDGET] == ["MIN", "MIN"] and all(sets.SETS[k][2] <= 4096 for k in sets.BUDGET)
    assert sets.build("schedule6_min_budget")[0] == problems.schedule(6, 1)


@pytest.mark.parametrize("name", sorted(sets.SETS))
def test_a_set_plans_the_instantiation_it_names(name):
    """from the host tables (the device half, Model.many_clauses_kernel(), is checked on the GPU); 257-512 clauses for the
    second budget set"""
    text = sets.build(name)[0]
    assert sets.planned(text) == sets.SETS[name][3]
    if name == "schedule22_min_budget":
        assert 257 <= W.model_of(text).n_clauses <= 512


@pytest.mark.parametrize("name", sets.WHOLE)
def test_every_instance_of_a_whole_set_ends_below_its_budget(name):
    text, roots, objective, budget = sets.build(name)
    res = sets.walked(name)
    assert len(roots) <= 64
    assert (res["status"] == W.DONE).all()
    assert 0 < res["nodes"].max() <= 20000 and res["nodes"].max() < budget
    assert (res["solutions"] > 0).any()
    if objective in ("MIN", "MAX"):
        assert (res["solutions"] > 1).any()  # some incumbent is improved on


@pytest.mark.parametrize("name", sets.BUDGET)
def test_some_instances_of_a_budget_set_stop_at_the_budget(name):
    text, roots, objective, budget = sets.build(name)
    res = sets.walked(name)
    limit = res["status"] == W.LIMIT
    assert limit.any() and not limit.all()
    assert (res["nodes"][limit] == budget).all() and (res["nodes"][~limit] < budget).all()
    assert (limit & (res["solutions"] > 0)).any()  # an anytime answer: stopped with an incumbent


def shipped_walk_kernels():
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == "cs_walk_clauses" and "<" in name:
                shipped.add(name)
    return shipped


def test_the_shipped_walk_kernels_are_exactly_the_eight():
    from test_host import FIXPOINT_FAMILIES
    assert "cs_walk_clauses" not in FIXPOINT_FAMILIES
    shipped = shipped_walk_kernels()
    for name in shipped:
        assert re.fullmatch(r"cs_walk_clauses<[1248], (true|false)>", name), name
    assert shipped == EIGHT == {s[3] for s in sets.SETS.values()}
