"""CPU tests of csgpu_solve_many_clauses_restarts / Model.solve_many_clauses_restarts (the ANY walk of solve_many_clauses
with a seeded rotation of every node's value order and Luby restarts): the interface is declared, exported and
prototyped; the argument errors that need no device, in their documented order; the host walk of
tests/many_walk_clauses_restarts.py against the walk it is derived from (tests/many_walk_objective.py); every figure that
tests/many_clause_restart_sets.py records about its sets, so that no GPU test passes vacuously; what restarts buy on the
tail of three schedule workloads, and the default base that follows from it; the shipped cs_walk_restart instantiations."""
import ctypes as C
import inspect
import re
import subprocess

import numpy as np
import pytest

import many_clause_restart_sets as rsets
import many_walk
import many_walk_clauses_restarts as R
import many_walk_objective as W
from csolve_amd import problems

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
FIELDS = many_walk.FIELDS
DONE, LIMIT, BAD_ROOT = many_walk.DONE, many_walk.LIMIT, many_walk.BAD_ROOT
EIGHT = {f"cs_walk_restart<{cpl}, {tree}>" for cpl in (1, 2, 4, 8) for tree in ("true", "false")}


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    L = _lib.load_library()
    name = "csgpu_solve_many_clauses_restarts"
    assert name in _lib.declared_symbols()
    assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 9
    internal = "csgpu_internal_many_clauses_restart_symbol"  # exported and prototyped, declared in cs_internal.h only
    assert internal not in _lib.declared_symbols() and len(getattr(L, internal).argtypes) == 3
    # the options are the struct that was there, and the calls of both families are what they were
    assert C.sizeof(_lib.ManyRestartOptions) == 24 and C.sizeof(_lib.ManyResult) == 40
    assert len(L.csgpu_solve_many_restarts.argtypes) == 9 and len(L.csgpu_solve_many_clauses.argtypes) == 8
    assert len(L.csgpu_solve_many_clauses_upto.argtypes) == 7 and len(L.csgpu_solve_many_clauses_resume.argtypes) == 9
    for method in ("solve_many_clauses_restarts", "many_clauses_restart_kernel", "solve_many_restarts", "solve_many_clauses"):
        assert callable(getattr(Model, method)), method
    sig = inspect.signature(Model.solve_many_clauses_restarts)
    assert sig.parameters["restart_base"].default == rsets.DEFAULT_BASE
    assert inspect.signature(Model.solve_many_restarts).parameters["restart_base"].default == 32
    assert not any("walk" in f or "many" in f or "restart" in f for f in _lib.PLAN_FAMILIES) and len(_lib.PLAN_FAMILIES) == 16
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert text.index("csgpu_solve_many_clauses_upto_resume") < text.index(name)  # the declaration comes after the up-to-k block


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyRestartOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(problems.schedule(5, 1))  # parsed, not finalized
    n = m.n_vars
    rows = np.zeros((2, n, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    seeds = np.zeros(2, dtype=np.uint32)
    restarts = np.full(2, -9, dtype=np.int32)
    ok = ManyRestartOptions(100, 8, 1, 0)

    def call(model=m._h, roots=rows.ctypes.data, sd=seeds.ctypes.data, count=2, opt=ok, results=res.ctypes.data):
        rc = L.csgpu_solve_many_clauses_restarts(model, roots, sd, count, C.byref(opt) if opt is not None else None, results,
                                                 None, restarts.ctypes.data, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    assert call(model=None)[0] == E_ARG
    assert call(roots=None)[0] == E_ARG
    assert call(results=None)[0] == E_ARG
    assert call(opt=None)[0] == E_ARG
    assert call(count=-1)[0] == E_ARG
    assert call(opt=ManyRestartOptions(0, 8, 1, 0))[0] == E_ARG
    assert call(opt=ManyRestartOptions(-5, 8, 1, 0))[0] == E_ARG
    rc, msg = call(opt=ManyRestartOptions(100, -1, 1, 0))
    assert rc == E_ARG and "restart_base" in msg
    for flags in (2, 3, 4, -1, 1 << 30):
        rc, msg = call(opt=ManyRestartOptions(100, 8, 1, flags))
        assert rc == E_ARG and "flags" in msg, flags
    # the order: the count before the budget, the budget before the base, the base before the flags, all of them before
    # the model's state
    assert "count" in call(count=-1, opt=ManyRestartOptions(0, -1, 1, 2))[1]
    assert "max_nodes" in call(opt=ManyRestartOptions(0, -1, 1, 2))[1]
    assert "restart_base" in call(opt=ManyRestartOptions(100, -1, 1, 2))[1]
    for good in (ok, ManyRestartOptions(100, 0, 0, 0), ManyRestartOptions(100, 0, 7, 1), ManyRestartOptions(1, 1 << 40, 7, 1)):
        rc, msg = call(opt=good)
        assert rc == E_STATE and "finalized" in msg
    assert call(sd=None)[0] == E_STATE  # no seeds is no error
    assert call(count=0)[0] == E_STATE  # an empty batch is no way round the state check
    assert (res == 0).all() and (restarts == -9).all()
    # the Python method: max_nodes is required, and a numpy batch on a model that is not finalized gets the library's
    # error (nothing is uploaded for it)
    with pytest.raises(TypeError):
        m.solve_many_clauses_restarts(rows)
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses_restarts(rows, max_nodes=10)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses_restarts(rows, max_nodes=10, restart_base=-1)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses_restarts(rows, max_nodes=0)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError) as e:
        m.many_clauses_restart_kernel()
    assert e.value.code == E_STATE


_ascending = {}


def _plain(name):
    """many_walk_objective.walk under ANY of every row of a set with a budget of 20,000 nodes, computed once"""
    if name not in _ascending:
        text, roots, _ = rsets.build(name)
        _ascending[name] = [W.walk(text, row, "ANY", 20000) for row in roots]
    return _ascending[name]


def _is_a_solution(text, row):
    from oracle.cs_oracle import Model as OModel, Oracle
    om = OModel.parse(text)
    om.set_domains(np.stack([row, row], 1).astype(np.int32))
    om.index()
    return Oracle(om).eval(om.root) == (1, 1)


@pytest.mark.parametrize("name", sorted(rsets.SETS))
def test_base_0_without_flags_is_the_existing_walk(name):
    text, roots, _ = rsets.build(name)
    budget = rsets.SETS[name][3]
    for i, row in enumerate(roots):
        want = W.walk(text, row, "ANY", budget)
        got = R.walk_restarts(text, row, 0, 12345 + i, max_nodes=budget)
        for f in FIELDS:
            assert got[f] == want[f], (name, i, f)
        assert got["restarts"] == 0
        assert (got["first"] is None) == (want["first"] is None)
        if want["first"] is not None:
            assert (got["first"] == want["first"]).all(), (name, i)
        if want["nodes"] > 5:  # and so is a budget below the walk
            part, ref = R.walk_restarts(text, row, 0, 1, max_nodes=5), W.walk(text, row, "ANY", 5)
            assert all(part[f] == ref[f] for f in FIELDS) and part["status"] == LIMIT


@pytest.mark.parametrize("name", sorted(rsets.SETS))
def test_restarts_change_the_walk_and_not_the_verdict(name):
    text, roots, _ = rsets.build(name)
    plain = _plain(name)
    evaluated = 0
    for base in rsets.SETS[name][1]:
        res = rsets.walk(name, base)
        decided = 0
        for i, want in enumerate(plain):
            assert res["root_props"][i] == want["root_props"]
            if want["status"] == LIMIT:  # the tail: the ascending walk is still at it after 20,000 nodes, and the row is
                assert res["status"][i] == DONE and res["solutions"][i] == 1  # solved all the same (checked below)
            else:
                assert res["status"][i] == want["status"] and res["solutions"][i] == want["solutions"], (name, base, i)
                decided += 1
            if res["restarts"][i] == 0:  # the first run ended before its first restart: the existing walk, field for field
                assert all(res[f][i] == want[f] for f in FIELDS), (name, base, i)
                if want["first"] is not None:
                    assert (res["first"][i] == want["first"]).all()
            if res["solutions"][i]:
                sol = res["first"][i]
                assert ((sol >= roots[i][:, 0]) & (sol <= roots[i][:, 1])).all(), (name, base, i)
                assert _is_a_solution(text, sol), (name, base, i)
                evaluated += 1
            else:
                assert (res["first"][i] == 0).all()
        assert (res["restarts"] > 0).any(), "a set without a restart tests nothing new"
        assert 2 * decided >= len(plain), "the ascending walk must decide most rows"
        assert (res["cuts"] <= res["nodes"]).all()
    if name == "schedule5_unsat":  # no row has a solution, and half of them are proven so only through restarts
        for base, most in ((1, 510), (2, 254)):
            res = rsets.walk(name, base)
            assert (res["solutions"] == 0).all() and len(roots) == 32
            assert int((res["status"] == BAD_ROOT).sum()) == 5 and int(((res["status"] == DONE) & (res["nodes"] == 0)).sum()) == 10
            assert int((res["restarts"] > 0).sum()) == 16 and int(res["restarts"].max()) == most
    else:
        assert evaluated >= 5


def test_the_answer_depends_on_row_seed_and_options_only():
    text, roots, _ = rsets.build("schedule6")
    a = R.walk_many_restarts(text, roots[:8], 1, seeds=np.arange(8) + 5)
    for i in range(8):
        alone = R.walk_restarts(text, roots[i], 1, i + 5)
        assert all(a[f][i] == alone[f] for f in FIELDS + ("restarts",))
    assert (a["restarts"] > 0).any()
    # a seed is 32 bits
    i = int(np.argmax(a["restarts"]))
    x = R.walk_restarts(text, roots[i], 1, 7)
    y = R.walk_restarts(text, roots[i], 1, 7 + 2 ** 32)
    assert x["restarts"] > 0 and all(x[f] == y[f] for f in FIELDS + ("restarts",))
    # and the seed matters: some restarting row walks differently under another one
    assert any(R.walk_restarts(text, roots[i], 1, s)["nodes"] != x["nodes"] for s in (8, 9, 10, 11))


@pytest.mark.parametrize("name", sorted(rsets.SETS))
def test_the_set_conditions_hold(name):
    _, bases, seeds, budget, kernel, recorded = rsets.SETS[name]
    text, roots, _ = rsets.build(name)
    assert len(roots) <= 64 and budget <= 8192 and kernel in EIGHT
    assert seeds is None or len(seeds) == len(roots)
    assert sorted(recorded) == sorted(bases)
    for base in bases:
        res = rsets.walk(name, base)
        largest, restarted = recorded[base]
        print(f"{name}, base {base}: largest walk {int(res['nodes'].max())} nodes, {int((res['restarts'] > 0).sum())} of "
              f"{len(res['nodes'])} restarted, at most {int(res['restarts'].max())} times")
        assert 0 < largest < budget
        assert (res["status"] != LIMIT).all(), (name, base)
        assert (int(res["nodes"].max()), int((res["restarts"] > 0).sum())) == (largest, restarted), (name, base)


def test_every_instantiation_has_a_set_with_four_restarting_instances():
    best = {}
    for name, (_, bases, _, _, kernel, recorded) in rsets.SETS.items():
        best[kernel] = max([best.get(kernel, 0)] + [recorded[b][1] for b in bases])
    assert set(best) == EIGHT and min(best.values()) >= 4, best


@pytest.mark.parametrize("name", sorted(rsets.SETS))
def test_the_sets_name_the_instantiation_their_tables_plan(name):
    assert rsets.planned(rsets.build(name)[0]) == rsets.SETS[name][4]


def test_restarts_cut_the_tail_and_the_default_base_has_the_fewest_nodes():
    """what the feature is for, on the host: the table of DESIGN 3.10, recomputed"""
    total = {base: 0 for base in rsets.TAIL_BASES}
    for name, (_, _, _, recorded) in rsets.TAIL.items():
        for base in (0,) + rsets.TAIL_BASES:
            res = rsets.tail_walk(name, base)
            got = (int(res["nodes"].sum()), int(res["nodes"].max()), int((res["status"] == LIMIT).sum()))
            print(f"{name}, base {base}: {got[0]} nodes in all, deepest {got[1]}, {got[2]} at the budget")
            assert got == recorded[base], (name, base)
            if base:
                total[base] += got[0]
    print("nodes in all over the three workloads:", total)
    assert min(total, key=lambda b: (total[b], b)) == rsets.DEFAULT_BASE and total[rsets.DEFAULT_BASE] == 18639
    assert total[32] > 3 * total[rsets.DEFAULT_BASE]  # the default of solve_many_restarts is visibly too large here
    # schedule(10,1) at the default base against the ascending walk: every row is solved, and the deepest walk -- what a
    # launch's duration follows -- shrinks by more than 50 x
    plain, res = rsets.tail_walk("schedule10", 0), rsets.tail_walk("schedule10", rsets.DEFAULT_BASE)
    assert (int(plain["nodes"].sum()), int(plain["nodes"].max())) == (45183, 20000) and int((plain["status"] == LIMIT).sum()) == 1
    assert (int(res["nodes"].sum()), int(res["nodes"].max())) == (1980, 366)
    assert (res["status"] == DONE).all() and (res["solutions"] == 1).all()
    assert res["nodes"].max() * 50 <= plain["nodes"].max() and res["nodes"].sum() * 20 <= plain["nodes"].sum()
    solved = plain["status"] == DONE
    assert (res["solutions"][solved] == plain["solutions"][solved]).all()


def shipped_walk_restart_kernels():
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == "cs_walk_restart" and "<" in name:
                shipped.add(name)
    return shipped


def test_shipped_restart_kernels_are_the_eight_the_sets_name():
    from test_solve_many_clauses_host import shipped_walk_kernels
    shipped = shipped_walk_restart_kernels()
    assert shipped == EIGHT
    assert {s[4] for s in rsets.SETS.values()} == shipped
    assert len(shipped_walk_kernels()) == 8  # the old family is what it was
