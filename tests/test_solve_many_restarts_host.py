"""CPU tests of csgpu_solve_many_restarts / Model.solve_many_restarts (the ANY walk of solve_many with a seeded rotation of
every node's value order and Luby restarts): the interface is declared, exported and prototyped; the argument errors
that need no device; csgpu_many_value against the restatement of its definition in tests/many_walk_restarts.py; that
host walk against the walk it is derived from (tests/many_walk.py); what restarts buy on the tail set; the budgets of the
GPU sets; the shipped cs_dive_restart instantiations."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import many_restart_sets
import many_walk
import many_walk_restarts
from conftest import golden
from csolve_amd import problems

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
FIELDS = many_walk_restarts.FIELDS
DONE = many_walk.DONE


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = _lib.load_library()
    for name, args in {"csgpu_solve_many_restarts": 9, "csgpu_many_value": 6}.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
    assert hasattr(L, "csgpu_internal_many_restart_symbol") and len(L.csgpu_internal_many_restart_symbol.argtypes) == 3
    assert re.search(r"#define\s+CSGPU_MANY_ROTATE_FIRST\s+1\b", text) and _lib.MANY_ROTATE_FIRST == 1
    opt = re.search(r"typedef struct csgpu_many_restart_options \{(.*?)\} csgpu_many_restart_options;", text, flags=re.S).group(1)
    assert re.findall(r"\w+(?=[,;])", opt) == [f for f, _ in _lib.ManyRestartOptions._fields_] == ["max_nodes", "restart_base", "seed", "flags"]
    assert C.sizeof(_lib.ManyRestartOptions) == 24
    assert [_lib.ManyRestartOptions.max_nodes.offset, _lib.ManyRestartOptions.restart_base.offset,
            _lib.ManyRestartOptions.seed.offset, _lib.ManyRestartOptions.flags.offset] == [0, 8, 16, 20]
    # the declaration comes after the up-to-k block
    assert text.index("csgpu_solve_many_upto_resume") < text.index("csgpu_many_restart_options")
    # the old calls, their records and their options are what they were
    assert len(L.csgpu_solve_many.argtypes) == 7 and len(L.csgpu_solve_many_checkpointed.argtypes) == 9
    assert len(L.csgpu_solve_many_resume.argtypes) == 8
    assert len(L.csgpu_solve_many_upto.argtypes) == 7 and len(L.csgpu_solve_many_upto_checkpointed.argtypes) == 9
    assert len(L.csgpu_solve_many_upto_resume.argtypes) == 8
    assert C.sizeof(_lib.ManyResult) == 40 and C.sizeof(_lib.ManyOptions) == 16 and C.sizeof(_lib.ManyUptoOptions) == 16
    assert [f for f, _ in _lib.ManyOptions._fields_] == ["objective", "reserved", "max_nodes"]
    assert [f for f, _ in _lib.ManyUptoOptions._fields_] == ["max_solutions", "reserved", "max_nodes"]
    for method in ("solve_many_restarts", "many_restart_kernel", "solve_many", "solve_many_upto", "classify_many"):
        assert callable(getattr(Model, method)), method
    assert not any("dive" in f or "many" in f or "restart" in f for f in _lib.PLAN_FAMILIES) and len(_lib.PLAN_FAMILIES) == 16


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyRestartOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(open(golden("problems", "queens8.txt")).read())  # parsed, not finalized
    rows = np.zeros((2, 8, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    seeds = np.zeros(2, dtype=np.uint32)
    restarts = np.full(2, -9, dtype=np.int32)
    ok = ManyRestartOptions(100, 8, 1, 0)

    def call(model=m._h, roots=rows.ctypes.data, sd=seeds.ctypes.data, count=2, opt=ok, results=res.ctypes.data):
        rc = L.csgpu_solve_many_restarts(model, roots, sd, count, C.byref(opt) if opt is not None else None, results, None,
                                         restarts.ctypes.data, None)
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
        m.solve_many_restarts(rows)
    with pytest.raises(CsolveError) as e:
        m.solve_many_restarts(rows, max_nodes=10)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.solve_many_restarts(rows, max_nodes=10, restart_base=-1)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError) as e:
        m.solve_many_restarts(rows, max_nodes=0)
    assert e.value.code == E_ARG


def test_many_value_is_the_restated_definition():
    from csolve_amd import _lib
    L = _lib.load_library()
    checked = 0
    for seed in (0, 1, 12345, 2 ** 32 - 1):
        for run in range(6):
            for var in (0, 1, 63, 64, 255):
                for width in (1, 2, 3, 9, 16, 255, 256):
                    for lo in (1, -7):
                        hi = lo + width - 1
                        for flags in (0, 1):
                            got = [L.csgpu_many_value(seed, run, var, _lib.Val(lo, hi), j, flags) for j in range(width)]
                            want = [many_walk_restarts.value(seed, run, var, lo, hi, j, flags) for j in range(width)]
                            assert got == want, (seed, run, var, width, lo, flags)
                            assert sorted(got) == list(range(lo, hi + 1)), "a permutation of [lo, hi]"
                            if run == 0 and flags == 0:
                                assert got == list(range(lo, hi + 1)), "run 0 is ascending"
                            # a rotation: one start, then ascending with one wrap
                            assert all((b - a) in (1, 1 - width) for a, b in zip(got, got[1:]))
                            checked += 1
    assert checked == 4 * 6 * 5 * 7 * 2 * 2
    # the rotation depends on the seed, the run and the variable
    starts = {(s, r, v): L.csgpu_many_value(s, r, v, _lib.Val(1, 256), 0, 1) for s in (1, 2) for r in (0, 1) for v in (0, 1)}
    assert len(set(starts.values())) >= 6
    # pinned values of the definition, worked out by hand from fmix32: seed 0, run 1, variable 0
    key = many_walk_restarts.fmix32(0 ^ many_walk_restarts.fmix32(0x9E3779B1 + 1))
    assert L.csgpu_many_value(0, 1, 0, _lib.Val(0, 255), 0, 0) == key >> 24
    assert many_walk_restarts.fmix32(0) == 0 and many_walk_restarts.fmix32(1) == 0x514E28B7  # murmur3's finalizer


def test_luby_next_is_what_the_helper_restates():
    from csolve_amd import _lib
    L = _lib.load_library()
    t, c = C.c_uint64(1), C.c_uint64(1)
    th, cn, seq = 1, 1, []
    for _ in range(64):
        assert (t.value, c.value) == (th, cn)
        seq.append(th)
        L.csgpu_luby_next(C.byref(t), C.byref(c))
        th, cn = many_walk_restarts.luby_next(th, cn)
    assert seq[:15] == [1, 1, 2, 1, 1, 2, 4, 1, 1, 2, 1, 1, 2, 4, 8]


def _is_a_solution(text, row):
    from oracle.cs_oracle import Model as OModel, Oracle
    om = OModel.parse(text)
    om.set_domains(np.stack([row, row], 1).astype(np.int32))
    om.index()
    return Oracle(om).eval(om.root) == (1, 1)


_ascending = {}


def _plain(name):
    """many_walk.dive under ANY of every row of a set, computed once"""
    if name not in _ascending:
        text, roots, _ = many_restart_sets.build(name)
        _ascending[name] = [many_walk.dive(text, row, "ANY") for row in roots]
    return _ascending[name]


@pytest.mark.parametrize("name", sorted(many_restart_sets.SETS))
def test_base_0_without_flags_is_the_existing_walk(name):
    text, roots, seeds = many_restart_sets.build(name)
    for i, (row, want) in enumerate(zip(roots, _plain(name))):
        if i > 0 and seeds is not None:
            break  # one row, 24 times
        got = many_walk_restarts.dive_restarts(text, row, 0, 12345 if seeds is None else int(seeds[i]))
        for f in FIELDS:
            assert got[f] == want[f], (name, i, f)
        assert got["restarts"] == 0
        assert (got["first"] is None) == (want["first"] is None)
        if want["first"] is not None:
            assert (got["first"] == want["first"]).all(), (name, i)
        # and so is a budget below the walk
        if want["nodes"] > 5:
            part, ref = many_walk_restarts.dive_restarts(text, row, 0, 1, max_nodes=5), many_walk.dive(text, row, "ANY", 5)
            assert all(part[f] == ref[f] for f in FIELDS) and part["status"] == many_walk.LIMIT


@pytest.mark.parametrize("name", sorted(many_restart_sets.SETS))
def test_restarts_change_the_walk_and_not_the_verdict(name):
    text, roots, seeds = many_restart_sets.build(name)
    plain = _plain(name)
    evaluated = 0
    for base in many_restart_sets.SETS[name][1]:
        res = many_restart_sets.walk(name, base)
        for i, want in enumerate(plain):
            assert res["status"][i] == want["status"] == DONE and res["solutions"][i] == want["solutions"], (name, base, i)
            assert res["root_props"][i] == want["root_props"]
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
        assert (res["cuts"] <= res["nodes"]).all()
    assert evaluated >= 5
    if name == "queens12_two":  # the rows without a solution are proven so (all twelve at the root node: no node)
        res = many_restart_sets.walk(name, 8)
        none = res["solutions"] == 0
        assert none.sum() == 12 and (res["status"][none] == DONE).all() and (res["nodes"][none] == 0).all()
    if name == "queens12_four":  # and here one of them after restarts: thresholds grow, the last run walks the whole tree
        res = many_restart_sets.walk(name, 1)
        none = res["solutions"] == 0
        assert none.sum() == 27 and (res["status"][none] == DONE).all() and (res["restarts"][none] > 0).any()
        assert res["restarts"][none].max() == 62 and res["nodes"][none].max() == 374
    if seeds is not None:  # one row under 24 seeds: every instance restarts, the seeds lead to different solutions
        res = many_restart_sets.walk(name, 1)
        assert (res["restarts"] > 0).all() and (res["solutions"] == 1).all()
        assert len({r.tobytes() for r in res["first"]}) >= 23


def test_the_answer_depends_on_row_seed_and_options_only():
    text, roots, _ = many_restart_sets.build("sudoku9")
    a = many_walk_restarts.dive_many_restarts(text, roots[:8], 1, seeds=np.arange(8) + 5)
    for i in range(8):
        alone = many_walk_restarts.dive_restarts(text, roots[i], 1, i + 5)
        assert all(a[f][i] == alone[f] for f in FIELDS + ("restarts",))
    # a seed is 32 bits
    x = many_walk_restarts.dive_restarts(text, roots[1], 1, 7)
    y = many_walk_restarts.dive_restarts(text, roots[1], 1, 7 + 2 ** 32)
    assert all(x[f] == y[f] for f in FIELDS + ("restarts",))


def test_restarts_cut_the_tail():
    """what the feature is for, on the host: 512 9x9 sudokus with 30 % givens, base 32"""
    _, base, _, recorded = many_restart_sets.TAIL
    text, roots, _ = many_restart_sets.build("tail")
    plain = many_walk.dive_many(text, roots, "ANY")
    res = many_restart_sets.walk("tail", base)
    print(f"tail: ascending walk {int(plain['nodes'].sum())} nodes, largest {int(plain['nodes'].max())}; restarts base {base}: "
          f"{int(res['nodes'].sum())} nodes, largest {int(res['nodes'].max())}, {int((res['restarts'] > 0).sum())} restarted")
    assert (plain["status"] == DONE).all() and (res["status"] == DONE).all()
    assert (res["solutions"] == plain["solutions"]).all()
    assert (int(plain["nodes"].sum()), int(plain["nodes"].max())) == recorded["ascending"]
    assert (int(res["nodes"].sum()), int(res["nodes"].max())) == recorded["restarts"]
    assert int((res["restarts"] > 0).sum()) == recorded["restarted"]
    assert res["nodes"].max() * 4 <= plain["nodes"].max()
    assert res["nodes"].sum() < plain["nodes"].sum()


def test_rotate_first_samples_distinct_solutions():
    base, seeds, budget, largest = many_restart_sets.SAMPLER
    text, roots, _ = many_restart_sets.build("sampler")
    res = many_restart_sets.walk("sampler", base, rotate_first=True)
    assert (res["status"] == DONE).all() and (res["solutions"] == 1).all()
    assert res["nodes"].max() == largest < budget
    assert len({r.tobytes() for r in res["first"]}) == 32
    for r in res["first"][::8]:
        assert _is_a_solution(text, r)
    # without the flag run 0 is the ascending walk whatever the seed: without restarts every seed finds the same grid
    plain = many_walk_restarts.dive_many_restarts(text, roots[:4], 0, seeds=seeds[:4])
    assert (plain["restarts"] == 0).all() and len({r.tobytes() for r in plain["first"]}) == 1


@pytest.mark.parametrize("name", sorted(many_restart_sets.SETS))
def test_no_row_of_a_gpu_set_reaches_its_budget(name):
    _, bases, _, budget, _, recorded = many_restart_sets.SETS[name]
    for base in bases:
        res = many_restart_sets.walk(name, base)
        largest, restarted = recorded[base]
        print(f"{name}, base {base}: largest walk {int(res['nodes'].max())} nodes, {int((res['restarts'] > 0).sum())} of "
              f"{len(res['nodes'])} restarted, at most {int(res['restarts'].max())} times")
        assert 0 < largest < budget
        assert (res["status"] == DONE).all(), (name, base)
        assert (int(res["nodes"].max()), int((res["restarts"] > 0).sum())) == (largest, restarted), (name, base)


def shipped_restart_kernels():
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == "cs_dive_restart" and "<" in name:
                shipped.add(name)
    return shipped


def test_shipped_restart_kernels_are_the_six_the_sets_name():
    from test_many_resume_host import shipped_resume_kernels
    from test_solve_many_host import shipped_dive_kernels
    from test_solve_many_upto_host import shipped_upto_kernels
    shipped = shipped_restart_kernels()
    assert len(shipped) == 6
    for name in shipped:
        assert re.fullmatch(r"cs_dive_restart<unsigned (char|short), ([124])>", name), name
    assert {s[4] for s in many_restart_sets.SETS.values()} == shipped
    # the old families are what they were
    assert len(shipped_dive_kernels()) == 6 and len(shipped_resume_kernels()) == 6 and len(shipped_upto_kernels()) == 6
