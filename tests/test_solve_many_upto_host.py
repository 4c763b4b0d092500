"""CPU tests of csgpu_solve_many_upto / Model.solve_many_upto (an instance stops at its k-th solution and keeps all k): the
interface is declared, exported and prototyped; the argument errors that need no device; the host walk the GPU tests
compare with (tests/many_walk_upto.py) against the walk it is derived from (tests/many_walk.py); the budgets of the GPU
sets; the shipped cs_dive_upto instantiations."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import many_sets
import many_upto_sets
import many_walk
import many_walk_upto
from conftest import golden
from csolve_amd import problems

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
FIELDS = many_walk_upto.FIELDS
NEW_CALLS = {"csgpu_solve_many_upto": 7, "csgpu_solve_many_upto_checkpointed": 9, "csgpu_solve_many_upto_resume": 8}


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = _lib.load_library()
    for name, args in NEW_CALLS.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
    assert hasattr(L, "csgpu_internal_many_upto_symbol") and len(L.csgpu_internal_many_upto_symbol.argtypes) == 3
    opt = re.search(r"typedef struct csgpu_many_upto_options \{(.*?)\} csgpu_many_upto_options;", text, flags=re.S).group(1)
    assert re.findall(r"\w+(?=[,;])", opt) == [f for f, _ in _lib.ManyUptoOptions._fields_] == ["max_solutions", "reserved", "max_nodes"]
    assert C.sizeof(_lib.ManyUptoOptions) == 16
    # the old calls, their records and their options are what they were
    assert len(L.csgpu_solve_many.argtypes) == 7 and len(L.csgpu_solve_many_checkpointed.argtypes) == 9
    assert len(L.csgpu_solve_many_resume.argtypes) == 8
    assert C.sizeof(_lib.ManyResult) == 40 and C.sizeof(_lib.ManyOptions) == 16
    assert [f for f, _ in _lib.ManyOptions._fields_] == ["objective", "reserved", "max_nodes"]
    for method in ("solve_many_upto", "classify_many", "many_upto_kernel", "resume_many", "solve_many_sliced"):
        assert callable(getattr(Model, method)), method
    assert not any("dive" in f or "many" in f or "upto" in f for f in _lib.PLAN_FAMILIES) and len(_lib.PLAN_FAMILIES) == 16


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyUptoOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(open(golden("problems", "queens8.txt")).read())  # parsed, not finalized
    rows = np.zeros((2, 8, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    slots = np.full(2, -1, dtype=np.int32)
    pool = C.create_string_buffer(64)  # stands for a pool: no call gets as far as looking into it
    ok = ManyUptoOptions(2, 0, 100)

    def plain(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data):
        rc = L.csgpu_solve_many_upto(model, roots, count, C.byref(opt) if opt is not None else None, results, None, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    def fresh(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data):
        rc = L.csgpu_solve_many_upto_checkpointed(model, roots, count, C.byref(opt) if opt is not None else None, results,
                                                  None, ck, sl, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    def resume(model=m._h, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data):
        rc = L.csgpu_solve_many_upto_resume(model, count, C.byref(opt) if opt is not None else None, results, None, ck, sl,
                                            None)
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
    for call in (fresh, resume):
        assert call(ck=None)[0] == E_ARG
        assert call(sl=None)[0] == E_ARG
    assert (res == 0).all() and (slots == -1).all()
    # the Python methods: max_nodes is required, and a numpy batch on a model that is not finalized gets the library's
    # error (nothing is uploaded for it)
    with pytest.raises(TypeError):
        m.solve_many_upto(rows, 2)
    with pytest.raises(CsolveError) as e:
        m.solve_many_upto(rows, 2, max_nodes=10)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.solve_many_upto(rows, 0, max_nodes=10)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError) as e:
        m.classify_many(rows, max_nodes=10)
    assert e.value.code == E_STATE
    with pytest.raises(ValueError, match="k-th solution"):
        m.solve_many_sliced(rows, "ALL", budgets=(4,), finish="search", max_solutions=2)


def test_no_device_means_loud_failure():
    """Without a HIP device a well-formed use fails with the library's error -- never a CPU search."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from csolve_amd import CsolveError
    from csolve_amd.solver import Model
    text, roots = problems.sudoku_roots(3, 0.4, [1, 2])
    m = Model.from_text(text)
    with pytest.raises(CsolveError):  # no root phase, no device tables
        m.finalize()
    with pytest.raises(CsolveError) as e:
        m.solve_many_upto(roots, 2, max_nodes=1000)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.classify_many(roots, max_nodes=1000)
    assert e.value.code == E_STATE


def _is_a_solution(text, row):
    from oracle.cs_oracle import Model as OModel, Oracle
    om = OModel.parse(text)
    om.set_domains(np.stack([row, row], 1).astype(np.int32))
    om.index()
    return Oracle(om).eval(om.root) == (1, 1)


@pytest.mark.parametrize("name", ["queens12_two", "sudoku9"])
def test_the_helper_is_the_existing_walk_with_another_stop(name):
    text, roots = many_upto_sets.build(name)
    if name == "queens12_two":  # the rows of the existing set, the first 24
        assert (roots == many_sets.build("queens12_two")[1][:24]).all()
    several = evaluated = 0
    for i, row in enumerate(roots):
        first = many_walk.dive(text, row, "ANY")
        every = many_walk.dive(text, row, "ALL")
        one = many_walk_upto.dive_upto(text, row, 1)
        whole = many_walk_upto.dive_upto(text, row, 2 ** 40)
        for f in FIELDS:
            assert one[f] == first[f], (name, i, f)
            assert whole[f] == every[f], (name, i, f)
        assert len(one["rows"]) == first["solutions"] and len(whole["rows"]) == every["solutions"]
        if first["first"] is not None:
            assert (one["rows"][0] == first["first"]).all() and (whole["rows"][0] == every["first"]).all()
        # distinct, fully valued, inside the root row
        assert len({r.tobytes() for r in whole["rows"]}) == len(whole["rows"])
        for r in whole["rows"]:
            assert r.shape == (roots.shape[1],) and ((r >= row[:, 0]) & (r <= row[:, 1])).all(), (name, i)
        if i < 6:
            for r in whole["rows"][:3]:
                assert _is_a_solution(text, r), (name, i)
                evaluated += 1
        # in walk order: what a smaller k keeps is the head of what a larger k keeps, with the counters of that moment
        for k in (2, 3, 5):
            part = many_walk_upto.dive_upto(text, row, k)
            assert part["status"] == many_walk.DONE and part["solutions"] == min(k, every["solutions"])
            assert len(part["rows"]) == part["solutions"]
            assert all((a == b).all() for a, b in zip(part["rows"], whole["rows"]))
            assert part["nodes"] <= every["nodes"]
            if every["solutions"] <= k - 1:  # the tree is exhausted below k: ALL, field for field
                assert all(part[f] == every[f] for f in FIELDS)
        several += every["solutions"] >= 2
        # slices of 1 + 7 + 56 + rest are the single walk, for k = 3
        want = many_walk_upto.dive_upto(text, row, 3)
        got = many_walk_upto.dive_sliced(text, row, [(1, 3), (7, 3), (56, 3), (1 << 40, 3)])
        assert all(got[f] == want[f] for f in FIELDS), (name, i)
        assert len(got["rows"]) == len(want["rows"]) and all((a == b).all() for a, b in zip(got["rows"], want["rows"]))
        # and a slice stops where the one walk with that budget stops
        w = many_walk_upto.WalkUpto(text, row)
        part, ref = w.run(8, 3), many_walk_upto.dive_upto(text, row, 3, 8)
        assert all(part[f] == ref[f] for f in FIELDS), (name, i)
    assert several >= 8 and evaluated >= 6


def test_a_slice_with_a_smaller_k_ends_an_instance_that_holds_it():
    text, roots = many_upto_sets.build("deep")
    ended = went_on = 0
    for row in roots[:12]:
        w = many_walk_upto.WalkUpto(text, row)
        part = w.run(50, 4)
        if part["status"] != many_walk.LIMIT:
            continue
        after = w.run(1 << 40, 1)
        assert after["status"] == many_walk.DONE
        if part["solutions"] >= 1:  # nothing is tried
            assert all(after[f] == part[f] for f in FIELDS[1:]) and len(after["rows"]) == len(part["rows"])
            ended += 1
        else:
            assert after["nodes"] > part["nodes"] and after["solutions"] == 1
            went_on += 1
    assert ended >= 1 and went_on >= 1


@pytest.mark.parametrize("name", sorted(many_upto_sets.SETS) + ["deep"])
def test_no_row_of_a_gpu_set_reaches_its_budget(name):
    """every row the GPU tests use, under every k they use: DONE, and below the recorded largest tree, which is far below
    the budget"""
    if name == "deep":
        ks, budget, largest = (many_upto_sets.DEEP[1],), many_upto_sets.DEEP[2], {many_upto_sets.DEEP[1]: many_upto_sets.DEEP[4]}
    else:
        _, ks, budget, _, largest = many_upto_sets.SETS[name]
    for k in ks:
        res = many_upto_sets.walk(name, k)
        assert 0 < largest[k] < budget
        assert (res["status"] == many_walk.DONE).all(), (name, k)
        assert res["nodes"].max() <= largest[k], (name, k, int(res["nodes"].max()))
        print(f"{name}, k = {k}: largest tree {int(res['nodes'].max())} nodes, solutions per instance {dict(zip(*map(np.ndarray.tolist, np.unique(res['solutions'], return_counts=True))))}")
    if name == "sudoku9":  # what the issue records for this set
        found = many_upto_sets.walk(name, 3)["solutions"]
        assert [int((found == 1).sum()), int((found == 2).sum()), int((found >= 3).sum())] == [13, 16, 35]
        assert many_upto_sets.walk(name, 2)["nodes"].max() == 18 and many_upto_sets.walk(name, 3)["nodes"].max() == 25
    if name == "queens12_two":
        assert int((many_upto_sets.walk(name, 2)["solutions"] == 0).sum()) == 6
    if name.startswith("sparse"):
        found = many_upto_sets.walk(name, 200)["solutions"]
        assert (found == 200).sum() > len(found) // 2, "most instances reach 200"
    if name == "deep":
        assert many_upto_sets.walk(name, 4)["nodes"].max() == 1311
        stopped = many_upto_sets.walk(name, 4, 50)
        assert (stopped["status"] == many_walk.LIMIT).sum() >= 8 and (stopped["nodes"][stopped["status"] == many_walk.LIMIT] == 50).all()


def test_some_sparse_instances_exhaust_their_tree_below_200():
    short = sum(int((many_upto_sets.walk(name, 200)["solutions"] < 200).sum()) for name in many_upto_sets.SETS if name.startswith("sparse"))
    assert short >= 1


def shipped_upto_kernels():
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == "cs_dive_upto" and "<" in name:
                shipped.add(name)
    return shipped


def test_shipped_upto_kernels_are_the_six_the_sets_name():
    from test_many_resume_host import shipped_resume_kernels
    from test_solve_many_host import shipped_dive_kernels
    shipped = shipped_upto_kernels()
    assert len(shipped) == 6
    for name in shipped:
        assert re.fullmatch(r"cs_dive_upto<unsigned (char|short), ([124])>", name), name
    assert {s[3] for s in many_upto_sets.SETS.values()} == shipped
    assert many_upto_sets.DEEP[3] in shipped
    assert len(shipped_dive_kernels()) == 6 and len(shipped_resume_kernels()) == 6  # the old families are what they were
