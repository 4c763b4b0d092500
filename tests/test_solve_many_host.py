"""CPU tests of csgpu_solve_many / Model.solve_many: the interface is declared, exported and prototyped; the argument
errors that need no device; the host walk the GPU tests compare with (tests/many_walk.py) against the existing oracle
tree walk; the instance generator; the shipped cs_dive_shave instantiations."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import many_sets
import many_walk
from conftest import golden
from csolve_amd import problems

E_ARG, E_LIMIT, E_STATE = -1, -4, -5


def _header():
    from csolve_amd import _lib
    return re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    text = _header()
    assert "csgpu_solve_many" in _lib.declared_symbols()
    for name, value in (("CSGPU_MANY_DONE", 0), ("CSGPU_MANY_LIMIT", 1), ("CSGPU_MANY_BAD_ROOT", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
    assert (_lib.MANY_DONE, _lib.MANY_LIMIT, _lib.MANY_BAD_ROOT) == (0, 1, 2)
    res = re.search(r"typedef struct csgpu_many_result \{(.*?)\} csgpu_many_result;", text, flags=re.S).group(1)
    assert re.findall(r"\w+(?=[,;])", res) == [f for f, _ in _lib.ManyResult._fields_]
    opt = re.search(r"typedef struct csgpu_many_options \{(.*?)\} csgpu_many_options;", text, flags=re.S).group(1)
    assert re.findall(r"\w+(?=[,;])", opt) == [f for f, _ in _lib.ManyOptions._fields_]
    assert C.sizeof(_lib.ManyResult) == 40 and C.sizeof(_lib.ManyOptions) == 16
    L = _lib.load_library()
    assert hasattr(L, "csgpu_solve_many") and L.csgpu_solve_many.argtypes is not None and len(L.csgpu_solve_many.argtypes) == 7
    assert callable(getattr(Model, "solve_many"))
    # the new family stays out of the plan dictionary
    assert not any("dive" in f or "many" in f for f in _lib.PLAN_FAMILIES)


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(open(golden("problems", "queens8.txt")).read())  # parsed, not finalized
    rows = np.zeros((2, 8, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    ok = ManyOptions(0, 0, 100)

    def call(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data):
        L.csgpu_model_from_text  # (the library is loaded)
        rc = L.csgpu_solve_many(model, roots, count, C.byref(opt) if opt is not None else None, results, None, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    assert call(model=None)[0] == E_ARG
    assert call(roots=None)[0] == E_ARG
    assert call(results=None)[0] == E_ARG
    assert call(opt=None)[0] == E_ARG
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
    # the Python method: max_nodes is required, and a numpy batch on a model that is not finalized gets the library's
    # error (nothing is uploaded for it)
    with pytest.raises(TypeError):
        m.solve_many(rows)
    with pytest.raises(CsolveError) as e:
        m.solve_many(rows, "ANY", max_nodes=10)
    assert e.value.code == E_STATE


def test_no_device_means_loud_failure():
    """Without a HIP device a well-formed use fails with the library's errors: the root phase with the HIP error, and
    solve_many on the model that could not be finalized with the state error -- never a CPU search."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from csolve_amd import CsolveError
    from csolve_amd.solver import Model
    text, roots = problems.sudoku_roots(3, 0.4, [1, 2])
    m = Model.from_text(text)
    with pytest.raises(CsolveError, match="hip|HIP|device"):
        m.root_propagate()
    with pytest.raises(CsolveError):  # no root phase, no device tables
        m.finalize()
    with pytest.raises(CsolveError) as e:
        m.solve_many(roots, "ANY", max_nodes=1000)
    assert e.value.code == E_STATE


@pytest.mark.parametrize("which", ["queens7", "sudoku9"])
def test_the_walk_gives_the_totals_of_the_oracle_tree_on_all(which):
    from test_gpu_search import oracle_all_tree
    text = {"queens7": lambda: problems.queens(7, "ALL"), "sudoku9": lambda: problems.sudoku(3, 0.35, 1, "ALL")}[which]()
    _, dom = many_walk.oracle_for(text)
    d = many_walk.dive(text, dom, "ALL", 1 << 40)
    assert d["status"] == many_walk.DONE and d["root_props"] == 0  # the root domains are a fixpoint already
    assert (d["nodes"], d["cuts"], d["solutions"], d["props"]) == oracle_all_tree(text, dom)


def test_the_walk_any_and_budget():
    from oracle.cs_oracle import Model as OModel, Oracle
    text = problems.queens(8, "ALL")
    _, dom = many_walk.oracle_for(text)
    every = many_walk.dive(text, dom, "ALL", 1 << 40)
    first = many_walk.dive(text, dom, "ANY", 1 << 40)
    assert every["solutions"] == 92 and first["solutions"] == 1 and first["status"] == many_walk.DONE
    assert 0 < first["nodes"] < every["nodes"]
    assert (first["first"] == every["first"]).all()  # ALL keeps the first one too
    om = OModel.parse(text)
    om.set_domains(np.stack([first["first"], first["first"]], 1).astype(np.int32))
    om.index()
    assert Oracle(om).eval(om.root) == (1, 1)
    for k in (1, 17, first["nodes"] - 1):
        d = many_walk.dive(text, dom, "ANY", k)
        assert d["status"] == many_walk.LIMIT and d["nodes"] == k and d["solutions"] == 0
    d = many_walk.dive(text, dom, "ANY", first["nodes"])  # the budget is not reached by the node that finishes
    assert d["status"] == many_walk.DONE and d["nodes"] == first["nodes"]
    d = many_walk.dive(text, dom, "ALL", every["nodes"])
    assert d["status"] == many_walk.DONE and d["solutions"] == 92
    # rows that are not searched
    bad = dom.copy()
    bad[3, 1] += 1
    assert many_walk.dive(text, bad, "ANY", 10)["status"] == many_walk.BAD_ROOT
    bad = dom.copy()
    bad[2] = (5, 4)
    assert many_walk.dive(text, bad, "ANY", 10)["status"] == many_walk.BAD_ROOT
    clash = dom.copy()
    clash[0], clash[1] = (3, 3), (3, 3)
    d = many_walk.dive(text, clash, "ALL", 10)
    assert (d["status"], d["nodes"], d["solutions"], d["root_props"]) == (many_walk.DONE, 0, 0, 0)


@pytest.mark.parametrize("box,revealed,seeds", [(3, 0.4, [1, 2, 7, 19]), (3, 0.3, [5]), (4, 0.6, [3])])
def test_sudoku_roots_are_the_instances_sudoku_writes(box, revealed, seeds):
    """the root domains of sudoku(box, revealed, seed) after the oracle's root phase = the oracle's root node on the
    generated row over the empty model (variables matched by name: sudoku() declares its givens first)"""
    from oracle.cs_oracle import Model as OModel, Oracle
    text, roots = problems.sudoku_roots(box, revealed, seeds)
    n = box * box
    assert roots.shape == (len(seeds), n * n, 2) and roots.dtype == np.int32
    assert "=" not in text.replace("<=", "") and text.count("all_different") == 3 * n
    orc, dom = many_walk.oracle_for(text)
    assert (dom == np.array([1, n])).all()
    names = orc.model.names()
    assert names == [f"C{r}_{c}" for r in range(n) for c in range(n)]
    for k, seed in enumerate(seeds):
        single = problems.sudoku(box, revealed, seed)
        assert int((roots[k, :, 0] == roots[k, :, 1]).sum()) == single.count(" = ")
        om = OModel.parse(single)
        o = Oracle(om)
        o.set_root_phase(True)
        assert o.propagate(om.root, om.n_vars) >= 0
        want = dict(zip(om.names(), map(tuple, o.domains().tolist())))
        status, got = orc.instance(roots[k], -1, 0, 0)
        assert status >= 0
        assert dict(zip(names, map(tuple, got.tolist()))) == want


@pytest.mark.parametrize("name,make", [
    ("queens8", lambda: problems.queens(8)), ("queens16", lambda: problems.queens(16)),
    ("queens8_all", lambda: problems.queens(8, "ALL")), ("sudoku9_s7", lambda: problems.sudoku(3, 0.4, 7)),
    ("sudoku25_s1", lambda: problems.sudoku(5, 0.4, 1)), ("schedule6_s1", lambda: problems.schedule(6, 1)),
])
def test_existing_generators_write_what_they_wrote(name, make):
    assert make() == open(golden("problems", name + ".txt")).read()


def shipped_dive_kernels():
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == "cs_dive_shave" and "<" in name:
                shipped.add(name)
    return shipped


def test_shipped_dive_kernels_are_those_the_sets_name():
    """the device-free half of the coverage test: the family is there, every name parses, and the sets of the GPU tests
    name exactly the shipped instantiations (that each set plans the one it names is checked on the device)"""
    from test_host import FIXPOINT_FAMILIES
    assert "cs_dive_shave" not in FIXPOINT_FAMILIES
    shipped = shipped_dive_kernels()
    assert shipped
    for name in shipped:
        m = re.fullmatch(r"cs_dive_shave<unsigned (char|short), ([124])>", name)
        assert m, name
    assert {s[3] for s in many_sets.SETS.values()} == shipped


@pytest.mark.parametrize("name", sorted(many_sets.SETS))
def test_no_instance_of_a_set_reaches_its_budget(name):
    """a sample of every set (the first eight rows and the last four) by the walk: DONE below the budget, and the
    recorded largest tree of the set is below the budget as well"""
    text, roots, objective, budget = many_sets.build(name)
    largest = many_sets.SETS[name][4]
    assert 0 < largest < budget
    sample = np.concatenate([roots[:8], roots[-4:]])
    res = many_walk.dive_many(text, sample, objective, budget)
    assert (res["status"] == many_walk.DONE).all() and res["nodes"].max() <= largest


def _plain(x):
    """a walk's answer as JSON holds it"""
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    return None if x is None else int(x)


def _walk_calls(text, row):
    """every call the recorded walks pin, on one root row: the whole result dict of each, and the open subtrees of every
    walk that stops at LIMIT"""
    import many_resume_walk
    import many_walk_upto
    calls = {}
    for objective in ("ANY", "ALL"):
        for budget in (1, 7, 1 << 62):
            calls[f"dive {objective} {budget}"] = many_walk.dive(text, row, objective, budget)
    w, parts = many_resume_walk.Walk(text, row, "ALL"), []
    while not parts or parts[-1][0]["status"] == many_walk.LIMIT:
        part = w.run(5)
        stopped = part["status"] == many_walk.LIMIT
        parts.append([part, w.open_subtrees() if stopped else None, w.has_last_value_frame() if stopped else None])
    calls["Walk ALL by 5"] = parts
    for k in (1, 2, 3, 1 << 40):
        calls[f"WalkUpto {k}"] = many_walk_upto.WalkUpto(text, row).run(1 << 62, k)
    slices = [(5, 2), (9, 1), (1 << 62, 3)]
    w, parts = many_walk_upto.WalkUpto(text, row), []
    for budget, k in slices:
        part = w.run(budget, k)
        parts.append([part, w.open_subtrees() if part["status"] == many_walk.LIMIT else None])
    calls["WalkUpto by slices"] = parts
    calls["dive_sliced"] = many_walk_upto.dive_sliced(text, row, slices)
    return _plain(calls)


def test_the_walks_give_what_the_three_separate_walks_gave():
    """tests/golden/many_walk/recorded.json holds what many_walk.dive, many_resume_walk.Walk and many_walk_upto.WalkUpto
    / dive_sliced answered while each had a loop of its own (recorded by _walk_calls at the last commit that had them):
    every field and every row of every call is still that, on queens-7 and four 9x9 sudokus under ALL and on three root
    rows that are not searched"""
    import json
    recorded = json.load(open(golden("many_walk", "recorded.json")))
    texts = {"queens7": problems.queens(7, "ALL"), "sudoku9": problems.sudoku_roots(3, 0.40, [1, 2, 3, 4], "ALL")[0]}
    sudoku_rows = problems.sudoku_roots(3, 0.40, [1, 2, 3, 4], "ALL")[1]
    assert [c["what"] for c in recorded] == ["root domains", "a solution", "lo > hi", "inconsistent at the root"] + ["sudoku row"] * 4
    assert recorded[0]["row"] == many_walk.oracle_for(texts["queens7"])[1].tolist()
    assert [c["row"] for c in recorded[4:]] == sudoku_rows[:4].tolist()
    for case in recorded:
        got = _walk_calls(texts[case["model"]], np.array(case["row"], dtype=np.int32))
        assert sorted(got) == sorted(case["calls"])
        for call, want in case["calls"].items():
            assert got[call] == want, (case["model"], case["what"], call)
