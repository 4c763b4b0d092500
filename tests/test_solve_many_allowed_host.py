"""CPU tests of csgpu_solve_many_allowed / _allowed_upto and Model.solve_many(..., branching="allowed"): the interface is
declared, exported and prototyped; the argument errors that need no device; the != relation the host walk reads from the
model's text (tests/many_walk_allowed.py) pinned against the oracle's own shaving; the walk's invariant; the walk against
the width walk it is derived from (tests/many_walk.py); the budgets of the GPU sets; the shipped instantiations."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import many_allowed_sets
import many_walk
import many_walk_allowed
from conftest import golden
from csolve_amd import problems

E_ARG, E_LIMIT, E_STATE = -1, -4, -5
FIELDS = many_walk.FIELDS
NEW_CALLS = {"csgpu_model_qualifies_many_allowed": 1, "csgpu_solve_many_allowed": 7, "csgpu_solve_many_allowed_upto": 7}
_walked = {}


def walked(name):
    """(text, roots, the allowed walk's answer under the set's own objective / k and budget), once per set"""
    if name not in _walked:
        text, roots, objective, k, budget = many_allowed_sets.build(name)
        want = many_walk_allowed.dive_many(text, roots, objective, budget) if k is None else \
            many_walk_allowed.upto_many(text, roots, k, budget)
        _walked[name] = (text, roots, want)
    return _walked[name]


def test_the_interface_is_declared_exported_and_prototyped():
    import inspect
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    raw = open(_lib.HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = _lib.load_library()
    for name, args in NEW_CALLS.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == args, name
        proto = re.search(rf"\bint {name}\((.*?)\);", text, flags=re.S)  # the header's prototype has as many parameters
        assert proto and len(proto.group(1).split(",")) == args, name
    for name in ("csgpu_internal_many_allowed_symbol", "csgpu_internal_many_allowed_upto_symbol"):
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == 3
        assert name not in raw  # cs_internal.h only
    # the specification stands in the header, beside the existing one
    for phrase in ("branching on the allowed values", "NOT a node", "next = value + 1", "128 values"):
        assert phrase in raw, phrase
    # options and records are the existing ones, as they were
    assert C.sizeof(_lib.ManyResult) == 40 and C.sizeof(_lib.ManyOptions) == 16 and C.sizeof(_lib.ManyUptoOptions) == 16
    assert [f for f, _ in _lib.ManyOptions._fields_] == ["objective", "reserved", "max_nodes"]
    assert [f for f, _ in _lib.ManyUptoOptions._fields_] == ["max_solutions", "reserved", "max_nodes"]
    assert len(L.csgpu_solve_many.argtypes) == 7 and len(L.csgpu_solve_many_upto.argtypes) == 7
    for method in ("solve_many", "solve_many_upto", "classify_many"):
        assert inspect.signature(getattr(Model, method)).parameters["branching"].default == "width", method
    for method in ("qualifies_many_allowed", "many_allowed_kernel", "many_allowed_upto_kernel"):
        assert callable(getattr(Model, method)), method
    assert not any("dive" in f or "many" in f or "allowed" in f for f in _lib.PLAN_FAMILIES) and len(_lib.PLAN_FAMILIES) == 16


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyOptions, ManyUptoOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(open(golden("problems", "queens8.txt")).read())  # parsed, not finalized
    rows = np.zeros((2, 8, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    ok, ok_k = ManyOptions(0, 0, 100), ManyUptoOptions(2, 0, 100)

    def plain(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data):
        rc = L.csgpu_solve_many_allowed(model, roots, count, C.byref(opt) if opt is not None else None, results, None, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    def upto(model=m._h, roots=rows.ctypes.data, count=2, opt=ok_k, results=res.ctypes.data):
        rc = L.csgpu_solve_many_allowed_upto(model, roots, count, C.byref(opt) if opt is not None else None, results, None, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    for call, options in ((plain, ManyOptions), (upto, ManyUptoOptions)):
        assert call(model=None)[0] == E_ARG
        assert call(roots=None)[0] == E_ARG
        assert call(results=None)[0] == E_ARG
        assert call(opt=None)[0] == E_ARG
        assert call(count=-1)[0] == E_ARG
        first = 0 if call is plain else 2
        assert call(opt=options(first, 0, 0))[0] == E_ARG
        assert call(opt=options(first, 0, -5))[0] == E_ARG
        assert "count" in call(count=-1, opt=options(first, 0, 0))[1]  # the count before the budget
        rc, msg = call()
        assert rc == E_STATE and "finalized" in msg
        assert call(count=0)[0] == E_STATE  # an empty batch is no way round the state check
    for objective in (2, 3):  # MIN / MAX: a limit of the call, named, before the model's state
        rc, msg = plain(opt=ManyOptions(objective, 0, 100))
        assert rc == E_LIMIT and "MIN" in msg and "MAX" in msg
    assert plain(opt=ManyOptions(7, 0, 100))[0] == E_ARG
    for k in (0, -3):
        rc, msg = upto(opt=ManyUptoOptions(k, 0, 100))
        assert rc == E_ARG and "max_solutions" in msg
    assert "max_nodes" in upto(opt=ManyUptoOptions(0, 0, 0))[1]  # the budget before k
    assert (res == 0).all()
    # a model without tables does not qualify, and NULL is no model
    assert L.csgpu_model_qualifies_many_allowed(m._h) == 0 and L.csgpu_model_qualifies_many_allowed(None) == 0
    assert m.qualifies_many_allowed() is False
    # the Python methods: the library's error for a numpy batch on a model that is not finalized (nothing is uploaded);
    # checkpoints= and an unknown rule are refused before the library is asked
    with pytest.raises(TypeError):
        m.solve_many(rows, branching="allowed")
    for use in (lambda: m.solve_many(rows, "ANY", max_nodes=10, branching="allowed"),
                lambda: m.solve_many_upto(rows, 2, max_nodes=10, branching="allowed"),
                lambda: m.classify_many(rows, max_nodes=10, branching="allowed")):
        with pytest.raises(CsolveError) as e:
            use()
        assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.solve_many_upto(rows, 0, max_nodes=10, branching="allowed")
    assert e.value.code == E_ARG
    pool = object()  # stands for a pool: it is not looked at
    with pytest.raises(ValueError, match="checkpoints"):
        m.solve_many(rows, "ANY", max_nodes=10, checkpoints=pool, branching="allowed")
    with pytest.raises(ValueError, match="checkpoints"):
        m.solve_many_upto(rows, 2, max_nodes=10, checkpoints=pool, branching="allowed")
    with pytest.raises(ValueError, match="branching"):
        m.solve_many(rows, "ANY", max_nodes=10, branching="narrowest")
    with pytest.raises(CsolveError) as e:  # the default is the call it was
        m.solve_many(rows, "ANY", max_nodes=10, branching="width")
    assert e.value.code == E_STATE


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
        m.solve_many(roots, "ANY", max_nodes=1000, branching="allowed")
    assert e.value.code == E_STATE


# ---- the relation of the host walk, pinned against the oracle ----------------------------------------------------------

def _pin(text, pairs, values_of):
    """for every (w, u) of `pairs`: u valued at a, w narrowed to [c, hi] and to [lo, c] for every c of values_of(w): the
    oracle's node `u = a` on the root state shaves exactly the bounds the relation forbids, up to the first value it does
    not forbid, and leaves every other bound of w where it is -> (cases, cases with a shaved bound)"""
    orc, dom = many_walk.oracle_for(text)
    rel = many_walk_allowed.relation(text)
    cases = shaved = 0
    for w, u in pairs:
        a = int(dom[u, 0] + dom[u, 1]) // 2
        forbidden = {a + d for x, d in rel[w] if x == u}
        lo_w, hi_w = int(dom[w, 0]), int(dom[w, 1])
        for c in values_of(w):
            for side in (0, 1):
                lo, hi = (c, hi_w) if side == 0 else (lo_w, c)
                if lo >= hi:
                    continue
                state = dom.copy()
                state[u] = (a, a)
                state[w] = (lo, hi)
                left = [x for x in range(lo, hi + 1) if x not in forbidden]
                status, out = orc.instance(state, u, a, a)
                cases += 1
                if not left:
                    assert status < 0, (w, u, a, lo, hi)
                    continue
                assert status >= 0, (w, u, a, lo, hi)
                assert (int(out[w, 0]), int(out[w, 1])) == (left[0], left[-1]), (w, u, a, lo, hi, out[w], sorted(forbidden))
                shaved += (left[0], left[-1]) != (lo, hi)
    return cases, shaved


@pytest.mark.parametrize("which", ["queens8", "wide20"])
def test_the_relation_is_the_oracles_on_every_pair_of_the_small_models(which):
    text = {"queens8": lambda: problems.queens(8, "ALL"), "wide20": lambda: many_allowed_sets.build("wide20_w96")[0]}[which]()
    _, dom = many_walk.oracle_for(text)
    n = dom.shape[0]
    rel = many_walk_allowed.relation(text)
    assert all((w, -d) in rel[u] for w in range(n) for u, d in rel[w]), "the relation is symmetric"
    if which == "queens8":
        assert all(sorted(d for x, d in rel[w] if x == u) == sorted({0, u - w, w - u}) for w in range(n) for u in range(n) if u != w)
    pairs = [(w, u) for w in range(n) for u in range(n) if w != u]
    cases, shaved = _pin(text, pairs, lambda w: range(int(dom[w, 0]), int(dom[w, 1]) + 1))
    print(f"{which}: {len(pairs)} pairs, {cases} nodes, {shaved} with a shaved bound")
    assert shaved >= len(pairs)  # (every related pair shaves somewhere, and most do on both sides of an interval)


@pytest.mark.parametrize("name", ["sudoku9_40_all", "sudoku16_any", "sparse40_e16", "sparse100_e16", "sparse150_e16",
                                  "sparse150_e16_w16", "sparse150_e8_w40"])
def test_the_relation_is_the_oracles_on_a_sample_of_the_large_models(name):
    text = many_allowed_sets.build(name)[0]
    _, dom = many_walk.oracle_for(text)
    rel = many_walk_allowed.relation(text)
    rng = problems.LCG(len(text))
    open_vars = [int(v) for v in np.flatnonzero(dom[:, 0] != dom[:, 1])]
    related = [(w, u) for w in open_vars for u in sorted({x for x, _ in rel[w]})]
    rng.shuffle(related)
    others = set()
    while len(others) < min(200, len(open_vars) * (len(open_vars) - 1) - len(related)):
        w, u = open_vars[rng.below(len(open_vars))], open_vars[rng.below(len(open_vars))]
        if w != u and not any(x == u for x, _ in rel[w]):
            others.add((w, u))
    a_mid = lambda w: range(int(dom[w, 0]), int(dom[w, 1]) + 1)
    cases, shaved = _pin(text, related[:200], a_mid)
    assert shaved >= len(related[:200])  # a related pair shaves somewhere: its offsets keep a mid value inside w's domain
    cases0, shaved0 = _pin(text, sorted(others), a_mid)
    assert shaved0 == 0  # an unrelated one nowhere
    print(f"{name}: {len(related)} related ordered pairs, {cases + cases0} nodes")


# ---- the walk ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(many_allowed_sets.SETS))
def test_no_row_of_a_gpu_set_reaches_its_budget_and_largest_is_the_walks(name):
    _, objective, k, budget, kernel, largest = many_allowed_sets.SETS[name]
    text, roots, want = walked(name)
    assert (want["status"] == many_walk.DONE).all(), name
    assert int(want["nodes"].max()) == largest < budget, (name, int(want["nodes"].max()))
    assert re.fullmatch(r"cs_dive_allowed<unsigned (char|short), [124], [14]>", kernel), kernel
    print(f"{name}: {len(roots)} instances, {int(want['nodes'].sum())} nodes, largest {largest}, {int(want['solutions'].sum())} solutions")


def test_the_sudoku_sets_have_the_node_counts_the_feature_was_proposed_with():
    """nodes total / deepest of the allowed rule, and of the width rule on the same rows"""
    for name, stop, allowed, width in (("sudoku9_30_any", 1, (702, 76), (3952, 1224)), ("sudoku9_40_all", None, (2347, 384), (4720, 1136)),
                                       ("sudoku9_25_upto2", 2, (3855, 3482), (26515, 15971))):
        text, roots, want = walked(name)
        assert (int(want["nodes"].sum()), int(want["nodes"].max())) == allowed, name
        by_width = [many_walk.Walk(text, row).run(1 << 40, stop)["nodes"] for row in roots]
        assert (sum(by_width), max(by_width)) == width, name


@pytest.mark.parametrize("name", sorted(n for n, s in many_allowed_sets.SETS.items() if s[1] == "ALL" and s[2] is None))
def test_all_counts_the_solutions_of_the_width_walk(name):
    text, roots, want = walked(name)
    by_width = many_walk.dive_many(text, roots, "ALL", 1 << 40)
    assert (want["solutions"] == by_width["solutions"]).all(), name
    assert (want["root_props"] == by_width["root_props"]).all()  # the root node is the same node
    # another tree, not a sub-tree: an instance may need more nodes than under the width rule, the set does differ
    assert (want["nodes"] != by_width["nodes"]).any(), "the set has a value the allowed rule skips"
    if name in many_allowed_sets.ROW_SETS:  # another order, the same SET of rows
        for i, row in enumerate(roots):
            a = many_walk_allowed.Walk(text, row).run(1 << 40)["rows"]
            b = many_walk.Walk(text, row).run(1 << 40)["rows"]
            assert len(a) == len(b) == len({r.tobytes() for r in a}) and {r.tobytes() for r in a} == {r.tobytes() for r in b}, (name, i)
    if name == "queens8_all":
        assert int(want["solutions"][0]) == 92


@pytest.mark.parametrize("name", ["queens8_all", "queens12_two", "sudoku9_40_all", "sudoku9_25_upto2", "sparse40_e16_w16", "wide20_w96"])
def test_at_every_node_the_bounds_are_allowed(name):
    """the specification's invariant, on the first rows of a set: at every node the walk enters, every open variable has
    at least two allowed values, the first is its lower bound and the last its upper bound"""
    text, roots, objective, k, budget = many_allowed_sets.build(name)
    seen = [0]

    def check(state, w, values):
        assert len(values) >= 2 and values[0] == state[w, 0] and values[-1] == state[w, 1], (name, w, state[w], values)
        seen[0] += 1

    for row in roots[:4]:
        walk = many_walk_allowed.Walk(text, row)
        if walk.open:  # the root node, then every node the walk enters
            for w in np.flatnonzero(walk.cur[:, 0] != walk.cur[:, 1]):
                check(walk.cur, int(w), many_walk_allowed.allowed(walk.rel, walk.cur, int(w)))
            walk.check = check
            walk.run(min(budget, 3000), 1 if objective == "ANY" else k)
    assert seen[0] > 100, name


def test_a_frame_goes_on_at_its_first_allowed_value():
    """the walk in slices of one node is the one walk (a frame is {node, variable, value + 1}), and under a budget it is the
    head of the whole walk"""
    text, roots, objective, k, budget = many_allowed_sets.build("sudoku9_40_all")
    for row in roots[:3]:
        whole = many_walk_allowed.Walk(text, row).run(1 << 40)
        walk = many_walk_allowed.Walk(text, row)
        out = walk.run(1)
        while out["status"] == many_walk.LIMIT:
            out = walk.run(1)
        assert all(out[f] == whole[f] for f in FIELDS)
        assert len(out["rows"]) == len(whole["rows"]) and all((a == b).all() for a, b in zip(out["rows"], whole["rows"]))
        for b in (1, 7):
            part = many_walk_allowed.dive(text, row, "ALL", b)
            assert (part["status"], part["nodes"]) == ((many_walk.LIMIT, b) if whole["nodes"] > b else (many_walk.DONE, whole["nodes"]))


def test_k_1_is_any_and_a_large_k_is_all():
    text, roots, objective, k, budget = many_allowed_sets.build("sudoku9_40_all")
    for row in roots[:8]:
        first, every = many_walk_allowed.dive(text, row, "ANY"), many_walk_allowed.dive(text, row, "ALL")
        one, whole = many_walk_allowed.upto(text, row, 1), many_walk_allowed.upto(text, row, 1 << 40)
        assert all(one[f] == first[f] and whole[f] == every[f] for f in FIELDS)
        assert (one["rows"][0] == first["first"]).all() and len(whole["rows"]) == every["solutions"]


def shipped_allowed_kernels(family):
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == family and "<" in name:
                shipped.add(name)
    return shipped


def test_shipped_kernels_are_those_the_sets_name():
    """the device-free half of the coverage test: both kernels are shipped for 8 / 16-bit entries x 1 / 2 / 4 variables per
    lane x 1 / 4 set words, and the sets of the GPU tests name every one of them (that each set plans the one it names is
    checked on the device); the older families are what they were"""
    from test_solve_many_host import shipped_dive_kernels
    from test_solve_many_upto_host import shipped_upto_kernels
    plain, upto = shipped_allowed_kernels("cs_dive_allowed"), shipped_allowed_kernels("cs_dive_allowed_upto")
    assert len(plain) == len(upto) == 12
    assert {s[4] for s in many_allowed_sets.SETS.values()} == plain
    assert {many_allowed_sets.upto_kernel(name) for name in many_allowed_sets.SETS} == upto
    assert len(shipped_dive_kernels()) == 6 and len(shipped_upto_kernels()) == 6
