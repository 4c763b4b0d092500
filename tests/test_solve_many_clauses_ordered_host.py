"""CPU tests of csgpu_solve_many_clauses_ordered / Model.solve_many_clauses_ordered: the interface is declared, exported
and prototyped; the argument errors that need no device; the host walk the GPU tests compare with
(tests/many_walk_ordered.py) against the recorded trees of order_walk under every order, against many_walk_objective
where nothing halves and against itself in slices; the new row sets; the frame bound; the shipped cs_walk_order
instantiations."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import many_clause_sets as sets
import many_walk_objective as W
import many_walk_ordered as O
import order_walk
from csolve_amd import problems

E_ARG, E_STATE = -1, -5
EIGHT = {f"cs_walk_order<{cpl}, {tree}>" for cpl in (1, 2, 4, 8) for tree in ("true", "false")}
SPLITS = (1, 2, 16, 256)


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model, Search
    for name in ("csgpu_solve_many_clauses_ordered", "csgpu_many_clauses_ordered_frames"):
        assert name in _lib.declared_symbols(), name
    L = _lib.load_library()
    assert len(L.csgpu_solve_many_clauses_ordered.argtypes) == 9
    assert len(L.csgpu_internal_many_clauses_order_symbol.argtypes) == 3
    assert C.sizeof(_lib.ManyOrderOptions) == 24
    for method in ("solve_many_clauses_ordered", "many_clauses_ordered_frames", "many_clauses_order_kernel"):
        assert callable(getattr(Model, method)), method
    assert Model.MANY_ORDERS == Search.ORDERS and list(Model.MANY_ORDERS) == O.ORDERS  # the names of csolve_gpu -o
    header = open(_lib.HEADER_PATH).read()
    for phrase in ("mid = (lo + hi) >> 1", "before any incumbent bound", "Prefer-failing is not part of this walk",
                   "halved h times with ceiling"):
        assert phrase in header, phrase


def test_argument_errors_come_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import CsolveError, ManyOrderOptions
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(problems.schedule(5, 1))  # MIN; parsed, not finalized
    n = m.n_vars
    rows = np.zeros((2, n, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    ok = ManyOrderOptions(2, 1, 256, 0, 100)

    def call(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data):
        rc = L.csgpu_solve_many_clauses_ordered(model, roots, count, C.byref(opt) if opt is not None else None, results, None,
                                                None, None, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    # csgpu_solve_many_clauses's own, in its order
    assert call(model=None)[0] == E_ARG
    assert call(roots=None)[0] == E_ARG
    assert call(results=None)[0] == E_ARG
    assert call(opt=None)[0] == E_ARG
    assert call(count=-1)[0] == E_ARG
    assert call(opt=ManyOrderOptions(2, 1, 256, 0, 0))[0] == E_ARG
    assert call(opt=ManyOrderOptions(7, 1, 256, 0, 100))[0] == E_ARG
    rc, msg = call(opt=ManyOrderOptions(3, 1, 256, 0, 100))  # MAX on a MIN model
    assert rc == E_ARG and "MIN" in msg and "MAX" in msg
    # the state comes before the new ones: they are raised after csgpu_solve_many_clauses's own
    for opt in (ok, ManyOrderOptions(2, 9, 256, 0, 100), ManyOrderOptions(2, 1, -1, 0, 100), ManyOrderOptions(2, 1, 256, 1, 100)):
        rc, msg = call(opt=opt)
        assert rc == E_STATE and "finalized" in msg
    assert call(count=0)[0] == E_STATE
    assert L.csgpu_many_clauses_ordered_frames(m._h, 256) == 0 and L.csgpu_many_clauses_ordered_frames(None, 256) == 0
    # the Python method: max_nodes is required, the order is one of the five names
    with pytest.raises(TypeError):
        m.solve_many_clauses_ordered(rows)
    with pytest.raises(KeyError):
        m.solve_many_clauses_ordered(rows, "MIN", max_nodes=10, order="widest")
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses_ordered(rows, "MIN", max_nodes=10)
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:
        m.solve_many_clauses_ordered(rows, "MAX", max_nodes=10, order="none", split_width=4)
    assert e.value.code == E_ARG


@pytest.mark.parametrize("name,order", O.RECORDED_PAIRS)
def test_the_walk_reproduces_the_recorded_all_trees(name, order):
    """from the root-domain row of the model as many_walk_objective.oracle_for normalises it: nodes, cuts, solutions and
    halvings of order_walk.all_tree, which was derived without a stack, an incumbent or a budget"""
    got = O.recorded_walk(name, order)
    assert got["status"] == O.DONE
    assert (got["nodes"], got["cuts"], got["solutions"], got["halvings"]) == order_walk.RECORDED[name, order]


def test_the_recorded_pairs_are_those_of_the_thirteen_sets():
    assert len(O.RECORDED_SETS) == 13 and "planted150" not in O.RECORDED_SETS and "sudoku9" not in O.RECORDED_SETS
    assert set(O.RECORDED_PAIRS) == {k for k in order_walk.RECORDED if k[0] in O.RECORDED_SETS}
    assert len(O.RECORDED_PAIRS) == 63  # all five orders but for wide3_sums, which has three
    assert W.model_of(order_walk.text_of("planted150")).n_clauses > 512


@pytest.mark.parametrize("name", sorted(sets.SETS))
def test_nothing_changes_where_nothing_halves(name):
    """smallest-domain with a split_width no narrower than the widest interval of the rows is many_walk_objective's walk,
    field for field, at the set's budget"""
    text, roots, objective, budget = sets.build(name)
    widest = int((roots[:, :, 1].astype(np.int64) - roots[:, :, 0] + 1).max())
    assert widest <= 2**31 - 1
    want = sets.walked(name)
    got = O.walk_many(text, roots, objective, budget, "smallest-domain", widest)
    for f in want:
        assert (got[f] == want[f]).all(), f
    assert (got["halvings"] == 0).all() and got["deepest"].max() < roots.shape[1]


@pytest.mark.parametrize("name,order,split", O.CASES)
def test_the_new_row_sets_meet_their_conditions(name, order, split):
    text, roots, objective, budget = O.build(name)
    res = O.walked(name, order, split)
    assert len(roots) <= 64
    if O.SETS[name][4]:
        assert (res["status"] == O.DONE).all()
        assert 0 < res["nodes"].max() <= 20000 and res["nodes"].max() < budget
        assert (res["solutions"] > 0).any()
    else:  # compared AT the budget, with LIMIT and the best so far
        limit = res["status"] == O.LIMIT
        assert limit.any() and not limit.all() and budget <= 4096
        assert (res["nodes"][limit] == budget).all() and (res["nodes"][~limit] < budget).all()
        assert (limit & (res["solutions"] > 0)).any()
    if name == "schedule5_open_min":  # the optimum of every row, proven; a stack the plain walk's n frames would not hold
        assert (res["best"] == 18).all() and (res["halvings"] > 0).all()
        assert res["deepest"].max() > roots.shape[1]
    if split < 256:
        assert (res["halvings"] > 0).any()


def test_the_sets_cover_every_objective_and_order():
    assert {s[1] for s in O.SETS.values()} == {"ANY", "MIN", "MAX"}  # ALL: the recorded trees
    assert {order for _, order, _ in O.CASES} == set(O.ORDERS)
    assert [(o, s) for n, o, s in O.CASES if n == "schedule5_open_min"] == [(o, s) for o in O.ORDERS for s in (256, 4)]
    for name in ("wcet_max", "linear12_any", "wide2_mid_any", "schedule6_min_budget"):
        orders = [o for n, o, _ in O.CASES if n == name]
        assert len(orders) == 2 and (name == "schedule6_min_budget" or "smallest-domain" not in orders)


def test_the_plain_walk_spends_its_budget_on_the_open_end_rows():
    """what the ordered walk is for: today's rule enumerates `end` above the incumbent, one cut child per value"""
    text, roots, objective, budget = O.build("schedule5_open_min")
    row = roots[0]
    plain = W.walk(text, row, objective, 2000)
    assert plain["status"] == W.LIMIT
    halved = O.walk(text, row, objective, 2000, "smallest-domain", 256)
    assert halved["status"] == O.DONE and halved["best"] == 18 and halved["nodes"] < 2000


def test_wide2_mid_needs_more_frames_than_variables():
    """under the default rule the recorded ALL walk of wide2_mid holds 5 frames with 4 variables"""
    got = O.recorded_walk("wide2_mid", "smallest-domain")
    n = W.oracle_for(order_walk.text_of("wide2_mid"))[1].shape[0]
    assert n == 4 and got["deepest"] > n


@pytest.mark.parametrize("name", O.WIDE)
def test_the_frame_bound_holds(name):
    """n + sum h(v) is never below the deepest stack plus the current node, for split_width 1, 2, 16 and 256"""
    text = order_walk.text_of(name)
    dom = W.oracle_for(text)[1]
    for split in SPLITS:
        bound = O.frames(dom, split)
        assert bound >= dom.shape[0]
        for order in ("smallest-domain", "largest-value"):
            got = O.walk(text, dom, "ALL", 4000, order, split)  # a budget: the deepest stack is reached early
            assert got["deepest"] + 1 <= bound, (split, order, got["deepest"], bound)
            assert got["halvings"] > 0


def test_the_frame_bound_of_the_row_sets():
    for name, order, split in O.CASES:
        text, roots, _, _ = O.build(name)
        assert O.walked(name, order, split)["deepest"].max() + 1 <= O.frames(W.oracle_for(text)[1], split)
    assert O.frames(np.array([[0, 0], [1, 256], [1, 257], [-2**31, 2**31 - 1]]), 256) == 4 + 0 + 0 + 1 + 24
    assert O.frames(np.array([[1, 5]]), 1) == 1 + 3  # 5 -> 3 -> 2 -> 1


def test_budget_slices_add_up():
    """a walk in slices is the walk with the summed budget: halvings are counted once per parent"""
    text, roots, objective, _ = O.build("schedule5_open_min")
    for row in roots[:3]:
        w, spent = O.Walk(text, row, objective, "none", 4), 0
        for budget in (1, 2, 7, 30, 1 << 40):
            part = w.run(budget)
            spent += budget
            ref = O.walk(text, row, objective, spent, "none", 4)
            assert {k: v for k, v in part.items() if k != "first"} == {k: v for k, v in ref.items() if k != "first"}
        assert part["status"] == O.DONE


def shipped_order_kernels():
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == "cs_walk_order" and "<" in name:
                shipped.add(name)
    return shipped


def test_the_shipped_order_kernels_are_exactly_the_eight():
    shipped = shipped_order_kernels()
    for name in shipped:
        assert re.fullmatch(r"cs_walk_order<[1248], (true|false)>", name), name
    assert shipped == EIGHT == {s[3].replace("cs_walk_clauses", "cs_walk_order") for s in sets.SETS.values()}
