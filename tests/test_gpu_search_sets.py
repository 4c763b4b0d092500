"""GPU tests of the device search engine on clause models (search_sets.py: `<`, `<=`, `=`, `!=`, two-literal
disjunctions, sums with constant factors; some variables hundreds of values wide): the ALL tree -- nodes, cuts, solutions
-- and the streamed solution set against the recorded walk of the oracle-backed engine and a brute force, by every route
that must not change the tree; MIN / MAX of a variable and of an expression against the extremes over that set; interval
halving on the device.  Nothing here is compared with a number the device produced."""
import functools

import numpy as np
import pytest

import search_sets as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAMES = list(S.SETS)
POOL, CHILDREN = 1 << 18, 1 << 14
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the solution set of a set, by the oracle-backed engine; its size is the table's"""
    st, found, _ = S.reference_walk(S.text_of(name))
    assert st["solutions"] == len(found) == S.SETS[name]["solutions"]
    return frozenset(found)


def _model(name, objective="ALL", fast_paths=True, kernel=None):
    from csolve_amd.solver import set_linear_fast_paths, solve_root
    try:
        set_linear_fast_paths(fast_paths)
        model = solve_root(S.text_of(name, objective))
    finally:
        set_linear_fast_paths(True)
    if kernel is not None:
        model.set_kernel(kernel)
    return model


def _points(model, rows):
    """solution rows of the model -> set of tuples (C1 .. Cn), and how many rows there were"""
    cols = S.columns(model.var_names())
    return {tuple(int(r[c]) for c in cols) for r in rows}, len(rows)


def _all_true(model, rows):
    if len(rows):
        rows = np.asarray(rows, dtype=np.int32)
        states = torch.from_numpy(np.ascontiguousarray(np.stack([rows, rows], 2))).cuda().contiguous()
        assert (model.eval_root(states).cpu().numpy() == 1).all()


def _all(model, pool=POOL, children=CHILDREN, parents=None, order=None, stream_rows=None):
    """an ALL search to its end with the solution stream on -> (engine, statistics, streamed rows)"""
    from csolve_amd.solver import Search
    s = Search(model, pool, children)
    if order is not None:
        s.set_strategy(order)
    if parents is not None:
        s.set_parents(parents)
    s.stream_solutions(stream_rows)
    s.put(model.root_state())
    batches = list(s.iter_solutions())
    rows = np.concatenate(batches) if batches else np.zeros((0, model.n_vars), dtype=np.int32)
    return s, s.stats, rows


def _check_all(name, model, s, st, rows):
    rec = S.SETS[name]
    assert st["done"] == 1 and st["pool"] == 0
    print(name, {k: st[k] for k in ("nodes", "cuts", "solutions", "props", "iterations")})
    assert (st["nodes"], st["cuts"], st["solutions"]) == (rec["nodes"], rec["cuts"], rec["solutions"])
    points, count = _points(model, rows)
    assert count == rec["solutions"], "a solution streamed twice or not at all"
    assert points == _reference(name)
    _all_true(model, rows)


@pytest.mark.parametrize("name", NAMES)
def test_all_tree_and_solution_set(name):
    """ALL by the default engine: nodes, cuts and solutions are the recorded walk's, the streamed rows are the
    reference set, each once and each true under the device's root evaluation; up to 1,024 solutions the store holds the
    same set"""
    model = _model(name)
    assert model.objective == 1 and (model.device_info()["tree_clauses"] > 0) == S.SETS[name]["tree"]
    s, st, rows = _all(model)
    _check_all(name, model, s, st, rows)
    stored = s.solutions(1 << 20)
    assert len(stored) == min(1024, S.SETS[name]["solutions"])
    points, _ = _points(model, stored)
    assert len(points) == len(stored) and points <= _reference(name)
    if S.SETS[name]["solutions"] <= 1024:
        assert points == _reference(name)


ROUTES = ["kernel1", "kernel6", "tree-interpreter", "evaluated", "small-pool", "one-parent", "64-parents", "tiny-stream"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_the_same_tree_by_every_route(name, route, monkeypatch):
    """what must not change an ALL tree: the general kernel or the clause-resident one for the fixpoints (the engine
    launches what Model.set_kernel chose, csgpu_internal_propagate_objdev), the clauses through the expression-tree
    interpreter instead of the linear fast paths, the root evaluation of every complete child, a pool of 2,000 rows,
    iterations of one parent (depth first, the single-workgroup expansion) and of 64, a stream that fills up after a few
    parents -- the recorded nodes, cuts and solutions and the reference set every time"""
    monkeypatch.delenv("CSGPU_SEARCH_EVAL", raising=False)
    model = _model(name, fast_paths=route != "tree-interpreter")
    if route == "tree-interpreter":
        assert model.device_info()["tree_clauses"] > 0
    if route == "kernel1":
        model.set_kernel(1)
    if route == "kernel6":
        if not model.qualifies(6):  # more than 512 clauses: the default engine already walked it by kernel 1
            assert model.n_clauses > 512
            return
        model.set_kernel(6)
    if route == "evaluated":
        monkeypatch.setenv("CSGPU_SEARCH_EVAL", "1")
    pool, children = (2000, 1024) if route == "small-pool" else (POOL, CHILDREN)
    parents = {"one-parent": 1, "64-parents": 64}.get(route)
    widest = int((model.domains()[:, 1].astype(np.int64) - model.domains()[:, 0] + 1).max())
    stream_rows = 4 * min(widest, 256) if route == "tiny-stream" else None
    s, st, rows = _all(model, pool, children, parents, stream_rows=stream_rows)
    _check_all(name, model, s, st, rows)
    if route == "small-pool":
        assert st["pool_peak"] <= 2000


@pytest.mark.parametrize("order", ["none", "smallest-domain", "largest-domain", "smallest-value", "largest-value"])
@pytest.mark.parametrize("name", ["narrow_sums7", "wide3_plain"])
def test_every_variable_order_finds_the_reference_set(name, order):
    """the five branching rules: other trees (a wide variable first, under largest-domain), the same solutions"""
    model = _model(name)
    s, st, rows = _all(model, order=order)
    assert st["done"] == 1 and st["solutions"] == S.SETS[name]["solutions"]
    points, count = _points(model, rows)
    assert count == st["solutions"] and points == _reference(name)
    _all_true(model, rows)


def _optimise(model, pool=POOL, children=CHILDREN, parents=None, slice_iterations=1 << 40):
    from csolve_amd.solver import Search
    s = Search(model, pool, children)
    if parents is not None:
        s.set_parents(parents)
    s.put(model.root_state())
    iterations = 0
    while True:
        st = s.run(slice_iterations)
        assert st["iterations"] - iterations <= slice_iterations
        iterations = st["iterations"]
        if st["done"]:
            return s, st


def _check_optimum(name, model, s, st, objective, optimum, value):
    assert st["done"] == 1
    print(name, objective, {k: st[k] for k in ("best", "nodes", "cuts", "solutions", "iterations")})
    row = s.best_solution()
    if optimum is None:
        assert st["solutions"] == 0 and row is None
        assert st["best"] == (INT32_MAX if objective.startswith("MIN") else INT32_MIN)
        return
    assert st["best"] == optimum and st["solutions"] >= 1
    assert row is not None and row[model.objective_var] == optimum
    points, _ = _points(model, [row])
    point = next(iter(points))
    assert point in _reference(name) and value(point) == optimum
    _all_true(model, [row])


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["min-var", "max-var", "min-expr", "max-expr"])
@pytest.mark.parametrize("name", NAMES)
def test_min_and_max_reach_the_extremes_of_the_solution_set(name, which):
    """MIN and MAX of the set's objective variable and of 2*C1 + C3: the search ends, `best` is the extreme over the
    reference set (below zero for several sets), best_solution() attains it, is a point of that set and true under the
    root evaluation; the infeasible set ends with the sentinel and no solution"""
    objective, optimum, value = S.optimisations(name)[which]
    model = _model(name, objective)
    assert model.objective == (2 if objective.startswith("MIN") else 3)
    s, st = _optimise(model)
    _check_optimum(name, model, s, st, objective, optimum, value)


@pytest.mark.parametrize("which", [1, 2], ids=["max-var", "min-expr"])
@pytest.mark.parametrize("name", ["narrow_sums7", "wide3_sums", "wide3_plain"])
def test_device_driven_and_host_driven_iterations_reach_the_same_optimum(name, which, monkeypatch):
    """the five ways of driving MIN / MAX iterations (one hipGraph per burst, the same launches one by one, every
    iteration from the host, the bookkeeping by one workgroup, every complete child evaluated) on a narrow set and on
    wide ones with and without expression-tree clauses: the recorded optimum each time, and the graph's statistics are
    those of the plain launches, of the one-workgroup bookkeeping and of the evaluated run"""
    objective, optimum, value = S.optimisations(name)[which]
    model = _model(name, objective)
    switches = ("CSGPU_SEARCH_GRAPH", "CSGPU_SEARCH_BURST", "CSGPU_SEARCH_BURST_SPLIT", "CSGPU_SEARCH_EVAL")
    stats = {}
    for mode, env in (("graph", {}), ("launches", {"CSGPU_SEARCH_GRAPH": "0"}), ("host", {"CSGPU_SEARCH_BURST": "0"}),
                      ("one-workgroup", {"CSGPU_SEARCH_BURST_SPLIT": "0"}), ("evaluated", {"CSGPU_SEARCH_EVAL": "1"})):
        for k in switches:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s, st = _optimise(model, 1 << 20, 1 << 16, parents=64, slice_iterations=21)
        _check_optimum(name, model, s, st, objective, optimum, value)
        stats[mode] = st
    assert stats["graph"] == stats["launches"]
    assert stats["graph"] == stats["one-workgroup"]
    assert stats["graph"] == stats["evaluated"]


@pytest.mark.parametrize("name", NAMES)
def test_any_returns_a_point_of_the_reference_set(name):
    from csolve_amd.solver import Search
    model = _model(name, "ANY")
    s = Search(model, POOL, CHILDREN)
    s.put(model.root_state())
    st = s.run()
    assert st["done"] == 1
    assert (st["solutions"] >= 1) == bool(_reference(name))
    if st["solutions"]:
        rows = s.solutions(1)
        points, _ = _points(model, rows)
        assert points <= _reference(name)
        _all_true(model, rows)


def test_take_and_put_across_a_halving():
    """open states whose branching interval is still wider than 256 values move to a second engine: both halve on
    their own, the solution counts add up to the recorded number and the streamed rows together are the reference set"""
    from csolve_amd.solver import Search
    name = "wide3_sums"
    model = _model(name)
    a, b = Search(model, POOL, CHILDREN), Search(model, POOL, CHILDREN)
    a.stream_solutions()
    b.stream_solutions()
    a.put(model.root_state())
    st = a.run(2)
    assert not st["done"] and st["pool"] >= 2
    stolen = a.take(st["pool"] // 2).contiguous()
    assert 0 < stolen.shape[0] < st["pool"]
    dom = stolen.cpu().numpy().astype(np.int64)
    width = dom[:, :, 1] - dom[:, :, 0] + 1
    # the branching interval of a state is its smallest open one: every open interval of such a state is wide
    branching = np.where(width > 1, width, 1 << 40).min(axis=1)
    assert (branching > 256).any(), "no taken state is about to be halved"
    b.put(stolen)
    rows_a = [r for batch in a.iter_solutions() for r in batch]
    rows_b = [r for batch in b.iter_solutions() for r in batch]
    assert a.stats["done"] == 1 and b.stats["done"] == 1 and b.stats["nodes"] > 0
    assert a.stats["solutions"] + b.stats["solutions"] == S.SETS[name]["solutions"] == len(rows_a) + len(rows_b)
    assert a.stats["nodes"] + b.stats["nodes"] == S.SETS[name]["nodes"]
    points, _ = _points(model, rows_a + rows_b)
    assert points == _reference(name)


def test_the_sets_reach_the_paths_they_are_meant_for():
    """across the table: models with and without expression-tree clauses on the device, several instantiations of the
    clause-resident kernel and a model it does not take, and a wide set whose whole ALL tree (the recorded one, which
    test_all_tree_and_solution_set pins the device to) has fewer nodes than the values of its widest root interval --
    enumerating that interval once would already need more"""
    tree, rounds, beyond = set(), {}, []
    for name in NAMES:
        model = _model(name)
        tree.add(model.device_info()["tree_clauses"] > 0)
        rounds[name] = model.plan()["rounds"]
        if not model.qualifies(6):
            beyond.append(name)
            assert rounds[name] is None
        print(name, "clauses", model.n_clauses, "kernel", model.kernel(), rounds[name])
    assert tree == {False, True}
    assert len({r for r in rounds.values() if r is not None}) >= 2
    assert beyond, "every model fits the clause-resident kernel"
    halved_on_the_device = []
    for name in S.WIDE:
        model = _model(name)
        widest = int((model.domains()[:, 1].astype(np.int64) - model.domains()[:, 0] + 1).max())
        assert widest > 256
        if S.SETS[name]["nodes"] < widest:
            s, st, rows = _all(model)
            assert st["nodes"] == S.SETS[name]["nodes"] < widest
            halved_on_the_device.append(name)
    assert halved_on_the_device
