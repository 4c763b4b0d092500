"""GPU tests of the device search engine under the reference's variable orders (-o none | smallest-domain |
largest-domain | smallest-value | largest-value) and of its ANY restarts (-r): the ALL tree of every set of
order_walk.RECORDED -- nodes, cuts, solutions, the streamed set, on != networks the propagations -- against the host walk
with the same rule, by every route that must not change it; MIN / MAX under every order against the recorded extremes;
the Luby schedule, counted in iterations, on instances without a solution, where every restart must leave a whole tree to
the run that ends the search.  Nothing here is compared with a number the device produced."""
import functools

import numpy as np
import pytest

import order_walk as W
import search_sets as S
from test_gpu_search_sets import CHILDREN, POOL, _all_true, _check_optimum

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROUTE_SETS = ["narrow_sums7", "wide2_mid", "planted80", "queens8"]
OPT_SETS = ["narrow_sums7", "wide2_straddle", "wide2_mid", "infeasible6"]
RESTARTED = {"narrow_sums7": 1, "wide2_straddle": 0, "wide2_mid": 2, "infeasible6": 3}  # set -> one of its four objectives


def _model(name, objective="ALL"):
    from csolve_amd.solver import solve_root
    text = W.text_of(name)
    assert text.count("ALL;") == 1
    return solve_root(text.replace("ALL;", objective + ";", 1))


def _points(model, rows, names):
    """solution rows of the model -> set of tuples in the order of `names`"""
    mine = model.var_names()
    cols = [mine.index(s) for s in names]
    return {tuple(int(r[c]) for c in cols) for r in rows}


def _all(model, order, prefer_failing=None, pool=POOL, children=CHILDREN, parents=None):
    """an ALL search to its end with the solution stream on, the strategy set before the root is put -> (statistics,
    streamed rows)"""
    from csolve_amd.solver import Search
    s = Search(model, pool, children)
    if prefer_failing is None:
        s.set_strategy(order)
    else:
        s.set_strategy(order, prefer_failing)
    if parents is not None:
        s.set_parents(parents)
    s.stream_solutions()
    s.put(model.root_state())
    batches = list(s.iter_solutions())
    rows = np.concatenate(batches) if batches else np.zeros((0, model.n_vars), dtype=np.int32)
    return s.stats, rows


def _check_tree(name, order, model, st, rows, props):
    """done, nothing left in the pool, the recorded nodes / cuts / solutions, the streamed rows the walk's set, each once
    and each true at the root; props: on a != network the propagations of the consistent children as well"""
    nodes, cuts, solutions, _ = W.RECORDED[name, order]
    print(name, order, {k: st[k] for k in ("nodes", "cuts", "solutions", "props", "iterations")})
    assert st["done"] == 1 and st["pool"] == 0
    assert (st["nodes"], st["cuts"], st["solutions"]) == (nodes, cuts, solutions)
    reference = W.walk(name, "smallest-domain")  # the same set under every order (test_order_walk_host.py)
    assert len(rows) == solutions, "a solution streamed twice or not at all"
    assert _points(model, rows, reference["names"]) == reference["found"]
    _all_true(model, rows)
    if props:
        assert name in W.NETWORKS and st["props"] == W.walk(name, order)["props"]


@pytest.mark.parametrize("name,order", W.PAIRS, ids=[f"{n}-{o}" for n, o in W.PAIRS])
def test_all_tree_under_every_variable_order(name, order):
    """a rule that picks another variable, a tie that does not go to the lowest index, negative lower bounds ordered
    after positive ones, the parent-set cut or the fused levels kept under a rule they do not implement: each walks
    another tree than the host walk's"""
    model = _model(name)
    st, rows = _all(model, order)
    _check_tree(name, order, model, st, rows, props=name in W.NETWORKS)


@pytest.mark.parametrize("route", ["one-parent", "64-parents", "small-pool"])
@pytest.mark.parametrize("order", W.NON_DEFAULT)
@pytest.mark.parametrize("name", ROUTE_SETS)
def test_routes_that_must_not_change_a_tree(name, order, route):
    """iterations of one parent (depth first, the single-workgroup expansion) and of 64, a pool of 2,000 rows with
    1,024 children: the same numbers and the same set each time"""
    model = _model(name)
    pool, children = (2000, 1024) if route == "small-pool" else (POOL, CHILDREN)
    st, rows = _all(model, order, pool=pool, children=children, parents={"one-parent": 1, "64-parents": 64}.get(route))
    _check_tree(name, order, model, st, rows, props=name in W.NETWORKS)
    if route == "small-pool":
        assert st["pool_peak"] <= 2000


@pytest.mark.parametrize("name", W.SETS_OF_THE_TABLE)
def test_the_default_rule_set_explicitly_is_the_default_engine(name):
    """set_strategy("smallest-domain", False) keeps the fused levels and the parent-set cut: the default record, on the
    != networks with the propagations"""
    model = _model(name)
    st, rows = _all(model, "smallest-domain", prefer_failing=False)
    _check_tree(name, "smallest-domain", model, st, rows, props=name in W.NETWORKS)
    if name in S.SETS:
        rec = S.SETS[name]
        assert (st["nodes"], st["cuts"], st["solutions"]) == (rec["nodes"], rec["cuts"], rec["solutions"])


def _optimise(model, order, restart_on_improvement=False, parents=None):
    from csolve_amd.solver import Search
    s = Search(model, POOL, CHILDREN)
    s.set_strategy(order)
    if restart_on_improvement:
        s.set_restart_on_improvement(True)
    if parents is not None:
        s.set_parents(parents)
    s.put(model.root_state())
    if parents is None:
        return s, s.run()
    for _ in range(1 << 20):  # an iteration per call: the engine looks at the incumbent after every one
        st = s.run(1)
        if st["done"]:
            return s, st
    raise AssertionError("the search did not end")


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["min-var", "max-var", "min-expr", "max-expr"])
@pytest.mark.parametrize("order", W.NON_DEFAULT)
@pytest.mark.parametrize("name", OPT_SETS)
def test_min_and_max_reach_the_extremes_under_every_order(name, order, which):
    """the search ends, `best` is the recorded extreme over the reference set, best_solution() attains it, lies in that
    set and is true at the root; the infeasible set ends with the sentinel and no solution"""
    objective, optimum, value = S.optimisations(name)[which]
    model = _model(name, objective)
    assert model.objective == (2 if objective.startswith("MIN") else 3)
    s, st = _optimise(model, order)
    _check_optimum(name, model, s, st, objective, optimum, value)
    assert st["restarts"] == 0


@pytest.mark.parametrize("order", W.NON_DEFAULT)
@pytest.mark.parametrize("name", OPT_SETS)
def test_restarts_on_improvement_reach_the_same_optimum(name, order):
    """one objective per set with a restart from the root on every better solution: the same optimum, and the search
    did restart (the infeasible set has no solution to restart on: none there).  One parent per iteration, depth first,
    and one iteration per call: the engine restarts when it sees a better incumbent with states still open, which it
    looks for between bursts of iterations -- with its default iterations of a thousand parents these small searches
    are over within the first burst"""
    objective, optimum, value = S.optimisations(name)[RESTARTED[name]]
    model = _model(name, objective)
    s, st = _optimise(model, order, restart_on_improvement=True, parents=1)
    _check_optimum(name, model, s, st, objective, optimum, value)
    if optimum is None:
        assert st["restarts"] == 0
    else:
        assert st["restarts"] >= 1


# ---- ANY restarts --------------------------------------------------------------------------------------------------

PIGEONS = {"pigeon7": (7, False), "pigeon8": (8, False), "pigeon7-tree": (7, True)}


@functools.lru_cache(maxsize=None)
def _pigeon_tree(which):
    """(nodes, cuts) of the whole tree of a pigeonhole model, by the host walk under the default rule"""
    n, tree = PIGEONS[which]
    got = W.all_tree(W.pigeon(n, tree, "ALL"), "smallest-domain")
    assert got["solutions"] == 0 and got["complete_false"] == 0
    return got["nodes"], got["cuts"]


@functools.lru_cache(maxsize=None)
def _pigeon_model(which):
    from csolve_amd.solver import solve_root
    n, tree = PIGEONS[which]
    model = solve_root(W.pigeon(n, tree))
    assert model.objective == 0 and (model.device_info()["tree_clauses"] > 0) == tree
    assert model.qualifies(7) == (not tree)
    return model


def _any(model, base, slice_iterations):
    """an ANY search driven in slices to its end, restarts of `base` set before the root is put (None: the default) ->
    (final statistics, [(iterations, nodes, cuts) at each restart], the engine)"""
    from csolve_amd.solver import Search
    s = Search(model, POOL, CHILDREN)
    if base is not None:
        s.set_restart(base)
    s.put(model.root_state())
    marks, restarts, iterations = [], 0, 0
    for _ in range(1 << 20):
        st = s.run(slice_iterations)
        assert st["iterations"] - iterations <= slice_iterations
        iterations = st["iterations"]
        if st["restarts"] != restarts:
            assert slice_iterations > 1 or st["restarts"] == restarts + 1
            restarts = st["restarts"]
            marks.append((st["iterations"], st["nodes"], st["cuts"]))
        if st["done"]:
            return st, marks, s
    raise AssertionError("the search did not end")


@pytest.mark.parametrize("base", [1, 2, 5])
@pytest.mark.parametrize("which", list(PIGEONS))
def test_any_restarts_keep_the_luby_schedule_and_the_whole_tree(which, base):
    """an instance without a solution, one iteration per call: restart k comes exactly luby(k) * base + 1 iterations
    after restart k - 1 (the reference's _fail_count > _fail_threshold * frequency, counted in iterations), the run
    that ends the search fits into its own allowance and is a complete walk -- the nodes and cuts of the host walk's
    tree --, no abandoned run has more nodes than that; the same search in one call and in slices of five ends with the
    same statistics (what the clipping of a device-driven burst is for)"""
    model = _pigeon_model(which)
    nodes, cuts = _pigeon_tree(which)
    st, marks, _ = _any(model, base, 1)
    print(which, base, {k: st[k] for k in ("iterations", "restarts", "nodes", "cuts")}, marks[:4])
    assert st["solutions"] == 0 and st["done"] == 1 and st["pool"] == 0
    assert st["restarts"] == len(marks)
    before = (0, 0, 0)
    for k, mark in enumerate(marks, start=1):
        assert mark[0] - before[0] == W.luby(k) * base + 1, (k, mark, before)
        assert mark[1] - before[1] <= nodes, (k, mark, before)
        before = mark
    assert 1 <= st["iterations"] - before[0] <= W.luby(len(marks) + 1) * base + 1
    assert (st["nodes"] - before[1], st["cuts"] - before[2]) == (nodes, cuts)
    if base in (1, 2):
        assert st["restarts"] >= 3, "the schedule was not exercised"
    for slice_iterations in (1 << 40, 5):
        other, _, _ = _any(model, base, slice_iterations)
        assert other["done"] == 1 and other["solutions"] == 0 and other["pool"] == 0
        assert {k: other[k] for k in ("iterations", "restarts", "nodes", "cuts")} == \
            {k: st[k] for k in ("iterations", "restarts", "nodes", "cuts")}, slice_iterations


@pytest.mark.parametrize("which", list(PIGEONS))
def test_any_without_restarts_walks_the_tree_once(which):
    model = _pigeon_model(which)
    for slice_iterations in (1, 1 << 40):
        st, marks, _ = _any(model, 0, slice_iterations)
        assert st["done"] == 1 and st["pool"] == 0 and st["solutions"] == 0
        assert st["restarts"] == 0 and not marks
        assert (st["nodes"], st["cuts"]) == _pigeon_tree(which)


@pytest.mark.parametrize("base", [0, 1, None], ids=["base0", "base1", "default"])
@pytest.mark.parametrize("which", ["queens24", "planted30"])
def test_any_restarts_on_instances_with_a_solution(which, base):
    """the search ends with exactly one solution accepted, true at the root (and, for the clause set, a point of the
    reference set); two runs with the same settings give identical statistics"""
    from csolve_amd import problems
    from csolve_amd.solver import solve_root
    model = solve_root(problems.queens(24) if which == "queens24" else S.text_of(which, "ANY"))
    assert model.objective == 0
    runs = []
    for _ in range(2):
        st, marks, s = _any(model, base, 1 << 40)
        assert st["done"] == 1 and st["solutions"] == 1
        if base == 0:
            assert st["restarts"] == 0
        rows = s.solutions(4)
        assert len(rows) == 1
        _all_true(model, rows)
        if which == "queens24":
            row = rows[0]
            assert len(set(row)) == 24 and len(set(row + np.arange(24))) == 24 and len(set(row - np.arange(24))) == 24
        else:
            reference = W.walk(which, "smallest-domain")
            assert _points(model, rows, reference["names"]) <= reference["found"]
        runs.append(st)
    assert runs[0] == runs[1]
