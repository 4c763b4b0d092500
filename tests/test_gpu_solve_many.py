"""GPU tests of Model.solve_many (csgpu_solve_many, cs_dive_shave): every instance of every set of tests/many_sets.py
against the host walk of tests/many_walk.py, which asks the oracle for every node; the budget; rows that are not
searched; launch independence; the search engine as corroboration; the coverage of the kernel family.
Every call passes a finite max_nodes."""
import numpy as np
import pytest

import many_sets
import many_walk

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("status", "root_props", "nodes", "cuts", "props", "solutions")
_models = {}
_walks = {}


def _model(text):
    from csolve_amd.solver import solve_root
    if text not in _models:
        _models[text] = solve_root(text)
    return _models[text]


def _set(name):
    """(text, roots, objective, budget, the walk's answer), built once"""
    if name not in _walks:
        text, roots, objective, budget = many_sets.build(name)
        _walks[name] = (text, roots, objective, budget, many_walk.dive_many(text, roots, objective, budget))
    return _walks[name]


def _run(model, roots, objective, budget, solutions=True):
    out = model.solve_many(torch.from_numpy(np.ascontiguousarray(roots)).cuda(), objective, max_nodes=budget,
                           solutions=solutions)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(got, want, label, rows=None):
    """every field of every instance; the first solution where there is one"""
    idx = np.arange(len(want["status"])) if rows is None else np.asarray(rows)
    for f in FIELDS:
        g, w = got[f].astype(np.int64), want[f][idx]
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, walk {w[bad[0]]}"
    if "first" in got:
        has = want["solutions"][idx] > 0
        assert (got["first"][has] == want["first"][idx][has]).all(), f"{label}: first solutions differ"
        assert (got["first"][~has] == 0).all(), f"{label}: a row without a solution was written"


@pytest.mark.parametrize("name", sorted(many_sets.SETS))
def test_every_instance_equals_the_walk(name):
    text, roots, objective, budget, want = _set(name)
    largest = int(want["nodes"].max())
    print(f"{name}: {len(roots)} instances, largest tree {largest} nodes, budget {budget}, "
          f"{int((want['nodes'] == 0).sum())} without a node, {int(want['solutions'].sum())} solutions")
    assert (want["status"] == many_walk.DONE).all() and largest < budget, "the set must stay below its budget"
    model = _model(text)
    assert model.many_kernel() == many_sets.SETS[name][3]
    _check(_run(model, roots, objective, budget), want, name)


def test_every_wave_draws_several_tickets():
    """sudoku9_any repeated until the batch has four times as many instances as the launch has waves: repeated instances
    give identical rows, whichever wave draws them and whatever it ran before"""
    text, roots, objective, budget, want = _set("sudoku9_any")
    model = _model(text)
    resident = model.many_waves(1 << 30)
    reps = -(-4 * resident // len(roots))
    big = np.tile(roots, (reps, 1, 1))
    waves = model.many_waves(len(big))
    print(f"{len(big)} instances on {waves} waves")
    assert waves == resident and len(big) >= 4 * waves
    _check(_run(model, big, objective, budget), want, "sudoku9_any tiled", rows=np.tile(np.arange(len(roots)), reps))


def test_the_budget_stops_an_instance_at_exactly_max_nodes():
    text, roots, objective, _, full = _set("queens12_two")
    budget = 2000
    over = full["nodes"] > budget
    assert over.any() and (~over).any(), "the budget must split the set"
    want = many_walk.dive_many(text, roots, objective, budget)
    assert (want["status"][over] == many_walk.LIMIT).all() and (want["nodes"][over] == budget).all()
    got = _run(_model(text), roots, objective, budget)
    _check(got, want, "queens12_two, budget 2000")
    assert (got["status"][over] == many_walk.LIMIT).all() and (got["nodes"][over] == budget).all()
    for f in FIELDS:  # those below the budget are as without it
        assert (got[f][~over] == full[f][~over]).all(), f


def test_bad_and_trivial_rows_leave_their_neighbours_alone():
    text, roots, objective, budget, want = _set("sudoku9_any")
    model = _model(text)
    batch = roots[:6].copy()
    alone = {f: want[f][:6].copy() for f in FIELDS + ("first",)}
    batch[1, 40] = (1, 10)  # outside the root domains
    batch[3, 7] = (6, 5)    # lo > hi
    solved = want["first"][4]
    batch[4] = np.stack([solved, solved], 1)  # a complete consistent row
    for i in (1, 3):
        for f in FIELDS:
            alone[f][i] = 0
        alone["status"][i] = many_walk.BAD_ROOT
        alone["first"][i] = 0
    for f in FIELDS:
        alone[f][4] = 0
    alone["solutions"][4] = 1
    alone["first"][4] = solved
    walked = many_walk.dive_many(text, batch, objective, budget)
    for f in FIELDS + ("first",):
        assert (walked[f] == alone[f]).all(), f
    _check(_run(model, batch, objective, budget), alone, "bad and trivial rows")
    without = _run(model, batch, objective, budget, solutions=False)  # d_solutions == NULL
    assert "first" not in without
    _check(without, alone, "no solution buffer")
    empty = model.solve_many(torch.empty((0, model.n_vars, 2), dtype=torch.int32, device="cuda"), "ANY", max_nodes=5)
    assert empty["status"].shape == (0,) and empty["first"].shape == (0, model.n_vars)


@pytest.mark.parametrize("name", ["sudoku9_any", "sudoku16_any", "queens12_two", "sparse100_e16"])
def test_every_first_solution_is_one(name):
    from oracle.cs_oracle import Model as OModel, Oracle
    text, roots, objective, budget, want = _set(name)
    got = _run(_model(text), roots, objective, budget)
    solved = np.flatnonzero(got["solutions"] > 0)
    assert solved.size > 0
    om = OModel.parse(text)
    for i in solved:
        row = got["first"][i]
        assert ((row >= roots[i, :, 0]) & (row <= roots[i, :, 1])).all(), f"instance {i}: outside its givens"
        om.set_domains(np.stack([row, row], 1).astype(np.int32))
        om.index()
        assert Oracle(om).eval(om.root) == (1, 1), f"instance {i}"


def test_launch_independence():
    text, roots, objective, budget, want = _set("sudoku9_all")
    model = _model(text)
    K = len(roots)
    whole = _run(model, roots, objective, budget)
    _check(whole, want, "one call")
    for part in (slice(0, K // 2), slice(K // 2, K)):
        _check(_run(model, roots[part], objective, budget), want, "halves", rows=np.arange(K)[part])
    perm = np.random.default_rng(5).permutation(K)
    _check(_run(model, roots[perm], objective, budget), want, "permuted", rows=perm)
    # two calls back to back on one stream, no host synchronisation in between: the ticket counters reset themselves
    dev = torch.from_numpy(roots).cuda()
    torch.cuda.synchronize()
    a = model.solve_many(dev, "ALL", max_nodes=budget)
    b = model.solve_many(dev[: K // 3], "ANY", max_nodes=budget)
    c = model.solve_many(dev, "ALL", max_nodes=budget)
    torch.cuda.synchronize()
    _check({k: v.cpu().numpy() for k, v in a.items()}, want, "first of three")
    _check({k: v.cpu().numpy() for k, v in c.items()}, want, "third of three")
    any_want = many_walk.dive_many(text, roots[: K // 3], "ANY", budget)
    _check({k: v.cpu().numpy() for k, v in b.items()}, any_want, "second of three")


@pytest.mark.parametrize("name,rows", [("queens12_two", 6), ("sudoku9_all", 6), ("sparse100_e16", 3)])
def test_all_totals_are_those_of_a_search_seeded_with_the_root(name, rows):
    """corroboration: the existing engine, seeded with the instance's root fixpoint (kernel 7, a `var < 0` node), walks
    the same ALL tree: the same nodes, cuts, solutions and propagations"""
    from csolve_amd.solver import Search
    text, roots, objective, budget, want = _set(name)
    assert objective == "ALL"
    model = _model(text)
    got = _run(model, roots, objective, budget)
    search = Search(model, 1 << 18, 1 << 14)
    compared = 0
    for i in np.flatnonzero(want["nodes"] > 0)[:rows]:
        node = torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32, device="cuda")
        state, res = model.propagate(torch.from_numpy(roots[i:i + 1].copy()).cuda(), node)
        assert int(res[0, 0]) > 0 and int(res[0, 1]) == got["root_props"][i]
        search.reset()
        search.put(state.contiguous())
        st = search.run()
        assert st["done"] == 1
        assert (st["nodes"], st["cuts"], st["solutions"], st["props"]) == tuple(int(got[f][i]) for f in ("nodes", "cuts", "solutions", "props"))
        compared += 1
    assert compared == rows


def test_the_sets_plan_every_shipped_instantiation():
    """coverage of the family: the cs_dive_shave instantiations the library ships are exactly those the sets of
    test_every_instance_equals_the_walk plan (and launch)"""
    from test_solve_many_host import shipped_dive_kernels
    planned = set()
    for name in many_sets.SETS:
        text = many_sets.build(name)[0]
        kernel = _model(text).many_kernel()
        assert kernel == many_sets.SETS[name][3], name
        planned.add(kernel)
    assert planned == shipped_dive_kernels()


def test_models_outside_kernel_7_are_refused_with_the_reason():
    from csolve_amd import CsolveError, problems
    model = _model(problems.schedule(6, 1))
    assert not model.qualifies(7) and model.many_kernel() is None
    rows = torch.from_numpy(model.domains()[None].copy()).cuda()
    with pytest.raises(CsolveError, match="does not qualify") as e:
        model.solve_many(rows, "ANY", max_nodes=100)
    assert e.value.code == -4
    plan = _model(problems.queens(12, "ALL")).plan()
    assert not any(v and "cs_dive_shave" in v for v in plan.values())  # the plan dictionary is what it was
