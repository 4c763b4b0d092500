"""GPU tests of Model.solve_many / solve_many_upto / classify_many with branching="allowed" (csgpu_solve_many_allowed and
_allowed_upto, cs_dive_allowed and cs_dive_allowed_upto): every instance of every set of tests/many_allowed_sets.py
against the host walk of tests/many_walk_allowed.py, which asks the oracle for every node and reads the != relation from
the model's text; up to k; the budget; rows that are not searched; calls queued with the width walk on one stream; more
instances than waves; the coverage of both kernels; the refusals.  Every call passes a finite max_nodes."""
import numpy as np
import pytest

import many_allowed_sets
import many_walk
import many_walk_allowed

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = many_walk.FIELDS
DONE, LIMIT, BAD_ROOT = many_walk.DONE, many_walk.LIMIT, many_walk.BAD_ROOT
SENTINEL = -77
_models, _sets, _walks = {}, {}, {}


def _model(text):
    from csolve_amd.solver import solve_root
    if text not in _models:
        _models[text] = solve_root(text)
    return _models[text]


def _set(name):
    """(text, roots, roots on the device, budget), built once"""
    if name not in _sets:
        text, roots, _, _, budget = many_allowed_sets.build(name)
        _sets[name] = (text, roots, torch.from_numpy(roots).cuda(), budget)
    return _sets[name]


def _walk(name, objective=None, k=None, budget=None):
    """the host walk of a set under ANY / ALL (k None) or up to k, once per (set, stop, budget)"""
    text, roots, _, set_budget = _set(name)
    budget = set_budget if budget is None else budget
    key = (name, objective, k, budget)
    if key not in _walks:
        _walks[key] = many_walk_allowed.dive_many(text, roots, objective, budget) if k is None else \
            many_walk_allowed.upto_many(text, roots, k, budget)
    return _walks[key]


def _host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


def _plain(model, dev, objective, budget, **more):
    return _host(model.solve_many(dev, objective, max_nodes=budget, branching="allowed", **more))


def _upto(model, dev, k, budget):
    rows = torch.full((dev.shape[0], k, model.n_vars), SENTINEL, dtype=torch.int32, device="cuda")
    return _host(model.solve_many_upto(dev, k, max_nodes=budget, solutions=rows, branching="allowed"))


def _check(got, want, label, rows=None):
    """every field of every instance; the first solution where there is one, zeros elsewhere; with `rows` in the answer,
    row j of an instance for j < its solutions and the sentinel in every row behind them"""
    idx = np.arange(len(want["status"])) if rows is None else np.asarray(rows)
    for f in FIELDS:
        g, w = got[f].astype(np.int64), want[f][idx]
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, walk {w[bad[0]]}"
    if "first" in got:
        has = want["solutions"][idx] > 0
        assert (got["first"][has] == want["first"][idx][has]).all(), f"{label}: first solutions differ"
        assert (got["first"][~has] == 0).all(), f"{label}: a row without a solution was written"
    if "rows" in got:
        k = got["rows"].shape[1]
        there = np.arange(k)[None, :] < want["solutions"][idx][:, None]
        assert (got["rows"][there] == want["rows"][idx][:, :k][there]).all(), f"{label}: solution rows differ"
        assert (got["rows"][~there] == SENTINEL).all(), f"{label}: a row behind an instance's solutions was written"


@pytest.mark.parametrize("objective", ["ANY", "ALL"])
@pytest.mark.parametrize("name", sorted(n for n, s in many_allowed_sets.SETS.items() if s[2] is None))
def test_every_instance_equals_the_walk(name, objective):
    """both objectives on every set of the plain call, under the set's budget (which its own objective stays below; the
    other one may reach it: LIMIT, with the walk's counters at that budget)"""
    text, roots, dev, budget = _set(name)
    want = _walk(name, objective)
    model = _model(text)
    assert model.qualifies_many_allowed()
    assert model.many_allowed_kernel() == many_allowed_sets.SETS[name][4]
    if many_allowed_sets.SETS[name][1] == objective:
        assert (want["status"] == DONE).all() and int(want["nodes"].max()) == many_allowed_sets.SETS[name][5] < budget
    print(f"{name} {objective}: {len(roots)} instances, {int(want['nodes'].sum())} nodes, largest tree {int(want['nodes'].max())}, "
          f"{int((want['status'] == LIMIT).sum())} at the budget {budget}, {int(want['solutions'].sum())} solutions")
    _check(_plain(model, dev, objective, budget), want, f"{name} {objective}")


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("name", sorted(many_allowed_sets.SETS))
def test_up_to_k_every_field_and_row_equals_the_walk(name, k):
    text, roots, dev, budget = _set(name)
    want = _walk(name, k=k)
    model = _model(text)
    assert model.many_allowed_upto_kernel() == many_allowed_sets.upto_kernel(name)
    if many_allowed_sets.SETS[name][2] == k:
        assert (want["status"] == DONE).all() and int(want["nodes"].max()) == many_allowed_sets.SETS[name][5] < budget
    got = _upto(model, dev, k, budget)
    _check(got, want, f"{name}, k = {k}")
    assert (got["solutions"] <= k).all()
    if k == 1:  # the ANY call, field for field, and its row
        first = _plain(model, dev, "ANY", budget)
        for f in FIELDS:
            assert (first[f] == got[f]).all(), f
        has = got["solutions"] > 0
        assert (first["first"][has] == got["rows"][has, 0]).all()


def test_classify_many_agrees_with_the_width_rule_where_both_decide():
    text, roots, dev, budget = _set("sudoku9_40_all")
    model = _model(text)
    a = model.classify_many(dev, max_nodes=budget, branching="allowed")
    w = model.classify_many(dev, max_nodes=budget)
    torch.cuda.synchronize()
    a, w = a.cpu().numpy(), w.cpu().numpy()
    want = _walk("sudoku9_40_all", k=2)
    assert (a == np.where(want["status"] == LIMIT, -1, want["solutions"])).all()
    both = (a >= 0) & (w >= 0)
    assert both.sum() >= len(roots) // 2 and (a[both] == w[both]).all()
    print(f"classes (allowed rule): {dict(zip(*map(np.ndarray.tolist, np.unique(a, return_counts=True))))}, decided by both: {int(both.sum())}")


@pytest.mark.parametrize("budget", [1, 7])
def test_the_budget_stops_an_instance_at_exactly_max_nodes(budget):
    text, roots, dev, _ = _set("sudoku9_25_upto2")
    model = _model(text)
    for objective in ("ANY", "ALL"):
        want = _walk("sudoku9_25_upto2", objective, budget=budget)
        assert (want["status"] == LIMIT).all() and (want["nodes"] == budget).all() and (want["solutions"] == 0).all()
        got = _plain(model, dev, objective, budget)
        _check(got, want, f"budget {budget} {objective}")
        assert (got["nodes"] == budget).all() and (got["status"] == LIMIT).all()
    want = _walk("sudoku9_25_upto2", k=2, budget=budget)
    _check(_upto(model, dev, 2, budget), want, f"budget {budget}, up to 2")


def test_bad_and_trivial_rows_leave_their_neighbours_alone():
    text, roots, dev, budget = _set("sudoku9_30_any")
    model = _model(text)
    want = _walk("sudoku9_30_any", "ANY")
    batch = roots[:7].copy()
    alone = {f: want[f][:7].copy() for f in FIELDS + ("first",)}
    batch[1, 40] = (1, 10)  # outside the root domains
    batch[3, 7] = (6, 5)    # lo > hi
    solved = want["first"][4]
    batch[4] = np.stack([solved, solved], 1)  # a complete consistent row: its one solution, no node
    clash = np.flatnonzero(roots[5, :9, 0] != roots[5, :9, 1])[:2]  # two open cells of the grid's first row, one value:
    assert len(clash) == 2                                          # an inconsistent root
    batch[5, clash] = 5
    for i in (1, 3, 4, 5):
        for f in FIELDS:
            alone[f][i] = 0
        alone["first"][i] = 0
    alone["status"][1] = alone["status"][3] = BAD_ROOT
    alone["solutions"][4] = 1
    alone["first"][4] = solved
    walked = many_walk_allowed.dive_many(text, batch, "ANY", budget)
    for f in FIELDS + ("first",):
        assert (walked[f] == alone[f]).all(), f
    assert walked["status"][5] == DONE and walked["nodes"][5] == 0 and walked["solutions"][5] == 0  # an inconsistent root
    bdev = torch.from_numpy(batch).cuda()
    _check(_plain(model, bdev, "ANY", budget), alone, "bad and trivial rows")
    without = _plain(model, bdev, "ANY", budget, solutions=False)  # d_solutions == NULL
    assert "first" not in without
    _check(without, alone, "no solution buffer")
    two = many_walk_allowed.upto_many(text, batch, 2, budget)
    _check(_upto(model, bdev, 2, budget), two, "bad and trivial rows, up to 2")
    empty = model.solve_many(torch.empty((0, model.n_vars, 2), dtype=torch.int32, device="cuda"), "ANY", max_nodes=5,
                             branching="allowed")
    assert empty["status"].shape == (0,) and empty["first"].shape == (0, model.n_vars)


def test_calls_of_both_rules_queued_on_one_stream():
    """no host synchronisation between them: the shared ticket counters are left at zero by every kernel of the family"""
    text, roots, dev, budget = _set("sudoku9_40_all")
    model = _model(text)
    rows = torch.full((len(roots), 2, model.n_vars), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    a = model.solve_many(dev, "ALL", max_nodes=budget, branching="allowed")
    b = model.solve_many(dev, "ALL", max_nodes=budget)
    c = model.solve_many_upto(dev, 2, max_nodes=budget, solutions=rows, branching="allowed")
    d = model.solve_many(dev[:11], "ANY", max_nodes=budget, branching="allowed")
    _check(_host(a), _walk("sudoku9_40_all", "ALL"), "allowed, first of four")
    _check(_host(b), many_walk.dive_many(text, roots, "ALL", budget), "width, second of four")
    _check(_host(c), _walk("sudoku9_40_all", k=2), "allowed up to 2, third of four")
    _check(_host(d), _walk("sudoku9_40_all", "ANY"), "allowed ANY, fourth of four", rows=np.arange(11))


def test_one_instance_and_more_instances_than_waves():
    text, roots, dev, budget = _set("queens8_all")
    model = _model(text)
    want = _walk("queens8_all", "ALL")
    _check(_plain(model, dev[:1], "ALL", budget), want, "K = 1")
    resident = model.many_waves(1 << 30)
    K = resident + 65
    big = dev[:1].expand(K, -1, -1).contiguous()
    assert model.many_waves(K) == resident
    got = _plain(model, big, "ALL", budget)
    _check(got, want, f"{K} copies on {resident} waves", rows=np.zeros(K, dtype=np.int64))
    two = _upto(model, big, 2, budget)
    _check(two, _walk("queens8_all", k=2), "copies, up to 2", rows=np.zeros(K, dtype=np.int64))


def test_the_sets_plan_every_shipped_instantiation():
    from test_solve_many_allowed_host import shipped_allowed_kernels
    plain, upto = set(), set()
    for name in many_allowed_sets.SETS:
        model = _model(_set(name)[0])
        plain.add(model.many_allowed_kernel())
        upto.add(model.many_allowed_upto_kernel())
        assert model.many_kernel() == many_allowed_sets.SETS[name][4].rsplit(",", 1)[0].replace("cs_dive_allowed", "cs_dive_shave") + ">"
    assert plain == shipped_allowed_kernels("cs_dive_allowed") and upto == shipped_allowed_kernels("cs_dive_allowed_upto")
    plan = _model(_set("queens8_all")[0]).plan()
    assert not any(v and "cs_dive_allowed" in v for v in plan.values())  # the plan dictionary is what it was


def test_models_the_walk_does_not_run_are_refused_with_the_reason():
    from csolve_amd import CsolveError, problems
    # kernel 7's model with root domains of 160 values: the width walk runs it, the allowed sets do not hold it
    wide = _model(problems.offsets(20, 160, 1, "ALL"))
    assert wide.qualifies(7) and wide.many_kernel() is not None
    assert not wide.qualifies_many_allowed() and wide.many_allowed_kernel() is None and wide.many_allowed_upto_kernel() is None
    rows = torch.from_numpy(wide.domains()[None].copy()).cuda()
    for use in (lambda r: wide.solve_many(r, "ANY", max_nodes=100, branching="allowed"),
                lambda r: wide.solve_many_upto(r, 2, max_nodes=100, branching="allowed")):
        for r in (rows, rows.cpu().numpy()):
            with pytest.raises(CsolveError, match="more than 128 values") as e:
                use(r)
            assert e.value.code == -4
    assert int(wide.solve_many(rows, "ANY", max_nodes=5)["nodes"][0]) == 5  # (the width call is what it was)
    other = _model(problems.schedule(6, 1))
    assert not other.qualifies(7) and not other.qualifies_many_allowed() and other.many_allowed_kernel() is None
    rows = torch.from_numpy(other.domains()[None].copy()).cuda()
    with pytest.raises(CsolveError, match="does not qualify") as e:
        other.solve_many(rows, "ANY", max_nodes=100, branching="allowed")
    assert e.value.code == -4
