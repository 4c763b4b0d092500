"""GPU tests of the spread of stopped allowed walks (csgpu_many_allowed_checkpoint_children / _fanout, kernels
cs_dive_allowed_children / cs_dive_allowed_fanout; Model.solve_many_spread and solve_many_sliced with
branching="allowed").  The counts and rows against the host helper tests/many_allowed_spread_walk.py on the resumable host
walk; the spread and the finish in a Search against the plain allowed ALL call (the parent's kernel)."""
import numpy as np
import pytest

import many_allowed_spread_walk as spread
import many_walk
import many_walk_allowed
from test_gpu_solve_many_allowed import SENTINEL, _host, _model, _set

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = many_walk.FIELDS
DONE, LIMIT = 0, 1
ROWS = 10  # instances walked on the host as well


@pytest.mark.parametrize("budget", [5, 40])
@pytest.mark.parametrize("name", ["queens12_two", "sudoku9_40_all"])
def test_children_and_fan_out_are_the_host_walks(name, budget):
    text, roots, dev, _ = _set(name)
    model = _model(text)
    K, n = min(len(roots), ROWS), model.n_vars
    pool = model.many_checkpoints(K)
    out = model.solve_many_allowed(dev[:K].contiguous(), "ALL", max_nodes=budget, checkpoints=pool)
    slots = out["slot"].contiguous()
    counts = model.checkpoint_children(pool, slots, branching="allowed").cpu().numpy()
    walks, want_rows, want_owner, fewer = [], [], [], 0
    for i in range(K):
        w = many_walk_allowed.Walk(text, roots[i])
        stopped = w.run(budget)["status"] == LIMIT
        assert (int(slots[i]) >= 0) == stopped
        assert counts[i] == (spread.count_children(w) if stopped else 0), (name, i)
        if stopped:
            assert counts[i] <= spread.width_count(w)
            fewer += counts[i] < spread.width_count(w)
            want_rows.append(spread.children_of(w))
            want_owner += [i] * int(counts[i])
    assert len(want_rows) >= 2
    if name == "sudoku9_40_all":
        assert fewer >= 1, "no slot shows the rule: a count below the width formula's"
    want_rows = np.concatenate(want_rows)
    total = int(counts.sum())
    offsets = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(torch.from_numpy(counts).cuda(), 0)
    rows, owner = model.checkpoint_fanout(pool, slots, offsets, total, branching="allowed")
    torch.cuda.synchronize()
    assert (rows.cpu().numpy() == want_rows).all() and (owner.cpu().numpy() == np.array(want_owner)).all()
    # one offset off by one: that instance and nobody else is left out; `total` too small: the last instance is
    first = int(np.flatnonzero(counts > 0)[0])
    last = int(np.flatnonzero(counts > 0)[-1])
    for wrong, lost in (("offset", first), ("total", last)):
        off2, total2 = offsets.clone(), total
        if wrong == "offset":
            off2[first + 1:] += 1  # instance `first` has one row too many; the rows after it move by one
            total2 = total + 1
        else:
            total2 = total - 1
        buf = torch.full((total + 1, n, 2), SENTINEL, dtype=torch.int32, device="cuda")
        own = torch.full((total + 1,), SENTINEL, dtype=torch.int32, device="cuda")
        model.checkpoint_fanout(pool, slots, off2, total2, rows=buf, owner=own, branching="allowed")
        torch.cuda.synchronize()
        lo, hi = int(off2[lost]), int(off2[lost + 1])
        assert bool((buf[lo:hi] == SENTINEL).all()) and bool((own[lo:hi] == SENTINEL).all()), wrong
        written = (own != SENTINEL).cpu().numpy()
        assert written.sum() == total - counts[lost], wrong
    pool.close()


SPREAD_SETS = ["queens8_all", "queens12_two", "sudoku9_40_all", "sparse40_e16_w16", "sparse40_e16"]  # the last two: NW 1 and 4
_plain = {}


def _one_call(name):
    if name not in _plain:
        text, roots, dev, budget = _set(name)
        _plain[name] = _host(_model(text).solve_many(dev, "ALL", max_nodes=budget, branching="allowed"))
        assert (_plain[name]["status"] == DONE).all()
    return _plain[name]


@pytest.mark.parametrize("budgets", [(2, 8), (16, 64), None], ids=["2-8", "16-64", "default"])
@pytest.mark.parametrize("name", SPREAD_SETS)
def test_the_spread_is_the_one_allowed_call(name, budgets):
    text, roots, dev, _ = _set(name)
    model = _model(text)
    want = _one_call(name)
    more = {} if budgets is None else {"budgets": budgets}
    out = model.solve_many_spread(dev, branching="allowed", **more)
    got = _host(out)
    for f in FIELDS + ("first",):
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, f"{name} {budgets}: {f} differs at {bad[0]}"
    print(f"{name} {budgets}: rounds {out['rounds']}, sub-instances {out['sub_instances']}, rows per round {out['round_rows']}")
    assert out["sub_instances"] == sum(out["round_rows"]) and out["rounds"] == 1 + len(out["round_rows"])
    if budgets == (2, 8) and name in ("queens8_all", "sudoku9_40_all"):
        assert out["rounds"] >= 3 and out["sub_instances"] > 0  # the test cannot pass without splitting


def test_one_round_leaves_the_owners_with_work_at_limit():
    text, roots, dev, _ = _set("sudoku9_40_all")
    model = _model(text)
    want = _one_call("sudoku9_40_all")
    out = model.solve_many_spread(dev, budgets=(8,), max_rounds=1, branching="allowed")
    got = _host(out)
    assert out["rounds"] == 1 and out["sub_instances"] == 0
    stopped = want["nodes"] > 8
    assert stopped.any() and (got["status"] == np.where(stopped, LIMIT, DONE)).all()
    for f in ("nodes", "cuts", "props", "solutions"):
        assert (got[f] <= want[f]).all() and (got[f][~stopped] == want[f][~stopped]).all()
    assert (got["nodes"][stopped] == 8).all()
    two = _host(model.solve_many_spread(dev, budgets=(8, 4), max_rounds=2, branching="allowed"))
    assert (two["status"][stopped] == LIMIT).any() and (two["nodes"] <= want["nodes"]).all() and (two["nodes"] >= got["nodes"]).all()


def test_the_width_spread_is_the_call_it_was():
    text, roots, dev, budget = _set("sudoku9_40_all")
    model = _model(text)
    want = _host(model.solve_many(dev, "ALL", max_nodes=1 << 14))
    got = _host(model.solve_many_spread(dev, budgets=(16, 64)))
    for f in FIELDS + ("first",):
        assert (got[f] == want[f]).all(), f


def test_slices_finished_in_a_search_find_the_solutions_of_the_one_call():
    text, roots, dev, _ = _set("queens8_all")
    model = _model(text)
    want = _one_call("queens8_all")
    out = model.solve_many_sliced(dev, "ALL", budgets=(8,), finish="search", branching="allowed")
    got = _host(out)
    assert out["sliced"]["searched"] == len(roots) >= 1
    assert (got["solutions"] == want["solutions"]).all() and (got["status"] == DONE).all() and (got["slot"] == -1).all()
    # finish="resume": slices alone, field for field
    again = model.solve_many_sliced(dev, "ALL", budgets=(8, 64, 4096), branching="allowed")
    for f in FIELDS + ("first",):
        assert (_host(again)[f] == want[f]).all(), f
    assert again["sliced"] == {"slices": 3, "searched": 0}
    text, roots, dev, budget = _set("sudoku9_25_upto2")
    model = _model(text)
    rows = torch.full((len(roots), 2, model.n_vars), SENTINEL, dtype=torch.int32, device="cuda")
    ref = _host(model.solve_many_upto(dev, 2, max_nodes=8 + 64 + budget, solutions=rows, branching="allowed"))
    rows2 = torch.full_like(rows, SENTINEL)
    upto = _host(model.solve_many_sliced(dev, budgets=(8, 64, budget), max_solutions=2, solutions=rows2, branching="allowed"))
    for f in FIELDS + ("rows",):
        assert (upto[f] == ref[f]).all(), f
