"""GPU tests of Model.solve_many_restarts (cs_dive_restart, csgpu_solve_many_restarts): every field, the restart count and
the solution row of every instance against the host walk of tests/many_walk_restarts.py, which asks the oracle for every
node; base 0 without flags against the ANY call; seeds per instance; ROTATE_FIRST as a sampler; the budget; queued
calls; rows that are not searched; the optional outputs.  Rows that must stay untouched are pre-filled with a sentinel.
Every call passes a finite max_nodes."""
import numpy as np
import pytest

import many_restart_sets
import many_walk_restarts

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = many_walk_restarts.FIELDS
ALL = FIELDS + ("restarts",)
DONE, LIMIT, BAD_ROOT = 0, 1, 2
SENTINEL = -7
_models = {}
_devs = {}


def _model(text):
    from csolve_amd.solver import solve_root
    if text not in _models:
        _models[text] = solve_root(text)
    return _models[text]


def _set(name):
    """(text, roots, roots on the device, seeds), built once"""
    text, roots, seeds = many_restart_sets.build(name)
    if name not in _devs:
        _devs[name] = torch.from_numpy(roots).cuda()
    return text, roots, _devs[name], seeds


def _host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


def _run(model, dev, base, budget, **kw):
    rows = torch.full((dev.shape[0], model.n_vars), SENTINEL, dtype=torch.int32, device="cuda")
    return _host(model.solve_many_restarts(dev, max_nodes=budget, restart_base=base, solutions=rows, **kw))


def _check(got, want, label, rows=None):
    """every field and the restarts of every instance; the solution row of an instance that has one, the sentinel elsewhere"""
    idx = np.arange(len(want["status"])) if rows is None else np.asarray(rows)
    for f in ALL:
        g, w = got[f].astype(np.int64), want[f][idx]
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, walk {w[bad[0]]}"
    has = want["solutions"][idx] > 0
    assert (got["first"][has] == want["first"][idx][has]).all(), f"{label}: solution rows differ"
    assert (got["first"][~has] == SENTINEL).all(), f"{label}: the row of an instance without a solution was written"


CASES = [(name, base) for name in sorted(many_restart_sets.SETS) for base in many_restart_sets.SETS[name][1]]


@pytest.mark.parametrize("name,base", CASES)
def test_every_field_restarts_and_row_equal_the_walk(name, base):
    text, roots, dev, seeds = _set(name)
    _, _, _, budget, kernel, recorded = many_restart_sets.SETS[name]
    want = many_restart_sets.walk(name, base)
    assert (want["status"] == DONE).all() and want["nodes"].max() < budget, "the set must stay below its budget"
    assert (want["restarts"] > 0).sum() == recorded[base][1] > 0, "the set must restart"
    model = _model(text)
    assert model.many_restart_kernel() == kernel
    assert model.many_kernel() == kernel.replace("cs_dive_restart", "cs_dive_shave")  # as it was
    got = _run(model, dev, base, budget, seed=many_restart_sets.SEED, seeds=seeds)
    print(f"{name}, base {base}: {len(roots)} instances, largest walk {int(want['nodes'].max())} nodes, "
          f"{int((want['restarts'] > 0).sum())} restarted, at most {int(want['restarts'].max())} times")
    _check(got, want, f"{name}, base {base}")


def test_base_0_without_flags_is_the_any_call():
    text, roots, dev, _ = _set("sudoku9")
    model = _model(text)
    budget = many_restart_sets.SETS["sudoku9"][3]
    want = model.solve_many(dev, "ANY", max_nodes=budget)
    got = model.solve_many_restarts(dev, max_nodes=budget, restart_base=0, seed=99)
    torch.cuda.synchronize()
    # every field of the records, and the rows
    assert torch.equal(torch.stack([got[f].long() for f in FIELDS]), torch.stack([want[f].long() for f in FIELDS]))
    assert torch.equal(got["first"], want["first"]) and (got["restarts"] == 0).all()
    assert (want["status"] == DONE).all() and (want["solutions"] == 1).all()
    # a budget below the largest walk stops both at the same node
    small_a = _host(model.solve_many(dev, "ANY", max_nodes=20))
    small_r = _host(model.solve_many_restarts(dev, max_nodes=20, restart_base=0))
    assert (small_a["status"] == LIMIT).any()
    for f in FIELDS + ("first",):
        assert (small_a[f] == small_r[f]).all(), f


def test_seeds_belong_to_the_instance():
    text, roots, dev, _ = _set("sudoku9")
    model = _model(text)
    budget, base, K = many_restart_sets.SETS["sudoku9"][3], 1, 24
    part = dev[:K].contiguous()
    seeds = np.array([1, 2, 3, 2 ** 32 - 1] * (K // 4), dtype=np.uint32)
    want = many_walk_restarts.dive_many_restarts(text, roots[:K], base, seeds=seeds, max_nodes=budget)
    assert (want["restarts"] > 0).sum() >= 8
    got = _run(model, part, base, budget, seeds=seeds)
    _check(got, want, "seeds per instance")
    # equals separate calls with a single seed (d_seeds == NULL: options->seed)
    differ = 0
    for s in (1, 2, 3, 2 ** 32 - 1):
        one = _run(model, part, base, budget, seed=s)
        mine = np.flatnonzero(seeds == s)
        for f in ALL + ("first",):
            assert (one[f][mine] == got[f][mine]).all(), (s, f)
        differ += int((one["nodes"] != got["nodes"]).sum())
    assert differ > 0, "the seed must matter"
    # a permutation of rows and seeds permutes the answers
    perm = np.random.default_rng(5).permutation(K)
    shuffled = _run(model, part[torch.from_numpy(perm).cuda()].contiguous(), base, budget, seeds=seeds[perm])
    for f in ALL + ("first",):
        assert (shuffled[f] == got[f][perm]).all(), f
    # seeds as a device tensor
    again = _run(model, part, base, budget, seeds=torch.from_numpy(seeds.view(np.int32)).cuda())
    for f in ALL + ("first",):
        assert (again[f] == got[f]).all(), f


def test_rotate_first_samples_distinct_valid_grids():
    base, seeds, budget, largest = many_restart_sets.SAMPLER
    text, roots, dev, sd = _set("sampler")
    model = _model(text)
    want = many_restart_sets.walk("sampler", base, rotate_first=True)
    assert want["nodes"].max() == largest < budget
    got = _run(model, dev, base, budget, seeds=sd, rotate_first=True)
    _check(got, want, "sampler")
    grids = got["first"].reshape(-1, 9, 9)
    digits = np.arange(1, 10)
    for g in grids:  # valid sudokus
        assert (np.sort(g, 1) == digits).all() and (np.sort(g.T, 1) == digits).all()
        assert all((np.sort(g[r:r + 3, c:c + 3].ravel()) == digits).all() for r in (0, 3, 6) for c in (0, 3, 6))
    assert len({g.tobytes() for g in grids}) >= 16
    # without the flag and without restarts every seed walks the ascending walk: one grid
    plain = _run(model, dev[:4].contiguous(), 0, budget, seeds=sd[:4])
    assert len({g.tobytes() for g in plain["first"]}) == 1 and (plain["restarts"] == 0).all()


def test_the_budget_counts_all_runs():
    text, roots, dev, _ = _set("sudoku9")
    model = _model(text)
    full = many_restart_sets.walk("sudoku9", 1)
    for budget in (100, 37):
        want = many_restart_sets.walk("sudoku9", 1, max_nodes=budget)
        over = full["nodes"] > budget
        assert over.sum() >= 4 and (~over).any(), "the budget must split the set"
        assert (want["status"][over] == LIMIT).all() and (want["nodes"][over] == budget).all()
        assert (want["restarts"][over] > 0).any(), "a stopped instance must have restarted"
        got = _run(model, dev, 1, budget, seed=many_restart_sets.SEED)
        _check(got, want, f"sudoku9, base 1, budget {budget}")
        assert (got["status"][over] == LIMIT).all() and (got["nodes"][over] == budget).all()
        assert (got["first"][over] == SENTINEL).all()
        for f in ALL:  # those below the budget are as without it
            assert (got[f][~over] == full[f][~over]).all(), f


def test_more_instances_than_waves_and_calls_queued_without_the_host():
    text, roots, dev, _ = _set("sudoku9")
    model = _model(text)
    budget = many_restart_sets.SETS["sudoku9"][3]
    want = many_restart_sets.walk("sudoku9", 8)
    resident = model.many_waves(1 << 30)
    reps = -(-4 * resident // len(roots))
    big = dev.repeat(reps, 1, 1).contiguous()
    K = big.shape[0]
    assert model.many_waves(K) == resident and K >= 4 * resident
    print(f"{K} instances on {resident} waves")
    torch.cuda.synchronize()
    a = model.solve_many_restarts(big, max_nodes=budget, restart_base=8, seed=many_restart_sets.SEED)
    b = model.solve_many_restarts(big, max_nodes=budget, restart_base=8, seed=many_restart_sets.SEED)  # queued behind a
    for got in (_host(a), _host(b)):
        for f in ALL + ("first",):
            tiled = np.tile(want[f], (reps,) + (1,) * (want[f].ndim - 1))
            bad = np.flatnonzero((got[f] != tiled).reshape(K, -1).any(axis=1))
            assert bad.size == 0, f"{f} differs for {bad.size} instances, first {bad[0]}"


def test_queued_behind_the_other_families_on_one_stream():
    """solve_many (ANY), solve_many_upto, solve_many_restarts, solve_many (ANY) back to back, no synchronisation in between:
    each equals its stand-alone answer, so every call left the ticket counters at zero and the workspace usable"""
    text, roots, dev, _ = _set("sudoku9")
    model = _model(text)
    budget = many_restart_sets.SETS["sudoku9"][3]
    alone_any = _host(model.solve_many(dev, "ANY", max_nodes=budget))
    alone_upto = _host(model.solve_many_upto(dev, 2, max_nodes=budget))
    torch.cuda.synchronize()
    a = model.solve_many(dev, "ANY", max_nodes=budget)
    b = model.solve_many_upto(dev, 2, max_nodes=budget)
    c = model.solve_many_restarts(dev, max_nodes=budget, restart_base=1, seed=many_restart_sets.SEED)
    d = model.solve_many(dev, "ANY", max_nodes=budget)
    e = model.solve_many_restarts(dev, max_nodes=budget, restart_base=8, seed=many_restart_sets.SEED)
    a, b, c, d, e = _host(a), _host(b), _host(c), _host(d), _host(e)
    for got, want, fields in ((a, alone_any, FIELDS + ("first",)), (b, alone_upto, FIELDS + ("rows",)),
                              (d, alone_any, FIELDS + ("first",))):
        for f in fields:
            assert (got[f] == want[f]).all(), f
    for got, base in ((c, 1), (e, 8)):
        want = many_restart_sets.walk("sudoku9", base)
        for f in ALL + ("first",):
            assert (got[f] == want[f]).all(), (base, f)


def test_bad_and_trivial_rows_leave_their_neighbours_alone():
    text, roots, dev, _ = _set("sudoku9")
    model = _model(text)
    budget = many_restart_sets.SETS["sudoku9"][3]
    want = many_restart_sets.walk("sudoku9", 1)
    batch = roots[:7].copy()
    batch[1, 40] = (1, 10)  # outside the root domains
    batch[3, 7] = (6, 5)    # lo > hi
    solved = want["first"][4]
    batch[4] = np.stack([solved, solved], 1)  # a fully given solved sudoku
    free = np.flatnonzero(roots[5, :, 0] != roots[5, :, 1])
    peer = next(int(v) for v in free[1:] if v // 9 == free[0] // 9)  # two cells of one row with the same value
    batch[5, free[0]] = batch[5, peer] = (3, 3)
    walked = many_walk_restarts.dive_many_restarts(text, batch, 1, seed=many_restart_sets.SEED, max_nodes=budget)
    assert walked["status"].tolist() == [DONE, BAD_ROOT, DONE, BAD_ROOT, DONE, DONE, DONE]
    assert (walked["nodes"][4], walked["solutions"][4]) == (0, 1) and (walked["first"][4] == solved).all()
    assert (walked["nodes"][5], walked["solutions"][5], walked["root_props"][5]) == (0, 0, 0)
    assert walked["restarts"][[1, 3, 4, 5]].tolist() == [0, 0, 0, 0]
    for i in (0, 2, 6):  # the neighbours are the instances they are alone
        assert all(walked[f][i] == want[f][i] for f in ALL) and (walked["first"][i] == want["first"][i]).all()
    assert walked["restarts"][[0, 2, 6]].max() > 0
    bdev = torch.from_numpy(batch).cuda()
    got = _run(model, bdev, 1, budget, seed=many_restart_sets.SEED)
    _check(got, walked, "bad and trivial rows")
    # the optional outputs: d_solutions == NULL, d_restarts == NULL, both
    for kw in (dict(solutions=False), dict(restarts=False), dict(solutions=False, restarts=False)):
        out = _host(model.solve_many_restarts(bdev, max_nodes=budget, restart_base=1, seed=many_restart_sets.SEED, **kw))
        assert ("first" in out) == ("solutions" not in kw) and ("restarts" in out) == ("restarts" not in kw)
        for f in out:
            assert (out[f] == (walked[f] if f != "first" else np.where(walked["solutions"][:, None] > 0, walked["first"], 0))).all(), (kw, f)
    empty = model.solve_many_restarts(torch.empty((0, model.n_vars, 2), dtype=torch.int32, device="cuda"), max_nodes=5)
    assert empty["status"].shape == (0,) and empty["first"].shape == (0, model.n_vars) and empty["restarts"].shape == (0,)


def test_models_outside_kernel_7_and_bad_options_are_refused():
    from csolve_amd import CsolveError, problems
    model = _model(problems.schedule(6, 1))
    assert not model.qualifies(7) and model.many_restart_kernel() is None
    rows = torch.from_numpy(model.domains()[None].copy()).cuda()
    with pytest.raises(CsolveError, match="does not qualify") as e:
        model.solve_many_restarts(rows, max_nodes=100)
    assert e.value.code == -4
    text, roots, dev, _ = _set("sudoku9")
    with pytest.raises(CsolveError, match="restart_base") as e:  # a finalized model: still before any launch
        _model(text).solve_many_restarts(dev, max_nodes=100, restart_base=-2)
    assert e.value.code == -1


def test_the_sets_launch_every_shipped_restart_instantiation():
    from test_solve_many_restarts_host import shipped_restart_kernels
    planned = set()
    for name in many_restart_sets.SETS:
        planned.add(_model(many_restart_sets.build(name)[0]).many_restart_kernel())
    assert planned == shipped_restart_kernels() and len(planned) == 6
    plan = _model(many_restart_sets.build("queens12_two")[0]).plan()
    assert not any(v and "cs_dive_restart" in v for v in plan.values())  # the plan dictionary is what it was
