"""GPU tests of Model.solve_many_upto (cs_dive_upto: csgpu_solve_many_upto, _upto_checkpointed, _upto_resume): every field
and every solution row of every instance against the host walk of tests/many_walk_upto.py, which asks the oracle for every
node; k = 1 against the ANY call and a k above every count against the ALL call; the budget; slices; a slice with a
smaller k; rows that are not searched; the two families queued on one stream; classify_many; the export of a checkpoint.
Rows that must stay untouched are pre-filled with a sentinel.  Every call passes a finite max_nodes."""
import numpy as np
import pytest

import many_sets
import many_upto_sets
import many_walk
import many_walk_upto

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = many_walk_upto.FIELDS
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
    """(text, roots, roots on the device), built once"""
    text, roots = many_upto_sets.build(name)
    if name not in _devs:
        _devs[name] = torch.from_numpy(roots).cuda()
    return text, roots, _devs[name]


def _buffer(K, k, n):
    return torch.full((K, k, n), SENTINEL, dtype=torch.int32, device="cuda")


def _host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


def _run(model, dev, k, budget, checkpoints=None):
    out = model.solve_many_upto(dev, k, max_nodes=budget, solutions=_buffer(dev.shape[0], k, model.n_vars),
                                checkpoints=checkpoints)
    return out, _host(out)


def _check(got, want, label, rows=None):
    """every field of every instance; row j of an instance for j < its solutions; the sentinel in every row behind them"""
    idx = np.arange(len(want["status"])) if rows is None else np.asarray(rows)
    for f in FIELDS:
        g, w = got[f].astype(np.int64), want[f][idx]
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, walk {w[bad[0]]}"
    if "rows" in got:
        k = got["rows"].shape[1]
        count = want["solutions"][idx]
        there = np.arange(k)[None, :] < count[:, None]
        assert (got["rows"][there] == want["rows"][idx][:, :k][there]).all(), f"{label}: solution rows differ"
        assert (got["rows"][~there] == SENTINEL).all(), f"{label}: a row behind an instance's solutions was written"


CASES = [(name, k) for name in sorted(many_upto_sets.SETS) for k in many_upto_sets.SETS[name][1]]


@pytest.mark.parametrize("name,k", CASES)
def test_every_field_and_row_equals_the_walk(name, k):
    text, roots, dev = _set(name)
    budget = many_upto_sets.SETS[name][2]
    want = many_upto_sets.walk(name, k)
    assert (want["status"] == DONE).all() and want["nodes"].max() < budget, "the set must stay below its budget"
    model = _model(text)
    assert model.many_upto_kernel() == many_upto_sets.SETS[name][3]
    assert model.many_kernel() == many_upto_sets.SETS[name][3].replace("cs_dive_upto", "cs_dive_shave")  # as it was
    _, got = _run(model, dev, k, budget)
    print(f"{name}, k = {k}: {len(roots)} instances, largest tree {int(want['nodes'].max())} nodes, "
          f"solutions per instance {dict(zip(*map(np.ndarray.tolist, np.unique(want['solutions'], return_counts=True))))}")
    _check(got, want, f"{name}, k = {k}")
    assert (got["solutions"] <= k).all()


@pytest.mark.parametrize("name", ["sudoku9", "queens12_two"])
def test_k_1_is_the_any_call(name):
    text, roots, dev = _set(name)
    model = _model(text)
    budget = many_upto_sets.SETS[name][2]
    want = _host(model.solve_many(dev, "ANY", max_nodes=budget))
    got = _host(model.solve_many_upto(dev, 1, max_nodes=budget))
    for f in FIELDS:
        assert (got[f] == want[f]).all(), f
    assert got["rows"].shape == (len(roots), 1, model.n_vars) and (got["rows"][:, 0] == want["first"]).all()
    assert (want["solutions"] == 1).any()


def test_a_k_above_every_count_is_the_all_call():
    text, roots, objective, budget = many_sets.build("sudoku9_all")
    model = _model(text)
    dev = torch.from_numpy(roots).cuda()
    want = _host(model.solve_many(dev, "ALL", max_nodes=budget))
    assert (want["status"] == DONE).all()
    k = int(want["solutions"].max()) + 1
    print(f"sudoku9_all: at most {k - 1} solutions per instance")
    assert k > 2
    _, got = _run(model, dev, k, budget)
    for f in FIELDS:
        assert (got[f] == want[f]).all(), f
    has = want["solutions"] > 0
    assert (got["rows"][has, 0] == want["first"][has]).all()
    there = np.arange(k)[None, :] < want["solutions"][:, None]
    assert (got["rows"][~there] == SENTINEL).all() and (got["rows"][there] != SENTINEL).all()
    # the rows of an instance are different solutions
    i = int(np.argmax(want["solutions"]))
    assert len({r.tobytes() for r in got["rows"][i, : k - 1]}) == k - 1


def test_the_budget_stops_an_instance_with_the_rows_it_has():
    text, roots, dev = _set("deep")
    _, k, budget, kernel, largest = many_upto_sets.DEEP
    model = _model(text)
    assert model.many_upto_kernel() == kernel
    full = many_upto_sets.walk("deep", k)
    assert (full["status"] == DONE).all() and full["nodes"].max() <= largest < budget
    _, got = _run(model, dev, k, budget)
    _check(got, full, "deep, whole")
    want = many_upto_sets.walk("deep", k, 50)
    over = full["nodes"] > 50
    assert over.sum() >= 8 and (~over).any(), "the budget must split the set"
    assert (want["solutions"][over] > 0).any(), "a stopped instance must hold a solution already"
    _, got = _run(model, dev, k, 50)
    _check(got, want, "deep, budget 50")
    assert (got["status"][over] == LIMIT).all() and (got["nodes"][over] == 50).all()
    for f in FIELDS:  # those below the budget are as without it
        assert (got[f][~over] == full[f][~over]).all(), f


def _slots_are_sound(got, capacity, label):
    stopped = got["status"] == LIMIT
    assert ((got["slot"] >= 0) == stopped).all(), f"{label}: a slot without a stop, or a stop without a slot"
    used = got["slot"][stopped]
    assert len(set(used.tolist())) == len(used) and (used < capacity).all(), f"{label}: slots {used}"


def test_slices_equal_the_whole():
    text, roots, dev = _set("deep")
    k = many_upto_sets.DEEP[1]
    model = _model(text)
    K = len(roots)
    _, whole = _run(model, dev, k, 1 << 14)
    pool = model.many_checkpoints(K)
    total, stopped = 0, []
    for step, b in enumerate((1, 7, 56, 16320)):
        if step == 0:
            out, got = _run(model, dev, k, b, checkpoints=pool)
        else:
            assert model.resume_many(out, max_nodes=b) is out
            got = _host(out)
        total += b
        _check(got, many_upto_sets.walk("deep", k, total), f"deep after {total} nodes in slices")
        _slots_are_sound(got, K, f"deep after {total}")
        stopped.append(int((got["status"] == LIMIT).sum()))
    print(f"deep: {K} instances, stopped after each slice: {stopped}")
    assert stopped[0] > 0 and stopped[2] > 0 and stopped[3] == 0 and (got["slot"] == -1).all()
    for f in FIELDS + ("rows",):
        assert (got[f] == whole[f]).all(), f
    # Model.solve_many_sliced drives the same calls
    sliced = model.solve_many_sliced(dev, budgets=(1, 7, 56, 16320), max_solutions=k)
    assert sliced["sliced"] == {"slices": 4, "searched": 0}
    again = _host(sliced)
    for f in FIELDS:
        assert (again[f] == whole[f]).all(), f
    there = np.arange(k)[None, :] < whole["solutions"][:, None]
    assert (again["rows"][there] == whole["rows"][there]).all() and (again["rows"][~there] == 0).all()


def test_more_instances_than_waves_in_slices_without_the_host():
    text, roots, dev = _set("deep")
    k = many_upto_sets.DEEP[1]
    model = _model(text)
    resident = model.many_waves(1 << 30)
    reps = -(-4 * resident // len(roots))
    big = dev.repeat(reps, 1, 1).contiguous()
    K = big.shape[0]
    assert model.many_waves(K) == resident and K >= 4 * resident
    _, want = _run(model, dev, k, 1 << 14)
    _check(want, many_upto_sets.walk("deep", k), "deep, one call")
    pool = model.many_checkpoints(K)
    print(f"{K} instances on {resident} waves, pool of {K * model.checkpoint_bytes() >> 20} MiB")
    rows = _buffer(K, k, model.n_vars)
    torch.cuda.synchronize()
    out = model.solve_many_upto(big, k, max_nodes=1, solutions=rows, checkpoints=pool)
    for b in (7, 56, 16320):
        model.resume_many(out, max_nodes=b)
    got = _host(out)
    for f in FIELDS + ("rows",):
        tiled = np.tile(want[f], (reps,) + (1,) * (want[f].ndim - 1))
        bad = np.flatnonzero((got[f] != tiled).reshape(K, -1).any(axis=1))
        assert bad.size == 0, f"{f} differs for {bad.size} instances, first {bad[0]}"
    assert (got["slot"] == -1).all()


def test_a_resume_with_a_smaller_k_ends_the_instances_that_hold_it():
    text, roots, dev = _set("deep")
    k = many_upto_sets.DEEP[1]
    model = _model(text)
    K = len(roots)
    pool = model.many_checkpoints(K)
    out, before = _run(model, dev, k, 50, checkpoints=pool)
    _check(before, many_upto_sets.walk("deep", k, 50), "deep, budget 50, with a pool")
    stopped = before["status"] == LIMIT
    holds = stopped & (before["solutions"] >= 1)
    goes_on = stopped & (before["solutions"] == 0)
    assert holds.sum() >= 2 and goes_on.sum() >= 2, "both kinds of instance must be there"
    model.resume_many(out, max_nodes=1 << 14, max_solutions=1)
    got = _host(out)
    assert got["rows"].shape == (K, k, model.n_vars)
    # those that held a solution: DONE, no node tried, the slot given back, rows and sentinels as they were
    assert (got["status"][holds] == DONE).all() and (got["slot"][holds] == -1).all()
    for f in FIELDS[1:] + ("rows",):
        assert (got[f][holds] == before[f][holds]).all(), f
    # everything that was not stopped is as it was
    for f in FIELDS + ("rows", "slot"):
        assert (got[f][~stopped] == before[f][~stopped]).all(), f
    # and the whole equals the host's stop-and-continue walk
    want = many_walk_upto.dive_many_upto(text, roots, k, slices=[(50, k), (1 << 14, 1)])
    _check(got, want, "k = 4 to 50 nodes, then k = 1")
    assert (got["status"] == DONE).all() and (got["solutions"][goes_on] <= 1).all()
    assert (got["nodes"][goes_on] > 50).all()


def test_bad_and_trivial_rows_leave_their_neighbours_alone():
    text, roots, dev = _set("sudoku9")
    model = _model(text)
    k, budget = 2, many_upto_sets.SETS["sudoku9"][2]
    want = many_upto_sets.walk("sudoku9", k)
    batch = roots[:7].copy()
    batch[1, 40] = (1, 10)  # outside the root domains
    batch[3, 7] = (6, 5)    # lo > hi
    solved = want["rows"][4, 0]
    batch[4] = np.stack([solved, solved], 1)  # a fully given solved sudoku
    free = np.flatnonzero(roots[5, :, 0] != roots[5, :, 1])
    peer = next(int(v) for v in free[1:] if v // 9 == free[0] // 9)  # two cells of one row with the same value
    batch[5, free[0]] = batch[5, peer] = (3, 3)
    walked = many_walk_upto.dive_many_upto(text, batch, k, budget)
    assert walked["status"].tolist() == [DONE, BAD_ROOT, DONE, BAD_ROOT, DONE, DONE, DONE]
    assert (walked["nodes"][4], walked["solutions"][4]) == (0, 1) and (walked["rows"][4, 0] == solved).all()
    assert (walked["nodes"][5], walked["solutions"][5], walked["root_props"][5]) == (0, 0, 0)
    for i in (0, 2, 6):  # the neighbours are the instances they are alone
        assert all(walked[f][i] == want[f][i] for f in FIELDS) and (walked["rows"][i] == want["rows"][i]).all()
    _, got = _run(model, torch.from_numpy(batch).cuda(), k, budget)
    _check(got, walked, "bad and trivial rows")
    without = _host(model.solve_many_upto(torch.from_numpy(batch).cuda(), k, max_nodes=budget, solutions=False))
    assert "rows" not in without  # d_solutions == NULL
    for f in FIELDS:
        assert (without[f] == walked[f]).all(), f
    empty = model.solve_many_upto(torch.empty((0, model.n_vars, 2), dtype=torch.int32, device="cuda"), 3, max_nodes=5)
    assert empty["status"].shape == (0,) and empty["rows"].shape == (0, 3, model.n_vars)


def test_both_families_queued_on_one_stream():
    """solve_many (ANY), solve_many_upto, solve_many (ALL) back to back, no synchronisation in between: each equals its
    stand-alone answer, so every call left the ticket counters at zero"""
    text, roots, dev = _set("sudoku9")
    model = _model(text)
    budget = many_upto_sets.SETS["sudoku9"][2]
    K = len(roots)
    alone_any = _host(model.solve_many(dev, "ANY", max_nodes=budget))
    _, alone_upto = _run(model, dev[: K // 3].contiguous(), 3, budget)
    alone_all = _host(model.solve_many(dev, "ALL", max_nodes=budget))
    part = dev[: K // 3].contiguous()
    rows = _buffer(K // 3, 3, model.n_vars)
    torch.cuda.synchronize()
    a = model.solve_many(dev, "ANY", max_nodes=budget)
    b = model.solve_many_upto(part, 3, max_nodes=budget, solutions=rows)
    c = model.solve_many(dev, "ALL", max_nodes=budget)
    d = model.solve_many_upto(dev, 2, max_nodes=budget, solutions=_buffer(K, 2, model.n_vars))
    a, b, c, d = _host(a), _host(b), _host(c), _host(d)
    for got, want, fields in ((a, alone_any, FIELDS + ("first",)), (b, alone_upto, FIELDS + ("rows",)),
                              (c, alone_all, FIELDS + ("first",))):
        for f in fields:
            assert (got[f] == want[f]).all(), f
    _check(b, many_upto_sets.walk("sudoku9", 3), "second of four", rows=np.arange(K // 3))
    _check(d, many_upto_sets.walk("sudoku9", 2), "fourth of four")


def test_classify_many():
    text, roots, dev = _set("sudoku9")
    model = _model(text)
    budget = many_upto_sets.SETS["sudoku9"][2]
    cls = model.classify_many(dev, max_nodes=budget)
    assert cls.dtype == torch.int8 and tuple(cls.shape) == (len(roots),)
    cls = cls.cpu().numpy()
    want = many_upto_sets.walk("sudoku9", 2)
    assert (cls == want["solutions"]).all()
    assert [int((cls == c).sum()) for c in (0, 1, 2)] == [0, 13, 51]
    tiny = many_upto_sets.walk("sudoku9", 2, 5)
    short = tiny["status"] == LIMIT
    assert short.any() and (~short).any()
    got = model.classify_many(dev, max_nodes=5).cpu().numpy()
    assert ((got == -1) == short).all() and (got[~short] == want["solutions"][~short]).all()
    bad = roots[:3].copy()
    bad[1, 0] = (0, 9)
    assert model.classify_many(torch.from_numpy(bad).cuda(), max_nodes=budget).cpu().numpy().tolist() == [int(cls[0]), -2, int(cls[2])]


def test_checkpoint_states_of_the_new_call_are_the_open_subtrees_of_the_host_walk():
    text, roots, dev = _set("deep")
    k = many_upto_sets.DEEP[1]
    model = _model(text)
    stopped = np.flatnonzero(many_upto_sets.walk("deep", k, 50)["status"] == LIMIT)
    i = int(stopped[0])
    walk = many_walk_upto.WalkUpto(text, roots[i])
    assert walk.run(50, k)["status"] == LIMIT
    pool = model.many_checkpoints(1)
    out, got = _run(model, dev[i:i + 1].contiguous(), k, 50, checkpoints=pool)
    assert got["status"][0] == LIMIT and got["slot"][0] == 0
    want = walk.open_subtrees()
    states = model.checkpoint_states(pool, 0)
    assert tuple(states.shape) == (len(walk.stack) + 1, model.n_vars, 2)
    assert (states.cpu().numpy() == want).all()


def test_the_sets_launch_every_shipped_upto_instantiation():
    from test_solve_many_upto_host import shipped_upto_kernels
    planned = set()
    for name in many_upto_sets.SETS:
        planned.add(_model(many_upto_sets.build(name)[0]).many_upto_kernel())
    assert planned == shipped_upto_kernels() and len(planned) == 6
    plan = _model(many_upto_sets.build("queens12_two")[0]).plan()
    assert not any(v and "cs_dive_upto" in v for v in plan.values())  # the plan dictionary is what it was
