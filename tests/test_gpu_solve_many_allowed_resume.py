"""GPU tests of the allowed-values walk in slices (Model.solve_many_allowed with a pool, resume_many on its answers:
csgpu_solve_many_allowed_checkpointed / _resume and the two up-to-k calls; kernels cs_dive_allowed_resume and
cs_dive_allowed_upto_resume).  The references are the plain allowed calls (the parent's kernels, pinned against the host
walk by test_gpu_solve_many_allowed.py) with the summed budget, and the resumable host walk tests/many_walk_allowed.py for
the content of a checkpoint.  Every set of tests/many_allowed_sets.py: between them all twelve (E, R, NW)."""
import numpy as np
import pytest

import many_allowed_sets
import many_walk
import many_walk_allowed
from test_gpu_solve_many_allowed import SENTINEL, _host, _model, _set

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = many_walk.FIELDS
DONE, LIMIT, BAD_ROOT, BAD_SLOT = 0, 1, 2, 3
MAX_CALLS = 10
# a checkpointed call with the first budget, then resumes while a slot is left (the last budget repeats, MAX_CALLS at most)
SEQUENCES = {"ones": ((1, 1, 1, 1, 1, 1), False),        # six slices of one node: six nodes, most instances at LIMIT
             "growing": ((7, 3, 64, 4096, 1 << 17), True),  # ... until no slot is left: every instance ends
             "short": ((5, 40), False)}                   # the sum stays below the trees: LIMIT
MODES = ["ANY", "ALL", 1, 2, 5]


def _rows_buffer(model, K, k):
    return torch.full((K, k, model.n_vars), SENTINEL, dtype=torch.int32, device="cuda")


def _one_call(model, dev, mode, budget):
    """the plain allowed call (cs_dive_allowed / cs_dive_allowed_upto) -> host arrays"""
    if isinstance(mode, str):
        return _host(model.solve_many(dev, mode, max_nodes=budget, branching="allowed"))
    return _host(model.solve_many_upto(dev, mode, max_nodes=budget, solutions=_rows_buffer(model, dev.shape[0], mode),
                                       branching="allowed"))


def _first_slice(model, dev, mode, budget, pool):
    if isinstance(mode, str):
        return model.solve_many_allowed(dev, mode, max_nodes=budget, checkpoints=pool)
    return model.solve_many_allowed(dev, max_nodes=budget, max_solutions=mode, checkpoints=pool,
                                    solutions=_rows_buffer(model, dev.shape[0], mode))


def _resume(model, out, mode, budget):
    if isinstance(mode, str):
        return model.resume_many(out, max_nodes=budget, objective=mode)
    return model.resume_many(out, max_nodes=budget)


def _sliced(model, dev, mode, budgets, until_done, pool):
    """-> (the answer on the host, the summed budget, calls made)"""
    out = _first_slice(model, dev, mode, budgets[0], pool)
    spent, calls = budgets[0], 1
    rest = list(budgets[1:])
    while bool((out["slot"] >= 0).any()) and (rest or until_done):
        assert calls < MAX_CALLS, "the slices do not come to an end"
        b = rest.pop(0) if rest else budgets[-1]
        _resume(model, out, mode, b)
        spent += b
        calls += 1
    return _host(out), spent, calls


def _same(got, want, label):
    for f in FIELDS + tuple(x for x in ("first", "rows") if x in want):
        assert f in got, (label, f)
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, f"{label}: {f} differs at {bad[0]}: got {got[f][tuple(bad[0])]}, one call {want[f][tuple(bad[0])]}"


@pytest.mark.parametrize("mode", MODES, ids=lambda m: m if isinstance(m, str) else f"k{m}")
@pytest.mark.parametrize("name", sorted(many_allowed_sets.SETS))
def test_slices_equal_the_one_call_with_the_summed_budget(name, mode):
    text, roots, dev, _ = _set(name)
    model = _model(text)
    assert model.many_allowed_resume_kernel() == many_allowed_sets.SETS[name][4].replace("cs_dive_allowed<", "cs_dive_allowed_resume<")
    assert model.many_allowed_upto_resume_kernel() == many_allowed_sets.SETS[name][4].replace("cs_dive_allowed<", "cs_dive_allowed_upto_resume<")
    pool = model.many_checkpoints(len(roots))
    _, objective, k, _, _, _ = many_allowed_sets.SETS[name]
    native = mode == (objective if k is None else k)  # the stop the set's budgets were chosen for: its trees are small
    for seq, (budgets, until_done) in SEQUENCES.items():
        if until_done and not native:  # another stop may meet far larger trees: the first four budgets, then LIMIT
            budgets, until_done = budgets[:4], False
        pool.reset()
        got, spent, calls = _sliced(model, dev, mode, budgets, until_done, pool)
        want = _one_call(model, dev, mode, spent)
        print(f"{name} {mode} {seq}: {calls} calls, {spent} nodes of budget, {int((want['status'] == LIMIT).sum())} at LIMIT")
        _same(got, want, f"{name} {mode} {seq}")
        assert ((got["slot"] >= 0) == (want["status"] == LIMIT)).all()
        if until_done:
            assert (want["status"] != LIMIT).all() and calls >= 2
        if seq == "short" and name in ("sudoku9_40_all", "queens12_two") and mode == "ALL":
            assert (want["status"] == LIMIT).any()
    pool.close()


@pytest.mark.parametrize("budget", [5, 40])
@pytest.mark.parametrize("name", ["queens12_two", "sudoku9_40_all"])
def test_a_checkpoint_holds_the_frames_of_the_host_walk(name, budget):
    text, roots, dev, _ = _set(name)
    model = _model(text)
    pool = model.many_checkpoints(len(roots))
    out = model.solve_many_allowed(dev, "ALL", max_nodes=budget, checkpoints=pool)
    slot = _host(out)["slot"]
    checked = deep = 0
    for i in range(min(len(roots), 10)):
        walk = many_walk_allowed.Walk(text, roots[i])
        part = walk.run(budget)
        assert (slot[i] >= 0) == (part["status"] == LIMIT), i
        if slot[i] < 0:
            continue
        states = model.checkpoint_states(pool, int(slot[i])).cpu().numpy()
        want = walk.open_subtrees()
        assert states.shape[0] == len(walk.frames()) == want.shape[0], (name, i)  # depth + 1
        assert (states == want).all(), (name, i)
        checked += 1
        deep += states.shape[0] - 1 >= 3
    assert checked >= 2
    if budget == 40:
        assert deep >= 1, "a checked slot of depth >= 3"
    pool.close()


def test_a_pool_that_runs_out_gives_one_slot():
    text, roots, dev, _ = _set("sudoku9_40_all")
    model = _model(text)
    plain = _one_call(model, dev, "ALL", 5)
    assert int((plain["status"] == LIMIT).sum()) >= 3
    pool = model.many_checkpoints(1)
    out = model.solve_many_allowed(dev, "ALL", max_nodes=5, checkpoints=pool)
    got = _host(out)
    _same(got, plain, "capacity 1")
    assert sorted(got["slot"][got["slot"] >= 0]) == [0] and (got["slot"] >= -1).all()
    kept = int(np.flatnonzero(got["slot"] == 0)[0])
    assert plain["status"][kept] == LIMIT
    others = torch.from_numpy(np.flatnonzero(got["slot"] < 0)).cuda()
    out["_records"][others] = SENTINEL  # the resume reads and writes the instance with the slot only
    out["first"][others] = SENTINEL
    model.resume_many(out, max_nodes=1 << 12, objective="ALL")
    after = _host(out)
    full = _one_call(model, dev, "ALL", 5 + (1 << 12))
    for f in FIELDS:
        assert after[f][kept] == full[f][kept], f
    assert (after["first"][kept] == full["first"][kept]).all() and after["slot"][kept] == -1
    rest = np.flatnonzero(got["slot"] < 0)
    assert (out["_records"][others].cpu().numpy() == SENTINEL).all() and (after["first"][rest] == SENTINEL).all()
    assert (after["slot"][rest] == -1).all()
    pool.close()


def _untouched(before, after, but=()):
    for f in before:
        if f not in but:
            assert (before[f] == after[f]).all(), f


def test_slots_of_the_two_walks_refuse_each_other():
    text, roots, dev, _ = _set("sudoku9_40_all")
    model = _model(text)
    K = len(roots)
    pool_a, pool_w = model.many_checkpoints(K + 4), model.many_checkpoints(K + 4)
    a = model.solve_many_allowed(dev, "ALL", max_nodes=5, checkpoints=pool_a)
    w = model.solve_many(dev, "ALL", max_nodes=5, checkpoints=pool_w)
    for out, marked, label in ((a, False, "an allowed slot through csgpu_solve_many_resume"),
                               (w, True, "a width slot through csgpu_solve_many_allowed_resume")):
        before = _host(out)
        stopped = before["slot"] >= 0
        assert stopped.sum() >= 3
        out["_allowed"] = marked  # the other walk's resume call
        model.resume_many(out, max_nodes=100, objective="ALL")
        after = _host(out)
        assert (after["status"][stopped] == BAD_SLOT).all(), label
        assert (after["status"][~stopped] == before["status"][~stopped]).all()
        _untouched(before, after, but=("status",))
        out["_allowed"] = not marked
        out["status"].copy_(torch.from_numpy(before["status"]).cuda())
    # a slot >= capacity and a free slot, through the allowed resume; the stopped neighbours go on
    before = _host(a)
    i, j = np.flatnonzero(before["slot"] >= 0)[:2]
    a["_slots"][int(i)] = K + 4
    a["_slots"][int(j)] = K + 3  # never handed out: it holds no checkpoint
    model.resume_many(a, max_nodes=1 << 12, objective="ALL")
    after = _host(a)
    full = _one_call(model, dev, "ALL", 5 + (1 << 12))
    for t, s in ((i, K + 4), (j, K + 3)):
        assert after["status"][t] == BAD_SLOT and after["slot"][t] == s
        for f in FIELDS[1:] + ("first",):
            assert (after[f][t] == before[f][t]).all(), f
    rest = np.setdiff1d(np.arange(K), [i, j])
    for f in FIELDS + ("first",):
        assert (after[f][rest] == full[f][rest]).all(), f
    # the counts and the fan-outs
    w_slots = w["slot"].contiguous()
    a2 = model.solve_many_allowed(dev, "ALL", max_nodes=5, checkpoints=model.many_checkpoints(K))
    pool_a2, a_slots = a2["_checkpoints"], a2["slot"].contiguous()
    for pool, slots, branching in ((pool_a2, a_slots, "width"), (pool_w, w_slots, "allowed")):
        counts = model.checkpoint_children(pool, slots, branching=branching).cpu().numpy()
        has = slots.cpu().numpy() >= 0
        assert (counts[has] == -1).all() and (counts[~has] == 0).all(), branching
        offsets = torch.arange(K + 1, dtype=torch.int64, device="cuda")  # one row each: nothing may be written
        rows = torch.full((K, model.n_vars, 2), SENTINEL, dtype=torch.int32, device="cuda")
        owner = torch.full((K,), SENTINEL, dtype=torch.int32, device="cuda")
        model.checkpoint_fanout(pool, slots, offsets, K, rows=rows, owner=owner, branching=branching)
        torch.cuda.synchronize()
        assert bool((rows == SENTINEL).all()) and bool((owner == SENTINEL).all()), branching
    # the right call on each: counts
    assert bool((model.checkpoint_children(pool_a2, a_slots, branching="allowed")[a_slots >= 0] > 0).all())
    assert bool((model.checkpoint_children(pool_w, w_slots)[w_slots >= 0] > 0).all())


def test_calls_of_both_walks_queued_on_one_stream_and_more_instances_than_waves():
    text, roots, dev, _ = _set("sudoku9_40_all")
    model = _model(text)
    K = len(roots)
    pool_w, pool_a = model.many_checkpoints(K), model.many_checkpoints(K)
    torch.cuda.synchronize()
    w = model.solve_many(dev, "ALL", max_nodes=9, checkpoints=pool_w)
    a = model.solve_many_allowed(dev, "ALL", max_nodes=9, checkpoints=pool_a)
    model.resume_many(w, max_nodes=1 << 12, objective="ALL")
    model.resume_many(a, max_nodes=1 << 12, objective="ALL")
    got_w, got_a = _host(w), _host(a)  # the first synchronisation
    _same(got_a, _one_call(model, dev, "ALL", 9 + (1 << 12)), "allowed, queued")
    _same(got_w, _host(model.solve_many(dev, "ALL", max_nodes=9 + (1 << 12))), "width, queued")
    assert (got_a["nodes"] != got_w["nodes"]).any()
    # resident waves + 65 instances, budget 3, resumed to the end
    text, roots, dev, budget = _set("queens8_all")
    model = _model(text)
    resident = model.many_waves(1 << 30)
    big = dev[:1].expand(resident + 65, -1, -1).contiguous()
    pool = model.many_checkpoints(resident + 65)
    out = model.solve_many_allowed(big, "ALL", max_nodes=3, checkpoints=pool)
    assert bool((out["slot"] >= 0).all())
    model.resume_many(out, max_nodes=budget, objective="ALL")
    want = _one_call(model, big, "ALL", 3 + budget)
    _same(_host(out), want, "more instances than waves")
    assert (want["status"] == DONE).all() and (want["solutions"] == 92).all()
    # the ticket counters are left at zero: a plain call of either walk gives its usual answer
    again = _one_call(model, dev, "ALL", budget)
    assert again["solutions"][0] == 92 and again["nodes"][0] == want["nodes"][0]
    assert int(model.solve_many(dev, "ALL", max_nodes=1 << 14)["solutions"][0]) == 92


def test_bad_solved_and_inconsistent_rows_among_stopping_neighbours():
    text, roots, dev, _ = _set("sudoku9_40_all")
    model = _model(text)
    batch = roots[:7].copy()
    batch[1, 40] = (1, 10)  # outside the root domains
    batch[3, 7] = (6, 5)    # lo > hi
    solved = _one_call(model, dev[:7], "ANY", 1 << 12)["first"][4]
    batch[4] = np.stack([solved, solved], 1)  # a complete consistent row
    clash = np.flatnonzero(roots[5, :9, 0] != roots[5, :9, 1])[:2]
    batch[5, clash] = 5     # an inconsistent root
    bdev = torch.from_numpy(batch).cuda()
    for mode in ("ALL", 2):
        plain = _one_call(model, bdev, mode, 1)
        assert list(plain["status"][[1, 3, 4, 5]]) == [BAD_ROOT, BAD_ROOT, DONE, DONE] and (plain["status"][[0, 2, 6]] == LIMIT).sum() >= 2
        pool = model.many_checkpoints(7)
        out = _first_slice(model, bdev, mode, 1, pool)
        got = _host(out)
        _same(got, plain, f"special rows, {mode}")
        assert (got["slot"][[1, 3, 4, 5]] == -1).all() and ((got["slot"] >= 0) == (plain["status"] == LIMIT)).all()
        _resume(model, out, mode, 1 << 12)
        _same(_host(out), _one_call(model, bdev, mode, 1 + (1 << 12)), f"special rows resumed, {mode}")
        pool.close()


def test_models_and_pools_the_calls_do_not_take_are_refused_with_the_reason():
    from csolve_amd import CsolveError, problems
    wide = _model(problems.offsets(20, 160, 1, "ALL"))  # kernel 7's model, root domains of 160 values
    assert wide.qualifies(7) and wide.many_allowed_resume_kernel() is None and wide.many_allowed_upto_resume_kernel() is None
    rows = torch.from_numpy(wide.domains()[None].copy()).cuda()
    pool = wide.many_checkpoints(2)
    for use in (lambda: wide.solve_many_allowed(rows, "ANY", max_nodes=100, checkpoints=pool),
                lambda: wide.solve_many_allowed(rows, max_nodes=100, max_solutions=2, checkpoints=pool),
                lambda: wide.solve_many_spread(rows, branching="allowed"),
                lambda: wide.checkpoint_children(pool, torch.zeros(1, dtype=torch.int32, device="cuda"), branching="allowed")):
        with pytest.raises(CsolveError, match="more than 128 values") as e:
            use()
        assert e.value.code == -4
    w = wide.solve_many(rows, "ANY", max_nodes=5, checkpoints=pool)  # (the width calls are what they were)
    assert int(w["nodes"][0]) == 5 and int(w["slot"][0]) == 0
    w["_allowed"] = True
    with pytest.raises(CsolveError, match="more than 128 values"):
        wide.resume_many(w, max_nodes=5)
    # a clause-kind pool
    text, _, dev, _ = _set("queens8_all")
    model = _model(text)
    if model.qualifies_many_clauses():
        cpool = model.many_clause_checkpoints(2)
        slots = torch.zeros(1, dtype=torch.int32, device="cuda")
        for use in (lambda: model.solve_many_allowed(dev, "ALL", max_nodes=5, checkpoints=cpool),
                    lambda: model.checkpoint_children(cpool, slots, branching="allowed"),
                    lambda: model.checkpoint_fanout(cpool, slots, torch.zeros(2, dtype=torch.int64, device="cuda"), 1,
                                                    branching="allowed")):
            with pytest.raises(CsolveError) as e:
                use()
            assert e.value.code == -1
