"""GPU tests of Model.solve_many_clauses_stream / Model.solve_many_clauses_all (cs_walk_stream,
csgpu_solve_many_clauses_stream): under ALL every solution of every instance of a clause model goes to one bounded stream,
and an instance the stream has no room for steps back and goes on in the next call.  The reference for status, nodes, cuts,
solutions and the rows in walk order is the host walk of tests/many_walk_clauses_upto.py (Walk(text, row).run(1 << 62,
None)), which asks the oracle for every node; for props and root_props, which kernel 6 counts in its own order, it is the
device's own solve_many_clauses(roots, "ALL").  Which instances find room in a call depends on the order the waves arrive
in: the tests assert only what holds for every order (test_solve_many_clauses_stream_host.py pins that property on a host
model of the call)."""
import functools

import numpy as np
import pytest

import many_clause_stream_sets as ssets
import many_walk_clauses_upto as U

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

COUNTERS = ("status", "nodes", "cuts", "solutions")  # what the host walk promises
OWN = ("props", "root_props")                        # what the counting call of the device promises
DONE, LIMIT, BAD_ROOT, BAD_SLOT, FULL = 0, 1, 2, 3, 4
FRESH = -2
BUDGET = 1 << 40
SENTINEL = -7


@functools.lru_cache(maxsize=None)
def _model(text):
    from csolve_amd.solver import solve_root
    return solve_root(text)


@functools.lru_cache(maxsize=None)
def _set(name):
    """(text, roots, roots on the device), built once"""
    text, roots = ssets.build(name)
    return text, roots, torch.from_numpy(np.array(roots)).cuda()


def _host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


@functools.lru_cache(maxsize=None)
def _counted(name):
    """the device's counting call, solve_many_clauses under ALL with an unlimited budget: the reference for props"""
    text, roots, dev = _set(name)
    return _host(_model(text).solve_many_clauses(dev, "ALL", max_nodes=BUDGET, solutions=False))


def _loop(model, dev, capacity, budget, max_calls, pool=None, first=None, out=None, after=None):
    """call, take the rows, zero the count, until every slot is -1 -- at most max_calls calls, so that a bug cannot spin.
    first: (slots, records, rows per owner so far) to go on from.  after(host answer, rows per owner): called per call.
    -> (the last answer on the host, the rows per owner in the order they were drained, one snapshot per call)"""
    K = dev.shape[0]
    pool = pool if pool is not None else model.many_clause_checkpoints(K)
    out = out if out is not None else model.many_stream(capacity)
    slots, results, per = first if first is not None else (None, None, [[] for _ in range(K)])
    trace = []
    for _ in range(max_calls):
        ans = model.solve_many_clauses_stream(dev, out, pool, slots, results, max_nodes=budget)
        slots, results = ans["_slots"], ans["_records"]
        host = _host(ans)
        attempts = int(out.count.item())
        owner, rows = out.take()
        assert int(out.count.item()) == 0 and owner.shape[0] == min(attempts, capacity)
        for o, r in zip(owner.cpu().numpy(), rows.cpu().numpy()):
            per[o].append(r)
        trace.append(dict(status=host["status"].copy(), slot=host["slot"].copy(), solutions=host["solutions"].copy(),
                          nodes=host["nodes"].copy(), attempts=attempts, taken=int(owner.shape[0])))
        if after is not None:
            after(host, per)
        if (host["slot"] == -1).all():
            return host, per, trace
    raise AssertionError(f"{max_calls} calls and some instance still has work left: slots {host['slot'].tolist()}")


def _check(got, per, want, label, counted=None):
    """every field of every instance; the rows drained for an instance are its walk's rows in walk order, each once"""
    for f in COUNTERS:
        g, w = got[f].astype(np.int64), np.array([d[f] for d in want], dtype=np.int64)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, walk {w[bad[0]]}"
    if counted is not None:
        for f in COUNTERS + OWN:
            bad = np.flatnonzero(got[f] != counted[f])
            assert bad.size == 0, f"{label}: {f} differs from the counting call for {bad.size} instances, first {bad[0]}"
    assert sum(len(r) for r in per) == sum(d["solutions"] for d in want), f"{label}: the number of rows drained"
    for i, d in enumerate(want):
        assert len(per[i]) == len(d["rows"]), f"{label}: instance {i} streamed {len(per[i])} rows, its walk has {len(d['rows'])}"
        if d["rows"]:
            assert (np.stack(per[i]) == np.stack(d["rows"])).all(), f"{label}: the rows of instance {i} are not its walk's, in walk order"


def _per_owner(owner, rows, K, per=None):
    per = per if per is not None else [[] for _ in range(K)]
    for o, r in zip(owner.cpu().numpy(), rows.cpu().numpy()):
        per[o].append(r)
    return per


# 1
@pytest.mark.parametrize("name", sorted(ssets.TABLE))
def test_one_call_with_room_for_everything_equals_the_walk(name):
    text, roots, dev = _set(name)
    want = ssets.walk(name)
    total = sum(d["solutions"] for d in want)
    model = _model(text)
    assert model.many_clauses_stream_kernel() == ssets.kernel(name)
    assert model.many_clauses_kernel() == ssets.kernel(name).replace("cs_walk_stream", "cs_walk_clauses")  # as it was
    K = len(roots)
    pool = model.many_clause_checkpoints(K)
    out = model.many_stream(total + 3)
    out.rows.fill_(SENTINEL)
    out.owner.fill_(SENTINEL)
    got = _host(model.solve_many_clauses_stream(dev, out, pool, max_nodes=BUDGET))
    print(f"{name}: {K} instances, {total} solutions, largest walk {max(d['nodes'] for d in want)} nodes")
    assert (got["status"] == DONE).all() and (got["slot"] == -1).all()
    assert int(out.count.item()) == total == int(got["solutions"].sum()) == ssets.TABLE[name][1]
    assert (out.rows[total:] == SENTINEL).all() and (out.owner[total:] == SENTINEL).all(), "a row behind the stream's end was written"
    owner, rows = out.take()
    owner, rows = owner.cpu().numpy(), rows.cpu().numpy()
    order = np.argsort(owner, kind="stable")  # grouped by owner, in index order within one
    bounds = np.searchsorted(owner[order], np.arange(K + 1))
    per = [list(rows[order[bounds[i]:bounds[i + 1]]]) for i in range(K)]
    _check(got, per, want, name, _counted(name))
    pool.close()


# 2
SMALL = [("tree20_all", 1), ("tree20_all", 7), ("mixed40_any", 1), ("mixed40_any", 7), ("schedule5_classes", 1),
         ("wcet_max", 16), ("linear20_all", 256), ("mixed120_any", 64)]


@pytest.mark.parametrize("name,capacity", SMALL)
def test_small_streams_lose_nothing_and_repeat_nothing(name, capacity):
    text, roots, dev = _set(name)
    want = ssets.walk(name)
    total = sum(d["solutions"] for d in want)
    assert total > capacity
    K = len(roots)
    got, per, trace = _loop(_model(text), dev, capacity, BUDGET, total + K + 2)
    print(f"{name}, capacity {capacity}: {K} instances, {total} solutions, {len(trace)} calls")
    _check(got, per, want, f"{name}, capacity {capacity}", _counted(name))
    assert (got["status"] == DONE).all() and len(trace) > 1
    assert any(((t["status"] == FULL) & (t["slot"] >= 0)).any() for t in trace[:-1]), "no instance stopped FULL with a checkpoint"
    assert all(t["taken"] == capacity for t in trace[:-1] if t["attempts"] > capacity)
    for t in trace:
        assert ((t["slot"] == FRESH) <= (t["status"] == FULL)).all(), "an instance that was not started has status FULL"
        assert ((t["slot"] >= 0) <= (t["status"] == FULL)).all(), "under this budget a checkpoint means FULL"
        assert (t["solutions"][t["slot"] == FRESH] == 0).all() and (t["nodes"][t["slot"] == FRESH] == 0).all()


# 3
def test_budget_and_stream_together():
    """schedule22_min_budget with 64 nodes and 16 rows per call.  After every call an instance that stands at N nodes has
    the counters of the host walk's run(N, None), and the rows drained for it so far are that walk's first `solutions`
    rows -- whichever wave won the race for a row."""
    name = "schedule22_min_budget"
    text, roots, dev = _set(name)
    want = ssets.walk(name)
    K = len(roots)
    assert U.Walk(text, roots[0]).run(64, None)["solutions"] == 39 and U.Walk(text, roots[2]).run(512, None)["solutions"] == 0
    walks = [U.Walk(text, row) for row in roots]  # each walked on to the node count its instance stands at
    at = [0] * K
    seen = {i: set() for i in range(K)}

    def after(host, per):
        for i in range(K):
            status, N = int(host["status"][i]), int(host["nodes"][i])
            seen[i].add(status)
            if status not in (LIMIT, FULL, DONE) or host["slot"][i] == FRESH:
                continue
            assert N >= at[i], f"instance {i} went back from {at[i]} to {N} nodes"
            part = walks[i].run(N - at[i], None) if N > at[i] else walks[i].result()
            at[i] = N
            for f in ("nodes", "cuts", "solutions"):
                assert int(host[f][i]) == part[f], f"instance {i} at {N} nodes: {f} {int(host[f][i])}, walk {part[f]}"
            assert len(per[i]) == part["solutions"], f"instance {i} at {N} nodes: {len(per[i])} rows drained, {part['solutions']} counted"
            assert all((a == b).all() for a, b in zip(per[i], part["rows"])), f"instance {i}: the rows drained are not the walk's first"

    total = sum(d["solutions"] for d in want)
    max_calls = total // 16 + K + 2 + sum(d["nodes"] // 64 + 1 for d in want)
    got, per, trace = _loop(_model(text), dev, 16, 64, max_calls, after=after)
    print(f"{name}, capacity 16, 64 nodes per call: {len(trace)} calls, {total} solutions")
    assert FULL in seen[0] and trace[0]["status"][0] == FULL, "instance 0 finds 39 solutions in its first 64 nodes"
    assert LIMIT in seen[2], "instance 2 finds no solution in its first 512 nodes"
    _check(got, per, want, f"{name}, budget 64, capacity 16", _counted(name))
    assert (got["status"] == DONE).all()


def _sentinel_records(K):
    return torch.full((K, 5), SENTINEL, dtype=torch.int64, device="cuda")


# 4
def test_finished_fresh_and_resumed_instances_in_one_call():
    name = "wcet_max"
    text, roots, dev = _set(name)
    want = ssets.walk(name)
    model = _model(text)
    K = len(roots)
    total = sum(d["solutions"] for d in want)
    pool = model.many_clause_checkpoints(K)
    out = model.many_stream(total)
    records = _sentinel_records(K)
    slots = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    slots[:12] = FRESH
    # call A: the first 12 start with 8 nodes each, the others are finished on entry (-1) and are not touched
    a = _host(model.solve_many_clauses_stream(dev, out, pool, slots, records, max_nodes=8))
    assert (records[12:] == SENTINEL).all() and (a["slot"][12:] == -1).all()
    stopped = np.flatnonzero(a["slot"] >= 0)
    assert stopped.size >= 4 and (a["status"][stopped] == LIMIT).all() and (a["nodes"][stopped] == 8).all()
    assert (stopped < 12).all() and len(set(a["slot"][stopped].tolist())) == stopped.size
    owner, rows = out.take()
    assert (owner < 12).all()
    per = _per_owner(owner, rows, K)
    # call B: those go on from their slots, 8 more start, the rest stay finished -- an entry below -2 is finished too
    slots[12:20] = FRESH
    slots[K - 1] = -5
    records[12:20] = 0
    b = _host(model.solve_many_clauses_stream(dev, out, pool, slots, records, max_nodes=BUDGET))
    assert (records[20:] == SENTINEL).all() and (b["slot"][20:K - 1] == -1).all() and b["slot"][K - 1] == -5
    assert (b["slot"][:20] == -1).all()
    owner, rows = out.take()
    assert (owner < 20).all()
    per = _per_owner(owner, rows, K, per)
    counted = {f: v[:20] for f, v in _counted(name).items()}
    _check({f: b[f][:20] for f in COUNTERS + OWN}, per[:20], want[:20], "fresh and resumed mixed", counted)
    assert not any(per[20:])
    pool.close()


# 5
def test_bad_slots_get_their_status_and_nothing_else():
    name = "wcet_max"
    text, roots, dev = _set(name)
    want = ssets.walk(name)
    model = _model(text)
    K = len(roots)
    deep = [i for i, d in enumerate(want) if d["nodes"] > 8][:4]
    assert len(deep) == 4
    four = dev[deep].contiguous()
    pool = model.many_clause_checkpoints(8)
    # slots 0 .. 3: checkpoints of solve_many_clauses under ALL; a second pool holds those of the up-to-k call
    made = model.solve_many_clauses(four, "ALL", max_nodes=4, checkpoints=pool)
    assert (_host(made)["slot"] >= 0).all()
    upto_pool = model.many_clause_checkpoints(4)
    upto = model.solve_many_clauses_upto(four, 1 << 20, max_nodes=4, solutions=False, checkpoints=upto_pool)
    assert (_host(upto)["slot"] >= 0).all()
    out = model.many_stream(4096)
    out.rows.fill_(SENTINEL)
    i = deep[0]
    for bad_pool, values in ((pool, (8, 1 << 30, 5, int(made["slot"][1]))), (upto_pool, (int(upto["slot"][2]),))):
        for value in values:  # past the pool, far past it, a free slot, an ALL checkpoint; an up-to-k checkpoint
            records = _sentinel_records(2)
            slots = torch.tensor([value, FRESH], dtype=torch.int32, device="cuda")
            got = _host(model.solve_many_clauses_stream(four[:2].contiguous(), out, bad_pool, slots, records, max_nodes=BUDGET))
            assert got["status"].tolist() == [BAD_SLOT, DONE] and got["slot"].tolist() == [value, -1], value
            assert got["root_props"][0] == -1 and all(got[f][0] == SENTINEL for f in ("nodes", "cuts", "props", "solutions"))
            assert all(got[f][1] == want[deep[1]][f] for f in COUNTERS)
            owner, rows = out.take()
            assert (owner == 1).all() and owner.shape[0] == want[deep[1]]["solutions"]
    # the checkpoints the refused calls looked at are intact: their own resumes go on to the end
    done = _host(model.resume_many_clauses(made, max_nodes=BUDGET))
    assert (done["status"] == DONE).all() and all(done["nodes"][j] == want[deep[j]]["nodes"] for j in range(4))
    # the reverse: a stream checkpoint handed to resume_many_clauses (ALL) and to the up-to-k resume
    pool.reset()
    ans = model.solve_many_clauses_stream(four, out, pool, max_nodes=4)
    before = _host(ans)
    out.take()
    had = before["slot"] >= 0
    assert had.all() and (before["status"] == LIMIT).all()
    for extra in ({"_objective": 1, "_best": None}, {"_upto": 5, "rows": torch.full((4, 5, model.n_vars), SENTINEL, dtype=torch.int32, device="cuda")}):
        other = dict(ans)
        other.update(extra)
        model.resume_many_clauses(other, max_nodes=BUDGET)
        got = _host(ans)
        assert (got["status"][had] == BAD_SLOT).all() and (got["status"][~had] == before["status"][~had]).all()
        for f in COUNTERS[1:] + OWN + ("slot",):
            assert (got[f] == before[f]).all(), f
        if "rows" in extra:
            assert (extra["rows"] == SENTINEL).all()
    # and by its own call it goes on: the counters were left alone
    done = _host(model.solve_many_clauses_stream(four, out, pool, ans["_slots"], ans["_records"], max_nodes=BUDGET))
    assert (done["status"] == DONE).all() and (done["slot"] == -1).all()
    assert all(done[f][j] == want[deep[j]][f] for j in range(4) for f in COUNTERS)
    for p in (pool, upto_pool):
        p.close()


# 6
def test_the_library_refuses_what_it_documents():
    from csolve_amd import CsolveError, problems
    text, roots, dev = _set("tree20_all")
    model = _model(text)
    other = _model(_set("wcet_max")[0])
    pool, foreign = model.many_clause_checkpoints(2), other.many_clause_checkpoints(2)
    out = model.many_stream(16)
    with pytest.raises(CsolveError, match="another model") as e:
        model.solve_many_clauses_stream(dev, out, foreign, max_nodes=10)
    assert e.value.code == -1
    queens = _model(problems.queens(8, "ALL"))  # a model of both families
    assert queens.qualifies(7) and queens.qualifies_many_clauses()
    rows = torch.from_numpy(queens.domains()[None].copy()).cuda()
    dive_pool = queens.many_checkpoints(2)
    with pytest.raises(CsolveError, match="other kind") as e:
        queens.solve_many_clauses_stream(rows, queens.many_stream(128), dive_pool, max_nodes=10)
    assert e.value.code == -1
    big = _model(problems.schedule(32, 1))
    assert big.n_clauses > 512 and not big.qualifies_many_clauses() and big.many_clauses_stream_kernel() is None
    rows = np.repeat(big.domains()[None], 2, 0)
    for r in (rows, torch.from_numpy(rows).cuda()):
        with pytest.raises(CsolveError, match="512") as e:  # before the pool is looked at
            big.solve_many_clauses_stream(r, big.many_stream(16), foreign, max_nodes=10)
        assert e.value.code == -4
    with pytest.raises(CsolveError, match="capacity") as e:
        model.solve_many_clauses_stream(dev, model.many_stream(0), pool, max_nodes=10)
    assert e.value.code == -1
    with pytest.raises(CsolveError, match="max_nodes") as e:
        model.solve_many_clauses_stream(dev, out, pool, max_nodes=0)
    assert e.value.code == -1
    # an empty batch launches nothing
    ans = model.solve_many_clauses_stream(dev[:0].contiguous(), out, pool, max_nodes=10)
    assert ans["status"].shape[0] == 0 and int(out.count.item()) == 0
    # the model of both families streams what solve_many_stream streams
    q = torch.from_numpy(np.repeat(queens.domains()[None], 2, 0).copy()).cuda()
    a_out, b_out = queens.many_stream(256), queens.many_stream(256)
    a = _host(queens.solve_many_clauses_stream(q, a_out, queens.many_clause_checkpoints(2), max_nodes=BUDGET))
    b = _host(queens.solve_many_stream(q, b_out, dive_pool, max_nodes=1 << 30))
    for f in COUNTERS:
        assert (a[f] == b[f]).all(), f
    assert a["solutions"].tolist() == [92, 92]
    (ao, ar), (bo, br) = a_out.take(), b_out.take()
    for inst in (0, 1):
        assert (ar[ao == inst] == br[bo == inst]).all()


# 7
def test_a_pool_that_is_too_small_loses_walks_not_rows():
    name = "schedule22_min_budget"
    text, roots, dev = _set(name)
    want = ssets.walk(name)
    model = _model(text)
    K = len(roots)
    assert K == 6
    pool = model.many_clause_checkpoints(2)
    total = sum(d["solutions"] for d in want)
    # 16 nodes per call, fewer than the smallest walk has: no instance ends in the call that starts it, each needs a slot,
    # slots are not handed back, so two instances go on to their end and four lose their walk
    assert min(d["nodes"] for d in want) > 16
    got, per, trace = _loop(model, dev, 16, 16, total // 16 + K + 2 + sum(d["nodes"] // 16 + 1 for d in want), pool=pool)
    drawn = set()
    for t in trace:
        drawn |= set(t["slot"][t["slot"] >= 0].tolist())
    assert drawn == {0, 1}, drawn
    lost = np.flatnonzero(got["status"] != DONE)
    print(f"pool of 2, capacity 16, 16 nodes: {len(trace)} calls, {lost.size} instances lost their walk")
    assert lost.size == 4
    assert (got["slot"] == -1).all()
    counted = _counted(name)
    for i in range(K):
        d = want[i]
        if got["status"][i] == DONE:  # unaffected
            _check({f: got[f][i:i + 1] for f in COUNTERS}, [per[i]], [d], f"instance {i}")
            assert got["props"][i] == counted["props"][i]
        else:  # stopped without a slot: LIMIT / FULL with the counters of that moment, its rows the head of its walk's
            assert got["status"][i] in (LIMIT, FULL)
            part = U.Walk(text, roots[i]).run(int(got["nodes"][i]), None) if got["nodes"][i] else None
            s = int(got["solutions"][i])
            assert len(per[i]) == s and got["nodes"][i] <= 16 and got["root_props"][i] == counted["root_props"][i]
            if part is not None:
                assert part["solutions"] == s and part["cuts"] == got["cuts"][i]
            assert all((a == b).all() for a, b in zip(per[i], d["rows"]))
    pool.close()


# 8
def test_two_calls_queued_without_the_host_between_them():
    name = "linear40_all"
    text, roots, dev = _set(name)
    want = ssets.walk(name)
    model = _model(text)
    K = len(roots)
    total = sum(d["solutions"] for d in want)
    pool = model.many_clause_checkpoints(K)
    out = model.many_stream(total)
    # behind a counting call, and behind each other: the ticket counters come back to zero
    plain = model.solve_many_clauses(dev, "ALL", max_nodes=BUDGET, solutions=False)
    a = model.solve_many_clauses_stream(dev, out, pool, max_nodes=256)
    b = model.solve_many_clauses_stream(dev, out, pool, a["_slots"], a["_records"], max_nodes=256)  # the count is not zeroed
    host = _host(b)
    plain = _host(plain)
    attempts = int(out.count.item())
    owner, rows = out.take()
    assert owner.shape[0] == attempts == int(host["solutions"].sum())
    per = _per_owner(owner, rows, K)
    assert (host["slot"] >= 0).any(), "256 nodes twice do not finish the deep instances"
    assert (host["nodes"][host["slot"] >= 0] == 512).all() and (host["status"][host["slot"] >= 0] == LIMIT).all()
    got, per, trace = _loop(model, dev, total, 256, K + 2 + max(d["nodes"] for d in want) // 256, pool=pool,
                            first=(b["_slots"], b["_records"], per), out=out)
    _check(got, per, want, "two calls queued, then the loop", plain)
    after = _host(model.solve_many_clauses(dev, "ALL", max_nodes=BUDGET, solutions=False))
    for f in COUNTERS + OWN:
        assert (after[f] == got[f]).all(), f
    pool.close()


# 9
def test_a_full_checkpoint_exports_its_open_subtrees():
    name = "wcet_max"
    text, roots, dev = _set(name)
    want = ssets.walk(name)
    model = _model(text)
    K = len(roots)
    pool = model.many_clause_checkpoints(K)
    out = model.many_stream(8)
    got = _host(model.solve_many_clauses_stream(dev, out, pool, max_nodes=BUDGET))
    full = np.flatnonzero((got["status"] == FULL) & (got["slot"] >= 0))
    assert full.size >= 1
    for i in full[:6].tolist():
        w = U.Walk(text, roots[i])
        if got["nodes"][i]:
            w.run(int(got["nodes"][i]), None)
        states, incumbent = model.clause_checkpoint_states(pool, int(got["slot"][i]))
        subtrees = w.open_subtrees()
        assert incumbent is None and tuple(states.shape) == subtrees.shape, i
        assert (states.cpu().numpy() == subtrees).all(), f"instance {i}"
    pool.close()


# 10
def test_solve_many_clauses_all_drives_the_loop():
    from csolve_amd import CsolveError, problems
    name = "tree20_all"
    text, roots, dev = _set(name)
    want = ssets.walk(name)
    model = _model(text)
    K = len(roots)
    counts = np.array([d["solutions"] for d in want])
    every = np.concatenate([np.stack(d["rows"]) for d in want if d["rows"]])
    for stream_rows in (65536, 16):
        ans = model.solve_many_clauses_all(dev, max_nodes=BUDGET, stream_rows=stream_rows)
        got = _host(ans)
        assert (got["offsets"] == np.concatenate([[0], np.cumsum(counts)])).all()
        assert (got["rows"] == every).all(), stream_rows
        for f in COUNTERS:
            assert (got[f] == np.array([d[f] for d in want])).all(), f
        for f in OWN:
            assert (got[f] == _counted(name)[f]).all(), f
        assert ans["calls"] == 1 if stream_rows == 65536 else ans["calls"] > 1
        assert "slot" not in ans and "stream" not in ans
    # a numpy batch is uploaded; the rows go to the caller drain by drain and nothing is kept
    per = [[] for _ in range(K)]

    def on_rows(owner, rows):
        assert owner.is_cuda and 0 < owner.shape[0] <= 16 and tuple(rows.shape) == (owner.shape[0], model.n_vars)
        _per_owner(owner, rows, K, per)

    ans = model.solve_many_clauses_all(np.array(roots), max_nodes=BUDGET, stream_rows=16, on_rows=on_rows)
    assert "rows" not in ans and "offsets" not in ans
    _check(_host(ans), per, want, "on_rows")
    # one call with a small stream: what is there so far, and what the caller goes on from
    part = model.solve_many_clauses_all(dev, max_nodes=BUDGET, stream_rows=16, max_calls=1)
    assert part["calls"] == 1 and part["rows"].shape[0] == 16 and int(part["offsets"][-1]) == 16
    assert bool((part["slot"] != -1).any())
    owner = np.repeat(np.arange(K), np.diff(part["offsets"].cpu().numpy()))
    per = [[] for _ in range(K)]
    for o, r in zip(owner, part["rows"].cpu().numpy()):
        per[o].append(r)
    got, per, _ = _loop(model, dev, 16, BUDGET, int(counts.sum()) + K + 2, pool=part["_checkpoints"],
                        first=(part["_slots"], part["_records"], per), out=part["stream"])
    _check(got, per, want, "max_calls=1, then the loop", _counted(name))
    # K = 0
    empty = model.solve_many_clauses_all(dev[:0].contiguous(), max_nodes=BUDGET, stream_rows=16)
    assert empty["calls"] == 1 and empty["rows"].shape[0] == 0 and empty["offsets"].tolist() == [0]
    # a model that does not qualify: the library's error, before anything is allocated for the batch
    big = _model(problems.schedule(32, 1))
    with pytest.raises(CsolveError, match="512") as e:
        big.solve_many_clauses_all(np.repeat(big.domains()[None], 2, 0), max_nodes=10)
    assert e.value.code == -4
