"""GPU tests of Model.solve_many_stream / Model.solve_many_all (cs_dive_stream, csgpu_solve_many_stream): under ALL every
solution of every instance goes to one bounded stream, and an instance the stream has no room for steps back and goes on
in the next call.  Expected values are those of the host walk of tests/many_walk.py (Walk(text, row).run(budget, None)),
which asks the oracle for every node and keeps every solution in walk order; nothing is taken from the code under test.
Which instances find room in a call depends on the order the waves arrive in: the tests assert only what holds for every
order."""
import numpy as np
import pytest

import many_upto_sets
import many_walk

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = many_walk.FIELDS
DONE, LIMIT, BAD_ROOT, BAD_SLOT, FULL = 0, 1, 2, 3, 4
FRESH = -2
BUDGET = 1 << 20  # by the host walk the largest tree of the six sets has 64,118 nodes
SENTINEL = -7
_models = {}
_devs = {}
_walks = {}


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


def _walk(name):
    """the ALL walk of every instance of the set, computed once and left alone: a list of result dicts with `rows`"""
    if name not in _walks:
        text, roots = many_upto_sets.build(name)
        _walks[name] = [many_walk.Walk(text, row).run(BUDGET, None) for row in roots]
        assert all(w["status"] == DONE for w in _walks[name])
    return _walks[name]


def _want(name, picked=None):
    walks = _walk(name)
    return [walks[i] for i in (range(len(walks)) if picked is None else picked)]


def _host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


def _loop(model, dev, capacity, budget, max_calls, pool=None, first=None, out=None):
    """call, take the rows, zero the count, until every slot is -1 -- at most max_calls calls, so that a bug cannot spin.
    first: (slots, records, rows per owner so far) to go on from.
    -> (the last answer on the host, the rows per owner in the order they were drained, one snapshot per call)"""
    K = dev.shape[0]
    pool = pool if pool is not None else model.many_checkpoints(K)
    out = out if out is not None else model.many_stream(capacity)
    slots, results, per = first if first is not None else (None, None, [[] for _ in range(K)])
    trace = []
    for _ in range(max_calls):
        ans = model.solve_many_stream(dev, out, pool, slots, results, max_nodes=budget)
        slots, results = ans["_slots"], ans["_records"]
        host = _host(ans)
        attempts = int(out.count.item())
        owner, rows = out.take()
        assert int(out.count.item()) == 0 and owner.shape[0] == min(attempts, capacity)
        for o, r in zip(owner.cpu().numpy(), rows.cpu().numpy()):
            per[o].append(r)
        trace.append(dict(status=host["status"].copy(), slot=host["slot"].copy(), solutions=host["solutions"].copy(),
                          attempts=attempts, taken=int(owner.shape[0])))
        if (host["slot"] == -1).all():
            return host, per, trace
    raise AssertionError(f"{max_calls} calls and some instance still has work left: slots {host['slot'].tolist()}")


def _check(got, per, want, label):
    """every field of every instance; the rows drained for an instance are its walk's rows in walk order, each once"""
    for f in FIELDS:
        g, w = got[f].astype(np.int64), np.array([d[f] for d in want], dtype=np.int64)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, walk {w[bad[0]]}"
    assert sum(len(r) for r in per) == sum(d["solutions"] for d in want), f"{label}: the number of rows drained"
    for i, d in enumerate(want):
        assert len(per[i]) == len(d["rows"]), f"{label}: instance {i} streamed {len(per[i])} rows, its walk has {len(d['rows'])}"
        if d["rows"]:
            assert (np.stack(per[i]) == np.stack(d["rows"])).all(), f"{label}: the rows of instance {i} are not its walk's, in walk order"
            assert len({r.tobytes() for r in per[i]}) == len(per[i]), f"{label}: instance {i} streamed a row twice"


@pytest.mark.parametrize("name", sorted(many_upto_sets.SETS))
def test_one_call_with_room_for_everything_equals_the_walk(name):
    text, roots, dev = _set(name)
    want = _want(name)
    total = sum(d["solutions"] for d in want)
    model = _model(text)
    assert model.many_stream_kernel() == many_upto_sets.SETS[name][3].replace("cs_dive_upto", "cs_dive_stream")
    assert model.many_kernel() == many_upto_sets.SETS[name][3].replace("cs_dive_upto", "cs_dive_shave")  # as it was
    K = len(roots)
    pool = model.many_checkpoints(K)
    out = model.many_stream(total + 3)
    out.rows.fill_(SENTINEL)
    out.owner.fill_(SENTINEL)
    ans = model.solve_many_stream(dev, out, pool, max_nodes=BUDGET)
    got = _host(ans)
    print(f"{name}: {K} instances, {total} solutions, largest tree {max(d['nodes'] for d in want)} nodes")
    assert (got["slot"] == -1).all()
    assert int(out.count.item()) == total == int(got["solutions"].sum())
    assert (out.rows[total:] == SENTINEL).all() and (out.owner[total:] == SENTINEL).all(), "a row behind the stream's end was written"
    owner, rows = out.take()
    owner, rows = owner.cpu().numpy(), rows.cpu().numpy()
    order = np.argsort(owner, kind="stable")  # grouped by owner, in index order within one
    bounds = np.searchsorted(owner[order], np.arange(K + 1))
    per = [list(rows[order[bounds[i]:bounds[i + 1]]]) for i in range(K)]
    _check(got, per, want, name)
    assert sum(1 for d in want if d["solutions"] >= 2) >= 4


# name, capacity, the rows of the set in use (None: all).  The 16-bit set is cut to the rows with 21, 60, 152, 304 and 570
# solutions (1,107 in all): with all twelve rows a stream of 64 rows would take 1,400 calls
SMALL = [("sudoku9", 1, None), ("sudoku9", 7, None), ("queens12_two", 7, None), ("queens12_two", 64, None),
         ("sudoku16", 7, None), ("sudoku16", 64, None), ("sparse40_e16", 64, (8, 9, 3, 0, 10))]


@pytest.mark.parametrize("name,capacity,picked", SMALL)
def test_small_streams_lose_nothing_and_repeat_nothing(name, capacity, picked):
    text, roots, dev = _set(name)
    if picked is not None:
        dev = dev[list(picked)].contiguous()
    want = _want(name, picked)
    total = sum(d["solutions"] for d in want)
    # the stream fills; and under the set's smallest capacity one instance alone has more solutions than the stream holds
    assert sum(1 for d in want if d["solutions"] >= 2) >= 4 and total > capacity
    assert max(d["solutions"] for d in want) > min(c for n, c, _ in SMALL if n == name)
    K = dev.shape[0]
    got, per, trace = _loop(_model(text), dev, capacity, BUDGET, total + K + 2)
    print(f"{name}, capacity {capacity}: {K} instances, {total} solutions, {len(trace)} calls")
    _check(got, per, want, f"{name}, capacity {capacity}")
    assert (got["status"] == DONE).all()
    assert any(((t["status"] == FULL) & (t["slot"] >= 0)).any() for t in trace[:-1]), "no instance stopped FULL with a checkpoint"
    assert all(t["taken"] == capacity for t in trace[:-1] if t["attempts"] > capacity)
    for t in trace:
        assert ((t["slot"] == FRESH) <= (t["status"] == FULL)).all(), "an instance that was not started has status FULL"
        assert ((t["slot"] >= 0) <= (t["status"] == FULL)).all(), "under this budget a checkpoint means FULL"
    if name == "sudoku9":
        # ten rows are solutions at the root: more than the stream holds, so some of them find no room in the first call
        assert sum(1 for d in want if d["nodes"] == 0 and d["solutions"] == 1) == 10 > capacity
        assert (trace[0]["slot"] == FRESH).any(), "no instance was left unstarted"
        left = trace[0]["slot"] == FRESH
        assert (trace[0]["solutions"][left] == 0).all()


def _found_per_slice(name, budget):
    """by the host walk in slices of `budget` nodes: the solutions all instances of the set find in slice 0, 1, ..."""
    text, roots = many_upto_sets.build(name)
    found = {}
    for row in roots:
        w, before, c = many_walk.Walk(text, row), 0, 0
        while True:
            part = w.run(budget, None)
            found[c] = found.get(c, 0) + part["solutions"] - before
            before, c = part["solutions"], c + 1
            if part["status"] != LIMIT:
                break
    return [found[c] for c in sorted(found)]


@pytest.mark.parametrize("capacity", [64, 16])
def test_budget_and_stream_together(capacity):
    """max_nodes 64 on queens12_two.  By the host walk the 24 instances together find 27 solutions in their first 64
    nodes and never more than 50 in any slice of 64: a stream of 64 rows, zeroed between the calls, cannot fill under
    this budget (every call ends LIMIT, none FULL -- asserted from the walk's figures), a stream of 16 rows fills in the
    first call, and there LIMIT and FULL both occur.  The final answer is the walk's in both."""
    text, roots, dev = _set("queens12_two")
    want = _want("queens12_two")
    total = sum(d["solutions"] for d in want)
    slices = _found_per_slice("queens12_two", 64)
    assert slices[0] == 27 and max(slices) == 50
    # a call that does not fill the stream takes every open instance 64 nodes on; a call that fills it drains `capacity` rows
    max_calls = total + len(roots) + 2 + max(d["nodes"] for d in want) // 64
    got, per, trace = _loop(_model(text), dev, capacity, 64, max_calls)
    print(f"queens12_two, capacity {capacity}, 64 nodes per call: {len(trace)} calls")
    _check(got, per, want, f"queens12_two, budget 64, capacity {capacity}")
    assert any(((t["status"] == LIMIT) & (t["slot"] >= 0)).any() for t in trace)
    if capacity > max(slices):
        assert not any((t["status"] == FULL).any() for t in trace) and len(trace) == len(slices)
    else:
        assert slices[0] > capacity and (trace[0]["status"] == FULL).any() and trace[0]["taken"] == capacity
        assert any((t["status"] == LIMIT).any() for t in trace) and any(((t["status"] == FULL) & (t["slot"] >= 0)).any() for t in trace)


def _sentinel_records(K):
    return torch.full((K, 5), SENTINEL, dtype=torch.int64, device="cuda")


def test_finished_fresh_and_resumed_instances_in_one_call():
    text, roots, dev = _set("sudoku9")
    want = _want("sudoku9")
    model = _model(text)
    K = len(roots)
    total = sum(d["solutions"] for d in want)
    pool = model.many_checkpoints(K)
    out = model.many_stream(total)
    records = _sentinel_records(K)
    slots = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    slots[:32] = FRESH
    # call A: the first 32 start with 8 nodes each, the others are finished on entry (-1) and are not touched
    a = _host(model.solve_many_stream(dev, out, pool, slots, records, max_nodes=8))
    assert (records[32:] == SENTINEL).all() and (a["slot"][32:] == -1).all()
    stopped = np.flatnonzero(a["slot"] >= 0)
    assert stopped.size >= 4 and (a["status"][stopped] == LIMIT).all() and (a["nodes"][stopped] == 8).all()
    assert (stopped < 32).all() and len(set(a["slot"][stopped].tolist())) == stopped.size
    owner, rows = out.take()
    assert (owner < 32).all()
    per = [[] for _ in range(K)]
    for o, r in zip(owner.cpu().numpy(), rows.cpu().numpy()):
        per[o].append(r)
    # call B: those go on from their slots, 16 more start, 16 stay finished -- and some slot entry below -2 is finished too
    slots[32:48] = FRESH
    slots[63] = -5
    records[32:48] = 0
    b = _host(model.solve_many_stream(dev, out, pool, slots, records, max_nodes=BUDGET))
    assert (records[48:] == SENTINEL).all() and (b["slot"][48:63] == -1).all() and b["slot"][63] == -5
    assert (b["slot"][:48] == -1).all()
    owner, rows = out.take()
    assert (owner < 48).all()
    for o, r in zip(owner.cpu().numpy(), rows.cpu().numpy()):
        per[o].append(r)
    _check({f: b[f][:48] for f in FIELDS}, per[:48], want[:48], "fresh and resumed mixed")
    assert not any(per[48:])


def test_a_slot_number_that_names_no_checkpoint():
    text, roots, dev = _set("sudoku9")
    want = _want("sudoku9")
    model = _model(text)
    pool = model.many_checkpoints(8)
    out = model.many_stream(256)
    out.rows.fill_(SENTINEL)
    records = _sentinel_records(4)
    slots = torch.tensor([8, 3, FRESH, 1 << 30], dtype=torch.int32, device="cuda")  # past the pool, never written, fresh, far past
    ans = model.solve_many_stream(dev[:4].contiguous(), out, pool, slots, records, max_nodes=BUDGET)
    got = _host(ans)
    assert got["status"].tolist() == [BAD_SLOT, BAD_SLOT, DONE, BAD_SLOT]
    assert got["slot"].tolist() == [8, 3, -1, 1 << 30]
    for i in (0, 1, 3):  # nothing but the status
        assert got["root_props"][i] == -1 and all(got[f][i] == SENTINEL for f in ("nodes", "cuts", "props", "solutions"))
    assert all(got[f][2] == want[2][f] for f in FIELDS)
    owner, rows = out.take()
    assert owner.shape[0] == want[2]["solutions"] and (owner == 2).all()
    assert (rows.cpu().numpy() == np.stack(want[2]["rows"])).all()
    assert (out.rows[owner.shape[0]:] == SENTINEL).all()
    assert _slots_drawn(model, pool) == 0


def _slots_drawn(model, pool):
    """slots drawn from the pool so far, told by drawing the rest: a checkpointed call of instances that all stop"""
    text, roots, dev = _set("sudoku9")
    deep = [i for i, d in enumerate(_want("sudoku9")) if d["nodes"] > 1][: pool.capacity]
    assert len(deep) == pool.capacity
    out = _host(model.solve_many(dev[deep].contiguous(), "ALL", max_nodes=1, checkpoints=pool))
    return pool.capacity - int((out["slot"] >= 0).sum())


def test_the_library_refuses_what_it_documents():
    from csolve_amd import CsolveError, problems
    text, roots, dev = _set("sudoku9")
    model = _model(text)
    other = _model(_set("queens12_two")[0])
    pool, foreign = model.many_checkpoints(2), other.many_checkpoints(2)
    out = model.many_stream(16)
    with pytest.raises(CsolveError, match="another model") as e:
        model.solve_many_stream(dev, out, foreign, max_nodes=10)
    assert e.value.code == -1
    sched = _model(problems.schedule(6, 1))
    assert not sched.qualifies(7) and sched.many_stream_kernel() is None
    rows = torch.from_numpy(sched.domains()[None].copy()).cuda()
    with pytest.raises(CsolveError, match="does not qualify") as e:  # before the pool is looked at
        sched.solve_many_stream(rows, sched.many_stream(16), foreign, max_nodes=10)
    assert e.value.code == -4
    with pytest.raises(CsolveError, match="capacity") as e:
        model.solve_many_stream(dev, model.many_stream(0), pool, max_nodes=10)
    assert e.value.code == -1
    with pytest.raises(CsolveError, match="max_nodes") as e:
        model.solve_many_stream(dev, out, pool, max_nodes=0)
    assert e.value.code == -1
    # an empty batch launches nothing
    ans = model.solve_many_stream(dev[:0].contiguous(), out, pool, max_nodes=10)
    assert ans["status"].shape[0] == 0 and int(out.count.item()) == 0


def test_a_pool_that_is_too_small_loses_walks_not_rows():
    text, roots, dev = _set("sudoku9")
    want = _want("sudoku9")
    model = _model(text)
    K = len(roots)
    pool = model.many_checkpoints(2)
    got, per, trace = _loop(model, dev, 8, BUDGET, sum(d["solutions"] for d in want) + K + 2, pool=pool)
    drawn = set()
    for t in trace:
        drawn |= set(t["slot"][t["slot"] >= 0].tolist())
    assert drawn <= {0, 1} and len(drawn) >= 1, drawn
    lost = np.flatnonzero(got["status"] != DONE)
    print(f"pool of 2, capacity 8: {len(trace)} calls, slots drawn {sorted(drawn)}, {lost.size} instances lost their walk")
    # sixteen instances have more than 8 solutions: none of them ends within one call, and two slots serve two of them
    assert sum(1 for d in want if d["solutions"] > 8) == 16 and lost.size >= 14
    assert (got["slot"] == -1).all()
    for i in range(K):
        d = want[i]
        if got["status"][i] == DONE:  # unaffected
            _check({f: got[f][i:i + 1] for f in FIELDS}, [per[i]], [d], f"instance {i}")
        else:  # stopped without a slot: FULL with the counters of that moment, its rows the head of its walk's
            assert got["status"][i] == FULL
            s = int(got["solutions"][i])
            assert s < d["solutions"] and len(per[i]) == s and got["nodes"][i] < d["nodes"] and got["root_props"][i] == d["root_props"]
            assert all((a == b).all() for a, b in zip(per[i], d["rows"]))


def test_two_calls_queued_without_the_host_between_them():
    text, roots, dev = _set("queens12_two")
    want = _want("queens12_two")
    model = _model(text)
    K = len(roots)
    total = sum(d["solutions"] for d in want)
    pool = model.many_checkpoints(K)
    out = model.many_stream(600)
    a = model.solve_many_stream(dev, out, pool, max_nodes=256)
    b = model.solve_many_stream(dev, out, pool, a["_slots"], a["_records"], max_nodes=256)  # the count is not zeroed
    host = _host(b)
    attempts = int(out.count.item())
    assert attempts >= int(host["solutions"].sum())
    owner, rows = out.take()
    assert owner.shape[0] == min(attempts, 600) == int(host["solutions"].sum())
    per = [[] for _ in range(K)]
    for o, r in zip(owner.cpu().numpy(), rows.cpu().numpy()):
        per[o].append(r)
    assert (host["slot"] != -1).any(), "256 nodes twice do not finish the deep instances"
    got, per, trace = _loop(model, dev, 600, 256, total + K + 2 + max(d["nodes"] for d in want) // 256, pool=pool,
                            first=(b["_slots"], b["_records"], per), out=out)
    _check(got, per, want, "two calls queued, then the loop")
    # and the older families behind it on the same stream: the ticket counters came back to zero
    plain = _host(model.solve_many(dev, "ALL", max_nodes=BUDGET))
    for f in FIELDS:
        assert (plain[f] == got[f]).all(), f


def test_a_full_checkpoint_exports_its_open_subtrees():
    from csolve_amd.solver import Search
    text, roots, dev = _set("sudoku9")
    want = _want("sudoku9")
    model = _model(text)
    K = len(roots)
    pool = model.many_checkpoints(K)
    out = model.many_stream(8)
    ans = model.solve_many_stream(dev, out, pool, max_nodes=BUDGET)
    got = _host(ans)
    full = np.flatnonzero((got["status"] == FULL) & (got["slot"] >= 0))
    assert full.size >= 1
    search = Search(model, 1 << 16, 1 << 12)
    for i in full[:4].tolist():
        states, complete = model.open_subtrees(pool, int(got["slot"][i]))
        below = int(complete.shape[0])
        if states.shape[0]:
            search.reset()
            search.put(states)
            st = search.run()
            assert st["done"] == 1
            below += int(st["solutions"])
        assert below == want[i]["solutions"] - int(got["solutions"][i]), f"instance {i}"
        assert below >= 1  # the refused solution itself lies below the checkpoint
    search.close()


def test_solve_many_all_drives_the_loop():
    text, roots, dev = _set("sudoku9")
    want = _want("sudoku9")
    model = _model(text)
    K = len(roots)
    counts = np.array([d["solutions"] for d in want])
    every = np.concatenate([np.stack(d["rows"]) for d in want if d["rows"]])
    for stream_rows in (65536, 16):
        ans = model.solve_many_all(dev, max_nodes=BUDGET, stream_rows=stream_rows)
        got = _host(ans)
        assert (got["offsets"] == np.concatenate([[0], np.cumsum(counts)])).all()
        assert (got["rows"] == every).all(), stream_rows
        for f in FIELDS:
            assert (got[f] == np.array([d[f] for d in want])).all(), f
        assert ans["calls"] == 1 if stream_rows == 65536 else ans["calls"] > 1
        assert "slot" not in ans and "stream" not in ans
    # a numpy batch is uploaded; the rows go to the caller drain by drain and nothing is kept
    per = [[] for _ in range(K)]

    def on_rows(owner, rows):
        assert owner.is_cuda and 0 < owner.shape[0] <= 16 and tuple(rows.shape) == (owner.shape[0], model.n_vars)
        for o, r in zip(owner.cpu().numpy(), rows.cpu().numpy()):
            per[o].append(r)

    ans = model.solve_many_all(roots, max_nodes=BUDGET, stream_rows=16, on_rows=on_rows)
    assert "rows" not in ans and "offsets" not in ans
    _check(_host(ans), per, want, "on_rows")
    # one call with a small stream: what is there so far, and what the caller goes on from
    part = model.solve_many_all(dev, max_nodes=BUDGET, stream_rows=16, max_calls=1)
    assert part["calls"] == 1 and part["rows"].shape[0] == 16 and int(part["offsets"][-1]) == 16
    assert bool((part["slot"] != -1).any())
    owner = np.repeat(np.arange(K), np.diff(part["offsets"].cpu().numpy()))
    per = [[] for _ in range(K)]
    for o, r in zip(owner, part["rows"].cpu().numpy()):
        per[o].append(r)
    got, per, _ = _loop(model, dev, 16, BUDGET, int(counts.sum()) + K + 2, pool=part["_checkpoints"],
                        first=(part["_slots"], part["_records"], per), out=part["stream"])
    _check(got, per, want, "max_calls=1, then the loop")
