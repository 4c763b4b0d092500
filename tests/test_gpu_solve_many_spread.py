"""GPU tests of the spread of stopped ALL walks: cs_dive_children / cs_dive_fanout / cs_dive_fold behind
csgpu_many_checkpoint_children, csgpu_many_checkpoint_fanout and csgpu_many_fold, and Model.solve_many_spread on top of them.
The yardsticks are the host model of tests/many_spread_walk.py (the children of a stopped walk in walk order, the fold)
and the one-budget oracle walk many_walk.dive_many(..., "ALL"), which test_gpu_solve_many.py computes once per set and
this module shares.  Every call passes a finite max_nodes."""
import numpy as np
import pytest

import many_sets
import many_spread_walk
import many_walk
from test_gpu_solve_many import _model, _set as _walked_set

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("status", "root_props", "nodes", "cuts", "props", "solutions")
DONE, LIMIT = 0, 1
SENTINEL = 0x5a5a5a5a
SPREAD_SETS = ("queens12_two", "sudoku9_all", "offsets40", "sparse40_e16", "sparse150_e16")
_sets, _stops = {}, {}


def _set(name):
    """(text, roots, roots on the device), built once"""
    if name not in _sets:
        text, roots, _, _ = many_sets.build(name)
        _sets[name] = (text, roots, torch.from_numpy(roots).cuda())
    return _sets[name]


def _host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if torch.is_tensor(v) and not k.startswith("_")}


def _stopped(name, rows=12, budget=16):
    """the first `rows` rows of a set, checkpointed under ALL with `budget` on the device and stopped on the host:
    (model, pool, the answer, host walks, host children rows per instance -- None where the walk did not stop)"""
    if (name, rows, budget) not in _stops:
        text, roots, dev = _set(name)
        model = _model(text)
        pool = model.many_checkpoints(rows)
        out = model.solve_many(dev[:rows].contiguous(), "ALL", max_nodes=budget, checkpoints=pool)
        walks, kids = [], []
        for i in range(rows):
            w = many_walk.Walk(text, roots[i])
            walks.append(w)
            kids.append(many_spread_walk.children_of(w) if w.run(budget)["status"] == LIMIT else None)
        _stops[name, rows, budget] = (model, pool, out, walks, kids)
    return _stops[name, rows, budget]


def _offsets(children):
    off = torch.zeros((children.shape[0] + 1,), dtype=torch.int64, device=children.device)
    torch.cumsum(children.clamp(min=0), 0, out=off[1:])
    return off


def _sentinel_rows(total, n, guard=4):
    rows = torch.full((total + guard, n, 2), SENTINEL, dtype=torch.int32, device="cuda")
    owner = torch.full((total + guard,), SENTINEL, dtype=torch.int32, device="cuda")
    return rows, owner


@pytest.mark.parametrize("name", sorted(many_sets.SETS))
def test_children_and_rows_are_the_host_walks_in_walk_order(name):
    """pools written by all six cs_dive_resume instantiations; n = 12, 40, 64, 81, 100, 150 and 256; root lower bounds
    2,000 apart on the sparse*_e16 sets; a finished entry (slot -1) behind every instance"""
    model, pool, out, walks, kids = _stopped(name)
    got = _host(out)
    K, n = len(kids), model.n_vars
    stopped = [i for i in range(K) if kids[i] is not None]
    assert stopped, "the budget must stop instances"
    assert ((got["slot"] >= 0) == np.array([k is not None for k in kids])).all()
    slots = torch.full((2 * K,), -1, dtype=torch.int32, device="cuda")
    slots[0::2] = out["slot"]
    children = model.checkpoint_children(pool, slots)
    want_children = np.zeros(2 * K, dtype=np.int64)
    for i in stopped:
        want_children[2 * i] = many_spread_walk.count_children(walks[i])
        assert want_children[2 * i] == len(kids[i]) >= 1
    torch.cuda.synchronize()
    assert (children.cpu().numpy() == want_children).all(), name
    total = int(want_children.sum())
    offsets = _offsets(children)
    assert int(offsets[-1]) == total  # tight: no row between two instances, none behind the last
    rows, owner = _sentinel_rows(total, n)
    model.checkpoint_fanout(pool, slots, offsets, total, rows, owner)
    torch.cuda.synchronize()
    want_rows = np.concatenate([kids[i] for i in stopped])
    want_owner = np.concatenate([np.full(len(kids[i]), 2 * i) for i in stopped])
    assert (rows[:total].cpu().numpy() == want_rows).all(), f"{name}: the fanned rows differ from the host walk's"
    assert (owner[:total].cpu().numpy() == want_owner).all()
    assert (rows[total:] == SENTINEL).all() and (owner[total:] == SENTINEL).all()
    print(f"{name}: n = {n}, {len(stopped)} of {K} stopped, {total} children, "
          f"{sum(w.has_last_value_frame() for w in walks if w.open)} walks with a one-child frame")


def test_bad_slots_and_bad_offsets_write_nothing():
    model, pool, out, walks, kids = _stopped("queens12_two")
    n = model.n_vars
    got = _host(out)
    stopped = np.flatnonzero(got["slot"] >= 0)
    assert stopped.size >= 4
    good = model.checkpoint_children(pool, out["slot"].contiguous()).clone()
    # slot numbers outside the pool: the first past it, and one far outside
    a, b = int(stopped[1]), int(stopped[2])
    slots = out["slot"].clone()
    slots[a], slots[b] = pool.capacity, 1 << 30
    children = model.checkpoint_children(pool, slots)
    want = good.clone()
    want[a] = want[b] = -1
    assert (children == want).all()
    offsets = _offsets(children)
    total = int(offsets[-1])
    rows, owner = _sentinel_rows(total, n)
    model.checkpoint_fanout(pool, slots, offsets, total, rows, owner)
    torch.cuda.synchronize()
    others = [i for i in stopped if i not in (a, b)]
    assert (rows[:total].cpu().numpy() == np.concatenate([kids[i] for i in others])).all()
    assert (owner[:total].cpu().numpy() == np.concatenate([np.full(len(kids[i]), i) for i in others])).all()
    assert (rows[total:] == SENTINEL).all() and (owner[total:] == SENTINEL).all()
    # and with offsets that promise them a row each: still nothing
    claimed = children.clone()
    claimed[a] = claimed[b] = 1
    offsets = _offsets(claimed)
    rows, owner = _sentinel_rows(total + 2, n)
    model.checkpoint_fanout(pool, slots, offsets, total + 2, rows, owner)
    torch.cuda.synchronize()
    for i in (a, b):
        assert (rows[int(offsets[i])] == SENTINEL).all() and owner[int(offsets[i])] == SENTINEL
    assert int((owner == SENTINEL).sum()) == 2 + 4
    # a fresh pool: no slot holds a checkpoint
    fresh = model.many_checkpoints(4)
    slots = torch.arange(4, dtype=torch.int32, device="cuda")
    children = model.checkpoint_children(fresh, slots)
    assert (children == -1).all()
    rows, owner = _sentinel_rows(4, n)
    model.checkpoint_fanout(fresh, slots, torch.arange(5, dtype=torch.int64, device="cuda"), 4, rows, owner)
    torch.cuda.synchronize()
    assert (rows == SENTINEL).all() and (owner == SENTINEL).all()
    # one count off by one: that instance writes nothing, the others write their rows where the offsets say
    slots = out["slot"].contiguous()
    c = int(stopped[2])
    claimed = good.clone()
    claimed[c] += 1
    offsets = _offsets(claimed)
    total = int(offsets[-1])
    rows, owner = _sentinel_rows(total, n)
    model.checkpoint_fanout(pool, slots, offsets, total, rows, owner)
    torch.cuda.synchronize()
    off = offsets.cpu().numpy()
    for i in stopped:
        part, own = rows[off[i]:off[i + 1]].cpu().numpy(), owner[off[i]:off[i + 1]].cpu().numpy()
        if i == c:
            assert (part == SENTINEL).all() and (own == SENTINEL).all()
        else:
            assert (part == kids[i]).all() and (own == i).all(), i
    assert (rows[total:] == SENTINEL).all()
    # rows that would lie past `total`: the last instance writes nothing
    offsets = _offsets(good)
    total = int(offsets[-1])
    rows, owner = _sentinel_rows(total, n)
    model.checkpoint_fanout(pool, slots, offsets, total - 1, rows, owner)
    torch.cuda.synchronize()
    last = int(stopped[-1])
    assert (rows[int(offsets[last]):] == SENTINEL).all() and (rows[:int(offsets[last])] != SENTINEL).all()


def test_a_clause_pool_is_refused():
    from csolve_amd import CsolveError, problems
    model = _model(problems.queens(8, "ALL"))  # a model of both families
    assert model.qualifies(7) and model.qualifies_many_clauses()
    clause_pool = model.many_clause_checkpoints(4)
    slots = torch.zeros((4,), dtype=torch.int32, device="cuda")
    with pytest.raises(CsolveError, match="other kind") as e:
        model.checkpoint_children(clause_pool, slots)
    assert e.value.code == -1
    with pytest.raises(CsolveError, match="other kind") as e:
        model.checkpoint_fanout(clause_pool, slots, torch.arange(5, dtype=torch.int64, device="cuda"), 4)
    assert e.value.code == -1


def test_the_fold_is_the_host_fold_and_folding_twice_counts_twice():
    model, pool, out, walks, kids = _stopped("queens12_two")
    text = _set("queens12_two")[0]
    K = len(kids)
    slots = out["slot"].contiguous()
    children = model.checkpoint_children(pool, slots)
    offsets = _offsets(children)
    total = int(offsets[-1])
    rows, owner = model.checkpoint_fanout(pool, slots, offsets, total)
    sub = model.solve_many(rows.contiguous(), "ALL", max_nodes=64, checkpoints=model.many_checkpoints(total))
    records = _host(sub)
    host_records = [{f: int(records[f][t]) for f in FIELDS} for t in range(total)]
    assert any(r["status"] == DONE and r["nodes"] == 0 and r["solutions"] == 0 for r in host_records), "no inconsistent root row"
    assert any(r["status"] == LIMIT for r in host_records), "no stopped sub-instance"
    want = many_spread_walk.fold(host_records, owner.cpu().numpy(), [{f: 0 for f in many_spread_walk.COUNTERS} for _ in range(K)])
    # the sub-records themselves are the host walk's
    stopped = [i for i in range(K) if kids[i] is not None]
    walked = many_walk.dive_many(text, np.concatenate([kids[i] for i in stopped]), "ALL", 64)
    for f in FIELDS:
        assert (records[f] == walked[f]).all(), f
    target = model.solve_many(_set("queens12_two")[2][:K].contiguous(), "ALL", max_nodes=16, checkpoints=model.many_checkpoints(K))
    before = _host(target)
    for times in (1, 2):
        model.fold_many(sub, owner.contiguous(), target)
        got = _host(target)
        for f in many_spread_walk.COUNTERS:
            assert (got[f] == before[f] + times * np.array([w[f] for w in want])).all(), (f, times)
        assert (got["status"] == before["status"]).all() and (got["root_props"] == before["root_props"]).all()


@pytest.mark.parametrize("name", SPREAD_SETS)
def test_the_spread_is_the_one_all_call(name):
    text, roots, objective, budget, want = _walked_set(name)
    assert objective == "ALL" and (want["status"] == DONE).all()
    model = _model(text)
    out = model.solve_many_spread(_set(name)[2], budgets=(16, 64))
    got = _host(out)
    print(f"{name}: {len(roots)} owners, {out['rounds']} rounds, {out['sub_instances']} sub-instances")
    for f in FIELDS + ("first",):
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(roots), -1).any(axis=1))
        assert bad.size == 0, f"{name}: {f} differs for {bad.size} owners, first {bad[0]}: got {got[f][bad[0]]}, walk {want[f][bad[0]]}"
    assert "slot" not in out and out["sub_instances"] > 0
    if name == "queens12_two":
        assert out["rounds"] >= 3


def test_a_budget_nothing_stops_at_is_solve_many_itself():
    text, roots, objective, budget, want = _walked_set("queens12_two")
    model = _model(text)
    dev = _set("queens12_two")[2]
    out = model.solve_many_spread(dev, budgets=(1 << 16,))
    assert out["rounds"] == 1 and out["sub_instances"] == 0
    got, plain = _host(out), _host(model.solve_many(dev, "ALL", max_nodes=1 << 16))
    for f in FIELDS + ("first",):
        assert (got[f] == plain[f]).all() and (got[f] == want[f]).all(), f


def test_one_round_leaves_the_stopped_owners_at_limit():
    text, roots, objective, budget, want = _walked_set("queens12_two")
    model = _model(text)
    out = model.solve_many_spread(_set("queens12_two")[2], budgets=(16, 64), max_rounds=1)
    assert out["rounds"] == 1 and out["sub_instances"] == 0
    got = _host(out)
    walk = many_walk.dive_many(text, roots, "ALL", 16)
    assert (walk["status"] == LIMIT).sum() > 8
    for f in FIELDS + ("first",):
        assert (got[f] == walk[f]).all(), f
    # and two rounds: the owners whose children all ended are DONE with the whole record, the others LIMIT
    out = model.solve_many_spread(_set("queens12_two")[2], budgets=(16, 64), max_rounds=2)
    got = _host(out)
    done = got["status"] == DONE
    assert out["rounds"] == 2 and out["sub_instances"] > 0 and (~done).any() and (got["status"][~done] == LIMIT).all()
    for f in FIELDS:
        assert (got[f][done] == want[f][done]).all(), f
    assert (got["nodes"][~done] < want["nodes"][~done]).all()


@pytest.mark.parametrize("name,budgets,max_rows", [("queens12_two", (16, 4096), 8), ("sudoku9_all", (16, 64), 40)])
def test_a_round_wider_than_max_rows_goes_on_in_place(name, budgets, max_rows):
    """queens12_two: every later round is too wide, the walks end in place; sudoku9_all: the rounds narrow until one is
    fanned out after all"""
    text, roots, objective, budget, want = _walked_set(name)
    model = _model(text)
    dev = _set(name)[2]
    pool = model.many_checkpoints(len(roots))
    first_round = model.solve_many(dev, "ALL", max_nodes=budgets[0], checkpoints=pool)
    children = int(model.checkpoint_children(pool, first_round["slot"].contiguous()).clamp(min=0).sum())
    assert children > max_rows, "round 1 must be too wide to fan out"
    out = model.solve_many_spread(dev, budgets=budgets, max_rows=max_rows)
    got = _host(out)
    print(f"{name}: {children} children after round 0, max_rows {max_rows}: {out['rounds']} rounds, "
          f"{out['sub_instances']} sub-instances")
    assert out["rounds"] >= 2 and out["sub_instances"] <= max_rows * (out["rounds"] - 2)
    for f in FIELDS + ("first",):
        assert (got[f] == want[f]).all(), f


def test_a_model_of_the_wrong_kind_is_refused():
    from csolve_amd import CsolveError, problems
    text = problems.schedule(6, 1)
    model = _model(text)
    rows = np.repeat(model.domains()[None], 2, 0).astype(np.int32)
    with pytest.raises(CsolveError, match="does not qualify") as e:
        model.solve_many_spread(rows, budgets=(16, 64))
    assert e.value.code == -4
