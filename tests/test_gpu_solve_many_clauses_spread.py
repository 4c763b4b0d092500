"""GPU tests of the spread of stopped ALL walks of clause models: cs_walk_children / cs_walk_fanout behind
csgpu_many_clause_checkpoint_children / _fanout, and Model.solve_many_clauses_spread on top of them and csgpu_many_fold.
The yardsticks are the host model of tests/many_clause_spread_walk.py for the children of a stopped walk in walk order,
and the one ALL call of solve_many_clauses itself for the driver: every field, props and root_props included, since a
child runs through the same rounds as a root row.  Every call passes a finite max_nodes."""
import functools

import numpy as np
import pytest

import many_clause_sets as sets
import many_clause_spread_walk as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("status", "root_props", "nodes", "cuts", "props", "solutions")
DONE, LIMIT = 0, 1
SENTINEL = 0x5a5a5a5a
KERNEL_SETS = ("tree20_all", "wcet_max", "linear20_all", "mixed40_any")  # <2,true>, <1,true>, <2,false>, <4,true> (n = 40)
SPREAD_SETS = KERNEL_SETS + ("linear40_all",)
BUDGETS = ((8, 32), (2, 1, 1, 1, 64))


@functools.lru_cache(maxsize=None)
def _model(text):
    from csolve_amd.solver import solve_root
    return solve_root(text)


@functools.lru_cache(maxsize=None)
def _set(name):
    """(text, roots, roots on the device, the set's budget), built once"""
    text, roots, _, budget = sets.build(name)
    return text, roots, torch.from_numpy(np.array(roots)).cuda(), budget


def _host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if torch.is_tensor(v) and not k.startswith("_")}


@functools.lru_cache(maxsize=None)
def _one_call(name):
    """solve_many_clauses(roots, "ALL", max_nodes = the set's budget) on the device (computed once, not to be changed)"""
    text, _, dev, budget = _set(name)
    got = _host(_model(text).solve_many_clauses(dev, "ALL", max_nodes=budget))
    assert (got["status"] == DONE).all(), f"{name}: the set's budget ends every ALL walk"
    return got


@functools.lru_cache(maxsize=None)
def _stopped(name, budget=8):
    """a set checkpointed under ALL with `budget` on the device and stopped on the host: (model, pool, the answer, host
    walks, host children rows per instance -- None where the walk did not stop)"""
    text, roots, dev, _ = _set(name)
    model = _model(text)
    pool = model.many_clause_checkpoints(len(roots))
    out = model.solve_many_clauses(dev, "ALL", max_nodes=budget, checkpoints=pool)
    walks, kids = [], []
    for row in roots:
        w, record = S.stopped_walk(text, row, budget)
        walks.append(w)
        kids.append(S.children_of(w) if record["status"] == LIMIT else None)
    return model, pool, out, walks, kids


def _offsets(children):
    off = torch.zeros((children.shape[0] + 1,), dtype=torch.int64, device=children.device)
    torch.cumsum(children.clamp(min=0), 0, out=off[1:])
    return off


def _sentinel_rows(total, n, guard=4):
    rows = torch.full((total + guard, n, 2), SENTINEL, dtype=torch.int32, device="cuda")
    owner = torch.full((total + guard,), SENTINEL, dtype=torch.int32, device="cuda")
    return rows, owner


def _nothing_written(model, pool, slots, offsets, total):
    rows, owner = _sentinel_rows(total, model.n_vars)
    model.clause_checkpoint_fanout(pool, slots, offsets, total, rows, owner)
    torch.cuda.synchronize()
    return bool((rows == SENTINEL).all()) and bool((owner == SENTINEL).all())


@pytest.mark.parametrize("name", KERNEL_SETS)
def test_children_and_rows_are_the_host_walks_in_walk_order(name):
    """pools written by four cs_walk_resume instantiations; a finished entry (slot -1) behind every instance"""
    model, pool, out, walks, kids = _stopped(name)
    got = _host(out)
    K, n = len(kids), model.n_vars
    stopped = [i for i in range(K) if kids[i] is not None]
    assert stopped, "the budget must stop instances"
    assert ((got["slot"] >= 0) == np.array([k is not None for k in kids])).all()
    slots = torch.full((2 * K,), -1, dtype=torch.int32, device="cuda")
    slots[0::2] = out["slot"]
    children = model.clause_checkpoint_children(pool, slots)
    want_children = np.zeros(2 * K, dtype=np.int64)
    for i in stopped:
        want_children[2 * i] = S.count_children(walks[i])
        assert want_children[2 * i] == len(kids[i]) >= 1
    torch.cuda.synchronize()
    assert (children.cpu().numpy() == want_children).all(), name
    total = int(want_children.sum())
    offsets = _offsets(children)
    assert int(offsets[-1]) == total  # tight: no row between two instances, none behind the last
    rows, owner = _sentinel_rows(total, n)
    model.clause_checkpoint_fanout(pool, slots, offsets, total, rows, owner)
    torch.cuda.synchronize()
    want_rows = np.concatenate([kids[i] for i in stopped])
    want_owner = np.concatenate([np.full(len(kids[i]), 2 * i) for i in stopped])
    assert (rows[:total].cpu().numpy() == want_rows).all(), f"{name}: the fanned rows differ from the host walk's"
    assert (owner[:total].cpu().numpy() == want_owner).all()
    assert (rows[total:] == SENTINEL).all() and (owner[total:] == SENTINEL).all()
    # and without an owner vector: the same rows
    rows2, _ = _sentinel_rows(total, n)
    from csolve_amd._lib import check, load_library
    check(load_library().csgpu_many_clause_checkpoint_fanout(pool._h, slots.data_ptr(), 2 * K, offsets.data_ptr(),
                                                             rows2.data_ptr(), None, total, None))
    torch.cuda.synchronize()
    assert (rows2 == rows).all()
    print(f"{name}: n = {n}, {len(stopped)} of {K} stopped, {total} children, "
          f"{sum(w.has_last_value_frame() for w in walks if w.open)} walks with a one-child frame, "
          f"{sum(len(w.frames()) == 1 for w in walks if w.open)} of depth 0")


def test_refused_slots_and_bad_offsets_write_nothing():
    model, pool, out, walks, kids = _stopped("linear20_all")
    n = model.n_vars
    got = _host(out)
    stopped = np.flatnonzero(got["slot"] >= 0)
    assert stopped.size >= 4
    good = model.clause_checkpoint_children(pool, out["slot"].contiguous()).clone()
    assert (good[torch.from_numpy(stopped).cuda()] >= 1).all()
    # slot numbers outside the pool: the first past it, and one far outside
    a, b = int(stopped[1]), int(stopped[2])
    slots = out["slot"].clone()
    slots[a], slots[b] = pool.capacity, 1 << 30
    children = model.clause_checkpoint_children(pool, slots)
    want = good.clone()
    want[a] = want[b] = -1
    assert (children == want).all()
    offsets = _offsets(children)
    total = int(offsets[-1])
    rows, owner = _sentinel_rows(total, n)
    model.clause_checkpoint_fanout(pool, slots, offsets, total, rows, owner)
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
    model.clause_checkpoint_fanout(pool, slots, offsets, total + 2, rows, owner)
    torch.cuda.synchronize()
    for i in (a, b):
        assert (rows[int(offsets[i])] == SENTINEL).all() and owner[int(offsets[i])] == SENTINEL
    assert int((owner == SENTINEL).sum()) == 2 + 4
    # a fresh pool: no slot holds a checkpoint
    fresh = model.many_clause_checkpoints(4)
    slots = torch.arange(4, dtype=torch.int32, device="cuda")
    assert (model.clause_checkpoint_children(fresh, slots) == -1).all()
    assert _nothing_written(model, fresh, slots, torch.arange(5, dtype=torch.int64, device="cuda"), 4)
    # one count off by one: that instance writes nothing, the others write their rows where the offsets say
    slots = out["slot"].contiguous()
    c = int(stopped[2])
    claimed = good.clone()
    claimed[c] += 1
    offsets = _offsets(claimed)
    total = int(offsets[-1])
    rows, owner = _sentinel_rows(total, n)
    model.clause_checkpoint_fanout(pool, slots, offsets, total, rows, owner)
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
    model.clause_checkpoint_fanout(pool, slots, offsets, total - 1, rows, owner)
    torch.cuda.synchronize()
    last = int(stopped[-1])
    assert (rows[int(offsets[last]):] == SENTINEL).all() and (owner[int(offsets[last]):] == SENTINEL).all()
    assert (owner[:int(offsets[last])] != SENTINEL).all()


def test_a_checkpoint_of_another_objective_is_refused():
    """the header's code: MIN's 2 (schedule6_min_budget at its budget) and up-to-k's 4; each slot holds a whole
    checkpoint that resume_many_clauses goes on with, and the spread takes none of them"""
    text, roots, objective, budget = sets.build("schedule6_min_budget")
    assert objective == "MIN"
    model = _model(text)
    pool = model.many_clause_checkpoints(len(roots))
    out = model.solve_many_clauses(np.array(roots), "MIN", max_nodes=budget, checkpoints=pool)
    slots = out["slot"].contiguous()
    stopped = slots >= 0
    assert int(stopped.sum()) >= 4
    children = model.clause_checkpoint_children(pool, slots)
    assert (children[stopped] == -1).all() and (children[~stopped] == 0).all()
    claimed = stopped.to(torch.int64)
    assert _nothing_written(model, pool, slots, _offsets(claimed), int(claimed.sum()))

    text, roots, dev, _ = _set("linear20_all")
    model = _model(text)
    pool = model.many_clause_checkpoints(len(roots))
    out = model.solve_many_clauses_upto(dev, 1 << 20, max_nodes=8, solutions=False, checkpoints=pool)
    slots = out["slot"].contiguous()
    stopped = slots >= 0
    assert int(stopped.sum()) >= 4
    children = model.clause_checkpoint_children(pool, slots)
    assert (children[stopped] == -1).all() and (children[~stopped] == 0).all()
    claimed = stopped.to(torch.int64)
    assert _nothing_written(model, pool, slots, _offsets(claimed), int(claimed.sum()))
    # the same instances checkpointed under ALL in the same slots are taken
    pool.reset()
    out = model.solve_many_clauses(dev, "ALL", max_nodes=8, checkpoints=pool)
    assert (model.clause_checkpoint_children(pool, out["slot"].contiguous())[out["slot"] >= 0] >= 1).all()


def test_a_kernel_7_pool_is_refused():
    from csolve_amd import CsolveError, problems
    model = _model(problems.queens(8, "ALL"))  # a model of both families
    assert model.qualifies(7) and model.qualifies_many_clauses()
    dive_pool = model.many_checkpoints(4)
    slots = torch.zeros((4,), dtype=torch.int32, device="cuda")
    with pytest.raises(CsolveError, match="other kind") as e:
        model.clause_checkpoint_children(dive_pool, slots)
    assert e.value.code == -1
    with pytest.raises(CsolveError, match="other kind") as e:
        model.clause_checkpoint_fanout(dive_pool, slots, torch.arange(5, dtype=torch.int64, device="cuda"), 4)
    assert e.value.code == -1
    # and the kernel-7 pair keeps refusing a clause pool
    with pytest.raises(CsolveError, match="other kind"):
        model.checkpoint_children(model.many_clause_checkpoints(4), slots)


@pytest.mark.parametrize("budgets", BUDGETS, ids=lambda b: "-".join(map(str, b)))
@pytest.mark.parametrize("name", SPREAD_SETS)
def test_the_spread_is_the_one_all_call(name, budgets):
    text, roots, dev, _ = _set(name)
    want = _one_call(name)
    out = _model(text).solve_many_clauses_spread(dev, budgets=budgets)
    got = _host(out)
    print(f"{name} {budgets}: {len(roots)} owners, {out['rounds']} rounds, rows per round {out['round_rows']}")
    for f in FIELDS + ("first",):
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(roots), -1).any(axis=1))
        assert bad.size == 0, (f"{name} {budgets}: {f} differs for {bad.size} owners, first {bad[0]}: got {got[f][bad[0]]}, "
                               f"the one call {want[f][bad[0]]}")
    assert "slot" not in out and "best" not in out and out["sub_instances"] > 0 and out["rounds"] >= 2


def test_a_budget_nothing_stops_at_is_solve_many_clauses_itself():
    text, roots, dev, budget = _set("linear20_all")
    out = _model(text).solve_many_clauses_spread(dev, budgets=(budget,))
    assert out["rounds"] == 1 and out["sub_instances"] == 0 and out["round_rows"] == []
    got, want = _host(out), _one_call("linear20_all")
    for f in FIELDS + ("first",):
        assert (got[f] == want[f]).all(), f


def test_one_round_leaves_the_stopped_owners_at_limit():
    text, roots, dev, _ = _set("linear20_all")
    model = _model(text)
    out = model.solve_many_clauses_spread(dev, budgets=(8, 32), max_rounds=1)
    assert out["rounds"] == 1 and out["sub_instances"] == 0
    got, plain = _host(out), _host(model.solve_many_clauses(dev, "ALL", max_nodes=8))
    assert (plain["status"] == LIMIT).sum() > 8
    for f in FIELDS + ("first",):
        assert (got[f] == plain[f]).all(), f
    # and two rounds: the owners whose children all ended are DONE with the whole record, the others LIMIT
    want = _one_call("linear20_all")
    out = model.solve_many_clauses_spread(dev, budgets=(8, 32), max_rounds=2)
    got = _host(out)
    done = got["status"] == DONE
    assert out["rounds"] == 2 and out["sub_instances"] > 0 and (~done).any() and (got["status"][~done] == LIMIT).all()
    for f in FIELDS:
        assert (got[f][done] == want[f][done]).all(), f
    assert (got["nodes"][~done] < want["nodes"][~done]).all()


def test_max_rows_0_resumes_every_round_in_place():
    text, roots, dev, _ = _set("linear20_all")
    want = _one_call("linear20_all")
    out = _model(text).solve_many_clauses_spread(dev, budgets=(8, 4096), max_rows=0)
    got = _host(out)
    assert out["rounds"] >= 3 and out["sub_instances"] == 0 and out["round_rows"] == [0] * (out["rounds"] - 1)
    for f in FIELDS + ("first",):
        assert (got[f] == want[f]).all(), f


def test_a_model_that_does_not_qualify_is_refused_as_solve_many_clauses_refuses_it():
    from csolve_amd import CsolveError, problems
    model = _model(problems.schedule(32, 1))  # more than 512 clauses
    assert not model.qualifies_many_clauses()
    rows = np.repeat(model.domains()[None], 2, 0).astype(np.int32)
    for r in (rows, torch.from_numpy(rows).cuda()):
        with pytest.raises(CsolveError) as plain:
            model.solve_many_clauses(r, "ALL", max_nodes=8)
        with pytest.raises(CsolveError) as spread:
            model.solve_many_clauses_spread(r, budgets=(8, 32))
        assert spread.value.code == plain.value.code == -4 and str(spread.value) == str(plain.value) and "512" in str(spread.value)
