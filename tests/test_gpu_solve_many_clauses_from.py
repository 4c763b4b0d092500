"""GPU tests of the start incumbents (cs_walk_from behind csgpu_solve_many_clauses_from / _from_resume), of the fan-out
and the best-value fold for stopped MIN / MAX walks (csgpu_many_clause_checkpoint_children_obj / _fanout_obj,
csgpu_many_fold_best) and of Model.solve_many_clauses_spread(roots, "MIN" / "MAX") on top of them.  The yardsticks are the
host model of tests/many_clause_from_walk.py, node for node, and solve_many_clauses itself: the walk without a start and
the optimum of the one call.  Every call passes a finite max_nodes."""
import ctypes as C
import functools

import numpy as np
import pytest

import many_clause_from_walk as F
import many_clause_sets as sets
import many_walk_objective as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("status", "nodes", "cuts", "solutions")
EVERY = ("status", "root_props", "nodes", "cuts", "props", "solutions")
DONE, LIMIT, BAD_SLOT = 0, 1, 3
E_ARG = -1
SENTINEL = 0x5a5a5a5a
ENTRY_SETS = (("schedule5_min", None), ("wcet_max", None), ("schedule22_min_budget", 100))  # <1, false>, <1, true>, <8, false>
SPREADS = (("schedule5_min", (8, 32), 64), ("wcet_max", (8, 32), 64), ("schedule6_min_budget", (16, 64), 64),
           ("schedule22_min_budget", (16, 32), 2))


@functools.lru_cache(maxsize=None)
def _model(text):
    from csolve_amd.solver import solve_root
    return solve_root(text)


@functools.lru_cache(maxsize=None)
def _set(name):
    """(text, roots, roots on the device, objective, the set's budget), built once"""
    text, roots, objective, budget = sets.build(name)
    return text, roots, torch.from_numpy(np.array(roots)).cuda(), objective, budget


def _host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if torch.is_tensor(v) and not k.startswith("_")}


def _starts_of(values):
    """[None or a value] -> int32 [K, 2] {best, have} on the device; an absent start carries a value that must not be read"""
    return torch.tensor([[SENTINEL, 0] if v is None else [int(v), 1] for v in values], dtype=torch.int32).cuda()


@functools.lru_cache(maxsize=None)
def _mixed(name, budget):
    """per row one of: no start, the value the walk without a start ends with, one worse, one better, and a value that
    empties dom[obj] at the root -> (values, the host model's answers), computed once"""
    text, roots, _, objective, _ = _set(name)
    ov = W.model_of(text).view.obj_var
    worse = 1 if objective == "MIN" else -1
    values = []
    for i, row in enumerate(roots):
        ref = W.walk(text, row, objective, budget)
        base = ref["best"] if ref["best"] is not None else int(row[ov, 1] if objective == "MIN" else row[ov, 0])
        values.append((None, base, base + worse, base - worse, int(row[ov, 0] if objective == "MIN" else row[ov, 1]))[i % 5])
    want = [F.walk_from(text, row, objective, v, budget) for row, v in zip(roots, values)]
    return tuple(values), want


def _same_as_host(got, want, what):
    for i, w in enumerate(want):
        for f in FIELDS:
            assert got[f][i] == w[f], (what, i, f, got[f][i], w[f])
        if w["best"] is None:  # nothing of its own: best and the row are untouched
            assert got["best"][i] == 0 and (got["first"][i] == 0).all(), (what, i)
        else:
            assert got["best"][i] == w["best"] and (got["first"][i] == w["first"]).all(), (what, i)


@pytest.mark.parametrize("name,budget", ENTRY_SETS, ids=[s[0] for s in ENTRY_SETS])
def test_the_entry_is_the_host_model(name, budget):
    text, roots, dev, objective, set_budget = _set(name)
    budget = budget or set_budget
    model = _model(text)
    assert model.many_clauses_from_kernel() == sets.SETS[name][3].replace("cs_walk_clauses", "cs_walk_from")
    values, want = _mixed(name, budget)
    got = _host(model.solve_many_clauses(dev, objective, max_nodes=budget, start=_starts_of(values)))
    _same_as_host(got, want, name)
    kinds = [(w["status"], w["nodes"] > 0, w["solutions"] > 0) for w in want]
    print(f"{name}: {len(roots)} rows, {sum(v is not None for v in values)} with a start, "
          f"{sum(k == (DONE, False, False) for k in kinds)} dead at the root, "
          f"{sum(k == (DONE, True, False) for k in kinds)} that prove their start")
    assert (DONE, False, False) in kinds and any(k[2] for k in kinds)
    whole = sets.SETS[name][4]
    assert (DONE, True, False) in kinds or not whole  # (a whole set: a start at the optimum is proven)
    assert (LIMIT, True, False) in kinds or whole  # (the budget set: stopped with nothing of its own)


@pytest.mark.parametrize("name,budget", ENTRY_SETS, ids=[s[0] for s in ENTRY_SETS])
def test_no_start_anywhere_is_solve_many_clauses(name, budget):
    text, roots, dev, objective, set_budget = _set(name)
    budget = budget or set_budget
    model = _model(text)
    want = _host(model.solve_many_clauses(dev, objective, max_nodes=budget))
    got = _host(model.solve_many_clauses(dev, objective, max_nodes=budget, start=_starts_of([None] * len(roots))))
    for f in EVERY + ("first", "best"):
        assert (got[f] == want[f]).all(), (name, f)
    # and with a pool: the checkpointed call's answer, the slots among it
    pool, pool2 = model.many_clause_checkpoints(len(roots)), model.many_clause_checkpoints(len(roots))
    want = _host(model.solve_many_clauses(dev, objective, max_nodes=16, checkpoints=pool))
    got = _host(model.solve_many_clauses(dev, objective, max_nodes=16, checkpoints=pool2, start=_starts_of([None] * len(roots))))
    for f in EVERY + ("first", "best"):
        assert (got[f] == want[f]).all(), (name, f)
    assert ((got["slot"] >= 0) == (want["slot"] >= 0)).all() and (got["slot"] >= 0).any()


def test_slices_add_up_and_an_untouched_best_stays_untouched():
    """budget 16 with a pool, then 48 more through csgpu_solve_many_clauses_from_resume, is one call with 64; a slot of
    another code is refused (an ALL checkpoint: a pool belongs to one model, and a model is searched in its own sense
    only, so a checkpoint of the other SENSE cannot be made in it -- the kernel compares the one header code)"""
    name = "schedule6_min_budget"
    text, roots, dev, objective, _ = _set(name)
    model = _model(text)
    values, _ = _mixed(name, 64)
    start = _starts_of(values)
    whole = _host(model.solve_many_clauses(dev, objective, max_nodes=64, start=start))
    pool = model.many_clause_checkpoints(len(roots))
    out = model.solve_many_clauses(dev, objective, max_nodes=16, checkpoints=pool, start=start)
    first = _host(out)
    stopped = first["status"] == LIMIT
    assert stopped.sum() >= 4 and (first["slot"][stopped] >= 0).all() and (stopped & (first["solutions"] == 0)).any()
    out["_best"][out["solutions"] == 0] = SENTINEL
    model.resume_many_clauses(out, max_nodes=48, own_solutions=True)
    got = _host(out)
    for f in EVERY + ("first",):
        assert (got[f] == whole[f]).all(), f
    found = whole["solutions"] > 0
    assert (got["best"][found] == whole["best"][found]).all()
    untouched = ~found & (first["solutions"] == 0)
    assert untouched.any() and (got["best"][untouched] == SENTINEL).all() and (whole["best"][~found] == 0).all()
    assert (untouched & stopped).any(), "an instance that was resumed and found nothing of its own"
    # the other resume continues the same checkpoints: the same records and rows
    pool.reset()
    out = model.solve_many_clauses(dev, objective, max_nodes=16, checkpoints=pool, start=start)
    model.resume_many_clauses(out, max_nodes=48)
    other = _host(out)
    for f in EVERY + ("first",):
        assert (other[f] == whole[f]).all(), f
    # and a checkpoint of csgpu_solve_many_clauses_checkpointed goes on through the new resume
    pool.reset()
    plain = _host(model.solve_many_clauses(dev, objective, max_nodes=64))
    out = model.solve_many_clauses(dev, objective, max_nodes=16, checkpoints=pool)
    model.resume_many_clauses(out, max_nodes=48, own_solutions=True)
    got = _host(out)
    for f in EVERY + ("first", "best"):
        assert (got[f] == plain[f]).all(), f
    # another code in the header: BAD_SLOT, nothing else of the instance is written
    pool.reset()
    out = model.solve_many_clauses(dev, "ALL", max_nodes=16, checkpoints=pool)
    before = _host(out)
    had = before["slot"] >= 0
    assert had.sum() >= 4
    out["_objective"] = W.CODE[objective]
    model.resume_many_clauses(out, max_nodes=48, own_solutions=True)
    got = _host(out)
    assert (got["status"][had] == BAD_SLOT).all() and (got["status"][~had] == before["status"][~had]).all()
    for f in EVERY[1:] + ("first", "slot"):
        assert (got[f] == before[f]).all(), f


def test_the_entries_refuse_what_is_theirs_after_the_errors_of_solve_many_clauses():
    from csolve_amd import problems
    from csolve_amd._lib import ManyOptions, load_library
    L = load_library()
    text, roots, dev, objective, _ = _set("schedule5_min")
    model = _model(text)
    K = len(roots)
    res = torch.full((K, 5), 77, dtype=torch.int64, device="cuda")
    start = _starts_of([None] * K)
    slots = torch.full((K,), 77, dtype=torch.int32, device="cuda")
    pool = model.many_clause_checkpoints(2)
    queens = _model(problems.queens(8, "ALL"))
    opt = ManyOptions(2, 0, 100)

    def fresh(st=start.data_ptr(), o=opt, ck=None, sl=None, count=K):
        return L.csgpu_solve_many_clauses_from(model._h, dev.data_ptr(), st, count, C.byref(o), res.data_ptr(), None, None, ck, sl, None)

    def resume(o=opt, ck=pool._h, sl=slots.data_ptr(), count=K):
        return L.csgpu_solve_many_clauses_from_resume(model._h, count, C.byref(o), res.data_ptr(), None, None, ck, sl, None)

    def refused(rc, *words):
        msg = L.csgpu_last_error().decode()
        assert rc == E_ARG and all(w in msg for w in words), (rc, msg)

    refused(fresh(st=None), "d_start")
    refused(fresh(st=None, o=ManyOptions(1, 0, 100)), "d_start")  # the start comes before the objective
    for code in (0, 1):
        refused(fresh(o=ManyOptions(code, 0, 100)), "MIN / MAX")
        refused(fresh(o=ManyOptions(code, 0, 100), ck=pool._h), "MIN / MAX")  # the objective before the pool
        refused(resume(o=ManyOptions(code, 0, 100)), "MIN / MAX")
    refused(fresh(ck=pool._h), "pool")
    refused(fresh(sl=slots.data_ptr()), "pool")
    refused(resume(ck=None), "pool")
    refused(resume(sl=None), "pool")
    refused(resume(ck=None, sl=None), "pool")
    foreign = queens.many_clause_checkpoints(2)
    refused(fresh(ck=foreign._h, sl=slots.data_ptr()), "another model")
    refused(fresh(ck=pool._h, sl=slots.data_ptr(), count=-1), "negative")
    assert fresh(count=0) == 0 and fresh(ck=pool._h, sl=slots.data_ptr(), count=0) == 0 and resume(count=0) == 0
    torch.cuda.synchronize()
    assert (res == 77).all() and (slots == 77).all()
    from csolve_amd import CsolveError
    with pytest.raises(CsolveError) as e:
        model.solve_many_clauses(dev, "ALL", max_nodes=10, start=start)
    assert e.value.code == E_ARG


@functools.lru_cache(maxsize=None)
def _stopped(budget=16):
    """schedule6_min_budget checkpointed under MIN with `budget` on the device and stopped on the host"""
    text, roots, dev, objective, _ = _set("schedule6_min_budget")
    model = _model(text)
    pool = model.many_clause_checkpoints(len(roots))
    out = model.solve_many_clauses(dev, objective, max_nodes=budget, checkpoints=pool)
    walks = [F.From(text, row, objective) for row in roots]
    records = [w.run(budget) for w in walks]
    kids = [F.children_of(w) if r["status"] == LIMIT else None for w, r in zip(walks, records)]
    return model, pool, out, walks, kids


def _offsets(children):
    off = torch.zeros((children.shape[0] + 1,), dtype=torch.int64, device=children.device)
    torch.cumsum(children.clamp(min=0), 0, out=off[1:])
    return off


def _sentinels(total, n, guard=4):
    return (torch.full((total + guard, n, 2), SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((total + guard,), SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((total + guard, 2), SENTINEL, dtype=torch.int32, device="cuda"))


def test_the_fan_out_lists_the_children_and_what_they_start_with():
    model, pool, out, walks, kids = _stopped()
    K, n = len(kids), model.n_vars
    stopped = [i for i in range(K) if kids[i] is not None]
    assert len(stopped) >= 4
    slots = out["slot"].contiguous()
    assert ((_host(out)["slot"] >= 0) == np.array([k is not None for k in kids])).all()
    children = model.clause_checkpoint_children(pool, slots, objective="MIN")
    want_children = np.array([0 if k is None else len(k) for k in kids])
    assert (children.cpu().numpy() == want_children).all()
    assert (model.clause_checkpoint_children(pool, slots)[slots >= 0] == -1).all()  # the ALL-only call keeps refusing them
    total = int(want_children.sum())
    offsets = _offsets(children)
    want_rows = np.concatenate([kids[i] for i in stopped])
    want_owner = np.concatenate([np.full(len(kids[i]), i) for i in stopped])
    incumbents = [walks[i].incumbent for i in range(K)]
    assert any(b is None for i, b in enumerate(incumbents) if kids[i] is not None) and \
        any(b is not None for i, b in enumerate(incumbents) if kids[i] is not None)
    # what the owners hold: nothing, a value that beats the checkpoint's, the checkpoint's own value, a worse one
    held = []
    for i, b in enumerate(incumbents):
        held.append((None, 20 if b is None else b - 1, 30 if b is None else b, 40 if b is None else b + 1)[i % 4])
    for owner_start in (None, held):
        rows, owner, start = _sentinels(total, n)
        model.clause_checkpoint_fanout(pool, slots, offsets, total, rows, owner, objective="MIN", start=start,
                                       owner_start=None if owner_start is None else _starts_of(owner_start))
        torch.cuda.synchronize()
        assert (rows[:total].cpu().numpy() == want_rows).all() and (owner[:total].cpu().numpy() == want_owner).all()
        want_start = []
        for i in stopped:
            b = incumbents[i]
            if owner_start is not None and owner_start[i] is not None and F.better(1, owner_start[i], b):
                b = owner_start[i]
            want_start.extend([[0, 0] if b is None else [b, 1]] * len(kids[i]))
        assert (start[:total].cpu().numpy() == np.array(want_start)).all()
        assert (rows[total:] == SENTINEL).all() and (owner[total:] == SENTINEL).all() and (start[total:] == SENTINEL).all()
    # one count off by one: that instance writes nothing at all
    c = stopped[1]
    claimed = children.clone()
    claimed[c] += 1
    off = _offsets(claimed)
    rows, owner, start = _sentinels(total + 1, n)
    model.clause_checkpoint_fanout(pool, slots, off, total + 1, rows, owner, objective="MIN", start=start)
    torch.cuda.synchronize()
    lo, hi = int(off[c]), int(off[c + 1])
    assert (rows[lo:hi] == SENTINEL).all() and (owner[lo:hi] == SENTINEL).all() and (start[lo:hi] == SENTINEL).all()
    assert int((owner == SENTINEL).sum()) == hi - lo + 4
    # asked for MAX's checkpoints: there are none
    assert (model.clause_checkpoint_children(pool, slots, objective="MAX")[slots >= 0] == -1).all()
    # an ALL checkpoint is refused, and nothing is written for it
    text, roots, dev, _, _ = _set("schedule6_min_budget")
    pool2 = model.many_clause_checkpoints(K)
    out2 = model.solve_many_clauses(dev, "ALL", max_nodes=16, checkpoints=pool2)
    slots2 = out2["slot"].contiguous()
    had = slots2 >= 0
    assert int(had.sum()) >= 4
    kids2 = model.clause_checkpoint_children(pool2, slots2, objective="MIN")
    assert (kids2[had] == -1).all() and (kids2[~had] == 0).all()
    claimed = had.to(torch.int64)
    rows, owner, start = _sentinels(int(claimed.sum()), n)
    model.clause_checkpoint_fanout(pool2, slots2, _offsets(claimed), int(claimed.sum()), rows, owner, objective="MIN", start=start)
    torch.cuda.synchronize()
    assert (rows == SENTINEL).all() and (owner == SENTINEL).all() and (start == SENTINEL).all()


@pytest.mark.parametrize("objective", ["MIN", "MAX"])
def test_the_best_fold_is_numpys(objective):
    model = _model(_set("schedule5_min")[0])
    #          row:  0   1   2   3   4    5   6   7   8   9  10  11
    owner = np.array([0,  1,  0, -1,  2,   1,  0,  4,  2,  4,  1, -5], dtype=np.int32)
    best = np.array([7, -3,  7, -9, 40,  -3,  5, 11, 40, 11, -4,  0], dtype=np.int32)
    sols = np.array([1,  2,  1,  1,  0,   1,  3,  1,  0,  1,  0,  1], dtype=np.int64)
    K = 6  # owner 2 has rows without solutions only, owners 3 and 5 have no rows
    records = np.zeros((len(owner), 5), dtype=np.int64)
    records[:, 4] = sols
    sub = {"status": torch.zeros(len(owner), dtype=torch.int32, device="cuda"), "_records": torch.from_numpy(records).cuda(),
           "best": torch.from_numpy(best).cuda()}
    has, value, row = model.fold_many_best(sub, torch.from_numpy(owner).cuda(), K, objective)
    torch.cuda.synchronize()
    for o in range(K):
        mine = [t for t in range(len(owner)) if owner[t] == o and sols[t] > 0]
        assert bool(has[o]) == bool(mine)
        if mine:
            top = min(best[t] for t in mine) if objective == "MIN" else max(best[t] for t in mine)
            assert int(value[o]) == top and int(row[o]) == min(t for t in mine if best[t] == top), o
        else:
            assert int(value[o]) == 0 and int(row[o]) == 0
    assert value.dtype == torch.int32 and has.dtype == torch.bool


@functools.lru_cache(maxsize=None)
def _one_call(name):
    """solve_many_clauses(roots, objective, max_nodes = 2^22) on the device (computed once, not to be changed)"""
    text, _, dev, objective, _ = _set(name)
    return _host(_model(text).solve_many_clauses(dev, objective, max_nodes=1 << 22))


@pytest.mark.parametrize("name,budgets,max_rounds", SPREADS, ids=[s[0] for s in SPREADS])
def test_the_spread_is_the_host_model(name, budgets, max_rounds):
    text, roots, dev, objective, _ = _set(name)
    want, info = F.spread_minmax(text, roots, objective, budgets, max_rounds)
    out = _model(text).solve_many_clauses_spread(dev, objective, budgets=budgets, max_rounds=max_rounds)
    got = _host(out)
    print(f"{name} {budgets}: {len(roots)} owners, {out['rounds']} rounds, rows per round {out['round_rows']}, {info}")
    assert out["rounds"] == info["rounds"] and out["sub_instances"] == info["sub_instances"]
    assert out["round_rows"] == info["per_round"]
    _same_as_host(got, want, name)
    assert "slot" not in out


@pytest.mark.parametrize("name,budgets,max_rounds", SPREADS[:3], ids=[s[0] for s in SPREADS[:3]])
def test_the_spread_proves_the_optimum_of_the_one_call(name, budgets, max_rounds):
    text, roots, dev, objective, _ = _set(name)
    model = _model(text)
    want = _one_call(name)
    assert (want["status"] == DONE).all()
    booked, solve = [], model.solve_many_clauses

    def recording(*args, **kw):
        ans = solve(*args, **kw)
        booked.append((ans["root_props"].clone(), ans["props"].clone()))
        return ans

    model.solve_many_clauses = recording
    try:
        out = model.solve_many_clauses_spread(dev, objective, budgets=budgets)
    finally:
        del model.solve_many_clauses
    got = _host(out)
    assert (got["status"] == DONE).all() and (got["best"] == want["best"]).all()
    assert (got["nodes"] >= want["nodes"]).all() and (got["solutions"] >= 1).all()
    ov = model.objective_var
    assert (got["first"][:, ov] == got["best"]).all()
    # props: what the kernel itself booked -- round 0's, and root_props + props of every sub-row
    assert len(booked) == out["rounds"]
    total = int(booked[0][1].sum()) + sum(int(r.sum()) + int(p.sum()) for r, p in booked[1:])
    assert int(got["props"].sum()) == total and (got["root_props"] == booked[0][0].cpu().numpy()).all()


def test_max_rows_0_resumes_in_place_and_still_proves_the_optimum():
    name = "schedule6_min_budget"
    text, roots, dev, objective, _ = _set(name)
    want = _one_call(name)
    assert want["nodes"].max() > 16 + 64  # so the second resume has work left
    out = _model(text).solve_many_clauses_spread(dev, objective, budgets=(16, 64, 4096), max_rows=0)
    got = _host(out)
    assert out["rounds"] >= 3 and out["sub_instances"] == 0 and out["round_rows"] == [0] * (out["rounds"] - 1)
    assert (got["status"] == DONE).all() and (got["best"] == want["best"]).all()
    for f in EVERY + ("first",):  # resumed in place, round 0 is the one walk
        assert (got[f] == want[f]).all(), f
    # a fan-out too wide in a later round: the sub-instances go on in place, under the own-solutions rule
    wide = _model(text).solve_many_clauses_spread(dev, objective, budgets=(16, 16, 4096), max_rows=800)
    got = _host(wide)
    assert wide["round_rows"][0] == 716 and wide["round_rows"][1] == 0
    assert (got["status"] == DONE).all() and (got["best"] == want["best"]).all()


def test_all_is_the_spread_it_was():
    text, roots, dev, _, _ = _set("linear20_all")
    model = _model(text)
    a = model.solve_many_clauses_spread(dev, budgets=(8, 32))
    b = model.solve_many_clauses_spread(dev, "ALL", budgets=(8, 32))
    assert a["rounds"] == b["rounds"] >= 2 and a["round_rows"] == b["round_rows"] and "best" not in a and "best" not in b
    ga, gb = _host(a), _host(b)
    assert set(ga) == set(gb)
    for f in ga:
        assert (ga[f] == gb[f]).all(), f
