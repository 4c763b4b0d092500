"""GPU tests of the ordered clause checkpoints (cs_walk_order_resume: csgpu_solve_many_clauses_ordered_checkpointed / _resume,
csgpu_many_clause_checkpoint_states on an ordered pool) and of Model.solve_many_clauses_sliced(..., order=).  Yardsticks:
the host walk of tests/many_walk_ordered.py for the counters after every slice, and Model.solve_many_clauses_ordered with
ONE budget -- which test_gpu_solve_many_clauses_ordered.py pins to that walk -- for every field at the end, props and the
stored rows included.  The slices are those of tests/many_ordered_resume_walk.py, which
test_solve_many_clauses_ordered_resume_host.py shows to stop instances between halves, above halving parents and on stacks
deeper than n_vars.  Every call passes a finite max_nodes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import many_clause_resume_walk
import many_clause_sets as sets
import many_ordered_resume_walk as R
import many_walk_objective as W
import many_walk_ordered as O
from csolve_amd._lib import CsolveError, ManyOptions, ManyOrderOptions, ManyStream, ManyUptoOptions, load_library
from csolve_amd.solver import Model, solve_root
from test_solve_many_clauses_ordered_resume_host import order_resume_kernel_of, shipped

pytestmark = pytest.mark.gpu

E_ARG = -1
DONE, LIMIT, BAD_SLOT = 0, 1, 3
COUNTERS = ("status", "nodes", "cuts", "solutions", "halvings")
EVERY = COUNTERS + ("props", "root_props", "first")
POISON = 0x5a5a5a5a
POISON64 = 0x5a5a5a5a5a5a5a5a


@functools.lru_cache(maxsize=None)
def model_of(text):
    return solve_root(text)


def host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


@functools.lru_cache(maxsize=None)
def one_call(name, order, split, budget=None):
    """the one solve_many_clauses_ordered call of a case, at its budget or another (computed once, not to be changed)"""
    text, roots, objective, own = O.build(name)
    return host(model_of(text).solve_many_clauses_ordered(np.array(roots), objective, max_nodes=own if budget is None else budget,
                                                          order=order, split_width=split))


def same(got, want, objective, label, rows=None, fields=EVERY):
    """the fields of every instance, and `best` where the instance has a solution under MIN / MAX"""
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    for f in fields:
        g, w = pick(got[f]), pick(want[f])
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if len(g) else np.zeros(0, dtype=int)
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}"
    if objective in ("MIN", "MAX"):
        has = pick(want["solutions"]) > 0
        assert (pick(got["best"])[has] == pick(want["best"])[has]).all(), f"{label}: best"


def slots_are_sound(got, capacity, label):
    stopped = got["status"] == LIMIT
    assert ((got["slot"] >= 0) == stopped).all(), f"{label}: a slot without a stop, or a stop without a slot"
    used = got["slot"][stopped]
    assert len(set(used.tolist())) == len(used) and (used < capacity).all(), f"{label}: slots {used}"


@pytest.mark.parametrize("name,order,split", O.CASES)
def test_a_walk_in_slices_is_the_one_call(name, order, split):
    text, roots, objective, budget = O.build(name)
    model = model_of(text)
    K = len(roots)
    dev = torch.from_numpy(np.array(roots)).cuda()
    pool = model.many_clause_ordered_checkpoints(K, split)
    assert pool.frames == O.frames(W.oracle_for(text)[1], split) and pool.clauses and pool.ordered
    after, _ = R.sliced(name, order, split)
    steps, total, stopped = R.slices(name), 0, []
    for k, b in enumerate(steps):
        if k == 0:
            out = model.solve_many_clauses_ordered(dev, objective, max_nodes=b, order=order, split_width=split, checkpoints=pool)
        else:
            assert model.resume_many_clauses(out, max_nodes=b) is out
        total += b
        got = host(out)
        label = f"{name} {order}/{split} after {steps[:k + 1]}"
        same(got, after[k], objective, label + " against the host walk", fields=COUNTERS)
        slots_are_sound(got, K, label)
        limit = got["status"] == LIMIT
        assert (got["nodes"][limit] == total).all(), label
        stopped.append(int(limit.sum()))
    print(f"{name} {order}/{split}: {K} instances, stopped after each of {steps}: {stopped}")
    assert total == budget and stopped[0] > 0 and (objective == "ANY" or (stopped[1] > 0 and stopped[2] > 0))
    same(got, one_call(name, order, split), objective, f"{name} {order}/{split} at the end against the one call")
    assert ((got["first"] == 0).all(axis=1) | (got["solutions"] > 0)).all()
    pool.close()


@pytest.mark.parametrize("name", sorted(sets.SETS))
def test_nothing_changes_where_nothing_halves(name):
    """smallest-domain and a split_width of the widest interval: the sliced ordered walk is the plain call, props included"""
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    widest = int((roots[:, :, 1].astype(np.int64) - roots[:, :, 0] + 1).max())
    plain = host(model.solve_many_clauses(np.array(roots), objective, max_nodes=budget))
    out = model.solve_many_clauses_sliced(torch.from_numpy(np.array(roots)).cuda(), objective,
                                          budgets=many_clause_resume_walk.slices(name), order="smallest-domain", split_width=widest)
    got = host(out)
    assert set(got) == set(plain) | {"halvings", "slot"}
    for f in plain:
        assert (got[f] == plain[f]).all(), f
    assert (got["halvings"] == 0).all() and ((got["slot"] >= 0) == (got["status"] == LIMIT)).all()
    assert out["sliced"]["searched"] == 0 and out["sliced"]["slices"] >= 3
    assert model.many_clauses_order_resume_kernel() == order_resume_kernel_of(sets.SETS[name][3])


def test_the_sets_plan_every_shipped_instantiation():
    planned = {model_of(sets.build(name)[0]).many_clauses_order_resume_kernel() for name in sets.SETS}
    assert planned == shipped("cs_walk_order_resume") and len(planned) == 8


def test_deep_stacks_and_their_states():
    """three copies of wide2_cut's root row under ALL, split_width 1: F = 31 frames for 5 variables; at 8 and 64 nodes the
    states of a slot are the host walk's open subtrees, more of them than n_vars"""
    name, order, split = R.DEEP
    text, roots, whole = R.all_row(name, order, split)
    model = model_of(text)
    n = model.n_vars
    rows = np.repeat(roots, 3, 0)
    pool = model.many_clause_ordered_checkpoints(3, split)
    assert pool.frames == 31 and model.clause_ordered_checkpoint_bytes(split) == 32 * (n + 1) * 8
    out = None
    for total, b in ((8, 8), (64, 56)):
        if out is None:
            out = model.solve_many_clauses_ordered(rows, "ALL", max_nodes=b, order=order, split_width=split, checkpoints=pool)
        else:
            model.resume_many_clauses(out, max_nodes=b)
        got = host(out)
        res, want, frames = R.stopped_all(name, order, split, total)
        assert frames > n and (got["status"] == LIMIT).all()
        slots_are_sound(got, 3, f"after {total}")
        for f in COUNTERS[1:]:
            assert (got[f] == res[f]).all(), (total, f)
        for i in range(3):
            states, best = model.clause_checkpoint_states(pool, int(got["slot"][i]))
            assert best is None and tuple(states.shape) == want.shape and (states.cpu().numpy() == want).all(), (total, i)
            open_states, complete, _ = model.open_clause_subtrees(pool, int(got["slot"][i]))
            assert open_states.shape[0] + complete.shape[0] <= frames
    model.resume_many_clauses(out, max_nodes=R.ALL_BUDGET - 64)
    got = host(out)
    one = host(model.solve_many_clauses_ordered(rows, "ALL", max_nodes=R.ALL_BUDGET, order=order, split_width=split))
    same(got, one, "ALL", "the deep rows at the end")
    assert (got["status"] == DONE).all() and (got["solutions"] == 260).all() and (got["halvings"] == whole["halvings"]).all()
    assert (got["slot"] == -1).all()
    with pytest.raises(CsolveError) as e:
        model.clause_checkpoint_states(pool, 3)
    assert e.value.code == E_ARG


SPLIT6 = ("schedule6_min_budget", "smallest-domain", 4)


def test_instances_without_a_slot_are_not_touched():
    name, order, split = SPLIT6
    text, roots, objective, budget = O.build(name)
    model = model_of(text)
    pool = model.many_clause_ordered_checkpoints(len(roots), split)
    out = model.solve_many_clauses_ordered(np.array(roots), objective, max_nodes=budget - 56, order=order, split_width=split,
                                           checkpoints=pool)
    before = host(out)
    done = np.flatnonzero(before["slot"] < 0)
    left = np.flatnonzero(before["slot"] >= 0)
    assert done.size >= 2 and left.size >= 2, "the budget must split the set"
    idx = torch.from_numpy(done).cuda()
    out["_records"][idx] = POISON64
    out["first"][idx] = POISON
    out["_best"][idx] = POISON
    out["_halvings"][idx] = POISON64
    model.resume_many_clauses(out, max_nodes=56)
    torch.cuda.synchronize()
    assert (out["_records"][idx] == POISON64).all() and (out["first"][idx] == POISON).all()
    assert (out["_best"][idx] == POISON).all() and (out["_halvings"][idx] == POISON64).all() and (out["slot"][idx] == -1).all()
    same(host(out), one_call(name, order, split), objective, "the resumed rows", rows=left)


def test_bad_slots_get_their_status_and_nothing_else():
    """a resume under another order, under another objective, a slot number outside the pool and a slot of a fresh pool
    that holds nothing: CSGPU_MANY_BAD_SLOT, only the status word written"""
    name, order, split = "schedule5_open_min", "none", 4
    text, roots, objective, budget = O.build(name)
    model = model_of(text)
    K = len(roots)
    dev = torch.from_numpy(np.array(roots)).cuda()
    pool = model.many_clause_ordered_checkpoints(K + 2, split)  # two slots are never drawn: they stay zeroed
    keep = EVERY[1:] + ("slot", "best")

    def first_slice():
        pool.reset()
        out = model.solve_many_clauses_ordered(dev, objective, max_nodes=64, order=order, split_width=split, checkpoints=pool)
        return out, host(out)

    out, before = first_slice()
    had = before["slot"] >= 0
    assert had.sum() >= 6 and (~had).any() and before["slot"].max() < K
    for key, other in (("_order", Model.MANY_ORDERS["largest-value"]), ("_objective", W.CODE["ALL"])):
        mine = out[key]
        out[key] = other
        model.resume_many_clauses(out, max_nodes=budget)
        got = host(out)
        assert (got["status"][had] == BAD_SLOT).all() and (got["status"][~had] == before["status"][~had]).all(), key
        for f in keep:
            assert (got[f] == before[f]).all(), (key, f)
        out[key] = mine
        out["status"][torch.from_numpy(np.flatnonzero(had)).cuda()] = LIMIT
    # and under what it was made under it goes on, but for the two whose slot numbers are spoilt
    stopped = np.flatnonzero(had)
    a, b = int(stopped[1]), int(stopped[3])
    out["slot"][a] = K + 2      # the first number past the pool
    out["slot"][b] = K + 1      # inside the pool, never written
    model.resume_many_clauses(out, max_nodes=budget - 64)
    got = host(out)
    assert got["status"][a] == BAD_SLOT and got["status"][b] == BAD_SLOT
    assert got["slot"][a] == K + 2 and got["slot"][b] == K + 1
    for f in EVERY[1:] + ("best",):
        assert (got[f][[a, b]] == before[f][[a, b]]).all(), f
    others = np.setdiff1d(np.arange(K), [a, b])
    same(got, one_call(name, order, split), objective, "the neighbours", rows=others)


def test_the_kinds_of_pool_are_not_mixed():
    """CSGPU_E_ARG before anything is launched: the sentinels in the records stay"""
    name, order, split = "schedule5_open_min", "none", 4
    text, roots, objective, budget = O.build(name)
    model = model_of(text)
    K, n = len(roots), model.n_vars
    dev = torch.from_numpy(np.array(roots)).cuda()
    L = load_library()
    plain_pool, ordered, other_split = (model.many_clause_checkpoints(K), model.many_clause_ordered_checkpoints(K, split),
                                        model.many_clause_ordered_checkpoints(K, 0))
    assert other_split.frames == model.many_clauses_ordered_frames(256) != ordered.frames
    res = torch.full((K, 5), -77, dtype=torch.int64, device="cuda")
    slots = torch.full((K,), -1, dtype=torch.int32, device="cuda")
    halv = torch.full((K,), -77, dtype=torch.int64, device="cuda")
    rows = torch.full((K, 2, n), -77, dtype=torch.int32, device="cuda")
    best = torch.full((K,), -77, dtype=torch.int32, device="cuda")
    opt = ManyOrderOptions(W.CODE[objective], 0, split, 0, 64)

    def ordered_calls(ck, hv, o=opt):
        a = L.csgpu_solve_many_clauses_ordered_checkpointed(model._h, dev.data_ptr(), K, C.byref(o), res.data_ptr(), None,
                                                            best.data_ptr(), hv, ck, slots.data_ptr(), None)
        b = L.csgpu_solve_many_clauses_ordered_resume(model._h, K, C.byref(o), res.data_ptr(), None, best.data_ptr(), hv, ck,
                                                      slots.data_ptr(), None)
        return a, b, L.csgpu_last_error().decode()

    a, b, msg = ordered_calls(plain_pool._h, halv.data_ptr())  # a plain clause pool
    assert a == b == E_ARG and "other kind" in msg
    a, b, msg = ordered_calls(other_split._h, halv.data_ptr())  # made for 256
    assert a == b == E_ARG and "split_width" in msg
    a, b, msg = ordered_calls(ordered._h, halv.data_ptr(), ManyOrderOptions(W.CODE[objective], 0, 0, 0, 64))  # 0 is 256
    assert a == b == E_ARG and "split_width" in msg
    a, b, msg = ordered_calls(ordered._h, None)  # d_halvings NULL
    assert a == b == E_ARG and "d_halvings" in msg
    a, b, msg = ordered_calls(None, halv.data_ptr())
    assert a == b == E_ARG
    # d_halvings comes before the pool, the order before d_halvings
    assert "d_halvings" in ordered_calls(plain_pool._h, None)[2]
    assert "order" in ordered_calls(plain_pool._h, None, ManyOrderOptions(W.CODE[objective], 7, split, 0, 64))[2]
    # an ordered pool given to every other entry that takes a clause pool
    mo, uo = ManyOptions(W.CODE[objective], 0, 64), ManyUptoOptions(2, 0, 64)
    stream = model.many_stream(8)
    st = stream.struct()
    assert isinstance(st, ManyStream)
    count64 = torch.full((K + 1,), -77, dtype=torch.int64, device="cuda")
    refused = [
        L.csgpu_solve_many_clauses_checkpointed(model._h, dev.data_ptr(), K, C.byref(mo), res.data_ptr(), None, best.data_ptr(),
                                                ordered._h, slots.data_ptr(), None),
        L.csgpu_solve_many_clauses_resume(model._h, K, C.byref(mo), res.data_ptr(), None, best.data_ptr(), ordered._h,
                                          slots.data_ptr(), None),
        L.csgpu_solve_many_clauses_upto_checkpointed(model._h, dev.data_ptr(), K, C.byref(uo), res.data_ptr(), rows.data_ptr(),
                                                     ordered._h, slots.data_ptr(), None),
        L.csgpu_solve_many_clauses_upto_resume(model._h, K, C.byref(uo), res.data_ptr(), rows.data_ptr(), ordered._h,
                                               slots.data_ptr(), None),
        L.csgpu_solve_many_clauses_from_resume(model._h, K, C.byref(mo), res.data_ptr(), None, best.data_ptr(), ordered._h,
                                               slots.data_ptr(), None),
        L.csgpu_solve_many_clauses_stream(model._h, dev.data_ptr(), K, C.byref(ManyOptions(1, 0, 64)), res.data_ptr(), ordered._h,
                                          slots.data_ptr(), C.byref(st), None),
        L.csgpu_many_clause_checkpoint_children(ordered._h, slots.data_ptr(), K, count64.data_ptr(), None),
        L.csgpu_many_clause_checkpoint_fanout(ordered._h, slots.data_ptr(), K, count64.data_ptr(), dev.data_ptr(), None, 4, None),
        L.csgpu_many_clause_checkpoint_children_obj(ordered._h, slots.data_ptr(), K, W.CODE[objective], count64.data_ptr(), None),
    ]
    assert refused == [E_ARG] * len(refused), refused
    assert "other kind" in L.csgpu_last_error().decode()
    # the Python calls say the same
    with pytest.raises(CsolveError, match="other kind") as e:
        model.solve_many_clauses(dev, objective, max_nodes=4, checkpoints=ordered)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError, match="other kind") as e:
        model.solve_many_clauses_upto(dev, 2, max_nodes=4, checkpoints=ordered)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError, match="other kind") as e:
        model.solve_many_clauses_ordered(dev, objective, max_nodes=4, order=order, split_width=split, checkpoints=plain_pool)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError, match="split_width") as e:
        model.solve_many_clauses_ordered(dev, objective, max_nodes=4, order=order, split_width=split, checkpoints=other_split)
    assert e.value.code == E_ARG
    torch.cuda.synchronize()
    for t in (res, halv, rows, best, count64):
        assert (t == -77).all()
    assert (slots == -1).all() and (dev.cpu().numpy() == roots).all()
    # a negative split_width makes no pool
    with pytest.raises(CsolveError) as e:
        model.many_clause_ordered_checkpoints(4, -1)
    assert e.value.code == E_ARG
    # all three kinds work side by side on the one model
    a = host(model.solve_many_clauses_ordered(dev, objective, max_nodes=64, order=order, split_width=split, checkpoints=ordered))
    same(a, one_call(name, order, split, 64), objective, "beside the other pools")
    assert (host(model.solve_many_clauses(dev, objective, max_nodes=8, checkpoints=plain_pool))["slot"] >= 0).any()


def test_a_full_pool_ends_an_instance_as_without_checkpoints():
    name, order, split = "schedule5_open_min", "none", 4
    text, roots, objective, budget = O.build(name)
    model = model_of(text)
    K, capacity = len(roots), 3
    dev = torch.from_numpy(np.array(roots)).cuda()
    pool = model.many_clause_ordered_checkpoints(capacity, split)
    part = one_call(name, order, split, 64)
    assert int((part["status"] == LIMIT).sum()) > capacity
    out = model.solve_many_clauses_ordered(dev, objective, max_nodes=64, order=order, split_width=split, checkpoints=pool)
    got = host(out)
    same(got, part, objective, "budget 64, three slots")
    kept = np.flatnonzero(got["slot"] >= 0)
    rest = np.setdiff1d(np.arange(K), kept)
    assert kept.size == capacity and sorted(got["slot"][kept].tolist()) == list(range(capacity))
    assert (got["status"][kept] == LIMIT).all() and (got["slot"][rest] == -1).all()
    model.resume_many_clauses(out, max_nodes=budget - 64)
    got = host(out)
    same(got, one_call(name, order, split), objective, "the three with a slot", rows=kept)
    same(got, part, objective, "everything else", rows=rest)
    assert (got["slot"] == -1).all()


def test_four_calls_queued_on_one_stream():
    """8, 24, 32 and the rest with no host synchronisation in between, on 32 rows: the one call"""
    name, order, split = "schedule5_open_min", "smallest-domain", 256
    text, roots, objective, budget = O.build(name)
    model = model_of(text)
    big = torch.from_numpy(np.tile(np.array(roots), (4, 1, 1))).cuda()
    assert big.shape[0] == 32
    pool = model.many_clause_ordered_checkpoints(big.shape[0], split)
    torch.cuda.synchronize()
    out = model.solve_many_clauses_ordered(big, objective, max_nodes=8, order=order, split_width=split, checkpoints=pool)
    model.resume_many_clauses(out, max_nodes=24)
    model.resume_many_clauses(out, max_nodes=32)
    model.resume_many_clauses(out, max_nodes=budget - 64)
    got = host(out)
    want = one_call(name, order, split)
    tiled = {f: np.tile(want[f], (4,) + (1,) * (want[f].ndim - 1)) for f in EVERY + ("best",)}
    same(got, tiled, objective, "four calls queued on one stream")
    assert (got["slot"] == -1).all() and (got["status"] == DONE).all()


def test_the_sliced_driver():
    name, order, split = "schedule5_open_min", "none", 4
    text, roots, objective, budget = O.build(name)
    model = model_of(text)
    dev = torch.from_numpy(np.array(roots)).cuda()
    want = one_call(name, order, split)
    assert (want["status"] == DONE).all() and (want["best"] == 18).all()
    out = model.solve_many_clauses_sliced(dev, objective, budgets=R.slices(name), order=order, split_width=split, finish="resume")
    assert out["sliced"] == {"slices": 4, "searched": 0}
    same(host(out), want, objective, "sliced, finish=resume")
    # a caller's pool is reset and used again
    pool = model.many_clause_ordered_checkpoints(len(roots), split)
    for _ in range(2):
        out = model.solve_many_clauses_sliced(dev, objective, budgets=(64, budget - 64), order=order, split_width=split,
                                              checkpoints=pool)
        same(host(out), want, objective, "sliced on the caller's pool")
    left = one_call(name, order, split, 64)["status"] == LIMIT
    out = model.solve_many_clauses_sliced(dev, objective, budgets=(8, 56), order=order, split_width=split, finish="search")
    got = host(out)
    print(f"{name}: {out['sliced']}")
    assert out["sliced"] == {"slices": 2, "searched": int(left.sum())} and left.sum() > 4
    assert (got["status"] == DONE).all() and (got["slot"] == -1).all()
    assert (got["best"] == want["best"]).all() and (got["best"] == 18).all()
    ov = model.objective_var
    assert (got["first"][:, ov] == got["best"]).all()
    rows = got["first"]
    truth = model.eval_root(torch.from_numpy(np.ascontiguousarray(np.stack([rows, rows], 2))).cuda())
    assert (truth == 1).all(), "a reported optimum's row does not satisfy the model"
    assert ((rows >= roots[:, :, 0]) & (rows <= roots[:, :, 1])).all(), "a row outside its instance"
    same(got, want, objective, "instances the walk finished itself", rows=np.flatnonzero(~left))
    with pytest.raises(ValueError):
        model.solve_many_clauses_sliced(dev, objective, budgets=(8,), order=order, max_solutions=2)
    with pytest.raises(ValueError):
        model.resume_many_clauses(out, max_nodes=5, max_solutions=2)
    # an empty batch
    empty = model.solve_many_clauses_sliced(np.zeros((0, model.n_vars, 2), dtype=np.int32), objective, budgets=(8, 56),
                                            order=order, split_width=split)
    assert empty["status"].shape == (0,) and empty["halvings"].shape == (0,) and empty["slot"].shape == (0,)
    assert model.resume_many_clauses(empty, max_nodes=5)["status"].shape == (0,)
