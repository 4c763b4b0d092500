"""GPU tests of the clause checkpoints (cs_walk_resume: csgpu_solve_many_clauses_checkpointed, csgpu_solve_many_clauses_resume,
csgpu_many_clause_checkpoint_states) and of Model.solve_many_clauses_sliced.  Yardsticks: the host walk of
tests/many_walk_objective.py for the counters after every slice, and Model.solve_many_clauses with ONE budget -- which
test_gpu_solve_many_clauses.py pins to that walk -- for every field at the end, props and the stored rows included.  The
slices are those of tests/many_clause_resume_walk.py, which test_many_clauses_resume_host.py shows to stop instances
inside their trees.  Every call passes a finite max_nodes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import many_clause_resume_walk as R
import many_clause_sets as sets
import many_walk_objective as W
from csolve_amd import problems
from csolve_amd._lib import CsolveError, ManyOptions, load_library
from csolve_amd.solver import solve_root
from test_many_clauses_resume_host import resume_kernel_of, shipped_walk_resume_kernels

pytestmark = pytest.mark.gpu

E_ARG = -1
DONE, LIMIT, BAD_SLOT = 0, 1, 3
COUNTERS = ("status", "nodes", "cuts", "solutions")
EVERY = COUNTERS + ("props", "root_props", "first")
POISON = 0x5a5a5a5a


@functools.lru_cache(maxsize=None)
def model_of(text):
    return solve_root(text)


def host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


@functools.lru_cache(maxsize=None)
def one_call(name, budget=None):
    """the one solve_many_clauses call of a set, at its budget or another (computed once, not to be changed)"""
    text, roots, objective, own = sets.build(name)
    return host(model_of(text).solve_many_clauses(np.array(roots), objective, max_nodes=own if budget is None else budget))


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


@pytest.mark.parametrize("name", sorted(sets.SETS))
def test_a_walk_in_slices_is_the_one_call(name):
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    assert model.many_clauses_kernel() == sets.SETS[name][3]  # the old call launches what it launched
    assert model.many_clauses_resume_kernel() == resume_kernel_of(name)
    K = len(roots)
    dev = torch.from_numpy(np.array(roots)).cuda()
    pool = model.many_clause_checkpoints(K)
    steps, total, stopped = R.slices(name), 0, []
    for k, b in enumerate(steps):
        if k == 0:
            out = model.solve_many_clauses(dev, objective, max_nodes=b, checkpoints=pool)
        else:
            assert model.resume_many_clauses(out, max_nodes=b) is out
        total += b
        got = host(out)
        label = f"{name} after {steps[:k + 1]}"
        want = sets.walked(name) if total == budget else W.walk_many(text, roots, objective, total)
        same(got, want, objective, label + " against the host walk", fields=COUNTERS)
        slots_are_sound(got, K, label)
        stopped.append(int((got["status"] == LIMIT).sum()))
        if total in (8, 64):  # and on the way every field of the one call, the stored rows included
            same(got, one_call(name, total), objective, label + " against the one call")
    print(f"{name}: {K} instances, stopped after each of {steps}: {stopped}")
    assert total == budget and stopped[0] > 0 and stopped[1] > 0
    same(got, one_call(name), objective, f"{name} at the end against the one call")
    for f in W.FIELDS:
        assert (got[f] == sets.walked(name)[f]).all(), f
    assert ((got["first"] == 0).all(axis=1) | (got["solutions"] > 0)).all()
    pool.close()


def test_the_sets_launch_every_shipped_resume_instantiation():
    planned = {model_of(sets.build(name)[0]).many_clauses_resume_kernel() for name in sets.SETS}
    assert planned == shipped_walk_resume_kernels() and len(planned) == 8


def test_instances_without_a_slot_are_not_touched():
    name = "schedule6_min_budget"
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    pool = model.many_clause_checkpoints(len(roots))
    out = model.solve_many_clauses(np.array(roots), objective, max_nodes=64, checkpoints=pool)
    before = host(out)
    done = np.flatnonzero(before["slot"] < 0)
    left = np.flatnonzero(before["slot"] >= 0)
    assert done.size >= 4 and left.size >= 4, "the budget must split the set"
    idx = torch.from_numpy(done).cuda()
    out["_records"][idx] = 0x5a5a5a5a5a5a5a5a
    out["first"][idx] = POISON
    out["_best"][idx] = POISON
    model.resume_many_clauses(out, max_nodes=budget - 64)
    torch.cuda.synchronize()
    assert (out["_records"][idx] == 0x5a5a5a5a5a5a5a5a).all() and (out["first"][idx] == POISON).all()
    assert (out["_best"][idx] == POISON).all() and (out["slot"][idx] == -1).all()
    same(host(out), one_call(name), objective, "the resumed rows", rows=left)


def test_bad_slots_get_their_status_and_nothing_else():
    """a slot equal to the capacity, a slot of a fresh zeroed pool (no magic word) and a checkpoint made under another
    objective, in one resume call each with its neighbours"""
    name = "linear20_all"
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    K = len(roots)
    dev = torch.from_numpy(np.array(roots)).cuda()
    pool = model.many_clause_checkpoints(K + 2)  # two slots are never drawn: they stay zeroed
    out = model.solve_many_clauses(dev, "ALL", max_nodes=64, checkpoints=pool)
    before = host(out)
    stopped = np.flatnonzero(before["status"] == LIMIT)
    assert stopped.size > 6 and before["slot"].max() < K
    a, b = int(stopped[1]), int(stopped[3])
    out["slot"][a] = K + 2      # the first number past the pool
    out["slot"][b] = K + 1      # inside the pool, never written
    model.resume_many_clauses(out, max_nodes=budget - 64)
    got = host(out)
    assert got["status"][a] == BAD_SLOT and got["status"][b] == BAD_SLOT
    assert got["slot"][a] == K + 2 and got["slot"][b] == K + 1
    for f in EVERY[1:]:
        assert (got[f][[a, b]] == before[f][[a, b]]).all(), f
    others = np.setdiff1d(np.arange(K), [a, b])
    same(got, one_call(name), "ALL", "the neighbours", rows=others)
    # an ALL checkpoint under ANY: every instance with a slot is refused, the others are not looked at
    pool.reset()
    out = model.solve_many_clauses(dev, "ALL", max_nodes=64, checkpoints=pool)
    before = host(out)
    out["_objective"] = W.CODE["ANY"]
    model.resume_many_clauses(out, max_nodes=budget)
    got = host(out)
    had = before["slot"] >= 0
    assert had.sum() == stopped.size and (got["status"][had] == BAD_SLOT).all() and (got["status"][~had] == before["status"][~had]).all()
    for f in EVERY[1:] + ("slot",):
        assert (got[f] == before[f]).all(), f
    # and under the objective it was made under it goes on
    out["_objective"] = W.CODE["ALL"]
    out["status"][torch.from_numpy(np.flatnonzero(had)).cuda()] = LIMIT
    model.resume_many_clauses(out, max_nodes=budget - 64)
    same(host(out), one_call(name), "ALL", "after the refusal")


def test_a_full_pool_ends_an_instance_as_without_checkpoints():
    name = "schedule5_min"
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    K, capacity = len(roots), 5
    dev = torch.from_numpy(np.array(roots)).cuda()
    pool = model.many_clause_checkpoints(capacity)
    plain = one_call(name, 8)
    assert int((plain["status"] == LIMIT).sum()) > capacity

    def first_call():
        out = model.solve_many_clauses(dev, objective, max_nodes=8, checkpoints=pool)
        got = host(out)
        same(got, plain, objective, "budget 8, five slots")
        kept = np.flatnonzero(got["slot"] >= 0)
        assert kept.size == capacity and sorted(got["slot"][kept].tolist()) == list(range(capacity))
        assert (got["status"][kept] == LIMIT).all() and (got["slot"][np.setdiff1d(np.arange(K), kept)] == -1).all()
        return out, kept

    out, kept = first_call()
    model.resume_many_clauses(out, max_nodes=budget - 8)
    got = host(out)
    same(got, one_call(name), objective, "the five with a slot", rows=kept)
    same(got, plain, objective, "everything else", rows=np.setdiff1d(np.arange(K), kept))
    assert (got["slot"] == -1).all()
    pool.reset()
    first_call()


def test_three_calls_queued_on_one_stream_and_more_instances_than_waves():
    """schedule5_min repeated to four times the resident waves, slices 8 and the rest (and 56 between them), no host in
    between: a wave reuses its workspace slice between a stopped and a fresh instance, and every copy equals its original"""
    name = "schedule5_min"
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    K = len(roots)
    resident = model.many_clauses_waves(1 << 30)
    reps = -(-4 * resident // K)
    big = torch.from_numpy(np.tile(np.array(roots), (reps, 1, 1))).cuda()
    assert big.shape[0] >= 4 * resident
    pool = model.many_clause_checkpoints(big.shape[0])
    print(f"{big.shape[0]} instances on {resident} waves, pool of {big.shape[0] * model.clause_checkpoint_bytes() >> 20} MiB")
    torch.cuda.synchronize()
    out = model.solve_many_clauses(big, objective, max_nodes=8, checkpoints=pool)
    model.resume_many_clauses(out, max_nodes=56)
    model.resume_many_clauses(out, max_nodes=budget - 64)
    got = host(out)
    want = one_call(name)
    tiled = {f: np.tile(want[f], (reps,) + (1,) * (want[f].ndim - 1)) for f in EVERY + ("best",)}
    same(got, tiled, objective, "three calls queued on one stream")
    assert (got["slot"] == -1).all()
    # the synchronised sequence, in two slices
    pool.reset()
    out = model.solve_many_clauses(big, objective, max_nodes=8, checkpoints=pool)
    part = host(out)
    assert int((part["status"] == LIMIT).sum()) == reps * int((one_call(name, 8)["status"] == LIMIT).sum()) > 0
    slots_are_sound(part, big.shape[0], "after the first slice")
    model.resume_many_clauses(out, max_nodes=budget - 8)
    same(host(out), tiled, objective, "8 and the rest")


@pytest.mark.parametrize("name,budget", [("schedule6_min_budget", 256), ("linear20_all", 64)])
def test_checkpoint_states_are_the_open_subtrees_of_the_host_walk(name, budget):
    text, roots, objective, _ = sets.build(name)
    model = model_of(text)
    if name == "schedule6_min_budget":
        stopped = R.finished6()[1][0]
    else:
        stopped = R.sliced(name)[1][2]
    picked = sorted(stopped)[:6]
    assert len(picked) >= 4
    if objective == "MIN":
        assert any(stopped[i][1] is None for i in stopped) and any(stopped[i][1] is not None for i in stopped)
        picked = sorted(set(picked) | {i for i in stopped if stopped[i][1] is None})
    pool = model.many_clause_checkpoints(len(picked))
    out = model.solve_many_clauses(np.array(roots)[picked], objective, max_nodes=budget, checkpoints=pool)
    got = host(out)
    assert (got["status"] == LIMIT).all() and (got["slot"] >= 0).all()
    for k, i in enumerate(picked):
        want, best = stopped[i]
        states, incumbent = model.clause_checkpoint_states(pool, int(got["slot"][k]))
        assert tuple(states.shape) == want.shape and (states.cpu().numpy() == want).all(), f"instance {i}"
        assert incumbent == best, (i, incumbent, best)
        open_states, complete, again = model.open_clause_subtrees(pool, int(got["slot"][k]))
        assert again == best and open_states.shape[0] + complete.shape[0] <= want.shape[0]
        assert not (open_states[:, :, 0] == open_states[:, :, 1]).all(dim=1).any()
    with pytest.raises(CsolveError) as e:
        model.clause_checkpoint_states(pool, len(picked))
    assert e.value.code == E_ARG


def test_a_search_finishes_what_the_walk_left_min():
    name = "schedule6_min_budget"
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    first, done = R.finished6()[0]
    left = first["status"] == LIMIT
    out = model.solve_many_clauses_sliced(torch.from_numpy(np.array(roots)).cuda(), "MIN", budgets=(256,), finish="search")
    got = host(out)
    print(f"{name}: {out['sliced']}")
    assert out["sliced"] == {"slices": 1, "searched": int(left.sum())} and left.sum() > 4
    assert (got["status"] == DONE).all() and (got["slot"] == -1).all()
    assert (got["best"] == done["best"]).all(), (got["best"], done["best"])
    ov = model.objective_var
    assert (got["first"][:, ov] == got["best"]).all()
    rows = got["first"]
    truth = model.eval_root(torch.from_numpy(np.ascontiguousarray(np.stack([rows, rows], 2))).cuda())
    assert (truth == 1).all(), "a reported optimum's row does not satisfy the model"
    assert ((rows >= roots[:, :, 0]) & (rows <= roots[:, :, 1])).all(), "a row outside its instance"
    same(got, one_call(name), objective, "instances the walk finished itself", rows=np.flatnonzero(~left))
    assert (got["nodes"][left] >= 256).all()


def test_a_search_finishes_what_the_walk_left_all():
    name = "linear20_all"
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    left = one_call(name, 64)["status"] == LIMIT
    out = model.solve_many_clauses_sliced(torch.from_numpy(np.array(roots)).cuda(), "ALL", budgets=(64,), finish="search")
    got = host(out)
    assert out["sliced"] == {"slices": 1, "searched": int(left.sum())} and left.sum() > 4
    assert (got["status"] == DONE).all() and (got["slot"] == -1).all()
    assert (got["solutions"] == sets.walked(name)["solutions"]).all()
    # finish="resume" with the budgets of the set is the one call
    out = model.solve_many_clauses_sliced(torch.from_numpy(np.array(roots)).cuda(), "ALL", budgets=R.slices(name))
    assert out["sliced"] == {"slices": 4, "searched": 0}
    same(host(out), one_call(name), objective, "sliced, finish=resume")


def test_the_kinds_of_pool_are_not_mixed():
    import many_sets
    text = problems.queens(8, "ALL")  # a model of both families
    model = model_of(text)
    assert model.qualifies(7) and model.qualifies_many_clauses()
    rows = np.concatenate([model.domains()[None], many_sets.queens_two(8, 7, 3)]).astype(np.int32)
    dev = torch.from_numpy(rows).cuda()
    clause_pool, dive_pool = model.many_clause_checkpoints(8), model.many_checkpoints(8)
    assert clause_pool.clauses and not dive_pool.clauses
    with pytest.raises(CsolveError, match="other kind") as e:
        model.solve_many(dev, "ALL", max_nodes=4, checkpoints=clause_pool)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError, match="other kind") as e:
        model.solve_many_clauses(dev, "ALL", max_nodes=4, checkpoints=dive_pool)
    assert e.value.code == E_ARG
    with pytest.raises(CsolveError, match="other kind") as e:
        model.solve_many_upto(dev, 2, max_nodes=4, checkpoints=clause_pool)
    assert e.value.code == E_ARG
    for states, pool in ((model.checkpoint_states, clause_pool), (model.clause_checkpoint_states, dive_pool)):
        with pytest.raises(CsolveError, match="other kind") as e:
            states(pool, 0)
        assert e.value.code == E_ARG
    other_text, other_roots, _, _ = sets.build("linear20_all")
    with pytest.raises(CsolveError, match="another model") as e:
        model_of(other_text).solve_many_clauses(np.array(other_roots), "ALL", max_nodes=4, checkpoints=clause_pool)
    assert e.value.code == E_ARG
    # null pool or slots, on a finalized model: after the checks of csgpu_solve_many_clauses
    L = load_library()
    res = torch.zeros((len(rows), 5), dtype=torch.int64, device="cuda")
    slots = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    opt = ManyOptions(1, 0, 4)
    for ck, sl in ((None, slots.data_ptr()), (clause_pool._h, None)):
        assert L.csgpu_solve_many_clauses_checkpointed(model._h, dev.data_ptr(), len(rows), C.byref(opt), res.data_ptr(), None,
                                                       None, ck, sl, None) == E_ARG
        assert L.csgpu_solve_many_clauses_resume(model._h, len(rows), C.byref(opt), res.data_ptr(), None, None, ck, sl,
                                                 None) == E_ARG
    # both kinds work side by side on the one model, and an empty batch launches nothing
    a = host(model.solve_many_clauses(dev, "ALL", max_nodes=4, checkpoints=clause_pool))
    b = host(model.solve_many(dev, "ALL", max_nodes=4, checkpoints=dive_pool))
    for f in COUNTERS:
        assert (a[f] == b[f]).all(), f
    assert (a["slot"] >= 0).any() and ((a["slot"] >= 0) == (b["slot"] >= 0)).all()
    empty = model.solve_many_clauses(np.zeros((0, model.n_vars, 2), dtype=np.int32), "ALL", max_nodes=5, checkpoints=clause_pool)
    assert model.resume_many_clauses(empty, max_nodes=5)["status"].shape == (0,)
