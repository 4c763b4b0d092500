"""GPU tests of the start incumbents of the ordered clause walk (cs_walk_order_from behind
csgpu_solve_many_clauses_ordered_from / _from_resume, Model.solve_many_clauses_ordered(..., start=) and
Model.resume_many_clauses(..., own_solutions=True) on an ordered answer).  Yardsticks: Model.solve_many_clauses_ordered
itself where no instance has a start (field for field, first, best and halvings, plain and checkpointed),
many_ordered_spread_walk.FromOrdered on the host where some have, and the one call with the summed budget for a walk in
slices.  The error ladders of the new entries behind "the model is not finalized" are walked here
(test_solve_many_clauses_ordered_spread_precedence.py walks the rest without a device)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import many_ordered_spread_walk as S
import many_walk_objective as W
import test_solve_many_clauses_ordered_spread_precedence as P
from csolve_amd._lib import ManyOrderOptions, load_library
from csolve_amd.solver import solve_root

pytestmark = pytest.mark.gpu

DONE, LIMIT = 0, 1
RECORD = ("status", "root_props", "nodes", "cuts", "props", "solutions")
CANARY = 0x5a5a5a5a
ORDERS = {"none": 0, "smallest-domain": 1, "largest-domain": 2, "smallest-value": 3, "largest-value": 4}


@functools.lru_cache(maxsize=None)
def model_of(text):
    return solve_root(text)


def host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


def same(got, want, label, fields=RECORD + ("halvings", "first", "best")):
    for f in fields:
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(got[f]), -1).any(axis=1))
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {got[f][bad[0]]}, want {want[f][bad[0]]}"


@pytest.mark.parametrize("name,objective,order,split,budgets", S.MINMAX_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_without_a_start_it_is_the_ordered_call_plain_and_checkpointed(name, objective, order, split, budgets):
    text, roots = S.rows_of(name)
    model = model_of(text)
    K = len(roots)
    dev = torch.from_numpy(np.array(roots)).cuda()
    none = torch.zeros((K, 2), dtype=torch.int32, device="cuda")
    none[:, 0] = 7  # `best` is not read where have == 0
    for budget in (budgets[0], S.FINISH):
        want = host(model.solve_many_clauses_ordered(dev, objective, max_nodes=budget, order=order, split_width=split))
        got = host(model.solve_many_clauses_ordered(dev, objective, max_nodes=budget, order=order, split_width=split, start=none))
        assert set(got) == set(want)
        same(got, want, f"{name} plain at {budget}")
        pool_a, pool_b = model.many_clause_ordered_checkpoints(K, split), model.many_clause_ordered_checkpoints(K, split)
        want = host(model.solve_many_clauses_ordered(dev, objective, max_nodes=budget, order=order, split_width=split,
                                                     checkpoints=pool_a))
        got = host(model.solve_many_clauses_ordered(dev, objective, max_nodes=budget, order=order, split_width=split,
                                                    checkpoints=pool_b, start=none))
        same(got, want, f"{name} checkpointed at {budget}")
        assert ((got["slot"] >= 0) == (got["status"] == LIMIT)).all() and ((want["slot"] >= 0) == (want["status"] == LIMIT)).all()
        assert (budget == S.FINISH) == (got["status"] == DONE).all()
        pool_a.close()
        pool_b.close()
    assert model.many_clauses_order_from_kernel() == model.many_clauses_order_resume_kernel().replace("cs_walk_order_resume",
                                                                                                      "cs_walk_order_from")


def _starts(name, objective, order, split):
    """per instance: none, a worse value, the optimum itself ("nothing beats it"), a value beyond every solution"""
    one = S.one_walk(name, objective, order, split)
    sense = W.SENSE[objective]
    worse = 3 if sense == 1 else -3
    starts = []
    for i in range(len(one["status"])):
        best = int(one["best"][i]) if one["solutions"][i] > 0 else 40
        starts.append((None, best + worse, best, best - 100 * worse)[i % 4])
    return starts


@pytest.mark.parametrize("name,objective,order,split,budgets", S.MINMAX_CASES[1:], ids=lambda x: str(x).replace(" ", ""))
def test_with_a_start_it_is_the_host_walk_and_reports_own_solutions_only(name, objective, order, split, budgets):
    text, roots = S.rows_of(name)
    model = model_of(text)
    n, K = model.n_vars, len(roots)
    starts = _starts(name, objective, order, split)
    walks = [S.walk_from(text, row, objective, order, split, s, S.FINISH) for row, s in zip(roots, starts)]
    assert any(w["status"] == DONE and w["solutions"] == 0 and w["nodes"] > 0 for w in walks), "nothing beats it, after a walk"
    assert any(w["solutions"] > 0 and s is not None for w, s in zip(walks, starts)), "a warm start that is improved"
    start = torch.tensor([[0 if s is None else s, s is not None] for s in starts], dtype=torch.int32, device="cuda")
    dev = torch.from_numpy(np.array(roots)).cuda()
    # the C entry itself, on buffers full of canaries: what the instance does not own is not written
    L = load_library()
    opt = ManyOrderOptions(W.CODE[objective], ORDERS[order], split, 0, S.FINISH)
    records = torch.zeros((K, 5), dtype=torch.int64, device="cuda")
    first = torch.full((K, n), CANARY, dtype=torch.int32, device="cuda")
    best = torch.full((K,), CANARY, dtype=torch.int32, device="cuda")
    halvings = torch.full((K,), CANARY, dtype=torch.int64, device="cuda")
    rc = L.csgpu_solve_many_clauses_ordered_from(model._h, dev.data_ptr(), start.data_ptr(), K, C.byref(opt), records.data_ptr(),
                                                 first.data_ptr(), best.data_ptr(), halvings.data_ptr(), None, None, None)
    assert rc == 0, L.csgpu_last_error().decode()
    torch.cuda.synchronize()
    records, first, best, halvings = records.cpu().numpy(), first.cpu().numpy(), best.cpu().numpy(), halvings.cpu().numpy()
    for i, w in enumerate(walks):
        got = dict(status=records[i, 0] & 0xffffffff, nodes=records[i, 1], cuts=records[i, 2], solutions=records[i, 4],
                   halvings=halvings[i])
        for f in got:
            assert got[f] == w[f], (name, i, starts[i], f, got[f], w[f])
        if w["solutions"] > 0:
            assert best[i] == w["best"] and (first[i] == w["first"]).all(), (name, i)
            assert starts[i] is None or S.better(W.SENSE[objective], int(best[i]), starts[i])
        else:
            assert best[i] == CANARY and (first[i] == CANARY).all(), "best and the row of an instance without an own solution"
    # the Python call gives the same
    out = host(model.solve_many_clauses_ordered(dev, objective, max_nodes=S.FINISH, order=order, split_width=split, start=start))
    assert (out["nodes"] == records[:, 1]).all() and (out["halvings"] == halvings).all()
    has = out["solutions"] > 0
    assert (out["best"][has] == best[has]).all() and (out["best"][~has] == 0).all() and (out["first"][~has] == 0).all()


@pytest.mark.parametrize("name,objective,order,split,budgets", S.MINMAX_CASES[1:3], ids=lambda x: str(x).replace(" ", ""))
def test_a_walk_in_slices_with_own_solutions_is_the_one_call(name, objective, order, split, budgets):
    text, roots = S.rows_of(name)
    model = model_of(text)
    K = len(roots)
    starts = _starts(name, objective, order, split)
    start = torch.tensor([[0 if s is None else s, s is not None] for s in starts], dtype=torch.int32, device="cuda")
    dev = torch.from_numpy(np.array(roots)).cuda()
    steps = (budgets[0], budgets[1], 3, S.FINISH)
    pool = model.many_clause_ordered_checkpoints(K, split)
    out, total, stopped = None, 0, []
    for k, b in enumerate(steps):
        if k == 0:
            out = model.solve_many_clauses_ordered(dev, objective, max_nodes=b, order=order, split_width=split, checkpoints=pool,
                                                   start=start)
        else:
            assert model.resume_many_clauses(out, max_nodes=b, own_solutions=True) is out
        total += b
        got = host(out)
        want = host(model.solve_many_clauses_ordered(dev, objective, max_nodes=total, order=order, split_width=split, start=start))
        same(got, want, f"{name} after {steps[:k + 1]}")
        assert ((got["slot"] >= 0) == (got["status"] == LIMIT)).all()
        stopped.append(int((got["status"] == LIMIT).sum()))
    assert stopped[0] > 0 and stopped[1] > 0 and stopped[-1] == 0, stopped
    # a checkpoint of either ordered MIN / MAX call goes on under either resume
    a = model.solve_many_clauses_ordered(dev, objective, max_nodes=budgets[0], order=order, split_width=split,
                                         checkpoints=pool.reset())
    model.resume_many_clauses(a, max_nodes=S.FINISH, own_solutions=True)
    b = model.solve_many_clauses_ordered(dev, objective, max_nodes=budgets[0], order=order, split_width=split,
                                         checkpoints=model.many_clause_ordered_checkpoints(K, split), start=start)
    model.resume_many_clauses(b, max_nodes=S.FINISH)
    one = host(model.solve_many_clauses_ordered(dev, objective, max_nodes=S.FINISH, order=order, split_width=split))
    same(host(a), one, "a plain checkpoint under the own-solutions resume")
    with_start = host(model.solve_many_clauses_ordered(dev, objective, max_nodes=S.FINISH, order=order, split_width=split, start=start))
    same(host(b), with_start, "a start checkpoint under the plain resume", fields=RECORD + ("halvings",))
    with pytest.raises(ValueError):
        model.resume_many_clauses(out, max_nodes=5, max_solutions=2)
    pool.close()


def test_an_earlier_fault_wins_on_a_finalized_model_and_an_empty_batch_is_a_success():
    from csolve_amd import problems
    L = load_library()
    K = P.K
    model, other = solve_root(problems.schedule(5, 1)), solve_root(problems.schedule(5, 1))
    unplanned = solve_root(problems.schedule(32, 1))  # more than 512 clauses: no cs_walk_* kernel
    assert model.qualifies_many_clauses() and not unplanned.qualifies_many_clauses()
    pool, foreign = model.many_clause_ordered_checkpoints(K, 4), other.many_clause_ordered_checkpoints(K, 4)
    other_split, clause_pool = model.many_clause_ordered_checkpoints(K, 16), model.many_clause_checkpoints(K)
    queens = solve_root(problems.queens(8, "ALL"))  # a pure != model, of csgpu_solve_many's family
    dive_pool = queens.many_checkpoints(K)
    relabelled = P.Pool.from_buffer_copy(C.string_at(pool._h.value, C.sizeof(P.Pool)))  # the model's own pool as kind 0
    assert relabelled.m == model._h.value and relabelled.capacity == K and relabelled.kind == 2 and relabelled.split_width == 4
    relabelled.kind = 0
    n = model.n_vars
    full = dict(roots=torch.zeros((K, n, 2), dtype=torch.int32, device="cuda"),
                results=torch.full((K, 5), 77, dtype=torch.int64, device="cuda"),
                slots=torch.full((K,), 77, dtype=torch.int32, device="cuda"),
                start=torch.full((4, 2), 77, dtype=torch.int32, device="cuda"),
                halvings=torch.full((K,), 77, dtype=torch.int64, device="cuda"),
                children=torch.full((K,), 77, dtype=torch.int64, device="cuda"),
                unsplit=torch.full((K,), 77, dtype=torch.int32, device="cuda"),
                offsets=torch.zeros((K + 1,), dtype=torch.int64, device="cuda"),
                rows=torch.full((4, n, 2), 77, dtype=torch.int32, device="cuda"),
                owner=torch.full((4,), 77, dtype=torch.int32, device="cuda"),
                sub=torch.full((4,), 77, dtype=torch.int64, device="cuda"))
    world = {k: v.data_ptr() for k, v in full.items()}
    world.update(model=model._h, unplanned=unplanned._h, pool=pool._h, foreign=foreign._h, other_split=other_split._h,
                 clause_pool=clause_pool._h, dive_pool=dive_pool._h, relabelled=C.addressof(relabelled))
    assert P.walk(L, world, ("from", "from_resume"), finalized=True) > 2 * 2 * 8
    assert P.walk(L, world, ("children", "fanout", "fold"), finalized=False) > 3 * 2 * 4  # the same ladders on real pools
    torch.cuda.synchronize()
    for k, v in full.items():
        assert (v == (0 if k in ("roots", "offsets") else 77)).all(), k
