"""GPU tests of the spread of the ordered clause walk: cs_walk_order_children / cs_walk_order_fanout behind
csgpu_many_clause_ordered_checkpoint_children / _fanout, cs_walk_fold_halvings behind csgpu_many_fold_halvings, and
Model.solve_many_clauses_spread(..., order=, split_width=).  Yardsticks: tests/many_ordered_spread_walk.py for the children,
the halving each fanned slot owes, the rows, owners and start incumbents, and for the spread's answer; and
Model.solve_many_clauses_ordered itself for every field of the record under ALL, props and root_props included.  The sets
and budgets are the helper's (ALL_CASES, MINMAX_CASES); test_solve_many_clauses_ordered_spread_host.py shows that their
checkpoints hold every kind of frame.  Every call passes a finite max_nodes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import many_ordered_spread_walk as S
import many_walk_objective as W
from csolve_amd._lib import CsolveError
from csolve_amd.solver import solve_root
from test_solve_many_clauses_ordered_spread_precedence import Pool

pytestmark = pytest.mark.gpu

E_ARG = -1
DONE, LIMIT = 0, 1
RECORD = ("status", "root_props", "nodes", "cuts", "props", "solutions")
CANARY = 0x5a5a5a5a
MAGIC_ORDER = 0x776f6b70
ORDERS = {"none": 0, "smallest-domain": 1, "largest-domain": 2, "smallest-value": 3, "largest-value": 4}
CODES = {"ALL": 1, "MIN": 2, "MAX": 3}


@functools.lru_cache(maxsize=None)
def model_of(text):
    return solve_root(text)


def host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


@functools.lru_cache(maxsize=None)
def one_call(name, objective, order, split):
    """the one solve_many_clauses_ordered call of a set, to the end (computed once, not to be changed)"""
    text, roots = S.rows_of(name)
    return host(model_of(text).solve_many_clauses_ordered(np.array(roots), objective, max_nodes=S.FINISH, order=order,
                                                          split_width=split))


def stopped(name, objective, order, split, budget):
    """the checkpointed device call of a set at `budget` -> (model, pool, answer, index of the stopped instances, their slots)"""
    text, roots = S.rows_of(name)
    model = model_of(text)
    pool = model.many_clause_ordered_checkpoints(len(roots), split)
    out = model.solve_many_clauses_ordered(np.array(roots), objective, max_nodes=budget, order=order, split_width=split,
                                           checkpoints=pool)
    index = torch.nonzero((out["status"] == LIMIT) & (out["slot"] >= 0)).flatten()
    return model, pool, out, index, out["slot"][index].contiguous()


def offsets_of(children):
    offsets = torch.zeros((children.shape[0] + 1,), dtype=torch.int64, device=children.device)
    torch.cumsum(children.clamp(min=0), 0, out=offsets[1:])
    return offsets, int(offsets[-1].item())


@pytest.mark.parametrize("name,objective,order,split,budgets", S.ALL_CASES + S.MINMAX_CASES,
                         ids=lambda x: str(x).replace(" ", ""))
def test_children_unsplit_and_rows_are_the_host_helpers(name, objective, order, split, budgets):
    model, pool, out, index, slots = stopped(name, objective, order, split, budgets[0])
    walks = S.stopped_walks(name, objective, order, split, budgets[0])
    want_index = [i for i, (_, r) in enumerate(walks) if r["status"] == S.LIMIT]
    assert index.cpu().tolist() == want_index and want_index, "the device stops where the host walk stops"
    assert max(len(walks[i][0].stack) for i in want_index) <= 16, "pushed frames of the checkpoints"
    children, unsplit = model.clause_ordered_checkpoint_children(pool, slots, objective, order)
    assert children.dtype == torch.int64 and unsplit.dtype == torch.int32
    assert children.cpu().tolist() == [S.count_children(walks[i][0]) for i in want_index]
    assert unsplit.cpu().tolist() == [S.unsplit_of(walks[i][0]) for i in want_index]
    offsets, total = offsets_of(children)
    want_rows = np.concatenate([S.children_of(walks[i][0]) for i in want_index])
    want_owner = np.repeat(np.arange(len(want_index)), children.cpu().numpy())
    if objective == "ALL":
        rows, owner = model.clause_ordered_checkpoint_fanout(pool, slots, objective, order, offsets, total)
    else:
        rows, owner, start = model.clause_ordered_checkpoint_fanout(pool, slots, objective, order, offsets, total)
        inc = [walks[i][0].incumbent for i in want_index]
        want = np.array([[0 if b is None else b, b is not None] for b in inc], dtype=np.int32)[want_owner]
        assert (start.cpu().numpy() == want).all(), "a row starts from its checkpoint's incumbent"
        # the owner's best replaces the header's only where it is strictly better
        sense = W.SENSE[objective]
        mine = np.array([[(50 if b is None else b) + (-1, 1, 0)[k % 3], k % 4 != 3] for k, b in enumerate(inc)], dtype=np.int32)
        _, _, start2 = model.clause_ordered_checkpoint_fanout(pool, slots, objective, order, offsets, total,
                                                              owner_start=torch.from_numpy(mine).cuda())
        want2 = []
        for (ob, oh), b in zip(mine.tolist(), inc):
            if oh and S.better(sense, ob, b):
                want2.append([ob, 1])
            else:
                want2.append([0 if b is None else b, int(b is not None)])
        assert (start2.cpu().numpy() == np.array(want2, dtype=np.int32)[want_owner]).all()
    assert total == len(want_rows) and (rows.cpu().numpy() == want_rows).all(), "the rows, in walk order"
    assert (owner.cpu().numpy() == want_owner).all()
    # the other objective's code, another order: every slot is refused, -1 and nothing written
    for obj2, order2 in (("MIN" if objective == "ALL" else "ALL", order), (objective, "largest-domain")):
        c2, u2 = model.clause_ordered_checkpoint_children(pool, slots, obj2, order2)
        assert (c2 == -1).all() and (u2 == 0).all()
    # offsets that do not match: nothing is written
    canary = torch.full((total + 1, model.n_vars, 2), CANARY, dtype=torch.int32, device="cuda")
    who = torch.full((total + 1,), CANARY, dtype=torch.int32, device="cuda")
    st = torch.full((total + 1, 2), CANARY, dtype=torch.int32, device="cuda")
    extra = dict(start=st) if objective != "ALL" else {}
    # (every instance is judged by itself: one more child each, twice the children, rows past `total`)
    for wrong in (offsets + torch.arange(len(offsets), device="cuda"), offsets * 2, offsets + total):
        model.clause_ordered_checkpoint_fanout(pool, slots, objective, order, wrong.contiguous(), total, rows=canary, owner=who,
                                               **extra)
        torch.cuda.synchronize()
        assert (canary == CANARY).all() and (who == CANARY).all() and (st == CANARY).all()
    pool.close()


def _hip():
    """the HIP runtime the process has loaded already"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return lib
    raise AssertionError("no HIP runtime loaded")


def test_every_refusal_is_minus_one_with_nothing_written():
    """edits of a copy of a good slot, written into a free slot of the pool: the kernels compare before they read"""
    name, objective, order, split, budgets = S.ALL_CASES[0]
    text, roots = S.rows_of(name)
    model = model_of(text)
    n, K = model.n_vars, len(roots)
    pool = model.many_clause_ordered_checkpoints(K + 1, split)  # one slot stays free: number `spare`
    out = model.solve_many_clauses_ordered(np.array(roots), objective, max_nodes=budgets[0], order=order, split_width=split,
                                           checkpoints=pool)
    torch.cuda.synchronize()
    walks = S.stopped_walks(name, objective, order, split, budgets[0])
    F = pool.frames
    raw = Pool.from_buffer_copy(C.string_at(pool._h.value, C.sizeof(Pool)))
    assert raw.kind == 2 and raw.frames == F and raw.split_width == split and raw.capacity == K + 1
    assert raw.slot_bytes == (F + 1) * (n + 1) * 8 == model.clause_ordered_checkpoint_bytes(split)
    hip = _hip()
    used = out["slot"].cpu().numpy()
    spare = (set(range(K + 1)) - set(used[used >= 0].tolist())).pop()

    def read(slot):
        buf = np.zeros((F + 1, n + 1, 2), dtype=np.int32)
        assert hip.hipMemcpy(buf.ctypes.data, raw.d_pool + slot * raw.slot_bytes, raw.slot_bytes, 2) == 0
        return buf

    def write(buf):
        assert buf.shape == (F + 1, n + 1, 2) and buf.dtype == np.int32
        assert hip.hipMemcpy(raw.d_pool + spare * raw.slot_bytes, buf.ctypes.data, raw.slot_bytes, 1) == 0

    def count(slot=None):
        slots = torch.tensor([spare if slot is None else slot], dtype=torch.int32, device="cuda")
        children, unsplit = model.clause_ordered_checkpoint_children(pool, slots, objective, order)
        c = int(children.item())
        # the fan-out of the same slot, with room for what a good slot would write: a refused one writes nothing
        rows = torch.full((max(c, 2) + 1, n, 2), CANARY, dtype=torch.int32, device="cuda")
        who = torch.full((max(c, 2) + 1,), CANARY, dtype=torch.int32, device="cuda")
        for claimed in (1, 2, max(c, 1)):
            offsets = torch.tensor([0, claimed], dtype=torch.int64, device="cuda")
            model.clause_ordered_checkpoint_fanout(pool, slots, objective, order, offsets, claimed, rows=rows, owner=who)
            torch.cuda.synchronize()
            if c <= 0 or claimed != c:
                assert (rows == CANARY).all() and (who == CANARY).all()
        return c, int(unsplit.item())

    # a walk stopped above pushed halving parents, its current node halving with neither half tried
    pick = next(i for i, (w, r) in enumerate(walks) if r["status"] == S.LIMIT and S.unsplit_of(w) == 1
                and S.kinds_of(w)["pushed_halving"] > 0)
    walk = walks[pick][0]
    good = read(int(used[pick]))
    depth = int(good[0, 0, 0])
    frames = S.frames_of(walk)
    assert good[0, 0, 1] == MAGIC_ORDER and depth == len(frames) - 1 and good[0, 1, 1] >> 1 == CODES[objective] | ORDERS[order] << 3
    write(good)
    assert count() == (S.count_children(walk), 1) and count(int(used[pick])) == (S.count_children(walk), 1)
    pushed = next(d for d, (node, v, nv) in enumerate(frames[:-1]) if S.frame_kind(node, v, nv, split, False) == "second")

    def edited(change, base=None):
        buf = (good if base is None else base).copy()
        change(buf)
        write(buf)
        return count()

    def setv(*path_value):
        *path, value = path_value
        return lambda buf: buf.__setitem__(tuple(path), value)

    bv = int(good[1 + depth, n, 0])
    lo, hi = int(good[1 + depth, bv, 0]), int(good[1 + depth, bv, 1])
    pv = int(good[1 + pushed, n, 0])
    plo = int(good[1 + pushed, pv, 0])
    cases = {
        "another magic": setv(0, 0, 1, 0x77636b70),
        "no magic": setv(0, 0, 1, 0),
        "another objective in the code": setv(0, 1, 1, (2 | ORDERS[order] << 3) << 1),
        "another order in the code": setv(0, 1, 1, (CODES[objective] | 2 << 3) << 1),
        "depth F": setv(0, 0, 0, F),
        "depth -1": setv(0, 0, 0, -1),
        "bv == n": setv(1 + depth, n, 0, n),
        "bv == -1 in a pushed frame": setv(1 + pushed, n, 0, -1),
        "empty bounds": setv(1 + depth, bv, 0, hi + 1),
        "bounds below the root domain": setv(1 + depth, bv, 0, -(1 << 31)),
        "a pushed halving frame with next == lo": setv(1 + pushed, n, 1, plo),
        "a halving frame with a next that is neither": setv(1 + depth, n, 1, lo + 1),
        "a pushed halving frame with a next that is neither": setv(1 + pushed, n, 1, plo + 1),
    }
    for label, change in cases.items():
        assert edited(change) == (-1, 0), label
    # an enumerating frame with several values left, of another stopped walk: `next` outside its bounds
    pick2 = next(i for i, (w, r) in enumerate(walks) if r["status"] == S.LIMIT and S.kinds_of(w)["several"] > 0)
    walk2 = walks[pick2][0]
    good2 = read(int(used[pick2]))
    frames2 = S.frames_of(walk2)
    enum = next(d for d, (node, v, nv) in enumerate(frames2)
                if S.frame_kind(node, v, nv, split, d == len(frames2) - 1) == "enumerating" and int(node[v, 1]) - nv + 1 > 1)
    assert edited(lambda buf: None, good2) == (S.count_children(walk2), S.unsplit_of(walk2))
    ev = int(good2[1 + enum, n, 0])
    elo, ehi = int(good2[1 + enum, ev, 0]), int(good2[1 + enum, ev, 1])
    assert ev == frames2[enum][1] and (elo, ehi) == tuple(frames2[enum][0][ev]) and ehi - elo + 1 <= split
    assert edited(setv(1 + enum, n, 1, ehi + 1), good2) == (-1, 0), "next above the bounds"
    assert edited(setv(1 + enum, n, 1, elo - 1), good2) == (-1, 0), "next below the bounds"
    assert edited(setv(1 + enum, n, 1, ehi), good2)[0] == S.count_children(walk2) - (ehi - frames2[enum][2]), "the last value alone"
    # the current node between its halves is good again, and owes nothing: one child fewer
    mid = (lo + hi) >> 1
    assert edited(setv(1 + depth, n, 1, mid + 1)) == (S.count_children(walk) - 1, 0)
    # a slot number outside the pool
    assert count(K + 1) == (-1, 0) and count(1 << 30) == (-1, 0)
    assert count(-1)[0] == 0
    pool.close()


def test_pools_of_the_other_kinds_are_refused_and_the_existing_calls_refuse_an_ordered_pool():
    name, objective, order, split, budgets = S.MINMAX_CASES[2]
    model, pool, out, index, slots = stopped(name, objective, order, split, budgets[0])
    from csolve_amd import problems
    queens = model_of(problems.queens(8, "ALL"))  # a pure != model: of csgpu_solve_many's family
    clause_pool, dive_pool = model.many_clause_checkpoints(4), queens.many_checkpoints(4)
    offsets = torch.zeros((slots.shape[0] + 1,), dtype=torch.int64, device="cuda")
    for bad in (clause_pool, dive_pool):  # the other two kinds
        with pytest.raises(CsolveError) as e:
            model.clause_ordered_checkpoint_children(bad, slots, objective, order)
        assert e.value.code == E_ARG and "other kind" in str(e.value)
        with pytest.raises(CsolveError) as e:
            model.clause_ordered_checkpoint_fanout(bad, slots, objective, order, offsets, 0)
        assert e.value.code == E_ARG and "other kind" in str(e.value)
    with pytest.raises(CsolveError) as e:
        model.clause_ordered_checkpoint_children(pool, slots, "ANY", order)
    assert e.value.code == E_ARG
    # the existing calls, unchanged: an ordered pool is of the other kind for each of them
    for call in (lambda: model.clause_checkpoint_children(pool, slots), lambda: model.clause_checkpoint_children(pool, slots, objective=objective),
                 lambda: model.clause_checkpoint_fanout(pool, slots, offsets, 0),
                 lambda: model.clause_checkpoint_fanout(pool, slots, offsets, 0, objective=objective),
                 lambda: model.solve_many_clauses(S.rows_of(name)[1].copy(), objective, max_nodes=8, checkpoints=pool,
                                                  start=torch.zeros((len(S.rows_of(name)[1]), 2), dtype=torch.int32, device="cuda"))):
        with pytest.raises(CsolveError) as e:
            call()
        assert e.value.code == E_ARG and "other kind" in str(e.value)
    clause_pool.close()
    dive_pool.close()
    pool.close()


def test_fold_many_halvings_adds_every_owned_row_once():
    model = model_of(S.rows_of("wcet_max")[0])
    sub = dict(status=torch.zeros(7, dtype=torch.int64, device="cuda"),
               halvings=torch.tensor([1, 0, 5, 1 << 40, 3, 2, 9], dtype=torch.int64, device="cuda"))
    owner = torch.tensor([2, 0, 2, 1, -1, 0, 2], dtype=torch.int32, device="cuda")
    result = dict(halvings=torch.tensor([10, 20, 30, 40], dtype=torch.int64, device="cuda"))
    assert model.fold_many_halvings(sub, owner, result) is result
    torch.cuda.synchronize()
    assert result["halvings"].cpu().tolist() == [12, 20 + (1 << 40), 45, 40]


def same_record(got, want, label, fields=RECORD + ("halvings", "first"), rows=None):
    for f in fields:
        g, w = (got[f], want[f]) if rows is None else (got[f][rows], want[f][rows])
        if len(g) == 0:
            continue
        bad = np.flatnonzero((np.asarray(g) != np.asarray(w)).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}"


@pytest.mark.parametrize("name,objective,order,split,budgets", S.ALL_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_the_all_spread_is_the_one_call_field_for_field(name, objective, order, split, budgets):
    text, roots = S.rows_of(name)
    model = model_of(text)
    want = one_call(name, objective, order, split)
    walked = S.one_walk(name, objective, order, split)
    same_record(want, walked, "the one call against the host walk", fields=("status", "nodes", "cuts", "solutions", "halvings", "first"))
    dev = torch.from_numpy(np.array(roots)).cuda()
    assert (want["status"] == DONE).all()
    for pair in (budgets, (1, 1)):
        out = model.solve_many_clauses_spread(dev, "ALL", budgets=pair, order=order, split_width=split)
        got = host(out)
        label = f"{name} {order}/{split} budgets {pair}"
        assert set(got) == set(want), label
        same_record(got, want, label)
        assert out["rounds"] > 2 and out["sub_instances"] == sum(out["round_rows"]) > 0, label


@pytest.mark.parametrize("name,objective,order,split,budgets", S.ALL_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_the_all_spread_through_the_fallback_and_cut_short(name, objective, order, split, budgets):
    text, roots = S.rows_of(name)
    model = model_of(text)
    want = one_call(name, objective, order, split)
    dev = torch.from_numpy(np.array(roots)).cuda()
    # the fallback: with max_rows=0 no round is fanned out (63 resumes in place of 1,024 nodes finish every row); with
    # max_rows=200 the first round is and a wider one goes on in place, with a budget that finishes it
    first_round = S.spread_of(name, objective, order, split, budgets, 2)[1]["per_round"][0]  # the host driver's, cut short
    for pair, kw in (((8, 1024), dict(max_rows=0)), ((8, 64, S.FINISH), dict(max_rows=max(first_round, 200)))):
        out = model.solve_many_clauses_spread(dev, "ALL", budgets=pair, order=order, split_width=split, **kw)
        got = host(out)
        label = f"{name} {order}/{split} budgets {pair} {kw}"
        assert set(got) == set(want), label
        same_record(got, want, label)
        if kw["max_rows"] == 0:
            assert out["sub_instances"] == 0 and set(out["round_rows"]) == {0}, label
        else:
            assert out["round_rows"][0] == first_round, label
    # cut short: owners with work left are LIMIT with what was folded, the others the one call's
    out = model.solve_many_clauses_spread(dev, "ALL", budgets=budgets, order=order, split_width=split, max_rounds=2)
    got = host(out)
    owners, info = S.spread_of(name, objective, order, split, budgets, 2)
    assert out["rounds"] == 2 and out["round_rows"] == info["per_round"]
    left = got["status"] == LIMIT
    assert left.any() and (len(left) == 1 or not left.all())
    for f in ("status", "nodes", "cuts", "solutions", "halvings"):
        assert got[f].tolist() == [o[f] for o in owners], f
    same_record(got, want, "owners that finished in two rounds", rows=np.flatnonzero(~left))
    if name == "wide3_plain":  # without `order` the plain spread, as before: no halving counts in its answer
        plain = model.solve_many_clauses_spread(dev, "ALL", budgets=(64, 1024), max_rounds=3)
        assert "halvings" not in plain


@pytest.mark.parametrize("name,objective,order,split,budgets", S.MINMAX_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_the_minmax_spread_proves_the_one_calls_optimum(name, objective, order, split, budgets):
    text, roots = S.rows_of(name)
    model = model_of(text)
    want = one_call(name, objective, order, split)
    dev = torch.from_numpy(np.array(roots)).cuda()
    assert (want["status"] == DONE).all()
    out = model.solve_many_clauses_spread(dev, objective, budgets=budgets, order=order, split_width=split)
    got = host(out)
    assert set(got) == set(want) and out["rounds"] > 2 and out["sub_instances"] > 0
    assert (got["status"] == want["status"]).all()
    has = want["solutions"] > 0
    assert ((got["solutions"] > 0) == has).all() and (got["best"][has] == want["best"][has]).all()
    rows = got["first"][has]
    ov = model.objective_var
    assert (rows[:, ov] == got["best"][has]).all(), "first is a solution of value best"
    truth = model.eval_root(torch.from_numpy(np.ascontiguousarray(np.stack([rows, rows], 2))).cuda())
    assert (truth == 1).all(), "a reported optimum's row does not satisfy the model"
    assert ((rows >= roots[has][:, :, 0]) & (rows <= roots[has][:, :, 1])).all(), "a row outside its instance"
    orc = W.oracle_for(text)[0]
    for row in rows[:4]:  # and with the oracle
        assert orc.instance(np.stack([row, row], 1).astype(np.int32), -1, 0, 0)[0] >= 0
    assert (got["first"][~has] == 0).all()
    again = host(model.solve_many_clauses_spread(dev, objective, budgets=budgets, order=order, split_width=split))
    for f in got:
        assert (got[f] == again[f]).all(), f"two runs differ in {f}"
    # the fallback: nothing is fanned out, the stopped walks go on in place to the same optimum
    inplace = model.solve_many_clauses_spread(dev, objective, budgets=budgets, order=order, split_width=split, max_rows=0)
    there = host(inplace)
    assert inplace["sub_instances"] == 0 and (there["status"] == DONE).all() and (there["best"][has] == want["best"][has]).all()
    same_record(there, want, "in place, the walk is the one call's")
