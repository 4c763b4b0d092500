"""GPU tests of Model.solve_many_clauses_wide (csgpu_solve_many_clauses_wide; cs_walk_wide, cs_walk_wide_resume: the clause
records in LDS).  On every set of tests/many_clause_sets.py (at most 512 clauses) the wide call equals solve_many_clauses
field for field, props included, and a checkpointed wide call resumed in slices equals the one wide call; past 512 clauses
(tests/many_clause_wide_sets.py) it equals the host walk; and the contracts of the entry."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import many_clause_sets as sets
import many_clause_wide_sets as wide
import many_walk_objective as W
from csolve_amd import problems
from csolve_amd._lib import CsolveError, ManyOptions, load_library
from csolve_amd.solver import solve_root

pytestmark = pytest.mark.gpu

E_ARG, E_LIMIT = -1, -4
BAD_SLOT = 3
SENTINEL = -77
RECORD = ("status", "root_props", "nodes", "cuts", "props", "solutions")
WALKED = ("status", "nodes", "cuts", "solutions")


@functools.lru_cache(maxsize=None)
def model_of(text):
    return solve_root(text)


def host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


def same_records(got, want, objective, where=None, fields=RECORD):
    """every field of every record, the stored row, and `best` where an instance has a solution"""
    for f in fields:
        assert (got[f] == want[f]).all(), (f, where, np.nonzero(got[f] != want[f])[0][:8], got[f][:8], want[f][:8])
    has = want["solutions"] > 0
    assert (got["first"][has] == want["first"][has]).all(), where
    assert (got["first"][~has] == 0).all(), where
    if objective in ("MIN", "MAX"):
        assert (got["best"][has] == want["best"][has]).all(), where
    else:
        assert "best" not in got


def sliced(model, rows, objective, slices):
    """a checkpointed wide call and its resumes, `slices` nodes each -> (the answer on the host, instances ever resumed)"""
    pool = model.many_clause_wide_checkpoints(len(rows))
    out = model.solve_many_clauses_wide(np.array(rows), objective, max_nodes=slices[0], checkpoints=pool)
    resumed = 0
    for budget in slices[1:]:
        resumed += int((host(out)["slot"] >= 0).sum())
        model.resume_many_clauses_wide(out, max_nodes=budget)
    got = host(out)
    pool.close()
    return got, resumed


@pytest.mark.parametrize("name", sorted(sets.SETS))
def test_the_wide_walk_is_the_plain_walk_on_every_set(name):
    """lane assignment and slot order are kernel 6's, so props and root_props are pinned as well"""
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    tree = sets.SETS[name][3].split(", ")[1].rstrip(">")
    assert model.qualifies_many_clauses() and model.qualifies_many_clauses_wide()
    assert model.many_clauses_wide_kernel() == f"cs_walk_wide<{tree}>"
    assert model.many_clauses_wide_resume_kernel() == f"cs_walk_wide_resume<{tree}>"
    assert model.many_clauses_kernel() == sets.SETS[name][3]  # and the plain plan is what it was
    assert "walk" not in " ".join(str(v) for v in model.plan().values())
    assert model.clause_wide_checkpoint_bytes() == model.clause_checkpoint_bytes() == (model.n_vars + 1) ** 2 * 8
    plain = host(model.solve_many_clauses(np.array(roots), objective, max_nodes=budget))
    got = host(model.solve_many_clauses_wide(np.array(roots), objective, max_nodes=budget))
    assert set(got) == set(plain)
    same_records(got, plain, objective, name)
    same_records(got, sets.walked(name), objective, name, fields=WALKED)


@pytest.mark.parametrize("name,slices", [("mixed40_any", (2, 5, 1 << 14)), ("linear20_all", (3, 40, 1 << 14)),
                                         ("schedule6_min_budget", (5, 51, 200))])
def test_wide_slices_are_the_one_wide_call(name, slices):
    text, roots, objective, _ = sets.build(name)
    model = model_of(text)
    whole = host(model.solve_many_clauses_wide(np.array(roots), objective, max_nodes=sum(slices)))
    got, resumed = sliced(model, roots, objective, slices)
    assert resumed > 0
    same_records(got, whole, objective, name)
    done = whole["status"] == W.DONE
    assert (got["slot"][done] == -1).all() and (got["slot"][~done] >= 0).all()
    if name == "schedule6_min_budget":  # some stop again at the end, with an incumbent
        assert (~done).any() and (whole["solutions"][~done] > 0).any()


@pytest.mark.parametrize("name", sorted(wide.CASES))
def test_past_512_clauses_the_wide_walk_is_the_host_walk(name):
    """status, nodes, cuts, solutions, best and the stored row against tests/many_walk_objective.py.  props have no
    independent reference up here -- kernel 6 cannot run these models, and the oracle narrows in another order -- so they
    are only held to themselves: two calls agree, and slices sum to the one call."""
    text, rows, objective, budget = wide.build(name)
    model = model_of(text)
    assert (model.domains() == W.oracle_for(text)[1]).all()  # the rows lie in the device tables' root domains
    assert model.n_clauses > 512 and not model.qualifies(6) and not model.qualifies_many_clauses()
    assert model.qualifies_many_clauses_wide() and model.many_clauses_kernel() is None
    tree = "true" if name.startswith("tree") else "false"
    assert model.many_clauses_wide_kernel() == f"cs_walk_wide<{tree}>"
    want = wide.walked(name)
    got = host(model.solve_many_clauses_wide(np.array(rows), objective, max_nodes=budget))
    same_records(got, want, objective, name, fields=WALKED)
    limit = got["status"] == W.LIMIT
    assert (got["nodes"][limit] == budget).all() and (got["nodes"][~limit] < budget).all()
    again = host(model.solve_many_clauses_wide(np.array(rows), objective, max_nodes=budget))
    same_records(again, got, objective, name)
    parts, resumed = sliced(model, rows, objective, (7, 50, budget - 57))
    assert resumed > 0
    same_records(parts, got, objective, name)
    if name == "schedule32_min":
        done = got["status"] == W.DONE
        assert (done & (got["solutions"] > 0)).any() and (limit & (got["solutions"] > 0)).any()
        assert got["status"][0] == W.LIMIT and got["solutions"][0] == 1 and got["best"][0] == 114
    if name == "sudoku_less_any":
        assert ((got["status"] == W.DONE) & (got["solutions"] == 1)).any() and limit.any()
        assert ((got["status"] == W.DONE) & (got["solutions"] == 0) & (got["nodes"] == 0)).any()
    if name == "sudoku_less_all":
        assert limit.any()


def test_the_plain_entry_still_refuses_more_than_512_clauses():
    for name in ("schedule32_min", "sudoku_less_any"):
        text, rows, objective, _ = wide.build(name)
        model = model_of(text)
        for r in (np.array(rows), torch.from_numpy(np.array(rows)).cuda()):
            with pytest.raises(CsolveError) as e:
                model.solve_many_clauses(r, objective, max_nodes=10)
            assert e.value.code == E_LIMIT and "512" in str(e.value)
        with pytest.raises(CsolveError) as e:
            model.many_clause_checkpoints(4)
        assert e.value.code == E_LIMIT
        assert model.clause_checkpoint_bytes() == 0 and model.clause_wide_checkpoint_bytes() == (model.n_vars + 1) ** 2 * 8


def _call(model, roots, objective, budget, rows, best, stream=None):
    """the library itself, on buffers of the test's own"""
    K = roots.shape[0]
    res = torch.full((max(K, 1), 5), SENTINEL, dtype=torch.int64, device="cuda")
    opt = ManyOptions(W.CODE[objective], 0, budget)
    # (an empty tensor has no address: any non-null pointer stands for the rows of an empty batch)
    rc = load_library().csgpu_solve_many_clauses_wide(model._h, roots.data_ptr() if K else res.data_ptr(), K, C.byref(opt),
                                                      res.data_ptr(),
                                                      rows.data_ptr() if rows is not None else None,
                                                      best.data_ptr() if best is not None else None, stream)
    assert rc == 0, load_library().csgpu_last_error()
    return res


def test_an_empty_batch_and_rows_outside_the_root_domains():
    text, rows, objective, budget = wide.build("schedule32_min")
    model = model_of(text)
    n = model.n_vars
    # count == 0: OK, nothing is launched, nothing is written
    empty = host(model.solve_many_clauses_wide(np.zeros((0, n, 2), dtype=np.int32), objective, max_nodes=5))
    assert empty["status"].shape == (0,) and empty["best"].shape == (0,)
    res = _call(model, torch.zeros((0, n, 2), dtype=torch.int32, device="cuda"), objective, 5, None, None)
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == SENTINEL).all()
    # BAD_ROOT: the status, zero counters, and nothing else -- the row and best keep what they held
    dom = model.domains()
    bad = np.array(rows[:4])
    bad[0, 3, 1] = dom[3, 1] + 1           # above the root domain
    bad[2, 5] = (dom[5, 0] + 1, dom[5, 0])  # lo > hi
    dev = torch.from_numpy(bad).cuda()
    first = torch.full((4, n), SENTINEL, dtype=torch.int32, device="cuda")
    best = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
    res = _call(model, dev, objective, budget, first, best)
    torch.cuda.synchronize()
    res, first, best = res.cpu().numpy(), first.cpu().numpy(), best.cpu().numpy()
    want = wide.walked("schedule32_min")
    head = np.ascontiguousarray(res[:, 0]).view(np.int32).reshape(4, 2)  # {status, root_props} lead the record
    assert head[:, 0].tolist() == [W.BAD_ROOT, want["status"][1], W.BAD_ROOT, want["status"][3]]
    for k in (0, 2):
        assert head[k, 1] == 0 and (res[k, 1:] == 0).all()
        assert (first[k] == SENTINEL).all() and best[k] == SENTINEL
    for k in (1, 3):
        assert res[k, 1] == want["nodes"][k] and res[k, 4] == want["solutions"][k] > 0
        assert (first[k] == want["first"][k]).all() and best[k] == want["best"][k]
    # the rows of sudoku_less_roots without the root domains: 1 .. 9 lies outside what the inequalities leave
    text, _ = wide.sudoku_less()
    loose = problems.sudoku_less_roots(*wide.SUDOKU, wide.SHARES)[1]
    got = host(model_of(text).solve_many_clauses_wide(loose, "ANY", max_nodes=10))
    assert (got["status"] == W.BAD_ROOT).all() and (got["nodes"] == 0).all() and (got["first"] == 0).all()


def test_pool_kinds_refuse_each_other():
    """on a model every family takes (8 queens: kernel 7, kernel 6 and the wide walk)"""
    text = problems.queens(8, "ALL")
    model = model_of(text)
    L = load_library()
    assert model.qualifies(7) and model.qualifies_many_clauses() and model.qualifies_many_clauses_wide()
    rows = np.repeat(model.domains()[None], 3, 0).astype(np.int32)
    dev = torch.from_numpy(rows).cuda()
    wpool = model.many_clause_wide_checkpoints(4)
    assert wpool.wide and wpool.clauses and not wpool.ordered
    older = {"dive": model.many_checkpoints(4), "clause": model.many_clause_checkpoints(4),
             "ordered": model.many_clause_ordered_checkpoints(4, 256)}
    res = torch.zeros((3, 5), dtype=torch.int64, device="cuda")
    slots = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    opt = ManyOptions(1, 0, 5)

    def refused(rc, what):
        assert rc == E_ARG and b"other kind" in L.csgpu_last_error(), (what, rc, L.csgpu_last_error())

    # a pool of an older kind into the wide entries
    for kind, pool in older.items():
        with pytest.raises(CsolveError) as e:
            model.solve_many_clauses_wide(dev, "ALL", max_nodes=5, checkpoints=pool)
        assert e.value.code == E_ARG and "other kind" in str(e.value), kind
        refused(L.csgpu_solve_many_clauses_wide_resume(model._h, 3, C.byref(opt), res.data_ptr(), None, None, pool._h,
                                                       slots.data_ptr(), None), kind)
    # the wide pool into every older entry that takes one: the checkpointed calls and the resumes, children, fan-out, states
    with pytest.raises(CsolveError) as e:
        model.solve_many_clauses(dev, "ALL", max_nodes=5, checkpoints=wpool)
    assert e.value.code == E_ARG and "other kind" in str(e.value)
    with pytest.raises(CsolveError) as e:
        model.solve_many(dev, "ALL", max_nodes=5, checkpoints=wpool)
    assert e.value.code == E_ARG and "other kind" in str(e.value)
    refused(L.csgpu_solve_many_clauses_resume(model._h, 3, C.byref(opt), res.data_ptr(), None, None, wpool._h, slots.data_ptr(),
                                              None), "clause resume")
    refused(L.csgpu_solve_many_resume(model._h, 3, C.byref(opt), res.data_ptr(), None, wpool._h, slots.data_ptr(), None),
            "resume")
    children = torch.zeros((3,), dtype=torch.int64, device="cuda")
    offsets = torch.zeros((4,), dtype=torch.int64, device="cuda")
    out_rows = torch.zeros((4, model.n_vars, 2), dtype=torch.int32, device="cuda")
    owner = torch.zeros((4,), dtype=torch.int32, device="cuda")
    refused(L.csgpu_many_clause_checkpoint_children(wpool._h, slots.data_ptr(), 3, children.data_ptr(), None), "clause children")
    refused(L.csgpu_many_checkpoint_children(wpool._h, slots.data_ptr(), 3, children.data_ptr(), None), "children")
    refused(L.csgpu_many_clause_checkpoint_fanout(wpool._h, slots.data_ptr(), 3, offsets.data_ptr(), out_rows.data_ptr(),
                                                  owner.data_ptr(), 4, None), "clause fan-out")
    refused(L.csgpu_many_checkpoint_fanout(wpool._h, slots.data_ptr(), 3, offsets.data_ptr(), out_rows.data_ptr(),
                                           owner.data_ptr(), 4, None), "fan-out")
    refused(L.csgpu_many_clause_ordered_checkpoint_children(wpool._h, slots.data_ptr(), 3, 1, 1, children.data_ptr(),
                                                            owner.data_ptr(), None), "ordered children")
    count, best, have = C.c_int64(), C.c_int32(), C.c_int32()
    refused(L.csgpu_many_clause_checkpoint_states(wpool._h, 0, out_rows.data_ptr(), 4, C.byref(count), C.byref(best),
                                                  C.byref(have), None), "clause states")
    refused(L.csgpu_many_checkpoint_states(wpool._h, 0, out_rows.data_ptr(), 4, C.byref(count), None), "states")
    # and each pool still serves its own family, the wide one included
    a = host(model.solve_many_clauses_wide(dev, "ALL", max_nodes=5, checkpoints=wpool))
    b = host(model.solve_many_clauses(dev, "ALL", max_nodes=5, checkpoints=older["clause"]))
    for f in RECORD + ("first",):
        assert (a[f] == b[f]).all(), f
    # (which wave draws which slot is the order of their atomic adds: the three numbers, in any order)
    assert (a["status"] == W.LIMIT).all() and sorted(a["slot"].tolist()) == sorted(b["slot"].tolist()) == [0, 1, 2]
    for pool in (wpool, *older.values()):
        pool.close()


def test_a_resume_under_another_objective_is_a_bad_slot():
    text, roots, objective, _ = sets.build("linear20_all")
    model = model_of(text)
    pool = model.many_clause_wide_checkpoints(len(roots))
    out = model.solve_many_clauses_wide(np.array(roots), "ALL", max_nodes=3, checkpoints=pool)
    before = host(out)
    stopped = before["slot"] >= 0
    assert stopped.any() and (before["status"][stopped] == W.LIMIT).all()
    out["_objective"] = W.CODE["ANY"]
    model.resume_many_clauses_wide(out, max_nodes=50)
    after = host(out)
    assert (after["status"][stopped] == BAD_SLOT).all() and (after["status"][~stopped] == before["status"][~stopped]).all()
    for f in RECORD[1:] + ("slot", "first"):  # the status word alone
        assert (after[f] == before[f]).all(), f
    out["_objective"] = W.CODE["ALL"]  # the checkpoints are intact: under their own objective the walk goes on
    model.resume_many_clauses_wide(out, max_nodes=1 << 14)
    whole = host(model.solve_many_clauses_wide(np.array(roots), "ALL", max_nodes=3 + (1 << 14)))
    same_records(host(out), whole, "ALL")
    pool.close()


def test_records_that_do_not_fit_lds_are_a_limit_that_names_the_bytes():
    text = problems.queens(96, "ALL")
    model = model_of(text)
    assert model.n_clauses > 10000 and not model.qualifies_many_clauses_wide()
    assert model.many_clauses_wide_kernel() is None and model.many_clauses_wide_waves(8) == 0
    assert model.clause_wide_checkpoint_bytes() == 0
    rows = np.repeat(model.domains()[None], 2, 0)
    for r in (rows, torch.from_numpy(rows).cuda()):
        with pytest.raises(CsolveError) as e:
            model.solve_many_clauses_wide(r, "ALL", max_nodes=10)
        assert e.value.code == E_LIMIT and "160 KiB" in str(e.value)
        need = [int(x) for x in re.findall(r"(\d+) bytes of LDS", str(e.value))]
        assert need and need[0] > 160 * 1024 and need[0] >= 16 * 10000
    with pytest.raises(CsolveError) as e:
        model.many_clause_wide_checkpoints(4)
    assert e.value.code == E_LIMIT


def test_a_batch_larger_than_the_resident_waves_and_two_queued_calls():
    text, rows, objective, budget = wide.build("sudoku_less_any")
    model = model_of(text)
    want = wide.walked("sudoku_less_any")
    K, reps = len(rows), 4096
    resident = model.many_clauses_wide_waves(1 << 30)
    assert resident >= 64 and model.many_clauses_wide_waves(3) == 4 and model.many_clauses_wide_waves(0) == 0
    assert reps * K > 2 * resident  # most instances are drawn by a wave that has walked another one: the ticket path
    one = host(model.solve_many_clauses_wide(np.array(rows), objective, max_nodes=budget))
    big = torch.from_numpy(np.tile(np.array(rows), (reps, 1, 1))).cuda()
    got = host(model.solve_many_clauses_wide(big, objective, max_nodes=budget))
    for f in RECORD:
        assert (got[f].reshape(reps, K) == one[f][None]).all(), f
    assert (got["first"].reshape(reps, K, -1) == one["first"][None]).all()
    same_records(one, want, objective, fields=WALKED)
    # two calls queued on one stream, no host in between: the tickets are back at zero, the workspace is shared
    dev = torch.from_numpy(np.array(rows)).cuda()
    perm = np.random.default_rng(5).permutation(K)
    shuffled = torch.from_numpy(np.array(rows)[perm]).cuda()
    a = model.solve_many_clauses_wide(dev, objective, max_nodes=budget)
    b = model.solve_many_clauses_wide(shuffled, "ALL", max_nodes=budget)
    a, b = host(a), host(b)
    same_records(a, one, objective)
    all_walk = wide.walked("sudoku_less_all")
    same_records(b, {f: v[perm] for f, v in all_walk.items()}, "ALL", fields=WALKED)
