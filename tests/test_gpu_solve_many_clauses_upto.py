"""GPU tests of Model.solve_many_clauses_upto (cs_walk_upto: csgpu_solve_many_clauses_upto, _upto_checkpointed, _upto_resume),
Model.classify_many_clauses and the up-to-k slices of Model.solve_many_clauses_sliced.  Yardsticks: the host walk of
tests/many_walk_clauses_upto.py over the sets of tests/many_clause_upto_sets.py, whose figures
test_solve_many_clauses_upto_host.py re-checks, for status, nodes, cuts, solutions and every row; the device's own
solve_many_clauses under ANY and ALL for every field, props included; kernel 6 itself, node by node, for the props of a k
in between; and checks that do not go through a walk at all (the rows satisfy every clause, differ pairwise, and a smaller
k keeps the head of a larger one's rows).  Every call passes a finite max_nodes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import many_clause_sets as sets
import many_clause_upto_sets as usets
import many_walk
import many_walk_clauses_upto as U
import many_walk_objective as W
from csolve_amd import problems
from csolve_amd._lib import CsolveError, ManyUptoOptions, load_library
from csolve_amd.solver import Model, solve_root
from test_gpu_solve_many_clauses import Stepped
from test_solve_many_clauses_upto_host import shipped_walk_upto_kernels

pytestmark = pytest.mark.gpu

E_ARG, E_LIMIT = -1, -4
DONE, LIMIT, BAD_ROOT, BAD_SLOT = 0, 1, 2, 3
SENTINEL = -77
COUNTERS = ("status", "nodes", "cuts", "solutions")  # what the host walk promises
EVERY = COUNTERS + ("props", "root_props")           # what another call of the device promises
# the methods under test, named at import: a library without them does not get as far as collecting this file
METHODS = (Model.solve_many_clauses_upto, Model.classify_many_clauses, Model.many_clauses_upto_kernel)
CASES = [(name, k) for name in sorted(usets.SETS) for k in usets.SETS[name][1]]


@functools.lru_cache(maxsize=None)
def model_of(text):
    return solve_root(text)


def host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


def device_rows(name):
    return torch.from_numpy(np.array(usets.build(name)[1])).cuda()


@functools.lru_cache(maxsize=None)
def answered(name, k, budget=None):
    """the device's answer for a set up to k at the set's budget, its rows written into a buffer full of SENTINEL
    (computed once, not to be changed)"""
    text, roots = usets.build(name)
    rows = torch.full((len(roots), k, roots.shape[1]), SENTINEL, dtype=torch.int32, device="cuda")
    out = model_of(text).solve_many_clauses_upto(np.array(roots), k, max_nodes=usets.SETS[name][2] if budget is None else budget,
                                                 solutions=rows)
    assert out["rows"] is rows
    return host(out)


def same(got, want, label, fields=COUNTERS + ("rows",), rows=None):
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    for f in fields:
        g, w = pick(got[f]), pick(want[f])
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if len(g) else np.zeros(0, dtype=int)
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, want {w[bad[0]]}"


def rows_equal_the_walk(got, want, k, label, blank=SENTINEL):
    """rows below `solutions` are the walk's, the others hold what the buffer held"""
    written = np.arange(k)[None, :] < want["solutions"][:, None]
    assert (got["rows"][written] == want["rows"][written]).all(), f"{label}: a row differs from the walk's"
    assert (got["rows"][~written] == blank).all(), f"{label}: a row at or past `solutions` was written"


@pytest.mark.parametrize("name,k", CASES)
def test_every_instance_equals_the_walk(name, k):
    text, roots = usets.build(name)
    model = model_of(text)
    assert (model.domains() == W.oracle_for(text)[1]).all()  # the rows lie in the device tables' root domains
    kernel = usets.SETS[name][3]
    assert model.qualifies_many_clauses() and model.many_clauses_upto_kernel() == kernel
    # the older calls launch what they launched, and the plan dictionary names none of the three
    assert model.many_clauses_kernel() == kernel.replace("cs_walk_upto", "cs_walk_clauses")
    assert model.many_clauses_resume_kernel() == kernel.replace("cs_walk_upto", "cs_walk_resume")
    assert "walk" not in " ".join(str(v) for v in model.plan().values())
    got, want = answered(name, k), usets.walk(name, k)
    same(got, want, f"{name}, k = {k}", fields=COUNTERS)
    rows_equal_the_walk(got, want, k, f"{name}, k = {k}")
    limit = got["status"] == LIMIT
    assert (got["nodes"][limit] == usets.SETS[name][2]).all() and (got["solutions"] <= k).all()
    if name == usets.UNDECIDED[0]:
        assert np.flatnonzero(limit).tolist() == [usets.UNDECIDED[1]]


def test_the_sets_launch_every_shipped_upto_instantiation():
    planned = {model_of(usets.build(name)[0]).many_clauses_upto_kernel() for name in usets.EIGHT}
    assert planned == shipped_walk_upto_kernels() and len(planned) == 8


@pytest.mark.parametrize("name", usets.EIGHT)
def test_k_1_is_any_field_for_field_and_row_for_row(name):
    text, roots = usets.build(name)
    model = model_of(text)
    dev = device_rows(name)
    one = host(model.solve_many_clauses_upto(dev, 1, max_nodes=usets.BUDGET))
    ref = host(model.solve_many_clauses(dev, "ANY", max_nodes=usets.BUDGET))
    same(one, ref, name, fields=EVERY)
    assert one["rows"].shape == (len(roots), 1, roots.shape[1]) and (one["rows"][:, 0] == ref["first"]).all()
    assert (one["solutions"] > 0).any()


@pytest.mark.parametrize("name,k", [("tree20_all", 64), ("wcet_max", 1200)])
def test_a_k_above_every_tree_is_all_field_for_field(name, k):
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    dev = device_rows(name)
    ref = host(model.solve_many_clauses(dev, "ALL", max_nodes=budget))
    assert (ref["status"] == DONE).all() and 1 < ref["solutions"].max() < k
    rows = torch.full((len(roots), k, roots.shape[1]), SENTINEL, dtype=torch.int32, device="cuda")
    got = host(model.solve_many_clauses_upto(dev, k, max_nodes=budget, solutions=rows))
    same(got, ref, name, fields=EVERY)
    has = ref["solutions"] > 0
    assert (got["rows"][has, 0] == ref["first"][has]).all()
    written = np.arange(k)[None, :] < ref["solutions"][:, None]
    assert (got["rows"][~written] == SENTINEL).all() and (got["rows"][written] != SENTINEL).any()
    for i in np.flatnonzero(has)[:6]:  # every solution of the tree, once
        mine = got["rows"][i, : ref["solutions"][i]]
        assert len({r.tobytes() for r in mine}) == len(mine)


class SteppedUpto(Stepped):
    """the up-to-k walk with every node through Model.propagate on kernel 6, one node per call: kernel 6's own props"""

    def __init__(self, model, text, row):
        super().__init__(model, text, row, "ALL")

    run = many_walk.Walk.run
    result = many_walk.Walk.result


@pytest.mark.parametrize("name", usets.EIGHT)
def test_props_are_kernel_6s_for_a_k_in_between(name):
    """props and root_props of up to four instances of at most 200 nodes under k = 5, and of two under k = 2: the same
    walk, each node one launch of kernel 6"""
    text, roots = usets.build(name)
    model = model_of(text)
    got = {k: answered(name, k) for k in (2, 5)}
    model.set_kernel(6)
    try:
        for k, most in ((5, 4), (2, 2)):
            want = usets.walk(name, k)
            picked = [i for i in np.argsort(-want["nodes"], kind="stable") if 0 < want["nodes"][i] <= 200][:most]
            assert picked
            for i in picked:
                ref = SteppedUpto(model, text, roots[i]).run(usets.BUDGET, k)
                for f in EVERY:
                    assert got[k][f][i] == ref[f], (f, k, i, got[k][f][i], ref[f])
                assert all((got[k]["rows"][i, j] == r).all() for j, r in enumerate(ref["rows"]))
                print(f"{name}[{i}], k = {k}: nodes {ref['nodes']} solutions {ref['solutions']} props {ref['props']} "
                      f"(oracle {want['props'][i]}) root_props {ref['root_props']} (oracle {want['root_props'][i]})")
    finally:
        model.set_kernel(0)


@pytest.mark.parametrize("name", usets.EIGHT)
def test_the_rows_are_solutions_without_asking_a_walk(name):
    """the rows of k = 2 are the first two of k = 5; every stored row makes every clause true; an instance's rows differ"""
    text, roots = usets.build(name)
    model = model_of(text)
    two, five = answered(name, 2), answered(name, 5)
    assert (two["solutions"] == np.minimum(five["solutions"], 2)).all()
    for i in range(len(roots)):
        s2, s5 = int(two["solutions"][i]), int(five["solutions"][i])
        assert (two["rows"][i, :s2] == five["rows"][i, :s2]).all(), i
        mine = five["rows"][i, :s5]
        assert len({r.tobytes() for r in mine}) == s5, f"instance {i}: a solution twice"
        assert ((mine >= roots[i, :, 0]) & (mine <= roots[i, :, 1])).all(), f"instance {i}: a row outside its root row"
    stored = five["rows"][np.arange(5)[None, :] < five["solutions"][:, None]]
    assert len(stored) >= len(roots) // 2
    states = torch.from_numpy(np.ascontiguousarray(np.stack([stored, stored], 2))).cuda()
    true = torch.ones((), dtype=torch.bool, device="cuda")
    for st in states:
        true = true & (model.eval_clauses(st) == 1).all()
    assert bool(true), "a stored row does not satisfy every clause"
    assert (model.eval_root(states) == 1).all()


def test_classify_many_clauses_holds_every_class():
    text, roots = usets.build("schedule5_classes")
    model = model_of(text)
    bad = np.array(roots[:1])
    bad[0, 0, 1] = model.domains()[0, 1] + 1  # outside the root domains
    rows = np.concatenate([np.array(roots), bad])
    cls = model.classify_many_clauses(rows, max_nodes=usets.BUDGET)
    assert cls.dtype == torch.int8 and cls.is_cuda
    want = np.zeros(33, dtype=np.int8)
    want[19], want[2], want[32] = 1, 2, -2
    assert (cls.cpu().numpy() == want).all(), cls
    got = answered("schedule5_classes", 2)
    assert got["nodes"][13] == 52 and got["solutions"][13] == 0
    assert int(((got["nodes"] == 0) & (got["solutions"] == 0)).sum()) == 29  # infeasible at the root
    # undecided within the budget
    name, i = usets.UNDECIDED
    cls = model_of(usets.build(name)[0]).classify_many_clauses(device_rows(name), max_nodes=usets.BUDGET).cpu().numpy()
    walk = usets.walk(name, 2)
    assert cls[i] == -1 and (np.delete(cls, i) == np.delete(walk["solutions"], i)).all()


def test_a_walk_in_slices_is_the_one_call():
    name = "schedule5_slices"
    text, roots = usets.build(name)
    model = model_of(text)
    K, dev = len(roots), device_rows(name)
    after, _ = usets.sliced()
    one = host(model.solve_many_clauses_upto(dev, 5, max_nodes=sum(usets.SLICES)))
    same(one, usets.walk(name, 5), "the one call")
    pool = model.many_clause_checkpoints(K)
    stopped = []
    for s, b in enumerate(usets.SLICES):
        if s == 0:
            out = model.solve_many_clauses_upto(dev, 5, max_nodes=b, checkpoints=pool)
        else:
            assert model.resume_many_clauses(out, max_nodes=b) is out
        got = host(out)
        same(got, after[s], f"after {usets.SLICES[:s + 1]}")
        assert ((got["slot"] >= 0) == (got["status"] == LIMIT)).all()
        used = got["slot"][got["slot"] >= 0]
        assert len(set(used.tolist())) == len(used) and (used < K).all()
        stopped.append(int((got["status"] == LIMIT).sum()))
    assert stopped == [29, 4, 0]
    same(got, one, "at the end against the one call", fields=EVERY + ("rows",))
    # the same three calls queued on one stream, no host in between
    pool.reset()
    torch.cuda.synchronize()
    out = model.solve_many_clauses_upto(dev, 5, max_nodes=usets.SLICES[0], checkpoints=pool)
    model.resume_many_clauses(out, max_nodes=usets.SLICES[1])
    model.resume_many_clauses(out, max_nodes=usets.SLICES[2])
    got = host(out)
    same(got, one, "three calls queued on one stream", fields=EVERY + ("rows",))
    assert (got["slot"] == -1).all()
    # and the method that makes them
    out = model.solve_many_clauses_sliced(dev, max_solutions=5, budgets=usets.SLICES, checkpoints=pool)
    assert out["sliced"] == {"slices": 3, "searched": 0}
    same(host(out), one, "solve_many_clauses_sliced", fields=EVERY + ("rows",))
    with pytest.raises(ValueError, match="k-th solution"):
        model.solve_many_clauses_sliced(dev, max_solutions=5, budgets=usets.SLICES, finish="search")
    pool.close()


def test_a_full_pool_ends_an_instance_as_without_checkpoints():
    name = "schedule5_slices"
    text, roots = usets.build(name)
    model = model_of(text)
    K, capacity, dev = len(roots), 16, device_rows(name)
    first, rest = usets.SLICES[0], sum(usets.SLICES[1:])
    plain = host(model.solve_many_clauses_upto(dev, 5, max_nodes=first))
    whole = host(model.solve_many_clauses_upto(dev, 5, max_nodes=first + rest))
    assert int((plain["status"] == LIMIT).sum()) == 29
    pool = model.many_clause_checkpoints(capacity)
    out = model.solve_many_clauses_upto(dev, 5, max_nodes=first, checkpoints=pool)
    got = host(out)
    same(got, plain, "budget 8, sixteen slots", fields=EVERY + ("rows",))
    kept = np.flatnonzero(got["slot"] >= 0)
    others = np.setdiff1d(np.arange(K), kept)
    assert kept.size == capacity and sorted(got["slot"][kept].tolist()) == list(range(capacity))
    assert int((got["status"][others] == LIMIT).sum()) == 13 and (got["slot"][others] == -1).all()
    model.resume_many_clauses(out, max_nodes=rest)
    got = host(out)
    same(got, whole, "the sixteen with a slot", fields=EVERY + ("rows",), rows=kept)
    same(got, plain, "everything else", fields=EVERY + ("rows",), rows=others)
    assert (got["slot"] == -1).all()
    pool.close()


def test_a_resume_with_a_smaller_k_ends_the_instances_that_hold_it():
    name = "schedule5_slices"
    text, roots = usets.build(name)
    model = model_of(text)
    K, dev = len(roots), device_rows(name)
    first, rest = usets.SLICES[0], sum(usets.SLICES[1:])
    pool = model.many_clause_checkpoints(K)
    out = model.solve_many_clauses_upto(dev, 5, max_nodes=first, checkpoints=pool)
    before = host(out)
    holds = (before["status"] == LIMIT) & (before["solutions"] >= 2)
    goes_on = (before["status"] == LIMIT) & (before["solutions"] < 2)
    assert holds.sum() >= 4 and goes_on.sum() >= 4
    model.resume_many_clauses(out, max_nodes=rest, max_solutions=2)
    got = host(out)
    assert got["rows"].shape == before["rows"].shape  # [K, 5, n] stays
    assert (got["status"][holds] == DONE).all() and (got["slot"][holds] == -1).all()
    for f in EVERY[1:] + ("rows",):
        assert (got[f][holds] == before[f][holds]).all(), f
    want = U.walk_many_upto(text, roots, None, slices=[(first, 5), (rest, 2)])
    same(got, want, "8 nodes up to 5, then up to 2")
    assert (got["status"] == DONE).all() and (got["solutions"][goes_on] == 2).all()
    pool.close()


def test_bad_slots_get_their_status_and_nothing_else():
    name = "schedule5_slices"
    text, roots = usets.build(name)
    model = model_of(text)
    K, dev = len(roots), device_rows(name)
    first, rest = usets.SLICES[0], sum(usets.SLICES[1:])
    whole = host(model.solve_many_clauses_upto(dev, 5, max_nodes=first + rest))
    pool = model.many_clause_checkpoints(K + 2)  # two slots are never drawn: they stay zeroed
    out = model.solve_many_clauses_upto(dev, 5, max_nodes=first, checkpoints=pool)
    before = host(out)
    stopped = np.flatnonzero(before["status"] == LIMIT)
    assert stopped.size == 29 and before["slot"].max() < K
    # the open subtrees of an up-to-k checkpoint are the host walk's, and it has no incumbent
    walks = usets.sliced()[1][0]
    for i in stopped[:6]:
        states, incumbent = model.clause_checkpoint_states(pool, int(before["slot"][i]))
        assert incumbent is None and tuple(states.shape) == walks[int(i)].shape, i
        assert (states.cpu().numpy() == walks[int(i)]).all(), f"instance {i}"
    a, b = int(stopped[1]), int(stopped[3])
    out["slot"][a] = K + 2  # the first number past the pool
    out["slot"][b] = K + 1  # inside the pool, never written
    model.resume_many_clauses(out, max_nodes=rest)
    got = host(out)
    assert got["status"][a] == BAD_SLOT and got["status"][b] == BAD_SLOT
    assert got["slot"][a] == K + 2 and got["slot"][b] == K + 1
    for f in EVERY[1:] + ("rows",):
        assert (got[f][[a, b]] == before[f][[a, b]]).all(), f
    same(got, whole, "the neighbours", fields=EVERY + ("rows",), rows=np.setdiff1d(np.arange(K), [a, b]))
    # an up-to-k checkpoint under the objectives of csgpu_solve_many_clauses_resume: refused under each of them
    pool.reset()
    out = model.solve_many_clauses_upto(dev, 5, max_nodes=first, checkpoints=pool)
    before = host(out)
    had = before["slot"] >= 0
    assert had.sum() == 29 and model.objective == W.CODE["MIN"]
    for objective in ("ANY", "ALL", "MIN"):
        other = {f: v for f, v in out.items() if f not in ("_upto", "rows")}
        other["_objective"], other["_best"] = W.CODE[objective], None
        model.resume_many_clauses(other, max_nodes=rest)
        got = host(out)
        assert (got["status"][had] == BAD_SLOT).all() and (got["status"][~had] == before["status"][~had]).all(), objective
        for f in EVERY[1:] + ("rows", "slot"):
            assert (got[f] == before[f]).all(), (objective, f)
    # and by its own resume it goes on
    model.resume_many_clauses(out, max_nodes=rest)
    same(host(out), whole, "after the refusals", fields=EVERY + ("rows",))
    # the reverse: a checkpoint made under ALL by solve_many_clauses, given to the up-to-k resume
    pool.reset()
    made = model.solve_many_clauses(dev, "ALL", max_nodes=first, checkpoints=pool)
    before = host(made)
    had = before["slot"] >= 0
    assert had.sum() >= 20
    as_upto = dict(made)
    as_upto["_upto"] = 5
    rows = torch.full((K, 5, roots.shape[1]), SENTINEL, dtype=torch.int32, device="cuda")
    as_upto["rows"] = rows
    model.resume_many_clauses(as_upto, max_nodes=rest)
    got = host(made)
    assert (got["status"][had] == BAD_SLOT).all() and (got["status"][~had] == before["status"][~had]).all()
    for f in EVERY[1:] + ("first", "slot"):
        assert (got[f] == before[f]).all(), f
    assert (rows == SENTINEL).all()
    model.resume_many_clauses(made, max_nodes=rest)  # under ALL it goes on
    got = host(made)
    assert (got["status"] == host(model.solve_many_clauses(dev, "ALL", max_nodes=first + rest))["status"]).all()
    pool.close()


def test_more_instances_than_waves_and_a_permutation():
    name, k, count = "linear20_all", 2, 20000
    text, roots = usets.build(name)
    model = model_of(text)
    assert count > model.many_clauses_waves(1 << 30) > 0
    idx = np.arange(count) % len(roots)
    want = usets.walk(name, k)
    big = torch.from_numpy(np.array(roots)[idx]).cuda()
    got = host(model.solve_many_clauses_upto(big, k, max_nodes=usets.BUDGET))
    same(got, {f: want[f][idx] for f in COUNTERS + ("rows",)}, "20,000 instances")
    own = answered(name, k)
    assert (got["props"] == own["props"][idx]).all() and (got["root_props"] == own["root_props"][idx]).all()
    perm = np.random.default_rng(5).permutation(count)
    shuffled = host(model.solve_many_clauses_upto(big[torch.from_numpy(perm).cuda()].contiguous(), k, max_nodes=usets.BUDGET))
    same(shuffled, {f: got[f][perm] for f in EVERY + ("rows",)}, "the permuted batch", fields=EVERY + ("rows",))


def test_errors_with_a_finalized_model():
    import many_sets
    text = problems.schedule(32, 1)
    model = model_of(text)
    assert model.n_clauses > 512 and not model.qualifies_many_clauses() and model.many_clauses_upto_kernel() is None
    rows = np.repeat(model.domains()[None], 2, 0)
    for r in (rows, torch.from_numpy(rows).cuda()):
        with pytest.raises(CsolveError) as e:
            model.solve_many_clauses_upto(r, 2, max_nodes=10)
        assert e.value.code == E_LIMIT and "512" in str(e.value)
    text = problems.queens(8, "ALL")  # a model of both families
    model = model_of(text)
    assert model.qualifies(7) and model.qualifies_many_clauses()
    rows = np.concatenate([model.domains()[None], many_sets.queens_two(8, 7, 3)]).astype(np.int32)
    dev = torch.from_numpy(rows).cuda()
    clause_pool, dive_pool = model.many_clause_checkpoints(8), model.many_checkpoints(8)
    with pytest.raises(CsolveError, match="other kind") as e:
        model.solve_many_clauses_upto(dev, 2, max_nodes=4, checkpoints=dive_pool)
    assert e.value.code == E_ARG
    other_text, other_roots = usets.build("linear20_all")
    with pytest.raises(CsolveError, match="another model") as e:
        model_of(other_text).solve_many_clauses_upto(np.array(other_roots), 2, max_nodes=4, checkpoints=clause_pool)
    assert e.value.code == E_ARG
    # a null pool or null slots, after the checks of csgpu_solve_many_clauses_upto; k < 1 before them
    L = load_library()
    res = torch.zeros((len(rows), 5), dtype=torch.int64, device="cuda")
    slots = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    opt = ManyUptoOptions(2, 0, 4)
    for ck, sl in ((None, slots.data_ptr()), (clause_pool._h, None)):
        assert L.csgpu_solve_many_clauses_upto_checkpointed(model._h, dev.data_ptr(), len(rows), C.byref(opt), res.data_ptr(),
                                                            None, ck, sl, None) == E_ARG
        assert L.csgpu_solve_many_clauses_upto_resume(model._h, len(rows), C.byref(opt), res.data_ptr(), None, ck, sl,
                                                      None) == E_ARG
    with pytest.raises(CsolveError, match="max_solutions") as e:
        model.solve_many_clauses_upto(dev, 0, max_nodes=4)
    assert e.value.code == E_ARG
    torch.cuda.synchronize()
    assert (res == 0).all() and (slots == -1).all()
    # an empty batch launches nothing
    empty = model.solve_many_clauses_upto(np.zeros((0, model.n_vars, 2), dtype=np.int32), 3, max_nodes=5, checkpoints=clause_pool)
    assert empty["status"].shape == (0,) and tuple(empty["rows"].shape) == (0, 3, model.n_vars)
    assert model.resume_many_clauses(empty, max_nodes=5)["status"].shape == (0,)
    assert model.classify_many_clauses(np.zeros((0, model.n_vars, 2), dtype=np.int32), max_nodes=5).shape == (0,)
    # a kernel-7 model that also qualifies here gives the rows of solve_many_upto, slices included
    for k in (1, 3, 100):
        a = host(model.solve_many_clauses_upto(dev, k, max_nodes=1 << 15))
        b = host(model.solve_many_upto(dev, k, max_nodes=1 << 15))
        same(a, b, f"queens-8, k = {k}")
        assert (a["status"] == DONE).all()
    a = model.solve_many_clauses_upto(dev, 3, max_nodes=4, checkpoints=clause_pool)
    b = model.solve_many_upto(dev, 3, max_nodes=4, checkpoints=dive_pool)
    assert (host(a)["slot"] >= 0).any()
    same(host(a), host(b), "queens-8, four nodes")
    same(host(model.resume_many_clauses(a, max_nodes=1 << 15)), host(model.resume_many(b, max_nodes=1 << 15)), "queens-8, resumed")
