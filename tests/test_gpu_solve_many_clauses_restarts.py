"""GPU tests of Model.solve_many_clauses_restarts (cs_walk_restart, csgpu_solve_many_clauses_restarts): status, nodes, cuts,
solutions, the restart count and the solution row of every instance of every set of tests/many_clause_restart_sets.py
against the host walk of tests/many_walk_clauses_restarts.py, which asks the oracle for every node; root_props of every
instance against kernel 6's own root node, and props against the same walk stepped through kernel 6 itself; base 0
without flags against the ANY call; seeds per instance; ROTATE_FIRST; the budget; batches larger than the grid; queued
calls; the workspace after an ordinary clause call; rows that are not searched; refusals.  Rows that must stay untouched
are pre-filled with a sentinel.  Every call passes a finite max_nodes.

root_props are, like props, kernel 6's (include/csolve_gpu.h: "props / root_props = kernel 6's props of the consistent
children / of the root"), which the oracle's need not equal and mostly do not: kernel 6 counts 41 narrowings of a
mixed120 root node where the oracle counts 42, 12 where it counts 16 on a schedule5 row; they differ for 5 of mixed120's
8 rows and 26 of schedule5's 32, under solve_many_clauses as under this call (the test prints the count per set).  So
the reference for root_props is one launch of kernel 6 over all root rows as `var < 0` nodes, every instance of every
set."""
import numpy as np
import pytest

import many_clause_restart_sets as rsets
import many_walk_clauses_restarts as R
import many_walk_objective as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("status", "nodes", "cuts", "solutions")  # against the host walk; root_props and props: against kernel 6
ALL = FIELDS + ("restarts",)
EVERY = ALL + ("props", "first")  # what another call of the device promises
DONE, LIMIT, BAD_ROOT = 0, 1, 2
SENTINEL = -7
_models = {}
_devs = {}


def _model(text):
    from csolve_amd.solver import solve_root
    if text not in _models:
        _models[text] = solve_root(text)
    return _models[text]


def _set(name):
    """(text, roots, roots on the device, seeds), built once"""
    text, roots, seeds = rsets.build(name)
    if name not in _devs:
        _devs[name] = torch.from_numpy(np.array(roots)).cuda()
    return text, roots, _devs[name], seeds


def _host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v) and not f.startswith("_")}


def _run(model, dev, base, budget, **kw):
    rows = torch.full((dev.shape[0], model.n_vars), SENTINEL, dtype=torch.int32, device="cuda")
    return _host(model.solve_many_clauses_restarts(dev, max_nodes=budget, restart_base=base, solutions=rows, **kw))


def _root_props(model, dev, want):
    """kernel 6's props of the root node of every row, one launch; 0 for a row that is not searched or inconsistent"""
    K = dev.shape[0]
    nodes = torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32, device="cuda").repeat(K, 1)
    nodes[:, 3] = torch.arange(K, dtype=torch.int32, device="cuda")  # node i is row i
    rows = dev.clone()
    rows[torch.from_numpy(want["status"] == BAD_ROOT).cuda()] = torch.from_numpy(model.domains()).cuda()  # not searched: not asked
    model.set_kernel(6)
    try:
        _, res = model.propagate(rows, nodes)
        res = res.cpu().numpy()
    finally:
        model.set_kernel(0)
    return np.where((want["status"] == BAD_ROOT) | (res[:, 0] < 0), 0, res[:, 1]).astype(np.int64)


def _check(got, want, label, root_props=None):
    """the fields and the restarts of every instance; root_props against kernel 6's where given; the solution row of an
    instance that has one, the sentinel elsewhere"""
    if root_props is not None:
        bad = np.flatnonzero(got["root_props"] != root_props)
        assert bad.size == 0, f"{label}: root_props differs from kernel 6's for {bad.size} instances, first {bad[0]}"
    for f in ALL:
        g, w = got[f].astype(np.int64), want[f]
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, walk {w[bad[0]]}"
    has = want["solutions"] > 0
    assert (got["first"][has] == want["first"][has]).all(), f"{label}: solution rows differ"
    assert (got["first"][~has] == SENTINEL).all(), f"{label}: the row of an instance without a solution was written"


_answers = {}


def _answered(name, base):
    """the device's answer for a set under `base` at its budget (computed once, not to be changed)"""
    if (name, base) not in _answers:
        text, roots, dev, seeds = _set(name)
        _answers[name, base] = _run(_model(text), dev, base, rsets.SETS[name][3], seed=rsets.SEED, seeds=seeds)
    return _answers[name, base]


CASES = [(name, base) for name in sorted(rsets.SETS) for base in rsets.SETS[name][1]]


@pytest.mark.parametrize("name,base", CASES)
def test_every_field_restarts_and_row_equal_the_walk(name, base):
    text, roots, dev, seeds = _set(name)
    _, _, _, budget, kernel, recorded = rsets.SETS[name]
    want = rsets.walk(name, base)
    assert (want["status"] != LIMIT).all() and want["nodes"].max() < budget, "the set must stay below its budget"
    assert (want["restarts"] > 0).sum() == recorded[base][1] > 0, "the set must restart"
    model = _model(text)
    assert (model.domains() == W.oracle_for(text)[1]).all()  # the rows lie in the device tables' root domains
    assert model.many_clauses_restart_kernel() == kernel
    assert model.many_clauses_kernel() == kernel.replace("cs_walk_restart", "cs_walk_clauses")  # as it was
    got = _answered(name, base)
    print(f"{name}, base {base}: {len(roots)} instances, largest walk {int(want['nodes'].max())} nodes, "
          f"{int((want['restarts'] > 0).sum())} restarted, at most {int(want['restarts'].max())} times")
    six = _root_props(model, dev, want)
    print(f"root_props: kernel 6's differ from the oracle's for {int((six != want['root_props']).sum())} instances")
    _check(got, want, f"{name}, base {base}", six)


class _Six:
    """Oracle.instance through Model.propagate on kernel 6, one node per call: kernel 6's own props"""

    def __init__(self, model):
        self.model = model

    def instance(self, state, v, lo, hi):
        st = torch.from_numpy(np.array(state, dtype=np.int32)[None]).cuda()
        node = torch.tensor([[v, lo, hi, 0]], dtype=torch.int32, device="cuda")
        out, res = self.model.propagate(st, node)
        res = res.cpu().numpy()[0]
        return (-1, None) if res[0] < 0 else (int(res[1]), out.cpu().numpy()[0])


@pytest.mark.parametrize("name", sorted(rsets.SETS))
def test_props_are_kernel_6s(name):
    """props and root_props of up to three restarting instances of at most 200 nodes: the same walk, each node one launch
    of kernel 6"""
    text, roots, dev, seeds = _set(name)
    base, budget = rsets.SETS[name][1][0], rsets.SETS[name][3]
    model = _model(text)
    got, want = _answered(name, base), rsets.walk(name, base)
    order = np.argsort(-want["nodes"], kind="stable")
    picked = [i for i in order if want["restarts"][i] > 0 and want["nodes"][i] <= 200][:3]
    assert picked
    model.set_kernel(6)
    try:
        for i in picked:
            seed = rsets.SEED if seeds is None else int(seeds[i])
            ref = R.walk_restarts(text, roots[i], base, seed, max_nodes=budget, orc=_Six(model))
            for f in ALL + ("props", "root_props"):
                assert got[f][i] == ref[f], (f, i, got[f][i], ref[f])
            print(f"{name}[{i}]: nodes {ref['nodes']} restarts {ref['restarts']} props {ref['props']} (oracle {want['props'][i]}) "
                  f"root_props {ref['root_props']} (oracle {want['root_props'][i]})")
    finally:
        model.set_kernel(0)


@pytest.mark.parametrize("name", ["schedule6", "mixed40", "schedule5_unsat"])
def test_base_0_without_flags_is_the_any_call(name):
    text, roots, dev, _ = _set(name)
    model = _model(text)
    budget = rsets.SETS[name][3]
    want = _host(model.solve_many_clauses(dev, "ANY", max_nodes=budget))
    got = _host(model.solve_many_clauses_restarts(dev, max_nodes=budget, restart_base=0, seed=99))
    for f in ("status", "root_props", "nodes", "cuts", "props", "solutions", "first"):  # every field of the records, and the rows
        assert (got[f] == want[f]).all(), f
    assert (got["restarts"] == 0).all() and (want["nodes"] > 0).any()
    # seeds do not matter without rotate_first, and a budget below the largest walk stops both at the same node
    small_a = _host(model.solve_many_clauses(dev, "ANY", max_nodes=7))
    small_r = _host(model.solve_many_clauses_restarts(dev, max_nodes=7, restart_base=0, seeds=np.arange(len(roots))))
    assert (small_a["status"] == LIMIT).any()
    for f in ("status", "root_props", "nodes", "cuts", "props", "solutions", "first"):
        assert (small_a[f] == small_r[f]).all(), f


def test_seeds_belong_to_the_instance():
    text, roots, dev, _ = _set("schedule6")
    model = _model(text)
    budget, base, K = 4096, 1, 24
    seeds = np.array([1, 2, 3, 2 ** 32 - 1] * (K // 4), dtype=np.uint32)
    want = R.walk_many_restarts(text, roots, base, seeds=seeds, max_nodes=budget)
    assert (want["restarts"] > 0).sum() >= 8 and (want["status"] == DONE).all()
    got = _run(model, dev, base, budget, seeds=seeds)
    _check(got, want, "seeds per instance", _root_props(model, dev, want))
    # equals separate calls with a single seed (d_seeds == NULL: options->seed)
    differ = 0
    for s in (1, 2, 3, 2 ** 32 - 1):
        one = _run(model, dev, base, budget, seed=s)
        mine = np.flatnonzero(seeds == s)
        for f in EVERY:
            assert (one[f][mine] == got[f][mine]).all(), (s, f)
        differ += int((one["nodes"] != got["nodes"]).sum())
    assert differ > 0, "the seed must matter"
    # a permutation of rows and seeds permutes the answers
    perm = np.random.default_rng(5).permutation(K)
    shuffled = _run(model, dev[torch.from_numpy(perm).cuda()].contiguous(), base, budget, seeds=seeds[perm])
    for f in EVERY:
        assert (shuffled[f] == got[f][perm]).all(), f
    # seeds as a device tensor
    again = _run(model, dev, base, budget, seeds=torch.from_numpy(seeds.view(np.int32)).cuda())
    for f in EVERY:
        assert (again[f] == got[f]).all(), f


def _is_a_solution(text, row):
    from oracle.cs_oracle import Model as OModel, Oracle
    om = OModel.parse(text)
    om.set_domains(np.stack([row, row], 1).astype(np.int32))
    om.index()
    return Oracle(om).eval(om.root) == (1, 1)


def test_rotate_first_gives_valid_and_mostly_distinct_solutions():
    text, roots, dev, _ = _set("schedule6")
    model = _model(text)
    widest = int(np.argmax((roots[:, :, 1] - roots[:, :, 0]).sum(1)))
    seeds = np.arange(1, 25, dtype=np.uint32)
    batch = np.repeat(np.array(roots[widest])[None], 24, 0)
    bdev = torch.from_numpy(batch).cuda()
    for base in (0, 1):  # one seeded walk, and with restarts
        want = R.walk_many_restarts(text, batch, base, seeds=seeds, rotate_first=True, max_nodes=4096)
        assert (want["status"] == DONE).all() and (want["solutions"] == 1).all()
        got = _run(model, bdev, base, 4096, seeds=seeds, rotate_first=True)
        _check(got, want, f"rotate_first, base {base}", _root_props(model, bdev, want))
        for row in got["first"]:
            assert ((row >= batch[0][:, 0]) & (row <= batch[0][:, 1])).all() and _is_a_solution(text, row)
        assert len({r.tobytes() for r in got["first"]}) >= 12, "mostly distinct"
    # without the flag and without restarts every seed walks the ascending walk: one solution
    plain = _run(model, bdev[:4].contiguous(), 0, 4096, seeds=seeds[:4])
    assert len({r.tobytes() for r in plain["first"]}) == 1 and (plain["restarts"] == 0).all()


def test_the_budget_counts_all_runs():
    name = "schedule6"
    text, roots, dev, _ = _set(name)
    model = _model(text)
    full = rsets.walk(name, 1)
    for budget in (60, 23):
        want = rsets.walk(name, 1, max_nodes=budget)
        over = full["nodes"] > budget
        assert over.sum() >= 3 and (~over).any(), "the budget must split the set"
        assert (want["status"][over] == LIMIT).all() and (want["nodes"][over] == budget).all()
        assert (want["restarts"][over] > 0).all(), "a stopped instance has restarted"
        got = _run(model, dev, 1, budget, seed=rsets.SEED)
        _check(got, want, f"{name}, base 1, budget {budget}", _root_props(model, dev, want))
        assert (got["status"][over] == LIMIT).all() and (got["nodes"][over] == budget).all()
        assert (got["first"][over] == SENTINEL).all()
        for f in ALL:  # those below the budget are as without it
            assert (got[f][~over] == full[f][~over]).all(), f


def test_more_instances_than_waves_and_calls_queued_without_the_host():
    name = "schedule5"
    text, roots, dev, _ = _set(name)
    model = _model(text)
    budget = rsets.SETS[name][3]
    own = _answered(name, 1)
    resident = model.many_clauses_waves(1 << 30)
    reps = -(-4 * resident // len(roots))
    big = dev.repeat(reps, 1, 1).contiguous()
    K = big.shape[0]
    assert K >= 4 * resident
    print(f"{K} instances on at most {resident} waves")
    torch.cuda.synchronize()
    a = model.solve_many_clauses_restarts(big, max_nodes=budget, restart_base=1, seed=rsets.SEED)
    b = model.solve_many_clauses_restarts(big, max_nodes=budget, restart_base=1, seed=rsets.SEED)  # queued behind a
    for got in (_host(a), _host(b)):
        for f in EVERY:
            w = np.where(own["solutions"][:, None] > 0, own[f], 0) if f == "first" else own[f]
            tiled = np.tile(w, (reps,) + (1,) * (w.ndim - 1))
            bad = np.flatnonzero((got[f] != tiled).reshape(K, -1).any(axis=1))
            assert bad.size == 0, f"{f} differs for {bad.size} instances, first {bad[0]}"


def test_queued_behind_the_other_clause_calls_on_one_stream():
    """solve_many_clauses (ANY), solve_many_clauses_upto, solve_many_clauses_restarts, solve_many_clauses (MIN) and restarts
    again back to back, no synchronisation in between: each equals its stand-alone answer, so every call left the ticket
    counters at zero and the workspace usable"""
    name = "schedule5"
    text, roots, dev, _ = _set(name)
    model = _model(text)
    budget = 1 << 15
    alone_any = _host(model.solve_many_clauses(dev, "ANY", max_nodes=budget))
    alone_upto = _host(model.solve_many_clauses_upto(dev, 2, max_nodes=budget))
    alone_min = _host(model.solve_many_clauses(dev, "MIN", max_nodes=budget))
    torch.cuda.synchronize()
    a = model.solve_many_clauses(dev, "ANY", max_nodes=budget)
    b = model.solve_many_clauses_upto(dev, 2, max_nodes=budget)
    c = model.solve_many_clauses_restarts(dev, max_nodes=rsets.SETS[name][3], restart_base=1, seed=rsets.SEED)
    d = model.solve_many_clauses(dev, "MIN", max_nodes=budget)
    e = model.solve_many_clauses_restarts(dev, max_nodes=rsets.SETS[name][3], restart_base=2, seed=rsets.SEED)
    a, b, c, d, e = _host(a), _host(b), _host(c), _host(d), _host(e)
    every = ("status", "root_props", "nodes", "cuts", "props", "solutions")
    for got, want, fields in ((a, alone_any, every + ("first",)), (b, alone_upto, every + ("rows",)),
                              (d, alone_min, every + ("first", "best"))):
        for f in fields:
            assert (got[f] == want[f]).all(), f
    for got, base in ((c, 1), (e, 2)):
        want = rsets.walk(name, base)
        for f in ALL + ("first",):
            assert (got[f] == want[f]).all(), (base, f)
        assert (got["props"] == _answered(name, base)["props"]).all()


def test_the_workspace_grows_for_the_restart_call_after_an_ordinary_clause_call():
    """a model whose first call of the family is an ordinary clause call: the workspace then holds n frames per wave, and
    the restart call, with the same waves, needs n + 1"""
    from csolve_amd.solver import solve_root
    name = "schedule6"
    text, roots, dev, _ = _set(name)
    model = solve_root(text)  # a model of its own: nothing of the family has run on it
    budget = rsets.SETS[name][3]
    resident = model.many_clauses_waves(1 << 30)
    reps = -(-resident // len(roots))
    big = dev.repeat(reps, 1, 1).contiguous()  # every resident wave walks, the last one in the last frames of the block
    assert big.shape[0] >= resident
    first = _host(model.solve_many_clauses(big, "ANY", max_nodes=budget))
    got = _host(model.solve_many_clauses_restarts(big, max_nodes=budget, restart_base=1, seed=rsets.SEED))
    again = _host(model.solve_many_clauses(big, "ANY", max_nodes=budget))
    want = rsets.walk(name, 1)
    for f in ALL + ("first",):
        assert (got[f].reshape((reps, len(roots)) + got[f].shape[1:]) == want[f][None]).all(), f
    for f in ("status", "root_props", "nodes", "cuts", "props", "solutions", "first"):
        assert (first[f] == again[f]).all(), f
    # and on a model of both families, behind solve_many, whose frames are sized for kernel 7
    from csolve_amd import problems
    text8 = problems.queens(8, "ALL")
    m8 = solve_root(text8)
    assert m8.qualifies(7) and m8.many_clauses_restart_kernel().startswith("cs_walk_restart<")
    rows = np.repeat(m8.domains()[None], 8, 0).astype(np.int32)
    a = _host(m8.solve_many(rows, "ANY", max_nodes=1 << 12))
    b = _host(m8.solve_many_clauses_restarts(rows, max_nodes=1 << 12, restart_base=1, seeds=np.arange(8)))
    c = _host(m8.solve_many_restarts(rows, max_nodes=1 << 12, restart_base=1, seeds=np.arange(8)))
    assert (a["solutions"] == 1).all() and (b["solutions"] == 1).all()
    for f in ("status", "nodes", "cuts", "solutions", "restarts", "first"):  # the two families walk the same walk
        assert (b[f] == c[f]).all(), f
    assert (b["restarts"] > 0).any()


def test_bad_and_trivial_rows_leave_their_neighbours_alone():
    name = "schedule5"
    text, roots, dev, _ = _set(name)
    model = _model(text)
    budget = rsets.SETS[name][3]
    want = rsets.walk(name, 1)
    _, dom = W.oracle_for(text)
    restarting = [int(i) for i in np.flatnonzero(want["restarts"] > 0)[:3]]
    batch = np.repeat(dom[None], 7, 0).astype(np.int32)
    for slot, i in zip((0, 2, 6), restarting):
        batch[slot] = roots[i]
    batch[1, 3, 1] = dom[3, 1] + 1                       # outside the root domains
    batch[3, 2] = (dom[2, 0] + 1, dom[2, 0])             # lo > hi
    solved = want["first"][restarting[0]]
    batch[4] = np.stack([solved, solved], 1)             # a solution already
    starts = [i for i, s in enumerate(model.var_names()) if s.endswith("_start")]
    batch[5, starts[0]] = batch[5, starts[1]] = max(dom[starts[0], 0], dom[starts[1], 0])  # two tasks at one time
    walked = R.walk_many_restarts(text, batch, 1, seed=rsets.SEED, max_nodes=budget)
    assert walked["status"].tolist() == [DONE, BAD_ROOT, DONE, BAD_ROOT, DONE, DONE, DONE]
    assert (walked["nodes"][4], walked["solutions"][4]) == (0, 1) and (walked["first"][4] == solved).all()
    assert (walked["nodes"][5], walked["solutions"][5], walked["root_props"][5]) == (0, 0, 0)
    assert walked["restarts"][[1, 3, 4, 5]].tolist() == [0, 0, 0, 0]
    for slot, i in zip((0, 2, 6), restarting):  # the neighbours are the instances they are alone
        assert all(walked[f][slot] == want[f][i] for f in ALL) and (walked["first"][slot] == want["first"][i]).all()
    assert walked["restarts"][[0, 2, 6]].min() > 0
    bdev = torch.from_numpy(batch).cuda()
    restarts = torch.full((7,), SENTINEL, dtype=torch.int32, device="cuda")  # the library itself: 0 is written, not left
    got = _run(model, bdev, 1, budget, seed=rsets.SEED)
    _check(got, walked, "bad and trivial rows", _root_props(model, bdev, walked))
    assert got["restarts"][[1, 3, 4, 5]].tolist() == [0, 0, 0, 0] and (got["props"][[1, 3, 4, 5]] == 0).all()
    import ctypes as C
    from csolve_amd._lib import ManyRestartOptions, load_library
    res = torch.zeros((7, 5), dtype=torch.int64, device="cuda")
    opt = ManyRestartOptions(budget, 1, rsets.SEED, 0)
    rc = load_library().csgpu_solve_many_clauses_restarts(model._h, bdev.data_ptr(), None, 7, C.byref(opt), res.data_ptr(), None,
                                                          restarts.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert (restarts.cpu().numpy() == walked["restarts"]).all()
    # the optional outputs: d_solutions == NULL, d_restarts == NULL, both
    for kw in (dict(solutions=False), dict(restarts=False), dict(solutions=False, restarts=False)):
        out = _host(model.solve_many_clauses_restarts(bdev, max_nodes=budget, restart_base=1, seed=rsets.SEED, **kw))
        assert ("first" in out) == ("solutions" not in kw) and ("restarts" in out) == ("restarts" not in kw)
        assert (out["root_props"] == got["root_props"]).all() and (out["props"] == got["props"]).all()
        for f in out:
            if f not in ("props", "root_props"):  # (kernel 6's: compared above)
                assert (out[f] == (walked[f] if f != "first" else np.where(walked["solutions"][:, None] > 0, walked["first"], 0))).all(), (kw, f)
    empty = model.solve_many_clauses_restarts(torch.empty((0, model.n_vars, 2), dtype=torch.int32, device="cuda"), max_nodes=5)
    assert empty["status"].shape == (0,) and empty["first"].shape == (0, model.n_vars) and empty["restarts"].shape == (0,)


def test_models_outside_the_family_and_bad_options_are_refused():
    from csolve_amd import CsolveError, problems
    model = _model(problems.schedule(32, 1))  # more than 512 clauses
    assert model.n_clauses > 512 and not model.qualifies_many_clauses() and model.many_clauses_restart_kernel() is None
    rows = np.repeat(model.domains()[None], 2, 0)
    for r in (rows, torch.from_numpy(rows).cuda()):
        with pytest.raises(CsolveError) as e:
            model.solve_many_clauses_restarts(r, max_nodes=10)
        assert e.value.code == -4 and "512" in str(e.value)
    seven = _model(problems.sudoku_roots(3, 0.4, [1])[0])  # 810 != clauses: kernel 7 only
    assert seven.qualifies(7) and not seven.qualifies(6) and seven.many_clauses_restart_kernel() is None
    rows = torch.from_numpy(np.repeat(seven.domains()[None], 2, 0)).cuda()
    with pytest.raises(CsolveError, match="does not qualify") as e:
        seven.solve_many_clauses_restarts(rows, max_nodes=10)
    assert e.value.code == -4
    assert (_host(seven.solve_many_restarts(rows, max_nodes=1 << 12))["solutions"] == 1).all()  # its own family takes it
    text, roots, dev, _ = _set("schedule5")
    model = _model(text)
    for kw, word in ((dict(restart_base=-2), "restart_base"), (dict(max_nodes=0), "max_nodes")):
        args = dict(max_nodes=100)
        args.update(kw)
        with pytest.raises(CsolveError, match=word) as e:  # a finalized model: still before any launch
            model.solve_many_clauses_restarts(dev, **args)
        assert e.value.code == -1
    import ctypes as C
    from csolve_amd._lib import ManyRestartOptions, load_library
    res = torch.zeros((len(roots), 5), dtype=torch.int64, device="cuda")
    opt = ManyRestartOptions(100, 1, 0, 2)  # a flag bit other than ROTATE_FIRST
    L = load_library()
    assert L.csgpu_solve_many_clauses_restarts(model._h, dev.data_ptr(), None, len(roots), C.byref(opt), res.data_ptr(), None, None, None) == -1
    assert "flags" in L.csgpu_last_error().decode()
    torch.cuda.synchronize()
    assert (res == 0).all()


def test_the_sets_launch_every_shipped_restart_instantiation():
    from test_solve_many_clauses_restarts_host import shipped_walk_restart_kernels
    planned = {_model(rsets.build(name)[0]).many_clauses_restart_kernel() for name in rsets.SETS}
    assert planned == shipped_walk_restart_kernels() and len(planned) == 8
    plan = _model(rsets.build("schedule5")[0]).plan()
    assert not any(v and "cs_walk" in str(v) for v in plan.values())  # the plan dictionary is what it was
