"""GPU tests of Model.solve_many_clauses (csgpu_solve_many_clauses, cs_walk_clauses): every instance of every set of
tests/many_clause_sets.py against the oracle walk of tests/many_walk_objective.py, field for field; props against the
same walk stepped through kernel 6 itself; budgets, sentinels, large batches, queued calls, root rows that are not
searched, the objective checks, the limits, and the corroboration by solve_many and by a Search."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import many_clause_sets as sets
import many_walk
import many_walk_objective as W
from csolve_amd import problems
from csolve_amd._lib import CsolveError, ManyOptions, load_library
from csolve_amd.solver import Search, solve_root

pytestmark = pytest.mark.gpu

E_ARG, E_LIMIT = -1, -4
SENTINEL = -77
INT_FIELDS = ("status", "nodes", "cuts", "solutions")


@functools.lru_cache(maxsize=None)
def model_of(text):
    return solve_root(text)


def host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v)}


@functools.lru_cache(maxsize=None)
def answered(name):
    """the device's answer for a set at its budget (computed once, not to be changed)"""
    text, roots, objective, budget = sets.build(name)
    return host(model_of(text).solve_many_clauses(np.array(roots), objective, max_nodes=budget))


def same_answers(got, want, objective, where=None):
    """status, nodes, cuts, solutions, best and the stored row of every instance"""
    for f in INT_FIELDS:
        assert (got[f] == want[f]).all(), (f, where, np.nonzero(got[f] != want[f])[0][:8], got[f][:8], want[f][:8])
    has = want["solutions"] > 0
    assert (got["first"][has] == want["first"][has]).all(), where
    assert (got["first"][~has] == 0).all(), where
    if objective in ("MIN", "MAX"):
        assert (got["best"][has] == want["best"][has]).all(), where
    else:
        assert "best" not in got


@pytest.mark.parametrize("name", sorted(sets.SETS))
def test_every_instance_equals_the_walk(name):
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    assert (model.domains() == W.oracle_for(text)[1]).all()  # the rows lie in the device tables' root domains
    assert model.qualifies_many_clauses() and model.many_clauses_kernel() == sets.SETS[name][3]
    assert "walk" not in " ".join(str(v) for v in model.plan().values())
    want = sets.walked(name)
    got = answered(name)
    same_answers(got, want, objective, name)
    if name in sets.WHOLE:
        assert (got["status"] == W.DONE).all() and got["nodes"].max() < budget
    else:  # a LIMIT instance stops at exactly max_nodes, whatever it has found
        limit = got["status"] == W.LIMIT
        assert limit.any() and (got["nodes"][limit] == budget).all() and (got["nodes"][~limit] < budget).all()


def test_the_sets_plan_every_shipped_instantiation():
    from test_solve_many_clauses_host import shipped_walk_kernels
    planned = {model_of(sets.build(name)[0]).many_clauses_kernel() for name in sets.SETS}
    assert planned == shipped_walk_kernels()


class Stepped(W.Walk):
    """the walk with every node through Model.propagate on kernel 6, one node per call: kernel 6's own props"""

    def __init__(self, model, text, row, objective):
        self.model = model
        super().__init__(text, row, objective)

    class _Six:
        def __init__(self, model):
            self.model = model

        def instance(self, state, v, lo, hi):
            st = torch.from_numpy(np.array(state, dtype=np.int32)[None]).cuda()
            node = torch.tensor([[v, lo, hi, 0]], dtype=torch.int32, device="cuda")
            out, res = self.model.propagate(st, node)
            res = res.cpu().numpy()[0]
            return (-1, None) if res[0] < 0 else (int(res[1]), out.cpu().numpy()[0])

    @property
    def orc(self):
        return self._Six(self.model)

    @orc.setter
    def orc(self, _):
        pass


@pytest.mark.parametrize("name", sorted(sets.SETS))
def test_props_are_kernel_6s(name):
    """props and root_props of up to four instances of at most 200 nodes: the same walk, each node one launch of kernel 6"""
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    got, want = answered(name), sets.walked(name)
    picked = [i for i in np.argsort(-want["nodes"], kind="stable") if 0 < want["nodes"][i] <= 200][:4]
    assert picked
    model.set_kernel(6)
    try:
        for i in picked:
            ref = Stepped(model, text, roots[i], objective).run(budget)
            for f in INT_FIELDS + ("props", "root_props"):
                assert got[f][i] == ref[f], (f, i, got[f][i], ref[f])
            print(f"{name}[{i}]: nodes {ref['nodes']} props {ref['props']} (oracle {want['props'][i]}) "
                  f"root_props {ref['root_props']} (oracle {want['root_props'][i]})")
    finally:
        model.set_kernel(0)


def _call(model, roots, objective, budget, rows, best, stream=None):
    """the library itself, on buffers of the test's own"""
    K = roots.shape[0]
    res = torch.zeros((K, 5), dtype=torch.int64, device="cuda")
    opt = ManyOptions(W.CODE[objective], 0, budget)
    rc = load_library().csgpu_solve_many_clauses(model._h, roots.data_ptr(), K, C.byref(opt), res.data_ptr(),
                                                 rows.data_ptr() if rows is not None else None,
                                                 best.data_ptr() if best is not None else None, stream)
    assert rc == 0, load_library().csgpu_last_error()
    return res


@pytest.mark.parametrize("name", sets.BUDGET)
def test_rows_without_a_solution_keep_what_they_held(name):
    text, roots, objective, budget = sets.build(name)
    model, want = model_of(text), sets.walked(name)
    # a smaller budget as well, so that some instances stop before their first solution
    for b, ref in ((budget, want), (3, W.walk_many(text, roots, objective, 3))):
        dev = torch.from_numpy(np.array(roots)).cuda()
        rows = torch.full((len(roots), model.n_vars), SENTINEL, dtype=torch.int32, device="cuda")
        best = torch.full((len(roots),), SENTINEL, dtype=torch.int32, device="cuda")
        res = _call(model, dev, objective, b, rows, best)
        torch.cuda.synchronize()
        rows, best, res = rows.cpu().numpy(), best.cpu().numpy(), res.cpu().numpy()
        none = ref["solutions"] == 0
        assert (res[:, 4] == ref["solutions"]).all() and (res[:, 1] == ref["nodes"]).all()
        assert (rows[none] == SENTINEL).all() and (best[none] == SENTINEL).all()
        assert (rows[~none] == ref["first"][~none]).all() and (best[~none] == ref["best"][~none]).all()
        if b == 3:
            assert none.any() and (ref["status"] == W.LIMIT).any()
    # ANY / ALL never write d_best
    dev = torch.from_numpy(np.array(roots)).cuda()
    best = torch.full((len(roots),), SENTINEL, dtype=torch.int32, device="cuda")
    _call(model, dev, "ANY", budget, None, best)
    torch.cuda.synchronize()
    assert (best.cpu().numpy() == SENTINEL).all()


def test_large_batches_queued_calls_halves_and_a_permutation():
    name = "schedule5_min"
    text, roots, objective, budget = sets.build(name)
    model, want = model_of(text), sets.walked(name)
    K = len(roots)
    resident = model.many_clauses_waves(1 << 30)
    assert resident >= 64 and model.many_clauses_waves(3) == 4 and model.many_clauses_waves(0) == 0
    reps = -(-4 * resident // K)
    big = torch.from_numpy(np.tile(np.array(roots), (reps, 1, 1))).cuda()
    assert big.shape[0] >= 4 * resident
    got = host(model.solve_many_clauses(big, objective, max_nodes=budget))
    for f in INT_FIELDS + ("props", "root_props", "best"):
        assert (got[f].reshape(reps, K) == answered(name)[f][None]).all(), f
    assert (got["first"].reshape(reps, K, -1) == answered(name)["first"][None]).all()
    same_answers({f: v[:K] for f, v in got.items()}, want, objective)
    # two calls queued on one stream, no host in between: the tickets are back at zero, the workspace is shared
    dev = torch.from_numpy(np.array(roots)).cuda()
    perm = np.random.default_rng(5).permutation(K)
    shuffled = torch.from_numpy(np.array(roots)[perm]).cuda()
    a = model.solve_many_clauses(dev, objective, max_nodes=budget)
    b = model.solve_many_clauses(shuffled, objective, max_nodes=budget)
    c = model.solve_many_clauses(dev[: K // 2].contiguous(), objective, max_nodes=budget)
    d = model.solve_many_clauses(dev[K // 2:].contiguous(), objective, max_nodes=budget)
    a, b, c, d = host(a), host(b), host(c), host(d)
    for f in INT_FIELDS + ("props", "root_props", "best", "first"):
        assert (a[f] == answered(name)[f]).all(), f
        assert (b[f] == answered(name)[f][perm]).all(), f
        assert (np.concatenate([c[f], d[f]]) == answered(name)[f]).all(), f
    # an empty batch launches nothing
    empty = host(model.solve_many_clauses(np.zeros((0, model.n_vars, 2), dtype=np.int32), objective, max_nodes=5))
    assert empty["status"].shape == (0,) and empty["best"].shape == (0,)


def test_root_rows_that_are_not_searched():
    text, roots, objective, budget = sets.build("schedule5_min")
    model = model_of(text)
    _, dom = W.oracle_for(text)
    solved = sets.walked("schedule5_min")["first"][0]
    rows = np.repeat(dom[None], 6, 0).astype(np.int32)
    rows[0, 3, 1] = dom[3, 1] + 1                      # outside the root domains
    rows[1, 2] = (dom[2, 0] + 1, dom[2, 0])            # lo > hi
    rows[2] = np.stack([solved, solved], 1)            # a solution already
    starts = [i for i, s in enumerate(model.var_names()) if s.endswith("_start")]
    rows[3, starts[0]] = rows[3, starts[1]] = max(dom[starts[0], 0], dom[starts[1], 0])  # two tasks at one time: inconsistent at the root
    rows[4] = roots[0]
    rows[5, 0, 0] = dom[0, 0] - 1                      # below the root domains
    got = host(model.solve_many_clauses(rows, objective, max_nodes=budget))
    want = W.walk_many(text, rows, objective, budget)
    assert want["status"].tolist() == [W.BAD_ROOT, W.BAD_ROOT, W.DONE, W.DONE, W.DONE, W.BAD_ROOT]
    assert want["nodes"][:4].tolist() == [0, 0, 0, 0] and want["solutions"][:4].tolist() == [0, 0, 1, 0]
    same_answers(got, want, objective)
    assert got["best"][2] == solved[model.objective_var] and (got["first"][2] == solved).all()
    assert (got["root_props"][[0, 1, 3, 5]] == 0).all() and (got["props"][[0, 1, 2, 3, 5]] == 0).all()


@pytest.mark.parametrize("objective", ["ANY", "ALL"])
def test_a_min_model_under_any_and_all_branches_on_the_objective_variable(objective):
    text, roots, _, _ = sets.build("schedule5_min")
    model = model_of(text)
    want = W.walk_many(text, roots[:12], objective, 500)
    got = host(model.solve_many_clauses(np.array(roots[:12]), objective, max_nodes=500))
    same_answers(got, want, objective)
    assert (want["solutions"] > 0).any()
    if objective == "ALL":  # "<obj>" is enumerated like every variable: more solutions than improving ones
        assert (want["solutions"] > sets.walked("schedule5_min")["solutions"][:12]).any()


def test_the_objective_must_be_the_models_own():
    text, roots, _, _ = sets.build("schedule5_min")  # MIN
    model = model_of(text)
    dev = torch.from_numpy(np.array(roots)).cuda()
    for rows in (dev, np.array(roots)):
        with pytest.raises(CsolveError) as e:
            model.solve_many_clauses(rows, "MAX", max_nodes=10)
        assert e.value.code == E_ARG
    text, roots, _, _ = sets.build("linear12_any")  # no objective variable
    model = model_of(text)
    for objective in ("MIN", "MAX"):
        with pytest.raises(CsolveError) as e:
            model.solve_many_clauses(torch.from_numpy(np.array(roots)).cuda(), objective, max_nodes=10)
        assert e.value.code == E_ARG and "objective" in str(e.value)
    text, roots, _, _ = sets.build("wcet_max")  # MAX
    with pytest.raises(CsolveError) as e:
        model_of(text).solve_many_clauses(np.array(roots), "MIN", max_nodes=10)
    assert e.value.code == E_ARG


def test_more_than_512_clauses_is_a_limit():
    text = problems.schedule(32, 1)
    model = model_of(text)
    assert model.n_clauses > 512 and not model.qualifies(6)
    assert not model.qualifies_many_clauses() and model.many_clauses_kernel() is None and model.many_clauses_waves(8) == 0
    rows = np.repeat(model.domains()[None], 2, 0)
    for r in (rows, torch.from_numpy(rows).cuda()):
        with pytest.raises(CsolveError) as e:
            model.solve_many_clauses(r, "MIN", max_nodes=10)
        assert e.value.code == E_LIMIT and "512" in str(e.value)


@pytest.mark.parametrize("objective", ["ANY", "ALL"])
def test_a_kernel_7_model_gives_the_answers_of_solve_many(objective):
    import many_sets
    text = problems.queens(8, "ALL")
    model = model_of(text)
    assert model.qualifies(7) and model.qualifies(6) and model.many_clauses_kernel().startswith("cs_walk_clauses<")
    rows = np.concatenate([model.domains()[None], many_sets.queens_two(8, 23, 3)]).astype(np.int32)
    a = host(model.solve_many(rows, objective, max_nodes=1 << 14))
    b = host(model.solve_many_clauses(rows, objective, max_nodes=1 << 14))
    c = host(model.solve_many(rows, objective, max_nodes=1 << 14))  # and the shared workspace serves both, in turn
    for f in INT_FIELDS + ("first",):
        assert (a[f] == b[f]).all() and (a[f] == c[f]).all(), f
    assert a["solutions"][0] == (92 if objective == "ALL" else 1)
    want = many_walk.dive_many(text, rows, objective, 1 << 14)
    for f in INT_FIELDS:
        assert (b[f] == want[f]).all(), f


def test_a_search_reaches_the_same_optimum():
    """corroboration on three instances: the engine, seeded with the instance's root fixpoint, proves the same optimum"""
    name = "schedule5_min"
    text, roots, objective, budget = sets.build(name)
    model, got = model_of(text), answered(name)
    picked = [int(i) for i in np.argsort(-got["nodes"], kind="stable")[:3]]
    for i in picked:
        assert got["status"][i] == W.DONE and got["solutions"][i] > 0
        state = torch.from_numpy(np.array(roots[i])[None]).cuda()
        fix, res = model.propagate(state, torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32, device="cuda"))
        assert int(res[0, 0]) >= 0
        search = Search(model)
        search.put(fix.contiguous())
        st = search.run()
        assert st["done"] == 1 and st["best"] == got["best"][i], (i, st["best"], got["best"][i])
        row = search.best_solution()
        assert row is not None and row[model.objective_var] == got["best"][i]
        search.close()
