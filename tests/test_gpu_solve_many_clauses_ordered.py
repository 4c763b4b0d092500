"""GPU tests of Model.solve_many_clauses_ordered (csgpu_solve_many_clauses_ordered, cs_walk_order): the recorded ALL trees
of order_walk under every order; the plain call's answers where nothing halves, props bit for bit; the row sets of
tests/many_walk_ordered.py against its host walk; root rows that are not searched, an empty batch, the frame count, the
argument errors and pure bisection; the eight instantiations."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import many_clause_sets as sets
import many_walk_objective as W
import many_walk_ordered as O
import order_walk
from csolve_amd._lib import CsolveError, ManyOrderOptions, load_library
from csolve_amd.solver import solve_root

pytestmark = pytest.mark.gpu

E_ARG, E_LIMIT = -1, -4
INT_FIELDS = ("status", "nodes", "cuts", "solutions", "halvings")


@functools.lru_cache(maxsize=None)
def model_of(text):
    return solve_root(text)


def host(out):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in out.items() if torch.is_tensor(v)}


def same_answers(got, want, objective, where=None):
    """status, nodes, cuts, solutions, halvings, best and the stored row of every instance"""
    for f in INT_FIELDS:
        assert (got[f] == want[f]).all(), (f, where, np.nonzero(got[f] != want[f])[0][:8], got[f][:8], want[f][:8])
    has = want["solutions"] > 0
    assert (got["first"][has] == want["first"][has]).all(), where
    assert (got["first"][~has] == 0).all(), where
    if objective in ("MIN", "MAX"):
        assert (got["best"][has] == want["best"][has]).all(), where
    else:
        assert "best" not in got


@pytest.mark.parametrize("name", O.RECORDED_SETS)
def test_all_trees_are_the_recorded_ones(name):
    """three copies of the root-domain row under ALL, every recorded order: DONE and the recorded tree on each copy"""
    text = order_walk.text_of(name)
    model = model_of(text)
    assert model.qualifies_many_clauses()
    assert (model.domains() == W.oracle_for(text)[1]).all()
    rows = np.repeat(O.root_row(text), 3, 0)
    for order in order_walk.orders_of(name):
        got = host(model.solve_many_clauses_ordered(rows, "ALL", max_nodes=order_walk.CAP + 1, order=order,
                                                    split_width=order_walk.SPLIT_WIDTH))
        want = order_walk.RECORDED[name, order]
        for i in range(3):
            assert got["status"][i] == O.DONE, (order, i)
            assert (got["nodes"][i], got["cuts"][i], got["solutions"][i], got["halvings"][i]) == want, (order, i)


def test_more_than_512_clauses_is_a_limit():
    text = order_walk.text_of("planted150")
    model = model_of(text)
    assert not model.qualifies_many_clauses() and model.many_clauses_order_kernel() is None
    assert model.many_clauses_ordered_frames(256) == 0
    rows = O.root_row(text)
    for r in (rows, torch.from_numpy(rows).cuda()):
        with pytest.raises(CsolveError) as e:
            model.solve_many_clauses_ordered(r, "ALL", max_nodes=10, order="largest-value")
        assert e.value.code == E_LIMIT and "512" in str(e.value)


@pytest.mark.parametrize("name", sorted(sets.SETS))
def test_nothing_changes_where_nothing_halves(name):
    """smallest-domain and a split_width no narrower than the widest interval of the rows: the plain call's answer, props
    included -- both kernels run the same rounds"""
    text, roots, objective, budget = sets.build(name)
    model = model_of(text)
    widest = int((roots[:, :, 1].astype(np.int64) - roots[:, :, 0] + 1).max())
    plain = host(model.solve_many_clauses(np.array(roots), objective, max_nodes=budget))
    got = host(model.solve_many_clauses_ordered(np.array(roots), objective, max_nodes=budget, order="smallest-domain",
                                                split_width=widest))
    assert set(got) == set(plain) | {"halvings"}
    for f in plain:
        assert (got[f] == plain[f]).all(), f
    assert (got["halvings"] == 0).all()
    assert model.many_clauses_order_kernel() == sets.SETS[name][3].replace("cs_walk_clauses", "cs_walk_order")


def test_the_sets_plan_every_shipped_instantiation():
    from test_solve_many_clauses_ordered_host import shipped_order_kernels
    planned = {model_of(sets.build(name)[0]).many_clauses_order_kernel() for name in sets.SETS}
    assert planned == shipped_order_kernels() and len(planned) == 8


@pytest.mark.parametrize("name,order,split", O.CASES)
def test_every_instance_equals_the_walk(name, order, split):
    text, roots, objective, budget = O.build(name)
    model = model_of(text)
    assert (model.domains() == W.oracle_for(text)[1]).all()  # the rows lie in the device tables' root domains
    want = O.walked(name, order, split)
    got = host(model.solve_many_clauses_ordered(np.array(roots), objective, max_nodes=budget, order=order, split_width=split))
    same_answers(got, want, objective, (name, order, split))
    if not O.SETS[name][4]:  # a LIMIT instance stops at exactly max_nodes, whatever it has found
        limit = got["status"] == O.LIMIT
        assert limit.any() and (got["nodes"][limit] == budget).all()
    assert want["deepest"].max() + 1 <= model.many_clauses_ordered_frames(split)


class Stepped(O.Walk):
    """the walk with every node through Model.propagate on kernel 6, one node per call: kernel 6's own props"""

    def __init__(self, model, *args):
        self.model = model
        super().__init__(*args)

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


def test_props_are_kernel_6s_where_intervals_are_halved():
    """props and root_props of three open-`end` rows, halves included: the same walk, each node one launch of kernel 6"""
    text, roots, objective, budget = O.build("schedule5_open_min")
    model = model_of(text)
    got = host(model.solve_many_clauses_ordered(np.array(roots), objective, max_nodes=budget, order="none", split_width=4))
    model.set_kernel(6)
    try:
        for i in range(3):
            ref = Stepped(model, text, roots[i], objective, "none", 4).run(budget)
            for f in INT_FIELDS + ("props", "root_props"):
                assert got[f][i] == ref[f], (f, i, got[f][i], ref[f])
    finally:
        model.set_kernel(0)


def test_root_rows_that_are_not_searched():
    text, roots, objective, budget = O.build("schedule5_open_min")
    model = model_of(text)
    _, dom = W.oracle_for(text)
    solved = O.walked("schedule5_open_min", "none", 4)["first"][0]
    rows = np.repeat(dom[None], 7, 0).astype(np.int32)
    rows[0] = roots[0]
    rows[1, 3, 0] = dom[3, 0] - 1                      # outside the root domains
    rows[2] = roots[1]
    rows[3] = np.stack([solved, solved], 1)            # a solution already
    starts = [i for i, s in enumerate(model.var_names()) if s.endswith("_start")]
    rows[4, starts[0]] = rows[4, starts[1]] = max(dom[starts[0], 0], dom[starts[1], 0])  # two tasks at one time: inconsistent at the root
    rows[5, 2] = (dom[2, 0] + 1, dom[2, 0])            # lo > hi
    rows[6] = roots[2]
    got = host(model.solve_many_clauses_ordered(rows, objective, max_nodes=budget, order="none", split_width=4))
    want = O.walk_many(text, rows, objective, budget, "none", 4)
    assert want["status"].tolist() == [O.DONE, O.BAD_ROOT, O.DONE, O.DONE, O.DONE, O.BAD_ROOT, O.DONE]
    assert want["nodes"][[1, 3, 4, 5]].tolist() == [0, 0, 0, 0] and want["solutions"][[1, 3, 4, 5]].tolist() == [0, 1, 0, 0]
    assert (want["nodes"][[0, 2, 6]] > 0).all()
    same_answers(got, want, objective)
    assert got["best"][3] == solved[model.objective_var] and (got["first"][3] == solved).all()
    assert (got["root_props"][[1, 4, 5]] == 0).all() and (got["props"][[1, 3, 4, 5]] == 0).all()


def test_an_empty_batch_the_frames_and_the_argument_errors():
    text, roots, objective, budget = O.build("schedule5_open_min")
    model = model_of(text)
    n = model.n_vars
    empty = host(model.solve_many_clauses_ordered(np.zeros((0, n, 2), dtype=np.int32), objective, max_nodes=5))
    assert empty["status"].shape == (0,) and empty["best"].shape == (0,) and empty["halvings"].shape == (0,)
    dom = model.domains()
    for split in (1, 2, 4, 16, 256, 2**31 - 1):
        assert model.many_clauses_ordered_frames(split) == O.frames(dom, split), split
    assert model.many_clauses_ordered_frames(0) == O.frames(dom, 256) and model.many_clauses_ordered_frames(-1) == 0
    assert model.many_clauses_ordered_frames(2**31 - 1) == n < model.many_clauses_ordered_frames(256)
    # the new errors: before anything is launched -- the sentinels in the result records stay, on host and device rows
    L = load_library()
    dev = torch.from_numpy(np.array(roots)).cuda()
    res = torch.full((len(roots), 5), -77, dtype=torch.int64, device="cuda")
    for opt in (ManyOrderOptions(2, 5, 256, 0, 100), ManyOrderOptions(2, -1, 256, 0, 100), ManyOrderOptions(2, 1, -4, 0, 100),
                ManyOrderOptions(2, 1, 256, 7, 100)):
        rc = L.csgpu_solve_many_clauses_ordered(model._h, dev.data_ptr(), len(roots), C.byref(opt), res.data_ptr(), None, None,
                                                None, None)
        assert rc == E_ARG and L.csgpu_last_error(), (opt.order, opt.split_width, opt.reserved)
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == -77).all()
    for kw in (dict(order=5), dict(split_width=-1)):
        for r in (dev, np.array(roots)):
            with pytest.raises(CsolveError) as e:
                model.solve_many_clauses_ordered(r, objective, max_nodes=10, **kw)
            assert e.value.code == E_ARG
    # split_width 0 is the engine's 256
    a = host(model.solve_many_clauses_ordered(dev, objective, max_nodes=budget, order="largest-value", split_width=0))
    same_answers(a, O.walked("schedule5_open_min", "largest-value", 256), objective)


@pytest.mark.parametrize("order", ["smallest-domain", "largest-value"])
def test_pure_bisection(order):
    """split_width 1: every open interval is halved down to a value"""
    text = order_walk.text_of("wide2_cut")
    model = model_of(text)
    rows = O.root_row(text)
    want = O.walk_many(text, rows, "ALL", order_walk.CAP, order, 1)
    # every node has two children, so 260 solutions need at least 259 parents; the stack outgrows the n frames of the plain walk
    assert want["status"][0] == O.DONE and want["halvings"][0] >= 259 and want["deepest"][0] + 1 > model.n_vars
    got = host(model.solve_many_clauses_ordered(rows, "ALL", max_nodes=order_walk.CAP, order=order, split_width=1))
    same_answers(got, want, "ALL", order)
    assert got["solutions"][0] == 260
