"""GPU tests of the fixpoint under an incumbent and of the MIN / MAX trees it shapes, on the pairs and the recorded trees of
objective_sets.py.

The fixpoint: Model.propagate_obj (csgpu_propagate_batch_obj) and the device-read incumbent of the search engine's
device-driven iterations (csgpu_internal_propagate_objdev) by the general kernel and the clause-resident one, with the
linear fast paths on and off, against the oracle on every drawn instance -- verdict, every bound, the open count --, in
batches around the wave size and in one that takes the grid-stride loop round more than once; without a bound and on
models without an objective the plain batched fixpoint, field for field; a consistent output fed back under its bound
stays as it is.

The trees: every optimisation of every set of search_sets.py by the device-driven engine with 1 and with 64 parents per
iteration, by the general and by the clause-resident kernel, and on three sets by every way of driving the iterations:
nodes, cuts, solutions, iterations, pool peak and optimum of the recorded walk of the oracle-backed engine, and the best
row the first child in child order that attains the optimum.  Nothing here is compared with a number the device
produced."""
import functools
import json
import os

import numpy as np
import pytest

import objective_sets as O
import search_sets as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INT32_MAX, INT32_MIN = O.INT32_MAX, O.INT32_MIN
PAIR_IDS = [O.pair_id(p) for p in O.PAIRS]
ORACLE_SAMPLE = 4096
POOL, CHILDREN = 1 << 20, 1 << 16  # pool_room_limit never binds on these trees (at most 400 open states)


def _model(name, objective, fast_paths=True, kernel=None):
    from csolve_amd.solver import set_linear_fast_paths, solve_root
    try:
        set_linear_fast_paths(fast_paths)
        model = solve_root(S.text_of(name, objective))
    finally:
        set_linear_fast_paths(True)
    if kernel is not None:
        model.set_kernel(kernel)
    return model


@functools.lru_cache(maxsize=None)
def _instances(pair):
    """the drawn instances of a pair with the oracle's reference, computed once and left unchanged; `order` sorts the
    nodes by their bound, so that the nodes of one launch lie next to each other"""
    inst = O.instances(pair)
    groups = O.groups(inst["bounds"])
    inst["order"] = np.concatenate([idx for _, idx in groups])
    at, inst["launches"] = 0, []
    for bound, idx in groups:
        inst["launches"].append((bound, at, at + len(idx)))
        at += len(idx)
    return inst


@functools.lru_cache(maxsize=None)
def _reference_under(pair, bound):
    """the oracle's reference of every node of a pair under one bound"""
    inst = _instances(pair)
    return O.refer(inst, np.tile(np.array(bound, dtype=np.int64), (len(inst["nodes"]), 1)))


def _configurations(pair, fast_paths=(True, False)):
    """the runs of a pair: kernel 1 and, where the model qualifies, kernel 6, with the linear fast paths on and off
    -> (what, model); the device's root fixpoint is the oracle's, and its objective variable the oracle's"""
    inst = _instances(pair)
    for fast in fast_paths:
        model = _model(*pair, fast_paths=fast)
        assert (model.domains() == inst["model"].domains()).all(), "the device's root fixpoint is not the oracle's"
        assert model.objective_var == inst["obj"] and model.objective == (2 if inst["sense"] == 1 else 3)
        assert model.qualifies(6) == (pair[0] != "planted150")  # more than 512 clauses: kernel 1 only
        for kernel in (1, 6) if model.qualifies(6) else (1,):
            model.set_kernel(kernel)
            yield (O.pair_id(pair), "fast paths" if fast else "interpreter", kernel), model
        model.close()


def _device_read(model, d_states, d_nodes, best, sense, obj_lo=INT32_MIN, obj_hi=INT32_MAX):
    """csgpu_internal_propagate_objdev: the bound is cs_objective_bound(sense, [obj_lo, obj_hi], *d_best), read by the
    kernel when it starts"""
    from csolve_amd import _lib
    B, n = d_nodes.shape[0], model.n_vars
    d_best = torch.tensor([best], dtype=torch.int32, device="cuda")
    out = torch.empty((B, n, 2), dtype=torch.int32, device="cuda")
    res = torch.empty((B, 4), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load_library().csgpu_internal_propagate_objdev(
        model._h, d_states.data_ptr(), d_nodes.data_ptr(), out.data_ptr(), res.data_ptr(), B, None, obj_lo, obj_hi,
        d_best.data_ptr(), sense, None))
    torch.cuda.synchronize()  # d_best must outlive the launch
    return out, res


def _run(model, d_states, d_sorted, inst, device_read=False):
    """every instance under its own bound, one launch per bound -> (out, res) in the order of inst["nodes"];
    device_read: the one-sided bounds as an incumbent in device memory instead (cut + 1 under MIN, cut - 1 under MAX)"""
    outs, ress = [], []
    sense = inst["sense"]
    for (lo, hi), a, b in inst["launches"]:
        one_sided = (lo == INT32_MIN and hi < INT32_MAX) if sense == 1 else (hi == INT32_MAX and lo > INT32_MIN)
        if device_read and one_sided:
            out, res = _device_read(model, d_states, d_sorted[a:b], hi + 1 if sense == 1 else lo - 1, sense)
        else:
            out, res = model.propagate_obj(d_states, d_sorted[a:b], lo, hi)
        outs.append(out)
        ress.append(res)
    torch.cuda.synchronize()
    out, res = torch.cat(outs).cpu().numpy(), torch.cat(ress).cpu().numpy()
    back = np.empty_like(inst["order"])
    back[inst["order"]] = np.arange(len(back))
    return out[back], res[back]


def _check(what, nodes, out, res, status, exp, n_vars):
    """verdict, every bound of every consistent node, the open count: bit for bit"""
    fail = status < 0
    wrong = np.nonzero((res[:, 0] < 0) != fail)[0]
    assert len(wrong) == 0, (what, "verdicts", len(wrong), nodes[wrong[:4]].tolist())
    bad = np.nonzero(~fail & (out != exp).any((1, 2)))[0]
    assert len(bad) == 0, (what, "bounds", len(bad), nodes[bad[:4]].tolist(), out[bad[:1]].tolist(), exp[bad[:1]].tolist())
    assert (res[~fail, 0] == (exp[~fail, :, 0] != exp[~fail, :, 1]).sum(1)).all(), (what, "open counts")


def _report(pair, record):
    print("objective bound:", O.pair_id(pair), json.dumps(record))
    out_dir = os.environ.get("CSOLVE_REPORT_DIR")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "objective_bound_parity.json")
        everything = json.load(open(path)) if os.path.exists(path) else {}
        everything[O.pair_id(pair)] = record
        json.dump(everything, open(path, "w"), indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _runs(pair):
    """every drawn instance under its own bound by the four configurations, each checked against the reference and
    fed back -> {what: (out, res)}; run once per pair and shared"""
    inst = _instances(pair)
    nodes, status, exp = inst["nodes"], inst["status"], inst["out"]
    fail = status < 0
    d_states = torch.from_numpy(inst["states"]).cuda()
    d_sorted = torch.from_numpy(np.ascontiguousarray(nodes[inst["order"]])).cuda()
    runs = {}
    for what, model in _configurations(pair):
        out, res = _run(model, d_states, d_sorted, inst)
        _check(what, nodes, out, res, status, exp, model.n_vars)
        runs[what] = (out, res)
        # the fixpoint property under the bound: the device leaves its own consistent outputs alone
        d_out = torch.from_numpy(np.ascontiguousarray(out[inst["order"]])).cuda()
        fed = 0
        for (lo, hi), a, b in inst["launches"]:
            ok = np.nonzero(~fail[inst["order"][a:b]])[0]
            if len(ok) == 0:
                continue
            again = np.stack([np.full(len(ok), -1), np.zeros(len(ok)), np.zeros(len(ok)), a + ok], 1).astype(np.int32)
            out2, res2 = model.propagate_obj(d_out, torch.from_numpy(again).cuda(), lo, hi)
            assert torch.equal(out2, d_out[a:b][torch.from_numpy(ok).cuda()]), (what, (lo, hi))
            assert bool((res2[:, 0] >= 0).all()) and bool((res2[:, 1] == 0).all()), (what, (lo, hi))
            fed += len(ok)
        assert fed == int((~fail).sum())
    return runs


@pytest.mark.parametrize("pair", O.PAIRS, ids=PAIR_IDS)
def test_results_under_a_bound_equal_the_reference(pair):
    """every drawn instance under its own bound, by kernel 1 and kernel 6 with the fast paths on and off: the oracle's
    verdict, every bound of every consistent node and the open count, bit for bit; the four runs equal each other; a
    consistent output fed back as a var = -1 parent under the same bound comes back unchanged with zero propagations.
    No instance is left out."""
    inst = _instances(pair)
    assert O.class_counts(inst) == O.CLASS_COUNTS[pair]
    fail = inst["status"] < 0
    runs = _runs(pair)
    assert len(runs) == (2 if pair[0] == "planted150" else 4)
    first = next(iter(runs.values()))
    for what, (out, res) in runs.items():
        assert ((res[:, 0] < 0) == (first[1][:, 0] < 0)).all() and (out[~fail] == first[0][~fail]).all(), what
        assert (res[~fail, 0] == first[1][~fail, 0]).all(), what
    _report(pair, {"instances": len(inst["nodes"]), "runs": len(runs), "instances_compared": len(inst["nodes"]) * len(runs),
                   "left_out": 0, "bounds": len(inst["launches"]), "classes": O.class_counts(inst)})


@pytest.mark.parametrize("pair", O.PAIRS, ids=PAIR_IDS)
def test_a_failed_node_names_a_variable(pair):
    """res[:, 3] of every failed node of those runs is a variable, in [0, n_vars).
    Also where no interval is empty: a tree that fails at a constant terminal or in a product's PROP_ERROR (the stack of
    cs_tree_revise pops the constant side of `q * a` before `a`) names the first variable of that tree.  Before that
    these nodes reported -1: 284 of the 1,128 failed nodes of narrow_sums7 MIN C3, 932 of the 1,982 of wide3_sums
    MIN C1, 824 of the 1,451 of wide3_sums MAX 2*C1 + C3, on every pair that keeps tree clauses."""
    inst = _instances(pair)
    fail = inst["status"] < 0
    n = inst["states"].shape[1]
    unnamed = {}
    for what, (out, res) in _runs(pair).items():
        bad = fail & ~((res[:, 3] >= 0) & (res[:, 3] < n))
        unnamed[what[1:]] = (int(bad.sum()), sorted(set(res[bad, 3].tolist())),
                             {k: int((inst["klass"][bad] == k).sum()) for k in O.CLASSES if (inst["klass"][bad] == k).any()})
    print("failed nodes without a variable:", O.pair_id(pair), int(fail.sum()), "failed", unnamed)
    assert all(count == 0 for count, _, _ in unnamed.values()), unnamed


@pytest.mark.parametrize("pair", O.PAIRS, ids=PAIR_IDS)
def test_batch_sizes_under_one_bound(pair):
    """all instances of a pair under one bound, cut into batches of 1, 63, 64, 65 and the rest, by every kernel and fast-path
    setting against the reference; then multi_processor_count * 32 * 16 + 1 nodes with repeated instances, so that the
    grid-stride loop runs more than once: every node of it equal between kernel 1 and kernel 6, a seeded sample of 4,096
    against the reference"""
    inst = _instances(pair)
    bound = O.common_bound(inst)
    ref = _reference_under(pair, bound)
    nodes, status, exp = inst["nodes"], ref["status"], ref["out"]
    assert 0 < int((ref["klass"] == "unmoved").sum()) and 0 < int((ref["klass"] == "empty").sum())
    d_states = torch.from_numpy(inst["states"]).cuda()
    d_nodes = torch.from_numpy(nodes).cuda()
    rng = np.random.default_rng(7)
    n_big = torch.cuda.get_device_properties(0).multi_processor_count * 32 * 16 + 1
    pick = rng.integers(len(nodes), size=n_big)
    sample = np.sort(rng.choice(n_big, size=ORACLE_SAMPLE, replace=False))
    d_big = d_nodes[torch.from_numpy(pick).cuda()].contiguous()
    d_sample = torch.from_numpy(sample).cuda()
    big = {}
    for what, model in _configurations(pair):
        outs, ress, at = [], [], 0
        for B in O.BATCHES + (len(nodes) - sum(O.BATCHES),):
            out, res = model.propagate_obj(d_states, d_nodes[at:at + B], *bound)
            outs.append(out)
            ress.append(res)
            at += B
        assert at == len(nodes)
        torch.cuda.synchronize()
        _check(what, nodes, torch.cat(outs).cpu().numpy(), torch.cat(ress).cpu().numpy(), status, exp, model.n_vars)
        if what[1] == "fast paths":
            out, res = model.propagate_obj(d_states, d_big, *bound)
            torch.cuda.synchronize()
            _check(what + (n_big,), nodes[pick[sample]], out[d_sample].cpu().numpy(), res[d_sample].cpu().numpy(),
                   status[pick[sample]], exp[pick[sample]], model.n_vars)
            big[what[2]] = (out, res)
    if 6 in big:
        ok = big[1][1][:, 0] >= 0
        assert torch.equal(big[6][1][:, 0] >= 0, ok), "verdicts of kernel 1 and kernel 6 differ"
        assert torch.equal(big[6][0][ok], big[1][0][ok]) and torch.equal(big[6][1][ok][:, 0], big[1][1][ok][:, 0])
    else:
        assert pair[0] == "planted150"


@pytest.mark.parametrize("pair", O.PAIRS, ids=PAIR_IDS)
def test_no_bound_is_the_plain_fixpoint(pair):
    """propagate_obj(INT32_MIN, INT32_MAX) equals propagate field for field, PROPS, revisions and rounds included, under
    the automatic choice of the kernel and under each set kernel -- and the unbounded children are the oracle's"""
    inst = _instances(pair)
    ref = _reference_under(pair, O.NO_BOUND)
    d_states = torch.from_numpy(inst["states"]).cuda()
    d_nodes = torch.from_numpy(inst["nodes"]).cuda()
    model = _model(*pair)
    for kernel in (0, 1, 6) if model.qualifies(6) else (0, 1):
        model.set_kernel(kernel)
        out, res = model.propagate_obj(d_states, d_nodes, *O.NO_BOUND)
        out0, res0 = model.propagate(d_states, d_nodes)
        torch.cuda.synchronize()
        ok = res0[:, 0] >= 0
        assert torch.equal(res, res0) and torch.equal(out[ok], out0[ok]), (pair, kernel)
        _check((pair, kernel), inst["nodes"], out.cpu().numpy(), res.cpu().numpy(), ref["status"], ref["out"], model.n_vars)
    model.close()


def _walk_inputs(text, model, seed, count=600):
    from test_gpu_instantiations import _nodes, _oracle, _walk_states
    orc = _oracle(text, model)
    rng = np.random.default_rng(seed)
    states = _walk_states(orc, model.domains(), rng, count=24)
    return torch.from_numpy(states).cuda(), torch.from_numpy(_nodes(rng, states, count)).cuda()


@pytest.mark.parametrize("name", ["narrow_sums7", "planted80", "queens8"])
def test_a_model_without_an_objective_ignores_the_bounds(name):
    """the ALL text of a set, and queens-8 (its own choice of kernel and kernel 7): any bounds, crossed ones included, change nothing, through
    propagate_obj and through the device-read incumbent"""
    from csolve_amd import problems
    from csolve_amd.solver import solve_root
    text = problems.queens(8) if name == "queens8" else S.text_of(name)
    model = solve_root(text)
    assert model.objective_var < 0
    d_states, d_nodes = _walk_inputs(text, model, 11)
    # queens-8 is a pure != network: the forbidden-set kernels and the shaving kernel, which take no bound at all
    kernels = [0] + ([7] if model.qualifies(7) else [])
    assert name != "queens8" or (model.kernel() in (5, 7) and 7 in kernels)
    for kernel in kernels:
        model.set_kernel(kernel)
        out0, res0 = model.propagate(d_states, d_nodes)
        torch.cuda.synchronize()
        ok = res0[:, 0] >= 0
        assert bool(ok.any()) and not bool(ok.all())
        for lo, hi in ((3, 2), (-1, 1), (5, INT32_MAX), (INT32_MIN, -7), (INT32_MAX, INT32_MIN)):
            out, res = model.propagate_obj(d_states, d_nodes, lo, hi)
            torch.cuda.synchronize()
            assert torch.equal(res, res0) and torch.equal(out[ok], out0[ok]), (name, kernel, lo, hi)
        for sense, best in ((1, 0), (2, 0), (1, INT32_MIN), (2, INT32_MAX)):
            out, res = _device_read(model, d_states, d_nodes, best, sense)
            assert torch.equal(res, res0) and torch.equal(out[ok], out0[ok]), (name, kernel, sense, best)
    model.close()


@pytest.mark.parametrize("pair", O.PAIRS, ids=PAIR_IDS)
def test_the_device_read_incumbent_equals_the_hosts_two_ints(pair):
    """the incumbent in a one-element device tensor (what enqueue_burst passes) against the bound as two ints (what
    one_iteration passes), on the whole instance set, equal outputs and results field for field: every drawn cut as the
    incumbent cut + 1 (MIN) or cut - 1 (MAX), and for sense 1 and sense 2 the "none yet" sentinels and both root
    extremes of "<obj>", where the host's ints are the Python statement of cs_objective_bound -- those runs against the
    oracle as well"""
    inst = _instances(pair)
    nodes, obj = inst["nodes"], inst["obj"]
    root_lo, root_hi = (int(x) for x in inst["model"].domains()[obj])
    d_states = torch.from_numpy(inst["states"]).cuda()
    d_nodes = torch.from_numpy(nodes).cuda()
    d_sorted = torch.from_numpy(np.ascontiguousarray(nodes[inst["order"]])).cuda()
    for what, model in _configurations(pair):
        out_h, res_h = _run(model, d_states, d_sorted, inst)
        out_d, res_d = _run(model, d_states, d_sorted, inst, device_read=True)
        ok = res_h[:, 0] >= 0
        assert (res_d == res_h).all() and (out_d[ok] == out_h[ok]).all(), what
        _check(what, nodes, out_d, res_d, inst["status"], inst["out"], model.n_vars)
        for sense in (1, 2):
            for best in (INT32_MAX if sense == 1 else INT32_MIN, root_lo, root_hi):
                bound = O.objective_bound(sense, *O.NO_BOUND, best)
                assert (bound == O.NO_BOUND) == (best in (INT32_MAX, INT32_MIN))
                out_h, res_h = model.propagate_obj(d_states, d_nodes, *bound)
                out_d, res_d = _device_read(model, d_states, d_nodes, best, sense)
                ok = res_h[:, 0] >= 0
                assert torch.equal(res_d, res_h) and torch.equal(out_d[ok], out_h[ok]), (what, sense, best)
                ref = _reference_under(pair, bound)
                _check(what + (sense, best), nodes, out_d.cpu().numpy(), res_d.cpu().numpy(), ref["status"], ref["out"],
                       model.n_vars)


# ---- the MIN / MAX trees ----

SWITCHES = ("CSGPU_SEARCH_GRAPH", "CSGPU_SEARCH_BURST", "CSGPU_SEARCH_BURST_SPLIT", "CSGPU_SEARCH_EVAL")
MODES = {"launches": {"CSGPU_SEARCH_GRAPH": "0"}, "one-workgroup": {"CSGPU_SEARCH_BURST_SPLIT": "0"},
         "evaluated": {"CSGPU_SEARCH_EVAL": "1"}, "host": {"CSGPU_SEARCH_BURST": "0"}}


@functools.lru_cache(maxsize=None)
def _engine(name, which, parents, lag=0):
    """the oracle-backed engine's walk -- the recorded one -- and its best row"""
    tree, eng = O.engine_tree(name, O.objective_text(name, which), parents, lag=lag)
    assert tree == (O.LAGGED_TREES if lag else O.TREES)[name, which, parents]
    return tree, None if eng.best_row is None else eng.best_row.copy(), eng.m.names()


def _walk(model, name, which, parents, what, lag=0):
    """one search to its end in one run: the recorded tree and the first child in child order that attains the optimum"""
    from csolve_amd.solver import Search
    tree, best_row, names = _engine(name, which, parents, lag)
    s = Search(model, POOL, CHILDREN)
    s.set_parents(parents)
    s.put(model.root_state())
    st = s.run()
    assert st["done"] == 1 and st["pool"] == 0
    got = tuple(int(st[k]) for k in ("nodes", "cuts", "solutions", "iterations", "pool_peak", "best"))
    print(name, which, parents, what, got)
    assert got == tree, (name, which, parents, what, got, tree)
    row = s.best_solution()
    assert model.var_names() == names
    assert (row is None) == (best_row is None) and (row is None or (row == best_row).all()), (name, which, parents, what)
    s.close()


@pytest.mark.parametrize("name", list(S.SETS))
def test_device_driven_trees_are_the_recorded_ones(name, monkeypatch):
    """every optimisation of a set, 1 and 64 parents per iteration, by the engine's own choice of the fixpoint kernel, by
    kernel 1 and, where the model qualifies, by kernel 6: nodes, cuts, solutions, iterations, pool peak and optimum of
    the recorded walk, in which an iteration sees every solution of the iterations before it.  A fixpoint that ignores
    the incumbent, applies it an iteration late or leaves "<obj>" unmarked walks a larger tree."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for which in O.OBJECTIVES:
        model = _model(name, O.objective_text(name, which))
        for kernel in (0, 1, 6) if model.qualifies(6) else (0, 1):
            model.set_kernel(kernel)
            for parents in O.PARENTS:
                _walk(model, name, which, parents, f"kernel {kernel}")
        model.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", O.LAGGED_SETS)
def test_every_way_of_driving_the_iterations_walks_its_recorded_tree(name, mode, monkeypatch):
    """the same launches one by one instead of one hipGraph per burst, the bookkeeping by one workgroup and every complete
    child evaluated walk the device-driven tree; the host-driven loop (CSGPU_SEARCH_BURST=0) reads an accept's results
    after the next iteration's fixpoints are launched, a fixed lag of one iteration, and walks the tree recorded for it"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    for which in O.OBJECTIVES:
        model = _model(name, O.objective_text(name, which))
        for parents in O.PARENTS:
            _walk(model, name, which, parents, mode, lag=1 if mode == "host" else 0)
        model.close()
