"""GPU tests of the expression-tree interpreter inside the batched fixpoint kernels, on the mixed-operator sets of
tree_sets.py (products of variables, a variable twice in a tree, NEG over a subexpression, `=` / `!=` between sums,
three-literal disjunctions, AND / OR / NOT below the top, saturating products, sums of 127 variables): kernel 1 and
kernel 6, with the linear fast paths on and off, against the oracle on the recorded instances -- and, independent of
that equality, every consistent device output is a fixpoint (the device and the oracle both leave it alone) that
contains the brute force's solutions below its node; the single-node paths with their trails, whose clause must mention
the narrowed variable anywhere in its tree; clause and root evaluation against the predicates; the search engine
against the brute force.  test_tree_sets_host.py checks on the CPU that no instance here can take more propagations
than its set's total width (at most 4,096), so nothing here can run long."""
import functools
import json
import os

import numpy as np
import pytest

import search_sets as S
import tree_sets as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K6_SETS = [n for n in T.NAMES if n != "bigtab"]  # 4,801 clauses are beyond kernel 6's 512
SINGLE = 100  # nodes per small set through the single-node paths


def _model(name, fast_paths=True, kernel=None):
    from csolve_amd.solver import set_linear_fast_paths, solve_root
    try:
        set_linear_fast_paths(fast_paths)
        model = solve_root(T.text_of(name))
    finally:
        set_linear_fast_paths(True)
    if kernel is not None:
        model.set_kernel(kernel)
    return model


@functools.lru_cache(maxsize=None)
def _instances(name):
    """the recorded instances: the oracle's walks from ITS root fixpoint, which the device's root phase must have
    reached as well"""
    return T.instances(name)


@functools.lru_cache(maxsize=None)
def _solutions(name):
    return T.solution_rows(name, _instances(name)["columns"])


def _run(model, d_states, nodes):
    """the recorded nodes in their batches of 1, 63, 64, 65 and 2,000 -> (states_out, results) of all of them"""
    outs, ress, at = [], [], 0
    for B in T.BATCHES:
        out, res = model.propagate(d_states, torch.from_numpy(nodes[at:at + B]).cuda())
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
        ress.append(res.cpu().numpy())
        at += B
    assert at == len(nodes)
    return np.concatenate(outs), np.concatenate(ress)


def _report(name, record):
    print("tree sets:", name, json.dumps(record))
    out_dir = os.environ.get("CSOLVE_REPORT_DIR")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "tree_sets_parity.json")
        everything = json.load(open(path)) if os.path.exists(path) else {}
        everything[name] = record
        json.dump(everything, open(path, "w"), indent=1, sort_keys=True)


@pytest.mark.parametrize("name", T.NAMES)
def test_batched_fixpoint_and_fixpoint_property(name):
    """kernel 1 and, where the model fits, kernel 6, each with the linear fast paths on and off, on every recorded
    instance: the oracle's verdict, every bound, the open count (PROPS is the kernels' own on tree models, but never more
    than the set's total width); the four runs equal each other exactly; every consistent output, fed back as a parent
    of a var = -1 node, comes back unchanged with zero propagations, and the oracle's full re-propagation leaves it alone
    too; on the brute-forced sets a consistent output holds every solution below its node and a failed node has none.
    No instance is left out of any of it."""
    inst = _instances(name)
    rec = T.RECORDED[name]
    states, nodes, status, exp = inst["states"], inst["nodes"], inst["status"], inst["out"]
    fail = status < 0
    assert len(nodes) == rec["instances"] and int(fail.sum()) == rec["failed"]
    d_states = torch.from_numpy(states).cuda()
    runs = {}
    for fast in (True, False):
        model = _model(name, fast)
        info = model.device_info()
        assert (model.domains() == inst["model"].domains()).all(), "the device's root fixpoint is not the oracle's"
        assert model.n_clauses == rec["clauses"] and info["tree_clauses"] == (rec["tree"] if fast else rec["tree_off"])
        assert info["max_tree"] <= T.MAX_TREE_NODES and (not fast or info["max_tree"] == rec["longest"])
        assert model.qualifies(6) == (name in K6_SETS)
        plan = model.plan()
        if name in K6_SETS:
            assert plan["rounds"] == f"cs_propagate_clause_rounds<{rec['cpl']}, true>", plan["rounds"]
        else:
            assert plan["rounds"] is None and rec["cpl"] is None
        # bigtab's tables stay in global memory, every other set's are copied into LDS
        assert plan["events"] == f"cs_propagate_events<true, {'false' if name == 'bigtab' else 'true'}, false>", plan["events"]
        for kernel in (1, 6) if name in K6_SETS else (1,):
            model.set_kernel(kernel)
            out, res = _run(model, d_states, nodes)
            what = (name, "fast paths" if fast else "interpreter", kernel)
            assert ((res[:, 0] < 0) == fail).all(), (what, nodes[np.nonzero((res[:, 0] < 0) != fail)[0][:4]].tolist())
            bad = np.nonzero(~fail & (out != exp).any((1, 2)))[0]
            assert len(bad) == 0, (what, len(bad), nodes[bad[:4]].tolist())
            assert (res[~fail, 0] == (exp[~fail, :, 0] != exp[~fail, :, 1]).sum(1)).all(), what
            assert res[:, 1].max() <= rec["width"], (what, int(res[:, 1].max()))
            runs[what] = (out, res)
            # the fixpoint property: the device leaves its own consistent outputs alone
            ok = np.nonzero(~fail)[0]
            again = np.stack([np.full(len(ok), -1), np.zeros(len(ok)), np.zeros(len(ok)), np.arange(len(ok))], 1).astype(np.int32)
            out2, res2 = model.propagate(torch.from_numpy(np.ascontiguousarray(out[ok])).cuda(), torch.from_numpy(again).cuda())
            torch.cuda.synchronize()
            out2, res2 = out2.cpu().numpy(), res2.cpu().numpy()
            assert (res2[:, 0] >= 0).all() and (res2[:, 1] == 0).all() and (out2 == out[ok]).all(), what
        model.close()
    first = next(iter(runs.values()))
    for what, (out, res) in runs.items():
        assert ((res[:, 0] < 0) == (first[1][:, 0] < 0)).all() and (out[~fail] == first[0][~fail]).all(), what
        assert (res[~fail, 0] == first[1][~fail, 0]).all(), what
    # the oracle's full re-propagation of the device's outputs changes nothing either
    out = first[0]
    for row in np.unique(out[~fail].reshape(int((~fail).sum()), -1), axis=0):
        state = row.reshape(out.shape[1:])
        st, again = inst["oracle"].instance(state, -1, 0, 0)
        assert st >= 0 and (again == state).all(), (name, state.tolist())
    if name in T.BRUTE:
        for what, (out, res) in runs.items():
            T.check_against_solutions(_solutions(name), states, nodes, np.where(res[:, 0] < 0, -1, 0), out)
    _report(name, {"variables": rec["vars"], "clauses": rec["clauses"], "tree_clauses": rec["tree"], "longest_tree": rec["longest"],
                   "kernel6_clauses_per_lane": rec["cpl"], "instances_compared": len(nodes) * len(runs), "left_out": 0,
                   "largest_props_device": int(max(r[1][:, 1].max() for r in runs.values())),
                   "largest_props_oracle": rec["props"], "total_width": rec["width"]})


def _replay(state, node, trace, lists):
    """apply a trail in order to the node's parent with the assignment made: every move narrows, and its clause
    mentions the moved variable -> the replayed state, whether a failure record or an emptied domain ends it"""
    v, lo, hi = node
    dom = state.copy()
    dom[v] = (lo, hi)
    failed = False
    for var, kind, bound, clause in trace:
        assert 0 <= clause < len(lists) and kind in (0, 1, 2)
        if kind == 2:
            failed = True
            continue
        assert var in lists[clause], ("clause", int(clause), "does not mention variable", int(var), sorted(lists[clause]))
        if kind == 0:
            assert bound > dom[var, 0]
            dom[var, 0] = bound
        else:
            assert bound < dom[var, 1]
            dom[var, 1] = bound
    return dom, failed or bool((dom[:, 0] > dom[:, 1]).any())


@pytest.mark.parametrize("name", T.SMALL)
def test_single_node_paths_and_trails(name):
    """100 value and interval nodes of every small set through propagate_one and propagate_one_traced: the batched
    verdicts and fixpoints (the oracle's); replaying the trail from the parent gives the fixpoint; every record's clause
    mentions the narrowed variable somewhere in its tree -- a variable missing from a tree clause's adjacency would
    leave the fixpoint wide, one listed with a clause that does not hold it would show here; a failed node's trail ends
    in a failure record or an emptied interval, also where the failure is a product's (no factor divides the wanted
    value) or a constant's and no variable is to blame"""
    inst = _instances(name)
    model = _model(name)
    om = inst["model"]
    assert model.n_clauses == om.n_clauses
    lists = T.clause_variables(om)
    pick = np.nonzero(inst["nodes"][:, 0] >= 0)[0]
    pick = pick[np.linspace(0, len(pick) - 1, SINGLE).astype(int)]
    failures = moved = 0
    for i in pick:
        v, lo, hi, p = (int(x) for x in inst["nodes"][i])
        parent, st, exp = inst["states"][p], inst["status"][i], inst["out"][i]
        got, props, out = model.propagate_one(parent, v, lo, hi)
        assert (got < 0) == (st < 0), (name, i)
        got_t, props_t, out_t, trace = model.propagate_one_traced(parent, v, lo, hi)
        replayed, failed = _replay(parent, (v, lo, hi), trace, lists)
        assert (got_t < 0) == (st < 0) == failed, (name, i)
        if st >= 0:
            assert (out == exp).all() and (out_t == exp).all() and (replayed == exp).all(), (name, i)
            assert got == got_t == int((exp[:, 0] != exp[:, 1]).sum())
            assert props_t <= len(trace) <= 2 * props_t and props_t <= T.RECORDED[name]["width"]
            moved += len(trace)
        else:
            failures += 1
    assert failures > 0 and moved > 0
    model.close()


@pytest.mark.parametrize("name", T.SMALL + ["longsum_prefix"])
def test_clause_and_root_evaluation(name):
    """eval_clauses and eval_root on the device: on complete assignments, satisfying and violating, clause i + 1 has the
    truth of predicate i (undecided where a compared side is a sentinel; a clause the root phase folded away is true)
    and the root the conjunction; on partial states of the walks every clause has the oracle's interval"""
    inst = _instances(name)
    om, orc, cols = inst["model"], inst["oracle"], inst["columns"]
    _, preds, bounds = T.generate_set(name)
    model = _model(name)
    assert model.n_clauses == om.n_clauses == 1 + len(preds) + 2 * len(bounds)
    root = om.domains()
    rows, pts = T.points(name, cols, box=root)  # inside the root intervals: finalize drops the clauses they entail
    inside = ((rows >= root[:, 0]) & (rows <= root[:, 1])).all(1)
    assert inside.all()
    complete = np.ascontiguousarray(np.stack([rows, rows], 2).astype(np.int32))
    partial = inst["states"][:: max(1, len(inst["states"]) // 40)]
    everything = np.concatenate([complete, partial])
    roots = model.eval_root(torch.from_numpy(everything).cuda()).cpu().numpy()
    true = false = 0
    for k, state in enumerate(everything):
        got = model.eval_clauses(torch.from_numpy(state).cuda().contiguous()).cpu().numpy()
        orc.set_domains(state)
        want = np.array([orc.eval(om.view.clause_node[c]) for c in range(om.n_clauses)])
        assert (got == want).all(), (name, k, np.nonzero((got != want).any(1))[0][:4].tolist())
        if k < len(complete):
            x = pts[k]
            for i, p in enumerate(preds):
                assert tuple(got[i + 1]) == T.truth(p, x) or (tuple(got[i + 1]) == (1, 1) and not inside[k]), (name, k, i, p.shape)
        lo, hi = orc.eval(om.root)
        assert roots[k] == (1 if lo > 0 or hi < 0 else (0 if lo == hi == 0 else 2)), (name, k)
        if k < len(complete) and all(p.decided is None or bool(p.decided(pts[k])) for p in preds) and inside[k]:
            holds = all(bool(p(pts[k])) for p in preds)
            assert roots[k] == int(holds)
            true, false = true + holds, false + (not holds)
    # sat_prod has products that are at a sentinel on all of their domain: no point decides every clause there
    assert name == "sat_prod" or (true > 0 and false > 0)
    model.close()


@pytest.mark.parametrize("route", ["default", "kernel1-interpreter", "kernel6-interpreter"])
@pytest.mark.parametrize("name", T.SEARCHED)
def test_search_engine_against_the_brute_force(name, route):
    """an ALL search by the default engine, and with every clause through the interpreter under kernel 1 and under
    kernel 6: the streamed solutions are the brute force's points, each once, and nodes, cuts and solutions are those of
    the oracle-backed engine's walk with the same branching rule"""
    from csolve_amd.solver import Search
    model = _model(name, fast_paths=route == "default")
    if route != "default":
        assert model.device_info()["tree_clauses"] == T.RECORDED[name]["tree_off"]
        model.set_kernel(1 if route == "kernel1-interpreter" else 6)
    s = Search(model, 1 << 18, 1 << 14)
    s.stream_solutions()
    s.put(model.root_state())
    batches = list(s.iter_solutions())
    st = s.stats
    rows = np.concatenate(batches) if batches else np.zeros((0, model.n_vars), dtype=np.int32)
    assert st["done"] == 1 and st["pool"] == 0
    assert (st["nodes"], st["cuts"], st["solutions"]) == T.RECORDED[name]["search"], (name, route)
    cols = S.columns(model.var_names())
    found = {tuple(int(r[c]) for c in cols) for r in rows}
    _, preds, bounds = T.generate_set(name)
    assert len(rows) == len(found) == st["solutions"] and found == S.brute_force(preds, bounds)
    s.close()
    model.close()
