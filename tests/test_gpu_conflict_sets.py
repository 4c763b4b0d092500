"""GPU tests of learnt conflict clauses (CS_OP_CONFL in cs_tree_eval / cs_tree_revise) on the sets of conflict_sets.py:
wide domains, negative and interior conflict values, values off the domain, a variable twice in a clause, clauses of one
and of 255 elements, clauses next to other expression trees, models that change kernel 6's class or leave it -- and leave
the `!=`-only kernels -- when the clauses arrive after finalize.  Every instance is judged by the order-free strong
reference (conflict_sets.strong / judge): none is left out.  test_conflict_sets_host.py checks on the CPU that no
instance here takes more than 4,096 propagations and that the oracle keeps the same two facts."""
import json
import os

import numpy as np
import pytest

import conflict_sets as K
import tree_sets as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E_ARG, E_LIMIT = -1, -4
NE_ONLY = (2, 3, 4, 5, 7)


def _models(name, directory, fast_paths=True, add=True):
    """-> (the model with the clauses in its dump, the model of the dump without them and, with `add`, the clauses
    added after finalize one by one)"""
    from csolve_amd.solver import Model, set_linear_fast_paths
    full, plain = K.save_models(name, str(directory))
    try:
        set_linear_fast_paths(fast_paths)
        built = Model.from_dump(full).finalize()
        added = Model.from_dump(plain).finalize()
        if add:
            for c in K.build(name)["clauses"]:
                added.add_conflict(c)  # finalizes again, under the same setting
    finally:
        set_linear_fast_paths(True)
    return built, added


def _run(model, d_states, nodes):
    """the instances in their batches of 1, 63, 64, 65 and the rest -> (states_out, results)"""
    outs, ress, at = [], [], 0
    for B in K.batches(len(nodes)):
        out, res = model.propagate(d_states, torch.from_numpy(nodes[at:at + B]).cuda())
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
        ress.append(res.cpu().numpy())
        at += B
    assert at == len(nodes)
    return np.concatenate(outs), np.concatenate(ress)


def _judge_all(name, out, failed, what):
    """the two facts on every instance -> [is the instance the legitimate "S failed, consistent but violated"]"""
    inst, clauses = K.instances(name), K.build(name)["clauses"]
    return np.array([K.judge(inst["failed"][i], inst["out"][i], failed[i], out[i], clauses, what + (i, inst["nodes"][i].tolist()))
                     for i in range(len(failed))])


def _report(name, record):
    print("conflict sets:", name, json.dumps(record))
    out_dir = os.environ.get("CSOLVE_REPORT_DIR")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "conflict_sets_parity.json")
        everything = json.load(open(path)) if os.path.exists(path) else {}
        everything[name] = record
        json.dump(everything, open(path, "w"), indent=1, sort_keys=True)


@pytest.mark.parametrize("name", K.NAMES)
def test_fixpoint_parity(name, tmp_path):
    """kernel 1 and, where the model fits, kernel 6; the linear fast paths on and off; the clauses in the model's dump and
    added after finalize; batches of 1, 63, 64, 65 and the rest.  Per instance the two facts decide; where S is consistent
    also the open count, and the output fed back as the parent of a var = -1 node comes back unchanged with zero
    propagations.  The built and the added model agree on every instance, so do the fast-path settings per kernel, and
    kernel 1 and kernel 6 wherever S is consistent."""
    b, inst, rec = K.build(name), K.instances(name), K.RECORDED[name]
    states, nodes, s_failed, s_out = inst["states"], inst["nodes"], inst["failed"], inst["out"]
    assert len(nodes) == rec["instances"] and int(s_failed.sum()) == rec["failed"]
    d_states = torch.from_numpy(states).cuda()
    ok = np.nonzero(~s_failed)[0]
    again = np.stack([np.full(len(ok), -1), np.zeros(len(ok)), np.zeros(len(ok)), np.arange(len(ok))], 1).astype(np.int32)
    runs, report, judged = {}, {}, 0
    for fast in (True, False):
        built, added = _models(name, tmp_path, fast)
        for how, model in (("built", built), ("added", added)):
            assert (model.domains() == b["root"]).all() and model.n_clauses == rec["clauses"]
            assert model.qualifies(6) == (rec["cpl"] is not None) and not any(model.qualifies(k) for k in NE_ONLY)
            plan = model.plan()
            assert plan["rounds"] == (f"cs_propagate_clause_rounds<{rec['cpl']}, true>" if rec["cpl"] else None), (how, plan["rounds"])
            assert plan["events"].startswith("cs_propagate_events<true,"), plan["events"]
            for kernel in (1, 6) if rec["cpl"] else (1,):
                model.set_kernel(kernel)
                what = (name, "fast paths" if fast else "interpreter", how, kernel)
                out, res = _run(model, d_states, nodes)
                failed = res[:, 0] < 0
                odd = _judge_all(name, out, failed, what)
                judged += len(nodes)
                assert (res[ok, 0] == (s_out[ok, :, 0] != s_out[ok, :, 1]).sum(1)).all(), what
                assert res[:, 1].max() <= rec["width"], (what, int(res[:, 1].max()))
                out2, res2 = model.propagate(torch.from_numpy(np.ascontiguousarray(out[ok])).cuda(), torch.from_numpy(again).cuda())
                torch.cuda.synchronize()
                out2, res2 = out2.cpu().numpy(), res2.cpu().numpy()
                assert (res2[:, 0] >= 0).all() and (res2[:, 1] == 0).all() and (out2 == out[ok]).all(), what
                runs[what] = (out, failed)
                report["/".join(str(w) for w in what[1:])] = {
                    "left_out": 0, "device_failed": int(failed.sum()),
                    "violated_but_consistent": int(odd.sum()), "largest_props": int(res[:, 1].max()),
                    "violated_but_consistent_by_class": {k: int(sum(k in s for s, o in zip(inst["classes"], odd) if o)) for k in K.CLASSES}}
        built.close()
        added.close()
    for (_, paths, how, kernel), (out, failed) in runs.items():
        for other in ((name, paths, "built", kernel), (name, "fast paths", how, kernel)):
            out0, failed0 = runs[other]
            both = ~failed & ~failed0
            assert (failed == failed0).all() and (out[both] == out0[both]).all(), ((name, paths, how, kernel), "against", other)
        out1 = runs[(name, paths, how, 1)][0]
        assert (out[ok] == out1[ok]).all()
    assert judged == len(runs) * rec["instances"] == (8 if rec["cpl"] else 4) * len(nodes)
    assert rec["classes"] == K.class_counts(inst["classes"])
    _report(name, {"clauses": rec["clauses"], "conflict_clauses": K.CONFLICTS, "kernel6_clauses_per_lane": rec["cpl"],
                   "instances": len(nodes), "S_failed": int(s_failed.sum()), "classes": rec["classes"],
                   "instances_judged": judged, "left_out": 0, "runs": report})


def test_a_long_clause_is_taken_at_255_elements_and_refused_beyond(tmp_path):
    """long255: the three clauses of 255 elements are in the tables (1 + count == CS_MAX_TREE_NODES); one of 256 is
    refused with CSGPU_E_LIMIT, one of none and one on a variable that is not there with CSGPU_E_ARG, and after each
    refusal the model answers as before"""
    from csolve_amd._lib import CsolveError
    b, inst = K.build("long255"), K.instances("long255")
    built, added = _models("long255", tmp_path)
    assert built.device_info()["max_tree"] == added.device_info()["max_tree"] == T.MAX_TREE_NODES
    d_states = torch.from_numpy(inst["states"]).cuda()
    d_nodes = torch.from_numpy(inst["nodes"][-300:]).cuda()

    def answer():
        out, res = added.propagate(d_states, d_nodes)
        torch.cuda.synchronize()
        return out.cpu().numpy(), res.cpu().numpy()

    out0, res0 = answer()
    n = added.n_vars
    for elems, code in (([(v, 1) for v in range(n)], E_LIMIT), ([], E_ARG), ([(0, 1), (n, 1)], E_ARG), ([(-1, 0)], E_ARG)):
        with pytest.raises(CsolveError) as e:
            added.add_conflict(elems)
        assert e.value.code == code, (len(elems), e.value)
        assert added.n_clauses == b["full"].n_clauses
        out, res = answer()
        ok = res0[:, 0] >= 0
        assert (res[:, :2] == res0[:, :2]).all() and (out[ok] == out0[ok]).all()
    built.close()
    added.close()


def test_kernel_6_revises_a_clause_of_255_elements(tmp_path):
    """long255 is past kernel 6's 512 clauses, so its long clauses run on kernel 1 alone.  The one model that holds a tree
    of 256 nodes under a conflict clause and still fits kernel 6: 255 variables of [0, 2] and nothing else (1 + 510
    clauses), plus one clause of 255 elements -- 512 clauses, eight per lane on every lane.  Conflict values 0 on the
    first 128 variables and 2 on the others; parents have all but two elements at their values (the clause has two open:
    a fixpoint), nodes give one of the two its value (the clause shaves the other's lower or upper bound) or another
    value (the clause holds), and var = -1 nodes re-propagate rows with one element open.  Kernel 1 and kernel 6, the
    clause in the dump and added after finalize, every instance against the strong reference"""
    from csolve_amd.solver import Model
    from oracle.cs_oracle import Oracle
    n = K.MAX_CONFLICT
    text = K._plain_text("255 variables of [0, 2]", [(0, 2)] * n, [])
    plain, full = K._oracle_model(text), K._oracle_model(text)
    clause = [(v, 0 if v < 128 else 2) for v in range(n)]
    full.append_clause(full.add_confl([(full.var_node(v), cv) for v, cv in clause]))
    full.index()
    assert plain.n_clauses == 511 and full.n_clauses == 512 and T.clauses_per_lane(512) == 8
    base = Oracle(plain)
    root = plain.domains()
    assert (root == (0, 2)).all()
    rng = np.random.default_rng(255)
    states, nodes = [], []
    for _ in range(48):
        i, j = (int(x) for x in rng.choice(n, size=2, replace=False))
        row = np.array([(cv, cv) for _, cv in clause], dtype=np.int32)
        row[i] = row[j] = (0, 2)
        states.append(row)
        p = len(states) - 1
        nodes += [(i, clause[i][1], clause[i][1], p), (i, 1, 1, p), (j, clause[j][1], 1, p) if clause[j][1] == 0 else (j, 1, 2, p)]
        one = row.copy()
        one[i] = (clause[i][1], clause[i][1])
        states.append(one)
        nodes.append((-1, 0, 0, len(states) - 1))
    states, nodes = np.stack(states), np.array(nodes, dtype=np.int32)
    want = []
    for v, lo, hi, p in nodes:
        row = states[p].copy()
        if v >= 0:
            row[v] = (lo, hi)
        want.append(K.strong(base, [clause], row))
    seen = set().union(*(w[2] for w in want))
    assert {"shave_lo", "shave_hi", "stopped", "two_open"} <= seen and not any(w[0] for w in want)
    paths = str(tmp_path / "full.model"), str(tmp_path / "plain.model")
    full.save(paths[0])
    plain.save(paths[1])
    built, added = Model.from_dump(paths[0]).finalize(), Model.from_dump(paths[1]).finalize()
    assert added.plan()["rounds"].startswith("cs_propagate_clause_rounds<8,") and added.device_info()["tree_clauses"] == 0
    added.add_conflict(clause)
    d_states, d_nodes = torch.from_numpy(states).cuda(), torch.from_numpy(nodes).cuda()
    for how, model in (("built", built), ("added", added)):
        assert model.n_clauses == 512 and model.qualifies(6) and model.device_info()["max_tree"] == T.MAX_TREE_NODES
        assert model.plan()["rounds"] == "cs_propagate_clause_rounds<8, true>"
        for kernel in (1, 6):
            model.set_kernel(kernel)
            out, res = model.propagate(d_states, d_nodes)
            torch.cuda.synchronize()
            out, res = out.cpu().numpy(), res.cpu().numpy()
            for i, (f, s_out, _) in enumerate(want):
                K.judge(f, s_out, res[i, 0] < 0, out[i], [clause], (how, kernel, i, nodes[i].tolist()))
                assert res[i, 0] == (s_out[:, 0] != s_out[:, 1]).sum()
        model.close()


def test_plans_after_an_add(tmp_path):
    """queens12_learnt: the model of the dump without the clauses qualifies for kernel 7; after the add no `!=`-only
    kernel qualifies, solve_many refuses with its reason, no resident server is planned, and propagate / propagate_one
    under the automatic choice give the strong reference's results.  across512: 505 clauses qualify for kernel 6 and for
    solve_many_clauses, 517 do not"""
    from csolve_amd._lib import CsolveError
    name = "queens12_learnt"
    b, inst = K.build(name), K.instances(name)
    _, model = _models(name, tmp_path, add=False)
    assert model.qualifies(7) and model.plan()["shave"] is not None and model.n_clauses == b["base_clauses"]
    for j, c in enumerate(b["clauses"]):
        model.add_conflict(c)
        assert model.n_clauses == b["base_clauses"] + j + 1 and not any(model.qualifies(k) for k in NE_ONLY), j
    plan = model.plan()
    assert all(plan[f] is None for f in ("lds", "bitset", "regs0", "packed", "shave", "shave_trace", "server", "step_shave")), plan
    assert model.qualifies(1) and model.qualifies(6)
    model.set_kernel(0)
    rows = torch.from_numpy(model.domains()[None].copy()).cuda()
    with pytest.raises(CsolveError, match="does not qualify") as e:
        model.solve_many(rows, "ANY", max_nodes=100)
    assert e.value.code == E_LIMIT
    out, res = _run(model, torch.from_numpy(inst["states"]).cuda(), inst["nodes"])
    _judge_all(name, out, res[:, 0] < 0, (name, "automatic"))
    pick = np.nonzero(inst["nodes"][:, 0] >= 0)[0]
    shaved = [i for i in pick if inst["classes"][i] & {"shave_lo", "shave_hi"}]
    assert len(shaved) >= 100
    for i in shaved[:100] + list(pick[:: len(pick) // 100]):
        v, lo, hi, p = (int(x) for x in inst["nodes"][i])
        st, props, got = model.propagate_one(inst["states"][p], v, lo, hi)
        K.judge(inst["failed"][i], inst["out"][i], st < 0, got, b["clauses"], (name, "propagate_one", int(i)))
    assert model.server_stats()[1] == 0, "a resident server started for a model that left kernel 7"
    model.close()

    name = "across512"
    b = K.build(name)
    _, model = _models(name, tmp_path, add=False)
    assert model.n_clauses == 505 and model.qualifies(6) and model.qualifies_many_clauses()
    assert model.plan()["rounds"] == "cs_propagate_clause_rounds<8, true>"
    for j, c in enumerate(b["clauses"]):
        model.add_conflict(c)
        fits = model.n_clauses <= 512
        assert model.qualifies(6) == fits and model.qualifies_many_clauses() == fits, (j, model.n_clauses)
    assert model.n_clauses == 517 and model.plan()["rounds"] is None
    model.close()


def _replay(state, node, trace, lists, clauses, base_clauses, base_oracle):
    """apply a trail in order to the node's parent with the assignment made: every move narrows and its clause mentions
    the moved variable; a move that names a conflict clause finds that clause, at that moment, with the moved variable
    as its one open element and the conflict value on the bound that moves, by one; and the converse: a move that names
    a clause of the base model is one the base model alone implies at that moment -- its fixpoint without the conflict
    clauses (the oracle's, on the replayed state) fails or has moved that bound at least as far --, so a conflict clause's
    shave cannot pass under the name of a base clause that happens to mention the variable -> (the replayed state,
    whether a failure record or an emptied domain ends it, moves by conflict clauses)"""
    v, lo, hi = node
    dom = state.copy()
    if v >= 0:
        dom[v] = (lo, hi)
    failed, by_conflict = False, 0
    for var, kind, bound, clause in trace:
        assert 0 <= clause < len(lists) and kind in (0, 1, 2)
        if kind == 2:
            failed = True
            continue
        assert var in lists[clause], ("clause", int(clause), "does not mention variable", int(var), sorted(lists[clause]))
        if clause >= base_clauses:
            c = clauses[clause - base_clauses]
            state_of, k = K.clause_state(dom, c)
            assert state_of == "unit" and c[k][0] == var, (int(clause), c, state_of, int(var))
            cv = c[k][1]
            assert (kind == 0 and dom[var, 0] == cv and bound == cv + 1) or (kind == 1 and dom[var, 1] == cv and bound == cv - 1), \
                (int(clause), c, int(var), int(kind), int(bound), dom[var].tolist())
            by_conflict += 1
        elif (dom[:, 0] <= dom[:, 1]).all():
            st, fix = base_oracle.instance(dom, -1, 0, 0)
            assert st < 0 or (fix[var, 0] >= bound if kind == 0 else fix[var, 1] <= bound), \
                ("the base model does not imply the move its clause is named for", int(clause), int(var), int(kind), int(bound))
        if kind == 0:
            assert bound > dom[var, 0]
            dom[var, 0] = bound
        else:
            assert bound < dom[var, 1]
            dom[var, 1] = bound
    return dom, failed or bool((dom[:, 0] > dom[:, 1]).any()), by_conflict


@pytest.mark.parametrize("name", K.TRAILED)
def test_trails(name, tmp_path):
    """propagate_one_traced on value and interval nodes, half of them nodes on which a conflict clause shaves: replaying
    the trail in order gives the fixpoint; a record that names a conflict clause names the right one -- clause
    base_clauses + j for the j-th clause, built in or added, which sits on the list of every one of its variables --, and
    a record that names a base clause is a move the base model alone implies; a failed node ends in a failure record or
    an emptied interval"""
    b, inst = K.build(name), K.instances(name)
    lists = T.clause_variables(b["full"])
    for j, c in enumerate(b["clauses"]):
        assert lists[b["base_clauses"] + j] == {v for v, _ in c}
    pick = np.nonzero(inst["nodes"][:, 0] >= 0)[0]
    shaved = [i for i in pick if inst["classes"][i] & {"shave_lo", "shave_hi"}]
    chosen = shaved[:: max(1, len(shaved) // 120)][:120] + list(pick[:: len(pick) // 120])
    for how, model in zip(("built", "added"), _models(name, tmp_path)):
        failures = moved = by_conflict = 0
        for i in chosen:
            v, lo, hi, p = (int(x) for x in inst["nodes"][i])
            parent = inst["states"][p]
            st, props, out, trace = model.propagate_one_traced(parent, v, lo, hi)
            replayed, failed, k = _replay(parent, (v, lo, hi), trace, lists, b["clauses"], b["base_clauses"], b["plain_oracle"])
            assert (st < 0) == failed, (name, how, int(i))
            K.judge(inst["failed"][i], inst["out"][i], st < 0, replayed, b["clauses"], (name, how, "traced", int(i)))
            if st >= 0:
                assert (out == replayed).all(), (name, how, int(i))
                moved += len(trace)
            else:
                failures += 1
            by_conflict += k
        print(name, how, "nodes", len(chosen), "failed", failures, "records", moved, "by conflict clauses", by_conflict)
        assert failures > 0 and moved > 0 and by_conflict >= 50, (name, how, failures, moved, by_conflict)
        model.close()


def _confl_value(dom, clause):
    """eval.c:258-277: elements in order; the first one that is not a value answers unknown, the first value other than
    its conflict value answers true; all at their conflict values: unknown"""
    for v, cv in clause:
        if dom[v, 0] != dom[v, 1]:
            return (0, 1)
        if dom[v, 0] != cv:
            return (1, 1)
    return (0, 1)


@pytest.mark.parametrize("name", K.NARROW)
def test_evaluation(name, tmp_path):
    """eval_clauses of the conflict clauses: on complete assignments 1 where an element differs from its conflict value
    and [0, 1] where all match; on partial states of the walks the "first non-value answers unknown" order; every clause
    of the model has the oracle's interval"""
    b, inst = K.build(name), K.instances(name)
    om, orc, base = b["full"], b["full_oracle"], b["base_clauses"]
    root = b["root"]
    rng = np.random.default_rng(5)
    pts = np.stack([rng.integers(root[:, 0], root[:, 1] + 1) for _ in range(60)])
    # complete assignments that match a clause on every element, where the root row has room for them
    for c in b["clauses"]:
        row = pts[len(c) % len(pts)].copy()
        for v, cv in c:
            row[v] = cv
        if ((row >= root[:, 0]) & (row <= root[:, 1])).all() and all(row[v] == cv for v, cv in c):
            pts = np.concatenate([pts, row[None]])
    complete = np.stack([pts, pts], 2).astype(np.int32)
    partial = inst["states"][:: max(1, len(inst["states"]) // 60)]
    everything = np.ascontiguousarray(np.concatenate([complete, partial]))
    for how, model in zip(("built", "added"), _models(name, tmp_path)):
        matched = true = unknown_partial = 0
        for k, state in enumerate(everything):
            got = model.eval_clauses(torch.from_numpy(state).cuda().contiguous()).cpu().numpy()
            orc.set_domains(state)
            want = np.array([orc.eval(om.view.clause_node[c]) for c in range(om.n_clauses)])
            assert (got == want).all(), (name, how, k, np.nonzero((got != want).any(1))[0][:4].tolist())
            for j, c in enumerate(b["clauses"]):
                mine = _confl_value(state, c)
                assert tuple(got[base + j]) == mine, (name, how, k, j, c, got[base + j].tolist())
                if k < len(complete):
                    all_match = all(state[v, 0] == cv for v, cv in c)
                    assert mine == ((0, 1) if all_match else (1, 1))
                    matched, true = matched + all_match, true + (not all_match)
                else:
                    unknown_partial += mine == (0, 1)
        assert matched >= 3 and true > 100 and unknown_partial > 100, (matched, true, unknown_partial)
        model.close()


def _subject(name, directory, how):
    """-> (the model that holds the clauses: from its dump, or re-finalized by twelve add_conflict calls; the model
    without them)"""
    built, plain = _models(name, directory, add=False)
    if how == "built":
        return built, plain
    built.close()
    other, added = _models(name, directory)
    other.close()
    return added, plain


def _search_all(model, route):
    """an ALL search from the model's root row -> (statistics, streamed rows)"""
    from csolve_amd.solver import Search
    model.set_kernel({"default": 0, "kernel1": 1, "kernel6": 6}[route])
    s = Search(model, 1 << 20, 1 << 16)
    s.stream_solutions()
    s.put(model.root_state())
    batches = list(s.iter_solutions())
    st = s.stats
    s.close()
    assert st["done"] == 1 and st["pool"] == 0
    return st, (np.concatenate(batches) if batches else np.zeros((0, model.n_vars), dtype=np.int32))


@pytest.mark.parametrize("how", ["built", "added"])
@pytest.mark.parametrize("route", ["default", "kernel1", "kernel6"])
@pytest.mark.parametrize("name", K.SEARCHED)
def test_search(name, route, how, tmp_path):
    """an ALL search on a model that holds implied conflict clauses -- in its dump, and added to the finalized model
    (queens-12: a kernel-7 model until then), whose tables and plans add_conflict rebuilt before the engine was made --
    by the default engine, by kernel 1 and by kernel 6: the streamed solutions are the base model's (narrow_implied: the
    brute force's points; queens-12: the recorded 14,200, each a placement without an attack), each once.  The same
    search of the model without the clauses runs next to it on the device: its tree is the oracle-backed engine's
    recorded one, and -- test_conflict_sets_host.py shows for that engine that the clauses never cost a node on these
    two sets -- the search with the clauses takes no more nodes than it"""
    b = K.build(name)
    model, plain = _subject(name, tmp_path, how)
    assert model.n_clauses == plain.n_clauses + K.CONFLICTS and not any(model.qualifies(k) for k in NE_ONLY)
    st, rows = _search_all(model, route)
    found = {tuple(int(x) for x in r) for r in rows}
    assert len(rows) == len(found) == st["solutions"] == K.SEARCH[name]["with"][2]
    if b["rows"] is not None:
        assert found == {tuple(int(x) for x in r) for r in b["rows"]}
    else:
        assert len(found) == K.QUEENS12_SOLUTIONS
        q = rows.astype(np.int64)
        i = np.arange(q.shape[1])
        for a in (q, q + i, q - i):  # columns and both diagonals: no two queens share one
            assert (np.sort(a, 1)[:, 1:] != np.sort(a, 1)[:, :-1]).all()
    st0, rows0 = _search_all(plain, route)
    print("conflict sets search:", name, route, how, "nodes", st["nodes"], "cuts", st["cuts"], "without the clauses", st0["nodes"], st0["cuts"],
          "oracle engine with / without", K.SEARCH[name]["with"][:2], K.SEARCH[name]["without"][:2])
    assert (st0["nodes"], st0["cuts"], st0["solutions"]) == K.SEARCH[name]["without"] and len(rows0) == st0["solutions"]
    assert K.SEARCH[name]["with"][0] <= K.SEARCH[name]["without"][0]  # what the host file shows
    assert st["nodes"] <= st0["nodes"], (st["nodes"], st0["nodes"], K.SEARCH[name])
    model.close()
    plain.close()


@pytest.mark.parametrize("how", ["built", "added"])
def test_solve_many_clauses_on_a_model_with_conflict_clauses(how, tmp_path):
    """narrow_implied, 64 root rows (consistent fixpoints of the walks), ALL, the clauses in the dump and added after
    finalize: every instance ends with as many solutions as the brute force has below its row"""
    name = "narrow_implied"
    inst = K.instances(name)
    model, other = _subject(name, tmp_path, how)
    other.close()
    assert model.qualifies_many_clauses()
    ok = np.nonzero(~inst["failed"])[0]
    rows = np.unique(inst["out"][ok].reshape(len(ok), -1), axis=0).reshape(-1, model.n_vars, 2)
    rows = np.ascontiguousarray(np.concatenate([K.build(name)["root"][None], rows[:: max(1, len(rows) // 63)][:63]]), dtype=np.int32)
    assert len(rows) == 64
    out = model.solve_many_clauses(rows, "ALL", max_nodes=1 << 20)
    torch.cuda.synchronize()
    want = np.array([int(K.solutions_below(name, r).sum()) for r in rows])
    assert (out["status"].cpu().numpy() == 0).all()
    assert (out["solutions"].cpu().numpy() == want).all(), (out["solutions"].cpu().numpy().tolist(), want.tolist())
    assert want[0] == len(K.build(name)["rows"]) and (want > 0).sum() > 20 and len(set(want.tolist())) > 5
    model.close()
