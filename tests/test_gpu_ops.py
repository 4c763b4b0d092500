"""GPU tests at operator level: the known-answer vectors of the reference's unit tests
(tests/golden/ref_unit_*.json) on the device.

  * eval vectors: each expression becomes the single clause of a model; the device's clause
    value (cs_eval_clauses, i.e. eval_<op>) must equal the reference's expected interval.
  * propagate vectors: the reference pins them with a mocked bind(), which cannot exist on a
    device that really narrows; so each case is wrapped into a clause (push true -> X, push false
    -> NOT(X), push an interval v -> EQ(X, v)) and the device's root fixpoint of that one clause is
    compared with the oracle's (the oracle itself is pinned on the raw vectors by the CPU tests).
    This drives every operator -- EQ LT NEG ADD MUL NOT AND OR WAND -- through the device with the
    reference's operand values, including the +-infinity sentinels and the saturating cases, and the learnt
    conflict clauses (PropagateConfl.*) through the same interpreter.
"""
import json
import os

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _cases(name):
    return json.load(open(golden(f"ref_unit_{name}.json")))["cases"]


def _build(case, wrap=None):
    """oracle-side model builder; every non-value terminal becomes a variable (the device treats
    constants as immutable), value terminals become constants"""
    from oracle.cs_oracle import Model as OModel
    m = OModel.empty()
    node = {}
    for name, t in case["terms"].items():
        lo, hi = t["dom"]
        node[name] = m.var_node(m.add_var(name, lo, hi)) if lo != hi else m.add_const(lo, hi)
    pending = dict((k, v) for k, v in case["exprs"].items() if v is not None)
    while pending:
        progressed = False
        for name, e in list(pending.items()):
            kids = e[1] if e[0] == "WAND" else ([k for k, _ in e[1]] if e[0] == "CONFL" else
                                                 [k for k in e[1:] if k is not None])
            if all(k in node for k in kids):
                if e[0] == "CONFL":
                    node[name] = m.add_confl([(node[k], v) for k, v in e[1]])
                else:
                    node[name] = m.add_wand([node[k] for k in kids]) if e[0] == "WAND" else \
                        m.add_node(e[0], node[e[1]], node[e[2]] if e[2] is not None else -1)
                del pending[name]
                progressed = True
        if not progressed:
            break
    top = node[case["target"]]
    if wrap is not None:
        lo, hi = wrap
        if (lo, hi) == (0, 0):
            top = m.add_node("NOT", top)
        elif not (lo > 0 or hi < 0) or lo != hi:
            top = m.add_node("EQ", top, m.add_const(lo, hi))
        elif (lo, hi) != (1, 1):
            top = m.add_node("EQ", top, m.add_const(lo, hi))
    m.set_root(m.add_wand([top]))
    return m


def test_eval_vectors_on_device(tmp_path):
    from csolve_amd.solver import Model
    cases = _cases("eval")
    for i, c in enumerate(cases):
        om = _build(c)
        om.index()
        path = str(tmp_path / f"e{i}.model")
        om.save(path)
        vals = Model.from_dump(path).eval_clauses_host()
        expect = c["expect"]
        if c["fn"] == "eval_wand":
            continue  # a wide-and root is split into its elements as clauses; covered by eval_root tests
        assert vals[0].tolist() == expect, (c["test"], c["fn"], vals[0].tolist(), expect)


def test_propagate_vectors_wrapped_vs_oracle(tmp_path):
    from csolve_amd.solver import Model
    from oracle.cs_oracle import Oracle
    cases = [c for c in _cases("propagate") if c["fn"] not in ("propagate", "propagate_wand", "propagate_term")]
    assert len(cases) > 100
    checked = 0
    for i, c in enumerate(cases):
        om = _build(c, wrap=tuple(c["val"]))
        if om.n_vars == 0:
            continue
        om.index()
        orc = Oracle(om)
        orc.set_root_phase(True)
        want = orc.propagate(om.root, 1 << 20)
        path = str(tmp_path / f"p{i}.model")
        om.save(path)
        gm = Model.from_dump(path)
        got = gm.root_propagate()
        assert (got < 0) == (want < 0), (c["test"], c["fn"], c["val"], got, want)
        if want >= 0:
            assert (gm.domains() == orc.domains()).all(), (c["test"], c["fn"], c["val"])
        checked += 1
    assert checked > 60


def _sat_text(n, m, seed):
    """fuzz/inputs/sat.txt style: 0/1 variables, three-literal clauses (one statement per clause: a conjunction
    written as a single statement stays ONE expression tree, and the device interprets trees of at most 256 nodes)"""
    rng = np.random.default_rng(seed)
    cl = []
    for _ in range(m):
        vs = rng.choice(n, size=3, replace=False)
        cl.append("(" + "|".join(("!" if rng.integers(2) else "") + f"x{v + 1}" for v in vs) + ")")
    return "ANY;\n" + "".join(c + ";\n" for c in cl) + "".join(f"0<=x{v + 1};x{v + 1}<=1;\n" for v in range(n))


def _walk_instances(orc, root, rng, count, accept=None):
    """(parents [k, n, 2], nodes [count, 4]): dives from the root; every parent is a fixpoint of the oracle (and one
    that accept() takes, where given)"""
    parents, nodes = [root.copy()], []
    cur = 0
    while len(nodes) < count:
        dom = parents[cur]
        open_vars = np.flatnonzero(dom[:, 0] != dom[:, 1])
        if len(open_vars) == 0:
            cur = 0
            continue
        v = int(rng.choice(open_vars))
        val = int(rng.integers(dom[v, 0], dom[v, 1] + 1))
        nodes.append((v, val, val, cur))
        st, out = orc.instance(dom, v, val, val)
        if st >= 0 and (accept is None or accept(out)) and rng.integers(4) != 0:
            parents.append(out.copy())
            cur = len(parents) - 1
        else:
            cur = 0
    return np.stack(parents).astype(np.int32), np.array(nodes, dtype=np.int32)


def test_learnt_conflict_clauses_against_the_oracle(tmp_path):
    """0/1 problems with conflict clauses (struct confl_t): the device's fixpoints, verdicts and PROPS equal the
    oracle's on dives from the root -- with the clauses in the model from the start, and with the same clauses added
    to a finalized model (csgpu_model_add_conflict); the general kernel and the clause-resident one agree.  Every
    instance is judged, by the order-free strong reference of conflict_sets.py: where it is consistent the oracle and
    the device equal it (and each other, PROPS included); where it failed each of them fails or ends in a state that
    violates a clause -- which the device, on 0/1 domains, never does"""
    import conflict_sets as K
    from csolve_amd.solver import Model
    from oracle.cs_oracle import Model as OModel, Oracle
    report = []
    for seed in range(4):
        rng = np.random.default_rng(100 + seed)
        n = 24 + 8 * seed
        m = int(4.2 * n)
        text = _sat_text(n, m, seed)
        confl = []
        for _ in range(12):
            k = int(rng.integers(2, 6))
            confl.append([(int(v), int(rng.integers(2))) for v in rng.choice(n, size=k, replace=False)])

        def oracle_model(with_conflicts):
            om = OModel.parse(text)
            if with_conflicts:
                for c in confl:
                    om.append_clause(om.add_confl([(om.var_node(v), val) for v, val in c]))
            om.index()
            o = Oracle(om)
            o.set_root_phase(True)
            assert o.propagate(om.root, 1 << 20) >= 0
            om.set_domains(o.domains())
            om.index()
            return om

        om = oracle_model(True)
        orc = Oracle(om)
        # a parent is a fixpoint that violates no clause: then it is the strong reference's fixpoint as well
        parents, nodes = _walk_instances(orc, om.domains(), rng, 600, accept=lambda out: not K.violated(out, confl))
        want = [orc.instance(parents[p], int(v), int(lo), int(hi)) for v, lo, hi, p in nodes]
        assert sum(1 for st, _ in want if st < 0) > 10 and sum(1 for st, _ in want if st >= 0) > 100

        path = str(tmp_path / f"sat{seed}.model")
        om.save(path)
        with_clauses = Model.from_dump(path).finalize()
        plain = oracle_model(False)
        # the root fixpoint without the conflicts may be wider: use the same domains so that only the clauses differ
        plain.set_domains(om.domains())
        plain.index()
        path2 = str(tmp_path / f"sat{seed}_plain.model")
        plain.save(path2)
        added = Model.from_dump(path2).finalize()
        plain_orc = Oracle(plain)
        strong = []
        for v, lo, hi, p in nodes:
            row = parents[p].copy()
            row[v] = (lo, hi)
            strong.append(K.strong(plain_orc, confl, row)[:2])
        for c in confl:
            added.add_conflict(c)
        assert added.n_clauses == with_clauses.n_clauses == m + len(confl) or added.n_clauses == with_clauses.n_clauses
        d_par, d_nodes = torch.from_numpy(parents).cuda(), torch.from_numpy(nodes).cuda()
        for gm in (with_clauses, added):
            for k in (1, 6):
                if not gm.qualifies(k):
                    continue
                gm.set_kernel(k)
                out, res = gm.propagate(d_par, d_nodes)
                torch.cuda.synchronize()
                out, res = out.cpu().numpy(), res.cpu().numpy()
                compared = skipped_ref = skipped_dev = 0
                for i, (st, exp) in enumerate(want):
                    # propagate_confl infers but never fails (propagate.c:461-471: with every element at its conflict
                    # value it answers PROP_NONE), so when two clauses push one variable opposite ways the outcome
                    # depends on the order of the revisions: the reference's depth-first order ends in a state that
                    # violates one of these (random, not implied) conflicts, the device's rounds see the bounds cross.
                    # The strong reference fails such a node, and failing it or ending in a violated state are the two
                    # answers it allows; no instance is left out.
                    s_failed, s_out = strong[i]
                    what = (seed, k, i, nodes[i].tolist(), st, res[i].tolist())
                    skipped_ref += K.judge(s_failed, s_out, st < 0, exp, confl, ("oracle",) + what)
                    skipped_dev += K.judge(s_failed, s_out, res[i, 0] < 0, out[i], confl, ("device",) + what)
                    compared += 1
                    if not s_failed:  # both equal the strong reference's fixpoint
                        assert st >= 0 and res[i, 0] >= 0 and (out[i] == exp).all(), what
                        assert res[i, 1] == st, (seed, k, i, "PROPS")
                    elif st < 0:
                        assert res[i, 0] < 0, what
                assert compared > 400, compared
                assert compared == len(want) == 600
                # how many instances have no order-independent answer is part of the record, not hidden
                report.append({"seed": int(seed), "kernel": k, "model": "clauses at build time" if gm is with_clauses else "added after finalize",
                               "instances": len(want), "compared": compared, "strong_reference_failed": sum(f for f, _ in strong),
                               "reference_state_violates_a_conflict": skipped_ref,
                               "device_state_violates_a_conflict": skipped_dev})
                assert skipped_dev == 0, "a consistent device state never violates a learnt clause: the rounds see the bounds cross"

    # the count of left-out instances is part of the evidence (profiles/ keeps the copy of a GPU run)
    import json
    import os
    out_dir = os.environ.get("CSOLVE_REPORT_DIR")
    print("conflict-clause parity:", json.dumps(report))
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        json.dump({"test": "tests/test_gpu_ops.py::test_learnt_conflict_clauses_against_the_oracle",
                   "note": "every instance is judged by the strong reference of tests/conflict_sets.py; where it fails, the "
                           "reference may end in a state that violates one of the random conflict clauses (propagate_confl "
                           "never fails, propagate.c:461-471): those are counted, none is left out",
                   "runs": report}, open(os.path.join(out_dir, "conflict_clause_parity.json"), "w"), indent=1)


def test_trail_of_one_node(tmp_path):
    """csgpu_propagate_one_traced: replaying the recorded narrowings in order gives the fixpoint, every record names
    a clause that mentions the narrowed variable, a failing node ends in a failure record, and the verdicts and
    fixpoints are those of the untraced call"""
    from csolve_amd import problems
    from csolve_amd.solver import solve_root
    from oracle.cs_oracle import Model as OModel, Oracle
    for text in (_sat_text(30, 90, 3), problems.queens(8), problems.schedule(6, 1)):
        gm = solve_root(text)
        om = OModel.parse(text)
        om.set_domains(gm.domains())
        om.normalize()
        om.index()
        assert om.n_clauses == gm.n_clauses
        orc = Oracle(om)
        rng = np.random.default_rng(9)
        parents, nodes = _walk_instances(orc, gm.domains(), rng, 120)
        # variables of every clause
        lists = [set() for _ in range(om.n_clauses)]
        for v in range(om.n_vars):
            for i in range(om.view.list_off[v], om.view.list_off[v + 1]):
                lists[om.view.list[i]].add(v)
        failures = 0
        for v, lo, hi, p in nodes:
            st, props, out, trace = gm.propagate_one_traced(parents[p], int(v), int(lo), int(hi))
            st0, props0, out0 = gm.propagate_one(parents[p], int(v), int(lo), int(hi))
            assert (st < 0) == (st0 < 0) and (st < 0 or (out == out0).all())
            # PROPS counts a lower and an upper bound moved by one revision once (propagate_term binds both at once)
            moved = int((trace[:, 1] != 2).sum())
            assert props <= moved <= 2 * props, (props, moved)
            dom = parents[p].copy()
            dom[v] = (lo, hi)
            for var, kind, bound, clause in trace:
                assert 0 <= clause < om.n_clauses
                if kind == 2:
                    continue
                assert var in lists[clause], (var, clause)
                if kind == 0:
                    assert bound > dom[var, 0]
                    dom[var, 0] = bound
                else:
                    assert bound < dom[var, 1]
                    dom[var, 1] = bound
            if st >= 0:
                assert (dom == out).all() and not (trace[:, 1] == 2).any()
            else:
                failures += 1
                assert (trace[:, 1] == 2).any() or (dom[:, 0] > dom[:, 1]).any()
        assert failures > 0


def test_causes_of_one_node():
    """csgpu_propagate_one_causes (kernel 7's tracing variant): replaying the records in order gives the fixpoint, every
    cause is a neighbour of the moved variable that is a value in the fixpoint (or the assigned variable), a failing
    node's replay empties a domain, and verdict / fixpoint / PROPS are those of the untraced call"""
    from csolve_amd import problems
    from csolve_amd.solver import solve_root
    from oracle.cs_oracle import Model as OModel, Oracle
    for text in (problems.queens(12), problems.queens(70), problems.offsets(40, 30, 5), problems.sudoku(3, 0.3, 2)):
        gm = solve_root(text)
        if not gm.qualifies(7):
            continue
        om = OModel.parse(text)
        om.set_domains(gm.domains())
        om.normalize()
        om.index()
        neigh = [set() for _ in range(om.n_vars)]
        members = [set() for _ in range(om.n_clauses)]
        for v in range(om.n_vars):
            for i in range(om.view.list_off[v], om.view.list_off[v + 1]):
                members[om.view.list[i]].add(v)
        for vs in members:
            for a in vs:
                neigh[a] |= vs - {a}
        orc = Oracle(om)
        rng = np.random.default_rng(17)
        parents, nodes = _walk_instances(orc, gm.domains(), rng, 150)
        failures = 0
        for v, lo, hi, p in nodes:
            st, props, out, trace = gm.propagate_one_causes(parents[p], int(v), int(lo), int(hi))
            st0, props0, out0 = gm.propagate_one(parents[p], int(v), int(lo), int(hi))
            assert (st < 0) == (st0 < 0)
            dom = parents[p].copy()
            dom[v] = (lo, hi)
            emptied = False
            for var, kind, bound, cause in trace:
                assert kind in (0, 1) and 0 <= var < om.n_vars and 0 <= cause < om.n_vars and cause != var
                # a variable that is a value at the root has no clause list (parser_support.c:341) and so no entry in
                # `neigh`; as a cause it is legitimate (its value can forbid the value a bound has just moved onto)
                root = gm.domains()
                assert cause in neigh[var] or var in neigh[cause] or root[cause, 0] == root[cause, 1] or \
                    root[var, 0] == root[var, 1], (var, cause)
                if kind == 0:
                    assert bound > dom[var, 0]
                    dom[var, 0] = bound
                else:
                    assert bound < dom[var, 1]
                    dom[var, 1] = bound
                if dom[var, 0] > dom[var, 1]:
                    emptied = True
                    break
            if st >= 0:
                assert not emptied and (dom == out).all() and (out == out0).all() and props == props0
                assert props == len(trace) or props >= len(trace)  # a record may stand for several unit moves
            else:
                failures += 1
                assert emptied
        assert failures > 0


def test_the_references_own_failure_chain_of_one_node():
    """csgpu_propagate_one_chain (cs_chain.hip.h: one wavefront walks the reference's depth-first propagation): on the
    failing nodes of random dives the variables it bumps -- the emptied variable, then the recursion stack, innermost
    first (propagate.c:33-54) -- and the narrowings made before the failure are exactly the oracle's, which restates
    that walk on the CPU; consistent nodes come out consistent with the reference's PROPS"""
    from csolve_amd import problems
    from csolve_amd.solver import solve_root
    from oracle.cs_oracle import Model as OModel, Oracle
    checked_fail = checked_ok = with_chain = 0
    for text in (problems.queens(8), problems.queens(16), problems.queens(40), problems.queens(64), problems.queens(128),
                 problems.sudoku(3, 0.3, 2), problems.offsets(20, 12, 3)):
        gm = solve_root(text)
        om = OModel.parse(text)
        om.set_domains(gm.domains())
        om.normalize()
        om.index()
        assert om.n_clauses == gm.n_clauses
        orc = Oracle(om)
        rng = np.random.default_rng(17)
        n = gm.n_vars
        for walk in range(16):
            dom = np.ascontiguousarray(gm.domains())
            for depth in range(n):
                open_vars = np.flatnonzero(dom[:, 0] != dom[:, 1])
                if len(open_vars) == 0:
                    break
                v = int(rng.choice(open_vars))
                # bounds fail more often than interior values: try both kinds
                val = int(dom[v, 0]) if rng.integers(3) == 0 else int(rng.integers(dom[v, 0], dom[v, 1] + 1))
                st, out = orc.instance(dom, v, val, val)
                want = orc.bumps()
                g_st, g_props, g_bumps = gm.propagate_one_chain(dom, v, val, val)
                assert (g_st < 0) == (st < 0), (text[:20], walk, depth, v, val)
                assert g_props == orc.props(), (text[:20], walk, depth, v, val, g_props, orc.props())
                assert g_bumps.tolist() == want.tolist(), (text[:20], walk, depth, v, val, g_bumps.tolist(), want.tolist())
                if st < 0:
                    checked_fail += 1
                    with_chain += len(want) > 1
                    break
                checked_ok += 1
                dom = out
    assert checked_fail >= 40 and checked_ok >= 200 and with_chain >= 8, (checked_fail, checked_ok, with_chain)
