"""Every kernel instantiation finalize can plan, against the oracle: for each shape of tests/kernel_catalogue.py the
plan finalize made (exact template-ids), then every planned kernel of the batched fixpoint through every entry point
it has, the single-node paths and the search step, on inputs from seeded oracle walks on the host."""
import zlib

import numpy as np
import pytest

import kernel_catalogue as cat
from fixpoint_inputs import model as _model, nodes as _nodes, oracle as _oracle, walk_states as _walk_states

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BATCHES = (1, 15, 16, 17, 63, 64, 65)
ORACLE_SAMPLE = 4096  # instances of the largest batch checked against the oracle (all of them against kernel 1)
SINGLE_NODES = 64     # value and interval nodes per single-node path


def _inputs(entry, model, n_big):
    """states and nodes of every batch of this entry, with the oracle's verdicts and fixpoints (small batches whole,
    the largest one on a seeded sample)"""
    orc = _oracle(entry.text(), model)
    rng = np.random.default_rng(zlib.crc32(entry.id.encode()))
    states = _walk_states(orc, model.domains(), rng)
    batches = [_nodes(rng, states, B) for B in BATCHES + (n_big,)]
    small = np.concatenate(batches[:-1])
    sample = np.sort(rng.choice(n_big, size=min(n_big, ORACLE_SAMPLE), replace=False))
    st, out, _ = orc.instances_nodes(states, np.concatenate([small, batches[-1][sample]]))
    return states, batches, sample, st, out


def _ids(entries):
    return [e.id for e in entries]


@pytest.mark.parametrize("entry", cat.ENTRIES, ids=_ids(cat.ENTRIES))
def test_plan(entry, monkeypatch):
    """finalize plans exactly the catalogued instantiations, and qualifies() says the same"""
    model = _model(entry, monkeypatch)
    plan = model.plan()
    assert {k: v for k, v in plan.items() if v is not None} == cat.PLANS[entry.id]
    fams = {1: "events", 2: "lds", 3: "bitset", 4: "regs0", 5: "packed", 6: "rounds", 7: "shave"}
    for k, fam in fams.items():
        assert model.qualifies(k) == (plan[fam] is not None), (k, fam)


def _kernels(model):
    return [k for k in (1, 2, 3, 4, 5, 6, 7) if model.qualifies(k)]


@pytest.mark.parametrize("entry", cat.ENTRIES, ids=_ids(cat.ENTRIES))
def test_batched_fixpoint(entry, monkeypatch):
    """every planned kernel of the batched fixpoint, every entry point (states, carried sets, sets-only), batches of
    1 .. 65 nodes and one that fills every CU's chunks, against the oracle: verdict, every bound, open count, PROPS"""
    model = _model(entry, monkeypatch)
    n, fw = model.n_vars, model.forbidden_words()
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_big = n_cus * 32 * 16 + 1
    states, batches, sample, st_all, exp_all = _inputs(entry, model, n_big)
    d_states = torch.from_numpy(states).cuda()
    # PROPS is the reference's count on pure != networks only: with a tree clause kernels 1 and 6 revise in their own
    # order (test_batch_vs_oracle_and_properties skips it on the schedule models for the same reason)
    props_exact = not entry.tree
    # rebuilt forbidden sets of the parents: the carried-set entry points start from them
    forb = None
    if fw:
        model.set_kernel(3)
        full = torch.stack([torch.full((len(states),), -1), torch.zeros(len(states)), torch.zeros(len(states)),
                            torch.arange(len(states))], 1).to(torch.int32).cuda()
        _, forb, r = model.propagate_fb(d_states, full)
        torch.cuda.synchronize()
        assert (r[:, 0] >= 0).all()

    def check(what, nodes, out, res, st, exp):
        out, res = out.cpu().numpy(), res.cpu().numpy()
        fail = st < 0
        assert ((res[:, 0] < 0) == fail).all(), (entry.id, what, np.nonzero((res[:, 0] < 0) != fail)[0][:8])
        bad = np.nonzero(~fail & (out != exp).any((1, 2)))[0]
        assert len(bad) == 0, (entry.id, what, nodes[bad[:4]].tolist())
        assert (res[~fail, 0] == (exp[~fail, :, 0] != exp[~fail, :, 1]).sum(1)).all(), (entry.id, what)
        if props_exact:
            assert (res[~fail, 1] == st[~fail]).all(), (entry.id, what)

    kernels = _kernels(model)
    assert 1 in kernels
    ran = set()
    for k in kernels:
        model.set_kernel(k)
        at = 0
        for i, B in enumerate(BATCHES):
            nodes = batches[i]
            st, exp = st_all[at:at + B], exp_all[at:at + B]
            at += B
            d_nodes = torch.from_numpy(nodes).cuda()
            out, res = model.propagate(d_states, d_nodes)
            torch.cuda.synchronize()
            check((k, B, "propagate"), nodes, out, res, st, exp)
            if k in (3, 4, 5):
                o, f, r = model.propagate_fb(d_states, d_nodes, forb_in=forb)
                torch.cuda.synchronize()
                check((k, B, "propagate_fb"), nodes, o, r, st, exp)
            if k == 4:
                sets_in = model.pack_sets(d_states)
                s_out, r_s = model.propagate_sets(sets_in, d_nodes)
                torch.cuda.synchronize()
                ok = r_s[:, 0] >= 0
                check((k, B, "propagate_sets"), nodes, model.unpack_sets(s_out.contiguous()), r_s, st, exp)
                assert torch.equal(s_out[ok], model.pack_sets(out[ok].contiguous())), (entry.id, k, B)
        ran.add(k)
    assert ran == set(kernels)

    # the largest batch: every instance against kernel 1, a seeded sample against the oracle, the carried sets of
    # kernels 3 / 4 / 5 against each other on the root-domain bits
    nodes = batches[-1]
    d_nodes = torch.from_numpy(nodes).cuda()
    st, exp = st_all[-len(sample):], exp_all[-len(sample):]
    model.set_kernel(1)
    o1, r1 = model.propagate(d_states, d_nodes)
    torch.cuda.synchronize()
    check((1, n_big, "propagate"), nodes[sample], o1[torch.from_numpy(sample).cuda()], r1[torch.from_numpy(sample).cuda()],
          st, exp)
    ok = r1[:, 0] >= 0
    sets = {}
    for k in kernels:
        if k == 1:
            continue
        model.set_kernel(k)
        entries = [("propagate", lambda: model.propagate(d_states, d_nodes))]
        if k in (3, 4, 5):
            entries.append(("propagate_fb", lambda: model.propagate_fb(d_states, d_nodes, forb_in=forb)))
        for what, run in entries:
            got = run()
            torch.cuda.synchronize()
            o, r = got[0], got[-1]
            assert torch.equal(r[:, 0] >= 0, ok), (entry.id, k, what)
            assert torch.equal(o[ok], o1[ok]), (entry.id, k, what)
            if props_exact:
                assert torch.equal(r[ok][:, :2], r1[ok][:, :2]), (entry.id, k, what)
            else:
                assert torch.equal(r[ok][:, 0], r1[ok][:, 0]), (entry.id, k, what)
            if what == "propagate_fb":
                sets[k] = got[1][ok]
    if sets:
        dom = model.domains()
        width = dom[:, 1].astype(np.int64) - dom[:, 0] + 1
        mask = np.zeros((n, fw), dtype=np.uint64)
        for q in range(fw):
            bits = np.clip(width - 64 * q, 0, 64)
            mask[:, q] = [np.uint64((1 << int(b)) - 1) if b < 64 else np.uint64(0xFFFFFFFFFFFFFFFF) for b in bits]
        d_mask = torch.from_numpy(mask.view(np.int64)).cuda()
        first = sets[min(sets)]
        for k in sets:
            assert torch.equal(first & d_mask, sets[k] & d_mask), (entry.id, k)


def _replay(state, node, trace, kinds):
    """apply a trail's bound moves in order to the node's parent with the assignment made: every move narrows;
    -> the replayed state and whether a failure record or an emptied domain ends it"""
    v, lo, hi = node
    dom = state.copy()
    dom[v] = (lo, hi)
    failed = False
    for var, kind, bound, _ in trace:
        assert kind in kinds and 0 <= var < len(dom), (var, kind)
        if kind == 2:
            failed = True
        elif kind == 0:
            assert bound > dom[var, 0], (var, kind, bound, dom[var].tolist())
            dom[var, 0] = bound
        else:
            assert bound < dom[var, 1], (var, kind, bound, dom[var].tolist())
            dom[var, 1] = bound
    return dom, failed or bool((dom[:, 0] > dom[:, 1]).any())


@pytest.mark.parametrize("entry", cat.ENTRIES, ids=_ids(cat.ENTRIES))
def test_single_node(entry, monkeypatch):
    """64 value and interval nodes each through propagate_one (the resident server, which must answer every call, and
    with CSGPU_SERVER=0 one launch), propagate_one_traced (the general kernel's tracing variant) and
    propagate_one_causes (through the server, and without it kernel 7's tracing variant) against the oracle: verdict,
    fixpoint, open count, PROPS; the trails replay to the fixpoint"""
    for server in ("1", "0"):
        monkeypatch.setenv("CSGPU_SERVER", server)
        model = _model(entry, monkeypatch)
        plan = model.plan()
        causes = plan["server"] if server == "1" else plan["shave_trace"]
        orc = _oracle(entry.text(), model)
        rng = np.random.default_rng(17)
        states = _walk_states(orc, model.domains(), rng, count=16)
        nodes = _nodes(rng, states, 2 * SINGLE_NODES)
        nodes = nodes[nodes[:, 0] >= 0][:SINGLE_NODES]
        assert len(nodes) == SINGLE_NODES
        for v, lo, hi, p in nodes:
            node = (int(v), int(lo), int(hi))
            where = (entry.id, server, node)
            st, exp = orc.instance(states[p], *node)
            got, props, out = model.propagate_one(states[p], *node)
            assert (got < 0) == (st < 0), where
            if st >= 0:
                assert (out == exp).all() and got == int((exp[:, 0] != exp[:, 1]).sum()), where
                assert entry.tree or props == st, where
            if server == "1":
                got, props, out, trace = model.propagate_one_traced(states[p], *node)
                replayed, failed = _replay(states[p], node, trace, (0, 1, 2))
                assert (got < 0) == (st < 0) == failed, where + ("traced",)
                if st >= 0:
                    assert (out == exp).all() and (replayed == exp).all(), where + ("traced",)
                    assert entry.tree or props == st, where + ("traced",)
            if causes:
                got, props, out, trace = model.propagate_one_causes(states[p], *node)
                replayed, failed = _replay(states[p], node, trace, (0, 1))
                assert (got < 0) == (st < 0) == failed, where + ("causes",)
                if st >= 0:
                    assert (out == exp).all() and (replayed == exp).all() and props == st, where + ("causes",)
        if server == "1" and plan["server"]:  # the server answered every call: no silent fall-back to a launch
            calls, starts = model.server_stats()
            assert calls == 2 * len(nodes) and starts >= 1, (entry.id, calls, starts)
        model.close()


SEARCH = [e for e in cat.ENTRIES if e.search]


@pytest.mark.parametrize("entry", SEARCH, ids=_ids(SEARCH))
def test_search_steps(entry, monkeypatch):
    """the whole ALL tree through the planned step kernel: nodes, cuts, solutions and props of the host walk"""
    from csolve_amd.solver import Search
    from test_gpu_search import oracle_all_tree
    monkeypatch.delenv("CSGPU_SEARCH_FUSED", raising=False)  # ALL on a model with a step kernel takes it
    monkeypatch.delenv("CSGPU_SEARCH_EVAL", raising=False)
    model = _model(entry, monkeypatch, "ALL")
    plan = model.plan()
    assert plan["step_packed"] or plan["step_shave"], entry.id
    s = Search(model, 1 << 16, 1 << 12)
    s.put(model.root_state())
    st = s.run(1 << 40)
    assert st["done"] == 1 and st["pool"] == 0
    calls, cuts, sols, props = oracle_all_tree(entry.text("ALL"), model.domains(), max_calls=400000)
    assert (st["nodes"], st["cuts"], st["solutions"], st["props"]) == (calls, cuts, sols, props), entry.id
