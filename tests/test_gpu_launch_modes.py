"""The batched fixpoint launched the ways its callers launch it, against the oracle: captured into a hipGraph and
replayed (A), on several streams of one model (B), and with the batch counted on the device (C).
tests/test_gpu_instantiations.py holds every instantiation against the oracle on plain launches of a batch the host
knows; here a small named subset of the catalogue, which reaches all seven kernel families, goes through the other three.

Reference: the CPU oracle (oracle/cs_oracle.py, instances_nodes), bit for bit -- verdict, every bound of every consistent
node, the open count, and PROPS on pure != networks.  Batches larger than ORACLE_SAMPLE are held against the oracle on a
seeded sample of rows (every row below 128 and the rows next to every size and count used here among them), and on ALL
rows against one plain launch of kernel 1 on the same nodes, which is itself held against the oracle on that sample.

Every output buffer is filled with a poison pattern before the launches that write it.  A row the kernel never wrote
shows as poison: in the result row of any node, or in the state row of a consistent one (an inconsistent node stores no
state).  Rows at or past a device count must still hold the poison afterwards.

Sizes.  Kernel 7 draws chunks of `csz` nodes from ticket counters: chunk c belongs to shard c mod S (S = min(grid, 64)), a
shard with more chunks than waves is dynamic (first chunk static, the others by ticket), the others use static shares
(cs_shave.hip.h).  csgpu_internal_shave_launch reports the launcher's grid, waves per workgroup and csz; with W = grid x
waves, the node counts here give 1, W - 1, W, W + 1, W + S + 1 and 2 W + 3 chunks, the last chunk full and one node short,
and n_cus * 32 * 16 + 1 nodes: launches with no dynamic shard, with some, and with all (asserted below).

Why poison finds a counter that was not reset.  A dynamic shard of count_x chunks and waves_x waves draws exactly count_x
tickets per launch (count_x - waves_x name chunks, and every wave draws one past the end and stops), and the wave that
draws ticket count_x - 1 stores 0.  Without that store the counter stands at count_x when the next launch of the same
counter block starts: its first ticket is count_x, the chunk index waves_x + count_x is past the end, so every wave stops
after its static chunk and the count_x - waves_x chunks that only a ticket names are never computed.  Nothing spins; the
rows of those chunks keep the poison.  In a graph every captured launch has a counter block of its own, so replay k + 1 of
a launch meets what replay k of the same launch left: with the reset removed, test_graph_replay fails at the second
replay for every kernel-7 entry, because each entry's sizes include launches whose shards are all dynamic.

Safety of the inputs: every node record in device memory names a parent row that exists and a variable in range (or -1),
also the records past a device count; poison goes into output buffers only."""
import ctypes as C
import functools
import types
import zlib

import numpy as np
import pytest

import fixpoint_inputs as fx
import kernel_catalogue as cat

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ORACLE_SAMPLE = 4096       # rows of an entry's nodes checked against the oracle (all of them against kernel 1)
POISON = -0x5A5A5A5B       # 0xA5A5A5A5 as int32: no status, count or bound of these models
POISON64 = -0x5A5A5A5A5A5A5A5B
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
OTHER_SIZES = (1, 17, 65)  # and the large batch: kernels 1 to 6

# ---- the subset of the catalogue: (entry, kernel) ----
SHAVE = ("dense-n40-e8-s1-f1", "dense-n100-e8-s1-f1", "dense-n150-e8-s1-f1",      # 8-bit table, R = 1, 2, 4
         "dense-n40-e16-s1-f1", "dense-n100-e16-s1-f1", "dense-n150-e16-s1-f1",   # 16-bit table, R = 1, 2, 4
         "dense-n64-e8-s1-f1")                                                    # FULL
SHAVE_R1, SHAVE_R2 = "dense-n40-e8-s1-f1", "dense-n100-e16-s1-f1"  # the two entries of A2, B1
SMALL = "n16"                # kernels 2, 3, 4 and 5 are all planned on it
FULL = "dense-n64-e8-s1-f1"  # kernel 4's FAST variants (carried sets, sets only) run on FULL models only
TREE = "cpl-n40-d2-tree"     # a clause that stays an expression tree: kernels 1 and 6
CASES = [(e, 7) for e in SHAVE] + [(SMALL, k) for k in (2, 3, 4, 5)] + [(FULL, 4), (TREE, 1), (TREE, 6)]
ENTRY_IDS = tuple(dict.fromkeys(e for e, _ in CASES))
FAMILY = {1: "events", 2: "lds", 3: "bitset", 4: "regs0", 5: "packed", 6: "rounds", 7: "shave"}


def _case_ids(cases):
    return [f"{e}-k{k}" for e, k in cases]


def _new_model(entry_id):
    entry = cat.BY_ID[entry_id]
    assert not entry.env, "the entries here are planned without measurement switches"
    return fx.model(entry, None)


def _geometry(model, batch):
    """(workgroups, waves per workgroup, nodes per chunk) of a kernel-7 launch of `batch` nodes"""
    from csolve_amd import _lib
    out = (C.c_int64 * 3)()
    _lib.check(_lib.load_library().csgpu_internal_shave_launch(model._h, int(batch), C.byref(out)))
    return int(out[0]), int(out[1]), int(out[2])


def _batches_of_chunks(model, target):
    """the batch sizes the launcher cuts into exactly `target` chunks: the last chunk full, and one node short"""
    found = set()
    for csz in (4, 2, 1):
        for short in (0, 1):
            b = target * csz - short
            if b >= 1:
                _, _, c = _geometry(model, b)
                if c == csz and -(-b // c) == target:
                    found.add(b)
    assert found, target
    return sorted(found)


def _dynamic_shards(grid, waves, chunks):
    """(dynamic shards, shards) of a launch, by the rule of cs_shave.hip.h: a shard draws tickets when it has more
    chunks than waves"""
    S = min(grid, 64)
    dyn = 0
    for s in range(S):
        count_x = (chunks - 1 - s) // S + 1 if chunks > s else 0
        waves_x = ((grid - 1 - s) // S + 1) * waves
        dyn += count_x > waves_x
    return dyn, S


def _chunk_targets(grid, waves):
    W, S = grid * waves, min(grid, 64)
    return (1, W - 1, W, W + 1, W + S + 1, 2 * W + 3)


@functools.lru_cache(maxsize=None)
def _reference(entry_id):
    """parent states and n_big node records of an entry, computed once and never changed: the oracle on the sampled rows,
    a plain kernel-1 launch on all rows (held against the oracle here), the rebuilt forbidden sets of the parents, and for
    a kernel-7 entry the batch sizes and device counts around its chunk edges"""
    entry = cat.BY_ID[entry_id]
    model = _new_model(entry_id)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_big = n_cus * 32 * 16 + 1
    ref = types.SimpleNamespace(id=entry_id, n=model.n_vars, n_big=n_big, props_exact=not entry.tree,
                                fw=model.forbidden_words(), sizes=OTHER_SIZES + (n_big,),
                                counts=(0, 1, 15, 16, 17, 65, n_big - 1, n_big, n_big + 5))
    if model.qualifies(7):
        grid, waves, csz = _geometry(model, n_big)
        targets = _chunk_targets(grid, waves)
        sizes = [b for t in targets for b in _batches_of_chunks(model, t)]
        assert max(sizes) < n_big and all(_geometry(model, b)[0] == grid for b in sizes if b >= (grid * waves - 1))
        ref.sizes = tuple(sorted(set(sizes))) + (n_big,)
        # what the launches of these sizes are: without a dynamic shard, with some, with all
        ref.kind = {}
        for b in ref.sizes:
            g, w, c = _geometry(model, b)
            dyn, S = _dynamic_shards(g, w, -(-b // c))
            ref.kind[b] = "none" if dyn == 0 else "all" if dyn == S else "some"
        assert set(ref.kind.values()) == {"none", "some", "all"}, (entry_id, ref.kind)
        # device counts under the host bound n_big: the same chunk edges in chunks of the bound's csz
        edges = sorted({t * csz - short for t in targets for short in range(2 if csz > 1 else 1)})
        assert edges[-1] < n_big - 1
        ref.counts = tuple(sorted({0, 1, 15, 16, 17, *edges, n_big - 1, n_big, n_big + 5}))
        ref.geometry = (grid, waves, csz)
        ref.two_w = _batches_of_chunks(model, 2 * grid * waves)[-1]
    orc = fx.oracle(entry.text(), model)
    rng = np.random.default_rng(zlib.crc32(entry_id.encode()) ^ 0x4C4D)
    ref.states = fx.walk_states(orc, model.domains(), rng)
    ref.nodes = fx.nodes(rng, ref.states, n_big)
    assert ((ref.nodes[:, 3] >= 0) & (ref.nodes[:, 3] < len(ref.states))).all()
    assert ((ref.nodes[:, 0] >= -1) & (ref.nodes[:, 0] < ref.n)).all()
    near = {r for e in ref.sizes + ref.counts + (n_big // 2,) for r in (e - 2, e - 1, e) if 0 <= r < n_big}
    fixed = np.array(sorted(set(range(min(128, n_big))) | near))
    rest = np.setdiff1d(np.arange(n_big), fixed)
    ref.sample = np.sort(np.concatenate([fixed, rng.choice(rest, size=ORACLE_SAMPLE - len(fixed), replace=False)]))
    ref.st, ref.exp, _ = orc.instances_nodes(ref.states, ref.nodes[ref.sample])
    ref.d_states = torch.from_numpy(ref.states).cuda()
    ref.d_nodes = torch.from_numpy(ref.nodes).cuda()
    model.set_kernel(1)
    ref.out, ref.res = model.propagate(ref.d_states, ref.d_nodes)
    torch.cuda.synchronize()
    _verify(ref, "kernel 1, plain", ref.out, ref.res, 0, n_big)
    ref.forb = None
    if ref.fw:  # rebuilt forbidden sets of the parents: the carried-set entry points start from them
        P = len(ref.states)
        model.set_kernel(3)
        full = torch.stack([torch.full((P,), -1), torch.zeros(P), torch.zeros(P), torch.arange(P)], 1).to(torch.int32).cuda()
        _, ref.forb, r = model.propagate_fb(ref.d_states, full)
        torch.cuda.synchronize()
        assert (r[:, 0] >= 0).all()
    model.close()
    return ref


def _verify(ref, what, out, res, first, count, total=None, forb=None):
    """out[i], res[i] for i < count are the fixpoint and result of node first + i: all rows against kernel 1, the sampled
    ones against the oracle, no poison in a result row or a consistent node's state (and carried sets); rows count ..
    total still hold the poison"""
    what = (ref.id, what, first, count)
    cols = 2 if ref.props_exact else 1  # with a tree clause kernels 1 and 6 revise in their own order: no PROPS there
    if count:
        r, r_ref = res[:count], ref.res[first:first + count]
        assert not bool((r == POISON).any()), what + ("poison in results", torch.nonzero((r == POISON).any(1))[:8].tolist())
        ok = r_ref[:, 0] >= 0
        assert torch.equal(r[:, 0] >= 0, ok), what
        same = (out[:count] == ref.out[first:first + count]).all(2).all(1)
        assert bool((same | ~ok).all()), what + (torch.nonzero(~same & ok)[:8].tolist(),)
        assert torch.equal(r[:, :cols][ok], r_ref[:, :cols][ok]), what
        if forb is not None:
            assert not bool(((forb[:count] == POISON64).all(2).all(1) & ok).any()), what + ("poison in sets",)
        a, z = np.searchsorted(ref.sample, (first, first + count))
        if z > a:
            idx = torch.from_numpy(ref.sample[a:z] - first).cuda()
            o, rr, st, exp = out[idx].cpu().numpy(), res[idx].cpu().numpy(), ref.st[a:z], ref.exp[a:z]
            fail = st < 0
            assert ((rr[:, 0] < 0) == fail).all(), what + (np.nonzero((rr[:, 0] < 0) != fail)[0][:8].tolist(),)
            bad = np.nonzero(~fail & (o != exp).any((1, 2)))[0]
            assert len(bad) == 0, what + (ref.nodes[ref.sample[a:z][bad[:4]]].tolist(),)
            assert (rr[~fail, 0] == (exp[~fail, :, 0] != exp[~fail, :, 1]).sum(1)).all(), what
            if ref.props_exact:
                assert (rr[~fail, 1] == st[~fail]).all(), what
    if total is not None and total > count:
        assert bool((res[count:total] == POISON).all()), what + ("results written past the count",)
        assert bool((out[count:total] == POISON).all()), what + ("states written past the count",)
        if forb is not None:
            assert bool((forb[count:total] == POISON64).all()), what + ("sets written past the count",)


class _Run:
    """one entry point of one kernel of a model on the reference's nodes: buffers, poison, launch, check"""

    def __init__(self, model, ref, kernel, how):
        self.model, self.ref, self.kernel, self.how = model, ref, kernel, how
        if how == "propagate_sets":
            self.sets_in = model.pack_sets(ref.d_states)

    def buffers(self, rows):
        n, fw = self.ref.n, self.ref.fw
        b = types.SimpleNamespace(rows=rows, res=torch.empty((rows, 4), dtype=torch.int32, device="cuda"), out=None, forb=None,
                                  sets=None)
        if self.how == "propagate_sets":
            b.sets = torch.empty((rows, n, fw), dtype=torch.int64, device="cuda")
        else:
            b.out = torch.empty((rows, n, 2), dtype=torch.int32, device="cuda")
        if self.how in ("propagate_fb", "fb"):
            b.forb = torch.empty((rows, n, fw), dtype=torch.int64, device="cuda")
        return self.poison(b)

    @staticmethod
    def poison(b):
        b.res.fill_(POISON)
        for t in (b.out,):
            if t is not None:
                t.fill_(POISON)
        for t in (b.forb, b.sets):
            if t is not None:
                t.fill_(POISON64)
        return b

    def launch(self, b, first=0, count=None, stream=None, d_count=None):
        """nodes first .. first + count into the buffers, on `stream` (None: the current one); d_count: the launch is
        sized for `count` and the device count decides (csgpu_internal_propagate_objdev / _fb)"""
        from csolve_amd import _lib
        from csolve_amd.solver import _stream_ptr
        m, ref = self.model, self.ref
        count = b.rows if count is None else count
        nodes = ref.d_nodes[first:first + count]
        assert count <= b.rows and first + count <= len(ref.d_nodes) and nodes.is_contiguous()
        if self.how == "propagate":
            m.propagate(ref.d_states, nodes, states_out=b.out[:count], results=b.res[:count], stream=stream)
        elif self.how == "propagate_fb":
            m.propagate_fb(ref.d_states, nodes, forb_in=ref.forb, states_out=b.out[:count], forb_out=b.forb[:count],
                           results=b.res[:count], stream=stream)
        elif self.how == "propagate_sets":
            m.propagate_sets(self.sets_in, nodes, sets_out=b.sets[:count], results=b.res[:count], stream=stream)
        elif self.how == "objdev":  # propagate plus d_batch: no incumbent, no bound
            _lib.check(_lib.load_library().csgpu_internal_propagate_objdev(
                m._h, ref.d_states.data_ptr(), nodes.data_ptr(), b.out.data_ptr(), b.res.data_ptr(), count,
                d_count.data_ptr(), INT32_MIN, INT32_MAX, None, 0, _stream_ptr(stream)))
        else:  # "fb": propagate_fb plus d_batch, the sets carried
            assert self.how == "fb"
            _lib.check(_lib.load_library().csgpu_internal_propagate_fb(
                m._h, ref.d_states.data_ptr(), ref.forb.data_ptr(), nodes.data_ptr(), b.out.data_ptr(), b.forb.data_ptr(),
                b.res.data_ptr(), count, d_count.data_ptr(), _stream_ptr(stream)))

    def check(self, what, b, first=0, count=None, total=None):
        count = b.rows if count is None else count
        out = b.out
        if self.how == "propagate_sets":  # a poisoned row unpacks to intervals that are no fixpoint of the reference
            out = self.model.unpack_sets(b.sets)
            torch.cuda.synchronize()
        _verify(self.ref, (self.kernel, self.how, what), out, b.res, first, count, total, b.forb)


def _entry_points(kernel):
    return ("propagate",) + (("propagate_fb",) if kernel in (3, 4, 5) else ()) + (("propagate_sets",) if kernel == 4 else ())


def _capture(side, launches):
    """one warm launch on the side stream, then `launches` captured on it into one graph: a chain, one stream"""
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launches[0]()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for launch in launches:
            launch()
    return graph


def test_subset_reaches_every_family():
    """the cases above launch all seven fixpoint families, kernel 7 at R = 1, 2 and 4 with 8-bit and with 16-bit table
    entries and once FULL, kernels 1 and 6 with a tree clause, kernel 4 with its FAST variants: from plan(), so that a
    later re-plan cannot empty a case"""
    import re
    plans = {}
    for e in ENTRY_IDS:
        model = _new_model(e)
        plans[e] = model.plan()
        for entry, k in CASES:
            if entry == e:
                assert model.qualifies(k) and plans[e][FAMILY[k]] is not None, (e, k)
        model.close()
    assert {k for _, k in CASES} == {1, 2, 3, 4, 5, 6, 7}
    shave = set()
    for e in SHAVE:
        m = re.fullmatch(r"cs_propagate_ne_shave<unsigned (char|short), (\d), \d, (true|false), false>", plans[e]["shave"])
        assert m, plans[e]["shave"]
        shave.add((m.group(1), int(m.group(2)), m.group(3) == "true"))
    assert {(t, r) for t, r, full in shave if not full} == {(t, r) for t in ("char", "short") for r in (1, 2, 4)}, shave
    assert any(full for _, _, full in shave), shave
    for e, r in ((SHAVE_R1, 1), (SHAVE_R2, 2)):
        assert f", {r}, 1, false, false>" in plans[e]["shave"], plans[e]["shave"]
    assert plans[TREE]["events"].startswith("cs_propagate_events<true,") and plans[TREE]["rounds"].endswith(", true>")
    assert plans[FULL]["regs1"].endswith("true, false>") and plans[FULL]["regs3"].endswith("true, true>")  # FAST
    assert all(plans[SMALL][f] is not None for f in ("lds", "bitset", "regs0", "regs2", "packed"))


# ---- A. graph capture and replay ----

@pytest.mark.parametrize("entry_id,kernel", CASES, ids=_case_ids(CASES))
def test_graph_replay(entry_id, kernel):
    """A1: every entry point of the kernel, three launches of different sizes per graph (all sizes of the entry, three at a
    time) into buffers of their own, replayed three times with the buffers poisoned before each replay: a counter that
    replay k left non-zero shows as poison after replay k + 1"""
    ref = _reference(entry_id)
    model = _new_model(entry_id)
    model.set_kernel(kernel)
    side = torch.cuda.Stream()
    sizes = list(ref.sizes if kernel == 7 else OTHER_SIZES + (ref.n_big,))
    groups = [sizes[i:i + 3] for i in range(0, len(sizes), 3)]
    if len(groups[-1]) < 3:  # the last group filled up with sizes of the one before
        groups[-1] = (groups[-1] + [s for s in sizes if s not in groups[-1]])[:3]
    assert all(len(set(g)) == 3 for g in groups), groups
    for how in _entry_points(kernel):
        run = _Run(model, ref, kernel, how)
        for group in groups:
            bufs = [run.buffers(b) for b in group]
            graph = _capture(side, [functools.partial(run.launch, b) for b in bufs])
            for replay in range(3):
                for b in bufs:
                    run.poison(b)
                torch.cuda.synchronize()
                graph.replay()
                torch.cuda.synchronize()
                for b in bufs:
                    run.check(("replay", replay, tuple(group)), b)
            del graph
    model.close()


@pytest.mark.parametrize("entry_id", (SHAVE_R1, SHAVE_R2))
def test_graph_replay_between_plain_launches(entry_id):
    """A2, kernel 7: a replay of the graph, a plain launch on the side stream the graph was captured on and one on the
    default stream with no host synchronisation between the three, then a second replay: all exact"""
    ref = _reference(entry_id)
    model = _new_model(entry_id)
    model.set_kernel(7)
    run = _Run(model, ref, 7, "propagate")
    side = torch.cuda.Stream()
    group = (ref.sizes[-3], ref.sizes[-2], ref.n_big)  # W + S + 1 and 2 W + 3 chunks, the large batch
    assert all(ref.kind[b] == "all" for b in group), ref.kind  # every shard draws tickets
    bufs = [run.buffers(b) for b in group]
    plain_side, plain_default = run.buffers(ref.sizes[-2]), run.buffers(ref.n_big)
    graph = _capture(side, [functools.partial(run.launch, b) for b in bufs])
    for b in bufs:
        run.poison(b)
    torch.cuda.synchronize()
    graph.replay()
    side.wait_stream(torch.cuda.current_stream())  # the graph's launches first; it is their counters the plain ones must not touch
    run.launch(plain_side, stream=side)
    run.launch(plain_default)
    torch.cuda.synchronize()
    for b in bufs + [plain_side, plain_default]:
        run.check("first replay and the plain launches", b)
    for b in bufs:
        run.poison(b)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for b in bufs:
        run.check("second replay", b)
    del graph
    model.close()


def test_graph_capture_past_the_reserve():
    """A3, kernel 7: 1,000 captured one-node launches take every counter block a model keeps for captured launches (960);
    the large batch captured after them runs without one, on static shares, and is still exact.  A model of its own."""
    ref = _reference(SHAVE_R1)
    model = _new_model(SHAVE_R1)
    model.set_kernel(7)
    run = _Run(model, ref, 7, "propagate")
    side = torch.cuda.Stream()
    small = run.buffers(1000)
    one = [types.SimpleNamespace(rows=1, out=small.out[i:i + 1], res=small.res[i:i + 1], forb=None, sets=None) for i in range(1000)]
    many = _capture(side, [functools.partial(run.launch, b, first=i) for i, b in enumerate(one)])
    big = run.buffers(ref.n_big)
    large = _capture(side, [functools.partial(run.launch, big)])
    for replay in range(2):
        run.poison(small)
        run.poison(big)
        torch.cuda.synchronize()
        many.replay()
        large.replay()
        torch.cuda.synchronize()
        run.check(("one node each", replay), small)
        run.check(("past the reserve", replay), big)
    del many, large
    model.close()


# ---- B. streams ----

@pytest.mark.parametrize("entry_id", (SHAVE_R1, SHAVE_R2))
def test_two_streams(entry_id):
    """B1, kernel 7: two side streams of one model, a large batch of different nodes on each, twice over with no host
    synchronisation in between"""
    ref = _reference(entry_id)
    model = _new_model(entry_id)
    model.set_kernel(7)
    run = _Run(model, ref, 7, "propagate")
    half = ref.n_big // 2
    grid, waves, csz = _geometry(model, half)
    assert _dynamic_shards(grid, waves, -(-half // csz)) == (min(grid, 64),) * 2  # every shard draws tickets
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    assert streams[0].cuda_stream != streams[1].cuda_stream
    bufs = [[run.buffers(half) for _ in streams] for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(2):
        for i, s in enumerate(streams):
            run.launch(bufs[rep][i], first=i * half, stream=s)
    torch.cuda.synchronize()
    for rep in range(2):
        for i in range(2):
            run.check(("stream", i, "launch", rep), bufs[rep][i], first=i * half)
    model.close()


def _hip():
    """the HIP runtime the process has loaded already"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
            lib.hipStreamDestroy.argtypes = [C.c_void_p]
            return lib
    raise AssertionError("no HIP runtime loaded")


def test_seventy_streams():
    """B2, kernel 7: seventy streams of one model, one launch of 2 W chunks of the same nodes on each, enqueued back to
    back.  A model keeps a counter block per stream for 64 streams; the launches on streams 65 to 70 get none and run on
    static shares, with the same results.  A model of its own, and streams of its own (torch hands out 32 per priority)."""
    ref = _reference(SHAVE_R1)
    model = _new_model(SHAVE_R1)
    model.set_kernel(7)
    run = _Run(model, ref, 7, "propagate")
    hip = _hip()
    handles = []
    try:
        for _ in range(70):
            h = C.c_void_p()
            assert hip.hipStreamCreate(C.byref(h)) == 0
            handles.append(h)
        assert len({h.value for h in handles}) == 70
        streams = [torch.cuda.ExternalStream(h.value) for h in handles]
        bufs = [run.buffers(ref.two_w) for _ in streams]
        torch.cuda.synchronize()
        for s, b in zip(streams, bufs):
            run.launch(b, stream=s)
        torch.cuda.synchronize()
        for i, b in enumerate(bufs):
            run.check(("stream", i), b)
    finally:
        torch.cuda.synchronize()
        for h in handles:
            hip.hipStreamDestroy(h)
        model.close()


# ---- C. device-counted batches ----

# kernels 1, 6 and 7 and, with the sets rebuilt, 3, 4 and 5 through csgpu_internal_propagate_objdev; the carried sets of
# 3, 4 and 5 through csgpu_internal_propagate_fb
COUNTED = [(e, k, "objdev") for e, k in CASES if k != 2] + [(SMALL, k, "fb") for k in (3, 4, 5)] + [(FULL, 4, "fb")]


def _device_counts(model, ref, kernel, how):
    """every count of the entry under the host bound n_big, each followed by a second launch into the same buffers with
    another count and nothing cleared in between (the poison included): rows below the count are the oracle's, rows at or
    past the larger of the two counts still hold the poison"""
    run = _Run(model, ref, kernel, how)
    B = ref.n_big
    b = run.buffers(B)
    counts = ref.counts
    for i, c in enumerate(counts):
        c2 = counts[(i + len(counts) // 2) % len(counts)]  # a larger one for the first half, a smaller one for the rest
        d_count = torch.tensor([c, c2], dtype=torch.int64, device="cuda")
        run.poison(b)
        torch.cuda.synchronize()
        run.launch(b, count=B, d_count=d_count[0:])
        torch.cuda.synchronize()
        run.check(("count", c), b, count=min(c, B), total=B)
        run.launch(b, count=B, d_count=d_count[1:])
        torch.cuda.synchronize()
        run.check(("count", c, "then", c2), b, count=min(max(c, c2), B), total=B)


@pytest.mark.parametrize("entry_id,kernel,how", COUNTED, ids=[f"{e}-k{k}-{h}" for e, k, h in COUNTED])
def test_device_count(entry_id, kernel, how):
    """the launch is sized for the host's bound (the large batch, all of its records valid) and clamps to a uint64 count
    in device memory: 0, 1, 15, 16, 17, for kernel 7 the counts at its six chunk edges (in chunks of the bound's csz, the
    last chunk full and one node short), bound - 1, bound, and bound + 5, which clamps to the bound"""
    ref = _reference(entry_id)
    model = _new_model(entry_id)
    model.set_kernel(kernel)
    assert model.kernel() == kernel
    _device_counts(model, ref, kernel, how)
    model.close()


def test_device_count_kernel_2_falls_through():
    """kernel 2 takes no device count: with set_kernel(2) and a d_batch the launcher falls through to the general
    kernels (1, or 6 where the model is left to choose), and the results are exact all the same"""
    ref = _reference(SMALL)
    model = _new_model(SMALL)
    model.set_kernel(2)
    assert model.kernel() == 2
    _device_counts(model, ref, 2, "objdev")
    model.close()
