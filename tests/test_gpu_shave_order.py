"""Kernel 7 against tests/shave_order_model.py: all four result fields of EVERY node -- status, props, revisions and
rounds, for an inconsistent node the failing variable and the props it had made by then -- and the stored rows of the
consistent ones.  Those fields depend on the order of the PUSH and VERIFY operations, which no oracle comparison pins
(the fixpoint is unique, the way to it is not): a change of that order passes the parity tests and still changes what
a caller receives.

One model per template case of the kernel (R, FULL, compile-time and run-time slot loop); nodes from seeded walks the
model itself makes on the host, in two batch sizes: 1,027 (static shares, partial last chunk) and the same nodes tiled
to 65,539 (tickets, more chunks than waves, partial last chunk).
"""
import zlib

import numpy as np
import pytest

import shave_order_model as som
from csolve_amd import problems

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL, LARGE = 1027, 65539
WALKS = 12


def _sudoku16() -> str:
    """a 16x16 sudoku-shaped network: every pair of cells that shares a row, a column or a box, ONCE (one slot)"""
    box, n = 4, 16
    lines = ["# 16x16 sudoku-shaped != network, one clause per related pair", "ANY;"]
    for a in range(n * n):
        ra, ca = divmod(a, n)
        for b in range(a + 1, n * n):
            rb, cb = divmod(b, n)
            if ra == rb or ca == cb or (ra // box == rb // box and ca // box == cb // box):
                lines.append(f"C{a} != C{b} + 0;")
    for a in range(n * n):
        lines.append(f"1 <= C{a}; C{a} <= {n};")
    return "\n".join(lines) + "\n"


# id -> (problem text, the kernel-7 instantiation finalize must plan)
SHAPES = {
    "queens8": (lambda: problems.queens(8), "cs_propagate_ne_shave<unsigned char, 1, 3, false, false>"),
    "queens64": (lambda: problems.queens(64), "cs_propagate_ne_shave<unsigned char, 1, 3, true, false>"),
    "queens70": (lambda: problems.queens(70), "cs_propagate_ne_shave<unsigned char, 2, 3, false, false>"),
    "queens128": (lambda: problems.queens(128), "cs_propagate_ne_shave<unsigned char, 2, 3, true, false>"),
    "sudoku16": (_sudoku16, "cs_propagate_ne_shave<unsigned char, 4, 1, true, false>"),
    "sparse40x2": (lambda: problems.sparse_ne(40, degree=3, width=4, per_pair=2, offset_spread=3),
                   "cs_propagate_ne_shave<unsigned char, 1, 0, false, false>"),
}


def _pick(rng, net, state, interval, tight=False):
    """an assignment to a random open variable of `state`: a value (bounds preferred) or an interval inside (tight: of
    two or three values -- states of narrow domains are where one value sets off rounds of others)"""
    open_vars = np.nonzero(state[:, 0] < state[:, 1])[0]
    if len(open_vars) == 0:
        return None
    v = int(open_vars[rng.integers(len(open_vars))])
    lo, hi = int(state[v, 0]), int(state[v, 1])
    if interval and hi - lo >= 2:
        a = int(rng.integers(lo, hi))
        b = int(rng.integers(a + 1, min(hi, a + 2) + 1 if tight else hi + 1))
        if (a, b) == (lo, hi):
            a += 1
        return v, a, b
    c = int(rng.integers(lo, hi + 1)) if rng.random() < 0.5 else (lo if rng.random() < 0.5 else hi)
    return v, c, c


def _generate(net, root, rng):
    """parent states from seeded walks of the model (values and intervals, each walk until it fails or every variable
    is a value: the deep states are where bounds cascade), then SMALL nodes on them"""
    states = [root]
    for walk in range(WALKS):
        cur = root
        tight = walk % 2 == 1
        for _ in range(2 * net.n if tight else net.n):
            pick = _pick(rng, net, cur, rng.random() < (0.8 if tight else 0.3), tight)
            if pick is None:
                break
            o = som.node(net, cur, *pick)
            if o.status < 0:
                break
            cur = o.state
            states.append(cur)
    states = np.ascontiguousarray(np.stack(states), dtype=np.int32)
    nodes = []
    # by hand: everything propagated at the root and on a deep state, every root bound value assigned at the root
    # (the sweep case: a bound of every neighbour moves)
    nodes += [(-1, 0, 0, 0), (-1, 0, 0, len(states) - 1)]
    for v in range(min(net.n, 24)):
        nodes += [(v, int(root[v, 0]), int(root[v, 0]), 0), (v, int(root[v, 1]), int(root[v, 1]), 0)]
    while len(nodes) < SMALL:
        p = int(rng.integers(len(states)))
        if rng.random() < 0.06:
            nodes.append((-1, 0, 0, p))
            continue
        pick = _pick(rng, net, states[p], rng.random() < 0.25)
        if pick is not None:
            nodes.append(pick + (p,))
    return states, np.array(nodes[:SMALL], dtype=np.int32)


_CASES = {}


def _case(shape):
    """the shape's model on the device, its inputs and what the order model says of them: computed once, shared"""
    if shape not in _CASES:
        from csolve_amd.solver import solve_root
        make, planned = SHAPES[shape]
        text = make()
        model = solve_root(text)
        assert model.plan()["shave"] == planned, (shape, model.plan()["shave"])
        net = som.Network(text)
        assert net.names == model.var_names(), shape
        root = model.domains().astype(np.int64)
        assert (root == net.domains).all(), shape
        rng = np.random.default_rng(zlib.crc32(shape.encode()))
        states, nodes = _generate(net, root, rng)
        res, rows, outs = som.run(net, states, nodes)
        _CASES[shape] = (model, states, nodes, res, rows, outs)
    return _CASES[shape]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_classes_reached(shape):
    """the generated nodes of every shape go through each path whose order the test is there to pin"""
    _, states, nodes, res, _, outs = _case(shape)
    parents = states[nodes[:, 3]]
    var = nodes[:, 0]
    pv = np.where(var >= 0, var, 0)
    plo, phi = parents[np.arange(len(nodes)), pv, 0], parents[np.arange(len(nodes)), pv, 1]
    inside = (var >= 0) & (nodes[:, 1] < nodes[:, 2]) & ((nodes[:, 1] > plo) | (nodes[:, 2] < phi))
    at_root_bound = (var >= 0) & (nodes[:, 3] == 0) & (nodes[:, 1] == nodes[:, 2]) & ((nodes[:, 1] == plo) | (nodes[:, 1] == phi))
    reached = {
        "var < 0": bool((var < 0).any()),
        "interval inside a domain": bool(inside.any()),
        "root bound value at the root, swept": any(o.sweeps > 0 for o, m in zip(outs, at_root_bound) if m),
        "fails in the push phase": any(o.fail_phase == "push" for o in outs),
        "fails in VERIFY": any(o.fail_phase == "verify" for o in outs),
        "rounds >= 2": bool(((res[:, 0] >= 0) & (res[:, 3] >= 2)).any()),
        "a bound walks more than one value": any(o.longest_walk >= 2 for o in outs),
    }
    assert all(reached.values()), (shape, [k for k, v in reached.items() if not v])


@pytest.mark.parametrize("batch", [SMALL, LARGE])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_order(shape, batch):
    model, states, nodes, res, rows, _ = _case(shape)
    reps = -(-batch // SMALL)
    nodes_b = np.tile(nodes, (reps, 1))[:batch]
    exp_res = torch.from_numpy(np.tile(res, (reps, 1))[:batch]).cuda()
    d_rows = torch.from_numpy(rows).cuda()
    model.set_kernel(7)
    try:
        out, got = model.propagate(torch.from_numpy(states).cuda(), torch.from_numpy(np.ascontiguousarray(nodes_b)).cuda())
        torch.cuda.synchronize()
    finally:
        model.set_kernel(0)
    bad = torch.nonzero((got != exp_res).any(1)).flatten()[:4].cpu().numpy()
    assert len(bad) == 0, (shape, batch, [(int(i), nodes_b[i].tolist(), got[int(i)].tolist(), exp_res[int(i)].tolist()) for i in bad])
    ok = torch.nonzero(exp_res[:, 0] >= 0).flatten()
    exp_rows = d_rows[ok % SMALL]
    wrong = torch.nonzero((out[ok] != exp_rows).flatten(1).any(1)).flatten()[:4]
    assert len(wrong) == 0, (shape, batch, [nodes_b[int(ok[int(i)])].tolist() for i in wrong])
