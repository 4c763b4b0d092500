"""Inputs of the batched-fixpoint tests: a catalogue entry's device model, its oracle, and seeded parent states and node
records.  Shared by tests/test_gpu_instantiations.py (plain launches) and tests/test_gpu_launch_modes.py (graph replay,
streams, device-counted batches)."""
import numpy as np


def model(entry, monkeypatch, objective="ANY"):
    from csolve_amd.solver import solve_root
    for k, v in entry.env.items():
        monkeypatch.setenv(k, v)
    return solve_root(entry.text(objective))


def oracle(text, model):
    from oracle.cs_oracle import Model as OModel, Oracle
    om = OModel.parse(text)
    om.set_domains(model.domains())
    om.index()
    return Oracle(om)


def walk_states(orc, root, rng, count=48, depth=6):
    """states at depths 0 .. depth of seeded oracle walks (value assignments to random open variables)"""
    states = [root]
    for _ in range(count):
        cur = root
        for _ in range(depth):
            open_vars = np.nonzero(cur[:, 0] < cur[:, 1])[0]
            if len(open_vars) == 0:
                break
            v = int(open_vars[rng.integers(len(open_vars))])
            val = int(rng.integers(cur[v, 0], cur[v, 1] + 1))
            st, out = orc.instance(cur, v, val, val)
            if st < 0:
                break
            cur = out
            states.append(cur)
    return np.ascontiguousarray(np.stack(states), dtype=np.int32)


def nodes(rng, states, count):
    """value, interval and full re-propagation (var = -1) nodes on seeded parents; parents repeat"""
    P, n, _ = states.shape
    parent = rng.integers(P, size=count)
    parent[1::5] = parent[0::5][: len(parent[1::5])]  # repeated parents next to each other
    nodes = np.zeros((count, 4), dtype=np.int32)
    nodes[:, 3] = parent
    keys = rng.random((count, n))
    keys[states[parent, :, 0] == states[parent, :, 1]] = -1.0
    var = keys.argmax(1)
    lo, hi = states[parent, var, 0].astype(np.int64), states[parent, var, 1].astype(np.int64)
    a = lo + (rng.random(count) * (hi - lo + 1)).astype(np.int64).clip(0, hi - lo)
    b = np.where(rng.random(count) < 0.25, a + (rng.random(count) * (hi - a + 1)).astype(np.int64).clip(0, hi - a), a)
    nodes[:, 0], nodes[:, 1], nodes[:, 2] = var, a, b
    nodes[rng.random(count) < 0.1, 0] = -1
    nodes[nodes[:, 0] == -1, 1:3] = 0
    return nodes
