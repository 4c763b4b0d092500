"""Kernel 7 restated in plain Python/numpy, operation for operation and in the kernel's order.

cs_shave_core::fixpoint (csolve_amd/csrc/cs_shave.hip.h) and the node prologue of cs_propagate_ne_shave decide more than
the fixpoint: `revisions`, `rounds`, the failing variable and a failing node's `props` depend on the ORDER in which
PUSH and VERIFY operations are made.  This module is that order, written down once, for
tests/test_gpu_shave_order.py to hold the kernel against.  It works on absolute values (the kernel's root-relative
bounds and its table bytes are an encoding of the same numbers).

The relation: a clause `a != b + d` says "a = c forbids b = c - d" and "b = c forbids a = c + d".  The k-th clause of
a pair (in the order of the problem text) is the pair's slot k, as in the dense table of cs_device.c.
"""
from __future__ import annotations

import re

import numpy as np

_TERM = re.compile(r"^\s*([A-Za-z_]\w*)\s*(?:([+-])\s*(\d+))?\s*$")


class Network:
    """A pure binary != network read from problem text: variables in order of first appearance, per ordered pair and
    slot the offset `off[u, k, w]` with "u = c forbids w = c - off" where `has[u, k, w]`, and deg[v] = clauses on v."""

    def __init__(self, text: str):
        self.names, index = [], {}
        lo, hi, clauses = {}, {}, []

        def var(name):
            if name not in index:
                index[name] = len(self.names)
                self.names.append(name)
            return index[name]

        def term(s):
            m = _TERM.match(s)
            assert m, s
            k = int(m.group(3) or 0)
            return var(m.group(1)), (-k if m.group(2) == "-" else k)

        body = "\n".join(line.split("#")[0] for line in text.splitlines())
        for stmt in body.split(";"):
            stmt = stmt.strip()
            if not stmt or stmt in ("ANY", "ALL"):
                continue
            if stmt.startswith("all_different"):
                terms = [term(t) for t in stmt[stmt.index("(") + 1:stmt.rindex(")")].split(",")]
                # a + ka != b + kb  <=>  a != b + (kb - ka); a pair occurs once per all_different
                for i in range(len(terms)):
                    for j in range(i):
                        clauses.append((terms[i][0], terms[j][0], terms[j][1] - terms[i][1]))
            elif "!=" in stmt:
                left, right = stmt.split("!=")
                (a, ka), (b, kb) = term(left), term(right)
                clauses.append((a, b, kb - ka))
            else:
                left, right = stmt.split("<=")
                if re.match(r"^\s*-?\d+\s*$", left):
                    lo[var(right.strip())] = int(left)
                else:
                    hi[var(left.strip())] = int(right)
        n = self.n = len(self.names)
        self.domains = np.array([[lo[v], hi[v]] for v in range(n)], dtype=np.int64)
        count = {}
        for a, b, _ in clauses:
            assert a != b
            count[(min(a, b), max(a, b))] = count.get((min(a, b), max(a, b)), 0) + 1
        self.slots = max(count.values())
        self.off = np.zeros((n, self.slots, n), dtype=np.int64)
        self.has = np.zeros((n, self.slots, n), dtype=bool)
        self.deg = np.zeros(n, dtype=np.int64)
        at = {}
        for a, b, d in clauses:
            key = (min(a, b), max(a, b))
            k = at.get(key, 0)
            at[key] = k + 1
            self.off[a, k, b], self.has[a, k, b] = d, True
            self.off[b, k, a], self.has[b, k, a] = -d, True
            self.deg[a] += 1
            self.deg[b] += 1


class Outcome:
    """what kernel 7 returns for a node, and what the node went through (the classes the test wants to see)"""
    __slots__ = ("status", "props", "revisions", "rounds", "state", "sweeps", "fail_phase", "longest_walk")

    @property
    def result(self):
        return (self.status, self.props, self.revisions, self.rounds)


def node(net: Network, parent: np.ndarray, var: int, nlo: int, nhi: int) -> Outcome:
    """one node: the parent's intervals [n, 2], the assignment var in [nlo, nhi] (var < 0: propagate everything)"""
    off, has, deg = net.off, net.has, net.deg
    lo, hi = parent[:, 0].astype(np.int64), parent[:, 1].astype(np.int64)
    out = Outcome()
    out.sweeps, out.fail_phase, out.longest_walk = 0, None, 0
    # ---- the node prologue: who has pushed already, the assignment, what is to be verified
    pushed = np.zeros(net.n, dtype=bool) if var < 0 else lo == hi
    dl, dh = np.zeros(net.n, dtype=bool), np.zeros(net.n, dtype=bool)
    if var >= 0:
        lo[var], hi[var] = nlo, nhi
        pushed[var] = False
        if nlo != nhi:
            dl[var] = dh[var] = True
    lo0, hi0 = lo.copy(), hi.copy()
    val = lo == hi
    push = val & ~pushed
    rounds = revisions = 0

    def push_var(u, c):
        nonlocal revisions, lo, hi
        revisions += int(deg[u])
        plo, phi = lo.copy(), hi.copy()
        for k in range(net.slots):  # one slot after the other, on the bounds as they stand
            f = c - off[u, k]
            lo = lo + ((lo == f) & has[u, k])
            hi = hi - ((hi == f) & has[u, k])
        dl[:] |= lo != plo
        dh[:] |= hi != phi

    def push_all(who):
        value = lo.copy()  # a pusher's value is the one it had when the phase began
        pushed[:] |= who
        for u in np.nonzero(who)[0]:
            push_var(u, value[u])

    def settle():
        nonlocal val
        crossed = np.nonzero(lo > hi)[0]
        val = lo == hi
        return int(crossed[0]) if len(crossed) else -1  # lowest register, lowest lane

    def forbidden(w, c):
        """does a valued variable forbid w = c?  (u = x forbids w = x - off[u, k, w])"""
        return bool((has[:, :, w] & (lo[:, None] - off[:, :, w] == c) & val[:, None]).any())

    def done(fail_v, phase=None):
        out.fail_phase = phase
        out.status = -1 if fail_v >= 0 else int((lo != hi).sum())
        out.props = int(((lo - lo0) + (hi0 - hi)).sum())
        out.revisions = revisions
        out.rounds = fail_v if fail_v >= 0 else rounds
        out.state = np.stack([lo, hi], 1)
        return out

    while True:
        # (1) PUSH, ascending
        push_all(push)
        fail_v = settle()
        if fail_v >= 0:
            return done(fail_v, "push")
        # (2a) sweeps while more bounds are dirty than variables are values
        while int((dl | dh).sum()) > int(val.sum()):
            out.sweeps += 1
            dl[:] = False
            dh[:] = False
            push_all(val.copy())
            fail_v = settle()
            if fail_v >= 0:
                return done(fail_v, "push")
        # (2) VERIFY: lower bounds, then upper bounds, ascending; the failure is noted after the loops
        fail_v = -1
        for side in (0, 1):
            todo = np.nonzero(dl if side == 0 else dh)[0]
            (dl if side == 0 else dh)[:] = False
            sign = 1 if side == 0 else -1
            for w in todo:
                cand = int(lo[w] if side == 0 else hi[w])
                revisions += int(deg[w])
                if not forbidden(w, cand):
                    continue
                other = int(hi[w] if side == 0 else lo[w])
                step = 0
                while True:  # one value at a time
                    step += 1
                    if (cand + step > other) if side == 0 else (cand - step < other):
                        break
                    if not forbidden(w, cand + sign * step):
                        break
                out.longest_walk = max(out.longest_walk, step)
                cand += sign * step
                if side == 0:
                    lo[w] = cand
                else:
                    hi[w] = cand
                if (cand > other) if side == 0 else (cand < other):
                    fail_v = int(w)
                if cand == other:
                    val[w] = True  # counts for the verifications that follow
        if fail_v >= 0:
            return done(fail_v, "verify")
        # (3) new values push next
        push = val & ~pushed
        if not push.any():
            return done(-1)
        rounds += 1


def run(net: Network, states: np.ndarray, nodes: np.ndarray):
    """every node of a batch -> (results [B, 4] int32, rows [B, n, 2] int32, the Outcomes)"""
    outs = [node(net, states[p], int(v), int(a), int(b)) for v, a, b, p in nodes]
    res = np.array([o.result for o in outs], dtype=np.int32).reshape(len(outs), 4)
    rows = np.stack([o.state for o in outs]).astype(np.int32)
    return res, rows, outs
