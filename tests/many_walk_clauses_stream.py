"""What csgpu_solve_many_clauses_stream is specified to compute (include/csolve_gpu.h), on the host with the oracle for
every node (a helper module of the solve_many_clauses_stream tests, no test itself).

Walk(text, root_row) is many_walk_clauses_upto.Walk -- the ALL walk of the clause model, "<obj>" an ordinary variable --
with run_stream(budget, room): run(budget, None) where a child that is a solution first asks room() for a row.  Refused,
the walk steps back: no counter has moved, the walk stands before that very value again and the status is FULL.

Call is the call itself on a list of instances: the stream (a count that the call only adds to, a capacity, the rows in
the order they were appended), the slot entry of every instance (-2 fresh, -1 finished, >= 0 a checkpoint) and its
record.  call(order, budget) serves the instances in `order`, which stands for the order the waves arrive in; one that
arrives when the stream is full already does not walk.  drain() takes the rows and zeroes the count."""
import many_walk_clauses_upto as U
from many_walk import BAD_ROOT, DONE, LIMIT  # noqa: F401

FULL, FRESH = 4, -2
FIELDS = ("status", "root_props", "nodes", "cuts", "props", "solutions")
ZERO = dict(status=FULL, root_props=0, nodes=0, cuts=0, props=0, solutions=0)


class Walk(U.Walk):
    def run_stream(self, budget, room):
        """at most `budget` more children; every solution asks room() first -> the counters so far (status FULL: a solution
        found no room and is not counted; LIMIT: stopped at the budget with work left)"""
        assert budget > 0
        out = self.out
        if not self.open:
            return self.result()
        out["status"] = DONE
        tried = 0
        while True:
            if tried >= budget:
                out["status"] = LIMIT
                return self.result()
            cur, v = self.cur, self.v
            value, last = self.nv, self.nv == cur[v, 1]
            status, child = self.orc.instance(cur, v, value, value)
            solved = status >= 0 and bool((child[:, 0] == child[:, 1]).all())
            if solved and not room():
                out["status"] = FULL  # nothing has moved: the next run tries `value` again
                return self.result()
            out["nodes"] += 1
            tried += 1
            descend = False
            if status < 0:
                out["cuts"] += 1
            else:
                out["props"] += status
                if solved:
                    out["solutions"] += 1
                    self.rows.append(child[:, 0].copy())
                else:
                    descend = True
            if descend:
                if not last:
                    self.stack.append((cur, v, value + 1))
                self.cur = child
                self.v, self.nv = self._branch(child)
            elif last:
                if not self.stack:
                    break
                self.cur, self.v, self.nv = self.stack.pop()
            else:
                self.nv = value + 1
        self.open = False
        return self.result()


class Call:
    def __init__(self, text, roots, capacity, pool=None):
        self.text, self.roots, self.capacity = text, roots, capacity
        K = len(roots)
        self.slots = [FRESH] * K
        self.records = [dict(ZERO, status=DONE) for _ in range(K)]
        self.walks = [None] * K
        self.pool = K if pool is None else pool  # slots the pool has left
        self.count, self.rows = 0, []

    def _room(self):
        self.count += 1
        return self.count <= self.capacity

    def call(self, order, budget):
        for i in order:
            if self.slots[i] != FRESH and self.slots[i] < 0:
                continue  # finished: nothing of it is read or written
            if self.count >= self.capacity:  # full at the draw
                if self.slots[i] == FRESH:
                    self.records[i] = dict(ZERO)
                continue
            if self.slots[i] == FRESH:
                w = Walk(self.text, self.roots[i])
                if w.rows:  # the root node is itself the solution
                    if not self._room():
                        self.records[i] = dict(ZERO)
                        continue
                    self.rows.append((i, w.rows[0]))
                    res = w.result()
                elif w.open:
                    res = w.run_stream(budget, self._room)
                    self.rows.extend((i, r) for r in res["rows"])
                else:  # a bad root row, or an inconsistent root node
                    res = w.result()
            else:
                w = self.walks[i]
                had = len(w.rows)
                res = w.run_stream(budget, self._room)
                self.rows.extend((i, r) for r in res["rows"][had:])
            self.records[i] = {f: res[f] for f in FIELDS}
            if res["status"] in (LIMIT, FULL):
                if self.slots[i] == FRESH:
                    self.slots[i] = i if self.pool > 0 else -1  # a slot of its own, or its walk is gone
                    self.pool -= self.pool > 0
                self.walks[i] = w if self.slots[i] >= 0 else None
            else:
                self.slots[i], self.walks[i] = -1, None

    def drain(self):
        """-> [(owner, row)] in stream order, the valid part; the count is zeroed"""
        taken, self.rows, self.count = self.rows[: self.capacity], [], 0
        return taken

    def left(self):
        return any(s != -1 for s in self.slots)
