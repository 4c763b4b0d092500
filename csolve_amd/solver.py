"""Thin Python view of the C ABI: problem models and batched propagation on torch
device buffers.  Mirrors the reference's operator vocabulary: a *model* (constraints +
variables), *states* (one interval per variable), *nodes* (an assignment applied to a
parent state), `propagate` (propagate_clauses for every node of a batch), `eval_root`.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools

import numpy as np
import torch

from ._lib import (MANY_ROTATE_FIRST, MANY_SLOT_FRESH, PLAN_FAMILIES, CsolveError, ManyOptions, ManyOrderOptions, ManyRestartOptions, ManyResult,
                   ManyStream, ManyUptoOptions, Node, Result, SearchStats, Val, check, demangle, load_library)

STATUS_FAIL = -1


def _stream_ptr(stream) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return int(stream.cuda_stream)


class Model:
    """A problem: host model + (after finalize) its device image."""

    def __init__(self, handle):
        self._h = handle
        self.finalized = False

    # ---- construction -----------------------------------------------------------------
    @classmethod
    def from_text(cls, text: str, weights_on: bool = True) -> "Model":
        L = load_library()
        h = C.c_void_p()
        check(L.csgpu_model_from_text(text.encode(), int(weights_on), C.byref(h)))
        return cls(h)

    @classmethod
    def from_file(cls, path: str, weights_on: bool = True) -> "Model":
        L = load_library()
        h = C.c_void_p()
        check(L.csgpu_model_from_file(path.encode(), int(weights_on), C.byref(h)))
        return cls(h)

    @classmethod
    def from_dump(cls, path: str) -> "Model":
        L = load_library()
        h = C.c_void_p()
        check(L.csgpu_model_from_dump(path.encode(), C.byref(h)))
        return cls(h)

    def close(self):
        if self._h:
            load_library().csgpu_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-side queries --------------------------------------------------------------
    @property
    def n_vars(self) -> int:
        return check(load_library().csgpu_model_num_vars(self._h))

    @property
    def n_clauses(self) -> int:
        return check(load_library().csgpu_model_num_clauses(self._h))

    @property
    def objective(self) -> int:
        return check(load_library().csgpu_model_objective(self._h))

    @property
    def objective_var(self) -> int:
        return load_library().csgpu_model_objective_var(self._h)

    def var_names(self):
        L = load_library()
        return [L.csgpu_model_var_name(self._h, i).decode() for i in range(self.n_vars)]

    def domains(self) -> np.ndarray:
        out = np.empty((self.n_vars, 2), dtype=np.int32)
        check(load_library().csgpu_model_get_domains(self._h, out.ctypes.data))
        return out

    def set_domains(self, dom: np.ndarray):
        dom = np.ascontiguousarray(dom, dtype=np.int32)
        assert dom.shape == (self.n_vars, 2)
        check(load_library().csgpu_model_set_domains(self._h, dom.ctypes.data))

    def device_info(self) -> dict:
        info = (C.c_int64 * 8)()
        check(load_library().csgpu_model_device_info(self._h, info))
        keys = ("adjacency_entries", "ne_clauses", "tree_clauses", "tree_nodes", "lds_bytes_per_node",
                "max_list", "skipped_clauses", "max_tree")
        return dict(zip(keys, [int(x) for x in info]))

    # ---- device phases ------------------------------------------------------------------
    def root_propagate(self) -> int:
        """propagate(root, size) on the device; -1 = infeasible, else narrowings."""
        st = C.c_int32()
        check(load_library().csgpu_model_root_propagate(self._h, C.byref(st)))
        return st.value

    def eval_clauses_host(self) -> np.ndarray:
        """eval_<op> of every clause on the current root domains (no finalize needed)."""
        out = np.empty((max(1, self.n_clauses), 2), dtype=np.int32)
        check(load_library().csgpu_model_eval_clauses_host(self._h, out.ctypes.data))
        return out[: self.n_clauses]

    def build_tables(self):
        """Host-only: clause lists + device tables in host memory (no HIP call)."""
        check(load_library().csgpu_model_build_tables(self._h))
        return self

    def normalize(self):
        """normalize(root): host-side rewrite of the trees between the two root propagations"""
        check(load_library().csgpu_model_normalize(self._h))
        return self

    def specialize(self, state, build_only: bool = False) -> "Model":
        """the model rewritten for the subtree below `state` ([n_vars][2] intervals inside the root
        domains): a copy with `state` as root domains, normalised (what the prefix has decided is folded away,
        normalize.c:67-316), propagated and finalized (entailed clauses leave the device tables).  Same results as
        this model for every state inside `state`; shorter clause lists.  build_only: host tables only (no GPU)."""
        state = np.ascontiguousarray(np.asarray(state.cpu() if hasattr(state, "cpu") else state), dtype=np.int32)
        state = state.reshape(-1, self.n_vars, 2)
        assert state.shape[0] == 1, "one state (a common prefix), not a batch"
        state = np.ascontiguousarray(state[0])
        h = C.c_void_p()
        check(load_library().csgpu_model_specialize(self._h, state.ctypes.data, C.byref(h)))
        m = Model(h)
        m.normalize()
        if build_only:
            return m.build_tables()
        if m.root_propagate() < 0:
            raise ValueError("INFEASIBLE PROBLEM")
        return m.finalize()

    def add_conflict(self, elems):
        """a learnt conflict clause "not all of var == value" for elems = [(var, value)] (csgpu_model_add_conflict)"""
        vs = np.ascontiguousarray([e[0] for e in elems], dtype=np.int32)
        cs = np.ascontiguousarray([e[1] for e in elems], dtype=np.int32)
        check(load_library().csgpu_model_add_conflict(self._h, len(elems), vs.ctypes.data, cs.ctypes.data))
        return self

    def finalize(self):
        check(load_library().csgpu_model_finalize(self._h))
        self.finalized = True
        return self

    def set_kernel(self, which: int):
        """0 automatic, 1 general kernel, 2 LDS-resident unit shaving, 3 forbidden sets in LDS,
        4 forbidden sets in registers, 5 the same with two or four nodes per wave, 6 clause-resident (small
        models), 7 interval-only shaving (2-5, 7: pure binary-NE models that fit, see csolve_gpu.h)"""
        check(load_library().csgpu_model_set_kernel(self._h, which))
        return self

    def qualifies(self, which: int) -> bool:
        return bool(load_library().csgpu_model_qualifies(self._h, which))

    def plan(self) -> dict:
        """The instantiation finalize planned for every kernel family (_lib.PLAN_FAMILIES): its template-id, read
        back from the launched kernel handle's dynamic symbol, or None where the family is not planned."""
        buf = C.create_string_buffer(1024)
        out = {}
        for i, fam in enumerate(PLAN_FAMILIES):
            check(load_library().csgpu_internal_plan_symbol(self._h, i, buf, len(buf)))
            out[fam] = demangle(buf.value.decode()) if buf.value else None
        return out

    def kernel(self) -> int:
        return check(load_library().csgpu_model_get_kernel(self._h))

    def root_state(self, device="cuda") -> torch.Tensor:
        """[1, n_vars, 2] int32 tensor of the root domains."""
        return torch.from_numpy(self.domains()).to(device).unsqueeze(0).contiguous()

    def propagate(self, states_in: torch.Tensor, nodes: torch.Tensor, states_out: torch.Tensor = None,
                  results: torch.Tensor = None, stream=None):
        """Batched propagate_clauses.

        states_in  [P, n_vars, 2] int32 (device)   parent states
        nodes      [B, 4] int32 (device)           rows (var, lo, hi, parent_row)
        returns (states_out [B, n_vars, 2], results [B, 4] = status, props, revisions, rounds)
        """
        n = self.n_vars
        assert states_in.is_cuda and nodes.is_cuda, "device tensors required"
        assert states_in.dtype == torch.int32 and nodes.dtype == torch.int32
        assert states_in.is_contiguous() and nodes.is_contiguous()
        assert states_in.shape[-2:] == (n, 2) and nodes.shape[-1] == 4
        B = nodes.shape[0]
        if states_out is None:
            states_out = torch.empty((B, n, 2), dtype=torch.int32, device=nodes.device)
        if results is None:
            results = torch.empty((B, 4), dtype=torch.int32, device=nodes.device)
        assert states_out.is_contiguous() and results.is_contiguous()
        assert states_out.shape == (B, n, 2) and results.shape == (B, 4)
        check(load_library().csgpu_propagate_batch(self._h, states_in.data_ptr(), nodes.data_ptr(),
                                                   states_out.data_ptr(), results.data_ptr(), B,
                                                   _stream_ptr(stream)))
        return states_out, results

    def propagate_obj(self, states_in: torch.Tensor, nodes: torch.Tensor, obj_lo: int, obj_hi: int, stream=None):
        """Batched propagate_clauses under an incumbent bound (csgpu_propagate_batch_obj): "<obj>" of every child is
        intersected with [obj_lo, obj_hi] before the child is propagated, and if that moved a bound the clauses of
        "<obj>" are propagated as well; (INT32_MIN, INT32_MAX) is no bound, and a model without an objective variable
        ignores both.  Tensors and return values as propagate()."""
        n = self.n_vars
        obj_lo, obj_hi = int(obj_lo), int(obj_hi)
        if not (-2**31 <= obj_lo <= 2**31 - 1 and -2**31 <= obj_hi <= 2**31 - 1):
            raise ValueError("obj_lo and obj_hi are int32 values")
        assert states_in.is_cuda and nodes.is_cuda, "device tensors required"
        assert states_in.dtype == torch.int32 and nodes.dtype == torch.int32
        assert states_in.is_contiguous() and nodes.is_contiguous()
        assert states_in.shape[-2:] == (n, 2) and nodes.shape[-1] == 4
        B = nodes.shape[0]
        states_out = torch.empty((B, n, 2), dtype=torch.int32, device=nodes.device)
        results = torch.empty((B, 4), dtype=torch.int32, device=nodes.device)
        check(load_library().csgpu_propagate_batch_obj(self._h, states_in.data_ptr(), nodes.data_ptr(),
                                                       states_out.data_ptr(), results.data_ptr(), B, obj_lo, obj_hi,
                                                       _stream_ptr(stream)))
        return states_out, results

    # ---- many instances of this model in one call (csgpu_solve_many) -------------------------------
    MANY_OBJECTIVES = {"ANY": 0, "ALL": 1, "MIN": 2, "MAX": 3}

    def _many_roots(self, roots, bad_option, probe, qualifies=None):
        """the root rows of a call of the solve_many family on the device -> (roots, K); a numpy array is uploaded.  On a
        model that is not finalized or not one of kernel 7 (`qualifies`: the entry's own rule instead), or with
        `bad_option`, probe(host pointer, K) makes the call itself first: the library says what is wrong before any
        device call (it touches no buffer), and nothing is uploaded for it"""
        n = self.n_vars
        if not torch.is_tensor(roots):
            roots = np.ascontiguousarray(roots, dtype=np.int32)
            assert roots.ndim == 3 and roots.shape[1:] == (n, 2), "roots is [K, n_vars, 2]"
            if not (self.qualifies(7) if qualifies is None else qualifies) or bad_option:
                probe(roots.ctypes.data, roots.shape[0])
            roots = torch.from_numpy(roots).cuda()
        assert roots.is_cuda and roots.dtype == torch.int32 and roots.is_contiguous()
        assert roots.dim() == 3 and tuple(roots.shape[1:]) == (n, 2), "roots is [K, n_vars, 2]"
        return roots, roots.shape[0]

    @staticmethod
    def _many_records(K, device) -> torch.Tensor:
        """K zeroed csgpu_many_result records of 40 bytes (one for an empty batch: the library wants a pointer)"""
        return torch.zeros((max(K, 1), 5), dtype=torch.int64, device=device)

    @staticmethod
    def _many_rows(solutions, shape, named, device):
        """the buffer for the solution rows: `solutions` True -> a zeroed int32 one of `shape`, False -> None, an int32
        device tensor of that shape -> itself"""
        if torch.is_tensor(solutions):
            assert solutions.is_cuda and solutions.dtype == torch.int32 and solutions.is_contiguous() and \
                tuple(solutions.shape) == shape, f"solutions is {named} int32 on the device"
            return solutions
        return torch.zeros(tuple(max(d, 0) for d in shape), dtype=torch.int32, device=device) if solutions else None

    MANY_BRANCHINGS = ("width", "allowed")

    @classmethod
    def _many_branching(cls, branching, checkpoints) -> bool:
        """is `branching` the allowed-values rule?  (that walk has no checkpoints)"""
        if branching not in cls.MANY_BRANCHINGS:
            raise ValueError(f"branching is one of {cls.MANY_BRANCHINGS}, not {branching!r}")
        if branching == "allowed" and checkpoints is not None:
            raise ValueError('branching="allowed" has no checkpoints: checkpoints= goes with branching="width"')
        return branching == "allowed"

    def qualifies_many_allowed(self) -> bool:
        """may solve_many(..., branching="allowed") run this model (kernel 7's rule, and no root domain of more than 128
        values)?  Host only: after build_tables or finalize"""
        return bool(load_library().csgpu_model_qualifies_many_allowed(self._h))

    def solve_many(self, roots, objective="ANY", *, max_nodes, solutions=True, stream=None, checkpoints=None,
                   branching="width") -> dict:
        """K instances of this model, a depth-first search per wavefront (csgpu_solve_many; the model must qualify for
        kernel 7).  roots: int32 [K, n_vars, 2] root rows inside the model's root domains, a torch tensor on the device
        (a numpy array is uploaded).  max_nodes: the budget per instance (children tried); there is no "unlimited".
        -> dict of device tensors [K]: status (0 done, 1 stopped at max_nodes, 2 bad root row), root_props, nodes, cuts,
        props, solutions, and with solutions=True `first` [K, n_vars] int32: the first solution of every instance that
        has one (zeros elsewhere).  Asynchronous on the stream; one call in flight per model.
        checkpoints: a pool of many_checkpoints(): an instance that stops at max_nodes keeps its walk in a slot of it
        (csgpu_solve_many_checkpointed); the answer then has `slot` [K] int32 (-1: no checkpoint) and is what
        resume_many() continues.  Without it the call is csgpu_solve_many.
        branching: "width" (the engine's rule: the smallest interval, every value of it) or "allowed" (the open variable
        with the fewest values that no valued neighbour forbids, and only those values: csgpu_solve_many_allowed, another
        tree with the same solutions; the model must pass qualifies_many_allowed(); its checkpoints go through
        solve_many_allowed())."""
        return self._solve_many(self._many_branching(branching, checkpoints), roots, objective, max_nodes, solutions, stream,
                                checkpoints)

    def _solve_many(self, allowed, roots, objective, max_nodes, solutions, stream, checkpoints) -> dict:
        """solve_many / solve_many_allowed: the plain or the checkpointed call of either walk"""
        L = load_library()
        n = self.n_vars
        plain = L.csgpu_solve_many_allowed if allowed else L.csgpu_solve_many
        pooled = L.csgpu_solve_many_allowed_checkpointed if allowed else L.csgpu_solve_many_checkpointed
        obj = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        opt = ManyOptions(obj, 0, int(max_nodes))
        roots, K = self._many_roots(roots, False, lambda ptr, count: check(
            plain(self._h, ptr, count, C.byref(opt), ptr, None, None)),
            qualifies=self.qualifies_many_allowed() if allowed else None)
        buf = self._many_records(K, roots.device)
        first = self._many_rows(bool(solutions), (K, n), "[K, n_vars]", roots.device)
        # (an empty batch still goes through the library's checks: any non-null pointer stands for its rows)
        if checkpoints is None:
            check(plain(self._h, roots.data_ptr() if K else buf.data_ptr(), K, C.byref(opt), buf.data_ptr(),
                        first.data_ptr() if solutions and K else None, _stream_ptr(stream)))
            return self._many_answer(buf, K, first)
        slots = torch.full((max(K, 1),), -1, dtype=torch.int32, device=roots.device)
        check(pooled(self._h, roots.data_ptr() if K else buf.data_ptr(), K, C.byref(opt), buf.data_ptr(),
                     first.data_ptr() if solutions and K else None, checkpoints._h, slots.data_ptr(), _stream_ptr(stream)))
        out = self._many_answer(buf, K, first, slots, checkpoints)
        if allowed:
            out["_allowed"] = True  # resume_many goes on through the allowed walk's resume calls
        return out

    def solve_many_allowed(self, roots, objective="ANY", *, max_nodes, max_solutions=None, checkpoints=None, solutions=True,
                           stream=None) -> dict:
        """the allowed-values walk with everything it has: without a pool solve_many(..., branching="allowed"), or with
        max_solutions=k solve_many_upto(..., branching="allowed") (`objective` does not apply); with
        checkpoints=many_checkpoints(cap) the checkpointed call of either (csgpu_solve_many_allowed_checkpointed /
        _allowed_upto_checkpointed): an instance that stops at max_nodes keeps its walk in a slot, the answer has `slot`
        [K] and is what resume_many() continues -- through the allowed walk's own resume calls.  A slot of this walk is
        no checkpoint of the width walk, and the other way round (BAD_SLOT)."""
        if max_solutions is not None:
            out = self._solve_many_upto("csgpu_solve_many_allowed_upto", self.qualifies_many_allowed(), roots, max_solutions,
                                        max_nodes, solutions, stream, checkpoints)
        else:
            out = self._solve_many(True, roots, objective, max_nodes, solutions, stream, checkpoints)
        if checkpoints is not None:
            out["_allowed"] = True
        return out

    @staticmethod
    def _many_answer(buf, K, first, slots=None, checkpoints=None) -> dict:
        """views of the csgpu_many_result records in `buf` (the answer keeps the buffers a resume writes to)"""
        res = buf[:K]
        head = res.view(torch.int32)  # [K, 10]: the two 32-bit fields lead the record
        out = {"status": head[:, 0], "root_props": head[:, 1], "nodes": res[:, 1], "cuts": res[:, 2], "props": res[:, 3],
               "solutions": res[:, 4]}
        if first is not None:
            out["first"] = first
        if slots is not None:
            out["slot"] = slots[:K]
            out["_records"], out["_slots"], out["_checkpoints"] = buf, slots, checkpoints
        return out

    def solve_many_upto(self, roots, k, *, max_nodes, solutions=True, stream=None, checkpoints=None,
                        branching="width") -> dict:
        """solve_many that leaves an instance right after its k-th solution and keeps all k (csgpu_solve_many_upto): the
        ALL walk, stopped as ANY stops after the first.  k = 1 is ANY, an instance with fewer than k solutions ends as
        under ALL; status DONE means solutions == min(k, solutions of the tree).  roots, max_nodes, stream, checkpoints:
        as solve_many.  -> the dict of solve_many with `rows` [K, k, n_vars] int32 in place of `first`: row j of instance
        i is its j-th solution in walk order, rows >= solutions[i] are not written.  solutions: True (a zeroed buffer),
        False (no rows), or an int32 device tensor [K, k, n_vars] to write into.  With a pool the answer has `slot` and
        is what resume_many() continues (csgpu_solve_many_upto_checkpointed).  branching: as solve_many ("allowed" is
        csgpu_solve_many_allowed_upto, without checkpoints)."""
        if self._many_branching(branching, checkpoints):
            return self._solve_many_upto("csgpu_solve_many_allowed_upto", self.qualifies_many_allowed(), roots, k, max_nodes,
                                         solutions, stream, None)
        return self._solve_many_upto("csgpu_solve_many_upto", None, roots, k, max_nodes, solutions, stream, checkpoints)

    def _solve_many_upto(self, entry, qualifies, roots, k, max_nodes, solutions, stream, checkpoints) -> dict:
        """solve_many_upto / solve_many_clauses_upto: `entry` and `entry`_checkpointed of the library, which take the same
        arguments in both families; `qualifies` as _many_roots takes it"""
        L = load_library()
        plain, pooled = getattr(L, entry), getattr(L, entry + "_checkpointed", None)  # (no pooled call: no checkpoints)
        n, k = self.n_vars, int(k)
        opt = ManyUptoOptions(k, 0, int(max_nodes))
        roots, K = self._many_roots(roots, k < 1, lambda ptr, count: check(
            plain(self._h, ptr, count, C.byref(opt), ptr, None, None)), qualifies=qualifies)
        buf = self._many_records(K, roots.device)
        rows = self._many_rows(solutions, (K, k, n), "[K, k, n_vars]", roots.device)
        rows_ptr = rows.data_ptr() if rows is not None and K and k >= 1 else None
        if checkpoints is None:
            check(plain(self._h, roots.data_ptr() if K else buf.data_ptr(), K, C.byref(opt), buf.data_ptr(), rows_ptr,
                        _stream_ptr(stream)))
            out = self._many_answer(buf, K, None)
        else:
            slots = torch.full((max(K, 1),), -1, dtype=torch.int32, device=roots.device)
            check(pooled(self._h, roots.data_ptr() if K else buf.data_ptr(), K, C.byref(opt), buf.data_ptr(), rows_ptr,
                         checkpoints._h, slots.data_ptr(), _stream_ptr(stream)))
            out = self._many_answer(buf, K, None, slots, checkpoints)
            out["_upto"] = k  # the resume goes on through `entry`_resume, with this k unless told another
        if rows is not None:
            out["rows"] = rows
        return out

    def many_stream(self, rows: int) -> "ManySolutionStream":
        """a solution stream of `rows` rows for solve_many_stream: the three device tensors of csgpu_many_stream and
        take()"""
        return ManySolutionStream(self, rows)

    def solve_many_stream(self, roots, out: "ManySolutionStream", pool: "ManyCheckpoints", slots=None, results=None, *,
                          max_nodes, stream=None) -> dict:
        """ONE call of csgpu_solve_many_stream: the ALL walk of solve_many, every solution appended to `out`; an instance
        the stream has no room for steps back to before that solution and stops with status 4 (FULL).  roots: as
        solve_many.  pool: many_checkpoints(); K slots never run out.  slots: int32 [K] on the device, per instance -2
        start, -1 finished (not touched), >= 0 go on from that slot -- by default all -2; results: the record buffer of
        the call before (the counters of a resumed instance are read from it), by default zeroed.  max_nodes: the budget
        of THIS call per instance.  -> the dict of solve_many(..., checkpoints=pool) without `first`; its `_slots` and
        `_records` are what the next call takes.  The rows are out.take()'s: take them before the next call."""
        return self._solve_many_stream("csgpu_solve_many_stream", self.qualifies(7), roots, out, pool, slots, results,
                                       max_nodes, stream)

    def _solve_many_stream(self, entry, qualifies, roots, out, pool, slots, results, max_nodes, stream) -> dict:
        """solve_many_stream and solve_many_clauses_stream: `entry` is the library's call, `qualifies` its rule"""
        call = getattr(load_library(), entry)
        opt = ManyOptions(1, 0, int(max_nodes))
        desc = out.struct()
        roots, K = self._many_roots(roots, out.capacity < 1, lambda ptr, count: check(
            call(self._h, ptr, count, C.byref(opt), ptr, pool._h if pool is not None else ptr, ptr, C.byref(desc), None)),
            qualifies=qualifies)
        buf = self._many_records(K, roots.device) if results is None else results
        if slots is None:
            slots = torch.full((max(K, 1),), MANY_SLOT_FRESH, dtype=torch.int32, device=roots.device)
        assert buf.is_cuda and buf.dtype == torch.int64 and buf.is_contiguous() and tuple(buf.shape) == (max(K, 1), 5)
        assert slots.is_cuda and slots.dtype == torch.int32 and slots.is_contiguous() and slots.shape[0] == max(K, 1)
        check(call(self._h, roots.data_ptr() if K else buf.data_ptr(), K, C.byref(opt), buf.data_ptr(), pool._h,
                   slots.data_ptr(), C.byref(desc), _stream_ptr(stream)))
        ans = self._many_answer(buf, K, None, slots, pool)
        ans["_roots"] = roots
        return ans

    def solve_many_all(self, roots, *, max_nodes, stream_rows=65536, on_rows=None, max_calls=None) -> dict:
        """every solution of every instance: solve_many_stream in a loop with a pool of K slots and a stream of
        `stream_rows` rows -- call, take the rows, zero the count, until no instance has work left.  Every instance
        then ends DONE with the record of solve_many(roots, "ALL") under an unlimited budget, whatever stream_rows and
        max_nodes (the budget per instance and call) are.  Synchronises after every call.
        -> the dict of solve_many without `first`, plus `calls`, and without on_rows `offsets` int64 [K + 1] and `rows`
        int32 [total, n_vars] on the device: rows[offsets[i]:offsets[i + 1]] are the solutions of instance i in walk order.
        on_rows(owner, rows): called with every drain that holds a row (device tensors int32 [m] and [m, n_vars], the
        rows of one instance in walk order within and across drains); nothing is kept then.
        max_calls: stop after that many calls; the answer then also has `slot`, `_slots`, `_records`, `_checkpoints`,
        `_roots` and `stream`, which solve_many_stream takes to go on."""
        return self._solve_many_all(self.solve_many_stream, self.many_checkpoints, self.qualifies(7), roots, max_nodes,
                                    stream_rows, on_rows, max_calls)

    def _solve_many_all(self, one_call, make_pool, qualifies, roots, max_nodes, stream_rows, on_rows, max_calls) -> dict:
        """the loop of solve_many_all and solve_many_clauses_all: `one_call` is the family's stream call, `make_pool` its
        pool and `qualifies` its rule"""
        out = self.many_stream(stream_rows)
        K = int(roots.shape[0])
        pool = slots = results = ans = None
        kept, calls = [], 0
        while True:
            # (a numpy batch on a model that cannot run the call gets the library's error from the call's own probe,
            # before anything is allocated for it)
            if pool is None and (torch.is_tensor(roots) or qualifies):
                pool = make_pool(max(K, 1))
            ans = one_call(roots, out, pool, slots, results, max_nodes=max_nodes)
            roots, slots, results = ans["_roots"], ans["_slots"], ans["_records"]
            calls += 1
            owner, rows = out.take()
            if on_rows is None:
                kept.append((owner, rows))
            elif owner.shape[0]:
                on_rows(owner, rows)
            left = K > 0 and bool((ans["slot"] != -1).any())
            if not left or (max_calls is not None and calls >= max_calls):
                break
        ans["calls"] = calls
        if on_rows is None:
            owner = torch.cat([o for o, _ in kept]).to(torch.int64)
            order = torch.sort(owner, stable=True).indices
            ans["rows"] = torch.cat([r for _, r in kept])[order]
            ans["offsets"] = torch.cat([torch.zeros(1, dtype=torch.int64, device=owner.device),
                                        torch.cumsum(torch.bincount(owner, minlength=K), 0)])
        if left:
            ans["stream"] = out
        else:
            for key in ("slot", "_slots", "_records", "_checkpoints", "_roots"):
                ans.pop(key)
            pool.close()
        return ans

    def many_stream_kernel(self):
        """the cs_dive_stream instantiation solve_many_stream launches"""
        return self._many_symbol("csgpu_internal_many_stream_symbol")

    def solve_many_restarts(self, roots, *, max_nodes, restart_base=32, seed=0, seeds=None, rotate_first=False,
                            solutions=True, restarts=True, stream=None) -> dict:
        """solve_many under ANY with Luby restarts and a seeded value order (csgpu_solve_many_restarts): a node tries its
        values in a rotation of the ascending order that depends on (seed of the instance, run, variable), and after
        more than threshold x restart_base failed children -- thresholds 1 1 2 1 1 2 4 ... -- the walk starts again from
        the root node's fixpoint with the next run's rotations.  The first run is the ascending walk of solve_many unless
        rotate_first.  restart_base=0: no restarts (with rotate_first: one seeded walk, a sampler).  seeds: uint32 [K]
        (int32 / int64 tensors and arrays are converted), one per instance, else `seed` for all: an instance's answer
        depends on its row, its seed and the options only.  max_nodes is the total over an instance's runs; a LIMIT
        instance can be run again with a larger budget, the walk is deterministic.  The default base of 32 comes from
        node counts of 9x9 sudokus on the host.  roots, solutions, stream: as solve_many.
        -> the dict of solve_many plus `restarts` [K] int32 (restarts=False: not counted, d_restarts is NULL); solutions
        may be an int32 device tensor [K, n_vars] to write into."""
        return self._solve_many_restarts("csgpu_solve_many_restarts", None, roots, max_nodes, restart_base, seed, seeds,
                                         rotate_first, solutions, restarts, stream)

    def _solve_many_restarts(self, entry, qualifies, roots, max_nodes, restart_base, seed, seeds, rotate_first, solutions,
                             restarts, stream) -> dict:
        """solve_many_restarts / solve_many_clauses_restarts: `entry` of the library, which takes the same arguments in
        both families; `qualifies` as _many_roots takes it"""
        call = getattr(load_library(), entry)
        n = self.n_vars
        opt = ManyRestartOptions(int(max_nodes), int(restart_base), int(seed) & 0xffffffff,
                                 MANY_ROTATE_FIRST if rotate_first else 0)
        roots, K = self._many_roots(roots, restart_base < 0, lambda ptr, count: check(
            call(self._h, ptr, None, count, C.byref(opt), ptr, None, None, None)), qualifies=qualifies)
        if seeds is not None:
            if not torch.is_tensor(seeds):
                seeds = torch.from_numpy((np.asarray(seeds).astype(np.int64) & 0xffffffff).astype(np.uint32).view(np.int32))
            seeds = seeds.to(device=roots.device, dtype=torch.int32).contiguous()  # the 32 bits are what counts
            assert tuple(seeds.shape) == (K,), "seeds is [K]"
        buf = self._many_records(K, roots.device)
        first = self._many_rows(solutions, (K, n), "[K, n_vars]", roots.device)
        count = torch.zeros((max(K, 1),), dtype=torch.int32, device=roots.device) if restarts else None
        check(call(self._h, roots.data_ptr() if K else buf.data_ptr(), seeds.data_ptr() if seeds is not None and K else None,
                   K, C.byref(opt), buf.data_ptr(), first.data_ptr() if first is not None and K else None,
                   count.data_ptr() if restarts else None, _stream_ptr(stream)))
        out = self._many_answer(buf, K, first)
        if restarts:
            out["restarts"] = count[:K]
        return out

    def solve_many_clauses(self, roots, objective="ANY", *, max_nodes, solutions=True, stream=None, checkpoints=None,
                           start=None) -> dict:
        """solve_many for clause models (csgpu_solve_many_clauses: `=`, `<`, disjunctions, expression trees; the model
        must satisfy qualifies_many_clauses()), a depth-first search per wavefront on kernel 6's fixpoint, also under
        "MIN" / "MAX": the model's own sense, each instance with a private incumbent, walked to the end of its tree.
        roots, max_nodes, solutions, stream: as solve_many.  -> the dict of solve_many; `first` is the stored row (ANY /
        ALL: the first solution; MIN / MAX: the best one found, the optimum when status is 0), and under MIN / MAX
        `best` [K] int32, meaningful where solutions > 0.  An instance that stops at max_nodes under MIN / MAX keeps the
        best found so far: an anytime answer.
        checkpoints: a pool of many_clause_checkpoints(): an instance that stops at max_nodes keeps its walk and its
        incumbent in a slot of it (csgpu_solve_many_clauses_checkpointed); the answer then has `slot` [K] int32 (-1: no
        checkpoint) and is what resume_many_clauses() continues.  Without it nothing changes.
        start: int32 [K, 2] on the device, {best, have} per instance (csgpu_solve_many_clauses_from, MIN / MAX only): an
        instance with have != 0 starts its walk with the incumbent `best`, which it did not find itself -- a warm start,
        or "prove that nothing beats 45".  `first` / `best` are then written only for solutions of the instance's own,
        each strictly better than its start; one that proves that nothing beats its start ends with status 0 and
        solutions == 0, its `best` and row untouched (zero).  have == 0 is the walk without a start.  None: today's
        calls, untouched."""
        L = load_library()
        n = self.n_vars
        obj = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        opt = ManyOptions(obj, 0, int(max_nodes))
        bad = obj not in (0, 1) and (obj not in (2, 3) or self.objective != obj or self.objective_var < 0)
        if start is not None:
            return self._solve_many_clauses_from(roots, obj, opt, bad, solutions, stream, checkpoints, start)
        roots, K = self._many_roots(roots, bad, lambda ptr, count: check(
            L.csgpu_solve_many_clauses(self._h, ptr, count, C.byref(opt), ptr, None, None, None)),
            qualifies=self.qualifies_many_clauses())
        buf = self._many_records(K, roots.device)
        first = self._many_rows(bool(solutions), (K, n), "[K, n_vars]", roots.device)
        best = torch.zeros((max(K, 1),), dtype=torch.int32, device=roots.device) if obj in (2, 3) else None
        if checkpoints is None:
            check(L.csgpu_solve_many_clauses(self._h, roots.data_ptr() if K else buf.data_ptr(), K, C.byref(opt), buf.data_ptr(),
                                             first.data_ptr() if solutions and K else None,
                                             best.data_ptr() if best is not None else None, _stream_ptr(stream)))
            out = self._many_answer(buf, K, first)
        else:
            slots = torch.full((max(K, 1),), -1, dtype=torch.int32, device=roots.device)
            check(L.csgpu_solve_many_clauses_checkpointed(self._h, roots.data_ptr() if K else buf.data_ptr(), K, C.byref(opt),
                                                          buf.data_ptr(), first.data_ptr() if solutions and K else None,
                                                          best.data_ptr() if best is not None else None, checkpoints._h,
                                                          slots.data_ptr(), _stream_ptr(stream)))
            out = self._many_answer(buf, K, first, slots, checkpoints)
            out["_objective"], out["_best"] = obj, best  # resume_many_clauses goes on under the same objective
        if best is not None:
            out["best"] = best[:K]
        return out

    def _solve_many_clauses_from(self, roots, obj, opt, bad, solutions, stream, checkpoints, start) -> dict:
        """solve_many_clauses with start incumbents: the one entry, with or without a pool"""
        L = load_library()
        n = self.n_vars
        roots, K = self._many_roots(roots, bad, lambda ptr, count: check(
            L.csgpu_solve_many_clauses_from(self._h, ptr, ptr, count, C.byref(opt), ptr, None, None, None, None, None)),
            qualifies=self.qualifies_many_clauses())
        assert torch.is_tensor(start) and start.is_cuda and start.dtype == torch.int32 and start.is_contiguous() and \
            tuple(start.shape) == (K, 2), "start is int32 [K, 2] on the device: {best, have}"
        buf = self._many_records(K, roots.device)
        first = self._many_rows(bool(solutions), (K, n), "[K, n_vars]", roots.device)
        best = torch.zeros((max(K, 1),), dtype=torch.int32, device=roots.device)
        slots = torch.full((max(K, 1),), -1, dtype=torch.int32, device=roots.device) if checkpoints is not None else None
        check(L.csgpu_solve_many_clauses_from(self._h, roots.data_ptr() if K else buf.data_ptr(),
                                              start.data_ptr() if K else buf.data_ptr(), K, C.byref(opt), buf.data_ptr(),
                                              first.data_ptr() if solutions and K else None, best.data_ptr(),
                                              checkpoints._h if checkpoints is not None else None,
                                              slots.data_ptr() if slots is not None else None, _stream_ptr(stream)))
        out = self._many_answer(buf, K, first, slots, checkpoints)
        if checkpoints is not None:
            out["_objective"], out["_best"] = obj, best
        out["best"] = best[:K]
        return out

    MANY_ORDERS = {"none": 0, "smallest-domain": 1, "largest-domain": 2, "smallest-value": 3, "largest-value": 4}

    def solve_many_clauses_ordered(self, roots, objective="ANY", *, max_nodes, order="smallest-domain", split_width=256,
                                   solutions=True, stream=None, checkpoints=None, start=None) -> dict:
        """solve_many_clauses under one of the engine's five variable orders, with wide intervals halved
        (csgpu_solve_many_clauses_ordered): the same walk, but the branching variable is the open one the order puts
        first -- "none", "smallest-domain", "largest-domain", "smallest-value", "largest-value", the names of
        `csolve_gpu -o`, ties to the lowest index -- and a node whose branching variable has more than `split_width`
        values (>= 1) has two children, [lo, mid] and [mid + 1, hi] with mid = (lo + hi) >> 1, instead of one per value.
        A row that leaves a variable at its root width (an open `end` of a schedule) is then bisected, not enumerated.
        roots, objective, max_nodes, solutions, stream: as solve_many_clauses.  -> the dict of solve_many_clauses and
        `halvings` [K] int64: the parents split in two.
        checkpoints: a pool of many_clause_ordered_checkpoints(capacity, split_width), made for this split_width: an
        instance that stops at max_nodes keeps its walk, its incumbent and its place between two halves in a slot of it
        (csgpu_solve_many_clauses_ordered_checkpointed); the answer then has `slot` [K] int32 (-1: no checkpoint) and is
        what resume_many_clauses() continues, under the same objective, order and split_width.  A walk in slices is the one
        call with the summed budget, field for field, `halvings` included.  Without it nothing changes.
        start: int32 [K, 2] on the device, {best, have} per instance, as solve_many_clauses(..., start=) and with its rules
        (csgpu_solve_many_clauses_ordered_from, MIN / MAX only, with or without a pool): `first` / `best` are written only
        for solutions of the instance's own.  have == 0 everywhere is the call without `start`, `halvings` included."""
        L = load_library()
        n = self.n_vars
        obj = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        opt = ManyOrderOptions(obj, self.MANY_ORDERS[order] if isinstance(order, str) else int(order), int(split_width), 0,
                               int(max_nodes))
        bad = obj not in (0, 1) and (obj not in (2, 3) or self.objective != obj or self.objective_var < 0)
        bad = bad or not 0 <= opt.order <= 4 or opt.split_width < 0
        if start is not None:
            return self._solve_many_clauses_ordered_from(roots, obj, opt, bad, solutions, stream, checkpoints, start)
        roots, K = self._many_roots(roots, bad, lambda ptr, count: check(
            L.csgpu_solve_many_clauses_ordered(self._h, ptr, count, C.byref(opt), ptr, None, None, None, None)),
            qualifies=self.qualifies_many_clauses())
        buf = self._many_records(K, roots.device)
        first = self._many_rows(bool(solutions), (K, n), "[K, n_vars]", roots.device)
        best = torch.zeros((max(K, 1),), dtype=torch.int32, device=roots.device) if obj in (2, 3) else None
        halvings = torch.zeros((max(K, 1),), dtype=torch.int64, device=roots.device)
        if checkpoints is None:
            check(L.csgpu_solve_many_clauses_ordered(self._h, roots.data_ptr() if K else buf.data_ptr(), K, C.byref(opt),
                                                     buf.data_ptr(), first.data_ptr() if solutions and K else None,
                                                     best.data_ptr() if best is not None else None, halvings.data_ptr(),
                                                     _stream_ptr(stream)))
            out = self._many_answer(buf, K, first)
        else:
            slots = torch.full((max(K, 1),), -1, dtype=torch.int32, device=roots.device)
            check(L.csgpu_solve_many_clauses_ordered_checkpointed(
                self._h, roots.data_ptr() if K else buf.data_ptr(), K, C.byref(opt), buf.data_ptr(),
                first.data_ptr() if solutions and K else None, best.data_ptr() if best is not None else None,
                halvings.data_ptr(), checkpoints._h, slots.data_ptr(), _stream_ptr(stream)))
            out = self._many_answer(buf, K, first, slots, checkpoints)
            # resume_many_clauses goes on under the same objective, order and split_width, from these counts
            out["_objective"], out["_best"] = obj, best
            out["_order"], out["_split_width"], out["_halvings"] = opt.order, opt.split_width, halvings
        if best is not None:
            out["best"] = best[:K]
        out["halvings"] = halvings[:K]
        return out

    def _solve_many_clauses_ordered_from(self, roots, obj, opt, bad, solutions, stream, checkpoints, start) -> dict:
        """solve_many_clauses_ordered with start incumbents: the one entry, with or without a pool"""
        L = load_library()
        n = self.n_vars
        roots, K = self._many_roots(roots, bad or obj not in (2, 3), lambda ptr, count: check(
            L.csgpu_solve_many_clauses_ordered_from(self._h, ptr, ptr, count, C.byref(opt), ptr, None, None, None, None, None,
                                                    None)), qualifies=self.qualifies_many_clauses())
        assert torch.is_tensor(start) and start.is_cuda and start.dtype == torch.int32 and start.is_contiguous() and \
            tuple(start.shape) == (K, 2), "start is int32 [K, 2] on the device: {best, have}"
        buf = self._many_records(K, roots.device)
        first = self._many_rows(bool(solutions), (K, n), "[K, n_vars]", roots.device)
        best = torch.zeros((max(K, 1),), dtype=torch.int32, device=roots.device)
        halvings = torch.zeros((max(K, 1),), dtype=torch.int64, device=roots.device)
        slots = torch.full((max(K, 1),), -1, dtype=torch.int32, device=roots.device) if checkpoints is not None else None
        check(L.csgpu_solve_many_clauses_ordered_from(
            self._h, roots.data_ptr() if K else buf.data_ptr(), start.data_ptr() if K else buf.data_ptr(), K, C.byref(opt),
            buf.data_ptr(), first.data_ptr() if solutions and K else None, best.data_ptr(), halvings.data_ptr(),
            checkpoints._h if checkpoints is not None else None, slots.data_ptr() if slots is not None else None,
            _stream_ptr(stream)))
        out = self._many_answer(buf, K, first, slots, checkpoints)
        if checkpoints is not None:
            out["_objective"], out["_best"] = obj, best
            out["_order"], out["_split_width"], out["_halvings"] = opt.order, opt.split_width, halvings
        out["best"] = best[:K]
        out["halvings"] = halvings[:K]
        return out

    def many_clauses_order_from_kernel(self):
        """the cs_walk_order_from instantiation solve_many_clauses_ordered(..., start=) launches, or None"""
        return self._many_symbol("csgpu_internal_many_clauses_order_from_symbol")

    def many_clauses_ordered_frames(self, split_width=256) -> int:
        """frames per wave of a solve_many_clauses_ordered call (csgpu_many_clauses_ordered_frames): n_vars + for every
        variable the halvings that bring its root width down to split_width; 0 if the model does not qualify.  Host only"""
        return int(load_library().csgpu_many_clauses_ordered_frames(self._h, int(split_width)))

    def many_clauses_order_kernel(self):
        """the cs_walk_order instantiation solve_many_clauses_ordered launches, or None"""
        return self._many_symbol("csgpu_internal_many_clauses_order_symbol")

    def many_clauses_order_resume_kernel(self):
        """the cs_walk_order_resume instantiation the checkpointed ordered calls launch, or None"""
        return self._many_symbol("csgpu_internal_many_clauses_order_resume_symbol")

    def many_clause_ordered_checkpoints(self, capacity: int, split_width=256) -> "ManyCheckpoints":
        """a pool of `capacity` checkpoint slots for solve_many_clauses_ordered(..., split_width=split_width, checkpoints=)
        (csgpu_many_clause_ordered_checkpoints_create): a ManyCheckpoints of the ordered clause kind, whose slots have
        the many_clauses_ordered_frames(split_width) + 1 frames that walk needs.  Every other call refuses it, as the
        ordered calls refuse a pool of many_clause_checkpoints() or one made for another split_width"""
        return ManyCheckpoints(self, capacity, clauses=True, split_width=split_width)

    def clause_ordered_checkpoint_bytes(self, split_width=256) -> int:
        """bytes of one ordered clause checkpoint slot, (many_clauses_ordered_frames(split_width) + 1) x (n_vars + 1) x 8,
        or 0 if the model does not qualify or split_width is negative (host only: after build_tables or finalize)"""
        return int(load_library().csgpu_many_clause_ordered_checkpoint_bytes(self._h, int(split_width)))

    def resume_many_clauses(self, result: dict, *, max_nodes, stream=None, max_solutions=None, own_solutions=False) -> dict:
        """continue, in place, the instances of a checkpointed solve_many_clauses answer that stopped with a checkpoint
        (csgpu_solve_many_clauses_resume): `max_nodes` more nodes each, under the answer's objective.  Counters
        accumulate; under MIN / MAX `first` / `best` are overwritten at every improvement, the incumbent travelling in
        the slot; under ANY / ALL `first` is written when `solutions` goes from 0 to 1.  Rows of instances without a
        slot are not touched.  -> result
        An answer of solve_many_clauses_upto(..., checkpoints=pool) goes on through csgpu_solve_many_clauses_upto_resume:
        its rows continue at index `solutions`.  max_solutions: the k of THIS slice, by default the answer's, exactly as
        in resume_many().
        own_solutions: continue through csgpu_solve_many_clauses_from_resume (MIN / MAX answers): `best` is written only
        for an instance with a solution of its own, never with the start incumbent its checkpoint carries.  A checkpoint
        of either MIN / MAX call may be continued either way.
        An answer of solve_many_clauses_ordered(..., checkpoints=pool) goes on through
        csgpu_solve_many_clauses_ordered_resume under its order and split_width; `halvings` accumulates with the other
        counters.  max_solutions is not for it; own_solutions continues a MIN / MAX answer through
        csgpu_solve_many_clauses_ordered_from_resume under the own-solutions rule (an answer of another objective, or one
        that does not say under which it was made: ValueError)."""
        if "_checkpoints" in result and "_order" in result:
            if max_solutions is not None:
                raise ValueError("max_solutions does not continue an answer of solve_many_clauses_ordered: the ordered walk "
                                 "has no up to k solutions")
            if own_solutions and result.get("_objective") not in (2, 3):
                raise ValueError("own_solutions continues a MIN / MAX answer of solve_many_clauses_ordered: only such a walk "
                                 "has an incumbent")
            opt = ManyOrderOptions(result["_objective"], result["_order"], result["_split_width"], 0, int(max_nodes))
            first, best = result.get("first"), result["_best"]
            K = result["status"].shape[0]
            L = load_library()
            entry = L.csgpu_solve_many_clauses_ordered_from_resume if own_solutions else L.csgpu_solve_many_clauses_ordered_resume
            check(entry(
                self._h, K, C.byref(opt), result["_records"].data_ptr(), first.data_ptr() if first is not None and K else None,
                best.data_ptr() if best is not None else None, result["_halvings"].data_ptr(), result["_checkpoints"]._h,
                result["_slots"].data_ptr(), _stream_ptr(stream)))
            return result
        if "_checkpoints" in result and "_upto" in result:
            return self._resume_many_upto(result, int(max_nodes), max_solutions, stream,
                                          entry="csgpu_solve_many_clauses_upto_resume")
        assert max_solutions is None, "max_solutions continues an answer of solve_many_clauses_upto"
        assert "_checkpoints" in result and "_objective" in result, "an answer of solve_many_clauses(..., checkpoints=pool)"
        opt = ManyOptions(result["_objective"], 0, int(max_nodes))
        first, best = result.get("first"), result["_best"]
        K = result["status"].shape[0]
        L = load_library()
        entry = L.csgpu_solve_many_clauses_from_resume if own_solutions else L.csgpu_solve_many_clauses_resume
        check(entry(self._h, K, C.byref(opt), result["_records"].data_ptr(),
                    first.data_ptr() if first is not None and K else None, best.data_ptr() if best is not None else None,
                    result["_checkpoints"]._h, result["_slots"].data_ptr(), _stream_ptr(stream)))
        return result

    def solve_many_clauses_upto(self, roots, k, *, max_nodes, solutions=True, stream=None, checkpoints=None) -> dict:
        """solve_many_clauses that leaves an instance right after its k-th solution and keeps all k
        (csgpu_solve_many_clauses_upto): the ALL walk -- "<obj>" an ordinary variable, no incumbent -- stopped as ANY
        stops after the first.  k = 1 is ANY, an instance with fewer than k solutions ends as under ALL; status DONE
        means solutions == min(k, solutions of the tree).  roots, max_nodes, stream: as solve_many_clauses.  -> the dict
        of solve_many_upto: `rows` [K, k, n_vars] int32, row j of instance i its j-th solution in walk order, rows >=
        solutions[i] not written.  solutions: True (a zeroed buffer), False (no rows), or an int32 device tensor
        [K, k, n_vars] to write into.  checkpoints: a pool of many_clause_checkpoints(); the answer then has `slot` and is
        what resume_many_clauses() continues (csgpu_solve_many_clauses_upto_checkpointed)."""
        return self._solve_many_upto("csgpu_solve_many_clauses_upto", self.qualifies_many_clauses(), roots, k, max_nodes,
                                     solutions, stream, checkpoints)

    def solve_many_clauses_restarts(self, roots, *, max_nodes, restart_base=1, seed=0, seeds=None, rotate_first=False,
                                    solutions=True, restarts=True, stream=None) -> dict:
        """solve_many_clauses under ANY with Luby restarts and a seeded value order (csgpu_solve_many_clauses_restarts):
        what solve_many_restarts is to solve_many, for the clause models.  A node tries its values in a rotation of the
        ascending order that depends on (seed of the instance, run, variable), and after more than threshold x
        restart_base failed children -- thresholds 1 1 2 1 1 2 4 ... -- the walk starts again from the root node's
        fixpoint with the next run's rotations.  The first run is the ascending walk of solve_many_clauses unless
        rotate_first; restart_base=0 is that call under ANY, field for field.  ANY only: "<obj>" is an ordinary variable.
        The default base of 1 has the fewest nodes in all of 1, 2, 4 .. 32 on three batches of schedule rows walked on
        the host; the 32 of solve_many_restarts costs 3.5 times as many there.  roots, max_nodes, seed,
        seeds, solutions, restarts, stream: as solve_many_restarts; the model must satisfy qualifies_many_clauses().
        -> the dict of solve_many_clauses under ANY plus `restarts` [K] int32."""
        return self._solve_many_restarts("csgpu_solve_many_clauses_restarts", self.qualifies_many_clauses(), roots, max_nodes,
                                         restart_base, seed, seeds, rotate_first, solutions, restarts, stream)

    def solve_many_clauses_stream(self, roots, out: "ManySolutionStream", pool: "ManyCheckpoints", slots=None, results=None,
                                  *, max_nodes, stream=None) -> dict:
        """ONE call of csgpu_solve_many_clauses_stream: solve_many_stream for the clause models.  The ALL walk of
        solve_many_clauses_upto -- "<obj>" an ordinary variable, no incumbent -- with every solution appended to `out`
        (many_stream()); an instance the stream has no room for steps back to before that solution and stops with status
        4 (FULL).  pool: many_clause_checkpoints(); K slots never run out.  roots, slots, results, max_nodes, stream and
        the answer: as solve_many_stream; the model must satisfy qualifies_many_clauses()."""
        return self._solve_many_stream("csgpu_solve_many_clauses_stream", self.qualifies_many_clauses(), roots, out, pool,
                                       slots, results, max_nodes, stream)

    def solve_many_clauses_all(self, roots, *, max_nodes, stream_rows=65536, on_rows=None, max_calls=None) -> dict:
        """every solution of every instance of a clause model ("every timetable of these windows"): the loop of
        solve_many_all over solve_many_clauses_stream with a pool of K clause slots.  Every instance ends DONE with the
        record of solve_many_clauses(roots, "ALL") under an unlimited budget, whatever stream_rows and max_nodes are.
        The answer (`offsets`, `rows`, `calls`), on_rows and max_calls: exactly as solve_many_all; what max_calls leaves
        is what solve_many_clauses_stream takes to go on."""
        return self._solve_many_all(self.solve_many_clauses_stream, self.many_clause_checkpoints, self.qualifies_many_clauses(),
                                    roots, max_nodes, stream_rows, on_rows, max_calls)

    def many_clauses_stream_kernel(self):
        """the cs_walk_stream instantiation solve_many_clauses_stream launches, or None"""
        return self._many_symbol("csgpu_internal_many_clauses_stream_symbol")

    def many_clauses_from_kernel(self):
        """the cs_walk_from instantiation solve_many_clauses(..., start=) and the own-solutions resume launch"""
        return self._many_symbol("csgpu_internal_many_clauses_from_symbol")

    def many_clauses_restart_kernel(self):
        """the cs_walk_restart instantiation solve_many_clauses_restarts launches, or None"""
        return self._many_symbol("csgpu_internal_many_clauses_restart_symbol")

    def many_clauses_upto_kernel(self):
        """the cs_walk_upto instantiation solve_many_clauses_upto and its checkpoint calls launch, or None"""
        return self._many_symbol("csgpu_internal_many_clauses_upto_symbol")

    def classify_many_clauses(self, roots, *, max_nodes, stream=None) -> torch.Tensor:
        """classify_many for clause models: is the solution (the timetable of a schedule row) unique?  -> int8 [K] on
        the device: 0 no solution, 1 exactly one, 2 several, -1 undecided within max_nodes (LIMIT), -2 bad root row.  A
        solve_many_clauses_upto with k = 2 and no rows."""
        return self._many_classes(self.solve_many_clauses_upto(roots, 2, max_nodes=max_nodes, solutions=False, stream=stream),
                                  stream)

    def many_clause_checkpoints(self, capacity: int) -> "ManyCheckpoints":
        """a pool of `capacity` checkpoint slots for solve_many_clauses(..., checkpoints=)
        (csgpu_many_clause_checkpoints_create): a ManyCheckpoints of the clause kind, which solve_many refuses as
        solve_many_clauses refuses a pool of many_checkpoints()"""
        return ManyCheckpoints(self, capacity, clauses=True)

    def clause_checkpoint_bytes(self) -> int:
        """bytes of one clause checkpoint slot, (n_vars + 1)^2 x 8, or 0 if the model does not qualify for
        solve_many_clauses (host only: after build_tables or finalize)"""
        return int(load_library().csgpu_many_clause_checkpoint_bytes(self._h))

    def many_clauses_resume_kernel(self):
        """the cs_walk_resume instantiation the checkpointed clause calls launch, or None"""
        return self._many_symbol("csgpu_internal_many_clauses_resume_symbol")

    # ---- clause models past 512 clauses: the records in LDS (csgpu_solve_many_clauses_wide) ----

    def qualifies_many_clauses_wide(self) -> bool:
        """may solve_many_clauses_wide run this model: at least one clause, and its clause records, the literal records of
        its two-literal disjunctions and the LDS slices of a workgroup's four waves fit the 160 KiB of a CU?  Models of at
        most 512 clauses qualify too.  Host only: what finalize planned, or after build_tables the same rule on the
        host tables"""
        return bool(load_library().csgpu_model_qualifies_many_clauses_wide(self._h))

    def many_clauses_wide_kernel(self):
        """the cs_walk_wide instantiation solve_many_clauses_wide launches, or None"""
        return self._many_symbol("csgpu_internal_many_clauses_wide_symbol")

    def many_clauses_wide_resume_kernel(self):
        """the cs_walk_wide_resume instantiation the checkpointed wide calls launch, or None"""
        return self._many_symbol("csgpu_internal_many_clauses_wide_resume_symbol")

    def many_clauses_wide_waves(self, count: int) -> int:
        """waves a solve_many_clauses_wide of `count` instances launches (0 if the model does not qualify)"""
        return int(load_library().csgpu_internal_many_clauses_wide_waves(self._h, int(count)))

    def solve_many_clauses_wide(self, roots, objective="ANY", *, max_nodes, solutions=True, stream=None,
                                checkpoints=None) -> dict:
        """solve_many_clauses for clause models past 512 clauses (csgpu_solve_many_clauses_wide): the same walk -- the
        branching rule, the private incumbent under "MIN" / "MAX", the counters, the statuses, max_nodes -- with the
        clause records in LDS, one copy per workgroup, in place of kernel 6's registers.  The model must satisfy
        qualifies_many_clauses_wide(); on a model that solve_many_clauses takes as well the two answers are equal field
        for field, props included.  roots, objective, max_nodes, solutions, stream and the answer: as solve_many_clauses.
        checkpoints: a pool of many_clause_wide_checkpoints(): an instance that stops at max_nodes keeps its walk and its
        incumbent in a slot of it (csgpu_solve_many_clauses_wide_checkpointed); the answer then has `slot` [K] int32 (-1:
        no checkpoint) and is what resume_many_clauses_wide() continues.
        Not on this walk: up to k solutions, the stream, restarts, the variable orders and halving, start incumbents, the
        spread over idle waves, clause_checkpoint_states and the Search finish, the sliced drivers."""
        L = load_library()
        n = self.n_vars
        obj = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        opt = ManyOptions(obj, 0, int(max_nodes))
        bad = obj not in (0, 1) and (obj not in (2, 3) or self.objective != obj or self.objective_var < 0)
        roots, K = self._many_roots(roots, bad, lambda ptr, count: check(
            L.csgpu_solve_many_clauses_wide(self._h, ptr, count, C.byref(opt), ptr, None, None, None)),
            qualifies=self.finalized and self.qualifies_many_clauses_wide())
        buf = self._many_records(K, roots.device)
        first = self._many_rows(bool(solutions), (K, n), "[K, n_vars]", roots.device)
        best = torch.zeros((max(K, 1),), dtype=torch.int32, device=roots.device) if obj in (2, 3) else None
        if checkpoints is None:
            check(L.csgpu_solve_many_clauses_wide(self._h, roots.data_ptr() if K else buf.data_ptr(), K, C.byref(opt),
                                                  buf.data_ptr(), first.data_ptr() if solutions and K else None,
                                                  best.data_ptr() if best is not None else None, _stream_ptr(stream)))
            out = self._many_answer(buf, K, first)
        else:
            slots = torch.full((max(K, 1),), -1, dtype=torch.int32, device=roots.device)
            check(L.csgpu_solve_many_clauses_wide_checkpointed(self._h, roots.data_ptr() if K else buf.data_ptr(), K,
                                                               C.byref(opt), buf.data_ptr(),
                                                               first.data_ptr() if solutions and K else None,
                                                               best.data_ptr() if best is not None else None, checkpoints._h,
                                                               slots.data_ptr(), _stream_ptr(stream)))
            out = self._many_answer(buf, K, first, slots, checkpoints)
            out["_objective"], out["_best"] = obj, best  # resume_many_clauses_wide goes on under the same objective
        if best is not None:
            out["best"] = best[:K]
        return out

    def many_clause_wide_checkpoints(self, capacity: int) -> "ManyCheckpoints":
        """a pool of `capacity` checkpoint slots for solve_many_clauses_wide(..., checkpoints=)
        (csgpu_many_clause_wide_checkpoints_create): a ManyCheckpoints of the wide clause kind.  Every other call that
        takes a pool refuses it, as the wide calls refuse a pool of any other kind"""
        return ManyCheckpoints(self, capacity, clauses=True, wide=True)

    def clause_wide_checkpoint_bytes(self) -> int:
        """bytes of one wide clause checkpoint slot, (n_vars + 1)^2 x 8, or 0 if the model does not qualify for
        solve_many_clauses_wide (host only: after build_tables or finalize)"""
        return int(load_library().csgpu_many_clause_wide_checkpoint_bytes(self._h))

    def resume_many_clauses_wide(self, result: dict, *, max_nodes, stream=None) -> dict:
        """continue, in place, the instances of a checkpointed solve_many_clauses_wide answer that stopped with a
        checkpoint (csgpu_solve_many_clauses_wide_resume): `max_nodes` more nodes each, under the answer's objective,
        exactly as resume_many_clauses() continues an answer of solve_many_clauses.  -> result"""
        assert "_checkpoints" in result and "_objective" in result and result["_checkpoints"].wide, \
            "an answer of solve_many_clauses_wide(..., checkpoints=pool)"
        opt = ManyOptions(result["_objective"], 0, int(max_nodes))
        first, best = result.get("first"), result["_best"]
        K = result["status"].shape[0]
        check(load_library().csgpu_solve_many_clauses_wide_resume(
            self._h, K, C.byref(opt), result["_records"].data_ptr(), first.data_ptr() if first is not None and K else None,
            best.data_ptr() if best is not None else None, result["_checkpoints"]._h, result["_slots"].data_ptr(),
            _stream_ptr(stream)))
        return result

    def clause_checkpoint_states(self, checkpoints: "ManyCheckpoints", slot: int, stream=None):
        """-> (states, best): the open subtrees of the clause checkpoint in `slot` as states [depth + 1, n_vars, 2] int32
        on the device, the oldest frame (the largest subtree) first, and the instance's incumbent or None
        (csgpu_many_clause_checkpoint_states).  The states are not at the fixpoint and not under the incumbent's bound
        yet: see open_clause_subtrees().  A pool of many_clause_ordered_checkpoints() is taken as well: up to
        many_clauses_ordered_frames() states, a pushed halving parent's being its second half."""
        n = self.n_vars
        rows = checkpoints.frames if checkpoints.ordered else n  # depth + 1 <= n; an ordered pool: <= its frames
        out = torch.empty((rows, n, 2), dtype=torch.int32, device="cuda")
        count, best, have = C.c_int64(), C.c_int32(), C.c_int32()
        check(load_library().csgpu_many_clause_checkpoint_states(checkpoints._h, int(slot), out.data_ptr(), rows, C.byref(count),
                                                                 C.byref(best), C.byref(have), _stream_ptr(stream)))
        return out[: count.value], (int(best.value) if have.value else None)

    def open_clause_subtrees(self, checkpoints: "ManyCheckpoints", slot: int):
        """clause_checkpoint_states() made ready for a Search: every state through the fixpoint as a `var < 0` node, under
        the incumbent's bound when there is one (propagate_obj), the inconsistent ones dropped.
        -> (open states [m, n_vars, 2] for Search.put, complete states [s, n_vars, 2]: each a solution of its own -- under
        an incumbent a better one -- which the engine must not be given, the incumbent or None for Search.set_best)"""
        states, best = self.clause_checkpoint_states(checkpoints, slot)
        nodes = torch.zeros((states.shape[0], 4), dtype=torch.int32, device=states.device)
        nodes[:, 0] = -1
        nodes[:, 3] = torch.arange(states.shape[0], dtype=torch.int32, device=states.device)
        if best is None:
            out, res = self.propagate(states.contiguous(), nodes)
        else:
            lo, hi = (-2**31, best - 1) if self.objective == 2 else (best + 1, 2**31 - 1)
            out, res = self.propagate_obj(states.contiguous(), nodes, lo, hi)
        alive = res[:, 0] >= 0
        complete = (out[:, :, 0] == out[:, :, 1]).all(dim=1)
        return out[alive & ~complete].contiguous(), out[alive & complete].contiguous(), best

    def solve_many_clauses_sliced(self, roots, objective="ANY", *, budgets, finish="resume", solutions=True,
                                  pool_capacity=1 << 18, max_children=1 << 14, checkpoints=None, max_solutions=None,
                                  order=None, split_width=256) -> dict:
        """solve_many_clauses in slices: a checkpointed call with budgets[0], then a resume with each following budget
        while an instance is at LIMIT -- a small budget for everybody, more for the few that need it.
        finish="resume": that is all (instances still at LIMIT stay so, with their slots and the best found so far).
        finish="search": after the last budget every instance still at LIMIT with a slot hands its open subtrees, and its
        incumbent, to one reused Search (reset, set_best, put, run) and ends DONE.  Under MIN / MAX `best` / `first`
        are the better of the walk's incumbent, the complete states and the engine's best_solution: the proven optimum;
        the row may differ from the single-wave walk's where several rows attain it.  `solutions` is the sum (ALL, and
        the improving solutions of MIN / MAX) or 1 if any part found one (ANY); `nodes`, `cuts` and `props` of those
        instances are the sums of both parts and NOT the single-wave walk's: the engine walks the open subtrees in its
        own order.  The engine walks with the model's own objective, which must be the one asked for.  Synchronises
        between the slices.  checkpoints: a pool of many_clause_checkpoints() to use, which is reset first (a caller that
        repeats the call saves making one); else a pool of K slots is made.
        -> the dict of solve_many_clauses plus `slot` and `sliced`: {"slices": calls made, "searched": instances finished
        by the Search}
        max_solutions=k: the slices are solve_many_clauses_upto calls (`objective` does not apply, the answer has
        `rows`), with finish="resume" only.
        order (one of MANY_ORDERS, with split_width): the slices are solve_many_clauses_ordered calls on a pool of
        many_clause_ordered_checkpoints(K, split_width) -- `checkpoints`, if given, must be one of those, made for this
        split_width -- the answer has `halvings`, and with finish="search" the Search is given the same order
        (set_strategy).  Not together with max_solutions."""
        assert finish in ("resume", "search") and len(budgets) >= 1
        if order is not None and max_solutions is not None:
            raise ValueError("order with max_solutions: the ordered walk has no up to k solutions")
        if max_solutions is not None and finish == "search":
            raise ValueError("finish=\"search\" with max_solutions: an engine search cannot stop at a k-th solution "
                             "per instance")
        obj = None if max_solutions is not None else self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        if finish == "search" and obj != self.objective:
            raise ValueError("finish=\"search\": a Search walks with the model's own objective, which must be the one asked for")
        if checkpoints is not None:
            pool = checkpoints.reset()
        elif order is not None:
            pool = self.many_clause_ordered_checkpoints(max(roots.shape[0], 1), split_width)
        else:
            pool = self.many_clause_checkpoints(max(roots.shape[0], 1))
        if order is not None:  # resume_many_clauses takes the order and the split_width from the answer
            out = self.solve_many_clauses_ordered(roots, objective, max_nodes=budgets[0], order=order, split_width=split_width,
                                                  solutions=solutions, checkpoints=pool)
        elif max_solutions is not None:  # resume_many_clauses takes the k from the answer
            out = self.solve_many_clauses_upto(roots, max_solutions, max_nodes=budgets[0], solutions=solutions, checkpoints=pool)
        else:
            out = self.solve_many_clauses(roots, objective, max_nodes=budgets[0], solutions=solutions, checkpoints=pool)
        return self._many_slices(out, pool, budgets, self.resume_many_clauses, obj,
                                 self.open_clause_subtrees if finish == "search" else None, pool_capacity, max_children, order)

    def _many_slices(self, out: dict, pool, budgets, resume, obj, open_subtrees, pool_capacity, max_children,
                     order=None) -> dict:
        """solve_many_sliced and solve_many_clauses_sliced after their first slice `out`: `resume` with each following
        budget while an instance is at LIMIT; then, where the finish is a Search, every instance still at LIMIT with a slot
        hands the (states, complete, best) of `open_subtrees` (else None) to one reused Search, which walks under
        `order` where the slices did"""
        slices = 1
        for budget in budgets[1:]:
            if not bool((out["status"] == 1).any()):
                break
            resume(out, max_nodes=budget)
            slices += 1
        searched = 0
        if open_subtrees is not None:
            left = torch.nonzero((out["status"] == 1) & (out["slot"] >= 0)).flatten().tolist()
            if left:
                search = Search(self, pool_capacity, max_children)
                if order is not None:
                    search.set_strategy(order)
                for i in left:
                    self._finish_by_search(search, out, i, obj, *open_subtrees(pool, int(out["slot"][i])))
                    searched += 1
                search.close()
        out["sliced"] = {"slices": slices, "searched": searched}
        return out

    def _finish_by_search(self, search: "Search", out: dict, i: int, obj: int, states, complete, best):
        """instance i of `out`, stopped with a checkpoint: its open subtrees `states` through `search` and its `complete`
        states, each a solution, the totals added.  best: the incumbent of a clause checkpoint, or None"""
        found = int(complete.shape[0])
        bounded, ov = obj in (2, 3), self.objective_var
        first = None
        if found and bounded:  # each complete state beats the walk's incumbent: the best of them
            values = complete[:, ov, 0]
            j = int(torch.argmin(values) if obj == 2 else torch.argmax(values))
            best, first = int(values[j]), complete[j, :, 0]
        elif found:
            first = complete[0, :, 0]
        nodes = cuts = props = 0
        if states.shape[0] and not (obj == 0 and found):
            search.reset()
            if best is not None:
                search.set_best(best)
            search.put(states)
            st = search.run()
            assert st["done"] == 1
            nodes, cuts, props = st["nodes"], st["cuts"], st["props"]
            found += st["solutions"]
            if bounded:
                row = search.best_solution()
                if row is not None and (best is None or (row[ov] < best if obj == 2 else row[ov] > best)):
                    best, first = int(row[ov]), torch.from_numpy(row.astype(np.int32)).to(states.device)
            elif st["solutions"] and first is None:
                first = torch.from_numpy(search.solutions(1)[0].astype(np.int32)).to(states.device)
        if obj == 0:
            found = min(found, 1)
        if first is not None and "first" in out and (bounded or int(out["solutions"][i]) == 0):
            out["first"][i] = first
        if bounded and best is not None:
            out["best"][i] = best
        out["solutions"][i] += found
        out["nodes"][i] += nodes
        out["cuts"][i] += cuts
        out["props"][i] += props
        out["status"][i] = 0
        out["slot"][i] = -1

    def qualifies_many_clauses(self) -> bool:
        """may solve_many_clauses run this model (finalized, kernel 6 planned, its LDS slices fit a CU)?"""
        return bool(load_library().csgpu_model_qualifies_many_clauses(self._h))

    def many_clauses_kernel(self):
        """the cs_walk_clauses instantiation solve_many_clauses launches, or None"""
        return self._many_symbol("csgpu_internal_many_clauses_symbol")

    def many_clauses_waves(self, count: int) -> int:
        """waves a solve_many_clauses of `count` instances launches"""
        return int(load_library().csgpu_internal_many_clauses_waves(self._h, int(count)))

    def classify_many(self, roots, *, max_nodes, stream=None, branching="width") -> torch.Tensor:
        """is the solution unique?  -> int8 [K] on the device: 0 no solution, 1 exactly one, 2 several, -1 undecided
        within max_nodes (LIMIT), -2 bad root row.  A solve_many_upto with k = 2 and no rows; branching as there."""
        return self._many_classes(self.solve_many_upto(roots, 2, max_nodes=max_nodes, solutions=False, stream=stream,
                                                       branching=branching), stream)

    @staticmethod
    def _many_classes(out: dict, stream) -> torch.Tensor:
        """the classes of classify_many / classify_many_clauses from an up-to-2 answer"""
        status, found = out["status"], out["solutions"]
        ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
        with ctx:
            cls = torch.where(status == 2, torch.full_like(found, -2), torch.where(status == 1, torch.full_like(found, -1), found))
            return cls.to(torch.int8)

    def many_checkpoints(self, capacity: int) -> "ManyCheckpoints":
        """a pool of `capacity` checkpoint slots for solve_many(..., checkpoints=) (csgpu_many_checkpoints_create); a
        slot stays with its instance until reset()"""
        return ManyCheckpoints(self, capacity)

    def checkpoint_bytes(self) -> int:
        """bytes of one checkpoint slot, 0 if the model does not qualify (host only: after build_tables or finalize)"""
        return int(load_library().csgpu_many_checkpoint_bytes(self._h))

    def resume_many(self, result: dict, *, max_nodes, objective="ANY", stream=None, max_solutions=None) -> dict:
        """continue, in place, the instances of a checkpointed solve_many answer that stopped with a checkpoint
        (csgpu_solve_many_resume): `max_nodes` more nodes each; counters accumulate, `first` is written when an
        instance's `solutions` goes from 0 to 1, rows of instances without a slot are not touched.  -> result
        An answer of solve_many_upto(..., checkpoints=pool) goes on through csgpu_solve_many_upto_resume (`objective`
        does not apply): its rows continue at index `solutions`.  max_solutions: the k of THIS slice, by default the
        answer's; an instance that already holds that many ends DONE untouched; with another k the rows are laid out
        anew for the call ([K, max(k), n_vars] stays or grows)."""
        assert "_checkpoints" in result, "an answer of solve_many(..., checkpoints=pool)"
        allowed = bool(result.get("_allowed"))  # an answer of solve_many_allowed: the allowed walk's resume calls
        if "_upto" in result:
            return self._resume_many_upto(result, int(max_nodes), max_solutions, stream,
                                          "csgpu_solve_many_allowed_upto_resume" if allowed else "csgpu_solve_many_upto_resume")
        assert max_solutions is None, "max_solutions continues an answer of solve_many_upto"
        obj = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        opt = ManyOptions(obj, 0, int(max_nodes))
        first = result.get("first")
        K = result["status"].shape[0]
        L = load_library()
        entry = L.csgpu_solve_many_allowed_resume if allowed else L.csgpu_solve_many_resume
        check(entry(self._h, K, C.byref(opt), result["_records"].data_ptr(), first.data_ptr() if first is not None and K else None,
                    result["_checkpoints"]._h, result["_slots"].data_ptr(), _stream_ptr(stream)))
        return result

    def _resume_many_upto(self, result: dict, max_nodes: int, max_solutions, stream,
                          entry="csgpu_solve_many_upto_resume") -> dict:
        """resume_many / resume_many_clauses on an up-to-k answer: `entry` is the family's resume call"""
        had = result["_upto"]
        k = had if max_solutions is None else int(max_solutions)
        opt = ManyUptoOptions(k, 0, max_nodes)
        rows = result.get("rows")
        K = result["status"].shape[0]
        L = load_library()

        def call(buf):
            check(getattr(L, entry)(self._h, K, C.byref(opt), result["_records"].data_ptr(),
                                    buf.data_ptr() if buf is not None and K and k >= 1 else None,
                                    result["_checkpoints"]._h, result["_slots"].data_ptr(), _stream_ptr(stream)))

        if rows is None or k == had or k < 1:
            call(rows)
            return result
        # the kernel indexes rows with the k of the call: a buffer laid out for this k, carrying the rows there are
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            laid = torch.zeros((K, k, rows.shape[2]), dtype=torch.int32, device=rows.device)
            keep = min(k, had)
            laid[:, :keep] = rows[:, :keep]
            call(laid)
            if k < had:
                rows[:, :k] = laid
            else:
                result["rows"], result["_upto"] = laid, k
        return result

    def checkpoint_states(self, checkpoints: "ManyCheckpoints", slot: int, stream=None) -> torch.Tensor:
        """the open subtrees of the checkpoint in `slot` as states [depth + 1, n_vars, 2] int32 on the device, the
        oldest frame (the largest subtree) first (csgpu_many_checkpoint_states).  They are not at the fixpoint yet:
        see open_subtrees()."""
        n = self.n_vars
        out = torch.empty((n, n, 2), dtype=torch.int32, device="cuda")  # depth + 1 <= n
        count = C.c_int64()
        check(load_library().csgpu_many_checkpoint_states(checkpoints._h, int(slot), out.data_ptr(), n, C.byref(count),
                                                          _stream_ptr(stream)))
        return out[: count.value]

    def open_subtrees(self, checkpoints: "ManyCheckpoints", slot: int):
        """checkpoint_states() made ready for a Search: every state through the fixpoint as a `var < 0` node, the
        inconsistent ones dropped.  -> (open states [m, n_vars, 2] for Search.put, complete states [s, n_vars, 2]: each
        a solution of its own, which the engine must not be given -- it branches on an open variable)"""
        states = self.checkpoint_states(checkpoints, slot)
        nodes = torch.zeros((states.shape[0], 4), dtype=torch.int32, device=states.device)
        nodes[:, 0] = -1
        nodes[:, 3] = torch.arange(states.shape[0], dtype=torch.int32, device=states.device)
        out, res = self.propagate(states.contiguous(), nodes)
        alive = res[:, 0] >= 0
        complete = (out[:, :, 0] == out[:, :, 1]).all(dim=1)
        return out[alive & ~complete].contiguous(), out[alive & complete].contiguous()

    def solve_many_sliced(self, roots, objective="ANY", *, budgets, finish="resume", solutions=True, pool_capacity=1 << 18,
                          max_children=1 << 14, max_solutions=None, branching="width") -> dict:
        """solve_many in slices: a checkpointed call with budgets[0], then a resume with each following budget while
        an instance is at LIMIT.  finish="resume": that is all (instances still at LIMIT stay so, with their slots).
        finish="search": after the last budget every instance still at LIMIT hands its open subtrees to a Search of
        its own (the whole device on one deep tree) and ends DONE: `solutions` is the sum (ALL) or 1 if either part
        found one (ANY), `first` the dive's if it has one, else the search's; `nodes`, `cuts` and `props` of those
        instances are the sum of both parts -- the engine walks the open subtrees in its own order and, for ANY, not
        up to the same node, so they are NOT the single-wave walk's.  The engine walks with the model's own objective,
        which must be the one asked for.  Synchronises between the slices.
        -> the dict of solve_many plus `slot` and `sliced`: {"slices": calls made, "searched": instances finished by
        a Search}
        max_solutions=k: the slices are solve_many_upto calls (`objective` does not apply, the answer has `rows`), with
        finish="resume" only.
        branching="allowed": the slices are solve_many_allowed calls.  finish="search" hands the engine [next, hi] of every
        frame, a cover of the allowed walk's open subtrees (the engine cuts the forbidden values itself): `solutions` is
        the walk's, the added counters are the engine's."""
        assert finish in ("resume", "search") and len(budgets) >= 1
        allowed = self._many_branching(branching, None)
        if max_solutions is not None:
            if finish == "search":
                raise ValueError("finish=\"search\" with max_solutions: an engine search cannot stop at a k-th solution "
                                 "per instance")
            obj, more = None, {}  # resume_many takes the k from the answer

            def first_slice(pool):
                if allowed:
                    return self.solve_many_allowed(roots, max_nodes=budgets[0], max_solutions=max_solutions, solutions=solutions,
                                                   checkpoints=pool)
                return self.solve_many_upto(roots, max_solutions, max_nodes=budgets[0], solutions=solutions, checkpoints=pool)
        else:
            obj, more = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective), {"objective": objective}
            if finish == "search" and obj != self.objective:
                raise ValueError("finish=\"search\": a Search walks with the model's own objective, which must be the one asked for")

            def first_slice(pool):
                if allowed:
                    return self.solve_many_allowed(roots, objective, max_nodes=budgets[0], solutions=solutions, checkpoints=pool)
                return self.solve_many(roots, objective, max_nodes=budgets[0], solutions=solutions, checkpoints=pool)
        pool = self.many_checkpoints(max(roots.shape[0], 1))
        return self._many_slices(first_slice(pool), pool, budgets, functools.partial(self.resume_many, **more), obj,
                                 (lambda pool, slot: (*self.open_subtrees(pool, slot), None)) if finish == "search" else None,
                                 pool_capacity, max_children)

    def checkpoint_children(self, checkpoints: "ManyCheckpoints", slots: torch.Tensor, stream=None,
                            branching="width") -> torch.Tensor:
        """the untried children of the checkpoints in `slots` (int32 [S] on the device) -> int64 [S]: 0 for a slot < 0,
        -1 for a slot that is refused (csgpu_many_checkpoint_children).  branching="allowed": the slots of the allowed
        walk, whose children are the untried values no valued variable forbids (csgpu_many_allowed_checkpoint_children);
        each call refuses the other walk's slots."""
        assert slots.is_cuda and slots.dtype == torch.int32 and slots.is_contiguous() and slots.dim() == 1
        L = load_library()
        entry = L.csgpu_many_allowed_checkpoint_children if self._many_branching(branching, None) else L.csgpu_many_checkpoint_children
        S = slots.shape[0]
        children = torch.empty((max(S, 1),), dtype=torch.int64, device=slots.device)
        check(entry(checkpoints._h, slots.data_ptr(), S, children.data_ptr(), _stream_ptr(stream)))
        return children[:S]

    def checkpoint_fanout(self, checkpoints: "ManyCheckpoints", slots: torch.Tensor, offsets: torch.Tensor, total: int,
                          rows: torch.Tensor = None, owner: torch.Tensor = None, stream=None, branching="width"):
        """the children of the checkpoints in `slots` as root rows, in walk order (csgpu_many_checkpoint_fanout): offsets
        int64 [S + 1], the exclusive prefix sum of checkpoint_children() on the device.  -> (rows int32 [total, n_vars, 2],
        owner int32 [total]: the index into `slots` a row came from); given buffers are written in place, and an instance
        whose count disagrees with its offsets writes nothing.  branching="allowed": as checkpoint_children
        (csgpu_many_allowed_checkpoint_fanout)"""
        L = load_library()
        entry = L.csgpu_many_allowed_checkpoint_fanout if self._many_branching(branching, None) else L.csgpu_many_checkpoint_fanout
        n, S, total = self.n_vars, slots.shape[0], int(total)
        assert slots.is_cuda and slots.dtype == torch.int32 and slots.is_contiguous() and slots.dim() == 1
        assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous() and tuple(offsets.shape) == (S + 1,)
        if rows is None:
            rows = torch.empty((max(total, 1), n, 2), dtype=torch.int32, device=slots.device)
        if owner is None:
            owner = torch.empty((max(total, 1),), dtype=torch.int32, device=slots.device)
        assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.numel() >= total * n * 2
        assert owner.dtype == torch.int32 and owner.is_contiguous() and owner.numel() >= total
        check(entry(checkpoints._h, slots.data_ptr(), S, offsets.data_ptr(), rows.data_ptr(), owner.data_ptr(), total,
                    _stream_ptr(stream)))
        return rows[:total], owner[:total]

    def fold_many(self, sub: dict, owner: torch.Tensor, result: dict, stream=None) -> dict:
        """add the records of the sub-instances `sub` (a checkpointed solve_many answer over fanned rows) to their owners
        in `result` (csgpu_many_fold): owner int32 [T] indexes result's instances.  Exactly once per batch: a second
        call counts it twice."""
        T = sub["status"].shape[0]
        assert owner.is_cuda and owner.dtype == torch.int32 and owner.is_contiguous() and owner.shape[0] == T
        check(load_library().csgpu_many_fold(sub["_records"].data_ptr(), owner.data_ptr(), T, result["_records"].data_ptr(),
                                             _stream_ptr(stream)))
        return result

    def solve_many_spread(self, roots, *, budgets=(256, 4096), max_rounds=64, max_rows=1 << 18, solutions=True, stream=None,
                          pool_bytes=1 << 30, pools=None, branching="width") -> dict:
        """solve_many under ALL whose stopped instances are spread over the idle waves: round 0 is a checkpointed
        solve_many with budgets[0]; every later round counts the untried children of the stopped instances
        (checkpoint_children), fans them out as root rows of their own (checkpoint_fanout) and walks those as a fresh
        checkpointed ALL batch with that round's budget (the last budget repeats).  A batch is folded into its owners
        exactly once, when it is left (fold_many); a sub-instance's owner is mapped through the owner vector of the level
        before.  The split is exact: an owner whose sub-instances all ended DONE is DONE with the record of the one ALL
        call, field for field, and `first` is the walk's first solution.
        max_rows: a round with more children is not fanned out, its stopped walks go on in place (resume_many) with that
        round's budget.  max_rounds (round 0 included): owners with work left after it end LIMIT with the counters
        folded so far, as does the owner of a stopped instance that got no slot.  Two alternating pools hold the
        checkpoints, each of at most pool_bytes; pools=(a, b): two pools of many_checkpoints() to use instead (a caller
        that times or repeats the call keeps them).  Synchronises once or twice per round (the counts of stopped
        instances and of their children).
        -> the dict of solve_many (device tensors [K]) plus `rounds`, `sub_instances` and `round_rows` (the rows fanned
        out for every round after round 0; 0 for a round that went on in place)
        branching="allowed": the same driver on the allowed-values walk -- every batch a solve_many_allowed, the children
        the untried ALLOWED values (csgpu_many_allowed_checkpoint_children / _fanout), the same fold; the answer is the
        record of solve_many(..., "ALL", branching="allowed")."""
        family = dict(solve=self.solve_many, resume=lambda batch, **kw: self.resume_many(batch, objective="ALL", **kw),
                      children=self.checkpoint_children, fanout=self.checkpoint_fanout, make_pool=self.many_checkpoints,
                      slot_bytes=self.checkpoint_bytes(), qualifies=True)
        if self._many_branching(branching, None):
            family.update(
                solve=self.solve_many_allowed, qualifies=self.qualifies_many_allowed(),
                children=lambda pool, slots, stream=None: self.checkpoint_children(pool, slots, stream, branching="allowed"),
                fanout=lambda pool, slots, offsets, total, stream=None: self.checkpoint_fanout(
                    pool, slots, offsets, total, stream=stream, branching="allowed"))
        return self._spread_call(functools.partial(self._solve_many_spread, family), family["make_pool"], family["slot_bytes"],
                                 roots, budgets, max_rounds, max_rows, solutions, stream, pool_bytes, pools)

    def _spread_call(self, driver, make_pool, slot_bytes, roots, budgets, max_rounds, max_rows, solutions, stream, pool_bytes,
                     pools) -> dict:
        """solve_many_spread and solve_many_clauses_spread around `driver`, one of the two below: the stream, the two pools
        and what the rounds of both share (_SpreadRounds)"""
        budgets = tuple(int(b) for b in budgets)
        assert len(budgets) >= 1 and max_rounds >= 1 and max_rows >= 0
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            sp = _SpreadRounds(make_pool, slot_bytes, budgets, stream, int(pool_bytes), pools)
            try:
                return driver(sp, roots, int(max_rounds), int(max_rows), bool(solutions), stream)
            finally:
                if sp.own_pools:
                    for p in sp.pools:
                        if p is not None:
                            p.close()

    def _solve_many_spread(self, family, sp, roots, max_rounds, max_rows, solutions, stream) -> dict:
        """the driver of solve_many_spread and solve_many_clauses_spread under ALL.  `family`: what the two differ in --
        `solve` (the family's solve_many, walked under "ALL"), `resume` (its resume in place), `children` and `fanout` (its
        count and fan-out of a pool), `make_pool`, `slot_bytes` and `qualifies` (False: the solve call itself refuses the
        model, before a pool is made for it); `halvings` (the ordered walk): `children` gives (children, unsplit), and the
        answers' `halvings` are folded beside the records (fold_many_halvings, and the unsplit of every fanned slot)"""
        BIG = 1 << 62  # "no solution yet": above every row number
        solve, resume = family["solve"], family["resume"]
        if not family["qualifies"]:  # the call says why, as it does without the spread
            solve(roots, "ALL", max_nodes=sp.budget(0), solutions=solutions, stream=stream)
        pool = sp.pool_for(0, int(roots.shape[0]))
        main = solve(roots, "ALL", max_nodes=sp.budget(0), solutions=solutions, stream=stream, checkpoints=pool)
        K, dev = sp.begin(main)
        pos = None  # per owner, in the row numbers of the batch: a solution of a row below it comes before the owner's `first`
        batch = main
        rounds, round_rows = 1, []

        def leave(last):
            """fold the batch and take its first solutions; its stopped instances without a slot (`last`: all its
            stopped instances) make their owners LIMIT"""
            nonlocal pos
            T = batch["status"].shape[0]
            rows = sp.count_stopped(batch, last)
            if sp.owner is not None:
                self.fold_many(batch, sp.owner, main, stream)
                if family.get("halvings"):
                    self.fold_many_halvings(batch, sp.owner, main, stream)
            if not solutions:
                return
            has = batch["solutions"] > 0
            if sp.owner is None:
                pos = torch.where(has, torch.zeros_like(rows), torch.full_like(rows, BIG))
                return
            lowest = torch.full((max(K, 1),), BIG, dtype=torch.int64, device=dev)
            lowest.scatter_reduce_(0, sp.owner.long(), torch.where(has, rows, torch.full_like(rows, BIG)), "amin")
            lowest = lowest[:K]
            take = lowest < pos
            src = batch["first"][lowest.clamp(max=max(T - 1, 0))]
            main["first"].copy_(torch.where(take[:, None], src, main["first"]))
            pos = torch.where(take, lowest, pos)

        while rounds < max_rounds and K > 0:
            index = torch.nonzero((batch["status"] == 1) & (batch["slot"] >= 0)).flatten()  # ascending; waits for the batch
            S = int(index.shape[0])
            if S == 0:
                break
            slots = batch["slot"][index].contiguous()
            children, unsplit = sp.counted(family["children"](pool, slots, stream))
            offsets = torch.zeros((S + 1,), dtype=torch.int64, device=dev)
            torch.cumsum(children.clamp(min=0), 0, out=offsets[1:])
            total = int(offsets[-1].item())
            if total > max_rows:  # too wide to fan out: the stopped walks go on where they are
                resume(batch, max_nodes=sp.budget(rounds), stream=stream)
                round_rows.append(0)
                rounds += 1
                continue
            sp.count_refused(index, children)
            if total == 0:
                break
            sp.owe(main, index, unsplit)
            rows, came_from = family["fanout"](pool, slots, offsets, total, stream=stream)
            leave(False)
            if solutions:
                pos = offsets[torch.searchsorted(index, pos)]
            sp.owner = sp.owners_of(index[came_from.long()]).to(torch.int32).contiguous()
            pool = sp.pool_for(rounds, total)
            batch = solve(rows, "ALL", max_nodes=sp.budget(rounds), solutions=solutions, stream=stream, checkpoints=pool)
            round_rows.append(total)
            rounds += 1
        leave(True)
        return sp.answer(main, rounds, round_rows)

    def clause_checkpoint_children(self, checkpoints: "ManyCheckpoints", slots: torch.Tensor, stream=None,
                                   objective=None) -> torch.Tensor:
        """checkpoint_children for a pool of many_clause_checkpoints() (csgpu_many_clause_checkpoint_children): the untried
        children of the clause checkpoints in `slots` (int32 [S] on the device) -> int64 [S]: 0 for a slot < 0, -1 for a
        slot that is refused, one written under another objective than ALL among them.  objective "MIN" / "MAX": the
        checkpoints of such a walk instead (csgpu_many_clause_checkpoint_children_obj), every other one refused"""
        assert slots.is_cuda and slots.dtype == torch.int32 and slots.is_contiguous() and slots.dim() == 1
        S = slots.shape[0]
        children = torch.empty((max(S, 1),), dtype=torch.int64, device=slots.device)
        if objective is not None:
            obj = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
            check(load_library().csgpu_many_clause_checkpoint_children_obj(checkpoints._h, slots.data_ptr(), S, obj,
                                                                           children.data_ptr(), _stream_ptr(stream)))
            return children[:S]
        check(load_library().csgpu_many_clause_checkpoint_children(checkpoints._h, slots.data_ptr(), S, children.data_ptr(),
                                                                   _stream_ptr(stream)))
        return children[:S]

    def clause_checkpoint_fanout(self, checkpoints: "ManyCheckpoints", slots: torch.Tensor, offsets: torch.Tensor, total: int,
                                 rows: torch.Tensor = None, owner: torch.Tensor = None, stream=None, objective=None,
                                 owner_start: torch.Tensor = None, start: torch.Tensor = None):
        """checkpoint_fanout for a pool of many_clause_checkpoints() (csgpu_many_clause_checkpoint_fanout): the children of
        the clause checkpoints in `slots` as root rows of solve_many_clauses, in walk order.  offsets, total, rows, owner
        and the answer: as checkpoint_fanout.  objective "MIN" / "MAX": the checkpoints of such a walk
        (csgpu_many_clause_checkpoint_fanout_obj); the answer is then (rows, owner, start), start int32 [total, 2] the
        {best, have} every row begins with in solve_many_clauses(..., start=): the strictly better of its checkpoint's
        incumbent and owner_start[i] (int32 [S, 2] on the device, or None)"""
        n, S, total = self.n_vars, slots.shape[0], int(total)
        assert slots.is_cuda and slots.dtype == torch.int32 and slots.is_contiguous() and slots.dim() == 1
        assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous() and tuple(offsets.shape) == (S + 1,)
        if rows is None:
            rows = torch.empty((max(total, 1), n, 2), dtype=torch.int32, device=slots.device)
        if owner is None:
            owner = torch.empty((max(total, 1),), dtype=torch.int32, device=slots.device)
        assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.numel() >= total * n * 2
        assert owner.dtype == torch.int32 and owner.is_contiguous() and owner.numel() >= total
        if objective is not None:
            obj = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
            if start is None:
                start = torch.empty((max(total, 1), 2), dtype=torch.int32, device=slots.device)
            assert start.dtype == torch.int32 and start.is_contiguous() and start.numel() >= total * 2
            assert owner_start is None or (owner_start.is_cuda and owner_start.dtype == torch.int32 and
                                           owner_start.is_contiguous() and tuple(owner_start.shape) == (S, 2))
            check(load_library().csgpu_many_clause_checkpoint_fanout_obj(
                checkpoints._h, slots.data_ptr(), S, obj, owner_start.data_ptr() if owner_start is not None and S else None,
                offsets.data_ptr(), rows.data_ptr(), owner.data_ptr(), start.data_ptr(), total, _stream_ptr(stream)))
            return rows[:total], owner[:total], start[:total]
        assert owner_start is None and start is None, "start incumbents travel with objective MIN / MAX"
        check(load_library().csgpu_many_clause_checkpoint_fanout(checkpoints._h, slots.data_ptr(), S, offsets.data_ptr(),
                                                                 rows.data_ptr(), owner.data_ptr(), total, _stream_ptr(stream)))
        return rows[:total], owner[:total]

    def fold_many_best(self, sub: dict, owner: torch.Tensor, K: int, objective, stream=None):
        """the best value every owner has in the batch `sub` (a MIN / MAX solve_many_clauses answer over fanned rows) and
        the LOWEST row that holds it (csgpu_many_fold_best): owner int32 [T], rows with owner < 0 or without a solution
        are skipped.  -> (has [K] bool, best [K] int32, row [K] int64; best and row are 0 where has is False)"""
        obj = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        T = sub["status"].shape[0]
        assert owner.is_cuda and owner.dtype == torch.int32 and owner.is_contiguous() and owner.shape[0] == T
        key = torch.full((max(int(K), 1),), -1, dtype=torch.int64, device=owner.device)  # all ones
        check(load_library().csgpu_many_fold_best(sub["_records"].data_ptr() if "_records" in sub else sub["status"].data_ptr(),
                                                  sub["best"].data_ptr() if T else key.data_ptr(), owner.data_ptr(), T, obj,
                                                  key.data_ptr(), _stream_ptr(stream)))
        key = key[:K]
        has = key != -1
        rank = (key >> 32) & 0xFFFFFFFF  # csgpu_many_key_decode, on the device
        best = torch.where(has, rank - (1 << 31) if obj == 2 else (1 << 31) - 1 - rank, torch.zeros_like(rank))
        return has, best.to(torch.int32), torch.where(has, key & 0xFFFFFFFF, torch.zeros_like(key))

    def _ordered_code(self, objective, order):
        obj = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        return obj, self.MANY_ORDERS[order] if isinstance(order, str) else int(order)

    def clause_ordered_checkpoint_children(self, checkpoints: "ManyCheckpoints", slots: torch.Tensor, objective, order,
                                           stream=None):
        """clause_checkpoint_children for a pool of many_clause_ordered_checkpoints()
        (csgpu_many_clause_ordered_checkpoint_children): the untried children, halves included, of the checkpoints in
        `slots` (int32 [S] on the device) that were written under `objective` ("ALL", "MIN" or "MAX") and `order` ->
        (children int64 [S]: 0 for a slot < 0, -1 for a refused slot; unsplit int32 [S]: 1 where the current node is a
        halving one with neither half tried, the halving its owner owes)"""
        assert slots.is_cuda and slots.dtype == torch.int32 and slots.is_contiguous() and slots.dim() == 1
        obj, order = self._ordered_code(objective, order)
        S = slots.shape[0]
        children = torch.empty((max(S, 1),), dtype=torch.int64, device=slots.device)
        unsplit = torch.zeros((max(S, 1),), dtype=torch.int32, device=slots.device)
        check(load_library().csgpu_many_clause_ordered_checkpoint_children(
            checkpoints._h, slots.data_ptr(), S, obj, order, children.data_ptr(), unsplit.data_ptr(), _stream_ptr(stream)))
        return children[:S], unsplit[:S]

    def clause_ordered_checkpoint_fanout(self, checkpoints: "ManyCheckpoints", slots: torch.Tensor, objective, order,
                                         offsets: torch.Tensor, total: int, rows: torch.Tensor = None,
                                         owner: torch.Tensor = None, stream=None, owner_start: torch.Tensor = None,
                                         start: torch.Tensor = None):
        """clause_checkpoint_fanout for a pool of many_clause_ordered_checkpoints()
        (csgpu_many_clause_ordered_checkpoint_fanout): the children of the checkpoints in `slots` as root rows of
        solve_many_clauses_ordered, in walk order, a half a row with its variable narrowed to that half.  offsets, total,
        rows, owner: as checkpoint_fanout.  -> (rows, owner) under "ALL"; under "MIN" / "MAX" (rows, owner, start), start
        int32 [total, 2] the {best, have} every row begins with in solve_many_clauses_ordered(..., start=): the strictly
        better of its checkpoint's incumbent and owner_start[i] (int32 [S, 2] on the device, or None)"""
        n, S, total = self.n_vars, slots.shape[0], int(total)
        obj, order = self._ordered_code(objective, order)
        assert slots.is_cuda and slots.dtype == torch.int32 and slots.is_contiguous() and slots.dim() == 1
        assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous() and tuple(offsets.shape) == (S + 1,)
        if rows is None:
            rows = torch.empty((max(total, 1), n, 2), dtype=torch.int32, device=slots.device)
        if owner is None:
            owner = torch.empty((max(total, 1),), dtype=torch.int32, device=slots.device)
        assert rows.dtype == torch.int32 and rows.is_contiguous() and rows.numel() >= total * n * 2
        assert owner.dtype == torch.int32 and owner.is_contiguous() and owner.numel() >= total
        if obj in (2, 3) and start is None:
            start = torch.empty((max(total, 1), 2), dtype=torch.int32, device=slots.device)
        assert start is None or (start.dtype == torch.int32 and start.is_contiguous() and start.numel() >= total * 2)
        assert owner_start is None or (owner_start.is_cuda and owner_start.dtype == torch.int32 and
                                       owner_start.is_contiguous() and tuple(owner_start.shape) == (S, 2))
        check(load_library().csgpu_many_clause_ordered_checkpoint_fanout(
            checkpoints._h, slots.data_ptr(), S, obj, order, owner_start.data_ptr() if owner_start is not None and S else None,
            offsets.data_ptr(), rows.data_ptr(), owner.data_ptr(), start.data_ptr() if start is not None else None, total,
            _stream_ptr(stream)))
        if start is not None:
            return rows[:total], owner[:total], start[:total]
        return rows[:total], owner[:total]

    def fold_many_halvings(self, sub: dict, owner: torch.Tensor, result: dict, stream=None) -> dict:
        """add the `halvings` of the sub-instances `sub` (a solve_many_clauses_ordered answer over fanned rows) to their
        owners' in `result` (csgpu_many_fold_halvings): owner int32 [T] indexes result's instances, rows with owner < 0
        are skipped.  Exactly once per batch, beside fold_many"""
        T = sub["status"].shape[0]
        assert owner.is_cuda and owner.dtype == torch.int32 and owner.is_contiguous() and owner.shape[0] == T
        check(load_library().csgpu_many_fold_halvings(sub["halvings"].data_ptr(), owner.data_ptr(), T,
                                                      result["halvings"].data_ptr(), _stream_ptr(stream)))
        return result

    def _ordered_spread_family(self, obj, order, split_width) -> dict:
        """what the two spread drivers run over on the ordered walk: its calls, its pools, and the halving counts"""
        W = int(split_width)
        return dict(
            solve=functools.partial(self.solve_many_clauses_ordered, order=order, split_width=W),
            resume=self.resume_many_clauses,
            children=lambda pool, slots, stream=None: self.clause_ordered_checkpoint_children(pool, slots, obj, order, stream),
            fanout=lambda pool, slots, offsets, total, stream=None, **kw: self.clause_ordered_checkpoint_fanout(
                pool, slots, obj, order, offsets, total, stream=stream, **kw),
            make_pool=lambda capacity: self.many_clause_ordered_checkpoints(capacity, W),
            slot_bytes=self.clause_ordered_checkpoint_bytes(W), qualifies=self.qualifies_many_clauses(), halvings=True)

    def solve_many_clauses_spread(self, roots, objective="ALL", *, budgets=(256, 4096), max_rounds=64, max_rows=1 << 18,
                                  solutions=True, stream=None, pool_bytes=1 << 30, pools=None, order=None,
                                  split_width=256) -> dict:
        """solve_many_spread for the clause models: solve_many_clauses under ALL whose stopped instances are spread over the
        idle waves, by the same driver over solve_many_clauses, resume_many_clauses, clause_checkpoint_children,
        clause_checkpoint_fanout and fold_many.  The split is exact here too: the kernel runs a root row and a child
        through the same rounds, and under ALL no incumbent narrows a node, so an owner whose sub-instances all ended DONE
        has the record of solve_many_clauses(roots, "ALL"), field for field, and its first solution.  budgets, max_rounds,
        max_rows, solutions, stream, pool_bytes and the answer: as solve_many_spread (no `best`); pools=(a, b): two pools
        of many_clause_checkpoints().  The model must satisfy qualifies_many_clauses(); one that does not is refused as
        solve_many_clauses refuses it.
        objective "MIN" / "MAX" (the model's own sense): the same rounds, pools, max_rows fallback (resume in place),
        max_rounds and answer keys, plus `best` [K].  A MIN / MAX walk's incumbent is sequential, so the split cannot
        reproduce the one call's TREE -- but a stopped walk's untried children are independent sub-problems and any known
        solution value bounds all of them: round 0 is a checkpointed solve_many_clauses under the objective, and every
        child of a later round starts (solve_many_clauses(..., start=)) from the strictly better of its checkpoint's
        incumbent and its owner's best after the fold of the batch it came from.  After every batch the counters are
        folded (fold_many) and an owner's `best` / `first` are replaced only by a strictly better value, from the lowest
        row of the batch that holds it (fold_many_best).  An owner ends with status 0 when all its sub-instances did, else
        1 with the best folded so far (`best` untouched and solutions == 0 if nothing was found).
        Promised: status 0 and `best` are those of solve_many_clauses(roots, objective) with a budget that finishes the
        instance, and the whole answer is deterministic in (roots, budgets, max_rounds, max_rows).
        Not promised: nodes / cuts / props / solutions are those of the walk that was made, which is larger than the one
        call's; `first` is a solution of value `best`, not necessarily the one call's row.
        order (a name of solve_many_clauses_ordered, with split_width): the same two drivers over the ordered walk --
        solve_many_clauses_ordered(..., start=), resume_many_clauses, clause_ordered_checkpoint_children,
        clause_ordered_checkpoint_fanout, two pools of many_clause_ordered_checkpoints(capacity, split_width) -- with the
        same promises against solve_many_clauses_ordered(roots, objective, order=, split_width=).  The answer adds
        `halvings` [K]: an owner's own count, plus 1 for each of its fanned checkpoints whose current node was a halving
        one with neither half tried, plus the counts of its sub-instances (fold_many_halvings, once per batch): under ALL
        the one call's.  None: the plain walk, exactly as before."""
        obj = self.MANY_OBJECTIVES[objective] if isinstance(objective, str) else int(objective)
        assert obj in (1, 2, 3), "solve_many_clauses_spread walks under ALL, or under the model's MIN / MAX"
        if order is not None:
            family = self._ordered_spread_family(obj, order, split_width)
        else:
            family = dict(solve=self.solve_many_clauses, resume=self.resume_many_clauses,
                          children=self.clause_checkpoint_children, fanout=self.clause_checkpoint_fanout,
                          make_pool=self.many_clause_checkpoints, slot_bytes=self.clause_checkpoint_bytes(),
                          qualifies=self.qualifies_many_clauses())
            if obj in (2, 3):
                family.update(
                    children=lambda pool, slots, stream=None: self.clause_checkpoint_children(pool, slots, stream, objective=obj),
                    fanout=functools.partial(self.clause_checkpoint_fanout, objective=obj))
        driver = functools.partial(self._solve_many_clauses_spread_best, obj, family) if obj in (2, 3) else \
            functools.partial(self._solve_many_spread, family)
        return self._spread_call(driver, family["make_pool"], family["slot_bytes"], roots, budgets, max_rounds, max_rows,
                                 solutions, stream, pool_bytes, pools)

    def _solve_many_clauses_spread_best(self, obj, family, sp, roots, max_rounds, max_rows, solutions, stream) -> dict:
        """the driver of solve_many_clauses_spread under MIN / MAX: the rounds of _solve_many_spread, with the incumbents.
        `family`: as there -- `solve` takes `start`, `resume` takes `own_solutions`, `fanout` takes `owner_start` and gives
        (rows, owner, start)"""
        minimise = obj == 2
        solve = family["solve"]
        if not family["qualifies"] or self.objective != obj:  # the call says why, as it does without the spread
            solve(roots, obj, max_nodes=sp.budget(0), solutions=solutions, stream=stream)
        pool = sp.pool_for(0, int(roots.shape[0]))
        main = solve(roots, obj, max_nodes=sp.budget(0), solutions=solutions, stream=stream, checkpoints=pool)
        K, dev = sp.begin(main)
        has = None  # per owner: it holds a solution; its value is main["best"], its row main["first"]
        batch = main
        rounds, round_rows = 1, []

        def leave(last):
            """fold the batch: the counters, then the best values, which replace an owner's only when strictly better; its
            stopped instances without a slot (`last`: all its stopped instances) make their owners LIMIT"""
            nonlocal has
            T = batch["status"].shape[0]
            sp.count_stopped(batch, last)
            if sp.owner is None:
                has = batch["solutions"] > 0
                return
            self.fold_many(batch, sp.owner, main, stream)
            if family.get("halvings"):
                self.fold_many_halvings(batch, sp.owner, main, stream)
            found, value, row = self.fold_many_best(batch, sp.owner, K, obj, stream)
            mine = main["best"]
            take = found & (~has | (value < mine if minimise else value > mine))
            if solutions:
                main["first"].copy_(torch.where(take[:, None], batch["first"][row.clamp(max=max(T - 1, 0))], main["first"]))
            mine.copy_(torch.where(take, value, mine))
            has = has | found

        while rounds < max_rounds and K > 0:
            index = torch.nonzero((batch["status"] == 1) & (batch["slot"] >= 0)).flatten()  # ascending; waits for the batch
            S = int(index.shape[0])
            if S == 0:
                break
            slots = batch["slot"][index].contiguous()
            children, unsplit = sp.counted(family["children"](pool, slots, stream))
            offsets = torch.zeros((S + 1,), dtype=torch.int64, device=dev)
            torch.cumsum(children.clamp(min=0), 0, out=offsets[1:])
            total = int(offsets[-1].item())
            if total > max_rows:  # too wide to fan out: the stopped walks go on where they are
                family["resume"](batch, max_nodes=sp.budget(rounds), stream=stream, own_solutions=sp.owner is not None)
                round_rows.append(0)
                rounds += 1
                continue
            sp.count_refused(index, children)
            if total == 0:
                break
            leave(False)  # before the fan-out: the children start from their owners' best after this fold
            sp.owe(main, index, unsplit)
            whose = sp.owners_of(index)
            owner_start = torch.stack([main["best"][whose], has[whose].to(torch.int32)], 1).contiguous()
            rows, came_from, start = family["fanout"](pool, slots, offsets, total, stream=stream, owner_start=owner_start)
            sp.owner = whose[came_from.long()].to(torch.int32).contiguous()
            pool = sp.pool_for(rounds, total)
            batch = solve(rows, obj, max_nodes=sp.budget(rounds), solutions=solutions, stream=stream, checkpoints=pool,
                          start=start)
            round_rows.append(total)
            rounds += 1
        leave(True)
        return sp.answer(main, rounds, round_rows)

    def _many_symbol(self, export: str):
        """the instantiation a family of solve_many launches for this model (template-id), by the library's `export`;
        None if the model does not qualify"""
        buf = C.create_string_buffer(1024)
        check(getattr(load_library(), export)(self._h, buf, len(buf)))
        return demangle(buf.value.decode()) if buf.value else None

    def many_kernel(self):
        """the cs_dive_shave instantiation solve_many launches"""
        return self._many_symbol("csgpu_internal_many_symbol")

    def many_resume_kernel(self):
        """the cs_dive_resume instantiation the checkpointed calls launch"""
        return self._many_symbol("csgpu_internal_many_resume_symbol")

    def many_upto_kernel(self):
        """the cs_dive_upto instantiation solve_many_upto and its checkpoint calls launch"""
        return self._many_symbol("csgpu_internal_many_upto_symbol")

    def many_allowed_kernel(self):
        """the cs_dive_allowed instantiation solve_many(..., branching="allowed") launches"""
        return self._many_symbol("csgpu_internal_many_allowed_symbol")

    def many_allowed_resume_kernel(self):
        """the cs_dive_allowed_resume instantiation solve_many_allowed(..., checkpoints=pool) and its resume launch"""
        return self._many_symbol("csgpu_internal_many_allowed_resume_symbol")

    def many_allowed_upto_resume_kernel(self):
        """the cs_dive_allowed_upto_resume instantiation of the up-to-k calls with a pool"""
        return self._many_symbol("csgpu_internal_many_allowed_upto_resume_symbol")

    def many_allowed_upto_kernel(self):
        """the cs_dive_allowed_upto instantiation solve_many_upto(..., branching="allowed") launches"""
        return self._many_symbol("csgpu_internal_many_allowed_upto_symbol")

    def many_restart_kernel(self):
        """the cs_dive_restart instantiation solve_many_restarts launches"""
        return self._many_symbol("csgpu_internal_many_restart_symbol")

    def many_waves(self, count: int) -> int:
        """waves a solve_many of `count` instances launches"""
        return int(load_library().csgpu_internal_many_waves(self._h, int(count)))

    def forbidden_words(self) -> int:
        """64-bit words of forbidden-set per variable (0: the model does not qualify)"""
        return load_library().csgpu_model_forbidden_words(self._h)

    def propagate_fb(self, states_in, nodes, forb_in=None, states_out=None, forb_out=None, results=None,
                     want_forb=True, stream=None):
        """Batched propagate_clauses with the forbidden sets carried next to the states.
        forb_in/forb_out: int64 tensors [rows, n_vars, FW] (None = rebuild / not wanted).
        returns (states_out, forb_out, results)"""
        n, fw = self.n_vars, self.forbidden_words()
        assert fw > 0, "model does not qualify for the forbidden-set kernel"
        assert states_in.is_cuda and states_in.dtype == torch.int32 and states_in.is_contiguous()
        assert nodes.is_cuda and nodes.dtype == torch.int32 and nodes.is_contiguous()
        B = nodes.shape[0]
        if states_out is None:
            states_out = torch.empty((B, n, 2), dtype=torch.int32, device=nodes.device)
        if results is None:
            results = torch.empty((B, 4), dtype=torch.int32, device=nodes.device)
        if forb_out is None and want_forb:
            forb_out = torch.empty((B, n, fw), dtype=torch.int64, device=nodes.device)
        if forb_in is not None:
            assert forb_in.dtype == torch.int64 and forb_in.is_contiguous() and forb_in.shape[-2:] == (n, fw)
            assert forb_in.shape[0] == states_in.shape[0]
        check(load_library().csgpu_propagate_batch_fb(
            self._h, states_in.data_ptr(), 0 if forb_in is None else forb_in.data_ptr(), nodes.data_ptr(),
            states_out.data_ptr(), 0 if forb_out is None else forb_out.data_ptr(), results.data_ptr(), B,
            _stream_ptr(stream)))
        return states_out, forb_out, results

    # ---- sets-only states (csgpu_sets_*) ---------------------------------------------------------
    def pack_sets(self, states: torch.Tensor, stream=None) -> torch.Tensor:
        """interval states [k, n_vars, 2] -> sets-only states [k, n_vars, FW] (int64)"""
        n, fw = self.n_vars, self.forbidden_words()
        assert states.is_cuda and states.dtype == torch.int32 and states.is_contiguous() and states.shape[-2:] == (n, 2)
        sets = torch.empty((states.shape[0], n, fw), dtype=torch.int64, device=states.device)
        check(load_library().csgpu_sets_pack(self._h, states.data_ptr(), sets.data_ptr(), states.shape[0], _stream_ptr(stream)))
        return sets

    def unpack_sets(self, sets: torch.Tensor, stream=None) -> torch.Tensor:
        n, fw = self.n_vars, self.forbidden_words()
        assert sets.is_cuda and sets.dtype == torch.int64 and sets.is_contiguous() and sets.shape[-2:] == (n, fw)
        states = torch.empty((sets.shape[0], n, 2), dtype=torch.int32, device=sets.device)
        check(load_library().csgpu_sets_unpack(self._h, sets.data_ptr(), states.data_ptr(), sets.shape[0], _stream_ptr(stream)))
        return states

    def propagate_sets(self, sets_in: torch.Tensor, nodes: torch.Tensor, sets_out: torch.Tensor = None,
                       results: torch.Tensor = None, stream=None):
        """Batched propagate_clauses on sets-only states -> (sets_out [B, n_vars, FW], results [B, 4])"""
        n, fw = self.n_vars, self.forbidden_words()
        assert sets_in.is_cuda and sets_in.dtype == torch.int64 and sets_in.is_contiguous() and sets_in.shape[-2:] == (n, fw)
        assert nodes.is_cuda and nodes.dtype == torch.int32 and nodes.is_contiguous() and nodes.shape[-1] == 4
        B = nodes.shape[0]
        if sets_out is None:
            sets_out = torch.empty((B, n, fw), dtype=torch.int64, device=nodes.device)
        if results is None:
            results = torch.empty((B, 4), dtype=torch.int32, device=nodes.device)
        check(load_library().csgpu_propagate_batch_sets(self._h, sets_in.data_ptr(), nodes.data_ptr(), sets_out.data_ptr(),
                                                        results.data_ptr(), B, _stream_ptr(stream)))
        return sets_out, results

    def eval_root(self, states: torch.Tensor, stream=None) -> torch.Tensor:
        """Three-valued value of the root wide-and per state: 1 true, 0 false, 2 undecided."""
        assert states.is_cuda and states.dtype == torch.int32 and states.is_contiguous()
        B = states.shape[0]
        truth = torch.empty((B,), dtype=torch.int32, device=states.device)
        check(load_library().csgpu_eval_batch(self._h, states.data_ptr(), truth.data_ptr(), B, _stream_ptr(stream)))
        return truth

    def eval_clauses(self, state: torch.Tensor, stream=None) -> torch.Tensor:
        """Interval value of every clause for ONE state: [n_clauses, 2]."""
        assert state.is_cuda and state.dtype == torch.int32 and state.is_contiguous()
        out = torch.empty((max(1, self.n_clauses), 2), dtype=torch.int32, device=state.device)
        check(load_library().csgpu_eval_clauses(self._h, state.data_ptr(), out.data_ptr(), _stream_ptr(stream)))
        return out[: self.n_clauses]

    def propagate_one(self, state: np.ndarray, var: int, lo: int, hi: int):
        """Single node through host buffers (the drop-in path)."""
        state = np.ascontiguousarray(state, dtype=np.int32)
        out = np.empty_like(state)
        res = Result()
        check(load_library().csgpu_propagate_one(self._h, state.ctypes.data, Node(var, lo, hi, 0),
                                                 out.ctypes.data, C.byref(res)))
        return res.status, res.props, out


    def propagate_one_causes(self, state: np.ndarray, var: int, lo: int, hi: int, cap: int = 4096):
        """One node of a pure != network with the cause of every bound move (csgpu_propagate_one_causes).
        -> (status, props, fixpoint or None, trace [k, 4] = {variable, 0 lo / 1 hi, new bound, causing variable})"""
        state = np.ascontiguousarray(state, dtype=np.int32)
        out = np.empty_like(state)
        res = Result()
        trace = np.empty((cap, 4), dtype=np.int32)
        cnt = C.c_int32()
        check(load_library().csgpu_propagate_one_causes(self._h, state.ctypes.data, Node(var, lo, hi, 0), out.ctypes.data,
                                                        C.byref(res), trace.ctypes.data, cap, C.byref(cnt)))
        if cnt.value > min(cap, 2048):
            raise OverflowError(f"{cnt.value} trace records, {min(cap, 2048)} kept")
        return res.status, res.props, (out if res.status >= 0 else None), trace[: cnt.value].copy()

    def propagate_one_chain(self, state: np.ndarray, var: int, lo: int, hi: int, cap: int = 4096):
        """The reference's own failure chain of one node (csgpu_propagate_one_chain).
        -> (status -1 / 0, props, bumped variables in the reference's order)"""
        state = np.ascontiguousarray(state, dtype=np.int32)
        st, props, cnt = C.c_int32(), C.c_int32(), C.c_int32()
        bumps = np.empty(cap, dtype=np.int32)
        check(load_library().csgpu_propagate_one_chain(self._h, state.ctypes.data, Node(var, lo, hi, 0), C.byref(st),
                                                        C.byref(props), bumps.ctypes.data, cap, C.byref(cnt)))
        return st.value, props.value, bumps[: min(cap, cnt.value)].copy()

    def propagate_one_traced(self, state: np.ndarray, var: int, lo: int, hi: int, cap: int = 4096):
        """One node with its trail (csgpu_propagate_one_traced).
        -> (status, props, fixpoint or None, trace [k, 4] = {variable, 0 lo / 1 hi / 2 failure, new bound, clause})"""
        state = np.ascontiguousarray(state, dtype=np.int32)
        out = np.empty_like(state)
        res = Result()
        trace = np.empty((cap, 4), dtype=np.int32)
        cnt = C.c_int32()
        check(load_library().csgpu_propagate_one_traced(self._h, state.ctypes.data, Node(var, lo, hi, 0), out.ctypes.data,
                                                        C.byref(res), trace.ctypes.data, cap, C.byref(cnt)))
        if cnt.value > cap:
            raise OverflowError(f"{cnt.value} trace records, room for {cap}")
        return res.status, res.props, (out if res.status >= 0 else None), trace[: cnt.value].copy()

    def propagate_values(self, state: np.ndarray, var: int, values):
        """Several values of `var` on one parent state, host buffers (the drop-in's sibling batch).
        -> (results [count, 4], states_out [count, n_vars, 2]); rows of inconsistent nodes are unspecified"""
        state = np.ascontiguousarray(state, dtype=np.int32)
        values = np.ascontiguousarray(values, dtype=np.int32)
        outs = np.empty((len(values),) + state.shape, dtype=np.int32)
        res = np.empty((len(values), 4), dtype=np.int32)
        check(load_library().csgpu_propagate_values(self._h, state.ctypes.data, var, values.ctypes.data, len(values),
                                                    outs.ctypes.data, res.ctypes.data))
        return res, outs

    def server_stats(self):
        """-> (calls, starts): single-node calls answered by the resident server or kernel 7's tracing launch, and the
        server's (re)starts, for this model (csgpu_debug_one_timing)"""
        seconds, calls, starts = (C.c_double * 4)(), C.c_uint64(), C.c_uint64()
        check(load_library().csgpu_debug_one_timing(self._h, seconds, C.byref(calls), C.byref(starts)))
        return calls.value, starts.value

    def root_propagate_limit(self, limit: int):
        """propagate(root, limit): at most limit + 1 sweeps.  -> (status, rounds)"""
        st, rounds = C.c_int32(), C.c_int32()
        check(load_library().csgpu_model_root_propagate_limit(self._h, limit, C.byref(st), C.byref(rounds)))
        return st.value, rounds.value


class _SpreadRounds:
    """what the rounds of the two spread drivers share (Model._solve_many_spread, Model._solve_many_clauses_spread_best):
    the two alternating pools, the budgets, the owners of a batch's rows, the owners that end LIMIT and the answer.
    pools: the caller's two, or None: pools of make_pool() that go with the call"""

    def __init__(self, make_pool, slot_bytes, budgets, stream, pool_bytes, pools):
        self.make_pool, self.slot_bytes, self.budgets, self.stream = make_pool, max(slot_bytes, 1), budgets, stream
        self.pool_bytes, self.own_pools = pool_bytes, pools is None
        self.pools = [None, None] if pools is None else list(pools)
        self.owner = None  # int32 [T]: the owner of every row of the batch; None for round 0 (every instance is its own)

    def pool_for(self, rnd, batch):
        """the pool of round `rnd`, empty: the one of round rnd - 1 is still read by the fan-out"""
        k = rnd % 2
        need = max(1, min(batch, self.pool_bytes // self.slot_bytes))
        if self.own_pools and (self.pools[k] is None or self.pools[k].capacity < need):
            if self.pools[k] is not None:
                self.pools[k].close()
            self.pools[k] = self.make_pool(need)
        else:
            self.pools[k].reset(self.stream)
        return self.pools[k]

    def budget(self, rnd):
        return self.budgets[min(rnd, len(self.budgets) - 1)]

    def begin(self, main):
        """round 0's answer `main` holds the owners -> (K, their device)"""
        self.K, self.dev = main["status"].shape[0], main["status"].device
        self.limited = torch.zeros((max(self.K, 1),), dtype=torch.int32, device=self.dev)  # owners that end LIMIT
        return self.K, self.dev

    def owners_of(self, index):
        return index if self.owner is None else self.owner.long()[index]

    def count_stopped(self, batch, last):
        """the batch is left: its stopped instances without a slot (`last`: all its stopped instances) make their owners
        LIMIT -> the batch's row numbers"""
        rows = torch.arange(batch["status"].shape[0], dtype=torch.int64, device=self.dev)
        stopped = batch["status"] == 1
        if not last:
            stopped = stopped & (batch["slot"] < 0)
        stopped = stopped | (batch["status"] == 3)  # (a resume in place refused its slot: BAD_SLOT)
        self.limited.index_add_(0, self.owners_of(rows), stopped.to(torch.int32))
        return rows

    @staticmethod
    def counted(children):
        """what a family's `children` gave -> (children, unsplit): unsplit is None for a walk without halving counts"""
        return children if isinstance(children, tuple) else (children, None)

    def owe(self, main, index, unsplit):
        """the stopped instances `index` are fanned out: the halving each owes (its current node had neither half tried,
        so no record counts that parent) goes to its owner, once"""
        if unsplit is not None:
            main["halvings"].index_add_(0, self.owners_of(index), unsplit.to(torch.int64))

    def count_refused(self, index, children):
        """refused slots (children < 0) among the stopped instances `index`: their work is lost"""
        self.limited.index_add_(0, self.owners_of(index), (children < 0).to(torch.int32))

    def answer(self, main, rounds, round_rows):
        status = main["status"]
        status.copy_(torch.where(status == 2, status, (self.limited[:self.K] > 0).to(status.dtype)))
        if self.own_pools:
            torch.cuda.current_stream().synchronize()  # the pools go with the call
        out = {k: v for k, v in main.items() if not k.startswith("_") and k != "slot"}
        out["rounds"], out["sub_instances"], out["round_rows"] = rounds, sum(round_rows), round_rows
        return out


class ManyCheckpoints:
    """A pool of checkpoint slots of one finalized model (csgpu_many_checkpoints), of one of four kinds: for solve_many
    (Model.many_checkpoints), for solve_many_clauses (Model.many_clause_checkpoints), for solve_many_clauses_ordered
    (Model.many_clause_ordered_checkpoints) or for solve_many_clauses_wide (Model.many_clause_wide_checkpoints).  It
    holds the model."""

    def __init__(self, model: Model, capacity: int, clauses: bool = False, split_width=None, wide: bool = False):
        self.model = model
        self.capacity = int(capacity)
        self.clauses = bool(clauses)  # the kind: of solve_many_clauses (csgpu_many_clause_checkpoints_create), else of solve_many
        # the third kind, of solve_many_clauses_ordered (csgpu_many_clause_ordered_checkpoints_create): made for one
        # split_width, a slot has `frames` + 1 frames
        self.ordered = split_width is not None
        self.split_width = int(split_width) if self.ordered else None
        # the fourth kind, of solve_many_clauses_wide (csgpu_many_clause_wide_checkpoints_create)
        self.wide = bool(wide)
        self._h = C.c_void_p()
        L = load_library()
        if self.ordered:
            assert self.clauses, "an ordered pool is a clause pool"
            check(L.csgpu_many_clause_ordered_checkpoints_create(model._h, self.capacity, self.split_width, C.byref(self._h)))
            self.frames = model.many_clauses_ordered_frames(self.split_width)
            return
        if self.wide:
            assert self.clauses, "a wide pool is a clause pool"
            check(L.csgpu_many_clause_wide_checkpoints_create(model._h, self.capacity, C.byref(self._h)))
            return
        create = L.csgpu_many_clause_checkpoints_create if self.clauses else L.csgpu_many_checkpoints_create
        check(create(model._h, self.capacity, C.byref(self._h)))

    def reset(self, stream=None):
        """every slot free again (asynchronous on the stream)"""
        check(load_library().csgpu_many_checkpoints_reset(self._h, _stream_ptr(stream)))
        return self

    def close(self):
        if self._h:
            load_library().csgpu_many_checkpoints_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ManySolutionStream:
    """The solution stream of Model.solve_many_stream (csgpu_many_stream): `rows` int32 [capacity, n_vars], `owner` int32
    [capacity] and `count`, one 64-bit device word that counts append attempts since it was last zeroed.  The kernel only
    adds to it: after a call the valid rows are the first min(count, capacity)."""

    def __init__(self, model: Model, rows: int):
        self.capacity = int(rows)  # (below 1: kept as given, so that the library refuses the call)
        cap = max(self.capacity, 1)
        self.rows = torch.empty((cap, model.n_vars), dtype=torch.int32, device="cuda")
        self.owner = torch.empty((cap,), dtype=torch.int32, device="cuda")
        self.count = torch.zeros((1,), dtype=torch.int64, device="cuda")

    def struct(self) -> ManyStream:
        return ManyStream(self.rows.data_ptr(), self.owner.data_ptr(), self.count.data_ptr(), self.capacity)

    def take(self):
        """-> (owner int32 [m], rows int32 [m, n_vars]): copies of the valid part, in stream order; the counter is zeroed
        on the current stream.  Waits for the calls queued before it."""
        m = min(int(self.count.item()), max(self.capacity, 0))
        owner, rows = self.owner[:m].clone(), self.rows[:m].clone()
        self.count.zero_()
        return owner, rows


def set_linear_fast_paths(on: bool):
    """Process-wide: whether models finalized from now on revise EQ / LT / two-literal OR clauses by direct
    bound propagation (default) or through the expression-tree interpreter (csgpu_set_linear_fast_paths)."""
    load_library().csgpu_set_linear_fast_paths(1 if on else 0)


class Search:
    """Device-resident tree search over a finalized model (csgpu_search_*): a LIFO pool of open
    states in HBM, expanded and propagated in batches.  One instance per GPU/rank."""

    def __init__(self, model: Model, pool_capacity: int = 1 << 20, max_children: int = 1 << 16):
        self.model = model
        self._h = C.c_void_p()
        check(load_library().csgpu_search_create(model._h, pool_capacity, max_children, C.byref(self._h)))
        self.device = torch.device("cuda", torch.cuda.current_device())  # the engine's (csgpu_search_create's)
        self.stats = None  # iter_solutions: the statistics of the finished run

    def close(self):
        if self._h:
            load_library().csgpu_search_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """forget pool, statistics, incumbent and seeds; keep the buffers"""
        check(load_library().csgpu_search_reset(self._h))

    def put(self, states: torch.Tensor):
        """append open states [k, n_vars, 2] (device) to the pool"""
        if states.numel() == 0:
            return
        assert states.is_cuda and states.dtype == torch.int32 and states.is_contiguous()
        assert states.shape[-2:] == (self.model.n_vars, 2)
        check(load_library().csgpu_search_put(self._h, states.data_ptr(), states.shape[0]))

    def take(self, max_states: int) -> torch.Tensor:
        """remove up to max_states of the oldest open states (largest subtrees)"""
        buf = torch.empty((max(1, max_states), self.model.n_vars, 2), dtype=torch.int32, device="cuda")
        cnt = C.c_int64()
        check(load_library().csgpu_search_take(self._h, buf.data_ptr(), max_states, C.byref(cnt)))
        return buf[: cnt.value]

    def set_parents(self, parents_per_iteration: int):
        check(load_library().csgpu_search_set_parents(self._h, int(parents_per_iteration)))

    def set_restart(self, iterations: int):
        check(load_library().csgpu_search_set_restart(self._h, int(iterations)))

    ORDERS = {"none": 0, "smallest-domain": 1, "largest-domain": 2, "smallest-value": 3, "largest-value": 4}

    def set_strategy(self, order="smallest-domain", prefer_failing: bool = False):
        """the reference's -o / -f (csgpu_search_set_strategy): set before the first state is put"""
        o = self.ORDERS[order] if isinstance(order, str) else int(order)
        check(load_library().csgpu_search_set_strategy(self._h, o, int(bool(prefer_failing))))

    def set_restart_on_improvement(self, on: bool = True):
        """MIN / MAX: restart from the seeds on every better solution (csolve.c:418-425)"""
        check(load_library().csgpu_search_set_restart_on_improvement(self._h, int(bool(on))))

    def share_incumbent(self, other: "Search"):
        """keep the incumbent in `other`'s word of device memory (MIN / MAX engines of one model on one device).
        While shared, set_parents beyond the device-driven limit is refused, best_solution() answers only on the
        engine whose own row attains the incumbent, and the library keeps the lender's memory until the last
        borrower is freed."""
        check(load_library().csgpu_search_share_incumbent(self._h, other._h))

    def set_best(self, best: int):
        check(load_library().csgpu_search_set_best(self._h, int(best)))

    def put_cost(self):
        """-> (seconds, states): host time put() has taken since reset() (copy + rebuilding the forbidden sets)"""
        sec, cnt = C.c_double(), C.c_int64()
        check(load_library().csgpu_search_put_cost(self._h, C.byref(sec), C.byref(cnt)))
        return sec.value, cnt.value

    def run(self, max_iterations: int = 1 << 62) -> dict:
        st = SearchStats()
        check(load_library().csgpu_search_run(self._h, max_iterations, C.byref(st)))
        return {k: getattr(st, k) for k, _ in SearchStats._fields_}

    def best_solution(self):
        """MIN/MAX: values of a solution attaining the incumbent, or None"""
        out = np.empty(self.model.n_vars, dtype=np.int32)
        rc = check(load_library().csgpu_search_best_solution(self._h, out.ctypes.data))
        return out if rc == 1 else None

    def solutions(self, max_solutions: int = 1024) -> np.ndarray:
        out = np.empty((max(1, max_solutions), self.model.n_vars), dtype=np.int32)
        k = load_library().csgpu_search_solutions(self._h, out.ctypes.data, max_solutions)
        check(k)
        return out[:k]

    # ---- the solution stream (csgpu_search_set_solution_stream) ----------------------------------------------------
    DEFAULT_STREAM_ROWS = 1 << 18

    def stream_solutions(self, rows: int | None = None):
        """turn the solution stream on with room for `rows` rows (before the first put): ALL streams every solution,
        ANY its one, MIN / MAX each improving one.  run() then returns early (done 0) when the stream is too full for
        its next iteration; drain and run on."""
        check(load_library().csgpu_search_set_solution_stream(self._h, int(rows or self.DEFAULT_STREAM_ROWS)))

    def pending_solutions(self):
        """-> (rows waiting, rows of room)"""
        rows, room = C.c_int64(), C.c_int64()
        check(load_library().csgpu_search_pending_solutions(self._h, C.byref(rows), C.byref(room)))
        return rows.value, room.value

    def drain_solutions(self, max_rows: int | None = None) -> np.ndarray:
        """every waiting row (at most max_rows), oldest first: [k, n_vars] int32 (host)"""
        rows, _ = self.pending_solutions()
        rows = rows if max_rows is None else min(rows, int(max_rows))
        out = np.empty((max(1, rows), self.model.n_vars), dtype=np.int32)
        cnt = C.c_int64()
        check(load_library().csgpu_search_drain_solutions(self._h, out.ctypes.data, rows, C.byref(cnt)))
        return out[: cnt.value]

    def drain_solutions_device(self, max_rows: int | None = None) -> torch.Tensor:
        """every waiting row (at most max_rows), oldest first: [k, n_vars] int32 on the engine's device (no host copy of
        the rows)"""
        rows, _ = self.pending_solutions()
        rows = rows if max_rows is None else min(rows, int(max_rows))
        out = torch.empty((max(1, rows), self.model.n_vars), dtype=torch.int32, device=self.device)
        cnt = C.c_int64()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream()
        check(load_library().csgpu_search_drain_solutions_device(self._h, out.data_ptr(), rows, C.byref(cnt),
                                                                 int(stream.cuda_stream)))
        return out[: cnt.value]

    def iter_solutions(self, slice_iterations: int = 64, device: bool = False):
        """run the search to its end in slices of `slice_iterations`, yielding every drained batch of rows (numpy, or
        torch on the engine's device); the final statistics are left in self.stats.  Turns the stream on with its
        default size if it is off."""
        try:
            self.pending_solutions()
        except CsolveError:
            self.stream_solutions()
        drain = self.drain_solutions_device if device else self.drain_solutions
        while True:
            st = self.run(slice_iterations)
            batch = drain()
            if len(batch):
                yield batch
            if st["done"]:
                break
        self.stats = st


def solve_root(text: str, weights_on: bool = True) -> Model:
    """Front end + root phase + finalize: parser.y's Input action up to clauses_init
    (propagate, normalize, propagate, env_generate, clauses_init)."""
    m = Model.from_text(text, weights_on)
    if m.root_propagate() < 0:
        raise ValueError("INFEASIBLE PROBLEM")
    m.normalize()
    if m.root_propagate() < 0:
        raise ValueError("INFEASIBLE PROBLEM")
    return m.finalize()
