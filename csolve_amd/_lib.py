"""ctypes loader of libcsolve_hip.so (the product's only compute path)."""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CSOLVE_HIP_LIB") or os.path.join(_HERE, "libcsolve_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "csolve_gpu.h")


class CsolveError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"csolve_gpu error {code}: {message}")
        self.code = code


class Val(C.Structure):
    _fields_ = [("lo", C.c_int32), ("hi", C.c_int32)]


class Node(C.Structure):
    _fields_ = [("var", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("parent", C.c_int32)]


class SearchStats(C.Structure):
    _fields_ = [("nodes", C.c_uint64), ("cuts", C.c_uint64), ("props", C.c_uint64), ("revisions", C.c_uint64),
                ("solutions", C.c_uint64), ("iterations", C.c_uint64), ("restarts", C.c_uint64), ("pool", C.c_int64), ("pool_peak", C.c_int64),
                ("best", C.c_int32), ("done", C.c_int32)]


# csgpu_shard_solution_fn: (user, rank, rows, count, best)
SHARD_SOLUTION_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int64, C.c_int32)


class ShardOptions(C.Structure):
    _fields_ = [("slice_iterations", C.c_int64), ("poll_iterations", C.c_int64), ("seed_states_per_rank", C.c_int64),
                ("low_water", C.c_int64), ("time_limit", C.c_double), ("on_solution", SHARD_SOLUTION_FN),
                ("user", C.c_void_p)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("props", C.c_int32), ("revisions", C.c_int32), ("rounds", C.c_int32)]


# csgpu_solve_many: status of an instance
MANY_DONE, MANY_LIMIT, MANY_BAD_ROOT = 0, 1, 2
MANY_BAD_SLOT = 3  # csgpu_solve_many_resume: the slot number names no checkpoint


class ManyResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("root_props", C.c_int32), ("nodes", C.c_int64), ("cuts", C.c_int64),
                ("props", C.c_int64), ("solutions", C.c_int64)]


class ManyOptions(C.Structure):
    _fields_ = [("objective", C.c_int32), ("reserved", C.c_int32), ("max_nodes", C.c_int64)]


class ManyUptoOptions(C.Structure):
    """csgpu_many_upto_options: an instance stops at its max_solutions-th solution"""
    _fields_ = [("max_solutions", C.c_int32), ("reserved", C.c_int32), ("max_nodes", C.c_int64)]


class ManyOrderOptions(C.Structure):
    """csgpu_many_order_options: a variable order of the engine's five, and the width above which an interval is halved"""
    _fields_ = [("objective", C.c_int32), ("order", C.c_int32), ("split_width", C.c_int32), ("reserved", C.c_int32),
                ("max_nodes", C.c_int64)]


MANY_ROTATE_FIRST = 1  # CSGPU_MANY_ROTATE_FIRST


class ManyRestartOptions(C.Structure):
    """csgpu_many_restart_options: Luby restarts (restart_base x 1 1 2 1 1 2 4 ... failures) with a seeded value order"""
    _fields_ = [("max_nodes", C.c_int64), ("restart_base", C.c_int64), ("seed", C.c_uint32), ("flags", C.c_int32)]


MANY_FULL = 4         # CSGPU_MANY_FULL: stopped because the solution stream had no room
MANY_SLOT_FRESH = -2  # CSGPU_MANY_SLOT_FRESH: d_slots[i] on entry, start instance i from its root row


class ManyStream(C.Structure):
    """csgpu_many_stream: the solution stream of csgpu_solve_many_stream, caller-owned device memory"""
    _fields_ = [("d_rows", C.c_void_p), ("d_owner", C.c_void_p), ("d_count", C.c_void_p), ("capacity", C.c_int64)]


def declared_symbols(header: str = HEADER_PATH):
    """Names of every function declared in include/csolve_gpu.h."""
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(csgpu_\w+)\s*\(", text)))


# kernel families of a model's plan, in the order of csgpu_internal_plan_symbol (cs_internal.h)
PLAN_FAMILIES = ("events", "traced", "rounds", "lds", "bitset", "regs0", "regs1", "regs2", "regs3", "packed",
                 "shave", "shave_trace", "server", "step_shave", "step_packed", "step_import")

_lib = None
_demangler = None


def demangle(symbol: str) -> str:
    """The template-id of a mangled kernel symbol, e.g. `cs_propagate_ne_lds<unsigned short, 4, 1, true>`: the
    C++ runtime's demangler, return type and parameter list dropped."""
    global _demangler
    if _demangler is None:
        cxx = C.CDLL("libstdc++.so.6")
        cxx.__cxa_demangle.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        cxx.__cxa_demangle.restype = C.c_void_p
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        _demangler = (cxx.__cxa_demangle, libc.free)
    fn, free = _demangler
    status = C.c_int()
    p = fn(symbol.encode(), None, None, C.byref(status))
    if status.value != 0 or not p:
        raise ValueError(f"cannot demangle {symbol!r}")
    try:
        text = C.string_at(p).decode()
    finally:
        free(p)
    if text.startswith("void "):
        text = text[5:]
    depth = 0
    for i, ch in enumerate(text):  # cut at the parameter list: the first '(' outside the template arguments
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return text[:i]
    return text


def load_library():
    """Load libcsolve_hip.so or raise -- there is nothing to fall back to."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C csolve_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch carries its own libamdhip64.so.7; load it first so the process has ONE HIP runtime
    # and device pointers / streams handed over from torch belong to the runtime we launch on.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.csgpu_last_error.restype = C.c_char_p
    L.csgpu_device_count.restype = C.c_int
    L.csgpu_set_device.argtypes = [C.c_int]
    L.csgpu_model_from_text.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.csgpu_model_from_file.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.csgpu_model_from_dump.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.csgpu_model_free.argtypes = [vp]
    L.csgpu_model_free.restype = None
    for f in ("csgpu_model_num_vars", "csgpu_model_num_clauses", "csgpu_model_objective",
              "csgpu_model_objective_var"):
        getattr(L, f).argtypes = [vp]
    L.csgpu_model_var_name.argtypes = [vp, C.c_int]
    L.csgpu_model_var_name.restype = C.c_char_p
    L.csgpu_model_get_domains.argtypes = [vp, vp]
    L.csgpu_model_set_domains.argtypes = [vp, vp]
    L.csgpu_model_device_info.argtypes = [vp, C.POINTER(i64)]
    L.csgpu_model_root_propagate.argtypes = [vp, C.POINTER(i32)]
    L.csgpu_model_finalize.argtypes = [vp]
    L.csgpu_model_normalize.argtypes = [vp]
    L.csgpu_model_specialize.argtypes = [vp, vp, C.POINTER(vp)]
    L.csgpu_model_build_tables.argtypes = [vp]
    L.csgpu_model_eval_clauses_host.argtypes = [vp, vp]
    L.csgpu_model_set_kernel.argtypes = [vp, C.c_int]
    L.csgpu_model_qualifies.argtypes = [vp, C.c_int]
    L.csgpu_set_linear_fast_paths.argtypes = [C.c_int]
    L.csgpu_sets_pack.argtypes = [vp, vp, vp, i64, vp]
    L.csgpu_sets_unpack.argtypes = [vp, vp, vp, i64, vp]
    L.csgpu_propagate_batch_sets.argtypes = [vp, vp, vp, vp, vp, i64, vp]
    L.csgpu_set_linear_fast_paths.restype = None
    L.csgpu_model_get_kernel.argtypes = [vp]
    L.csgpu_propagate_batch.argtypes = [vp, vp, vp, vp, vp, i64, vp]
    L.csgpu_propagate_batch_obj.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, vp]
    # the incumbent read from device memory (cs_internal.h): what the device-driven search iterations launch; tests only
    L.csgpu_internal_propagate_objdev.argtypes = [vp, vp, vp, vp, vp, i64, vp, i32, i32, vp, C.c_int, vp]
    L.csgpu_internal_propagate_fb.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, vp]
    L.csgpu_internal_shave_launch.argtypes = [vp, i64, C.POINTER(i64 * 3)]
    L.csgpu_model_forbidden_words.argtypes = [vp]
    L.csgpu_propagate_batch_fb.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp]
    L.csgpu_eval_batch.argtypes = [vp, vp, vp, i64, vp]
    L.csgpu_eval_clauses.argtypes = [vp, vp, vp, vp]
    L.csgpu_search_create.argtypes = [vp, i64, i64, C.POINTER(vp)]
    L.csgpu_search_free.argtypes = [vp]
    L.csgpu_search_free.restype = None
    L.csgpu_search_reset.argtypes = [vp]
    L.csgpu_search_put.argtypes = [vp, vp, i64]
    L.csgpu_search_put_host.argtypes = [vp, vp, i64]
    L.csgpu_search_take.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.csgpu_search_take_host.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.csgpu_plan_transfers.argtypes = [vp, C.c_int, i64, i64, vp, C.POINTER(C.c_int)]
    L.csgpu_shard_region_size.argtypes = [C.c_int, C.c_int, i64, C.POINTER(C.c_size_t)]
    L.csgpu_shard_region_init.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, i64]
    L.csgpu_shard_barrier.argtypes = [vp]
    L.csgpu_text_num_vars.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    L.csgpu_shard_default_options.argtypes = [C.POINTER(ShardOptions)]
    L.csgpu_shard_default_options.restype = None
    L.csgpu_shard_run.argtypes = [vp, vp, C.c_int, vp, C.POINTER(ShardOptions), C.POINTER(SearchStats),
                                  C.POINTER(SearchStats)]
    L.csgpu_search_set_best.argtypes = [vp, i32]
    L.csgpu_model_add_conflict.argtypes = [vp, i32, vp, vp]
    L.csgpu_search_put_cost.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i64)]
    L.csgpu_objective_better.argtypes = [C.c_int, Val, i32]
    L.csgpu_objective_bound.argtypes = [C.c_int, Val, i32]
    L.csgpu_objective_bound.restype = Val
    L.csgpu_objective_best.argtypes = [C.c_int, Val, i32]
    L.csgpu_objective_best.restype = i32
    L.csgpu_luby_next.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.csgpu_luby_next.restype = None
    L.csgpu_step_check.argtypes = [Val, C.c_uint32]
    L.csgpu_step_val.argtypes = [Val, C.c_uint32, C.c_uint32]
    L.csgpu_step_val.restype = i32
    L.csgpu_search_share_incumbent.argtypes = [vp, vp]
    L.csgpu_search_set_parents.argtypes = [vp, i64]
    L.csgpu_search_set_restart.argtypes = [vp, i64]
    L.csgpu_search_run.argtypes = [vp, i64, C.POINTER(SearchStats)]
    L.csgpu_search_solutions.argtypes = [vp, vp, i64]
    L.csgpu_search_best_solution.argtypes = [vp, vp]
    L.csgpu_search_solutions.restype = i64
    L.csgpu_search_set_solution_stream.argtypes = [vp, i64]
    L.csgpu_search_drain_solutions.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.csgpu_search_drain_solutions_device.argtypes = [vp, vp, i64, C.POINTER(i64), vp]
    L.csgpu_search_pending_solutions.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.csgpu_propagate_one.argtypes = [vp, vp, Node, vp, C.POINTER(Result)]
    L.csgpu_propagate_one_traced.argtypes = [vp, vp, Node, vp, C.POINTER(Result), vp, i32, C.POINTER(i32)]
    L.csgpu_propagate_one_causes.argtypes = [vp, vp, Node, vp, C.POINTER(Result), vp, i32, C.POINTER(i32)]
    L.csgpu_propagate_values.argtypes = [vp, vp, i32, vp, i32, vp, vp]
    L.csgpu_model_root_propagate_limit.argtypes = [vp, i64, C.POINTER(i32), C.POINTER(i32)]
    L.csgpu_propagate_one_chain.argtypes = [vp, vp, Node, C.POINTER(i32), C.POINTER(i32), vp, i32, C.POINTER(i32)]
    L.csgpu_search_set_strategy.argtypes = [vp, C.c_int, C.c_int]
    L.csgpu_search_set_restart_on_improvement.argtypes = [vp, C.c_int]
    L.csgpu_internal_plan_symbol.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t]
    L.csgpu_solve_many.argtypes = [vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp]
    L.csgpu_internal_many_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_internal_many_waves.argtypes = [vp, i64]
    L.csgpu_internal_many_waves.restype = i64
    L.csgpu_internal_many_resume_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_many_checkpoint_bytes.argtypes = [vp]
    L.csgpu_many_checkpoint_bytes.restype = C.c_size_t
    L.csgpu_many_checkpoints_create.argtypes = [vp, i64, C.POINTER(vp)]
    L.csgpu_many_checkpoints_reset.argtypes = [vp, vp]
    L.csgpu_many_checkpoints_free.argtypes = [vp]
    L.csgpu_many_checkpoints_free.restype = None
    L.csgpu_solve_many_checkpointed.argtypes = [vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp, vp]
    L.csgpu_solve_many_resume.argtypes = [vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp, vp]
    L.csgpu_many_checkpoint_states.argtypes = [vp, C.c_int32, vp, i64, C.POINTER(i64), vp]
    L.csgpu_many_checkpoint_children.argtypes = [vp, vp, i64, vp, vp]
    L.csgpu_many_checkpoint_fanout.argtypes = [vp, vp, i64, vp, vp, vp, i64, vp]
    L.csgpu_many_fold.argtypes = [vp, vp, i64, vp, vp]
    L.csgpu_solve_many_upto.argtypes = [vp, vp, i64, C.POINTER(ManyUptoOptions), vp, vp, vp]
    L.csgpu_solve_many_upto_checkpointed.argtypes = [vp, vp, i64, C.POINTER(ManyUptoOptions), vp, vp, vp, vp, vp]
    L.csgpu_solve_many_upto_resume.argtypes = [vp, i64, C.POINTER(ManyUptoOptions), vp, vp, vp, vp, vp]
    L.csgpu_internal_many_upto_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_model_qualifies_many_allowed.argtypes = [vp]
    L.csgpu_solve_many_allowed.argtypes = [vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp]
    L.csgpu_solve_many_allowed_upto.argtypes = [vp, vp, i64, C.POINTER(ManyUptoOptions), vp, vp, vp]
    L.csgpu_internal_many_allowed_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_internal_many_allowed_upto_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_solve_many_allowed_checkpointed.argtypes = [vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp, vp]
    L.csgpu_solve_many_allowed_resume.argtypes = [vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp, vp]
    L.csgpu_solve_many_allowed_upto_checkpointed.argtypes = [vp, vp, i64, C.POINTER(ManyUptoOptions), vp, vp, vp, vp, vp]
    L.csgpu_solve_many_allowed_upto_resume.argtypes = [vp, i64, C.POINTER(ManyUptoOptions), vp, vp, vp, vp, vp]
    L.csgpu_many_allowed_checkpoint_children.argtypes = [vp, vp, i64, vp, vp]
    L.csgpu_many_allowed_checkpoint_fanout.argtypes = [vp, vp, i64, vp, vp, vp, i64, vp]
    L.csgpu_internal_many_allowed_resume_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_internal_many_allowed_upto_resume_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_solve_many_restarts.argtypes = [vp, vp, vp, i64, C.POINTER(ManyRestartOptions), vp, vp, vp, vp]
    L.csgpu_internal_many_restart_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_solve_many_stream.argtypes = [vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp, C.POINTER(ManyStream), vp]
    L.csgpu_internal_many_stream_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_solve_many_clauses.argtypes = [vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp]
    L.csgpu_model_qualifies_many_clauses.argtypes = [vp]
    L.csgpu_internal_many_clauses_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_internal_many_clauses_waves.argtypes = [vp, i64]
    L.csgpu_internal_many_clauses_waves.restype = i64
    L.csgpu_internal_many_clauses_resume_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_many_clause_checkpoint_bytes.argtypes = [vp]
    L.csgpu_many_clause_checkpoint_bytes.restype = C.c_size_t
    L.csgpu_many_clause_checkpoints_create.argtypes = [vp, i64, C.POINTER(vp)]
    L.csgpu_solve_many_clauses_checkpointed.argtypes = [vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp, vp, vp]
    L.csgpu_solve_many_clauses_resume.argtypes = [vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp, vp, vp]
    L.csgpu_many_clause_checkpoint_states.argtypes = [vp, C.c_int32, vp, i64, C.POINTER(i64), C.POINTER(C.c_int32),
                                                      C.POINTER(C.c_int32), vp]
    L.csgpu_many_clause_checkpoint_children.argtypes = [vp, vp, i64, vp, vp]
    L.csgpu_many_clause_checkpoint_fanout.argtypes = [vp, vp, i64, vp, vp, vp, i64, vp]
    L.csgpu_solve_many_clauses_upto.argtypes = [vp, vp, i64, C.POINTER(ManyUptoOptions), vp, vp, vp]
    L.csgpu_solve_many_clauses_upto_checkpointed.argtypes = [vp, vp, i64, C.POINTER(ManyUptoOptions), vp, vp, vp, vp, vp]
    L.csgpu_solve_many_clauses_upto_resume.argtypes = [vp, i64, C.POINTER(ManyUptoOptions), vp, vp, vp, vp, vp]
    L.csgpu_internal_many_clauses_upto_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_solve_many_clauses_restarts.argtypes = [vp, vp, vp, i64, C.POINTER(ManyRestartOptions), vp, vp, vp, vp]
    L.csgpu_internal_many_clauses_restart_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_solve_many_clauses_stream.argtypes = [vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp, C.POINTER(ManyStream), vp]
    L.csgpu_internal_many_clauses_stream_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_solve_many_clauses_from.argtypes = [vp, vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp, vp, vp]
    L.csgpu_solve_many_clauses_from_resume.argtypes = [vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp, vp, vp]
    L.csgpu_many_clause_checkpoint_children_obj.argtypes = [vp, vp, i64, C.c_int, vp, vp]
    L.csgpu_many_clause_checkpoint_fanout_obj.argtypes = [vp, vp, i64, C.c_int, vp, vp, vp, vp, vp, i64, vp]
    L.csgpu_many_fold_best.argtypes = [vp, vp, vp, i64, C.c_int, vp, vp]
    L.csgpu_many_best_key.argtypes = [C.c_int, C.c_int32, C.c_uint32]
    L.csgpu_many_best_key.restype = C.c_uint64
    L.csgpu_many_key_decode.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
    L.csgpu_internal_many_clauses_from_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_solve_many_clauses_ordered.argtypes = [vp, vp, i64, C.POINTER(ManyOrderOptions), vp, vp, vp, vp, vp]
    L.csgpu_many_clauses_ordered_frames.argtypes = [vp, C.c_int32]
    L.csgpu_many_clauses_ordered_frames.restype = i64
    L.csgpu_internal_many_clauses_order_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_many_clause_ordered_checkpoint_bytes.argtypes = [vp, C.c_int32]
    L.csgpu_many_clause_ordered_checkpoint_bytes.restype = C.c_size_t
    L.csgpu_many_clause_ordered_checkpoints_create.argtypes = [vp, i64, C.c_int32, C.POINTER(vp)]
    L.csgpu_solve_many_clauses_ordered_checkpointed.argtypes = [vp, vp, i64, C.POINTER(ManyOrderOptions), vp, vp, vp, vp, vp, vp,
                                                                vp]
    L.csgpu_solve_many_clauses_ordered_resume.argtypes = [vp, i64, C.POINTER(ManyOrderOptions), vp, vp, vp, vp, vp, vp, vp]
    L.csgpu_internal_many_clauses_order_resume_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_solve_many_clauses_ordered_from.argtypes = [vp, vp, vp, i64, C.POINTER(ManyOrderOptions), vp, vp, vp, vp, vp, vp, vp]
    L.csgpu_solve_many_clauses_ordered_from_resume.argtypes = [vp, i64, C.POINTER(ManyOrderOptions), vp, vp, vp, vp, vp, vp, vp]
    L.csgpu_many_clause_ordered_checkpoint_children.argtypes = [vp, vp, i64, C.c_int, C.c_int, vp, vp, vp]
    L.csgpu_many_clause_ordered_checkpoint_fanout.argtypes = [vp, vp, i64, C.c_int, C.c_int, vp, vp, vp, vp, vp, i64, vp]
    L.csgpu_many_fold_halvings.argtypes = [vp, vp, i64, vp, vp]
    L.csgpu_internal_many_clauses_order_from_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_model_qualifies_many_clauses_wide.argtypes = [vp]
    L.csgpu_solve_many_clauses_wide.argtypes = [vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp]
    L.csgpu_many_clause_wide_checkpoint_bytes.argtypes = [vp]
    L.csgpu_many_clause_wide_checkpoint_bytes.restype = C.c_size_t
    L.csgpu_many_clause_wide_checkpoints_create.argtypes = [vp, i64, C.POINTER(vp)]
    L.csgpu_solve_many_clauses_wide_checkpointed.argtypes = [vp, vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp, vp, vp]
    L.csgpu_solve_many_clauses_wide_resume.argtypes = [vp, i64, C.POINTER(ManyOptions), vp, vp, vp, vp, vp, vp]
    L.csgpu_internal_many_clauses_wide_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_internal_many_clauses_wide_resume_symbol.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.csgpu_internal_many_clauses_wide_waves.argtypes = [vp, i64]
    L.csgpu_internal_many_clauses_wide_waves.restype = i64
    L.csgpu_many_value.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, Val, C.c_uint32, C.c_int32]
    L.csgpu_many_value.restype = C.c_int32
    L.csgpu_debug_one_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    _lib = L
    return L


def check(rc: int):
    if rc < 0:
        raise CsolveError(rc, load_library().csgpu_last_error().decode())
    return rc
