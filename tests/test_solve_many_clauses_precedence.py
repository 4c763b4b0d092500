"""Which of two faults an entry of the csgpu_solve_many_clauses family reports: the earlier one of its ladder.  Every
entry makes its checks in one documented order -- the pointers, the count, the budget; its own options; the stream; the
objective; the model; the start; the order; the pool; then an empty batch is a success -- and the tests of each entry pin
its errors one at a time.  Here every fault of a ladder is made alone, and together with the next fault of the ladder that
it can be combined with: the call must answer with the earlier one's code and message.  The CPU test walks the rungs up to
"the model is not finalized" on parsed models; the GPU test walks the rest on finalized ones.  No call gets as far as a
launch: the buffers are never read or written."""
import ctypes as C

import numpy as np
import pytest

OK, E_ARG, E_LIMIT, E_STATE = 0, -1, -4, -5
K = 2


class _Pool(C.Structure):
    """csgpu_many_checkpoints as cs_capi.hip lays it out (kind 0: of csgpu_many_checkpoints_create, 1: of the clause one)"""
    _fields_ = [("m", C.c_void_p), ("capacity", C.c_int64), ("slot_bytes", C.c_size_t), ("d_pool", C.c_void_p),
                ("d_next", C.c_void_p), ("counted", C.c_int), ("kind", C.c_int), ("d_zero", C.c_void_p)]


def _entries(L):
    """name -> (the call on a dict of arguments, what its budget is called, the objective it is called with or None)"""
    from csolve_amd._lib import ManyOptions, ManyOrderOptions, ManyRestartOptions, ManyStream, ManyUptoOptions

    def opt(p):
        return C.byref(ManyOptions(p["objective"], 0, p["max_nodes"]))

    def upto(p):
        return C.byref(ManyUptoOptions(p["k"], 0, p["max_nodes"]))

    def restart(p):
        return C.byref(ManyRestartOptions(p["max_nodes"], p["base"], 7, p["flags"]))

    def order(p):
        return C.byref(ManyOrderOptions(p["objective"], p["order"], p["split"], p["reserved"], p["max_nodes"]))

    def out(p):
        return C.byref(ManyStream(p["rows"], p["owner"], p["counter"], p["cap"]))

    return {
        "clauses": (lambda p: L.csgpu_solve_many_clauses(p["model"], p["roots"], p["count"], opt(p), p["results"], None, None, None),
                    "instance", 2),
        "checkpointed": (lambda p: L.csgpu_solve_many_clauses_checkpointed(p["model"], p["roots"], p["count"], opt(p), p["results"],
                                                                           None, None, p["ck"], p["slots"], None), "slice", 2),
        "resume": (lambda p: L.csgpu_solve_many_clauses_resume(p["model"], p["count"], opt(p), p["results"], None, None, p["ck"],
                                                               p["slots"], None), "slice", 2),
        "from": (lambda p: L.csgpu_solve_many_clauses_from(p["model"], p["roots"], p["start"], p["count"], opt(p), p["results"],
                                                           None, None, p["ck"], p["slots"], None), "instance", 2),
        "from_resume": (lambda p: L.csgpu_solve_many_clauses_from_resume(p["model"], p["count"], opt(p), p["results"], None, None,
                                                                         p["ck"], p["slots"], None), "slice", 2),
        "upto": (lambda p: L.csgpu_solve_many_clauses_upto(p["model"], p["roots"], p["count"], upto(p), p["results"], None, None),
                 "instance", None),
        "upto_checkpointed": (lambda p: L.csgpu_solve_many_clauses_upto_checkpointed(p["model"], p["roots"], p["count"], upto(p),
                                                                                     p["results"], None, p["ck"], p["slots"], None),
                              "slice", None),
        "upto_resume": (lambda p: L.csgpu_solve_many_clauses_upto_resume(p["model"], p["count"], upto(p), p["results"], None,
                                                                         p["ck"], p["slots"], None), "slice", None),
        "restarts": (lambda p: L.csgpu_solve_many_clauses_restarts(p["model"], p["roots"], None, p["count"], restart(p),
                                                                   p["results"], None, None, None), "instance", None),
        "ordered": (lambda p: L.csgpu_solve_many_clauses_ordered(p["model"], p["roots"], p["count"], order(p), p["results"], None,
                                                                 None, None, None), "instance", 2),
        "stream": (lambda p: L.csgpu_solve_many_clauses_stream(p["model"], p["roots"], p["count"], opt(p), p["results"], p["ck"],
                                                               p["slots"], out(p), None), "slice", 1),
    }


POOLED = ("checkpointed", "resume", "from_resume", "upto_checkpointed", "upto_resume", "stream")
DEFAULTS = dict(count=K, max_nodes=100, k=2, base=0, flags=0, order=1, split=0, reserved=0, cap=4, ck=None, slots=None)


def _ladder(name, budgeted, objective, finalized):
    """the faults of entry `name` in the order it must report them: (arguments to change, code, words of the message; a
    word after "!" must be absent).  A value that is a string names an object of the test's world."""
    rungs = []
    if not finalized:  # 1: the pointers, the count, the budget
        rungs += [({"results": None}, E_ARG, "null argument"), ({"count": -1}, E_ARG, "negative instance"),
                  ({"max_nodes": 0}, E_ARG, "every " + budgeted)]
        if name.startswith("upto"):  # 2: the entry's own options
            rungs += [({"k": 0}, E_ARG, "max_solutions")]
        if name == "restarts":
            rungs += [({"base": -1}, E_ARG, "restart_base"), ({"flags": 2}, E_ARG, "unknown flags")]
        if name == "stream":  # 3: ALL, and a stream that takes a row (no other objective gets past it)
            rungs += [({"objective": 0}, E_ARG, "walks under ALL"), ({"cap": 0}, E_ARG, "room for"),
                      ({"rows": None}, E_ARG, "null pointer in the solution stream")]
        elif objective is not None:  # 4: the objective, against the model
            rungs += [({"objective": 7}, E_ARG, "no objective 7"), ({"model": "plain"}, E_ARG, "has none"),
                      ({"objective": 3}, E_ARG, "cannot be searched")]
        return rungs + [({}, E_STATE, "not finalized")]  # 5
    rungs += [({"model": "unplanned"}, E_LIMIT, "does not qualify"), ({"count": 1 << 31}, E_LIMIT, "2^31 - 65")]  # 5
    if name == "from":  # 6: the start, MIN / MAX, the pool and the slots together
        rungs += [({"start": None}, E_ARG, "d_start"), ({"objective": 1}, E_ARG, "MIN / MAX"),
                  ({"ck": "pool"}, E_ARG, "a plain one neither")]
    if name == "from_resume":
        rungs += [({"objective": 1}, E_ARG, "MIN / MAX"), ({"slots": None}, E_ARG, "a plain one neither"),
                  ({"ck": None, "slots": None}, E_ARG, "pool and slot numbers", "!neither")]
    if name == "ordered":  # 7
        rungs += [({"order": 5}, E_ARG, "no variable order 5"), ({"split": -1}, E_ARG, "split_width"),
                  ({"reserved": 1}, E_ARG, "reserved must be 0")]
    if name in POOLED or name == "from":  # 8: the pool (the stream's and the start entries' NULLs were refused above)
        if name not in ("stream", "from", "from_resume"):
            rungs += [({"slots": None}, E_ARG, "pool and slot numbers")]
        rungs += [({"ck": "foreign", "slots": "slots"}, E_ARG, "another model")]
        if name.startswith("from"):  # MIN / MAX: no model of both families has an objective, so the model's own pool, relabelled
            rungs += [({"ck": "relabelled", "slots": "slots"}, E_ARG, "other kind")]
        else:
            rungs += [({"model": "both", "ck": "dive_pool", "slots": "slots", "objective": 1}, E_ARG, "other kind")]
    return rungs + [({"count": 0}, OK)]  # 9: nothing to do


def _walk(L, world, finalized):
    """every fault of every ladder alone, then with the next one it does not share an argument with"""
    calls = 0
    for name, (call, budgeted, objective) in _entries(L).items():
        base = dict(DEFAULTS, model="model", roots="roots", results="results", start="start", rows="rows", owner="owner",
                    counter="counter", objective=objective)
        if name in POOLED:
            base.update(ck="pool", slots="slots")
        rungs = _ladder(name, budgeted, objective, finalized)
        for i, (fault, code, *words) in enumerate(rungs):
            later = next((f for f, *_ in rungs[i + 1:] if not set(f) & set(fault)), None)
            for both in (fault,) if later is None else (fault, dict(later, **fault)):
                args = {k: world[v] if isinstance(v, str) else v for k, v in dict(base, **both).items()}
                rc = call(args)
                msg = L.csgpu_last_error().decode()
                assert rc == code, (name, both, rc, msg)
                for w in words:
                    assert (w[1:] not in msg) if w.startswith("!") else (w in msg), (name, both, w, msg)
                calls += 1
    return calls


def test_an_earlier_fault_wins_before_the_model_is_finalized():
    from csolve_amd import _lib, problems
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(problems.schedule(5, 1))            # MIN; parsed, not finalized
    plain = Model.from_text(problems.linear(12, 1, "ALL"))  # no objective variable
    roots = np.zeros((K, m.n_vars, 2), dtype=np.int32)
    results, slots = np.full((K, 5), 77, dtype=np.int64), np.full(K, 77, dtype=np.int32)
    start, rows = np.zeros((K, 2), dtype=np.int32), np.zeros((4, m.n_vars), dtype=np.int32)
    owner, counter = np.zeros(4, dtype=np.int32), np.zeros(1, dtype=np.uint64)
    pool = _Pool(kind=1)
    world = dict(model=m._h, plain=plain._h, roots=roots.ctypes.data, results=results.ctypes.data, slots=slots.ctypes.data,
                 start=start.ctypes.data, rows=rows.ctypes.data, owner=owner.ctypes.data, counter=counter.ctypes.data,
                 pool=C.addressof(pool))
    assert _walk(L, world, finalized=False) > 11 * 2 * 4
    assert (results == 77).all() and (slots == 77).all() and not rows.any() and not counter.any()


@pytest.mark.gpu
def test_an_earlier_fault_wins_on_a_finalized_model_and_an_empty_batch_is_a_success():
    torch = pytest.importorskip("torch")
    from csolve_amd import _lib, problems
    from csolve_amd.solver import solve_root
    L = _lib.load_library()
    model, other = solve_root(problems.schedule(5, 1)), solve_root(problems.schedule(5, 1))
    unplanned = solve_root(problems.schedule(32, 1))  # more than 512 clauses: no cs_walk_* kernel
    both = solve_root(problems.queens(8, "ALL"))      # a pure != model, of csgpu_solve_many's family too
    assert model.qualifies_many_clauses() and both.qualifies_many_clauses() and not unplanned.qualifies_many_clauses()
    pool, foreign, dive_pool = model.many_clause_checkpoints(K), other.many_clause_checkpoints(K), both.many_checkpoints(K)
    relabelled = _Pool.from_buffer_copy(C.string_at(pool._h.value, C.sizeof(_Pool)))
    assert relabelled.m == model._h.value and relabelled.capacity == K and relabelled.kind == 1
    relabelled.kind = 0
    roots = torch.zeros((K, model.n_vars, 2), dtype=torch.int32, device="cuda")
    results = torch.full((K, 5), 77, dtype=torch.int64, device="cuda")
    slots = torch.full((K,), 77, dtype=torch.int32, device="cuda")
    start = torch.zeros((K, 2), dtype=torch.int32, device="cuda")
    rows = torch.full((4, model.n_vars), 77, dtype=torch.int32, device="cuda")
    owner = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    world = dict(model=model._h, unplanned=unplanned._h, both=both._h, roots=roots.data_ptr(), results=results.data_ptr(),
                 slots=slots.data_ptr(), start=start.data_ptr(), rows=rows.data_ptr(), owner=owner.data_ptr(),
                 counter=counter.data_ptr(), pool=pool._h, foreign=foreign._h, dive_pool=dive_pool._h,
                 relabelled=C.addressof(relabelled))
    assert _walk(L, world, finalized=True) > 11 * 2 * 3
    torch.cuda.synchronize()
    assert (results == 77).all() and (slots == 77).all() and (rows == 77).all() and (owner == 77).all() and not counter.any()
