"""Which of two faults the entries of the ordered spread report: the earlier one of their ladders (include/csolve_gpu.h, "the
ordered walk: start incumbents, and stopped walks spread"), in the manner of test_solve_many_clauses_precedence.py.  Every
fault of a ladder is made alone, and together with the next fault of the ladder that it shares no argument with: the call
answers with the earlier one's code and message.  This file walks what needs no device -- csgpu_solve_many_clauses_ordered_
from / _from_resume up to "the model is not finalized", and the whole ladders of the count, the fan-out and the halving
fold, which read nothing of a pool but its kind.  test_gpu_solve_many_clauses_ordered_from.py walks the rest on finalized
models.  No call gets as far as a launch: the buffers are never read or written."""
import ctypes as C

import numpy as np

OK, E_ARG, E_LIMIT, E_STATE = 0, -1, -4, -5
K = 2


class Pool(C.Structure):
    """csgpu_many_checkpoints as cs_capi.hip lays it out (kind 0: of csgpu_many_checkpoints_create, 1: of the clause one,
    2: of the ordered clause one)"""
    _fields_ = [("m", C.c_void_p), ("capacity", C.c_int64), ("slot_bytes", C.c_size_t), ("d_pool", C.c_void_p),
                ("d_next", C.c_void_p), ("counted", C.c_int), ("kind", C.c_int), ("d_zero", C.c_void_p), ("frames", C.c_int),
                ("split_width", C.c_int)]


def entries(L):
    """name -> the call on a dict of arguments"""
    from csolve_amd._lib import ManyOrderOptions

    def order(p):
        return C.byref(ManyOrderOptions(p["objective"], p["order"], p["split"], p["reserved"], p["max_nodes"]))

    return {
        "from": lambda p: L.csgpu_solve_many_clauses_ordered_from(p["model"], p["roots"], p["start"], p["count"], order(p),
                                                                  p["results"], None, None, p["halvings"], p["ck"], p["slots"],
                                                                  None),
        "from_resume": lambda p: L.csgpu_solve_many_clauses_ordered_from_resume(p["model"], p["count"], order(p), p["results"],
                                                                                None, None, p["halvings"], p["ck"], p["slots"],
                                                                                None),
        "children": lambda p: L.csgpu_many_clause_ordered_checkpoint_children(p["ck"], p["slots"], p["count"], p["objective"],
                                                                              p["order"], p["children"], p["unsplit"], None),
        "fanout": lambda p: L.csgpu_many_clause_ordered_checkpoint_fanout(p["ck"], p["slots"], p["count"], p["objective"],
                                                                          p["order"], p["owner_start"], p["offsets"], p["rows"],
                                                                          p["owner"], p["start"], p["total"], None),
        "fold": lambda p: L.csgpu_many_fold_halvings(p["sub"], p["owner"], p["total"], p["halvings"], None),
    }


DEFAULTS = dict(count=K, max_nodes=100, order=1, split=4, reserved=0, ck=None, slots=None, total=4, owner_start=None)


def ladder(name, finalized):
    """the faults of entry `name` in the order it must report them: (arguments to change, code, words of the message; a
    word after "!" must be absent).  A value that is a string names an object of the test's world.  finalized False: the
    rungs that need no device; True: the rungs behind "the model is not finalized" (the walks only)"""
    if name == "fold":
        return [({"sub": None}, E_ARG, "null argument"), ({"halvings": None}, E_ARG, "null argument"),
                ({"total": -1}, E_ARG, "negative record"), ({"total": 256 * 0x7fffffff + 1}, E_LIMIT, "2^39"), ({"total": 0}, OK)]
    if name in ("children", "fanout"):
        rungs = [({"ck": None}, E_ARG, "null argument"), ({"slots": None}, E_ARG, "null argument")]
        rungs += [({"unsplit": None}, E_ARG, "null argument")] if name == "children" else [({"rows": None}, E_ARG, "null argument")]
        rungs += [({"count": -1}, E_ARG, "negative instance")]
        if name == "fanout":
            rungs += [({"total": -1}, E_ARG, "negative row")]
        rungs += [({"objective": 0}, E_ARG, "not objective 0"), ({"order": 5}, E_ARG, "no variable order 5"),
                  ({"ck": "clause_pool"}, E_ARG, "other kind"), ({"ck": "dive_pool"}, E_ARG, "other kind"),
                  ({"count": 1 << 31}, E_LIMIT, "2^31 - 1")]
        if name == "fanout":
            rungs += [({"start": None}, E_ARG, "d_start"),
                      ({"objective": 1, "start": "start"}, E_ARG, "NULL under ALL")]
        return rungs + [({"count": 0}, OK)]
    budgeted = "slice" if name == "from_resume" else "instance"
    if not finalized:
        return [({"results": None}, E_ARG, "null argument"), ({"count": -1}, E_ARG, "negative instance"),
                ({"max_nodes": 0}, E_ARG, "every " + budgeted), ({"objective": 7}, E_ARG, "no objective 7"),
                ({"model": "plain"}, E_ARG, "has none"), ({"objective": 3}, E_ARG, "cannot be searched"),
                ({}, E_STATE, "not finalized")]
    rungs = [({"model": "unplanned"}, E_LIMIT, "does not qualify"), ({"count": 1 << 31}, E_LIMIT, "2^31 - 65"),
             ({"order": 5}, E_ARG, "no variable order 5"), ({"split": -1}, E_ARG, "split_width"),
             ({"reserved": 1}, E_ARG, "reserved must be 0")]
    if name == "from":
        rungs += [({"start": None}, E_ARG, "d_start"), ({"objective": 1}, E_ARG, "MIN / MAX"),
                  ({"ck": None}, E_ARG, "a plain one neither")]
    else:
        rungs += [({"objective": 1}, E_ARG, "MIN / MAX"), ({"slots": None}, E_ARG, "a plain one neither"),
                  ({"ck": None, "slots": None}, E_ARG, "pool and slot numbers", "!neither")]
    rungs += [({"halvings": None}, E_ARG, "d_halvings"), ({"ck": "foreign", "slots": "slots"}, E_ARG, "another model"),
              ({"ck": "clause_pool", "slots": "slots"}, E_ARG, "other kind"),
              # (no model of both families has an objective: the model's own pool, relabelled as one of the kernel-7 kind)
              ({"ck": "relabelled", "slots": "slots"}, E_ARG, "other kind"),
              ({"ck": "other_split", "slots": "slots"}, E_ARG, "made for split_width")]
    return rungs + [({"count": 0}, OK)]


def walk(L, world, names, finalized):
    """every fault of every ladder alone, then with the next one it does not share an argument with -> the calls made"""
    calls = 0
    table = entries(L)
    for name in names:
        call = table[name]
        base = dict(DEFAULTS, model="model", roots="roots", results="results", start="start", halvings="halvings",
                    children="children", unsplit="unsplit", offsets="offsets", rows="rows", owner="owner", sub="sub",
                    objective=2)
        if name != "fold":
            base.update(ck="pool", slots="slots")
        rungs = ladder(name, finalized)
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


def test_an_earlier_fault_wins_where_no_device_is_needed():
    from csolve_amd import _lib, problems
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(problems.schedule(5, 1))            # MIN; parsed, not finalized
    plain = Model.from_text(problems.linear(12, 1, "ALL"))  # no objective variable
    roots = np.zeros((K, m.n_vars, 2), dtype=np.int32)
    results, slots = np.full((K, 5), 77, dtype=np.int64), np.full(K, 77, dtype=np.int32)
    start, halvings = np.full((4, 2), 77, dtype=np.int32), np.full(K, 77, dtype=np.int64)
    children, unsplit = np.full(K, 77, dtype=np.int64), np.full(K, 77, dtype=np.int32)
    offsets, rows = np.zeros(K + 1, dtype=np.int64), np.full((4, m.n_vars, 2), 77, dtype=np.int32)
    owner, sub = np.full(4, 77, dtype=np.int32), np.full(4, 77, dtype=np.int64)
    pool, clause_pool, dive_pool = Pool(kind=2, frames=m.n_vars, split_width=4), Pool(kind=1), Pool(kind=0)
    world = dict(model=m._h, plain=plain._h, roots=roots.ctypes.data, results=results.ctypes.data, slots=slots.ctypes.data,
                 start=start.ctypes.data, halvings=halvings.ctypes.data, children=children.ctypes.data,
                 unsplit=unsplit.ctypes.data, offsets=offsets.ctypes.data, rows=rows.ctypes.data, owner=owner.ctypes.data,
                 sub=sub.ctypes.data, pool=C.addressof(pool), clause_pool=C.addressof(clause_pool),
                 dive_pool=C.addressof(dive_pool))
    assert walk(L, world, ("from", "from_resume", "children", "fanout", "fold"), finalized=False) > 5 * 2 * 3
    for a in (results, slots, start, halvings, children, unsplit, rows, owner, sub):
        assert (a == 77).all()


def test_the_python_calls_refuse_what_the_library_refuses():
    import pytest
    from csolve_amd import problems
    from csolve_amd._lib import CsolveError
    from csolve_amd.solver import Model
    m = Model.from_text(problems.schedule(5, 1))
    rows = np.zeros((K, m.n_vars, 2), dtype=np.int32)
    with pytest.raises(CsolveError) as e:
        m.many_clauses_order_from_kernel()
    assert e.value.code == E_STATE
    with pytest.raises(CsolveError) as e:  # the library says why before anything is uploaded
        m.solve_many_clauses_ordered(rows, "MIN", max_nodes=8, order="none", split_width=4, start=np.zeros((K, 2), np.int32))
    assert e.value.code == E_STATE
    # the refusals of resume_many_clauses for an ordered answer that existing tests pin stay; own_solutions needs MIN / MAX
    for answer in ({"_checkpoints": None, "_order": 0}, {"_checkpoints": None, "_order": 0, "_objective": 1}):
        with pytest.raises(ValueError):
            m.resume_many_clauses(answer, max_nodes=5, own_solutions=True)
        with pytest.raises(ValueError):
            m.resume_many_clauses(answer, max_nodes=5, max_solutions=2)
