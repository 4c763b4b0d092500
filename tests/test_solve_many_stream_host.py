"""CPU tests of csgpu_solve_many_stream / Model.solve_many_stream (ALL, every solution appended to one bounded stream): the
interface is declared, exported and prototyped; the argument errors, in the documented order, with no device; the shipped
cs_dive_stream instantiations beside the older families."""
import ctypes as C
import re
import subprocess

import numpy as np

import many_upto_sets
from conftest import golden

E_ARG, E_LIMIT, E_STATE = -1, -4, -5


def _header():
    from csolve_amd import _lib
    return open(_lib.HEADER_PATH).read()


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import ManySolutionStream, Model
    raw = _header()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = _lib.load_library()
    assert "csgpu_solve_many_stream" in _lib.declared_symbols()
    assert hasattr(L, "csgpu_solve_many_stream") and len(L.csgpu_solve_many_stream.argtypes) == 9
    assert hasattr(L, "csgpu_internal_many_stream_symbol") and len(L.csgpu_internal_many_stream_symbol.argtypes) == 3
    assert "csgpu_internal_many_stream_symbol" not in raw  # cs_internal.h only
    # the two constants
    assert re.search(r"#define CSGPU_MANY_FULL 4\b", text) and _lib.MANY_FULL == 4
    assert re.search(r"#define CSGPU_MANY_SLOT_FRESH \(-2\)", text) and _lib.MANY_SLOT_FRESH == -2
    assert (_lib.MANY_DONE, _lib.MANY_LIMIT, _lib.MANY_BAD_ROOT, _lib.MANY_BAD_SLOT) == (0, 1, 2, 3)
    # the struct: 32 bytes, the header's field names in the header's order
    body = re.search(r"typedef struct csgpu_many_stream \{(.*?)\} csgpu_many_stream;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [f for f, _ in _lib.ManyStream._fields_] == ["d_rows", "d_owner", "d_count", "capacity"]
    assert C.sizeof(_lib.ManyStream) == 32
    assert [getattr(_lib.ManyStream, f).offset for f, _ in _lib.ManyStream._fields_] == [0, 8, 16, 24]
    # the old calls keep their argument counts, their records and their options
    old = {"csgpu_solve_many": 7, "csgpu_solve_many_checkpointed": 9, "csgpu_solve_many_resume": 8, "csgpu_solve_many_upto": 7,
           "csgpu_solve_many_upto_checkpointed": 9, "csgpu_solve_many_upto_resume": 8, "csgpu_solve_many_restarts": 9,
           "csgpu_many_checkpoint_states": 6, "csgpu_many_checkpoints_create": 3}
    for name, args in old.items():
        assert len(getattr(L, name).argtypes) == args, name
    assert C.sizeof(_lib.ManyResult) == 40 and C.sizeof(_lib.ManyOptions) == 16
    for method in ("many_stream", "solve_many_stream", "solve_many_all", "many_stream_kernel"):
        assert callable(getattr(Model, method)), method
    assert callable(ManySolutionStream.take)
    assert not any("dive" in f or "many" in f or "stream" in f for f in _lib.PLAN_FAMILIES) and len(_lib.PLAN_FAMILIES) == 16


def test_argument_errors_come_in_the_documented_order_before_any_device_call():
    from csolve_amd import _lib
    from csolve_amd._lib import ManyOptions, ManyStream
    from csolve_amd.solver import Model
    L = _lib.load_library()
    m = Model.from_text(open(golden("problems", "queens8.txt")).read())  # parsed, not finalized
    rows = np.zeros((2, 8, 2), dtype=np.int32)
    res = np.zeros((2, 5), dtype=np.int64)
    slots = np.full(2, -2, dtype=np.int32)
    pool = C.create_string_buffer(64)  # stands for a pool: no call gets as far as looking into it
    mem = np.zeros(64, dtype=np.int64)  # stands for device memory: nothing is launched
    p = mem.ctypes.data
    ok, good = ManyOptions(1, 0, 100), ManyStream(p, p, p, 4)

    def call(model=m._h, roots=rows.ctypes.data, count=2, opt=ok, results=res.ctypes.data, ck=pool, sl=slots.ctypes.data, out=good):
        rc = L.csgpu_solve_many_stream(model, roots, count, C.byref(opt) if opt is not None else None, results, ck, sl,
                                       C.byref(out) if out is not None else None, None)
        msg = L.csgpu_last_error().decode()
        assert rc < 0 and msg, (rc, msg)
        return rc, msg

    # 1. null arguments, the count, the budget
    for missing in ("model", "roots", "opt", "results", "ck", "sl", "out"):
        rc, msg = call(**{missing: None})
        assert rc == E_ARG and "null" in msg, (missing, msg)
    assert call(count=-1)[0] == E_ARG and "count" in call(count=-1)[1]
    for budget in (0, -5):
        rc, msg = call(opt=ManyOptions(1, 0, budget))
        assert rc == E_ARG and "max_nodes" in msg
    assert "count" in call(count=-1, opt=ManyOptions(0, 0, 0), out=ManyStream(p, p, p, 0))[1]
    assert "max_nodes" in call(opt=ManyOptions(0, 0, 0), out=ManyStream(p, p, p, 0))[1]
    # 2. the objective: ALL alone, and CSGPU_E_ARG for MIN / MAX too (csgpu_solve_many says CSGPU_E_LIMIT for those)
    for objective in (0, 2, 3, 7, -1):
        rc, msg = call(opt=ManyOptions(objective, 0, 100), out=ManyStream(p, p, p, 0))
        assert rc == E_ARG and "ALL" in msg, (objective, msg)
    # 3. the stream
    for capacity in (0, -3):
        rc, msg = call(out=ManyStream(p, p, p, capacity))
        assert rc == E_ARG and "capacity" in msg
    for bad in (ManyStream(None, p, p, 4), ManyStream(p, None, p, 4), ManyStream(p, p, None, 4)):
        rc, msg = call(out=bad)
        assert rc == E_ARG and "null" in msg
    # 4. the model's state, after all of them; an empty batch is no way round it
    rc, msg = call()
    assert rc == E_STATE and "finalized" in msg
    assert call(count=0)[0] == E_STATE
    # nothing was touched
    assert (res == 0).all() and (slots == -2).all() and (mem == 0).all()


def shipped_kernels(family):
    from csolve_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    shipped = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("_Z"):
            name = _lib.demangle(parts[2])
            if name.split("<")[0] == family and "<" in name:
                shipped.add(name)
    return shipped


def test_shipped_stream_kernels_are_six_beside_six_of_each_older_family():
    shipped = shipped_kernels("cs_dive_stream")
    assert len(shipped) == 6
    for name in shipped:
        assert re.fullmatch(r"cs_dive_stream<unsigned (char|short), ([124])>", name), name
    # the six sets of the GPU tests name exactly these
    assert {s[3].replace("cs_dive_upto", "cs_dive_stream") for s in many_upto_sets.SETS.values()} == shipped
    for family in ("cs_dive_shave", "cs_dive_resume", "cs_dive_upto", "cs_dive_restart"):
        old = shipped_kernels(family)
        assert len(old) == 6, family
        assert {n.replace(family, "cs_dive_stream") for n in old} == shipped, family
