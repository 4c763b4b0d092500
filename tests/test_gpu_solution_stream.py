"""GPU tests of the solution stream (csgpu_search_set_solution_stream and the drains): every solution of an ALL
search reaches the caller -- not only the 1,024 rows of the store -- through the fused levels, the separate-kernel
path and the command line; ANY streams its one solution, MIN / MAX each improving one."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _engine(text, strategy=None, stream_rows=None, pool=1 << 18, children=1 << 14):
    from csolve_amd.solver import Search, solve_root
    model = solve_root(text)
    s = Search(model, pool, children)
    if strategy is not None:
        s.set_strategy(strategy)
    s.stream_solutions(stream_rows)
    s.put(model.root_state())
    return model, s


def _enumerate(s, slice_iterations=1 << 40):
    """run to the end, draining after every call: (rows, stats, calls)"""
    batches, calls = [], 0
    while True:
        st = s.run(slice_iterations)
        calls += 1
        batches.append(s.drain_solutions())
        if st["done"]:
            break
    return np.concatenate(batches), st, calls


def _as_set(rows):
    return {tuple(int(x) for x in r) for r in rows}


def _valid_queens(rows, n):
    c = np.arange(n)
    for r in rows:
        assert len(set(r)) == n and len(set(r + c)) == n and len(set(r - c)) == n, r


def _all_true(model, rows):
    states = torch.from_numpy(np.stack([rows, rows], 2).astype(np.int32)).cuda().contiguous()
    truth = model.eval_root(states).cpu().numpy()
    assert (truth == 1).all()


def _queens12_rows():
    from csolve_amd import problems
    model, s = _engine(problems.queens(12, "ALL"))
    rows = np.concatenate(list(s.iter_solutions()))
    return model, s, rows


def test_queens12_all_streams_every_solution():
    """queens-12 ALL on the fused levels with the default stream: 14,200 rows, pairwise distinct, every one a valid
    placement, as many as the search counted -- the store alone keeps 1,024."""
    model, s, rows = _queens12_rows()
    assert s.stats["done"] == 1 and s.stats["solutions"] == 14200
    assert rows.shape == (14200, 12)
    assert len(_as_set(rows)) == 14200
    _valid_queens(rows, 12)
    assert len(s.solutions(1 << 20)) == 1024  # the store is what it was
    assert s.pending_solutions()[0] == 0


def test_tiny_stream_returns_early_and_loses_nothing():
    """A stream of four parents' worth of rows: run returns early (done 0) hundreds of times; the drained rows are
    the same set as with the default stream, each once."""
    from csolve_amd import problems
    _, _, want = _queens12_rows()
    model, s = _engine(problems.queens(12, "ALL"), stream_rows=4 * 12)
    rows, st, calls = _enumerate(s)
    assert calls >= 200
    assert st["solutions"] == 14200 and len(rows) == 14200
    assert _as_set(rows) == _as_set(want)


def _oracle_solutions(text):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from cpu_engine import OracleEngine
    from oracle.cs_oracle import Model as OModel, Oracle
    om = OModel.parse(text)
    o0 = Oracle(om)
    o0.set_root_phase(True)
    assert o0.propagate(om.root, om.n_vars) >= 0
    om.set_domains(o0.domains())
    om.index()
    eng = OracleEngine(om, parents_per_iteration=64)
    eng.put(torch.from_numpy(om.domains()).unsqueeze(0).contiguous())
    st = eng.run(1 << 30)
    assert st["done"] == 1
    return _as_set(eng.found)


def test_separate_kernel_path_streams_the_same_set():
    """queens-10 ALL through the separate kernels (order "none": no fused levels) gives the fused path's 724 rows."""
    from csolve_amd import problems
    _, fused = _engine(problems.queens(10, "ALL"))
    a, st_a, _ = _enumerate(fused)
    _, sep = _engine(problems.queens(10, "ALL"), strategy="none")
    b, st_b, _ = _enumerate(sep)
    assert st_a["solutions"] == st_b["solutions"] == 724
    assert len(a) == len(b) == 724
    assert _as_set(a) == _as_set(b)


@pytest.mark.parametrize("name,args,strategy", [("offsets", (6, 6, 1), "none"), ("linear", (4, 1), None)])
def test_non_queens_all_matches_the_oracle(name, args, strategy):
    """Non-queens ALL models (a != network of irregular shape on the separate kernels; a linear mixture whose complete
    children are evaluated): the streamed rows equal, as a set, the solutions the oracle-backed CPU engine finds, and
    every row evaluates true."""
    from csolve_amd import problems
    text = getattr(problems, name)(*args, objective="ALL")
    model, s = _engine(text, strategy=strategy, stream_rows=1 << 12)
    rows, st, _ = _enumerate(s)
    want = _oracle_solutions(text)
    assert len(want) > 1024
    assert st["solutions"] == len(rows) == len(want)
    assert _as_set(rows) == want
    _all_true(model, rows)


def _check_improving(model, s, rows, st, minimise=True):
    assert len(rows) >= 1
    obj = rows[:, model.objective_var]
    steps = np.diff(obj)
    assert (steps < 0).all() if minimise else (steps > 0).all()
    _all_true(model, rows)
    assert obj[-1] == st["best"]
    assert (rows[-1] == s.best_solution()).all()


@pytest.mark.parametrize("burst", ["1", "0"])
@pytest.mark.parametrize("name,best", [("ref_schedule", 11), ("schedule6_s1", 22)])
def test_min_streams_each_improving_solution(name, best, burst, monkeypatch):
    """MIN, with bursts and driven from the host: the rows' objective values strictly decrease, every row evaluates
    true, the last attains the optimum and is best_solution()."""
    monkeypatch.setenv("CSGPU_SEARCH_BURST", burst)
    model, s = _engine(open(golden("problems", name + ".txt")).read(), pool=1 << 20, children=1 << 16)
    rows, st, _ = _enumerate(s)
    assert st["best"] == best
    _check_improving(model, s, rows, st)


def test_min_with_restart_on_improvement():
    """schedule-6 MIN restarting from its seed on every better solution: the same rule holds across restarts."""
    from csolve_amd.solver import Search, solve_root
    model = solve_root(open(golden("problems", "schedule6_s1.txt")).read())
    s = Search(model, 1 << 20, 1 << 16)
    s.set_restart_on_improvement(True)
    s.stream_solutions()
    s.put(model.root_state())
    rows, st, _ = _enumerate(s, 64)
    assert st["best"] == 22 and st["restarts"] >= 1
    _check_improving(model, s, rows, st)


@pytest.mark.parametrize("burst", ["1", "0"])
def test_any_streams_its_one_solution(burst, monkeypatch):
    """queens-64 ANY, with bursts (cs_accept_block) and driven from the host (cs_accept): one row, the one the store
    holds."""
    from csolve_amd import problems
    monkeypatch.setenv("CSGPU_SEARCH_BURST", burst)
    model, s = _engine(problems.queens(64), pool=1 << 20, children=1 << 16)
    rows, st, _ = _enumerate(s, 5000)
    assert st["solutions"] == 1 and rows.shape == (1, 64)
    assert (rows[0] == s.solutions(1)[0]).all()
    _valid_queens(rows, 64)


def test_partial_drains_wrap_the_ring():
    """Drains of 0, 1 and 7 rows while rows are waiting, on a stream of 23 rows that wraps many times: 0 leaves the
    stream as it is, the others take the oldest rows; over the search every one of queens-10's 724 solutions comes out
    once -- the same set as one drain of everything.  The device drain takes partial batches alike."""
    from csolve_amd import problems
    _, whole = _engine(problems.queens(10, "ALL"))
    want, _, _ = _enumerate(whole)
    for device in (False, True):
        _, s = _engine(problems.queens(10, "ALL"), stream_rows=23)
        drain = (lambda k: s.drain_solutions_device(k).cpu().numpy()) if device else s.drain_solutions
        got, zero_with_rows = [], 0
        while True:
            st = s.run(1 << 40)
            waiting = s.pending_solutions()
            if waiting[0] > 0:
                zero_with_rows += 1
                assert len(drain(0)) == 0 and s.pending_solutions() == waiting
                one = drain(1)
                assert len(one) == 1 and s.pending_solutions() == (waiting[0] - 1, waiting[1] + 1)
                got.append(one)
            got.append(drain(7))
            if st["done"] and s.pending_solutions()[0] == 0:
                break
        rows = np.concatenate(got)
        assert zero_with_rows >= 50
        assert st["solutions"] == len(rows) == 724
        assert _as_set(rows) == _as_set(want)


def test_device_drain_matches_host_drain():
    """queens-10 ALL drained on the device: a tensor on the engine's device holding the host drain's set."""
    from csolve_amd import problems
    _, h = _engine(problems.queens(10, "ALL"))
    host, _, _ = _enumerate(h)
    _, d = _engine(problems.queens(10, "ALL"), stream_rows=100)
    batches = list(d.iter_solutions(slice_iterations=4, device=True))
    assert all(b.device == d.device and b.dtype == torch.int32 for b in batches)
    dev = torch.cat(batches).cpu().numpy()
    assert d.stats["solutions"] == 724 and len(dev) == 724
    assert _as_set(dev) == _as_set(host)


def test_stream_state_rules():
    """reset empties the stream and keeps it on; enabling after a put or on a shared-incumbent engine is
    CSGPU_E_STATE; fewer rows than one parent's children is CSGPU_E_ARG; without the stream the store still stops at
    1,024 rows."""
    from csolve_amd import problems
    from csolve_amd._lib import CsolveError
    from csolve_amd.solver import Search, solve_root
    E_ARG, E_STATE = -1, -5
    model = solve_root(problems.queens(10, "ALL"))
    s = Search(model, 1 << 18, 1 << 14)
    with pytest.raises(CsolveError) as e:
        s.stream_solutions(9)  # < 10 values of the widest root interval
    assert e.value.code == E_ARG
    s.stream_solutions(10)
    s.put(model.root_state())
    st = s.run(1 << 40)  # returns once the first rows leave less than one parent's worth of room
    assert st["done"] == 0 and s.pending_solutions()[0] > 0
    s.reset()
    assert s.pending_solutions() == (0, 10)
    s.put(model.root_state())
    with pytest.raises(CsolveError) as e:
        s.stream_solutions(1 << 10)
    assert e.value.code == E_STATE
    rows, st, _ = _enumerate(s)
    assert len(rows) == st["solutions"] == 724

    m12 = solve_root(problems.queens(12, "ALL"))
    off = Search(m12, 1 << 18, 1 << 14)
    off.put(m12.root_state())
    st = off.run(1 << 40)
    assert st["solutions"] == 14200 and len(off.solutions(1 << 20)) == 1024
    with pytest.raises(CsolveError) as e:
        off.pending_solutions()
    assert e.value.code == E_STATE

    sched = solve_root(open(golden("problems", "schedule6_s1.txt")).read())
    a, b = Search(sched, 1 << 20, 1 << 16), Search(sched, 1 << 20, 1 << 16)
    a.share_incumbent(b)
    for eng in (a, b):
        with pytest.raises(CsolveError) as e:
            eng.stream_solutions()
        assert e.value.code == E_STATE
    c, d = Search(sched, 1 << 20, 1 << 16), Search(sched, 1 << 20, 1 << 16)
    c.stream_solutions()
    with pytest.raises(CsolveError) as e:
        d.share_incumbent(c)
    assert e.value.code == E_STATE


def test_cli_prints_every_all_solution():
    """csolve_gpu on queens-12 ALL: 14,200 distinct SOLUTION lines, and the last line counts as many."""
    from csolve_amd import problems
    exe = os.path.join(ROOT, "csolve_amd", "csolve_gpu")
    p = subprocess.run([exe, "-"], input=problems.queens(12, "ALL"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    sol = [ln for ln in lines if "SOLUTION:" in ln]
    pat = re.compile(r"#1: SOLUTION: (X\d+ = \d+, ){12}BEST: 0")
    assert all(pat.fullmatch(ln) for ln in sol)
    assert len(sol) == 14200 and len(set(sol)) == 14200
    assert lines[-1].endswith("SOLUTIONS: 14200")
