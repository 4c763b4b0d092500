"""csolve_gpu -j N: the sharded search as N rank processes coordinated in C (csgpu_shard_run, cs_shard.c), and the
coordinator's API through ctypes."""
import ctypes as C
import mmap
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
from csolve_amd import problems
from csolve_amd._lib import SHARD_SOLUTION_FN, SearchStats, ShardOptions, check, load_library

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "csolve_amd", "csolve_gpu")
CSGPU_E_STATE = -5
STATS = re.compile(r"^#(\d+): CALLS: (\d+), CUTS: (\d+), PROPS: (\d+), .*SOLUTIONS: (\d+)$")


def cli(args, problem, tmp_path=None, timeout=300):
    if not os.path.exists(problem):
        path = tmp_path / "problem.txt"
        path.write_text(problem)
        problem = str(path)
    p = subprocess.run([EXE] + list(args) + [problem], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
    return p.stdout


def solution_lines(out):
    return [line for line in out.splitlines() if ": SOLUTION: " in line]


def values(line):
    body = line.split(": SOLUTION: ", 1)[1]
    pairs = dict(re.findall(r"([^\s,=]+) = (-?\d+)", body.rsplit(", BEST:", 1)[0]))
    best = int(body.rsplit("BEST: ", 1)[1])
    return {k: int(v) for k, v in pairs.items()}, best


def stats_lines(out):
    return [STATS.match(line) for line in out.splitlines() if STATS.match(line)]


def assert_queens(vals, n):
    xs = [vals[f"X{i}"] for i in range(1, n + 1)]
    assert sorted(xs) == list(range(1, n + 1))
    assert len({x + i for i, x in enumerate(xs)}) == n and len({x - i for i, x in enumerate(xs)}) == n


def test_queens8_all_two_ranks():
    out = cli(["-j", "2"], golden("problems", "queens8_all.txt"))
    sols = solution_lines(out)
    assert len(sols) == 92 and len({line.split(": ", 1)[1] for line in sols}) == 92
    for line in sols:
        assert line.startswith(("#1: ", "#2: ")) and line.endswith("BEST: 0")
        assert_queens(values(line)[0], 8)
    lines = out.splitlines()
    st = stats_lines(out)
    assert [m.group(1) for m in st] == ["2", "1"]
    assert lines[-1].startswith("#1: CALLS: ") and lines[-2].startswith("#2: CALLS: ")
    assert all(m.group(5) == "92" for m in st)


def test_queens12_all_four_ranks_partition_the_tree(tmp_path):
    text = problems.queens(12, "ALL")
    out = cli(["-j", "4"], text, tmp_path)
    sols = solution_lines(out)
    assert len(sols) == 14200 and len({line.split(": ", 1)[1] for line in sols}) == 14200
    st = stats_lines(out)
    assert [m.group(1) for m in st] == ["2", "3", "4", "1"]
    assert all(int(m.group(2)) > 0 for m in st), "every rank expanded nodes"
    assert all(m.group(5) == "14200" for m in st)
    one = stats_lines(cli(["-j", "1"], text, tmp_path))
    assert len(one) == 1 and one[0].group(5) == "14200"
    assert sum(int(m.group(2)) for m in st) == int(one[0].group(2))  # CALLS: the same tree, partitioned
    assert sum(int(m.group(3)) for m in st) == int(one[0].group(3))  # CUTS


def test_min_reports_one_optimal_row(tmp_path):
    out = cli(["-j", "3"], golden("problems", "schedule6_s1.txt"))
    sols = solution_lines(out)
    assert len(sols) == 1 and sols[0].endswith("BEST: 22"), out[-500:]
    assert len(stats_lines(out)) == 3

    from csolve_amd.solver import Model
    text = problems.schedule(8, 1)
    out = cli(["-j", "4"], text, tmp_path)
    sols = solution_lines(out)
    assert len(sols) == 1, out[-500:]
    vals, best = values(sols[0])
    assert best == 31
    m = Model.from_text(text)
    names = m.var_names()
    assert m.objective_var >= 0 and vals[names[m.objective_var]] == 31
    row = np.array([[vals[nm], vals[nm]] for nm in names], dtype=np.int32)
    m.set_domains(row)
    clauses = m.eval_clauses_host()
    assert (clauses[:, 0] == clauses[:, 1]).all() and (clauses[:, 0] != 0).all(), "the row violates the model"


def test_max_reports_one_optimal_row():
    """examples/wcet.txt, MAX 1560: the incumbent is the largest over the ranks (INT32_MIN before the first)"""
    from csolve_amd.solver import Model
    path = golden("problems", "ref_wcet.txt")
    out = cli(["-j", "2"], path)
    sols = solution_lines(out)
    assert len(sols) == 1, out[-500:]
    vals, best = values(sols[0])
    assert best == 1560
    st = stats_lines(out)
    assert [m.group(1) for m in st] == ["2", "1"] and int(st[0].group(5)) >= 1 and st[0].group(5) == st[1].group(5)
    m = Model.from_text(open(path).read())
    names = m.var_names()
    assert vals[names[m.objective_var]] == 1560
    m.set_domains(np.array([[vals[nm], vals[nm]] for nm in names], dtype=np.int32))
    clauses = m.eval_clauses_host()
    assert (clauses[:, 0] == clauses[:, 1]).all() and (clauses[:, 0] != 0).all(), "the row violates the model"


def test_any_reports_the_first_solution_only(tmp_path):
    out = cli(["-j", "2"], problems.queens(24), tmp_path)
    sols = solution_lines(out)
    assert len(sols) == 1, out[-500:]
    assert_queens(values(sols[0])[0], 24)
    st = stats_lines(out)
    assert [m.group(1) for m in st] == ["2", "1"] and all(m.group(5) == "1" for m in st)


def test_time_limit_is_shared(tmp_path):
    import time
    t0 = time.monotonic()
    out = cli(["-j", "2", "-t", "1"], problems.queens(40, "ALL"), tmp_path, timeout=120)
    assert time.monotonic() - t0 < 90
    assert [m.group(1) for m in stats_lines(out)] == ["2", "1"]


def test_one_job_is_the_single_path():
    """-j 1 and -j 0 take the path of no -j: the same lines (the order in which that path prints ALL rows varies from
    run to run with the device's scheduling), the same one statistics line"""
    q8 = golden("problems", "queens8_all.txt")
    outs = [cli(args, q8) for args in (["-j", "1"], [], ["-j", "0"])]
    lines = [out.splitlines() for out in outs]
    assert sorted(lines[0]) == sorted(lines[1]) == sorted(lines[2])
    assert lines[0][-1] == lines[1][-1] == lines[2][-1] and lines[0][-1].startswith("#1: CALLS: ")
    assert all(line.startswith("#1: ") for line in lines[0]) and len(solution_lines(outs[0])) == 92
    for name in ("ref_schedule.txt", "schedule6_s1.txt"):  # MIN: one row and one statistics line, byte for byte
        path = golden("problems", name)
        plain = cli([], path)
        assert cli(["-j", "1"], path) == plain and cli(["-j", "0"], path) == plain
        assert len(solution_lines(plain)) == 1 and plain.count("CALLS:") == 1


# ---- the API through ctypes -------------------------------------------------------------------------------------------

def engine(text):
    from csolve_amd.solver import Search, solve_root
    model = solve_root(text)
    return model, Search(model, 1 << 18, 1 << 14)


def region(world, n, rows=256):
    L = load_library()
    size = C.c_size_t()
    check(L.csgpu_shard_region_size(world, n, rows, C.byref(size)))
    buf = mmap.mmap(-1, size.value)
    addr = C.addressof(C.c_char.from_buffer(buf))
    check(L.csgpu_shard_region_init(addr, size.value, world, n, rows))
    return buf, addr


def test_take_host_is_take_plus_a_copy():
    L = load_library()
    text = problems.queens(10, "ALL")
    model, seeder = engine(text)
    seeder.put(model.root_state())
    seeder.run(3)
    frontier = seeder.take(1 << 20)
    assert frontier.shape[0] > 8
    _, a = engine(text)
    _, b = engine(text)
    a.put(frontier.contiguous())
    b.put(frontier.contiguous())  # the same pool, in the same order
    want = a.take(5).cpu().numpy()
    host = np.zeros((7, model.n_vars, 2), dtype=np.int32)
    cnt = C.c_int64()
    check(L.csgpu_search_take_host(b._h, host.ctypes.data, 5, C.byref(cnt)))
    assert cnt.value == 5 and (host[:5] == want).all()
    assert a.run(0)["pool"] == b.run(0)["pool"] == frontier.shape[0] - 5
    rest = np.zeros((frontier.shape[0], model.n_vars, 2), dtype=np.int32)
    check(L.csgpu_search_take_host(b._h, rest.ctypes.data, 1 << 20, C.byref(cnt)))
    assert cnt.value == frontier.shape[0] - 5 and (rest[: cnt.value] == a.take(1 << 20).cpu().numpy()).all()
    check(L.csgpu_search_take_host(b._h, host.ctypes.data, 5, C.byref(cnt)))
    assert cnt.value == 0


def test_restarts_are_refused_before_the_region_is_used():
    L = load_library()
    model, s = engine(problems.queens(12))  # ANY: Luby restarts on by default
    buf, addr = region(2, model.n_vars)
    opts = ShardOptions()
    L.csgpu_shard_default_options(C.byref(opts))
    assert (opts.slice_iterations, opts.poll_iterations, opts.seed_states_per_rank, opts.low_water) == (64, 4, 64, 64)
    root = np.ascontiguousarray(model.domains(), dtype=np.int32)
    local, totals = SearchStats(), SearchStats()
    rc = L.csgpu_shard_run(s._h, addr, 0, root.ctypes.data, C.byref(opts), C.byref(local), C.byref(totals))
    assert rc == CSGPU_E_STATE  # returned at once: rank 1 never exists, so a barrier would never open
    assert b"restart" in L.csgpu_last_error()
    model2, t = engine(problems.schedule(6, 1))
    t.set_restart_on_improvement(True)
    buf2, addr2 = region(2, model2.n_vars)
    root2 = np.ascontiguousarray(model2.domains(), dtype=np.int32)
    assert L.csgpu_shard_run(t._h, addr2, 0, root2.ctypes.data, C.byref(opts), C.byref(local),
                             C.byref(totals)) == CSGPU_E_STATE


def test_a_run_without_a_stream_leaves_the_last_error_alone():
    """an engine with no solution stream (MIN) is a normal case: csgpu_shard_run sets no error on its way"""
    L = load_library()
    model, s = engine(golden_text("ref_schedule.txt"))
    buf, addr = region(1, model.n_vars)
    assert L.csgpu_shard_barrier(None) == -1
    before = L.csgpu_last_error()
    opts = ShardOptions()
    L.csgpu_shard_default_options(C.byref(opts))
    root = np.ascontiguousarray(model.domains(), dtype=np.int32)
    local, totals = SearchStats(), SearchStats()
    check(L.csgpu_shard_run(s._h, addr, 0, root.ctypes.data, C.byref(opts), C.byref(local), C.byref(totals)))
    assert totals.best == 11 and totals.done == 1
    assert L.csgpu_last_error() == before


def golden_text(name):
    return open(golden("problems", name)).read()


def test_one_rank_is_a_plain_run():
    L = load_library()
    text = problems.queens(9, "ALL")
    model, plain = engine(text)
    plain.put(model.root_state())
    ref = plain.run()
    assert ref["done"] and ref["solutions"] == 352
    _, s = engine(text)
    s.stream_solutions(4096)
    buf, addr = region(1, model.n_vars)
    rows = []

    def keep(user, rank, values, count, best):
        assert rank == 0 and best == 0
        arr = np.ctypeslib.as_array(values, shape=(count * model.n_vars,))
        rows.extend(arr.reshape(count, model.n_vars).copy())

    fn = SHARD_SOLUTION_FN(keep)
    opts = ShardOptions()
    L.csgpu_shard_default_options(C.byref(opts))
    opts.on_solution = fn
    root = np.ascontiguousarray(model.domains(), dtype=np.int32)
    local, totals = SearchStats(), SearchStats()
    check(L.csgpu_shard_run(s._h, addr, 0, root.ctypes.data, C.byref(opts), C.byref(local), C.byref(totals)))
    for k in ("nodes", "cuts", "solutions"):
        assert getattr(local, k) == ref[k] and getattr(totals, k) == ref[k], k
    assert totals.done == 1 and totals.pool == 0
    assert len(rows) == 352 and len({tuple(r) for r in rows}) == 352
