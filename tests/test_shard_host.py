"""Host side of the C coordinator of csolve_gpu -j (csolve_amd/csrc/cs_shard.c): the transfer plan against
parallel.plan_transfers, the shared region's size and init, and the launcher without a device.  No GPU needed."""
import ctypes as C
import mmap
import os
import re
import subprocess
import time

import numpy as np
import pytest

from conftest import ROOT, golden
from csolve_amd import parallel
from csolve_amd._lib import CsolveError, check, load_library

CSGPU_E_ARG = -1


def c_plan(pools, low_water, max_give=1 << 62):
    L = load_library()
    p = np.asarray(pools, dtype=np.int64)
    out = np.zeros((max(1, len(p) // 2), 3), dtype=np.int64)
    count = C.c_int()
    check(L.csgpu_plan_transfers(p.ctypes.data, len(p), low_water, max_give, out.ctypes.data, C.byref(count)))
    return [tuple(int(v) for v in row) for row in out[: count.value]]


def test_plan_equals_the_python_plan():
    rng = np.random.default_rng(7)
    cases = 0
    for world in range(1, 17):
        for low_water in (0, 1, 8, 64, 1000):
            for _ in range(40):
                scale = int(rng.choice([4, 100, 5000, 1 << 20]))
                pools = rng.integers(0, scale, size=world)
                if rng.random() < 0.3:
                    pools[rng.integers(0, world, size=max(1, world // 2))] = 0  # dry ranks
                if rng.random() < 0.2:
                    pools[:] = pools[0]  # ties everywhere
                assert c_plan(pools, low_water) == parallel.plan_transfers(pools.tolist(), low_water), (pools, low_water)
                cases += 1
    assert cases >= 3000


def test_plan_caps_a_transfer_and_pairs_each_rank_once():
    rng = np.random.default_rng(11)
    for world in range(2, 17):
        for _ in range(100):
            pools = rng.integers(0, 10000, size=world)
            pools[rng.integers(0, world)] = 0
            cap = int(rng.integers(1, 50))
            plan = c_plan(pools, 64, cap)
            ranks = [r for src, dst, _ in plan for r in (src, dst)]
            assert len(ranks) == len(set(ranks))
            assert all(0 < cnt <= cap for _, _, cnt in plan)
            assert all(pools[src] > pools[dst] for src, dst, _ in plan)
    assert c_plan([10, 0], 64, 3) == [(0, 1, 3)]


def test_plan_rejects_bad_arguments():
    L = load_library()
    p = np.array([1, 2], dtype=np.int64)
    out = np.zeros((1, 3), dtype=np.int64)
    count = C.c_int()
    assert L.csgpu_plan_transfers(p.ctypes.data, 0, 64, 10, out.ctypes.data, C.byref(count)) == CSGPU_E_ARG
    assert L.csgpu_plan_transfers(p.ctypes.data, 2, 64, 0, out.ctypes.data, C.byref(count)) == CSGPU_E_ARG
    neg = np.array([-1, 5], dtype=np.int64)
    assert L.csgpu_plan_transfers(neg.ctypes.data, 2, 64, 10, out.ctypes.data, C.byref(count)) == CSGPU_E_ARG


def region_size(world, n_vars, inbox_rows):
    size = C.c_size_t()
    rc = load_library().csgpu_shard_region_size(world, n_vars, inbox_rows, C.byref(size))
    return rc, size.value


def test_region_size_and_init():
    L = load_library()
    for world, n, rows in ((0, 8, 16), (9, 8, 16), (-1, 8, 16), (2, 0, 16), (2, 8, 0)):
        assert region_size(world, n, rows)[0] == CSGPU_E_ARG, (world, n, rows)
    rc, small = region_size(2, 8, 16)
    assert rc == 0 and small > 0
    rc, big = region_size(2, 8, 32)
    assert rc == 0 and big - small == 2 * 16 * 8 * 8  # two inboxes, 16 more rows of 8 csgpu_val each
    assert region_size(8, 8, 16)[1] > region_size(2, 8, 16)[1]
    assert region_size(2, 16, 16)[1] > small
    buf = mmap.mmap(-1, big)
    addr = C.addressof(C.c_char.from_buffer(buf))
    try:
        assert L.csgpu_shard_region_init(addr, big - 1, 2, 8, 32) == CSGPU_E_ARG  # one byte short
        assert L.csgpu_shard_region_init(addr, big, 9, 8, 32) == CSGPU_E_ARG
        assert L.csgpu_shard_region_init(addr, big, 2, 0, 32) == CSGPU_E_ARG
        check(L.csgpu_shard_region_init(addr, big, 2, 8, 32))
        one = mmap.mmap(-1, region_size(1, 8, 32)[1])
        a1 = C.addressof(C.c_char.from_buffer(one))
        check(L.csgpu_shard_region_init(a1, len(one), 1, 8, 32))
        check(L.csgpu_shard_barrier(a1))  # a world of one never waits
        with pytest.raises(CsolveError):
            check(L.csgpu_shard_barrier(None))
    finally:
        del addr
        buf.close()


def _rank_processes(tag):
    found = []
    for pid in os.listdir("/proc"):
        if not pid.isdigit():
            continue
        try:
            with open(f"/proc/{pid}/cmdline", "rb") as f:
                cmd = f.read().split(b"\0")
        except OSError:
            continue
        if b"--shard-rank" in cmd and tag.encode() in b" ".join(cmd):
            found.append(int(pid))
    return found


def test_ranks_without_a_device_fail_loudly_and_leave_nothing(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    problem = tmp_path / "queens8_all_nodevice.txt"
    problem.write_text(open(golden("problems", "queens8_all.txt")).read())
    exe = os.path.join(ROOT, "csolve_amd", "csolve_gpu")
    t0 = time.monotonic()
    p = subprocess.run([exe, "-j", "3", str(problem)], capture_output=True, text=True, timeout=60)
    assert time.monotonic() - t0 < 60
    assert p.returncode == 1 and "error:" in p.stderr, (p.returncode, p.stderr)
    assert "rank" in p.stderr
    assert _rank_processes(str(problem)) == []


def test_the_launcher_makes_no_hip_call(tmp_path):
    """The launcher of -j parses, spawns and supervises without a single HIP call (a HIP call, even hipFree(NULL),
    starts the runtime and opens the device in the process every rank is spawned from).  The HIP runtime logs every API
    call with the caller's pid at AMD_LOG_LEVEL=4: the launcher's pid must not appear, the ranks' do."""
    problem = tmp_path / "queens8_all_hiplog.txt"
    problem.write_text(open(golden("problems", "queens8_all.txt")).read())
    exe = os.path.join(ROOT, "csolve_amd", "csolve_gpu")
    env = dict(os.environ, AMD_LOG_LEVEL="4")
    p = subprocess.Popen([exe, "-j", "2", str(problem)], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                         env=env, text=True)
    _, err = p.communicate(timeout=120)
    pids = {int(m) for m in re.findall(r"\[pid:(\d+) ", err)}
    assert pids, "the ranks' HIP calls are logged (else this test sees nothing)"
    assert p.pid not in pids, [line for line in err.splitlines() if f"[pid:{p.pid} " in line][:5]
    assert _rank_processes(str(problem)) == []


def test_text_num_vars_is_host_only():
    L = load_library()
    n = C.c_int()
    check(L.csgpu_text_num_vars(open(golden("problems", "queens8_all.txt")).read().encode(), 1, C.byref(n)))
    assert n.value == 8
    assert L.csgpu_text_num_vars(b"ANY; x = ;", 1, C.byref(n)) == -2  # CSGPU_E_PARSE
    assert b"syntax error" in L.csgpu_last_error()
