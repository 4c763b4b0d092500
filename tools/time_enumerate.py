"""Enumeration of queens-N ALL on one GPU (default queens-16, 14,772,512 solutions): the same search three ways, the
variants alternating in one process, one JSON line per run --
  count   the stream off: the solutions are counted, not kept (what bench.py's search record times);
  device  the solution stream on, drained after every run call into a reused device buffer;
  host    the stream on, drained into a reused pinned host buffer, every batch checksummed (the consumer).
Each line: variant, round, seconds (put + runs + drains, device synchronised), rows and bytes drained, the search's
solutions, run calls, checksum (host).  The engine buffers are those of bench.py's search record and are allocated
outside the timed region.
usage: time_enumerate.py [--n 16] [--rounds 3] [--variants count,device,host] [--stream-rows R] [--package-root DIR]
--package-root imports csolve_amd from another tree (a build of another commit: the count-only baseline)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--variants", default="count,device,host")
ap.add_argument("--stream-rows", type=int, default=1 << 26)
ap.add_argument("--children", type=int, default=1 << 23)
ap.add_argument("--package-root", default=ROOT)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from csolve_amd import problems  # noqa: E402
from csolve_amd._lib import check, load_library  # noqa: E402
from csolve_amd.solver import Search, solve_root  # noqa: E402

torch.cuda.set_device(0)
model = solve_root(problems.queens(args.n, "ALL"))
n = model.n_vars
variants = args.variants.split(",")
engines, bufs = {}, {}
for v in variants:
    engines[v] = Search(model, 8 * args.children, args.children)
    if v != "count":
        engines[v].stream_solutions(args.stream_rows)
if "device" in variants:
    bufs["device"] = torch.empty((args.stream_rows, n), dtype=torch.int32, device="cuda")
if "host" in variants:
    bufs["host"] = torch.empty((args.stream_rows, n), dtype=torch.int32, pin_memory=True)
root = model.root_state()
L = load_library()


def once(v):
    s = engines[v]
    s.reset()
    rows, calls, checksum = 0, 0, 0
    got = C.c_int64()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.put(root)
    while True:
        st = s.run(1 << 40)
        calls += 1
        if v == "device":
            check(L.csgpu_search_drain_solutions_device(s._h, bufs[v].data_ptr(), args.stream_rows, C.byref(got),
                                                        torch.cuda.current_stream().cuda_stream))
            rows += got.value
        elif v == "host":
            check(L.csgpu_search_drain_solutions(s._h, bufs[v].data_ptr(), args.stream_rows, C.byref(got)))
            rows += got.value
            checksum += int(bufs[v].numpy()[: got.value].sum(dtype=np.int64))
        if st["done"]:
            break
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(variant=v, n=args.n, seconds=round(dt, 6), rows=rows, bytes=rows * n * 4, solutions=st["solutions"],
                iterations=st["iterations"], run_calls=calls, checksum=checksum if v == "host" else None, stream_rows=args.stream_rows if v != "count" else 0)


for v in variants:  # warm-up: first launches, the planner, the pool's first touch
    once(v)
for r in range(args.rounds):
    for v in variants:
        print(json.dumps(dict(once(v), round=r)), flush=True)
