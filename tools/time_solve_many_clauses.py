#!/usr/bin/env python3
"""K instances of one clause model through Model.solve_many_clauses, and the SAME instances through the per-instance loop
that was the only route for such models: one Search, reset and seeded per instance (the instance's root fixpoint, put,
run), one after the other -- on a sample of the instances when all K would take minutes (the output says how many).
Both routes run in this process after a warm-up, interleaved, so that a drift of the machine falls on both alike.

Prints one JSON line: medians and ranges of both routes, instances/s and their ratio, what the call decided, and a
seeded sample of the device's answers re-checked against the host walk (tests/many_walk_objective.py).  Under MIN / MAX
the optimum of every DONE instance of the loop's sample is compared with the engine's as well.

  python tools/time_solve_many_clauses.py --set schedule5_min [--count 4096] [--reps 5] [--loop-sample 128] [--check 16]
  sets: the names of tests/many_clause_sets.py; the set's rows are repeated with other seeds up to --count.

--sliced B1,B2,... [--finish resume|search] [--budget N] times, in place of the per-instance loop, the sliced route
(Model.solve_many_clauses_sliced on one reused pool: a checkpointed call with B1, a resume per further budget while an
instance is at LIMIT, then with --finish search one reused Search for every instance still stopped) beside the one call
with the summed budget (or --budget), interleaved in this process; the first slice is timed on its own as well.  The
sliced answers of the seeded sample are re-checked against the host walk: field for field with --finish resume; with
--finish search every instance DONE and `best` the host walk's proven optimum where 32,768 more nodes prove one.

--upto K [--budget N] times, in place of the per-instance loop, Model.solve_many_clauses_upto(k=K) beside the ANY and the
ALL call of the same rows and the same budget, the three interleaved in this process: what "is the timetable unique?"
(K = 2) or "K alternatives per row" costs between the one row of ANY and the whole tree of ALL.  The seeded sample is
re-checked against the host walk (tests/many_walk_clauses_upto.py), rows included.  With --sliced the slices are up-to-K
calls (solve_many_clauses_sliced(max_solutions=K), --finish resume only) beside the one up-to-K call.

--restarts BASE [--rotate-first] [--budget N] times Model.solve_many_clauses_restarts(restart_base=BASE) beside the ANY call
of the same rows and the same budget (default 20,000), and the restart call with base 0 -- which is the ANY walk -- beside
both, the three interleaved in this process.  The rows are not a set of the tests: --count windows of problems.schedule(10,
1) as tests/many_clause_restart_sets.py draws its tail workload (width 30, at most 40 values for `end`, rows seed 11), walk
seed 7.  A launch lasts as long as its deepest instance: the output has the deepest walk and the nodes in all of both
calls.  The seeded sample is re-checked against the host walk (tests/many_walk_clauses_restarts.py).

--stream ROWS [--budget N] times three routes to every solution of every instance, interleaved in this process after a
warm-up: the counting ALL call (solve_many_clauses, no rows at all), ONE solve_many_clauses_stream call into a stream with
room for everything (pool and stream made once, reset per repetition), and the loop solve_many_clauses_all with a stream
of ROWS rows (its pool and stream made per repetition, as a caller's would be).  The rows are those of
tests/many_clause_stream_sets.py (--set one of its names, default wcet_max), repeated up to --count; every walk ends within
the default budget of 16,000 nodes.  The records of both stream routes must equal the counting call's in every field, and
the rows of the seeded sample the host walk's, in walk order.

--spread B1,B2,... [--spread-rows ROWS] [--budget N] times Model.solve_many_clauses_spread (ALL; the stopped instances of a
round fanned out over the waves of the next, budget B1 for round 0, B2 for round 1, the last one repeated; --spread-rows:
its max_rows) beside the counting ALL call of solve_many_clauses on the same rows (--set, walked under ALL whatever the
set's objective, repeated up to --count) and the same budget, interleaved in this process after a warm-up, two pools kept
over the calls: medians and ranges of --reps, rounds and rows per round, the launch of round 0 alone, and whether every
field of every instance -- props and root_props included -- and every first solution equals the one call's.
--spread-objective own (default all): on a MIN / MAX set, the one call and the spread walk under the set's objective instead
(solve_many_clauses_spread(roots, "MIN" / "MAX"): start incumbents); the check is then that every instance the one call
ends is ended by the spread with the same optimum, and the spread's own nodes are printed beside the one call's.

--spread B1,B2,... --order NAME --split W [--spread-objective own] times the ORDERED spread
(solve_many_clauses_spread(..., order=NAME, split_width=W)) beside the one solve_many_clauses_ordered call of the same rows
and prints the nodes and the halving counts of both, as --spread does; --set may then be a set of
tests/many_walk_ordered.py as well (schedule5_open_min: the rows that leave `end` at its root width).

--order NAME --split W [--budget N] times Model.solve_many_clauses_ordered(order=NAME, split_width=W) beside the plain call
of solve_many_clauses on the same rows and the same budget, alternating in this process after a warm-up (--set: a set of
tests/many_clause_sets.py or of tests/many_walk_ordered.py, e.g. schedule5_open_min, whose rows leave `end` at its root
width; repeated up to --count): medians and ranges of both, both node totals, how many rows each leaves at LIMIT, the
time per node of both, whether every field equals the plain call's (what smallest-domain gives where nothing halves),
and the seeded sample of the ordered answers re-checked against the host walk (tests/many_walk_ordered.py).

--order NAME --split W --sliced B1,B2,... [--finish resume|search] times the sliced ordered route
(Model.solve_many_clauses_sliced(order=NAME, split_width=W) on one reused pool of many_clause_ordered_checkpoints) beside
the ONE ordered call with the summed budget, alternating in this process after a warm-up; the first slice -- the fresh
checkpointed call with B1 -- is timed on its own as well, so `--sliced N` with an N no instance reaches is the cost of the
checkpoint switch alone.  Every field of the sliced answer must equal the one call's (--finish resume; with --finish
search every instance ends DONE and `best` is the one call's where that one is DONE), and the seeded sample is re-checked
against the host walk.

--wide [--set NAME] [--budget N] times Model.solve_many_clauses_wide (the clause records in LDS, no 512-clause limit).  NAME
is a case of tests/many_clause_wide_sets.py (default sudoku_less_any; schedule32_min, ...: past 512 clauses), whose rows are
repeated up to --count: the wide call beside one Search per instance -- the only other route for such a model -- on a
sample, alternating in this process after a warm-up.  Or NAME is a set of tests/many_clause_sets.py (at most 512 clauses):
then the wide call beside the plain call of solve_many_clauses on the same rows and budget -- the price of LDS records --
with every field compared, and the Search loop beside both.  The output has the resident workgroups per CU and the LDS
per workgroup of the kernels, and the seeded sample re-checked against the host walk.  --loop-iterations N stops the engine
after N iterations per instance (a MIN row without a deadline has no end a measurement could wait for); the output says
how many instances of the sample that left unfinished."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from csolve_amd.solver import Search, solve_root  # noqa: E402


def commit():
    try:
        return open(os.path.join(ROOT, "csolve_amd", "csrc", "build", "COMMIT")).read().strip()
    except OSError:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()


def spread(ts, scale=1e3):
    return {"median": round(statistics.median(ts) * scale, 3), "min": round(min(ts) * scale, 3), "max": round(max(ts) * scale, 3),
            "reps": len(ts)}


def main():
    import many_clause_sets as sets
    import many_walk_objective as W
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default=None, help="a set of tests/many_clause_sets.py (default schedule5_min); with --stream one "
                                                "of tests/many_clause_stream_sets.py (default wcet_max)")
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-sample", type=int, default=128)
    ap.add_argument("--check", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sliced", default=None, help="B1,B2,...: the budgets of the sliced route")
    ap.add_argument("--finish", default="resume", choices=("resume", "search"))
    ap.add_argument("--upto", type=int, default=None, help="K: time solve_many_clauses_upto beside the ANY and the ALL call")
    ap.add_argument("--budget", type=int, default=None, help="the one call's budget (default: the set's, or the sum of --sliced)")
    ap.add_argument("--restarts", type=int, default=None, help="BASE: time solve_many_clauses_restarts beside the ANY call")
    ap.add_argument("--rotate-first", action="store_true", help="with --restarts: run 0 rotates as well")
    ap.add_argument("--stream", type=int, default=None, help="ROWS: time the counting ALL call, one stream call with room for "
                                                             "everything and the loop with a stream of ROWS rows")
    ap.add_argument("--spread", default=None, help="B1,B2,...: time solve_many_clauses_spread beside the counting ALL call")
    ap.add_argument("--spread-rows", type=int, default=1 << 18, help="max_rows of solve_many_clauses_spread")
    ap.add_argument("--spread-objective", default="all", choices=("all", "own"),
                    help="own: walk a MIN / MAX set under its objective (the spread with start incumbents)")
    ap.add_argument("--order", default=None, help="NAME: time solve_many_clauses_ordered beside the plain call (with --split)")
    ap.add_argument("--split", type=int, default=256, help="with --order: split_width")
    ap.add_argument("--loop-iterations", type=int, default=1 << 62, help="with --wide: at most so many engine iterations per "
                                                                         "instance of the Search loop (default: to the end)")
    ap.add_argument("--wide", action="store_true", help="time solve_many_clauses_wide beside one Search per instance, and on a "
                                                        "set of at most 512 clauses beside the plain call as well")
    args = ap.parse_args()
    if args.wide:
        if args.order is not None or args.spread is not None or args.stream is not None or args.sliced or \
                args.upto is not None or args.restarts is not None:
            ap.error("--wide: without --order, --spread, --stream, --sliced, --upto and --restarts")
        return wide_route(args)
    if args.order is not None and args.spread is None:
        if args.stream is not None or args.upto is not None or args.restarts is not None:
            ap.error("--order NAME: without --stream, --upto and --restarts")
        return order_sliced_route(args) if args.sliced else order_route(args)
    if args.spread is not None:
        if args.stream is not None or args.sliced or args.upto is not None or args.restarts is not None:
            ap.error("--spread B1,B2,...: without --stream, --sliced, --upto and --restarts")
        return spread_route(args)
    if args.stream is not None:
        if args.stream < 1 or args.sliced or args.upto is not None or args.restarts is not None:
            ap.error("--stream ROWS: ROWS >= 1, without --sliced, --upto and --restarts")
        return stream_route(args)
    args.set = args.set or "schedule5_min"
    if args.set not in sets.SETS:
        ap.error(f"--set: one of {sorted(sets.SETS)}")
    if args.restarts is not None:
        if args.restarts < 0 or args.sliced or args.upto is not None:
            ap.error("--restarts BASE: BASE >= 0, without --sliced and --upto")
        return restart_route(args)
    if args.upto is not None and (args.upto < 1 or args.finish == "search"):
        ap.error("--upto K: K >= 1, and with --sliced --finish resume only")
    text, base, objective, budget = sets.build(args.set)
    budgets = tuple(int(b) for b in args.sliced.split(",")) if args.sliced else None
    if budgets:
        budget = sum(budgets)
    if args.budget:
        budget = args.budget
    roots = np.tile(np.array(base), (-(-args.count // len(base)), 1, 1))[:args.count]
    count = len(roots)
    model = solve_root(text)
    dev = torch.from_numpy(roots).cuda()
    rng = np.random.default_rng(args.seed)
    sample = np.sort(rng.choice(count, size=min(args.loop_sample, count), replace=False))
    search = Search(model, 1 << 18, 1 << 14)
    node = torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32, device="cuda")

    def many():
        torch.cuda.synchronize()
        t = time.perf_counter()
        if args.upto is not None:
            out = model.solve_many_clauses_upto(dev, args.upto, max_nodes=budget)
        else:
            out = model.solve_many_clauses(dev, objective, max_nodes=budget)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def loop():
        total, bests = 0, {}
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in sample:
            state, res = model.propagate(dev[i:i + 1], node)
            if int(res[0, 0]) <= 0:  # inconsistent, or solved by the root node
                continue
            search.reset()
            search.put(state)
            st = search.run()
            total += st["nodes"]
            bests[int(i)] = (st["best"], st["solutions"])
        torch.cuda.synchronize()
        return time.perf_counter() - t, total, bests

    if budgets:
        return sliced_route(args, model, text, roots, dev, objective, budget, budgets, many, rng, W)
    if args.upto is not None:
        return upto_route(args, model, text, roots, dev, budget, many, rng)
    for _ in range(2):  # warm-up: code load, workspace, the engine's buffers
        many()
    loop()
    many_times, loop_times = [], []
    for _ in range(args.reps):
        dt, out = many()
        many_times.append(dt)
        dt, loop_nodes, bests = loop()
        loop_times.append(dt)
    host = {k: v.cpu().numpy() for k, v in out.items() if torch.is_tensor(v)}

    picks = rng.choice(count, size=min(args.check, count), replace=False)
    want = W.walk_many(text, roots[picks], objective, budget)
    has = want["solutions"] > 0
    ok = all((host[f][picks] == want[f]).all() for f in W.FIELDS) and bool((host["first"][picks][has] == want["first"][has]).all())
    if objective in ("MIN", "MAX"):
        ok = ok and bool((host["best"][picks][has] == want["best"][has]).all())
        done = [i for i in bests if host["status"][i] == 0 and host["solutions"][i] > 0]
        same_optimum = all(bests[i][0] == host["best"][i] for i in done)
    else:
        done, same_optimum = [], None

    t_many, t_loop = statistics.median(many_times), statistics.median(loop_times)
    many_rate, loop_rate = count / t_many, len(sample) / t_loop
    print(json.dumps({
        "tool": "time_solve_many_clauses", "commit": commit(), "command": " ".join(sys.argv), "set": args.set,
        "objective": objective, "instances": count, "max_nodes": budget, "n_vars": model.n_vars, "clauses": model.n_clauses,
        "kernel": model.many_clauses_kernel(), "waves": model.many_clauses_waves(count),
        "status_counts": np.bincount(host["status"], minlength=3).tolist(), "nodes": int(host["nodes"].sum()),
        "largest_tree": int(host["nodes"].max()), "solutions": int(host["solutions"].sum()),
        "solve_many_clauses_ms": spread(many_times), "solve_many_clauses_instances_per_s": round(many_rate),
        "solve_many_clauses_nodes_per_s": round(int(host["nodes"].sum()) / t_many),
        "loop_instances": len(sample), "loop_nodes": loop_nodes, "loop_s": spread(loop_times, 1.0),
        "loop_instances_per_s": round(loop_rate), "ratio_instances_per_s": round(many_rate / loop_rate, 1),
        "optima_compared_with_the_engine": len(done), "same_optimum": same_optimum,
        "oracle_checked": len(picks), "oracle_ok": bool(ok),
    }))
    return 0 if ok and same_optimum is not False else 1


def wide_route(args):
    """the wide call beside one Search per instance and, at most 512 clauses, beside the plain call"""
    import many_clause_sets as sets
    import many_clause_wide_sets as wsets
    import many_walk_objective as W
    name = args.set or "sudoku_less_any"
    if name not in wsets.CASES and name not in sets.SETS:
        raise SystemExit(f"--wide: --set is one of {sorted(wsets.CASES)} or of {sorted(sets.SETS)}")
    text, base, objective, budget = (wsets if name in wsets.CASES else sets).build(name)
    budget = args.budget or budget
    roots = np.tile(np.array(base), (-(-args.count // len(base)), 1, 1))[:args.count]
    count = len(roots)
    model = solve_root(text)
    dev = torch.from_numpy(roots).cuda()
    rng = np.random.default_rng(args.seed)
    sample = np.sort(rng.choice(count, size=min(args.loop_sample, count), replace=False))
    search = Search(model, 1 << 18, 1 << 14)
    node = torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32, device="cuda")
    plain = model.qualifies_many_clauses()

    def timed(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def loop():  # the engine has no node budget per instance: --loop-iterations bounds its steps instead
        total, unfinished = 0, 0
        for i in sample:
            state, res = model.propagate(dev[i:i + 1], node)
            if int(res[0, 0]) <= 0:  # inconsistent, or solved by the root node
                continue
            search.reset()
            search.put(state)
            st = search.run(args.loop_iterations)
            total += st["nodes"]
            unfinished += st["done"] == 0
        return total, unfinished

    calls = {"wide": lambda: model.solve_many_clauses_wide(dev, objective, max_nodes=budget), "loop": loop}
    if plain:
        calls["plain"] = lambda: model.solve_many_clauses(dev, objective, max_nodes=budget)
    for _ in range(2):  # warm-up: code load, workspace, the engine's buffers
        for call in calls.values():
            timed(call)
    times, outs = {k: [] for k in calls}, {}
    for _ in range(args.reps):  # alternating: a drift of the machine falls on all alike
        for k, call in calls.items():
            dt, outs[k] = timed(call)
            times[k].append(dt)
    host = {k: {f: v.cpu().numpy() for f, v in outs[k].items() if torch.is_tensor(v)} for k in calls if k != "loop"}
    got = host["wide"]
    same = all(bool((got[f] == host["plain"][f]).all()) for f in got) if plain else None
    picks = rng.choice(count, size=min(args.check, count), replace=False)
    want = W.walk_many(text, roots[picks], objective, budget)
    has = want["solutions"] > 0
    ok = all((got[f][picks] == want[f]).all() for f in W.FIELDS) and bool((got["first"][picks][has] == want["first"][has]).all())
    if objective in ("MIN", "MAX"):
        ok = ok and bool((got["best"][picks][has] == want["best"][has]).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    wide_rate, loop_rate = count / med["wide"], len(sample) / med["loop"]
    waves = model.many_clauses_wide_waves(1 << 30)
    record = {
        "tool": "time_solve_many_clauses", "route": "wide", "commit": commit(), "command": " ".join(sys.argv), "set": name,
        "objective": objective, "instances": count, "max_nodes": budget, "n_vars": model.n_vars, "clauses": model.n_clauses,
        "wide_kernel": model.many_clauses_wide_kernel(), "wide_waves": model.many_clauses_wide_waves(count),
        "wide_resident_waves": waves, "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
        "wide_workgroups_per_cu": waves // 4 // torch.cuda.get_device_properties(0).multi_processor_count,
        "status_counts": np.bincount(got["status"], minlength=3).tolist(), "nodes": int(got["nodes"].sum()),
        "largest_tree": int(got["nodes"].max()), "solutions": int(got["solutions"].sum()),
        "wide_ms": spread(times["wide"]), "wide_instances_per_s": round(wide_rate),
        "wide_ns_per_node": round(med["wide"] * 1e9 / max(int(got["nodes"].sum()), 1), 2),
        "loop_instances": len(sample), "loop_nodes": int(outs["loop"][0]), "loop_iterations_at_most": args.loop_iterations,
        "loop_unfinished": int(outs["loop"][1]), "loop_s": spread(times["loop"], 1.0),
        "loop_instances_per_s": round(loop_rate), "wide_over_loop_instances_per_s": round(wide_rate / loop_rate, 1),
    }
    if plain:
        pw = model.many_clauses_waves(1 << 30)
        record.update({"plain_kernel": model.many_clauses_kernel(), "plain_ms": spread(times["plain"]),
                       "plain_resident_waves": pw,
                       "plain_workgroups_per_cu": pw // 4 // torch.cuda.get_device_properties(0).multi_processor_count,
                       "wide_over_plain": round(med["wide"] / med["plain"], 4), "every_field_equals_the_plain_call": same})
    record.update({"oracle_checked": len(picks), "oracle_ok": bool(ok)})
    print(json.dumps(record))
    return 0 if ok and same is not False else 1


def order_route(args):
    """the ordered call beside the plain call of the same rows, same budget, same build"""
    import many_clause_sets as sets
    import many_walk_ordered as O
    name = args.set or "schedule5_min"
    if name not in sets.SETS and name not in O.SETS:
        raise SystemExit(f"--order: --set is one of {sorted(set(sets.SETS) | set(O.SETS))}")
    if args.order not in O.ORDERS or args.split < 1:
        raise SystemExit(f"--order is one of {O.ORDERS}, --split at least 1")
    text, base, objective, budget = (sets if name in sets.SETS else O).build(name)
    budget = args.budget or budget
    roots = np.tile(np.array(base), (-(-args.count // len(base)), 1, 1))[:args.count]
    count = len(roots)
    model = solve_root(text)
    dev = torch.from_numpy(roots).cuda()
    rng = np.random.default_rng(args.seed)

    def timed(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    calls = {"plain": lambda: model.solve_many_clauses(dev, objective, max_nodes=budget),
             "ordered": lambda: model.solve_many_clauses_ordered(dev, objective, max_nodes=budget, order=args.order,
                                                                 split_width=args.split)}
    for _ in range(2):  # warm-up: code load, workspace
        for call in calls.values():
            timed(call)
    times, outs = {k: [] for k in calls}, {}
    for _ in range(args.reps):  # alternating: a drift of the machine falls on both alike
        for k, call in calls.items():
            dt, outs[k] = timed(call)
            times[k].append(dt)
    host = {k: {f: v.cpu().numpy() for f, v in o.items() if torch.is_tensor(v)} for k, o in outs.items()}
    plain, got = host["plain"], host["ordered"]
    same = all(bool((got[f] == plain[f]).all()) for f in plain)
    picks = rng.choice(count, size=min(args.check, count), replace=False)
    want = O.walk_many(text, roots[picks], objective, budget, args.order, args.split)
    has = want["solutions"] > 0
    ok = all((got[f][picks] == want[f]).all() for f in ("status", "nodes", "cuts", "solutions", "halvings")) and \
        bool((got["first"][picks][has] == want["first"][has]).all())
    if objective in ("MIN", "MAX"):
        ok = ok and bool((got["best"][picks][has] == want["best"][has]).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    nodes = {k: int(host[k]["nodes"].sum()) for k in calls}
    print(json.dumps({
        "tool": "time_solve_many_clauses", "route": "order", "commit": commit(), "command": " ".join(sys.argv), "set": name,
        "objective": objective, "order": args.order, "split_width": args.split, "instances": count, "max_nodes": budget,
        "n_vars": model.n_vars, "clauses": model.n_clauses, "kernel": model.many_clauses_kernel(),
        "order_kernel": model.many_clauses_order_kernel(), "waves": model.many_clauses_waves(count),
        "frames_per_wave": {"plain": model.n_vars, "ordered": model.many_clauses_ordered_frames(args.split)},
        "plain_ms": spread(times["plain"]), "ordered_ms": spread(times["ordered"]),
        "ordered_over_plain": round(med["ordered"] / med["plain"], 4),
        "plain_nodes": nodes["plain"], "ordered_nodes": nodes["ordered"],
        "plain_ns_per_node": round(med["plain"] * 1e9 / max(nodes["plain"], 1), 2),
        "ordered_ns_per_node": round(med["ordered"] * 1e9 / max(nodes["ordered"], 1), 2),
        "plain_status_counts": np.bincount(plain["status"], minlength=3).tolist(),
        "ordered_status_counts": np.bincount(got["status"], minlength=3).tolist(),
        "plain_largest_tree": int(plain["nodes"].max()), "ordered_largest_tree": int(got["nodes"].max()),
        "halvings": int(got["halvings"].sum()), "every_field_equals_the_plain_call": same,
        "oracle_checked": len(picks), "oracle_ok": bool(ok),
    }))
    return 0 if ok else 1


def order_sliced_route(args):
    """the sliced ordered route beside the one ordered call with the summed budget, same rows, same build"""
    import many_clause_sets as sets
    import many_walk_ordered as O
    name = args.set or "schedule5_min"
    if name not in sets.SETS and name not in O.SETS:
        raise SystemExit(f"--order: --set is one of {sorted(set(sets.SETS) | set(O.SETS))}")
    if args.order not in O.ORDERS or args.split < 1:
        raise SystemExit(f"--order is one of {O.ORDERS}, --split at least 1")
    text, base, objective, _ = (sets if name in sets.SETS else O).build(name)
    budgets = tuple(int(b) for b in args.sliced.split(","))
    budget = sum(budgets)
    roots = np.tile(np.array(base), (-(-args.count // len(base)), 1, 1))[:args.count]
    count = len(roots)
    model = solve_root(text)
    dev = torch.from_numpy(roots).cuda()
    rng = np.random.default_rng(args.seed)
    pool = model.many_clause_ordered_checkpoints(count, args.split)
    how = dict(order=args.order, split_width=args.split)

    def timed(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    calls = {"one": lambda: model.solve_many_clauses_ordered(dev, objective, max_nodes=budget, **how),
             "first": lambda: model.solve_many_clauses_ordered(dev, objective, max_nodes=budgets[0], checkpoints=pool.reset(), **how),
             "sliced": lambda: model.solve_many_clauses_sliced(dev, objective, budgets=budgets, finish=args.finish,
                                                               checkpoints=pool, **how)}
    for _ in range(2):  # warm-up: code load, workspace, the engine's buffers
        for call in calls.values():
            timed(call)
    times, outs = {k: [] for k in calls}, {}
    for _ in range(args.reps):  # alternating: a drift of the machine falls on all alike
        for k, call in calls.items():
            dt, outs[k] = timed(call)
            times[k].append(dt)
    sliced_info = outs["sliced"]["sliced"]
    host = {k: {f: v.cpu().numpy() for f, v in o.items() if torch.is_tensor(v) and not f.startswith("_")} for k, o in outs.items()}
    one, got = host["one"], host["sliced"]
    if args.finish == "resume":
        same = all(bool((got[f] == one[f]).all()) for f in one)
    else:
        done = (one["status"] == 0) & (one["solutions"] > 0)
        same = bool((got["status"] == 0).all())
        if objective in ("MIN", "MAX"):
            same = same and bool((got["best"][done] == one["best"][done]).all())
    picks = rng.choice(count, size=min(args.check, count), replace=False)
    want = O.walk_many(text, roots[picks], objective, budget, args.order, args.split)
    has = want["solutions"] > 0
    ok = all((one[f][picks] == want[f]).all() for f in ("status", "nodes", "cuts", "solutions", "halvings")) and \
        bool((one["first"][picks][has] == want["first"][has]).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "tool": "time_solve_many_clauses", "route": "order-sliced", "commit": commit(), "command": " ".join(sys.argv), "set": name,
        "objective": objective, "order": args.order, "split_width": args.split, "instances": count, "n_vars": model.n_vars,
        "clauses": model.n_clauses, "order_kernel": model.many_clauses_order_kernel(),
        "order_resume_kernel": model.many_clauses_order_resume_kernel(), "waves": model.many_clauses_waves(count),
        "frames_per_wave": model.many_clauses_ordered_frames(args.split), "slot_bytes": model.clause_ordered_checkpoint_bytes(args.split),
        "one_call_max_nodes": budget, "one_call_status_counts": np.bincount(one["status"], minlength=3).tolist(),
        "one_call_nodes": int(one["nodes"].sum()), "one_call_largest_tree": int(one["nodes"].max()), "one_call_ms": spread(times["one"]),
        "budgets": list(budgets), "finish": args.finish, "sliced": sliced_info,
        "stopped_after_the_first_slice": int((host["first"]["status"] == 1).sum()),
        "first_slice_ms": spread(times["first"]), "sliced_ms": spread(times["sliced"]),
        "sliced_status_counts": np.bincount(got["status"], minlength=3).tolist(), "sliced_nodes": int(got["nodes"].sum()),
        "first_slice_over_one_call": round(med["first"] / med["one"], 4), "sliced_over_one_call": round(med["sliced"] / med["one"], 4),
        "sliced_equals_the_one_call": bool(same), "oracle_checked": len(picks), "oracle_ok": bool(ok),
    }))
    return 0 if ok and same else 1


def restart_route(args):
    """the restart call beside the ANY call of the same rows, same budget, same build; and base 0 beside both"""
    import many_clause_restart_sets as rsets
    import many_clause_sets as sets
    import many_walk_clauses_restarts as R
    from csolve_amd import problems
    tasks, width, deadline, _ = rsets.TAIL["schedule10"]
    text = problems.schedule(tasks, 1)
    roots = np.ascontiguousarray(sets.windows(text, args.count, 11, width, sets._starts(deadline)), dtype=np.int32)
    count, budget, seed = len(roots), args.budget or rsets.TAIL_BUDGET, rsets.TAIL_SEED
    model = solve_root(text)
    dev = torch.from_numpy(roots).cuda()
    rng = np.random.default_rng(args.seed)

    def timed(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    calls = {
        "any": lambda: model.solve_many_clauses(dev, "ANY", max_nodes=budget),
        "base0": lambda: model.solve_many_clauses_restarts(dev, max_nodes=budget, restart_base=0, seed=seed),
        "restarts": lambda: model.solve_many_clauses_restarts(dev, max_nodes=budget, restart_base=args.restarts, seed=seed,
                                                              rotate_first=args.rotate_first),
    }
    for _ in range(2):  # warm-up: code load, workspace
        for call in calls.values():
            timed(call)
    times, outs = {k: [] for k in calls}, {}
    for _ in range(args.reps):
        for k, call in calls.items():
            dt, outs[k] = timed(call)
            times[k].append(dt)
    host = {k: {f: v.cpu().numpy() for f, v in o.items() if torch.is_tensor(v)} for k, o in outs.items()}
    picks = rng.choice(count, size=min(args.check, count), replace=False)
    want = R.walk_many_restarts(text, roots[picks], args.restarts, seed=seed, rotate_first=args.rotate_first, max_nodes=budget)
    has = want["solutions"] > 0
    got = host["restarts"]
    ok = all((got[f][picks] == want[f]).all() for f in ("status", "nodes", "cuts", "solutions", "restarts")) and \
        bool((got["first"][picks][has] == want["first"][has]).all())
    same = all(bool((host["base0"][f] == host["any"][f]).all()) for f in ("status", "root_props", "nodes", "cuts", "props", "solutions", "first"))
    med = {k: statistics.median(v) for k, v in times.items()}
    record = {
        "tool": "time_solve_many_clauses", "route": "restarts", "commit": commit(), "command": " ".join(sys.argv),
        "rows": f"schedule({tasks},1), width {width}, deadline {deadline}, rows seed 11", "walk_seed": seed,
        "restart_base": args.restarts, "rotate_first": bool(args.rotate_first), "instances": count, "max_nodes": budget,
        "n_vars": model.n_vars, "clauses": model.n_clauses, "kernel": model.many_clauses_kernel(),
        "restart_kernel": model.many_clauses_restart_kernel(), "waves": model.many_clauses_waves(count),
        "any_ms": spread(times["any"]), "base0_ms": spread(times["base0"]), "restarts_ms": spread(times["restarts"]),
        "any_over_restarts": round(med["any"] / med["restarts"], 2), "base0_over_any": round(med["base0"] / med["any"], 3),
        "base0_equals_any": same,
    }
    for k in ("any", "restarts"):
        h = host[k]
        record.update({f"{k}_status_counts": np.bincount(h["status"], minlength=3).tolist(), f"{k}_nodes": int(h["nodes"].sum()),
                       f"{k}_deepest": int(h["nodes"].max()), f"{k}_nodes_p50_p99_p999": [int(np.percentile(h["nodes"], q)) for q in (50, 99, 99.9)],
                       f"{k}_solutions": int(h["solutions"].sum())})
    record.update({"restarted": int((got["restarts"] > 0).sum()), "most_restarts": int(got["restarts"].max()),
                   "oracle_checked": len(picks), "oracle_ok": bool(ok)})
    print(json.dumps(record))
    return 0 if ok and same else 1


def stream_route(args):
    """the counting ALL call, one stream call with room for everything, and the loop with a small stream"""
    import many_clause_stream_sets as ssets
    import many_walk_clauses_upto as U
    name = args.set or "wcet_max"
    if name not in ssets.TABLE:
        raise SystemExit(f"--stream: --set is one of {sorted(ssets.TABLE)}")
    text, base = ssets.build(name)
    budget = args.budget or ssets.BUDGET
    roots = np.tile(np.array(base), (-(-args.count // len(base)), 1, 1))[:args.count]
    count = len(roots)
    model = solve_root(text)
    dev = torch.from_numpy(roots).cuda()
    rng = np.random.default_rng(args.seed)
    fields = ("status", "root_props", "nodes", "cuts", "props", "solutions")

    def timed(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    counting = lambda: model.solve_many_clauses(dev, "ALL", max_nodes=budget, solutions=False)  # noqa: E731
    total = int(timed(counting)[1]["solutions"].sum().item())
    pool = model.many_clause_checkpoints(count)
    out = model.many_stream(max(total, 1))

    def streamed():
        return model.solve_many_clauses_stream(dev, out, pool, max_nodes=budget)

    def looped():
        return model.solve_many_clauses_all(dev, max_nodes=budget, stream_rows=args.stream)

    def fresh():  # between the repetitions, outside the timed part
        pool.reset()
        out.count.zero_()

    for _ in range(2):  # warm-up: code load, workspace
        timed(counting), fresh(), timed(streamed), timed(looped)
    times = {"count": [], "stream": [], "loop": []}
    for _ in range(args.reps):
        dt, counted = timed(counting)
        times["count"].append(dt)
        fresh()
        dt, one = timed(streamed)
        times["stream"].append(dt)
        dt, every = timed(looped)
        times["loop"].append(dt)
    host = lambda o: {k: v.cpu().numpy() for k, v in o.items() if torch.is_tensor(v) and not k.startswith("_")}  # noqa: E731
    calls = int(every["calls"])
    counted, one, every = host(counted), host(one), host(every)
    attempts = int(out.count.item())
    owner, rows = (a.cpu().numpy() for a in out.take())
    same = all(bool((one[f] == counted[f]).all()) and bool((every[f] == counted[f]).all()) for f in fields)
    same = same and attempts == total == int(every["offsets"][-1]) and bool((one["slot"] == -1).all())
    picks = rng.choice(count, size=min(args.check, count), replace=False)
    ok = True
    for i in picks:
        want = U.Walk(text, roots[i]).run(budget, None)
        mine = rows[owner == i]  # in stream order, which is walk order within one instance
        lo, hi = int(every["offsets"][i]), int(every["offsets"][i + 1])
        ok = ok and all(int(one[f][i]) == want[f] for f in U.FIELDS) and len(mine) == len(want["rows"]) == hi - lo
        if ok and want["rows"]:
            ok = bool((mine == np.stack(want["rows"])).all()) and bool((every["rows"][lo:hi] == np.stack(want["rows"])).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "tool": "time_solve_many_clauses", "route": "stream", "commit": commit(), "command": " ".join(sys.argv), "set": name,
        "instances": count, "max_nodes": budget, "n_vars": model.n_vars, "clauses": model.n_clauses,
        "kernel": model.many_clauses_kernel(), "stream_kernel": model.many_clauses_stream_kernel(),
        "waves": model.many_clauses_waves(count), "slot_bytes": model.clause_checkpoint_bytes(),
        "status_counts": np.bincount(counted["status"], minlength=5).tolist(), "nodes": int(counted["nodes"].sum()),
        "largest_tree": int(counted["nodes"].max()), "solutions": total,
        "solutions_per_node": round(total / max(int(counted["nodes"].sum()), 1), 3),
        "count_ms": spread(times["count"]), "stream_ms": spread(times["stream"]), "loop_ms": spread(times["loop"]),
        "stream_rows": args.stream, "loop_calls": calls,
        "stream_over_count": round(med["stream"] / med["count"], 3), "loop_over_count": round(med["loop"] / med["count"], 3),
        "records_equal_the_counting_call": bool(same), "oracle_checked": len(picks), "oracle_ok": bool(ok),
    }))
    return 0 if ok and same else 1


def spread_route(args):
    """the spread beside the counting ALL call of the same rows, same budget, same build; with --order NAME --split W the
    ordered spread beside the one ordered call"""
    import many_clause_sets as sets
    name = args.set or "linear20_all"
    ordered = args.order is not None
    source = sets
    if ordered:
        import many_walk_ordered as O
        if args.order not in O.ORDERS or args.split < 1:
            raise SystemExit(f"--order is one of {O.ORDERS}, --split at least 1")
        source = sets if name in sets.SETS else O
    if name not in source.SETS:
        raise SystemExit(f"--spread: --set is one of {sorted(source.SETS)}")
    text, base, objective, budget = source.build(name)
    own = args.spread_objective == "own"
    if own and objective not in ("MIN", "MAX"):
        raise SystemExit(f"--spread-objective own: {name} is walked under {objective}, not MIN / MAX")
    objective = objective if own else "ALL"
    budget = args.budget or budget
    budgets = tuple(int(b) for b in args.spread.split(","))
    roots = np.tile(np.array(base), (-(-args.count // len(base)), 1, 1))[:args.count]
    count = len(roots)
    model = solve_root(text)
    dev = torch.from_numpy(roots).cuda()
    fields = ("status", "root_props", "nodes", "cuts", "props", "solutions", "first")
    walk = dict(order=args.order, split_width=args.split) if ordered else {}
    solve = model.solve_many_clauses_ordered if ordered else model.solve_many_clauses
    make_pool = (lambda capacity: model.many_clause_ordered_checkpoints(capacity, args.split)) if ordered else \
        model.many_clause_checkpoints
    if ordered:
        fields += ("halvings",)
    slot_bytes = model.clause_ordered_checkpoint_bytes(args.split) if ordered else model.clause_checkpoint_bytes()
    per_pool = max(1, min(max(count, args.spread_rows), (1 << 30) // slot_bytes))  # a slot per row, 1 GiB at the most
    pools = (make_pool(per_pool), make_pool(per_pool))  # kept: a caller that repeats the call

    def timed(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    calls = {"all": lambda: solve(dev, objective, max_nodes=budget, **walk),
             "spread": lambda: model.solve_many_clauses_spread(dev, objective, budgets=budgets, max_rows=args.spread_rows,
                                                               pools=pools, **walk)}
    for call in calls.values():  # warm-up: code load, workspace, the allocator's blocks
        timed(call)
        timed(call)
    times, outs = {k: [] for k in calls}, {}
    for _ in range(args.reps):  # interleaved: a drift of the machine falls on both alike
        for k, call in calls.items():
            dt, outs[k] = timed(call)
            times[k].append(dt)
    one, got = outs["all"], outs["spread"]
    # where the time of the spread goes: the launch of round 0 alone
    first_ms = statistics.median(timed(lambda: solve(dev, objective, max_nodes=budgets[0], checkpoints=pools[0].reset(),
                                                     **walk))[0] for _ in range(3)) * 1e3
    done = one["status"] == 0  # (an instance the one call leaves at LIMIT has no whole record to compare with)
    if own:  # the optimum and DONE are promised, the walk that was made is another
        fields = ("status", "best")
    differing = {f: int((got[f] != one[f])[done].reshape(int(done.sum()), -1).any(dim=1).sum()) for f in fields}
    same = not any(differing.values())
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "tool": "time_solve_many_clauses", "route": "spread", "commit": commit(), "command": " ".join(sys.argv), "set": name,
        "objective": objective, "spread_nodes": int(got["nodes"].sum()),
        **({"order": args.order, "split_width": args.split, "halvings": int(one["halvings"].sum()),
            "spread_halvings": int(got["halvings"].sum()), "order_from_kernel": model.many_clauses_order_from_kernel()}
           if ordered else {}),
        "instances": count, "max_nodes_of_the_one_call": budget, "n_vars": model.n_vars, "clauses": model.n_clauses,
        "kernel": model.many_clauses_order_kernel() if ordered else model.many_clauses_kernel(),
        "resume_kernel": model.many_clauses_order_resume_kernel() if ordered else model.many_clauses_resume_kernel(),
        "waves": model.many_clauses_waves(count), "slot_bytes": slot_bytes, "budgets": list(budgets), "max_rows": args.spread_rows,
        "all_ms": spread(times["all"]), "spread_ms": spread(times["spread"]),
        "all_over_spread": round(med["all"] / med["spread"], 3),
        "all_status_counts": torch.bincount(one["status"].long(), minlength=3).tolist(),
        "spread_status_counts": torch.bincount(got["status"].long(), minlength=3).tolist(),
        "nodes": int(one["nodes"].sum()), "largest_tree": int(one["nodes"].max()), "solutions": int(one["solutions"].sum()),
        "rounds": got["rounds"], "sub_instances": got["sub_instances"], "rows_per_round": got["round_rows"],
        "round_0_ms": round(first_ms, 3),
        "instances_that_differ_where_the_one_call_is_done": differing,
        "every_field_equals_the_one_call_where_it_is_done": same,
    }))
    return 0 if same else 1


def upto_route(args, model, text, roots, dev, budget, upto, rng):
    """the up-to-K call beside the ANY and the ALL call of the same rows, same budget, same build"""
    import many_walk_clauses_upto as U
    count = len(roots)

    def under(objective):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = model.solve_many_clauses(dev, objective, max_nodes=budget)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    for _ in range(2):  # warm-up: code load, workspace
        under("ANY"), upto(), under("ALL")
    times = {"any": [], "upto": [], "all": []}
    for _ in range(args.reps):
        dt, first = under("ANY")
        times["any"].append(dt)
        dt, out = upto()
        times["upto"].append(dt)
        dt, every = under("ALL")
        times["all"].append(dt)
    host, first, every = ({k: v.cpu().numpy() for k, v in o.items() if torch.is_tensor(v)} for o in (out, first, every))
    picks = rng.choice(count, size=min(args.check, count), replace=False)
    want = U.walk_many_upto(text, roots[picks], args.upto, budget)
    ok = all((host[f][picks] == want[f]).all() for f in U.FIELDS) and bool((host["rows"][picks] == want["rows"]).all())
    med = {k: statistics.median(v) for k, v in times.items()}
    found = np.minimum(host["solutions"], 2)
    print(json.dumps({
        "tool": "time_solve_many_clauses", "route": "upto", "commit": commit(), "command": " ".join(sys.argv), "set": args.set,
        "instances": count, "max_nodes": budget, "max_solutions": args.upto, "n_vars": model.n_vars, "clauses": model.n_clauses,
        "kernel": model.many_clauses_kernel(), "upto_kernel": model.many_clauses_upto_kernel(),
        "waves": model.many_clauses_waves(count),
        "any_ms": spread(times["any"]), "upto_ms": spread(times["upto"]), "all_ms": spread(times["all"]),
        "upto_over_any": round(med["upto"] / med["any"], 3), "all_over_upto": round(med["all"] / med["upto"], 3),
        "any_nodes": int(first["nodes"].sum()), "upto_nodes": int(host["nodes"].sum()), "all_nodes": int(every["nodes"].sum()),
        "any_status_counts": np.bincount(first["status"], minlength=3).tolist(),
        "upto_status_counts": np.bincount(host["status"], minlength=3).tolist(),
        "all_status_counts": np.bincount(every["status"], minlength=3).tolist(),
        "upto_largest_tree": int(host["nodes"].max()), "all_largest_tree": int(every["nodes"].max()),
        "upto_solutions": int(host["solutions"].sum()), "all_solutions": int(every["solutions"].sum()),
        "done_with_0_1_2_or_more_solutions": np.bincount(found[host["status"] == 0], minlength=3).tolist(),
        "upto_instances_per_s": round(count / med["upto"]),
        "oracle_checked": len(picks), "oracle_ok": bool(ok),
    }))
    return 0 if ok else 1


def sliced_route(args, model, text, roots, dev, objective, budget, budgets, many, rng, W):
    count = len(roots)
    pool = model.many_clause_checkpoints(count)
    upto = {} if args.upto is None else {"max_solutions": args.upto}

    def first_slice():
        pool.reset()
        torch.cuda.synchronize()
        t = time.perf_counter()
        if args.upto is not None:
            out = model.solve_many_clauses_upto(dev, args.upto, max_nodes=budgets[0], checkpoints=pool)
        else:
            out = model.solve_many_clauses(dev, objective, max_nodes=budgets[0], checkpoints=pool)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def sliced():
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = model.solve_many_clauses_sliced(dev, objective, budgets=budgets, finish=args.finish, checkpoints=pool, **upto)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    many()  # warm-up: code load, workspace, the engine's buffers
    first_slice()
    sliced()
    many_times, first_times, sliced_times = [], [], []
    for _ in range(args.reps):
        dt, one = many()
        many_times.append(dt)
        dt, part = first_slice()
        first_times.append(dt)
        stopped_first = int((part["status"] == 1).sum())
        dt, out = sliced()
        sliced_times.append(dt)
    host = {k: v.cpu().numpy() for k, v in out.items() if torch.is_tensor(v) and not k.startswith("_")}
    one = {k: v.cpu().numpy() for k, v in one.items() if torch.is_tensor(v)}

    picks = rng.choice(count, size=min(args.check, count), replace=False)
    if args.upto is not None:
        import many_walk_clauses_upto as U
        want = U.walk_many_upto(text, roots[picks], args.upto, sum(budgets))
        ok = all((host[f][picks] == want[f]).all() for f in U.FIELDS) and bool((host["rows"][picks] == want["rows"]).all())
    elif args.finish == "resume":
        want = W.walk_many(text, roots[picks], objective, sum(budgets))
        has = want["solutions"] > 0
        ok = all((host[f][picks] == want[f]).all() for f in W.FIELDS) and bool((host["first"][picks][has] == want["first"][has]).all())
        if objective in ("MIN", "MAX"):
            ok = ok and bool((host["best"][picks][has] == want["best"][has]).all())
    else:
        want = W.walk_many(text, roots[picks], objective, sum(budgets) + 32768)
        proven = (want["status"] == 0) & (want["solutions"] > 0)
        ok = bool((host["status"] == 0).all())
        if objective in ("MIN", "MAX"):
            ok = ok and bool((host["best"][picks][proven] == want["best"][proven]).all())
        else:
            ok = ok and bool((host["solutions"][picks][proven] == want["solutions"][proven]).all())
    t_many, t_sliced = statistics.median(many_times), statistics.median(sliced_times)
    print(json.dumps({
        "tool": "time_solve_many_clauses", "route": "sliced", "commit": commit(), "command": " ".join(sys.argv), "set": args.set,
        "objective": objective if args.upto is None else None, "max_solutions": args.upto,
        "instances": count, "n_vars": model.n_vars, "clauses": model.n_clauses,
        "kernel": model.many_clauses_kernel(), "resume_kernel": model.many_clauses_resume_kernel(),
        "upto_kernel": model.many_clauses_upto_kernel(),
        "waves": model.many_clauses_waves(count), "slot_bytes": model.clause_checkpoint_bytes(),
        "one_call_max_nodes": budget, "one_call_status_counts": np.bincount(one["status"], minlength=3).tolist(),
        "one_call_nodes": int(one["nodes"].sum()), "one_call_largest_tree": int(one["nodes"].max()),
        "one_call_ms": spread(many_times),
        "budgets": list(budgets), "finish": args.finish, "sliced": out["sliced"], "stopped_after_the_first_slice": stopped_first,
        "first_slice_ms": spread(first_times), "sliced_ms": spread(sliced_times),
        "sliced_status_counts": np.bincount(host["status"], minlength=3).tolist(), "sliced_nodes": int(host["nodes"].sum()),
        "sliced_over_one_call": round(t_sliced / t_many, 3),
        "oracle_checked": len(picks), "oracle_ok": bool(ok),
    }))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
