#!/usr/bin/env python3
"""K instances of one model through Model.solve_many, and the SAME instances through the per-instance loop that was the
only route before it: one Search, reset and seeded per instance (the instance's root fixpoint by kernel 7, put, run),
one after the other -- on a sample of the instances when all K would take minutes (the output says how many).

Prints one JSON line: instances/s and nodes/s of both routes, their ratio, the spread over the repetitions, the launch
time as a function of max_nodes (bulk against tail), and a seeded sample of the device's answers re-checked against the
oracle walk (tests/many_walk.py).

  python tools/time_solve_many.py --set sudoku9 [--count 65536] [--reps 5] [--loop-sample 256] [--check 32]
                                  [--sliced B0,B1,... [--finish resume|search]] [--upto K]
                                  [--restarts BASE [--seed S]] [--revealed R] [--stream ROWS]
                                  [--spread B0,B1,... [--spread-rows ROWS]] [--max-nodes N]
                                  [--branching allowed [--upto K] [--objective ANY|ALL]]
  --sliced: the same instances through Model.solve_many_sliced as well (a checkpointed call with budget B0, a resume
  with every following budget; --finish search: what is left after the last budget through one Search per instance):
  the time of the whole, the time until the answers of the first slice are there, and whether it found what the one
  call found.
  --upto K: Model.solve_many_upto (an instance stops at its K-th solution, all K rows kept) on the same instances beside
  the ANY and the ALL call of solve_many, all three in this process after a warm-up, same budget: medians and ranges of
  --reps, what each call decided, the share of instances a k = 2 call classifies as unique / several / none / undecided,
  and the sampled answers (fields and rows) re-checked against the host walk of tests/many_walk_upto.py.
  --restarts BASE: Model.solve_many_restarts (Luby restarts x BASE failures, seeded value order, seed --seed) beside the
  ANY call of solve_many on the same instances, both in this process after a warm-up, interleaved, same budget: medians
  and ranges of --reps, sum and largest `nodes` of both calls, the share of instances that restarted, and --check sampled
  answers re-checked against the host walk of tests/many_walk_restarts.py.
  --revealed R: the sudoku sets with this share of givens for every instance instead of the set's own (the deep tails
  of 9x9 sudokus are at 0.30 and 0.25).
  --stream ROWS: Model.solve_many_stream (ALL, every solution appended to one shared stream) beside the counting ALL call
  of solve_many on the same instances, in this process after a warm-up, interleaved, same budget: (a) the ALL call, (b)
  one stream call with room for every solution, (c) the loop call / take / zero with a stream of ROWS rows, which fills
  (the output says how many calls it took); medians and ranges of --reps, whether every record of (b) and (c) equals (a)'s
  and every solution arrived, and --check sampled instances' rows re-checked against the host walk of tests/many_walk.py.
  --spread B0,B1,...: Model.solve_many_spread (ALL; the stopped instances of a round fanned out over the waves of the next,
  budget B0 for round 0, B1 for round 1, the last one repeated; --spread-rows: its max_rows) beside the counting ALL call of
  solve_many on the same instances, in this process after a warm-up, interleaved, two pools kept over the calls: medians and
  ranges of --reps, rounds and rows per round, the launch of round 0 alone, and whether every field of every instance and
  every first solution equals the one call's.
  --branching allowed: ONLY this comparison -- Model.solve_many(..., branching="allowed") (the open variable with the fewest
  values no valued neighbour forbids, only those values) beside the width call of the same build on the same rows, in this
  process after a warm-up, interleaved, same budget; with --upto K both through solve_many_upto.  For both rules: nodes
  total, the deepest instance, ms per call (median and range of --reps) and ns per node; the ratios allowed / width; whether
  both found the same `solutions` where neither stopped at the budget; --check sampled answers of the allowed call re-checked
  against the host walk of tests/many_walk_allowed.py.  --objective: instead of the set's own.
  --branching allowed with --sliced B1,B2,... and / or --spread B0,B1: instead of that comparison, the allowed walk in slices
  (Model.solve_many_sliced(branching="allowed"), with --upto K its up-to-k slices) beside the one allowed call with the budget
  --max-nodes, and the allowed spread (Model.solve_many_spread(branching="allowed")) beside the one allowed ALL call and the
  width spread with the same budgets on the same rows: interleaved after a warm-up, medians and ranges of --reps, nodes in
  total, rounds and rows, and whether every field equals the one allowed call's.
  sets: sudoku9 (9x9, revealed 0.35-0.45, ANY), queens12 / queens13 (two queens placed at random, ALL), sudoku16 (16x16, 0.6, ANY),
  sparse40 (a sparse != network of 40 variables, 16-bit table, three of them open: nearly every node is a solution, ALL)
"""
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

from csolve_amd import problems  # noqa: E402
from csolve_amd.solver import Search, solve_root  # noqa: E402


def instances(which, count, revealed=None):
    if revealed is not None:
        if which not in ("sudoku9", "sudoku16"):
            raise SystemExit("--revealed applies to the sudoku sets")
        text, rows = problems.sudoku_roots(3 if which == "sudoku9" else 4, revealed, list(range(1, count + 1)))
        return text, rows, "ANY", 1 << 18
    if which == "sudoku9":
        parts, per = [], -(-count // 11)
        for i in range(11):  # revealed 0.35, 0.36, ... 0.45
            text, rows = problems.sudoku_roots(3, 0.35 + 0.01 * i, list(range(1 + i * per, 1 + (i + 1) * per)))
            parts.append(rows)
        return text, np.concatenate(parts)[:count], "ANY", 1 << 16
    if which == "sudoku16":
        text, rows = problems.sudoku_roots(4, 0.6, list(range(1, count + 1)))
        return text, rows, "ANY", 1 << 16
    if which == "queens12":
        import many_sets
        return problems.queens(12, "ALL"), many_sets.queens_two(12, count, 7), "ALL", 1 << 20
    if which == "queens13":
        import many_sets
        return problems.queens(13, "ALL"), many_sets.queens_two(13, count, 7), "ALL", 1 << 22
    if which == "sparse40":
        import many_sets
        text = many_sets._sparse16(40, 3)
        return text, many_sets.narrowed(text, count, 3, 2, 8), "ALL", 1 << 20
    raise SystemExit(f"no set {which}")


def both_rules(args, model, text, roots, dev, objective, budget, count):
    """--branching allowed: the width call and the allowed call on the same rows, interleaved -> the JSON record"""
    import many_walk_allowed

    def call(rule):
        torch.cuda.synchronize()
        t = time.perf_counter()
        if args.upto is None:
            out = model.solve_many(dev, objective, max_nodes=budget, branching=rule)
        else:
            out = model.solve_many_upto(dev, args.upto, max_nodes=budget, branching=rule)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    rules = ("width", "allowed")
    for rule in rules:  # warm-up: code load, workspace, the allocator's blocks
        call(rule)
        call(rule)
    series, outs = {rule: [] for rule in rules}, {}
    for _ in range(args.reps):
        for rule in rules:
            dt, outs[rule] = call(rule)
            series[rule].append(dt)
    rec = {"what": "solve_many, branching width against allowed", "set": args.set, "revealed": args.revealed, "instances": count,
           "objective": objective if args.upto is None else f"up to {args.upto}", "max_nodes": budget, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "commit": commit(), "waves": model.many_waves(count),
           "kernels": {"width": model.many_kernel() if args.upto is None else model.many_upto_kernel(),
                       "allowed": model.many_allowed_kernel() if args.upto is None else model.many_allowed_upto_kernel()}}
    for rule in rules:
        out, ts = outs[rule], series[rule]
        nodes = int(out["nodes"].sum())
        rec[rule] = {"nodes": nodes, "deepest": int(out["nodes"].max()), "solutions": int(out["solutions"].sum()),
                     "status": torch.bincount(out["status"].long(), minlength=3).tolist(),
                     "ms": {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3),
                            "max": round(max(ts) * 1e3, 3)},
                     "ns_per_node": round(statistics.median(ts) * 1e9 / max(nodes, 1), 2)}
    w, a = rec["width"], rec["allowed"]
    rec["allowed_over_width"] = {"nodes": round(a["nodes"] / max(w["nodes"], 1), 4), "deepest": round(a["deepest"] / max(w["deepest"], 1), 4),
                                 "ms": round(a["ms"]["median"] / w["ms"]["median"], 4),
                                 "ns_per_node": round(a["ns_per_node"] / w["ns_per_node"], 4)}
    done = (outs["width"]["status"] == 0) & (outs["allowed"]["status"] == 0)
    rec["same_solutions_where_both_finished"] = bool((outs["width"]["solutions"] == outs["allowed"]["solutions"])[done].all())
    rec["both_finished"] = int(done.sum())
    rng = np.random.default_rng(args.seed)
    sample = sorted(rng.choice(count, size=min(args.check, count), replace=False).tolist())
    got = {f: outs["allowed"][f].cpu().numpy() for f in many_walk_allowed.FIELDS}
    good = 0
    for i in sample:
        if args.upto is None:
            want = many_walk_allowed.dive(text, roots[i], objective, budget)
        else:
            want = many_walk_allowed.upto(text, roots[i], args.upto, budget)
        good += all(int(got[f][i]) == want[f] for f in many_walk_allowed.FIELDS)
    rec["checked_against_the_host_walk"] = {"instances": len(sample), "equal": good}
    return rec


def allowed_slices_and_spread(args, model, dev, objective, budget, count):
    """--branching allowed with --sliced / --spread -> the JSON record"""
    def timed(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def measure(variants):
        for call in variants.values():  # warm-up: code load, workspace, pools, the allocator's blocks
            timed(call)
            timed(call)
        series, outs = {name: [] for name in variants}, {}
        for _ in range(args.reps):
            for name, call in variants.items():
                dt, outs[name] = timed(call)
                series[name].append(dt)
        ms = {name: {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3), "max": round(max(ts) * 1e3, 3)}
              for name, ts in series.items()}
        return ms, outs

    def equal(a, b, fields):
        return all(bool((a[f] == b[f]).all()) for f in fields)

    fields = ("status", "root_props", "nodes", "cuts", "props", "solutions")
    rec = {"what": "solve_many, the allowed walk in slices and spread", "set": args.set, "revealed": args.revealed, "instances": count,
           "max_nodes": budget, "reps": args.reps, "device": torch.cuda.get_device_name(0), "commit": commit(),
           "waves": model.many_waves(count), "kernels": {"resume": model.many_allowed_resume_kernel(),
                                                         "upto_resume": model.many_allowed_upto_resume_kernel()}}
    if args.spread:
        budgets = tuple(int(b) for b in args.spread.split(","))
        slot = max(model.checkpoint_bytes(), 1)
        pools = {rule: tuple(model.many_checkpoints(max(1, min(max(count, args.spread_rows), (1 << 30) // slot))) for _ in range(2))
                 for rule in ("allowed", "width")}
        ms, outs = measure({
            "one_allowed_call": lambda: model.solve_many(dev, "ALL", max_nodes=budget, branching="allowed"),
            "allowed_spread": lambda: model.solve_many_spread(dev, budgets=budgets, max_rows=args.spread_rows, pools=pools["allowed"],
                                                              branching="allowed"),
            "one_width_call": lambda: model.solve_many(dev, "ALL", max_nodes=budget),
            "width_spread": lambda: model.solve_many_spread(dev, budgets=budgets, max_rows=args.spread_rows, pools=pools["width"])})
        rec["spread"] = {"budgets": list(budgets), "ms": ms,
                         "nodes": {name: int(out["nodes"].sum()) for name, out in outs.items()},
                         "deepest": {name: int(outs[name]["nodes"].max()) for name in ("one_allowed_call", "one_width_call")},
                         "at_limit": {name: int((out["status"] == 1).sum()) for name, out in outs.items()},
                         "rounds": {name: outs[name]["rounds"] for name in ("allowed_spread", "width_spread")},
                         "round_rows": {name: outs[name]["round_rows"] for name in ("allowed_spread", "width_spread")},
                         "allowed_spread_equals_one_allowed_call": equal(outs["allowed_spread"], outs["one_allowed_call"], fields + ("first",)),
                         "width_spread_equals_one_width_call": equal(outs["width_spread"], outs["one_width_call"], fields + ("first",))}
    if args.sliced:
        budgets = tuple(int(b) for b in args.sliced.split(","))
        if args.upto is None:
            one = lambda: model.solve_many(dev, objective, max_nodes=budget, branching="allowed")  # noqa: E731
            cut = lambda: model.solve_many_sliced(dev, objective, budgets=budgets, branching="allowed")  # noqa: E731
            rows = "first"
        else:
            one = lambda: model.solve_many_upto(dev, args.upto, max_nodes=budget, branching="allowed")  # noqa: E731
            cut = lambda: model.solve_many_sliced(dev, budgets=budgets, max_solutions=args.upto, branching="allowed")  # noqa: E731
            rows = "rows"
        ms, outs = measure({"one_allowed_call": one, "allowed_sliced": cut})
        done = (outs["one_allowed_call"]["status"] != 1) & (outs["allowed_sliced"]["status"] != 1)
        rec["sliced"] = {"budgets": list(budgets), "objective": objective if args.upto is None else f"up to {args.upto}", "ms": ms,
                         "calls": outs["allowed_sliced"]["sliced"]["slices"],
                         "nodes": {name: int(out["nodes"].sum()) for name, out in outs.items()},
                         "deepest": int(outs["one_allowed_call"]["nodes"].max()),
                         "at_limit": {name: int((out["status"] == 1).sum()) for name, out in outs.items()},
                         "equal_where_both_finished": all(bool((outs["allowed_sliced"][f] == outs["one_allowed_call"][f])[done].all())
                                                          for f in fields + (rows,))}
    return rec


def commit():
    try:
        return open(os.path.join(ROOT, "csolve_amd", "csrc", "build", "COMMIT")).read().strip()
    except OSError:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="sudoku9")
    ap.add_argument("--count", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-sample", type=int, default=256)
    ap.add_argument("--check", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sliced", default=None, help="budgets of the slices, e.g. 256,4096")
    ap.add_argument("--finish", default="resume", choices=("resume", "search"))
    ap.add_argument("--upto", type=int, default=None, help="K: time solve_many_upto beside the ANY and the ALL call")
    ap.add_argument("--restarts", type=int, default=None, help="BASE: time solve_many_restarts beside the ANY call")
    ap.add_argument("--revealed", type=float, default=None, help="share of givens of every sudoku (default: the set's own)")
    ap.add_argument("--stream", type=int, default=None, help="ROWS: time solve_many_stream beside the counting ALL call")
    ap.add_argument("--spread", default=None, help="budgets of the rounds of solve_many_spread, e.g. 256,4096")
    ap.add_argument("--spread-rows", type=int, default=1 << 18, help="max_rows of solve_many_spread")
    ap.add_argument("--max-nodes", type=int, default=None, help="the budget of the one call (default: the set's own)")
    ap.add_argument("--branching", default="width", choices=("width", "allowed"),
                    help="allowed: time the allowed-values walk beside the width walk (with or without --upto K), nothing else")
    ap.add_argument("--objective", default=None, choices=("ANY", "ALL"), help="instead of the set's own (--branching allowed)")
    args = ap.parse_args()
    count = args.count or {"sudoku9": 65536, "queens12": 16384, "queens13": 48, "sudoku16": 4096, "sparse40": 256}[args.set]
    text, roots, objective, budget = instances(args.set, count, args.revealed)
    budget = args.max_nodes or budget
    model = solve_root(text)
    dev = torch.from_numpy(roots).cuda()
    if args.branching == "allowed" and (args.sliced or args.spread):
        print(json.dumps(allowed_slices_and_spread(args, model, dev, args.objective or objective, budget, count)))
        return
    if args.branching == "allowed":
        print(json.dumps(both_rules(args, model, text, roots, dev, args.objective or objective, budget, count)))
        return

    def many(max_nodes, rows=dev):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = model.solve_many(rows, objective, max_nodes=max_nodes)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    many(budget)  # warm-up: code load, workspace
    many(budget)
    times = []
    for _ in range(args.reps):
        dt, out = many(budget)
        times.append(dt)
    nodes = int(out["nodes"].sum())
    status = torch.bincount(out["status"].long(), minlength=3).tolist()
    t_many = statistics.median(times)
    # bulk against tail: the launch time under smaller budgets (instances beyond a budget stop there)
    per_budget = {}
    largest = int(out["nodes"].max())
    for b in sorted({16, 64, 256, 1024, 4096, max(1, largest)}):
        if b <= budget:
            per_budget[b] = round(statistics.median(many(b)[0] for _ in range(3)) * 1e3, 3)

    sliced = None
    if args.sliced:
        budgets = tuple(int(b) for b in args.sliced.split(","))

        def first_slice():
            pool = model.many_checkpoints(count)
            torch.cuda.synchronize()
            t = time.perf_counter()
            model.solve_many(dev, objective, max_nodes=budgets[0], checkpoints=pool)
            torch.cuda.synchronize()
            return time.perf_counter() - t

        def whole():
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = model.solve_many_sliced(dev, objective, budgets=budgets, finish=args.finish)
            torch.cuda.synchronize()
            return time.perf_counter() - t, res

        first_slice()
        whole()  # warm-up: the pool, the engine's buffers
        firsts = [first_slice() for _ in range(args.reps)]
        wholes = []
        for _ in range(args.reps):
            dt, res = whole()
            wholes.append(dt)
        left = res["status"] == 1
        found = bool(((res["solutions"] > 0) == (out["solutions"] > 0))[~left].all())
        same = all(bool((res[f] == out[f])[~left].all()) for f in ("nodes", "cuts", "props", "solutions"))
        sliced = {"budgets": list(budgets), "finish": args.finish, "calls": res["sliced"]["slices"],
                  "searched": res["sliced"]["searched"], "still_at_limit": int(left.sum()),
                  "ms": {"median": round(statistics.median(wholes) * 1e3, 3), "min": round(min(wholes) * 1e3, 3),
                         "max": round(max(wholes) * 1e3, 3), "reps": args.reps},
                  "first_slice_ms": {"median": round(statistics.median(firsts) * 1e3, 3), "min": round(min(firsts) * 1e3, 3),
                                     "max": round(max(firsts) * 1e3, 3)},
                  "finds_what_one_call_finds": found,
                  # finish=search: the engine's own walk below the checkpoints, so only finish=resume can say yes
                  "counters_equal_one_call": same, "kernel": model.many_resume_kernel(),
                  "slot_bytes": model.checkpoint_bytes()}

    rng = np.random.default_rng(args.seed)
    upto = None
    if args.upto is not None:
        import many_walk_upto

        def timed(call):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = call()
            torch.cuda.synchronize()
            return time.perf_counter() - t, res

        calls = {"any": lambda: model.solve_many(dev, "ANY", max_nodes=budget),
                 "all": lambda: model.solve_many(dev, "ALL", max_nodes=budget),
                 "upto": lambda: model.solve_many_upto(dev, args.upto, max_nodes=budget)}
        for call in calls.values():  # warm-up: code load, workspace, the allocator's blocks
            timed(call)
            timed(call)
        series = {name: [] for name in calls}
        answers = {}
        for _ in range(args.reps):  # interleaved: a drift of the machine falls on all three alike
            for name, call in calls.items():
                dt, answers[name] = timed(call)
                series[name].append(dt)

        def summary(name):
            ts, res = series[name], answers[name]
            return {"ms": {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3),
                           "max": round(max(ts) * 1e3, 3), "reps": args.reps},
                    "status_counts": torch.bincount(res["status"].long(), minlength=3).tolist(),
                    "nodes": int(res["nodes"].sum()), "largest_tree": int(res["nodes"].max()),
                    "solutions": int(res["solutions"].sum())}

        cls = model.classify_many(dev, max_nodes=budget)
        share = {name: int((cls == value).sum()) for name, value in (("none", 0), ("unique", 1), ("several", 2),
                                                                      ("limit", -1), ("bad_root", -2))}
        picks_u = rng.choice(count, size=min(args.check, count), replace=False)
        want_u = many_walk_upto.dive_many_upto(text, roots[picks_u], args.upto, budget)
        got_u = {k: v[torch.from_numpy(picks_u).cuda()].cpu().numpy() for k, v in answers["upto"].items() if torch.is_tensor(v)}
        upto_ok = all((got_u[f] == want_u[f]).all() for f in many_walk_upto.FIELDS) and bool((got_u["rows"] == want_u["rows"]).all())
        same_as_any = all(bool((answers["upto"][f] == answers["any"][f]).all()) for f in many_walk_upto.FIELDS)
        upto = {"k": args.upto, "kernel": model.many_upto_kernel(), "max_nodes": budget,
                "any": summary("any"), "all": summary("all"), "upto": summary("upto"),
                "classes_k2": share, "every_field_equals_any": same_as_any,
                "oracle_checked": len(picks_u), "oracle_ok": bool(upto_ok)}

    restarts = None
    if args.restarts is not None:
        import many_walk_restarts

        def timed_r(call):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = call()
            torch.cuda.synchronize()
            return time.perf_counter() - t, res

        calls_r = {"any": lambda: model.solve_many(dev, "ANY", max_nodes=budget),
                   "restarts": lambda: model.solve_many_restarts(dev, max_nodes=budget, restart_base=args.restarts,
                                                                 seed=args.seed)}
        for call in calls_r.values():  # warm-up: code load, workspace, the allocator's blocks
            timed_r(call)
            timed_r(call)
        series_r = {name: [] for name in calls_r}
        answers_r = {}
        for _ in range(args.reps):  # interleaved: a drift of the machine falls on both alike
            for name, call in calls_r.items():
                dt, answers_r[name] = timed_r(call)
                series_r[name].append(dt)

        def summary_r(name):
            ts, res = series_r[name], answers_r[name]
            return {"ms": {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3),
                           "max": round(max(ts) * 1e3, 3), "reps": args.reps},
                    "status_counts": torch.bincount(res["status"].long(), minlength=3).tolist(),
                    "nodes": int(res["nodes"].sum()), "largest_walk": int(res["nodes"].max()),
                    "solutions": int(res["solutions"].sum())}

        picks_r = rng.choice(count, size=min(args.check, count), replace=False)
        want_r = many_walk_restarts.dive_many_restarts(text, roots[picks_r], args.restarts, seed=args.seed, max_nodes=budget)
        got_r = {k: v[torch.from_numpy(picks_r).cuda()].cpu().numpy() for k, v in answers_r["restarts"].items() if torch.is_tensor(v)}
        has_r = want_r["solutions"] > 0
        restarts_ok = all((got_r[f] == want_r[f]).all() for f in many_walk_restarts.FIELDS + ("restarts",)) and \
            bool((got_r["first"][has_r] == want_r["first"][has_r]).all())
        both = (answers_r["any"]["status"] == 0) & (answers_r["restarts"]["status"] == 0)
        restarts = {"base": args.restarts, "seed": args.seed, "revealed": args.revealed, "kernel": model.many_restart_kernel(),
                    "max_nodes": budget, "any": summary_r("any"), "restarts": summary_r("restarts"),
                    "restarted_instances": int((answers_r["restarts"]["restarts"] > 0).sum()),
                    "restarted_share": round(float((answers_r["restarts"]["restarts"] > 0).float().mean()), 4),
                    "most_restarts": int(answers_r["restarts"]["restarts"].max()),
                    "same_verdict_where_both_done": bool((answers_r["any"]["solutions"] == answers_r["restarts"]["solutions"])[both].all()),
                    "oracle_checked": len(picks_r), "oracle_ok": bool(restarts_ok)}

    streamed = None
    if args.stream is not None:
        import many_walk as walk_s
        fields = ("status", "root_props", "nodes", "cuts", "props", "solutions")
        counted = model.solve_many(dev, "ALL", max_nodes=budget)
        total = int(counted["solutions"].sum())
        pool = model.many_checkpoints(count)
        roomy, small = model.many_stream(total + 1), model.many_stream(args.stream)

        def one_call():  # (b): room for everything
            pool.reset()
            roomy.count.zero_()
            return model.solve_many_stream(dev, roomy, pool, max_nodes=budget), 1, None

        def loop_s():  # (c): call, take the rows, zero the count, while an instance has work left
            pool.reset()
            slots = results = None
            calls, kept = 0, []
            while True:
                ans = model.solve_many_stream(dev, small, pool, slots, results, max_nodes=budget)
                slots, results = ans["_slots"], ans["_records"]
                calls += 1
                kept.append(small.take())
                if not bool((ans["slot"] != -1).any()):
                    return ans, calls, kept

        def timed_s(call):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = call()
            torch.cuda.synchronize()
            return time.perf_counter() - t, res

        calls_s = {"all": lambda: (model.solve_many(dev, "ALL", max_nodes=budget), 1, None), "stream_roomy": one_call,
                   "stream_loop": loop_s}
        for call in calls_s.values():  # warm-up: code load, workspace, the allocator's blocks
            timed_s(call)
            timed_s(call)
        series_s = {name: [] for name in calls_s}
        answers_s = {}
        for _ in range(args.reps):  # interleaved: a drift of the machine falls on all three alike
            for name, call in calls_s.items():
                dt, answers_s[name] = timed_s(call)
                series_s[name].append(dt)

        def summary_s(name):
            ts, (res, calls, _) = series_s[name], answers_s[name]
            return {"ms": {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3),
                           "max": round(max(ts) * 1e3, 3), "reps": args.reps}, "calls": calls,
                    "records_equal_all": all(bool((res[f] == counted[f]).all()) for f in fields)}

        # the rows of sampled instances, from the roomy call and from the loop, against the host walk
        picks_s = rng.choice(count, size=min(args.check, count), replace=False)
        n_roomy = int(roomy.count.item())
        owner_b, rows_b = roomy.owner[:n_roomy].cpu().numpy(), roomy.rows[:n_roomy].cpu().numpy()
        owner_c = torch.cat([o for o, _ in answers_s["stream_loop"][2]]).cpu().numpy()
        rows_c = torch.cat([r for _, r in answers_s["stream_loop"][2]]).cpu().numpy()
        rows_ok = n_roomy == total and len(owner_c) == total
        for i in picks_s:
            want_rows = walk_s.Walk(text, roots[i]).run(budget, None)["rows"]
            for owner, rows in ((owner_b, rows_b), (owner_c, rows_c)):
                mine = rows[owner == i]
                rows_ok = rows_ok and len(mine) == len(want_rows) and all((a == b).all() for a, b in zip(mine, want_rows))
        streamed = {"rows": args.stream, "kernel": model.many_stream_kernel(), "max_nodes": budget, "solutions": total,
                    "nodes": int(counted["nodes"].sum()), "largest_tree": int(counted["nodes"].max()),
                    "most_solutions_of_an_instance": int(counted["solutions"].max()),
                    "all": summary_s("all"), "stream_roomy": summary_s("stream_roomy"), "stream_loop": summary_s("stream_loop"),
                    "oracle_checked": len(picks_s), "oracle_ok": bool(rows_ok)}

    spread = None
    if args.spread:
        fields_p = ("status", "root_props", "nodes", "cuts", "props", "solutions", "first")
        budgets_p = tuple(int(b) for b in args.spread.split(","))
        slot_bytes = model.checkpoint_bytes()
        per_pool = max(1, min(max(count, args.spread_rows), (1 << 30) // slot_bytes))  # a slot per row, 1 GiB at the most
        pools_p = (model.many_checkpoints(per_pool), model.many_checkpoints(per_pool))  # kept: a caller that repeats the call

        def timed_p(call):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = call()
            torch.cuda.synchronize()
            return time.perf_counter() - t, res

        calls_p = {"all": lambda: model.solve_many(dev, "ALL", max_nodes=budget),
                   "spread": lambda: model.solve_many_spread(dev, budgets=budgets_p, max_rows=args.spread_rows, pools=pools_p)}
        for call in calls_p.values():  # warm-up: code load, workspace, the allocator's blocks
            timed_p(call)
            timed_p(call)
        series_p = {name: [] for name in calls_p}
        answers_p = {}
        for _ in range(args.reps):  # interleaved: a drift of the machine falls on both alike
            for name, call in calls_p.items():
                dt, answers_p[name] = timed_p(call)
                series_p[name].append(dt)
        one, res_p = answers_p["all"], answers_p["spread"]

        def ms_p(name):
            ts = series_p[name]
            return {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3), "max": round(max(ts) * 1e3, 3),
                    "reps": args.reps}

        # where the time of the spread goes: the launch of round 0 alone, and the largest tree below a row of the last round
        first_ms = statistics.median(timed_p(lambda: model.solve_many(dev, "ALL", max_nodes=budgets_p[0],
                                                                      checkpoints=pools_p[0].reset()))[0] for _ in range(3)) * 1e3
        spread = {"budgets": list(budgets_p), "max_rows": args.spread_rows, "max_nodes_of_the_one_call": budget,
                  "all_ms": ms_p("all"), "spread_ms": ms_p("spread"),
                  "all_status_counts": torch.bincount(one["status"].long(), minlength=3).tolist(),
                  "spread_status_counts": torch.bincount(res_p["status"].long(), minlength=3).tolist(),
                  "nodes": int(one["nodes"].sum()), "largest_tree": int(one["nodes"].max()), "solutions": int(one["solutions"].sum()),
                  "rounds": res_p["rounds"], "sub_instances": res_p["sub_instances"], "rows_per_round": res_p["round_rows"],
                  "round_0_ms": round(first_ms, 3), "slot_bytes": slot_bytes,
                  # (an instance the one call leaves at LIMIT has no whole record to compare with)
                  "every_field_equals_the_one_call_where_it_is_done":
                      all(bool((res_p[f] == one[f])[one["status"] == 0].all()) for f in fields_p)}

    # the per-instance loop: one Search, reset and seeded per instance
    sample =np.sort(rng.choice(count, size=min(args.loop_sample, count), replace=False))
    search = Search(model, 1 << 18, 1 << 14)
    node = torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32, device="cuda")

    def loop():
        total = 0
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in sample:
            state, res = model.propagate(dev[i:i + 1], node)
            st = int(res[0, 0])
            if st <= 0:  # inconsistent, or solved by the root node
                continue
            search.reset()
            search.put(state)
            total += search.run()["nodes"]
        torch.cuda.synchronize()
        return time.perf_counter() - t, total

    loop()  # warm-up
    loop_times = []
    for _ in range(max(2, args.reps // 2)):
        dt, loop_nodes = loop()
        loop_times.append(dt)
    t_loop = statistics.median(loop_times)

    # a seeded sample of the answers against the oracle walk
    import many_walk
    picks = rng.choice(count, size=min(args.check, count), replace=False)
    want = many_walk.dive_many(text, roots[picks], objective, budget)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    checked_ok = all((host[f][picks] == want[f]).all() for f in ("status", "root_props", "nodes", "cuts", "props", "solutions"))
    has = want["solutions"] > 0
    checked_ok = bool(checked_ok and (host["first"][picks][has] == want["first"][has]).all())

    many_rate, loop_rate = count / t_many, len(sample) / t_loop
    print(json.dumps({
        "tool": "time_solve_many", "commit": commit(), "command": " ".join(sys.argv), "set": args.set, "objective": objective,
        "instances": count, "max_nodes": budget, "status_counts": status, "nodes": nodes, "largest_tree": largest,
        "waves": model.many_waves(count), "kernel": model.many_kernel(),
        "solve_many_ms": {"median": round(t_many * 1e3, 3), "min": round(min(times) * 1e3, 3), "max": round(max(times) * 1e3, 3),
                          "reps": args.reps},
        "solve_many_instances_per_s": round(many_rate), "solve_many_nodes_per_s": round(nodes / t_many),
        "launch_ms_by_max_nodes": per_budget,
        "loop_instances": len(sample), "loop_nodes": loop_nodes,
        "loop_s": {"median": round(t_loop, 4), "min": round(min(loop_times), 4), "max": round(max(loop_times), 4),
                   "reps": len(loop_times)},
        "loop_instances_per_s": round(loop_rate), "loop_nodes_per_s": round(loop_nodes / t_loop),
        "ratio_instances_per_s": round(many_rate / loop_rate, 1),
        "oracle_checked": len(picks), "oracle_ok": checked_ok,
        **({"sliced": sliced} if sliced else {}),
        **({"upto": upto} if upto else {}),
        **({"restarts": restarts} if restarts else {}),
        **({"stream": streamed} if streamed else {}),
        **({"spread": spread} if spread else {}),
    }))
    return 0 if checked_ok and (upto is None or upto["oracle_ok"]) and (restarts is None or restarts["oracle_ok"]) and \
        (streamed is None or streamed["oracle_ok"]) else 1


if __name__ == "__main__":
    sys.exit(main())
