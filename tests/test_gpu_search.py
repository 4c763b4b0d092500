"""GPU tests of the device-resident search engine: solution counts, optima and solution
validity against the goldens of the compiled reference (tests/golden/solve_stats.json) and
the oracle."""
import json
import os

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _solve(text, pool=1 << 18, children=1 << 14, iters=1 << 40):
    from csolve_amd.solver import Search, solve_root
    model = solve_root(text)
    s = Search(model, pool, children)
    s.put(model.root_state())
    st = s.run(iters)
    return model, s, st


@pytest.mark.parametrize("n,count", [(4, 2), (6, 4), (8, 92), (10, 724), (12, 14200)])
def test_all_solutions_of_queens(n, count):
    """queens-8/10/12 ALL: 92 / 724 / 14,200 solutions (the reference's own counts)."""
    from csolve_amd import problems
    model, s, st = _solve(problems.queens(n, "ALL"))
    assert st["done"] == 1 and st["pool"] == 0
    assert st["solutions"] == count
    assert st["nodes"] - st["cuts"] >= st["solutions"]
    sols = s.solutions(1024)
    assert len(sols) == min(count, 1024)
    # every stored solution is a valid placement
    for row in sols[:200]:
        assert len(set(row)) == n and len(set(row + np.arange(n))) == n and len(set(row - np.arange(n))) == n


@pytest.mark.parametrize("n", [16, 64, 128])
def test_any_stops_at_first_solution(n):
    """ANY: depth-first enough (64 open states expanded per iteration) to reach a first solution of
    queens-64 and queens-128 (BASELINE configs[3] instance) with a small pool; the solution is valid."""
    from csolve_amd import problems
    model, s, st = _solve(problems.queens(n), pool=1 << 20, children=1 << 16, iters=5000)
    assert st["done"] == 1 and st["solutions"] >= 1
    row = s.solutions(1)[0]
    assert len(set(row)) == n and len(set(row + np.arange(n))) == n and len(set(row - np.arange(n))) == n
    truth = model.eval_root(torch.from_numpy(np.stack([row, row], 1)[None].astype(np.int32)).cuda())
    assert int(truth[0]) == 1


@pytest.mark.parametrize("name,best", [("ref_schedule", 11), ("schedule6_s1", 22), ("ref_wcet", 1560)])
def test_optimisation_reaches_the_reference_optimum(name, best):
    """MIN / MAX with the incumbent bound pushed into every batch: examples/schedule.txt -> 11,
    schedule-6 -> 22, examples/wcet.txt -> 1560 (reference goldens)."""
    model, s, st = _solve(open(golden("problems", name + ".txt")).read(), pool=1 << 20, children=1 << 16)
    assert st["done"] == 1
    assert st["best"] == best
    assert st["solutions"] >= 1
    # the kept solution attains the optimum and satisfies every constraint
    row = s.best_solution()
    assert row is not None and row[model.objective_var] == best
    truth = model.eval_root(torch.from_numpy(np.stack([row, row], 1)[None].astype(np.int32)).cuda())
    assert int(truth[0]) == 1


def test_schedule_12_reaches_the_optimum_the_reference_needs_six_minutes_for():
    """BASELINE configs[4] shape (schedule.txt-style MIN, seeded): the largest instance of the generator the compiled
    reference finishes -- 12 tasks, 233,056,571 calls, 351 s, optimum 45 (tests/golden/solve_stats.json; 14 and 16
    tasks do not finish within 25 minutes each) -- is solved to the same optimum by the device engine, search
    exhausted, with a solution that attains it and satisfies every constraint."""
    want = next(r for r in json.load(open(golden("solve_stats.json"))) if r["problem"] == "schedule12_s1")
    assert want["best"] == 45 and want["calls"] == 233056571
    model, s, st = _solve(open(golden("problems", "schedule12_s1.txt")).read(), pool=1 << 22, children=1 << 16)
    assert st["done"] == 1 and st["best"] == want["best"]
    row = s.best_solution()
    assert row is not None and row[model.objective_var] == want["best"]
    truth = model.eval_root(torch.from_numpy(np.stack([row, row], 1)[None].astype(np.int32)).cuda())
    assert int(truth[0]) == 1
    names = model.var_names()
    mine = {names[i]: int(row[i]) for i in range(len(names))}
    assert mine["end"] == want["last_solution"]["end"] == 45


def test_schedule_16_incumbents_are_feasible_schedules():
    """schedule-16 MIN (the size BASELINE configs[4] names) is beyond the compiled reference (no result in 25 minutes)
    and would take the engine hours to exhaust; what can be checked is that a bounded run produces incumbents that
    are feasible schedules: every constraint true under the oracle-independent device evaluation AND under the
    oracle, the objective equal to the reported bound"""
    from csolve_amd import problems
    from oracle.cs_oracle import Model as OModel, Oracle
    text = problems.schedule(16, 1)
    model, s, st = _solve(text, pool=1 << 22, children=1 << 16, iters=3000)
    assert st["solutions"] >= 1 and st["best"] < 2**31 - 1
    row = s.best_solution()
    assert row is not None and row[model.objective_var] == st["best"]
    om = OModel.parse(text)
    om.set_domains(np.stack([row, row], 1).astype(np.int32))
    om.index()
    assert Oracle(om).eval(om.root) == (1, 1)
    more = s.run(3000)
    assert more["best"] <= st["best"]


@pytest.mark.parametrize("which", ["queens7", "offsets6x5", "offsets5x9", "offsets40x8", "offsets64x8", "sudoku9", "sudoku16"])
def test_search_counters_match_oracle_tree_on_all(which):
    """For ALL the set of explored nodes does not depend on the walking order as long as the
    branching variable of a state is a function of the state: compare CALLS/CUTS/solutions with a
    plain CPU walk of the same tree that uses the oracle for every child (the engine counts the children
    that a parent's own forbidden set rules out without launching them; the walk propagates every one)."""
    from csolve_amd import problems
    # the last four take cs_step_shave (one wave per parent: 40 and 64 variables in one register per lane, 81 in two,
    # 256 in four); the first three cs_step_packed
    text = {"queens7": lambda: problems.queens(7, "ALL"), "offsets6x5": lambda: problems.offsets(6, 5, 2, "ALL"),
            "offsets5x9": lambda: problems.offsets(5, 9, 4, "ALL"), "offsets40x8": lambda: problems.offsets(40, 8, 1, "ALL"),
            "offsets64x8": lambda: problems.offsets(64, 8, 1, "ALL"), "sudoku9": lambda: problems.sudoku(3, 0.35, 1, "ALL"),
            "sudoku16": lambda: problems.sudoku(4, 0.6, 3, "ALL")}[which]()
    model, s, st = _solve(text)
    calls, cuts, sols, props = oracle_all_tree(text, model.domains())
    assert (st["nodes"], st["cuts"], st["solutions"]) == (calls, cuts, sols)
    # the engine's propagations are those of the consistent children: on a != network the reference's PROPS
    assert st["props"] == props


def oracle_all_tree(text, root, max_calls=None):
    """The ALL tree below the root domains `root`, walked on the host with the oracle for every child and the
    engine's branching rule -> (nodes, cuts, solutions, props).  max_calls: give up (AssertionError) beyond it."""
    from oracle.cs_oracle import Model as OModel, Oracle
    om = OModel.parse(text)
    om.set_domains(root)
    om.index()
    orc = Oracle(om)
    calls = cuts = sols = props = 0
    stack = [root]
    while stack:
        state = stack.pop()
        width = (state[:, 1] - state[:, 0]).astype(np.int64)
        width[width == 0] = 1 << 40
        v = int(np.argmin(width))  # smallest open interval, ties -> lowest index (cs_branch)
        for val in range(state[v, 0], state[v, 1] + 1):
            calls += 1
            status, out = orc.instance(state, v, val, val)
            if status < 0:
                cuts += 1
                continue
            props += status
            if (out[:, 0] == out[:, 1]).all():
                sols += 1
            else:
                stack.append(out)
        assert max_calls is None or calls <= max_calls, f"ALL tree beyond {max_calls} nodes"
    return calls, cuts, sols, props


@pytest.mark.parametrize("which", ["queens11", "offsets40x8", "sudoku9", "sudoku9_30"])
def test_fused_levels_walk_the_tree_of_the_separate_kernels(which, monkeypatch):
    """ALL through the level kernels of cs_step.hip.h (one launch per frontier) and, with CSGPU_SEARCH_FUSED=0, through
    branch / emit / fixpoint / classify / scatter: the same nodes, cuts, solutions and propagations; stored solutions
    satisfy the root"""
    from csolve_amd import problems
    text = {"queens11": lambda: problems.queens(11, "ALL"), "offsets40x8": lambda: problems.offsets(40, 8, 1, "ALL"),
            "sudoku9": lambda: problems.sudoku(3, 0.35, 1, "ALL"), "sudoku9_30": lambda: problems.sudoku(3, 0.30, 3, "ALL")}[which]()
    runs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("CSGPU_SEARCH_FUSED", fused)
        model, s, st = _solve(text)
        assert st["done"] == 1 and st["pool"] == 0
        runs.append({k: st[k] for k in ("nodes", "cuts", "solutions", "props")})
        rows = s.solutions(32)
        assert len(rows) == min(32, st["solutions"])
        for row in rows:
            truth = model.eval_root(torch.from_numpy(np.stack([row, row], 1)[None].astype(np.int32)).cuda())
            assert int(truth[0]) == 1
    assert runs[0] == runs[1], runs


def test_take_and_put_move_subtrees_between_engines():
    """Work stealing primitive: states taken from one pool and put into another are explored
    there; the two engines together find every solution exactly once."""
    from csolve_amd import problems
    from csolve_amd.solver import Search, solve_root
    model = solve_root(problems.queens(9, "ALL"))
    a, b = Search(model, 1 << 16, 1 << 12), Search(model, 1 << 16, 1 << 12)
    a.put(model.root_state())
    a.run(3)
    stolen = a.take(10)
    assert 0 < stolen.shape[0] <= 10
    b.put(stolen.contiguous())
    sa, sb = a.run(), b.run()
    assert sa["done"] and sb["done"]
    assert sa["solutions"] + sb["solutions"] == 352


def test_search_is_reproducible():
    """Two runs of the same search expand the same nodes in the same order (pool rows are assigned
    from child indices, not from the order in which workgroups finish)."""
    from csolve_amd import problems
    runs = [_solve(problems.queens(40), pool=1 << 20, children=1 << 16, iters=400)[2] for _ in range(3)]
    assert runs[0]["solutions"] >= 1
    assert all(r == runs[0] for r in runs)


def test_command_line_front_prints_in_the_reference_format():
    """csolve_amd/csolve_gpu: reference input conventions, reference output line formats."""
    import os
    import re
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "csolve_amd", "csolve_gpu")
    p = subprocess.run([exe, golden("problems", "queens8_all.txt")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().split("\n")
    sols = [l for l in lines if l.startswith("#1: SOLUTION: ")]
    assert len(sols) == 92 and all(re.fullmatch(r"#1: SOLUTION: (X\d+ = \d+, ){8}BEST: 0", l) for l in sols)
    assert re.fullmatch(r"#1: CALLS: \d+, CUTS: \d+, PROPS: \d+, CONFL: 0, RESTARTS: \d+, LEVEL: .*SOLUTIONS: 92", lines[-1])
    p = subprocess.run([exe, golden("problems", "ref_schedule.txt")], capture_output=True, text=True, timeout=120)
    assert p.stdout.count("SOLUTION: ") == 1 and "end = 11, <obj> = 11, " in p.stdout and "BEST: 11" in p.stdout
    p = subprocess.run([exe, "-"], input="ANY; x = 1; x = 2;", capture_output=True, text=True, timeout=60)
    assert p.stdout.strip() == "INFEASIBLE PROBLEM"
    p = subprocess.run([exe, "-"], input="ANY; x = ;", capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "error: syntax error" in p.stderr and "in line 1" in p.stderr
    p = subprocess.run([exe, "-"], input="ANY; x != x; 0 <= x; x <= 3;", capture_output=True, text=True, timeout=60)
    assert "INFEASIBLE PROBLEM" in p.stdout or "NO SOLUTION FOUND" in p.stdout


@pytest.mark.parametrize("order", ["none", "smallest-domain", "largest-domain", "smallest-value", "largest-value"])
@pytest.mark.parametrize("prefer", [False, True])
def test_the_references_variable_orders_and_failure_counts(order, prefer):
    """-o / -f (strategy.c:79-121) in the engine: whatever the branching rule, ALL finds every solution, ANY a valid one,
    MIN the optimum; with the default rule set explicitly the tree is the default engine's"""
    from csolve_amd import problems
    from csolve_amd.solver import Search, solve_root
    model = solve_root(problems.queens(8, "ALL"))
    s = Search(model, 1 << 16, 1 << 12)
    s.set_strategy(order, prefer)
    s.put(model.root_state())
    st = s.run()
    assert st["done"] == 1 and st["solutions"] == 92
    if order == "smallest-domain" and not prefer:
        ref = Search(model, 1 << 16, 1 << 12)
        ref.put(model.root_state())
        rst = ref.run()
        assert (st["nodes"], st["cuts"], st["props"]) == (rst["nodes"], rst["cuts"], rst["props"])
    model = solve_root(problems.queens(24))
    s = Search(model, 1 << 18, 1 << 14)
    s.set_strategy(order, prefer)
    s.put(model.root_state())
    st = s.run(200000)
    assert st["done"] == 1 and st["solutions"] >= 1
    row = s.solutions(1)[0]
    assert len(set(row)) == 24 and len(set(row + np.arange(24))) == 24 and len(set(row - np.arange(24))) == 24
    model = solve_root(open(golden("problems", "schedule6_s1.txt")).read())
    s = Search(model, 1 << 18, 1 << 14)
    s.set_strategy(order, prefer)
    s.set_restart_on_improvement(True)
    s.put(model.root_state())
    st = s.run()
    assert st["done"] == 1 and st["best"] == 22 and st["restarts"] >= 1


def test_command_line_flags_of_the_reference(tmp_path):
    """csolve_gpu -o / -f / -r / -t / -c / -j (main.c:51-130): the same solutions and optimum under every flag set, a
    time limit ends an ALL run early"""
    import os
    import subprocess
    from conftest import ROOT
    from csolve_amd import problems
    exe = os.path.join(ROOT, "csolve_amd", "csolve_gpu")
    for flags in (["-o", "none", "-f", "true"], ["-o", "largest-domain", "-f", "false", "-c", "true", "-j", "4"],
                  ["-r", "0"], ["-o", "smallest-value", "-r", "100", "-t", "60"]):
        p = subprocess.run([exe] + flags + [golden("problems", "queens8_all.txt")], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.count("SOLUTION: ") == 92, (flags, p.stderr)
        p = subprocess.run([exe] + flags + [golden("problems", "ref_schedule.txt")], capture_output=True, text=True, timeout=120)
        assert p.stdout.count("SOLUTION: ") == 1 and "BEST: 11" in p.stdout, (flags, p.stdout[-300:])
    big = tmp_path / "q40all.txt"
    big.write_text(problems.queens(40, "ALL"))
    p = subprocess.run([exe, "-t", "1", str(big)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "CALLS:" in p.stdout
    p = subprocess.run([exe, "-o", "sideways", golden("problems", "queens8_all.txt")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "error: invalid order" in p.stderr


def test_reset_runs_the_same_search_again():
    from csolve_amd import problems
    from csolve_amd.solver import Search, solve_root
    model = solve_root(problems.queens(9, "ALL"))
    s = Search(model, 1 << 16, 1 << 12)
    runs = []
    for _ in range(2):
        s.reset()
        s.put(model.root_state())
        runs.append(s.run())
    assert runs[0]["solutions"] == 352 and runs[0] == runs[1]


def test_two_engines_share_the_incumbent():
    """Two engines on halves of a MIN search that tell each other their incumbents after every slice
    (what ShardedSearch does across ranks; set_best must not lose an incumbent the engine has found but
    not yet reported): same optimum as one engine, fewer nodes than two independent halves."""
    from csolve_amd import problems
    from csolve_amd.solver import Search, solve_root
    model = solve_root(problems.schedule(8, 1))
    one = Search(model, 1 << 18, 1 << 14)
    one.put(model.root_state())
    ref = one.run()
    assert ref["done"] and ref["best"] == 31
    a, b = Search(model, 1 << 18, 1 << 14), Search(model, 1 << 18, 1 << 14)
    a.put(model.root_state())
    st = a.run(6)
    assert not st["done"] and st["pool"] >= 2
    b.put(a.take(st["pool"] // 2).contiguous())
    sa = sb = None
    for _ in range(100000):
        sa, sb = a.run(8), b.run(8)
        best = min(sa["best"], sb["best"])
        a.set_best(best)
        b.set_best(best)
        if sa["done"] and sb["done"]:
            break
    assert sa["done"] and sb["done"]
    assert min(sa["best"], sb["best"]) == 31
    row = a.best_solution() if sa["best"] == 31 and a.best_solution() is not None else b.best_solution()
    assert row is not None and row[model.objective_var] == 31


@pytest.mark.parametrize("pool,children", [(600, 128), (2000, 1024), (40000, 4096)])
def test_small_pools_still_walk_the_whole_tree(pool, children):
    """A pool that is far too small for breadth: the engine sizes its batches by what fits (and falls back to
    depth-first below its reserve) and still finds every solution exactly once."""
    from csolve_amd import problems
    model, s, st = _solve(problems.queens(10, "ALL"), pool=pool, children=children)
    assert st["done"] == 1 and st["solutions"] == 724 and st["pool_peak"] <= max(pool, children + 1)


@pytest.mark.parametrize("name,best", [("ref_schedule", 11), ("schedule6_s1", 22), ("ref_wcet", 1560)])
def test_device_driven_iterations_equal_host_driven_ones(name, best, monkeypatch):
    """ANY / MIN / MAX iterations are enqueued sixteen at a time with the bookkeeping on the device (one hipGraph);
    CSGPU_SEARCH_BURST=0 drives every iteration from the host and CSGPU_SEARCH_GRAPH=0 enqueues the launches one
    by one: same optimum and a valid solution every way, and an iteration budget that is not a multiple of
    sixteen is kept exactly."""
    from csolve_amd.solver import Search, solve_root
    text = open(golden("problems", name + ".txt")).read()
    model = solve_root(text)
    stats = {}
    for mode, env in (("graph", {}), ("launches", {"CSGPU_SEARCH_GRAPH": "0"}), ("host", {"CSGPU_SEARCH_BURST": "0"}),
                      ("one-workgroup", {"CSGPU_SEARCH_BURST_SPLIT": "0"}), ("evaluated", {"CSGPU_SEARCH_EVAL": "1"})):
        monkeypatch.delenv("CSGPU_SEARCH_GRAPH", raising=False)
        monkeypatch.delenv("CSGPU_SEARCH_BURST", raising=False)
        monkeypatch.delenv("CSGPU_SEARCH_BURST_SPLIT", raising=False)
        monkeypatch.delenv("CSGPU_SEARCH_EVAL", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = Search(model, 1 << 20, 1 << 16)
        s.set_parents(64)  # the same batches in every mode
        s.put(model.root_state())
        iterations = 0
        for _ in range(1000000):
            before = iterations
            st = s.run(21)
            iterations = st["iterations"]
            assert iterations - before <= 21
            if st["done"]:
                break
        assert st["done"] == 1 and st["best"] == best, mode
        row = s.best_solution()
        assert row is not None and row[model.objective_var] == best
        truth = model.eval_root(torch.from_numpy(np.stack([row, row], 1)[None].astype(np.int32)).cuda())
        assert int(truth[0]) == 1
        stats[mode] = st
    assert stats["graph"] == stats["launches"]  # the graph is only a way of launching
    # a MIN / MAX iteration's bookkeeping by sixteen / thirty-two workgroups or by one: the same nodes in the same places
    assert stats["graph"] == stats["one-workgroup"]
    # models without expression-tree clauses launch no root evaluation for their complete children (it can only say
    # "true"); CSGPU_SEARCH_EVAL=1 evaluates them all the same: not one is rejected, the search is the same search
    assert stats["graph"] == stats["evaluated"]
    # the host-driven loop learns of a new incumbent one iteration later, so it may expand a few more nodes
    assert stats["host"]["nodes"] >= stats["graph"]["nodes"]


def test_children_cut_by_their_parents_set_are_counted_not_launched(monkeypatch):
    """Values that a parent's own forbidden set rules out are cut without a fixpoint launch
    (CSGPU_SEARCH_HOLES=0 launches every value of the interval): the same tree either way --
    nodes, cuts, solutions -- for ALL; ANY reaches a valid solution either way (its value order is a
    rotation of the launched children, so the first solution may differ)."""
    from csolve_amd import problems
    from csolve_amd.solver import Search, solve_root
    for n, objective in ((9, "ALL"), (11, "ALL"), (40, "ANY")):
        model = solve_root(problems.queens(n, objective))
        runs = []
        for holes in ("1", "0"):
            monkeypatch.setenv("CSGPU_SEARCH_HOLES", holes)
            s = Search(model, 1 << 18, 1 << 14)
            s.put(model.root_state())
            st = s.run(20000)
            assert st["done"] == 1 and st["solutions"] >= 1
            runs.append({k: st[k] for k in ("nodes", "cuts", "solutions")})
            row = s.solutions(1)[0]
            assert len(set(row)) == n and len(set(row + np.arange(n))) == n and len(set(row - np.arange(n))) == n
        if objective == "ALL":
            assert runs[0] == runs[1]


def test_lanes_on_one_gpu_reach_the_same_results():
    """LaneSearch: several engines of one model on one GPU, a host thread each, exchanging incumbent and open
    states like ranks do.  ALL: the same tree (nodes, cuts, solutions) as one engine, reproducible run to run; MIN:
    the same optimum, with a solution that attains it on the lane that found it."""
    from csolve_amd import problems
    from csolve_amd.parallel import LaneSearch
    from csolve_amd.solver import Search, solve_root
    model = solve_root(problems.queens(10, "ALL"))
    one = Search(model, 1 << 18, 1 << 14)
    one.put(model.root_state())
    ref = one.run()
    runs = []
    for _ in range(2):
        lanes = [Search(model, 1 << 18, 1 << 14) for _ in range(3)]
        tot = LaneSearch(lanes, model.objective, slice_iterations=4, seed_states_per_lane=16, low_water=16).run(model.root_state())
        runs.append(tot)
        assert tot["done"] == 1
        assert (tot["nodes"], tot["cuts"], tot["solutions"]) == (ref["nodes"], ref["cuts"], ref["solutions"])
        assert all(x > 0 for x in tot["lanes"])
    # the totals are the tree's; which lane walks which subtree is not fixed: the fused levels (cs_step.hip.h) hand
    # parents to waves by ticket, so the order of a frontier's survivors in the pool -- and with it the frontier a
    # lane seeds the others from -- depends on timing
    for k in ("nodes", "cuts", "solutions", "props", "best", "done"):
        assert runs[0][k] == runs[1][k], k
    # MIN: the lanes keep ONE incumbent in device memory (share_incumbent), so what a lane prunes depends on when
    # the others find their solutions: the optimum is fixed, the node counts are not
    model = solve_root(problems.schedule(8, 1))
    for _ in range(2):
        lanes = [Search(model, 1 << 18, 1 << 14) for _ in range(4)]
        tot = LaneSearch(lanes, model.objective).run(model.root_state())
        assert tot["done"] == 1 and tot["best"] == 31
        rows = [e.best_solution() for e in lanes]
        assert any(r is not None and r[model.objective_var] == 31 for r in rows)
        # only a row that attains the common incumbent is ever shown; LaneSearch picks it
        assert all(r is None or r[model.objective_var] == 31 for r in rows)


def test_a_shared_incumbent_survives_its_owner_and_refuses_to_be_decoupled():
    """csgpu_search_share_incumbent: the lender may be freed first (its memory stays until the last borrower is
    gone), set_parents cannot take a sharing engine off the device-driven iterations, and an engine whose own
    row was overtaken by another engine's improvement reports no best solution instead of a stale one."""
    from csolve_amd import problems
    from csolve_amd._lib import CsolveError
    from csolve_amd.solver import Search, solve_root
    model = solve_root(problems.schedule(8, 1))
    lender = Search(model, 1 << 18, 1 << 14)
    a = Search(model, 1 << 18, 1 << 20)  # room for more parents per iteration than the device-driven path takes
    b = Search(model, 1 << 18, 1 << 14)
    a.share_incumbent(lender)
    b.share_incumbent(a)  # collapses onto the lender
    with pytest.raises(CsolveError):
        lender.share_incumbent(a)  # a lender cannot borrow
    with pytest.raises(CsolveError):
        a.set_parents(1 << 20)  # would switch `a` to host-driven iterations that bypass the shared word
    a.set_parents(64)
    lender.close()  # deferred inside the library
    torch.cuda.synchronize()
    # `a` finds an incumbent; `b`, which shares the word, is bounded by it
    a.put(model.root_state())
    st = a.run(40)
    while st["best"] == 2**31 - 1 and not st["done"]:
        st = a.run(8)
    first = st["best"]
    row = a.best_solution()
    assert row is not None and row[model.objective_var] == first
    b.put(model.root_state())
    stb = b.run()
    assert stb["done"] == 1 and stb["best"] == 31
    rb = b.best_solution()
    sta = a.run()
    assert sta["done"] == 1 and sta["best"] == 31
    ra = a.best_solution()
    # whoever reached 31 first holds the row; the other one's row (if any) was overtaken and is not shown
    rows = [r for r in (ra, rb) if r is not None]
    assert len(rows) >= 1 and all(r[model.objective_var] == 31 for r in rows)
    if first > 31:
        assert rb is not None or ra is not None
    a.close()
    b.close()
    torch.cuda.synchronize()


def _bench_search(extra, ranks=1, timeout=420):
    """bench.py --workload search in child processes (the process group lives and dies with them) -> the JSON line"""
    import subprocess
    import sys
    from conftest import ROOT
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable]
    if ranks > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
                "--master-port", str(port)]
    cmd += [os.path.join(ROOT, "bench.py"), "--workload", "search", "--gpus", str(ranks), "--steps", "1", "--warmup", "0"] + extra
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def test_the_coordinator_runs_over_rccl_with_device_tensors():
    """the `nccl` branch of ShardedSearch with a world of one rank: all_gather_into_tensor / all_reduce on device
    tensors through RCCL, the same walk as without a process group, per-rank clocks in the bench record"""
    rec = _bench_search(["--search-queens", "10", "--process-group", "--comm", "nccl"])
    assert rec["config"]["process_group"] == "nccl" and rec["config"]["solutions"] == 724
    plain = _bench_search(["--search-queens", "10"])
    assert plain["config"]["process_group"] is None
    assert (plain["config"]["nodes"], plain["config"]["cuts"]) == (rec["config"]["nodes"], rec["config"]["cuts"])
    r = rec["ranks"][0]
    assert 0.0 <= r["idle_fraction"] < 1.0 and r["busy_seconds"] > 0 and r["put_states"] >= 1


def test_four_ranks_on_one_gpu_walk_the_single_engine_tree():
    """four ranks sharing cuda:0 (gloo, host tensors between them): the status page is in use, every rank seeded
    itself, the totals equal the one-rank tree, and the cost of rebuilding forbidden sets of seeded and stolen
    states is a small part of a rank's time"""
    one = _bench_search(["--search-queens", "12"])
    rec = _bench_search(["--search-queens", "12", "--comm", "gloo", "--same-device"], ranks=4)
    assert rec["config"]["solutions"] == one["config"]["solutions"] == 14200
    assert (rec["config"]["nodes"], rec["config"]["cuts"]) == (one["config"]["nodes"], one["config"]["cuts"])
    assert len(rec["ranks"]) == 4 and all(n > 0 for n in rec["config"]["nodes_per_rank"])
    assert all(r["put_fraction"] is not None and r["put_fraction"] < 0.05 for r in rec["ranks"]), rec["ranks"]


def test_the_engine_applies_the_incumbent_like_the_reference_unit_vectors():
    """test/test_objective.c ObjectiveBetter / ObjectiveUpdateVal / ObjectiveUpdateBest on the device: an engine
    given the incumbent `best` expands a node whose objective variable is `val`; children survive with the
    tightened objective interval exactly when objective_better() holds, and a solution updates the incumbent"""
    from csolve_amd.solver import Search, solve_root
    cases = json.load(open(golden("ref_unit_objective.json")))["cases"]
    checked = 0
    for c in cases:
        if c.get("objective") not in ("MIN", "MAX") or c["fn"] not in ("better", "update_val") or c["val"] is None:
            continue
        lo, hi = c["val"]
        # the objective variable x with the vector's interval and a free 0/1 variable to branch on
        model = solve_root(f"{c['objective']} x; {lo} <= x; x <= {hi}; 0 <= y; y <= 1;")
        s = Search(model, 1 << 10, 1 << 8)
        s.put(model.root_state())
        s.set_best(c["best"])
        st = s.run(1)
        from csolve_amd import _lib
        b = _lib.load_library().csgpu_objective_bound(model.objective, _lib.Val(lo, hi), c["best"])
        better = c["expect"] if c["fn"] == "better" else b.lo <= b.hi
        if c["fn"] == "update_val":
            assert [b.lo, b.hi] == c["expect_val"]
        if better and lo == hi:  # the children are complete assignments: solutions, and the incumbent moves
            assert st["solutions"] >= 1 and st["best"] == lo and st["cuts"] == 0, (c, st)
        elif better:
            kids = s.take(4).cpu().numpy()
            assert kids.shape[0] == 2 and st["cuts"] == 0, (c, st)
            ov = model.objective_var
            got = sorted([int(k[ov, 0]), int(k[ov, 1])] for k in kids)
            # branched on y: both children carry the bounded interval; branched on x itself (a tie of two-value
            # intervals goes to the lower index): the children are the values of the bounded interval
            assert got == [[b.lo, b.hi]] * 2 or (b.hi - b.lo == 1 and got == [[b.lo, b.lo], [b.hi, b.hi]]), (c, got)
        else:
            assert st["pool"] == 0 and st["cuts"] == 2, (c, st)
        checked += 1
        s.close()
    assert checked >= 20
    # ObjectiveUpdateBest: the incumbent after the first solution is the objective's lower (MIN) / upper (MAX) bound
    for text, best in (("MIN x; -17 <= x; x <= 5;", -17), ("MAX x; -3 <= x; x <= 17;", 17)):
        model = solve_root(text)
        s = Search(model, 1 << 10, 1 << 8)
        s.put(model.root_state())
        st = s.run()
        assert st["done"] == 1 and st["best"] == best
        s.close()


def test_complete_nodes_of_a_ne_network_need_no_root_evaluation(monkeypatch):
    """ALL on pure != networks: the engine counts complete consistent children as solutions without evaluating the root
    (a clause between two valued variables was revised when the second became a value); with CSGPU_SEARCH_EVAL=1 it
    evaluates them all the same -- same solutions, nodes and cuts, and the stored rows satisfy every clause"""
    from csolve_amd import problems
    for text in (problems.queens(9, "ALL"), problems.offsets(7, 6, 3).replace("ANY;", "ALL;", 1)):
        runs = []
        for ev in ("0", "1"):
            monkeypatch.setenv("CSGPU_SEARCH_EVAL", ev)
            model, s, st = _solve(text)
            assert st["done"] == 1
            runs.append((st["solutions"], st["nodes"], st["cuts"]))
            rows = s.solutions(64)
            for row in rows:
                truth = model.eval_root(torch.from_numpy(np.stack([row, row], 1)[None].astype(np.int32)).cuda())
                assert int(truth[0]) == 1
        assert runs[0] == runs[1] and runs[0][0] > 0, runs


@pytest.mark.gpu
def test_split_bookkeeping_of_min_iterations_walks_the_same_tree(monkeypatch):
    """Iterations of up to 1,024 parents (the default of MIN / MAX): branching + emitting by sixteen workgroups and
    classification by thirty-two give, counter for counter, the search of the single-workgroup kernels."""
    from csolve_amd import problems
    from csolve_amd.solver import Search, solve_root
    model = solve_root(problems.schedule(8, seed=3))
    stats = {}
    monkeypatch.setenv("CSGPU_SEARCH_PARENTS_MAX", "1024")  # what one workgroup can scan: the same batches in every mode
    for mode in ("split", "one", "evaluated"):
        monkeypatch.delenv("CSGPU_SEARCH_BURST_SPLIT", raising=False)
        monkeypatch.delenv("CSGPU_SEARCH_EVAL", raising=False)
        if mode == "one":
            monkeypatch.setenv("CSGPU_SEARCH_BURST_SPLIT", "0")
        if mode == "evaluated":  # the root evaluation of complete children, left out for models without tree clauses
            monkeypatch.setenv("CSGPU_SEARCH_EVAL", "1")
        s = Search(model, 1 << 21, 1 << 17)
        s.put(model.root_state())
        st = s.run(1 << 30)
        assert st["done"] == 1
        stats[mode] = st
    assert stats["split"] == stats["one"] == stats["evaluated"]
    assert stats["split"]["iterations"] > 10 and stats["split"]["nodes"] > 10000
    # the default, 2,048 parents (thirty-two workgroups): the same optimum over fewer, fuller iterations
    monkeypatch.delenv("CSGPU_SEARCH_PARENTS_MAX", raising=False)
    monkeypatch.delenv("CSGPU_SEARCH_EVAL", raising=False)
    s = Search(model, 1 << 21, 1 << 17)
    s.put(model.root_state())
    wide = s.run(1 << 30)
    assert wide["done"] == 1 and wide["best"] == stats["split"]["best"] and wide["iterations"] <= stats["split"]["iterations"]


def _prefix_state(model, steps, seed):
    """a consistent state `steps` assignments below the root: seeded random variable, lowest value, propagated"""
    rng = np.random.default_rng(seed)
    state = model.root_state()
    for _ in range(steps):
        dom = state[0].cpu().numpy()
        open_vars = [v for v in range(model.n_vars) if dom[v, 0] != dom[v, 1] and v != model.objective_var]
        if not open_vars:
            break
        v = int(rng.choice(open_vars))
        for value in range(int(dom[v, 0]), int(dom[v, 1]) + 1):
            nodes = torch.tensor([[v, value, value, 0]], dtype=torch.int32, device="cuda")
            out, res = model.propagate(state, nodes)
            if int(res[0, 0]) >= 0:
                state = out[:1].contiguous()
                break
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("which,steps", [("schedule8", 3), ("schedule8", 6), ("ref_wcet", 4), ("queens10", 2), ("sudoku9", 5)])
def test_a_model_specialised_for_a_subtree_gives_the_subtrees_results(which, steps):
    """csgpu_model_specialize + normalize + finalize rewrite the tables for the subtree below a prefix
    state (what the prefix decided is folded, entailed clauses leave the lists).  Results-neutral: the search below
    the prefix finds the same solutions / the same optimum with either model, over the same tree."""
    from csolve_amd import problems
    from csolve_amd.solver import Search, solve_root
    text = {"schedule8": lambda: problems.schedule(8, seed=3), "queens10": lambda: problems.queens(10, "ALL"),
            "ref_wcet": lambda: open(golden("problems", "ref_wcet.txt")).read(),
            "sudoku9": lambda: problems.sudoku(3, 0.3, 2).replace("ANY", "ALL", 1)}[which]()
    model = solve_root(text)
    prefix = _prefix_state(model, steps, seed=11)
    special = model.specialize(prefix)
    info, info_s = model.device_info(), special.device_info()
    # nothing is added, and what the prefix decided is gone from the lists
    assert info_s["adjacency_entries"] <= info["adjacency_entries"]
    runs = []
    for m in (model, special):
        s = Search(m, 1 << 19, 1 << 15)
        s.put(prefix)
        st = s.run(1 << 40)
        assert st["done"] == 1
        sols = sorted(map(tuple, s.solutions(4096).tolist())) if m.objective == 1 else None
        runs.append((st, sols, s.best_solution()))
    (a, sa, ba), (b, sb, bb) = runs
    assert a["solutions"] == b["solutions"] and a["best"] == b["best"] and sa == sb
    if model.objective in (2, 3) and ba is not None:
        assert bb is not None and ba[model.objective_var] == bb[model.objective_var]
    if model.objective == 1:  # ALL: the same tree, node for node
        assert (a["nodes"], a["cuts"]) == (b["nodes"], b["cuts"])
    print(which, steps, "adjacency", info["adjacency_entries"], "->", info_s["adjacency_entries"],
          "clauses", model.n_clauses, "->", special.n_clauses, "nodes", a["nodes"], b["nodes"])


def test_a_refused_engine_leaves_its_model_open_to_conflicts():
    """csgpu_search_create checks max_children and pool_capacity before it counts the engine on its model: after two
    refused engines the model still takes a learnt conflict clause (csgpu_model_add_conflict refuses one while an
    engine holds the model's device tables)."""
    from csolve_amd import problems
    from csolve_amd._lib import CsolveError
    from csolve_amd.solver import Search, solve_root
    model = solve_root(problems.queens(8))
    with pytest.raises(CsolveError):
        Search(model, 1 << 20, 1 << 30)  # max_children too large
    with pytest.raises(CsolveError):
        Search(model, 1 << 31, 1 << 16)  # pool_capacity too large
    model.add_conflict([(0, 1), (1, 3)])  # raised CsolveError while the refused engines were still counted
