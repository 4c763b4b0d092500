"""CPU tests of the spread of the ordered clause walk as it is specified (many_ordered_spread_walk, no device): the
children of a stopped many_walk_ordered.Walk, halves included, walked as root rows of their own and folded back, against
the one walk.

Under ALL the fold is exact: every owner equals the one many_walk_ordered.walk in status, nodes, cuts, solutions, halvings
and first, for budget pairs from the sets' own down to (1, 1).  The oracle's props are not compared on the host, for the
reason given in many_clause_spread_walk.  Under MIN / MAX status and best are the one walk's, first is a solution of value
best, and the answer is deterministic.  The tests assert that their inputs hold every kind of frame: without a pushed
halving parent, a current node with neither half tried, one between its halves, an enumerating frame with several values
left, a sub-row that is inconsistent as a root and (MIN / MAX) one whose start bound empties dom[obj], they would prove
nothing.  Every set finishes within 2^15 nodes per row."""
import numpy as np
import pytest

import many_ordered_spread_walk as S
import many_walk_objective as W
import many_walk_ordered as O

ALL_BUDGETS = {"wcet_max": [(8, 64), (3, 7), (1, 1)], "wide2_mid": [(8, 64), (2, 5), (1, 1)], "wide3_plain": [(8, 64), (1, 1)]}


def _first_budget_kinds(name, objective, order, split, budget):
    kinds = dict(pushed_halving=0, unsplit=0, between=0, several=0)
    for walk, record in S.stopped_walks(name, objective, order, split, budget):
        if record["status"] == S.LIMIT:
            for k, x in S.kinds_of(walk).items():
                kinds[k] += x
    return kinds


def test_the_sets_finish_and_hold_every_kind_of_frame():
    for name, objective, order, split, _ in S.ALL_CASES + S.MINMAX_CASES:
        one = S.one_walk(name, objective, order, split)
        assert (one["status"] == S.DONE).all() and one["nodes"].max() < S.FINISH, (name, order)
        assert one["halvings"].max() > 0, (name, order)
    # measured at the first budget of three sets (the fanned checkpoints of round 1).  `several` counts every enumerating
    # frame, pushed or current, with more than one value left
    assert _first_budget_kinds("wcet_max", "ALL", "largest-value", 4, 8) == dict(pushed_halving=70, unsplit=4, between=2, several=12)
    kinds = _first_budget_kinds("schedule6_min_budget", "MIN", "smallest-value", 4, 16)
    assert kinds == dict(pushed_halving=181, unsplit=4, between=2, several=94)
    kinds = _first_budget_kinds("schedule5_open_min", "MIN", "none", 4, 4)
    assert (kinds["pushed_halving"], kinds["unsplit"]) == (32, 8)


def test_children_of_a_stopped_walk_follow_the_walks_own_rule():
    """every child row differs from its frame's node in the one variable, lies inside it, and the children of a frame
    tile exactly what the walk has left of the variable; the count is the rows'; unsplit is the current node's alone"""
    seen = dict(unsplit=0, second=0, enumerating=0)
    for name, objective, order, split, budgets in (S.ALL_CASES[0], S.MINMAX_CASES[2]):
        for walk, record in S.stopped_walks(name, objective, order, split, budgets[0]):
            if record["status"] != S.LIMIT:
                continue
            rows = S.children_of(walk)
            assert len(rows) == S.count_children(walk) and rows.dtype == np.int32
            frames = S.frames_of(walk)
            at = 0
            for d in range(len(frames) - 1, -1, -1):  # the current node first
                node, v, nv = frames[d]
                current = d == len(frames) - 1
                kind = S.frame_kind(node, v, nv, split, current)
                seen[kind] += 1
                lo, hi = int(node[v, 0]), int(node[v, 1])
                left = lo if kind == "unsplit" else nv  # what the walk has left of the variable: [left, hi]
                kids = S.frame_children(node, v, nv, split, current)
                assert len(kids) == (2 if kind == "unsplit" else 1 if kind == "second" else hi - nv + 1)
                for a, b in kids:
                    row = rows[at]
                    others = np.arange(len(node)) != v
                    assert (row[others] == node[others]).all() and tuple(row[v]) == (a, b) and a == left and b <= hi
                    assert (a == b) == (kind == "enumerating") or b - a + 1 <= split
                    left = b + 1
                    at += 1
                assert left == hi + 1
                if kind != "enumerating":
                    mid = (lo + hi) >> 1
                    assert kids[-1] == (mid + 1, hi) and (kind == "second" or kids[0] == (lo, mid))
            assert at == len(rows)
            assert S.unsplit_of(walk) == int(S.frame_kind(*frames[-1], split, True) == "unsplit")
    assert min(seen.values()) > 0, seen


@pytest.mark.parametrize("name,objective,order,split,budgets", S.ALL_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_the_all_spread_is_the_one_walk_halvings_included(name, objective, order, split, budgets):
    one = S.one_walk(name, objective, order, split)
    assert budgets in ALL_BUDGETS[name]
    total = dict(pushed_halving=0, unsplit=0, between=0, several=0, dead_rows=0)
    for pair in ALL_BUDGETS[name]:
        owners, info = S.spread_of(name, objective, order, split, pair)
        assert info["rounds"] > 2 and info["sub_instances"] == sum(info["per_round"])
        for i, o in enumerate(owners):
            for f in ("status", "nodes", "cuts", "solutions", "halvings"):
                assert o[f] == one[f][i], (pair, i, f, o[f], one[f][i])
            if one["solutions"][i] > 0:
                assert (o["first"] == one["first"][i]).all(), (pair, i)
            else:
                assert o["first"] is None
        for k in total:
            total[k] += info[k]
    assert total["pushed_halving"] > 0 and total["several"] > 0 and total["dead_rows"] > 0, total
    if name == "wcet_max":  # the set that holds every kind
        assert min(total.values()) > 0, total


def test_the_all_spread_cut_short_leaves_limit_owners_with_what_was_folded():
    name, objective, order, split, budgets = S.ALL_CASES[0]
    one = S.one_walk(name, objective, order, split)
    owners, info = S.spread_of(name, objective, order, split, budgets, 2)
    assert info["rounds"] == 2
    left = np.array([o["status"] == S.LIMIT for o in owners])
    assert left.any() and not left.all()
    for i, o in enumerate(owners):
        if left[i]:
            assert 0 < o["nodes"] < one["nodes"][i] and o["halvings"] <= one["halvings"][i]
        else:
            assert all(o[f] == one[f][i] for f in ("status", "nodes", "cuts", "solutions", "halvings"))


@pytest.mark.parametrize("name,objective,order,split,budgets", S.MINMAX_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_the_minmax_spread_proves_the_one_walks_optimum(name, objective, order, split, budgets):
    text, roots = S.rows_of(name)
    one = S.one_walk(name, objective, order, split)
    owners, info = S.spread_of(name, objective, order, split, budgets)
    ov = W.model_of(text).view.obj_var
    orc = W.oracle_for(text)[0]
    assert info["rounds"] > 2 and info["pushed_halving"] > 0 and info["dead_rows"] > 0
    assert info["emptied"] > 0, "no sub-row whose start bound empties dom[obj]"
    for i, o in enumerate(owners):
        assert o["status"] == one["status"][i] == S.DONE
        if one["solutions"][i] == 0:
            assert o["best"] is None and o["first"] is None and o["solutions"] == 0
            continue
        assert o["best"] == one["best"][i] and o["first"][ov] == o["best"]
        row = np.stack([o["first"], o["first"]], 1).astype(np.int32)
        assert ((row >= roots[i][:, :1]) & (row <= roots[i][:, 1:])).all(), "a row outside its instance"
        status, _ = orc.instance(row, -1, 0, 0)
        assert status >= 0, "first does not satisfy the model"
    # deterministic: a second run of the drivers, not the cached one.  The whole spread of `schedule5_open_min` makes
    # 200,000 to 360,000 sub-instances on the host (ten seconds and more): there the two runs are cut short after four
    # rounds: halves fanned out three times and the first folds of the incumbents
    if name == "schedule5_open_min":
        owners, info = S.spread_minmax(text, roots, objective, order, split, budgets, 4)
        assert info["rounds"] == 4 and info["pushed_halving"] > 0 and info["unsplit"] > 0 and info["dead_rows"] > 0
        again, info2 = S.spread_minmax(text, roots, objective, order, split, budgets, 4)
    else:
        again, info2 = S.spread_minmax(text, roots, objective, order, split, budgets)
    assert info2 == info
    if True:
        for a, b in zip(owners, again):
            assert {k: v for k, v in a.items() if k != "first"} == {k: v for k, v in b.items() if k != "first"}
            assert (a["first"] is None and b["first"] is None) or (a["first"] == b["first"]).all()


def test_a_walk_from_a_start_incumbent():
    """have == 0 is the ordered walk; a start bounds the root row; nothing beats the optimum; only own solutions count"""
    name, objective, order, split, _ = S.MINMAX_CASES[2]
    text, roots = S.rows_of(name)
    one = S.one_walk(name, objective, order, split)
    sense = W.SENSE[objective]
    checked = 0
    for i in (0, 5, 11):
        plain = O.walk(text, roots[i], objective, S.FINISH, order, split)
        none = S.walk_from(text, roots[i], objective, order, split)
        for f in S.FIELDS + ("root_props", "props", "best"):
            assert none[f] == plain[f], f
        if plain["solutions"] == 0:
            continue
        best = int(one["best"][i])
        proof = S.walk_from(text, roots[i], objective, order, split, start=best)
        assert proof["status"] == S.DONE and proof["solutions"] == 0 and proof["best"] is None and proof["first"] is None
        worse = best + 3 if sense == 1 else best - 3
        warm = S.walk_from(text, roots[i], objective, order, split, start=worse)
        assert warm["status"] == S.DONE and warm["best"] == best and warm["nodes"] <= plain["nodes"]
        checked += 1
    assert checked >= 2


def test_the_interface_is_declared_exported_and_prototyped():
    from csolve_amd import _lib
    from csolve_amd.solver import Model
    L = _lib.load_library()
    calls = {"csgpu_solve_many_clauses_ordered_from": 12, "csgpu_solve_many_clauses_ordered_from_resume": 10,
             "csgpu_many_clause_ordered_checkpoint_children": 8, "csgpu_many_clause_ordered_checkpoint_fanout": 12,
             "csgpu_many_fold_halvings": 5}
    for name, args in calls.items():
        assert name in _lib.declared_symbols(), name
        assert hasattr(L, name) and len(getattr(L, name).argtypes) == args, name
    name = "csgpu_internal_many_clauses_order_from_symbol"  # exported and prototyped, declared in cs_internal.h only
    assert name not in _lib.declared_symbols() and len(getattr(L, name).argtypes) == 3
    for method in ("clause_ordered_checkpoint_children", "clause_ordered_checkpoint_fanout", "fold_many_halvings",
                   "many_clauses_order_from_kernel"):
        assert callable(getattr(Model, method)), method
    import inspect
    assert "start" in inspect.signature(Model.solve_many_clauses_ordered).parameters
    spread = inspect.signature(Model.solve_many_clauses_spread).parameters
    assert spread["order"].default is None and spread["split_width"].default == 256
    header = open(_lib.HEADER_PATH).read()
    for phrase in ("d_unsplit[i] = 1", "csgpu_many_fold_halvings", "neither mid + 1 nor, for the current node only, lo"):
        assert phrase in header, phrase
    for section in ("Not on this walk: up to k", "Not built on the ordered walk:"):
        listed = header[header.index(section):]
        listed = listed[:listed.index("*/")]
        assert "start incumbents" not in listed.split(".")[0] and "restarts" in listed and "the solution stream" in listed


def test_the_shipped_library_holds_the_eight_instantiations():
    from test_solve_many_clauses_ordered_resume_host import shipped
    names = shipped("cs_walk_order_from")
    assert names == {f"cs_walk_order_from<{cpl}, {tree}>" for cpl in (1, 2, 4, 8) for tree in ("true", "false")}
    import subprocess
    from csolve_amd import _lib
    symbols = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for kernel in ("cs_walk_order_children", "cs_walk_order_fanout", "cs_walk_fold_halvings"):  # not templated
        assert f"{len(kernel)}{kernel}" in symbols, kernel
