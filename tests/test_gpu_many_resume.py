"""GPU tests of the checkpoints of Model.solve_many (cs_dive_resume: csgpu_solve_many_checkpointed, csgpu_solve_many_resume,
csgpu_many_checkpoint_states).  The yardstick is Model.solve_many with ONE budget, which test_gpu_solve_many.py pins to
the oracle walk node for node: a walk in slices must equal, field for field, the one call with the summed budget.  The
host walk that stops and goes on (tests/many_resume_walk.py) is used directly for the smallest set and for the open
subtrees.  Every call passes a finite max_nodes."""
import numpy as np
import pytest

import many_resume_walk
import many_sets
import many_walk
from test_many_resume_host import resume_kernel_of, shipped_resume_kernels

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("status", "root_props", "nodes", "cuts", "props", "solutions")
DONE, LIMIT, BAD_SLOT = 0, 1, 3
_models = {}
_sets = {}


def _model(text):
    from csolve_amd.solver import solve_root
    if text not in _models:
        _models[text] = solve_root(text)
    return _models[text]


def _set(name):
    """(text, roots, roots on the device, objective, budget), built once"""
    if name not in _sets:
        text, roots, objective, budget = many_sets.build(name)
        _sets[name] = (text, roots, torch.from_numpy(roots).cuda(), objective, budget)
    return _sets[name]


def _host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if torch.is_tensor(v) and not k.startswith("_")}


def _one_call(model, dev, objective, budget):
    return _host(model.solve_many(dev, objective, max_nodes=budget))


def _same(got, want, label, rows=None):
    """every field of every instance, and the first solutions (zero rows where there is none, in both)"""
    for f in FIELDS + ("first",):
        g, w = got[f], want[f]
        if rows is not None:
            g, w = g[rows], w[rows]
        if len(g) == 0:
            continue
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{label}: {f} differs for {bad.size} instances, first {bad[0]}: got {g[bad[0]]}, one call {w[bad[0]]}"


def _slots_are_sound(got, capacity, label):
    """a slot for exactly the stopped instances (the pool is large enough), all different, inside the pool"""
    stopped = got["status"] == LIMIT
    assert ((got["slot"] >= 0) == stopped).all(), f"{label}: a slot without a stop, or a stop without a slot"
    used = got["slot"][stopped]
    assert len(set(used.tolist())) == len(used) and (used < capacity).all(), f"{label}: slots {used}"


@pytest.mark.parametrize("name", sorted(many_sets.SETS))
def test_split_equals_whole(name):
    """budget 1, then 7, 56 and the set's own more: after every slice the one call with the summed budget"""
    text, roots, dev, objective, budget = _set(name)
    model = _model(text)
    assert model.many_kernel() == many_sets.SETS[name][3]  # the old call launches what it launched
    assert model.many_resume_kernel() == resume_kernel_of(name)
    K = len(roots)
    steps = (1, 3, 4, budget) if name == "sudoku16_any" else (1, 7, 56, budget)
    pool = model.many_checkpoints(K)
    total, stopped = 0, []
    for k, b in enumerate(steps):
        if k == 0:
            out = model.solve_many(dev, objective, max_nodes=b, checkpoints=pool)
        else:
            assert model.resume_many(out, max_nodes=b, objective=objective) is out
        total += b
        got = _host(out)
        _same(got, _one_call(model, dev, objective, total), f"{name} after {steps[:k + 1]}")
        _slots_are_sound(got, K, f"{name} after {steps[:k + 1]}")
        stopped.append(int((got["status"] == LIMIT).sum()))
        if name == "queens12_two" and k == 1:
            walk = many_walk.dive_many(text, roots, objective, 8)
            _same(got, walk, "queens12_two after (1, 7) against the host walk")
    print(f"{name}: {K} instances, stopped after each of {steps}: {stopped}")
    assert stopped[0] > 0 and stopped[2] > 0, "instances must stop and go on inside their trees"
    assert stopped[3] == 0 and (got["slot"] == -1).all()


def test_rows_of_finished_instances_are_not_touched():
    text, roots, dev, objective, budget = _set("sudoku9_any")
    model = _model(text)
    K = len(roots)
    pool = model.many_checkpoints(K)
    out = model.solve_many(dev, objective, max_nodes=64, checkpoints=pool)
    before = _host(out)
    done = np.flatnonzero(before["status"] == DONE)
    left = np.flatnonzero(before["status"] == LIMIT)
    assert done.size > 8 and left.size > 8, "the budget must split the set"
    idx = torch.from_numpy(done).cuda()
    out["_records"][idx] = 0x5a5a5a5a5a5a5a5a
    out["first"][idx] = 0x5a5a5a5a
    model.resume_many(out, max_nodes=budget, objective=objective)
    torch.cuda.synchronize()
    assert (out["_records"][idx] == 0x5a5a5a5a5a5a5a5a).all() and (out["first"][idx] == 0x5a5a5a5a).all()
    after = _host(out)
    assert (after["slot"] == -1).all()
    _same(after, _one_call(model, dev, objective, 64 + budget), "the resumed rows", rows=left)


def test_an_empty_pool_ends_an_instance_as_without_checkpoints():
    from csolve_amd import CsolveError
    text, roots, dev, objective, budget = _set("queens12_two")
    model = _model(text)
    pool = model.many_checkpoints(5)
    plain = _one_call(model, dev, objective, 4)
    full = _one_call(model, dev, objective, budget)
    assert int((plain["status"] == LIMIT).sum()) > 5

    def first_call():
        out = model.solve_many(dev, objective, max_nodes=4, checkpoints=pool)
        got = _host(out)
        _same(got, plain, "budget 4, five slots")
        kept = np.flatnonzero(got["slot"] >= 0)
        assert kept.size == 5 and sorted(got["slot"][kept].tolist()) == [0, 1, 2, 3, 4]
        assert (got["status"][kept] == LIMIT).all() and (got["slot"][np.setdiff1d(np.arange(len(roots)), kept)] == -1).all()
        return out, kept

    out, kept = first_call()
    model.resume_many(out, max_nodes=budget, objective=objective)
    got = _host(out)
    others = np.setdiff1d(np.arange(len(roots)), kept)
    _same(got, full, "the five with a slot", rows=kept)
    _same(got, plain, "everything else", rows=others)
    assert (got["slot"] == -1).all()
    pool.reset()
    first_call()
    # a pool belongs to its model
    other = _model(_set("sudoku9_all")[0])
    with pytest.raises(CsolveError, match="another model") as e:
        other.solve_many(_set("sudoku9_all")[2], "ALL", max_nodes=4, checkpoints=pool)
    assert e.value.code == -1
    with pytest.raises(CsolveError, match="does not qualify") as e:
        from csolve_amd import problems
        _model(problems.schedule(6, 1)).many_checkpoints(4)
    assert e.value.code == -4


def test_more_instances_than_waves_in_slices_without_the_host():
    text, roots, dev, objective, budget = _set("queens12_two")
    model = _model(text)
    resident = model.many_waves(1 << 30)
    reps = -(-4 * resident // len(roots))
    big = dev.repeat(reps, 1, 1).contiguous()
    K = big.shape[0]
    assert model.many_waves(K) == resident and K >= 4 * resident
    want = _one_call(model, dev, objective, 16 + 64 + 65536)
    assert (want["status"] == DONE).all()
    pool = model.many_checkpoints(K)
    print(f"{K} instances on {resident} waves, pool of {K * model.checkpoint_bytes() >> 20} MiB")
    torch.cuda.synchronize()
    out = model.solve_many(big, objective, max_nodes=16, checkpoints=pool)
    model.resume_many(out, max_nodes=64, objective=objective)
    model.resume_many(out, max_nodes=65536, objective=objective)
    got = _host(out)
    tiled = {f: np.tile(want[f], (reps,) + (1,) * (want[f].ndim - 1)) for f in FIELDS + ("first",)}
    _same(got, tiled, "three calls queued on one stream")
    assert (got["slot"] == -1).all()


def test_a_slot_number_outside_the_pool_is_refused_by_the_kernel():
    """a range check, compared before anything is read: the instance gets CSGPU_MANY_BAD_SLOT and is otherwise as it was"""
    text, roots, dev, objective, budget = _set("queens12_two")
    model = _model(text)
    K = len(roots)
    pool = model.many_checkpoints(K)
    out = model.solve_many(dev, objective, max_nodes=4, checkpoints=pool)
    before = _host(out)
    stopped = np.flatnonzero(before["status"] == LIMIT)
    assert stopped.size > 4
    a, b = int(stopped[1]), int(stopped[3])
    out["slot"][a] = K          # the first number past the pool
    out["slot"][b] = 1 << 30    # far outside
    model.resume_many(out, max_nodes=budget, objective=objective)
    got = _host(out)
    assert got["status"][a] == BAD_SLOT and got["status"][b] == BAD_SLOT
    assert got["slot"][a] == K and got["slot"][b] == 1 << 30
    for f in FIELDS[1:] + ("first",):
        assert (got[f][[a, b]] == before[f][[a, b]]).all(), f
    others = np.setdiff1d(np.arange(K), [a, b])
    _same(got, _one_call(model, dev, objective, 4 + budget), "the neighbours", rows=others)


@pytest.mark.parametrize("name", ["sudoku9_all", "queens12_two"])
def test_a_search_finishes_what_the_dive_left_all(name):
    text, roots, dev, objective, budget = _set(name)
    assert objective == "ALL"
    model = _model(text)
    full = _one_call(model, dev, objective, budget)
    part = _one_call(model, dev, objective, 64)
    left = part["status"] == LIMIT
    assert left.sum() > 4
    out = model.solve_many_sliced(dev, objective, budgets=(64,), finish="search")
    got = _host(out)
    print(f"{name}: {out['sliced']}, {int(full['solutions'].sum())} solutions")
    assert out["sliced"] == {"slices": 1, "searched": int(left.sum())}
    assert (got["status"] == DONE).all() and (got["slot"] == -1).all()
    assert (got["solutions"] == full["solutions"]).all()
    _same(got, full, "instances the dive finished itself", rows=np.flatnonzero(~left))
    dive_had_one = left & (part["solutions"] > 0)
    assert (got["first"][dive_had_one] == full["first"][dive_had_one]).all()  # the dive's first solution stays
    assert (got["nodes"][left] >= 64).all()


def test_a_search_finishes_what_the_dive_left_any():
    text, roots, dev, objective, budget = _set("sudoku9_any")
    model = _model(text)
    full = _one_call(model, dev, objective, budget)
    left = _one_call(model, dev, objective, 8)["status"] == LIMIT
    assert left.sum() > 16
    out = model.solve_many_sliced(dev, objective, budgets=(8,), finish="search")
    got = _host(out)
    print(f"sudoku9_any: {out['sliced']}")
    assert out["sliced"]["searched"] == int(left.sum())
    assert (got["status"] == DONE).all()
    assert ((got["solutions"] > 0) == (full["solutions"] > 0)).all() and (got["solutions"] <= 1).all()
    solved = np.flatnonzero(got["solutions"] > 0)
    assert (left[solved]).any(), "some solution must be the search's"
    rows = got["first"][solved]
    assert ((rows >= roots[solved, :, 0]) & (rows <= roots[solved, :, 1])).all(), "a solution outside its givens"
    states = torch.from_numpy(np.ascontiguousarray(np.stack([rows, rows], 2))).cuda()
    truth = model.eval_root(states)
    assert (truth == 1).all(), "a reported first solution does not satisfy the model"
    assert (got["first"][got["solutions"] == 0] == 0).all()


def test_checkpoint_states_are_the_open_subtrees_of_the_host_walk():
    text, roots, dev, objective, budget = _set("sudoku9_all")
    model = _model(text)
    picked, walks, with_last = [], {}, 0
    for i in range(len(roots)):  # four stopped instances, by the host walk; one at least before a variable's last value
        w = many_resume_walk.Walk(text, roots[i], "ALL")
        if w.run(64)["status"] != LIMIT:
            continue
        if len(picked) == 3 and with_last == 0 and not w.has_last_value_frame():
            continue
        picked.append(i)
        walks[i] = w
        with_last += w.has_last_value_frame()
        if len(picked) == 4:
            break
    assert len(picked) == 4 and with_last >= 1
    pool = model.many_checkpoints(len(picked))
    out = model.solve_many(dev[picked].contiguous(), "ALL", max_nodes=64, checkpoints=pool)
    got = _host(out)
    assert (got["status"] == LIMIT).all()
    full = _one_call(model, dev[picked].contiguous(), "ALL", budget)
    for k, i in enumerate(picked):
        want = walks[i].open_subtrees()
        states = model.checkpoint_states(pool, int(got["slot"][k]))
        assert tuple(states.shape) == (len(walks[i].stack) + 1, model.n_vars, 2)
        assert (states.cpu().numpy() == want).all(), f"instance {i}"
        # and made ready for the engine: consistent ones only, complete ones apart; together they hold the rest
        open_states, complete = model.open_subtrees(pool, int(got["slot"][k]))
        below = sum(many_walk.dive(text, s, "ALL")["solutions"] for s in open_states.cpu().numpy()) + complete.shape[0]
        assert below == full["solutions"][k] - got["solutions"][k]
        assert not (open_states[:, :, 0] == open_states[:, :, 1]).all(dim=1).any()
    from csolve_amd import CsolveError
    with pytest.raises(CsolveError) as e:
        model.checkpoint_states(pool, len(picked))
    assert e.value.code == -1


def test_the_sets_launch_every_shipped_resume_instantiation():
    planned = set()
    for name in many_sets.SETS:
        planned.add(_model(_set(name)[0]).many_resume_kernel())
    assert planned == shipped_resume_kernels() and len(planned) == 6
