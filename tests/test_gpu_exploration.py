"""First-play urgency and the growing exploration rate in the leaf-parallel search on the MI355X
(azh_engine_set_exploration): every iteration of the HIP engine equals the numpy restatement
(tests/exploration_reference.py) — over late positions and from the start position, with the solver off and on, over nodes
of more than 64, 128 and 192 edges — the mode changes what is selected, off is off, the device loop equals host stepping
across re-roots, every cell of the mode table's new row refuses in the table's words, and the UAI front-end plays legal
moves with the options set."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import link, model
from tests import engine_harness as eh
from tests import exploration_reference as xr
from tests import helpers
from tests import leaf_lockstep as lls

pytestmark = pytest.mark.gpu

ROOT = helpers.ROOT
UAI = lls.UAI
FPU, RATE, BOTH = (0.25, 0.0, 0.0), (-1.0, 19652.0, 1.25), (0.25, 19652.0, 1.25)
PARAMS = [FPU, RATE, BOTH]
SHAPES = [(1, 1, 1, UAI, 0), (1, 64, 3, UAI, 0), (5, 7, 3, 0, helpers.BLOCK4_MASK), (5, 64, 1, 0, 0)]   # (G, K, VL, flags, blockers)
# (shape, parameters, family, solver): late positions (few empty cells: finished nodes, short games) and the start position
# (levels with N == 0 and with few visited children under wide nodes); one case with the solver on
CASES = [(shape, params, family, False) for family in ("late", "start") for shape in SHAPES for params in PARAMS]
CASES.append(((5, 7, 3, 0, helpers.BLOCK4_MASK), BOTH, "late", True))


def _engine(G, K, VL, flags, blockers=0, visits=160, seed=11, params=None, solver=False, family="late"):
    return lls.engine(G, flags, blockers, visits, seed, start=family, leaf_batch=(K, VL), solver=solver, exploration=params)


_RESULTS = {}   # case -> what it met: every case runs once per session, whoever asks first


def _case(case):
    return lls.memo(_RESULTS, case, lambda: _lock_step(*case))


def _lock_step(shape, params, family, solver, limit=400, **more):
    """The engine against the restatement, iteration by iteration, until every game's move is due.  -> what the run met."""
    G, K, VL, flags, blockers = shape
    seen = {"differs": 0, "zero_levels": 0, "sparse_levels": 0, "fpu_picks": 0, "idx64": 0, "idx128": 0, "idx192": 0, "proven": 0}
    e, cfg = _engine(G, K, VL, flags, blockers, params=params, solver=solver, family=family, **more)
    assert e.exploration() == tuple(float(np.float32(v)) for v in params)
    ls = lls.LockStep(e, cfg, VL, solver=solver)
    for rec in ls.until_due(limit):
        for r in rec.games.values():
            off = ls.select(r.pre, r.state.root_visits, dict(r.settings, fpu_reduction=-1.0, c_base=0.0))
            seen["differs"] += int(off.leaf_edge != r.batch.leaf_edge)   # what the search selects with the mode off
            seen["proven"] += len(r.proven)
            _levels(r.batch, r.pre, seen)
    e.close()
    return seen


def _levels(b, pre, seen):
    """What the batch's first path met, level by level, on the tree before the batch (no virtual loss yet): levels without
    a visit (N == 0), levels with at most two visited children under more unvisited ones, picks of an unvisited child beside
    a visited one; and the lane round of every edge the batch took."""
    edges, node = pre[2], 0
    for ed in b.paths[0]:
        first, M = b.info[node][0], b.info[node][1] & 0xFFFF
        if first + M <= len(edges):
            n = edges[first:first + M, 1]
            visited = int((n > 0).sum())
            seen["zero_levels"] += visited == 0
            seen["sparse_levels"] += 0 < visited <= 2 < M
            seen["fpu_picks"] += visited > 0 and int(n[ed - first]) == 0
        node = b.child[ed]
    for key, count in zip(("idx64", "idx128", "idx192"), lls.lane_rounds(b)):
        seen[key] += count


@pytest.mark.parametrize("case", CASES, ids=["%s-G%dK%dVL%d-%d%s" % (c[2], c[0][0], c[0][1], c[0][2], PARAMS.index(c[1]),
                                                                    "-solver" if c[3] else "") for c in CASES])
def test_every_iteration_equals_the_restatement(case):
    _case(case)


def test_the_matrix_met_empty_and_sparse_levels_and_proofs():
    seen = [_case(case) for case in CASES]
    total = {k: sum(s[k] for s in seen) for k in seen[0]}
    assert total["zero_levels"] > 0 and total["sparse_levels"] > 0 and total["fpu_picks"] > 0 and total["proven"] > 0, total


def test_the_mode_differs_from_off():
    """Over the late family: batches whose leaf edges are not what the search selects on the same tree with the mode off —
    for each of the three parameter sets."""
    for params in PARAMS:
        differs = sum(_case(case)["differs"] for case in CASES if case[2] == "late" and case[1] == params and not case[3])
        assert differs > 0, params


# ------------------------------------------------------------------ wide nodes

_WIDE = {}


def _wide():
    if "seen" not in _WIDE:
        roots = eh._wide_roots()
        _WIDE["seen"] = _lock_step((len(roots), 8, 3, 0, 0), BOTH, roots, False, limit=200, visits=48, seed=20261109)
    return _WIDE["seen"]


def test_nodes_of_65_to_193_edges():
    _wide()


def test_the_wide_case_selected_edges_in_every_round_of_lanes():
    """(so the two sums ran over every round: a term left out of a round changes f, and with it every unvisited child's
    score at that node)"""
    seen = _wide()
    assert seen["idx64"] > 0 and seen["idx128"] > 0 and seen["idx192"] > 0, seen


# ------------------------------------------------------------------ off is off


def _one_leaf_iteration(e, net, dtype):
    e.select()
    e.leaves()
    e.eval(net, dtype)
    e.backup()


def test_switched_on_and_off_again_is_an_untouched_engine():
    net = eh.net(2)
    a, _ = _engine(4, 1, 1, 0, visits=24)
    b, _ = _engine(4, 1, 1, 0, visits=24)
    a.set_leaf_batch(8, 2)
    a.set_exploration(*BOTH)
    assert a.exploration() == tuple(float(np.float32(v)) for v in BOTH)
    a.set_exploration(*xr.OFF)
    a.set_leaf_batch(1, 1)
    assert a.exploration() == xr.OFF == b.exploration()
    a.run(net, 60, link.DTYPE_BF16)
    b.run(net, 60, link.DTYPE_BF16)
    eh.same(eh.dump(a, raw=True), eh.dump(b, raw=True))
    assert a.stats() == b.stats() and a.stats()["plies"] > 0
    # the one-leaf calls are back, and the batch calls are not
    for x in (a, b):
        _one_leaf_iteration(x, net, link.DTYPE_BF16)
        with pytest.raises(link.AzhError) as ei:
            x.batch_leaves()
        assert str(ei.value) == "ataxxzero_hip error -2: azh_engine_batch_leaves: one leaf per game: use azh_engine_leaves"
    eh.same(eh.dump(a, raw=True), eh.dump(b, raw=True))
    # and K = 1 with the mode on runs through the batch calls
    a.set_exploration(*FPU)
    with pytest.raises(link.AzhError) as ei:
        a.leaves()
    assert str(ei.value) == ("ataxxzero_hip error -2: azh_engine_leaves: 1 leaves per game with azh_engine_set_exploration: "
                             "use azh_engine_batch_leaves")
    a.select()
    kind, lb, _ = a.batch_leaves()
    assert kind.shape == (4, 1)
    a.set_batch_evals(*helpers.synthetic_evals_distinct(lb.reshape(-1, 2)))
    a.backup()
    a.close(), b.close()


@pytest.mark.parametrize("K,dtype", [(1, link.DTYPE_F32), (16, link.DTYPE_F16)])
def test_device_loop_equals_host_stepping_across_re_roots(K, dtype):
    net = eh.net(2)
    n = 100 if K == 1 else 30
    a, _ = _engine(2, K, 2, 0, visits=64, params=BOTH)
    b, _ = _engine(2, K, 2, 0, visits=64, params=BOTH)
    a.run(net, n, dtype)
    a.sync()
    for _ in range(n):
        b.select()
        b.eval(net, dtype)
        b.backup()
    eh.same(eh.dump(a, raw=True), eh.dump(b, raw=True))
    assert a.stats() == b.stats() and a.stats()["plies"] > 0    # (moves were played inside the loop: re-roots with the mode on)
    a.close(), b.close()


# ------------------------------------------------------------------ refusals: the ninth row of the mode table

SETTER = "azh_engine_set_exploration"
PHRASE = "first-play urgency or a growing exploration rate (azh_engine_set_exploration)"


@pytest.mark.parametrize("kwargs,cause", [(dict(flags=link.FLAG_NO_REUSE | link.FLAG_TWO_NETS), "AZH_FLAG_TWO_NETS"),
                                          (dict(flags=link.FLAG_NO_REUSE | link.FLAG_EVAL_CACHE), "AZH_FLAG_EVAL_CACHE"),
                                          (dict(flags=link.FLAG_NO_REUSE | link.FLAG_SYMMETRY_AVG), "AZH_FLAG_SYMMETRY_AVG"),
                                          (dict(flags=link.FLAG_NO_REUSE, select_budget=4), "select_budget > 0")])
def test_every_create_time_cause(kwargs, cause):
    cfg = lls.config(4, kwargs.pop("flags"), visits=24, seed=7, **kwargs)
    e = link.Engine(cfg)
    for params in PARAMS:
        lls.refused(lambda: e.set_exploration(*params), -4, "%s: not supported with %s" % (SETTER, cause))
        assert e.exploration() == xr.OFF
    e.set_exploration(*xr.OFF)     # switching off is no request for the mode
    e.close()


def test_gumbel_and_forced_playouts_in_both_orders():
    others = {"gumbel": ("azh_engine_set_gumbel", lambda e: e.set_gumbel(4), lambda e: e.set_gumbel(0),
                         "the Gumbel root search (azh_engine_set_gumbel)"),
              "forced": ("azh_engine_set_forced_playouts", lambda e: e.set_forced_playouts(2.0),
                         lambda e: e.set_forced_playouts(0.0), "forced playouts (azh_engine_set_forced_playouts)")}
    for setter, on, off, phrase in others.values():
        e = link.Engine(lls.config(4, link.FLAG_NO_REUSE, visits=24, seed=7))
        on(e)
        lls.refused(lambda: e.set_exploration(*FPU), -4, "%s: not supported with %s" % (SETTER, phrase))
        assert e.exploration() == xr.OFF
        off(e)
        e.set_exploration(*RATE)
        lls.refused(lambda: on(e), -4, "%s: not supported with %s" % (setter, PHRASE))
        e.set_exploration(*xr.OFF)
        on(e)
        off(e)
        e.close()


def test_it_composes_with_the_other_modes():
    e = link.Engine(lls.config(4, link.FLAG_NO_REUSE, visits=24, seed=7))
    e.set_exploration(*BOTH)
    e.set_leaf_batch(4, 2)
    e.set_solver(True)
    e.set_playout_cap(8, 16384)
    e.set_temperature(np.ones(400, dtype=np.float32), None)
    e.set_resign(0.1, 2, 0)
    e.set_random_symmetry(True)
    for _ in range(30):
        e.select()
        kind, lb, _ = e.batch_leaves()
        assert kind.shape == (4, 4)
        e.set_batch_evals(*helpers.synthetic_evals_distinct(lb.reshape(-1, 2)))
        e.backup()
    assert e.stats()["plies"] > 0
    e.close()


def test_a_selected_batch_bad_arguments_and_an_unchanged_engine():
    e = link.Engine(lls.config(4, link.FLAG_NO_REUSE, visits=24, seed=7))
    twin = link.Engine(lls.config(4, link.FLAG_NO_REUSE, visits=24, seed=7))
    for x in (e, twin):
        x.set_exploration(*FPU)
    bad = [(np.nan, 0.0, 0.0), (0.25, np.nan, 0.0), (0.25, 1.0, np.nan), (np.inf, 0.0, 0.0), (-np.inf, 0.0, 0.0),
           (0.25, np.inf, 0.0), (0.25, 1.0, np.inf), (0.25, -1.0, 0.0), (0.25, 1.0, -0.5)]
    for args in bad:
        lls.refused(lambda: e.set_exploration(*args), -2, SETTER + ": need finite arguments, c_base >= 0 and c_init >= 0")
        assert e.exploration() == FPU
    e.select()
    kind, lb, _ = e.batch_leaves()
    for args in (BOTH, xr.OFF):      # requests and switching off alike
        lls.refused(lambda: e.set_exploration(*args), -3, SETTER + ": a selected batch awaits its backup")
        assert e.exploration() == FPU
    lls.refused(lambda: e.set_exploration(np.nan, 0.0, 0.0), -2, SETTER + ": need finite arguments, c_base >= 0 and c_init >= 0")
    e.set_batch_evals(*helpers.synthetic_evals_distinct(lb.reshape(-1, 2)))
    e.backup()
    eh.step(twin, K=2)               # (K = 2: any K but 1 takes the batch calls; here K is 1 under the mode)
    for _ in range(30):
        eh.step(e, K=2), eh.step(twin, K=2)
    eh.same(eh.dump(e, raw=True), eh.dump(twin, raw=True))
    assert e.stats() == twin.stats() and e.stats()["plies"] > 0
    # (-1, 0, c_init): nothing is on, and c_init is not kept
    e.set_exploration(-1.0, 0.0, 5.0)
    assert e.exploration() == xr.OFF
    e.set_exploration(-3.0, 2.0, 0.5)
    assert e.exploration() == (-1.0, 2.0, 0.5)
    e.close(), twin.close()


def test_the_header_holds_the_row():
    with open(os.path.join(ROOT, "include", "ataxxzero_hip.h")) as f:
        text = " ".join(f.read().replace(" *", " ").split())
    assert "Nine modes are switched" in text
    assert "exploration fpu_reduction >= 0 || TWO_NETS, EVAL_CACHE, SYMMETRY_AVG; select_budget > 0 Gumbel, forced playouts" in text
    assert '"first-play urgency or a growing exploration rate (azh_engine_set_exploration)"' in text


# ------------------------------------------------------------------ the front-end


@pytest.mark.parametrize("more", [[], ["--parallel-leaves", "16", "--solver", "--reuse-tree"]], ids=["k1", "k16-solver-reuse"])
def test_cli_plays_legal_moves(tmp_path, more):
    from ataxxzero_amd import uai
    script = "uai\nisready\nposition fen x5o/7/7/7/7/7/o5x x\ngo movetime 200\nmoves g2\ngo movetime 200\nquit\n"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "uai_interface.py"), "--network-path", lls.npy(tmp_path),
                          "--fpu-reduction", "0.25", "--cpuct-base", "19652", "--cpuct-init", "1.25", "--visits", "64"] + more,
                         input=script, capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ))
    assert out.returncode == 0, out.stderr[-2000:]
    best = [l.split()[1] for l in out.stdout.splitlines() if l.startswith("bestmove")]
    assert len(best) == 2
    pos = uai.Position.initial()
    legal, _ = pos.legal_moves()
    assert uai.decode_move(best[0]) in legal
    pos.move(uai.decode_move("g2"))
    legal, _ = pos.legal_moves()
    assert uai.decode_move(best[1]) in legal


def test_searcher_refuses_symmetry_averaging_before_any_device_call(tmp_path, monkeypatch):
    from ataxxzero_amd import uai
    touched = []
    monkeypatch.setattr(link, "Net", lambda *a, **k: touched.append("net"))
    monkeypatch.setattr(link, "Engine", lambda *a, **k: touched.append("engine"))
    monkeypatch.setattr(model, "load_model", lambda *a, **k: touched.append("load"))
    for kwargs in (dict(fpu_reduction=0.2), dict(cpuct_base=19652.0, cpuct_init=1.25)):
        with pytest.raises(ValueError, match="symmetry averaging is not available with fpu_reduction or cpuct_base"):
            uai.Searcher(str(tmp_path / "absent.npy"), symmetry_average=True, **kwargs)
    assert touched == []


def test_searcher_visits_sum_exactly_at_k1(tmp_path):
    from ataxxzero_amd import uai
    s = uai.Searcher(lls.npy(tmp_path), dtype="f16", fpu_reduction=0.25, cpuct_base=19652.0, cpuct_init=1.25)
    edges = s.root_visits(uai.Position.initial(), visits=100)
    assert sum(n for _, n in edges) == 100 and s.last_steps == 100
