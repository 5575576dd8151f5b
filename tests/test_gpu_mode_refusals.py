"""Who refuses whom among the eight search modes of the engine (playout cap, forced playouts, Gumbel root search, temperature,
resign, random symmetry, leaf batch, solver), on the MI355X: every ordered pair of modes, every (mode, create-time cause)
cell, the selected-batch refusal of every setter, that a refused call changes nothing, and the leaf buffers across changes
of K and the solver.  A characterisation: the expected codes and messages are literals (include/ataxxzero_hip.h, "Search
modes: who refuses whom"), not produced by the library under test."""
import numpy as np
import pytest

from ataxxzero_amd import link
from oracle import oracle_lib as orc
from tests import helpers

pytestmark = pytest.mark.gpu

G, VISITS, PLIES = 4, 24, 400
TEMPS = np.ones(PLIES, dtype=np.float32)
ODD_BLOCKERS = 1 << 1      # one cell beside a corner: not its own image under the mirrors, and clear of the start position

# mode -> (setter, on-request, off-request, the phrase another setter's refusal names it by)
MODES = {
    "cap": ("azh_engine_set_playout_cap", lambda e: e.set_playout_cap(8, 16384), lambda e: e.set_playout_cap(0, 0),
            "the playout cap (azh_engine_set_playout_cap)"),
    "forced": ("azh_engine_set_forced_playouts", lambda e: e.set_forced_playouts(2.0), lambda e: e.set_forced_playouts(0.0),
               "forced playouts (azh_engine_set_forced_playouts)"),
    "gumbel": ("azh_engine_set_gumbel", lambda e: e.set_gumbel(4), lambda e: e.set_gumbel(0),
               "the Gumbel root search (azh_engine_set_gumbel)"),
    "temperature": ("azh_engine_set_temperature", lambda e: e.set_temperature(TEMPS, None), lambda e: e.set_temperature(None, None),
                    "a temperature table (azh_engine_set_temperature)"),
    "resign": ("azh_engine_set_resign", lambda e: e.set_resign(0.1, 2, 0), lambda e: e.set_resign(0.0, 0, 0), None),
    "symmetry": ("azh_engine_set_random_symmetry", lambda e: e.set_random_symmetry(True), lambda e: e.set_random_symmetry(False),
                 None),
    "leaf": ("azh_engine_set_leaf_batch", lambda e: e.set_leaf_batch(4, 1), lambda e: e.set_leaf_batch(1, 1),
             "more than one leaf per game (azh_engine_set_leaf_batch)"),
    "solver": ("azh_engine_set_solver", lambda e: e.set_solver(True), lambda e: e.set_solver(False), "the solver"),
}
# what a refusal of the mode's own setter says before the cause
REFUSAL = {m: "not supported with " for m in MODES}
REFUSAL["leaf"] = "more than one leaf per game is not supported with "
REFUSAL["solver"] = "the solver is not supported with "
# the excluded pairs, unordered
EXCLUDED = {frozenset(p) for p in [("gumbel", "cap"), ("gumbel", "forced"), ("gumbel", "temperature"), ("gumbel", "leaf"),
                                   ("gumbel", "solver"), ("forced", "leaf"), ("forced", "solver")]}

GUMBEL_NEEDS = ("azh_engine_set_gumbel: the engine must have been created with AZH_FLAG_NO_REUSE and dirichlet_weight 0 "
                "(the schedule assumes a fresh root, and its noise is the Gumbel)")
ODD_BLOCKERS_CAUSE = ("a blockers mask (0x2) that is not its own image under all 8 symmetries (the tower takes one blocker "
                      "plane per launch)")
FLAGS = {"AZH_FLAG_TWO_NETS": link.FLAG_TWO_NETS, "AZH_FLAG_ONE_RANDOM_MOVE": link.FLAG_ONE_RANDOM_MOVE,
         "AZH_FLAG_SAMPLE_POW5": link.FLAG_SAMPLE_POW5, "AZH_FLAG_PY_POSTERIOR": link.FLAG_PY_POSTERIOR,
         "AZH_FLAG_EVAL_CACHE": link.FLAG_EVAL_CACHE, "AZH_FLAG_SYMMETRY_AVG": link.FLAG_SYMMETRY_AVG}
REFUSED_FLAGS = {
    "leaf": ("AZH_FLAG_TWO_NETS", "AZH_FLAG_EVAL_CACHE", "AZH_FLAG_SYMMETRY_AVG"),
    "solver": ("AZH_FLAG_TWO_NETS", "AZH_FLAG_EVAL_CACHE", "AZH_FLAG_SYMMETRY_AVG"),
    "cap": ("AZH_FLAG_TWO_NETS", "AZH_FLAG_ONE_RANDOM_MOVE"),
    "forced": ("AZH_FLAG_TWO_NETS", "AZH_FLAG_ONE_RANDOM_MOVE"),
    "gumbel": ("AZH_FLAG_TWO_NETS", "AZH_FLAG_ONE_RANDOM_MOVE", "AZH_FLAG_SAMPLE_POW5", "AZH_FLAG_EVAL_CACHE"),
    "resign": ("AZH_FLAG_TWO_NETS", "AZH_FLAG_ONE_RANDOM_MOVE"),
    "temperature": ("AZH_FLAG_ONE_RANDOM_MOVE", "AZH_FLAG_SAMPLE_POW5", "AZH_FLAG_PY_POSTERIOR", "AZH_FLAG_TWO_NETS"),
    "symmetry": ("AZH_FLAG_TWO_NETS", "AZH_FLAG_SYMMETRY_AVG"),
}
# (mode, engine arguments, the whole message) of every cell of the table: the flags, then the causes that are not flags
CELLS = [(m, dict(flags=link.FLAG_NO_REUSE | FLAGS[f]), "%s: %s%s" % (MODES[m][0], REFUSAL[m], f))
         for m in MODES for f in REFUSED_FLAGS[m]]
CELLS += [(m, dict(select_budget=4), "%s: %sselect_budget > 0" % (MODES[m][0], REFUSAL[m])) for m in ("leaf", "solver")]
CELLS += [("gumbel", dict(flags=0), GUMBEL_NEEDS), ("gumbel", dict(dirichlet_weight=0.25), GUMBEL_NEEDS),
          ("symmetry", dict(blockers=ODD_BLOCKERS), "azh_engine_set_random_symmetry: not supported with " + ODD_BLOCKERS_CAUSE)]


def _engine(flags=link.FLAG_NO_REUSE, dirichlet_weight=0.0, select_budget=0, blockers=0, seed=7):
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    cfg = link.Config(games=G, visits=VISITS, max_plies=PLIES, edges_per_node=96, c_puct=1.0, dirichlet_alpha=0.15,
                      dirichlet_weight=dirichlet_weight, start_turn=0, seed=seed, start_x=int(p.pieces[0]),
                      start_o=int(p.pieces[1]), blockers=blockers, flags=flags, select_budget=select_budget)
    return link.Engine(cfg)


def _refused(call, e, code, message):
    with pytest.raises(link.AzhError) as ei:
        call(e)
    assert str(ei.value) == "ataxxzero_hip error %d: %s" % (code, message)


def _select(e, leaf_parallel=False):
    """select and hand the batch its evaluations; the backup is the caller's"""
    e.select()
    if leaf_parallel:
        kind, lb, edge = e.batch_leaves()
        assert kind.shape == edge.shape == (G, e.K) and lb.shape == (G, e.K, 2)
        e.set_batch_evals(*helpers.synthetic_evals_distinct(lb.reshape(-1, 2)))
    else:
        need, lb = e.leaves()
        assert need.shape == (G,) and lb.shape == (G, 2)
        e.set_evals(*helpers.synthetic_evals_distinct(lb))


def _step(e, iterations, leaf_parallel=False):
    for _ in range(iterations):
        _select(e, leaf_parallel)
        e.backup()


def _assert_equal(a, b):
    for g in range(G):
        assert a.game_state(g).as_tuple() == b.game_state(g).as_tuple()
        for x, y in zip(a.tree(g), b.tree(g)):
            assert x.shape == y.shape and (x == y).all()


@pytest.mark.parametrize("a", list(MODES))
def test_every_ordered_pair_of_modes(a):
    for b in MODES:
        if b == a:
            continue
        e = _engine()
        MODES[a][1](e)
        if frozenset((a, b)) in EXCLUDED:
            _refused(MODES[b][1], e, -4, "%s: %s%s" % (MODES[b][0], REFUSAL[b], MODES[a][3]))
        else:
            MODES[b][1](e)
        MODES[a][2](e)
        MODES[b][1](e)
        MODES[b][2](e)
        e.close()


def test_gumbel_beside_the_root_policy_table_alone():
    e = _engine()
    e.set_temperature(None, TEMPS)
    _refused(MODES["gumbel"][1], e, -4, "azh_engine_set_gumbel: not supported with " + MODES["temperature"][3])
    e.set_temperature(None, None)
    e.set_gumbel(4)
    _refused(lambda x: x.set_temperature(None, TEMPS), e, -4,
             "azh_engine_set_temperature: not supported with " + MODES["gumbel"][3])
    e.close()


@pytest.mark.parametrize("mode,kwargs,message", CELLS, ids=["%s-%d" % (c[0], i) for i, c in enumerate(CELLS)])
def test_every_create_time_cause(mode, kwargs, message):
    e = _engine(**kwargs)
    _refused(MODES[mode][1], e, -4, message)
    MODES[mode][2](e)                 # switching off is no request for the mode
    if not kwargs.get("flags", 0) & link.FLAG_TWO_NETS:
        _step(e, 3)
    e.close()


def test_several_causes_name_one_of_them():
    e = _engine(flags=link.FLAG_NO_REUSE | link.FLAG_ONE_RANDOM_MOVE | link.FLAG_TWO_NETS)
    with pytest.raises(link.AzhError) as ei:
        e.set_temperature(TEMPS, None)
    assert str(ei.value) in ["ataxxzero_hip error -4: azh_engine_set_temperature: not supported with " + f
                             for f in ("AZH_FLAG_ONE_RANDOM_MOVE", "AZH_FLAG_TWO_NETS")]
    e.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_a_selected_batch_refuses_on_and_off(mode):
    setter, on, off, _ = MODES[mode]
    e = _engine()
    _select(e)
    _refused(on, e, -3, setter + ": a selected batch awaits its backup")
    _refused(off, e, -3, setter + ": a selected batch awaits its backup")
    e.backup()
    on(e)
    off(e)
    e.close()


# setter -> (engine arguments, the mode that is on beside it) under which its on-request is refused and the engine steps
REFUSING = {"cap": ({}, "gumbel"), "forced": ({}, "gumbel"), "gumbel": ({}, "forced"), "temperature": ({}, "gumbel"),
            "resign": (dict(flags=link.FLAG_NO_REUSE | link.FLAG_ONE_RANDOM_MOVE), None),
            "symmetry": (dict(blockers=ODD_BLOCKERS), None), "leaf": ({}, "forced"), "solver": ({}, "forced")}


@pytest.mark.parametrize("mode", list(MODES))
def test_a_refused_call_changes_nothing(mode):
    kwargs, beside = REFUSING[mode]
    e, twin = _engine(**kwargs), _engine(**kwargs)
    for x in (e, twin):
        if beside:
            MODES[beside][1](x)
        _step(x, 3)
    with pytest.raises(link.AzhError) as ei:
        MODES[mode][1](e)
    assert str(ei.value).startswith("ataxxzero_hip error -4: " + MODES[mode][0] + ": ")
    for _ in range(10):
        _step(e, 3), _step(twin, 3)
        _assert_equal(e, twin)
    assert e.stats() == twin.stats() and e.stats()["plies"] > 0    # (30 iterations at 24 visits: past a move)
    e.close(), twin.close()


def test_leaf_buffers_across_k_and_the_solver():
    """K 4, 1, 4, the solver on, K 8 (larger buffers), the solver off, K 1: the batch has the shape of the search in force
    after every change, and the engine ends equal to a twin whose G K-slot buffers had their largest size from the start and
    which reached every setting by the other order of the two calls."""
    e, twin = _engine(), _engine()
    twin.set_leaf_batch(8, 1)
    twin.set_leaf_batch(1, 1)
    changes = [(lambda x: x.set_leaf_batch(4, 1), 4, False), (lambda x: x.set_leaf_batch(1, 1), 1, False),
               (lambda x: x.set_leaf_batch(4, 1), 4, False), (lambda x: x.set_solver(True), 4, True),
               (lambda x: x.set_leaf_batch(8, 1), 8, True), (lambda x: x.set_solver(False), 8, False),
               (lambda x: x.set_leaf_batch(1, 1), 1, False)]
    for change, K, solver in changes:
        change(e)
        twin.set_solver(solver)
        twin.set_leaf_batch(K, 1)
        parallel = K > 1 or solver
        for x in (e, twin):
            assert x.K == K
            _step(x, 4, parallel)
            if parallel:
                _refused(lambda y: y.leaves(), x, -2, "azh_engine_leaves: %d leaves per game%s: use azh_engine_batch_leaves"
                         % (K, " with the solver" if solver else ""))
            else:
                _refused(lambda y: y.batch_leaves(), x, -2, "azh_engine_batch_leaves: one leaf per game: use azh_engine_leaves")
        _assert_equal(e, twin)
    assert e.stats() == twin.stats() and e.stats()["plies"] > 0    # (4 iterations of 4, 1, 4, 4, 8, 8 and 1 leaves: 120 visits)
    e.close(), twin.close()
