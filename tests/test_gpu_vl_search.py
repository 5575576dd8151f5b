"""Leaf-parallel search with virtual loss on the MI355X (azh_engine_set_leaf_batch): every iteration of the HIP engine
equals the numpy restatement (tests/vl_reference.py), the device loop equals host stepping, K = 1 is today's search, and
the UAI front-end searches exactly the visits it is asked for."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import link
from tests import engine_harness as eh
from tests import helpers
from tests import leaf_lockstep as lls
from tests import vl_reference as vlr
from tests.engine_harness import _positions

pytestmark = pytest.mark.gpu

ROOT = helpers.ROOT
UAI = lls.UAI


def _engine(G, K, VL, flags, blockers=0, visits=300, seed=11):
    return lls.engine(G, flags, blockers, visits, seed, start=_positions(G, blockers), leaf_batch=(K, VL))


CASES = [  # (G, K, VL, flags, blockers)
    (1, 2, 1, UAI, 0), (1, 64, 3, UAI, 0), (1, 16, 3, 0, 0), (5, 7, 3, 0, 0), (5, 16, 1, UAI, 0), (5, 64, 1, 0, 0),
    (5, 2, 3, UAI, 0), (5, 16, 3, 0, helpers.BLOCK4_MASK),
]
SEEN = {"collision": 0, "terminal": 0, "truncated": 0}


@pytest.mark.parametrize("G,K,VL,flags,blockers", CASES)
def test_every_iteration_equals_the_restatement(G, K, VL, flags, blockers):
    e, cfg = _engine(G, K, VL, flags, blockers)
    for rec in lls.LockStep(e, cfg, VL).until_due(past_due=False):
        for r in rec.games.values():
            k = len(r.batch.kind)
            SEEN["collision"] += r.batch.kind.count(vlr.LEAF_COLLISION)
            SEEN["terminal"] += r.batch.kind.count(vlr.LEAF_TERMINAL)
            SEEN["truncated"] += int(k < K and r.state.root_visits + k == cfg.visits)
    e.close()


def test_the_matrix_met_collisions_terminal_paths_and_truncation():
    assert SEEN["collision"] > 0 and SEEN["terminal"] > 0 and SEEN["truncated"] > 0, SEEN


@pytest.mark.parametrize("G,K,dtype", [(3, 16, link.DTYPE_F32), (3, 16, link.DTYPE_F16), (9, 64, link.DTYPE_BF16)])
def test_device_loop_equals_host_stepping(G, K, dtype):
    net = eh.net(2)
    n = 40
    a, _ = _engine(G, K, 2, 0, visits=200)
    b, _ = _engine(G, K, 2, 0, visits=200)
    a.run(net, n, dtype)
    a.sync()
    for _ in range(n):
        b.select()
        b.eval(net, dtype)
        b.backup()
    sa, ta = eh.dump(a)
    sb, tb = eh.dump(b)
    assert sa == sb
    for x, y in zip(ta, tb):
        for u, v in zip(x, y):
            assert (u == v).all()
    assert a.stats() == b.stats() and a.collisions() == b.collisions()
    assert a.stats()["plies"] > 0  # moves were played inside the loop (re-roots under K leaves per game)
    a.close(), b.close()


def test_k1_through_the_new_call_is_the_one_leaf_search_and_bad_combinations_fail():
    net = eh.net(2)
    a, _ = _engine(4, 1, 1, 0)
    b, cfg = lls.engine(4, start=_positions(4, 0))
    a.set_leaf_batch(8, 2)   # there and back again, between iterations
    a.set_leaf_batch(1, 1)
    a.run(net, 30, link.DTYPE_BF16)
    b.run(net, 30, link.DTYPE_BF16)
    sa, ta = eh.dump(a)
    sb, tb = eh.dump(b)
    assert sa == sb and all((u == v).all() for x, y in zip(ta, tb) for u, v in zip(x, y))
    # errors: the G-sized calls under K > 1, unsupported flags and budgets, bounds
    a.set_leaf_batch(4, 1)
    with pytest.raises(link.AzhError):
        a.leaves()
    with pytest.raises(link.AzhError):
        a.set_evals(np.zeros((4, 833), np.float32), np.zeros(4, np.float32))
    for bad in [(0, 1), (65, 1), (4, 0), (4, 17)]:
        with pytest.raises(link.AzhError):
            a.set_leaf_batch(*bad)
    for flags, budget in [(link.FLAG_TWO_NETS, 0), (link.FLAG_EVAL_CACHE, 0), (0, 4)]:
        cfg.flags, cfg.select_budget = flags, budget
        c = link.Engine(cfg)
        with pytest.raises(link.AzhError):
            c.set_leaf_batch(8, 1)
        c.set_leaf_batch(1, 1)
        c.close()
    a.close(), b.close()


def test_searcher_visits_sum_exactly(tmp_path):
    from ataxxzero_amd import uai
    s = uai.Searcher(lls.npy(tmp_path), dtype="f16", parallel_leaves=16)
    edges = s.root_visits(uai.Position.initial(), visits=200)
    assert sum(n for _, n in edges) == 200 and s.last_steps == 200
    edges = s.root_visits(uai.Position.initial(), seconds=0.05)
    assert sum(n for _, n in edges) == s.last_steps > 16


def test_cli_parallel_leaves_plays_legal_moves(tmp_path):
    net = lls.npy(tmp_path)
    script = "uai\nisready\nposition fen x5o/7/7/7/7/7/o5x x\ngo movetime 200\nmoves g2\ngo movetime 200\nquit\n"
    env = dict(os.environ)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "uai_interface.py"), "--network-path", net,
                          "--parallel-leaves", "16", "--virtual-loss", "2", "--visits", "64"],
                         input=script, capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    best = [l.split()[1] for l in out.stdout.splitlines() if l.startswith("bestmove")]
    assert len(best) == 2
    from ataxxzero_amd import uai
    pos = uai.Position.initial()
    legal, _ = pos.legal_moves()
    assert uai.decode_move(best[0]) in legal
    pos.move(uai.decode_move("g2"))
    legal, _ = pos.legal_moves()
    assert uai.decode_move(best[1]) in legal
