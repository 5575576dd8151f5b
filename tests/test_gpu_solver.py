"""Proven wins and losses in the leaf-parallel search on the MI355X (azh_engine_set_solver): every iteration of the HIP
engine equals the numpy restatement (tests/solver_reference.py) — proofs, marks and all — the device loop equals host
stepping across re-roots, switching the solver on and off again changes nothing, and the UAI front-end plays the move it
has proven."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import link
from oracle import oracle_lib as orc
from tests import engine_harness as eh
from tests import helpers
from tests import leaf_lockstep as lls
from tests import solver_reference as sr

pytestmark = pytest.mark.gpu

ROOT = helpers.ROOT
UAI = lls.UAI


def _engine(G, K, VL, flags, blockers=0, visits=300, seed=11, solver=True):
    return lls.engine(G, flags, blockers, visits, seed, leaf_batch=(K, VL), solver=solver)


CASES = [  # (G, K, VL, flags, blockers)
    (1, 1, 1, UAI, 0), (1, 7, 3, 0, 0), (1, 64, 3, UAI, 0), (5, 1, 1, 0, 0), (5, 7, 1, UAI, 0), (5, 64, 1, 0, 0),
    (5, 7, 3, UAI, helpers.BLOCK4_MASK), (5, 64, 3, 0, helpers.BLOCK4_MASK),
]
_RESULTS = {}   # case -> what it met: every case runs once per session, whoever asks first


def _case(case):
    return lls.memo(_RESULTS, case, lambda: _lock_step(*case))


@pytest.mark.parametrize("case", CASES)
def test_every_iteration_equals_the_restatement(case):
    _case(case)


def _lock_step(G, K, VL, flags, blockers):
    SEEN = {"win": 0, "loss": 0, "chained": 0, "root": 0, "hits": 0}
    e, cfg = _engine(G, K, VL, flags, blockers, visits=160)
    nodes = 0
    for rec in lls.LockStep(e, cfg, VL, solver=True, root_proofs=True).until_due():
        for r in rec.games.values():
            SEEN["hits"] += r.batch.proven_hits
            nodes += len(r.proven)
            for node, value, _, levels in r.proven:
                SEEN["win" if value == 1 else "loss"] += 1
                SEEN["chained"] += int(levels > 1)
                SEEN["root"] += int(node == 0)
    assert e.proof_stats() == {"proven_nodes": nodes, "proven_hits": SEEN["hits"]}
    e.close()
    return SEEN


def test_the_matrix_met_win_loss_chained_and_root_proofs():
    seen = [_case(case) for case in CASES]
    total = {k: sum(s[k] for s in seen) for k in seen[0]}
    assert all(v > 0 for v in total.values()), total


def _same(x, y):
    return x[0] == y[0] and all((u == v).all() for a, b in zip(x[1], y[1]) for u, v in zip(a, b)) and \
        all((u == v).all() for u, v in zip(x[2], y[2]))


def _subtree(tree, root):
    """The subtree of node `root` as the re-root leaves it: nodes breadth-first in (parent, edge) order, a node's edges at
    the running edge count (tests/test_gpu_play_moves.py does the same) -> (boards, info, edges, moves)."""
    boards, info, edges, moves = tree
    order, at = [root], 0
    nb, ni, ne, nm = [], [], [], []
    while at < len(order):
        old = order[at]
        first, M = int(info[old, 0]), int(info[old, 1] & 0xFFFF)
        nb.append(boards[old])
        ni.append([len(ne) if M else 0, int(info[old, 1]), 0, int(info[old, 3])])
        for j in range(M):
            row = [int(v) for v in edges[first + j]]
            if row[3] != sr.NONE:
                order.append(row[3])
                row[3] = len(order) - 1
            ne.append(row)
            nm.append(int(moves[first + j]))
        at += 1
    return (np.array(nb, np.uint64).reshape(-1, 2), np.array(ni, np.uint32).reshape(-1, 4),
            np.array(ne, np.uint32).reshape(-1, 4), np.array(nm, np.uint16))


LOOPS = [(3, 1, link.DTYPE_F32, 30, 100), (3, 16, link.DTYPE_F16, 100, 60), (9, 64, link.DTYPE_BF16, 100, 60)]
_LOOP_RESULTS = {}


def _loop(case):
    return lls.memo(_LOOP_RESULTS, case, lambda: _device_loop(*case))


@pytest.mark.parametrize("case", LOOPS)
def test_device_loop_equals_host_stepping_and_proofs_survive_re_roots(case):
    _loop(case)


def _device_loop(G, K, dtype, visits, n):
    net = eh.net(2)
    a, _ = _engine(G, K, 2, 0, visits=visits)
    b, _ = _engine(G, K, 2, 0, visits=visits)
    a.run(net, n, dtype)
    a.sync()
    carried = 0
    for _ in range(n):
        before = [(b.game_state(g), b.tree(g)) for g in range(G)]
        b.select()   # (plays the moves that are due: the re-root)
        for g, (s0, t0) in enumerate(before):
            s1 = b.game_state(g)
            if s0.phase == 2 and s1.ply == s0.ply + 1 and s1.n_nodes > 1:
                # the kept subtree, marks included, is the old tree's subtree of the new root
                t1 = b.tree(g)
                first, M = int(t0[1][0, 0]), int(t0[1][0, 1] & 0xFFFF)
                kids = [int(c) for c in t0[2][first:first + M, 3] if int(c) != sr.NONE and
                        (t0[0][int(c)] == t1[0][0]).all()]
                assert kids
                exp = _subtree(t0, kids[0])
                assert all(x.shape == y.shape and (x == y).all() for x, y in zip(exp, t1))
                assert ((b.tree_raw(g)[:, 3] >> 31) == sr.finished_bits(t1)).all()
                carried += sum(1 for row in t1[1] if sr.is_proven(row))
        b.eval(net, dtype)
        b.backup()
    assert _same(eh.dump(a, raw=True), eh.dump(b, raw=True))
    assert a.stats() == b.stats() and a.proof_stats() == b.proof_stats()
    assert a.stats()["plies"] > 0 and a.proof_stats()["proven_nodes"] > 0
    a.close(), b.close()
    return carried


def test_proven_nodes_were_carried_into_new_trees():
    assert sum(_loop(case) for case in LOOPS) > 0


def test_play_moves_carries_the_marks():
    net = eh.net(2)
    e, cfg = _engine(2, 16, 2, 0, visits=400)
    e.run(net, 12, link.DTYPE_F32)
    e.sync()
    moved = 0
    for g in range(2):
        t0 = e.tree(g)
        first, M = int(t0[1][0, 0]), int(t0[1][0, 1] & 0xFFFF)
        best = max(range(M), key=lambda j: int(t0[2][first + j, 1]))
        child = int(t0[2][first + best, 3])
        if child == sr.NONE or e.game_state(g).phase != 1:
            continue
        mv = np.full(2, link.NO_MOVE, np.uint16)
        mv[g] = t0[3][first + best]
        status = e.play_moves(mv)[g]
        assert status in (link.PLAY_KEPT, link.PLAY_FINISHED)
        t1 = e.tree(g)
        assert all(x.shape == y.shape and (x == y).all() for x, y in zip(_subtree(t0, child), t1))
        assert ((e.tree_raw(g)[:, 3] >> 31) == sr.finished_bits(t1)).all()
        assert e.root_proofs(g, 1)[0][0] == sr.decided_value(t1[1][0])
        moved += 1
    assert moved > 0
    e.close()


def test_switched_on_and_off_again_is_an_untouched_engine():
    net = eh.net(2)
    for K in (1, 16):
        a, _ = _engine(4, K, 2, 0, solver=False)
        b, _ = _engine(4, K, 2, 0, solver=False)
        a.set_solver(True)
        a.set_solver(False)
        a.run(net, 30, link.DTYPE_BF16)
        b.run(net, 30, link.DTYPE_BF16)
        assert _same(eh.dump(a, raw=True), eh.dump(b, raw=True)) and a.stats() == b.stats()
        assert a.proof_stats() == {"proven_nodes": 0, "proven_hits": 0}
        if K == 1:   # the one-leaf calls are back
            a.select()
            a.leaves()
            a.eval(net, link.DTYPE_BF16)
            a.backup()
        a.close(), b.close()


def test_refusals():
    cfg = lls.config(4)
    for flags, budget, word in [(link.FLAG_TWO_NETS, 0, "AZH_FLAG_TWO_NETS"), (link.FLAG_EVAL_CACHE, 0, "AZH_FLAG_EVAL_CACHE"),
                                (link.FLAG_SYMMETRY_AVG, 0, "AZH_FLAG_SYMMETRY_AVG"), (0, 4, "select_budget > 0")]:
        cfg.flags, cfg.select_budget = flags, budget
        c = link.Engine(cfg)
        with pytest.raises(link.AzhError) as ei:
            c.set_solver(True)
        assert "the solver is not supported with " + word in str(ei.value)
        c.set_solver(False)
        c.close()
    cfg.flags, cfg.select_budget = 0, 0
    c = link.Engine(cfg)
    c.set_solver(True)
    # K = 1 under the solver runs through the batch calls
    with pytest.raises(link.AzhError):
        c.leaves()
    with pytest.raises(link.AzhError):
        c.set_evals(np.zeros((4, 833), np.float32), np.zeros(4, np.float32))
    c.select()
    kind, lb, le = c.batch_leaves()
    assert kind.shape == (4, 1)
    with pytest.raises(link.AzhError):   # between iterations only
        c.set_solver(False)
    c.set_batch_evals(*helpers.synthetic_evals_distinct(lb.reshape(-1, 2)))
    c.backup()
    c.set_solver(False)
    c.leaves()
    c.close()


def _mates():
    """Blocker-free fixture positions whose side to move wins in exactly 1 and in exactly 3 plies (host minimax):
    {plies: (packed words, set of the moves that win that fast)}."""
    out = {}
    for w0, w1, bl in sr.late_positions(4):
        if bl != 0:
            continue
        for plies in (1, 3):
            if plies in out:
                continue
            p = sr._pos(w0, w1, 0)
            if sr._minimax(p, plies, {}, nodes=20000) != 1 or (plies == 3 and sr._minimax(p, 1, {}) == 1):
                continue
            wins = set()
            for mv in orc.movegen(p):
                q = sr._pos(w0, w1, 0)
                orc.lib().orc_makemove(q, int(mv) & 0xFF, int(mv) >> 8)
                if sr._minimax(q, plies - 1, {}, nodes=20000) == -1:
                    wins.add(int(mv))
            out[plies] = ((w0, w1), wins)
        if len(out) == 2:
            break
    assert len(out) == 2
    return out


@pytest.mark.parametrize("K", [1, 16])
def test_genmove_plays_the_mating_move(tmp_path, K):
    from ataxxzero_amd import uai
    s = uai.Searcher(lls.npy(tmp_path), dtype="f16", parallel_leaves=K, virtual_loss=2, solver=True)
    for plies, ((w0, w1), wins) in _mates().items():
        pos = uai.Position(w0 & ~(1 << 63), w1, w0 >> 63)
        for _ in range(3):
            mv = s.genmove(pos, visits=400)
            assert s.last_proven == "win" and s.last_proofs[0] == 1
            # a proven winning move wins; the first one in edge order is played
            proven = [m for m, v in s.last_proofs[1] if v == -1]
            assert mv == proven[0]
            q = sr._pos(w0, w1, 0)
            orc.lib().orc_makemove(q, mv & 0xFF, mv >> 8)
            assert sr._minimax(q, 8, {}, nodes=200000) == -1
            if plies == 1:
                assert mv in wins


def test_cli_solver_reports_a_proven_win(tmp_path):
    from ataxxzero_amd import uai
    (w0, w1), _ = _mates()[3]
    pos = uai.Position(w0 & ~(1 << 63), w1, w0 >> 63)
    script = "uai\nisready\nposition fen %s\ngo movetime 200\nquit\n" % pos.fen()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "uai_interface.py"), "--network-path", lls.npy(tmp_path),
                          "--solver", "--visits", "400", "--show-pv"],
                         input=script, capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert "info string proven win" in lines
    best = [l.split()[1] for l in lines if l.startswith("bestmove")]
    legal, _ = pos.legal_moves()
    assert len(best) == 1 and uai.decode_move(best[0]) in legal
    assert any(l.startswith("info nodes ") for l in lines)
