"""Random symmetry per evaluation on the MI355X (azh_engine_set_random_symmetry): an engine with the mode on in lock step
with one that has it off and is fed the same logits brought back through the symmetry's permutation (one-leaf and K-leaf
kernels, the reference flags, a level budget, the solver), the evaluation cache, the device loop against host stepping, the
game lines, off is off, the refusals and the two CLIs.  The restatement is tests/symmetry_reference.py."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ataxxzero_amd import link, model
from oracle import oracle_lib as orc
from tests import engine_harness as eh
from tests import helpers
from tests import solver_reference as solver_ref
from tests import symmetry_reference as sr

pytestmark = pytest.mark.gpu

ROOT = helpers.ROOT
SEED = 20261017
VISITS = 24
UAI = link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR
# (game, ply) of tests/golden/random_play_games.jsonl.gz: the mid-game positions with the most legal moves (112-123), whose
# grandchildren — the side with the many stones to move again — reach past 128 moves
MIDGAME = [(4, 70), (1, 64), (1, 62), (4, 30), (1, 66)]


def _midgame(G):
    """G packed mid-game boards (x | turn << 63, o) of the reference's random-play games"""
    with gzip.open(os.path.join(helpers.GOLDEN, "random_play_games.jsonl.gz")) as f:
        games = [json.loads(l) for l in f.read().splitlines() if l.strip()]
    out = []
    for gi, ply in MIDGAME[:G]:
        x = o = 0
        for i, v in enumerate(games[gi]["boards"][ply]):      # cell index x + 7 y, y = 0 at rank 7
            sq = i % 7 + 7 * (6 - i // 7)
            x |= (v == 1) << sq
            o |= (v == 2) << sq
        out.append([x | ((ply % 2) << 63), o])
    return np.array(out, dtype=np.uint64)


def _late(G, max_empty=8):
    """G distinct unfinished fixture positions without blockers, a few plies before the end"""
    ps = [(w0, w1) for w0, w1, bl in solver_ref.late_positions(max_empty) if bl == 0]
    assert len(ps) >= G
    return np.array([ps[(i * len(ps)) // G] for i in range(G)], dtype=np.uint64)


def _engine(G, visits=VISITS, flags=0, budget=0, weight=0.25, blockers=0, max_plies=60, seed=SEED, start=None, positions=None):
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    x, o, turn = start if start is not None else (int(p.pieces[0]), int(p.pieces[1]), 0)
    cfg = link.Config(games=G, visits=visits, max_plies=max_plies, edges_per_node=96, c_puct=1.0, dirichlet_alpha=0.15,
                      dirichlet_weight=weight, start_turn=turn, seed=seed, start_x=x, start_o=o, blockers=blockers,
                      flags=flags, select_budget=budget)
    e = link.Engine(cfg)
    if positions is not None:
        e.set_positions(positions, np.zeros(G, np.int32))
    return e


class _Coverage:
    """what the evaluated nodes of a lock-step run were: their symmetries, their widest edge counts, the layers of their jumps"""

    def __init__(self):
        self.symmetries, self.layers, self.over64, self.over128, self.evaluated = set(), set(), 0, 0, 0

    def add(self, leaf_boards, symmetries):
        """leaf_boards (n, 2) u64 (mover, opponent) of evaluated nodes: their edges are the mover's legal moves"""
        if not len(leaf_boards):
            return
        moves, counts, _ = link.rules_batch(np.ascontiguousarray(leaf_boards, dtype=np.uint64), 0)   # (the mover as x, x to move)
        self.symmetries |= {int(s) for s in symmetries}
        self.evaluated += len(counts)
        self.over64 += int((counts > 64).sum())
        self.over128 += int((counts > 128).sum())
        for row, n in zip(moves, counts):
            self.layers |= {sr.policy_index(int(m)) % 17 for m in row[:n] if (int(m) & 0xFF) != (int(m) >> 8)}

    def check(self):
        assert self.symmetries == set(range(8)), self.symmetries
        assert self.over64 > 0 and self.over128 > 0, (self.over64, self.over128, self.evaluated)
        assert self.layers == set(range(16)), self.layers


def _images_are_right(cov, uids, plain, image, need):
    """the mode-on engine's leaf boards are T_s of the mode-off engine's, s = eval_symmetry(seed, uid, the plain board)
    -> s per row (0 where nothing is evaluated)"""
    ss = np.zeros(len(plain), dtype=np.int64)
    for i in np.nonzero(need)[0]:
        m, o = int(plain[i, 0]), int(plain[i, 1])
        s = link.eval_symmetry(SEED, uids[i], m, o)
        assert s == sr.eval_symmetry(SEED, uids[i], m, o)
        assert (int(image[i, 0]), int(image[i, 1])) == (sr.board(s, m), sr.board(s, o)), (i, s)
        ss[i] = s
    cov.add(plain[np.nonzero(need)[0]], ss[np.nonzero(need)[0]])
    return ss


def _plies_played(prev, now, played):
    for g, (p, n) in enumerate(zip(prev, now)):
        played[g] += int((p.uid, p.ply) != (n.uid, n.ply))


def _lock_step_one_leaf(flags=0, budget=0, min_plies=3, until_wide=False):
    """A (mode on) against B (mode off), the step-wise API: A's boards evaluated once by the f32 tower, A given those rows, B
    the rows brought back through perm_s and the same values, over at least min_plies plies of every game (until_wide: and
    until a node of more than 128 edges has been evaluated) -> the coverage, and A's counters"""
    G = 5
    net, pos = eh.net(2), _midgame(G)
    a = _engine(G, flags=flags, budget=budget, positions=pos)
    b = _engine(G, flags=flags, budget=budget, positions=pos)
    a.set_random_symmetry(True)
    cov, played = _Coverage(), np.zeros(G, dtype=np.int64)
    for it in range(600):
        st = [b.game_state(g) for g in range(G)]
        na, nb = a.select(), b.select()
        (need_a, lb_a), (need_b, lb_b) = a.leaves(), b.leaves()
        assert na == nb and (need_a == need_b).all()
        ss = _images_are_right(cov, [s.uid for s in st], lb_b, lb_a, need_b)
        logits, values = net.forward(lb_a, 0, link.DTYPE_F32)
        logits = logits.reshape(G, 833)
        a.set_evals(logits, values)
        b.set_evals(sr.logits_of_the_position(logits, ss), values)
        a.backup()
        b.backup()
        eh.same(eh.dump(a), eh.dump(b))
        _plies_played(st, [b.game_state(g) for g in range(G)], played)
        if played.min() >= min_plies and (cov.over128 or not until_wide):
            break
    assert played.min() >= min_plies, played
    stats = a.stats()
    assert stats == b.stats()
    a.close(), b.close()
    return cov, stats


def test_lock_step_one_leaf_kernel():
    cov, stats = _lock_step_one_leaf(until_wide=True)
    cov.check()
    assert stats["plies"] >= 15


@pytest.mark.parametrize("flags,budget", [(UAI, 0), (0, 3)])
def test_lock_step_with_the_reference_flags_and_with_a_level_budget(flags, budget):
    cov, stats = _lock_step_one_leaf(flags, budget)
    assert len(cov.symmetries) >= 6 and cov.over64 > 0
    if budget:
        assert stats["parked"] > 0          # a parked descent resumes and its leaf is seen under the same s


def test_cache_on_builds_the_trees_of_cache_off():
    G = 5
    net, pos = eh.net(2), _midgame(G)
    c = _engine(G, flags=link.FLAG_EVAL_CACHE, positions=pos)
    d = _engine(G, positions=pos)
    played = np.zeros(G, dtype=np.int64)
    for e in (c, d):
        e.set_random_symmetry(True)
    for it in range(600):
        st = [d.game_state(g) for g in range(G)]
        c.select(), d.select()
        (need_c, lb_c), (need_d, lb_d) = c.leaves(), d.leaves()
        assert ((need_c == 0) | (need_c == need_d)).all()               # the cache only ever removes evaluations
        assert (lb_c[need_c != 0] == lb_d[need_c != 0]).all()
        for e, lb in ((c, lb_c), (d, lb_d)):
            logits, values = net.forward(lb, 0, link.DTYPE_F32)
            e.set_evals(logits, values)
            e.backup()
        for g in range(G):
            sc, sd = c.game_state(g), d.game_state(g)
            assert (sc.phase, sc.arena, sc.n_nodes, sc.n_edges, sc.ply, sc.root_visits, sc.uid) == \
                   (sd.phase, sd.arena, sd.n_nodes, sd.n_edges, sd.ply, sd.root_visits, sd.uid)
            tc, td = c.tree(g), d.tree(g)
            assert (tc[0] == td[0]).all() and (tc[2] == td[2]).all() and (tc[3] == td[3]).all()
            assert (tc[1][:, :3] == td[1][:, :3]).all()                   # (word 3 also keeps the value when caching)
        _plies_played(st, [d.game_state(g) for g in range(G)], played)
        if played.min() >= 2 and c.stats()["cache_hits"] > 0:
            break
    sc, sd = c.stats(), d.stats()
    assert played.min() >= 2 and sc["cache_hits"] > 0 and sc["nn_evals"] + sc["cache_hits"] == sd["nn_evals"]
    c.close(), d.close()


def _lock_step_k_leaves(solver):
    G, K = 3, 4
    net = eh.net(2)
    pos = _late(G) if solver else _midgame(G)
    visits = 48 if solver else VISITS
    a = _engine(G, visits=visits, positions=pos)
    b = _engine(G, visits=visits, positions=pos)
    for e in (a, b):
        e.set_leaf_batch(K, 1)
        if solver:
            e.set_solver(True)
    a.set_random_symmetry(True)
    cov, played = _Coverage(), np.zeros(G, dtype=np.int64)
    for it in range(300):
        st = [b.game_state(g) for g in range(G)]
        na, nb = a.select(), b.select()
        (kind_a, lb_a, le_a), (kind_b, lb_b, le_b) = a.batch_leaves(), b.batch_leaves()
        assert na == nb and (kind_a == kind_b).all() and (le_a == le_b).all()
        need = ((kind_b == link.LEAF_EVAL) | (kind_b == link.LEAF_ROOT)).reshape(-1)
        assert (lb_a.reshape(-1, 2)[~need] == 0).all()
        uids = [st[i // K].uid for i in range(G * K)]
        ss = _images_are_right(cov, uids, lb_b.reshape(-1, 2), lb_a.reshape(-1, 2), need)
        logits, values = net.forward(lb_a.reshape(-1, 2), 0, link.DTYPE_F32)
        logits = logits.reshape(G * K, 833)
        a.set_batch_evals(logits, values)
        b.set_batch_evals(sr.logits_of_the_position(logits, ss), values)
        a.backup()
        b.backup()
        eh.same(eh.dump(a, raw=True), eh.dump(b, raw=True))
        _plies_played(st, [b.game_state(g) for g in range(G)], played)
        if played.min() >= 3 and (not solver or a.proof_stats()["proven_nodes"] > 0):
            break
    assert played.min() >= 3, played
    assert a.stats() == b.stats() and a.proof_stats() == b.proof_stats()
    proofs = a.proof_stats()
    a.close(), b.close()
    return cov, proofs


def test_lock_step_k_leaf_kernel():
    cov, _ = _lock_step_k_leaves(solver=False)
    assert len(cov.symmetries) >= 6 and cov.over64 > 0 and cov.evaluated > 60


def test_lock_step_k_leaf_kernel_with_the_solver():
    cov, proofs = _lock_step_k_leaves(solver=True)
    assert proofs["proven_nodes"] > 0 and len(cov.symmetries) >= 6


@pytest.mark.parametrize("games,extras", [(5, False), (33, False), (130, False), (33, True)])
def test_device_loop_equals_host_stepping(games, extras):
    """extras: the playout cap and forced playouts on as well"""
    net, n = eh.net(2), 200
    engines = []
    for _ in range(2):
        e = _engine(games, visits=16, max_plies=400, start=eh.late_start())
        e.set_random_symmetry(True)
        if extras:
            e.set_playout_cap(4, 16384)
            e.set_forced_playouts(2.0)
        engines.append(e)
    a, b = engines
    la, lb = [], []
    for chunk in range(6):        # (a handful of games needs more than one chunk before one of them has ended)
        a.run(net, n, link.DTYPE_BF16)
        a.sync()
        for _ in range(n):
            b.select()
            b.eval(net, link.DTYPE_BF16)
            b.backup()
        eh.same(eh.dump(a), eh.dump(b))
        assert a.stats() == b.stats()
        la += a.drain_json()
        lb += b.drain_json()
        if la:
            break
    assert a.stats()["plies"] > 5 * games
    assert sorted(la) == sorted(lb) and len(la) > 0
    a.close(), b.close()


def test_game_lines_of_a_mode_on_run_are_real_games():
    """the self-play start: its four blockers are their own image under all 8 symmetries"""
    G = 5
    p = orc.pos_from_fen(orc.START_FEN_SELFPLAY)
    e = _engine(G, visits=8, max_plies=400, blockers=helpers.BLOCK4_MASK, start=(int(p.pieces[0]), int(p.pieces[1]), 0))
    e.set_random_symmetry(True)
    net, lines = eh.net(2), []
    for _ in range(60):
        e.run(net, 100, link.DTYPE_BF16)
        lines += e.drain_json()
        if len(lines) >= G:
            break
    assert len(lines) >= G
    for line in lines:
        entry = json.loads(line)
        assert list(entry) == ["boards", "dists", "moves", "result"] and entry["result"] in (1, 2)
        assert helpers.replay_game_entry(entry, orc.START_FEN_SELFPLAY) == entry["result"]
    assert e.stats()["edge_overflow"] == 0
    e.close()


def test_off_is_off():
    net, n, G = eh.net(2), 400, 5
    ref = _engine(G, visits=12, max_plies=400, start=eh.late_start())
    never = _engine(G, visits=12, max_plies=400, start=eh.late_start())
    never.set_random_symmetry(False)
    off = _engine(G, visits=12, max_plies=400, start=eh.late_start())
    off.set_random_symmetry(True)
    off.set_random_symmetry(False)
    on = _engine(G, visits=12, max_plies=400, start=eh.late_start())
    on.set_random_symmetry(True)
    want = []
    for chunk in range(5):        # (until every slot's worth of games has ended)
        for e in (ref, never, off, on):
            e.run(net, n, link.DTYPE_F32)
            e.sync()
        lines = ref.drain_json()
        for e in (never, off):
            eh.same(eh.dump(ref), eh.dump(e))
            assert e.drain_json() == lines and e.stats() == ref.stats()
        want += lines
        if len(want) >= G:
            break
    assert len(want) >= G
    assert [t[2].tobytes() for t in eh.dump(on)[1]] != [t[2].tobytes() for t in eh.dump(ref)[1]]    # (and on is not off)
    for e in (ref, never, off, on):
        e.close()


def test_refusals_leave_the_engine_as_it_was():
    net = eh.net(2)
    inner = ((1 << 8) | (1 << 40), (1 << 12) | (1 << 36), 0)       # a start position that keeps clear of the corners
    corners = (1 << 0) | (1 << 6) | (1 << 42) | (1 << 48)
    for kwargs, word in [(dict(flags=link.FLAG_ARENA), "AZH_FLAG_TWO_NETS"), (dict(flags=link.FLAG_SYMMETRY_AVG), "AZH_FLAG_SYMMETRY_AVG"),
                         (dict(blockers=1 << 0, start=inner), "blockers")]:
        e = _engine(4, **kwargs)
        with pytest.raises(link.AzhError, match=word):
            e.set_random_symmetry(True)
        e.set_random_symmetry(False)              # switching off is no request for the mode
        if kwargs.get("flags") == link.FLAG_ARENA:
            e.run_arena(net, net, 30, link.DTYPE_F32)
        else:
            e.run(net, 30, link.DTYPE_F32)
        e.sync()
        assert e.stats()["steps"] > 0
        e.close()
    e = _engine(4, blockers=corners, start=inner)     # the four corners are their own image: accepted
    e.set_random_symmetry(True)
    e.run(net, 60, link.DTYPE_F32)
    e.sync()
    assert e.stats()["plies"] > 0
    e.select()
    with pytest.raises(link.AzhError, match="awaits its backup"):
        e.set_random_symmetry(False)
    need, lb = e.leaves()
    e.set_evals(*net.forward(lb, corners, link.DTYPE_F32))
    e.backup()
    e.set_random_symmetry(False)
    e.close()


def test_the_two_clis(tmp_path):
    conv, bn = model.random_init(2, 128, seed=3, perturb_bn=True)
    net_path = str(tmp_path / "model-001.npy")
    model.save_model(net_path, conv, bn)
    games_path = str(tmp_path / "model-001-0.json")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "accelerated_generate_games.py"), "--network", net_path,
                          "--output-games", games_path, "--random-symmetry", "--game-count", "6", "--visits", "16",
                          "--buffer-size", "4"], cwd=ROOT, capture_output=True, timeout=600)
    assert res.returncode == 0, (res.stdout.decode()[-2000:], res.stderr.decode()[-2000:])
    lines = [l for l in open(games_path) if l.strip()]
    assert len(lines) == 6
    for line in lines:
        entry = json.loads(line)
        assert helpers.replay_game_entry(entry, orc.START_FEN_SELFPLAY) == entry["result"]
    proc = subprocess.Popen([sys.executable, os.path.join(ROOT, "uai_interface.py"), "--network-path", net_path, "--random-symmetry",
                             "--visits", "32"], cwd=ROOT, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True)

    def send(s):
        proc.stdin.write(s + "\n")
        proc.stdin.flush()

    def read_until(prefix):
        while True:
            line = proc.stdout.readline()
            assert line, proc.stderr.read()[-2000:]
            if line.startswith(prefix):
                return line.strip()

    send("uai")
    read_until("uaiok")
    send("isready")
    read_until("readyok")
    send("uainewgame")
    send("go movetime 100")
    best = read_until("bestmove ").split()[1]
    assert best in [orc.move_string(m) for m in orc.movegen(orc.pos_from_fen(orc.START_FEN_PLAIN))]
    send("quit")
    proc.wait(timeout=30)
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "uai_interface.py"), "--network-path", net_path, "--random-symmetry",
                          "--symmetry-average"], cwd=ROOT, capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"exclude each other" in bad.stderr
