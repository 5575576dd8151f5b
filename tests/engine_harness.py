"""What the GPU search tests share: the late start position, a cached random net, the engine of the root-mode tests, one
iteration of the step-wise API, dumps of the engines' states and trees and their comparison, the staged records, the
generator's command line, the wide roots, the raw mark's invariant, the resign rule recounted from records, and the lock step
of a device engine with the CPU oracle.  The root-mode tests (playout cap, forced playouts, Gumbel, temperature, resign, hostile
evaluations) build their engines with root_engine; the tests that start from other positions (the random symmetry, the
leaf-parallel search: tests/leaf_lockstep.py) keep builders of their own.  Importing this touches no device."""
import functools
import gzip
import json
import os
import subprocess
import sys

import numpy as np

from ataxxzero_amd import link, model
from oracle import oracle_lib as orc
from tests import helpers
from tests import resign_reference
from tests.helpers import synthetic_evals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 424242
C_PUCT, ALPHA = 1.0, 0.15          # root_engine's exploration constant and Dirichlet alpha

# Positions with many legal moves, found on the CPU with the oracle's uniformly random play from the plain start position
# (x5o/7/7/7/7/7/o5x x, no blockers): the widest with at most 128 moves (128) and the widest of all (157) in 20,000 games.
WIDE_FEN_MID = "1xxoo2/x3o2/oooooo1/1ooooo1/1o2o1o/1oo1xx1/1oo1x1x o"
WIDE_FEN_BIG = "2oo1xx/o2o3/o2oooo/2oo2o/2oo3/o1oooo1/1o2o2 o"


@functools.lru_cache(maxsize=None)
def late_start_fen():
    """An unfinished fixture position with 10-14 empty squares and both sides well alive: games from it last a few dozen
    plies, so thresholds, tree reuse, game ends and restarts all occur within a few hundred iterations."""
    for rec in helpers.load_gz("rules_noblock.json.gz"):
        p = orc.pos_from_fen(rec["fen"])
        x, o = int(p.pieces[0]), int(p.pieces[1])
        if orc.result(p) != 0 or len(orc.movegen(p)) == 0:
            continue
        if 10 <= 49 - bin(x | o).count("1") <= 14 and min(bin(x).count("1"), bin(o).count("1")) >= 10:
            return rec["fen"]
    raise AssertionError("no such fixture position")


def late_start():
    """that position as (x, o, turn)"""
    p = orc.pos_from_fen(late_start_fen())
    return int(p.pieces[0]), int(p.pieces[1]), int(p.turn)


START = late_start()


@functools.lru_cache(maxsize=None)
def net(blocks=1, seed=3):
    conv, bn = model.random_init(blocks, 128, seed=seed, perturb_bn=True)
    return link.Net(conv, bn)


def root_engine(games, visits, *, weight, seed=SEED, flags=0, max_plies=400, edges_per_node=96, cap=None, forced=None,
                gumbel=None, temperature=None, resign=None, symmetry=False, K=1):
    """An engine at START (no blockers, C_PUCT, ALPHA) with the root modes asked for, each given as its setter
    takes it: cap (fast visits, full per 65536), forced k, gumbel (m, c_visit, c_scale), temperature (move table, root table),
    resign (q below, consecutive, play-through per 65536).  The setters are called in one order, resign last, so where a mode
    refuses another it is always the same call that raises.  `weight` has no default: the root noise decides what a test of a
    root mode sees, so every caller says it."""
    x, o, turn = START
    cfg = link.Config(games=games, visits=visits, max_plies=max_plies, edges_per_node=edges_per_node, c_puct=C_PUCT,
                      dirichlet_alpha=ALPHA, dirichlet_weight=weight, start_turn=turn, seed=seed, start_x=x, start_o=o, blockers=0,
                      flags=flags)
    e = link.Engine(cfg)
    if cap is not None:
        e.set_playout_cap(*cap)
    if forced is not None:
        e.set_forced_playouts(forced)
    if temperature is not None:
        e.set_temperature(*temperature)
    if symmetry:
        e.set_random_symmetry(True)
    if K > 1:
        e.set_leaf_batch(K, 1)
    if gumbel is not None:
        e.set_gumbel(*gumbel)
    if resign is not None:
        e.set_resign(*resign)
    return e


def step(e, evals=helpers.synthetic_evals_distinct, K=1):
    """one iteration of the step-wise API (K > 1: of the leaf-parallel one) -> (need, leaf boards, logits, values)"""
    e.select()
    if K == 1:
        need, lb = e.leaves()
        logits, values = evals(lb)
        e.set_evals(logits, values)
    else:
        need, lb, _ = e.batch_leaves()
        logits, values = evals(lb.reshape(-1, 2))
        e.set_batch_evals(logits, values)
    e.backup()
    return need, lb, logits, values


def dump(e, slots=None, raw=False):
    """(state words, trees) of the slots, and with `raw` the trees' raw edge words as a third part"""
    slots = range(e.G) if slots is None else slots
    out = [e.game_state(g).as_tuple() for g in slots], [e.tree(g) for g in slots]
    return out + ([e.tree_raw(g) for g in slots],) if raw else out


def same(da, db):
    assert len(da) == len(db) and da[0] == db[0]
    for x, y in zip(da[1], db[1]):
        for u, v in zip(x, y):
            assert u.shape == v.shape and (u == v).all()
    for u, v in zip(*(d[2] if len(d) == 3 else [] for d in (da, db))):
        assert u.shape == v.shape and (u == v).all()


def staged(e):
    """the words of the records a fetch takes off the device; their lines are drained and dropped"""
    e.fetch()
    words = e.staged_records().copy()
    e.drain_json()
    return words


def records(words):
    """[(slot, uid, result, kind word, [(move, word 5, {move: count}, (x, o))])] of staged record words (markers skipped)"""
    return [tuple(r[:5]) for r in link.records(words)]


def records3(words):
    """the same without the boards: [(slot, uid, result, kind word, [(move, word 5, {move: count})])]"""
    return [(slot, uid, result, kind, [row[:3] for row in rows]) for slot, uid, result, kind, rows in records(words)]


def generator(tmp_path, *flags):
    """accelerated_generate_games.py on a fresh one-block net, 20 games -> (the finished process, the games file)"""
    conv, bn = model.random_init(1, 128, seed=5)
    net_path = str(tmp_path / "model-004.npy")
    model.save_model(net_path, conv, bn)
    games_path = str(tmp_path / "model-004-0.json")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "accelerated_generate_games.py"), "--network", net_path,
                          "--output-games", games_path, "--visits", "6", "--buffer-size", "16", "--seed", "9",
                          "--game-count", "20", "--max-seconds", "60"] + list(flags), cwd=ROOT, capture_output=True, timeout=200)
    return res, games_path


# ------------------------------------------------------------------ the resign rule, recounted from records

def mover(ply):
    """games of these engines begin at START, ply 0, and every move (a pass too) hands the turn over"""
    return 1 + (START[2] + ply) % 2


def resign_sequence(rows, kind):
    """a record's plies as the reference rule takes them: [(mover, q bits, counted?)] from its own word-5 values"""
    return [(mover(p),) + resign_reference.decode_word5(w5, bool(kind & link.REC_KIND_PLAYOUT_CAP))
            for p, (_, w5, _, _) in enumerate(rows)]


def ends_finished(rows, n_before):
    """the last board plus the last move is a position the rules adjudicate as finished"""
    move, _, _, (x, o) = rows[-1]
    turn = (START[2] + n_before + len(rows) - 1) % 2
    board = np.array([[x | (turn << 63), o]], dtype=np.uint64)
    after = link.makemove_batch(board, np.array([move], dtype=np.uint16))
    return int(link.rules_batch(after, 0)[2][0]) != 0


def check_resign_records(recs, q_below, consecutive, share, seed=SEED):
    """Every record against the reference rule on its own word-5 values -> the resign stats recounted from the records."""
    stats = {"resigned": 0, "playthrough": 0, "playthrough_fired": 0, "playthrough_false": 0}
    for slot, uid, result, kind, rows in recs:
        assert kind & link.REC_KIND_VALUES and result in (1, 2), (uid, kind, result)
        seq = resign_sequence(rows, kind)
        fire = resign_reference.first_fire(seq, q_below, consecutive)
        through = link.resign_playthrough(seed, uid, share)
        if kind & link.REC_KIND_RESIGNED:
            assert not through, uid                               # a game plays through iff the draw says so
            assert fire == (len(rows) - 1, seq[-1][0]), (uid, fire, len(rows))    # no longer, no shorter
            assert result == 3 - seq[-1][0], uid
            stats["resigned"] += 1
        else:
            assert through or fire is None, (uid, fire)
            assert ends_finished(rows, 0), uid
            if through:
                stats["playthrough"] += 1
                if fire is not None:
                    stats["playthrough_fired"] += 1
                    stats["playthrough_false"] += int(result != 3 - fire[1])
    return stats


def _oracle_follow(oe, net, blockers, iterations, dtype=link.DTYPE_F32, thin=False, net_b=None):
    """The oracle plays `iterations` search iterations, its leaves evaluated by the tower the device-resident loop uses for
    them — the f32 tower, or a 16-bit tower with one board per workgroup (`thin`): both are bit-identical wherever a board
    sits in a launch (tests/test_gpu_net.py) — i.e. exactly what the loop computes for itself.  `net_b`: the arena's
    second net, for the leaves whose mover it is (need class 2, uai_ringmaster.py:221-265)."""
    G = oe.G
    logits = np.zeros((G, 833), np.float32)
    values = np.zeros(G, np.float32)
    for _ in range(iterations):
        _, need = oe.select()
        lb = None
        for cls, n in ((1, net), (2, net_b)):
            idx = np.nonzero(need == cls)[0] if net_b is not None else (np.nonzero(need)[0] if cls == 1 else [])
            if len(idx):
                lb = oe.leaf_boards() if lb is None else lb
                p, v = n.forward(lb[idx], blockers, dtype, thin=thin)
                logits[idx] = p.reshape(len(idx), 833)
                values[idx] = v.reshape(-1)
        oe.backup(logits, values)


def compare_all(oe, ge, games, nan_aware=False):
    """nan_aware: a NaN prior or total score must be a NaN on both sides, whatever its sign and payload — the only words of
    a tree that are not a function of IEEE arithmetic alone (which NaN an operation hands on is the hardware's choice)."""
    for g in games:
        so, sg = oe.game_state(g), ge.game_state(g)
        assert so.as_tuple() == sg.as_tuple(), (g, so.as_tuple(), sg.as_tuple())
        to, tg = oe.tree(g), ge.tree(g)
        for name, a, b in zip(("boards", "info", "edges", "moves"), to, tg):
            assert a.shape == b.shape, (g, name)
            if nan_aware and name == "edges":
                a, b = a.copy(), b.copy()
                for col in (0, 2):
                    na, nb = _is_nan_bits(a[:, col]), _is_nan_bits(b[:, col])
                    assert (na == nb).all(), (g, name, col)
                    a[na, col] = b[nb, col] = 0x7FC00000
            assert (a == b).all(), (g, name)


def make_pair(games, visits, max_plies=400, edges_per_node=96, seed=77, fen=orc.START_FEN_SELFPLAY, weight=0.25,
              flags=0, select_budget=0):
    ocfg = orc.make_config(games, visits, seed=seed, fen_str=fen, max_plies=max_plies,
                           edges_per_node=edges_per_node, weight=weight, flags=flags, select_budget=select_budget)
    gcfg = link.Config(**{n: getattr(ocfg, n) for n, _ in orc.Config._fields_})
    return orc.Engine(ocfg), link.Engine(gcfg)


def run_lockstep(oe, ge, iterations, check_every=1, evaluator=synthetic_evals):
    G = oe.G
    o_games, g_lines = [], []
    for it in range(iterations):
        n_o, need_o = oe.select()
        n_g = ge.select()
        need_g, lb_g = ge.leaves()
        lb_o = oe.leaf_boards()
        assert n_o == n_g and (need_o == need_g).all(), it
        assert (lb_o[need_o == 1] == lb_g[need_o == 1]).all(), it
        logits, values = evaluator(lb_o)
        oe.backup(logits, values)
        ge.set_evals(logits, values)
        ge.backup()
        if it % check_every == 0 or it == iterations - 1:
            compare_all(oe, ge, range(G))
        o_games += oe.pop_games()
        g_lines += ge.drain_json()
    return o_games, g_lines


def check_marks(ge, games):
    """The early request's mark (bit 31 of a prior in the device's edge records, azh_engine_tree_raw): at most ONE marked edge
    per node, and only on an edge whose child exists, is not a finished position and has 1 .. 128 moves — what lets the
    descent request the marked child's records without a check.  -> (nodes with a mark, marks on an edge index >= 64)."""
    marked_nodes = high = 0
    for g in games:
        _, info, _, _ = ge.tree(g)
        raw = ge.tree_raw(g)
        mark = (raw[:, 0] >> 31) != 0
        for n in range(len(info)):
            first, m = int(info[n, 0]), int(info[n, 1] & 0xFFFF)
            idx = np.nonzero(mark[first:first + m])[0]
            assert len(idx) <= 1, (g, n, idx.tolist())
            if len(idx):
                assert m <= 128, (g, n, m)
                z, w = int(raw[first + idx[0], 2]), int(raw[first + idx[0], 3])
                assert (z >> 16) != 0xFFFF and (w >> 31) == 0 and 1 <= ((w >> 23) & 0xFF) <= 128, (g, n, int(idx[0]), hex(z), hex(w))
                marked_nodes += 1
                high += int(idx[0]) >= 64
        # no mark outside the nodes' ranges either (every edge belongs to exactly one node)
        assert int(mark.sum()) <= len(info)
    return marked_nodes, high


def root_mark(e, g=0):
    """check_marks' invariant at the root of game g alone -> the root edge that carries the mark, or None"""
    _, info, _, _ = e.tree(g)
    raw = e.tree_raw(g)
    first, m = int(info[0, 0]), int(info[0, 1] & 0xFFFF)
    idx = np.nonzero((raw[first:first + m, 0] >> 31) != 0)[0]
    assert len(idx) <= 1, idx.tolist()
    if len(idx):
        z, w = int(raw[first + idx[0], 2]), int(raw[first + idx[0], 3])
        assert m <= 128 and (z >> 16) != 0xFFFF and (w >> 31) == 0 and 1 <= ((w >> 23) & 0xFF) <= 128, (m, hex(z), hex(w))
        return int(idx[0])
    return None


def _wide_roots():
    """Four roots: 117 moves (the `wide` family starts at 129 moves: this one is the widest board of the `random` family), 165
    moves, the 193-move board, and a mid-game board of 112-123 moves whose grandchildren pass 128."""
    mid = max(_edge_positions("random"), key=lambda r: len(r["moves"]))
    assert len(mid["moves"]) == 117
    return [_pack(mid["fen"]), _pack(_edge_positions("wide", (165,))[0]["fen"]), _pack(_edge_positions("wide", (193,))[0]["fen"]),
            _midgame(4, 70)]


def _positions(G, blockers):
    """G distinct unfinished fixture positions of the given blocker set, the last one near the end of its game."""
    name = "rules_block4.json.gz" if blockers else "rules_noblock.json.gz"
    out = []
    for rec in helpers.load_gz(name):
        p = orc.pos_from_fen(rec["fen"])
        if orc.result(p) != 0 or len(orc.movegen(p)) == 0:
            continue
        empty = 49 - bin(int(p.pieces[0]) | int(p.pieces[1]) | int(p.blockers)).count("1")
        out.append((empty, [int(p.pieces[0]) | (p.turn << 63), int(p.pieces[1])]))
    out.sort(key=lambda t: -t[0])
    picks = [out[i * (len(out) // (2 * G + 1))][1] for i in range(G - 1)] + [min(out, key=lambda t: t[0])[1]]
    return np.array(picks, dtype=np.uint64)


def _is_nan_bits(w):
    return ((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0)


def _pack(fen):
    p = orc.pos_from_fen(fen)
    return [int(p.pieces[0]) | (p.turn << 63), int(p.pieces[1])]


def _edge_positions(family, moves=None, sets="none"):
    return [r for r in helpers.load_gz("rules_edge.json.gz")["positions"]
            if r["set"] == sets and r["family"] == family and (moves is None or len(r["moves"]) in moves)]


def _midgame(gi, ply):
    """A board of tests/golden/random_play_games.jsonl.gz, packed (tests/test_gpu_random_symmetry.py reads them the same way)."""
    with gzip.open(os.path.join(helpers.GOLDEN, "random_play_games.jsonl.gz")) as f:
        games = [json.loads(l) for l in f.read().splitlines() if l.strip()]
    x = o = 0
    for i, v in enumerate(games[gi]["boards"][ply]):
        sq = i % 7 + 7 * (6 - i // 7)
        x |= (v == 1) << sq
        o |= (v == 2) << sq
    return [x | ((ply % 2) << 63), o]
