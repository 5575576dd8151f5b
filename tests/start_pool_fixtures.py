"""What the start-pool tests share (tests/test_start_pool_host.py, tests/test_gpu_start_pool.py): four start positions with four
different wall maps, built on the CPU from the fixture positions the search harness already uses; engines on one of them or
on the pool; the oracle's records and the device's ring records in one shape, keyed by uid.  Importing this touches no device.

The oracle has one mask per engine.  A game is a function of (seed, uid, start, mask, evaluations) and of nothing else, so the
device's record of uid u under a pool equals the record an oracle engine created with entry (u // stride) % n's start and mask
produces for the same uid: records are compared by uid, never slots in lock step."""
import functools

import numpy as np

from ataxxzero_amd import link
from oracle import oracle_lib as orc
from tests import engine_harness as eh
from tests import helpers

SEED = 424242
BOARD = (1 << 49) - 1


def _cells(mask):
    return [sq for sq in range(49) if (mask >> sq) & 1]


def _pos(x, o, walls, turn):
    p = orc.Pos()
    p.pieces[0], p.pieces[1], p.blockers, p.turn = x, o, walls, turn
    return p


def moves_under(entry, walls):
    """the legal moves of the entry's start position if the walls were `walls` (the oracle's move generator)"""
    x, o, _, turn = entry
    return sorted(int(m) for m in orc.movegen(_pos(x, o, walls, turn)))


def _reach(stones):
    out = 0
    for sq in _cells(stones):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if 0 <= sq % 7 + dx < 7 and 0 <= sq // 7 + dy < 7:
                    out |= 1 << (sq + dx + 7 * dy)
    return out


def _invariant(mask):
    return all(link.symmetry_board(s, mask) == mask for s in (1, 2, 4))


@functools.lru_cache(maxsize=None)
def block4_start():
    """a late position of the default four walls' fixture file: 10-14 empty cells, both sides well alive"""
    for rec in helpers.load_gz("rules_block4.json.gz"):
        p = orc.pos_from_fen(rec["fen"])
        x, o = int(p.pieces[0]), int(p.pieces[1])
        if orc.result(p) != 0 or len(orc.movegen(p)) == 0 or int(p.blockers) != helpers.BLOCK4_MASK:
            continue
        if 10 <= 45 - bin(x | o).count("1") <= 14 and min(bin(x).count("1"), bin(o).count("1")) >= 10:
            return x, o, helpers.BLOCK4_MASK, int(p.turn)
    raise AssertionError("no such fixture position")


@functools.lru_cache(maxsize=None)
def entries():
    """Four (x, o, walls, turn): the late position without walls; a late position on the default four walls; the late position
    with an asymmetric mask on two of its empty cells; the late position with all but three of its empty cells walled, so that
    a side soon has no move.  Each start's legal moves differ under each other entry's mask (checked here, on the CPU): a game
    played on the wrong mask cannot produce the right record."""
    x, o, turn = eh.START
    empty = BOARD & ~(x | o)
    near = [sq for sq in _cells(empty & _reach(o if turn else x))]
    assert len(near) >= 6
    asym = next(m for m in ((1 << a) | (1 << b) for a in near for b in near if a < b) if not _invariant(m))
    keep = [sq for sq in near if not (asym >> sq) & 1][:3]              # (three cells the mover reaches stay open)
    dense = empty & ~sum(1 << sq for sq in keep)
    out = [(x, o, 0, turn), block4_start(), (x, o, asym, turn), (x, o, dense, turn)]
    for i, e in enumerate(out):
        p = _pos(*e)
        assert orc.result(p) == 0 and len(orc.movegen(p)) > 0 and not (e[0] | e[1]) & e[2], i
        for j, other in enumerate(out):
            assert i == j or moves_under(e, e[2]) != moves_under(e, other[2]), (i, j)
    assert len({e[2] for e in out}) == 4 and not _invariant(asym)
    return out


def fen_of(entry):
    """the entry as a FEN with its walls ('-')"""
    x, o, walls, turn = entry
    rows = []
    for rank in range(6, -1, -1):
        row, gap = "", 0
        for f in range(7):
            sq = f + 7 * rank
            c = "x" if (x >> sq) & 1 else "o" if (o >> sq) & 1 else "-" if (walls >> sq) & 1 else None
            if c is None:
                gap += 1
            else:
                row += (str(gap) if gap else "") + c
                gap = 0
        rows.append(row + (str(gap) if gap else ""))
    return "/".join(rows) + (" o" if turn else " x")


def config(entry, games, visits, flags=0, weight=0.25, seed=SEED, max_plies=400, select_budget=0):
    x, o, walls, turn = entry
    return dict(games=games, visits=visits, max_plies=max_plies, edges_per_node=96, c_puct=1.0, dirichlet_alpha=0.15,
                dirichlet_weight=weight, start_turn=turn, seed=seed, start_x=x, start_o=o, blockers=walls, flags=flags,
                select_budget=select_budget)


def device_engine(entry, games, visits, **kw):
    return link.Engine(link.Config(**config(entry, games, visits, **kw)))


def oracle_engine(entry, games, visits, **kw):
    return orc.Engine(orc.Config(**config(entry, games, visits, **kw)))


def pooled_engine(pool, games, visits, stride=1, **kw):
    """a device engine created on the pool's first entry, with the pool set"""
    e = device_engine(pool[0], games, visits, **kw)
    e.set_start_pool(pool, stride)
    return e


# ------------------------------------------------------------------ records, by uid

def device_records(words):
    """{uid: (result, [(x, o, move, [target words in record order])])} of staged ring record words"""
    out = {}
    for r in link.records(words):
        assert r.uid not in out
        out[r.uid] = (r.result & 0xFF, [(b[0], b[1], mv, [m | (c << 16) for m, c in t.items()]) for mv, _, t, b in r.plies])
    return out


def oracle_records(oe, into):
    """pops the oracle's finished games into {uid: the same shape}, from the packed records themselves (mcts_oracle.h)"""
    buf = np.zeros(1 << 20, dtype=np.uint8)
    while orc.lib().orc_engine_pending_games(oe.h):
        n = orc.lib().orc_engine_pop_game(oe.h, buf.ctypes.data, buf.nbytes)
        assert n > 0
        raw = bytes(buf[:n])
        _, uid, plies, res = (int(v) for v in np.frombuffer(raw[:16], dtype=np.int32))
        if (res >> 30) & 1:
            continue
        off, rows = 16, []
        for _ in range(plies):
            x, o = (int(v) for v in np.frombuffer(raw[off:off + 16], dtype=np.uint64))
            mv, nd = (int(v) for v in np.frombuffer(raw[off + 16:off + 20], dtype=np.uint16))
            off += 24
            rows.append((x, o, mv, [int(w) for w in np.frombuffer(raw[off:off + 4 * nd], dtype=np.uint32)]))
            off += 4 * nd
        into[uid & 0xFFFFFFFF] = (res & 0xFF, rows)


def oracle_games_of(entry, uids, games, visits, evaluate, max_iterations=40000, **kw):
    """{uid: record} for `uids` from an oracle engine created with the entry's start and mask; evaluate(leaf boards (G, 2)) ->
    (logits (G, 833), values (G,)) with the entry's walls"""
    oe = oracle_engine(entry, games, visits, **kw)
    got = {}
    for _ in range(max_iterations):
        if all(u in got for u in uids):
            break
        oe.select()
        logits, values = evaluate(oe.leaf_boards())
        oe.backup(logits, values)
        oracle_records(oe, got)
    assert all(u in got for u in uids), sorted(set(uids) - set(got))
    return {u: got[u] for u in uids}


def check_against_oracle(found, pool, games, visits, evaluator_of, stride=1, **kw):
    """every device record of `found` ({uid: record}) equals the record of its uid from the oracle engine of its entry"""
    assert found
    for k, entry in enumerate(pool):
        uids = [u for u in found if link.start_pool_entry(u, len(pool), stride) == k]
        want = oracle_games_of(entry, uids, games, visits, evaluator_of(entry), **kw) if uids else {}
        for u in uids:
            assert found[u] == want[u], (u, k)


def never_on_a_wall(found, pool, stride=1):
    for u, (_, rows) in found.items():
        walls = pool[link.start_pool_entry(u, len(pool), stride)][2]
        assert all(not (x | o) & walls for x, o, _, _ in rows), u
