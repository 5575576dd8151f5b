"""Host side of the batched self-play generator: configuration, the device-resident
generation loop and the reference-format game writers.

Mirrors what accelerated_generate_games.py:24-83 does around the C++ workers: load the
net, keep thousands of games in flight, append finished games as JSON lines (flushing
per batch so looper.py's line counter, looper.py:5-12, sees them), print a `Rate:` line.
"""
import json
import os
import re
import time

import numpy as np

from . import link, model

START_FEN_SELFPLAY = "x5o/7/3-3/2-1-2/3-3/7/o5x x"   # cpp/self_play_client.cpp:23
START_FEN_PLAIN = "x5o/7/7/7/7/7/o5x x"               # ataxx_rules.py:44-50, cpp/ataxx.cpp:11 family
DEFAULT_SEED = 20260101


def parse_fen(fen):
    """-> (x, o, blockers, turn) bitboards; FEN rows run from rank 7 down (cpp/ataxx.cpp:14-90)."""
    parts = fen.split()
    x = o = bl = 0
    sq = 42
    for c in parts[0]:
        if c in "xX":
            x |= 1 << sq
            sq += 1
        elif c in "oO":
            o |= 1 << sq
            sq += 1
        elif c == "-":
            bl |= 1 << sq
            sq += 1
        elif c in "1234567":
            sq += int(c)
        elif c == "/":
            sq -= 14
        else:
            raise ValueError("bad FEN %r" % fen)
    turn = 1 if len(parts) > 1 and parts[1] in "oO" else 0
    return x, o, bl, turn


def parse_fen_file(path):
    """A file of start positions, one FEN per line (blank lines and lines that begin with '#' skipped) -> the FENs.
    ValueError, with the file and line named, for a line parse_fen does not take, a position the engine would refuse
    (start_refusal) and a file without a position."""
    fens = []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            try:
                why = start_refusal(*parse_fen(line))
            except ValueError as err:
                why = str(err)
            if why:
                raise ValueError("%s, line %d: %s" % (path, number, why))
            fens.append(line)
    if not fens:
        raise ValueError("%s holds no position" % path)
    return fens


def start_refusal(x, o, blockers, turn):
    """Why the engine refuses a start position (azh_engine_set_start_pool's checks, host arithmetic), or None."""
    board = (1 << 49) - 1
    if (x | o | blockers) & ~board:
        return "a row is longer than 7 cells"
    if x & o or (x | o) & blockers:
        return "a stone stands on a wall or on another stone"
    if not x or not o:
        return "a side has no stone"
    empty, own, reach = board & ~(x | o | blockers), (o if turn else x), 0
    for sq in range(49):
        if (own >> sq) & 1:
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if 0 <= sq % 7 + dx < 7 and 0 <= sq // 7 + dy < 7:
                        reach |= 1 << (sq + dx + 7 * dy)
    if not reach & empty:
        return "the position is finished (the side to move has no move)"
    return None


def symmetric_blockers(blockers):
    """Is the wall mask its own image under all 8 symmetries of the board?  (link.symmetry_board; host arithmetic)"""
    return all(link.symmetry_board(s, blockers) == blockers for s in (1, 2, 4))


def symmetry_refusal(blockers):
    """Why the random symmetry does not go with an asymmetric wall mask, in the words of the engine's own refusal
    (azh_engine_set_random_symmetry)."""
    return ("not supported with a blockers mask (0x%x) that is not its own image under all 8 symmetries (the tower takes one "
            "blocker plane per launch)" % blockers)


def make_config(games, visits, seed=DEFAULT_SEED, fen=START_FEN_SELFPLAY, max_plies=400, edges_per_node=96,
                c_puct=1.0, dirichlet_alpha=0.15, dirichlet_weight=0.25, flags=0, select_budget=0):
    """Search constants default to cpp/self_play_client.cpp:31-34."""
    x, o, bl, turn = parse_fen(fen)
    return link.Config(games=games, visits=visits, max_plies=max_plies, edges_per_node=edges_per_node,
                       c_puct=c_puct, dirichlet_alpha=dirichlet_alpha, dirichlet_weight=dirichlet_weight,
                       start_turn=turn, seed=seed, start_x=x, start_o=o, blockers=bl, flags=flags,
                       select_budget=select_budget)


def process_index_from_path(path):
    """looper.py:70-74 names the per-process files model-%03i-%i.json; the trailing index
    selects the GPU and the RNG stream so N generator processes shard over N GPUs."""
    m = re.search(r"-(\d+)\.json$", os.path.basename(path))
    return int(m.group(1)) if m else 0


def select_device(index):
    n = link.require_gpu()
    dev = int(os.environ["AZH_DEVICE"]) if "AZH_DEVICE" in os.environ else index % n
    link.check(link.load().azh_set_device(dev))
    return dev


def temperature_table(max_plies, start, final=None, halflife=0.0, cutoff=None):
    """A per-ply temperature schedule for link.Engine.set_temperature, (max_plies,) float32:
    t(p) = final + (start - final) * 2 ** (-p / halflife) for halflife > 0, else start; t(p) = final for p >= cutoff where a
    cutoff is given; computed in float64 and rounded to f32; a value below 1/64, the smallest temperature the engine draws
    at, becomes 0 (the most visited move).  AlphaZero: (1, 0, cutoff=30); KataGo: (0.8, 0.2, halflife=board width)."""
    final = start if final is None else final
    p = np.arange(int(max_plies), dtype=np.float64)
    t = final + (start - final) * 2.0 ** (-p / halflife) if halflife > 0 else np.full(int(max_plies), float(start))
    if cutoff is not None:
        t[p >= cutoff] = final
    t = t.astype(np.float32)
    t[t < np.float32(1.0 / 64.0)] = 0.0
    return t


def temperature_tables(max_plies, temperature=None, temperature_final=None, halflife=0.0, cutoff=None,
                       root_policy_temperature=None, root_policy_temperature_final=1.0):
    """The generator's temperature flags -> (move table or None, root policy table or None), or ValueError: the move's
    temperature runs from `temperature` to `temperature_final` (default: the same), the root policy's from
    `root_policy_temperature` to `root_policy_temperature_final` (default 1), both with `halflife` (0: no decay, the final
    value then holds from `cutoff` on only); end points of 0 or in [1/64, 64] for the move, in [1/4, 64] for the policy."""
    if not halflife >= 0.0 or (cutoff is not None and cutoff < 0):
        raise ValueError("--temperature-halflife and --temperature-cutoff must not be negative")
    if temperature is None and (temperature_final is not None or cutoff is not None):
        raise ValueError("--temperature-final and --temperature-cutoff need --temperature")
    if temperature is None and root_policy_temperature is None and halflife:
        raise ValueError("--temperature-halflife needs --temperature or --root-policy-temperature")
    move = root = None
    if temperature is not None:
        final = temperature if temperature_final is None else temperature_final
        for t in (temperature, final):
            if not (t == 0.0 or 1.0 / 64.0 <= t <= 64.0):
                raise ValueError("--temperature and --temperature-final must be 0 or lie in [1/64, 64]")
        move = temperature_table(max_plies, temperature, final, halflife, cutoff)
    if root_policy_temperature is not None:
        for t in (root_policy_temperature, root_policy_temperature_final):
            if not 0.25 <= t <= 64.0:
                raise ValueError("--root-policy-temperature and --root-policy-temperature-final must lie in [1/4, 64]")
        root = temperature_table(max_plies, root_policy_temperature, root_policy_temperature_final, halflife, None)
    return move, root


class SelfPlay:
    """`games` concurrent MCTS self-play games on one GPU with the built-in net.

    With `streams` = 2 the games are split into two half-batches, each with its own engine
    and HIP stream, sharing one set of packed weights — the reference's double buffer
    (cpp/self_play_client.cpp:593-600, two fill buffers of `buffer_entries` rows): while one
    half runs its tree kernels or the ramp or tail of its tower launch, the other half's tower fills
    the idle CUs (+10 % at 4096 games, +24 % at 2048, nothing from 16384 on:
    profiles/round4_half_batches_and_reserved_cus.txt; bench.py's and the generator's default).
    The halves are independent game shards (distinct Philox streams, their own uids).

    `fast_visits` > 0 turns playout cap randomization on in every half-batch engine (link.Engine.set_playout_cap): a share
    `full_fraction` of the plies is searched with `visits` and root noise, the others with `fast_visits` and none.

    `forced_playouts` = k > 0 turns forced playouts and policy target pruning on in every half-batch engine
    (link.Engine.set_forced_playouts), on the plies that get root noise.

    `random_symmetry` turns the random symmetry per evaluation on in every half-batch engine
    (link.Engine.set_random_symmetry): every leaf goes to the net as its image under a symmetry drawn per (seed, uid,
    position); the start position's blockers must be their own image under all 8 symmetries.

    `start_fens` sets a pool of start positions in every half-batch engine (link.Engine.set_start_pool): game uid of an
    engine starts from entry uid % n and is played on its walls; `fen` is then the start of no game.

    `resign` = (q_below, consecutive, playthrough_fraction) turns the recorded search value and resignation on in every
    half-batch engine (link.Engine.set_resign); (0, 1, 0) records values and never resigns.

    `temperature` = (move table or None, root policy table or None), as temperature_tables makes them, sets the per-ply
    temperature of the move played and of the root policy in every half-batch engine (link.Engine.set_temperature).

    `gumbel` = (m, c_visit, c_scale) turns the Gumbel root search with sequential halving on in every half-batch engine
    (link.Engine.set_gumbel): the engines are created with FLAG_NO_REUSE and dirichlet_weight 0, which the mode needs — its
    schedule assumes a fresh root, and its noise is the Gumbel — and every ply's `dists` are the improved policy.  Not with
    the playout cap, forced playouts, a temperature, FLAG_EVAL_CACHE, FLAG_ONE_RANDOM_MOVE or FLAG_SAMPLE_POW5."""

    def __init__(self, conv_weights, bn_params, games, visits, dtype="bf16", seed=DEFAULT_SEED,
                 fen=START_FEN_SELFPLAY, streams=1, fast_visits=0, full_fraction=0.25, forced_playouts=0.0,
                 random_symmetry=False, resign=None, temperature=None, gumbel=None, start_fens=None, **cfg):
        self.dtype = link.DTYPES[dtype]
        if gumbel:
            cfg = dict(cfg, flags=cfg.get("flags", 0) | link.FLAG_NO_REUSE, dirichlet_weight=0.0)
        self.net = link.Net(conv_weights, bn_params, model.BN_EPSILON)
        if streams < 1 or games < streams:
            raise ValueError("games (%d) must be at least the number of half-batches (%d)" % (games, streams))
        # (an uneven split gives the first games % streams engines one game more)
        sizes = [games // streams + (1 if i < games % streams else 0) for i in range(streams)]
        self.engines = [link.Engine(make_config(sizes[i], visits, seed=seed + 1000003 * i, fen=fen, **cfg))
                        for i in range(streams)]
        self.engine = self.engines[0]
        self.games = games
        if start_fens:      # every half-batch engine maps its own uids onto the pool
            for e in self.engines:
                e.set_start_pool(start_fens)
        if fast_visits:
            self.set_playout_cap(fast_visits, full_fraction)
        if forced_playouts:
            self.set_forced_playouts(forced_playouts)
        if random_symmetry:
            self.set_random_symmetry(True)
        if resign:
            self.set_resign(*resign)
        if temperature and (temperature[0] is not None or temperature[1] is not None):
            self.set_temperature(*temperature)
        if gumbel:
            self.set_gumbel(*gumbel)

    def run(self, iterations):
        # every engine's whole run is enqueued on its own stream (the calls are asynchronous): the half-batches then
        # advance independently on the GPU, one's tree phase and tower tail filled by the other's tower.  The engines'
        # iterations are enqueued in turn (azh_engines_run), so that the second half starts with the first launches
        # enqueued and not a run's worth of host time later (profiles/round6_interleaved_enqueue_ab.txt).
        if len(self.engines) > 1:
            link.run_engines(self.engines, self.net, iterations, self.dtype)
            return
        for e in self.engines:
            e.run(self.net, iterations, self.dtype)

    def sync(self):
        for e in self.engines:
            e.sync()

    def set_visits(self, visits):
        for e in self.engines:
            e.set_visits(visits)

    def set_playout_cap(self, fast_visits, full_fraction=0.25):
        """Playout cap randomization in every half-batch engine; fast_visits = 0 turns it off."""
        for e in self.engines:
            e.set_playout_cap(fast_visits, link.full_per_65536(full_fraction))

    def set_forced_playouts(self, k):
        """Forced playouts and policy target pruning in every half-batch engine; k = 0 turns them off."""
        for e in self.engines:
            e.set_forced_playouts(k)

    def set_random_symmetry(self, on=True):
        """The random symmetry per evaluation in every half-batch engine."""
        for e in self.engines:
            e.set_random_symmetry(on)

    def set_resign(self, q_below, consecutive, playthrough_fraction=0.1):
        """The recorded search value and resignation in every half-batch engine; consecutive = 0 turns them off."""
        for e in self.engines:
            e.set_resign(q_below, consecutive, link.full_per_65536(playthrough_fraction))

    def set_temperature(self, move_temperature=None, root_policy_temperature=None):
        """The per-ply temperature tables in every half-batch engine; None, None turns both off."""
        for e in self.engines:
            e.set_temperature(move_temperature, root_policy_temperature)

    def set_gumbel(self, m, c_visit=50.0, c_scale=1.0):
        """The Gumbel root search in every half-batch engine; m = 0 turns it off."""
        for e in self.engines:
            e.set_gumbel(m, c_visit, c_scale)

    def resign_stats(self):
        total = {}
        for e in self.engines:
            for k, v in e.resign_stats().items():
                total[k] = total.get(k, 0) + v
        return total

    def set_thin_batches(self, mode):
        """1: the towers run one board per workgroup (a handful of leaves per iteration: the tail of a run under a game
        limit); 0: the 3-board workgroups; -1: by each engine's size (link.Engine.set_thin_batches)."""
        for e in self.engines:
            e.set_thin_batches(mode)

    def set_positions(self, boards, plies):
        lo = 0
        for e in self.engines:
            e.set_positions(boards[lo:lo + e.G], plies[lo:lo + e.G])
            lo += e.G

    def positions(self):
        """(root boards packed (G,2) u64, plies (G,)) of all slots: what set_positions takes."""
        boards, plies = [], []
        for e in self.engines:
            for g in range(e.G):
                boards.append(e.tree(g)[0][0])
                plies.append(e.game_state(g).ply)
        return np.asarray(boards, dtype=np.uint64), np.asarray(plies, dtype=np.int32)

    def set_emit_order(self, by_uid):
        for e in self.engines:
            e.set_emit_order(by_uid)

    def set_record_blockers(self, on=True):
        """Every line gains "blockers", the start position's wall cells (link.Engine.set_record_blockers)."""
        for e in self.engines:
            e.set_record_blockers(on)

    def set_game_limit(self, games):
        """`games` games in all, then the slots go idle.  uids are per engine: half-batch i of K plays its own uids
        0 .. ceil((games - i) / K) - 1, so the limits add up to `games` (and may be raised later, like the engine's)."""
        k = len(self.engines)
        if games < k:
            raise ValueError("a game limit of %d needs at most %d half-batches" % (games, games))
        for i, e in enumerate(self.engines):
            e.set_game_limit((games + k - 1 - i) // k)

    def fetch(self):
        """sync + finished games off the device; `drain` then formats them on the host while the GPU does something else"""
        for e in self.engines:
            e.fetch()

    def drain(self):
        lines = []
        for e in self.engines:
            lines += e.drain_json()
        return lines

    def stats(self):
        total = {}
        for e in self.engines:
            for k, v in e.stats().items():
                total[k] = total.get(k, 0) + v
        return total

    def timing_reset(self, enable=True):
        for e in self.engines:
            e.timing_reset(enable)

    def timing(self):
        total = {}
        for e in self.engines:
            for k, v in e.timing().items():
                total[k] = total.get(k, 0) + v
        return total

    def close(self):
        for e in self.engines:
            e.close()
        self.net.close()


def python_move(mv):
    """u16 move -> the Python generator's move value (generate_games.py:51 stores the
    ataxx_rules tuple; json turns it into nested lists): ["c",[x,y]] / [[x0,y0],[x1,y1]]."""
    if mv == 0xFFFF:
        return "pass"
    frm, to = mv & 0xFF, mv >> 8
    end = [to % 7, 6 - to // 7]
    if frm == to:
        return ["c", end]
    return [[frm % 7, 6 - frm // 7], end]


def board_cells(x, o):
    """49 ints, index x + 7*y with y = 0 at rank 7 (ataxx_rules.py:74-80)."""
    return [1 if (x >> (c + 7 * (6 - r))) & 1 else (2 if (o >> (c + 7 * (6 - r))) & 1 else 0)
            for r in range(7) for c in range(7)]


def random_play_entries(n_games, seed, max_plies=400):
    """Uniform-random games on the GPU in generate_games.py's entry shape (:20,:50-51,:68):
    {"boards": [...], "moves": [...], "result": r}; unfinished games have result None."""
    x, o, bl, turn = parse_fen(START_FEN_PLAIN)
    plies, results, boards, moves = link.random_play(n_games, seed, x, o, bl, turn, max_plies)
    out = []
    for g in range(n_games):
        n = int(plies[g])
        out.append({
            "boards": [board_cells(int(boards[g, p, 0]), int(boards[g, p, 1])) for p in range(n)],
            "moves": [python_move(int(moves[g, p])) for p in range(n)],
            "result": int(results[g]) if results[g] else None,
        })
    return out
