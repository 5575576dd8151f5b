"""Single-position search for the UAI front-end: what engine.MCTSEngine.genmove does
(engine.py:474-530) with the tree, the search and the net on the GPU.

One game slot, the Python engine's search semantics (first-max ties, 833-way posterior, no
Dirichlet: AZH_FLAG_TIE_FIRST | AZH_FLAG_PY_POSTERIOR), a fresh tree per call — which is what
the reference engine ends up with when a UAI master sends one `moves` message per ply
(engine.set_state, engine.py:452-472).  With `visits` the search is exactly `visits` MCTS steps
(uai_interface.py:44-46); with a time budget it runs until the time is used.  The move is then
sampled on the host exactly like sample_with_exponential_weight (engine.py:532-548).

With `reuse_tree` (an option, off by default) one engine lives for the whole dialogue and its tree follows the game:
at every `go` the searcher walks from the position its tree is rooted at to the session's position — the same position,
or one or two moves away (engine.set_state's grandchild rule, engine.py:452-472, and the one-move case), played on the
device with azh_engine_play_moves so that the subtree, its counts and priors are kept — and starts a fresh tree only when
the new position is not there.  The root's edges and the principal variation come from azh_engine_root_report.

With `solver` (an option, off by default) the search proves wins and losses in its tree ("Proven wins and
losses"; every K then runs through the leaf-parallel kernel): a move that is proven to win is played without sampling, a
root that is proven lost plays its most visited move, and a timed search stops as soon as the root is proven.

With `fpu_reduction` and / or `cpuct_base` (options, off by default) an unvisited move scores its parent's mean score less a
reduction, not 0, and the exploration factor grows with the logarithm of the visits ("First-play urgency and the
exploration rate"; every K then runs through the leaf-parallel kernel, as under the solver).
"""
import random
import time

import numpy as np

from . import link, model, selfplay

FILES = "abcdefg"


def encode_square(sq):
    return "%s%i" % (FILES[sq % 7], sq // 7 + 1)


def encode_move(mv):
    """u16 from | to << 8 -> UAI string (uai_interface.py:11-17); 0xFFFF -> "0000"."""
    if mv == 0xFFFF:
        return "0000"
    frm, to = mv & 0xFF, mv >> 8
    return encode_square(to) if frm == to else encode_square(frm) + encode_square(to)


def decode_move(s):
    """UAI string -> u16 (uai_interface.py:24-32)."""
    if s in ("pass", "none", "0000"):
        return 0xFFFF
    sq = lambda t: FILES.index(t[0].lower()) + 7 * (int(t[1]) - 1)
    if len(s) == 2:
        return sq(s) | (sq(s) << 8)
    if len(s) == 4:
        return sq(s[:2]) | (sq(s[2:]) << 8)
    raise Exception("Bad UAI move string: %r" % s)


class Position:
    """Board bookkeeping of the front-end, with the GPU rules behind it."""

    def __init__(self, x, o, turn, blockers=0):
        self.x, self.o, self.turn, self.blockers = x, o, turn, blockers

    @staticmethod
    def initial(fen=selfplay.START_FEN_PLAIN):
        return Position.from_fen(fen)

    @staticmethod
    def from_fen(fen):
        x, o, bl, turn = selfplay.parse_fen(fen)
        return Position(x, o, turn, bl)

    def __eq__(self, other):
        return isinstance(other, Position) and (self.x, self.o, self.turn, self.blockers) == (
            other.x, other.o, other.turn, other.blockers)

    def copy(self):
        return Position(self.x, self.o, self.turn, self.blockers)

    def fen(self):
        """FEN in the reference's dialect (ataxx_rules.py fen(): ranks 7..1, x/o/digits, side to move), walls as '-', the
        character selfplay.parse_fen and the reference's parser read (cpp/ataxx.cpp:14-90)."""
        rows = []
        for r in range(6, -1, -1):
            row, run = "", 0
            for f in range(7):
                bit = 1 << (f + 7 * r)
                ch = "x" if self.x & bit else ("o" if self.o & bit else ("-" if self.blockers & bit else None))
                if ch is None:
                    run += 1
                else:
                    row += (str(run) if run else "") + ch
                    run = 0
            rows.append(row + (str(run) if run else ""))
        return "/".join(rows) + (" x" if self.turn == 0 else " o")

    def packed(self):
        return link.pack_board(self.x, self.o, self.turn)

    def legal_moves(self):
        moves, counts, results = link.rules_batch(self.packed().reshape(1, 2), self.blockers)
        return [int(m) for m in moves[0, :counts[0]]], int(results[0])

    def move(self, mv):
        out = link.makemove_batch(self.packed().reshape(1, 2), np.array([mv], dtype=np.uint16))[0]
        self.x, self.o, self.turn = int(out[0]) & ~(1 << 63), int(out[1]), int(out[0]) >> 63

    def __str__(self):
        rows = []
        for r in range(6, -1, -1):
            rows.append(" ".join("X" if (self.x >> (f + 7 * r)) & 1 else ("O" if (self.o >> (f + 7 * r)) & 1 else
                                                                          ("-" if (self.blockers >> (f + 7 * r)) & 1 else "."))
                                 for f in range(7)))
        return "\n".join(rows)


def find_path(root, target, successors, max_plies=2):
    """The moves that lead from position `root` to position `target` in at most `max_plies` plies, or None.
    `successors(position)` yields (move, position after it) in move generation order; positions are compared with ==.
    [] when the positions are equal; a shorter path wins, and of two paths of the same length the first one in move
    order (first move, then second), which is the order of engine.set_state's two loops (engine.py:458-460)."""
    if root == target:
        return []
    frontier = [(root, [])]
    for _ in range(max_plies):
        deeper = []
        for position, path in frontier:
            for move, child in successors(position):
                if child == target:
                    return path + [move]
                deeper.append((child, path + [move]))
        frontier = deeper
    return None


class GpuSuccessors:
    """Move generator for find_path on the GPU rules, positions as (x, o, turn) on a board with the walls `blockers`.
    prefetch() generates the moves of many positions with one rules call and one make-move call."""

    def __init__(self, blockers=0):
        self.known, self.blockers = {}, blockers

    def prefetch(self, positions):
        todo = [p for p in dict.fromkeys(positions) if p not in self.known]
        if not todo:
            return
        boards = np.array([link.pack_board(*p) for p in todo], dtype=np.uint64)
        moves, counts, results = link.rules_batch(boards, self.blockers)
        rows = [(i, int(m)) for i in range(len(todo)) if results[i] == 0 for m in moves[i, :counts[i]]]
        after = link.makemove_batch(boards[[i for i, _ in rows]], np.array([m for _, m in rows], dtype=np.uint16)) if rows else []
        for p in todo:
            self.known[p] = []
        for (i, m), b in zip(rows, after):
            self.known[todo[i]].append((m, (int(b[0]) & ~(1 << 63), int(b[1]), int(b[0]) >> 63)))

    def __call__(self, position):
        self.prefetch([position])
        return self.known[position]


class Searcher:
    TIME_CAP_VISITS = 20000  # arena size of a time-controlled search (per leaf of a leaf-parallel iteration, below)
    MAX_VISITS = 60000       # the engine's limit (16-bit visit counts); a search of this many visits holds about 3.5 KB of
                             # tree per visit (96 edge slots of 18 bytes per node, two arenas): at most about 210 MB

    def __init__(self, network_path, dtype="f16", symmetry_average=False, parallel_leaves=1, virtual_loss=1,
                 reuse_tree=False, show_pv=False, solver=False, random_symmetry=False, fpu_reduction=None, cpuct_base=None,
                 cpuct_init=0.0):
        # parallel_leaves = K > 1: leaf-parallel search with virtual loss ("Leaf-parallel search"): up to K
        # leaves per iteration in one tower launch.  An extension; 1 is the reference's one-leaf search.
        if not 1 <= parallel_leaves <= link.MAX_LEAVES_PER_GAME or not 1 <= virtual_loss <= link.MAX_VIRTUAL_LOSS:
            raise ValueError("need 1 <= parallel_leaves <= %d and 1 <= virtual_loss <= %d"
                             % (link.MAX_LEAVES_PER_GAME, link.MAX_VIRTUAL_LOSS))
        if parallel_leaves > 1 and symmetry_average:
            raise ValueError("symmetry averaging is not available with parallel_leaves > 1")
        if solver and symmetry_average:
            raise ValueError("symmetry averaging is not available with the solver")
        if random_symmetry and symmetry_average:
            raise ValueError("a random symmetry per evaluation is not available with symmetry averaging")
        # fpu_reduction, cpuct_base, cpuct_init: first-play urgency and the growing exploration rate
        # (azh_engine_set_exploration); None leaves a knob off.  self.exploration: the setter's arguments, or None
        self.exploration = None
        if fpu_reduction is not None or cpuct_base is not None:
            if symmetry_average:
                raise ValueError("symmetry averaging is not available with fpu_reduction or cpuct_base")
            if (fpu_reduction is not None and not 0.0 <= fpu_reduction < float("inf")) or \
                    (cpuct_base is not None and not 0.0 < cpuct_base < float("inf")) or not 0.0 <= cpuct_init < float("inf"):
                raise ValueError("need fpu_reduction >= 0, cpuct_base > 0 and cpuct_init >= 0, all finite")
            self.exploration = (-1.0 if fpu_reduction is None else float(fpu_reduction),
                                0.0 if cpuct_base is None else float(cpuct_base), float(cpuct_init))
        self.parallel_leaves, self.virtual_loss = parallel_leaves, virtual_loss
        # random_symmetry: every position is evaluated under one of the 8 symmetries of the board, drawn per (engine seed,
        # position) — link.Engine.set_random_symmetry; the net's orientation bias averages out over a search at no tower work
        self.random_symmetry = random_symmetry
        # solver: proven wins and losses (azh_engine_set_solver).  last_proofs: (root value, [(move, value of the move's
        # child for the side to move there)] in edge order) after the last search, None without the solver;
        # last_proven: "win" / "loss" when genmove's move came from a proof, else None
        self.solver, self.last_proofs, self.last_proven = solver, None, None
        # symmetry_average: every evaluation is nn_evals.evaluate (nn_evals.py:48-62); with one game the
        # eight images ride in the same tower launch, so it costs no time
        self.extra_flags = link.FLAG_SYMMETRY_AVG if symmetry_average else 0
        conv, bn = model.load_model(network_path)
        self.net = link.Net(conv, bn, model.BN_EPSILON)
        self.dtype = link.DTYPES[dtype]
        self.last_steps = 0
        self.last_seconds = 0.0
        # reuse_tree: one engine for the session, its tree re-rooted along the moves played (module docstring).
        # show_pv: the root report of the last search is kept for Session's `info nodes ... pv ...` line.
        self.reuse_tree, self.show_pv = reuse_tree, show_pv
        self.last_inherited = 0   # root visits the last search started with (0 without reuse_tree)
        self.last_report = None   # link.RootReport of the last search (reuse_tree or show_pv)
        self.last_note = None     # why the last search was shorter than asked, or None
        self.engine = None        # the session's engine (reuse_tree)
        self.root = None          # (x, o, turn) the session engine's tree is rooted at; None: no tree to keep
        self.root_blockers = 0    # the walls the session engine was created with: another mask, another engine

    def time_cap(self):
        """Visit cap of a time-controlled search: grows with the leaves per iteration, up to the engine's limit."""
        return min(self.TIME_CAP_VISITS * self.parallel_leaves, self.MAX_VISITS)

    # ------------------------------------------------------------ the session engine (reuse_tree)

    def new_game(self):
        """`uainewgame`: the next search starts from a fresh tree whatever the position."""
        self.root = None

    def close(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None
        self.root = None

    def _random_symmetry_on(self, pos):
        """May the engine of this search evaluate under a random symmetry?  Not on walls that are not their own image under
        all 8: the search then runs without it and last_note says so, in the engine's words."""
        if self.random_symmetry and not selfplay.symmetric_blockers(pos.blockers):
            self.last_note = "the random symmetry is " + selfplay.symmetry_refusal(pos.blockers)
            return False
        return self.random_symmetry

    def _session_engine(self, pos):
        if self.engine is not None and self.root_blockers != pos.blockers:
            self.close()   # an engine keeps one wall mask: a position on another board starts a fresh engine and tree
        if self.engine is None:
            # visits = the engine's limit: no move ever comes due on the device
            cfg = link.Config(games=1, visits=self.MAX_VISITS, max_plies=400, edges_per_node=96, c_puct=1.0,
                              dirichlet_alpha=0.15, dirichlet_weight=0.0, start_turn=pos.turn, seed=random.getrandbits(63),
                              start_x=pos.x, start_o=pos.o, blockers=pos.blockers,
                              flags=link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR | self.extra_flags)
            self.engine = link.Engine(cfg)
            self.root_blockers = pos.blockers
            if self._random_symmetry_on(pos):
                self.engine.set_random_symmetry(True)
            if self.parallel_leaves > 1:
                self.engine.set_leaf_batch(self.parallel_leaves, self.virtual_loss)
            if self.solver:
                self.engine.set_solver(True)
            if self.exploration:
                self.engine.set_exploration(*self.exploration)
        return self.engine

    def _bring_tree_to(self, pos):
        """The session engine's tree rooted at `pos`: kept where `pos` is the tree's root or at most two moves below it."""
        eng = self._session_engine(pos)
        target = (pos.x, pos.o, pos.turn)
        path = None
        if self.root is not None:
            successors = GpuSuccessors(pos.blockers)
            successors.prefetch([child for _, child in successors(self.root)])
            path = find_path(self.root, target, successors)
        for move in path or []:
            if eng.play_moves([move])[0] <= 0:   # (not a root edge, or an idle slot: a finished root)
                path = None
                break
        if path is None:
            eng.set_positions(pos.packed().reshape(1, 2), [0])
        self.root = target
        return eng

    def _root_visits_reusing(self, pos, visits, seconds):
        """The search on the session's tree: `visits` MORE steps (K > 1: more root visits) on top of the inherited ones,
        or until the time is used; never past the engine's limit of MAX_VISITS root visits."""
        K = self.parallel_leaves
        start = time.time()
        eng = self._bring_tree_to(pos)
        state = eng.game_state(0)
        inherited = rv = state.root_visits
        limit = self.MAX_VISITS
        target = limit if visits is None else min(inherited + visits, limit)
        self.last_note = None
        self._random_symmetry_on(pos)   # (the session engine was made without it on asymmetric walls: every search says so)
        if visits is not None and inherited + visits > limit:
            self.last_note = "search shortened to %d of %d visits: %d inherited, the tree holds %d" % (
                target - inherited, visits, inherited, limit)
        if state.phase == 0 and rv < target:
            eng.run(self.net, 1, self.dtype)   # the root's evaluation
            state = eng.game_state(0)
        while rv < target and (seconds is None or time.time() - start < seconds):
            if state.phase != 1:
                if state.phase == 2:   # the arena is full: the device's own move is due, and a run would play it
                    self.last_note = self.last_note or "search stopped at %d visits: the tree's arena is full" % rv
                break
            todo = target - rv
            if todo >= K:
                chunk = todo // K if seconds is None else min(todo // K, 64 if K == 1 else 16)
                eng.run(self.net, chunk, self.dtype)
            else:   # K > 1: the last batch is cut to the visits that are missing
                eng.set_leaf_batch(todo, self.virtual_loss)
                eng.run(self.net, 1, self.dtype)
                eng.sync()
                eng.set_leaf_batch(K, self.virtual_loss)
            state = eng.game_state(0)   # (waits for the run)
            if state.root_visits == rv:
                break   # a finished root: nothing to search
            rv = state.root_visits
            if seconds is not None and self._root_proven(eng):
                break
        self.last_report = eng.root_report(0, 1)[0]
        self._keep_proofs(eng, self.last_report.moves)
        self.last_inherited = inherited
        self.last_steps, self.last_seconds = rv - inherited, max(time.time() - start, 1e-9)
        return [(int(m), int(n)) for m, n in zip(self.last_report.moves, self.last_report.visits) if n > 0]

    def _root_proven(self, eng):
        return self.solver and eng.root_proofs(0, 1)[0][0] != 0

    def _keep_proofs(self, eng, moves):
        """last_proofs from the engine; `moves`: the root's moves in edge order."""
        self.last_proofs = None
        if self.solver:
            root, kids = eng.root_proofs(0, 1)[0]
            self.last_proofs = (root, [(int(m), int(kids[j])) for j, m in enumerate(moves)])

    def root_visits(self, pos, visits=None, seconds=None):
        """-> [(move u16, visits)] over the expanded root edges after the search."""
        self.last_inherited, self.last_report, self.last_note, self.last_proofs = 0, None, None, None
        if self.reuse_tree:
            return self._root_visits_reusing(pos, visits, seconds)
        if self.parallel_leaves > 1 or self.solver or self.exploration:   # (both run every K through the leaf-parallel kernel)
            return self._root_visits_parallel(pos, visits, seconds)
        cap = visits if visits is not None else self.TIME_CAP_VISITS
        cfg = link.Config(games=1, visits=cap + 1, max_plies=400, edges_per_node=96, c_puct=1.0, dirichlet_alpha=0.15,
                          dirichlet_weight=0.0, start_turn=pos.turn, seed=random.getrandbits(63), start_x=pos.x,
                          start_o=pos.o, blockers=pos.blockers,
                          flags=link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR | self.extra_flags)
        eng = link.Engine(cfg)
        start = time.time()
        try:
            if self._random_symmetry_on(pos):
                eng.set_random_symmetry(True)
            if visits is not None:
                eng.run(self.net, 1 + visits, self.dtype)  # root evaluation + `visits` steps
                steps = visits
            else:
                eng.run(self.net, 2, self.dtype)
                steps = 1
                while time.time() - start < seconds and steps + 64 < cap:
                    eng.run(self.net, 64, self.dtype)
                    eng.sync()
                    steps += 64
            eng.sync()
            boards, info, edges, moves = eng.tree(0)
            if self.show_pv:
                self.last_report = eng.root_report(0, 1)[0]
        finally:
            eng.close()
        self.last_steps, self.last_seconds = steps, max(time.time() - start, 1e-9)
        first, n = int(info[0, 0]), int(info[0, 1] & 0xFFFF)
        return [(int(moves[first + j]), int(edges[first + j, 1])) for j in range(n) if int(edges[first + j, 3]) != 0xFFFFFFFF]

    def _root_visits_parallel(self, pos, visits, seconds):
        """The leaf-parallel search: iterations of up to K leaves until the root has `visits` visits (exactly: the last
        batch is truncated) or the time is used; last_steps counts root visits, not iterations."""
        K = self.parallel_leaves
        target = visits if visits is not None else self.time_cap()
        cfg = link.Config(games=1, visits=target, max_plies=400, edges_per_node=96, c_puct=1.0, dirichlet_alpha=0.15,
                          dirichlet_weight=0.0, start_turn=pos.turn, seed=random.getrandbits(63), start_x=pos.x,
                          start_o=pos.o, blockers=pos.blockers,
                          flags=link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR | self.extra_flags)
        eng = link.Engine(cfg)
        start = time.time()
        try:
            eng.set_leaf_batch(K, self.virtual_loss)
            if self.solver:
                eng.set_solver(True)
            if self.exploration:
                eng.set_exploration(*self.exploration)
            if self._random_symmetry_on(pos):
                eng.set_random_symmetry(True)
            eng.run(self.net, 1, self.dtype)  # the root evaluation
            rv = 0
            while rv < target and (seconds is None or time.time() - start < seconds):
                # no run may go past the iteration that reaches the target: the move would be played in the next one
                chunk = -(-(target - rv) // K)
                if seconds is not None:
                    chunk = min(chunk, 16)
                eng.run(self.net, chunk, self.dtype)
                now = eng.game_state(0).root_visits  # (waits for the run)
                if now == rv:
                    break  # a finished root: nothing to search
                rv = now
                if seconds is not None and self._root_proven(eng):
                    break
            eng.sync()
            boards, info, edges, moves = eng.tree(0)
            if self.show_pv:
                self.last_report = eng.root_report(0, 1)[0]
            self._keep_proofs(eng, moves[int(info[0, 0]):int(info[0, 0]) + int(info[0, 1] & 0xFFFF)])
        finally:
            eng.close()
        self.last_steps, self.last_seconds = rv, max(time.time() - start, 1e-9)
        first, n = int(info[0, 0]), int(info[0, 1] & 0xFFFF)
        return [(int(moves[first + j]), int(edges[first + j, 1])) for j in range(n) if int(edges[first + j, 3]) != 0xFFFFFFFF]

    def pv_line(self):
        """`info nodes <root visits> inherited <n> score <q> pv <moves>` for the last search (show_pv), or None: q is
        W / n of the line's first edge for the side to move, mapped to [-1, 1]."""
        r = self.last_report
        if r is None:
            return None
        text = "info nodes %d inherited %d" % (r.root_visits, self.last_inherited)
        if len(r.pv):
            j = r.moves.tolist().index(int(r.pv[0]))
            score = 2.0 * float(r.scores[j]) / float(r.visits[j]) - 1.0
            if self.last_proofs is not None and self.last_proofs[1][j][1] != 0:
                score = -float(self.last_proofs[1][j][1])   # a proven first edge: the child's mover loses = this side wins
            text += " score %.4f pv %s" % (score, " ".join(encode_move(int(m)) for m in r.pv))
        return text

    def genmove(self, pos, visits=None, seconds=None, exponent=5.0):
        legal, result = pos.legal_moves()
        self.last_proven = None
        if not legal:
            self.last_inherited, self.last_report, self.last_note, self.last_proofs = 0, None, None, None
            return 0xFFFF  # the reference answers "pass" when no edge was visited (engine.py:495-496)
        edges = self.root_visits(pos, visits=visits, seconds=seconds)
        if not edges:
            return legal[0]
        if self.last_proofs is not None:
            root, kids = self.last_proofs
            winning = [mv for mv, v in kids if v == -1]
            if winning:   # the first proven winning move in edge order, without sampling
                self.last_proven = "win"
                return winning[0]
            if root == -1:   # every move loses: the most visited one, the first on a tie
                self.last_proven = "loss"
                return max(edges, key=lambda t: t[1])[0]
        # sample_with_exponential_weight (engine.py:532-548)
        total = float(sum(n for _, n in edges))
        max_visits = max(n for _, n in edges)
        weights = {mv: (n / total) ** exponent for mv, n in edges if n >= max_visits * 0.5}
        norm = 1.0 / sum(weights.values())
        x = random.random()
        for mv, w in weights.items():  # sample_by_weight (engine.py:38-47)
            if x <= w * norm:
                return mv
            x -= w * norm
        return next(iter(weights))


# ---------------------------------------------------------------- text protocol

def xy_to_square(xy):
    """(x, y) with y = 0 at rank 7 (the reference's board coordinates) -> "a7"-style square."""
    return FILES[xy[0]] + str(7 - xy[1])


def square_to_xy(text):
    return FILES.index(text[0].lower()), 7 - int(text[1])


def xy_move_to_text(move):
    """Reference move value ("pass" | ("c", (x, y)) | ((x0, y0), (x1, y1))) -> UAI text."""
    if move == "pass":
        return "0000"
    return "".join(xy_to_square(part) for part in move if part != "c")


def text_to_xy_move(text):
    if text in ("pass", "none", "0000"):
        return "pass"
    if len(text) not in (2, 4):
        raise Exception("Bad UAI move string: %r" % (text,))
    squares = [square_to_xy(text[k:k + 2]) for k in range(0, len(text), 2)]
    return ("c", squares[0]) if len(squares) == 1 else (squares[0], squares[1])


class Session:
    """One UAI dialogue (the command set of uai_interface.py:41-88) over a Searcher.  Commands are looked up in a
    table of (prefix, handler) pairs; every handler returns the lines to print."""

    def __init__(self, searcher, visits=None, safety_ms=0, show_game=False, log=None):
        self.searcher, self.visits, self.safety_ms, self.show_game, self.log = searcher, visits, safety_ms, show_game, log
        self.position = Position.initial()
        self.table = [
            ("uainewgame", self.on_newgame),
            ("uai", self.on_hello),
            ("isready", lambda rest: ["readyok"]),
            ("moves ", self.on_moves),
            ("position fen ", self.on_fen),
            ("go movetime ", self.on_go),
            ("showboard", lambda rest: str(self.position).split("\n") + ["boardok"]),
        ]

    def on_hello(self, rest):
        return ["id name AtaxxZero-MI355X", "id author ataxxzero_amd", "uaiok"]

    def on_newgame(self, rest):
        self.position = Position.initial()
        if getattr(self.searcher, "reuse_tree", False):
            self.searcher.new_game()
        return []

    def on_moves(self, rest):
        for text in rest.split():
            self.position.move(decode_move(text))
        return []

    def on_fen(self, rest):
        self.position = Position.from_fen(rest)
        if self.show_game and self.log is not None:
            print("===\n%s" % (self.position,), file=self.log)
        return []

    def on_go(self, rest):
        if self.visits is not None:
            move = self.searcher.genmove(self.position, visits=self.visits)
        else:
            budget_ms = max(int(rest) - self.safety_ms, 1)
            move = self.searcher.genmove(self.position, seconds=budget_ms * 1e-3)
        # (no search yet: a session whose first `go` meets a position without a move)
        speed = self.searcher.last_steps / self.searcher.last_seconds if self.searcher.last_seconds else 0.0
        lines = ["info speed %f nps" % (speed,)]
        if getattr(self.searcher, "last_note", None):
            lines.append("info string %s" % (self.searcher.last_note,))
        if getattr(self.searcher, "last_proven", None):
            lines.append("info string proven %s" % (self.searcher.last_proven,))
        if getattr(self.searcher, "show_pv", False) and self.searcher.pv_line():
            lines.append(self.searcher.pv_line())
        return lines + ["bestmove %s" % (encode_move(move),)]

    def handle(self, line):
        """-> (lines to print, keep going)."""
        if line == "quit":
            return [], False
        for prefix, handler in self.table:
            exact = not prefix.endswith(" ")
            if (line == prefix) if exact else line.startswith(prefix):
                return handler(line[len(prefix):]), True
        return [], True  # unknown commands are ignored, as the reference does

    def serve(self, source, sink):
        for raw in source:
            out, more = self.handle(raw.rstrip("\n"))
            for text in out:
                print(text, file=sink)
            sink.flush()
            if not more:
                break
