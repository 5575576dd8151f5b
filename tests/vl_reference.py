"""Plain numpy restatement of the leaf-parallel search with virtual loss ("Leaf-parallel search").

It works on the arrays Engine.tree(g) returns — boards (n, 2) u64 packed (x | turn << 63, o), info (n, 4) u32
(first edge, n_edges | result << 16, 0, terminal value bits), edges (m, 4) u32 (prior bits, visits, W bits, child or
0xFFFFFFFF), moves (m,) u16 — and on the rules of the repository's oracle (oracle/oracle_lib.py) for the nodes a path
expands.  select() gives each slot's kind, leaf edge and leaf board; backup() the edge words after the backup.  Priors of
new nodes are not restated here: backup() takes them from the engine's dump, and tests/priors_reference.py restates them.

The arena-full rule (select with node_cap / edge_cap): a path that would expand a node the arenas cannot hold — the
game has node_cap nodes already, or the unfinished child's M2 edges do not fit (n_edges + M2 > edge_cap) or are more than
255 — is DROPPED: kind NONE, its leaf edge the edge it stood on, no node and no edge added, and it keeps its virtual loss
until the backup like every other path of the batch.  The batch ends with it (no later path is selected), and the game's
move is FORCED: after this batch's backup the move is due whatever the root's visit count, and the next select plays it
— forced_move() below, the ordinary draw proportional to the root edges' visits.
"""
import ctypes

import numpy as np

from oracle import oracle_lib as orc

NONE = 0xFFFFFFFF
LEAF_NONE, LEAF_EVAL, LEAF_TERMINAL, LEAF_ROOT, LEAF_COLLISION = 0, 1, 2, 3, 5
WIN_BITS, LOSS_BITS = 0x3F800000, 0xBF800000   # +1.0f, -1.0f: info word 3 of a proven node
F32 = np.float32


def _f(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def _bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def expand_position(word0, word1, move, blockers):
    """(packed child board, result, legal moves, terminal value bits) after `move` — make_node's view of a new node."""
    p = orc.Pos()
    p.pieces[0] = int(word0) & ~(1 << 63)
    p.pieces[1] = int(word1)
    p.blockers = int(blockers)
    p.turn = int(word0) >> 63
    orc.lib().orc_makemove(ctypes.byref(p), int(move) & 0xFF, int(move) >> 8)
    moves = np.zeros(256, dtype=np.uint16)
    m = ctypes.c_int(0)
    res = orc.lib().orc_result(ctypes.byref(p), moves.ctypes.data, ctypes.byref(m))
    tv = 0
    if res != 0:
        v = F32(1.0) if res == 1 else F32(-1.0)
        tv = _bits(-v if p.turn == 1 else v)
    packed = (int(p.pieces[0]) | (int(p.turn) << 63), int(p.pieces[1]))
    return packed, res, (moves[:m.value].copy() if res == 0 else np.zeros(0, np.uint16)), tv


def leaf_board(word0, word1):
    x, o, turn = int(word0) & ~(1 << 63), int(word1), int(word0) >> 63
    return (o, x) if turn else (x, o)


def puct_scores(prior, W, n, N, c_puct):
    """total_action_score (:310-324) in f32, the oracle's operation order."""
    sq = np.sqrt(F32(1 + int(N)))
    out = np.empty(len(n), dtype=np.float32)
    c = F32(c_puct)
    for j in range(len(n)):
        nj = int(n[j])
        q = F32(W[j]) / F32(nj) if nj else F32(0.0)
        u = (sq / (F32(1.0) + F32(nj))) * (c * F32(prior[j]))
        out[j] = F32(u + q)
    return out


def pick(scores, tie_first):
    best, bj = None, -1
    for j, s in enumerate(scores):
        if np.isnan(s):
            continue
        if best is None or s > best or (s == best and not tie_first):
            best, bj = s, j
    return max(bj, 0)


class Batch:
    """One iteration's selected batch and the working tree it left (virtual losses kept apart)."""


def is_proven(info_row):
    """Decided without being a finished position: result bits 0 and the bits of +1.0f or -1.0f in info word 3
    (tests/solver_reference.py)."""
    return (int(info_row[1]) >> 16) == 0 and int(info_row[3]) in (WIN_BITS, LOSS_BITS)


def select(tree, root_visits, visits, K, VL, c_puct, tie_first, blockers, node_cap=None, edge_cap=None, *,
           proven_end_paths=False, scores=None):
    """The batch of one game in search phase 1: k = max(1, min(K, visits - root_visits)) paths as if one after the other.
    node_cap, edge_cap: the arenas' sizes (both None: unbounded) — the arena-full rule of the module's docstring.
    proven_end_paths: a path ends at a proven node as at a finished position (TERMINAL), the root excepted — the descent of
    tests/solver_reference.py.  scores(priors, W, n, N) -> the M f32 scores of a level, n the effective visits
    n + VL * vl and N their sum; the default is puct_scores with c_puct (tests/exploration_reference.py has another).
    -> Batch with .kind, .leaf_edge (NONE: none), .leaf_board (mover, opponent; (0, 0) unless EVAL), .paths, .leaf_node,
    .over (a path was dropped: the batch ended there and the move is forced), .nodes0 (nodes from this id on were created
    by this batch) and .proven_hits (the paths that ended at a proven node)."""
    boards, info, edges, moves = tree
    boards = [tuple(int(v) for v in b) for b in boards]
    info = [list(int(v) for v in r) for r in info]
    marked = {x for x in range(1, len(info)) if is_proven(info[x])} if proven_end_paths else set()
    if scores is None:
        def scores(P, W, n, N):
            return puct_scores(P, W, n, N, c_puct)
    prior = [int(e[0]) for e in edges]
    n = [int(e[1]) for e in edges]
    W = [int(e[2]) for e in edges]
    child = [int(e[3]) for e in edges]
    mv = [int(m) for m in moves]
    nodes0, edges0 = len(boards), len(n)
    vl = [0] * len(n)
    k = max(1, min(K, visits - root_visits))
    b = Batch()
    b.kind, b.leaf_edge, b.leaf_board, b.paths, b.leaf_node = [], [], [], [], []
    b.over = False
    capped = node_cap is not None or edge_cap is not None
    for p in range(k):
        node, path = 0, []
        while True:
            first, M, res = info[node][0], info[node][1] & 0xFFFF, info[node][1] >> 16
            if res != 0 or M == 0 or node in marked:
                kind = LEAF_TERMINAL
                break
            if node >= nodes0:
                kind = LEAF_COLLISION
                break
            rng = range(first, first + M)
            ne = [n[e] + VL * vl[e] for e in rng]
            sc = scores([_f(prior[e]) for e in rng], [_f(W[e]) for e in rng], ne, sum(ne))
            e = first + pick(sc, tie_first)
            path.append(e)
            if child[e] != NONE:
                node = child[e]
                continue
            cb, res2, mvs, tv = expand_position(boards[node][0], boards[node][1], mv[e], blockers)
            if capped and ((node_cap is not None and len(boards) >= node_cap) or
                           (res2 == 0 and ((edge_cap is not None and len(n) + len(mvs) > edge_cap) or len(mvs) > 255))):
                kind = LEAF_NONE   # dropped: the path stays at `node`, on the edge it stood on
                b.over = True
                break
            cid = len(boards)
            boards.append(cb)
            if res2 != 0:
                info.append([0, res2 << 16, 0, tv])
                kind = LEAF_TERMINAL
            else:
                info.append([len(n), len(mvs), 0, 0])
                for m in mvs:
                    prior.append(0), n.append(0), W.append(0), child.append(NONE), mv.append(int(m)), vl.append(0)
                kind = LEAF_EVAL
            child[e] = cid
            node = cid
            break
        for e in path:
            vl[e] += 1
        b.kind.append(kind)
        b.leaf_edge.append(path[-1] if path else NONE)
        b.leaf_node.append(node)
        b.leaf_board.append(leaf_board(*boards[node]) if kind == LEAF_EVAL else (0, 0))
        b.paths.append(path)
        if b.over:
            break
    b.nodes0, b.edges0 = nodes0, edges0
    b.proven_hits = sum(1 for p, kd in enumerate(b.kind) if kd == LEAF_TERMINAL and b.leaf_node[p] in marked)
    b.boards, b.info, b.prior, b.n, b.W, b.child, b.moves = boards, info, prior, n, W, child, mv
    return b


def backup(b, values):
    """Edge words (prior bits, visits, W bits, child) after the batch's backup; values[p] is slot p's evaluation.  EVAL and
    TERMINAL paths in path order, each step() part 4 (:449-459); COLLISION paths add nothing.  -> (edges (m, 4) u32 with
    prior 0 for the batch's new edges, root visits added)."""
    n, W = list(b.n), list(b.W)
    added = 0
    for p, path in enumerate(b.paths):
        kind = b.kind[p]
        if kind not in (LEAF_EVAL, LEAF_TERMINAL):
            continue
        v = F32(values[p]) if kind == LEAF_EVAL else _f(b.info[b.leaf_node[p]][3])
        sc = F32((v + F32(1.0)) * F32(0.5))
        for e in reversed(path):
            sc = F32(F32(1.0) - sc)
            W[e] = _bits(F32(_f(W[e]) + sc))
            n[e] += 1
        added += 1 if path else 0
    out = np.zeros((len(n), 4), dtype=np.uint32)
    out[:, 0] = b.prior
    out[:, 1] = n
    out[:, 2] = W
    out[:, 3] = b.child
    return out, added


def move_is_due(b, root_visits_after, visits):
    """After the batch's backup: the game's move is due — the root has its visits, or the batch dropped a path."""
    return root_visits_after >= visits or b.over


def forced_move(tree, root_visits, seed, uid, ply):
    """The move the select after a due move plays (flags without SAMPLE_POW5 / ONE_RANDOM_MOVE): the draw proportional to
    the root edges' visits, r = (philox(seed; uid, ply, stream 1, 0)[0] * root_visits) >> 32 against the running sum of the
    visits in edge order — the first edge whose running sum exceeds r; edge 0 if there is none (a root without a visit).
    -> (edge index, move)."""
    boards, info, edges, moves = tree
    first, M = int(info[0][0]), int(info[0][1]) & 0xFFFF
    out = (ctypes.c_uint32 * 4)()
    orc.lib().orc_probe_philox(int(seed), int(uid), int(ply), 1, 0, out)
    r = (int(out[0]) * int(root_visits)) >> 32
    cum, chosen = 0, -1
    for j in range(M):
        cum += int(edges[first + j][1])
        if chosen < 0 and cum > r:
            chosen = j
    chosen = max(chosen, 0)
    return chosen, int(moves[first + chosen])


def expected_tree(b, values, post_tree):
    """The whole dump after the backup: boards, info and edges restated, the priors of the batch's new edges taken from
    `post_tree` (the engine's); every other prior is unchanged."""
    edges, added = backup(b, values)
    if len(post_tree[2]) == len(edges):
        edges[b.edges0:, 0] = post_tree[2][b.edges0:, 0]
    boards = np.array(b.boards, dtype=np.uint64).reshape(-1, 2)
    info = np.array(b.info, dtype=np.uint32).reshape(-1, 4)
    moves = np.array(b.moves, dtype=np.uint16)
    return (boards, info, edges, moves), added
