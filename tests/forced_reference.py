"""Plain numpy restatement of forced playouts and policy target pruning ("Forced playouts and policy target
pruning"; include/ataxxzero_hip.h, azh_engine_set_forced_playouts).

It works on the arrays Engine.tree(g) returns, like tests/vl_reference.py, whose PUCT scores, tie rule, expansion and backup
it reuses: select() takes one path — the root level by the forced-playout rule, every level below it the one-leaf PUCT
descent — and prune() gives the visit counts a ply's record carries, by the loop of the definition.  Every f32 operation is a
single numpy float32 operation in the order the definition writes it.
"""
import numpy as np

from tests import vl_reference as vlr

F32 = np.float32
NONE = vlr.NONE


def bound(prior, N, k):
    """sqrtf((k * P) * (float)N): the visits an edge of prior P is owed at N root visits, as a real number"""
    return np.sqrt(F32(F32(k) * F32(prior)) * F32(int(N)))


def owed(prior, n, N, k):
    """mask of the root edges that are owed a visit: n >= 1 and (float)n < sqrtf((k * P) * (float)N)"""
    return np.array([int(nj) >= 1 and F32(int(nj)) < bound(pj, N, k) for pj, nj in zip(prior, n)], dtype=bool)


def select(tree, root_visits, k, full, c_puct, tie_first, blockers):
    """One path of a game in search phase 1 -> a vl_reference.Batch of one slot (kind, leaf_edge, leaf_node, leaf_board,
    paths and the working tree: vl_reference.backup and expected_tree take it), with .owed (the root's owed mask; empty
    mask on a ply the mode does not act on), .forced (the root edge index taken by the rule, or None) and .puct (the
    root's PUCT arg-max)."""
    boards, info, edges, moves = tree
    boards = [tuple(int(v) for v in b) for b in boards]
    info = [list(int(v) for v in r) for r in info]
    prior = [int(e[0]) for e in edges]
    n = [int(e[1]) for e in edges]
    W = [int(e[2]) for e in edges]
    child = [int(e[3]) for e in edges]
    mv = [int(m) for m in moves]
    b = vlr.Batch()
    b.edges0 = len(n)
    b.owed, b.forced, b.puct = np.zeros(0, dtype=bool), None, None
    node, path = 0, []
    while True:
        first, M, res = info[node][0], info[node][1] & 0xFFFF, info[node][1] >> 16
        if res != 0 or M == 0:
            kind = vlr.LEAF_TERMINAL
            break
        rng = range(first, first + M)
        pr = [vlr._f(prior[e]) for e in rng]
        ne = [n[e] for e in rng]
        sc = vlr.puct_scores(pr, [vlr._f(W[e]) for e in rng], ne, sum(ne), c_puct)
        j = vlr.pick(sc, tie_first)
        if node == 0:
            b.puct = j
            if k > 0 and full:
                b.owed = owed(pr, ne, root_visits, k)
                idx = np.nonzero(b.owed)[0]
                if len(idx):
                    j = b.forced = int(idx[0] if tie_first else idx[-1])
        e = first + j
        path.append(e)
        if child[e] != NONE:
            node = child[e]
            continue
        cb, res2, mvs, tv = vlr.expand_position(boards[node][0], boards[node][1], mv[e], blockers)
        cid = len(boards)
        boards.append(cb)
        if res2 != 0:
            info.append([0, res2 << 16, 0, tv])
            kind = vlr.LEAF_TERMINAL
        else:
            info.append([len(n), len(mvs), 0, 0])
            for m in mvs:
                prior.append(0), n.append(0), W.append(0), child.append(NONE), mv.append(int(m))
            kind = vlr.LEAF_EVAL
        child[e] = cid
        node = cid
        break
    b.kind, b.leaf_edge, b.leaf_node, b.paths = [kind], [path[-1] if path else NONE], [node], [path]
    b.leaf_board = [vlr.leaf_board(*boards[node]) if kind == vlr.LEAF_EVAL else (0, 0)]
    b.boards, b.info, b.prior, b.n, b.W, b.child, b.moves = boards, info, prior, n, W, child, mv
    return b


def best_edge(n):
    """the root edge with the most visits, ties to the lowest index"""
    return int(np.argmax(np.asarray(n, dtype=np.int64)))


def score(prior, q, m, sq, c_puct):
    """((sq / (1.0f + (float)m)) * (c_puct * P)) + q"""
    return F32(F32(F32(sq) / F32(F32(1.0) + F32(int(m)))) * F32(F32(c_puct) * F32(prior))) + F32(q)


def prune_parts(prior, W, n, k, c_puct):
    """-> (written counts m (M,) u32, f (M,) the visits each edge may lose, S the best edge's score, sq, b)"""
    n = [int(v) for v in n]
    M, N = len(n), sum(n)
    out = np.array(n, dtype=np.uint32)
    f = np.zeros(M, dtype=np.int64)
    if M == 0:
        return out, f, F32(0.0), F32(1.0), 0
    sq = np.sqrt(F32(1 + N))
    b = best_edge(n)
    S = vlr.puct_scores([F32(prior[b])], [F32(W[b])], [n[b]], N, c_puct)[0]
    for j in range(M):
        if j == b or n[j] < 1:
            continue
        f[j] = int(np.floor(bound(prior[j], N, k)))
        q = F32(W[j]) / F32(n[j])
        m = n[j]
        for _ in range(int(f[j])):
            if m >= 1 and score(prior[j], q, m - 1, sq, c_puct) < S:
                m -= 1
            else:
                break
        if m < n[j] and m <= 1:
            m = 0
        out[j] = m
    return out, f, S, sq, b


def prune(prior, W, n, k, c_puct):
    """the visit counts written into the ply's record ((M,) u32; 0: the edge is left out), by the loop as defined"""
    return prune_parts(prior, W, n, k, c_puct)[0]


def root_arrays(tree):
    """(prior f32, W f32, n u32, moves u16, child) of the root's edges of an Engine.tree dump"""
    _, info, edges, moves = tree
    first, M = int(info[0][0]), int(info[0][1]) & 0xFFFF
    e = np.ascontiguousarray(edges[first:first + M])
    return (e[:, 0].copy().view(np.float32), e[:, 2].copy().view(np.float32), e[:, 1].copy(), moves[first:first + M].copy(),
            e[:, 3].copy())
