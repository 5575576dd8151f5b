"""Plain numpy restatement of first-play urgency and the growing exploration rate of the leaf-parallel search (DESIGN.md,
"First-play urgency and the exploration rate"), on top of tests/vl_reference.py and tests/solver_reference.py, whose
arrays-in / arrays-out style it keeps.

scores() is one level's arithmetic: with r = fpu_reduction, at a node whose children hold the effective counts n (N their
sum), total scores W and priors P,
    sq = sqrt(1 + N)
    c  = logf(((1 + N) + c_base) / c_base) + c_init   if c_base > 0, else c_puct
    f  = max(wave_sum(W) / N - r * sqrt(wave_sum(P over the visited children)), 0)   if r >= 0 and N > 0, else 0 (a NaN: 0)
    score_j = (sq / (1 + n_j)) * (c * P_j) + (W_j / n_j if n_j else f)
every operation a single f32 one, the two sums in the engine's lane order (priors_reference.wave_sum), the logarithm the
oracle's deterministic one.  With r < 0 and c_base == 0 it is vl_reference.puct_scores.

select() is solver_reference.select — with no proven node vl_reference.select, step for step — with scores() in the place of
puct_scores: one more way to score a level, nothing else.  Its Batch goes to vl_reference.backup / expected_tree or to
solver_reference's, as the run has the solver off or on.
"""
import numpy as np

from oracle import oracle_lib as orc
from tests import priors_reference as pr
from tests import solver_reference as sr
from tests import vl_reference as vlr

F32 = np.float32
NONE = vlr.NONE
OFF = (-1.0, 0.0, 0.0)


def mode_on(r, c_base):
    return r >= 0 or c_base > 0


def logf(x):
    return F32(orc.lib().orc_probe_logf(float(F32(x))))


def rate(N, c_puct, c_base, c_init):
    """c of a node whose children hold N effective visits."""
    if not c_base > 0:
        return F32(c_puct)
    cb = F32(c_base)
    return F32(logf(F32(F32(F32(1 + int(N)) + cb) / cb)) + F32(c_init))


def fpu(prior, W, n, N, r):
    """f: the Q of the node's unvisited children."""
    if not r >= 0 or int(N) == 0:
        return F32(0.0)
    with np.errstate(all="ignore"):
        wsum = pr.wave_sum(np.asarray(W, dtype=np.float32))
        psum = pr.wave_sum(np.array([abs(F32(p)) if int(nj) else F32(0.0) for p, nj in zip(prior, n)], dtype=np.float32))
        qx = F32(wsum / F32(int(N)))
        f = F32(qx - F32(F32(r) * np.sqrt(psum)))
    return f if f > 0 else F32(0.0)


def scores(prior, W, n, N, c_puct, r, c_base, c_init):
    """The M scores of one node (f32).  N: the sum of n."""
    sq = np.sqrt(F32(1 + int(N)))
    c, f = F32(c_puct), F32(0.0)
    if mode_on(r, c_base):
        c, f = rate(N, c_puct, c_base, c_init), fpu(prior, W, n, N, r)
    out = np.empty(len(n), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(len(n)):
            nj = int(n[j])
            q = F32(W[j]) / F32(nj) if nj else f
            u = (sq / (F32(1.0) + F32(nj))) * (c * abs(F32(prior[j])))
            out[j] = F32(u + q)
    return out


def select(tree, root_visits, visits, K, VL, c_puct, tie_first, blockers, r, c_base, c_init):
    """solver_reference.select (every proven node but the root ends a path like a finished position; none proven:
    vl_reference.select) with scores() for the level.  -> vl_reference's Batch with solver_reference's .nodes0 and
    .proven_hits."""
    boards, info, edges, moves = tree
    boards = [tuple(int(v) for v in b) for b in boards]
    info = [list(int(v) for v in row) for row in np.array(info, dtype=np.uint32).reshape(-1, 4)]
    marked = {x for x in range(1, len(info)) if sr.is_proven(info[x])}
    prior = [int(e[0]) for e in edges]
    n = [int(e[1]) for e in edges]
    W = [int(e[2]) for e in edges]
    child = [int(e[3]) for e in edges]
    mv = [int(m) for m in moves]
    nodes0, edges0 = len(boards), len(n)
    vl = [0] * len(n)
    k = max(1, min(K, visits - root_visits))
    b = vlr.Batch()
    b.kind, b.leaf_edge, b.leaf_board, b.paths, b.leaf_node = [], [], [], [], []
    b.over = False
    for p in range(k):
        node, path = 0, []
        while True:
            first, M, res = info[node][0], info[node][1] & 0xFFFF, info[node][1] >> 16
            if res != 0 or M == 0 or node in marked:
                kind = vlr.LEAF_TERMINAL
                break
            if node >= nodes0:
                kind = vlr.LEAF_COLLISION
                break
            rng = range(first, first + M)
            ne = [n[e] + VL * vl[e] for e in rng]
            sc = scores([vlr._f(prior[e]) for e in rng], [vlr._f(W[e]) for e in rng], ne, sum(ne), c_puct, r, c_base, c_init)
            e = first + vlr.pick(sc, tie_first)
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
                    prior.append(0), n.append(0), W.append(0), child.append(NONE), mv.append(int(m)), vl.append(0)
                kind = vlr.LEAF_EVAL
            child[e] = cid
            node = cid
            break
        for e in path:
            vl[e] += 1
        b.kind.append(kind)
        b.leaf_edge.append(path[-1] if path else NONE)
        b.leaf_node.append(node)
        b.leaf_board.append(vlr.leaf_board(*boards[node]) if kind == vlr.LEAF_EVAL else (0, 0))
        b.paths.append(path)
    b.edges0, b.nodes0 = edges0, nodes0
    b.boards, b.info, b.prior, b.n, b.W, b.child, b.moves = boards, info, prior, n, W, child, mv
    b.proven_hits = sum(1 for p, kd in enumerate(b.kind) if kd == vlr.LEAF_TERMINAL and b.leaf_node[p] in marked)
    return b
