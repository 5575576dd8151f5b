"""Plain numpy restatement of the Gumbel root search with sequential halving ("Gumbel root search with sequential
halving"; include/ataxxzero_hip.h, azh_engine_set_gumbel).

It works on the arrays Engine.tree(g) returns, like tests/vl_reference.py, whose PUCT scores, tie rule, expansion and backup
it reuses, as tests/forced_reference.py does: select() takes one path — the root level by the schedule's rule, every level
below it the one-leaf PUCT descent — and root() gives the move a ply plays and the counts its record carries.  Every f32
operation is a single numpy float32 operation in the order the definition writes it; the logarithm, the exponential and
Philox are the oracle's probes (held bit for bit against the device by test_detmath_bits_match_oracle and, at the edges and over
the Gumbel draw's whole grid, by tests/test_gpu_detmath_edges.py), the 64-lane sum is
tests/priors_reference.wave_sum.
"""
import ctypes

import numpy as np

from oracle import oracle_lib as orc
from tests import priors_reference as pr
from tests import vl_reference as vlr

F32 = np.float32
NONE = vlr.NONE
STREAM_GUMBEL = 7


def seq(r, V):
    """the considered visit counts for r considered actions and V simulations"""
    if r <= 1:
        return list(range(V))
    L = int(np.ceil(np.log2(r)))
    assert 2 ** (L - 1) < r <= 2 ** L
    k, visits, out = r, [0] * r, []
    while len(out) < V:
        extra = max(1, V // (L * k))
        for _ in range(extra):
            out.extend(visits[:k])
            for i in range(k):
                visits[i] += 1
        k = max(2, k // 2)
    return out[:V]


def logf(x):
    return F32(orc.lib().orc_probe_logf(float(F32(x))))


def noise(seed, uid, ply, M):
    """g_j = -logf(-logf(u)), u = ((float)(x >> 9) + 0.5f) * 2^-23, x = word 0 of philox(seed; uid, ply, 7, j) -> (M,) f32"""
    out = np.zeros(M, dtype=np.float32)
    w = (ctypes.c_uint32 * 4)()
    for j in range(M):
        orc.lib().orc_probe_philox(int(seed), int(uid), int(ply), STREAM_GUMBEL, j, w)
        u = F32(F32(F32(int(w[0]) >> 9) + F32(0.5)) * F32(2.0 ** -23))
        assert 0.0 < u < 1.0
        out[j] = -logf(-logf(u))
    return out


def logit(prior):
    """l_j = P_j > 0 ? logf(P_j) : -inf"""
    return logf(prior) if F32(prior) > 0 else F32(-np.inf)


def a_values(prior, g):
    """a_j = g_j + l_j -> (M,) f32"""
    with np.errstate(all="ignore"):
        return np.array([F32(F32(gj) + logit(pj)) for pj, gj in zip(prior, g)], dtype=np.float32)


def ks_of(n, c_visit, c_scale):
    n_max = max([int(v) for v in n], default=0)
    with np.errstate(all="ignore"):
        return F32(F32(F32(c_visit) + F32(n_max)) * F32(c_scale))


def score(a, W, n, ks):
    """s_j = n_j >= 1 ? a_j + ks * (W_j / (float)n_j) : a_j"""
    with np.errstate(all="ignore"):
        if int(n) < 1:
            return F32(a)
        return F32(F32(a) + F32(F32(ks) * F32(F32(W) / F32(int(n)))))


def best(scores, mask):
    """the masked edge with the greatest score: a NaN never wins, equal scores go to the lowest index; None if none wins"""
    top, bj = None, None
    for j, (s, ok) in enumerate(zip(scores, mask)):
        if not ok or np.isnan(s):
            continue
        if top is None or s > top:
            top, bj = s, j
    return bj


def root_choice(a, W, n, cv, c_visit, c_scale):
    """the root edge a fresh descent takes when the schedule's entry is cv, or None (the PUCT level)"""
    ks = ks_of(n, c_visit, c_scale)
    return best([score(aj, Wj, nj, ks) for aj, Wj, nj in zip(a, W, n)], [int(nj) == int(cv) for nj in n])


def select(tree, root_visits, visits, m, a, c_visit, c_scale, c_puct, tie_first, blockers):
    """One path of a game in search phase 1 -> a vl_reference.Batch of one slot (vl_reference.backup and expected_tree take
    it), with .gumbel (the root edge taken by the rule, or None: the PUCT level), .puct (the root's PUCT arg-max), .cv (the
    schedule's entry, or None past its end) and .root_edge (the root edge index the path took)."""
    boards, info, edges, moves = tree
    boards = [tuple(int(v) for v in b) for b in boards]
    info = [list(int(v) for v in r) for r in info]
    prior = [int(e[0]) for e in edges]
    n = [int(e[1]) for e in edges]
    W = [int(e[2]) for e in edges]
    child = [int(e[3]) for e in edges]
    mv = [int(x) for x in moves]
    b = vlr.Batch()
    b.edges0 = len(n)
    b.gumbel, b.puct, b.cv, b.root_edge = None, None, None, None
    node, path = 0, []
    while True:
        first, M, res = info[node][0], info[node][1] & 0xFFFF, info[node][1] >> 16
        if res != 0 or M == 0:
            kind = vlr.LEAF_TERMINAL
            break
        rng = range(first, first + M)
        ne = [n[e] for e in rng]
        sc = vlr.puct_scores([vlr._f(prior[e]) for e in rng], [vlr._f(W[e]) for e in rng], ne, sum(ne), c_puct)
        j = vlr.pick(sc, tie_first)
        if node == 0:
            b.puct = j
            if m > 0 and root_visits < visits:
                b.cv = seq(min(m, M), visits)[root_visits]
                b.gumbel = root_choice(a, [vlr._f(W[e]) for e in rng], ne, b.cv, c_visit, c_scale)
                if b.gumbel is not None:
                    j = b.gumbel
            b.root_edge = j
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
            for x in mvs:
                prior.append(0), n.append(0), W.append(0), child.append(NONE), mv.append(int(x))
            kind = vlr.LEAF_EVAL
        child[e] = cid
        node = cid
        break
    b.kind, b.leaf_edge, b.leaf_node, b.paths = [kind], [path[-1] if path else NONE], [node], [path]
    b.leaf_board = [vlr.leaf_board(*boards[node]) if kind == vlr.LEAF_EVAL else (0, 0)]
    b.boards, b.info, b.prior, b.n, b.W, b.child, b.moves = boards, info, prior, n, W, child, mv
    return b


def next_mark(tree, mark, j):
    """The root's prefetch mark (the edge index carrying it, or None) after a descent took root edge j of the tree `tree` as it
    stood BEFORE the descent: an edge without a child is being expanded and moves nothing; nor does a root of more than 128
    edges, nor the marked edge chosen again; else the old mark goes, and the new edge gets one iff its child is an unfinished
    position of 1 .. 128 moves."""
    _, info, edges, _ = tree
    first, M = int(info[0][0]), int(info[0][1]) & 0xFFFF
    c = int(edges[first + j][3])
    if c == NONE or M > 128 or j == mark:
        return mark
    cm, cres = int(info[c][1]) & 0xFFFF, int(info[c][1]) >> 16
    return j if cres == 0 and 1 <= cm <= 128 else None


def root(prior, W, n, v0, g, c_visit, c_scale):
    """The ply played from a root: -> (edge of the move, counts (M,) u32 of its record; 0: the edge is left out)."""
    with np.errstate(all="ignore"):
        n = [int(v) for v in n]
        M, N = len(n), sum(n)
        n_max = max(n)
        ks = ks_of(n, c_visit, c_scale)
        a = a_values(prior, g)
        move = best([score(a[j], W[j], n[j], ks) for j in range(M)], [v == n_max for v in n])
        move = 0 if move is None else move
        q = [F32(F32(W[j]) / F32(n[j])) if n[j] >= 1 else None for j in range(M)]
        sp = pr.wave_sum([F32(prior[j]) if n[j] >= 1 else F32(0.0) for j in range(M)])
        sw = pr.wave_sum([F32(F32(prior[j]) * q[j]) if n[j] >= 1 else F32(0.0) for j in range(M)])
        if sp > 0:
            v_mix = F32(F32(F32(v0) + F32(F32(F32(N) / sp) * sw)) / F32(F32(1.0) + F32(N)))
        else:
            v_mix = F32(v0)
        x = np.array([F32(logit(prior[j]) + F32(ks * (q[j] if n[j] >= 1 else v_mix))) for j in range(M)], dtype=np.float32)
        x_max = pr._max(x)
        w = (pr.expf((x - x_max).astype(np.float32)) * F32(65535.0)).astype(np.float32)
        counts = np.array([min(int(v), 65535) for v in w], dtype=np.uint32)
        if not counts.any():
            counts[move] = 65535     # no count at all: the record carries the move played, alone
        return move, counts


def improved_policy(prior, W, n, v0, c_visit, c_scale):
    """softmax(l + ks completedQ) in float64 from the same inputs: what the counts quantise (for the property tests)"""
    n = np.asarray(n, dtype=np.int64)
    P, W = np.asarray(prior, dtype=np.float64), np.asarray(W, dtype=np.float64)
    ks = (c_visit + n.max()) * c_scale
    vis = n >= 1
    q = np.where(vis, W / np.maximum(n, 1), 0.0)
    sp = P[vis].sum()
    v_mix = (v0 + n.sum() / sp * (P[vis] * q[vis]).sum()) / (1 + n.sum()) if sp > 0 else v0
    with np.errstate(all="ignore"):
        x = np.log(P) + ks * np.where(vis, q, v_mix)
    e = np.exp(x - x.max())
    return e / e.sum()
