"""Plain numpy restatement of first-play urgency and the growing exploration rate of the leaf-parallel search (DESIGN.md,
"First-play urgency and the exploration rate"), on top of tests/vl_reference.py, whose arrays-in / arrays-out
style it keeps.

scores() is one level's arithmetic: with r = fpu_reduction, at a node whose children hold the effective counts n (N their
sum), total scores W and priors P,
    sq = sqrt(1 + N)
    c  = logf(((1 + N) + c_base) / c_base) + c_init   if c_base > 0, else c_puct
    f  = max(wave_sum(W) / N - r * sqrt(wave_sum(P over the visited children)), 0)   if r >= 0 and N > 0, else 0 (a NaN: 0)
    score_j = (sq / (1 + n_j)) * (c * P_j) + (W_j / n_j if n_j else f)
every operation a single f32 one, the two sums in the engine's lane order (priors_reference.wave_sum), the logarithm the
oracle's deterministic one.  With r < 0 and c_base == 0 it is vl_reference.puct_scores.

select() is vl_reference.select — the one descent — with scores() in the place of puct_scores and proven nodes ending paths
as under the solver: one more way to score a level, nothing else.  Its Batch goes to vl_reference.backup / expected_tree or
to solver_reference's, as the run has the solver off or on.
"""
import numpy as np

from oracle import oracle_lib as orc
from tests import priors_reference as pr
from tests import vl_reference as vlr

F32 = np.float32
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




def select(tree, root_visits, visits, K, VL, c_puct, tie_first, blockers, r, c_base, c_init, node_cap=None, edge_cap=None):
    """vl_reference.select with scores() for the level and every proven node but the root ending a path like a finished
    position (none proven: nothing ends differently)."""
    return vlr.select(tree, root_visits, visits, K, VL, c_puct, tie_first, blockers, node_cap, edge_cap, proven_end_paths=True,
                      scores=lambda P, W, n, N: scores(P, W, n, N, c_puct, r, c_base, c_init))
