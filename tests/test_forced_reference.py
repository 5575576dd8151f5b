"""Policy target pruning without a device: the library's host export (azh_forced_prune, the per-edge function the device's
ply record uses) against the numpy restatement (tests/forced_reference.py) on synthetic roots, and the properties of the
restatement itself."""
import numpy as np
import pytest

from ataxxzero_amd import link
from tests import forced_reference as fr
from tests import vl_reference as vlr

F32 = np.float32
C_PUCT = 1.0
SIZES = (1, 2, 63, 64, 65, 128, 129, 200)
KS = (0.5, 2.0, 8.0)
SEED = 20261017   # (chosen so that the sample holds all four kinds of edge, by the restatement alone: test below)


def _roots(per_case=84):
    """A few thousand roots as a search leaves them: priors from a Dirichlet with Dirichlet noise mixed in (weight 0.25),
    N <= 800 visits spread roughly in proportion to prior times a per-edge preference, total scores n q with q around the
    edge's worth.  -> [(prior, W, n, k)]"""
    rng = np.random.default_rng(SEED)
    out = []
    for M in SIZES:
        for k in KS:
            for _ in range(per_case):
                p = rng.dirichlet(np.full(M, 0.6)).astype(np.float32)
                noise = rng.dirichlet(np.full(M, 0.15)).astype(np.float32)
                prior = (F32(0.25) * noise + F32(0.75) * p).astype(np.float32)
                N = int(rng.integers(0, 801))
                worth = rng.uniform(0.15, 0.85, size=M)
                pull = prior.astype(np.float64) * np.exp(4.0 * (worth - 0.5)) + 1e-12
                n = rng.multinomial(N, pull / pull.sum()).astype(np.uint32)
                q = np.clip(worth + rng.normal(0.0, 0.08, size=M), 0.0, 1.0)
                W = (n * q).astype(np.float32)
                out.append((prior, W, n, k))
    return out


@pytest.fixture(scope="module")
def roots():
    return _roots()


@pytest.fixture(scope="module")
def parts(roots):
    return [fr.prune_parts(prior, W, n, k, C_PUCT) for prior, W, n, k in roots]


def test_the_host_export_equals_the_restatement(roots, parts):
    assert len(roots) >= 2000
    for (prior, W, n, k), (want, _, _, _, _) in zip(roots, parts):
        got = link.forced_prune(prior, W, n, k, C_PUCT)
        assert got.dtype == np.uint32 and (got == want).all(), (len(n), k, int(n.sum()))
    # the prior's sign bit is the descent's mark in the device's records: the rule reads the magnitude
    prior, W, n, k = roots[len(roots) // 2]
    assert (link.forced_prune(-prior, W, n, k, C_PUCT) == fr.prune(prior, W, n, k, C_PUCT)).all()
    for bad in (-1.0, float("nan")):
        with pytest.raises(link.AzhError):
            link.forced_prune(prior, W, n, bad, C_PUCT)
    assert len(link.forced_prune(prior[:0], W[:0], n[:0], 2.0, C_PUCT)) == 0


def test_properties_of_the_restatement(roots, parts):
    kinds = {"untouched": 0, "full": 0, "bound": 0, "zero": 0}
    for (prior, W, n, k), (m, f, S, sq, b) in zip(roots, parts):
        n64, m64 = n.astype(np.int64), m.astype(np.int64)
        if len(n) == 0:
            continue
        assert b == int(np.argmax(n64)) and m64[b] == n64[b]                 # the best edge is untouched
        for j in range(len(n)):
            if j == b or n64[j] == 0:
                assert m64[j] == n64[j]
                continue
            taken = n64[j] - m64[j]
            q = F32(W[j]) / F32(n64[j])
            if m64[j] == 0 and taken > 0:
                # pruned to 0: the loop stopped at 0 or 1 (one left over is dropped too)
                kinds["zero"] += 1
                assert n64[j] - 1 <= f[j]
                continue
            assert 0 <= taken <= f[j]
            assert m64[j] != 1 or taken == 0                                   # nothing ends at 1 after a reduction
            if taken == 0:
                kinds["untouched"] += 1
                assert f[j] == 0 or not fr.score(prior[j], q, m64[j] - 1, sq, C_PUCT) < S
                continue
            # reduced: every visit taken left the edge below S; it stopped at the bound or used all it may lose
            assert fr.score(prior[j], q, m64[j], sq, C_PUCT) < S
            if taken == f[j]:
                kinds["full"] += 1
            else:
                kinds["bound"] += 1
                assert fr.score(prior[j], q, m64[j] - 1, sq, C_PUCT) >= S
    assert all(v > 0 for v in kinds.values()), kinds


def test_a_vanishing_k_leaves_everything(roots):
    for prior, W, n, _ in roots[::40]:
        assert (fr.prune(prior, W, n, 1e-30, C_PUCT) == n).all()
        assert (link.forced_prune(prior, W, n, 1e-30, C_PUCT) == n).all()
        assert (link.forced_prune(prior, W, n, 0.0, C_PUCT) == n).all()


def test_the_order_of_the_other_edges_does_not_matter(roots):
    rng = np.random.default_rng(5)
    checked = 0
    for prior, W, n, k in roots[::25]:
        if len(n) < 3:
            continue
        b = fr.best_edge(n)
        if int((n == n[b]).sum()) > 1:
            continue   # (several most-visited edges: which one is `b` depends on the order by definition)
        perm = rng.permutation(len(n))
        want = fr.prune(prior, W, n, k, C_PUCT)
        assert (fr.prune(prior[perm], W[perm], n[perm], k, C_PUCT) == want[perm]).all()
        checked += 1
    assert checked > 30


def test_owed_and_the_root_choice():
    # N = 100, k = 2: an edge of prior 0.08 is owed sqrt(16) = 4 visits, one of prior 0.5 sqrt(100) = 10
    prior = np.array([0.5, 0.08, 0.08, 0.34], dtype=np.float32)
    n = [96, 3, 0, 1]
    mask = fr.owed(prior, n, 100, 2.0)
    assert mask.tolist() == [False, True, False, True]      # 96 >= 10; 3 < 4; never visited: not owed; 1 < 8.2
    assert not fr.owed(prior, n, 100, 0.0).any()
    tree = (np.zeros((5, 2), np.uint64), np.array([[0, 4, 0, 0]] + [[0, 1 << 16, 0, vlr._bits(F32(1.0))]] * 4, np.uint32),
            np.array([[vlr._bits(p), v, vlr._bits(F32(0.5 * v)), c] for p, v, c in zip(prior, n, (1, 2, vlr.NONE, 4))], np.uint32),
            np.arange(4, dtype=np.uint16))
    last = fr.select(tree, 100, 2.0, True, 1.0, False, 0)
    first = fr.select(tree, 100, 2.0, True, 1.0, True, 0)
    fast = fr.select(tree, 100, 2.0, False, 1.0, False, 0)
    assert last.forced == 3 and last.paths[0] == [3] and first.forced == 1 and first.paths[0] == [1]
    assert fast.forced is None and not fast.owed.any() and fast.paths[0] == [fast.puct]
    assert last.kind == [vlr.LEAF_TERMINAL] and last.puct == fast.puct
