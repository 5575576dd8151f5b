"""The per-ply temperature (azh_engine_set_temperature), the parts that need no device: the host restatement of the device's
choice (azh_temperature_pick) against tests/temperature_reference.py, weights included; its distribution; the schedule
(selfplay.temperature_table) and the validation of the generator's flags."""
import numpy as np
import pytest

from ataxxzero_amd import link, selfplay
from tests import temperature_reference as ref

SEED = 0x0F1E2D3C_4B5A6978
MS = (1, 2, 63, 64, 65, 128, 129, 256)
TS = (0.0, 1.0 / 64.0, 0.1, 0.5, 0.8, 1.0, 1.25, 4.0, 64.0)


def count_vectors(M, rng):
    """name -> (M,) visit counts: interleaved zeros, ties for the maximum, one edge with every visit, all ones, counts up to
    65535 (with the largest possible one present)"""
    zeros = rng.integers(1, 400, size=M)
    zeros[::2] = 0
    if M == 1:
        zeros[0] = 7
    ties = rng.integers(0, 50, size=M)
    ties[rng.integers(0, M, size=min(M, 3))] = 50
    single = np.zeros(M, dtype=np.int64)
    single[M // 2] = 400
    big = rng.integers(0, 65536, size=M)
    big[M - 1] = 65535
    return {"zeros": zeros, "ties": ties, "single": single, "ones": np.ones(M, dtype=np.int64), "big": big}


def test_pick_and_weights_equal_the_reference():
    rng = np.random.default_rng(5)
    checked = 0
    for M in MS:
        for name, n in count_vectors(M, rng).items():
            for T in TS:
                want_q = ref.weights(n, T)
                for uid, ply in ((0, 0), (3, 17), (4095, 399), (2 ** 32 - 1, 1)):
                    j, q = link.temperature_pick(n, T, SEED, uid, ply, weights=True)
                    assert [int(v) for v in q] == want_q, (M, name, T)
                    assert j == ref.pick_from(want_q, ref.v0_of(SEED, uid, ply)), (M, name, T, uid, ply)
                    assert j == link.temperature_pick(n, T, SEED, uid, ply)
                    assert n[j] > 0  # an edge without a visit is never played
                    checked += 1
                if T not in (0.0, 1.0):
                    assert max(want_q) == 1 << 20 and all(want_q[k] == 1 << 20 for k in range(M) if n[k] == n.max())
    assert checked == len(MS) * 5 * len(TS) * 4


def test_temperature_one_is_the_proportional_draw_and_zero_the_first_maximum():
    rng = np.random.default_rng(6)
    for M in MS:
        for name, n in count_vectors(M, rng).items():
            first_max = int(np.argmax(n))
            cum = np.cumsum(n)
            for uid in range(12):
                v0 = ref.v0_of(SEED, uid, 2 * uid)
                r = (v0 * int(n.sum())) >> 32
                assert link.temperature_pick(n, 1.0, SEED, uid, 2 * uid) == int(np.nonzero(cum > r)[0][0])
                assert link.temperature_pick(n, 0.0, SEED, uid, 2 * uid) == first_max


def test_a_root_without_a_visit_yields_edge_zero():
    for T in TS:
        j, q = link.temperature_pick(np.zeros(9, dtype=np.uint32), T, SEED, 1, 2, weights=True)
        assert j == 0 and (int(q.sum()) == 0 or T == 0.0)


def test_pick_refuses_bad_arguments():
    n = np.array([3, 4], dtype=np.uint32)
    for T in (float("nan"), -1.0, 0.001, 65.0, float("inf")):
        with pytest.raises(link.AzhError):
            link.temperature_pick(n, T, SEED, 0, 0)
    with pytest.raises(link.AzhError):
        link.temperature_pick(np.zeros(0, dtype=np.uint32), 1.0, SEED, 0, 0)
    with pytest.raises(link.AzhError):
        link.temperature_pick(np.ones(257, dtype=np.uint32), 1.0, SEED, 0, 0)


DIST_VECTORS = (
    np.array([10, 5, 1, 0, 20, 7]),
    np.array([340, 30, 20, 10]),
    np.concatenate([np.arange(1, 34), np.arange(32, 0, -1)]),   # 65 edges: more than one 64-edge round
)
PAIRS = 200000


def test_distribution_of_the_pick():
    """Over 200,000 (uid, ply) pairs at a fixed seed each edge's frequency lies within five standard deviations plus the
    quantisation step plus the f32 error of det_logf / det_expf of n^(1/T) / sum (float64).  The reference alone is held to
    the same bound, on the same pairs."""
    uids, plies = np.divmod(np.arange(PAIRS), 100)
    v0 = np.array([ref.v0_of(SEED, int(u), int(p)) for u, p in zip(uids, plies)], dtype=np.uint64)
    pick = link.load().azh_temperature_pick
    for n in DIST_VECTORS:
        M = len(n)
        cn = np.ascontiguousarray(n, dtype=np.uint32)
        ptr = link._ptr(cn)
        for T in (0.5, 2.0):
            p = n.astype(np.float64) ** (1.0 / T)
            p[n == 0] = 0.0
            p /= p.sum()
            bound = 5.0 * np.sqrt(p * (1.0 - p) / PAIRS) + M * 2.0 ** -20 + 1e-5
            q = np.array(ref.weights(n, T), dtype=np.uint64)
            r = (v0 * q.sum()) >> np.uint64(32)
            ref_picks = np.searchsorted(np.cumsum(q), r, side="right")
            ref_freq = np.bincount(ref_picks, minlength=M) / PAIRS
            assert (np.abs(ref_freq - p) <= bound).all(), (n, T, "the reference")
            got = np.fromiter((pick(ptr, M, T, SEED, int(u), int(pl), None) for u, pl in zip(uids, plies)), dtype=np.int64,
                              count=PAIRS)
            freq = np.bincount(got, minlength=M) / PAIRS
            assert (np.abs(freq - p) <= bound).all(), (n, T, np.abs(freq - p).max())
            assert (got == ref_picks).all()


def test_table():
    t = selfplay.temperature_table(400, 0.8, 0.2, 19, None)
    assert t.dtype == np.float32 and t.shape == (400,)
    assert t[0] == np.float32(0.8) and t[19] == np.float32(0.5) and abs(float(t[399]) - 0.2) < 1e-6
    assert (np.diff(t) <= 0).all() and (t >= np.float32(0.2)).all()
    assert (t == ref.table(400, 0.8, 0.2, 19, None)).all()
    up = selfplay.temperature_table(50, 1.1, 1.25, 19, None)   # a rising schedule is monotone too
    assert (np.diff(up) >= 0).all() and up[0] == np.float32(1.1)
    # AlphaZero's: ones for 30 plies, then the most visited move
    az = selfplay.temperature_table(400, 1.0, 0.0, 0, 30)
    assert (az[:30] == 1).all() and (az[30:] == 0).all()
    # a decay towards 0 snaps to 0 below 1/64 and nowhere else
    d = selfplay.temperature_table(400, 1.0, 0.0, 4, None)
    assert d[0] == 1 and d[4] == np.float32(0.5) and d[20] == np.float32(2.0 ** -5) and d[24] == np.float32(2.0 ** -6)
    assert (d[25:] == 0).all() and (d[:25] >= np.float32(1.0 / 64.0)).all()
    assert (d == ref.table(400, 1.0, 0.0, 4, None)).all()
    # cutoff with a decay, a constant table, the default final
    c = selfplay.temperature_table(60, 0.8, 0.2, 19, 40)
    assert (c[40:] == np.float32(0.2)).all() and (c[:40] == t[:40]).all()
    assert (c == ref.table(60, 0.8, 0.2, 19, 40)).all()
    assert (selfplay.temperature_table(7, 0.7) == np.float32(0.7)).all()
    assert (selfplay.temperature_table(7, 0.7, None, 3.0, None) == np.float32(0.7)).all()


def test_generator_flags_are_validated():
    tables = selfplay.temperature_tables
    assert tables(400) == (None, None)
    move, root = tables(400, 1.0, 0.0, 0.0, 30)
    assert root is None and (move == ref.table(400, 1.0, 0.0, 0, 30)).all()
    move, root = tables(400, 0.8, 0.2, 19.0, None, 1.25, 1.1)
    assert (move == ref.table(400, 0.8, 0.2, 19, None)).all() and (root == ref.table(400, 1.25, 1.1, 19, None)).all()
    move, root = tables(400, None, None, 19.0, None, 1.25)       # the policy alone: R1 defaults to 1, the half-life is shared
    assert move is None and root[0] == np.float32(1.25) and root[19] == np.float32(1.125)
    move, root = tables(400, 0.5, None, 0.0, 10, 1.25, 1.1)       # the cutoff is the move's alone
    assert (move == np.float32(0.5)).all() and (root == np.float32(1.25)).all()
    bad = [
        dict(temperature=-0.5), dict(temperature=float("nan")), dict(temperature=0.001), dict(temperature=65.0),
        dict(temperature=1.0, temperature_final=0.01), dict(temperature=1.0, temperature_final=-1.0),
        dict(temperature_final=0.5), dict(cutoff=30), dict(halflife=19.0),
        dict(temperature=1.0, halflife=-1.0), dict(temperature=1.0, cutoff=-1), dict(temperature=1.0, halflife=float("nan")),
        dict(root_policy_temperature=0.0), dict(root_policy_temperature=0.2), dict(root_policy_temperature=65.0),
        dict(root_policy_temperature=float("nan")), dict(root_policy_temperature=1.25, root_policy_temperature_final=0.1),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            tables(400, **kw)
