"""The priors restatement (tests/priors_reference.py) on the CPU: bit for bit the C oracle's priors over one-leaf searches
(root noise, both flag sets, nodes of more than 64 moves), close to a float64 evaluation of the same definition, and the
formula's own values on degenerate rows."""
import numpy as np
import pytest

from oracle import oracle_lib as orc
from tests import helpers
from tests import priors_reference as pr
from tests import symmetry_reference as sym

UAI = orc.FLAG_NO_REUSE | orc.FLAG_TIE_FIRST | orc.FLAG_PY_POSTERIOR
SEED = 20261018
ALPHA, WEIGHT = 0.15, 0.25
# float64 bound: 4 x the largest error the restatement shows on the rows of _rows() (measured: see the test's docstring)
F64_BOUND = 4 * 2.74e-8


def _wide_root():
    """The first 129-move position of the `wide` family (no blockers) of the edge fixtures, packed (x | turn << 63, o)."""
    for rec in helpers.load_gz("rules_edge.json.gz")["positions"]:
        if rec["set"] == "none" and rec["family"] == "wide" and len(rec["moves"]) == 129:
            p = orc.pos_from_fen(rec["fen"])
            return np.array([[int(p.pieces[0]) | (p.turn << 63), int(p.pieces[1])]], dtype=np.uint64)
    raise AssertionError("no such fixture position")


_ROWS = {}


def _rows():
    """One-leaf searches of the C oracle -> [(flags, noise or None, logits row, the node's moves, the oracle's prior bits)],
    every evaluated node of every iteration.  Computed once."""
    if _ROWS:
        return _ROWS["rows"]
    rows = []
    for flags, weight, wide, visits, iters in [(0, WEIGHT, False, 12, 60), (0, WEIGHT, True, 12, 45),
                                               (UAI, 0.0, False, 12, 40), (UAI, 0.0, True, 12, 30)]:
        cfg = orc.make_config(games=1, visits=visits, seed=SEED, fen_str=orc.START_FEN_PLAIN, flags=flags, weight=weight,
                              alpha=ALPHA)
        oe = orc.Engine(cfg)
        if wide:
            oe.set_positions(_wide_root(), np.array([20], np.int32))
        for _ in range(iters):
            oe.select()
            st = oe.game_state(0)
            lb = oe.leaf_boards()
            logits, values = helpers.synthetic_evals_distinct(lb)
            oe.backup(logits, values)
            if st.leaf_kind not in (orc.LEAF_EVAL, orc.LEAF_ROOT):
                continue
            boards, info, edges, moves = oe.tree(0)
            first, M = int(info[st.leaf_node, 0]), int(info[st.leaf_node, 1]) & 0xFFFF
            noise = (ALPHA, weight, SEED, st.uid, st.ply) if st.leaf_kind == orc.LEAF_ROOT and weight > 0 else None
            rows.append((flags, noise, logits[0].copy(), moves[first:first + M].copy(), edges[first:first + M, 0].copy()))
        oe.close()
    _ROWS["rows"] = rows
    return rows


def test_bit_for_bit_the_c_oracle():
    rows = _rows()
    seen = {"noise": 0, "plain": 0, "uai": 0, "wide": 0, "wide_uai": 0}
    for flags, noise, row, moves, want in rows:
        got = pr.priors(row, moves, flags, 0, noise)
        assert got.dtype == np.uint32 and (got == want).all(), (flags, noise, len(moves))
        seen["noise"] += noise is not None
        seen["plain"] += flags == 0 and noise is None
        seen["uai"] += flags == UAI
        seen["wide"] += flags == 0 and len(moves) > 64
        seen["wide_uai"] += flags == UAI and len(moves) > 64
    assert seen["noise"] >= 3 and min(seen.values()) > 0 and len(rows) > 100, seen


def _float64(flags, noise, row, moves):
    row = np.asarray(row, dtype=np.float64)
    idx = [sym.policy_index(int(m)) for m in moves]
    if flags & pr.FLAG_PY_POSTERIOR:
        soft = np.exp(row - row.max())
        soft /= soft.sum()
        P = soft[idx] / (soft[idx].sum() + np.float64(np.float32(1e-6)))
    else:
        ex = np.exp(row[idx] - row[idx].max())
        P = ex / ex.sum()
    if noise is not None:
        alpha, w, seed, uid, ply = noise
        gm = np.array([orc.lib().orc_probe_gamma(float(np.float32(alpha)), seed, uid, ply, j) for j in range(len(idx))], np.float64)
        w = np.float64(np.float32(w))
        P = w * gm / gm.sum() + (np.float64(1.0) - w) * P
    return P


def test_close_to_a_float64_evaluation_of_the_definition():
    """Largest |restatement - float64| over the rows of _rows(), measured on the CPU: 2.74e-8 (about half an ulp of the
    largest priors, which lie between 0.25 and 0.5).  The bound is 4 x that, 1.1e-7, because the rows are a sample.  Without
    PY_POSTERIOR the float64 side is the plain softmax over the legal moves, whose sum is 1: the f32 priors' own sum (in
    float64) is within the same bound of 1 (measured: 1.08e-7).  With PY_POSTERIOR the definition divides by the legal
    mass + 1e-6, so the sum is 1 only up to 1e-6 / mass and is not checked."""
    worst = worst_sum = 0.0
    for flags, noise, row, moves, _ in _rows():
        got = pr.priors(row, moves, flags, 0, noise).view(np.float32).astype(np.float64)
        err = float(np.abs(got - _float64(flags, noise, row, moves)).max())
        worst = max(worst, err)
        if not flags & pr.FLAG_PY_POSTERIOR:
            worst_sum = max(worst_sum, abs(float(got.sum()) - 1.0))
    print("largest error %.3g, largest |sum - 1| %.3g" % (worst, worst_sum))
    assert worst <= F64_BOUND
    assert worst_sum <= F64_BOUND


def _f(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def test_degenerate_rows_give_the_formulas_values():
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    moves = orc.movegen(p)
    M = len(moves)
    idx = [sym.policy_index(int(m)) for m in moves]
    assert M == 16 and len(set(idx)) == M
    # all logits equal: exp(0) = 1 for every move, S = M exactly
    got = _f(pr.priors(np.full(833, 0.25, np.float32), moves))
    assert (got == np.float32(1.0) / np.float32(M)).all()
    # one logit 200 above the rest: exp(-200) is 0 in f32, so the one move has prior exactly 1 and the others exactly 0
    row = np.zeros(833, np.float32)
    row[idx[5]] = 200.0
    got = _f(pr.priors(row, moves))
    assert got[5] == 1.0 and (np.delete(got, 5) == 0.0).all()
    # -inf on every legal index: l - mx is NaN, exp gives 0, S = 0 and the priors are the zeros themselves (no 0 / 0)
    row = np.zeros(833, np.float32)
    row[idx] = -np.inf
    bits = pr.priors(row, moves)
    assert (bits == 0).all()
    # the same row with PY_POSTERIOR: the legal moves have mass 0 of a finite total; 0 / (0 + 1e-6) = 0
    assert (pr.priors(row, moves, pr.FLAG_PY_POSTERIOR) == 0).all()
    # NaN on one legal index: that move's prior is 0 (never the maximum of a PUCT comparison among positive priors), the
    # others share the softmax of the remaining logits
    row = np.linspace(-1.0, 1.0, 833).astype(np.float32)
    clean = _f(pr.priors(row, np.delete(moves, 3)))
    row[idx[3]] = np.nan
    got = _f(pr.priors(row, moves))
    assert got[3] == 0.0 and not np.isnan(got).any() and (np.delete(got, 3) > 0).all()
    assert np.abs(np.delete(got, 3) - clean).max() <= F64_BOUND
    # M == 1: the only move has prior 1 whatever its logit; with root noise w * (gm / gm) + (1 - w) * 1
    got = _f(pr.priors(np.linspace(-3.0, 3.0, 833).astype(np.float32), moves[:1]))
    assert got.shape == (1,) and got[0] == 1.0
    got = _f(pr.priors(np.zeros(833, np.float32), moves[:1], 0, 0, (ALPHA, WEIGHT, SEED, 0, 0)))
    assert got[0] == np.float32(np.float32(WEIGHT) * np.float32(1.0) + np.float32(np.float32(1.0) - np.float32(WEIGHT)))
    # M == 0 (a node without edges is never evaluated, but the formula has nothing to divide)
    assert len(pr.priors(np.zeros(833, np.float32), moves[:0])) == 0


def test_wave_sum_is_the_lane_order_not_the_index_order():
    t = np.float32(2.0 ** -24)
    # lanes 2 and 3 meet first (2^-23, which 1 can hold); one after the other each 2^-24 would be lost
    v = np.array([1.0, 0.0, t, t], dtype=np.float32)
    seq = np.float32(0.0)
    for x in v:
        seq = np.float32(seq + x)
    assert seq == np.float32(1.0) and pr.wave_sum(v) == np.float32(1.0 + 2.0 ** -23)
    # term 64 goes to lane 0 before any lane meets another: (1 + 2^-24) is lost there, though lane 1 holds another 2^-24
    v = np.zeros(65, dtype=np.float32)
    v[0], v[1], v[64] = 1.0, t, t
    assert pr.wave_sum(v) == np.float32(1.0)
    v[1], v[64] = 0.0, 0.0
    v[2], v[3] = t, t
    assert pr.wave_sum(v) == np.float32(1.0 + 2.0 ** -23)


@pytest.mark.parametrize("s", range(1, 8))
def test_a_row_of_the_image_gives_the_positions_priors(s):
    """The evaluator saw T_s(position): its row, read through the symmetry, gives the priors of the position's own row."""
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    moves = orc.movegen(p)
    own = np.linspace(-2.0, 2.0, 833).astype(np.float32)[np.random.RandomState(s).permutation(833)]
    image = np.zeros(833, np.float32)
    image[sym.PERMS[s]] = own                      # image[perm_s[i]] = own[i]
    for flags in (0, pr.FLAG_PY_POSTERIOR):
        assert (pr.priors(image, moves, flags, s) == pr.priors(own, moves, flags, 0)).all()
