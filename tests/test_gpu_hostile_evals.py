"""Every root mode under evaluations that are not finite, on the MI355X: forced playouts with target pruning, the playout cap,
the random symmetry per evaluation, both temperature tables, the Gumbel root search and the leaf-parallel search, each fed by
helpers.HostileEvaluator — NaN rows of both signs, +inf and -inf logits, one logit 1e30 above the rest, equal logits, NaN and
infinite values placed so that the most visited root edge's W, or every visited edge's, is a NaN when the ply ends, values of
exactly +-1 — with one slot in lock step with the mode's numpy restatement iteration by iteration: the whole tree, the priors
of every evaluated node (tests/priors_reference.py), the root visits, and every ply's record and move.  Then the device loop
on a net whose evaluations are not finite for some positions (helpers.nonfinite_net) against host stepping.

A NaN is compared as a NaN whatever its sign and payload (which NaN an operation hands on is the hardware's choice, as in
tests/engine_harness.compare_all); every other word bit for bit."""
import json
import random

import numpy as np
import pytest

from ataxxzero_amd import link, training
from tests import engine_harness as eh
from tests import forced_reference as fr
from tests import gumbel_reference as gr
from tests import helpers
from tests import priors_reference as pr
from tests import symmetry_reference as sym
from tests import temperature_reference as tr
from tests import vl_reference as vlr
from tests.engine_harness import ALPHA, C_PUCT, SEED

pytestmark = pytest.mark.gpu

C_VISIT, C_SCALE = 50.0, 1.0
MAX_PLIES = 400
F32 = np.float32
MOVE_T = (0.0, 1.0 / 64.0, 0.37, 1.0, 64.0)
ROOT_R = (0.25, 1.0, 64.0)
PERIOD = 9      # the schedule repeats every 9 plies


class Mode:
    """One root mode: how its engine is made and what the restatement of its select and of its ply's record is."""

    def __init__(self, name, games, visits, weight=0.25, gumbel=0, forced=0.0, cap=None, symmetry=False, K=1, move_table=None,
                 root_table=None):
        self.name, self.games, self.visits, self.weight, self.gumbel, self.forced = name, games, visits, weight, gumbel, forced
        self.cap, self.symmetry, self.K, self.move_table, self.root_table = cap, symmetry, K, move_table, root_table

    def engine(self, games=None, visits=None, max_plies=MAX_PLIES, flags=0):
        tables = None
        if self.move_table is not None or self.root_table is not None:
            tables = (None if self.move_table is None else self.move_table[:max_plies],
                      None if self.root_table is None else self.root_table[:max_plies])
        return eh.root_engine(games or self.games, visits or self.visits, weight=self.weight, flags=link.FLAG_NO_REUSE | flags,
                              max_plies=max_plies, cap=self.cap or None, forced=self.forced or None, temperature=tables,
                              symmetry=self.symmetry, K=self.K, gumbel=(self.gumbel, C_VISIT, C_SCALE) if self.gumbel else None)

    def full(self, uid, ply):
        return True if self.cap is None else bool(link.playout_cap_kind(SEED, uid, ply, self.cap[1]))

    def threshold(self, uid, ply, visits=None):
        return (visits or self.visits) if self.full(uid, ply) else self.cap[0]

    def select(self, pre, st, root):
        if self.gumbel:
            return gr.select(pre, st.root_visits, self.visits, self.gumbel, root[0], C_VISIT, C_SCALE, C_PUCT, False, 0)
        if self.forced:
            return fr.select(pre, st.root_visits, self.forced, self.full(st.uid, st.ply), C_PUCT, False, 0)
        b = vlr.select(pre, st.root_visits, self.threshold(st.uid, st.ply), self.K, 1, C_PUCT, False, 0)
        assert not b.over
        return b


def _table(values):
    return np.array([values[p % len(values)] for p in range(MAX_PLIES)], dtype=np.float32)


MODES = {
    "gumbel4": Mode("gumbel4", 1, 16, weight=0.0, gumbel=4),
    "gumbel16": Mode("gumbel16", 2, 33, weight=0.0, gumbel=16),
    "forced": Mode("forced", 2, 33, forced=2.0),
    "temperature": Mode("temperature", 2, 20, move_table=_table(MOVE_T), root_table=_table(ROOT_R)),
    "cap_forced": Mode("cap_forced", 2, 24, forced=2.0, cap=(6, 32768)),
    "symmetry": Mode("symmetry", 2, 16, symmetry=True),
    "leaf_parallel": Mode("leaf_parallel", 2, 24, K=4),
}


def _schedule(key):
    """(uid, ply, phase, root visits (plus the path's index in a batch), tops) -> the injections.  tops: the path's root edge
    will have the most visits of the root after this visit (None: not known).  The NaN's sign goes by uid + ply, inverted on
    the last ply of a period: a game of nine plies meets a NaN row of either sign (plies 0 and 8) and NaN values of either sign
    (plies 4 and 5), whatever its uid."""
    uid, ply, phase, rv, tops = key
    p = ply % PERIOD
    neg = ((uid + ply) % 2 == 1) != (p == 8)
    out = []
    if phase == 0:
        name = {0: "row_nan", 1: "row_inf3", 2: "row_neginf", 3: "row_spike", 4: "row_equal", 5: "value_nan", 8: "row_nan"}.get(p)
        if name:
            out.append((name, neg))
    else:
        if p == 1:
            out.append(("value_plus1" if rv % 2 else "value_minus1", False))
        if p in (4, 8) and tops:
            out.append(("value_nan", neg))            # the most visited root edge's W is a NaN when the ply ends
        if p == 5:
            out.append(("value_nan", neg))            # ... every visited edge's
        if p == 6:
            out.append((("value_pinf", "value_ninf", "value_nan")[rv % 3], neg))
        if p == 7:
            out.append((("row_part_nan", "row_inf3", "row_neginf")[rv % 3], neg))
    return out


def _is_nan_bits(w):
    return (w & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def _canon(edges):
    e = np.array(edges, dtype=np.uint32, copy=True)
    e[_is_nan_bits(e[:, 2]), 2] = 0x7FC00000
    return e


def _same_tree(want, got, what):
    for name, a, b in zip(("boards", "info", "edges", "moves"), want, got):
        assert a.shape == b.shape, (what, name)
        if name == "edges":
            a, b = _canon(a), _canon(b)
        assert (a == b).all(), (what, name)


def _node_edges(tree, node):
    first, M = int(tree[1][node][0]), int(tree[1][node][1]) & 0xFFFF
    return tree[2][first:first + M], tree[3][first:first + M]


def _root_n(tree):
    return fr.root_arrays(tree)[2].astype(np.int64)


def _symmetry(mode, uid, board):
    return sym.eval_symmetry(SEED, uid, board[0], board[1]) if mode.symmetry else 0


def _expected_ply(mode, tree, st, root, seen, counted):
    """(move u16, {move: count}, full) of the ply played from `tree`: the host's functions and the restatement agree"""
    prior, W, n, moves, child = fr.root_arrays(tree)
    full = mode.full(st.uid, st.ply)
    with np.errstate(all="ignore"):
        if mode.gumbel:
            _, g, v0 = root
            j, counts = link.gumbel_root(prior, W, n, v0, g, C_VISIT, C_SCALE)
            rj, rcounts = gr.root(prior, W, n, v0, g, C_VISIT, C_SCALE)
            assert j == rj and (counts == rcounts).all(), (st.uid, st.ply)
            assert counts.max() == 65535
            written = {int(mv): int(c) for mv, c in zip(moves, counts) if c != 0}
            if counted:
                # (a root with every prior zero, or every visited W a NaN, has no finite greatest logit by construction)
                alone = len(written) == 1 and len(prior) > 1 and written == {int(moves[j]): 65535}
                seen["target_is_the_move_alone"] += int(alone and not prior.any())
                seen["nan_W_target_is_the_move_alone"] += int(alone and prior.any() and np.isnan(W[n > 0]).all())
                seen["edge0_by_default"] += int(n.max() > 0 and np.isnan(W[n == n.max()]).all() and j == 0)
                seen["v0_nan"] += int(np.isnan(v0))
        else:
            T = float(mode.move_table[st.ply]) if mode.move_table is not None else 1.0
            j, _ = tr.pick(n, T, SEED, st.uid, st.ply)
            assert j == link.temperature_pick(n, T, SEED, st.uid, st.ply)
            if T == 1.0:
                assert j == vlr.forced_move(tree, st.root_visits, SEED, st.uid, st.ply)[0]
            if mode.forced and full:
                m = fr.prune(prior, W, n, mode.forced, C_PUCT)
                assert (m == link.forced_prune(prior, W, n, mode.forced, C_PUCT)).all()
                written = {int(mv): int(c) for mv, c, ch in zip(moves, m, child) if ch != vlr.NONE and c != 0}
                seen["pruned_plies"] += int((m != n).any())      # (any slot's: the pruning does act in this run)
                if counted:
                    b = fr.best_edge(n)
                    seen["S_nan_prunes_nothing"] += int(np.isnan(W[b]) and (m == n).all() and (n > 0).sum() > 1)
            else:
                written = {int(mv): int(c) for mv, c, ch in zip(moves, n, child) if ch != vlr.NONE}
            if counted:
                seen["T=%g" % T] = seen.get("T=%g" % T, 0) + 1
    if counted:
        b = int(np.argmax(n))
        vis = n > 0
        seen["best_edge_W_nan"] += int(np.isnan(W[b]))
        seen["every_visited_W_nan"] += int(vis.any() and np.isnan(W[vis]).all())
        seen["all_priors_zero"] += int(not prior.any())
        seen["one_prior_only"] += int((prior > 0).sum() == 1 and len(prior) > 1)
        seen["equal_priors"] += int(len(prior) > 1 and (prior == prior[0]).all() and prior[0] > 0)
        seen["full" if full else "fast"] += 1
    return int(moves[j]), written, int(full)


def _check_lines(lines):
    entries = []
    for line in lines:
        line = line.decode() if isinstance(line, bytes) else line
        assert "null" not in line and "NaN" not in line and "nan" not in line, line[:200]
        entry = json.loads(line)
        assert len(entry["boards"]) == len(entry["moves"]) == len(entry["dists"]) > 0
        for d, mv in zip(entry["dists"], entry["moves"]):
            if mv != "pass":
                assert len(d) > 0 and abs(sum(d.values()) - 1.0) < 1e-6, (mv, d)
                assert all(v > 0 for v in d.values())
        entries.append(entry)
    random.seed(7)
    feats, pols, vals = training.make_minibatch(entries, 200)
    assert feats.shape[0] == pols.shape[0] == 200 and np.isfinite(pols).all() and np.isfinite(vals).all()
    assert np.allclose(pols.reshape(200, -1).sum(axis=1), 1.0, atol=1e-5)


def _lock_step(mode, games_wanted=2, plies_checked=12, max_iterations=20000):
    """Slot 0 against the restatement, iteration by iteration, over the first `plies_checked` plies of `games_wanted` complete
    games; every slot's every ply's record against the expected one -> (counters, the evaluator's counters, lines)."""
    e = mode.engine()
    G, K = e.G, mode.K
    hostile = helpers.HostileEvaluator(_schedule)
    seen = {k: 0 for k in ("target_is_the_move_alone", "nan_W_target_is_the_move_alone", "edge0_by_default", "v0_nan",
                           "S_nan_prunes_nothing", "pruned_plies",
                           "best_edge_W_nan", "every_visited_W_nan", "W_inf", "all_priors_zero", "one_prior_only",
                           "equal_priors", "full", "fast", "iterations", "forced_on_nan_W", "gumbel_level_puct",
                           "gumbel_differs", "zero_prior_nodes", "partly_nan_rows", "nodes", "roots", "noise_roots",
                           "tempered_roots", "symmetries", "collisions", "records", "plies")}
    symmetries = set()
    expected, roots, lines, done0 = {}, {}, [], 0
    for it in range(max_iterations):
        st = [e.game_state(g) for g in range(G)]
        s0 = st[0]
        checked = s0.ply < plies_checked
        b = pre = None
        if s0.phase == 1 and checked:
            pre = e.tree(0)
            with np.errstate(all="ignore"):
                b = mode.select(pre, s0, roots.get(0))
        root_board = vlr.leaf_board(*(int(v) for v in e.tree(0)[0][0])) if s0.phase == 0 else None
        # the keys of the rows: what is known of each slot before the step
        keys = [None] * (G * K)
        for g in range(G):
            if st[g].phase == 0:
                keys[g * K] = (st[g].uid, st[g].ply, 0, 0, None)
            elif st[g].phase == 1:
                n0 = _root_n(pre) if (g == 0 and b is not None) else None
                first0 = int(pre[1][0][0]) if n0 is not None else 0
                for p in range(K):
                    tops = None
                    if n0 is not None and p < len(b.paths) and b.paths[p]:
                        j = b.paths[p][0] - first0
                        tops = bool(n0[j] + 1 >= n0.max())
                    keys[g * K + p] = (st[g].uid, st[g].ply, 1, st[g].root_visits + p, tops)
        e.select()
        if K == 1:
            need, lb = e.leaves()
            needed = need != 0
        else:
            kind, lb, le = e.batch_leaves()
            lb = lb.reshape(-1, 2)
            needed = ((kind == link.LEAF_EVAL) | (kind == link.LEAF_ROOT)).reshape(-1)
        counted = [bool(needed[i]) and i < K and checked for i in range(G * K)]
        logits, values = hostile(lb, keys, counted)
        if K == 1:
            e.set_evals(logits, values)
        else:
            e.set_batch_evals(logits, values)
        e.backup()
        s2 = [e.game_state(g) for g in range(G)]
        post = e.tree(0)
        seen["iterations"] += 1
        with np.errstate(all="ignore"):
            if b is not None:
                assert (s2[0].uid, s2[0].ply) == (s0.uid, s0.ply)
                k = len(b.kind)
                if K > 1:
                    assert list(kind[0, :k]) == b.kind and (kind[0, k:] == 0).all(), it
                    assert list(le[0, :k]) == b.leaf_edge, it
                    seen["collisions"] += b.kind.count(vlr.LEAF_COLLISION)
                want, added = vlr.expected_tree(b, values[:K], post)
                _same_tree(want, post, (mode.name, it))
                assert s2[0].root_visits == s0.root_visits + added, it
                for p in range(k):
                    if b.kind[p] != vlr.LEAF_EVAL:
                        continue
                    # the evaluated node: the evaluator saw its board's image, and its priors are the row's
                    s = _symmetry(mode, s0.uid, b.leaf_board[p])
                    image = tuple(sym.board(s, w) for w in b.leaf_board[p]) if s else tuple(b.leaf_board[p])
                    assert tuple(int(v) for v in lb[p]) == image, (it, p, s)
                    ed, mv = _node_edges(post, b.leaf_node[p])
                    wantp = pr.priors(logits[p], mv, 0, s)
                    assert (ed[:, 0] == wantp).all(), (it, p, s)
                    symmetries.add(s)
                    seen["nodes"] += 1
                    seen["zero_prior_nodes"] += int(not wantp.any())
                    row = sym.logits_of_the_position(logits[p], s)[0]
                    at = row[[sym.policy_index(int(m)) for m in mv]]
                    seen["partly_nan_rows"] += int(np.isnan(at).any() and not np.isnan(at).all() and wantp.any())
                seen["W_inf"] += int(np.isinf(fr.root_arrays(post)[1]).any())
                if mode.gumbel:
                    seen["gumbel_level_puct"] += int(b.gumbel is None)
                    seen["gumbel_differs"] += int(b.gumbel is not None and b.gumbel != b.puct)
                if mode.forced and b.forced is not None:
                    first0 = int(pre[1][0][0])
                    seen["forced_on_nan_W"] += int(np.isnan(vlr._f(int(pre[2][first0 + b.forced][2]))))
            if s0.phase == 0 and (s2[0].uid, s2[0].ply, s2[0].phase) == (s0.uid, s0.ply, 1) and checked:
                # the root was evaluated: its priors, with the ply's noise and root temperature where it gets them
                s = _symmetry(mode, s0.uid, root_board)
                image = tuple(sym.board(s, w) for w in root_board) if s else tuple(root_board)
                assert tuple(int(v) for v in lb[0]) == image
                ed, mv = _node_edges(post, 0)
                full = mode.full(s0.uid, s0.ply)
                noise = (ALPHA, mode.weight, SEED, s0.uid, s0.ply) if full else None
                R = float(mode.root_table[s0.ply]) if (mode.root_table is not None and full) else 1.0
                wantp = tr.tempered_priors(logits[0], mv, R, symmetry=s, noise=noise)
                assert (ed[:, 0] == wantp).all(), (it, s, R)
                seen["roots"] += 1
                seen["noise_roots"] += int(full and mode.weight > 0)
                seen["tempered_roots"] += int(R != 1.0)
                symmetries.add(s)
            for g in range(G):
                if mode.gumbel and st[g].phase == 0 and s2[g].phase == 1:
                    prior = fr.root_arrays(post if g == 0 else e.tree(g))[0]
                    gn = link.gumbel_noise(SEED, st[g].uid, st[g].ply, len(prior))
                    roots[g] = (gr.a_values(prior, gn), gn, F32(F32(values[g * K] + F32(1.0)) * F32(0.5)))
                if s2[g].phase == 2 and st[g].phase != 2:
                    # the move of this ply is due: the next iteration plays it from this tree
                    assert s2[g].root_visits >= mode.threshold(s2[g].uid, s2[g].ply)
                    expected[(s2[g].uid, s2[g].ply)] = _expected_ply(mode, post if g == 0 else e.tree(g), s2[g], roots.get(g),
                                                                     seen, g == 0 and s2[g].ply < plies_checked)
        if any(a.uid != c.uid for a, c in zip(st, s2)):
            e.fetch()
            for slot, uid, result, kind, rows in eh.records3(e.staged_records()):
                assert bool(kind & link.REC_KIND_GUMBEL) == bool(mode.gumbel) and \
                    bool(kind & link.REC_KIND_FORCED) == bool(mode.forced) and \
                    bool(kind & link.REC_KIND_PLAYOUT_CAP) == (mode.cap is not None), hex(kind)
                for ply, (move, w5, counts) in enumerate(rows):
                    wmove, wcounts, wfull = expected[(uid, ply)]
                    assert (move, counts) == (wmove, wcounts), (uid, ply, move, wmove, counts, wcounts)
                    assert len(counts) > 0 and all(0 < c <= 65535 for c in counts.values())
                    assert mode.cap is None or w5 == wfull
                    seen["plies"] += 1
                seen["records"] += 1
                done0 += int(slot == 0)
            lines += e.drain_json()
            if done0 >= games_wanted:
                break
    assert done0 >= games_wanted, (done0, json.dumps(seen, sort_keys=True))
    seen["symmetries"] = len(symmetries)
    e.close()
    print("\n%s counters: %s\n%s injections: %s" % (mode.name, json.dumps(seen, sort_keys=True), mode.name,
                                                  sorted((k[0], "neg" if k[1] else "pos", v) for k, v in hostile.seen.items())))
    _check_lines(lines)
    assert len(lines) == seen["records"]
    return seen, hostile.seen


def _assert_injections(inj, roots=True):
    """every phenomenon of the schedule was met at a checked ply, the NaNs with both signs"""
    names = ["value_plus1", "value_minus1", "value_pinf", "value_ninf", "row_part_nan"]
    if roots:
        names += ["row_inf3", "row_neginf", "row_spike", "row_equal"]
    for name in names:
        assert inj.get((name, False), 0) + inj.get((name, True), 0) > 0, (name, inj)
    for name in ("row_nan", "value_nan"):
        assert inj.get((name, False), 0) > 0 and inj.get((name, True), 0) > 0, (name, inj)


def _assert_common(seen):
    assert seen["best_edge_W_nan"] > 0 and seen["every_visited_W_nan"] > 0 and seen["W_inf"] > 0, seen
    assert seen["zero_prior_nodes"] > 0 and seen["partly_nan_rows"] > 0 and seen["nodes"] > 100 and seen["roots"] >= 12, seen
    assert seen["plies"] >= 18 and seen["records"] >= 2, seen


@pytest.mark.parametrize("name", ["gumbel4", "gumbel16"])
def test_gumbel(name):
    seen, inj = _lock_step(MODES[name])
    _assert_injections(inj)
    _assert_common(seen)
    # no noise is mixed in: a NaN, +inf or -inf row leaves every root prior zero, the spike one prior only
    assert seen["all_priors_zero"] >= 3 and seen["one_prior_only"] > 0 and seen["equal_priors"] > 0, seen
    # a candidate set whose scores are all NaN fell to the PUCT level, a root whose most visited edges' scores are to edge 0,
    # and the roots without a finite greatest logit recorded the move played alone
    assert seen["gumbel_level_puct"] > 0 and seen["edge0_by_default"] > 0 and seen["target_is_the_move_alone"] >= 3, seen
    assert seen["gumbel_differs"] > 0 and seen["v0_nan"] > 0 and seen["nan_W_target_is_the_move_alone"] > 0, seen


def test_forced_playouts_with_pruning():
    seen, inj = _lock_step(MODES["forced"])
    _assert_injections(inj)
    _assert_common(seen)
    assert seen["noise_roots"] == seen["roots"] and seen["forced_on_nan_W"] > 0, seen
    assert seen["S_nan_prunes_nothing"] > 0 and seen["pruned_plies"] > 0, seen


def test_both_temperature_tables():
    seen, inj = _lock_step(MODES["temperature"])
    _assert_injections(inj)
    _assert_common(seen)
    assert all(seen.get("T=%g" % T, 0) > 0 for T in MOVE_T), seen
    assert seen["tempered_roots"] > 0 and seen["tempered_roots"] < seen["roots"], seen


def test_the_playout_cap_with_forced_playouts_on():
    seen, inj = _lock_step(MODES["cap_forced"], games_wanted=3)
    _assert_injections(inj)
    assert seen["fast"] > 0 and seen["full"] > 0 and 0 < seen["noise_roots"] < seen["roots"], seen
    assert seen["best_edge_W_nan"] > 0 and seen["every_visited_W_nan"] > 0 and seen["zero_prior_nodes"] > 0, seen
    assert seen["all_priors_zero"] > 0, seen       # a FAST ply's root gets no noise: a NaN row leaves it without a prior
    assert seen["plies"] >= 18 and seen["records"] >= 2, seen


def test_the_random_symmetry():
    seen, inj = _lock_step(MODES["symmetry"])
    _assert_injections(inj)
    _assert_common(seen)
    assert seen["symmetries"] == 8, seen


def test_the_leaf_parallel_search():
    seen, inj = _lock_step(MODES["leaf_parallel"])
    _assert_injections(inj)
    _assert_common(seen)


# ------------------------------------------------------------------ the device loop

_NET = []


def _net():
    if not _NET:
        _NET.append(link.Net(*helpers.nonfinite_net()))
    return _NET[0]


@pytest.mark.parametrize("games", [5, 33])
@pytest.mark.parametrize("name", ["gumbel4", "gumbel16", "forced", "temperature", "cap_forced", "symmetry", "leaf_parallel"])
def test_device_loop_equals_host_stepping(name, games):
    """run(net, 500) against 500 host-stepped iterations of a twin engine on the net whose evaluations are not finite for some
    positions: the move-playing launch obeys the rules of the step-wise path.  Compared six times on the way, at uneven
    distances (every ply of an engine without tree reuse takes the same number of iterations: after 500 the modes with one
    threshold stand at fresh roots, and even distances would show one stage of a ply only), the last time after all 500.
    Games end at 40 plies at the latest and are kept (on this
    net the Gumbel search's games do not end by themselves within 250 plies), so every slot has written a record by then: the
    records and lines of the two engines are compared on games, never on none."""
    mode, net = MODES[name], _net()
    a, b = (mode.engine(games, 8, max_plies=40, flags=link.FLAG_KEEP_UNFINISHED) for _ in range(2))
    nan_w = finite_w = zero_nodes = prior_nodes = 0
    la, lb, ra, rb = [], [], [], []
    for n in (95, 101, 99, 103, 97, 5):
        a.run(net, n, link.DTYPE_BF16)
        a.sync()
        for _ in range(n):
            b.select()
            b.eval(net, link.DTYPE_BF16)
            b.backup()
        (sa, ta), (sb, tb) = eh.dump(a), eh.dump(b)
        assert sa == sb
        for g, (x, y) in enumerate(zip(ta, tb)):
            _same_tree(x, y, (name, g, n))
            w = x[2][x[2][:, 1] > 0, 2]
            nan_w += int(_is_nan_bits(w).sum())
            finite_w += int((~_is_nan_bits(w)).sum())
            for node in range(len(x[1])):
                ed, _ = _node_edges(x, node)
                if len(ed) and (int(x[1][node][1]) >> 16) == 0:
                    zero_nodes += int(not ed[:, 0].any())
                    prior_nodes += int(bool(ed[:, 0].any()))
        assert a.stats() == b.stats()
        a.fetch(), b.fetch()
        ra, rb = ra + eh.records3(a.staged_records()), rb + eh.records3(b.staged_records())
        la, lb = la + a.drain_json(), lb + b.drain_json()
    assert a.stats()["plies"] > 2 * games
    print("\n%s %d games: W NaN %d, W finite %d, evaluated nodes without a prior %d, with priors %d"
          % (name, games, nan_w, finite_w, zero_nodes, prior_nodes))
    # finite and non-finite evaluations both reached the trees
    assert nan_w > 0 and finite_w > 0 and zero_nodes > 0 and prior_nodes > 0, (nan_w, finite_w, zero_nodes, prior_nodes)
    assert sorted(la) == sorted(lb) and len(ra) == len(rb) == len(la)
    assert sorted(map(repr, ra)) == sorted(map(repr, rb))
    assert len(la) >= games
    for slot, uid, result, kind, rows in ra:
        for move, w5, counts in rows:
            assert len(counts) > 0 and all(0 < c <= 65535 for c in counts.values())
    _check_lines(la)
    a.close(), b.close()
