"""The leaf-parallel search on the MI355X where tests/test_gpu_vl_search.py does not reach: the priors of a batch's new nodes
and of the root (bit for bit tests/priors_reference.py), nodes of 65 to 193 edges, full arenas (the arena-full rule of
tests/vl_reference.py), and the need mask and leaf compaction over many slots.  Every test runs the HIP engine in lock step
with the host's restatement, iteration by iteration."""
import numpy as np
import pytest

from ataxxzero_amd import link
from oracle import oracle_lib as orc
from tests import engine_harness as eh
from tests import helpers
from tests import priors_reference as pr
from tests import solver_reference as sor
from tests import symmetry_reference as sym
from tests import vl_reference as vlr
from tests.engine_harness import _edge_positions, _pack, _wide_roots

pytestmark = pytest.mark.gpu

UAI = link.FLAG_NO_REUSE | link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR
ALPHA, WEIGHT = 0.15, 0.25
SEEN = {"eval_slots": 0, "symmetries": set(), "root_noise": 0, "idx64": 0, "idx128": 0, "idx192": 0, "wide_proofs": 0,
        "over_first": 0, "over_inside": 0, "forced_moves": 0, "mask_offsets": set()}


def _engine(positions, K, VL, flags, visits, seed, edges_per_node=96, ply=10):
    G = len(positions)
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    cfg = link.Config(games=G, visits=visits, max_plies=400, edges_per_node=edges_per_node, c_puct=1.0, dirichlet_alpha=ALPHA,
                      dirichlet_weight=0.0 if flags else WEIGHT, start_turn=0, seed=seed, start_x=int(p.pieces[0]),
                      start_o=int(p.pieces[1]), blockers=0, flags=flags)
    e = link.Engine(cfg)
    e.set_positions(np.array(positions, dtype=np.uint64), np.full(G, ply, np.int32))
    e.set_leaf_batch(K, VL)
    return e, cfg


def _fixture_positions(G):
    """G unfinished blocker-free fixture positions, spread over the file (repeated in order when G exceeds them)."""
    ps = []
    for rec in helpers.load_gz("rules_noblock.json.gz"):
        p = orc.pos_from_fen(rec["fen"])
        if orc.result(p) == 0 and len(orc.movegen(p)) > 0:
            ps.append(_pack(rec["fen"]))
    step = max(1, len(ps) // G)
    return [ps[(i * step) % len(ps)] for i in range(G)]


def _same_tree(exp, post):
    for a, x in zip(exp, post):
        assert a.shape == x.shape and (a == x).all()


class LockStep:
    """One engine against the restatement.  step() runs one iteration (select, the synthetic evaluations, backup) and checks
    it: the batch (kinds, leaf edges, leaf boards, the number of paths), the whole tree after the backup, the priors of every
    evaluated node against tests/priors_reference.py, the state, the move a due game plays and the overflow counter."""

    def __init__(self, e, cfg, K, VL, solver=False, symmetry=False, caps=False):
        self.e, self.cfg, self.K, self.VL, self.solver, self.symmetry = e, cfg, K, VL, solver, symmetry
        self.caps = (e.node_cap, e.edge_cap) if caps else (None, None)
        self.G = e.G
        self.due = np.zeros(self.G, bool)      # the move became due at some backup
        self.overflows = 0
        self.proven = []                       # (edge count of the node, value)

    def _symmetry(self, uid, board):
        return sym.eval_symmetry(self.cfg.seed, uid, board[0], board[1]) if self.symmetry else 0

    def _image(self, s, board):
        return (sym.board(s, board[0]), sym.board(s, board[1])) if s else tuple(board)

    def step(self):
        e, cfg, K, G, flags = self.e, self.cfg, self.K, self.G, self.cfg.flags
        pre = [e.tree(g) for g in range(G)]
        st = [e.game_state(g) for g in range(G)]
        e.select()
        kind, lb, le = e.batch_leaves()
        batches, roots, syms = {}, {}, {}
        for g in range(G):
            if st[g].phase == 1:
                if self.solver:
                    b = sor.select(pre[g], st[g].root_visits, cfg.visits, K, self.VL, cfg.c_puct, bool(flags & 2), 0)
                    b.over = False
                else:
                    b = vlr.select(pre[g], st[g].root_visits, cfg.visits, K, self.VL, cfg.c_puct, bool(flags & 2), 0, *self.caps)
                k = len(b.kind)
                assert list(kind[g, :k]) == b.kind and (kind[g, k:] == 0).all(), (g, list(kind[g]), b.kind)
                assert list(le[g, :k]) == b.leaf_edge
                assert e.game_state(g).path_len == k          # the batch ended with its last path (a dropped one included)
                ss = [self._symmetry(st[g].uid, x) if kd == vlr.LEAF_EVAL else 0 for kd, x in zip(b.kind, b.leaf_board)]
                assert [tuple(int(v) for v in x) for x in lb[g, :k]] == [self._image(s, x) for s, x in zip(ss, b.leaf_board)]
                batches[g], syms[g] = b, ss
                SEEN["symmetries"] |= {s for s, kd in zip(ss, b.kind) if kd == vlr.LEAF_EVAL} if self.symmetry else set()
                SEEN["eval_slots"] = max(SEEN["eval_slots"], b.kind.count(vlr.LEAF_EVAL))
                if b.over:
                    SEEN["over_first" if k == 1 else "over_inside"] += 1
                    self.overflows += 1
                for path in b.paths:          # the index of every edge the descent selected, at its level
                    node = 0
                    for ed in path:
                        j = ed - b.info[node][0]
                        SEEN["idx64"] += j >= 64
                        SEEN["idx128"] += j >= 128
                        SEEN["idx192"] += j >= 192
                        node = b.child[ed]
            elif st[g].phase == 0:
                assert kind[g, 0] == vlr.LEAF_ROOT and (kind[g, 1:] == 0).all()
                board = vlr.leaf_board(*pre[g][0][0])
                s = self._symmetry(st[g].uid, board)
                assert tuple(int(v) for v in lb[g, 0]) == self._image(s, board)
                roots[g] = s
            else:
                assert (kind[g] == 0).all()
                if st[g].phase == 2:
                    self._check_played_move(g, pre[g], st[g])
        logits, values = helpers.synthetic_evals_distinct(lb.reshape(-1, 2))
        e.set_batch_evals(logits, values)
        e.backup()
        for g, b in batches.items():
            post = e.tree(g)
            if self.solver:
                exp, added, proven = sor.expected_tree(b, values[g * K:(g + 1) * K], post)
                self.proven += [(b.info[x][1] & 0xFFFF, v) for x, v, _, _ in proven]
            else:
                exp, added = vlr.expected_tree(b, values[g * K:(g + 1) * K], post)
            _same_tree(exp, post)             # (every prior but the new nodes' is the one of the dump before)
            for p, kd in enumerate(b.kind):
                if kd == vlr.LEAF_EVAL:
                    first, M = b.info[b.leaf_node[p]][0], b.info[b.leaf_node[p]][1] & 0xFFFF
                    assert first >= b.edges0
                    want = pr.priors(logits[g * K + p], post[3][first:first + M], flags, syms[g][p])
                    assert (post[2][first:first + M, 0] == want).all(), (g, p, M)
            after = e.game_state(g)
            assert after.root_visits == st[g].root_visits + added
            due = vlr.move_is_due(b, after.root_visits, cfg.visits)
            assert after.phase == (2 if due else 1)
            self.due[g] |= due
        for g, s in roots.items():
            post = e.tree(g)
            first, M = int(post[1][0, 0]), int(post[1][0, 1]) & 0xFFFF
            noise = (ALPHA, cfg.dirichlet_weight, cfg.seed, st[g].uid, st[g].ply)
            want = pr.priors(logits[g * K], post[3][first:first + M], flags, s, noise)
            assert (post[2][first:first + M, 0] == want).all(), (g, M)
            SEEN["root_noise"] += int(cfg.dirichlet_weight > 0)
            rest = np.ones(len(post[2]), bool)
            rest[first:first + M] = False
            assert all((a == x).all() for a, x in zip((pre[g][0], pre[g][1], pre[g][3]), (post[0], post[1], post[3])))
            assert (pre[g][2][:, 1:] == post[2][:, 1:]).all() and (pre[g][2][rest, 0] == post[2][rest, 0]).all()
            assert e.game_state(g).phase == 1
        assert e.stats()["edge_overflow"] == self.overflows

    def _check_played_move(self, g, pre, st):
        """A due game: this select gave it no leaf and played vl_reference.forced_move on the tree the backup left."""
        now = self.e.game_state(g)
        j, mv = vlr.forced_move(pre, st.root_visits, self.cfg.seed, st.uid, st.ply)
        board, res, _, _ = vlr.expand_position(pre[0][0][0], pre[0][0][1], mv, 0)
        if res == 0 and now.uid == st.uid:
            assert now.ply == st.ply + 1 and now.phase == 0
            assert tuple(int(v) for v in self.e.tree(g)[0][0]) == board
            SEEN["forced_moves"] += 1
        else:
            assert res != 0 or now.ply == 0   # the game ended with the move (or at the ply limit): the slot began its next game


def _run_until_due(ls, limit=200):
    for _ in range(limit):
        ls.step()
        if ls.due.all():
            break
    assert ls.due.all()


# ------------------------------------------------------------------ 1. pinned priors

PRIOR_CASES = [(2, 7, 2, 0, False), (2, 16, 1, UAI, False), (1, 64, 3, 0, False), (2, 7, 2, 0, True)]


@pytest.mark.parametrize("G,K,VL,flags,symmetry", PRIOR_CASES)
def test_priors_of_new_nodes_and_of_the_root(G, K, VL, flags, symmetry):
    from tests.engine_harness import _positions
    e, cfg = _engine(_positions(G, 0), K, VL, flags, visits=64, seed=20261018)
    if symmetry:
        e.set_random_symmetry(True)
    _run_until_due(LockStep(e, cfg, K, VL, symmetry=symmetry))
    e.close()


def test_the_prior_cases_used_every_wave_the_noise_and_several_symmetries():
    assert SEEN["eval_slots"] >= 5 and SEEN["root_noise"] >= 5 and len(SEEN["symmetries"]) >= 4, SEEN


# ------------------------------------------------------------------ 2. wide nodes


@pytest.mark.parametrize("flags", [0, UAI])
def test_nodes_of_65_to_193_edges(flags):
    """(seed: one under which the root noise of the 193-move board in slot 2 makes the descent take its last edge, found
    with the restatement on the host)"""
    e, cfg = _engine(_wide_roots(), 8, 3, flags, visits=48, seed=20261109)
    _run_until_due(LockStep(e, cfg, 8, 3))
    e.close()


def test_a_proof_at_a_node_of_more_than_64_edges():
    """The solver over wide roots.  The boards of the `near` family (one or two empty cells) have at most 26 moves, so they
    cannot make the proof pass read a node in more than one round of 64 lanes; these four roots of the `wide` family (149 to
    168 moves) each have a move that takes the opponent's last stones, and the search finds it within its 48 visits, which
    proves the root — a node of more than 128 edges — a win."""
    wide = _edge_positions("wide")
    e, cfg = _engine([_pack(wide[i]["fen"]) for i in (15, 13, 16, 5)], 8, 3, 0, visits=48, seed=20261018)
    e.set_solver(True)
    ls = LockStep(e, cfg, 8, 3, solver=True)
    _run_until_due(ls)
    SEEN["wide_proofs"] += sum(1 for M, v in ls.proven if M > 64)
    assert e.proof_stats()["proven_nodes"] == len(ls.proven)
    assert any(M > 128 and v == 1 for M, v in ls.proven), ls.proven
    e.close()


def test_the_wide_cases_selected_edges_in_every_round_of_lanes():
    assert SEEN["idx64"] > 0 and SEEN["idx128"] > 0 and SEEN["idx192"] > 0 and SEEN["wide_proofs"] > 0, SEEN


# ------------------------------------------------------------------ 3. full arenas

def test_full_arenas_drop_the_path_end_the_batch_and_force_the_move():
    """edges_per_node = 8, the least azh_engine_create accepts: 48 nodes and 384 edges per game at 40 visits, of which the
    roots (151 and 158 moves) take a good part.  Chosen on the host with the restatement: slot 0's second batch cannot
    expand its first path, slot 1's second batch drops its third.  Nodes cannot run out before edges do (DESIGN.md,
    "Leaf-parallel search": a tree has at most 1 + root_visits nodes), so that branch is not forced.  After the forced moves
    the engine goes on for 20 more iterations in lock step (it meets further full arenas on the way)."""
    wide = _edge_positions("wide")
    e, cfg = _engine([_pack(wide[1]["fen"]), _pack(wide[5]["fen"])], 8, 2, 0, visits=40, seed=20261018, edges_per_node=8)
    assert (e.node_cap, e.edge_cap) == (48, 384)
    ls = LockStep(e, cfg, 8, 2, caps=True)
    _run_until_due(ls)
    assert SEEN["over_first"] >= 1 and SEEN["over_inside"] >= 1 and ls.overflows >= 2, SEEN
    for _ in range(20):
        ls.step()
    assert SEEN["forced_moves"] >= 2, SEEN
    e.close()


# ------------------------------------------------------------------ 4. many slots

@pytest.mark.parametrize("G,K", [(130, 7), (33, 64), (5, 33)])
def test_need_mask_and_leaf_list_over_many_slots(G, K):
    """Engine a evaluates through its own need mask and compacted leaf list; engine b is given the evaluations of exactly the
    ROOT / EVAL slots of the host's copy of the batch.  A game's K need bits start at bit (g K) mod 32 of the mask."""
    net, VL = eh.net(2), 2
    thin = G * K <= link.THIN_MAX_GAMES
    a, cfg = _engine(_fixture_positions(G), K, VL, 0, visits=24, seed=20261018)
    b, _ = _engine(_fixture_positions(G), K, VL, 0, visits=24, seed=20261018)
    rng = np.random.RandomState(G * K)
    SEEN["mask_offsets"] |= {(g * K) % 32 for g in range(G)}
    for it in range(12):
        sample = sorted(rng.choice(G, size=min(10, G), replace=False))
        pre = {g: (b.tree(g), b.game_state(g)) for g in sample}
        na, nb = a.select(), b.select()
        kind, lb, le = b.batch_leaves()
        need = np.nonzero(((kind == link.LEAF_EVAL) | (kind == link.LEAF_ROOT)).reshape(-1))[0]
        assert na == nb == len(need)
        logits = np.zeros((G * K, 833), np.float32)
        values = np.zeros(G * K, np.float32)
        if len(need):
            l, v = net.forward(lb.reshape(-1, 2)[need], 0, link.DTYPE_F32, thin=thin)
            logits[need], values[need] = l.reshape(-1, 833), v.reshape(-1)
        a.eval(net, link.DTYPE_F32)
        b.set_batch_evals(logits, values)
        a.backup()
        b.backup()
        (sa, ta), (sb, tb) = eh.dump(a), eh.dump(b)
        assert sa == sb
        for x, y in zip(ta, tb):
            _same_tree(x, y)
        assert a.stats() == b.stats() and a.collisions() == b.collisions()
        for g in sample:
            tree, st = pre[g]
            if st.phase != 1:
                continue
            ref = vlr.select(tree, st.root_visits, cfg.visits, K, VL, cfg.c_puct, False, 0)
            k = len(ref.kind)
            assert list(kind[g, :k]) == ref.kind and (kind[g, k:] == 0).all() and list(le[g, :k]) == ref.leaf_edge
            assert [tuple(int(v) for v in x) for x in lb[g, :k]] == ref.leaf_board
            exp, added = vlr.expected_tree(ref, values[g * K:(g + 1) * K], tb[g])
            _same_tree(exp, tb[g])
            for p, kd in enumerate(ref.kind):
                if kd == vlr.LEAF_EVAL:
                    first, M = ref.info[ref.leaf_node[p]][0], ref.info[ref.leaf_node[p]][1] & 0xFFFF
                    assert (tb[g][2][first:first + M, 0] == pr.priors(logits[g * K + p], tb[g][3][first:first + M])).all()
    assert a.stats()["plies"] > 0
    a.close(), b.close()


def test_the_many_slot_cases_met_unaligned_mask_offsets():
    assert len(SEEN["mask_offsets"]) == 32, SEEN
