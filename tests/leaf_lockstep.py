"""What the lock-step tests of the leaf-parallel search share (tests/test_gpu_vl_search.py, _vl_edges, _solver, _exploration,
_search_sets): one engine builder, and one LockStep that runs the HIP engine against the numpy restatement
(tests/vl_reference.py, its descent scored by tests/exploration_reference.py and its proofs by tests/solver_reference.py)
iteration by iteration.  step() asserts everything and returns what it met; what a file wants to have met it counts from
those records itself."""
import types

import numpy as np
import pytest

from ataxxzero_amd import link, model
from oracle import oracle_lib as orc
from tests import exploration_reference as xr
from tests import helpers
from tests import priors_reference as pr
from tests import solver_reference as sr
from tests import symmetry_reference as sym
from tests import vl_reference as vlr

UAI = link.FLAG_NO_REUSE | link.FLAG_TIE_FIRST | link.FLAG_PY_POSTERIOR
ALPHA, WEIGHT = 0.15, 0.25


def late(G, blockers, max_empty=10):
    """G distinct unfinished fixture positions of the blocker set with at most `max_empty` empty cells, spread over them."""
    ps = [(w0, w1) for w0, w1, bl in sr.late_positions(max_empty) if bl == blockers]
    assert len(ps) >= G
    return np.array([ps[(i * len(ps)) // G] for i in range(G)], dtype=np.uint64)


def config(G, flags=0, blockers=0, visits=300, seed=11, max_plies=400, edges_per_node=96, **more):
    p = orc.pos_from_fen(orc.START_FEN_PLAIN)
    return link.Config(games=G, visits=visits, max_plies=max_plies, edges_per_node=edges_per_node, c_puct=1.0,
                       dirichlet_alpha=ALPHA, dirichlet_weight=0.0 if flags else WEIGHT, start_turn=0, seed=seed,
                       start_x=int(p.pieces[0]), start_o=int(p.pieces[1]), blockers=blockers, flags=flags, **more)


def engine(G, flags=0, blockers=0, visits=300, seed=11, max_plies=400, edges_per_node=96, start="late", ply=10,
           leaf_batch=None, solver=False, exploration=None, sets=None, **more):
    """start: "late" (late(G, blockers) at ply 10), "start" (the start position), or G packed positions, loaded at `ply`.
    leaf_batch: (K, VL).  -> (engine, cfg)"""
    cfg = config(G, flags, blockers, visits, seed, max_plies, edges_per_node, **more)
    e = link.Engine(cfg)
    if not isinstance(start, str):
        e.set_positions(np.array(start, dtype=np.uint64), np.full(G, ply, np.int32))
    elif start == "late":
        e.set_positions(late(G, blockers), np.full(G, 10, np.int32))
    else:
        assert start == "start"
    if leaf_batch is not None:
        e.set_leaf_batch(*leaf_batch)
    if solver:
        e.set_solver(True)
    if exploration is not None:
        e.set_exploration(*exploration)
    if sets is not None:
        e.set_search_sets(sets)
    return e, cfg


class LockStep:
    """One engine against the restatement.  step() runs one iteration (select, the synthetic evaluations, backup) and checks
    it: the batch (kinds, leaf edges, leaf boards, the number of paths), the slots without a batch, the whole tree after the
    backup (the finished bits too while the solver is on), the root's visits and the phase.

    settings(g, tree, state) -> the settings in force at that root, a dict with the keys of link.SearchSet; the default is the
    engine's own (VL: what set_leaf_batch was given).  symmetry: the evaluation symmetry is on.  The switches: priors (of
    every evaluated node and root against tests/priors_reference.py), caps (the arena-full rule with the engine's arena
    sizes), root_proofs (azh_engine_root_proofs against the tree), played_move (a due game plays vl_reference.forced_move),
    overflow (the overflow counter counts the dropped paths)."""

    def __init__(self, e, cfg, VL=1, solver=False, settings=None, symmetry=False, priors=False, caps=False, root_proofs=False,
                 played_move=False, overflow=False):
        self.e, self.cfg, self.solver, self.symmetry, self.G = e, cfg, solver, symmetry, e.G
        own = dict(zip(("fpu_reduction", "c_base", "c_init"), e.exploration()), visits=cfg.visits, leaves=e.K, virtual_loss=VL,
                   c_puct=cfg.c_puct)
        self.settings = settings or (lambda g, tree, state: own)
        self.priors, self.root_proofs, self.played_move, self.overflow = priors, root_proofs, played_move, overflow
        self.caps = (e.node_cap, e.edge_cap) if caps else (None, None)
        self.tie_first = bool(cfg.flags & link.FLAG_TIE_FIRST)
        self.due = np.zeros(self.G, bool)      # the move became due at some backup
        self.overflows = 0

    def select(self, tree, root_visits, t):
        """The restatement's batch on `tree` with the values of settings t."""
        args = (tree, root_visits, t["visits"], t["leaves"], t["virtual_loss"], t["c_puct"], self.tie_first, self.cfg.blockers)
        if xr.mode_on(t["fpu_reduction"], t["c_base"]):
            return xr.select(*args, t["fpu_reduction"], t["c_base"], t["c_init"], *self.caps)
        return (sr.select if self.solver else vlr.select)(*args, *self.caps)

    def _symmetry(self, uid, board):
        return sym.eval_symmetry(self.cfg.seed, uid, board[0], board[1]) if self.symmetry else 0

    @staticmethod
    def _image(s, board):
        return (sym.board(s, board[0]), sym.board(s, board[1])) if s else tuple(board)

    def step(self, skip=()):
        """skip: slots whose batch is left unchecked.  -> a record: .games {g: (.state and .pre, the state and tree before;
        .batch, .settings, .syms, .post, .added, .proven, .due)} of the games that searched, .states (every slot's state
        before), .played (the slots whose forced move was checked, with played_move), .kind, .lb, .le, .logits, .values."""
        e, G, K, flags = self.e, self.G, self.e.K, self.cfg.flags
        pre = [e.tree(g) for g in range(G)]
        st = [e.game_state(g) for g in range(G)]
        e.select()
        kind, lb, le = e.batch_leaves()
        assert kind.shape == (G, K)
        games, roots, played = {}, {}, []
        for g in range(G):
            if st[g].phase == 1 and g in skip:
                continue
            if st[g].phase == 1:
                t = self.settings(g, pre[g], st[g])
                b = self.select(pre[g], st[g].root_visits, t)
                k = len(b.kind)
                assert b.over or k == max(1, min(t["leaves"], t["visits"] - st[g].root_visits))
                assert list(kind[g, :k]) == b.kind and (kind[g, k:] == 0).all(), (g, t, list(kind[g]), b.kind)
                assert list(le[g, :k]) == b.leaf_edge, (g, t)
                assert e.game_state(g).path_len == k          # the batch ended with its last path (a dropped one included)
                ss = [self._symmetry(st[g].uid, x) if kd == vlr.LEAF_EVAL else 0 for kd, x in zip(b.kind, b.leaf_board)]
                images = [self._image(s, x) for s, x in zip(ss, b.leaf_board)]
                assert [tuple(int(v) for v in x) for x in lb[g, :k]] == images, (g, t)
                games[g] = types.SimpleNamespace(state=st[g], pre=pre[g], batch=b, settings=t, syms=ss)
                self.overflows += int(b.over)
            elif st[g].phase == 0:
                assert kind[g, 0] == vlr.LEAF_ROOT and (kind[g, 1:] == 0).all()
                board = vlr.leaf_board(*pre[g][0][0])
                roots[g] = self._symmetry(st[g].uid, board)
                assert tuple(int(v) for v in lb[g, 0]) == self._image(roots[g], board)
            else:
                assert (kind[g] == 0).all()          # the move is due (this select plays it), or the slot is idle
                if self.played_move and st[g].phase == 2 and self._played_move(g, pre[g], st[g]):
                    played.append(g)
        logits, values = helpers.synthetic_evals_distinct(lb.reshape(-1, 2))
        e.set_batch_evals(logits, values)
        e.backup()
        proofs = e.root_proofs() if self.root_proofs else None
        for g, r in games.items():
            b, r.post = r.batch, e.tree(g)
            if self.solver:
                exp, r.added, r.proven = sr.expected_tree(b, values[g * K:(g + 1) * K], r.post)
                # the edge records carry the "finished" bit exactly where the child is decided
                assert ((e.tree_raw(g)[:, 3] >> 31) == sr.finished_bits(r.post)).all()
            else:
                (exp, r.added), r.proven = vlr.expected_tree(b, values[g * K:(g + 1) * K], r.post), []
            for a, x in zip(exp, r.post):         # (every prior but the new nodes' is the one of the dump before)
                assert a.shape == x.shape and (a == x).all(), g
            if self.priors:
                for p, kd in enumerate(b.kind):
                    if kd == vlr.LEAF_EVAL:
                        first, M = b.info[b.leaf_node[p]][0], b.info[b.leaf_node[p]][1] & 0xFFFF
                        assert first >= b.edges0
                        want = pr.priors(logits[g * K + p], r.post[3][first:first + M], flags, r.syms[p])
                        assert (r.post[2][first:first + M, 0] == want).all(), (g, p, M)
            if proofs is not None:                # the root's record says what the tree says
                first, M = int(r.post[1][0, 0]), int(r.post[1][0, 1] & 0xFFFF)
                assert proofs[g][0] == sr.decided_value(r.post[1][0])
                assert list(proofs[g][1][:M]) == [sr.decided_value(r.post[1][c]) if c != sr.NONE else 0
                                                  for c in (int(v) for v in r.post[2][first:first + M, 3])]
            after = e.game_state(g)
            assert after.root_visits == r.state.root_visits + r.added
            r.due = vlr.move_is_due(b, after.root_visits, r.settings["visits"])    # at the visits of the settings in force
            assert after.phase == (2 if r.due else 1), (g, after.root_visits, r.settings, after.phase)
            self.due[g] |= r.due
        if self.priors:
            for g, s in roots.items():
                self._root_priors(g, s, pre[g], st[g], logits[g * K])
        if self.overflow:
            assert e.stats()["edge_overflow"] == self.overflows
        return types.SimpleNamespace(games=games, states=st, played=played, kind=kind, lb=lb, le=le, logits=logits,
                                     values=values)

    def _root_priors(self, g, s, pre, st, logits):
        """A root's evaluation set its priors — the noise included — and nothing else."""
        cfg, post = self.cfg, self.e.tree(g)
        first, M = int(post[1][0, 0]), int(post[1][0, 1]) & 0xFFFF
        noise = (cfg.dirichlet_alpha, cfg.dirichlet_weight, cfg.seed, st.uid, st.ply)
        want = pr.priors(logits, post[3][first:first + M], cfg.flags, s, noise)
        assert (post[2][first:first + M, 0] == want).all(), (g, M)
        rest = np.ones(len(post[2]), bool)
        rest[first:first + M] = False
        assert all((a == x).all() for a, x in zip((pre[0], pre[1], pre[3]), (post[0], post[1], post[3])))
        assert (pre[2][:, 1:] == post[2][:, 1:]).all() and (pre[2][rest, 0] == post[2][rest, 0]).all()
        assert self.e.game_state(g).phase == 1

    def _played_move(self, g, pre, st):
        """A due game: this select gave it no leaf and played vl_reference.forced_move on the tree the backup left.  -> the
        game went on from the move's position (else it ended with the move, or at the ply limit)."""
        now = self.e.game_state(g)
        j, mv = vlr.forced_move(pre, st.root_visits, self.cfg.seed, st.uid, st.ply)
        board, res, _, _ = vlr.expand_position(pre[0][0][0], pre[0][0][1], mv, self.cfg.blockers)
        if res == 0 and now.uid == st.uid:
            assert now.ply == st.ply + 1 and now.phase == 0
            assert tuple(int(v) for v in self.e.tree(g)[0][0]) == board
            return True
        assert res != 0 or now.ply == 0   # the slot began its next game
        return False

    def until_due(self, limit=400, past_due=True):
        """step() until every game's move has become due, at most `limit` times; yields the records.  past_due: a game whose
        move has come due goes on being checked, through the move and at its next root, while the others search."""
        for _ in range(limit):
            yield self.step(() if past_due else np.nonzero(self.due)[0])
            if self.due.all():
                return
        raise AssertionError("moves not due after %d iterations: %s" % (limit, self.due))


def lane_rounds(b):
    """How many edges the batch's descents took at index >= 64, >= 128, >= 192 of their level (the rounds of 64 lanes)."""
    out = [0, 0, 0]
    for path in b.paths:
        node = 0
        for ed in path:
            j = ed - b.info[node][0]
            out[0] += j >= 64
            out[1] += j >= 128
            out[2] += j >= 192
            node = b.child[ed]
    return out


def memo(results, key, run):
    """run() once per key and session, whoever asks first: its result, or the exception it ended with, raised again."""
    if key not in results:
        try:
            results[key] = run()
        except BaseException as err:
            results[key] = err
    if isinstance(results[key], BaseException):
        raise results[key]
    return results[key]


def npy(tmp_path):
    conv, bn = model.random_init(2, 128, seed=5, perturb_bn=True)
    path = str(tmp_path / "net.npy")
    model.save_model(path, conv, bn)
    return path


def refused(call, code, message):
    with pytest.raises(link.AzhError) as ei:
        call()
    assert str(ei.value) == "ataxxzero_hip error %d: %s" % (code, message)
