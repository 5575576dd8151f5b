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
from tests import leaf_lockstep as lls
from tests import priors_reference as pr
from tests import vl_reference as vlr
from tests.engine_harness import _edge_positions, _pack, _wide_roots

pytestmark = pytest.mark.gpu

UAI = lls.UAI
SEEN = {"eval_slots": 0, "symmetries": set(), "root_noise": 0, "idx64": 0, "idx128": 0, "idx192": 0, "wide_proofs": 0,
        "over_first": 0, "over_inside": 0, "forced_moves": 0, "mask_offsets": set()}


def _engine(positions, K, VL, flags, visits, seed, edges_per_node=96, ply=10):
    return lls.engine(len(positions), flags, 0, visits, seed, edges_per_node=edges_per_node, start=positions, ply=ply,
                      leaf_batch=(K, VL))


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


def _run_until_due(e, cfg, VL, limit=200, **more):
    """Lock step (tests/leaf_lockstep.py) with the priors, the played moves and the overflow counter checked, until every
    game's move is due.  -> (the LockStep, [(edge count of a proven node, its value)])"""
    ls = lls.LockStep(e, cfg, VL, priors=True, played_move=True, overflow=True, **more)
    proven = []
    for rec in ls.until_due(limit):
        proven += _count(rec, ls)
    return ls, proven


def _count(rec, ls):
    """What an iteration met, into SEEN.  -> [(edge count of a node it proved, the value)]"""
    proven = []
    for r in rec.games.values():
        b = r.batch
        evals = [s for s, kd in zip(r.syms, b.kind) if kd == vlr.LEAF_EVAL]
        SEEN["symmetries"] |= set(evals) if ls.symmetry else set()
        SEEN["eval_slots"] = max(SEEN["eval_slots"], len(evals))
        if b.over:
            SEEN["over_first" if len(b.kind) == 1 else "over_inside"] += 1
        for key, count in zip(("idx64", "idx128", "idx192"), lls.lane_rounds(b)):   # every edge the descent took
            SEEN[key] += count
        proven += [(b.info[x][1] & 0xFFFF, v) for x, v, _, _ in r.proven]
    SEEN["root_noise"] += sum(1 for st in rec.states if st.phase == 0 and ls.cfg.dirichlet_weight > 0)
    SEEN["forced_moves"] += len(rec.played)
    return proven


# ------------------------------------------------------------------ 1. pinned priors

PRIOR_CASES = [(2, 7, 2, 0, False), (2, 16, 1, UAI, False), (1, 64, 3, 0, False), (2, 7, 2, 0, True)]


@pytest.mark.parametrize("G,K,VL,flags,symmetry", PRIOR_CASES)
def test_priors_of_new_nodes_and_of_the_root(G, K, VL, flags, symmetry):
    from tests.engine_harness import _positions
    e, cfg = _engine(_positions(G, 0), K, VL, flags, visits=64, seed=20261018)
    if symmetry:
        e.set_random_symmetry(True)
    _run_until_due(e, cfg, VL, symmetry=symmetry)
    e.close()


def test_the_prior_cases_used_every_wave_the_noise_and_several_symmetries():
    assert SEEN["eval_slots"] >= 5 and SEEN["root_noise"] >= 5 and len(SEEN["symmetries"]) >= 4, SEEN


# ------------------------------------------------------------------ 2. wide nodes


@pytest.mark.parametrize("flags", [0, UAI])
def test_nodes_of_65_to_193_edges(flags):
    """(seed: one under which the root noise of the 193-move board in slot 2 makes the descent take its last edge, found
    with the restatement on the host)"""
    e, cfg = _engine(_wide_roots(), 8, 3, flags, visits=48, seed=20261109)
    _run_until_due(e, cfg, 3)
    e.close()


def test_a_proof_at_a_node_of_more_than_64_edges():
    """The solver over wide roots.  The boards of the `near` family (one or two empty cells) have at most 26 moves, so they
    cannot make the proof pass read a node in more than one round of 64 lanes; these four roots of the `wide` family (149 to
    168 moves) each have a move that takes the opponent's last stones, and the search finds it within its 48 visits, which
    proves the root — a node of more than 128 edges — a win."""
    wide = _edge_positions("wide")
    e, cfg = _engine([_pack(wide[i]["fen"]) for i in (15, 13, 16, 5)], 8, 3, 0, visits=48, seed=20261018)
    e.set_solver(True)
    _, proven = _run_until_due(e, cfg, 3, solver=True)
    SEEN["wide_proofs"] += sum(1 for M, v in proven if M > 64)
    assert e.proof_stats()["proven_nodes"] == len(proven)
    assert any(M > 128 and v == 1 for M, v in proven), proven
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
    ls, _ = _run_until_due(e, cfg, 2, caps=True)
    assert SEEN["over_first"] >= 1 and SEEN["over_inside"] >= 1 and ls.overflows >= 2, SEEN
    for _ in range(20):
        _count(ls.step(), ls)
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
