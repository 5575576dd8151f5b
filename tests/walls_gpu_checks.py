"""The device checks of tests/test_gpu_walls.py on the sample store, run in a process of their own for the reason
tests/samples_gpu_checks.py gives: torch's runtime must be loaded first.  `python -m tests.walls_gpu_checks OUT.json` runs every
check and writes {name: "ok" | traceback}; after a check that ends in a device error nothing more is run."""
import numpy as np
import torch

from ataxxzero_amd import link, model, selfplay, training
from tests import fresh_process
from tests import rules_reference as rr
from tests import walls_fixtures as wf
from tests.store_checks import arrays_of, first_three, host, same, store_of_entries

F32 = np.float32
PASS = link.SAMPLES_PLY_PASS
ASYMMETRIC = selfplay.parse_fen(wf.ASYMMETRIC_FEN)[2]
DEFAULT = selfplay.parse_fen(wf.DEFAULT_FEN)[2]


# ---------------------------------------------------------------- 8. the gather

def check_gather_with_walls():
    entries, _ = wf.mixed_entries()
    store = store_of_entries(entries, spare=8)
    masks = store.game_blockers()
    assert masks.tolist() == [DEFAULT, 0, ASYMMETRIC, ASYMMETRIC, DEFAULT, 0]
    # every (game, ply, symmetry) of a grid: all 8 symmetries, both movers, the three kinds of game
    grid = [(g, ply, s) for g, e in enumerate(entries) for ply in range(min(4, len(e["moves"]))) if e["moves"][ply] != "pass"
            for s in range(8)]
    assert len(grid) >= 6 * 3 * 8
    got = host(store.gather(np.array(grid, dtype=np.int32)))
    want = first_three(entries, grid)
    same(got, want)
    walls = got[0][..., 3].reshape(len(grid), -1).sum(axis=1)
    assert [int(walls[i]) for i, (g, _, _) in enumerate(grid)] == [(0 if not masks[g] else 4) for g, _, _ in grid]
    images = {got[0][i, :, :, 3].tobytes() for i, (g, _, _) in enumerate(grid) if g == 2}
    assert len(images) == 8                                      # the asymmetric map under each symmetry
    # the reference draws: make_minibatch's samples
    import random
    for seed in range(2):
        random.seed(seed)
        want = training.make_minibatch_reference(entries, 128)
        state = random.getstate()
        random.seed(seed)
        same(host(training.make_minibatch_device(store, 0, len(entries), 128)), want)
        assert random.getstate() == state
    # device draws: the rows are the gather of the draws the host restates
    n = 256
    draws_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    out = host(store.draw_gather(n, 77, 3, 0, len(entries), 0.0, draws_out=draws_out))
    draws = draws_out.cpu().numpy()
    for i in range(n):
        assert tuple(int(v) for v in draws[i]) == store.draw(77, 3, i, 0, len(entries)), i
    same(out, host(store.gather(draws[:, :3])))
    same(out, first_three(entries, [tuple(int(v) for v in row[:3]) for row in draws]))
    assert {int(g) for g in draws[:, 0]} == set(range(6)) and {int(s) for s in draws[:, 2]} == set(range(8))
    assert store.status() == 0
    # refusals leave the store as it was
    before = store.counts()
    a = link.entries_to_arrays(entries[:2])
    for masks_in in ([1 << 49, 0], [int(a.boards[3][0]) & -int(a.boards[3][0]), 0], [0, int(a.boards[-1][1]) & -int(a.boards[-1][1])]):
        a.blockers = np.array(masks_in, dtype=np.uint64)
        try:
            store.add_arrays(a)
        except link.AzhError as err:
            assert "error -2" in str(err), err
        else:
            raise AssertionError("walls %r were accepted" % (masks_in,))
        assert store.counts() == before and store.game_blockers().tolist() == masks.tolist()
    try:
        store.add_entries([dict(entries[0], blockers=[23, 17])])
    except ValueError:
        pass
    else:
        raise AssertionError("a descending wall list was accepted")
    assert store.counts() == before
    # an unwalled store never allocates the masks and gathers what it did
    plain = store_of_entries([entries[1], entries[5]])
    assert plain.game_blockers().tolist() == [0, 0]
    rows = [(g, ply, s) for g in (0, 1) for ply in (0, 1) for s in range(8)]
    same(host(plain.gather(np.array(rows, dtype=np.int32))), first_three([entries[1], entries[5]], rows))
    plain.close()
    store.close()


# ---------------------------------------------------------------- 9. the surprise kernel

def seam_positions():
    """(mover, opponent, walls = the asymmetric map) with 1, 64 and 65 legal moves AFTER the walls have taken some away, found
    among seeded random boards; and the stuck corner: its only moves without walls go onto wall cells."""
    rng = np.random.default_rng(41)
    found = {}
    for _ in range(200000):
        if {64, 65} <= set(found):
            break
        cells = rng.choice(3, size=49, p=[0.6, 0.25, 0.15])
        mover = sum(1 << i for i in range(49) if cells[i] == 1) & ~ASYMMETRIC
        opponent = sum(1 << i for i in range(49) if cells[i] == 2) & ~ASYMMETRIC
        n = len(link.samples_legal(mover, opponent, ASYMMETRIC))
        if n in (64, 65) and n not in found and len(link.samples_legal(mover, opponent)) > n:
            found[n] = (mover, opponent, ASYMMETRIC)
    assert {64, 65} <= set(found), sorted(found)
    # a1 holds the mover's only stone; b1 and c1 are walls (a clone and a jump gone), a2 is empty, the rest is the opponent's
    corner_walls = (1 << 1) | (1 << 2)
    everything = (1 << 49) - 1
    found[1] = (1, everything & ~(1 | corner_walls | (1 << 7)), corner_walls)
    stuck = (1, everything & ~(1 | corner_walls), corner_walls)
    return found, stuck


def surprise_games():
    rng = np.random.default_rng(43)
    found, stuck = seam_positions()

    def ply(view, k=None):
        mover, opponent, walls = view
        legal = link.samples_legal(mover, opponent, walls)
        k = min(len(legal), k or int(rng.integers(1, 12)))
        chosen = rng.choice(legal, size=k, replace=False)
        return mover, opponent, 0, chosen, rng.dirichlet(np.ones(k)).astype(F32)

    removed = {}
    for n, (mover, opponent, walls) in found.items():
        gone = set(link.samples_legal(mover, opponent).tolist()) - set(link.samples_legal(mover, opponent, walls).tolist())
        assert len(link.samples_legal(mover, opponent, walls)) == n and gone
        removed[n] = ({i % 17 == 16 for i in gone})
    assert any(True in kinds for kinds in removed.values()) and any(False in kinds for kinds in removed.values())
    assert removed[1] == {True, False}                           # the corner: a wall takes a clone, another a jump
    assert len(link.samples_legal(*stuck)) == 0 and len(link.samples_legal(stuck[0], stuck[1])) == 2
    seams = [ply(found[64], 64), ply(found[65], 65), ply(found[65], 64), ply(found[64], 5), ply(found[65], 1)]
    corner = [ply(found[1], 1), (stuck[0], stuck[1], PASS, [], []), ply(found[1], 1)]

    def from_fixture(fen, count):
        out = []
        for entry, positions in wf.games(fen, 2):
            for board in positions[:count]:
                if rr.legal_moves(board):
                    out.append(ply(wf.mover_view(board)))
        return out
    return [(ASYMMETRIC, seams), (found[1][2], corner), (0, from_fixture(wf.PLAIN_FEN, 4)),
            (DEFAULT, from_fixture(wf.DEFAULT_FEN, 5)), (DEFAULT, from_fixture(wf.DEFAULT_FEN, 2)),
            (ASYMMETRIC, from_fixture(wf.ASYMMETRIC_FEN, 4))]


def check_surprise_with_walls():
    games = surprise_games()
    assert len(games) <= 8
    a = arrays_of(games)
    store = link.SampleStore(len(a.games), len(a.ply_flags), len(a.target_index))
    store.add_arrays(a)
    n = len(a.ply_flags)
    flags = store.mirror()[1]
    plies = [(walls,) + p for walls, ps in games for p in ps]
    rng = np.random.default_rng(47)
    logits = (3.0 * rng.standard_normal((n, 833))).astype(F32)

    def expected(rows):
        want, bare, illegal = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32), 0
        for i, (walls, mover, opponent, f, t_index, t_weight) in enumerate(plies):
            if int(flags[i]) & (PASS | link.SAMPLES_PLY_BAD):
                continue
            want[i], k = link.samples_surprise_host_blockers(rows[i], mover, opponent, walls, t_index, t_weight)
            bare[i], _ = link.samples_surprise_host_blockers(rows[i], mover, opponent, 0, t_index, t_weight)
            illegal += k
        return want, bare, illegal

    want, bare, illegal = expected(logits)
    stuck_at = len(games[0][1]) + 1
    assert illegal == 0 and int(flags[stuck_at]) & PASS and want[stuck_at] == 0
    # on the seam plies the walls take moves away by construction: the unmasked softmax ran over wall cells
    assert (want > 0).sum() >= n - 3 and (want[:5] != bare[:5]).all()
    dev = torch.from_numpy(logits).cuda()
    for first, last in ((0, n), (2, n - 1), (4, 6), (stuck_at, stuck_at + 1), (n - 1, n)):     # ranges that span mask changes
        got, bad = store.surprise_from_logits(first, dev[first:last].contiguous())
        assert got.tobytes() == want[first:last].tobytes(), (first, last, got, want[first:last])
        assert bad == 0
    # the tower-fed pass: per mask the net is shown that mask; chunks of 3 plies are cut inside a mask's run and at its end
    conv, bn = model.random_init(2, 64, seed=7, perturb_bn=True)
    net = link.Net(conv, bn)
    rows = np.zeros((n, 833), dtype=F32)
    for walls in sorted({p[0] for p in plies}):
        at = [i for i, p in enumerate(plies) if p[0] == walls]
        boards = np.array([(plies[i][1], plies[i][2]) for i in at], dtype=np.uint64)
        out, _ = net.forward(boards, walls, link.DTYPE_F32)
        rows[at] = np.asarray(out, dtype=F32).reshape(len(at), 833)
    fed, _ = store.surprise_from_logits(0, torch.from_numpy(rows).cuda())
    want_net, bare_net, _ = expected(rows)
    assert fed.tobytes() == want_net.tobytes()
    for chunk in (3, 0, 7):
        got, bad = store.surprise(net, link.DTYPE_F32, 0, len(games), chunk=chunk)
        assert bad == 0 and got.tobytes() == fed.tobytes(), (chunk, got, fed)
    part, _ = store.surprise(net, link.DTYPE_F32, 1, 4, chunk=3)                               # a window of games
    lo, hi = int(a.games[1][0]), int(a.games[4][0]) + int(a.games[4][1])
    assert part.tobytes() == fed[lo:hi].tobytes()
    # the same plies stored without their masks: the pass the trainer made before, a different KL
    a.blockers = np.zeros(len(a.games), dtype=np.uint64)
    bare_store = link.SampleStore(len(a.games), len(a.ply_flags), len(a.target_index))
    bare_store.add_arrays(a)
    unmasked, _ = bare_store.surprise(net, link.DTYPE_F32, 0, len(games), chunk=3)
    assert (unmasked[:5] != got[:5]).all() and (unmasked[8:16] == got[8:16]).all()       # (plies 8 .. 15: the game without walls)
    net.close()
    bare_store.close()
    store.close()


CHECKS = [check_gather_with_walls, check_surprise_with_walls]


if __name__ == "__main__":
    fresh_process.main(CHECKS)
