"""The auxiliary training targets on the host (include/ataxxzero_hip.h, "Auxiliary targets"): azh_samples_final_owners and the
record path against tests/aux_reference.py's restatement on cell lists, the two host pipelines against each other and against
that restatement, the heads, their losses, the sidecar, and a training run on the CPU device.  The four ingest refusals are
checked here on the function the store calls (azh_samples_check_owners); that a refused call leaves a store as it was needs a
store, which lives in device memory: tests/aux_gpu_checks.py."""
import json
import os
import random

import numpy as np
import pytest
import torch

from ataxxzero_amd import link, model, training
from tests import aux_fixtures as fx
from tests import aux_reference as ar
from tests import rules_reference as rr
from tests import walls_fixtures as wf

F32 = np.float32
SEED = 11          # of the pipelines' draws: its 160 samples hold each weight both ways (test_both_branches_are_covered)


def popcount(v):
    return bin(int(v)).count("1")


def owners_of(board, move):
    x, o, walls = board.masks()
    return link.samples_final_owners(x, o, walls, board.turn, move)


def refused(board, move):
    with pytest.raises(link.AzhError, match="error -2"):
        owners_of(board, move)
    with pytest.raises(ar.Refused):
        ar.final_owners(board, move)


# ---------------------------------------------------------------- owners

def test_golden_games():
    entries = fx.golden_entries()
    counts = []
    for e in entries:
        want = ar.entry_owners(e)
        last = len(e["boards"]) - 1
        board = ar.entry_board(e, last)
        assert owners_of(board, ar.move_code(e["moves"][last])) == want
        assert link.entry_owners(e) == want[:2]
        final = rr.make_move(board, ar.move_code(e["moves"][last]))
        assert want[2] == e["result"] == rr.result(final) and not rr.legal_moves(final)      # terminal, the mover stuck
        assert want[0] & want[1] == 0 and want[0] | want[1] == (1 << 49) - 1
        counts.append((popcount(want[0]), popcount(want[1]), final.count(rr.EMPTY)))
    assert counts[1] == (28, 21, 1) and counts[4] == (23, 26, 1)          # the empty cell went to the side not to move
    assert [c[2] for c in counts].count(0) == 4


def test_walled_games():
    for (entry, positions), cells in zip(fx.walled_games(), [[17, 23, 25, 31]] * 3 + [wf.ASYMMETRIC_CELLS] * 3):
        assert entry["blockers"] == cells
        want = ar.entry_owners(entry)
        assert want[2] == entry["result"] != 0
        assert link.entry_owners(entry) == want[:2]
        walls = link.cells_to_blockers(cells)
        assert want[0] & want[1] == 0 and (want[0] | want[1]) & walls == 0 and want[0] | want[1] | walls == (1 << 49) - 1
        margin = popcount(want[0]) - popcount(want[1])
        assert entry["result"] == (2 if margin < 0 else 1)


def test_truncated_games_have_no_owners():
    for entry, _ in fx.walled_games():
        short = fx.cut(entry)
        assert len(short["boards"]) == fx.PLIES_CUT and link.entry_owners(short) == (0, 0) == ar.entry_owners(short)[:2]


def test_a_last_move_of_pass():
    stuck = rr.Board.from_fen("7/7/7/7/ooo4/ooo4/xoo4 x")            # x has no move, o has: the pass hands the turn over
    assert not rr.legal_moves(stuck)
    assert owners_of(stuck, rr.PASS) == (0, 0, 0) == ar.final_owners(stuck, rr.PASS)
    # after the pass the other side is stuck as well: the empty cells go to the side that passed
    both = rr.Board.from_fen("x--4/---4/---4/7/---4/---4/o--4 x")
    assert not rr.legal_moves(both) and not rr.legal_moves(rr.make_move(both, rr.PASS))
    got = owners_of(both, rr.PASS)
    assert got == ar.final_owners(both, rr.PASS) and got[2] == 1
    assert popcount(got[0]) == 49 - 16 - 1 and got[1] == 1 << 0


def test_refusals():
    start = rr.Board.from_fen("x5o/7/7/7/7/7/o5x x")
    refused(start, rr.PASS)                                           # a pass with a move available
    refused(start, 0 | 2 << 8)                                        # a source that is not the mover's (o's stone on a1)
    refused(start, 3 | 5 << 8)                                        # a source that is empty
    refused(start, 6 | 6 << 8)                                        # a destination that is not empty: a clone onto a stone
    refused(rr.Board.from_fen("x5o/7/7/7/7/7/o3x1x x"), 6 | 4 << 8)   # ... a jump onto one
    refused(start, 6 | 3 << 8)                                        # a wrong distance: three files
    refused(start, 6 | 5 << 8)                                        # ... one file, named as a jump
    refused(start, 24 | 24 << 8)                                      # a clone with no stone next to it
    for move in (0xFF | 5 << 8, 6 | 0x31 << 8, 0x1FFFF):              # squares beyond the board; a word beyond 16 bits
        with pytest.raises(link.AzhError, match="error -2"):
            owners_of(start, move)
    walled = rr.Board.from_fen("x5o/7/7/7/6-/5--/o4-x x")
    refused(walled, 6 | 5 << 8)                                       # a destination on a wall: a clone
    refused(walled, 6 | 20 << 8)                                      # ... a jump
    x, o, walls = start.masks()
    for args in ((x, o, 1 << 6), (x, o, 1 << 0), (x | 1 << 0, o, 0), (x, o, 1 << 49)):    # a stone on a wall; overlap; bit 49
        with pytest.raises(link.AzhError, match="error -2"):
            link.samples_final_owners(*args, 0, 6 | 5 << 8)
    # the one board on which the reference's two orders of adjudication disagree: the mover stuck, its opponent without stones
    freak = rr.Board.from_fen("7/7/7/7/---4/---4/x--4 o")
    assert rr.orders_disagree(rr.make_move(freak, rr.PASS))
    refused(freak, rr.PASS)
    # every legal move of a few positions is accepted, and nothing else among all 16-bit board moves
    for board in (start, walled, fx.walled_games()[3][1][30]):
        legal = set(rr.legal_moves(board))
        x, o, walls = board.masks()
        for frm in range(49):
            for to in range(49):
                move = frm | to << 8
                if move in legal:
                    assert owners_of(board, move) == ar.final_owners(board, move)
                else:
                    with pytest.raises(link.AzhError, match="error -2"):
                        link.samples_final_owners(x, o, walls, board.turn, move)


def test_a_side_without_stones():
    # the last move takes o's last stone: every empty cell goes to x, whoever is to move
    board = rr.Board.from_fen("7/7/7/7/7/7/xo5 x")
    got = owners_of(board, 0 | 2 << 8)
    assert got == ar.final_owners(board, 0 | 2 << 8) == ((1 << 49) - 1, 0, 1)


def test_ingest_refusals_on_the_host():
    entry = fx.walled_games()[3][0]
    x, o, result = ar.entry_owners(entry)
    walls = link.cells_to_blockers(entry["blockers"])
    check = link.load().azh_samples_check_owners
    assert check(x, o, walls, result) == 0 and check(0, 0, walls, 0) == 0 and check(0, 0, 0, 2) == 0
    cell = next(b for b in range(49) if x >> b & 1)
    wall = next(b for b in range(49) if walls >> b & 1)
    assert popcount(x) != popcount(o)
    for what, args in (("overlap", (x, o | 1 << cell, walls, result)), ("on walls", (x | 1 << wall, o, walls, result)),
                       ("beyond", (x | 1 << 49, o, walls, result)), ("unowned", (x & ~(1 << cell), o, walls, result)),
                       ("margin", (o, x, walls, result)), ("margin", (x, o, walls, 3 - result)),
                       ("margin", (x, o, walls, 0))):
        assert check(*args) == -2, what
        assert what in link.load().azh_last_error().decode(), (what, link.load().azh_last_error())


def test_the_host_pipelines_refuse_what_a_store_refuses():
    entry = fx.walled_games()[0][0]
    wrong = dict(entry, result=3 - entry["result"])                   # the margin contradicts the recorded result
    unnamed = {k: v for k, v in fx.walled_games()[3][0].items() if k != "blockers"}
    with pytest.raises(link.AzhError, match="error -2"):
        link.entry_owners(wrong)
    with pytest.raises(link.AzhError, match="error -2"):
        link.entries_to_arrays([entry, wrong], aux=True)
    with pytest.raises(link.AzhError, match="error -2"):
        training.aux_targets(wrong, 3, 0)
    for fn in (training.make_minibatch_reference, training.make_minibatch):
        with pytest.raises(link.AzhError, match="error -2"):
            fn([wrong], 4, 0.0, aux=True)
        assert len(fn([wrong], 4, 0.0)) == 3                          # without aux nobody looks at the game's end
    # a walled game whose line does not name its walls: its wall cells look empty, the game unfinished — no owners, or refused
    try:
        assert link.entry_owners(unnamed) == (0, 0)
    except link.AzhError as err:
        assert "error -2" in str(err)


# ---------------------------------------------------------------- records

def test_record_path_equals_line_path():
    for fen, mask in ((wf.PLAIN_FEN, 0), (wf.ASYMMETRIC_FEN, link.cells_to_blockers(wf.ASYMMETRIC_CELLS))):
        games = fx.passless_games(fen, 2)
        whole = [fx.record_of(e, positions, uid) for uid, (e, positions) in enumerate(games)]
        short = fx.record_of(fx.cut(games[0][0]), games[0][1][:fx.PLIES_CUT], 2)
        recs = whole + [short]
        packed = link.pack_records(np.concatenate(recs), mask, aux=True)
        lines = [json.loads(link.format_record_json(r, blockers=mask if mask else None)) for r in recs]
        from_lines = link.entries_to_arrays(lines, aux=True)
        assert packed.owners is not None and packed.owners.dtype == np.uint64 and packed.owners.shape == (3, 2)
        assert packed.owners.tobytes() == from_lines.owners.tobytes()
        assert packed.owners[:2].all() and not packed.owners[2].any()
        for name in link.SampleArrays.__slots__:                      # and the rest is what it is without aux
            plain = getattr(link.pack_records(np.concatenate(recs), mask), name)
            assert getattr(packed, name).tobytes() == plain.tobytes() == getattr(from_lines, name).tobytes(), name
        for (e, _), row in zip(games, packed.owners):
            assert tuple(int(v) for v in row) == ar.entry_owners(e)[:2]
    assert link.pack_records(np.concatenate(recs), mask).owners is None


def test_a_record_with_an_illegal_last_move():
    entry, positions = fx.passless_games(wf.PLAIN_FEN, 1)[0]
    rec = fx.record_of(entry, positions)
    at = len(rec) - len(entry["dists"][-1]) - 2                       # the last ply's move | nd << 16
    assert int(rec[at]) & 0xFFFF == rr.move_from_string(entry["moves"][-1])
    x, o, _ = positions[-1].masks()
    stone = next(sq for sq in range(49) if (x | o) >> sq & 1)
    bad = rec.copy()
    bad[at] = (int(rec[at]) & 0xFFFF0000) | stone | stone << 8         # a clone onto a stone
    for call in (lambda: link.pack_records(bad, 0, aux=True), lambda: link.pack_records(np.concatenate([rec, bad]), 0, aux=True)):
        with pytest.raises(link.AzhError, match="error -2"):
            call()
    assert len(link.pack_records(bad, 0).games) == 1                  # without aux the record is what it always was


# ---------------------------------------------------------------- the sample pipelines

def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == F32 and g.shape == w.shape and g.tobytes() == w.tobytes()


@pytest.fixture(scope="module")
def batches():
    entries = fx.mixed_entries()
    out = {}
    for name, fn in (("reference", training.make_minibatch_reference), ("batched", training.make_minibatch)):
        for aux in (False, True):
            random.seed(SEED)
            out[name, aux] = fn(entries, 160, 0.0, aux=aux)
            out[name, aux, "state"] = random.getstate()
    return entries, out


def test_pipelines_agree(batches):
    _, out = batches
    assert len(out["reference", True]) == 7 and len(out["reference", False]) == 3
    same(out["batched", True], out["reference", True])
    same(out["reference", True][:3], out["reference", False])
    same(out["batched", True][:3], out["batched", False])
    assert out["reference", True, "state"] == out["reference", False, "state"] == out["batched", True, "state"]
    shapes = [a.shape for a in out["reference", True]]
    assert shapes == [(160, 7, 7, 4), (160, 7, 7, 17), (160, 1), (160, 7, 7), (160, 1), (160, 7, 7, 17), (160, 2)]


def test_pipelines_match_the_restatement(batches):
    """The draws are found again from the arrays' own rows: every (game, ply, symmetry) whose three arrays are the row's."""
    entries, out = batches
    feats, pols, vals, ownership, score, reply, weight = out["reference", True]
    random.seed(SEED)
    draws = []
    for _ in range(160):
        entry, ply, s = training._draw_sample(entries)
        draws.append((next(g for g, e in enumerate(entries) if e is entry), ply, s))
    assert random.getstate() == out["reference", True, "state"]
    same((ownership, score, reply, weight), ar.batch(entries, draws))
    for i, (g, ply, s) in enumerate(draws[:40]):
        same(training.aux_targets(entries[g], ply, s), tuple(a[i] for a in (ownership, score, reply, weight)))


def test_both_branches_are_covered(batches):
    _, out = batches
    feats, _, _, ownership, score, reply, weight = out["reference", True]
    assert set(np.unique(weight).tolist()) == {0.0, 1.0}
    for column in (0, 1):
        assert 0 < weight[:, column].sum() < 160
    has, lacks = weight[:, 0] == 1, weight[:, 0] == 0
    assert not ownership[lacks].any() and not score[lacks].any()
    assert (np.abs(ownership[has]).sum(axis=(1, 2)) == 49 - feats[has][..., 3].sum(axis=(1, 2))).all()   # every cell but the walls
    assert (ownership[has].sum(axis=(1, 2)) == score[has, 0]).all() and (np.abs(score[has]) <= 49).all()
    assert (ownership[has][feats[has][..., 3] == 1] == 0).all()                                          # 0 on the walls
    assert not reply[weight[:, 1] == 0].any()
    assert (np.abs(1 - reply[weight[:, 1] == 1].sum(axis=(1, 2, 3))) < 1e-3).all()
    assert feats[has][..., 3].any() and not feats[has][..., 3].all(axis=(1, 2)).any()


def test_reply_is_absent_after_the_last_ply_and_before_a_pass_or_a_fast_ply():
    entry = fx.walled_games()[0][0]
    last = len(entry["boards"]) - 1
    assert training.aux_targets(entry, last, 3)[3].tolist() == [1.0, 0.0] == ar.targets(entry, last, 3)[3].tolist()
    assert training.aux_targets(entry, last - 1, 3)[3].tolist() == [1.0, 1.0]
    capped = fx.with_full(entry)
    assert [training.aux_targets(capped, p, 0)[3][1] for p in (0, 1, 2, 3)] == [0.0, 0.0, 1.0, 0.0]
    passed = dict(entry, moves=list(entry["moves"]), dists=list(entry["dists"]))
    passed["moves"][5], passed["dists"][5] = "pass", {}
    halved = dict(entry, dists=[{k: v * 0.5 for k, v in d.items()} for d in entry["dists"]])
    for e in (passed, halved):
        for got in (training.aux_targets(e, 4, 6), ar.targets(e, 4, 6)):
            assert got[3][1] == 0.0 and not got[2].any()
    one = fx.cut(entry, 1)
    assert training.aux_targets(one, 0, 0)[3].tolist() == [0.0, 0.0]


# ---------------------------------------------------------------- the network

def test_network_without_heads_is_the_network_it_was():
    torch.manual_seed(5)
    plain = training.Network(2, 32)
    keys = ["convs.%d.weight" % i for i in range(5)]
    keys += [k for i in range(5) for k in ("bns.%d.running_mean" % i, "bns.%d.running_var" % i, "bns.%d.num_batches_tracked" % i)]
    keys += ["policy.weight", "value_conv.weight", "fc.weight", "fc.bias"]
    assert list(plain.state_dict()) == keys == list(training.Network(2, 32, aux_heads=False).state_dict())
    assert not hasattr(plain, "aux_conv") and len(plain.to_numpy()[0]) == 2 * 2 + 5
    torch.manual_seed(5)
    state = torch.random.get_rng_state()
    torch.manual_seed(5)
    headed = training.Network(2, 32, aux_heads=True)
    after_headed = torch.random.get_rng_state()
    torch.manual_seed(5)
    training.Network(2, 32)
    assert torch.equal(after_headed, torch.random.get_rng_state()) and not torch.equal(state, after_headed)   # the heads drew nothing
    for k in keys:
        assert torch.equal(plain.state_dict()[k], headed.state_dict()[k]), k
    assert list(headed.state_dict())[:len(keys)] == keys
    assert set(headed.state_dict()) - set(keys) == {"aux_conv.weight", "aux_fc.weight", "aux_fc.bias", "reply_conv.weight"}
    conv, bn = headed.to_numpy()
    assert len(conv) == 2 * 2 + 5 and len(bn) == 2 * 5
    for a, b in zip(conv + bn, sum(plain.to_numpy(), [])):
        assert a.tobytes() == b.tobytes()


def test_heads_forward_and_sidecar(tmp_path):
    conv, bn = model.random_init(1, 32, seed=2, perturb_bn=True)
    net = training.Network(1, 32, aux_heads=True, aux_seed=7)
    net.load_numpy(conv, bn)
    net.eval()
    same_seed, other = training.Network(1, 32, aux_heads=True, aux_seed=7), training.Network(1, 32, aux_heads=True, aux_seed=8)
    for k, a in net.aux_to_numpy().items():
        assert a.dtype == F32 and a.tobytes() == same_seed.aux_to_numpy()[k].tobytes()
        assert k == "aux_fc_bias" or a.tobytes() != other.aux_to_numpy()[k].tobytes()
    assert np.abs(net.aux_to_numpy()["reply_conv"]).max() <= 2 * 0.2 * (2.0 / 32) ** 0.5 + 1e-6     # truncated at two sigma
    x = torch.from_numpy(np.random.default_rng(1).random((5, 4, 7, 7), dtype=F32))
    with torch.no_grad():
        policy, value = net(x)
        own, score, reply = net.aux_forward(x)
        policy2, value2, own2, score2, reply2 = net.forward_all(x)   # all five heads from one pass through the tower
    assert torch.equal(policy, policy2) and torch.equal(value, value2)
    assert own.shape == (5, 7, 7) and score.shape == (5, 1) and reply.shape == (5, 7, 7, 17) and float(own.abs().max()) < 1
    assert torch.equal(own, own2) and torch.equal(score, score2) and torch.equal(reply, reply2)
    assert policy.shape == (5, 7, 7, 17) and value.shape == (5, 1)
    path = training.aux_sidecar(str(tmp_path / "model-002.npy"))
    assert path.endswith("model-002.npy.aux.npz")
    with open(path, "wb") as f:
        np.savez(f, **net.aux_to_numpy())
    with np.load(path, allow_pickle=False) as kept:                 # plain arrays: readable with pickle refused
        assert sorted(kept.files) == ["aux_conv", "aux_fc_bias", "aux_fc_weight", "reply_conv"]
        assert other.load_aux_numpy(kept)
        assert not training.Network(1, 64, aux_heads=True).load_aux_numpy(kept)           # the shapes do not fit
    for k, a in net.aux_to_numpy().items():
        assert a.tobytes() == other.aux_to_numpy()[k].tobytes()


def test_weighted_means():
    rng = np.random.default_rng(3)
    n = 12
    conv, bn = model.random_init(1, 32, seed=4, perturb_bn=True)
    net = training.Network(1, 32, aux_heads=True, aux_seed=5)
    net.load_numpy(conv, bn)
    net.eval()
    feats = rng.random((n, 7, 7, 4)).astype(F32)
    ownership = rng.integers(-1, 2, size=(n, 7, 7)).astype(F32)
    score = rng.integers(-49, 50, size=(n, 1)).astype(F32)
    reply = rng.dirichlet(np.ones(833), size=n).astype(F32).reshape(n, 7, 7, 17)
    weight = np.array([[1, 1], [1, 0], [0, 1], [0, 0]] * 3, dtype=F32)
    tensors = [torch.from_numpy(a) for a in (feats, ownership, score, reply)]
    with torch.no_grad():
        own_p, score_p, logits = (t.double().numpy() for t in net.aux_forward(tensors[0].permute(0, 3, 1, 2)))
        got = [float(v) for v in training.aux_losses(net, *tensors, torch.from_numpy(weight))]
        zero = [float(v) for v in training.aux_losses(net, *tensors, torch.zeros(n, 2))]
        reply_only = [float(v) for v in training.aux_losses(net, *tensors, torch.from_numpy(weight * np.array([0, 1], dtype=F32)))]
    per_own = ((own_p - ownership) ** 2).reshape(n, -1).mean(axis=1)
    per_score = ((score_p - score.astype(np.float64) / 49) ** 2).reshape(n)
    z = logits.reshape(n, -1)
    logp = z - z.max(axis=1, keepdims=True) - np.log(np.exp(z - z.max(axis=1, keepdims=True)).sum(axis=1, keepdims=True))
    per_reply = -(reply.reshape(n, -1).astype(np.float64) * logp).sum(axis=1)
    wf_, wr = weight[:, 0].astype(np.float64), weight[:, 1].astype(np.float64)
    want = [(wf_ * per_own).sum() / max(1, wf_.sum()), (wf_ * per_score).sum() / max(1, wf_.sum()),
            (wr * per_reply).sum() / max(1, wr.sum())]
    assert got == pytest.approx(want, rel=1e-6) and min(want) > 0
    assert zero == [0.0, 0.0, 0.0] and reply_only[:2] == [0.0, 0.0] and reply_only[2] == pytest.approx(want[2], rel=1e-6)


# ---------------------------------------------------------------- training on the CPU device

def test_training_run_on_the_cpu_device(tmp_path):
    entries = [fx.cut(e, 40) for e, _ in fx.walled_games()] * 2 + [e for e, _ in fx.walled_games()]      # 18 games
    games = str(tmp_path / "games.json")
    with open(games, "w") as f:
        for e in entries:
            f.write(json.dumps(e) + "\n")
    conv, bn = model.random_init(1, 32, seed=3)
    old = str(tmp_path / "model-001.npy")
    model.save_model(old, conv, bn)

    def run(name, **named):
        new, lines = str(tmp_path / name), []
        net = training.train([games], old, new, steps=3, minibatch_size=16, device=torch.device("cpu"), log=lines.append, **named)
        with open(new, "rb") as f:
            return new, f.read(), lines, net

    plain, plain_bytes, plain_lines, _ = run("plain.npy")
    zero, zero_bytes, zero_lines, _ = run("zero.npy", aux_ownership=0.0, aux_score=0.0, aux_reply=0.0)
    assert plain_bytes == zero_bytes
    assert [l.replace(zero, plain) for l in zero_lines] == plain_lines
    assert not os.path.exists(training.aux_sidecar(plain)) and not os.path.exists(training.aux_sidecar(zero))
    new, new_bytes, lines, net = run("aux.npy", aux_ownership=1.5, aux_score=0.5, aux_reply=0.15)
    assert os.path.exists(training.aux_sidecar(new)) and new_bytes != plain_bytes
    assert [a.shape for a in model.load_model(new)[0]] == [a.shape for a in conv]
    assert any("of 8 training games have owners" in l for l in lines)
    assert [int(m.num_batches_tracked) for m in net.bns] == [3] * 3   # three steps, one pass through the tower each
    step0 = next(l for l in lines if l.startswith("Step:    0 -- loss:"))
    assert step0.startswith(next(l for l in plain_lines if l.startswith("Step:    0"))[:-1]) and \
        " own: " in step0 and " score: " in step0 and " reply: " in step0 and step0.endswith(")")
    fresh = training.aux_random_init(32, training.AUX_SEED)
    with np.load(training.aux_sidecar(new), allow_pickle=False) as kept:
        for k, a in fresh.items():
            assert kept[k].shape == a.shape and kept[k].dtype == F32 and kept[k].tobytes() != a.tobytes(), k     # the heads moved
            assert kept[k].tobytes() == net.aux_to_numpy()[k].tobytes()
    # the next generation reads the heads back
    assert any("freshly initialised" in l for l in lines)             # (old_path had no sidecar)
    os.replace(training.aux_sidecar(new), training.aux_sidecar(old))
    _, _, lines3, _ = run("aux3.npy", aux_ownership=1.5)
    assert any("read from" in l for l in lines3)
