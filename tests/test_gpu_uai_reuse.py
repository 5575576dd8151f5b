"""The UAI front-end with --reuse-tree / --show-pv on the MI355X: the session's tree follows the game whatever messages
produce the position (`moves a b`, one `moves` per ply, `position fen`), `--visits N` means N more steps on top of the
inherited ones, the engine's visit limit shortens a search and says so, and with both options off nothing changes."""
import random

import pytest

from ataxxzero_amd import link, model, uai

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def net_path(tmp_path_factory):
    conv, bn = model.random_init(2, 128, seed=3)
    path = str(tmp_path_factory.mktemp("net") / "net.npy")
    model.save_model(path, conv, bn)
    return path


def _session(net_path, visits=200, **options):
    searcher = uai.Searcher(net_path, dtype="f16", **options)
    return uai.Session(searcher, visits=visits), searcher


def _go(session):
    out, more = session.handle("go movetime 1000")
    assert more and out[-1].startswith("bestmove ")
    return out


def _visits_below(tree, path):
    """Sum of the edge visits of the node the moves of `path` lead to from the root: its visit count as a root."""
    boards, info, edges, moves = tree
    node = 0
    for mv in path:
        first, m = int(info[node, 0]), int(info[node, 1] & 0xFFFF)
        j = moves[first:first + m].tolist().index(mv)
        assert int(edges[first + j, 3]) != NONE
        node = int(edges[first + j, 3])
    first, m = int(info[node, 0]), int(info[node, 1] & 0xFFFF)
    return int(edges[first:first + m, 1].sum())


def _first_search(net_path, **options):
    session, s = _session(net_path, **options)
    session.handle("uainewgame")
    _go(session)
    assert s.last_inherited == 0 and s.last_steps == 200 and s.last_report.root_visits == 200
    a, b = int(s.last_report.pv[0]), int(s.last_report.pv[1])
    return session, s, a, b, s.engine.tree(0)


@pytest.mark.parametrize("K", [1, 8])
def test_the_grandchild_is_inherited_through_a_moves_message(net_path, K):
    session, s, a, b, tree = _first_search(net_path, reuse_tree=True, parallel_leaves=K, virtual_loss=2)
    want = _visits_below(tree, [a, b])
    session.handle("moves %s %s" % (uai.encode_move(a), uai.encode_move(b)))
    _go(session)
    print("K", K, "inherited", s.last_inherited, "steps", s.last_steps)
    assert s.last_inherited == want > 0
    assert s.last_steps == 200 and s.engine.game_state(0).root_visits == want + 200 == s.last_report.root_visits
    assert s.engine.game_state(0).ply == 2 and s.engine.stats()["plies"] == 0   # the host's two moves, none sampled
    # the same position again: the search goes on
    _go(session)
    assert s.last_inherited == want + 200 and s.engine.game_state(0).root_visits == want + 400
    s.close()


def test_the_grandchild_is_inherited_through_position_fen(net_path):
    session, s, a, b, tree = _first_search(net_path, reuse_tree=True)
    want = _visits_below(tree, [a, b])
    pos = uai.Position.initial()
    pos.move(a)
    pos.move(b)
    session.handle("position fen " + pos.fen())
    _go(session)
    assert s.last_inherited == want > 0 and s.last_steps == 200
    # an unrelated position and a new game start from nothing
    session.handle("position fen xxx1ooo/xx3oo/x2o2x/3x3/o2x2o/oo3xx/ooo1xxx x")
    _go(session)
    assert s.last_inherited == 0 and s.last_report.root_visits == 200
    session.handle("uainewgame")
    _go(session)
    assert s.last_inherited == 0
    session.handle("uainewgame")   # the tree IS rooted at the start position now: a new game still starts from nothing
    _go(session)
    assert s.last_inherited == 0 and s.last_report.root_visits == 200
    s.close()


def test_one_moves_message_per_ply_takes_the_one_move_path(net_path):
    session, s, a, b, tree = _first_search(net_path, reuse_tree=True)
    session.handle("moves " + uai.encode_move(a))
    _go(session)
    assert s.last_inherited == _visits_below(tree, [a]) > 0 and s.engine.game_state(0).ply == 1
    tree = s.engine.tree(0)
    c = int(s.last_report.pv[0])
    session.handle("moves " + uai.encode_move(c))
    _go(session)
    assert s.last_inherited == _visits_below(tree, [c]) > 0 and s.engine.game_state(0).ply == 2
    s.close()


def test_with_reuse_off_the_dialogue_is_todays(net_path):
    dialogue = ["uai", "isready", "uainewgame", "go movetime 100", "moves c2", "go movetime 100", "moves f6 b2",
                "go movetime 100", "position fen xxx1ooo/xx3oo/x2o2x/3x3/o2x2o/oo3xx/ooo1xxx x", "go movetime 100"]
    kinds = {}
    for reuse in (False, True):
        random.seed(5)
        session, s = _session(net_path, visits=150, reuse_tree=reuse)
        kinds[reuse] = []
        for line in dialogue:
            out, more = session.handle(line)
            assert more
            kinds[reuse].append([" ".join(text.split()[:2]) if text.startswith("info") else text.split()[0] for text in out])
            if line.startswith("go"):
                assert out[0].startswith("info speed ") and out[0].endswith(" nps") and len(out) == 2
                assert s.last_steps == 150
                if not reuse:
                    assert s.last_inherited == 0 and s.engine is None and s.last_report is None
        s.close()
    assert kinds[False] == kinds[True]
    assert kinds[False][3] == ["info speed", "bestmove"] and kinds[False][0] == ["id", "id", "uaiok"]


@pytest.mark.parametrize("reuse", [False, True])
def test_show_pv_line_parses_and_its_moves_are_legal(net_path, reuse):
    session, s = _session(net_path, reuse_tree=reuse, show_pv=True)
    session.handle("uainewgame")
    for _ in range(2):
        out = _go(session)
        assert [text.split()[0:2] for text in out[:-1]] == [["info", "speed"], ["info", "nodes"]]
        words = out[1].split()
        assert words[0:2] == ["info", "nodes"] and words[3] == "inherited" and words[5] == "score" and words[7] == "pv"
        nodes, inherited, score = int(words[2]), int(words[4]), float(words[6])
        assert inherited == s.last_inherited and nodes == inherited + 200 and -1.0 <= score <= 1.0
        line = words[8:]
        assert 2 <= len(line) <= link.PV_MAX
        pos = uai.Position(session.position.x, session.position.o, session.position.turn)
        for text in line:
            legal, result = pos.legal_moves()
            assert result == 0 and uai.decode_move(text) in legal
            pos.move(uai.decode_move(text))
        session.handle("moves %s %s" % (line[0], line[1]))
    assert (s.last_inherited > 0) == reuse
    s.close()


def test_the_engines_visit_limit_shortens_the_search_and_says_so(net_path):
    """25000 more visits per `go` on one position, K = 32: the third search is cut at the engine's 60000 visits (the root's
    own move comes due on the device there), the fourth has nothing left to do — and the session goes on from that tree:
    the host's moves are played in place of the due one, and the device never samples."""
    session, s = _session(net_path, visits=25000, reuse_tree=True, parallel_leaves=32, virtual_loss=1)
    session.handle("uainewgame")
    seen = []
    for _ in range(4):
        out = _go(session)
        seen.append((s.last_inherited, s.last_steps, [t for t in out if t.startswith("info string")]))
    print(seen)
    assert [(i, n) for i, n, _ in seen] == [(0, 25000), (25000, 25000), (50000, 10000), (60000, 0)]
    assert seen[0][2] == [] and seen[1][2] == []
    assert "shortened to 10000 of 25000" in seen[2][2][0] and "shortened to 0 of 25000" in seen[3][2][0]
    assert s.engine.game_state(0).phase == 2
    tree = s.engine.tree(0)
    a, b = int(s.last_report.pv[0]), int(s.last_report.pv[1])
    want = _visits_below(tree, [a, b])
    session.handle("moves %s %s" % (uai.encode_move(a), uai.encode_move(b)))
    session.visits = 320
    _go(session)
    assert s.last_inherited == want > 0 and s.last_steps == 320
    state = s.engine.game_state(0)
    assert (state.ply, state.phase, state.root_visits) == (2, 1, want + 320) and s.engine.stats()["plies"] == 0
    s.close()
