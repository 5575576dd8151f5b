"""The game limit with loaded positions on the CPU oracle: the cases, the engines and the free run the limit's tests (oracle
and device) measure against."""
from oracle import oracle_lib as orc
from tests.helpers import synthetic_evals

LIMIT_CASES = [(6, 5), (6, 3), (12, 11), (12, 6)]   # (G, N): one slot past the limit, and half of them


LIMIT_PLIES = 160


def cells_of(board):
    p = orc.Pos()
    p.pieces[0], p.pieces[1] = int(board[0]) & ((1 << 63) - 1), int(board[1])
    return [int(v) for v in orc.board_cells(p)]


def free_run(G, N):
    """The loaded engine WITHOUT a limit, played until its first G games are over (computed once per case): what each uid's game
    is when nothing stops or delays it, and when it ends.  -> (games by uid, iteration each uid < G ended at)"""
    if (G, N) not in _free_runs:
        from tests.helpers import cohort_positions
        boards, plies = cohort_positions(G, N)
        e = limit_engine(G)
        e.set_positions(boards, plies)
        games, ended = {}, {}
        for it in range(6000):
            step(e)
            for g in range(G):
                if g not in ended and e.game_state(g).uid != g:
                    ended[g] = it
            for rec in e.pop_games(partial=True):
                games[rec["uid"]] = rec
            if len(ended) == G:
                break
        assert len(ended) == G
        _free_runs[(G, N)] = ({u: r for u, r in games.items() if u < G}, ended)
    return _free_runs[(G, N)]


_free_runs = {}


def limit_engine(G, flags=0, fen=orc.START_FEN_SELFPLAY):
    return orc.Engine(orc.make_config(G, 4, seed=11, fen_str=fen, max_plies=LIMIT_PLIES, flags=flags))


def step(e, evaluator=synthetic_evals):
    n, _ = e.select()
    e.backup(*evaluator(e.leaf_boards()))
    return n
