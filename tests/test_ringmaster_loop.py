"""The host loop of uai_ringmaster.py on the CPU: the script itself, run in a child process, with `arena.Match` replaced by a
recording stand-in (no device, no library), after the pattern of tests/test_generator_loop.py.  The stand-in is arena.Match with
a scripted engine behind it, so the match's own bookkeeping (drain, finished, lost_games) is the product's; what is checked is
the match's END: an odd cohort from openings is scored game for game and the script stops there, records lost on the device or
a cohort that ended short give exit code 3 instead of an endless search, and lost_games is asked only where its answer means
something — between a fetch and the next run.
"""
import json
import os
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = r'''
import json, os, runpy, sys
sys.path.insert(0, %(root)r)
from ataxxzero_amd import arena, model, selfplay

calls = []
LOG = %(log)r
MODE = os.environ.get("FAKE_MATCH", "healthy")
# the run (1 = the one before the loop) in which the game with this uid ends: scattered, and one long game, so that the
# match is still running at the loop's first look at lost_games (its 16th round)
ENDS = {0: 3, 1: 40, 2: 9, 3: 12, 4: 14, 5: 2, 6: 5, 7: 6}


class FakeNet:
    def close(self):
        pass


class FakeEngine:
    """`G` slots, slot g holding uid g.  Under the contract of azh_engine_set_game_limit a slot past the limit is idle: it
    is never searched, its game never ends, no counter moves for it.  FAKE_MATCH=strays is the engine before that contract
    covered loaded positions: every slot plays, and the games past the limit are counted like any other.
    FAKE_MATCH=overflow: the record of game 2 does not fit the ring (counted, never handed out, ring_overflow = 1).
    FAKE_MATCH=short: game 2 ends and is counted, and its record never reaches the host, with no overflow to explain it."""

    def __init__(self, G):
        self.G = G
        self.limit = None
        self.runs = 0
        self.ring = []           # ended on the device, not yet fetched
        self.staged = []         # fetched, not yet drained
        self.done = set()
        self.counters = {"games": 0, "dropped": 0, "ring_overflow": 0}

    def set_game_limit(self, n):
        calls.append(["limit", n])
        self.limit = n

    def set_thin_batches(self, mode):
        calls.append(["thin", mode])

    def run_arena(self, net_a, net_b, iterations, dtype):
        live = [u for u in range(self.G) if u not in self.done and (MODE == "strays" or u < self.limit)]
        calls.append(["run", iterations, live])
        self.runs += 1
        for u in live:
            if ENDS[u] <= self.runs:
                self.done.add(u)
                self.counters["games"] += 1
                if u == 2 and MODE == "overflow":
                    self.counters["ring_overflow"] += 1
                elif not (u == 2 and MODE == "short"):
                    self.ring.append(u)

    def fetch(self):
        calls.append(["fetch"])
        self.staged += self.ring
        self.ring = []

    def drain_json(self):
        out, self.staged = self.staged, []
        calls.append(["drain", out])
        cells = [0] * 49
        cells[0], cells[48] = 1, 2
        return [json.dumps({"slot": u, "uid": u, "moves": ["a2"], "boards": [cells], "result": 1}).encode() for u in out]

    def stats(self):
        calls.append(["stats", dict(self.counters)])
        return dict(self.counters)

    def close(self):
        calls.append(["close"])
        with open(LOG, "w") as f:
            json.dump(calls, f)


BaseMatch = arena.Match


class RecordingMatch(BaseMatch):
    def __init__(self, weights_a, weights_b, visits, games=1024, dtype="f16", seed=0, max_plies=400, opening_depth=0):
        calls.append(["create", games, visits, opening_depth])
        self.net_a, self.net_b, self.dtype = FakeNet(), FakeNet(), dtype
        self.engine = FakeEngine(games)
        self.games, self.opening_depth = games, opening_depth
        self.openings = [["a%%d" %% (k + 2), "g%%d" %% (k + 1), "b1"][:opening_depth] for k in range(games // 2)] if opening_depth else None
        self.opening_boards = None
        self.limit, self.finished, self.thin = None, 0, False

    def lost_games(self):
        why = BaseMatch.lost_games(self)
        calls.append(["lost_games", why])
        return why


arena.Match = RecordingMatch
selfplay.select_device = lambda index: index
model.load_model = lambda path: ([], [])
sys.argv = ["uai_ringmaster.py"] + %(argv)r
runpy.run_path(os.path.join(%(root)r, "uai_ringmaster.py"), run_name="__main__")
'''

ENGINES = ["--engine", "python uai_interface.py --network-path a.npy --visits 8",
           "--engine", "python uai_interface.py --network-path b.npy --visits 8"]


def ringmaster(tmp_path, argv, mode="healthy"):
    log = str(tmp_path / "calls.json")
    code = STUB % {"root": ROOT, "log": log, "argv": ENGINES + argv}
    env = dict(os.environ, FAKE_MATCH=mode)
    proc = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=120)
    calls = json.load(open(log)) if os.path.exists(log) else None
    return proc.returncode, proc.stdout.decode(), proc.stderr.decode(), calls


def names(calls):
    return [c[0] for c in calls if c[0] in ("run", "fetch", "lost_games", "drain")]


def assert_lost_games_only_between_a_fetch_and_the_next_run(calls):
    seq = names(calls)
    assert "lost_games" in seq
    for i, name in enumerate(seq):
        if name == "lost_games":
            assert seq[i - 1] == "fetch" and seq[i + 1] == "run", seq[max(i - 3, 0):i + 3]


def test_odd_cohort_from_openings_is_scored_game_for_game_and_the_script_stops_there(tmp_path):
    rc, out, err, calls = ringmaster(tmp_path, ["--game-count", "5", "--opening-depth", "3"])
    assert rc == 0, out + err
    assert ["create", 6, 8, 3] in calls and ["limit", 5] in calls           # six slots (both ways of three pairings), five games
    wins = [l for l in out.splitlines() if l.startswith("Wins:")]
    assert len(wins) == 5 and wins[-1] == "Wins: 3 - 2 (annulled: 0)"        # x wins every game: net a's in the even slots, net b's in the odd ones
    drained = [u for c in calls if c[0] == "drain" for u in c[1]]
    assert drained == [0, 2, 3, 4, 1]                                       # scattered ends, every uid once, nothing past the cohort
    games = [l for l in out.splitlines() if l.startswith("Game:")]
    assert len(games) == 5 and all("with opening: [a" in g for g in games)
    # slot 5 is never searched, and nothing is searched once the fifth game has been handed out
    assert all(5 not in c[2] for c in calls if c[0] == "run")
    last = max(i for i, c in enumerate(calls) if c[0] == "drain")
    assert calls[last][1] == [1] and [c[0] for c in calls[last + 1:]] == ["close"]
    # while the long game was still running the match was asked, and had nothing to report
    asked = [c[1] for c in calls if c[0] == "lost_games"]
    assert len(asked) >= 2 and all(a is None for a in asked)
    assert_lost_games_only_between_a_fetch_and_the_next_run(calls)


def test_the_stand_in_shows_what_strays_past_the_limit_did_to_a_healthy_match(tmp_path):
    """An engine that plays and counts the sixth slot's game (the game limit before it covered loaded positions) reaches
    games + dropped = 5 while game 1 of the cohort is still running: the match reports its end and the script gives up on a
    healthy match — the assertions above are not vacuous."""
    rc, out, err, calls = ringmaster(tmp_path, ["--game-count", "5", "--opening-depth", "3"], mode="strays")
    assert rc == 3 and "4 of 5 games were scored" in err
    assert any(5 in c[2] for c in calls if c[0] == "run")


def test_records_lost_on_the_device_end_the_match_with_exit_code_3(tmp_path):
    rc, out, err, calls = ringmaster(tmp_path, ["--game-count", "5", "--opening-depth", "3"], mode="overflow")
    assert rc == 3, out + err
    # (games 0, 3 and 4 had been scored by then; game 1 was still running)
    assert "did not fit the device's record ring" in err and "3 of 5 games were scored" in err
    assert len([l for l in out.splitlines() if l.startswith("Wins:")]) == 3
    # the loop ends within 16 rounds of the device's report (lost_games is looked at every 16th round)
    lost = max(i for i, c in enumerate(calls) if c[0] == "run" and 2 in c[2])    # the run in which game 2 ended
    assert sum(1 for c in calls[lost + 1:] if c[0] == "run") <= 16
    assert calls[-1] == ["close"]
    assert_lost_games_only_between_a_fetch_and_the_next_run(calls)


def test_a_cohort_that_ended_with_fewer_games_handed_out_ends_with_exit_code_3(tmp_path):
    rc, out, err, calls = ringmaster(tmp_path, ["--game-count", "5", "--opening-depth", "3"], mode="short")
    assert rc == 3, out + err
    assert "the engine has ended all 5 games of the match" in err and "4 of 5 games were scored" in err
    # not before the cohort's last game had ended on the device: every earlier answer was None
    asked = [c[1] for c in calls if c[0] == "lost_games"]
    assert asked[-1] is not None and all(a is None for a in asked[:-1]) and len(asked) >= 2
    ended_all = next(i for i, c in enumerate(calls) if c[0] == "stats" and c[1]["games"] + c[1]["dropped"] >= 5)
    assert sum(1 for c in calls[ended_all:] if c[0] == "run") <= 1           # the run enqueued under the drain, and no more
    assert_lost_games_only_between_a_fetch_and_the_next_run(calls)


def test_more_slots_than_games_leaves_the_slots_past_the_cohort_unsearched(tmp_path):
    rc, out, err, calls = ringmaster(tmp_path, ["--game-count", "6", "--concurrent", "8", "--opening-depth", "3"])
    assert rc == 0, out + err
    assert ["create", 8, 8, 3] in calls and ["limit", 6] in calls
    assert len([l for l in out.splitlines() if l.startswith("Wins:")]) == 6
    assert sorted(u for c in calls if c[0] == "drain" for u in c[1]) == [0, 1, 2, 3, 4, 5]
    assert all(max(c[2], default=0) < 6 for c in calls if c[0] == "run")
