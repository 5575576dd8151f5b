"""bench.py --dump-outputs on the CPU: the arrays dump_outputs writes from an engine's state, with a stand-in engine (the
GPU run itself: tests/test_gpu_cli.py::test_bench_plain_run_dumps_the_same_outputs_twice)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from ataxxzero_amd import link  # noqa: E402


class FakeEngine:
    """game g: a root with g + 1 edges (move 7 * j + g, prior 0.5 / (j + 1), visits j + 1, score -0.25 j) and one child"""

    def __init__(self, games, turn):
        self.G, self.turn = games, turn

    def game_state(self, g):
        s = link.GameState()
        s.n_nodes, s.n_edges, s.ply, s.uid = 2, g + 1, 10 + g, 100 * self.turn + g
        return s

    def tree(self, g):
        n = g + 1
        boards = np.array([[(1 << g) | (self.turn << 63), 1 << 48], [0, 0]], dtype=np.uint64)
        info = np.array([[0, n, 0, 0], [n, 0, 0, 0]], dtype=np.uint32)
        edges = np.zeros((n, 4), dtype=np.uint32)
        edges[:, 0] = (0.5 / np.arange(1, n + 1)).astype(np.float32).view(np.uint32)
        edges[:, 1] = np.arange(1, n + 1)
        edges[:, 2] = (-0.25 * np.arange(n)).astype(np.float32).view(np.uint32)
        edges[:, 3] = 0xFFFFFFFF
        return boards, info, edges, (7 * np.arange(n) + g).astype(np.uint16)


class FakeSelfPlay:
    def __init__(self):
        self.engines = [FakeEngine(3, 0), FakeEngine(2, 1)]


def test_dump_outputs_writes_the_engine_state_as_float_arrays(tmp_path):
    counters = {"steps": 1234, "nn_evals": 1000, "games": 2}
    bench.dump_outputs(FakeSelfPlay(), counters, str(tmp_path))
    out = {f[:-4]: np.load(str(tmp_path / f)) for f in os.listdir(str(tmp_path))}
    assert sorted(out) == ["counters", "game_state", "root_edges", "root_position"]
    assert all(a.dtype in (np.float32, np.float64) and a.size > 0 for a in out.values())
    c = out["counters"]
    assert len(c) == len(link.STAT_NAMES) and c[link.STAT_NAMES.index("steps")] == 1234 and c[link.STAT_NAMES.index("dropped")] == 0
    names = [n for n, _ in link.GameState._fields_]
    st = out["game_state"]
    assert st.shape == (5, 10) and list(st[:, names.index("uid")]) == [0, 1, 2, 100, 101]
    assert list(st[:, names.index("ply")]) == [10, 11, 12, 10, 11]
    pos = out["root_position"]
    assert pos.shape == (5, 50) and list(pos[:, 49]) == [0, 0, 0, 1, 1]     # side to move
    for slot, g in enumerate([0, 1, 2, 0, 1]):
        assert pos[slot, g] == 1 and pos[slot, 48] == 2 and (pos[slot, :48] != 0).sum() == 1
    e = out["root_edges"]
    assert e.shape == (1 + 2 + 3 + 1 + 2, 5) and list(e[:, 0]) == [0, 1, 1, 2, 2, 2, 3, 4, 4]
    assert list(e[3:6, 1]) == [2, 9, 16] and list(e[3:6, 3]) == [1, 2, 3]
    assert list(e[3:6, 2]) == [np.float32(0.5 / k) for k in (1, 2, 3)] and list(e[3:6, 4]) == [0, -0.25, -0.5]
    bench.dump_outputs(FakeSelfPlay(), counters, str(tmp_path / "again"))
    for name, a in out.items():
        assert (np.load(str(tmp_path / "again" / (name + ".npy"))) == a).all(), name


def test_dump_outputs_keeps_a_fixed_sample_of_an_array_over_its_share(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 5 * 8 * 4)   # a share of four root-edge rows
    for run in ("a", "b"):
        bench.dump_outputs(FakeSelfPlay(), {}, str(tmp_path / run))
    a, b = np.load(str(tmp_path / "a" / "root_edges.npy")), np.load(str(tmp_path / "b" / "root_edges.npy"))
    assert a.shape == (4, 5) and (a == b).all()
    assert list(a[:, 0]) == sorted(a[:, 0])          # rows stay in slot order
    assert np.load(str(tmp_path / "a" / "game_state.npy")).shape == (2, 10)   # (400 bytes over a share of 160)
    assert np.load(str(tmp_path / "a" / "counters.npy")).shape == (len(link.STAT_NAMES),)   # (within its share)
