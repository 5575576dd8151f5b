"""ctypes binding of libataxxzero_hip.so (include/ataxxzero_hip.h).

Mirror of the reference's link.py (link.py:6-32): the same four module-level
callables — launch_threads, get_workload, complete_workload, shutdown — with the
same argument order, bound to the GPU library instead of
./cpp/self_play_client.so, plus the `azh_*` device-resident entry points.

There is no CPU fallback: if the library is missing it is built with hipcc; if
no MI355X is visible every compute call raises AzhError.
"""
import collections
import ctypes
import os

import numpy as np

from . import build as _build

POLICY_SIZE = 833
FEATURE_SIZE = 196
MAX_MOVES = 256
STAT_COUNT = 16
THIN_MAX_GAMES = 512        # AZH_THIN_MAX_GAMES: engines of at most this many game slots evaluate with one board per workgroup
DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2
DTYPES = {"f32": DTYPE_F32, "fp32": DTYPE_F32, "float32": DTYPE_F32, "bf16": DTYPE_BF16,
          "f16": DTYPE_F16, "fp16": DTYPE_F16}
FORWARD_PLAIN, FORWARD_THIN, FORWARD_SYM = 0, 1, 2          # azh_net_forward's modes
LEAF_NONE, LEAF_EVAL, LEAF_TERMINAL, LEAF_ROOT = 0, 1, 2, 3
LEAF_COLLISION = 5          # leaf-parallel search: the path met a node an earlier path of its batch created
MAX_LEAVES_PER_GAME, MAX_VIRTUAL_LOSS = 64, 16
STAT_COLLISIONS = 15        # AZH_STAT_COLLISIONS (not in STAT_NAMES, whose order the bench's dumps follow): Engine.collisions()
FLAG_NO_REUSE, FLAG_TIE_FIRST, FLAG_PY_POSTERIOR, FLAG_SAMPLE_POW5, FLAG_KEEP_UNFINISHED, FLAG_TWO_NETS = 1, 2, 4, 8, 16, 32
FLAG_ARENA = 63
FLAG_SYMMETRY_AVG = 128    # nn_evals.py:48-62 on every evaluation
FLAG_ONE_RANDOM_MOVE = 64  # cpp/self_play_client.cpp:515-552 (compile-time variant of the reference client)
FLAG_EVAL_CACHE = 256      # engine.py:127-234: positions a game's search has already evaluated are not evaluated again
# azh_engine_play_moves / azh_engine_root_report (include/ataxxzero_hip.h)
PLAY_NONE, PLAY_KEPT, PLAY_FRESH, PLAY_FINISHED, PLAY_ILLEGAL, PLAY_BUSY = 0, 1, 2, 3, -1, -2
NO_MOVE = 0xFFFF            # a slot azh_engine_play_moves leaves alone
PV_MAX = 32
ROOT_REPORT_PV = 4 + 4 * MAX_MOVES
ROOT_REPORT_WORDS = ROOT_REPORT_PV + 1 + 2 * PV_MAX
ROOT_PROOF_WORDS = 1 + MAX_MOVES   # azh_engine_root_proofs
HIP_STREAM_LEGACY = 1                                                 # hipStreamLegacy: the null stream as a handle
SAMPLES_PLY_PASS, SAMPLES_PLY_FULL, SAMPLES_PLY_BAD = 1, 2, 4       # azh_samples_*: a ply's flags
SAMPLES_GAME_HAS_FULL, SAMPLES_GAME_HAS_VALUES = 1 << 8, 1 << 9     # beside the result in a game's third word
STAT_NAMES = ["steps", "nn_evals", "levels", "children", "new_moves", "plies", "games", "dropped",
              "edge_overflow", "reroot_nodes", "reroot_edges", "ring_overflow", "cache_hits", "parked", "reroot_spills"]


class AzhError(RuntimeError):
    pass


class Config(ctypes.Structure):
    _fields_ = [("games", ctypes.c_int32), ("visits", ctypes.c_int32), ("max_plies", ctypes.c_int32),
                ("edges_per_node", ctypes.c_int32), ("c_puct", ctypes.c_float),
                ("dirichlet_alpha", ctypes.c_float), ("dirichlet_weight", ctypes.c_float),
                ("start_turn", ctypes.c_int32), ("seed", ctypes.c_uint64), ("start_x", ctypes.c_uint64),
                ("start_o", ctypes.c_uint64), ("blockers", ctypes.c_uint64),
                ("flags", ctypes.c_uint32), ("select_budget", ctypes.c_uint32)]


class GameState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("phase", "arena", "n_nodes", "n_edges", "ply", "root_visits",
                                              "leaf_kind", "leaf_node", "path_len")] + [("uid", ctypes.c_uint32)]

    def as_tuple(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


class RootReport:
    """One slot's record of azh_engine_root_report: root_visits, result (0: not finished), expanded (root edges with a
    child), the root's edges in move generation order — moves (M,) u16, visits (M,) u32, scores (M,) f32 (total score W,
    seen from the side to move), priors (M,) f32 — and the principal variation: pv (L,) u16 moves, pv_visits (L,) u32."""
    __slots__ = ("root_visits", "result", "expanded", "moves", "visits", "scores", "priors", "pv", "pv_visits")

    def __init__(self, words):
        self.root_visits, m, self.expanded, self.result = (int(v) for v in words[:4])
        rows = words[4:4 + 4 * m].reshape(m, 4)
        self.moves = rows[:, 0].astype(np.uint16)
        self.visits = rows[:, 1].copy()
        self.scores = rows[:, 2].copy().view(np.float32)
        self.priors = rows[:, 3].copy().view(np.float32)
        n = int(words[ROOT_REPORT_PV])
        line = words[ROOT_REPORT_PV + 1:ROOT_REPORT_PV + 1 + 2 * n].reshape(n, 2)
        self.pv = line[:, 0].astype(np.uint16)
        self.pv_visits = line[:, 1].copy()


class Timing(ctypes.Structure):
    _fields_ = [("select_ms", ctypes.c_double), ("net_ms", ctypes.c_double), ("backup_ms", ctypes.c_double),
                ("iterations", ctypes.c_int64), ("net_evals", ctypes.c_int64)]


class SearchSet(ctypes.Structure):                            # azh_search_set
    _fields_ = [("visits", ctypes.c_int32), ("leaves", ctypes.c_int32), ("virtual_loss", ctypes.c_int32),
                ("c_puct", ctypes.c_float), ("fpu_reduction", ctypes.c_float), ("c_base", ctypes.c_float),
                ("c_init", ctypes.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


SEARCH_SETS_MAX = 16
SET_STAT_GAMES, SET_STAT_X_WINS, SET_STAT_O_WINS, SET_STAT_UNDECIDED, SET_STAT_COUNT = 0, 1, 2, 3, 4

_vp, _i32, _u64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_float
_P = ctypes.POINTER

# name -> (restype, argtypes); every symbol include/ataxxzero_hip.h declares
SIGNATURES = {
    "azh_last_error": (ctypes.c_char_p, []),
    "azh_device_count": (ctypes.c_int, []),
    "azh_set_device": (ctypes.c_int, [ctypes.c_int]),
    "azh_device_pci_bus_id": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
    "azh_perft": (ctypes.c_int, [_u64, _u64, _u64, ctypes.c_int, ctypes.c_int, _P(_u64)]),
    "azh_rules_batch": (ctypes.c_int, [ctypes.c_int, _vp, _u64, _vp, _vp, _vp]),
    "azh_makemove_batch": (ctypes.c_int, [ctypes.c_int, _vp, _vp, _vp]),
    "azh_features_batch": (ctypes.c_int, [ctypes.c_int, _vp, _u64, _vp]),
    "azh_random_play": (ctypes.c_int, [ctypes.c_int, _u64, _u64, _u64, _u64, ctypes.c_int, ctypes.c_int,
                                       _vp, _vp, _vp, _vp]),
    "azh_probe_detmath": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, _vp, _u64, _vp]),
    "azh_alphabeta_search": (ctypes.c_int, [ctypes.c_int, _vp, _u64, _vp, ctypes.c_int, _u64, _vp, _vp, _vp, _vp]),
    "azh_alphabeta_host": (ctypes.c_int, [_u64, _u64, _u64, ctypes.c_int, ctypes.c_int, _u64, _vp, _vp, _vp, _vp]),
    "azh_alphabeta_play": (ctypes.c_int, [ctypes.c_int, _u64, _u64, _u64, _u64, ctypes.c_int, _vp, _vp, ctypes.c_int, _u64,
                                          _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "azh_net_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, _vp, _f32, _P(_vp)]),
    "azh_net_destroy": (None, [_vp]),
    "azh_net_forward": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _u64, _vp, _vp, _vp]),
    "azh_net_bench": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P(_f32)]),
    "azh_net_tower_choice": (ctypes.c_int, [ctypes.c_int] * 8 + [_vp]),
    "azh_net_stamps": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp]),
    "azh_engine_create": (ctypes.c_int, [_P(Config), _P(_vp)]),
    "azh_engine_destroy": (None, [_vp]),
    "azh_engine_node_cap": (ctypes.c_int, [_vp]),
    "azh_engine_edge_cap": (ctypes.c_int, [_vp]),
    "azh_engine_select": (ctypes.c_int, [_vp, _P(_i32)]),
    "azh_engine_leaves": (ctypes.c_int, [_vp, _vp, _vp]),
    "azh_engine_leaf_features": (ctypes.c_int, [_vp, _vp, _vp]),
    "azh_engine_eval": (ctypes.c_int, [_vp, _vp, ctypes.c_int]),
    "azh_engine_set_evals": (ctypes.c_int, [_vp, _vp, _vp]),
    "azh_engine_backup": (ctypes.c_int, [_vp]),
    "azh_engine_run": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int]),
    "azh_engines_run": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int]),
    "azh_engine_run_arena": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int]),
    "azh_engine_sync": (ctypes.c_int, [_vp]),
    "azh_engine_set_visits": (ctypes.c_int, [_vp, ctypes.c_int]),
    "azh_engine_set_thin_batches": (ctypes.c_int, [_vp, ctypes.c_int]),
    "azh_engine_set_leaf_batch": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "azh_engine_batch_leaves": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "azh_engine_set_batch_evals": (ctypes.c_int, [_vp, _vp, _vp]),
    "azh_engine_set_playout_cap": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "azh_playout_cap_kind": (ctypes.c_int, [_u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    "azh_engine_set_forced_playouts": (ctypes.c_int, [_vp, _f32]),
    "azh_forced_prune": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _f32, _f32, _vp]),
    "azh_engine_set_gumbel": (ctypes.c_int, [_vp, ctypes.c_int, _f32, _f32]),
    "azh_gumbel_considered_visits": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp]),
    "azh_gumbel_noise": (ctypes.c_int, [_u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, _vp]),
    "azh_gumbel_root": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _f32, _vp, _f32, _f32, _vp, _P(_i32)]),
    "azh_engine_set_random_symmetry": (ctypes.c_int, [_vp, ctypes.c_int]),
    "azh_eval_symmetry": (ctypes.c_int, [_u64, ctypes.c_uint32, _u64, _u64]),
    "azh_engine_set_resign": (ctypes.c_int, [_vp, _f32, ctypes.c_int, ctypes.c_int]),
    "azh_resign_playthrough": (ctypes.c_int, [_u64, ctypes.c_uint32, ctypes.c_uint32]),
    "azh_engine_resign_stats": (ctypes.c_int, [_vp, _vp]),
    "azh_engine_set_temperature": (ctypes.c_int, [_vp, _vp, _vp]),
    "azh_temperature_pick": (ctypes.c_int, [_vp, ctypes.c_int, _f32, _u64, ctypes.c_uint32, ctypes.c_uint32, _vp]),
    "azh_symmetry_board": (_u64, [ctypes.c_int, _u64]),
    "azh_symmetry_move": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint16]),
    "azh_symmetry_policy_index": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "azh_engine_set_solver": (ctypes.c_int, [_vp, ctypes.c_int]),
    "azh_engine_proof_stats": (ctypes.c_int, [_vp, _vp]),
    "azh_engine_set_exploration": (ctypes.c_int, [_vp, _f32, _f32, _f32]),
    "azh_engine_exploration": (ctypes.c_int, [_vp, _vp]),
    "azh_exploration_scores": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _f32, _f32, _f32, _f32, _vp]),
    "azh_engine_set_search_sets": (ctypes.c_int, [_vp, ctypes.c_int, _vp]),
    "azh_engine_search_sets": (ctypes.c_int, [_vp, _P(_i32), _vp]),
    "azh_search_set_pairing": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_int, _vp]),
    "azh_engine_search_set_stats": (ctypes.c_int, [_vp, _vp]),
    "azh_engine_root_proofs": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp]),
    "azh_engine_play_moves": (ctypes.c_int, [_vp, _vp, _vp]),
    "azh_engine_root_report": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp]),
    "azh_engine_root_report_device": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp]),
    "azh_engine_game_state": (ctypes.c_int, [_vp, ctypes.c_int, _P(GameState)]),
    "azh_engine_tree": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "azh_engine_tree_raw": (ctypes.c_int, [_vp, ctypes.c_int, _vp]),
    "azh_engine_stats": (ctypes.c_int, [_vp, _vp]),
    "azh_engine_tree_stamps": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp]),
    "azh_engine_timing_reset": (ctypes.c_int, [_vp, ctypes.c_int]),
    "azh_engine_timing": (ctypes.c_int, [_vp, _P(Timing)]),
    "azh_engine_fetch": (ctypes.c_int, [_vp]),
    "azh_engine_query": (ctypes.c_int, [_vp]),
    "azh_engine_implicit_fetches": (ctypes.c_longlong, [_vp]),
    "azh_engine_staged_records": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _P(ctypes.c_int64)]),
    "azh_engine_drain_json": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _P(ctypes.c_int64), _P(_i32)]),
    "azh_format_record_json": (ctypes.c_int, [_vp, ctypes.c_int64, _i32, _vp, ctypes.c_int64, _P(ctypes.c_int64)]),
    "azh_engine_set_emit_order": (ctypes.c_int, [_vp, ctypes.c_int]),
    "azh_engine_set_record_blockers": (ctypes.c_int, [_vp, ctypes.c_int]),
    "azh_format_record_json_blockers": (ctypes.c_int, [_vp, ctypes.c_int64, _i32, _u64, _vp, ctypes.c_int64,
                                                       _P(ctypes.c_int64)]),
    "azh_engine_set_positions": (ctypes.c_int, [_vp, _vp, _vp]),
    "azh_engine_set_start_pool": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "azh_start_pool_entry": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_int, ctypes.c_int]),
    "azh_engine_uid_blockers": (ctypes.c_int, [_vp, ctypes.c_uint32, _vp]),
    "azh_engine_set_game_limit": (ctypes.c_int, [_vp, ctypes.c_int64]),
    "azh_samples_create": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _P(_vp)]),
    "azh_samples_destroy": (None, [_vp]),
    "azh_samples_add_games": (ctypes.c_int, [_vp, _vp]),
    "azh_samples_pack_records": (ctypes.c_int, [_vp, ctypes.c_int64, _u64, _vp, ctypes.c_int64, ctypes.c_int, _vp]),
    "azh_samples_add_records": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _u64, _vp, ctypes.c_int64, ctypes.c_int]),
    "azh_samples_game_blockers": (ctypes.c_int, [_vp, _vp]),
    "azh_samples_surprise_host_blockers": (ctypes.c_int, [_vp, _u64, _u64, _u64, _vp, _vp, ctypes.c_int, _P(_f32), _P(_i32)]),
    "azh_samples_counts": (ctypes.c_int, [_vp, _vp]),
    "azh_samples_mirror": (ctypes.c_int, [_vp, _vp, _vp]),
    "azh_samples_gather": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_double, _vp, ctypes.c_size_t]),
    "azh_samples_draw_gather": (ctypes.c_int, [_vp, ctypes.c_int, _u64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_double, _vp, _vp, ctypes.c_size_t]),
    "azh_samples_draw": (ctypes.c_int, [_u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_int64, _vp,
                                        ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "azh_samples_status": (ctypes.c_int, [_vp, _P(ctypes.c_int64)]),
    "azh_samples_surprise_logits": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _vp, _vp, _P(ctypes.c_int64),
                                                   ctypes.c_size_t]),
    "azh_samples_surprise": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, _vp, _P(ctypes.c_int64)]),
    "azh_samples_set_surprise_chunk": (ctypes.c_int, [_vp, ctypes.c_int]),
    "azh_samples_surprise_ms": (ctypes.c_int, [_vp, _vp]),
    "azh_samples_legal": (ctypes.c_int, [_u64, _u64, _u64, _vp, _P(_i32)]),
    "azh_samples_surprise_host": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _P(_f32), _P(_i32)]),
    "azh_samples_set_ply_weights": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _vp]),
    "azh_samples_clear_ply_weights": (ctypes.c_int, [_vp]),
    "azh_samples_ply_cum": (ctypes.c_int, [_vp, _vp, _vp, _vp, _P(_i32)]),
    "azh_samples_final_owners": (ctypes.c_int, [_u64, _u64, _u64, ctypes.c_int, ctypes.c_uint32, _vp, _P(_i32)]),
    "azh_samples_check_owners": (ctypes.c_int, [_u64, _u64, _u64, ctypes.c_uint32]),
    "azh_samples_game_owners": (ctypes.c_int, [_vp, _vp]),
    "azh_samples_read_plies": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64]),
    "azh_samples_ply_targets": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp]),
    "azh_samples_retarget": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _u64, _vp, ctypes.c_size_t]),
    "azh_samples_retarget_host": (ctypes.c_int, [_vp, _vp, _vp, _P(_i32), _P(ctypes.c_double)]),
    "azh_samples_prove": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, _u64, ctypes.c_int, _vp]),
    "azh_samples_proofs": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp, _vp]),
    "azh_samples_value_returns": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_double]),
    "azh_samples_clear_value_returns": (ctypes.c_int, [_vp]),
    "azh_samples_read_value_returns": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp]),
    "azh_samples_value_returns_host": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_uint32, ctypes.c_double, _vp]),
    # the reference's ABI, link.py:8-32
    "launch_threads": (None, [ctypes.c_char_p, ctypes.c_int, _vp, _vp, ctypes.c_int, ctypes.c_int]),
    "get_workload": (ctypes.c_int, []),
    "complete_workload": (None, [ctypes.c_int, _vp, _vp]),
    "shutdown": (None, []),
}

_dll = None


def library_path():
    return _build.LIB


def load():
    """Load (building first if needed) the HIP library and type its symbols."""
    global _dll
    if _dll is not None:
        return _dll
    path = os.environ.get("AZH_LIB") or _build.build()  # AZH_LIB: load a specific build (A/B runs)
    dll = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(dll, name)
        fn.restype = res
        fn.argtypes = args
    _dll = dll
    return dll


def check(rc):
    if rc != 0:
        raise AzhError("ataxxzero_hip error %d: %s" % (rc, load().azh_last_error().decode(errors="replace")))


def device_count():
    n = load().azh_device_count()
    return max(n, 0)


def require_gpu():
    n = load().azh_device_count()
    if n <= 0:
        raise AzhError("no MI355X / HIP device visible (azh_device_count = %d: %s); this package has no CPU "
                       "fallback" % (n, load().azh_last_error().decode(errors="replace")))
    return n


def pci_bus_id(device):
    buf = ctypes.create_string_buffer(64)
    check(load().azh_device_pci_bus_id(int(device), buf, 64))
    return buf.value.decode()


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


# ------------------------------------------------------------------ reference ABI (link.py:8-32)

def launch_threads(output_path, visits, fill_buffer1, fill_buffer2, buffer_entries, thread_count):
    load().launch_threads(output_path, visits, fill_buffer1, fill_buffer2, buffer_entries, thread_count)


def get_workload():
    return load().get_workload()


def complete_workload(workload, posteriors, values):
    load().complete_workload(workload, posteriors, values)


def shutdown():
    load().shutdown()


def format_record_json(rec, with_ids=False, blockers=None):
    """The JSON line (bytes, no newline) of one finished-game record — uint32 words as the device loop leaves them in its
    ring — in the reference's entry format (cpp/self_play_client.cpp:565-578,639-641).  blockers: None, or a wall mask (bit
    = file + 7 * rank): the line gains "blockers", its cells in the index of the line's boards, in front
    (azh_format_record_json_blockers).  Host code only: no GPU needed."""
    rec = np.ascontiguousarray(rec, dtype=np.uint32)

    def call(buf, used):
        if blockers is None:
            return load().azh_format_record_json(_ptr(rec), rec.size, int(bool(with_ids)), _ptr(buf), buf.nbytes,
                                                 ctypes.byref(used))
        return load().azh_format_record_json_blockers(_ptr(rec), rec.size, int(bool(with_ids)), int(blockers), _ptr(buf),
                                                      buf.nbytes, ctypes.byref(used))
    buf = np.zeros(1 << 16, dtype=np.uint8)
    used = ctypes.c_int64(0)
    rc = call(buf, used)
    if rc == -6:
        buf = np.zeros(used.value, dtype=np.uint8)
        rc = call(buf, used)
    check(rc)
    return bytes(buf[:used.value])


# The finished-game record, as csrc/record.h defines it and under its names: the header's words, then per ply 6 fixed words
# {x lo, x hi, o lo, o hi, move | nd << 16, word 5} and nd x (move | count << 16).
RECORD_MAGIC = 0x415A4847
REC_MAGIC, REC_SLOT, REC_UID, REC_PLIES, REC_RESULT, REC_WORDS, REC_RANDOM_PLY_PLUS_1, REC_KIND = range(8)
REC_HDR_WORDS, REC_PLY_WORDS, REC_MAXD = 8, 6, 256
REC_KIND_MASK, REC_KIND_WHOLE, REC_KIND_DROPPED, REC_KIND_LOADED = 3, 0, 1, 2      # bits 0-1 of the kind word
REC_KIND_PLAYOUT_CAP, REC_KIND_FORCED, REC_KIND_VALUES, REC_KIND_RESIGNED, REC_KIND_GUMBEL = 4, 8, 16, 32, 64
REC_KIND_MODES = 124
REC_PLY_FULL_BIT, REC_PLY_Q_BITS = 0x80000000, 0x7FFFFFFF                           # word 5 under REC_KIND_VALUES

Record = collections.namedtuple("Record", "slot uid result kind plies words")


def records(words, markers=False):
    """The records of `words` (uint32, one record after the other, as Engine.staged_records returns them), one Record each:
    slot, uid, result, the kind word, plies = [(move, word 5, {move: count}, (x, o))] and the record's own words (a view).
    A dropped game's marker is left out unless `markers`.  Asserts the magic, that every record lies within `words` and that
    its plies walk to its end exactly."""
    pos = 0
    while pos < len(words):
        assert pos + REC_HDR_WORDS <= len(words) and words[pos] == RECORD_MAGIC, pos
        slot, uid, n_plies, result, n, kind = (int(words[pos + i]) for i in (REC_SLOT, REC_UID, REC_PLIES, REC_RESULT,
                                                                            REC_WORDS, REC_KIND))
        assert REC_HDR_WORDS <= n <= len(words) - pos, (pos, n)
        rec, plies, q = words[pos:pos + n], [], REC_HDR_WORDS
        pos += n
        if kind & REC_KIND_MASK == REC_KIND_DROPPED:
            if not markers:
                continue
            n_plies = 0                      # (the marker's ply count is the dropped game's: it carries none of them)
        for _ in range(n_plies):
            assert q + REC_PLY_WORDS <= n, (uid, q, n)
            x_lo, x_hi, o_lo, o_hi, head, word5 = (int(w) for w in rec[q:q + REC_PLY_WORDS])
            q += REC_PLY_WORDS
            targets = rec[q:q + (head >> 16)]
            q += head >> 16
            plies.append((head & 0xFFFF, word5, {int(w) & 0xFFFF: int(w) >> 16 for w in targets},
                          (x_lo | x_hi << 32, o_lo | o_hi << 32)))
        assert q == n, (uid, q, n)
        yield Record(slot, uid, result, kind, plies, rec)


def blockers_to_cells(mask):
    """A wall mask (bit = file + 7 * rank) -> the ascending list of its cells in the game line's index x + 7 y (y = 0 at rank
    7): a line's "blockers"."""
    return [c for c in range(49) if (int(mask) >> (c % 7 + 7 * (6 - c // 7))) & 1]


def cells_to_blockers(cells):
    """A line's "blockers" -> the wall mask."""
    mask = 0
    for c in cells:
        mask |= 1 << (c % 7 + 7 * (6 - c // 7))
    return mask


def start_pool_entry(uid, n, stride=1):
    """The entry of a start pool of n entries that game `uid` starts from, (uid // stride) % n (azh_start_pool_entry; host
    arithmetic, no device)."""
    r = load().azh_start_pool_entry(int(uid), int(n), int(stride))
    if r < 0:
        check(r)
    return r


def search_set_pairing(uid, n):
    """-> (set of x, set of o) in game `uid` among n search sets (Engine.set_search_sets): uids 2q and 2q + 1 are the q-th
    unordered pair, in lexicographic order and round robin, with the colours swapped (azh_search_set_pairing; host arithmetic,
    no device)."""
    out = np.zeros(2, dtype=np.int32)
    check(load().azh_search_set_pairing(int(uid), int(n), _ptr(out)))
    return int(out[0]), int(out[1])


def playout_cap_kind(seed, uid, ply, full_per_65536):
    """Playout cap randomization: 1 if ply `ply` of game `uid` of an engine with `seed` is a FULL ply, else 0
    (azh_playout_cap_kind; host arithmetic, no GPU needed)."""
    return int(load().azh_playout_cap_kind(int(seed), int(uid), int(ply), int(full_per_65536)))


class TowerChoice(ctypes.Structure):                           # azh_tower_choice
    _fields_ = [("kernel", ctypes.c_char * 64)] + [(f, ctypes.c_int32) for f in ("boards", "threads", "lds_bytes", "per_cu")]


def tower_choice(filters, dtype, thin=False, stamped=False, pair=False, variant1=False, six_boards=False, lds_range_ok=True):
    """Which tower kernel such a launch runs (azh_net_tower_choice: the library's own dispatch; host arithmetic, no GPU
    needed): (0, {kernel, boards, threads, lds_bytes, per_cu}), (-2, None) refused, (1, None) no pair kernel here."""
    c = TowerChoice()
    rc = int(load().azh_net_tower_choice(filters, dtype, thin, stamped, pair, variant1, six_boards, lds_range_ok, ctypes.byref(c)))
    return rc, ({"kernel": c.kernel.decode(), **{f: getattr(c, f) for f in ("boards", "threads", "lds_bytes", "per_cu")}}
                if rc == 0 else None)


def forced_prune(prior, W, n, k, c_puct):
    """Policy target pruning (Engine.set_forced_playouts): the visit counts written into a ply's record for a root with
    priors `prior` (after the noise mix), total scores `W` and visits `n` — (M,) u32, 0 where the edge is left out
    (azh_forced_prune; host arithmetic, no GPU needed)."""
    prior = np.ascontiguousarray(prior, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    n = np.ascontiguousarray(n, dtype=np.uint32)
    if not len(prior) == len(W) == len(n):
        raise ValueError("prior, W and n must have one entry per root edge")
    out = np.zeros(len(n), dtype=np.uint32)
    check(load().azh_forced_prune(_ptr(prior), _ptr(W), _ptr(n), len(n), float(k), float(c_puct), _ptr(out)))
    return out


def gumbel_considered_visits(m, visits):
    """Gumbel root search (Engine.set_gumbel): the sequential-halving schedule for m considered actions and `visits`
    simulations — (visits,) u16, entry t the visit count an edge must have to be a candidate of simulation t
    (azh_gumbel_considered_visits; host arithmetic, no GPU needed)."""
    out = np.zeros(max(int(visits), 1), dtype=np.uint16)
    check(load().azh_gumbel_considered_visits(int(m), int(visits), _ptr(out)))
    return out


def gumbel_noise(seed, uid, ply, M):
    """Gumbel root search: the Gumbel(0, 1) draws g_j of the M root edges of ply `ply` of game `uid` of an engine with `seed`
    — (M,) f32 (azh_gumbel_noise; host arithmetic, no GPU needed)."""
    out = np.zeros(max(int(M), 1), dtype=np.float32)
    check(load().azh_gumbel_noise(int(seed), int(uid), int(ply), int(M), _ptr(out)))
    return out[:int(M)]


def gumbel_root(prior, W, n, v0, noise, c_visit, c_scale):
    """Gumbel root search: the ply played from a root with priors `prior`, total scores `W`, visits `n`, the root's own score
    v0 and the draws `noise` -> (edge of the move, (M,) u32 counts of the improved policy in the ply's record, 0 where the
    edge is left out) (azh_gumbel_root; host arithmetic, no GPU needed)."""
    prior = np.ascontiguousarray(prior, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    n = np.ascontiguousarray(n, dtype=np.uint32)
    noise = np.ascontiguousarray(noise, dtype=np.float32)
    if not len(prior) == len(W) == len(n) == len(noise):
        raise ValueError("prior, W, n and noise must have one entry per root edge")
    counts = np.zeros(len(n), dtype=np.uint32)
    move = ctypes.c_int32(0)
    check(load().azh_gumbel_root(_ptr(prior), _ptr(W), _ptr(n), len(n), float(v0), _ptr(noise), float(c_visit), float(c_scale),
                                 _ptr(counts), ctypes.byref(move)))
    return int(move.value), counts


def exploration_scores(prior, W, n, c_puct, fpu_reduction=-1.0, c_base=0.0, c_init=0.0):
    """First-play urgency and the exploration rate (Engine.set_exploration): the scores of one node's edges with priors
    `prior`, total scores `W` and effective visit counts `n` — (M,) f32; with (-1, 0, 0) the reference's PUCT scores
    (azh_exploration_scores; host arithmetic, no GPU needed)."""
    prior = np.ascontiguousarray(prior, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    n = np.ascontiguousarray(n, dtype=np.uint32)
    if not len(prior) == len(W) == len(n):
        raise ValueError("prior, W and n must have one entry per edge")
    out = np.zeros(max(len(n), 1), dtype=np.float32)
    check(load().azh_exploration_scores(_ptr(prior), _ptr(W), _ptr(n), len(n), float(c_puct), float(fpu_reduction), float(c_base),
                                        float(c_init), _ptr(out)))
    return out[:len(n)]


def eval_symmetry(seed, uid, mover, opponent):
    """Random symmetry per evaluation (Engine.set_random_symmetry): the symmetry 0..7 under which the position (mover,
    opponent) of game `uid` of an engine with `seed` is evaluated (azh_eval_symmetry; host arithmetic, no GPU needed)."""
    return int(load().azh_eval_symmetry(int(seed), int(uid), int(mover), int(opponent)))


def resign_playthrough(seed, uid, per_65536):
    """Resignation (Engine.set_resign): 1 if game `uid` of an engine with `seed` is a play-through game — it runs to its real
    end whatever the rule says — else 0 (azh_resign_playthrough; host arithmetic, no GPU needed)."""
    return int(load().azh_resign_playthrough(int(seed), int(uid), int(per_65536)))


def temperature_pick(visits, temperature, seed, uid, ply, weights=False):
    """Temperature of the move played (Engine.set_temperature): the root edge chosen from the visit counts `visits` (in edge
    order) at `temperature` for ply `ply` of game `uid` of an engine with `seed`; with `weights` -> (edge, the (M,) u32
    fixed-point weights the choice was made on) (azh_temperature_pick; host arithmetic, no GPU needed)."""
    visits = np.ascontiguousarray(visits, dtype=np.uint32)
    q = np.zeros(len(visits), dtype=np.uint32) if weights else None
    j = load().azh_temperature_pick(_ptr(visits), len(visits), float(temperature), int(seed), int(uid), int(ply), _ptr(q))
    if j < 0:
        check(j)
    return (int(j), q) if weights else int(j)


def symmetry_board(s, bitboard):
    """T_s on a bitboard: bit 0 of s mirrors x, bit 1 mirrors y, bit 2 then transposes (azh_symmetry_board; host arithmetic)."""
    return int(load().azh_symmetry_board(int(s), int(bitboard)))


def symmetry_move(s, move):
    """T_s on a move (u16 from | to << 8): both squares by the symmetry (azh_symmetry_move; host arithmetic)."""
    rc = int(load().azh_symmetry_move(int(s), int(move)))
    if rc < 0:
        check(rc)
    return rc


def symmetry_policy_index(s, index):
    """T_s on a flat policy index 119 x + 17 y + layer (all 833): logits of the position [i] = logits of the image
    [symmetry_policy_index(s, i)] (azh_symmetry_policy_index; host arithmetic)."""
    rc = int(load().azh_symmetry_policy_index(int(s), int(index)))
    if rc < 0:
        check(rc)
    return rc


def full_per_65536(full_fraction):
    """The setter's integer for a share of FULL plies in [0, 1]."""
    if not 0.0 <= full_fraction <= 1.0:
        raise ValueError("full_fraction must lie in [0, 1]")
    return int(round(full_fraction * 65536))


# ------------------------------------------------------------------ rules

def pack_board(x, o, turn):
    return np.array([int(x) | (int(turn) << 63), int(o)], dtype=np.uint64)


def perft(x, o, blockers, turn, depth):
    out = ctypes.c_uint64(0)
    check(load().azh_perft(int(x), int(o), int(blockers), int(turn), int(depth), ctypes.byref(out)))
    return int(out.value)


def rules_batch(boards, blockers):
    boards = np.ascontiguousarray(boards, dtype=np.uint64).reshape(-1, 2)
    n = len(boards)
    moves = np.zeros((n, MAX_MOVES), dtype=np.uint16)
    counts = np.zeros(n, dtype=np.int32)
    results = np.zeros(n, dtype=np.int32)
    check(load().azh_rules_batch(n, _ptr(boards), int(blockers), _ptr(moves), _ptr(counts), _ptr(results)))
    return moves, counts, results


def makemove_batch(boards, moves):
    boards = np.ascontiguousarray(boards, dtype=np.uint64).reshape(-1, 2)
    moves = np.ascontiguousarray(moves, dtype=np.uint16)
    out = np.zeros_like(boards)
    check(load().azh_makemove_batch(len(boards), _ptr(boards), _ptr(moves), _ptr(out)))
    return out


def features_batch(leaf_boards, blockers):
    leaf_boards = np.ascontiguousarray(leaf_boards, dtype=np.uint64).reshape(-1, 2)
    out = np.zeros((len(leaf_boards), 7, 7, 4), dtype=np.float32)
    check(load().azh_features_batch(len(leaf_boards), _ptr(leaf_boards), int(blockers), _ptr(out)))
    return out


def random_play(n_games, seed, x, o, blockers, turn, max_plies=400, trace=True):
    plies = np.zeros(n_games, dtype=np.int32)
    results = np.zeros(n_games, dtype=np.int32)
    boards = np.zeros((n_games, max_plies, 2), dtype=np.uint64) if trace else None
    moves = np.zeros((n_games, max_plies), dtype=np.uint16) if trace else None
    check(load().azh_random_play(n_games, int(seed), int(x), int(o), int(blockers), int(turn), max_plies,
                                 _ptr(plies), _ptr(results), _ptr(boards), _ptr(moves)))
    return plies, results, boards, moves


ALPHABETA_MAX_DEPTH, ALPHABETA_UNBOUNDED_DEPTH, ALPHABETA_WIN = 8, 3, 1000   # AZH_ALPHABETA_*; rule 1's 1000
AlphaBeta = collections.namedtuple("AlphaBeta", "moves values depth_done nodes")


def _wall_arguments(blockers, n):
    """blockers: one mask for every board, or one mask per board -> (the word, the per-board array or None)"""
    if np.ndim(blockers) == 0:
        return int(blockers), None
    return 0, _board_masks(blockers, n)


def alphabeta_search(boards, blockers, depth, node_budget=0, outputs=("moves", "values", "depth_done", "nodes")):
    """The depth-limited material alpha-beta search of n packed boards on the device, one wave per root
    (azh_alphabeta_search) -> AlphaBeta(moves (n,) u16 — best(p, depth), 0xFFFF for a finished root —, values (n,) i32,
    depth_done (n,) i32, nodes (n,) u64); a field left out of `outputs` is None.  blockers: one wall mask, or one per
    board.  node_budget 0: no limit (depth <= 3 only)."""
    boards = np.ascontiguousarray(boards, dtype=np.uint64).reshape(-1, 2)
    n = len(boards)
    word, masks = _wall_arguments(blockers, n)
    out = {"moves": np.zeros(n, dtype=np.uint16), "values": np.zeros(n, dtype=np.int32),
           "depth_done": np.zeros(n, dtype=np.int32), "nodes": np.zeros(n, dtype=np.uint64)}
    out = {k: (v if k in outputs else None) for k, v in out.items()}
    check(load().azh_alphabeta_search(n, _ptr(boards), word, _ptr(masks), int(depth), int(node_budget), _ptr(out["moves"]),
                                      _ptr(out["values"]), _ptr(out["depth_done"]), _ptr(out["nodes"])))
    return AlphaBeta(**out)


def alphabeta_host(x, o, blockers, turn, depth, node_budget=0):
    """The same search of one position as a plain negamax on the host, without pruning -> (move, value, depth_done, nodes)
    (azh_alphabeta_host; host arithmetic, no GPU needed)."""
    move, value, done, nodes = ctypes.c_uint16(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_uint64(0)
    check(load().azh_alphabeta_host(int(x), int(o), int(blockers), int(turn), int(depth), int(node_budget), ctypes.addressof(move),
                                    ctypes.addressof(value), ctypes.addressof(done), ctypes.addressof(nodes)))
    return int(move.value), int(value.value), int(done.value), int(nodes.value)


def teacher_thresholds(probabilities):
    """Per-ply probabilities of a random move -> azh_alphabeta_play's u32 thresholds, floor(p * 2**32)."""
    return np.array([min(int(p * 2 ** 32), 2 ** 32 - 1) for p in probabilities], dtype=np.uint32)


def alphabeta_play(n_games, seed, x, o, blockers, turn, depth, node_budget=0, thresholds=(), max_plies=400, starts=None):
    """Teacher games on the device (azh_alphabeta_play): every ply's training move is the alpha-beta search's, the move
    played a uniformly random one where the Philox draw of (seed; game, ply) falls below thresholds[ply]
    -> (plies, results, boards (n, max_plies, 2) (x, o), training moves, played moves (n, max_plies)).
    starts: None, or (packed boards (n, 2), wall masks (n,)), a start position and a wall map per game."""
    thresholds = np.ascontiguousarray(thresholds, dtype=np.uint32)
    first = masks = None
    if starts is not None:
        first = np.ascontiguousarray(starts[0], dtype=np.uint64).reshape(-1, 2)
        masks = _board_masks(starts[1], n_games)
        if len(first) != n_games:
            raise ValueError("%d start positions for %d games" % (len(first), n_games))
    plies = np.zeros(n_games, dtype=np.int32)
    results = np.zeros(n_games, dtype=np.int32)
    boards = np.zeros((n_games, max_plies, 2), dtype=np.uint64)
    training = np.zeros((n_games, max_plies), dtype=np.uint16)
    played = np.zeros((n_games, max_plies), dtype=np.uint16)
    check(load().azh_alphabeta_play(n_games, int(seed), int(x), int(o), int(blockers), int(turn), _ptr(first), _ptr(masks),
                                    int(depth), int(node_budget), _ptr(thresholds) if len(thresholds) else None,
                                    len(thresholds), max_plies, _ptr(plies), _ptr(results), _ptr(boards), _ptr(training),
                                    _ptr(played)))
    return plies, results, boards, training, played


def probe_detmath(kind, values=None, aux=None, seed=0):
    values = None if values is None else np.ascontiguousarray(values, dtype=np.float32)
    aux = None if aux is None else np.ascontiguousarray(aux, dtype=np.uint32)
    n = len(values) if kind in (0, 1) else len(aux) // (3 if kind == 2 else 4)
    out = np.zeros(4 * n if kind == 3 else n, dtype=np.uint32)
    check(load().azh_probe_detmath(kind, n, _ptr(values), _ptr(aux), int(seed), _ptr(out)))
    return out


# ------------------------------------------------------------------ network

def _board_masks(blockers, n):
    masks = np.ascontiguousarray(blockers, dtype=np.uint64).ravel()
    if masks.size != n:
        raise ValueError("%d wall masks for %d boards" % (masks.size, n))
    return masks


class Net:
    """Device-resident policy/value net (model.Network forward, model.py:38-79).
    AzhError (error -2, the message names the tower layer): a tower convolution weight, a batch-norm mean or a derived
    scale or shift is not finite — raised here, before a device is needed; or, from forward() and the engine's launches,
    a finite tower weight is infinite in the dtype asked for (the net still serves the other dtypes).  The two 1x1 heads,
    fc_w and fc_b may hold anything.
    Activations may still overflow from finite weights; infinities and NaNs then travel as IEEE arithmetic has them (ReLU
    keeps a NaN) in every tower but the default bf16 one at 128 filters (k_tower2, k_tower2_thin and k_tower2_pair in
    bf16), whose ReLU turns a NaN activation into 0: include/ataxxzero_hip.h at azh_net_forward."""

    def __init__(self, conv_weights, bn_params, bn_eps=1e-3):
        blocks = (len(conv_weights) - 5) // 2
        filters = int(conv_weights[0].shape[-1])
        if len(conv_weights) != 2 * blocks + 5 or len(bn_params) != 2 * (2 * blocks + 1):
            raise ValueError("weight lists do not match model.py's layout (2B+5 / 2(2B+1) arrays)")
        conv_flat = np.concatenate([np.asarray(a, dtype=np.float32).ravel() for a in conv_weights])
        bn_flat = np.concatenate([np.asarray(a, dtype=np.float32).ravel() for a in bn_params])
        self.blocks, self.filters = blocks, filters
        h = ctypes.c_void_p()
        check(load().azh_net_create(blocks, filters, _ptr(conv_flat), _ptr(bn_flat), bn_eps, ctypes.byref(h)))
        self.h = h

    def _forward(self, mode, leaf_boards, blockers, dtype):
        leaf_boards = np.ascontiguousarray(leaf_boards, dtype=np.uint64).reshape(-1, 2)
        n = len(leaf_boards)
        logits = np.zeros((n, 7, 7, 17), dtype=np.float32)
        values = np.zeros((n, 1), dtype=np.float32)
        masks = None if np.ndim(blockers) == 0 else _board_masks(blockers, n)
        check(load().azh_net_forward(self.h, dtype, mode, n, _ptr(leaf_boards), 0 if masks is not None else int(blockers),
                                     _ptr(masks), _ptr(logits), _ptr(values)))
        return logits, values

    def forward(self, leaf_boards, blockers, dtype=DTYPE_BF16, thin=False):
        """thin: one board per workgroup (the kernel for a handful of boards, AZH_FORWARD_THIN).  blockers: one wall
        mask for every board, or an array of one mask per board (all of them in one launch)."""
        return self._forward(FORWARD_THIN if thin else FORWARD_PLAIN, leaf_boards, blockers, dtype)

    def forward_sym(self, leaf_boards, blockers, dtype=DTYPE_BF16):
        """nn_evals.evaluate (nn_evals.py:48-62): mean over the 8 dihedral images, one tower launch."""
        return self._forward(FORWARD_SYM, leaf_boards, blockers, dtype)

    def bench(self, n, iters=20, dtype=DTYPE_BF16, thin=False):
        """Average milliseconds per tower launch over n synthetic boards."""
        ms = ctypes.c_float(0)
        check(load().azh_net_bench(self.h, dtype, FORWARD_THIN if thin else FORWARD_PLAIN, n, iters, ctypes.byref(ms)))
        return float(ms.value)

    def stamps(self, n, wgs=64):
        out = np.zeros((wgs, 4, 128), dtype=np.uint64)
        check(load().azh_net_stamps(self.h, n, wgs, _ptr(out)))
        return out

    def close(self):
        if getattr(self, "h", None):
            load().azh_net_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ engine

def run_engines(engines, net, iterations, dtype=DTYPE_BF16):
    """engine.run for several engines of one GPU, their iterations enqueued in turn (azh_engines_run)."""
    handles = (ctypes.c_void_p * len(engines))(*[e.h for e in engines])
    check(load().azh_engines_run(handles, len(engines), net.h, dtype, iterations))


class Engine:
    """Batched self-play search on the GPU (cpp/self_play_client.cpp's workers)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.G = cfg.games
        h = ctypes.c_void_p()
        check(load().azh_engine_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self.node_cap = load().azh_engine_node_cap(h)
        self.edge_cap = load().azh_engine_edge_cap(h)
        self._json = np.zeros(1 << 22, dtype=np.uint8)
        self.K = 1

    def close(self):
        if getattr(self, "h", None):
            load().azh_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def select(self):
        n = ctypes.c_int32(0)
        check(load().azh_engine_select(self.h, ctypes.byref(n)))
        return int(n.value)

    def leaves(self):
        need = np.zeros(self.G, dtype=np.int32)
        boards = np.zeros((self.G, 2), dtype=np.uint64)
        check(load().azh_engine_leaves(self.h, _ptr(need), _ptr(boards)))
        return need, boards

    def leaf_features(self, n):
        out = np.zeros((max(n, 1), 7, 7, 4), dtype=np.float32)
        games = np.zeros(max(n, 1), dtype=np.int32)
        check(load().azh_engine_leaf_features(self.h, _ptr(out), _ptr(games)))
        return out[:n], games[:n]

    def eval(self, net, dtype=DTYPE_BF16):
        check(load().azh_engine_eval(self.h, net.h, dtype))

    def set_evals(self, logits, values):
        logits = np.ascontiguousarray(logits, dtype=np.float32).reshape(self.G, POLICY_SIZE)
        values = np.ascontiguousarray(values, dtype=np.float32).reshape(self.G)
        check(load().azh_engine_set_evals(self.h, _ptr(logits), _ptr(values)))

    def backup(self):
        check(load().azh_engine_backup(self.h))

    def run(self, net, iterations, dtype=DTYPE_BF16):
        check(load().azh_engine_run(self.h, net.h, dtype, iterations))

    def run_arena(self, net_a, net_b, iterations, dtype=DTYPE_BF16):
        check(load().azh_engine_run_arena(self.h, net_a.h, net_b.h, dtype, iterations))

    def sync(self):
        check(load().azh_engine_sync(self.h))

    def set_visits(self, visits):
        check(load().azh_engine_set_visits(self.h, visits))

    def set_playout_cap(self, fast_visits, full_per_65536):
        """Playout cap randomization: FAST plies are played at `fast_visits` root visits without root noise, FULL
        plies — a share full_per_65536 / 65536, drawn per (uid, ply) — as today; game lines gain "full".  fast_visits = 0:
        off.  Between iterations only."""
        check(load().azh_engine_set_playout_cap(self.h, int(fast_visits), int(full_per_65536)))

    def set_forced_playouts(self, k):
        """Forced playouts at the root and policy target pruning in the records, on the plies whose root gets
        the Dirichlet mix: a root edge with n >= 1 visits is owed sqrt(k P N) of them, and the counts that go into the game's
        `dists` leave out the forced visits PUCT would not have spent.  k = 0: off (the default); KataGo uses 2."""
        check(load().azh_engine_set_forced_playouts(self.h, float(k)))

    def set_gumbel(self, m, c_visit=50.0, c_scale=1.0):
        """Gumbel root search with sequential halving: the root considers m actions drawn by the Gumbel-top-k
        trick, spends the ply's visits on them by sequential halving, plays the survivor, and the game's `dists` carry the
        improved policy softmax(logits + sigma(completedQ)) over ALL root moves.  m = 0: off (the default); mctx uses 16, 50, 1.
        Needs an engine created with FLAG_NO_REUSE and dirichlet_weight 0.  Between iterations only."""
        check(load().azh_engine_set_gumbel(self.h, int(m), float(c_visit), float(c_scale)))

    def set_random_symmetry(self, on=True):
        """Random symmetry per evaluation: every position goes to the evaluator as its image under a symmetry
        drawn per (seed, uid, position) — link.eval_symmetry — and its logits come back through that symmetry's move map;
        leaves() / batch_leaves() / leaf_features() return the image.  No tower work is added.  Between iterations only."""
        check(load().azh_engine_set_random_symmetry(self.h, 1 if on else 0))

    def set_resign(self, q_below, consecutive, playthrough_per_65536):
        """The search's value in the game records, and resignation: every ply's record carries q = W_b / n_b of
        the most visited root edge (game lines gain "values"), and a game whose mover had `consecutive` counted plies in a row
        with q < q_below ends there, result = 3 - mover (the line gains "resigned") — unless it is a play-through game, a share
        playthrough_per_65536 / 65536 drawn per uid (link.resign_playthrough).  consecutive = 0: off; q_below = 0 records
        values and never resigns.  Between iterations only."""
        check(load().azh_engine_set_resign(self.h, float(q_below), int(consecutive), int(playthrough_per_65536)))

    def set_temperature(self, move_temperature=None, root_policy_temperature=None):
        """Per-ply temperature of the move played and of the root policy: two tables of max_plies floats, or None
        (off).  move_temperature[p] = 1 plays ply p in proportion to the visits, 0 the most visited move, T in [1/64, 64] in
        proportion to visits^(1/T) (link.temperature_pick restates the choice); the recorded `dists` stay the search's.
        root_policy_temperature[p] = R in [1/4, 64] divides the root's logits by R on the plies that get noise.
        selfplay.temperature_table makes the tables.  Between iterations only."""
        def table(t, name):
            if t is None:
                return None
            t = np.ascontiguousarray(t, dtype=np.float32)
            if t.shape != (self.cfg.max_plies,):
                raise ValueError("%s must have max_plies = %d entries" % (name, self.cfg.max_plies))
            return t
        mt = table(move_temperature, "move_temperature")
        rt = table(root_policy_temperature, "root_policy_temperature")
        check(load().azh_engine_set_temperature(self.h, _ptr(mt), _ptr(rt)))

    def resign_stats(self):
        """-> {"resigned", "playthrough", "playthrough_fired", "playthrough_false"}: games resigned; play-through games
        finished; those in which the rule fired; of those, the ones the side it fired for did not lose."""
        out = np.zeros(4, dtype=np.uint64)
        check(load().azh_engine_resign_stats(self.h, _ptr(out)))
        return {"resigned": int(out[0]), "playthrough": int(out[1]), "playthrough_fired": int(out[2]),
                "playthrough_false": int(out[3])}

    def set_thin_batches(self, mode):
        """0: the 3-board tower; 1: one board per workgroup (a handful of leaves per iteration); -1: by the engine's size."""
        check(load().azh_engine_set_thin_batches(self.h, int(mode)))

    def set_leaf_batch(self, leaves_per_game, virtual_loss=1):
        """Leaf-parallel search: up to K leaves per game and iteration, spread by a virtual loss ("Leaf-parallel
        search").  Between iterations only; K = 1 is the one-leaf search."""
        check(load().azh_engine_set_leaf_batch(self.h, int(leaves_per_game), int(virtual_loss)))
        self.K = int(leaves_per_game)

    def set_solver(self, on=True):
        """Proven wins and losses in the tree ("Proven wins and losses").  While it is on every K, 1 included,
        runs through the leaf-parallel kernel (batch_leaves / set_batch_evals).  Between iterations only."""
        check(load().azh_engine_set_solver(self.h, 1 if on else 0))

    def set_exploration(self, fpu_reduction=-1.0, c_base=0.0, c_init=0.0):
        """First-play urgency (fpu_reduction >= 0: an unvisited child's Q is its parent's mean score less fpu_reduction *
        sqrt(visited policy mass), not 0) and the exploration rate that grows with log N (c_base > 0: c = log((1 + N + c_base)
        / c_base) + c_init, not c_puct) — DESIGN.md, "First-play urgency and the exploration rate".  While either is on every
        K, 1 included, runs through the leaf-parallel kernel (batch_leaves / set_batch_evals).  The defaults switch both off.
        Between iterations only."""
        check(load().azh_engine_set_exploration(self.h, float(fpu_reduction), float(c_base), float(c_init)))

    def exploration(self):
        """-> (fpu_reduction, c_base, c_init) in force: (-1, 0, 0) while the mode is off."""
        out = np.zeros(3, dtype=np.float32)
        check(load().azh_engine_exploration(self.h, _ptr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def set_search_sets(self, sets):
        """Search settings per side ("Search settings per side"): `sets` is a list of up to 16 dicts with the keys
        of SearchSet (visits, leaves, virtual_loss, c_puct, fpu_reduction, c_base, c_init) or tuples in that order.  In game
        uid x and o search with the sets link.search_set_pairing(uid, n) names, every ply with the set of the side to move at
        its root, and the device tallies the results (search_set_stats).  While it is on every K, 1 included, runs through
        the leaf-parallel kernel (batch_leaves / set_batch_evals).  An empty list: off.  Between iterations only."""
        rows = (SearchSet * max(len(sets), 1))()
        for i, t in enumerate(sets):
            rows[i] = SearchSet(**t) if isinstance(t, dict) else SearchSet(*t)
        check(load().azh_engine_set_search_sets(self.h, len(sets), ctypes.cast(rows, ctypes.c_void_p)))

    def search_sets(self):
        """-> the sets in force, a list of dicts (empty while the mode is off)."""
        n = ctypes.c_int32(0)
        rows = (SearchSet * SEARCH_SETS_MAX)()
        check(load().azh_engine_search_sets(self.h, ctypes.byref(n), ctypes.cast(rows, ctypes.c_void_p)))
        return [rows[i].as_dict() for i in range(n.value)]

    def search_set_stats(self):
        """-> (n, n, 4) uint64, indexed [set of x][set of o][SET_STAT_GAMES / _X_WINS / _O_WINS / _UNDECIDED]: the games that
        ended since set_search_sets, counted on the device."""
        n = len(self.search_sets())
        out = np.zeros((n, n, SET_STAT_COUNT), dtype=np.uint64)
        check(load().azh_engine_search_set_stats(self.h, _ptr(out)))
        return out

    def proof_stats(self):
        """-> {"proven_nodes", "proven_hits"}: nodes the proof pass proved; paths that ended at a proven node."""
        out = np.zeros(2, dtype=np.uint64)
        check(load().azh_engine_proof_stats(self.h, _ptr(out)))
        return {"proven_nodes": int(out[0]), "proven_hits": int(out[1])}

    def root_proofs(self, first=0, n=None):
        """-> [(root value, child values (M,) int32 in root edge order)] for the slots first .. first + n - 1: 0 not decided,
        +1 / -1 the side to move at that node wins / loses (azh_engine_root_proofs)."""
        n = self.G - first if n is None else n
        out = np.zeros((max(n, 1), ROOT_PROOF_WORDS), dtype=np.int32)
        check(load().azh_engine_root_proofs(self.h, int(first), int(n), _ptr(out)))
        return [(int(out[i, 0]), out[i, 1:].copy()) for i in range(n)]

    def batch_leaves(self):
        """-> kind (G, K) int32, leaf boards (G, K, 2) u64 (mover, opponent), leaf edge (G, K) u32 of the current batch."""
        kind = np.zeros((self.G, self.K), dtype=np.int32)
        boards = np.zeros((self.G, self.K, 2), dtype=np.uint64)
        edge = np.zeros((self.G, self.K), dtype=np.uint32)
        check(load().azh_engine_batch_leaves(self.h, _ptr(kind), _ptr(boards), _ptr(edge)))
        return kind, boards, edge

    def set_batch_evals(self, logits, values):
        """Evaluations of the batch by slot: logits (G K, 833), values (G K,)."""
        logits = np.ascontiguousarray(logits, dtype=np.float32).reshape(self.G * self.K, POLICY_SIZE)
        values = np.ascontiguousarray(values, dtype=np.float32).reshape(self.G * self.K)
        check(load().azh_engine_set_batch_evals(self.h, _ptr(logits), _ptr(values)))

    def collisions(self):
        """Paths of the leaf-parallel search that ended at a node created earlier in their batch (AZH_STAT_COLLISIONS)."""
        out = np.zeros(STAT_COUNT, dtype=np.uint64)
        check(load().azh_engine_stats(self.h, _ptr(out)))
        return int(out[STAT_COLLISIONS])

    def set_positions(self, boards, plies):
        """Every slot restarts at boards[g] (packed x | turn << 63, o) / plies[g] with a fresh tree (counted, not written)."""
        boards = np.ascontiguousarray(boards, dtype=np.uint64).reshape(self.G, 2)
        plies = np.ascontiguousarray(plies, dtype=np.int32).reshape(self.G)
        check(load().azh_engine_set_positions(self.h, _ptr(boards), _ptr(plies)))

    def set_start_pool(self, starts, stride=1):
        """A start position and wall map per game: game uid starts from entry (uid // stride) % n of `starts` — FEN strings,
        or (x, o, blockers, turn) tuples of bitboards — and is played on its walls (azh_engine_set_start_pool; before the
        first select).  stride 2: a two-net match, whose slots 2k and 2k + 1 share a map.  An empty list takes the pool away."""
        from . import selfplay
        rows = [selfplay.parse_fen(e) if isinstance(e, str) else tuple(int(v) for v in e) for e in starts]
        x, o, bl = (np.array([r[i] for r in rows], dtype=np.uint64) for i in range(3))
        turn = np.array([r[3] for r in rows], dtype=np.int32)
        check(load().azh_engine_set_start_pool(self.h, len(rows), _ptr(x), _ptr(o), _ptr(bl), _ptr(turn), int(stride)))

    def uid_blockers(self, uid):
        """The walls game `uid` is played on: its pool entry's, or the engine's mask (azh_engine_uid_blockers)."""
        out = ctypes.c_uint64(0)
        check(load().azh_engine_uid_blockers(self.h, int(uid), ctypes.byref(out)))
        return int(out.value)

    def record_blockers(self, words):
        """One wall mask per record of `words` (staged_records; markers included): what SampleStore.add_records takes as
        `blockers` for the records of an engine with a start pool."""
        return np.array([self.uid_blockers(r.uid) for r in records(words, markers=True)], dtype=np.uint64)

    def set_emit_order(self, by_uid):
        """True: finished games are handed out in uid order (unbiased prefixes); False: as they finish."""
        check(load().azh_engine_set_emit_order(self.h, 1 if by_uid else 0))

    def set_record_blockers(self, on=True):
        """Every line drain_json writes gains "blockers", the engine's mask as the wall cells in the index of the line's
        boards (azh_engine_set_record_blockers)."""
        check(load().azh_engine_set_record_blockers(self.h, 1 if on else 0))

    def set_game_limit(self, games):
        """Play uids 0 .. games - 1 only; slots past the limit go idle (call before the first iteration)."""
        check(load().azh_engine_set_game_limit(self.h, int(games)))

    def play_moves(self, moves):
        """The host names the move of every slot (u16 from | to << 8; NO_MOVE leaves the slot alone): the root edge's child
        becomes the root with its subtree (PLAY_KEPT), or a fresh one-node tree is started (PLAY_FRESH).  -> status (G,)
        int32 of PLAY_* (azh_engine_play_moves)."""
        moves = np.ascontiguousarray(moves, dtype=np.uint16).reshape(self.G)
        status = np.zeros(self.G, dtype=np.int32)
        check(load().azh_engine_play_moves(self.h, _ptr(moves), _ptr(status)))
        return status

    def root_report(self, first=0, n=None):
        """-> [RootReport] for the slots first .. first + n - 1 (all from `first` on by default): root edges and principal
        variation, a few KB per slot instead of the whole tree (azh_engine_root_report)."""
        n = self.G - first if n is None else n
        out = np.zeros((max(n, 1), ROOT_REPORT_WORDS), dtype=np.uint32)
        check(load().azh_engine_root_report(self.h, int(first), int(n), _ptr(out)))
        return [RootReport(out[i]) for i in range(n)]

    def root_report_device(self, out, first=0, n=None):
        """The same records written into `out`, a contiguous int32 GPU tensor with room for n rows of ROOT_REPORT_WORDS (uint32
        words; torch has no such dtype), by the same kernel: nothing is copied to the host, and the call returns when the
        kernel has completed (azh_engine_root_report_device).  What SampleStore.retarget reads."""
        import torch
        n = self.G - first if n is None else n
        if not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= n * ROOT_REPORT_WORDS):
            raise ValueError("out must be a contiguous int32 GPU tensor of at least n * ROOT_REPORT_WORDS words")
        check(load().azh_engine_root_report_device(self.h, int(first), int(n), ctypes.c_void_p(out.data_ptr())))
        return out

    def game_state(self, g):
        s = GameState()
        check(load().azh_engine_game_state(self.h, g, ctypes.byref(s)))
        return s

    def tree(self, g):
        s = self.game_state(g)
        boards = np.zeros((s.n_nodes, 2), dtype=np.uint64)
        info = np.zeros((s.n_nodes, 4), dtype=np.uint32)
        edges = np.zeros((s.n_edges, 4), dtype=np.uint32)
        moves = np.zeros(s.n_edges, dtype=np.uint16)
        check(load().azh_engine_tree(self.h, g, _ptr(boards), _ptr(info), _ptr(edges), _ptr(moves)))
        return boards, info, edges, moves

    def tree_raw(self, g):
        """The game's edges as the 16-byte device records (prior bits with the descent's mark in bit 31, score bits,
        visits | child << 16, the child's edge range): diagnostic, azh_engine_tree_raw."""
        edges = np.zeros((self.game_state(g).n_edges, 4), dtype=np.uint32)
        check(load().azh_engine_tree_raw(self.h, g, _ptr(edges)))
        return edges

    def stats(self):
        out = np.zeros(STAT_COUNT, dtype=np.uint64)
        check(load().azh_engine_stats(self.h, _ptr(out)))
        return {n: int(out[i]) for i, n in enumerate(STAT_NAMES)}

    def tree_stamps(self, net, dtype=DTYPE_BF16):
        """(G, 10): 8 s_memrealtime readings (100 MHz) of one stamped tree launch of the device loop (two iterations are
        run), then the levels descended and the children scanned."""
        out = np.zeros((self.G, 10), dtype=np.uint64)
        check(load().azh_engine_tree_stamps(self.h, net.h, dtype, _ptr(out)))
        return out

    def timing_reset(self, enable=True):
        """False / 0: off; True / 1: every iteration of the device loop is event-timed; n: every n-th."""
        check(load().azh_engine_timing_reset(self.h, int(enable)))

    def timing(self):
        t = Timing()
        check(load().azh_engine_timing(self.h, ctypes.byref(t)))
        return {"select_ms": t.select_ms, "net_ms": t.net_ms, "backup_ms": t.backup_ms, "iterations": t.iterations}

    def fetch(self):
        """Wait for the work enqueued so far and take its finished games off the device; the next drain_json formats
        them without touching the GPU (so the next run can be enqueued in between)."""
        check(load().azh_engine_fetch(self.h))

    def busy(self):
        """True while work enqueued on this engine's streams is still in flight (a query: never waits)."""
        rc = load().azh_engine_query(self.h)
        if rc < 0:
            check(rc)
        return rc == 1

    def implicit_fetches(self):
        """Times a drain had to fetch by itself (= waited for the device); 0 in a loop that fetches before it drains."""
        return int(load().azh_engine_implicit_fetches(self.h))

    def staged_records(self):
        """Diagnostic: the record words fetch() took off the device and drain_json() has not yet formatted (uint32, the
        ring's layout: include/ataxxzero_hip.h, azh_format_record_json); nothing is consumed."""
        n = ctypes.c_int64(0)
        rc = load().azh_engine_staged_records(self.h, None, 0, ctypes.byref(n))
        if rc not in (0, -6):
            check(rc)
        out = np.zeros(max(int(n.value), 1), dtype=np.uint32)
        check(load().azh_engine_staged_records(self.h, _ptr(out), out.size, ctypes.byref(n)))
        return out[:int(n.value)]

    def drain_json(self):
        """Finished games since the last call, as a list of JSON lines (bytes, no newline)."""
        lines = []
        while True:
            used = ctypes.c_int64(0)
            n = ctypes.c_int32(0)
            rc = load().azh_engine_drain_json(self.h, _ptr(self._json), self._json.nbytes, ctypes.byref(used),
                                              ctypes.byref(n))
            if rc == -6:
                self._json = np.zeros(self._json.nbytes * 2, dtype=np.uint8)
                continue
            check(rc)
            if n.value == 0:
                break
            lines.extend(bytes(self._json[:used.value]).split(b"\n")[:-1])
        return lines


# ------------------------------------------------------------------ device-resident training samples

class CSampleArrays(ctypes.Structure):                        # azh_sample_arrays
    _fields_ = [(n, ctypes.c_int64) for n in ("n_games", "n_plies", "n_targets")] + \
               [(n, _vp) for n in ("games", "boards", "ply_flags", "values", "target_start", "target_index", "target_weight",
                                   "game_blockers", "game_owners")]


class CSampleOutputs(ctypes.Structure):                       # azh_sample_outputs
    _fields_ = [(n, _vp) for n in ("features", "policy", "value", "ownership", "score", "reply", "aux_weight")]


class _OptionalOwners:
    __slots__ = ("owners",)                                   # kept apart: SampleArrays.__slots__ names the arrays every game has


class SampleArrays(_OptionalOwners):
    """Games as azh_samples_add_games takes them: games (G, 4) u32 {first ply, plies, result | SAMPLES_GAME_*, random_ply + 1},
    boards (P, 2) u64, ply_flags (P,) u8, values (P,) f64, target_start (P + 1,) i32, target_index (T,) u16, target_weight
    (T,) f32; blockers (G,) u64, every game's wall mask (bit = file + 7 * rank; default: none has walls); owners: None, or
    (G, 2) u64, the cells x and o own at each game's end, both 0 for a game whose final position is not terminal
    (include/ataxxzero_hip.h, "Auxiliary targets")."""
    __slots__ = ("games", "boards", "ply_flags", "values", "target_start", "target_index", "target_weight", "blockers")

    def __init__(self, games, boards, ply_flags, values, target_start, target_index, target_weight, blockers=None,
                 owners=None):
        self.games = np.ascontiguousarray(games, dtype=np.uint32).reshape(-1, 4)
        self.boards = np.ascontiguousarray(boards, dtype=np.uint64).reshape(-1, 2)
        self.ply_flags = np.ascontiguousarray(ply_flags, dtype=np.uint8)
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.target_start = np.ascontiguousarray(target_start, dtype=np.int32)
        self.target_index = np.ascontiguousarray(target_index, dtype=np.uint16)
        self.target_weight = np.ascontiguousarray(target_weight, dtype=np.float32)
        self.blockers = (np.zeros(len(self.games), dtype=np.uint64) if blockers is None
                         else np.ascontiguousarray(blockers, dtype=np.uint64))
        if len(self.blockers) != len(self.games):
            raise ValueError("one blockers mask per game")
        self.owners = None if owners is None else np.ascontiguousarray(owners, dtype=np.uint64).reshape(-1, 2)
        if self.owners is not None and len(self.owners) != len(self.games):
            raise ValueError("two owner masks per game")

    def c_arrays(self):
        """-> the azh_sample_arrays of these arrays, the counts their lengths.  It points into them: keep them alive."""
        return CSampleArrays(len(self.games), len(self.ply_flags), len(self.target_index),
                             *[None if a is None else a.ctypes.data for a in (
                                 self.games, self.boards, self.ply_flags, self.values, self.target_start, self.target_index,
                                 self.target_weight, self.blockers, self.owners)])


# bit x + 7 (6 - y) of a bitboard is the cell the game line's boards[ply][x + 7 y] names
_CELL_BIT = np.array([1 << (c % 7 + 7 * (6 - c // 7)) for c in range(49)], dtype=np.uint64)
MOVE_PASS = 0xFFFF           # the ring record's move word of a pass


def samples_final_owners(x, o, blockers, o_to_move, move):
    """The ring record's 16-bit `move` (from | to << 8, a clone from == to, MOVE_PASS) played by x (o: o_to_move) on the
    bitboards x, o with walls `blockers` -> (x-owned mask, o-owned mask, result) of the position reached: 0, 0, 0 when it is not
    terminal.  AzhError (-2) for a move that is not legal there (azh_samples_final_owners; host arithmetic, no GPU needed)."""
    owners, result = np.zeros(2, dtype=np.uint64), ctypes.c_int32(0)
    check(load().azh_samples_final_owners(int(x), int(o), int(blockers), int(bool(o_to_move)), int(move), _ptr(owners),
                                          ctypes.byref(result)))
    return int(owners[0]), int(owners[1]), int(result.value)


def entry_move_word(mv):
    """A game line's move — UAI text, "pass", or the reference's nested lists ["c", [x, y]] / [[x0, y0], [x1, y1]] — as the
    ring record's 16-bit move word."""
    if mv == "pass":
        return MOVE_PASS
    if isinstance(mv, str):
        from .uai import text_to_xy_move
        mv = text_to_xy_move(mv)
        if mv == "pass":
            return MOVE_PASS
    to = int(mv[1][0]) + 7 * (6 - int(mv[1][1]))
    frm = to if mv[0] == "c" else int(mv[0][0]) + 7 * (6 - int(mv[0][1]))
    return frm | to << 8


def entry_owners(entry):
    """(x-owned, o-owned) of a parsed game line: samples_final_owners of its last board, the side to move there (x on even
    plies), its "blockers" and the last move.  AzhError (-2) where a store would refuse them (azh_samples_check_owners)."""
    n = len(entry["boards"])
    cells = np.asarray(entry["boards"][n - 1], dtype=np.int8)
    x, o = (int(((cells == v) * _CELL_BIT).sum(dtype=np.uint64)) for v in (1, 2))
    walls = cells_to_blockers(entry.get("blockers", ()))
    own_x, own_o, _ = samples_final_owners(x, o, walls, (n - 1) % 2, entry_move_word(entry["moves"][n - 1]))
    # the store's own check (a margin that contradicts the recorded result among it): the host pipeline, which never fills a
    # store, refuses the games a store refuses
    check(load().azh_samples_check_owners(own_x, own_o, walls, int(entry["result"]) & 0xFFFFFFFF))
    return own_x, own_o


def entries_to_arrays(entries, aux=False):
    """Parsed game lines -> SampleArrays, with the conversions of training._entry_arrays (weights np.float32 of the parsed
    double, "pass" keys skipped, an entry without `dists` a one-hot on the move played), in the order given; an entry's
    "blockers" becomes its game's mask, after training.check_blockers (ValueError).  aux: with `owners`, every game's
    found by entry_owners (AzhError for a game whose last move is not legal at its last board).  Host only."""
    from . import training
    owners = [entry_owners(e) for e in entries] if aux else None
    games, boards, flags, values, starts, index, weight = [], [], [], [], [np.zeros(1, dtype=np.int32)], [], []
    masks = []
    plies = targets = 0
    for number, entry in enumerate(entries):
        training.check_blockers(entry, "entry %d" % number)
        masks.append(cells_to_blockers(entry.get("blockers", ())))
        cells, idx, wts, start = training._entry_arrays(entry)
        n = len(entry["boards"])
        if n < 1 or cells.shape != (n, 49) or cells.min() < 0 or cells.max() > 2:
            raise ValueError("an entry needs at least one ply and boards of 49 cells in 0..2")
        word = int(entry["result"])
        f = np.array([SAMPLES_PLY_PASS if m == "pass" else 0 for m in entry["moves"][:n]], dtype=np.uint8)
        if "full" in entry:
            word |= SAMPLES_GAME_HAS_FULL
            f |= np.where(np.asarray(entry["full"][:n], dtype=bool), SAMPLES_PLY_FULL, 0).astype(np.uint8)
        if "values" in entry:
            word |= SAMPLES_GAME_HAS_VALUES
            values.append(np.asarray(entry["values"][:n], dtype=np.float64))
        else:
            values.append(np.zeros(n, dtype=np.float64))
        games.append((plies, n, word, entry["random_ply"] + 1 if "random_ply" in entry else 0))
        boards.append(np.stack([((cells == 1) * _CELL_BIT).sum(axis=1, dtype=np.uint64),
                                ((cells == 2) * _CELL_BIT).sum(axis=1, dtype=np.uint64)], axis=1))
        flags.append(f)
        starts.append(start[1:] + targets)
        index.append(idx.astype(np.uint16))
        weight.append(wts)
        plies += n
        targets += int(start[-1])

    def cat(parts, dtype):
        return np.concatenate(parts).astype(dtype, copy=False) if parts else np.zeros(0, dtype=dtype)
    return SampleArrays(np.array(games, dtype=np.uint32).reshape(-1, 4), cat(boards, np.uint64).reshape(-1, 2),
                        cat(flags, np.uint8), cat(values, np.float64), cat(starts, np.int32), cat(index, np.uint16),
                        cat(weight, np.float32), np.array(masks, dtype=np.uint64),
                        owners=np.array(owners, dtype=np.uint64).reshape(-1, 2) if aux else None)


def _record_walls(blockers):
    """blockers as the records calls take the walls: -> (the scalar mask, the array of one mask per record or None)."""
    if np.ndim(blockers) == 0:
        return int(blockers), None
    return 0, np.ascontiguousarray(blockers, dtype=np.uint64).ravel()


def pack_records(records, blockers=0, aux=False):
    """Ring records (Engine.staged_records) -> SampleArrays holding what parsing the games' own lines would give; blockers:
    the wall mask of the engine that wrote them, which a line written with "blockers" carries — or, for an engine with a
    start pool, an array of one mask per record (Engine.record_blockers).  aux: with `owners`, every game's from its last
    ply's boards and move word (AzhError -2 for a last move that is not legal there).  (azh_samples_pack_records; host code,
    no GPU needed.)"""
    rec = np.ascontiguousarray(records, dtype=np.uint32).ravel()
    mask, masks = _record_walls(blockers)

    def call(c):
        check(load().azh_samples_pack_records(_ptr(rec), rec.size, mask, _ptr(masks), 0 if masks is None else masks.size,
                                              int(bool(aux)), ctypes.byref(c)))
        return c.n_games, c.n_plies, c.n_targets
    g, p, t = call(CSampleArrays())                            # no arrays: the counts only
    a = SampleArrays(np.zeros((max(g, 1), 4), np.uint32), np.zeros((p, 2), np.uint64), np.zeros(p, np.uint8), np.zeros(p),
                     np.zeros(p + 1, np.int32), np.zeros(max(t, 1), np.uint16), np.zeros(max(t, 1), np.float32),
                     owners=np.zeros((max(g, 1), 2), np.uint64) if aux else None)   # (a null `games` asks for the counts)
    call(a.c_arrays())
    a.games, a.blockers, a.owners = a.games[:g], a.blockers[:g], a.owners[:g] if aux else None
    a.target_index, a.target_weight = a.target_index[:t], a.target_weight[:t]
    return a


def samples_draw(seed, step, sample, first_game, n_games, games, ply_flags, candidates=None, cum=None):
    """One sample's draw of SampleStore.draw_gather restated on the host from mirror arrays -> (game, ply, symmetry, attempts
    used), (-1, -1, -1, 64) when all 64 attempts fail; with candidates and cum (SampleStore.ply_cum) the weighted ply choice
    (azh_samples_draw; host arithmetic, no GPU needed)."""
    games = np.ascontiguousarray(games, dtype=np.uint32).reshape(-1, 4)
    ply_flags = np.ascontiguousarray(ply_flags, dtype=np.uint8)
    candidates = None if candidates is None else np.ascontiguousarray(candidates, dtype=np.uint16)
    cum = None if cum is None else np.ascontiguousarray(cum, dtype=np.uint32)
    if any(a is not None and len(a) != len(ply_flags) for a in (candidates, cum)):
        raise ValueError("candidates and cum hold one entry per ply")
    out = np.zeros(4, dtype=np.int32)
    check(load().azh_samples_draw(int(seed), int(step), int(sample), int(first_game), int(n_games), _ptr(games), len(games),
                                  _ptr(ply_flags), _ptr(candidates), _ptr(cum), _ptr(out)))
    return tuple(int(v) for v in out)


def samples_draw_weighted(seed, step, sample, first_game, n_games, games, ply_flags, candidates, cum):
    """samples_draw with the weighted ply choice, from the mirrors SampleStore.mirror and SampleStore.ply_cum return."""
    return samples_draw(seed, step, sample, first_game, n_games, games, ply_flags, candidates, cum)


def samples_legal(mover, opponent, blockers=0):
    """The legal moves of a position (the mover's and the opponent's stones and the walls as bitboards) as flat policy indices
    in the device movegen's order -> u16 array (azh_samples_legal; host arithmetic)."""
    index, n = np.zeros(833, dtype=np.uint16), ctypes.c_int32(0)
    check(load().azh_samples_legal(int(mover), int(opponent), int(blockers), _ptr(index), ctypes.byref(n)))
    return index[:n.value].copy()


def samples_surprise_host_blockers(logits, mover, opponent, blockers, target_index, target_weight):
    """samples_surprise_host with the legal moves found from the position and its walls
    (azh_samples_surprise_host_blockers; host arithmetic)."""
    logits = np.ascontiguousarray(logits, dtype=np.float32).ravel()
    if logits.size != 833:
        raise ValueError("833 logits")
    target_index = np.ascontiguousarray(target_index, dtype=np.uint16)
    target_weight = np.ascontiguousarray(target_weight, dtype=np.float32)
    if len(target_index) != len(target_weight):
        raise ValueError("one weight per target")
    kl, illegal = ctypes.c_float(0.0), ctypes.c_int32(0)
    check(load().azh_samples_surprise_host_blockers(_ptr(logits), int(mover), int(opponent), int(blockers),
                                                    _ptr(target_index) if len(target_index) else None,
                                                    _ptr(target_weight) if len(target_weight) else None, len(target_index),
                                                    ctypes.byref(kl), ctypes.byref(illegal)))
    return np.float32(kl.value), int(illegal.value)


def samples_surprise_host(logits, legal_index, target_index, target_weight):
    """One ply's policy surprise KL(target || softmax of the logits over the legal moves) as the store's kernel computes and
    stores it -> (f32 KL, targets with a positive weight that are not legal) (azh_samples_surprise_host; host arithmetic)."""
    logits = np.ascontiguousarray(logits, dtype=np.float32).ravel()
    if logits.size != 833:
        raise ValueError("833 logits")
    legal_index = np.ascontiguousarray(legal_index, dtype=np.uint16)
    target_index = np.ascontiguousarray(target_index, dtype=np.uint16)
    target_weight = np.ascontiguousarray(target_weight, dtype=np.float32)
    if len(target_index) != len(target_weight):
        raise ValueError("one weight per target")
    kl, illegal = ctypes.c_float(0.0), ctypes.c_int32(0)
    check(load().azh_samples_surprise_host(_ptr(logits), _ptr(legal_index) if len(legal_index) else None, len(legal_index),
                                           _ptr(target_index) if len(target_index) else None,
                                           _ptr(target_weight) if len(target_weight) else None, len(target_index),
                                           ctypes.byref(kl), ctypes.byref(illegal)))
    return np.float32(kl.value), int(illegal.value)


def retarget_host(report):
    """One root report record (ROOT_REPORT_WORDS uint32) -> (index (n,) u16, weight (n,) f32, value): the policy target and
    the value a reanalysed ply takes from it, n == 0 (value 0.0) for a record that leaves its ply as it was; AzhError (-2) for
    a malformed record (azh_samples_retarget_host; host arithmetic, no GPU needed)."""
    report = np.ascontiguousarray(report, dtype=np.uint32).ravel()
    if report.size != ROOT_REPORT_WORDS:
        raise ValueError("a record has %d words" % ROOT_REPORT_WORDS)
    index, weight = np.zeros(MAX_MOVES, dtype=np.uint16), np.zeros(MAX_MOVES, dtype=np.float32)
    n, value = ctypes.c_int32(0), ctypes.c_double(0.0)
    check(load().azh_samples_retarget_host(_ptr(report), _ptr(index), _ptr(weight), ctypes.byref(n), ctypes.byref(value)))
    return index[:n.value].copy(), weight[:n.value].copy(), float(value.value)


def value_returns_host(values, proofs, result, lam):
    """The lambda-returns G_p of one game (include/ataxxzero_hip.h, "lambda-returns as value targets") -> (T,) f64: values
    (T,) the search's value of every ply, proofs (T,) its proof words or None, result the game's (0 .. 2), lam in [0, 1]
    (azh_samples_value_returns_host; host arithmetic, no GPU needed)."""
    values = np.ascontiguousarray(values, dtype=np.float64).ravel()
    proofs = None if proofs is None else np.ascontiguousarray(proofs, dtype=np.int32).ravel()
    if proofs is not None and len(proofs) != len(values):
        raise ValueError("one proof word per ply")
    out = np.zeros(max(len(values), 1), dtype=np.float64)
    check(load().azh_samples_value_returns_host(_ptr(values) if len(values) else None, _ptr(proofs), len(values), int(result),
                                                float(lam), _ptr(out)))
    return out[:len(values)]


def hip_runtimes():
    """The HIP runtime libraries mapped into this process (paths).  torch ships its own: imported BEFORE this package's
    library is loaded, both resolve to that one copy (same soname) and share streams and memory; loaded after it, the
    process holds two runtimes that know nothing of each other's handles."""
    with open("/proc/self/maps") as f:
        return sorted({line.split()[-1] for line in f if "libamdhip64" in line})


_shared_runtime = None


def require_torch_runtime():
    """Raises unless torch and this library run on ONE HIP runtime: a SampleStore enqueues on torch's streams and writes
    torch's tensors."""
    global _shared_runtime
    if _shared_runtime is None:
        import torch  # noqa: F401  (its runtime is mapped by the import)
        load()
        _shared_runtime = hip_runtimes()
    if len(_shared_runtime) != 1:
        raise AzhError("torch and libataxxzero_hip.so hold separate HIP runtimes in this process (%s): import torch before "
                       "anything loads the library (train.py does), or use a fresh process" % ", ".join(_shared_runtime))


class SampleStore:
    """Finished games in device memory and the kernel that writes minibatches from them ("Device-resident
    samples").  Outputs are torch tensors on the GPU: features (n, 7, 7, 4), policy (n, 7, 7, 17), value (n, 1), f32.
    The process must hold one HIP runtime (require_torch_runtime)."""

    def __init__(self, cap_games, cap_plies, cap_targets):
        require_torch_runtime()
        h = ctypes.c_void_p()
        check(load().azh_samples_create(int(cap_games), int(cap_plies), int(cap_targets), ctypes.byref(h)))
        self.h = h
        self._mirror = None

    def close(self):
        if getattr(self, "h", None):
            load().azh_samples_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_arrays(self, a):
        """The games of a SampleArrays, with their owners when it has them (azh_samples_add_games)."""
        self._mirror = None
        check(load().azh_samples_add_games(self.h, ctypes.byref(a.c_arrays())))

    def add_entries(self, entries, aux=False):
        """Parsed game lines, in the order given (entries_to_arrays)."""
        self.add_arrays(entries_to_arrays(entries, aux=aux))

    def add_records(self, records, blockers=0, aux=False):
        """Ring records as Engine.staged_records returns them, and the wall mask of the engine that wrote them — or, for an
        engine with a start pool, an array of one mask per record (Engine.record_blockers); aux: with every game's owners
        (azh_samples_add_records)."""
        rec = np.ascontiguousarray(records, dtype=np.uint32).ravel()
        mask, masks = _record_walls(blockers)
        self._mirror = None
        check(load().azh_samples_add_records(self.h, _ptr(rec), rec.size, mask, _ptr(masks),
                                             0 if masks is None else masks.size, int(bool(aux))))

    def game_owners(self):
        """-> (G, 2) u64: the cells x and o own at every stored game's end, 0 and 0 for a game without owners
        (azh_samples_game_owners)."""
        n = self.counts()["games"]
        owners = np.zeros((max(n, 1), 2), np.uint64)
        check(load().azh_samples_game_owners(self.h, _ptr(owners)))
        return owners[:n]

    def game_blockers(self):
        """-> (G,) u64: every stored game's wall mask, 0 for a game without walls (azh_samples_game_blockers)."""
        n = self.counts()["games"]
        masks = np.zeros(max(n, 1), np.uint64)
        check(load().azh_samples_game_blockers(self.h, _ptr(masks)))
        return masks[:n]

    def counts(self):
        out = np.zeros(4, dtype=np.int64)
        check(load().azh_samples_counts(self.h, _ptr(out)))
        return {"games": int(out[0]), "plies": int(out[1]), "targets": int(out[2]), "bad_plies": int(out[3])}

    def mirror(self):
        """-> (games (G, 4) u32, ply_flags (P,) u8): the host's copy of what a draw is checked against."""
        if self._mirror is None:
            c = self.counts()
            games, flags = np.zeros((max(c["games"], 1), 4), np.uint32), np.zeros(max(c["plies"], 1), np.uint8)
            check(load().azh_samples_mirror(self.h, _ptr(games), _ptr(flags)))
            self._mirror = games[:c["games"]], flags[:c["plies"]]
        return self._mirror

    # features, policy, value; ownership, score, reply, aux_weight: a sample's shape in each output tensor
    _SHAPES = ((7, 7, 4), (7, 7, 17), (1,), (7, 7), (1,), (7, 7, 17), (2,))

    @staticmethod
    def outputs(n, device="cuda", count=3):
        import torch
        return tuple(torch.empty((n,) + shape, dtype=torch.float32, device=device) for shape in SampleStore._SHAPES[:count])

    @staticmethod
    def aux_outputs(n, device="cuda"):
        """outputs and the four auxiliary tensors: ownership (n, 7, 7), score (n, 1), reply (n, 7, 7, 17), aux_weight (n, 2)."""
        return SampleStore.outputs(n, device, count=7)

    @staticmethod
    def _pointers(out, n):
        """-> (the azh_sample_outputs of three tensors, or of seven with the auxiliary targets; the stream to enqueue on)."""
        import torch
        if len(out) not in (3, 7):
            raise ValueError("out must be 3 tensors, or 7 with the auxiliary targets")
        shapes = tuple((n,) + shape for shape in SampleStore._SHAPES[:len(out)])
        for t, shape in zip(out, shapes):
            if not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError("out must be contiguous float32 GPU tensors of shapes %r" % (shapes,))
        # (torch's default stream is the null stream, handle 0 — which the C entry points read as "the store's own stream,
        # and wait": hipStreamLegacy names the null stream itself, so the call is ordered behind torch's work and returns)
        return CSampleOutputs(*[t.data_ptr() for t in out]), torch.cuda.current_stream().cuda_stream or HIP_STREAM_LEGACY

    def gather(self, draws, value_blend=0.0, out=None, aux=False):
        """The minibatch of the draws (n, 3) of (game, ply, symmetry), enqueued on torch's current stream; `out`: the three
        tensors to write, or seven: the auxiliary targets behind the three (fresh ones by default: outputs, or aux_outputs
        under aux).  A draw on a bad ply raises the host pipeline's AssertionError."""
        draws = np.ascontiguousarray(draws, dtype=np.int32).reshape(-1, 3)
        out = self.outputs(len(draws), count=7 if aux else 3) if out is None else out
        ptrs, stream = self._pointers(out, len(draws))
        rc = load().azh_samples_gather(self.h, len(draws), _ptr(draws), float(value_blend), ctypes.byref(ptrs), stream)
        if rc == -2:
            raise AssertionError("policy target does not sum to one")
        check(rc)
        return out

    def draw_gather(self, n, seed, step, first_game, n_games, value_blend=0.0, out=None, draws_out=None, aux=False):
        """A minibatch of n samples drawn on the device from games [first_game, first_game + n_games) with Philox keyed by
        `seed` at counter `step`; out, aux: as gather; draws_out: an (n, 4) int32 GPU tensor that receives (game, ply,
        symmetry, attempts)."""
        import torch
        out = self.outputs(n, count=7 if aux else 3) if out is None else out
        ptrs, stream = self._pointers(out, n)
        if draws_out is not None and not (draws_out.is_cuda and draws_out.dtype == torch.int32 and
                                          tuple(draws_out.shape) == (n, 4) and draws_out.is_contiguous()):
            raise ValueError("draws_out must be a contiguous int32 GPU tensor of shape (n, 4)")
        check(load().azh_samples_draw_gather(self.h, int(n), int(seed), int(step), int(first_game), int(n_games),
                                             float(value_blend), ctypes.byref(ptrs),
                                             ctypes.c_void_p(draws_out.data_ptr()) if draws_out is not None else None, stream))
        return out

    def draw(self, seed, step, sample, first_game, n_games):
        """What draw_gather draws for one sample, from the host mirror (samples_draw)."""
        games, flags = self.mirror()
        return samples_draw(seed, step, sample, first_game, n_games, games, flags)

    # policy surprise weighting ("Policy surprise weighting")

    def _game_plies(self, first_game, n_games):
        games, _ = self.mirror()
        if not (0 <= first_game and 1 <= n_games and first_game + n_games <= len(games)):
            raise ValueError("games [%d, %d) of %d" % (first_game, first_game + n_games, len(games)))
        return int(games[first_game + n_games - 1][0]) + int(games[first_game + n_games - 1][1]) - int(games[first_game][0])

    def surprise(self, net, dtype, first_game, n_games, chunk=0):
        """KL(policy target || the prior of `net`, a link.Net, in `dtype`) of every ply of games [first_game, first_game +
        n_games) -> (f32 array, one per ply; targets that are no legal moves: 0 for games the engine wrote).  chunk: plies
        per tower launch (0: 16384)."""
        kl, illegal = np.zeros(self._game_plies(first_game, n_games), dtype=np.float32), ctypes.c_int64(0)
        check(load().azh_samples_set_surprise_chunk(self.h, int(chunk)))
        check(load().azh_samples_surprise(self.h, net.h, int(dtype), int(first_game), int(n_games), _ptr(kl),
                                          ctypes.byref(illegal)))
        return kl, int(illegal.value)

    def surprise_ms(self):
        """HIP-event milliseconds of the last surprise(): (board packing and tower, surprise kernel)."""
        ms = np.zeros(2, dtype=np.float32)
        check(load().azh_samples_surprise_ms(self.h, _ptr(ms)))
        return float(ms[0]), float(ms[1])

    def surprise_from_logits(self, first_ply, logits):
        """The same for plies [first_ply, first_ply + n) from an (n, 833) float32 GPU tensor of logits, enqueued on torch's
        current stream."""
        import torch
        if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.shape[1] == 833 and
                logits.is_contiguous() and len(logits) >= 1):
            raise ValueError("logits must be a contiguous float32 GPU tensor of shape (n, 833)")
        kl, illegal = np.zeros(len(logits), dtype=np.float32), ctypes.c_int64(0)
        check(load().azh_samples_surprise_logits(self.h, int(first_ply), len(logits), ctypes.c_void_p(logits.data_ptr()),
                                                 _ptr(kl), ctypes.byref(illegal),
                                                 torch.cuda.current_stream().cuda_stream or HIP_STREAM_LEGACY))
        return kl, int(illegal.value)

    def set_ply_weights(self, first_game, n_games, weights):
        """One weight >= 0 per ply of games [first_game, first_game + n_games): draw_gather then picks a game's ply in
        proportion to its candidates' weights (kept in units of 1 / 65536).  A refused call changes nothing."""
        w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
        if len(w) != self._game_plies(first_game, n_games):
            raise ValueError("one weight per ply of the games")
        check(load().azh_samples_set_ply_weights(self.h, int(first_game), int(n_games), _ptr(w)))

    def clear_ply_weights(self):
        check(load().azh_samples_clear_ply_weights(self.h))

    def ply_cum(self):
        """-> (candidates (P,) u16, candidate_count (G,) u32, cum (P,) u32, weights held?): the mirror of the weighted draw;
        cum[first ply + k] is the running sum of the weights of the game's candidates 0 .. k."""
        c = self.counts()
        cand, count = np.zeros(max(c["plies"], 1), np.uint16), np.zeros(max(c["games"], 1), np.uint32)
        cum, present = np.zeros(max(c["plies"], 1), np.uint32), ctypes.c_int32(0)
        check(load().azh_samples_ply_cum(self.h, _ptr(cand), _ptr(count), _ptr(cum), ctypes.byref(present)))
        return cand[:c["plies"]], count[:c["games"]], cum[:c["plies"]], bool(present.value)

    def draw_weighted(self, seed, step, sample, first_game, n_games):
        """What draw_gather draws for one sample while weights are held, from the host mirrors (samples_draw_weighted)."""
        games, flags = self.mirror()
        cand, _, cum, _ = self.ply_cum()
        return samples_draw_weighted(seed, step, sample, first_game, n_games, games, flags, cand, cum)

    def status(self):
        """Samples of draw_gather that found no drawable ply in 64 attempts (written as zeros) since the store was made;
        waits for the device."""
        n = ctypes.c_int64(0)
        check(load().azh_samples_status(self.h, ctypes.byref(n)))
        return int(n.value)

    # reanalysis of stored plies ("Reanalysis of stored plies")

    def read_plies(self, plies, targets=True):
        """The stored plies (n, 2) of (game, ply) read back from the device -> (boards (n, 2) u64 of (x, o), values (n,) f64,
        flags (n,) u8, target_start (n + 1,) i32, index u16, weight f32): what the store holds now, the targets in stored
        order; targets=False: index and weight are None (azh_samples_read_plies)."""
        plies = np.ascontiguousarray(plies, dtype=np.int32).reshape(-1, 2)
        n = len(plies)
        boards, values = np.zeros((n, 2), dtype=np.uint64), np.zeros(n, dtype=np.float64)
        flags, start = np.zeros(n, dtype=np.uint8), np.zeros(n + 1, dtype=np.int32)
        lib = load()
        check(lib.azh_samples_read_plies(self.h, n, _ptr(plies), _ptr(boards), _ptr(values), _ptr(flags), _ptr(start), None,
                                         None, 0))
        if not targets:
            return boards, values, flags, start, None, None
        total = int(start[n])
        index, weight = np.zeros(max(total, 1), dtype=np.uint16), np.zeros(max(total, 1), dtype=np.float32)
        check(lib.azh_samples_read_plies(self.h, n, _ptr(plies), _ptr(boards), _ptr(values), _ptr(flags), _ptr(start),
                                         _ptr(index), _ptr(weight), total))
        return boards, values, flags, start, index[:total], weight[:total]

    def ply_targets(self, plies):
        """Diagnostic -> (n, 2) u32 of (first target, targets): where the targets of the plies (n, 2) of (game, ply) lie in the
        store (azh_samples_ply_targets)."""
        plies = np.ascontiguousarray(plies, dtype=np.int32).reshape(-1, 2)
        out = np.zeros((len(plies), 2), dtype=np.uint32)
        check(load().azh_samples_ply_targets(self.h, len(plies), _ptr(plies), _ptr(out)))
        return out

    def retarget(self, plies, reports, blockers=0):
        """The plies (n, 2) of (game, ply) take the first n records of `reports`, an int32 GPU tensor of root reports
        (Engine.root_report_device) searched on the walls `blockers`, as their policy target and value -> status (n,) int32:
        1 changed, 0 left as it was.  A refused call changes nothing (azh_samples_retarget)."""
        import torch
        plies = np.ascontiguousarray(plies, dtype=np.int32).reshape(-1, 2)
        n = len(plies)
        if not (reports.is_cuda and reports.dtype == torch.int32 and reports.is_contiguous() and
                reports.numel() >= n * ROOT_REPORT_WORDS):
            raise ValueError("reports must be a contiguous int32 GPU tensor of at least n * ROOT_REPORT_WORDS words")
        status = np.zeros(n, dtype=np.int32)
        check(load().azh_samples_retarget(self.h, n, _ptr(plies), ctypes.c_void_p(reports.data_ptr()), int(blockers),
                                          _ptr(status), torch.cuda.current_stream().cuda_stream or HIP_STREAM_LEGACY))
        return status

    # proven outcomes for stored plies ("Proven outcomes for stored plies")

    PROOF_STATS = ("visited", "wins", "losses", "contradicted", "retargeted", "nodes")   # AZH_PROOF_*

    def prove(self, first_game, n_games, depth, node_budget=0, retarget_wins=False):
        """The alpha-beta search of every eligible ply of games [first_game, first_game + n_games) that has no proof yet, at
        (depth, node_budget) as alphabeta_search takes them; a value of 1000 or more in magnitude becomes the ply's proof, and
        minibatches then train its value on the proven outcome; retarget_wins: a ply newly proven won also takes its move as
        its policy target -> this call's counts, a dict over PROOF_STATS.  A refused call changes nothing (azh_samples_prove).
        Minibatch calls enqueued on torch's current stream are waited for first."""
        import torch
        torch.cuda.current_stream().synchronize()
        stats = np.zeros(len(self.PROOF_STATS), dtype=np.uint64)
        check(load().azh_samples_prove(self.h, int(first_game), int(n_games), int(depth), int(node_budget),
                                       int(bool(retarget_wins)), _ptr(stats)))
        return dict(zip(self.PROOF_STATS, (int(v) for v in stats)))

    def proofs(self, plies):
        """The plies (n, 2) of (game, ply) -> (proof (n,) i32: 0 or the proving search's value; move (n,) u16 and depth_done
        (n,) i32 of the ply's last search, 0xFFFF and 0 before one), read back from the device (azh_samples_proofs)."""
        plies = np.ascontiguousarray(plies, dtype=np.int32).reshape(-1, 2)
        n = len(plies)
        proof, move, done = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.int32)
        check(load().azh_samples_proofs(self.h, n, _ptr(plies), _ptr(proof), _ptr(move), _ptr(done)))
        return proof, move, done

    # lambda-returns as value targets ("Lambda-returns as value targets")

    def value_returns(self, first_game, n_games, lam):
        """The TD(lambda) return G_p of every ply of the games [first_game, first_game + n_games) that carry values, from the
        stored values and proofs as they are now, one wave per game; minibatches then write (float)G_p as the value target of
        a covered ply.  Run it after retarget and prove: either leaves the returns stale; calling it again recomputes.  A
        refused call changes nothing (azh_samples_value_returns).  Minibatch calls enqueued on torch's current stream are
        waited for first."""
        import torch
        torch.cuda.current_stream().synchronize()
        check(load().azh_samples_value_returns(self.h, int(first_game), int(n_games), float(lam)))

    def clear_value_returns(self):
        """Minibatches are again what they were before the first value_returns (azh_samples_clear_value_returns)."""
        check(load().azh_samples_clear_value_returns(self.h))

    def read_value_returns(self, plies):
        """The plies (n, 2) of (game, ply) -> (G (n,) f64, 0.0 where absent; present (n,) bool), read back from the device
        (azh_samples_read_value_returns)."""
        plies = np.ascontiguousarray(plies, dtype=np.int32).reshape(-1, 2)
        n = len(plies)
        out, present = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int32)
        check(load().azh_samples_read_value_returns(self.h, n, _ptr(plies), _ptr(out), _ptr(present)))
        return out, present != 0
