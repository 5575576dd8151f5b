// Device code of the search engine that more than one translation unit compiles: the engine's parameter block, the HBM
// layout helpers of the tree arenas, game start, the re-root (reroot_game: also behind the moves a host names, k_play_moves in
// engine.hip) and the ply advance (sample the move, record the ply, re-root, finish or restart the game).  engine.hip owns the tree kernels; net_kernels.hip compiles advance_game too, because the device-resident
// loop plays the queued moves INSIDE the tower launch (advance_worker below, round 6): the tower leaves no wave slot and no
// LDS beside itself, so a re-root launch on a side stream waited most of its life for the tower's first workgroups to retire,
// and its cross-stream events cost every iteration 7-10 us whether or not a move was due (profiles/round6_reroots_in_the_tower_launch.txt).
// Nothing here does floating-point arithmetic whose result could depend on the translation unit's contraction mode (the
// pruning's arithmetic, azh_device.h's forced_* functions, switches contraction off itself).
#pragma once

#include "azh_device.h"
#include "azh_host.h"
#include "record.h"

namespace azh {

// (the finished-game record's layout, RING_MAGIC and the REC_* constants: record.h)
constexpr int REC_STRIDE_WORDS = REC_HDR_WORDS + REC_MAXD;  // a ply as it waits on the device for its game to end
constexpr int NSTAT = AZH_STAT_COUNT;
constexpr int BFS_QL = 384;  // re-root frontier entries kept in LDS; later ones spill to bfs_spill in HBM

// One start position of the pool: stones, walls, side to move (0: x).
struct StartEntry {
    u64 x, o, blockers;
    int turn, pad;
};

struct EngineParams {
    int G, visits, node_cap, edge_cap, path_cap, max_plies;
    float c_puct, alpha, noise_w;
    u32 k0, k1;
    u64 start_x, start_o, blockers;
    int start_turn;
    u32 flags;
    int select_budget;  // tree levels per select launch and game (0 = unlimited), azh_config.select_budget
    u32 uid_limit;       // azh_engine_set_game_limit: games with uid >= this are not started (0 = no limit); a slot whose
                         // next game would be one of them goes idle (phase 3: no leaf, no move, nothing to back up)
    u32 *tt;             // AZH_FLAG_EVAL_CACHE: [2][G][tt_size] open-addressed table of evaluated nodes, keyed by the board
    int tt_size;         // power of two >= 4 * node_cap
    int *no_emit;        // [G] start ply + 1 when the slot's current game was started from a loaded position
                         // (azh_engine_set_positions), else 0: such a game is played, counted and its record assembled and
                         // handed to the host like any other, but it lacks the plies before the start, so no line is written.
                         // NO_EMIT_LOADED beside it: azh_engine_set_positions wrote the word and no host move has since —
                         // what tells a loaded game that has not begun from the fresh root azh_engine_play_moves leaves
    azh_game_state *gs;
    int *force;
    int *adv_list;   // games whose move is due (phase 2), appended by mark_game, consumed by k_advance_list
    int *adv_count;
    int *adv_done;   // tickets of k_advance_list's workgroups: the last one to finish empties the queue
    int *path;
    ulonglong2 *node_board;
    uint4 *node_info;
    uint4 *edge;
    u16 *edge_move;
    ulonglong2 *leaf_board;
    int *need_eval;
    int *leaf_list;
    int *leaf_count;
    int *leaf_list2;   // arena: leaves of the games whose mover is net B
    int *leaf_count2;
    int *tree_done;    // tickets of the workgroups of a k_tree launch (the last one compacts the leaf list): TICKET_SHARDS
                       // counters, TICKET_STRIDE ints apart, and one on top of them (a single word takes ~88 atomics per
                       // microsecond: thousands of workgroups finishing together would queue on it)
    u32 *need_mask;    // [2][mask_words] one bit per game: its leaf goes to the net (row 1: to net B, arena); set by
    int mask_words;    // k_tree's workgroups with one atomic OR each, read and cleared by the workgroup that finishes last
    u64 *stamps;       // diagnostic instantiation of k_tree only: [G][TREE_STAMPS] s_memrealtime readings (100 MHz)
    float *logits;
    float *values;
    u32 *rec;
    u32 *ring;
    u64 ring_cap_words;
    u64 *ring_head;
    u64 *stats;
    u32 *bfs_spill;  // [G][3][node_cap] frontier entries beyond BFS_QL
    // playout cap randomization (azh_engine_set_playout_cap; DESIGN.md "Playout cap randomization"), off while fast_visits == 0
    int fast_visits;       // root-visit threshold of a FAST ply (a FULL ply's is `visits`)
    u32 full_per_65536;    // a ply is FULL iff (philox(uid, ply, STREAM_PLAYOUT_CAP).v[0] >> 16) < this
    u32 *ply_kind;         // [G] the kind of the ply each slot is searching, derived where the ply begins (begin_ply): PLY_FULL,
                           // or the FAST ply's threshold — the tree kernels read one word instead of running Philox per mark
    // forced playouts and policy target pruning (azh_engine_set_forced_playouts), off while forced_k == 0
    float forced_k;        // a root edge with n >= 1 visits is owed sqrt(forced_k * P * N) of them, on the plies that get root noise
    // random symmetry per evaluation (azh_engine_set_random_symmetry; DESIGN.md "Random symmetry per evaluation"), off while 0
    u32 random_symmetry;   // the evaluator sees T_s of every leaf board and apply_priors gathers through T_s of every move
    u32 *eval_key;         // [G] the key word of each slot's game (eval_symmetry_key), written where a game begins (begin_game_key):
                           // s = eval_symmetry_of(key, the position) — no Philox block on the tree kernels' per-iteration path
    // recorded search value and resignation (azh_engine_set_resign), off while resign_plies == 0
    float resign_below;       // a counted ply is bad for its mover iff q < this
    u32 resign_plies;         // the rule fires when the mover's counter of consecutive bad plies reaches this
    u32 resign_through;       // game uid plays through iff (philox(uid, 0, STREAM_RESIGN).v[0] >> 16) < this
    u32 *resign_state;        // [G] bits 0-7 / 8-15: the counter of side 1 / 2, bits 16-17: the side the rule first fired for;
                              // cleared where a game begins (begin_game_key's callers), written by k_advance_list's advance_game
    u64 *resign_stats;        // [AZH_RESIGN_STAT_COUNT] once-per-game counts (global atomics at a game's end)
    // temperature of the move played and of the root policy (azh_engine_set_temperature), each off while null
    const float *move_temperature;         // [max_plies] 1: the proportional draw, 0: the most visited move, else n^(1/T) in
                                           // fixed point (temperature_weight); read by k_advance_list's advance_game alone
    const float *root_policy_temperature;  // [max_plies] apply_priors divides the logits of a noise ply's root by this
    // Gumbel root search with sequential halving (azh_engine_set_gumbel), off while gumbel_m == 0
    int gumbel_m;               // considered actions at the root
    float gumbel_c_visit, gumbel_c_scale;
    const u16 *gumbel_seq;      // [gumbel_m][visits] row r - 1: the considered visit counts for r actions at the current `visits`
    float *gumbel_a;            // [G][MAX_MOVES] a_j = g_j + l_j of every root edge, written by the root's backup
    float *gumbel_v0;           // [G] the root's own value as a [0, 1] score, written beside it
    // a start position and wall map per game (azh_engine_set_start_pool; DESIGN.md "A start position per game"), off while null
    const StartEntry *pool;     // [pool_n] game uid starts from entry (uid / pool_stride) % pool_n
    u32 pool_n, pool_stride;
    u64 *slot_mask;             // [G] the wall mask of each slot's current game, written where a game begins (init_game_at)
    u64 *leaf_mask;             // [slots] beside leaf_board: the mask of the game that selected the slot's leaf, written by that
                                // select — the tower reads it, never slot_mask (the launch's first workgroups restart games)
    // first-play urgency and the exploration rate (azh_engine_set_exploration), read by vl_select_game alone; off
    // while fpu_reduction < 0 and c_base == 0 (exploration_on)
    float fpu_reduction;        // an unvisited child's Q is the node's mean score less this * sqrt(visited policy mass); < 0: 0
    float c_base, c_init;       // c = log((1 + N + c_base) / c_base) + c_init; c_base == 0: the constant c_puct
    // search settings per side (azh_engine_set_search_sets; DESIGN.md "Search settings per side"), off while search_sets is null
    const azh_search_set *search_sets;  // [n_search_sets] on the device: k_vl_tree loads the set of the root's mover (a table
    int n_search_sets;                  // in this block would ride in every launch's kernel arguments)
    u32 *slot_sets;             // [G] the set of x | the set of o << 8 in each slot's current game (search_set_pairing), written
                                // where a game begins (begin_game_key)
    u64 *set_stats;             // [n][n][AZH_SET_STAT_COUNT] once-per-game counts by (set of x, set of o): global atomics at a
                                // game's end, in k_advance_list's advance_game alone
};

// The walls slot g's game is played on (g wave-uniform: one scalar 8-byte load); the engine's one mask while no pool is set.
__device__ inline u64 game_blockers(const EngineParams &P, int g) { return P.pool ? P.slot_mask[g] : P.blockers; }

constexpr u32 PLY_FULL = 0x80000000u;
constexpr int NO_EMIT_LOADED = 1 << 30;        // no_emit: the game stands where azh_engine_set_positions put it (max_plies < 2^30)
constexpr int NO_EMIT_PLY = NO_EMIT_LOADED - 1;  // no_emit: start ply + 1

// The game limit's "has not begun" (azh_engine_set_game_limit): nothing in flight, a one-node root nobody has
// evaluated, and no move of this game played — a game the engine started stands at ply 0, a loaded one at its loaded ply with
// the mark azh_engine_play_moves takes away.  The same test on an idle slot (phase 3) finds the loaded game it was idled with.
__device__ inline bool game_unbegun(const azh_game_state &s, int no_emit)
{
    const bool at_start = (no_emit & NO_EMIT_LOADED) ? s.ply == (no_emit & NO_EMIT_PLY) - 1 : s.ply == 0 && no_emit == 0;
    return s.leaf_kind == AZH_LEAF_NONE && s.n_nodes == 1 && s.root_visits == 0 && at_start;
}

// A ply of slot g begins (game start and restart, after a re-root, a loaded position, the setter itself): its kind.
__device__ inline void begin_ply(const EngineParams &P, int g, u32 uid, int ply)
{
    if (P.fast_visits != 0 && lane_id() == 0) {
        asm volatile("" : "+v"(uid));  // the Philox block in vector registers: its callers have no scalar registers to spare
        P.ply_kind[g] = playout_cap_full(P.k0, P.k1, uid, (u32)ply, P.full_per_65536) ? PLY_FULL : (u32)P.fast_visits;
    }
}

// A game of slot g begins (start, restart, a loaded position, the game limit's late starts: init_game_at): its key word.
__device__ inline void begin_game_key(const EngineParams &P, int g, u32 uid)
{
    if (P.random_symmetry != 0u && lane_id() == 0) {
        asm volatile("" : "+v"(uid));  // (as begin_ply: the block in vector registers)
        P.eval_key[g] = eval_symmetry_key(P.k0, P.k1, uid);
    }
    if (P.resign_plies != 0u && lane_id() == 0)  // the game's resign counters (the same instantiations: every game start but
        P.resign_state[g] = 0u;                  // the tower kernels', which play no move while the mode is on)
    if (P.search_sets != nullptr && lane_id() == 0)  // the game's pairing (search settings per side; the same instantiations)
        P.slot_sets[g] = search_set_pairing(uid, (u32)P.n_search_sets);
}

// The kind word of slot g's ply as the tree kernels use it (g wave-uniform: a scalar load); PLY_FULL while the mode is off.
__device__ inline u32 ply_kind_of(const EngineParams &P, int g) { return P.fast_visits != 0 ? P.ply_kind[g] : PLY_FULL; }
// root visits at which the ply's move is due
__device__ inline int ply_threshold(const EngineParams &P, u32 kind) { return (kind & PLY_FULL) ? P.visits : (int)kind; }

// Per-block (= per-game wave) LDS scratch shared by the tree phases.
struct TreeLds {
    u16 moves[MAX_MOVES];
    u32 old[WAVE], pref[WAVE + 1];
    union {              // the sampling weights are dead before the re-root copy starts
        u64 w[MAX_MOVES];
        u32 q[3][BFS_QL];  // frontier queue: old node id, the node's packed edge range (old arena), parent edge (new arena)
    };
};
// All G waves of a launch must be resident at once (the kernel lasts as long as its deepest descent):
// 16 games per CU at G = 4096, so the scratch has to stay under 160 KiB / 16.
static_assert(sizeof(TreeLds) <= 8192, "TreeLds: keep >= 20 game waves per CU");

struct Arena {
    ulonglong2 *nb;
    uint4 *ni;
    uint4 *ed;
    u16 *em;
};

__device__ inline Arena arena_of(const EngineParams &P, int a, int g)
{
    const size_t slot = (size_t)a * P.G + g;
    Arena A;
    A.nb = P.node_board + slot * P.node_cap;
    A.ni = P.node_info + slot * P.node_cap;
    A.ed = P.edge + slot * P.edge_cap;
    A.em = P.edge_move + slot * P.edge_cap;
    return A;
}

// The 16-byte edge record.  Everything a PUCT level needs about a child sits in it: 16 B per child instead of the 24
// of a separate (first_edge, n_edges) array — the descents of thousands of games are in flight together and their
// level loads share the memory system (tools/tree_stamps.py: a level costs 0.93 us at 1024 games, 1.37 at 4096).
//   x  prior (f32 bits; >= 0, so bit 31 is free: it MARKS the child the last descent through this node chose —
//      select_game's early request of the next level; never read by anything that decides, masked out of the documented
//      tree, PRIOR_MASK)                     y  total score W (f32 bits)
//   z  visits (bits 0-15) | child node (bits 16-31, ENONE = not expanded)
//   w  the child's first edge (bits 0-22) | its edge count (bits 23-30) | finished position (bit 31); 0 in an edge without
//      a child
// visits <= 60000 and nodes <= visits + 8 (azh_engine_create), edges per game < 2^23, moves per position <= 255.
constexpr u32 ENONE = 0xFFFFu;
__device__ inline u32 edge_visits(const uint4 &e) { return e.z & 0xFFFFu; }
__device__ inline u32 edge_child(const uint4 &e) { return e.z >> 16; }
__device__ inline uint4 fresh_edge(u32 prior_bits) { return make_uint4(prior_bits, 0u, ENONE << 16, 0u); }
__device__ inline u32 pack_kid(u32 first, u32 n_edges, u32 finished) { return first | (n_edges << 23) | (finished << 31); }
__device__ inline u32 kid_first(u32 w) { return w & 0x7FFFFFu; }
__device__ inline int kid_count(u32 w) { return (int)((w >> 23) & 0xFFu); }
__device__ inline bool kid_finished(u32 w) { return (w >> 31) != 0u; }

// ONE_RANDOM_MOVE (:515-518): ply of the uniformly random move, uniform on 0..119, a pure function of
// (seed, game uid).
__device__ inline int random_ply_of(const EngineParams &P, u32 uid)
{
    const Philox4 r = philox(P.k0, P.k1, uid, 0u, STREAM_RANDOM_PLY, 0u);
    return (int)(((u64)r.v[0] * 120ull) >> 32);
}

__device__ inline void add_stat(const EngineParams &P, int g, int k, u64 v)
{
    if (v)
        P.stats[(size_t)g * NSTAT + k] += v;
}

// ------------------------------------------------------------------ evaluation cache (AZH_FLAG_EVAL_CACHE)
// A position the search of this game has already evaluated is not sent to the net again: engine.py's NNEvaluator.cache
// (engine.py:127-234; the C++ generator has none).  Transpositions and re-visited positions are about a quarter of all
// leaves at 400 sims/move.  Per game and arena an open-addressed table maps a board to a node that carries its
// evaluation (priors on its edges, value in node_info.w); the net is deterministic, so copying that evaluation is what
// evaluating again would give.  The root is never a source: its priors carry this ply's noise.
__host__ __device__ inline u32 tt_hash(u64 w0, u64 w1, u32 mask)
{
    const u64 k = (w0 * 0x9E3779B97F4A7C15ULL) ^ ((w1 + 0x7F4A7C15ULL) * 0xC2B2AE3D27D4EB4FULL);
    return (u32)(k >> 40) & mask;
}

__device__ inline u32 *tt_of(const EngineParams &P, int a, int g)
{
    return P.tt + ((size_t)a * P.G + g) * (size_t)P.tt_size;
}

// Node holding the evaluation of board (w0, w1), or NONE.  Wave-wide: lane l looks at slot h + l (the chain up to the
// first empty slot is searched in one round trip for the slots and one for the candidates' boards).
__device__ inline u32 tt_lookup(const u32 *tt, u32 mask, const Arena &A, u64 w0, u64 w1)
{
    const int lane = lane_id();
    const u32 id = tt[(tt_hash(w0, w1, mask) + (u32)lane) & mask];
    const u64 empties = __ballot(id == NONE);
    const u64 before = empties ? (empties & (0ULL - empties)) - 1ULL : ~0ULL;  // lanes ahead of the first empty slot
    bool match = false;
    if (((before >> lane) & 1ULL) && id != NONE) {
        const ulonglong2 b = A.nb[id];
        match = b.x == w0 && b.y == w1;
    }
    const u64 hits = __ballot(match);
    if (!hits)
        return NONE;
    return (u32)read_lane((int)id, __ffsll((long long)hits) - 1);
}

// One lane enters `id` under its board (linear probing; several lanes of the wave may insert at once).
__device__ inline void tt_insert(u32 *tt, u32 mask, u64 w0, u64 w1, u32 id)
{
    u32 slot = tt_hash(w0, w1, mask);
    for (u32 tries = 0; tries <= mask; tries++) {
        if (atomicCAS(&tt[slot], NONE, id) == NONE)
            return;
        slot = (slot + 1) & mask;
    }
}

__device__ inline void tt_clear(u32 *tt, int size)
{
    for (int i = lane_id(); i < size; i += WAVE)
        tt[i] = NONE;
}

// Fresh tree at the start position in arena 0 (generate_game :510-512,
// MCTS::init_from_scratch :380-383).  Wave-cooperative; s_moves is LDS scratch.  KEY: the instantiation that writes the game's
// key word of the random symmetry (begin_game_key) — every caller's but the tower kernels' advance_game, see there.
template <bool KEY = true>
__device__ inline void init_game_at(const EngineParams &P, int g, u32 uid, azh_game_state &s, u16 *s_moves, Board b, int ply,
                                    int loaded, u64 walls)
{
    const int lane = lane_id();
    Arena A = arena_of(P, 0, g);
    int res;
    const int M = wave_movegen(b, walls, s_moves, &res);
    wave_sync();
    for (int j = lane; j < M; j += WAVE) {
        A.ed[j] = fresh_edge(0u);
        A.em[j] = s_moves[j];
    }
    if (lane == 0) {
        A.nb[0] = make_ulonglong2(pack_word0(b), b.o);
        A.ni[0] = make_uint4(0u, (u32)M | ((u32)res << 16), 0u, 0u);
        P.force[g] = 0;
        P.no_emit[g] = loaded ? (ply + 1) | NO_EMIT_LOADED : 0;
        if (P.pool)
            P.slot_mask[g] = walls;
    }
    if (P.flags & AZH_FLAG_EVAL_CACHE)
        tt_clear(tt_of(P, 0, g), P.tt_size);
    begin_ply(P, g, uid, ply);
    if constexpr (KEY)
        begin_game_key(P, g, uid);
    wave_sync();
    s.phase = 0;
    s.arena = 0;
    s.n_nodes = 1;
    s.n_edges = M;
    s.ply = ply;
    s.root_visits = 0;
    s.leaf_kind = AZH_LEAF_NONE;
    s.leaf_node = 0;
    s.path_len = 0;
    s.uid = uid;
}

// The pool entry game `uid` starts from: round robin over the entries, `stride` consecutive uids sharing one (azh_start_pool_entry).
__host__ __device__ inline u32 start_pool_entry(u32 uid, u32 n, u32 stride) { return (uid / stride) % n; }

// Fresh game at the configured start position (the pool's entry of its uid where a pool is set) — or, past the game limit, no game: the slot goes idle.
template <bool KEY = true>
__device__ inline void init_game(const EngineParams &P, int g, u32 uid, azh_game_state &s, u16 *s_moves)
{
    if (P.uid_limit != 0u && uid >= P.uid_limit) {
        s.phase = 3;
        s.uid = uid;
        s.leaf_kind = AZH_LEAF_NONE;
        s.path_len = 0;
        s.root_visits = 0;
        if (lane_id() == 0) {
            P.force[g] = 0;
            P.no_emit[g] = 0;  // (the game that ended here may have been a loaded one: nothing is left to resume)
        }
        return;
    }
    Board b;
    b.x = P.start_x;
    b.o = P.start_o;
    b.turn = P.start_turn;
    u64 walls = P.blockers;
    if (P.pool) {
        const StartEntry &en = P.pool[start_pool_entry(uid, P.pool_n, P.pool_stride)];
        b.x = en.x;
        b.o = en.o;
        b.turn = en.turn;
        walls = en.blockers;
    }
    init_game_at<KEY>(P, g, uid, s, s_moves, b, 0, 0, walls);
}

constexpr u32 PRIOR_MASK = 0x7FFFFFFFu;  // the prior proper (bit 31 marks the remembered child)

// ------------------------------------------------------------------ re-root

struct RerootStats {
    u64 nodes = 0, edges = 0, spill = 0;  // AZH_STAT_REROOT_NODES / _EDGES / _SPILLS of this re-root
};

// The root edge with move `mv` has been played: the tree of the position after it is built in the other arena B — the
// subtree of the edge's child `c` with its counts and priors, or (c == ENONE: no child, or a tree that is not kept) a
// fresh one-node tree — the evaluation cache's table of that arena is rebuilt, the arenas flip and the ply goes up.
// `rootw`: the root's packed board.  Returns the adjudication of the new root (0: not finished).  Used by advance_game
// (the move the device sampled) and by k_play_moves (a move the host names, engine.hip).
__device__ inline int reroot_game(const EngineParams &P, int g, TreeLds &L, azh_game_state &s, const Arena &A, const Arena &B,
                                  const ulonglong2 rootw, u32 mv, u32 c, RerootStats &st)
{
    u16 *s_moves = L.moves;
    u32 *s_old = L.old, *s_pref = L.pref;
    u32 *spill = P.bfs_spill + (size_t)g * 3 * P.node_cap;
    const int node_cap = P.node_cap;
    // frontier queue accessors: LDS for the first BFS_QL nodes, HBM beyond
    auto q_put = [&](u32 i, u32 a, u32 b, u32 d) {
        if (i < (u32)BFS_QL) {
            L.q[0][i] = a; L.q[1][i] = b; L.q[2][i] = d;
        } else {
            spill[i] = a; spill[node_cap + i] = b; spill[2 * node_cap + i] = d;
        }
    };
    auto q_get = [&](u32 i, int f) -> u32 { return i < (u32)BFS_QL ? L.q[f][i] : spill[(size_t)f * node_cap + i]; };
    const int lane = lane_id();
    const u64 lt = (1ULL << lane) - 1ULL;
    // MCTS::play (:475-492): keep the chosen child's subtree, compacted breadth-first
    // into the other arena (children keep their edge order).
    int result;
    if (c == ENONE) {
        // miss: fresh tree from the position after the move (:479-483)
        const Board nbrd = make_move(unpack_board(rootw.x, rootw.y), (int)(mv & 0xFF), (int)(mv >> 8));
        const int Mn = wave_movegen(nbrd, game_blockers(P, g), s_moves, &result);
        wave_sync();
        const int Mw = result != 0 ? 0 : Mn;
        for (int j = lane; j < Mw; j += WAVE) {
            B.ed[j] = fresh_edge(0u);
            B.em[j] = s_moves[j];
        }
        if (lane == 0) {
            float tv = result == 1 ? 1.0f : -1.0f;
            if (nbrd.turn == 1)
                tv = -tv;
            B.nb[0] = make_ulonglong2(pack_word0(nbrd), nbrd.o);
            B.ni[0] = result != 0 ? make_uint4(0u, (u32)result << 16, 0u, f2u(tv)) : make_uint4(0u, (u32)Mw, 0u, 0u);
        }
        s.n_nodes = 1;
        s.n_edges = Mw;
        s.root_visits = 0;
    } else {
        const uint4 cinfo = A.ni[c];
        result = (int)(cinfo.y >> 16);
        // Breadth-first copy, up to 64 frontier nodes per pass.  Nodes are numbered in
        // (parent order, edge order) and a node's edges land at the running edge count,
        // exactly as the node-at-a-time loop of the oracle does, so the compacted arena is
        // bit-identical.  The frontier (old node id, old edge range, parent edge) is queued in
        // LDS when a child is discovered — its edge range is part of the edge that leads to it —
        // so one pass costs ONE dependent memory round trip.
        u32 t = 1, eb = 0, rv = 0, qs = 0;
        if (lane == 0)
            q_put(0u, c, pack_kid(cinfo.x, cinfo.y & 0xFFFFu, (cinfo.y >> 16) != 0u), 0u);
        wave_sync();
        while (qs < t) {
            const u32 nchunk = min(t - qs, (u32)WAVE);
            u32 of = 0, Mq = 0, kw = 0, old = 0, pe = 0;
            if ((u32)lane < nchunk) {
                old = q_get(qs + lane, 0);
                kw = q_get(qs + lane, 1);
                pe = q_get(qs + lane, 2);
                of = kid_first(kw);
                Mq = (u32)kid_count(kw);
            }
            const u32 incl = (u32)wave_incl_scan((int)Mq);
            const u32 Ef = (u32)bcast_last((int)incl);
            if ((u32)lane < nchunk) {
                const u32 nf = Mq ? eb + incl - Mq : 0u;
                s_old[lane] = of;
                s_pref[lane] = incl - Mq;
                // node copy: not on the dependent chain (nothing below waits for these loads)
                B.nb[qs + lane] = A.nb[old];
                const uint4 oinfo = A.ni[old];
                B.ni[qs + lane] = make_uint4(nf, oinfo.y, 0u, oinfo.w);
                if (qs + lane > 0)  // the edge that leads here was copied in an earlier pass: now it learns the new range
                    reinterpret_cast<u32 *>(&B.ed[pe])[3] = pack_kid(nf, Mq, kid_finished(kw));
            }
            if (lane == 0)
                s_pref[nchunk] = Ef;
            wave_sync();
            for (u32 e0 = 0; e0 < Ef; e0 += WAVE) {
                const u32 e = e0 + (u32)lane;
                const bool valid = e < Ef;
                uint4 ed = fresh_edge(0u);
                u16 m = 0;
                if (valid) {
                    u32 lo = 0, hi = nchunk;  // largest i with s_pref[i] <= e
                    while (hi - lo > 1) {
                        const u32 mid = (lo + hi) >> 1;
                        if (s_pref[mid] <= e) lo = mid;
                        else hi = mid;
                    }
                    const u32 src = s_old[lo] + (e - s_pref[lo]);
                    ed = A.ed[src];
                    m = A.em[src];
                    if (qs == 0 && lo == 0)
                        rv += edge_visits(ed);
                }
                const bool has = valid && edge_child(ed) != ENONE;
                const u64 mask = __ballot(has);
                const u32 dst = eb + e;
                if (has) {
                    const u32 nc = t + (u32)__popcll(mask & lt);
                    q_put(nc, edge_child(ed), ed.w, dst);
                    ed.z = (ed.z & 0xFFFFu) | (nc << 16);  // (ed.w still names the OLD range: rewritten when the child is copied)
                }
                if (valid) {
                    B.ed[dst] = ed;
                    B.em[dst] = m;
                }
                t += (u32)__popcll(mask);
            }
            eb += Ef;
            qs += nchunk;
            wave_sync();
        }
        s.n_nodes = (int)t;
        s.n_edges = (int)eb;
        s.root_visits = (int)wave_sum_u32(rv);
        st.nodes = t;
        st.edges = eb;
        st.spill = t > (u32)BFS_QL ? 1 : 0;
    }
    if (P.flags & AZH_FLAG_EVAL_CACHE) {
        // the kept subtree's evaluations stay usable: rebuild the table of the new arena from its nodes (all but the
        // root, whose priors are about to get this ply's noise; finished positions carry no priors)
        u32 *tt = tt_of(P, 1 - s.arena, g);
        tt_clear(tt, P.tt_size);
        __threadfence();
        wave_sync();
        for (u32 n = 1u + (u32)lane; n < (u32)s.n_nodes; n += WAVE) {
            const uint4 info = B.ni[n];
            if ((info.y >> 16) == 0u && (info.y & 0xFFFFu) != 0u) {
                const ulonglong2 b = B.nb[n];
                tt_insert(tt, (u32)P.tt_size - 1u, b.x, b.y, n);
            }
        }
    }
    s.arena = 1 - s.arena;
    s.ply += 1;
    wave_sync();
    return result;
}

// ------------------------------------------------------------------ ply advance

// Policy target pruning (azh_engine_set_forced_playouts; DESIGN.md, "Forced playouts and policy target pruning"): the visit
// distribution of the ply's record, rec, from the root's M edges (N = root visits) with the forced visits that PUCT would
// not have spent taken back (forced_prune_edge); an edge pruned to 0 is left out.  Returns the number of entries written.
// Reads the edges again in two rolled loops of its own instead of sharing advance_game's registers: advance_game is part of
// the tower kernels, which have no register to spare.
__device__ inline int record_pruned_counts(const EngineParams &P, const Arena &A, u32 first, int M, u32 N, u32 *rec)
{
    const int lane = lane_id();
    u64 key = 0;  // the most visited edge, ties to the lowest index: it keeps its visits and sets the bar S
#pragma unroll 1
    for (int j = lane; j < M; j += WAVE) {
        const u64 kk = ((u64)(reinterpret_cast<const u32 *>(&A.ed[first + j])[2] & 0xFFFFu) << 32) | (u64)(0xFFFFFFFFu - (u32)j);
        key = kk > key ? kk : key;
    }
    key = wave_max_u64(key);
    const int best = M > 0 ? (int)(0xFFFFFFFFu - (u32)key) : 0;
    const u32 n_b = (u32)(key >> 32);
    const uint2 bw = *reinterpret_cast<const uint2 *>(&A.ed[first + (u32)best]);
    const float sq = sqrtf((float)(1u + N));
    const float S = forced_score(u2f(bw.x & PRIOR_MASK), n_b ? u2f(bw.y) / (float)n_b : 0.0f, n_b, sq, P.c_puct);
    const u64 lt = (1ULL << lane) - 1ULL;
    int nd = 0;
#pragma unroll 1
    for (int j0 = 0; j0 < M; j0 += WAVE) {
        const int j = j0 + lane;
        bool has = false;
        u32 word = 0;
        if (j < M) {
            const uint4 ev = A.ed[first + j];
            u32 wr = edge_visits(ev);
            if (j != best && wr >= 1u)
                wr = forced_prune_edge(u2f(ev.x & PRIOR_MASK), u2f(ev.y), wr, N, P.forced_k, P.c_puct, sq, S);
            has = edge_child(ev) != ENONE && wr != 0u;
            word = (u32)A.em[first + j] | (wr << 16);
        }
        const u64 mask = __ballot(has);
        if (has)
            rec[REC_HDR_WORDS + nd + __popcll(mask & lt)] = word;
        nd += __popcll(mask);
    }
    return nd;
}

// The move of a ply whose temperature T is not 1 (azh_engine_set_temperature; DESIGN.md, "Temperature of the move and of the
// root policy"): the wave's form of temperature_pick_root.  nv: this lane's visit counts of root edges lane + 64 k (0 beyond
// M), v0: word 0 of the ply's sampling block.  T == 0: the most visited edge, the first on a tie; else the proportional scan
// on the fixed-point weights q in place of the counts.
__device__ inline int tempered_choice(const u32 (&nv)[4], int M, float T, u32 v0)
{
    const int lane = lane_id();
    u64 key = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = lane + 64 * k;
        if (j < M) {
            const u64 kk = ((u64)nv[k] << 32) | (u64)(0xFFFFFFFFu - (u32)j);
            key = kk > key ? kk : key;
        }
    }
    key = wave_max_u64(key);
    if (M <= 0)
        return 0;
    if (T == 0.0f)
        return (int)(0xFFFFFFFFu - (u32)key);
    const float lmax = det_logf((float)(u32)(key >> 32));
    u32 q[4];
    u32 part = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        q[k] = lane + 64 * k < M ? temperature_weight(nv[k], lmax, T) : 0u;
        part += q[k];
    }
    const u32 S = wave_sum_u32(part);  // <= 256 * 2^20
    const u32 r = (u32)(((u64)v0 * (u64)S) >> 32);
    int chosen = -1;
    u32 run = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = lane + 64 * k;
        const int incl = wave_incl_scan((int)q[k]);
        const u32 cum = run + (u32)incl;
        const u64 mask = __ballot(j < M && cum > r);
        if (chosen < 0 && mask)
            chosen = 64 * k + (__ffsll((long long)mask) - 1);
        run += (u32)bcast_last(incl);
    }
    return chosen < 0 ? 0 : chosen;
}

// Gumbel root search (azh_engine_set_gumbel; DESIGN.md, "Gumbel root search with sequential halving"): the move of the ply
// and its record's counts, the wave's form of gumbel_root.  `chosen` receives the edge with n_max visits and the greatest
// a + ks q (the lowest index among equal ones); rec gets move | c << 16 of every root edge, expanded or not, whose count c of
// the improved policy softmax(l + ks completedQ) is >= 1, in edge order.  Returns the number of entries written.  Rolled loops
// over the edges of its own, as record_pruned_counts: only k_advance_list's instantiation of advance_game calls it.
__device__ inline int gumbel_record(const EngineParams &P, const Arena &A, u32 first, int M, u32 N, int g, u32 *rec, int &chosen)
{
#pragma clang fp contract(off)
    const int lane = lane_id();
    const float *ga = P.gumbel_a + (size_t)g * MAX_MOVES;
    u32 nm = 0;
#pragma unroll 1
    for (int j = lane; j < M; j += WAVE)
        nm = max(nm, reinterpret_cast<const u32 *>(&A.ed[first + j])[2] & 0xFFFFu);
    const u32 n_max = wave_max_u32(nm);
    const float ks = gumbel_ks(P.gumbel_c_visit, P.gumbel_c_scale, n_max);
    u64 key = 0;
    float psp = 0.0f, psw = 0.0f;  // this lane's terms of the two sums, in edge order from 0 (an unvisited edge adds 0)
#pragma unroll 1
    for (int j = lane; j < M; j += WAVE) {
        const uint4 ev = A.ed[first + j];
        const u32 n = edge_visits(ev);
        const float pr = u2f(ev.x & PRIOR_MASK);
        if (n == n_max) {
            const u64 kk = gumbel_key(gumbel_score(ga[j], u2f(ev.y), n, ks), (u32)j);
            key = kk > key ? kk : key;
        }
        const float tw = n >= 1u ? pr * (u2f(ev.y) / (float)n) : 0.0f;
        psp = psp + (n >= 1u ? pr : 0.0f);
        psw = psw + tw;
    }
    key = wave_max_u64(key);
    chosen = key ? (int)(0xFFFFFFFFu - (u32)key) : 0;
    const float sp = wave_sum_f32(psp), sw = wave_sum_f32(psw);
    const float v_mix = gumbel_v_mix(P.gumbel_v0[g], N, sp, sw);
    float xm = -INFINITY;
#pragma unroll 1
    for (int j = lane; j < M; j += WAVE) {
        const uint4 ev = A.ed[first + j];
        const u32 n = edge_visits(ev);
        const float x = gumbel_target_logit(u2f(ev.x & PRIOR_MASK), n >= 1u ? u2f(ev.y) / (float)n : v_mix, ks);
        if (x > xm)
            xm = x;
    }
    const float x_max = wave_max_f32(xm);
    const u64 lt = (1ULL << lane) - 1ULL;
    int nd = 0;
#pragma unroll 1
    for (int j0 = 0; j0 < M; j0 += WAVE) {
        const int j = j0 + lane;
        u32 c = 0, word = 0;
        if (j < M) {
            const uint4 ev = A.ed[first + j];
            const u32 n = edge_visits(ev);
            c = gumbel_count(gumbel_target_logit(u2f(ev.x & PRIOR_MASK), n >= 1u ? u2f(ev.y) / (float)n : v_mix, ks), x_max);
            word = (u32)A.em[first + j] | (c << 16);
        }
        const u64 mask = __ballot(c != 0u);
        if (c != 0u)
            rec[REC_HDR_WORDS + nd + __popcll(mask & lt)] = word;
        nd += __popcll(mask);
    }
    // no count at all (gumbel_root's rule): the record carries the move played with 65535 and nothing else
    if (nd == 0 && M > 0) {
        if (lane == 0)
            rec[REC_HDR_WORDS] = (u32)A.em[first + chosen] | (65535u << 16);
        nd = 1;
    }
    return nd;
}

// OWN: the instantiation of the move-playing launch of its own, k_advance_list: the one that can record pruned counts (forced
// playouts), write a game's key word (random symmetry), and record the ply's value and resign (azh_engine_set_resign).  The
// tower kernels carry the
// other one: they have no register to spare for the pruning (a 16-bit tower went to scratch memory with it), so while forced
// playouts are on the device loop plays the queued moves in a k_advance_list launch of its own in front of the tower.
// The same goes for the key word of the random symmetry, one Philox block where a game begins: inlined in the tower kernels
// it sent k_tower2<1, false> and <2, false> to scratch memory (12 bytes per lane, 2 VGPR spills;
// profiles/random_symmetry.txt), so their instantiation starts games without it and that mode, too, plays its moves in
// k_advance_list.  The ply's value, the resign rule and its once-per-game counts live in the OWN instantiation alone for the
// same reason, and so does the ply's move temperature (tempered_choice), and the move and the improved policy of the Gumbel
// root search (gumbel_record).
template <bool OWN>
__device__ inline void advance_game(const EngineParams &P, int g, TreeLds &L)
{
    u16 *s_moves = L.moves;
    u32 *s_pref = L.pref;
    u64 *s_w = L.w;
    const int lane = lane_id();
    azh_game_state s = P.gs[g];
    // while (root.all_edge_visits < global_visits) step();  (:522-525)
    if (s.phase != 2)
        return;
    Arena A = arena_of(P, s.arena, g);
    Arena B = arena_of(P, 1 - s.arena, g);
    const uint4 rinfo = A.ni[0];
    const u32 first = rinfo.x;
    const int M = (int)(rinfo.y & 0xFFFFu);

    // sample_proportionally_to_visits (:495-506) on integer visit counts
    const Philox4 rr = philox(P.k0, P.k1, s.uid, (u32)s.ply, STREAM_SAMPLE, 0u);
    const u32 N = (u32)s.root_visits;
    const u32 r = (u32)(((u64)rr.v[0] * (u64)N) >> 32);
    u32 nv[4], ch[4], mvs[4];  // visits, child node, move of this lane's root edges
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = lane + 64 * k;
        uint4 ev = fresh_edge(0u);
        mvs[k] = 0;
        if (j < M) {
            ev = A.ed[first + j];
            mvs[k] = A.em[first + j];
        }
        nv[k] = edge_visits(ev);
        ch[k] = edge_child(ev);
    }
    int chosen = -1;
    if (P.flags & AZH_FLAG_SAMPLE_POW5) {
        // sample_with_exponential_weight (engine.py:532-548), exponent 5: weights (n/N)^5 over
        // edges with n >= max/2; the common 1/N^5 cancels, so the integers n^5 are exact.
        u64 mk = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            mk = (u64)nv[k] > mk ? (u64)nv[k] : mk;
        const u64 maxn = wave_max_u64(mk);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = lane + 64 * k;
            if (j < M) {
                const u64 n = nv[k];
                s_w[j] = (2 * n >= maxn) ? n * n * n * n * n : 0ull;
            }
        }
        wave_sync();
        if (lane == 0) {
            u64 T = 0;
            for (int j = 0; j < M; j++)
                T += s_w[j];
            const u64 R = ((u64)rr.v[0] << 32) | (u64)rr.v[1];
            const u64 rq = __umul64hi(R, T);
            u64 cum = 0;
            int c = -1;
            for (int j = 0; j < M; j++) {
                cum += s_w[j];
                if (c < 0 && cum > rq)
                    c = j;
            }
            s_pref[0] = (u32)c;
        }
        wave_sync();
        chosen = (int)s_pref[0];
        wave_sync();
    } else {
        // the ply's temperature (azh_engine_set_temperature), in k_advance_list's instantiation alone: an entry of 1 is the
        // draw below on the raw counts, any other one chooses on fixed-point weights
        bool tempered = false;
        if constexpr (OWN) {
            if (P.move_temperature != nullptr) {
                const float T = P.move_temperature[s.ply];
                if (T != 1.0f) {
                    tempered = true;
                    chosen = tempered_choice(nv, M, T, rr.v[0]);
                }
            }
        }
        if (!tempered) {
            u32 run = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                const int incl = wave_incl_scan((int)nv[k]);
                const u32 cum = run + (u32)incl;
                const u64 mask = __ballot(j < M && cum > r);
                if (chosen < 0 && mask)
                    chosen = 64 * k + (__ffsll((long long)mask) - 1);
                run += (u32)bcast_last(incl);
            }
        }
    }
    if (chosen < 0)
        chosen = 0;
    if (P.flags & AZH_FLAG_ONE_RANDOM_MOVE) {
        const int rp = random_ply_of(P, s.uid);
        if (s.ply == rp) {
            // AT the randomization point: a uniformly random legal move (:531-540)
            chosen = (int)(((u64)rr.v[1] * (u64)(u32)M) >> 32);
        } else if (s.ply > rp) {
            // AFTER it: the most visited move (:543-551), first maximum in movegen order
            u64 key = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                if (j < M) {
                    const u64 kk = ((u64)nv[k] << 32) | (u64)(0xFFFFFFFFu - (u32)j);
                    key = kk > key ? kk : key;
                }
            }
            key = wave_max_u64(key);
            chosen = (int)(0xFFFFFFFFu - (u32)key);
        }
    }

    // record the ply (:565-572): board, move, visit distribution over expanded edges — on a ply forced playouts act on
    // (the plies whose root got the noise) the pruned counts instead; the move above and the re-root below see the raw ones
    u32 *rec = P.rec + ((size_t)g * P.max_plies + s.ply) * REC_STRIDE_WORDS;
    const u64 lt = (1ULL << lane) - 1ULL;
    int nd = 0;
    bool pruned = false;
    bool gumbel = false;  // the Gumbel root search: the move and the counts are the mode's own (no draw is used)
    if constexpr (OWN) {
        pruned = P.forced_k != 0.0f && (ply_kind_of(P, g) & PLY_FULL) != 0u;
        gumbel = P.gumbel_m != 0;
        if (gumbel)
            nd = gumbel_record(P, A, first, M, N, g, rec, chosen);
    }
    if (gumbel) {
    } else if (pruned) {
        nd = record_pruned_counts(P, A, first, M, N, rec);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = lane + 64 * k;
            const bool has = j < M && ch[k] != ENONE;
            const u64 mask = __ballot(has);
            if (has)
                rec[REC_HDR_WORDS + nd + __popcll(mask & lt)] = mvs[k] | (nv[k] << 16);
            nd += __popcll(mask);
        }
    }
    const int ck = chosen >> 6, cl = chosen & 63;
    const u32 my_mv = ck == 0 ? mvs[0] : (ck == 1 ? mvs[1] : (ck == 2 ? mvs[2] : mvs[3]));
    const u32 my_ch = ck == 0 ? ch[0] : (ck == 1 ? ch[1] : (ck == 2 ? ch[2] : ch[3]));
    const u32 mv = (u32)read_lane((int)my_mv, cl);
    const u32 c = (P.flags & AZH_FLAG_NO_REUSE) ? ENONE : (u32)read_lane((int)my_ch, cl);  // arena engines rebuild the tree every ply
    const ulonglong2 rootw = A.nb[0];
    u32 w5 = 0;  // word 5 of the ply's record while the mode is on
    // The ply's value and the resign rule (azh_engine_set_resign): q = W_b / n_b of the most visited root edge b (ties: the
    // lowest index), one f32 division; a counted ply (not a FAST one) with q < resign_below advances the mover's counter,
    // any other counted ply resets it; the rule fires when the counter reaches resign_plies.
    bool resign = false;
    u32 mover = 0, rs_word = 0;
    if constexpr (OWN) {
        w5 = (P.fast_visits != 0 && (P.ply_kind[g] & PLY_FULL)) ? 1u : 0u;
        if (P.resign_plies != 0u) {
            u64 key = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                if (j < M) {
                    const u64 kk = ((u64)nv[k] << 32) | (u64)(0xFFFFFFFFu - (u32)j);
                    key = kk > key ? kk : key;
                }
            }
            key = wave_max_u64(key);
            const u32 n_b = (u32)(key >> 32);
            float q = 0.5f;
            if (n_b != 0u)
                q = u2f(reinterpret_cast<const u32 *>(&A.ed[first + (0xFFFFFFFFu - (u32)key)])[1]) / (float)n_b;
            // the rule sees q as the record holds it, without its sign (q >= 0 from any finite evaluator): a pure function of
            // the record, and neither a NaN nor an infinity of either sign is ever below
            q = u2f(f2u(q) & 0x7FFFFFFFu);
            mover = (rootw.x & TURN_BIT) ? 2u : 1u;
            rs_word = P.resign_state[g];
            if (n_b != 0u && (P.fast_visits == 0 || w5 != 0u)) {
                const u32 sh = mover == 1u ? 0u : 8u;
                u32 cnt = (rs_word >> sh) & 0xFFu;
                cnt = q < P.resign_below ? min(cnt + 1u, 255u) : 0u;
                rs_word = (rs_word & ~(0xFFu << sh)) | (cnt << sh);
                if (cnt >= P.resign_plies) {
                    if ((rs_word >> 16) == 0u)
                        rs_word |= mover << 16;
                    resign = !resign_playthrough(P.k0, P.k1, s.uid, P.resign_through);
                }
            }
            w5 = f2u(q) | (w5 << 31);
        }
    }
    if (lane == 0) {
        const u64 bx = rootw.x & ~TURN_BIT;
        rec[0] = (u32)bx;
        rec[1] = (u32)(bx >> 32);
        rec[2] = (u32)rootw.y;
        rec[3] = (u32)(rootw.y >> 32);
        rec[4] = (mv & 0xFFFFu) | ((u32)nd << 16);
        if constexpr (OWN)
            rec[5] = w5;
        else
            rec[5] = (P.fast_visits != 0 && (P.ply_kind[g] & PLY_FULL)) ? 1u : 0u;  // playout cap: 1 = searched in full
        rec[6] = 0;
        rec[7] = 0;
    }

    // MCTS::play (:475-492), the evaluation-cache rebuild, the arena flip
    RerootStats rs;
    int result;
    if (resign) {
        // the mover resigns: the ply above is the record's last, its move is not played, the game ends here
        result = 3 - (int)mover;
        s.ply += 1;
        __threadfence();
        wave_sync();
    } else {
        result = reroot_game(P, g, L, s, A, B, rootw, mv, c, rs);
    }
    const u64 st_nodes = rs.nodes, st_edges = rs.edges, st_spill = rs.spill;

    u64 st_games = 0, st_dropped = 0, st_ring = 0;
    const bool cut = result == 0 && s.ply >= P.max_plies;
    // ONE_RANDOM_MOVE: "Skipping game with no board state just after the uniformly random move" (:632-637)
    const bool no_sample = result != 0 && (P.flags & AZH_FLAG_ONE_RANDOM_MOVE) && random_ply_of(P, s.uid) + 1 >= s.ply;
    // A game that is dropped leaves an 8-word marker in the ring, so the host knows this uid will never come
    // (uid-ordered emission, azh_engine_set_emit_order).
    auto drop_marker = [&]() {
        u64 off = 0;
        if (lane == 0)
            off = atomicAdd((unsigned long long *)P.ring_head, 8ull);
        off = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(off >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)off);
        if (off + 8 > P.ring_cap_words) {
            st_ring = 1;
        } else if (lane == 0) {
            u32 *out = P.ring + off;
            out[0] = RING_MAGIC; out[1] = (u32)g; out[2] = s.uid; out[3] = (u32)s.ply;
            out[4] = 0; out[5] = 8; out[6] = 0; out[7] = 1;  // word 7: dropped
        }
    };
    const int loaded = P.no_emit[g] & NO_EMIT_PLY;  // start ply + 1 of a game that began at a loaded position, else 0
    const int p0 = loaded ? loaded - 1 : 0;     // first ply this game recorded
    u32 sets_word = 0;  // search settings per side: the pairing of the game that may end here (its successor's start overwrites it)
    if constexpr (OWN) {
        if (P.search_sets != nullptr)
            sets_word = P.slot_sets[g];
    }
    if (no_sample) {
        st_dropped = 1;
        drop_marker();
        init_game<OWN>(P, g, s.uid + (u32)P.G, s, s_moves);
    } else if (result != 0 || (cut && (P.flags & AZH_FLAG_KEEP_UNFINISHED))) {
        // finished: emit the packed record (generate_game :577-578, Worker :637-642)
        const u32 *recg = P.rec + (size_t)g * P.max_plies * REC_STRIDE_WORDS;
        int words = 0;
        for (int p = p0 + lane; p < s.ply; p += WAVE)
            words += 6 + (int)(recg[(size_t)p * REC_STRIDE_WORDS + 4] >> 16);
        words = wave_sum_int(words) + 8;
        u64 off = 0;
        if (lane == 0)
            off = atomicAdd((unsigned long long *)P.ring_head, (unsigned long long)words);
        off = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(off >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)off);
        if (off + (u64)words <= P.ring_cap_words) {
            u32 *out = P.ring + off;
            if (lane == 0) {
                out[0] = RING_MAGIC;
                out[1] = (u32)g;
                out[2] = s.uid;
                out[3] = (u32)(s.ply - p0);   // plies in the record
                out[4] = (u32)result;
                out[5] = (u32)words;
                out[6] = (P.flags & AZH_FLAG_ONE_RANDOM_MOVE) ? (u32)random_ply_of(P, s.uid) + 1u : 0u;
                out[7] = (loaded ? 2u : 0u)   // 2: partial game (begins at a loaded position): formatted by the host, not written
                         | (P.fast_visits != 0 ? REC_KIND_PLAYOUT_CAP : 0u) | (P.forced_k != 0.0f ? REC_KIND_FORCED : 0u);
                if constexpr (OWN) {
                    if (P.gumbel_m != 0)
                        out[7] |= REC_KIND_GUMBEL;
                    if (P.resign_plies != 0u) {
                        out[7] |= REC_KIND_VALUES | (resign ? REC_KIND_RESIGNED : 0u);
                        // once-per-game counts: resigned; play-through games that reached their end, those the rule fired
                        // in, and of those the ones the side it first fired for did not lose
                        const u32 fired = rs_word >> 16;
                        if (resign) {
                            atomicAdd((unsigned long long *)&P.resign_stats[AZH_RESIGN_STAT_RESIGNED], 1ull);
                        } else if (result != 0 && resign_playthrough(P.k0, P.k1, s.uid, P.resign_through)) {
                            atomicAdd((unsigned long long *)&P.resign_stats[AZH_RESIGN_STAT_PLAYTHROUGH], 1ull);
                            if (fired != 0u)
                                atomicAdd((unsigned long long *)&P.resign_stats[AZH_RESIGN_STAT_FIRED], 1ull);
                            if (fired != 0u && (u32)result != 3u - fired)
                                atomicAdd((unsigned long long *)&P.resign_stats[AZH_RESIGN_STAT_FALSE], 1ull);
                        }
                    }
                }
            }
            u32 pos = 8;
            for (int p = p0; p < s.ply; p++) {
                const u32 *rp = recg + (size_t)p * REC_STRIDE_WORDS;
                const u32 ndp = rp[4] >> 16;
                if (lane < 6)
                    out[pos + lane] = rp[lane];
                for (u32 j = lane; j < ndp; j += WAVE)
                    out[pos + 6 + j] = rp[REC_HDR_WORDS + j];
                pos += 6 + ndp;
            }
            st_games = cut ? 0 : 1;
        } else {
            st_ring = 1;
        }
        st_dropped = cut ? 1 : 0;  // arena: "invalid" -> annulled (uai_ringmaster.py:147-150)
        init_game<OWN>(P, g, s.uid + (u32)P.G, s, s_moves);
    } else if (cut) {
        st_dropped = 1;  // null-result games are skipped (:628-631)
        drop_marker();
        init_game<OWN>(P, g, s.uid + (u32)P.G, s, s_moves);
    } else {
        s.phase = 0;
        begin_ply(P, g, s.uid, s.ply);
        if constexpr (OWN) {
            if (P.resign_plies != 0u && lane == 0)
                P.resign_state[g] = rs_word;
        }
    }
    if constexpr (OWN) {
        // search settings per side: the once-per-game tally by (set of x, set of o), wherever the game was counted above
        if (P.search_sets != nullptr && (st_games | st_dropped) != 0 && lane == 0) {
            u64 *t = P.set_stats + ((size_t)(sets_word & 0xFFu) * (size_t)P.n_search_sets + (size_t)((sets_word >> 8) & 0xFFu)) *
                                       AZH_SET_STAT_COUNT;
            atomicAdd((unsigned long long *)&t[AZH_SET_STAT_GAMES], 1ull);
            if (cut)
                atomicAdd((unsigned long long *)&t[AZH_SET_STAT_UNDECIDED], 1ull);
            else if (result == 1 || result == 2)
                atomicAdd((unsigned long long *)&t[result == 1 ? AZH_SET_STAT_X_WINS : AZH_SET_STAT_O_WINS], 1ull);
        }
    }
    if (lane == 0) {
        P.force[g] = 0;
        P.gs[g] = s;
    }
    {
        const u64 inc = lane == AZH_STAT_PLIES ? 1ull
                      : lane == AZH_STAT_GAMES ? (u64)st_games
                      : lane == AZH_STAT_DROPPED ? (u64)st_dropped
                      : lane == AZH_STAT_RING_OVERFLOW ? (u64)st_ring
                      : lane == AZH_STAT_REROOT_NODES ? st_nodes
                      : lane == AZH_STAT_REROOT_EDGES ? st_edges
                      : lane == AZH_STAT_REROOT_SPILLS ? st_spill : 0ull;
        if (lane < NSTAT)
            add_stat(P, g, lane, inc);
    }
}

// The queued moves of one search iteration, played by `workers` workgroups of the tower launch (its first ones: at_head) that follows the
// tree launch which queued them (mark_game): worker w takes the games adv_list[w], adv_list[w + workers], ... (one wave; the
// workgroup's other waves return at once), the last worker to finish empties the queue.  `smem`: the workgroup's LDS (the
// tower's image: not in use by a worker).  The tree launch behind the tower finds every move played — same stream, kernel
// order — exactly as it did behind the side stream's k_advance_list.
struct AdvanceHook {
    int workers;      // 0: the launch plays no moves (evaluations outside the device loop)
    int at_head;      // 1: the workers are the launch's FIRST workgroups — a launch of more workgroups than the chip has slots,
                      // whose last ones wait for earlier ones to retire; 0: its last workgroups — a launch that fits the chip at
                      // once, where every workgroup starts at once anyway and workers in front would only push tiles onto CUs
                      // that already hold one (set per launch by the tower's launch functions)
    EngineParams P;
};

__device__ inline void advance_worker(const EngineParams &P, unsigned char *smem, int worker, int workers)
{
    TreeLds &L = *reinterpret_cast<TreeLds *>(smem);
    const int n = *P.adv_count;
    for (int i = worker; i < n; i += workers) {
        advance_game<false>(P, P.adv_list[i], L);
        wave_sync();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane_id() == 0 &&
        __hip_atomic_fetch_add(P.adv_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == workers - 1) {
        __hip_atomic_store(P.adv_count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(P.adv_done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace azh
