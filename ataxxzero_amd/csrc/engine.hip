// Batched MCTS self-play engine for gfx950: thousands of concurrent search trees
// resident in HBM as structure-of-arrays, one wavefront per game.
//
// Replaces the worker threads of the reference's cpp/self_play_client.cpp
// (file:line under /root/reference):
//   select_game   PUCT descent + expansion      MCTS::select_principal_variation :386-417,
//                                               MCTSNode::select_action :333-366,
//                                               total_action_score :310-324, step() :419-447
//   backup_game   priors, root noise, backup    Evaluations::populate :204-271, step() :449-459
//   mark_game     "is the move due?"            generate_game :522-525
//   advance_game  sample, record, re-root       sample_proportionally_to_visits :495-506,
//                                               generate_game :526-578, MCTS::play :475-492
//   k_play_moves  a move the host names          MCTS.play, engine.py:411-424 (the same re-root: reroot_game)
//   k_root_report root edges, principal line     MCTSEngine.genmove's report, engine.py:474-530
// Each game contributes exactly one leaf per search iteration, so the per-iteration evaluation
// batch is the number of concurrent games.  The device-resident loop (run_loop) runs an
// iteration as TWO launches on one stream — the fused tower, then k_tree = backup + mark + the
// next select + the leaf-list compaction, one wave per game, four games per workgroup — with the
// queued moves (advance_game, engine_device.h) played by the first workgroups of the tower launch.  The step-wise API
// (azh_engine_select / _backup, used by the lock-step parity tests and the reference ABI) launches
// the same k_tree one half at a time (enqueue_tree): mode 2 (select + compaction) -> k_advance_list ->
// (evaluator) -> mode 1 (backup + mark).
//
// HBM layout (per game, two ping-pong arenas so re-rooting compacts by copying):
//   node_board [2][G][node_cap]  16 B  x stones | turn<<63, o stones
//   node_info  [2][G][node_cap]  16 B  first_edge, n_edges | result<<16, -, terminal value
//   edge       [2][G][edge_cap]  16 B  prior f32 | total score f32 | visits u16, child node u16 | the child's edge
//                                       range: first_edge (23 bits), n_edges (8 bits), finished (1 bit) — a derived
//                                       copy of the child's node_info, so a PUCT level is ONE 16-byte load per child
//   edge_move  [2][G][edge_cap]   2 B  from | to<<8
// A node's children are one contiguous edge range, so PUCT reads them with a
// single coalesced 16-byte-per-lane load; children are bump-allocated by the one
// wave that owns the game (no atomics inside a tree).
//
// Determinism contract: given the same config and the same evaluator outputs the
// engine reproduces oracle/mcts_oracle.c bit for bit (ties -> last maximal edge,
// Philox-keyed randomness, fixed f32 operation order; compiled -ffp-contract=off).
#include <algorithm>
#include <map>

#include <hip/hip_ext.h>

#include "azh_device.h"
#include "azh_host.h"
#include "engine_device.h"

namespace azh {

// Games (one wave each) per workgroup of the fused tree kernel.  Up to 8192 games every game wave is resident at once (8
// waves per SIMD) and the number hardly matters (tree phase 0.084-0.086 ms for 1 / 2 / 4 at 4096 games); beyond that the
// waves come in rounds, and a workgroup gives its slots back only when its slowest game is done: at 16384 games 0.183 ms
// with one game per workgroup, 0.203 with 2, 0.222 with 4, 0.233 with 8, 0.311 with 16 (tools/tree_waves_sweep.sh,
// profiles/round3_tree_waves_sweep.txt; one game per workgroup needs the sharded tickets below: with a single ticket word
// it was the slowest at 0.253).  -DAZH_TREE_WAVES=n forces one value.
#ifdef AZH_TREE_WAVES
constexpr int TREE_WAVES_SMALL = AZH_TREE_WAVES, TREE_WAVES_LARGE = AZH_TREE_WAVES;
#else
constexpr int TREE_WAVES_SMALL = 4, TREE_WAVES_LARGE = 1;
#endif
constexpr int TREE_ONE_ROUND_GAMES = 8192;  // 8 waves x 4 SIMDs x 256 CUs
constexpr int TICKET_SHARDS = 64, TICKET_STRIDE = 32;
// stamps of the diagnostic k_tree<true> (azh_engine_tree_stamps): wave start, state loaded, backup done, mark done,
// descent done (leaf edge chosen / parked / terminal), expansion done, state stored, workgroup done (all four games)
constexpr int TREE_STAMPS = 10;  // + [8] levels descended, [9] children scanned in this launch

__device__ inline u64 tree_stamp()
{
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the phase's memory operations are part of the phase
    const u64 t = __builtin_amdgcn_s_memrealtime();  // 100 MHz, the same counter on every XCD (s_memtime is per XCD, shader clock)
    __builtin_amdgcn_sched_barrier(0);
    return t;
}

// azh_engine_set_positions: every slot restarts at a given position and ply (fresh tree, uid = slot).  Under a game limit
// the slots past it are loaded all the same and left idle, as k_limit_slots would leave them: either call order, one state.
__global__ __launch_bounds__(WAVE) void k_init_positions(EngineParams P, const ulonglong2 *boards, const int *plies)
{
    __shared__ u16 s_moves[MAX_MOVES];
    const int g = blockIdx.x;
    azh_game_state s;
    const ulonglong2 w = boards[g];
    // (under a start pool the slot plays on the walls of the uid it gets, its slot number)
    const u64 walls = P.pool ? P.pool[start_pool_entry((u32)g, P.pool_n, P.pool_stride)].blockers : P.blockers;
    init_game_at(P, g, (u32)g, s, s_moves, unpack_board(w.x, w.y), plies[g], 1, walls);
    if (P.uid_limit != 0u && (u32)g >= P.uid_limit)
        s.phase = 3;
    if (threadIdx.x == 0)
        P.gs[g] = s;
}

// azh_engine_set_game_limit: a slot whose game is past the limit and has not begun (game_unbegun) goes idle and keeps what it
// holds; an idle slot whose game is below a (raised) limit starts it — the loaded game it was idled with where it holds one
// (same root, ply and record start; the words a game's start writes are written again), else a fresh game at the start
// position.
__global__ __launch_bounds__(WAVE) void k_limit_slots(EngineParams P)
{
    __shared__ u16 s_moves[MAX_MOVES];
    const int g = blockIdx.x;
    azh_game_state s = P.gs[g];
    const int mark = P.no_emit[g];
    if (s.phase == 3 && s.uid < P.uid_limit) {
        if ((mark & NO_EMIT_LOADED) && game_unbegun(s, mark)) {
            begin_ply(P, g, s.uid, s.ply);
            begin_game_key(P, g, s.uid);
            s.phase = 0;
        } else {
            init_game(P, g, s.uid, s, s_moves);
        }
        if (threadIdx.x == 0)
            P.gs[g] = s;
    } else if (s.phase == 0 && game_unbegun(s, mark) && s.uid >= P.uid_limit) {  // (no root evaluation in flight either)
        if (threadIdx.x == 0)
            P.gs[g].phase = 3;
    }
}

// azh_engine_set_start_pool (before the first select): every slot starts its game again, from the entry of its uid
__global__ __launch_bounds__(WAVE) void k_restart(EngineParams P)
{
    __shared__ u16 s_moves[MAX_MOVES];
    const int g = blockIdx.x;
    azh_game_state s = P.gs[g];
    init_game(P, g, s.uid, s, s_moves);
    if (threadIdx.x == 0)
        P.gs[g] = s;
}

__global__ __launch_bounds__(WAVE) void k_init(EngineParams P)
{
    __shared__ u16 s_moves[MAX_MOVES];
    const int g = blockIdx.x;
    azh_game_state s;
    init_game(P, g, (u32)g, s, s_moves);
    if (threadIdx.x == 0)
        P.gs[g] = s;
    for (int k = threadIdx.x; k < NSTAT; k += WAVE)
        P.stats[(size_t)g * NSTAT + k] = 0;
}

// azh_engine_set_playout_cap: the kind of the ply every slot is at (one thread per slot)
__global__ void k_ply_kinds(EngineParams P)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < P.G)
        P.ply_kind[g] = playout_cap_full(P.k0, P.k1, P.gs[g].uid, (u32)P.gs[g].ply, P.full_per_65536) ? PLY_FULL
                                                                                                     : (u32)P.fast_visits;
}

// azh_engine_set_random_symmetry: the key word of the game every slot is at (one thread per slot)
__global__ void k_eval_keys(EngineParams P)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < P.G)
        P.eval_key[g] = eval_symmetry_key(P.k0, P.k1, P.gs[g].uid);
}

// azh_engine_set_search_sets: the pairing of the game every slot is at (one thread per slot)
__global__ void k_slot_sets(EngineParams P)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < P.G)
        P.slot_sets[g] = search_set_pairing(P.gs[g].uid, (u32)P.n_search_sets);
}

// The symmetry under which `node` of slot g's tree goes to the evaluator (0, the identity, while the mode is off): a function
// of the game's key word and the node's own board, so the select that sends the position, the backup that gathers its logits,
// the root's re-evaluation at a later ply and a transposition's source node all agree on it.  g, node: wave-uniform.
__device__ inline int eval_symmetry_at(const EngineParams &P, const Arena &A, int g, int node)
{
    if (P.random_symmetry == 0u)
        return 0;
    const ulonglong2 w = A.nb[node];
    const Board b = unpack_board(w.x, w.y);
    return __builtin_amdgcn_readfirstlane(eval_symmetry_of(P.eval_key[g], b.turn ? b.o : b.x, b.turn ? b.x : b.o));
}

// ------------------------------------------------------------------ select + expand

// Q + U of one edge (total_action_score :310-324) — IEEE division and square root in the fixed order the oracle restates.
// (Approximate division and square root, an upper bound of what precomputing q = W/n and r = cP/(1+n) at backup time could
// buy, did not pay for giving up bit-exactness: profiles/round5_puct_chain_ab.txt.)
__device__ inline float puct_score(float prior, float W, u32 n, float sq, float c_puct)
{
    prior = __builtin_fabsf(prior);  // (the sign bit may carry the descent's mark: a source modifier, no instruction)
    const float q = n ? W / (float)n : 0.0f;
    const float u = (sq / (1.0f + (float)n)) * (c_puct * prior);
    return u + q;
}

// `s` is the game's state, held in registers by the caller (the same values in all 64 lanes); written back here.
// Returns what the leaf needs: 0 nothing, 1 an evaluation (by net A), 2 an evaluation by net B (arena).  `pk`: the ply's kind
// word (forced playouts act on the plies whose root got the noise).
// POOL: the instantiation for an engine with a start pool (azh_engine_set_start_pool) — the expansion generates moves on the
// slot's own walls and the leaf's mask is written beside its board.  Without it no instruction of the kernel knows of the pool.
template <bool STAMP = false, bool POOL = false>
__device__ inline int select_game(const EngineParams &P, int g, azh_game_state &s, u16 *s_moves, u32 pk, u64 *st = nullptr)
{
    const int lane = lane_id();
    Arena A = arena_of(P, s.arena, g);
    int *path = P.path + (size_t)g * P.path_cap;

    int kind = AZH_LEAF_NONE, leaf_node = 0, depth = 0, over = 0;
    u64 st_steps = 0, st_evals = 0, st_levels = 0, st_children = 0, st_newmoves = 0, st_cached = 0, st_parked = 0;
    u64 leaf_mover = 0, leaf_opp = 0;

    if (s.phase >= 2) {
        // 2: the move of this game is due: its re-root runs after this select (the next tower launch's first workgroups), no leaf now
        // 3: the slot is idle (azh_engine_set_game_limit: every game it was to play has been played)
        kind = AZH_LEAF_NONE;
    } else if (s.phase == 0 && (P.flags & AZH_FLAG_TWO_NETS) && (A.ni[0].y & 0xFFFFu) == 1u) {
        // arena: a single legal move is played without search (uai_ringmaster.py:114-116)
        kind = AZH_LEAF_NONE;
        s.phase = 1;
        over = 2;  // sets the force flag without counting an overflow
    } else if (s.phase == 0) {
        // the root's priors are (re)computed with noise (:380-383, :485-490)
        kind = AZH_LEAF_ROOT;
        st_evals = 1;
        const ulonglong2 w = A.nb[0];
        const Board b = unpack_board(w.x, w.y);
        leaf_mover = b.turn ? b.o : b.x;
        leaf_opp = b.turn ? b.x : b.o;
    } else {
        // a descent parked by the level budget resumes at the node it stopped at (same tree: nothing of this
        // game was touched in between)
        const bool resume = s.leaf_kind == AZH_LEAF_DESCENT;
        st_steps = resume ? 0 : 1;
        u32 node = resume ? (u32)s.leaf_node : 0u;
        depth = resume ? s.path_len : 0;
        const uint4 rinfo = A.ni[node];
        // edge range of the node being scanned, in the packed form the edges carry for their children
        u32 kid = pack_kid(rinfo.x, rinfo.y & 0xFFFFu, (rinfo.y >> 16) != 0u);
        int levels_done = 0;
        // N of the node being scanned (the sum of its children's visits) without a wave reduction on the level's critical
        // path: for the root it is the game's root_visits; below, every visit of the edge into a node but the first —
        // the one that created the node — went on into one of its children, so N = that edge's visits - 1 (the
        // bookkeeping identity tests/test_gpu_engine.py checks at full size).  A resumed descent does not have the edge it
        // came through at hand and sums once.
        bool have_n = !resume;
        u32 n_node = (u32)s.root_visits;
        // sqrt(1 + N) of the node about to be scanned, computed as soon as N is known — at the END of the level above, while
        // the node's records are still on their way — instead of after their arrival: the IEEE square root (a dozen
        // instructions) leaves the chain between the arrival of a level's records and the request for the next level's.
        // Same function of the same argument: nothing the oracle could see (profiles/round5_sqrt_early_ab.txt).
        auto sqrt_1p = [](u32 n) {
            float r = sqrtf((float)(1u + n));
            asm volatile("" : "+v"(r));  // computed HERE (the optimiser would otherwise sink it to its use behind the wait)
            return r;
        };
        float sq_node = sqrt_1p(n_node);
        // The path of the descent: lane k keeps the k-th entry added in this launch and the entries are stored together
        // afterwards (every 64 levels when there is no budget): a store per level would have to be acknowledged before
        // the next level's records count as arrived (vmcnt counts stores in order with the loads).
        u32 path_buf = 0;
        int path_base = depth;
        auto push_path = [&](u32 eidx) {
            if (lane == depth - path_base)
                path_buf = eidx;
            depth++;
            if (depth - path_base == WAVE) {
                path[path_base + lane] = (int)path_buf;
                path_base = depth;
            }
        };
        // Early request of the next level (never changes what is selected): a node remembers which child the last descent
        // through it chose — the sign bit of that child's prior (priors are >= 0; one ballot finds it, and every node has
        // room for it, the fully visited nodes of the upper levels included; rounds 3-4 kept an index in the spare word of the
        // node's first unvisited edge instead: profiles/round5_hint_sign_ab.txt).  When a node's records arrive, the
        // remembered child's own records — its range is in this node's records — are requested at once and the scores are
        // computed while they are in flight; if the scores pick that child, the next level starts with its records
        // already on the way: a level then costs max(memory latency, its instructions) instead of their sum.
        // (two records per lane: nodes of up to 128 moves take this path — a third of the nodes of a mid-game position have
        // more than 64)
        // Two sets of record registers take turns without a register-to-register copy: a level that scans set a requests
        // the remembered child's records into set b; if the scores pick that child, the next level — a second copy of the
        // level's code — scans set b and requests into set a.  Only set a is ever live across the loop's back edge.
        uint4 ea0 = fresh_edge(0u), ea1 = fresh_edge(0u), eb0 = fresh_edge(0u), eb1 = fresh_edge(0u);
        bool cur_loaded = false;  // the records of the node about to be scanned have been requested (set a at the loop's head)
        // Every lane loads: lanes past the node's last edge read that last edge again (same cache line, no traffic) — no
        // lane mask around the load, so no register has to be cleared or merged per request; every use below is masked by
        // live0 / live1 or reads a lane the node's edge count has been checked against.  (cnt >= 1 at both call sites.)
        auto load_children = [&](u32 k, uint4 &r0, uint4 &r1) {
            const int cnt = kid_count(k);
            const u32 f = kid_first(k), last = (u32)cnt - 1u;
            r0 = A.ed[f + min((u32)lane, last)];
            if (cnt > WAVE)
                r1 = A.ed[f + min((u32)(lane + WAVE), last)];
        };
        u32 sel_eidx = 0;
        // One level of the fast path (all but a handful of nodes): one edge per lane, two beyond 64 moves.  Same arithmetic
        // as the general path below; the arg-max is a 32-bit max of the score bits plus ballots for the tie rule, instead of
        // a 64-bit (score, index) key reduction — this loop is a latency chain, instructions count.  Scans (c0, c1),
        // requests into (p0, p1).  true: descended into a child; false: the chosen edge has no child (sel_eidx: expand it).
        auto fast_level = [&](uint4 &c0, uint4 &c1, uint4 &p0, uint4 &p1, int M, u32 first) -> bool {
            if (!cur_loaded)
                load_children(kid, c0, c1);
            cur_loaded = false;
            const uint4 &e0 = c0, &e1 = c1;
            const bool two = M > WAVE;
            const bool live0 = lane < M, live1 = two && lane + WAVE < M;
            // the remembered child, requested before anything is scored
            int pv = -1, pred = -1;
            {
                // (a mark is only ever set on an edge whose child exists, is not a finished position and has 1 .. 128 moves
                // — below — and none of that changes while the edge lives: nothing to check here, one lane read)
                // (no live mask: a lane past the node's last edge holds a copy of that last edge, so the FIRST set bit is
                // always the marked edge itself — and a bare compare writes the lane mask without a detour through a register)
                const u64 mk0 = __ballot((int)e0.x < 0);
                const u64 mk1 = two ? __ballot((int)e1.x < 0) : 0ull;
                if (mk0 | mk1) {
                    pv = mk0 ? __ffsll((long long)mk0) - 1 : WAVE + __ffsll((long long)mk1) - 1;
                    const u32 pk = pv < WAVE ? (u32)read_lane((int)e0.w, pv) : (u32)read_lane((int)e1.w, pv - WAVE);
                    load_children(pk, p0, p1);
                    pred = pv;
                }
            }
            const u32 n0 = edge_visits(e0), n1 = edge_visits(e1);
            float sq1;
            if (have_n)
                sq1 = sq_node;
            else  // (have_n is false here; the inner test is kept because the instruction schedule changes without it)
                sq1 = sqrtf((float)(1u + (have_n ? n_node : wave_sum_u32((live0 ? n0 : 0u) + (live1 ? n1 : 0u)))));
            u32 bits0, bits1 = 0u;
            bool valid0, valid1 = false;
            {
                const float score = puct_score(u2f(e0.x), u2f(e0.y), n0, sq1, P.c_puct);
                valid0 = live0 && score >= 0.0f;  // NaN scores are never selected by either reference
                bits0 = valid0 ? f2u(score + 0.0f) : 0u;
            }
            if (two) {
                const float score = puct_score(u2f(e1.x), u2f(e1.y), n1, sq1, P.c_puct);
                valid1 = live1 && score >= 0.0f;
                bits1 = valid1 ? f2u(score + 0.0f) : 0u;
            }
            const u32 top = wave_max_u32(bits0 > bits1 ? bits0 : bits1);
            const u64 cand0 = __ballot(valid0 && bits0 == top);
            const u64 cand1 = two ? __ballot(valid1 && bits1 == top) : 0ull;
            int bj = 0;
            if (P.flags & AZH_FLAG_TIE_FIRST) {
                if (cand0)
                    bj = __ffsll((long long)cand0) - 1;
                else if (cand1)
                    bj = WAVE + __ffsll((long long)cand1) - 1;
            } else {
                if (cand1)
                    bj = WAVE + 63 - __clzll((long long)cand1);
                else if (cand0)
                    bj = 63 - __clzll((long long)cand0);
            }
            const u32 eidx = first + (u32)bj;
            push_path(eidx);
            // the chosen edge: visits | child << 16, and the child's range
            u32 zsel, wsel;
            if (bj < WAVE) {
                zsel = (u32)read_lane((int)e0.z, bj);
                wsel = (u32)read_lane((int)e0.w, bj);
            } else {
                zsel = (u32)read_lane((int)e1.z, bj - WAVE);
                wsel = (u32)read_lane((int)e1.w, bj - WAVE);
            }
            const u32 child = zsel >> 16;
            if (child == ENONE) {
                sel_eidx = eidx;
                return false;
            }
            // remember the choice (stored only when it changes)
            if (bj != pv) {
                // the mark moves: the lane that holds the edge chosen last time clears its prior's sign bit, the lane that
                // holds the newly chosen edge sets it.  Two predicated stores: bj and pv may be 64 apart, i.e. the two
                // edges of ONE lane — as one store with a per-lane choice of the edge that lane dropped its clear, and the
                // node kept two marks for good (found by the round-5 review; tests/test_gpu_engine.py reads the raw marks).
                // The mark moves in about one level of a hundred: the second store is not on the level's usual path.
                const bool markable = !kid_finished(wsel) && kid_count(wsel) > 0 && kid_count(wsel) <= 2 * WAVE;
                if (pv >= 0 && lane == (pv & 63))
                    reinterpret_cast<u32 *>(&A.ed[first + (u32)pv])[0] = (pv >= WAVE ? e1.x : e0.x) & PRIOR_MASK;
                if (markable && lane == (bj & 63))
                    reinterpret_cast<u32 *>(&A.ed[first + (u32)bj])[0] = (bj >= WAVE ? e1.x : e0.x) | ~PRIOR_MASK;
            }
            node = child;
            kid = wsel;
            n_node = (zsel & 0xFFFFu) - 1u;
            have_n = true;
            sq_node = sqrt_1p(n_node);  // (while the requested records are on their way)
            if (pred == bj)
                cur_loaded = true;  // the records requested before the scores were computed are the next level's
            return true;
        };
        // what every level starts with: the level budget, finished positions, the counters.  true: the descent ends here.
        int M = 0;
        u32 first = 0;
        auto level_begin = [&]() -> bool {
            if (P.select_budget != 0 && levels_done == P.select_budget) {
                kind = AZH_LEAF_DESCENT;  // park: no leaf for the evaluator from this game this iteration
                leaf_node = (int)node;
                st_parked = 1;
                return true;
            }
            levels_done++;
            M = kid_count(kid);
            first = kid_first(kid);
            if (kid_finished(kid) || M == 0) {
                kind = AZH_LEAF_TERMINAL;  // select_action -> NO_MOVE (:336-340)
                leaf_node = (int)node;
                return true;
            }
            st_levels += 1;
            st_children += (u64)M;
            return false;
        };
        // Forced playouts (azh_engine_set_forced_playouts; DESIGN.md, "Forced playouts and policy target pruning"): at the
        // root of a fresh descent on a ply whose root got the noise, an edge with n >= 1 visits and n < sqrt(k P N) is OWED a
        // visit and the descent takes it — among several the last in edge order, or the first (AZH_FLAG_TIE_FIRST) — instead
        // of the PUCT arg-max.  One wave-uniform branch in front of the loop: all four records per lane (a root has up to 256
        // edges) in the loop's record registers, which hold nothing yet; if an edge is owed, the root's level is done here
        // (path entry, counters, the mark exactly as fast_level moves it) and the loop starts at the child, else the loop
        // runs as it always has.  Nothing of it lives across the loop's back edge.
        if (P.forced_k != 0.0f && !resume && (pk & PLY_FULL) != 0u) {
            const int M0 = kid_count(kid);
            const u32 f0 = kid_first(kid);
            uint4 *const rp[4] = {&ea0, &ea1, &eb0, &eb1};
            u64 ow[4], mk[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                bool owed = false, marked = false;
                if (j < M0) {
                    const uint4 r = A.ed[f0 + j];
                    *rp[k] = r;
                    const u32 n = edge_visits(r);
                    owed = n >= 1u && edge_child(r) != ENONE && (float)n < forced_bound(P.forced_k, __builtin_fabsf(u2f(r.x)), n_node);
                    marked = (int)r.x < 0;
                }
                ow[k] = __ballot(owed);
                mk[k] = __ballot(marked);
            }
            int bj = -1, pv = -1;
            if (P.flags & AZH_FLAG_TIE_FIRST) {
#pragma unroll
                for (int k = 3; k >= 0; k--)
                    if (ow[k])
                        bj = 64 * k + __ffsll((long long)ow[k]) - 1;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (ow[k])
                        bj = 64 * k + 63 - __clzll((long long)ow[k]);
            }
            if (bj >= 0) {
#pragma unroll
                for (int k = 3; k >= 0; k--)
                    if (mk[k])
                        pv = 64 * k + __ffsll((long long)mk[k]) - 1;
                const int bk = bj >> 6;
                const u32 mz = bk == 0 ? ea0.z : (bk == 1 ? ea1.z : (bk == 2 ? eb0.z : eb1.z));
                const u32 mw = bk == 0 ? ea0.w : (bk == 1 ? ea1.w : (bk == 2 ? eb0.w : eb1.w));
                const u32 zsel = (u32)read_lane((int)mz, bj & 63), wsel = (u32)read_lane((int)mw, bj & 63);
                levels_done = 1;
                st_levels += 1;
                st_children += (u64)M0;
                push_path(f0 + (u32)bj);
                if (M0 <= 2 * WAVE && bj != pv) {  // (wider nodes carry no mark: the general level never sets one)
                    const bool markable = !kid_finished(wsel) && kid_count(wsel) > 0 && kid_count(wsel) <= 2 * WAVE;
                    if (pv >= 0 && lane == (pv & 63))
                        reinterpret_cast<u32 *>(&A.ed[f0 + (u32)pv])[0] = (pv >= WAVE ? ea1.x : ea0.x) & PRIOR_MASK;
                    if (markable && lane == (bj & 63))
                        reinterpret_cast<u32 *>(&A.ed[f0 + (u32)bj])[0] = (bj >= WAVE ? ea1.x : ea0.x) | ~PRIOR_MASK;
                }
                node = zsel >> 16;
                kid = wsel;
                n_node = (zsel & 0xFFFFu) - 1u;
                sq_node = sqrt_1p(n_node);
            }
        }
        bool expand = false;
        // Gumbel root search (azh_engine_set_gumbel; DESIGN.md, "Gumbel root search with sequential halving"): at the root of
        // a fresh descent the edge with exactly cv visits — the entry of the sequential-halving schedule for this simulation —
        // and the greatest a + ks q is taken, the lowest index among equal scores, in place of the PUCT arg-max.  The shape of
        // the forced-playout branch above: four records per lane in the loop's record registers, every lane keeps the child
        // data of its own best edge (the winning lane's best is the winner), the root's level is done here — path entry,
        // counters, the mark as fast_level moves it — and the loop starts at the child, or is skipped when the edge has no
        // child yet (a first visit: the expansion below).  No edge with cv visits (or a root past the schedule's end, after
        // azh_engine_set_visits lowered the threshold): the loop runs as it always has.
        if (P.gumbel_m != 0 && !resume && kid_count(kid) > 0 && n_node < (u32)P.visits) {
            const int M0 = kid_count(kid);
            const u32 f0 = kid_first(kid);
            const u32 cv = P.gumbel_seq[(size_t)(min(P.gumbel_m, M0) - 1) * (size_t)P.visits + n_node];
            const float *ga = P.gumbel_a + (size_t)g * MAX_MOVES;
            uint4 *const rp[4] = {&ea0, &ea1, &eb0, &eb1};
            u64 mk[4];
            float av[4];
            u32 nmx = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                bool marked = false;
                av[k] = 0.0f;
                if (j < M0) {
                    const uint4 r = A.ed[f0 + j];
                    *rp[k] = r;
                    av[k] = ga[j];
                    nmx = max(nmx, edge_visits(r));
                    marked = (int)r.x < 0;
                }
                mk[k] = __ballot(marked);
            }
            const float ks = gumbel_ks(P.gumbel_c_visit, P.gumbel_c_scale, wave_max_u32(nmx));
            u64 key = 0;
            u32 mine = 0, mkid = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                if (j < M0 && edge_visits(*rp[k]) == cv) {
                    const u64 kj = gumbel_key(gumbel_score(av[k], u2f(rp[k]->y), cv, ks), (u32)j);
                    if (kj > key) {
                        key = kj;
                        mine = rp[k]->z;
                        mkid = rp[k]->w;
                    }
                }
            }
            key = wave_max_u64(key);
            if (key) {
                const int bj = (int)(0xFFFFFFFFu - (u32)key);
                const u32 zsel = (u32)read_lane((int)mine, bj & 63), wsel = (u32)read_lane((int)mkid, bj & 63);
                levels_done = 1;
                st_levels += 1;
                st_children += (u64)M0;
                push_path(f0 + (u32)bj);
                if ((zsel >> 16) == ENONE) {
                    sel_eidx = f0 + (u32)bj;
                    expand = true;
                } else {
                    int pv = -1;
#pragma unroll
                    for (int k = 3; k >= 0; k--)
                        if (mk[k])
                            pv = 64 * k + __ffsll((long long)mk[k]) - 1;
                    if (M0 <= 2 * WAVE && bj != pv) {  // (wider nodes carry no mark: the general level never sets one)
                        const bool markable = !kid_finished(wsel) && kid_count(wsel) > 0 && kid_count(wsel) <= 2 * WAVE;
                        if (pv >= 0 && lane == (pv & 63))
                            reinterpret_cast<u32 *>(&A.ed[f0 + (u32)pv])[0] = (pv >= WAVE ? ea1.x : ea0.x) & PRIOR_MASK;
                        if (markable && lane == (bj & 63))
                            reinterpret_cast<u32 *>(&A.ed[f0 + (u32)bj])[0] = (bj >= WAVE ? ea1.x : ea0.x) | ~PRIOR_MASK;
                    }
                    node = zsel >> 16;
                    kid = wsel;
                    n_node = (zsel & 0xFFFFu) - 1u;
                    sq_node = sqrt_1p(n_node);
                }
            }
        }
        if (!expand)
        for (;;) {
            if (level_begin())
                break;
            if (M <= 2 * WAVE) {
                if (!fast_level(ea0, ea1, eb0, eb1, M, first)) {
                    expand = true;
                    break;
                }
                if (!cur_loaded)
                    continue;  // (the next level requests its records itself, into set a)
                // the remembered child was chosen: its records are on their way into set b (it has 1 .. 128 moves)
                if (level_begin())
                    break;
                if (!fast_level(eb0, eb1, ea0, ea1, M, first)) {
                    expand = true;
                    break;
                }
                continue;  // (cur_loaded: set a holds the next level's records)
            } else {
            const int rounds = (M + 63) >> 6;
            uint4 *const evp[4] = {&ea0, &ea1, &eb0, &eb1};  // the fast path's record registers (whatever they held is dead:
#define ev(k) (*evp[k])                                        // cur_loaded is cleared below)
            u32 nsum = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                if (k < rounds && j < M) {
                    ev(k) = A.ed[first + j];
                    nsum += edge_visits(ev(k));
                }
            }
            const u32 ntot = have_n ? n_node : wave_sum_u32(nsum);
            const float sq = have_n ? sq_node : sqrtf((float)(1u + ntot));
            // arg-max with ties to the LAST maximal edge (:354) — or the FIRST, python's max()
            // (engine.py:291), in the arena: scores are >= 0, so their bit patterns order like
            // the floats and (bits << 32 | index or ~index) is a total order; NaN scores (never
            // selected by either reference) and empty lanes map to key 0.
            const u32 tie_flip = (P.flags & AZH_FLAG_TIE_FIRST) ? 0xFFFFFFFFu : 0u;
            // every lane keeps the child data of its own best edge: the winning lane's best IS the winner, so
            // no array is indexed by the (run-time) round of the winner (that put the arrays in scratch memory
            // and a scratch round trip into every level)
            u64 key = 0;
            u32 mine = ev(0).z, mkid = ev(0).w;  // (lane 0 always holds edge 0: the key-0 default below)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                if (k < rounds && j < M) {
                    const float score = puct_score(u2f(ev(k).x), u2f(ev(k).y), edge_visits(ev(k)), sq, P.c_puct);
                    const u64 kj = score >= 0.0f ? (((u64)f2u(score + 0.0f)) << 32) | (u64)((u32)j ^ tie_flip) : 0ull;
                    if (kj > key) {
                        key = kj;
                        mine = ev(k).z;
                        mkid = ev(k).w;
                    }
                }
            }
#undef ev
            key = wave_max_u64(key);
            const int bj = key ? (int)((u32)key ^ tie_flip) : 0;  // key 0: edge 0 = lane 0's round-0 default
            const u32 eidx = first + (u32)bj;
            push_path(eidx);
            const u32 zsel = (u32)read_lane((int)mine, bj & 63);
            const u32 child = zsel >> 16;
            if (child != ENONE) {
                node = child;
                kid = (u32)read_lane((int)mkid, bj & 63);
                n_node = (zsel & 0xFFFFu) - 1u;
                have_n = true;
                sq_node = sqrt_1p(n_node);
                cur_loaded = false;
                continue;
            }
            sel_eidx = eidx;
            expand = true;
            break;
            }
        }
        if (expand) {
            // expand (:429-439)
            if constexpr (STAMP) st[4] = tree_stamp();
            const u32 eidx = sel_eidx;
            const u32 mv = A.em[eidx];
            const ulonglong2 pw = A.nb[node];
            const Board cb = make_move(unpack_board(pw.x, pw.y), (int)(mv & 0xFF), (int)(mv >> 8));
            int res2;
            const int M2 = wave_movegen(cb, POOL ? P.slot_mask[g] : P.blockers, s_moves, &res2);
            wave_sync();
            if (s.n_nodes >= P.node_cap || (res2 == 0 && (s.n_edges + M2 > P.edge_cap || M2 > 255))) {
                over = 1;
                kind = AZH_LEAF_NONE;
                leaf_node = 0;
                depth = 0;
            } else {
            const u32 cid = (u32)s.n_nodes;
            s.n_nodes += 1;
            u32 known = NONE;  // a node of this tree that already carries the evaluation of this position
            if ((P.flags & AZH_FLAG_EVAL_CACHE) && res2 == 0)
                known = tt_lookup(tt_of(P, s.arena, g), (u32)P.tt_size - 1u, A, pack_word0(cb), cb.o);
            if (res2 != 0) {
                float tv = res2 == 1 ? 1.0f : -1.0f;
                if (cb.turn == 1)
                    tv = -tv;
                if (lane == 0)
                    A.ni[cid] = make_uint4(0u, (u32)res2 << 16, 0u, f2u(tv));
                kind = AZH_LEAF_TERMINAL;
            } else if (known != NONE) {
                // same position, same moves in the same order: take the priors and the value, no evaluation
                const uint4 kinfo = A.ni[known];
                const u32 nf = (u32)s.n_edges;
                for (int j = lane; j < M2; j += WAVE) {
                    A.ed[nf + j] = fresh_edge(A.ed[kinfo.x + j].x & PRIOR_MASK);  // (without the other node's mark)
                    A.em[nf + j] = s_moves[j];
                }
                s.n_edges += M2;
                if (lane == 0)
                    A.ni[cid] = make_uint4(nf, (u32)M2, 0u, kinfo.w);
                kind = AZH_LEAF_TERMINAL;  // "value known": backed up from node_info.w like a finished position
                st_cached = 1;
                st_newmoves = (u64)M2;
            } else {
                const u32 nf = (u32)s.n_edges;
                for (int j = lane; j < M2; j += WAVE) {
                    A.ed[nf + j] = fresh_edge(0u);
                    A.em[nf + j] = s_moves[j];
                }
                s.n_edges += M2;
                if (lane == 0)
                    A.ni[cid] = make_uint4(nf, (u32)M2, 0u, 0u);
                kind = AZH_LEAF_EVAL;
                st_evals = 1;
                st_newmoves = (u64)M2;
            }
            if (lane == 0) {
                A.nb[cid] = make_ulonglong2(pack_word0(cb), cb.o);
                // the edge gets its child (an edge without a child has no visits: the first one creates it) and the child's range
                reinterpret_cast<uint2 *>(&A.ed[eidx])[1] =
                    make_uint2(cid << 16, res2 != 0 ? pack_kid(0u, 0u, 1u) : pack_kid((u32)(s.n_edges - M2), (u32)M2, 0u));
            }
            leaf_node = (int)cid;
            leaf_mover = cb.turn ? cb.o : cb.x;
            leaf_opp = cb.turn ? cb.x : cb.o;
            }
        }
        // the path entries of this launch, one store for all of them (none after an overflow: depth is 0 then)
        if (lane < depth - path_base)
            path[path_base + lane] = (int)path_buf;
    }

    s.leaf_kind = kind;
    s.leaf_node = leaf_node;
    s.path_len = depth;
    if constexpr (STAMP) {
        st[5] = tree_stamp();
        if (st[4] == 0)
            st[4] = st[5];  // no expansion: the descent ended at a finished position, parked, or there was none
        st[8] = st_levels;
        st[9] = st_children;
    }
    int need = (kind == AZH_LEAF_EVAL || kind == AZH_LEAF_ROOT) ? 1 : 0;
    if (need && (P.flags & AZH_FLAG_TWO_NETS))
        need = 1 + ((s.ply + g) & 1);  // net A (1) / net B (2) is to move; even slots give x to A
    if (P.random_symmetry != 0u && need)  // the evaluator sees the position's image (the node keeps the position itself)
        wave_symmetry_boards(eval_symmetry_of(P.eval_key[g], leaf_mover, leaf_opp), leaf_mover, leaf_opp);
    if (lane == 0) {
        P.gs[g] = s;
        P.need_eval[g] = need;
        P.leaf_board[g] = make_ulonglong2(leaf_mover, leaf_opp);
        if constexpr (POOL)
            P.leaf_mask[g] = P.slot_mask[g];
        if (over)
            P.force[g] = 1;
    }
    {   // counters: lane k owns counter k, one read-modify-write round trip for all of them
        const u64 inc = lane == AZH_STAT_STEPS ? st_steps
                      : lane == AZH_STAT_NN_EVALS ? st_evals
                      : lane == AZH_STAT_LEVELS ? st_levels
                      : lane == AZH_STAT_CHILDREN ? st_children
                      : lane == AZH_STAT_NEW_MOVES ? st_newmoves
                      : lane == AZH_STAT_EDGE_OVERFLOW ? (u64)(over == 1)
                      : lane == AZH_STAT_CACHE_HITS ? st_cached
                      : lane == AZH_STAT_PARKED ? st_parked : 0ull;
        if (lane < NSTAT)
            add_stat(P, g, lane, inc);
    }
    return need;
}

// ------------------------------------------------------------------ priors + backup

// Evaluations::populate (:204-271): the priors of `node` from one row of logits — a softmax over the legal moves' logits,
// identical to the reference's 833-way softmax renormalised over the legal moves — then, at the root (`root`: the root of a
// ply that gets noise — every ply, or with the playout cap on the FULL ones), the Dirichlet mix keyed by (uid, ply).
// `sym` (wave-uniform; eval_symmetry_at): the row holds the logits of the position's image under that symmetry, so a move's
// logit is the one of its image; 0: the row is the position's own.  Wave-cooperative.
__device__ inline void apply_priors(const EngineParams &P, const Arena &A, int node, const float *row, bool root, u32 uid,
                                    u32 ply, int sym)
{
    const int lane = lane_id();
    const auto logit_index = [sym](u32 mv) { return policy_index(sym != 0 ? symmetry_move(sym, mv) : mv); };
    {
        const uint4 info = A.ni[node];
        const u32 first = info.x;
        const int M = (int)(info.y & 0xFFFFu);
        const int rounds = (M + 63) >> 6;
        float l[4], ex[4];
        float pr[4];
        if (P.flags & AZH_FLAG_PY_POSTERIOR) {
            // engine.py:197-203: softmax over all 833 logits, gather the legal moves, divide by
            // (their sum + 1e-6)
            float mx = -INFINITY, S;
            if (sym != 0) {
                // The row holds the image's logits: they are summed in the POSITION's index order (row[T_s(i)] for i ascending),
                // the same terms in the same order as over a row brought back through the permutation — the f32 sum is
                // invariant under a permutation only in exact arithmetic, and the priors are part of the bit-exact contract.
                // Two rolled passes (the maximum does not depend on the order): the index map is not worth 14 copies.
#pragma unroll 1
                for (int i = lane; i < AZH_POLICY_SIZE; i += WAVE) {
                    const float v = row[i];
                    if (v > mx)
                        mx = v;
                }
                mx = wave_max_f32(mx);
                float part = 0.0f;
#pragma unroll 1
                for (int i = lane; i < AZH_POLICY_SIZE; i += WAVE)
                    part = part + det_expf(row[symmetry_policy_index(sym, i)] - mx);
                S = wave_sum_f32(part);
            } else {
                float la[14];
#pragma unroll
                for (int t = 0; t < 14; t++) {
                    const int i = lane + 64 * t;
                    la[t] = i < AZH_POLICY_SIZE ? row[i] : -INFINITY;
                    if (la[t] > mx)
                        mx = la[t];
                }
                mx = wave_max_f32(mx);
                float part = 0.0f;
#pragma unroll
                for (int t = 0; t < 14; t++)
                    if (lane + 64 * t < AZH_POLICY_SIZE)
                        part = part + det_expf(la[t] - mx);
                S = wave_sum_f32(part);
            }
            float lpart = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                ex[k] = 0.0f;
                if (k < rounds && j < M) {
                    ex[k] = det_expf(row[logit_index(A.em[first + j])] - mx) / S;
                    lpart = lpart + ex[k];
                }
            }
            const float den = wave_sum_f32(lpart) + 1e-6f;
#pragma unroll
            for (int k = 0; k < 4; k++)
                pr[k] = ex[k] / den;
        } else {
            // the root policy's temperature (azh_engine_set_temperature): at the root of a noise ply whose entry R is not 1
            // every legal move's logit is multiplied by 1 / R before the maximum is taken; the multiply by 1.0f everywhere
            // else leaves every logit's bits as they are
            float inv = 1.0f;
            if (root && P.root_policy_temperature != nullptr) {
                const float R = P.root_policy_temperature[ply];
                if (R != 1.0f)
                    inv = 1.0f / R;
            }
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                l[k] = -INFINITY;
                if (k < rounds && j < M) {
                    l[k] = row[logit_index(A.em[first + j])] * inv;
                    if (l[k] > mx)
                        mx = l[k];
                }
            }
            mx = wave_max_f32(mx);
            float part = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                ex[k] = 0.0f;
                if (k < rounds && j < M) {
                    ex[k] = det_expf(l[k] - mx);
                    part = part + ex[k];
                }
            }
            const float S = wave_sum_f32(part);
#pragma unroll
            for (int k = 0; k < 4; k++)
                pr[k] = S > 0.0f ? ex[k] / S : ex[k];
        }
        if (root && P.noise_w > 0.0f) {
            float gm[4];
            float gpart = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int j = lane + 64 * k;
                gm[k] = 0.0f;
                if (k < rounds && j < M) {
                    gm[k] = det_gamma(P.alpha, P.k0, P.k1, uid, ply, (u32)j);
                    gpart = gpart + gm[k];
                }
            }
            const float T = wave_sum_f32(gpart);
            const float w = P.noise_w, omw = 1.0f - w;
            if (T > 0.0f) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float d = gm[k] / T;
                    const float t1 = w * d;
                    const float t2 = omw * pr[k];
                    pr[k] = t1 + t2;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = lane + 64 * k;
            if (k < rounds && j < M)  // (stored without a sign: bit 31 is the descent's mark.  Priors are >= 0 and never NaN —
                                      // det_expf is 0 for a NaN argument — so the mask changes nothing: belt and braces)
                reinterpret_cast<u32 *>(&A.ed[first + j])[0] = f2u(pr[k]) & PRIOR_MASK;
        }
    }
}

// `s`: the game's state in the caller's registers (uniform over the lanes); updated, not stored.  `pk`: the ply's kind word.
__device__ inline void backup_game(const EngineParams &P, int g, azh_game_state &s, u32 pk)
{
    const int lane = lane_id();
    const int kind = s.leaf_kind;
    if (kind == AZH_LEAF_NONE || kind == AZH_LEAF_DESCENT)
        return;  // nothing evaluated; a parked descent keeps its state
    Arena A = arena_of(P, s.arena, g);

    if (kind == AZH_LEAF_EVAL || kind == AZH_LEAF_ROOT)
        apply_priors(P, A, s.leaf_node, P.logits + (size_t)g * AZH_POLICY_SIZE, kind == AZH_LEAF_ROOT && (pk & PLY_FULL) != 0u,
                     s.uid, (u32)s.ply, eval_symmetry_at(P, A, g, s.leaf_node));

    if (P.gumbel_m != 0 && kind == AZH_LEAF_ROOT) {
        // Gumbel root search: a_j = g_j + l_j of every root edge from the prior just stored (each lane reads back what it
        // wrote itself), and the root's own value as a score; the ply's select and its move read both
        const uint4 rinfo = A.ni[0];
        const int M = (int)(rinfo.y & 0xFFFFu);
        float *ga = P.gumbel_a + (size_t)g * MAX_MOVES;
#pragma unroll 1
        for (int j = lane; j < M; j += WAVE) {
            u32 jv = (u32)j;
            asm volatile("" : "+v"(jv));  // (the Philox block in vector registers, as begin_ply)
            const float l = gumbel_logit(u2f(reinterpret_cast<const u32 *>(&A.ed[rinfo.x + j])[0] & PRIOR_MASK));
            ga[j] = gumbel_noise(P.k0, P.k1, s.uid, (u32)s.ply, jv) + l;
        }
        if (lane == 0)
            P.gumbel_v0[g] = (P.values[g] + 1.0f) * 0.5f;
    }
    if ((P.flags & AZH_FLAG_EVAL_CACHE) && kind == AZH_LEAF_EVAL) {
        // the leaf now carries an evaluation: remember its value and enter it in the table
        if (lane == 0) {
            reinterpret_cast<u32 *>(&A.ni[s.leaf_node])[3] = f2u(P.values[g]);
            const ulonglong2 b = A.nb[s.leaf_node];
            tt_insert(tt_of(P, s.arena, g), (u32)P.tt_size - 1u, b.x, b.y, (u32)s.leaf_node);
        }
    }
    if (kind == AZH_LEAF_EVAL || kind == AZH_LEAF_TERMINAL) {
        // step() part 4 (:449-459): flip the score at every edge on the way up.
        const float v = kind == AZH_LEAF_EVAL ? P.values[g] : u2f(A.ni[s.leaf_node].w);
        const float sc0 = (v + 1.0f) * 0.5f;
        const float fa = 1.0f - sc0, fb = 1.0f - fa, fc = 1.0f - fb;
        const int *path = P.path + (size_t)g * P.path_cap;
        for (int i = lane; i < s.path_len; i += WAVE) {
            const int flips = s.path_len - i;
            const float val = flips == 1 ? fa : ((flips & 1) ? fc : fb);
            u32 *e = reinterpret_cast<u32 *>(&A.ed[path[i]]);
            e[1] = f2u(u2f(e[1]) + val);
            e[2] += 1u;  // visits: the low half of the word (<= 60000, never carries into the child id)
        }
        if (s.path_len > 0)
            s.root_visits += 1;
    }
    if (kind == AZH_LEAF_ROOT)
        s.phase = 1;
    s.leaf_kind = AZH_LEAF_NONE;
}

// The tree phases (backup_game, mark_game, select_game) run in one kernel, k_tree below, for the device-resident loop
// and the step-wise API alike; only the queued re-roots have a kernel of their own (k_advance_list).

// while (root.all_edge_visits < global_visits) step();  (:522-525): once the threshold is reached the move is due.
// The game is only MARKED here (phase 2) and queued; the next select gives it no leaf, and the re-root
// (advance_game) then runs from the queue in the first workgroups of the next tower launch (or in a k_advance_list launch
// of its own in front of it), beside the tower of the other games — a deep
// subtree copy (one dependent round trip per tree level) no longer sits on every iteration's critical path.
// `forced`: force[g], loaded by the caller beside the state; `pk`: the ply's kind word (playout cap: a FAST ply's move is
// due at fast_visits).
// mark_game_at: the same with the threshold given (k_vl_tree: the visits of the ply's search set).
__device__ inline void mark_game_at(const EngineParams &P, int g, azh_game_state &s, int forced, int threshold)
{
    if (s.phase == 1 && s.leaf_kind != AZH_LEAF_DESCENT && (s.root_visits >= threshold || forced != 0)) {
        s.phase = 2;
        if (lane_id() == 0)
            P.adv_list[atomicAdd(P.adv_count, 1)] = g;
    }
}

__device__ inline void mark_game(const EngineParams &P, int g, azh_game_state &s, int forced, u32 pk)
{
    mark_game_at(P, g, s, forced, ply_threshold(P, pk));
}

__global__ __launch_bounds__(WAVE) void k_advance_list(EngineParams P)
{
    __shared__ TreeLds L;
    const int n = *P.adv_count;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        advance_game<true>(P, P.adv_list[i], L);
        wave_sync();
    }
    // the workgroup that finishes last empties the queue (every workgroup has read the count by then): no memset
    // command behind the kernel, and the kernel's own completion is the event the next tree launch waits for
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (threadIdx.x == 0 &&
        __hip_atomic_fetch_add(P.adv_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
        __hip_atomic_store(P.adv_count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(P.adv_done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// azh_engine_play_moves: the host names the move of every game (0xFFFF: none), one wave per game.  The move is looked up
// among the root's edges and played through reroot_game — the re-root of advance_game without its sampling, its ply record
// and its game bookkeeping: no random number, no record, AZH_STAT_PLIES untouched, and the game never becomes a line
// (no_emit, as a loaded position).  A game whose own move was due (phase 2) stays in the move queue until
// k_unqueue_played, launched behind this kernel, takes it out.
__global__ __launch_bounds__(WAVE) void k_play_moves(EngineParams P, const u16 *moves, int *status)
{
    __shared__ TreeLds L;
    const int g = blockIdx.x, lane = lane_id();
    const u32 want = moves[g];
    if (want == 0xFFFFu) {
        if (lane == 0)
            status[g] = AZH_PLAY_NONE;
        return;
    }
    azh_game_state s = P.gs[g];
    if (s.phase == 3) {
        if (lane == 0)
            status[g] = AZH_PLAY_BUSY;
        return;
    }
    Arena A = arena_of(P, s.arena, g);
    Arena B = arena_of(P, 1 - s.arena, g);
    const uint4 rinfo = A.ni[0];
    const u32 first = rinfo.x;
    const int M = (int)(rinfo.y & 0xFFFFu);  // (0 at a finished root: every move is refused)
    int chosen = -1;
    u32 child = ENONE;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = lane + 64 * k;
        u32 ch = ENONE;
        bool hit = false;
        if (j < M) {
            hit = (u32)A.em[first + j] == want;
            ch = edge_child(A.ed[first + j]);
        }
        const u64 mask = __ballot(hit);
        if (chosen < 0 && mask) {
            const int l = __ffsll((long long)mask) - 1;
            chosen = 64 * k + l;
            child = (u32)read_lane((int)ch, l);
        }
    }
    if (chosen < 0) {
        if (lane == 0)
            status[g] = AZH_PLAY_ILLEGAL;
        return;
    }
    const u32 c = (P.flags & AZH_FLAG_NO_REUSE) ? ENONE : child;
    RerootStats rs;
    const int result = reroot_game(P, g, L, s, A, B, A.nb[0], want, c, rs);
    s.ply = min(s.ply, P.max_plies - 1);
    begin_ply(P, g, s.uid, s.ply);
    s.phase = result != 0 ? 3 : 0;
    s.leaf_kind = AZH_LEAF_NONE;  // (a descent parked by select_budget is given up with the tree it was in)
    s.leaf_node = 0;
    s.path_len = 0;
    if (lane == 0) {
        P.force[g] = 0;
        P.no_emit[g] = s.ply + 1;
        P.gs[g] = s;
        status[g] = result != 0 ? AZH_PLAY_FINISHED : (c == ENONE ? AZH_PLAY_FRESH : AZH_PLAY_KEPT);
    }
    const u64 inc = lane == AZH_STAT_REROOT_NODES ? rs.nodes
                  : lane == AZH_STAT_REROOT_EDGES ? rs.edges
                  : lane == AZH_STAT_REROOT_SPILLS ? rs.spill : 0ull;
    if (lane < NSTAT)
        add_stat(P, g, lane, inc);
}

// Behind k_play_moves: the move queue keeps, in their order, the games whose own move is still due (one wave).
__global__ __launch_bounds__(WAVE) void k_unqueue_played(EngineParams P)
{
    const int lane = lane_id();
    const int n = *P.adv_count;
    const u64 lt = (1ULL << lane) - 1ULL;
    int kept = 0;
    for (int base = 0; base < n; base += WAVE) {
        const int i = base + lane;
        int g = 0;
        bool keep = false;
        if (i < n) {
            g = P.adv_list[i];
            keep = P.gs[g].phase == 2;
        }
        const u64 mask = __ballot(keep);  // (every lane's load has returned: the stores below land at or before `base`)
        if (keep)
            P.adv_list[kept + __popcll(mask & lt)] = g;
        kept += __popcll(mask);
    }
    if (lane == 0)
        *P.adv_count = kept;
}

// azh_engine_root_proofs: one wave per game — the decided value (0: none, +1 / -1: the side to move there wins / loses) of
// the root and of the child of every root edge, from the marks the solver and the expansion of finished positions leave
// (node_info.w; the finished bit of the edge's range word).
__global__ __launch_bounds__(WAVE) void k_root_proofs(EngineParams P, int first_game, int *out)
{
    const int g = first_game + (int)blockIdx.x, lane = lane_id();
    int *rec = out + (size_t)blockIdx.x * AZH_ROOT_PROOF_WORDS;
    const azh_game_state s = P.gs[g];
    Arena A = arena_of(P, s.arena, g);
    const uint4 rinfo = A.ni[0];
    const int M = min((int)(rinfo.y & 0xFFFFu), AZH_MAX_MOVES);
    // (AZH_FLAG_EVAL_CACHE keeps a node's evaluation in the same word: only an exact +-1 of a finished or proven node counts)
    const bool rdec = (rinfo.y >> 16) != 0u || (!(P.flags & AZH_FLAG_EVAL_CACHE) && (rinfo.w & 0x7FFFFFFFu) == 0x3F800000u);
    if (lane == 0)
        rec[0] = rdec ? ((rinfo.w >> 31) ? -1 : 1) : 0;
    for (int j = lane; j < AZH_MAX_MOVES; j += WAVE) {
        int v = 0;
        if (j < M) {
            const uint4 ev = A.ed[rinfo.x + j];
            if (edge_child(ev) != ENONE && kid_finished(ev.w))
                v = (A.ni[edge_child(ev)].w >> 31) ? -1 : 1;
        }
        rec[1 + j] = v;
    }
}

// azh_engine_root_report: one wave per game writes the fixed-size record the header documents — the root's edges and
// the principal variation.  The walk is a dependent chain of at most AZH_PV_MAX levels: once per `go`, not per iteration.
__global__ __launch_bounds__(WAVE) void k_root_report(EngineParams P, int first_game, u32 *out)
{
    const int g = first_game + (int)blockIdx.x, lane = lane_id();
    u32 *rec = out + (size_t)blockIdx.x * AZH_ROOT_REPORT_WORDS;
    const azh_game_state s = P.gs[g];
    Arena A = arena_of(P, s.arena, g);
    const uint4 rinfo = A.ni[0];
    const int M = min((int)(rinfo.y & 0xFFFFu), AZH_MAX_MOVES);
    int expanded = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = lane + 64 * k;
        uint4 row = make_uint4(0u, 0u, 0u, 0u);
        bool has = false;
        if (j < M) {
            const uint4 ev = A.ed[rinfo.x + j];
            row = make_uint4((u32)A.em[rinfo.x + j], edge_visits(ev), ev.y, ev.x & PRIOR_MASK);
            has = edge_child(ev) != ENONE;
        }
        u32 *r = rec + 4 + 4 * j;  // (records are AZH_ROOT_REPORT_WORDS apart: word stores, no 16-byte alignment)
        r[0] = row.x; r[1] = row.y; r[2] = row.z; r[3] = row.w;
        expanded += __popcll(__ballot(has));
    }
    if (lane == 0) {
        rec[0] = (u32)s.root_visits;
        rec[1] = (u32)M;
        rec[2] = (u32)expanded;
        rec[3] = rinfo.y >> 16;
    }
    // principal variation: lane d keeps the pair of depth d
    u32 pv_move = 0, pv_n = 0;
    int len = 0;
    u32 kid = pack_kid(rinfo.x, (u32)M, (rinfo.y >> 16) != 0u);
    while (len < AZH_PV_MAX && !kid_finished(kid) && kid_count(kid) > 0) {
        const u32 first = kid_first(kid);
        const int Mk = kid_count(kid);
        u64 key = 0;
        u32 mine_z = ENONE << 16, mine_w = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = lane + 64 * k;
            if (j < Mk) {
                const uint4 ev = A.ed[first + j];
                const u64 kj = ((u64)edge_visits(ev) << 32) | (u64)(0xFFFFFFFFu - (u32)j);  // most visits, first on a tie
                if (kj > key) {
                    key = kj;
                    mine_z = ev.z;
                    mine_w = ev.w;
                }
            }
        }
        key = wave_max_u64(key);
        const u32 n = (u32)(key >> 32);
        if (n == 0u)
            break;
        const int bj = (int)(0xFFFFFFFFu - (u32)key);
        const u32 z = (u32)read_lane((int)mine_z, bj & 63);
        const u32 w = (u32)read_lane((int)mine_w, bj & 63);
        const u32 mv = A.em[first + (u32)bj];
        if (lane == len) {
            pv_move = mv;
            pv_n = n;
        }
        len++;
        if ((z >> 16) == ENONE)
            break;
        kid = w;
    }
    u32 *pv = rec + AZH_ROOT_REPORT_PV;
    if (lane == 0)
        pv[0] = (u32)len;
    if (lane < AZH_PV_MAX) {
        pv[1 + 2 * lane] = pv_move;
        pv[2 + 2 * lane] = pv_n;
    }
}

// The dense, game-ordered list(s) of the games whose leaf needs the evaluator (need_eval != 0; with two nets one list
// per class), written inside the tree launch by the workgroup that finishes last.  Every workgroup ORs its games' need bits into a bit mask (one returning agent-scope atomic per workgroup,
// performed before it draws its ticket from an agent-scope counter); the workgroup whose ticket is the last reads the
// mask — 16 bytes per 128 games — expands it in game order and clears it for the next launch.  Atomics and L1-bypassing
// loads on both sides, so no fence is needed (MI355X_MICROARCH.md, hand-off forms).  One kernel and one kernel boundary
// less per search iteration, and a tail of about a microsecond whatever the number of games.
template <int TREE_WAVES>
__device__ inline void compact_leaves(const EngineParams &P, int two, int *s_cnt /* [2][TREE_WAVES] */)
{
    constexpr int TREE_THREADS = TREE_WAVES * WAVE;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int nw = P.mask_words;
    const int c = (nw + TREE_THREADS - 1) / TREE_THREADS;  // consecutive mask words per thread (1 up to 8192 games)
    const int lo = min(nw, t * c), hi = min(nw, lo + c);
    u32 *m1p = P.need_mask, *m2p = P.need_mask + nw;
    int n1 = 0, n2 = 0;
    for (int k = lo; k < hi; k++) {
        n1 += __popc(__hip_atomic_load(&m1p[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (two)
            n2 += __popc(__hip_atomic_load(&m2p[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    const int i1 = wave_incl_scan(n1), i2 = wave_incl_scan(n2);
    if (lane == WAVE - 1) {
        s_cnt[w] = i1;
        s_cnt[TREE_WAVES + w] = i2;
    }
    __syncthreads();
    int b1 = i1 - n1, b2 = i2 - n2, t1 = 0, t2 = 0;
#pragma unroll
    for (int k = 0; k < TREE_WAVES; k++) {
        b1 += k < w ? s_cnt[k] : 0;
        b2 += k < w ? s_cnt[TREE_WAVES + k] : 0;
        t1 += s_cnt[k];
        t2 += s_cnt[TREE_WAVES + k];
    }
    for (int k = lo; k < hi; k++) {
        u32 m = __hip_atomic_load(&m1p[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (m)
            __hip_atomic_store(&m1p[k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (; m; m &= m - 1)
            P.leaf_list[b1++] = 32 * k + (__ffs((int)m) - 1);
        if (two) {
            u32 m2 = __hip_atomic_load(&m2p[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (m2)
                __hip_atomic_store(&m2p[k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (; m2; m2 &= m2 - 1)
                P.leaf_list2[b2++] = 32 * k + (__ffs((int)m2) - 1);
        }
    }
    if (t == 0) {
        *P.leaf_count = t1;
        if (two)
            *P.leaf_count2 = t2;
        __hip_atomic_store(&P.tree_done[TICKET_SHARDS * TICKET_STRIDE], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// A tree workgroup's ticket, drawn by its thread 0 behind its ORs into need_mask (`seen`: what those fetch_ors returned):
// whether this workgroup is the last of the launch, the one that calls compact_leaves.
__device__ inline int last_tree_workgroup(const EngineParams &P, u32 seen)
{
    // the ORs have returned, i.e. have been performed, before the ticket is drawn
    asm volatile("s_waitcnt vmcnt(0)" : : "v"(seen) : "memory");
    // two-level ticket: the workgroup that completes its shard draws a ticket of the top counter
    const int shard = (int)(blockIdx.x % TICKET_SHARDS);
    const int in_shard = ((int)gridDim.x - 1 - shard) / TICKET_SHARDS + 1;
    int last = 0;
    if (__hip_atomic_fetch_add(&P.tree_done[shard * TICKET_STRIDE], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_shard - 1) {
        __hip_atomic_store(&P.tree_done[shard * TICKET_STRIDE], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int shards = min((int)gridDim.x, TICKET_SHARDS);
        last = __hip_atomic_fetch_add(&P.tree_done[TICKET_SHARDS * TICKET_STRIDE], 1, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT) == shards - 1;
    }
    return last;
}

// The tree phase of a search iteration as ONE launch: a wave owns a game through backup -> "is the move due?" ->
// the next select, with the game's state in registers throughout; TREE_WAVES games share a workgroup (each wave on
// its own: wave_sync, never a workgroup barrier, inside a game), and the last workgroup to finish compacts the leaf
// list.  mode bit 0: backup + mark, bit 1: select (+ compaction).
template <bool STAMP, int TREE_WAVES, bool POOL = false>
__global__ __launch_bounds__(TREE_WAVES * WAVE) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_tree(EngineParams P, int mode, int two)
{
    __shared__ u16 s_moves[TREE_WAVES][MAX_MOVES];  // per game: the move list of the node being expanded
    __shared__ int s_cnt[2 * TREE_WAVES];
    __shared__ int s_need[TREE_WAVES];
    __shared__ int s_last;
    static_assert(32 % TREE_WAVES == 0, "a workgroup's need bits must lie in one word of the mask");
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform: the game's addresses are scalars
    const int g = blockIdx.x * TREE_WAVES + w;
    u64 st[TREE_STAMPS] = {};
    int need = 0;
    if constexpr (STAMP) st[0] = tree_stamp();
    if (g < P.G) {
        azh_game_state s = P.gs[g];
        const int forced = P.force[g];  // (same round trip as the state)
        const u32 pk = ply_kind_of(P, g);
        if constexpr (STAMP) st[1] = tree_stamp();
        if (mode & 1) {
            backup_game(P, g, s, pk);
            if constexpr (STAMP) st[2] = tree_stamp();
            mark_game(P, g, s, forced, pk);
        }
        if constexpr (STAMP) {
            st[3] = tree_stamp();
            if (!(mode & 1)) st[2] = st[3];
        }
        if (mode & 2)
            need = select_game<STAMP, POOL>(P, g, s, s_moves[w], pk, st);  // stores the state
        else if (lane_id() == 0)
            P.gs[g] = s;
    }
    if (!(mode & 2))
        return;
    if (lane_id() == 0)
        s_need[w] = need;
    if constexpr (STAMP) st[6] = tree_stamp();
    __syncthreads();
    if constexpr (STAMP) {
        st[7] = tree_stamp();
        if (g < P.G && lane_id() < TREE_STAMPS) {
            u64 v = st[0];
#pragma unroll
            for (int k = 1; k < TREE_STAMPS; k++)
                v = lane_id() == k ? st[k] : v;
            P.stamps[(size_t)g * TREE_STAMPS + lane_id()] = v;
        }
    }
    if (threadIdx.x == 0) {
        u32 m1 = 0, m2 = 0;
#pragma unroll
        for (int k = 0; k < TREE_WAVES; k++) {
            const int v = s_need[k];
            m1 |= (u32)(two ? v == 1 : v != 0) << k;
            m2 |= (u32)(two && v == 2) << k;
        }
        const int g0 = blockIdx.x * TREE_WAVES;
        u32 seen = 0;
        if (m1)
            seen |= __hip_atomic_fetch_or(&P.need_mask[g0 >> 5], m1 << (g0 & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (m2)
            seen |= __hip_atomic_fetch_or(&P.need_mask[P.mask_words + (g0 >> 5)], m2 << (g0 & 31), __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
        s_last = last_tree_workgroup(P, seen);
    }
    __syncthreads();
    if (s_last)
        compact_leaves<TREE_WAVES>(P, two, s_cnt);
}

// Reference feature rows for the dense leaf list (cpp/self_play_client.cpp:174-202).
// masks: null, or the wall mask of every board (indexed as boards) in place of `blockers`
__global__ void k_features(const ulonglong2 *boards, const int *list, int n, u64 blockers, const u64 *masks, float *out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * 49)
        return;
    const int row = idx / 49, c = idx % 49;
    const int x = c / 7, y = c % 7, sq = x + 7 * (6 - y);
    const int game = list ? list[row] : row;
    const ulonglong2 b = boards[game];
    if (masks)
        blockers = masks[game];
    float4 f;
    f.x = 1.0f;
    f.y = (float)((b.x >> sq) & 1ULL);
    f.z = (float)((b.y >> sq) & 1ULL);
    f.w = (float)((blockers >> sq) & 1ULL);
    reinterpret_cast<float4 *>(out)[idx] = f;
}

__global__ void k_reduce_stats(const u64 *stats, int G, u64 *out)
{
    const int k = blockIdx.x;
    u64 acc = 0;
    for (int g = threadIdx.x; g < G; g += blockDim.x)
        acc += stats[(size_t)g * NSTAT + k];
    __shared__ u64 s_acc[256];
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off)
            s_acc[threadIdx.x] += s_acc[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        out[k] = s_acc[0];
}

}  // namespace azh

#include "vl_search.h"

using namespace azh;

// ------------------------------------------------------------------ host

// The leaf buffers of EngineParams as one value.  The engine keeps two sets, its own G-slot one and the G K-slot one of the
// leaf-parallel search, and P points at one of them.
struct LeafBuffers {
    ulonglong2 *leaf_board = nullptr;
    u64 *leaf_mask = nullptr;
    int *need_eval = nullptr, *leaf_list = nullptr, mask_words = 0;
    u32 *need_mask = nullptr;
    float *logits = nullptr, *values = nullptr;
    void read(const EngineParams &P)
    {
        leaf_board = P.leaf_board; leaf_mask = P.leaf_mask; need_eval = P.need_eval; leaf_list = P.leaf_list;
        need_mask = P.need_mask; mask_words = P.mask_words; logits = P.logits; values = P.values;
    }
    void write(EngineParams &P) const
    {
        P.leaf_board = leaf_board; P.leaf_mask = leaf_mask; P.need_eval = need_eval; P.leaf_list = leaf_list;
        P.need_mask = need_mask; P.mask_words = mask_words; P.logits = logits; P.values = values;
    }
};

struct azh_engine {
    azh_config cfg;
    EngineParams P;
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    float *d_feat = nullptr;       // azh_engine_leaf_features: [G] rows, allocated by the first call
    float *d_sym_logits = nullptr, *d_sym_values = nullptr;  // AZH_FLAG_SYMMETRY_AVG scratch, allocated by the first evaluation
    u16 *d_play_moves = nullptr;   // azh_engine_play_moves: moves [G] and status [G], allocated by the first call
    int *d_play_status = nullptr;
    u32 *d_report = nullptr;       // azh_engine_root_report: [G][AZH_ROOT_REPORT_WORDS], allocated by the first call
    u64 *d_stat_out = nullptr;
    u16 *d_gumbel_seq = nullptr;     // azh_engine_set_gumbel: the considered-visits table, gumbel_seq_cap entries, allocated by the
    size_t gumbel_seq_cap = 0;       // first call that needs them (a larger m * visits later allocates again)
    float *d_move_temperature = nullptr, *d_root_policy_temperature = nullptr;  // azh_engine_set_temperature: [max_plies] each,
                                                                                // allocated by the first call that brings one
    // finished games formatted but not yet handed out
    std::vector<std::string> pending;
    size_t pending_pos = 0;
    // records taken off the device (azh_engine_fetch) and not yet formatted
    std::vector<uint32_t> staged;
    // an explicit azh_engine_fetch covers the drain sequence that follows it: until that sequence has ended (a drain call
    // that hands out no game) a drain with nothing staged returns empty instead of fetching — the caller has enqueued
    // its next run in between, and a fetch would wait for that run
    bool fetch_covers_drain = false;
    // work has been enqueued since the last fetch (its finished games are still on the device): a drain by a caller that
    // never fetches fetches when this is set — once per round, whether it drains in a loop until nothing comes or once
    bool unfetched_work = true;
    long long implicit_fetches = 0;  // fetches made by azh_engine_drain_json itself (azh_engine_implicit_fetches)
    // uid-ordered emission: finished games wait here until every game with a smaller uid has been handed out or
    // is known to have been dropped ("" = dropped)
    bool emit_by_uid = false;
    bool record_blockers = false;  // every line gains "blockers", the engine's mask (azh_engine_set_record_blockers)
    std::map<uint32_t, std::string> held;
    uint32_t next_uid = 0;
    bool order_broken = false;  // records were lost (ring overflow): some uid will never come, see azh_engine_drain_json
    // timing: every `timing_stride`-th iteration of the device loop is bracketed by events on the engine's stream
    // (tower start, tower end, start of the next tower = end of the tree phase).  Sampling keeps the event packets —
    // each a barrier in the queue, a few microseconds — out of most iterations of the region being measured.
    int timing_stride = 0;  // 0 = off
    long long loop_iter = 0;
    std::vector<hipEvent_t> events;  // 3 per sample: tower start, tower end, tree phase end
    size_t samples = 0;
    std::vector<int> close_of;       // per sample: index of the event that closes its tree phase
    bool close_pending = false;      // the last sample's tree phase is closed at the start of the next iteration
    int *h_count = nullptr;  // pinned
    // pinned staging of azh_engine_fetch: the ring's head and its records are copied here (a copy into pageable memory is
    // staged by the runtime through buffers of its own and may serialise with other streams' copies), then into `staged`
    u64 *h_head = nullptr;
    u32 *h_stage = nullptr;
    size_t h_stage_words = 0;
    std::vector<u32 *> h_stage_retired;
    bool selected = false;
    bool begun = false;  // a tree launch has been enqueued (the first select): the start position, pool included, is settled
    StartEntry *d_pool = nullptr;        // azh_engine_set_start_pool: the entries on the device (pool_cap of them) and on the host
    size_t pool_cap = 0;
    std::vector<StartEntry> pool;
    bool arena_lists = false;  // run_arena: one leaf list per net
    bool stamp_next = false;   // azh_engine_tree_stamps: the next fused tree launch of the loop is the stamped instantiation
    int thin_mode = -1;        // azh_engine_set_thin_batches: 0 the 3-board tower, 1 one board per workgroup, -1 by the engine's size
    int adv_workers = 8;       // workgroups at the head of every tower launch of the device loop that play the queued moves
    // leaf-parallel search (azh_engine_set_leaf_batch): K leaves per game and iteration in slots g K + p.  With K > 1 the
    // leaf buffers of P (boards, need flags, list, need mask, logits, values) point at G K-slot buffers; with K = 1 at the
    // engine's own G-slot ones, and every launch is the one-leaf search's.
    VlParams V{};
    int vl_slots_cap = 0;  // slots the G K buffers were allocated for
    LeafBuffers g_leaves;   // the engine's own G-slot buffers
    LeafBuffers vl_leaves;  // the G K-slot buffers (kept while K = 1 is in force)
    // proven wins and losses (azh_engine_set_solver): while it is on, every K — 1 included — runs through k_vl_tree and the
    // G K-slot buffers (vl_active: P's leaf buffers point at them), and its backup is followed by the proof pass
    bool vl_active = false;   // (the solver's own switch is V.solver)
    int32_t *d_proofs = nullptr;  // azh_engine_root_proofs: [G][AZH_ROOT_PROOF_WORDS], allocated by the first call
    // search settings per side (azh_engine_set_search_sets): the sets in force on the host (P.n_search_sets of them) and the
    // device's table, AZH_SEARCH_SETS_MAX entries allocated by the first call that brings sets; P.search_sets points at it
    // while the mode is on
    azh_search_set sets[AZH_SEARCH_SETS_MAX] = {};
    azh_search_set *d_sets = nullptr;
};

static int leaf_k(const azh_engine *e) { return e->V.K > 1 ? e->V.K : 1; }

static bool explores(const azh_engine *e) { return exploration_on(e->P.fpu_reduction, e->P.c_base); }

static bool search_sets_on(const azh_engine *e) { return e->P.n_search_sets != 0; }

// what beside K keeps the leaf-parallel kernel in force, for the errors of the one-leaf calls ("" if nothing; `joint`: " with" / " and")
static std::string vl_beside(const azh_engine *e, const char *joint)
{
    const char *mode = explores(e) ? " azh_engine_set_exploration" : search_sets_on(e) ? " azh_engine_set_search_sets" : "";  // (never both)
    if (!e->V.solver && !mode[0])
        return "";
    return std::string(joint) + (e->V.solver ? " the solver" : "") + (e->V.solver && mode[0] ? " and" : "") + mode;
}

// the tower for this engine's leaf batches: one board per workgroup for engines (or batches the host says are) small
// the wall mask of every leaf slot, for the tower and k_features: null (the engine's one mask) while no pool is set
static const unsigned long long *leaf_masks(const azh_engine *e) { return e->P.pool ? (const unsigned long long *)e->P.leaf_mask : nullptr; }

// the walls game `uid` is played on
static u64 uid_blockers(const azh_engine *e, u32 uid)
{
    return e->pool.empty() ? e->P.blockers : e->pool[start_pool_entry(uid, (u32)e->pool.size(), e->P.pool_stride)].blockers;
}

static int thin_batches(const azh_engine *e)
{
    return e->thin_mode >= 0 ? e->thin_mode : (e->P.G * leaf_k(e) <= AZH_THIN_MAX_GAMES ? 1 : 0);  // (by slots: G K)
}

static const size_t MAX_TIMED_SAMPLES = 8192;

template <typename T> static int dev_alloc(azh_engine *e, T **p, size_t count)
{
    void *q = nullptr;
    AZH_HIP(hipMalloc(&q, count * sizeof(T)));
    AZH_HIP(hipMemset(q, 0, count * sizeof(T)));
    e->allocs.push_back(q);
    *p = (T *)q;
    return 0;
}

#define AZH_TRY(call) do { if (int _rc = (call)) return _rc; } while (0)  // (as AZH_HIP: the failure is the caller's result)

// allocate on first use: zeroed and owned by e->allocs like every other device buffer
template <typename T> static int dev_alloc_once(azh_engine *e, T **p, size_t count) { return *p ? 0 : dev_alloc(e, p, count); }

// ------------------------------------------------------------------ the search modes: who refuses whom
//
// Ten modes are switched between iterations, by a setter each.  What a mode cannot run beside (create-time flags and settings,
// other modes) is stated here once, and mode_refusal answers for every setter.  In words: the table "Search modes: who refuses
// whom" of include/ataxxzero_hip.h and of DESIGN.md.

enum { MODE_NONE = -1, MODE_CAP, MODE_FORCED, MODE_GUMBEL, MODE_TEMPERATURE, MODE_RESIGN, MODE_SYMMETRY, MODE_LEAF_BATCH, MODE_SOLVER,
       MODE_EXPLORATION, MODE_SEARCH_SETS };

// Is `bb` its own image under all 8 symmetries?  (the two mirrors and the transposition generate them)
static bool symmetry_invariant(u64 bb)
{
    return symmetry_board(1, bb) == bb && symmetry_board(2, bb) == bb && symmetry_board(4, bb) == bb;
}

struct ModeInfo {
    const char *setter, *phrase;  // a refusal calls the mode by its phrase: another setter's (with "(<setter>)" behind it if
    bool cited, subject;          // `cited`), and its own if `subject`: "<phrase> is not supported with", not "not supported with"
    bool own_advance;             // while it is on, the device loop plays the queued moves in a launch of their own (RunLoop::own)
    bool (*on)(const azh_engine *);
    u32 refused_flags;  // (the create-time requirements that are no flags: mode_refusal)
};

constexpr u32 ROOT_FLAGS = AZH_FLAG_TWO_NETS | AZH_FLAG_ONE_RANDOM_MOVE, LEAF_FLAGS = AZH_FLAG_TWO_NETS | AZH_FLAG_EVAL_CACHE | AZH_FLAG_SYMMETRY_AVG;
#define ON(expr) [](const azh_engine *e) -> bool { return expr; }
static const ModeInfo MODES[] = {  // (in the order of the MODE_ constants)
    {"azh_engine_set_playout_cap", "the playout cap", true, false, false, ON(e->P.fast_visits != 0), ROOT_FLAGS},
    {"azh_engine_set_forced_playouts", "forced playouts", true, false, true, ON(e->P.forced_k != 0.0f), ROOT_FLAGS},
    {"azh_engine_set_gumbel", "the Gumbel root search", true, false, true, ON(e->P.gumbel_m != 0),
     ROOT_FLAGS | AZH_FLAG_SAMPLE_POW5 | AZH_FLAG_EVAL_CACHE},
    // (a move temperature needs the launch of its own, a root-policy table does not: RunLoop::begin asks for the former itself)
    {"azh_engine_set_temperature", "a temperature table", true, false, false, ON(e->P.move_temperature || e->P.root_policy_temperature),
     ROOT_FLAGS | AZH_FLAG_SAMPLE_POW5 | AZH_FLAG_PY_POSTERIOR},
    {"azh_engine_set_resign", "recorded values and resignation", true, false, true, ON(e->P.resign_plies != 0u), ROOT_FLAGS},
    {"azh_engine_set_random_symmetry", "the random symmetry", true, false, true, ON(e->P.random_symmetry != 0u),
     AZH_FLAG_TWO_NETS | AZH_FLAG_SYMMETRY_AVG},
    {"azh_engine_set_leaf_batch", "more than one leaf per game", true, true, false, ON(e->V.K > 1), LEAF_FLAGS},
    {"azh_engine_set_solver", "the solver", false, true, false, ON(e->V.solver != 0), LEAF_FLAGS},
    {"azh_engine_set_exploration", "first-play urgency or a growing exploration rate", true, false, false,
     ON(exploration_on(e->P.fpu_reduction, e->P.c_base)), LEAF_FLAGS},
    // (own_advance: the tally of the games' results lives in k_advance_list's advance_game, and so does the slot word's write)
    {"azh_engine_set_search_sets", "search settings per side", true, false, true, ON(e->P.n_search_sets != 0),
     LEAF_FLAGS | AZH_FLAG_ONE_RANDOM_MOVE},
};
#undef ON

// The pairs of modes that do not run beside each other, each once: whichever of the two asks second is refused.  (With several
// modes on, a refusal names the first pair listed here.)
static const int EXCLUDED[][2] = {
    {MODE_GUMBEL, MODE_CAP},    {MODE_GUMBEL, MODE_FORCED},     {MODE_GUMBEL, MODE_TEMPERATURE}, {MODE_GUMBEL, MODE_LEAF_BATCH},
    {MODE_GUMBEL, MODE_SOLVER}, {MODE_FORCED, MODE_LEAF_BATCH}, {MODE_FORCED, MODE_SOLVER},
    // (both restate the root's PUCT with q = 0 for an unvisited edge and the constant c_puct)
    {MODE_GUMBEL, MODE_EXPLORATION}, {MODE_FORCED, MODE_EXPLORATION},
    // (a set carries its side's threshold and exploration knobs: a second source for either is an ambiguity)
    {MODE_GUMBEL, MODE_SEARCH_SETS}, {MODE_FORCED, MODE_SEARCH_SETS}, {MODE_CAP, MODE_SEARCH_SETS}, {MODE_EXPLORATION, MODE_SEARCH_SETS},
};

// The create-time flags a mode can be refused with; of several set at once a refusal names the first one listed here.
#define NAMED(flag) {flag, #flag}
static const struct { u32 bit; const char *name; } FLAG_NAMES[] = {
    NAMED(AZH_FLAG_TWO_NETS),     NAMED(AZH_FLAG_ONE_RANDOM_MOVE), NAMED(AZH_FLAG_SAMPLE_POW5),
    NAMED(AZH_FLAG_PY_POSTERIOR), NAMED(AZH_FLAG_EVAL_CACHE),      NAMED(AZH_FLAG_SYMMETRY_AVG),
};
#undef NAMED

// The random symmetry's cause against the masks games are played on — the pool's entries, or `blockers` where there is none:
// empty if every one is its own image under the 8 symmetries, else the refusal's words with the first mask that is not.
static std::string asymmetric_mask(const StartEntry *pool, size_t n, u64 blockers)
{
    for (size_t i = 0; i < (pool ? n : 1); i++) {
        const u64 bb = pool ? pool[i].blockers : blockers;
        if (symmetry_invariant(bb & BOARD_MASK))
            continue;
        char mask[32];
        snprintf(mask, sizeof(mask), "0x%llx", (unsigned long long)bb);
        return std::string("a blockers mask (") + mask + ") that is not its own image under all 8 symmetries (the tower takes one "
               "blocker plane per launch)";
    }
    return "";
}

// May `mode` come on in this engine now?  Empty: yes; else why not, as the refusal reads after "<setter>: ".  The flags are looked
// at first, then what else a mode requires of the engine's configuration, then the modes that are on.
static std::string mode_refusal(const azh_engine *e, int mode)
{
    const ModeInfo &m = MODES[mode];
    const std::string head = m.subject ? std::string(m.phrase) + " is not supported with " : "not supported with ";
    for (const auto &f : FLAG_NAMES)
        if (e->P.flags & m.refused_flags & f.bit)
            return head + f.name;
    if ((mode == MODE_LEAF_BATCH || mode == MODE_SOLVER || mode == MODE_EXPLORATION || mode == MODE_SEARCH_SETS) && e->P.select_budget > 0)
        return head + "select_budget > 0";
    if (mode == MODE_GUMBEL && (!(e->P.flags & AZH_FLAG_NO_REUSE) || e->P.noise_w != 0.0f))
        return "the engine must have been created with AZH_FLAG_NO_REUSE and dirichlet_weight 0 (the schedule assumes a fresh "
               "root, and its noise is the Gumbel)";
    if (mode == MODE_SYMMETRY) {
        const std::string why = asymmetric_mask(e->pool.empty() ? nullptr : e->pool.data(), e->pool.size(), e->P.blockers);
        if (!why.empty())
            return head + why;
    }
    for (const auto &pair : EXCLUDED) {
        const int other = pair[0] == mode ? pair[1] : pair[1] == mode ? pair[0] : MODE_NONE;
        if (other != MODE_NONE && MODES[other].on(e))
            return head + MODES[other].phrase + (MODES[other].cited ? std::string(" (") + MODES[other].setter + ")" : "");
    }
    return "";
}

// What every mode setter does between the checks of its own arguments (-1, -2) and its first change: -3 while a selected batch
// awaits its backup, -4 where `mode` may not come on (MODE_NONE: the call switches something off, which is no request), then the
// stream is drained.  Every check comes before the first change, so a refused call leaves the engine as it was.  `who`: the
// calling entry point, for its errors.
static int mode_request(azh_engine *e, const char *who, int mode)
{
    if (e->selected)
        return azh_fail(-3, "%s: a selected batch awaits its backup", who);
    const std::string why = mode != MODE_NONE ? mode_refusal(e, mode) : "";
    if (!why.empty())
        return azh_fail(-4, "%s: %s", who, why.c_str());
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int azh_engine_create(const azh_config *cfg, azh_engine **out)
{
    if (!cfg || !out)
        return azh_fail(-1, "azh_engine_create: null argument");
    if (cfg->games <= 0 || cfg->visits <= 0 || cfg->visits > 60000 || cfg->max_plies <= 0 ||
        cfg->edges_per_node < 8)
        return azh_fail(-2, "azh_engine_create: bad config (games %d visits %d max_plies %d edges_per_node %d)",
                        cfg->games, cfg->visits, cfg->max_plies, cfg->edges_per_node);
    if ((long long)(cfg->visits + 8) * cfg->edges_per_node >= (1 << 23))
        return azh_fail(-2, "azh_engine_create: (visits + 8) * edges_per_node = %lld edges per game do not fit the 23-bit edge "
                            "index of the tree's edge records", (long long)(cfg->visits + 8) * cfg->edges_per_node);
    if (azh_require_device())
        return -3;
    azh_engine *e = new azh_engine();
    e->cfg = *cfg;
    EngineParams &P = e->P;
    memset(&P, 0, sizeof(P));
    P.G = cfg->games;
    P.visits = cfg->visits;
    P.node_cap = cfg->visits + 8;
    P.edge_cap = P.node_cap * cfg->edges_per_node;
    P.path_cap = P.node_cap;
    P.max_plies = cfg->max_plies;
    P.c_puct = cfg->c_puct;
    P.fpu_reduction = -1.0f;  // (azh_engine_set_exploration: off)
    P.alpha = cfg->dirichlet_alpha;
    P.noise_w = cfg->dirichlet_weight;
    P.k0 = (u32)cfg->seed;
    P.k1 = (u32)(cfg->seed >> 32);
    P.start_x = cfg->start_x;
    P.start_o = cfg->start_o;
    P.blockers = cfg->blockers;
    P.start_turn = cfg->start_turn;
    P.flags = cfg->flags;
    P.select_budget = (int)cfg->select_budget;

    const size_t G = (size_t)P.G;
    // ring of finished-game records (64 KiB per slot between two drains)
    P.ring_cap_words = std::max<size_t>((size_t)1 << 22, G * 16384);
    int rc = 0;
    rc |= dev_alloc(e, &P.gs, G);
    rc |= dev_alloc(e, &P.force, G);
    rc |= dev_alloc(e, &P.no_emit, G);
    P.tt_size = 1;
    while (P.tt_size < 4 * P.node_cap)
        P.tt_size <<= 1;
    if (cfg->flags & AZH_FLAG_EVAL_CACHE)
        rc |= dev_alloc(e, &P.tt, 2 * G * (size_t)P.tt_size);
    rc |= dev_alloc(e, &P.adv_list, G);
    rc |= dev_alloc(e, &P.adv_count, 1);
    rc |= dev_alloc(e, &P.adv_done, 1);
    rc |= dev_alloc(e, &P.path, G * P.path_cap);
    rc |= dev_alloc(e, &P.node_board, 2 * G * P.node_cap);
    rc |= dev_alloc(e, &P.node_info, 2 * G * P.node_cap);
    rc |= dev_alloc(e, &P.edge, 2 * G * P.edge_cap);
    rc |= dev_alloc(e, &P.edge_move, 2 * G * P.edge_cap);
    rc |= dev_alloc(e, &P.leaf_board, G);
    rc |= dev_alloc(e, &P.leaf_mask, G);
    rc |= dev_alloc(e, &P.slot_mask, G);
    rc |= dev_alloc(e, &P.need_eval, G);
    rc |= dev_alloc(e, &P.leaf_list, G);
    rc |= dev_alloc(e, &P.leaf_count, 1);
    rc |= dev_alloc(e, &P.leaf_list2, G);
    rc |= dev_alloc(e, &P.leaf_count2, 1);
    rc |= dev_alloc(e, &P.tree_done, (size_t)TICKET_SHARDS * TICKET_STRIDE + 1);
    P.mask_words = (P.G + 31) / 32;
    rc |= dev_alloc(e, &P.need_mask, 2 * (size_t)P.mask_words);
    rc |= dev_alloc(e, &P.logits, G * AZH_POLICY_SIZE);
    rc |= dev_alloc(e, &P.values, G);
    rc |= dev_alloc(e, &P.rec, G * P.max_plies * REC_STRIDE_WORDS);
    rc |= dev_alloc(e, &P.ring, P.ring_cap_words);
    rc |= dev_alloc(e, &P.ring_head, 1);
    rc |= dev_alloc(e, &P.stats, G * NSTAT);
    rc |= dev_alloc(e, &P.bfs_spill, G * 3 * P.node_cap);
    rc |= dev_alloc(e, &e->d_stat_out, NSTAT);
    rc |= dev_alloc(e, &e->V.proofs, G * AZH_PROOF_STAT_COUNT);
    if (rc) {
        azh_engine_destroy(e);
        return rc;
    }
    if (hipStreamCreate(&e->stream) != hipSuccess ||
        hipHostMalloc((void **)&e->h_count, sizeof(int)) != hipSuccess ||
        hipHostMalloc((void **)&e->h_head, sizeof(u64)) != hipSuccess) {
        azh_engine_destroy(e);
        return azh_fail(-4, "azh_engine_create: stream / pinned allocation failed");
    }
    // one move-playing workgroup per 128 game slots (an iteration queues about one game in 400 at 400 sims/move, one in 200
    // at 200), at least 8, at most 64, a multiple of 8 (the tiles behind them keep their XCD)
    e->adv_workers = std::min(64, std::max(8, (P.G / 128 + 7) / 8 * 8));
    e->V.K = 1;
    e->V.vl = 1;
    e->V.path_cap = P.path_cap;
    e->g_leaves.read(P);
    hipLaunchKernelGGL(k_init, dim3(P.G), dim3(WAVE), 0, e->stream, P);
    if (hipStreamSynchronize(e->stream) != hipSuccess) {
        azh_engine_destroy(e);
        return azh_fail(-5, "azh_engine_create: init kernel failed");
    }
    *out = e;
    return 0;
}

extern "C" void azh_engine_destroy(azh_engine *e)
{
    if (!e)
        return;
    if (e->stream)
        (void)hipStreamSynchronize(e->stream);
    for (auto ev : e->events)
        (void)hipEventDestroy(ev);
    for (void *p : e->allocs)
        (void)hipFree(p);
    if (e->h_count)
        (void)hipHostFree(e->h_count);
    if (e->h_head)
        (void)hipHostFree(e->h_head);
    if (e->h_stage)
        (void)hipHostFree(e->h_stage);
    for (u32 *q : e->h_stage_retired)
        (void)hipHostFree(q);
    if (e->stream)
        (void)hipStreamDestroy(e->stream);
    delete e;
}

extern "C" int azh_engine_node_cap(const azh_engine *e) { return e ? e->P.node_cap : -1; }
extern "C" int azh_engine_edge_cap(const azh_engine *e) { return e ? e->P.edge_cap : -1; }

constexpr int ADV_GRID = 64;  // one wave each; a search iteration queues G * (1 / visits + ...) re-roots: about 11 at 4096 games

// the queued re-roots in a launch of their own (always after a select has passed over the queued games)
static int enqueue_advance(azh_engine *e)
{
    e->unfetched_work = true;  // (every path that can finish a game goes through here)
    hipExtLaunchKernelGGL(k_advance_list, dim3(ADV_GRID), dim3(WAVE), 0, e->stream, nullptr, nullptr, 0, e->P);
    AZH_HIP(hipGetLastError());
    return 0;
}

// one leaf list per net (arena)
static int two_lists(const azh_engine *e) { return (e->P.flags & AZH_FLAG_TWO_NETS) && e->arena_lists; }

// One tree launch on the engine's stream, for the device-resident loop and the step-wise API alike.  mode bit 0: backup +
// mark, bit 1: select + leaf list.
static int enqueue_tree(azh_engine *e, int mode, bool stamped = false)
{
    const int two = two_lists(e);
    e->begun = true;
    const bool small = e->P.G <= TREE_ONE_ROUND_GAMES;
    const int waves = small ? TREE_WAVES_SMALL : TREE_WAVES_LARGE;
    const dim3 grid((e->P.G + waves - 1) / waves), block(waves * WAVE);
    const bool pool = e->P.pool != nullptr;  // (the instantiations that know of the start pool)
#define TREE_LAUNCH(STAMP, WAVES)                                                                                              \
    do {                                                                                                                       \
        if (pool)                                                                                                              \
            hipExtLaunchKernelGGL((k_tree<STAMP, WAVES, true>), grid, block, 0, e->stream, nullptr, nullptr, 0, e->P, mode, two); \
        else                                                                                                                   \
            hipExtLaunchKernelGGL((k_tree<STAMP, WAVES>), grid, block, 0, e->stream, nullptr, nullptr, 0, e->P, mode, two);    \
    } while (0)
    if (e->vl_active)  // leaf-parallel search: one workgroup per game (not stamped: azh_engine_tree_stamps refuses)
        hipExtLaunchKernelGGL(k_vl_tree, dim3(e->P.G), dim3(VL_WAVES * WAVE), 0, e->stream, nullptr, nullptr, 0, e->P, e->V, mode);
    else if (stamped && small)
        TREE_LAUNCH(true, TREE_WAVES_SMALL);
    else if (stamped)
        TREE_LAUNCH(true, TREE_WAVES_LARGE);
    else if (small)
        TREE_LAUNCH(false, TREE_WAVES_SMALL);
    else
        TREE_LAUNCH(false, TREE_WAVES_LARGE);
#undef TREE_LAUNCH
    AZH_HIP(hipGetLastError());
    return 0;
}

static int enqueue_select(azh_engine *e) { return enqueue_tree(e, 2) || enqueue_advance(e); }

static int enqueue_backup(azh_engine *e) { return enqueue_tree(e, 1); }

extern "C" int azh_engine_select(azh_engine *e, int32_t *n_leaves_out)
{
    if (!e)
        return azh_fail(-1, "azh_engine_select: null engine");
    if (enqueue_select(e))
        return -1;
    AZH_HIP(hipMemcpyAsync(e->h_count, e->P.leaf_count, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    AZH_HIP(hipStreamSynchronize(e->stream));
    e->selected = true;
    if (n_leaves_out)
        *n_leaves_out = *e->h_count;
    return 0;
}

extern "C" int azh_engine_leaves(azh_engine *e, int32_t *need_eval, uint64_t *leaf_boards)
{
    if (!e)
        return azh_fail(-1, "azh_engine_leaves: null engine");
    if (e->vl_active)
        return azh_fail(-2, "azh_engine_leaves: %d leaves per game%s: use azh_engine_batch_leaves", leaf_k(e),
                        vl_beside(e, " with").c_str());
    AZH_HIP(hipStreamSynchronize(e->stream));
    if (need_eval)
        AZH_HIP(hipMemcpy(need_eval, e->P.need_eval, (size_t)e->P.G * 4, hipMemcpyDeviceToHost));
    if (leaf_boards)
        AZH_HIP(hipMemcpy(leaf_boards, e->P.leaf_board, (size_t)e->P.G * 16, hipMemcpyDeviceToHost));
    return 0;
}

// Dense feature rows of the current leaf batch, in leaf-list (game) order.
extern "C" int azh_engine_leaf_features(azh_engine *e, float *out, int32_t *games_out)
{
    if (!e || !out)
        return azh_fail(-1, "azh_engine_leaf_features: null argument");
    if (e->vl_active)
        return azh_fail(-2, "azh_engine_leaf_features: not available with %d leaves per game%s", leaf_k(e),
                        vl_beside(e, " and").c_str());
    AZH_HIP(hipStreamSynchronize(e->stream));
    int n = 0;
    AZH_HIP(hipMemcpy(&n, e->P.leaf_count, 4, hipMemcpyDeviceToHost));
    if (n <= 0)
        return 0;
    AZH_TRY(dev_alloc_once(e, &e->d_feat, (size_t)e->P.G * AZH_FEATURE_SIZE));
    hipLaunchKernelGGL(k_features, dim3((n * 49 + 255) / 256), dim3(256), 0, e->stream,
                       (const ulonglong2 *)e->P.leaf_board, (const int *)e->P.leaf_list, n, e->P.blockers,
                       (const u64 *)leaf_masks(e), e->d_feat);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipStreamSynchronize(e->stream));
    AZH_HIP(hipMemcpy(out, e->d_feat, (size_t)n * AZH_FEATURE_SIZE * 4, hipMemcpyDeviceToHost));
    if (games_out)
        AZH_HIP(hipMemcpy(games_out, e->P.leaf_list, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the engine's leaf boards and evaluation arrays as a tower batch of at most G listed games
static NetBatch leaf_batch(const azh_engine *e, const int *list, const int *count)
{
    NetBatch b;
    b.boards = (const unsigned long long *)e->P.leaf_board;
    b.list = list;
    b.count = count;
    b.max_n = e->P.G;
    b.blockers = e->P.blockers;
    b.masks = leaf_masks(e);
    b.logits = e->P.logits;
    b.values = e->P.values;
    return b;
}

// one evaluation of the listed leaves by `net`; with AZH_FLAG_SYMMETRY_AVG the 8-way averaged one
static int launch_eval(azh_engine *e, azh_net *net, int dtype, const int *list, const int *count, const AdvanceHook *hook = nullptr)
{
    NetBatch b = leaf_batch(e, list, count);
    NetOptions o;
    o.hook = hook;
    if (!(e->P.flags & AZH_FLAG_SYMMETRY_AVG)) {
        b.max_n = e->P.G * leaf_k(e);
        o.thin = thin_batches(e);
        return azh_net_launch(net, dtype, b, e->stream, o);
    }
    AZH_TRY(dev_alloc_once(e, &e->d_sym_logits, (size_t)e->P.G * 8 * AZH_POLICY_SIZE));
    AZH_TRY(dev_alloc_once(e, &e->d_sym_values, (size_t)e->P.G * 8));
    o.sym_logits = e->d_sym_logits;
    o.sym_values = e->d_sym_values;
    o.thin = e->thin_mode >= 0 ? e->thin_mode : (e->P.G * 8 <= AZH_THIN_MAX_GAMES ? 1 : 0);  // (8 virtual boards per leaf)
    return azh_net_launch(net, dtype, b, e->stream, o);
}

extern "C" int azh_engine_eval(azh_engine *e, azh_net *net, int dtype)
{
    if (!e || !net)
        return azh_fail(-1, "azh_engine_eval: null argument");
    return launch_eval(e, net, dtype, e->P.leaf_list, e->P.leaf_count);
}

extern "C" int azh_engine_set_evals(azh_engine *e, const float *logits, const float *values)
{
    if (!e || !logits || !values)
        return azh_fail(-1, "azh_engine_set_evals: null argument");
    if (e->vl_active)
        return azh_fail(-2, "azh_engine_set_evals: %d leaves per game%s: use azh_engine_set_batch_evals", leaf_k(e),
                        vl_beside(e, " with").c_str());
    AZH_HIP(hipMemcpyAsync(e->P.logits, logits, (size_t)e->P.G * AZH_POLICY_SIZE * 4, hipMemcpyHostToDevice, e->stream));
    AZH_HIP(hipMemcpyAsync(e->P.values, values, (size_t)e->P.G * 4, hipMemcpyHostToDevice, e->stream));
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int azh_engine_backup(azh_engine *e)
{
    if (!e)
        return azh_fail(-1, "azh_engine_backup: null engine");
    if (enqueue_backup(e))
        return -1;
    AZH_HIP(hipStreamSynchronize(e->stream));
    e->selected = false;
    return 0;
}

// Device-resident loop.  Iteration = select -> tower -> backup -> "is the move due?"; consecutive iterations run
// backup + mark + the next select of one game in a single fused launch (k_tree), and the queued re-roots
// inside the tower launch that follows (its first workgroups).
//
// The queued moves (sample, record, re-root: advance_game) are played by the first workgroups of the tower launch that
// follows the tree launch which queued them — dispatched before any tile's workgroup, done after ~0.1 ms, and the next
// tree launch, behind the tower on the same stream, finds every move played: one stream, two launches per iteration.
// (Rounds 3-5 ran them as a launch of their own on a high-priority side stream beside the tower; that launch mostly waited
// for the tower's first workgroups to retire and its events cost every iteration 7-10 us:
// profiles/round6_reroots_in_the_tower_launch.txt.)
//
// A run is enqueued as begin() + `iterations` x iteration(): azh_engine_run does that for one engine, azh_engines_run for
// several with their iterations interleaved, so that the half-batches of a GPU all start with the first launches enqueued
// instead of one after the other's whole run.
struct RunLoop {
    azh_engine *e;
    azh_net *net_a, *net_b;
    int dtype, iterations;
    bool pair = false;
    bool own = false;  // a mode with own_advance (MODES) or a move temperature: the queued moves in a k_advance_list launch of
                       // their own, on the engine's stream, in front of the tower (the tower kernels' advance_game records no
                       // pruned counts, writes no key word and knows no ply value and no temperature: engine_device.h)
    AdvanceHook hook;

    int begin()
    {
        // arena: the two nets' towers as one launch (AZH_ARENA_PAIR=0: two launches back to back, for A/B runs)
        const char *pair_s = getenv("AZH_ARENA_PAIR");  // (read per call: a test switches it inside one process)
        const bool pair_env = !(pair_s && atoi(pair_s) == 0);
        pair = pair_env && two_lists(e) && !(e->P.flags & AZH_FLAG_SYMMETRY_AVG);
        own = e->P.move_temperature != nullptr;
        for (const ModeInfo &m : MODES)
            own = own || (m.own_advance && m.on(e));
        hook.workers = e->adv_workers;
        hook.at_head = 1;   // (decided per launch by the tower's launch functions: in front only where workgroups queue for slots)
        hook.P = e->P;
        e->unfetched_work = true;  // (every path that can finish a game goes through a re-root)
        if (enqueue_tree(e, 2))  // select + leaf list
            return -1;
        if (own && enqueue_advance(e))
            return -1;
        return 0;
    }

    int iteration(int it)
    {
        const AdvanceHook *moves = own ? nullptr : &hook;
        const bool rec = e->timing_stride > 0 && e->loop_iter % e->timing_stride == 0 && e->samples < MAX_TIMED_SAMPLES;
        hipEvent_t *ev = rec ? &e->events[3 * e->samples] : nullptr;
        if (e->close_pending) {
            // the tree phase of the previous sample ends where this tower starts
            if (rec) {
                e->close_of[e->samples - 1] = (int)(3 * e->samples);  // this sample's start event doubles as the end
            } else {
                AZH_HIP(hipEventRecord(e->events[3 * (e->samples - 1) + 2], e->stream));
                e->close_of[e->samples - 1] = (int)(3 * (e->samples - 1) + 2);
            }
            e->close_pending = false;
        }
        if (rec) AZH_HIP(hipEventRecord(ev[0], e->stream));
        int rc = 1;
        if (net_b && pair) {  // both nets' leaf lists in ONE tower launch (1: not applicable -> one after the other)
            NetOptions o;
            o.thin = thin_batches(e);
            o.hook = moves;
            rc = azh_net_launch_pair(net_a, net_b, dtype, leaf_batch(e, e->P.leaf_list, e->P.leaf_count), e->P.leaf_list2,
                                     e->P.leaf_count2, e->stream, o);
        }
        if (rc == 1) {
            rc = launch_eval(e, net_a, dtype, e->P.leaf_list, e->P.leaf_count, moves);   // (the first launch plays the moves)
            if (rc == 0 && net_b)
                rc = launch_eval(e, net_b, dtype, e->P.leaf_list2, e->P.leaf_count2);
        }
        if (rc) return rc;
        if (rec) AZH_HIP(hipEventRecord(ev[1], e->stream));
        const int last = it + 1 == iterations;
        const bool stamped = e->stamp_next && !last;
        if (enqueue_tree(e, last ? 1 : 3, stamped))
            return -1;
        if (stamped)
            e->stamp_next = false;
        if (!last && own && enqueue_advance(e)) return -1;
        if (rec) {
            e->samples++;
            if (last) {
                AZH_HIP(hipEventRecord(ev[2], e->stream));
                e->close_of[e->samples - 1] = (int)(3 * (e->samples - 1) + 2);
            } else {
                e->close_pending = true;
            }
        }
        e->loop_iter++;
        return 0;
    }
};

static int run_loop(azh_engine *e, azh_net *net_a, azh_net *net_b, int dtype, int iterations)
{
    if (iterations <= 0)
        return 0;
    RunLoop L{e, net_a, net_b, dtype, iterations};
    int rc = L.begin();
    for (int it = 0; it < iterations && rc == 0; it++)
        rc = L.iteration(it);
    return rc;
}

// The same run for several engines of one GPU (the half-batches of selfplay.SelfPlay), their iterations enqueued in turn:
// enqueueing engine after engine lets the second one start only when the first one's whole run — two launches per iteration,
// a few milliseconds of host time per 250 iterations — has been enqueued, and finish that much later, alone on the chip.
extern "C" int azh_engines_run(azh_engine *const *engines, int n, azh_net *net, int dtype, int iterations)
{
    if (!engines || n < 1 || !net || iterations < 0)
        return azh_fail(-1, "azh_engines_run: bad argument");
    for (int i = 0; i < n; i++)
        if (!engines[i])
            return azh_fail(-1, "azh_engines_run: null engine");
    if (iterations == 0)
        return 0;
    std::vector<RunLoop> loops;
    for (int i = 0; i < n; i++)
        loops.push_back(RunLoop{engines[i], net, nullptr, dtype, iterations});
    int rc = 0;
    for (int i = 0; i < n && rc == 0; i++)
        rc = loops[i].begin();
    for (int it = 0; it < iterations && rc == 0; it++)
        for (int i = 0; i < n && rc == 0; i++)
            rc = loops[i].iteration(it);
    return rc;
}

extern "C" int azh_engine_run(azh_engine *e, azh_net *net, int dtype, int iterations)
{
    if (!e || !net || iterations < 0)
        return azh_fail(-1, "azh_engine_run: bad argument");
    return run_loop(e, net, nullptr, dtype, iterations);
}

extern "C" int azh_engine_run_arena(azh_engine *e, azh_net *net_a, azh_net *net_b, int dtype, int iterations)
{
    if (!e || !net_a || !net_b || iterations < 0)
        return azh_fail(-1, "azh_engine_run_arena: bad argument");
    if (!(e->P.flags & AZH_FLAG_TWO_NETS))
        return azh_fail(-2, "azh_engine_run_arena: engine was not created with AZH_FLAG_TWO_NETS");
    e->arena_lists = true;
    const int rc = run_loop(e, net_a, net_b, dtype, iterations);
    e->arena_lists = false;
    return rc;
}

// Diagnostic: two search iterations of the device loop, the tree launch between the two towers being the stamped
// instantiation of k_tree; out [games][10] u64 = s_memrealtime readings (100 MHz) per game: wave start, state loaded,
// backup done, mark done, descent done, expansion done, state stored, workgroup done; then the levels descended and the
// children scanned by that descent.
extern "C" int azh_engine_tree_stamps(azh_engine *e, azh_net *net, int dtype, uint64_t *out)
{
    if (!e || !net || !out)
        return azh_fail(-1, "azh_engine_tree_stamps: null argument");
    if (e->vl_active)
        return azh_fail(-2, "azh_engine_tree_stamps: not available with %d leaves per game%s", leaf_k(e),
                        vl_beside(e, " and").c_str());
    AZH_TRY(dev_alloc_once(e, &e->P.stamps, (size_t)e->P.G * TREE_STAMPS));
    AZH_HIP(hipMemsetAsync(e->P.stamps, 0, (size_t)e->P.G * TREE_STAMPS * 8, e->stream));
    e->stamp_next = true;
    const int rc = run_loop(e, net, nullptr, dtype, 2);
    e->stamp_next = false;
    if (rc)
        return rc;
    AZH_HIP(hipStreamSynchronize(e->stream));
    AZH_HIP(hipMemcpy(out, e->P.stamps, (size_t)e->P.G * TREE_STAMPS * 8, hipMemcpyDeviceToHost));
    return 0;
}

// Leaf-parallel search: K leaves per game and iteration, spread by a virtual loss of `virtual_loss` visits
// (vl_search.h), and the solver and the exploration mode on top of it.  k_vl_tree and the G K-slot buffers are in force while
// K > 1 or the solver, the exploration mode or search sets are on; K = 1 without any of them is the one-leaf search and its kernels.  `who`: the
// calling entry point, for its errors.  `explore`: null (the exploration mode stays as it is), or the three values of
// azh_engine_set_exploration, which are the call's request then.  `sets`: -1 (the search sets stay as they are), or the number
// of sets azh_engine_set_search_sets is about to put in force, which is the call's request then; that caller fills in the
// sets themselves once this has succeeded.
static int set_leaf_mode(azh_engine *e, int leaves_per_game, int virtual_loss, bool solver, const char *who,
                         const float *explore = nullptr, int sets = -1)
{
    const bool explore_on = explore ? exploration_on(explore[0], explore[1]) : explores(e);
    const bool sets_on = sets >= 0 ? sets > 0 : search_sets_on(e);
    const bool want = leaves_per_game > 1 || solver || explore_on || sets_on;
    AZH_TRY(mode_request(e, who, sets >= 0 ? (sets_on ? MODE_SEARCH_SETS : MODE_NONE)
                                 : explore ? (explore_on ? MODE_EXPLORATION : MODE_NONE)
                                 : leaves_per_game > 1 ? MODE_LEAF_BATCH : solver ? MODE_SOLVER : MODE_NONE));
    EngineParams &P = e->P;
    const size_t n = (size_t)P.G * (size_t)leaves_per_game;
    if (want && (int)n > e->vl_slots_cap) {
        // slot buffers for G K leaves (kept for the engine's life; a larger K later allocates again)
        LeafBuffers b;
        b.mask_words = (int)((n + 31) / 32);
        int rc = 0;
        rc |= dev_alloc(e, &e->V.kind, n);
        rc |= dev_alloc(e, &e->V.leaf_edge, n);
        rc |= dev_alloc(e, &e->V.leaf_node, n);
        rc |= dev_alloc(e, &e->V.path_len, n);
        rc |= dev_alloc(e, &e->V.path, n * (size_t)P.path_cap);
        rc |= dev_alloc(e, &b.leaf_board, n);
        rc |= dev_alloc(e, &b.leaf_mask, n);
        rc |= dev_alloc(e, &b.need_eval, n);
        rc |= dev_alloc(e, &b.leaf_list, n);
        rc |= dev_alloc(e, &b.need_mask, 2 * (size_t)b.mask_words);
        rc |= dev_alloc(e, &b.logits, n * AZH_POLICY_SIZE);
        rc |= dev_alloc(e, &b.values, n);
        if (rc) {
            e->g_leaves.write(P);
            e->V.K = 1;
            e->V.solver = 0;
            P.fpu_reduction = -1.0f;
            P.c_base = P.c_init = 0.0f;
            P.search_sets = nullptr;
            P.n_search_sets = 0;
            e->vl_active = false;
            e->vl_slots_cap = 0;
            return rc;
        }
        e->vl_leaves = b;
        e->vl_slots_cap = (int)n;
    }
    (want ? e->vl_leaves : e->g_leaves).write(P);
    e->V.K = leaves_per_game;
    e->V.vl = virtual_loss;
    e->V.solver = solver ? 1 : 0;
    if (explore) {
        P.fpu_reduction = explore[0] >= 0.0f ? explore[0] : -1.0f;
        P.c_base = explore[1];
        P.c_init = explore[1] > 0.0f ? explore[2] : 0.0f;  // (ignored with the constant c)
    }
    e->vl_active = want;
    return 0;
}

// Between iterations only; K = 1 restores the one-leaf search and its kernels (unless the solver is on).
extern "C" int azh_engine_set_leaf_batch(azh_engine *e, int leaves_per_game, int virtual_loss)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_leaf_batch: null engine");
    if (leaves_per_game < 1 || leaves_per_game > VL_MAX_LEAVES || virtual_loss < 1 || virtual_loss > VL_MAX_LOSS)
        return azh_fail(-2, "azh_engine_set_leaf_batch: need 1 <= leaves_per_game <= %d and 1 <= virtual_loss <= %d",
                        VL_MAX_LEAVES, VL_MAX_LOSS);
    for (int i = 0; i < e->P.n_search_sets; i++)
        if (leaves_per_game < e->sets[i].leaves)
            return azh_fail(-2, "azh_engine_set_leaf_batch: %d is below the leaves %d of search set %d", leaves_per_game,
                            e->sets[i].leaves, i);
    return set_leaf_mode(e, leaves_per_game, virtual_loss, e->V.solver != 0, "azh_engine_set_leaf_batch");
}

// Proven wins and losses on (every K through k_vl_tree, its backup followed by the proof pass) or off (today's dispatch;
// marks already in the tree stay).  Between iterations only.
extern "C" int azh_engine_set_solver(azh_engine *e, int on)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_solver: null engine");
    return set_leaf_mode(e, leaf_k(e), e->V.vl, on != 0, "azh_engine_set_solver");
}

// First-play urgency (fpu_reduction >= 0) and the exploration rate that grows with log N (c_base > 0) in the leaf-parallel
// kernel; while either is on every K — 1 included — runs through k_vl_tree, as under the solver.  Definition: the header and
// DESIGN.md.  Between iterations only.
extern "C" int azh_engine_set_exploration(azh_engine *e, float fpu_reduction, float c_base, float c_init)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_exploration: null engine");
    if (!std::isfinite(fpu_reduction) || !std::isfinite(c_base) || !std::isfinite(c_init) || c_base < 0.0f || c_init < 0.0f)
        return azh_fail(-2, "azh_engine_set_exploration: need finite arguments, c_base >= 0 and c_init >= 0");
    const float explore[3] = {fpu_reduction, c_base, c_init};
    return set_leaf_mode(e, leaf_k(e), e->V.vl, e->V.solver != 0, "azh_engine_set_exploration", explore);
}

// The three values in force: out [3] = fpu_reduction (-1: off), c_base (0: the constant c_puct), c_init.
extern "C" int azh_engine_exploration(const azh_engine *e, float *out)
{
    if (!e || !out)
        return azh_fail(-1, "azh_engine_exploration: bad argument");
    out[0] = e->P.fpu_reduction;
    out[1] = e->P.c_base;
    out[2] = e->P.c_init;
    return 0;
}

// One node's M scores under the rule of azh_engine_set_exploration, from the functions vl_select_game uses and the 64-lane
// sums restated on the host (gumbel_lane_sum).  Host arithmetic only.
extern "C" int azh_exploration_scores(const float *prior, const float *W, const uint32_t *n, int M, float c_puct, float fpu_reduction,
                                      float c_base, float c_init, float *scores_out)
{
    if (!prior || !W || !n || !scores_out || M < 1 || M > MAX_MOVES)
        return azh_fail(-1, "azh_exploration_scores: bad argument (need every array and 1 <= M <= %d)", MAX_MOVES);
    if (!std::isfinite(fpu_reduction) || !std::isfinite(c_base) || !std::isfinite(c_init) || c_base < 0.0f || c_init < 0.0f)
        return azh_fail(-2, "azh_exploration_scores: need finite arguments, c_base >= 0 and c_init >= 0");
    u32 N = 0;
    float tp[MAX_MOVES];
    for (int j = 0; j < M; j++) {
        N += n[j];
        tp[j] = n[j] ? fabsf(prior[j]) : 0.0f;
    }
    const float sq = sqrtf((float)(1u + N));
    float c = c_puct, f = 0.0f;
    if (exploration_on(fpu_reduction, c_base)) {
        c = exploration_c(N, c_puct, c_base, c_init);
        f = exploration_fpu(gumbel_lane_sum(W, M), gumbel_lane_sum(tp, M), N, fpu_reduction);
    }
    for (int j = 0; j < M; j++)
        scores_out[j] = exploration_score(fabsf(prior[j]), W[j], n[j], sq, c, f);
    return 0;
}

// Search settings per side: the two sides of a game search with a set each (its pairing: search_set_pairing), every K through
// k_vl_tree, and the device tallies the results by (set of x, set of o).  Definition: the header and DESIGN.md.  Between
// iterations only; n = 0 switches the mode off.
extern "C" int azh_engine_set_search_sets(azh_engine *e, int n, const azh_search_set *sets)
{
    const char *who = "azh_engine_set_search_sets";
    if (!e || (n > 0 && !sets))
        return azh_fail(-1, "%s: null argument", who);
    if (n < 0 || n > AZH_SEARCH_SETS_MAX)
        return azh_fail(-2, "%s: need 0 <= n <= %d", who, AZH_SEARCH_SETS_MAX);
    for (int i = 0; i < n; i++) {
        const azh_search_set &t = sets[i];
        if (t.visits < 1 || t.visits > e->P.visits)
            return azh_fail(-2, "%s: set %d: need 1 <= visits <= %d (the engine's)", who, i, e->P.visits);
        if (t.leaves < 1 || t.leaves > leaf_k(e))
            return azh_fail(-2, "%s: set %d: need 1 <= leaves <= %d (azh_engine_set_leaf_batch)", who, i, leaf_k(e));
        if (t.virtual_loss < 1 || t.virtual_loss > VL_MAX_LOSS || t.leaves * t.virtual_loss > VL_MAX_LEAVES * VL_MAX_LOSS)
            return azh_fail(-2, "%s: set %d: need 1 <= virtual_loss <= %d", who, i, VL_MAX_LOSS);
        if (!std::isfinite(t.c_puct) || t.c_puct < 0.0f)
            return azh_fail(-2, "%s: set %d: need a finite c_puct >= 0", who, i);
        if (!std::isfinite(t.fpu_reduction) || !std::isfinite(t.c_base) || !std::isfinite(t.c_init) || t.c_base < 0.0f || t.c_init < 0.0f)
            return azh_fail(-2, "%s: set %d: need finite arguments, c_base >= 0 and c_init >= 0", who, i);
    }
    if (n > 0) {  // (allocations change nothing a refused call could show; a failed one is the call's failure before any change)
        AZH_TRY(dev_alloc_once(e, &e->d_sets, (size_t)AZH_SEARCH_SETS_MAX));
        AZH_TRY(dev_alloc_once(e, &e->P.slot_sets, (size_t)e->P.G));
        AZH_TRY(dev_alloc_once(e, &e->P.set_stats, (size_t)AZH_SEARCH_SETS_MAX * AZH_SEARCH_SETS_MAX * AZH_SET_STAT_COUNT));
    }
    AZH_TRY(set_leaf_mode(e, leaf_k(e), e->V.vl, e->V.solver != 0, who, nullptr, n));  // (-3, -4; the stream is idle after it)
    for (int i = 0; i < n; i++) {
        e->sets[i] = sets[i];
        if (!(e->sets[i].fpu_reduction >= 0.0f))
            e->sets[i].fpu_reduction = -1.0f;
        if (!(e->sets[i].c_base > 0.0f))
            e->sets[i].c_init = 0.0f;  // (ignored with the constant c, as azh_engine_set_exploration)
    }
    e->P.n_search_sets = n;
    e->P.search_sets = n > 0 ? e->d_sets : nullptr;
    if (n == 0)
        return 0;
    AZH_HIP(hipMemcpy(e->d_sets, e->sets, (size_t)n * sizeof(azh_search_set), hipMemcpyHostToDevice));
    AZH_HIP(hipMemset(e->P.set_stats, 0, (size_t)AZH_SEARCH_SETS_MAX * AZH_SEARCH_SETS_MAX * AZH_SET_STAT_COUNT * 8));
    hipLaunchKernelGGL(k_slot_sets, dim3((e->P.G + 255) / 256), dim3(256), 0, e->stream, e->P);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// The sets in force: *n_out their number, sets_out (or null) the sets themselves.
extern "C" int azh_engine_search_sets(const azh_engine *e, int32_t *n_out, azh_search_set *sets_out)
{
    if (!e || !n_out)
        return azh_fail(-1, "azh_engine_search_sets: bad argument");
    *n_out = e->P.n_search_sets;
    for (int i = 0; sets_out && i < e->P.n_search_sets; i++)
        sets_out[i] = e->sets[i];
    return 0;
}

// out [2] = the set of x, the set of o in game `uid` among n sets.  Host arithmetic only: the function the kernels call.
extern "C" int azh_search_set_pairing(uint32_t uid, int n, int32_t *out)
{
    if (!out)
        return azh_fail(-1, "azh_search_set_pairing: null out");
    if (n < 1 || n > AZH_SEARCH_SETS_MAX)
        return azh_fail(-2, "azh_search_set_pairing: need 1 <= n <= %d", AZH_SEARCH_SETS_MAX);
    const u32 w = search_set_pairing(uid, (u32)n);
    out[0] = (int32_t)(w & 0xFFu);
    out[1] = (int32_t)(w >> 8);
    return 0;
}

// The tally of the games' results by (set of x, set of o) since the sets were set: out [n][n][AZH_SET_STAT_COUNT].
extern "C" int azh_engine_search_set_stats(azh_engine *e, uint64_t *out)
{
    if (!e || !out)
        return azh_fail(-1, "azh_engine_search_set_stats: bad argument");
    const size_t n = (size_t)e->P.n_search_sets;
    if (n == 0)
        return 0;
    AZH_HIP(hipStreamSynchronize(e->stream));
    AZH_HIP(hipMemcpy(out, e->P.set_stats, n * n * AZH_SET_STAT_COUNT * 8, hipMemcpyDeviceToHost));
    return 0;
}

// Sums over the games of the proof pass's counters: out [AZH_PROOF_STAT_COUNT].
extern "C" int azh_engine_proof_stats(azh_engine *e, uint64_t *out)
{
    if (!e || !out)
        return azh_fail(-1, "azh_engine_proof_stats: bad argument");
    AZH_HIP(hipStreamSynchronize(e->stream));
    std::vector<uint64_t> h((size_t)e->P.G * AZH_PROOF_STAT_COUNT);
    AZH_HIP(hipMemcpy(h.data(), e->V.proofs, h.size() * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < AZH_PROOF_STAT_COUNT; k++)
        out[k] = 0;
    for (size_t i = 0; i < h.size(); i++)
        out[i % AZH_PROOF_STAT_COUNT] += h[i];
    return 0;
}

// The current batch: per slot g K + p its kind (AZH_LEAF_*), leaf board (mover, opponent; zero unless the slot needs the
// net) and the last edge of its path (0xFFFFFFFF: none).  Any pointer may be NULL.
extern "C" int azh_engine_batch_leaves(azh_engine *e, int32_t *kind, uint64_t *leaf_boards, uint32_t *leaf_edge)
{
    if (!e)
        return azh_fail(-1, "azh_engine_batch_leaves: null engine");
    if (!e->vl_active)
        return azh_fail(-2, "azh_engine_batch_leaves: one leaf per game: use azh_engine_leaves");
    AZH_HIP(hipStreamSynchronize(e->stream));
    const size_t n = (size_t)e->P.G * leaf_k(e);
    if (kind)
        AZH_HIP(hipMemcpy(kind, e->V.kind, n * 4, hipMemcpyDeviceToHost));
    if (leaf_boards)
        AZH_HIP(hipMemcpy(leaf_boards, e->P.leaf_board, n * 16, hipMemcpyDeviceToHost));
    if (leaf_edge)
        AZH_HIP(hipMemcpy(leaf_edge, e->V.leaf_edge, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// Evaluations of the current batch from outside: logits [G K][833], values [G K], by slot.
extern "C" int azh_engine_set_batch_evals(azh_engine *e, const float *logits, const float *values)
{
    if (!e || !logits || !values)
        return azh_fail(-1, "azh_engine_set_batch_evals: null argument");
    if (!e->vl_active)
        return azh_fail(-2, "azh_engine_set_batch_evals: one leaf per game: use azh_engine_set_evals");
    const size_t n = (size_t)e->P.G * leaf_k(e);
    AZH_HIP(hipMemcpyAsync(e->P.logits, logits, n * AZH_POLICY_SIZE * 4, hipMemcpyHostToDevice, e->stream));
    AZH_HIP(hipMemcpyAsync(e->P.values, values, n * 4, hipMemcpyHostToDevice, e->stream));
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int azh_engine_set_thin_batches(azh_engine *e, int mode)
{
    if (!e || mode < -1 || mode > 1)
        return azh_fail(-1, "azh_engine_set_thin_batches: mode is -1 (by size), 0 or 1");
    e->thin_mode = mode;  // (host state only: takes effect with the next launches enqueued)
    return 0;
}

// The considered-visits rows r = 1 .. m of the Gumbel root search for a threshold of `visits`, on the device (the stream is idle).
static int gumbel_upload_table(azh_engine *e, int m, int visits)
{
    const size_t n = (size_t)m * (size_t)visits;
    std::vector<u16> h(n);
    for (int r = 1; r <= m; r++)
        gumbel_considered_visits(r, visits, h.data() + (size_t)(r - 1) * visits);
    if (n > e->gumbel_seq_cap) {
        if (dev_alloc(e, &e->d_gumbel_seq, n))
            return -1;
        e->gumbel_seq_cap = n;
    }
    AZH_HIP(hipMemcpy(e->d_gumbel_seq, h.data(), n * sizeof(u16), hipMemcpyHostToDevice));
    e->P.gumbel_seq = e->d_gumbel_seq;
    return 0;
}

// Root-visit threshold for the coming moves (1 .. the value the engine was created with; the
// arenas are sized for that).  Takes effect at the next k_advance.
extern "C" int azh_engine_set_visits(azh_engine *e, int visits)
{
    if (!e || visits < 1 || visits > e->cfg.visits)
        return azh_fail(-1, "azh_engine_set_visits: need 1 <= visits <= %d", e ? e->cfg.visits : 0);
    if (visits < e->P.fast_visits)
        return azh_fail(-2, "azh_engine_set_visits: %d is below the playout cap's fast_visits %d", visits, e->P.fast_visits);
    for (int i = 0; i < e->P.n_search_sets; i++)
        if (visits < e->sets[i].visits)
            return azh_fail(-2, "azh_engine_set_visits: %d is below the visits %d of search set %d", visits, e->sets[i].visits, i);
    if (e->P.gumbel_m != 0 && (long long)e->P.gumbel_m * visits > GUMBEL_MAX_TABLE)
        return azh_fail(-2, "azh_engine_set_visits: the Gumbel root search is on with m = %d: m * visits may not exceed %d",
                        e->P.gumbel_m, GUMBEL_MAX_TABLE);
    AZH_HIP(hipStreamSynchronize(e->stream));
    if (e->P.gumbel_m != 0 && gumbel_upload_table(e, e->P.gumbel_m, visits))  // (the rows for the new threshold)
        return -1;
    e->P.visits = visits;
    return 0;
}

// Playout cap randomization: FAST plies (threshold fast_visits, no root noise) and FULL plies (threshold `visits`, noise),
// the kind a pure function of (seed, uid, ply).  Definition: the header and DESIGN.md.  Between iterations only.
extern "C" int azh_engine_set_playout_cap(azh_engine *e, int fast_visits, int full_per_65536)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_playout_cap: null engine");
    if (fast_visits < 0 || fast_visits > e->P.visits || full_per_65536 < 0 || full_per_65536 > 65536)
        return azh_fail(-2, "azh_engine_set_playout_cap: need 0 <= fast_visits <= visits (%d) and 0 <= full_per_65536 <= 65536",
                        e->P.visits);
    AZH_TRY(mode_request(e, "azh_engine_set_playout_cap", fast_visits != 0 ? MODE_CAP : MODE_NONE));
    if (fast_visits == 0) {
        e->P.fast_visits = 0;
        e->P.full_per_65536 = 0;
        return 0;
    }
    if (dev_alloc_once(e, &e->P.ply_kind, (size_t)e->P.G))
        return -1;
    e->P.fast_visits = fast_visits;
    e->P.full_per_65536 = (u32)full_per_65536;
    hipLaunchKernelGGL(k_ply_kinds, dim3((e->P.G + 255) / 256), dim3(256), 0, e->stream, e->P);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// The kind of ply `ply` of game `uid` under `seed`: 1 FULL, 0 FAST.  Host arithmetic only.
extern "C" int azh_playout_cap_kind(uint64_t seed, uint32_t uid, uint32_t ply, uint32_t full_per_65536)
{
    return playout_cap_full((u32)seed, (u32)(seed >> 32), uid, ply, full_per_65536) ? 1 : 0;
}

// Forced playouts at the root and policy target pruning in the record (KataGo), on the plies whose root priors get the
// Dirichlet mix.  Definition: the header and DESIGN.md.  Between iterations only.
extern "C" int azh_engine_set_forced_playouts(azh_engine *e, float k)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_forced_playouts: null engine");
    if (!(k >= 0.0f) || k > 3.0e38f)
        return azh_fail(-2, "azh_engine_set_forced_playouts: need a finite k >= 0 (0: off)");
    AZH_TRY(mode_request(e, "azh_engine_set_forced_playouts", k != 0.0f ? MODE_FORCED : MODE_NONE));
    e->P.forced_k = k;
    return 0;
}

// The visit counts policy target pruning writes for a root (out [M]; 0: the edge is left out of the record).  Host arithmetic
// only: the rule advance_game applies, forced_prune_edge.
extern "C" int azh_forced_prune(const float *prior, const float *W, const uint32_t *n, int M, float k, float c_puct, uint32_t *out)
{
    if (!prior || !W || !n || !out || M < 0)
        return azh_fail(-1, "azh_forced_prune: bad argument");
    if (!(k >= 0.0f) || k > 3.0e38f)
        return azh_fail(-2, "azh_forced_prune: need a finite k >= 0");
    forced_prune_root(prior, W, n, M, k, c_puct, out);
    return 0;
}

// Gumbel root search with sequential halving (Danihelka et al., ICLR 2022).  Definition: the header and DESIGN.md.  Between
// iterations only.
extern "C" int azh_engine_set_gumbel(azh_engine *e, int m, float c_visit, float c_scale)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_gumbel: null engine");
    if (m < 0 || m > GUMBEL_MAX_ACTIONS)
        return azh_fail(-2, "azh_engine_set_gumbel: need 0 <= m <= %d (0: off)", GUMBEL_MAX_ACTIONS);
    if (m != 0 && (!(c_visit >= 0.0f) || c_visit > 3.0e38f || !(c_scale > 0.0f) || c_scale > 3.0e38f))
        return azh_fail(-2, "azh_engine_set_gumbel: need a finite c_visit >= 0 and a finite c_scale > 0");
    if ((long long)m * e->P.visits > GUMBEL_MAX_TABLE)
        return azh_fail(-2, "azh_engine_set_gumbel: m * visits = %lld may not exceed %d", (long long)m * e->P.visits,
                        GUMBEL_MAX_TABLE);
    AZH_TRY(mode_request(e, "azh_engine_set_gumbel", m != 0 ? MODE_GUMBEL : MODE_NONE));
    if (m == 0) {
        e->P.gumbel_m = 0;
        e->P.gumbel_c_visit = 0.0f;
        e->P.gumbel_c_scale = 0.0f;
        return 0;
    }
    const size_t G = (size_t)e->P.G;
    if (dev_alloc_once(e, &e->P.gumbel_a, G * MAX_MOVES) || dev_alloc_once(e, &e->P.gumbel_v0, G))
        return -1;
    if (gumbel_upload_table(e, m, e->P.visits))
        return -1;
    if (e->P.gumbel_m == 0) {
        // a ply whose root was evaluated before the mode came on has no noise of its own: it is searched with a_j = 0 and
        // a root value of one half (the next root evaluation of the slot writes both)
        const std::vector<float> half(G, 0.5f);
        AZH_HIP(hipMemset(e->P.gumbel_a, 0, G * MAX_MOVES * sizeof(float)));
        AZH_HIP(hipMemcpy(e->P.gumbel_v0, half.data(), G * sizeof(float), hipMemcpyHostToDevice));
    }
    e->P.gumbel_c_visit = c_visit;
    e->P.gumbel_c_scale = c_scale;
    e->P.gumbel_m = m;
    return 0;
}

// One row of the schedule: the considered visit counts for m actions and `visits` simulations, out [visits].  Host arithmetic only.
extern "C" int azh_gumbel_considered_visits(int m, int visits, uint16_t *out)
{
    if (!out || m < 1 || m > GUMBEL_MAX_ACTIONS || visits < 1 || visits > 60000)
        return azh_fail(-1, "azh_gumbel_considered_visits: bad argument (need out, 1 <= m <= %d and 1 <= visits <= 60000)",
                        GUMBEL_MAX_ACTIONS);
    gumbel_considered_visits(m, visits, out);
    return 0;
}

// g_j of the root edges j < M of ply `ply` of game `uid` under `seed`, out [M].  Host arithmetic only.
extern "C" int azh_gumbel_noise(uint64_t seed, uint32_t uid, uint32_t ply, int M, float *out)
{
    if (!out || M < 0 || M > MAX_MOVES)
        return azh_fail(-1, "azh_gumbel_noise: bad argument (need out and 0 <= M <= %d)", MAX_MOVES);
    for (int j = 0; j < M; j++)
        out[j] = gumbel_noise((u32)seed, (u32)(seed >> 32), uid, ply, (u32)j);
    return 0;
}

// The move and the record's counts of a whole root: the device's ply restated on the host (gumbel_root).  Host arithmetic only.
extern "C" int azh_gumbel_root(const float *prior, const float *W, const uint32_t *n, int M, float v0, const float *noise,
                               float c_visit, float c_scale, uint32_t *counts_out, int32_t *move_out)
{
    if (!prior || !W || !n || !noise || !counts_out || !move_out || M < 1 || M > MAX_MOVES)
        return azh_fail(-1, "azh_gumbel_root: bad argument (need every array and 1 <= M <= %d)", MAX_MOVES);
    if (!(c_visit >= 0.0f) || c_visit > 3.0e38f || !(c_scale > 0.0f) || c_scale > 3.0e38f)
        return azh_fail(-2, "azh_gumbel_root: need a finite c_visit >= 0 and a finite c_scale > 0");
    *move_out = gumbel_root(prior, W, n, M, v0, noise, c_visit, c_scale, counts_out);
    return 0;
}

// The search's own value in every ply's record, and resignation of decided games.  Definition: the header and DESIGN.md.
// Between iterations only; every slot's counters are cleared.
extern "C" int azh_engine_set_resign(azh_engine *e, float q_below, int consecutive, int playthrough_per_65536)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_resign: null engine");
    if (consecutive < 0 || consecutive > 255)
        return azh_fail(-2, "azh_engine_set_resign: need 0 <= consecutive <= 255 (0: off)");
    if (consecutive != 0 && (!(q_below >= 0.0f) || !(q_below < 1.0f) || playthrough_per_65536 < 0 || playthrough_per_65536 > 65536))
        return azh_fail(-2, "azh_engine_set_resign: need 0 <= q_below < 1 and 0 <= playthrough_per_65536 <= 65536");
    AZH_TRY(mode_request(e, "azh_engine_set_resign", consecutive != 0 ? MODE_RESIGN : MODE_NONE));
    if (consecutive == 0) {
        e->P.resign_plies = 0u;
        e->P.resign_below = 0.0f;
        e->P.resign_through = 0u;
        return 0;
    }
    if (dev_alloc_once(e, &e->P.resign_state, (size_t)e->P.G) || dev_alloc_once(e, &e->P.resign_stats, (size_t)AZH_RESIGN_STAT_COUNT))
        return -1;
    AZH_HIP(hipMemset(e->P.resign_state, 0, (size_t)e->P.G * sizeof(u32)));
    e->P.resign_below = q_below;
    e->P.resign_plies = (u32)consecutive;
    e->P.resign_through = (u32)playthrough_per_65536;
    return 0;
}

// Per-ply temperature of the move played and of the root policy.  Definition: the header and DESIGN.md.  Between iterations
// only.
static bool temperature_entry_ok(float t, bool move)
{
    if (move)
        return t == 0.0f || (t >= 1.0f / 64.0f && t <= 64.0f);  // (false for a NaN)
    return t >= 0.25f && t <= 64.0f;
}

extern "C" int azh_engine_set_temperature(azh_engine *e, const float *move_temperature, const float *root_policy_temperature)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_temperature: null engine");
    const int n = e->P.max_plies;
    for (int p = 0; move_temperature && p < n; p++)
        if (!temperature_entry_ok(move_temperature[p], true))
            return azh_fail(-2, "azh_engine_set_temperature: move_temperature[%d] = %g: need 0 or 1/64 <= T <= 64", p,
                            (double)move_temperature[p]);
    for (int p = 0; root_policy_temperature && p < n; p++)
        if (!temperature_entry_ok(root_policy_temperature[p], false))
            return azh_fail(-2, "azh_engine_set_temperature: root_policy_temperature[%d] = %g: need 1/4 <= R <= 64", p,
                            (double)root_policy_temperature[p]);
    AZH_TRY(mode_request(e, "azh_engine_set_temperature", move_temperature || root_policy_temperature ? MODE_TEMPERATURE : MODE_NONE));
    // the engine's two tables are allocated once and kept; a null argument only takes the pointer out of the parameters
    if (move_temperature && dev_alloc_once(e, &e->d_move_temperature, (size_t)n))
        return -1;
    if (root_policy_temperature && dev_alloc_once(e, &e->d_root_policy_temperature, (size_t)n))
        return -1;
    if (move_temperature)
        AZH_HIP(hipMemcpy(e->d_move_temperature, move_temperature, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    if (root_policy_temperature)
        AZH_HIP(hipMemcpy(e->d_root_policy_temperature, root_policy_temperature, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    e->P.move_temperature = move_temperature ? e->d_move_temperature : nullptr;
    e->P.root_policy_temperature = root_policy_temperature ? e->d_root_policy_temperature : nullptr;
    return 0;
}

// The move a ply's temperature chooses from a root's visit counts: the device's choice restated on the host
// (temperature_pick_root).  Returns the edge index; q_out (or null) receives the M weights.  Host arithmetic only.
extern "C" int azh_temperature_pick(const uint32_t *visits, int M, float temperature, uint64_t seed, uint32_t uid, uint32_t ply,
                                    uint32_t *q_out)
{
    if (!visits || M < 1 || M > MAX_MOVES)
        return azh_fail(-1, "azh_temperature_pick: bad argument (need visits and 1 <= M <= %d)", MAX_MOVES);
    if (!temperature_entry_ok(temperature, true))
        return azh_fail(-2, "azh_temperature_pick: temperature %g: need 0 or 1/64 <= T <= 64", (double)temperature);
    const Philox4 rr = philox((u32)seed, (u32)(seed >> 32), uid, ply, STREAM_SAMPLE, 0u);
    return temperature_pick_root(visits, M, temperature, rr.v[0], q_out);
}

// Is game `uid` under `seed` a play-through game?  Host arithmetic only.
extern "C" int azh_resign_playthrough(uint64_t seed, uint32_t uid, uint32_t playthrough_per_65536)
{
    return resign_playthrough((u32)seed, (u32)(seed >> 32), uid, playthrough_per_65536) ? 1 : 0;
}

// The once-per-game counts of the resign rule since create: out [AZH_RESIGN_STAT_COUNT] (zeros before the mode was ever on).
extern "C" int azh_engine_resign_stats(azh_engine *e, uint64_t *out)
{
    if (!e || !out)
        return azh_fail(-1, "azh_engine_resign_stats: bad argument");
    for (int k = 0; k < AZH_RESIGN_STAT_COUNT; k++)
        out[k] = 0;
    if (!e->P.resign_stats)
        return 0;
    AZH_HIP(hipStreamSynchronize(e->stream));
    AZH_HIP(hipMemcpy(out, e->P.resign_stats, AZH_RESIGN_STAT_COUNT * 8, hipMemcpyDeviceToHost));
    return 0;
}

// Random symmetry per evaluation: every position goes to the evaluator as its image under a symmetry that is a pure function
// of (seed, uid, position), and its logits are gathered through the same symmetry's move map.  Definition: the header and
// DESIGN.md.  Between iterations only.
extern "C" int azh_engine_set_random_symmetry(azh_engine *e, int on)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_random_symmetry: null engine");
    AZH_TRY(mode_request(e, "azh_engine_set_random_symmetry", on ? MODE_SYMMETRY : MODE_NONE));
    if (!on) {
        e->P.random_symmetry = 0u;
        return 0;
    }
    if (dev_alloc_once(e, &e->P.eval_key, (size_t)e->P.G))
        return -1;
    e->P.random_symmetry = 1u;
    hipLaunchKernelGGL(k_eval_keys, dim3((e->P.G + 255) / 256), dim3(256), 0, e->stream, e->P);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// The symmetry (0..7) under which the position (mover, opponent) of game `uid` is evaluated by an engine created with `seed`.
// Host arithmetic only: the functions the kernels call.
extern "C" int azh_eval_symmetry(uint64_t seed, uint32_t uid, uint64_t mover, uint64_t opponent)
{
    return eval_symmetry_of(eval_symmetry_key((u32)seed, (u32)(seed >> 32), uid), mover, opponent);
}

// T_s on a bitboard (bits beyond the 49 cells are dropped; s is taken modulo 8).  Host arithmetic only.
extern "C" uint64_t azh_symmetry_board(int s, uint64_t bitboard) { return symmetry_board(s & 7, bitboard); }

// T_s on a flat policy index (all 833: the permutation that brings an image's logits back).  Host arithmetic only.
extern "C" int azh_symmetry_policy_index(int s, int index)
{
    if (s < 0 || s > 7 || index < 0 || index >= AZH_POLICY_SIZE)
        return azh_fail(-1, "azh_symmetry_policy_index: need 0 <= s <= 7 and 0 <= index < %d", AZH_POLICY_SIZE);
    return symmetry_policy_index(s, index);
}

// T_s on a move (u16 from | to << 8; a value that is no board move, a pass, comes back as it is).  Host arithmetic only.
extern "C" int azh_symmetry_move(int s, uint16_t move)
{
    if (s < 0 || s > 7)
        return azh_fail(-1, "azh_symmetry_move: need 0 <= s <= 7");
    return (int)symmetry_move(s, (u32)move);
}

// At most `games` games are played: uids 0 .. games - 1 (slot g plays uids g, g + G, ...).  A slot whose next game
// would be past the limit goes idle, so the batch thins out as the last games end and no search is spent on games
// nobody asked for — what a generator given a target count (accelerated_generate_games.py --game-count) wants in
// uid order, where line N only appears once the slowest of the first N games has ended.  The limit may be RAISED later
// (games that were dropped leave the caller short of lines): idle slots whose next game is now below it start it.
// Games that have begun are never stopped.  A slot past the limit that has not begun (game_unbegun: at ply 0, or at the ply
// azh_engine_set_positions loaded it at) goes idle and keeps what it holds; raised, it resumes that game.  The contract: the
// header.
extern "C" int azh_engine_set_game_limit(azh_engine *e, int64_t games)
{
    if (!e || games < 1 || games > 0xFFFFFFFFll)
        return azh_fail(-1, "azh_engine_set_game_limit: bad argument");
    AZH_HIP(hipStreamSynchronize(e->stream));
    e->P.uid_limit = (u32)games;
    hipLaunchKernelGGL(k_limit_slots, dim3(e->P.G), dim3(WAVE), 0, e->stream, e->P);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// Order in which finished games are handed out.  0 (default): as they finish.  1: by game uid — a game waits until
// every game with a smaller uid has been written or dropped.  Games that finish first are the SHORT ones, so a
// consumer that stops reading after N lines (looper.py:51-64 kills the generator at --game-count lines) gets a
// length-biased sample in finish order; in uid order the first N lines are the first N games started, whatever
// their length.
extern "C" int azh_engine_set_record_blockers(azh_engine *e, int on)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_record_blockers: null engine");
    e->record_blockers = on != 0;  // (read when fetched records are formatted: takes effect from the next fetch on)
    return 0;
}

extern "C" int azh_engine_set_emit_order(azh_engine *e, int by_uid)
{
    if (!e)
        return azh_fail(-1, "azh_engine_set_emit_order: null engine");
    if (e->next_uid != 0 || !e->held.empty())
        return azh_fail(-2, "azh_engine_set_emit_order: games have already been handed out in uid order");
    e->emit_by_uid = by_uid != 0;
    return 0;
}

// A start position and wall map per game: the header.  Validation first, then the change: a refused call leaves the engine as it was.
extern "C" int azh_start_pool_entry(uint32_t uid, int n, int stride)
{
    if (n < 1 || stride < 1)
        return azh_fail(-1, "azh_start_pool_entry: need n >= 1 and stride >= 1");
    return (int)start_pool_entry(uid, (u32)n, (u32)stride);
}

extern "C" int azh_engine_uid_blockers(const azh_engine *e, uint32_t uid, uint64_t *out)
{
    if (!e || !out)
        return azh_fail(-1, "azh_engine_uid_blockers: null argument");
    *out = uid_blockers(e, uid) & BOARD_MASK;
    return 0;
}

extern "C" int azh_engine_set_start_pool(azh_engine *e, int n, const uint64_t *x, const uint64_t *o, const uint64_t *blockers,
                                         const int32_t *turn, int stride)
{
    const char *who = "azh_engine_set_start_pool";
    if (!e || (n > 0 && (!x || !o || !blockers || !turn)))
        return azh_fail(-1, "%s: null argument", who);
    if (n < 0 || n > AZH_START_POOL_MAX || (n > 0 && stride < 1))
        return azh_fail(-2, "%s: need 0 <= n <= %d and stride >= 1 (n %d, stride %d)", who, AZH_START_POOL_MAX, n, stride);
    std::vector<StartEntry> pool((size_t)n);
    for (int i = 0; i < n; i++) {
        const u64 bx = x[i], bo = o[i], bl = blockers[i];
        const char *why = nullptr;
        if ((bx | bo | bl) & ~BOARD_MASK)
            why = "bits beyond the 49 cells";
        else if (bx & bo)
            why = "a cell holds stones of both sides";
        else if ((bx | bo) & bl)
            why = "a stone stands on a wall";
        else if (!bx || !bo)
            why = "a side has no stone";
        else if (turn[i] != 0 && turn[i] != 1)
            why = "the side to move is neither 0 (x) nor 1 (o)";
        else {
            // (get_board_result: the board is full, or the side to move cannot move and the empty cells go to the other)
            const u64 empty = BOARD_MASK & ~(bx | bo | bl), own = turn[i] ? bo : bx;
            if (!((single_jump_bb(own) | double_jump_bb(own)) & empty))
                why = "the position is finished (the side to move has no move)";
        }
        if (why)
            return azh_fail(-2, "%s: entry %d (x %#llx, o %#llx, blockers %#llx, turn %d): %s", who, i, (unsigned long long)bx,
                            (unsigned long long)bo, (unsigned long long)bl, (int)turn[i], why);
        pool[(size_t)i] = StartEntry{bx, bo, bl, (int)turn[i], 0};
    }
    if (e->selected)
        return azh_fail(-3, "%s: a selected batch awaits its backup", who);
    if (e->begun)
        return azh_fail(-4, "%s: the engine has begun to search (the pool, like the start position it replaces, is set before "
                            "the first select)", who);
    if (n > 0 && e->P.random_symmetry != 0u) {
        const std::string why = asymmetric_mask(pool.data(), pool.size(), 0ULL);
        if (!why.empty())
            return azh_fail(-4, "%s: the random symmetry is not supported with %s", who, why.c_str());
    }
    AZH_HIP(hipStreamSynchronize(e->stream));
    if ((size_t)n > e->pool_cap) {
        StartEntry *d = nullptr;
        AZH_TRY(dev_alloc(e, &d, (size_t)n));
        e->d_pool = d;
        e->pool_cap = (size_t)n;
    }
    if (n > 0)
        AZH_HIP(hipMemcpy(e->d_pool, pool.data(), (size_t)n * sizeof(StartEntry), hipMemcpyHostToDevice));
    e->pool.swap(pool);
    e->P.pool = n > 0 ? e->d_pool : nullptr;
    e->P.pool_n = (u32)n;
    e->P.pool_stride = n > 0 ? (u32)stride : 0u;
    // every slot starts again: the game of its uid from its entry (n = 0: from the configured start position)
    hipLaunchKernelGGL(k_restart, dim3(e->P.G), dim3(WAVE), 0, e->stream, e->P);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// Every slot restarts at a given position: boards [G][2] packed (x | turn << 63, o), plies [G] (the ply the position is at;
// < max_plies).  Fresh trees, uids = slot numbers.  Games started this way are played and counted like any other, but
// their records would lack the plies before the start, so they are not written (the slot's NEXT game is a normal one).
// Under a game limit in force the slots past it are loaded and left idle (k_init_positions), as the limit set afterwards
// leaves them.
// A measurement set-up hook: bench.py loads the positions a long-running generator was found at
// (profiles/round2_steady_state_positions.npz) instead of waiting a game generation for the steady state to form.
extern "C" int azh_engine_set_positions(azh_engine *e, const uint64_t *boards, const int32_t *plies)
{
    if (!e || !boards || !plies)
        return azh_fail(-1, "azh_engine_set_positions: null argument");
    AZH_HIP(hipStreamSynchronize(e->stream));
    const size_t G = (size_t)e->P.G;
    // uids restart at the slot numbers: whatever the previous games left behind (undrained records, games held back
    // for uid order) belongs to uids that are about to be reused, and is discarded with them
    e->pending.clear();
    e->pending_pos = 0;
    e->staged.clear();
    e->held.clear();
    e->next_uid = 0;
    e->order_broken = false;
    AZH_HIP(hipMemsetAsync(e->P.ring_head, 0, 8, e->stream));
    for (size_t g = 0; g < G; g++) {
        const uint64_t x = boards[2 * g] & ~TURN_BIT, o = boards[2 * g + 1];
        if (plies[g] < 0 || plies[g] >= e->P.max_plies || (x & o) || ((x | o) & (uid_blockers(e, (u32)g) | ~BOARD_MASK)) || !x || !o)
            return azh_fail(-2, "azh_engine_set_positions: slot %zu: bad position or ply %d", g, plies[g]);
    }
    ulonglong2 *d_b = nullptr;
    int *d_p = nullptr;
    hipError_t rc = hipMalloc((void **)&d_b, G * 16);
    if (rc == hipSuccess) rc = hipMalloc((void **)&d_p, G * 4);
    if (rc == hipSuccess) rc = hipMemcpy(d_b, boards, G * 16, hipMemcpyHostToDevice);
    if (rc == hipSuccess) rc = hipMemcpy(d_p, plies, G * 4, hipMemcpyHostToDevice);
    if (rc == hipSuccess) rc = hipMemsetAsync(e->P.adv_count, 0, sizeof(int), e->stream);
    if (rc == hipSuccess) {
        hipLaunchKernelGGL(k_init_positions, dim3(e->P.G), dim3(WAVE), 0, e->stream, e->P, (const ulonglong2 *)d_b, (const int *)d_p);
        rc = hipStreamSynchronize(e->stream);
    }
    (void)hipFree(d_b);
    (void)hipFree(d_p);
    AZH_HIP(rc);
    return 0;
}

// The host names the move of every slot (moves [G], 0xFFFF: none); status_out [G] = AZH_PLAY_*.  Definition: the header.
extern "C" int azh_engine_play_moves(azh_engine *e, const uint16_t *moves, int32_t *status_out)
{
    if (!e || !moves || !status_out)
        return azh_fail(-1, "azh_engine_play_moves: null argument");
    if (e->selected)
        return azh_fail(-3, "azh_engine_play_moves: a selected batch awaits its backup");
    if (e->P.flags & AZH_FLAG_TWO_NETS)
        return azh_fail(-4, "azh_engine_play_moves: not available on AZH_FLAG_TWO_NETS engines");
    const size_t G = (size_t)e->P.G;
    if (dev_alloc_once(e, &e->d_play_moves, G) || dev_alloc_once(e, &e->d_play_status, G))
        return -1;
    AZH_HIP(hipMemcpyAsync(e->d_play_moves, moves, G * sizeof(u16), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_play_moves, dim3(e->P.G), dim3(WAVE), 0, e->stream, e->P, (const u16 *)e->d_play_moves, e->d_play_status);
    hipLaunchKernelGGL(k_unqueue_played, dim3(1), dim3(WAVE), 0, e->stream, e->P);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipMemcpyAsync(status_out, e->d_play_status, G * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// Root edges and principal variation of n_games slots: n_games records of AZH_ROOT_REPORT_WORDS u32 (layout: the header).
extern "C" int azh_engine_root_report(azh_engine *e, int first_game, int n_games, uint32_t *out)
{
    if (!e || !out || first_game < 0 || n_games < 1 || first_game > e->P.G - n_games)
        return azh_fail(-1, "azh_engine_root_report: bad argument");
    if (dev_alloc_once(e, &e->d_report, (size_t)e->P.G * AZH_ROOT_REPORT_WORDS))
        return -1;
    hipLaunchKernelGGL(k_root_report, dim3(n_games), dim3(WAVE), 0, e->stream, e->P, first_game, e->d_report);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipMemcpyAsync(out, e->d_report, (size_t)n_games * AZH_ROOT_REPORT_WORDS * 4, hipMemcpyDeviceToHost, e->stream));
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// The same records left in a device array of the caller's: no copy to the host (azh_samples_retarget reads them there).
extern "C" int azh_engine_root_report_device(azh_engine *e, int first_game, int n_games, uint32_t *d_out)
{
    if (!e || !d_out || first_game < 0 || n_games < 1 || first_game > e->P.G - n_games)
        return azh_fail(-1, "azh_engine_root_report_device: bad argument");
    hipLaunchKernelGGL(k_root_report, dim3(n_games), dim3(WAVE), 0, e->stream, e->P, first_game, d_out);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// Decided values of the root and of its edges' children: n_games records of AZH_ROOT_PROOF_WORDS i32 (layout: the header).
extern "C" int azh_engine_root_proofs(azh_engine *e, int first_game, int n_games, int32_t *out)
{
    if (!e || !out || first_game < 0 || n_games < 1 || first_game > e->P.G - n_games)
        return azh_fail(-1, "azh_engine_root_proofs: bad argument");
    if (dev_alloc_once(e, &e->d_proofs, (size_t)e->P.G * AZH_ROOT_PROOF_WORDS))
        return -1;
    hipLaunchKernelGGL(k_root_proofs, dim3(n_games), dim3(WAVE), 0, e->stream, e->P, first_game, e->d_proofs);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipMemcpyAsync(out, e->d_proofs, (size_t)n_games * AZH_ROOT_PROOF_WORDS * 4, hipMemcpyDeviceToHost, e->stream));
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int azh_engine_sync(azh_engine *e)
{
    if (!e)
        return azh_fail(-1, "azh_engine_sync: null engine");
    AZH_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

extern "C" int azh_engine_game_state(azh_engine *e, int game, azh_game_state *out)
{
    if (!e || !out || game < 0 || game >= e->P.G)
        return azh_fail(-1, "azh_engine_game_state: bad argument");
    AZH_HIP(hipStreamSynchronize(e->stream));
    AZH_HIP(hipMemcpy(out, e->P.gs + game, sizeof(azh_game_state), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int azh_engine_tree(azh_engine *e, int game, uint64_t *boards, uint32_t *info, uint32_t *edges,
                               uint16_t *moves)
{
    if (!e || game < 0 || game >= e->P.G)
        return azh_fail(-1, "azh_engine_tree: bad argument");
    azh_game_state s;
    if (azh_engine_game_state(e, game, &s))
        return -1;
    const size_t slot = (size_t)s.arena * e->P.G + game;
    if (boards) AZH_HIP(hipMemcpy(boards, e->P.node_board + slot * e->P.node_cap, (size_t)s.n_nodes * 16, hipMemcpyDeviceToHost));
    if (info) AZH_HIP(hipMemcpy(info, e->P.node_info + slot * e->P.node_cap, (size_t)s.n_nodes * 16, hipMemcpyDeviceToHost));
    if (edges) {
        AZH_HIP(hipMemcpy(edges, e->P.edge + slot * e->P.edge_cap, (size_t)s.n_edges * 16, hipMemcpyDeviceToHost));
        for (int j = 0; j < s.n_edges; j++) {  // device record (prior, W, visits | child << 16, child's range) -> documented row
            uint32_t *r = edges + 4 * (size_t)j;
            const uint32_t w = r[1], z = r[2];
            r[0] &= PRIOR_MASK;  // (the sign bit is the descent's mark, not part of the tree)
            r[1] = z & 0xFFFFu;
            r[2] = w;
            r[3] = (z >> 16) == 0xFFFFu ? 0xFFFFFFFFu : (z >> 16);
        }
    }
    if (moves) AZH_HIP(hipMemcpy(moves, e->P.edge_move + slot * e->P.edge_cap, (size_t)s.n_edges * 2, hipMemcpyDeviceToHost));
    return 0;
}

// Diagnostic: the game's edge records as they lie in HBM (the 16-byte device record described at the top of this file,
// the descent's mark in bit 31 of word 0 included) — what azh_engine_tree turns into the documented rows.  For the test
// of the mark's invariants: at most one marked edge per node, and only on an edge whose child exists, is unfinished and
// has 1 .. 128 moves.
extern "C" int azh_engine_tree_raw(azh_engine *e, int game, uint32_t *edges)
{
    if (!e || !edges || game < 0 || game >= e->P.G)
        return azh_fail(-1, "azh_engine_tree_raw: bad argument");
    azh_game_state s;
    if (azh_engine_game_state(e, game, &s))
        return -1;
    const size_t slot = (size_t)s.arena * e->P.G + game;
    AZH_HIP(hipMemcpy(edges, e->P.edge + slot * e->P.edge_cap, (size_t)s.n_edges * 16, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int azh_engine_stats(azh_engine *e, uint64_t *out)
{
    if (!e || !out)
        return azh_fail(-1, "azh_engine_stats: bad argument");
    hipLaunchKernelGGL(k_reduce_stats, dim3(NSTAT), dim3(256), 0, e->stream, (const u64 *)e->P.stats, e->P.G, e->d_stat_out);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipStreamSynchronize(e->stream));
    AZH_HIP(hipMemcpy(out, e->d_stat_out, NSTAT * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int azh_engine_timing_reset(azh_engine *e, int enable)
{
    if (!e)
        return azh_fail(-1, "azh_engine_timing_reset: null engine");
    AZH_HIP(hipStreamSynchronize(e->stream));
    e->timing_stride = enable > 0 ? enable : 0;
    e->samples = 0;
    e->close_pending = false;
    e->loop_iter = 0;
    if (e->timing_stride && e->events.empty()) {
        e->events.resize(3 * MAX_TIMED_SAMPLES);
        for (auto &ev : e->events)
            AZH_HIP(hipEventCreate(&ev));
        e->close_of.assign(MAX_TIMED_SAMPLES, -1);
    }
    return 0;
}

extern "C" int azh_engine_timing(azh_engine *e, azh_timing *out)
{
    if (!e || !out)
        return azh_fail(-1, "azh_engine_timing: bad argument");
    AZH_HIP(hipStreamSynchronize(e->stream));
    memset(out, 0, sizeof(*out));
    for (size_t i = 0; i < e->samples; i++) {
        if (e->close_of[i] < 0)
            continue;  // the run ended with this sample's tree phase still open (never: the last iteration closes it)
        float b = 0, c = 0;
        AZH_HIP(hipEventElapsedTime(&b, e->events[3 * i], e->events[3 * i + 1]));
        AZH_HIP(hipEventElapsedTime(&c, e->events[3 * i + 1], e->events[(size_t)e->close_of[i]]));
        out->net_ms += b;
        out->select_ms += c;  // the fused tree launch (backup + mark + select), the compaction and the gaps around them
        out->iterations += 1;
    }
    return 0;
}

// Takes the finished-game records off the device: waits for the work enqueued so far, copies the record ring to the host
// and empties it.  azh_engine_drain_json formats what was fetched without touching the device, so a caller may start its
// next run between the two calls and the formatting (a quarter of a millisecond per 150-ply game) and its own file
// writes happen under that run instead of in front of it.  Calling azh_engine_fetch is optional: a drain with nothing
// fetched fetches — but never inside the drain sequence that follows an explicit fetch (up to and including the first
// drain call that hands out no game): there "nothing staged" means "no game finished", and a fetch would wait for the run
// the caller has enqueued in between (round 3's loop did exactly that and ran sequentially without saying so).
static int fetch_records(azh_engine *e)
{
    // Everything on the engine's OWN stream: a fetch of one half-batch must not wait for the other half's run (the
    // legacy null stream would: the engines' streams are blocking streams).
    AZH_HIP(hipStreamSynchronize(e->stream));
    e->unfetched_work = false;
    AZH_HIP(hipMemcpyAsync(e->h_head, e->P.ring_head, 8, hipMemcpyDeviceToHost, e->stream));
    AZH_HIP(hipStreamSynchronize(e->stream));
    u64 head = *e->h_head;
    if (head > e->P.ring_cap_words) {
        // A record or a drop marker did not fit (AZH_STAT_RING_OVERFLOW counts them): its uid will never come, and
        // uid order would wait for it for ever.  From here on the order is given up instead of the games: what is
        // held is handed out, and later games are handed out as they arrive.
        head = e->P.ring_cap_words;
        e->order_broken = true;
    }
    if (head > 0) {
        if ((size_t)head > e->h_stage_words) {
            // (grows to the largest fetch seen, in powers of two from 4 MiB: a round's records, not the ring's capacity)
            size_t want = (size_t)1 << 20;
            while (want < (size_t)head)
                want <<= 1;
            // (the outgrown buffer is kept until the engine is destroyed: freeing pinned memory waits for the whole device,
            // i.e. for the other half-batch's run)
            if (e->h_stage)
                e->h_stage_retired.push_back(e->h_stage);
            e->h_stage = nullptr;
            e->h_stage_words = 0;
            AZH_HIP(hipHostMalloc((void **)&e->h_stage, want * 4));
            e->h_stage_words = want;
        }
        AZH_HIP(hipMemcpyAsync(e->h_stage, e->P.ring, (size_t)head * 4, hipMemcpyDeviceToHost, e->stream));
        AZH_HIP(hipMemsetAsync(e->P.ring, 0, (size_t)head * 4, e->stream));
        AZH_HIP(hipMemsetAsync(e->P.ring_head, 0, 8, e->stream));
        AZH_HIP(hipStreamSynchronize(e->stream));
        e->staged.insert(e->staged.end(), e->h_stage, e->h_stage + (size_t)head);
    }
    return 0;
}

// 1 while work enqueued on the engine is still in flight, 0 when it is idle: a query, never a wait.  (Everything a run
// enqueues is on the engine's one stream, so an idle stream means an idle engine.)
extern "C" int azh_engine_query(azh_engine *e)
{
    if (!e)
        return azh_fail(-1, "azh_engine_query: null engine");
    const hipError_t rc = hipStreamQuery(e->stream);
    if (rc == hipErrorNotReady)
        return 1;
    AZH_HIP(rc);
    return 0;
}

extern "C" int azh_engine_fetch(azh_engine *e)
{
    if (!e)
        return azh_fail(-1, "azh_engine_fetch: null engine");
    const int rc = fetch_records(e);
    if (rc == 0)
        e->fetch_covers_drain = true;
    return rc;
}

extern "C" long long azh_engine_implicit_fetches(const azh_engine *e) { return e ? e->implicit_fetches : -1; }

// Diagnostic: the records an azh_engine_fetch has taken off the device and no drain has formatted yet, as they lie in the
// ring (layout: azh_format_record_json); nothing is consumed.  For tests that read what a game line does not carry: uids,
// visit counts, the plies' "full" words.
extern "C" int azh_engine_staged_records(azh_engine *e, uint32_t *buf, int64_t cap, int64_t *words)
{
    if (!e || !words || (!buf && cap > 0))
        return azh_fail(-1, "azh_engine_staged_records: null argument");
    *words = (int64_t)e->staged.size();
    if (*words > cap)
        return azh_fail(-6, "azh_engine_staged_records: %lld words staged, the buffer has %lld", (long long)*words, (long long)cap);
    if (*words)
        memcpy(buf, e->staged.data(), (size_t)*words * 4);
    return 0;
}

// the fetched records -> lines (in uid order where that is asked for); host work only
static void format_staged(azh_engine *e)
{
    std::vector<uint32_t> host;
    host.swap(e->staged);
    std::vector<std::pair<uint32_t, size_t>> order;  // (uid, offset)
    size_t pos = 0;
    // (two fetches may sit behind each other in the staging buffer: a fetch that ended in a record cut off by a full
    // ring is followed by the next one's first header, which the scan finds again at the next magic word)
    while (pos + REC_HDR_WORDS <= host.size()) {
        if (host[pos] != RING_MAGIC) {
            pos++;
            continue;
        }
        // (a payload word may equal the magic — board halves are arbitrary bit patterns: a header counts only if the
        // record it announces is whole and its ply structure walks to its end exactly)
        if (!azh_record_well_formed(host.data() + pos, host.size() - pos, (uint32_t)e->P.max_plies, nullptr)) {
            pos++;
            continue;
        }
        const RecordView rec{host.data() + pos};
        order.emplace_back(rec.uid(), pos);
        pos += rec.words();
    }
    std::sort(order.begin(), order.end());
    const bool ids = (e->P.flags & AZH_FLAG_TWO_NETS) != 0;
    for (auto &o : order) {
        const RecordView rec{host.data() + o.second};
        std::string line = rec.dropped()        ? std::string()
                           : e->record_blockers ? azh_format_game_json_blockers(rec.w, ids, uid_blockers(e, rec.uid()) & BOARD_MASK)
                                                : azh_format_game_json(rec.w, ids);
        if (rec.loaded() && !ids)
            line.clear();  // a game that began at a loaded position: record drained and formatted like any other
                           // (the measured path does the same work per finished ply), but it is not a whole game.
                           // (The arena hands such games out: a match from given openings — uai_ringmaster.py:185-196 —
                           // loads the position after the opening; the caller knows the opening moves.)
        if (e->emit_by_uid && !e->order_broken)
            e->held[o.first] = std::move(line);
        else if (!line.empty())
            e->pending.push_back(std::move(line));
    }
    // (belt and braces: the longest possible game, 400 plies, outlives a few generations of short ones in the
    // other slots — not sixteen)
    if (e->held.size() > 16 * (size_t)e->P.G + 64)
        e->order_broken = true;
    if (e->emit_by_uid) {
        for (auto it = e->held.begin(); it != e->held.end() && (e->order_broken || it->first == e->next_uid);
             it = e->held.erase(it)) {
            if (!it->second.empty())
                e->pending.push_back(std::move(it->second));
            e->next_uid = it->first + 1;
        }
    }
}

extern "C" int azh_engine_drain_json(azh_engine *e, char *buf, int64_t cap, int64_t *used, int32_t *n_games)
{
    if (!e || !buf || !used || !n_games)
        return azh_fail(-1, "azh_engine_drain_json: null argument");
    *used = 0;
    *n_games = 0;
    if (e->pending_pos >= e->pending.size()) {
        e->pending.clear();
        e->pending_pos = 0;
        if (e->staged.empty() && !e->fetch_covers_drain && e->unfetched_work) {
            // a caller that never fetches: the drain does (and waits for whatever is enqueued) — once per round: the call
            // that ends a drain loop finds no work enqueued since this fetch and returns empty without another one, and
            // a caller that drains with ONE call per round gets a fetch in every round
            e->implicit_fetches++;
            const int rc = fetch_records(e);
            if (rc)
                return rc;
        }
        if (!e->staged.empty())
            format_staged(e);
        if (e->pending.empty())
            e->fetch_covers_drain = false;  // the sequence the explicit fetch covered ends with this (empty) call
    }
    while (e->pending_pos < e->pending.size()) {
        const std::string &line = e->pending[e->pending_pos];
        if (*used + (int64_t)line.size() + 1 > cap)
            break;
        memcpy(buf + *used, line.data(), line.size());
        buf[*used + line.size()] = '\n';
        *used += (int64_t)line.size() + 1;
        *n_games += 1;
        e->pending_pos++;
    }
    if (*n_games == 0 && e->pending_pos < e->pending.size())
        return azh_fail(-6, "azh_engine_drain_json: buffer of %lld bytes cannot hold one game line (%zu bytes)",
                        (long long)cap, e->pending[e->pending_pos].size() + 1);
    return 0;
}
