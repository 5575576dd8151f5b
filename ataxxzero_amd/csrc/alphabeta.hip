// Depth-limited material alpha-beta search on the device: a net-free teacher and a fixed strength anchor
// ("Alpha-beta search").  azh_alphabeta_search, azh_alphabeta_play and the host's plain negamax
// azh_alphabeta_host, which states the same definition without pruning and without a device.
//
// One wave per root position; the search itself is alphabeta_search.h, which the sample store's proof pass shares.
#include <vector>

#include "alphabeta_search.h"
#include "azh_device.h"
#include "azh_host.h"

namespace azh {

constexpr u32 STREAM_TEACHER = 9u;    // azh_alphabeta_play: counter (game, ply, 9, 0)

__global__ __launch_bounds__(AB_WAVES *WAVE) void k_alphabeta(const ulonglong2 *boards, int n, u64 blockers,
                                                              const u64 *blockers_per_board, int depth, u64 budget,
                                                              u16 *moves_out, int *values_out, int *depth_done_out,
                                                              unsigned long long *nodes_out)
{
    __shared__ AbStack stacks[AB_WAVES];
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    const int r = uni((int)blockIdx.x * AB_WAVES + wave);
    if (r >= n)
        return;  // the whole wave: nothing below waits for another wave
    AbStack *s = &stacks[wave];
    const ulonglong2 w = boards[r];
    const Board root = unpack_board(w.x, w.y);
    const u64 bl = blockers_per_board ? blockers_per_board[r] : blockers;
    const AbAnswer a = ab_search_position(root, bl, s, depth, budget);
    if (lane == 0) {
        moves_out[r] = (u16)a.move;
        values_out[r] = a.value;
        depth_done_out[r] = a.depth_done;
        nodes_out[r] = a.nodes;
    }
}

// One ply of every live teacher game: search, record, play.  final != 0: only adjudicate the games still open.
__global__ __launch_bounds__(AB_WAVES *WAVE) void k_alphabeta_play_ply(ulonglong2 *boards, const u64 *blockers_per_game, int n,
                                                                       int depth, u64 budget, u32 k0, u32 k1, int ply,
                                                                       int max_plies, u32 threshold, int final, int *plies,
                                                                       int *results, ulonglong2 *trace_boards,
                                                                       u16 *training_moves, u16 *played_moves, int *live)
{
    __shared__ AbStack stacks[AB_WAVES];
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    const int g = uni((int)blockIdx.x * AB_WAVES + wave);
    if (g >= n)
        return;
    if (uni(results[g]) != 0)
        return;
    AbStack *s = &stacks[wave];
    const ulonglong2 w = boards[g];
    const Board root = unpack_board(w.x, w.y);
    const u64 bl = blockers_per_game[g];
    int res;
    const int M = uni(wave_movegen(root, bl, s->moves[0], &res));
    res = uni(res);
    wave_sync();
    if (res != 0 || final) {
        if (lane == 0)
            results[g] = res;
        return;
    }
    const AbAnswer a = ab_search_root(root, bl, s, M, depth, budget);
    u32 played = a.move;
    const Philox4 rnd = philox(k0, k1, (u32)g, (u32)ply, STREAM_TEACHER, 0u);
    if (rnd.v[0] < threshold) {
        const u32 j = (u32)(((u64)rnd.v[1] * (u64)(u32)M) >> 32);
        played = (u32)uni((int)s->moves[0][j < (u32)M ? j : 0u]);
    }
    const Board nb = make_move(root, (int)(played & 0xFF), (int)(played >> 8));
    if (lane == 0) {
        const size_t cell = (size_t)g * (size_t)max_plies + (size_t)ply;
        trace_boards[cell] = make_ulonglong2(root.x, root.o);
        training_moves[cell] = (u16)a.move;
        played_moves[cell] = (u16)played;
        boards[g] = make_ulonglong2(pack_word0(nb), nb.o);
        plies[g] = ply + 1;
        atomicAdd(live, 1);
    }
}

// ---------------------------------------------------------------- the host's plain negamax

struct HostSearch {
    u64 blockers, budget, nodes;
    bool abandoned;
};

static int host_movegen(const Board &b, u64 blockers, u16 *moves)
{
    const u64 own = b.turn ? b.o : b.x;
    const u64 empty = BOARD_MASK & ~(b.x | b.o | blockers);
    int n = 0;
    for (u64 c = own; c; c &= c - 1) {
        const int from = __builtin_ctzll(c);
        for (u64 t = double_jump_bb(1ULL << from) & empty; t; t &= t - 1)
            moves[n++] = (u16)(from | (__builtin_ctzll(t) << 8));
    }
    for (u64 cl = single_jump_bb(own) & empty; cl; cl &= cl - 1) {
        const int to = __builtin_ctzll(cl);
        moves[n++] = (u16)(to | (to << 8));
    }
    return n;
}

// value(p, d) as the definition states it; the caller has counted p.
static int host_value(HostSearch &h, const Board &b, int d)
{
    const int res = ab_result(b, h.blockers);
    if (res != 0)
        return ab_terminal(res, b.turn, d);
    if (d == 0)
        return ab_leaf_value(b, h.blockers);
    u16 moves[MAX_MOVES];
    const int M = host_movegen(b, h.blockers, moves);
    int best = -AB_INF;
    for (int i = 0; i < M; i++) {
        h.nodes++;
        if (h.budget && h.nodes > h.budget) {
            h.abandoned = true;
            return 0;
        }
        const int v = -host_value(h, make_move(b, moves[i] & 0xFF, moves[i] >> 8), d - 1);
        if (h.abandoned)
            return 0;
        if (v > best)
            best = v;
    }
    return best;
}

}  // namespace azh

using namespace azh;

namespace {
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { AZH_HIP(hipMalloc(&p, bytes ? bytes : 1)); return 0; }
    template <typename T> T *as() { return (T *)p; }
};

bool position_ok(uint64_t x, uint64_t o, uint64_t blockers)
{
    return !((x | o | blockers) & ~BOARD_MASK) && !(x & o) && !((x | o) & blockers);
}
}  // namespace

extern "C" int azh_alphabeta_search(int n, const uint64_t *boards, uint64_t blockers, const uint64_t *blockers_per_board,
                                    int depth, uint64_t node_budget, uint16_t *moves_out, int32_t *values_out,
                                    int32_t *depth_done_out, uint64_t *nodes_out)
{
    if (n < 0 || !boards)
        return azh_fail(-1, "azh_alphabeta_search: bad argument");
    if (const char *why = limits_refusal(depth, node_budget))
        return azh_fail(-2, "azh_alphabeta_search: %s", why);
    for (int i = 0; i < n; i++)
        if (!position_ok(boards[2 * i] & ~TURN_BIT, boards[2 * i + 1], blockers_per_board ? blockers_per_board[i] : blockers))
            return azh_fail(-2, "azh_alphabeta_search: board %d: stones or walls overlap or lie beyond the 49 cells", i);
    if (azh_require_device())
        return -3;
    if (n == 0)
        return 0;
    DevBuf db, dw, dm, dv, dd, dn;
    if (db.alloc((size_t)n * 16) || dm.alloc((size_t)n * 2) || dv.alloc((size_t)n * 4) || dd.alloc((size_t)n * 4) ||
        dn.alloc((size_t)n * 8))
        return -4;
    if (blockers_per_board && dw.alloc((size_t)n * 8))
        return -4;
    AZH_HIP(hipMemcpy(db.p, boards, (size_t)n * 16, hipMemcpyHostToDevice));
    if (blockers_per_board)
        AZH_HIP(hipMemcpy(dw.p, blockers_per_board, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_alphabeta, dim3((n + AB_WAVES - 1) / AB_WAVES), dim3(AB_WAVES * WAVE), 0, 0, db.as<ulonglong2>(), n,
                       blockers, blockers_per_board ? dw.as<u64>() : (const u64 *)nullptr, depth, (u64)node_budget,
                       dm.as<u16>(), dv.as<int>(), dd.as<int>(), dn.as<unsigned long long>());
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipDeviceSynchronize());
    if (moves_out) AZH_HIP(hipMemcpy(moves_out, dm.p, (size_t)n * 2, hipMemcpyDeviceToHost));
    if (values_out) AZH_HIP(hipMemcpy(values_out, dv.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (depth_done_out) AZH_HIP(hipMemcpy(depth_done_out, dd.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (nodes_out) AZH_HIP(hipMemcpy(nodes_out, dn.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int azh_alphabeta_host(uint64_t x, uint64_t o, uint64_t blockers, int turn, int depth, uint64_t node_budget,
                                  uint16_t *move_out, int32_t *value_out, int32_t *depth_done_out, uint64_t *nodes_out)
{
    if (turn != 0 && turn != 1)
        return azh_fail(-1, "azh_alphabeta_host: bad argument");
    if (const char *why = limits_refusal(depth, node_budget))
        return azh_fail(-2, "azh_alphabeta_host: %s", why);
    if (!position_ok(x, o, blockers))
        return azh_fail(-2, "azh_alphabeta_host: stones or walls overlap or lie beyond the 49 cells");
    Board root;
    root.x = x;
    root.o = o;
    root.turn = turn;
    HostSearch h;
    h.blockers = blockers;
    h.budget = node_budget;
    h.nodes = 0;
    h.abandoned = false;
    uint16_t move = 0xFFFF;
    int value = 0, done = 0;
    const int res = ab_result(root, blockers);
    if (res != 0) {
        value = ab_terminal(res, turn, depth);
        done = depth;
    } else {
        u16 moves[MAX_MOVES];
        const int M = host_movegen(root, blockers, moves);
        for (int d = 1; d <= depth && !h.abandoned; d++) {
            int best = -AB_INF, best_index = 0;
            for (int i = 0; i < M; i++) {
                h.nodes++;
                if (h.budget && h.nodes > h.budget) {
                    h.abandoned = true;
                    break;
                }
                const int v = -host_value(h, make_move(root, moves[i] & 0xFF, moves[i] >> 8), d - 1);
                if (h.abandoned)
                    break;
                if (v > best) {
                    best = v;
                    best_index = i;
                }
            }
            if (h.abandoned)
                break;
            move = moves[best_index];
            value = best;
            done = d;
        }
    }
    if (move_out) *move_out = move;
    if (value_out) *value_out = value;
    if (depth_done_out) *depth_done_out = done;
    if (nodes_out) *nodes_out = h.nodes;
    return 0;
}

extern "C" int azh_alphabeta_play(int n_games, uint64_t seed, uint64_t x, uint64_t o, uint64_t blockers, int turn,
                                  const uint64_t *starts, const uint64_t *blockers_per_game, int depth, uint64_t node_budget,
                                  const uint32_t *random_per_2_32, int n_schedule, int max_plies, int32_t *plies,
                                  int32_t *results, uint64_t *boards_out, uint16_t *training_moves_out,
                                  uint16_t *played_moves_out)
{
    if (n_games < 0 || max_plies <= 0 || n_schedule < 0 || (n_schedule > 0 && !random_per_2_32) || (!starts && turn != 0 && turn != 1))
        return azh_fail(-1, "azh_alphabeta_play: bad argument");
    if (const char *why = limits_refusal(depth, node_budget))
        return azh_fail(-2, "azh_alphabeta_play: %s", why);
    std::vector<uint64_t> hb((size_t)n_games * 2), hw((size_t)n_games);
    for (int g = 0; g < n_games; g++) {
        hb[2 * g] = starts ? starts[2 * g] : (x | ((uint64_t)turn << 63));
        hb[2 * g + 1] = starts ? starts[2 * g + 1] : o;
        hw[g] = blockers_per_game ? blockers_per_game[g] : blockers;
        if (!position_ok(hb[2 * g] & ~TURN_BIT, hb[2 * g + 1], hw[g]))
            return azh_fail(-2, "azh_alphabeta_play: game %d: stones or walls overlap or lie beyond the 49 cells", g);
    }
    if (azh_require_device())
        return -3;
    if (n_games == 0)
        return 0;
    const size_t cells = (size_t)n_games * (size_t)max_plies;
    DevBuf db, dw, dp, dr, dt, dtm, dpm, dl;
    if (db.alloc((size_t)n_games * 16) || dw.alloc((size_t)n_games * 8) || dp.alloc((size_t)n_games * 4) ||
        dr.alloc((size_t)n_games * 4) || dt.alloc(cells * 16) || dtm.alloc(cells * 2) || dpm.alloc(cells * 2) || dl.alloc(4))
        return -4;
    AZH_HIP(hipMemcpy(db.p, hb.data(), (size_t)n_games * 16, hipMemcpyHostToDevice));
    AZH_HIP(hipMemcpy(dw.p, hw.data(), (size_t)n_games * 8, hipMemcpyHostToDevice));
    AZH_HIP(hipMemset(dp.p, 0, (size_t)n_games * 4));
    AZH_HIP(hipMemset(dr.p, 0, (size_t)n_games * 4));
    AZH_HIP(hipMemset(dt.p, 0, cells * 16));
    AZH_HIP(hipMemset(dtm.p, 0, cells * 2));
    AZH_HIP(hipMemset(dpm.p, 0, cells * 2));
    const dim3 grid((n_games + AB_WAVES - 1) / AB_WAVES), block(AB_WAVES * WAVE);
    // one launch per ply, so that no launch outlives one search per game; a last one adjudicates the games cut at max_plies
    for (int ply = 0; ply <= max_plies; ply++) {
        const int final = ply == max_plies;
        AZH_HIP(hipMemset(dl.p, 0, 4));
        hipLaunchKernelGGL(k_alphabeta_play_ply, grid, block, 0, 0, db.as<ulonglong2>(), dw.as<u64>(), n_games, depth,
                           (u64)node_budget, (u32)seed, (u32)(seed >> 32), ply, max_plies,
                           ply < n_schedule ? random_per_2_32[ply] : 0u, final, dp.as<int>(), dr.as<int>(), dt.as<ulonglong2>(),
                           dtm.as<u16>(), dpm.as<u16>(), dl.as<int>());
        AZH_HIP(hipGetLastError());
        int live = 0;
        AZH_HIP(hipMemcpy(&live, dl.p, 4, hipMemcpyDeviceToHost));
        if (live == 0 && !final)
            break;  // every game has its result
    }
    if (plies) AZH_HIP(hipMemcpy(plies, dp.p, (size_t)n_games * 4, hipMemcpyDeviceToHost));
    if (results) AZH_HIP(hipMemcpy(results, dr.p, (size_t)n_games * 4, hipMemcpyDeviceToHost));
    if (boards_out) AZH_HIP(hipMemcpy(boards_out, dt.p, cells * 16, hipMemcpyDeviceToHost));
    if (training_moves_out) AZH_HIP(hipMemcpy(training_moves_out, dtm.p, cells * 2, hipMemcpyDeviceToHost));
    if (played_moves_out) AZH_HIP(hipMemcpy(played_moves_out, dpm.p, cells * 2, hipMemcpyDeviceToHost));
    return 0;
}
