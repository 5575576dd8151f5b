// The depth-limited material alpha-beta search of one position by one wave ("Alpha-beta search"): what
// azh_alphabeta_search, azh_alphabeta_play (alphabeta.hip) and azh_samples_prove (samples.hip) run.
//
// The plies above the last one run wave-uniformly on an explicit stack in LDS (no device recursion); the last ply, which is
// nearly all of the work, is wave-parallel: every lane makes its own moves of the node's LDS move list, adjudicates and scores
// the children with bit tests, and one wave reduction takes the maximum.
#pragma once

#include "azh_device.h"
#include "azh_host.h"

namespace azh {

constexpr int AB_WIN = 1000;
constexpr int AB_INF = 1 << 20;       // beyond every value: |value| <= AB_WIN + AZH_ALPHABETA_MAX_DEPTH
constexpr int AB_BIAS = 1 << 16;      // makes a score a positive key
constexpr int AB_MAX_DEPTH = AZH_ALPHABETA_MAX_DEPTH;
constexpr int AB_WAVES = 4;           // roots (waves) per workgroup

// 0, or why (depth, node_budget) is refused
inline const char *limits_refusal(int depth, uint64_t node_budget)
{
    if (depth < 1 || depth > AZH_ALPHABETA_MAX_DEPTH)
        return "depth must be 1 .. AZH_ALPHABETA_MAX_DEPTH";
    if (node_budget == 0 && depth > AZH_ALPHABETA_UNBOUNDED_DEPTH)
        return "node_budget 0 (no limit) is accepted up to depth AZH_ALPHABETA_UNBOUNDED_DEPTH only";
    if (node_budget != 0 && node_budget < AZH_MAX_MOVES)
        return "node_budget must be 0 or at least AZH_MAX_MOVES";
    return nullptr;
}

// Adjudication of a position by bit tests, no move list: wave_movegen's *result (cpp/self_play_client.cpp:109-144).
__host__ __device__ inline int ab_result(const Board &b, u64 blockers)
{
    int p1 = __builtin_popcountll(b.x), p2 = __builtin_popcountll(b.o);
    const int bl = __builtin_popcountll(blockers);
    if (p1 == 0) return 2;
    if (p2 == 0) return 1;
    const u64 own = b.turn ? b.o : b.x;
    const u64 empty = BOARD_MASK & ~(b.x | b.o | blockers);
    if (((single_jump_bb(own) | double_jump_bb(own)) & empty) == 0ULL) {  // the mover is stuck: the empties go to the opponent
        if (b.turn == 0) p2 += 49 - p1 - p2 - bl;
        else p1 += 49 - p1 - p2 - bl;
    }
    if (p1 + p2 + bl == 49)
        return p1 < p2 ? 2 : 1;
    return 0;
}

// Rule 1: the value of a finished position with result `res`, seen from its side to move, `rem` plies of depth left.
__host__ __device__ inline int ab_terminal(int res, int turn, int rem)
{
    return res == turn + 1 ? AB_WIN + rem : -(AB_WIN + rem);
}

// value(p, 0) of any position
__host__ __device__ inline int ab_leaf_value(const Board &b, u64 blockers)
{
    const int res = ab_result(b, blockers);
    if (res != 0)
        return ab_terminal(res, b.turn, 0);
    const int d = __builtin_popcountll(b.x) - __builtin_popcountll(b.o);
    return b.turn ? -d : d;
}

// The stack of one wave.  Everything in it is wave-uniform: every lane writes and reads the same words.
struct AbPly {
    u64 x, o;
    int cnt, cur, alpha, beta, best, pad;
};
struct AbStack {
    u16 moves[AB_MAX_DEPTH][MAX_MOVES];
    AbPly ply[AB_MAX_DEPTH];
};

__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// A node with one ply of depth left: the maximum over its M listed moves of -value(child, 0), as the key
// (score + AB_BIAS) << 32 | ~index, so that the greatest key is the greatest score and the first move among equal ones.
__device__ inline u64 ab_last_ply(const Board &b, u64 blockers, const u16 *moves, int M)
{
    u64 key = 0;
    for (int i = lane_id(); i < M; i += WAVE) {
        const u32 mv = moves[i];
        const Board c = make_move(b, (int)(mv & 0xFF), (int)(mv >> 8));
        const int s = -ab_leaf_value(c, blockers);
        const u64 k = ((u64)(u32)(s + AB_BIAS) << 32) | (u64)(~(u32)i);
        key = k > key ? k : key;
    }
    return wave_max_u64(key);
}

struct AbAnswer {
    u32 move;
    int value, depth_done;
    u64 nodes;
};

// The whole search of one root by one wave (all 64 lanes enter and leave together).  s->moves[0] holds the root's M moves
// (wave_movegen, synced) and the root is not finished.
__device__ inline AbAnswer ab_search_root(const Board &root, u64 blockers, AbStack *s, int M, int depth, u64 budget)
{
    AbAnswer a;
    a.move = 0xFFFFu;
    a.value = 0;
    a.depth_done = 0;
    a.nodes = 0;
    for (int d = 1; d <= depth; d++) {
        u32 best_index = 0;
        int best_value;
        bool abandoned = false;
        if (d == 1) {
            const u64 key = ab_last_ply(root, blockers, s->moves[0], M);
            a.nodes += (u64)M;
            best_value = (int)(u32)(key >> 32) - AB_BIAS;
            best_index = ~(u32)key;
        } else {
            int k = 0;
            s->ply[0].x = root.x;
            s->ply[0].o = root.o;
            s->ply[0].cnt = M;
            s->ply[0].cur = 0;
            s->ply[0].alpha = -AB_INF;
            s->ply[0].beta = AB_INF;
            s->ply[0].best = -AB_INF;
            for (;;) {
                AbPly *p = &s->ply[k];
                const int cur = uni(p->cur);
                int ret;
                if (cur >= uni(p->cnt) || uni(p->alpha) >= uni(p->beta)) {
                    // every move searched, or a cut: the node's value (a bound after a cut) goes up
                    if (k == 0)
                        break;
                    ret = -uni(p->best);
                    k--;
                } else {
                    const u32 mv = (u32)uni((int)s->moves[k][cur]);
                    p->cur = cur + 1;
                    Board b;
                    b.x = p->x;
                    b.o = p->o;
                    b.turn = (root.turn + k) & 1;
                    const Board c = make_move(b, (int)(mv & 0xFF), (int)(mv >> 8));
                    a.nodes++;
                    if (budget && a.nodes > budget) {
                        abandoned = true;
                        break;
                    }
                    const int rem = d - k - 1;  // >= 1: the nodes of this loop have two plies or more left
                    int res;
                    wave_sync();
                    const int Mc = uni(wave_movegen(c, blockers, s->moves[k + 1], &res));
                    res = uni(res);
                    wave_sync();
                    if (res != 0) {
                        ret = -ab_terminal(res, c.turn, rem);
                    } else if (rem == 1) {
                        const u64 key = ab_last_ply(c, blockers, s->moves[k + 1], Mc);
                        a.nodes += (u64)Mc;
                        ret = -((int)(u32)(key >> 32) - AB_BIAS);
                    } else {
                        AbPly *q = &s->ply[k + 1];
                        q->x = c.x;
                        q->o = c.o;
                        q->cnt = Mc;
                        q->cur = 0;
                        q->alpha = -uni(p->beta);
                        q->beta = -uni(p->alpha);
                        q->best = -AB_INF;
                        k++;
                        continue;
                    }
                }
                // `ret` is the score of the move before the cursor of ply k
                AbPly *u = &s->ply[k];
                if (ret > uni(u->best)) {  // strictly: the first move of the greatest score stays
                    u->best = ret;
                    if (k == 0)
                        best_index = (u32)(uni(u->cur) - 1);
                }
                if (ret > uni(u->alpha))
                    u->alpha = ret;
            }
            best_value = uni(s->ply[0].best);
            if (budget && a.nodes > budget)
                abandoned = true;
        }
        if (abandoned)
            break;
        a.move = (u32)uni((int)s->moves[0][best_index < (u32)M ? best_index : 0u]);
        a.value = best_value;
        a.depth_done = d;
    }
    return a;
}

// What azh_alphabeta_search reports for one position, finished ones included (rule 1 with the whole depth, no move, no nodes):
// the root's moves go to s->moves[0], then ab_search_root.  One wave, all 64 lanes.
__device__ inline AbAnswer ab_search_position(const Board &root, u64 blockers, AbStack *s, int depth, u64 budget)
{
    int res;
    const int M = uni(wave_movegen(root, blockers, s->moves[0], &res));
    res = uni(res);
    wave_sync();
    if (res != 0) {
        AbAnswer a;
        a.move = 0xFFFFu;
        a.value = ab_terminal(res, root.turn, depth);
        a.depth_done = depth;
        a.nodes = 0;
        return a;
    }
    return ab_search_root(root, blockers, s, M, depth, budget);
}

}  // namespace azh
