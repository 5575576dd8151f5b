// Device building blocks for the gfx950 tree kernels: 7x7 bitboards, wave64
// helpers, deterministic f32 math and Philox4x32-10.
//
// Rules follow the reference's C++ rules (file:line under /root/reference):
//   neighbourhood masks  cpp/bitboards.hpp:32-33, cpp/bitboards.cpp:6-39
//   makemove             cpp/makemove.cpp:56-76
//   movegen order        cpp/movegen.cpp:10-79
//   adjudication         cpp/self_play_client.cpp:109-144
// written as shift-and-mask arithmetic derived from the board geometry
// (bit = file + 7*rank), one wavefront cooperating on a position.
//
// Everything here is compiled with -ffp-contract=off: the f32 results of the
// search (priors, scores) are part of the engine's bit-exact contract with the
// CPU oracle, so every operation is a single IEEE basic op in a fixed order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace azh {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned short u16;

constexpr u64 BOARD_MASK = 0x1FFFFFFFFFFFFULL;
constexpr u64 TURN_BIT = 1ULL << 63;
constexpr u32 NONE = 0xFFFFFFFFu;
constexpr int MAX_MOVES = 256;
constexpr int WAVE = 64;

// ---------------------------------------------------------------- bitboards

// Mask of the files a stone may land on after moving df files sideways.
__host__ __device__ constexpr u64 file_mask(int f)
{
    u64 m = 0;
    for (int r = 0; r < 7; r++)
        m |= 1ULL << (f + 7 * r);
    return m;
}

__host__ __device__ constexpr u64 landing_files(int df)
{
    u64 m = 0;
    for (int f = 0; f < 7; f++)
        if (f - df >= 0 && f - df < 7)
            m |= file_mask(f);
    return m;
}

__host__ __device__ constexpr u64 shift_board(u64 bb, int s)
{
    return s >= 0 ? (bb << s) : (bb >> (-s));
}

// Union over the set squares of the ring at Chebyshev distance D.
template <int D>
__host__ __device__ constexpr u64 ring_bb(u64 bb)
{
    u64 out = 0;
    for (int dr = -D; dr <= D; dr++) {
        for (int df = -D; df <= D; df++) {
            int adf = df < 0 ? -df : df, adr = dr < 0 ? -dr : dr;
            if ((adf > adr ? adf : adr) != D)
                continue;
            out |= shift_board(bb, df + 7 * dr) & landing_files(df);
        }
    }
    return out & BOARD_MASK;
}

__host__ __device__ inline u64 single_jump_bb(u64 bb) { return ring_bb<1>(bb); }
__host__ __device__ inline u64 double_jump_bb(u64 bb) { return ring_bb<2>(bb); }

struct Board {
    u64 x;  // x stones (side to move is kept separately)
    u64 o;
    int turn;
};

__host__ __device__ inline Board unpack_board(u64 w0, u64 w1)
{
    Board b;
    b.x = w0 & ~TURN_BIT;
    b.o = w1;
    b.turn = (int)(w0 >> 63);
    return b;
}

__host__ __device__ inline u64 pack_word0(const Board &b) { return b.x | ((u64)b.turn << 63); }

// cpp/makemove.cpp:56-76
__host__ __device__ inline Board make_move(Board b, int from, int to)
{
    u64 own = b.turn ? b.o : b.x;
    u64 opp = b.turn ? b.x : b.o;
    u64 to_bb = 1ULL << to, from_bb = 1ULL << from;
    u64 captured = single_jump_bb(to_bb) & opp;
    own &= ~from_bb;
    own ^= to_bb;
    own ^= captured;
    opp ^= captured;
    Board r;
    r.x = b.turn ? opp : own;
    r.o = b.turn ? own : opp;
    r.turn = b.turn ^ 1;
    return r;
}

// cpp/self_play_client.cpp:220-237, engine.py:75,98-110: flat index into (7,7,17).
__host__ __device__ inline int policy_index(u32 move)
{
    int from = move & 0xFF, to = (move >> 8) & 0xFF;
    int fx = from % 7, fy = 6 - from / 7;
    int tx = to % 7, ty = 6 - to / 7;
    int layer;
    if (from == to) {
        layer = 16;
    } else {
        int dx = tx - fx, dy = ty - fy;
        if (dx == -2) layer = dy + 2;
        else if (dx == 2) layer = 13 + dy;
        else layer = 5 + 2 * (dx + 1) + (dy > 0 ? 1 : 0);
    }
    return 119 * tx + 17 * ty + layer;
}

// ---------------------------------------------------------------- wave64 helpers

__device__ inline int lane_id() { return (int)(threadIdx.x & 63); }

// One wave owns a game; several such waves share a workgroup and take different paths, so nothing inside a game's
// code may wait for the other waves.  What the game's 64 lanes hand each other through LDS or global memory needs only
// this: earlier accesses of the wave are complete (workgroup-scope fence = the waitcnt a __syncthreads() would issue) and
// the compiler keeps later ones behind it.  LDS and the CU's vector L1 serve a wave's accesses in issue order.
// (The same at wavefront scope, without any waitcnt, made nothing faster: profiles/round6_wave_sync_scope_ab.txt.)
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Cross-lane traffic goes through DPP (VALU speed), not ds_bpermute (an LDS round trip per
// hop): the PUCT descent is a dependent chain of ~15 reductions per tree level.
// gfx9 DPP controls: quad_perm 0x00-0xFF, row_shr:n 0x110+n, row_mirror 0x140,
// row_half_mirror 0x141, row_bcast15 0x142, row_bcast31 0x143.
template <int CTRL, int ROW_MASK = 0xF>
__device__ inline int dpp_i32(int old, int src)
{
    return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, 0xF, false);
}

__device__ inline int bcast_last(int v) { return __builtin_amdgcn_readlane(v, 63); }
// value of lane `src`, where src is the same in every lane (a scalar): v_readlane, no LDS hop
__device__ inline int read_lane(int v, int src) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(src)); }

// Inclusive prefix sum over the 64 lanes.
__device__ inline int wave_incl_scan(int v)
{
    v += dpp_i32<0x111>(0, v);          // row_shr:1 (lanes without a source add 0)
    v += dpp_i32<0x112>(0, v);          // row_shr:2
    v += dpp_i32<0x114>(0, v);          // row_shr:4
    v += dpp_i32<0x118>(0, v);          // row_shr:8  -> inclusive within each row of 16
    v += dpp_i32<0x142, 0xA>(0, v);     // row_bcast15 into rows 1 and 3
    v += dpp_i32<0x143, 0xC>(0, v);     // row_bcast31 into rows 2 and 3
    return v;
}

// Reductions leave the result in lane 63 and broadcast it through a scalar register.
__device__ inline int wave_sum_int(int v)
{
    v += dpp_i32<0xB1>(0, v);           // quad_perm [1,0,3,2]
    v += dpp_i32<0x4E>(0, v);           // quad_perm [2,3,0,1]
    v += dpp_i32<0x141>(0, v);          // row_half_mirror
    v += dpp_i32<0x140>(0, v);          // row_mirror
    v += dpp_i32<0x142, 0xA>(0, v);
    v += dpp_i32<0x143, 0xC>(0, v);
    return bcast_last(v);
}

__device__ inline u32 wave_sum_u32(u32 v) { return (u32)wave_sum_int((int)v); }

// f32 sum in the canonical order of the engine/oracle contract: the xor butterfly with
// offsets 1, 2, 4, 8, 16, 32 (pairs, quads, ... halves); lane 63 carries exactly that
// value (every add below pairs the two operands the butterfly pairs).
__device__ inline float wave_sum_f32(float v)
{
    v = v + __int_as_float(dpp_i32<0xB1>(0, __float_as_int(v)));
    v = v + __int_as_float(dpp_i32<0x4E>(0, __float_as_int(v)));
    v = v + __int_as_float(dpp_i32<0x141>(0, __float_as_int(v)));
    v = v + __int_as_float(dpp_i32<0x140>(0, __float_as_int(v)));
    v = v + __int_as_float(dpp_i32<0x142, 0xA>(0, __float_as_int(v)));
    v = v + __int_as_float(dpp_i32<0x143, 0xC>(0, __float_as_int(v)));
    return __int_as_float(bcast_last(__float_as_int(v)));
}

__device__ inline float wave_max_f32(float v)
{
    const auto mx = [](float a, float b) { return b > a ? b : a; };
    v = mx(v, __int_as_float(dpp_i32<0xB1>(__float_as_int(v), __float_as_int(v))));
    v = mx(v, __int_as_float(dpp_i32<0x4E>(__float_as_int(v), __float_as_int(v))));
    v = mx(v, __int_as_float(dpp_i32<0x141>(__float_as_int(v), __float_as_int(v))));
    v = mx(v, __int_as_float(dpp_i32<0x140>(__float_as_int(v), __float_as_int(v))));
    v = mx(v, __int_as_float(dpp_i32<0x142, 0xA>(__float_as_int(v), __float_as_int(v))));
    v = mx(v, __int_as_float(dpp_i32<0x143, 0xC>(__float_as_int(v), __float_as_int(v))));
    return __int_as_float(bcast_last(__float_as_int(v)));
}

__device__ inline u32 wave_max_u32(u32 v)
{
    const auto mx = [](u32 a, u32 b) { return b > a ? b : a; };
    v = mx(v, (u32)dpp_i32<0xB1>((int)v, (int)v));
    v = mx(v, (u32)dpp_i32<0x4E>((int)v, (int)v));
    v = mx(v, (u32)dpp_i32<0x141>((int)v, (int)v));
    v = mx(v, (u32)dpp_i32<0x140>((int)v, (int)v));
    v = mx(v, (u32)dpp_i32<0x142, 0xA>((int)v, (int)v));
    v = mx(v, (u32)dpp_i32<0x143, 0xC>((int)v, (int)v));
    return (u32)bcast_last((int)v);
}

// max of a 64-bit key (used for arg-max as (score bits << 32) | index)
template <int CTRL, int ROW_MASK = 0xF>
__device__ inline u64 dpp_max_u64(u64 v)
{
    const u32 lo = (u32)dpp_i32<CTRL, ROW_MASK>((int)(u32)v, (int)(u32)v);
    const u32 hi = (u32)dpp_i32<CTRL, ROW_MASK>((int)(u32)(v >> 32), (int)(u32)(v >> 32));
    const u64 o = ((u64)hi << 32) | lo;
    return o > v ? o : v;
}

__device__ inline u64 wave_max_u64(u64 v)
{
    v = dpp_max_u64<0xB1>(v);
    v = dpp_max_u64<0x4E>(v);
    v = dpp_max_u64<0x141>(v);
    v = dpp_max_u64<0x140>(v);
    v = dpp_max_u64<0x142, 0xA>(v);
    v = dpp_max_u64<0x143, 0xC>(v);
    const u32 lo = (u32)bcast_last((int)(u32)v), hi = (u32)bcast_last((int)(u32)(v >> 32));
    return ((u64)hi << 32) | lo;
}

// ---------------------------------------------------------------- wave movegen

// Wave-cooperative move generation + adjudication for one position.
// Lane sq (< 49) owns square sq.  Moves are written to `moves` (if non-null) in
// the reference's order: jumps by ascending (from, to), then clones ascending
// (cpp/movegen.cpp:10-79).  Returns the move count (wave-uniform); *result gets
// get_board_result (cpp/self_play_client.cpp:109-144).
__device__ inline int wave_movegen(const Board &b, u64 blockers, u16 *moves, int *result)
{
    int lane = lane_id();
    u64 own = b.turn ? b.o : b.x;
    u64 opp = b.turn ? b.x : b.o;
    u64 empty = BOARD_MASK & ~(b.x | b.o | blockers);
    u64 targets = 0;
    if (lane < 49 && ((own >> lane) & 1ULL))
        targets = double_jump_bb(1ULL << lane) & empty;
    int cnt = __popcll(targets);
    int incl = wave_incl_scan(cnt);
    int jumps = bcast_last(incl);
    u64 clones = single_jump_bb(own) & empty;
    int n_clones = __popcll(clones);
    int total = jumps + n_clones;
    if (moves) {
        int pos = incl - cnt;
        while (targets) {
            int to = __ffsll((long long)targets) - 1;
            moves[pos++] = (u16)(lane | (to << 8));
            targets &= targets - 1;
        }
        if (lane < 49 && ((clones >> lane) & 1ULL)) {
            int idx = jumps + __popcll(clones & ((1ULL << lane) - 1ULL));
            moves[idx] = (u16)(lane | (lane << 8));
        }
    }
    if (result) {
        int p1 = __popcll(b.x), p2 = __popcll(b.o), bl = __popcll(blockers);
        int emp = 49 - p1 - p2 - bl;
        int res = 0;
        if (p1 == 0) res = 2;
        else if (p2 == 0) res = 1;
        else {
            if (total == 0) {
                if (b.turn == 0) p2 += emp;
                else p1 += emp;
            }
            if (p1 + p2 + bl == 49)
                res = p1 < p2 ? 2 : 1;
        }
        *result = res;
        if (p1 == 0 || p2 == 0)
            total = 0;  // the reference adjudicates before generating moves
    }
    (void)opp;
    return total;
}

// ---------------------------------------------------------------- deterministic math

__host__ __device__ inline float u2f(u32 u)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float f; __builtin_memcpy(&f, &u, 4); return f;
#endif
}
__host__ __device__ inline u32 f2u(float f)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(f);
#else
    u32 u; __builtin_memcpy(&u, &f, 4); return u;
#endif
}

// exp(x): 0 below -87, clamped above 88; ~2e-7 relative error.
__host__ __device__ inline float det_expf(float x)
{
    if (!(x >= -87.0f))
        return 0.0f;
    if (x > 88.0f)
        x = 88.0f;
    float t = x * 1.44269504f;
    float n = (t + 12582912.0f) - 12582912.0f;
    float r = __builtin_fmaf(n, -0.693359375f, x);
    r = __builtin_fmaf(n, 2.12194440e-4f, r);
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    float rr = r * r;
    float y = __builtin_fmaf(p, rr, r);
    y = y + 1.0f;
    int ni = (int)n;
    return y * u2f((u32)(ni + 127) << 23);
}

// log(x) for normal x > 0; ~2e-7 relative error.
__host__ __device__ inline float det_logf(float x)
{
    if (!(x >= 1.17549435e-38f))
        return -87.33654475f;
    u32 b = f2u(x);
    int e = (int)((b >> 23) & 255u) - 126;
    float m = u2f((b & 0x007FFFFFu) | 0x3F000000u);
    if (m < 0.70710678f) {
        e -= 1;
        m = (m + m) - 1.0f;
    } else {
        m = m - 1.0f;
    }
    float z = m * m;
    float p = 7.0376836292e-2f;
    p = __builtin_fmaf(p, m, -1.1514610310e-1f);
    p = __builtin_fmaf(p, m, 1.1676998740e-1f);
    p = __builtin_fmaf(p, m, -1.2420140846e-1f);
    p = __builtin_fmaf(p, m, 1.4249322787e-1f);
    p = __builtin_fmaf(p, m, -1.6668057665e-1f);
    p = __builtin_fmaf(p, m, 2.0000714765e-1f);
    p = __builtin_fmaf(p, m, -2.4999993993e-1f);
    p = __builtin_fmaf(p, m, 3.3333331174e-1f);
    float y = (m * z) * p;
    float fe = (float)e;
    y = __builtin_fmaf(fe, -2.12194440e-4f, y);
    y = __builtin_fmaf(z, -0.5f, y);
    float r = m + y;
    return __builtin_fmaf(fe, 0.693359375f, r);
}

struct Philox4 {
    u32 v[4];
};

// Philox4x32-10 (Salmon et al., SC'11).
__host__ __device__ inline Philox4 philox(u32 k0, u32 k1, u32 c0, u32 c1, u32 c2, u32 c3)
{
    for (int round = 0; round < 10; round++) {
        u64 p0 = (u64)0xD2511F53u * c0;
        u64 p1 = (u64)0xCD9E8D57u * c2;
        u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0;
        u32 n1 = (u32)p1;
        u32 n2 = (u32)(p0 >> 32) ^ c3 ^ k1;
        u32 n3 = (u32)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    Philox4 r;
    r.v[0] = c0; r.v[1] = c1; r.v[2] = c2; r.v[3] = c3;
    return r;
}

constexpr u32 STREAM_SAMPLE = 1u;
constexpr u32 STREAM_RANDOM_PLAY = 2u;
constexpr u32 STREAM_RANDOM_PLY = 3u;
constexpr u32 STREAM_PLAYOUT_CAP = 4u;
constexpr u32 STREAM_EVAL_SYMMETRY = 5u;
constexpr u32 STREAM_RESIGN = 6u;

// Playout cap randomization (azh_engine_set_playout_cap): is ply `ply` of game `uid` searched in FULL?  A pure function of
// the engine's Philox key, so a trainer or a test restates it without a device (azh_playout_cap_kind).
__host__ __device__ inline bool playout_cap_full(u32 k0, u32 k1, u32 uid, u32 ply, u32 full_per_65536)
{
    return (philox(k0, k1, uid, ply, STREAM_PLAYOUT_CAP, 0u).v[0] >> 16) < full_per_65536;
}

// Resignation (azh_engine_set_resign): does game `uid` play through to its real end whatever the rule says?  A pure function
// of the engine's Philox key (azh_resign_playthrough).
__host__ __device__ inline bool resign_playthrough(u32 k0, u32 k1, u32 uid, u32 per_65536)
{
    return (philox(k0, k1, uid, 0u, STREAM_RESIGN, 0u).v[0] >> 16) < per_65536;
}
// Forced playouts and policy target pruning (azh_engine_set_forced_playouts; DESIGN.md, "Forced playouts and policy target
// pruning").  Every f32 operation is a single IEEE one in the order written, in whichever translation unit this is compiled
// (the tower's unit contracts by default: the pragmas keep a multiply and an add apart here).
// The visits a root edge of prior `prior` is owed at N root visits, as a real number: sqrt(k P N).
__host__ __device__ inline float forced_bound(float k, float prior, u32 N)
{
#pragma clang fp contract(off)
    return sqrtf((k * prior) * (float)N);
}
// Q + U of an edge with n visits and mean score q (puct_score's operation order; sq = sqrt(1 + N)).
__host__ __device__ inline float forced_score(float prior, float q, u32 n, float sq, float c_puct)
{
#pragma clang fp contract(off)
    const float u = (sq / (1.0f + (float)n)) * (c_puct * prior);
    return u + q;
}
// The per-edge rule of the pruning: the visits written into the ply's record for a root edge other than the most visited one
// (n >= 1 visits, total score W, prior `prior` without its mark) when that one's score is S: up to floor(sqrt(k P N)) visits
// are taken back, one at a time, while the edge with one visit fewer would still score below S; an edge that lost a visit
// and is left with one is left out (0).
__host__ __device__ inline u32 forced_prune_edge(float prior, float W, u32 n, u32 N, float k, float c_puct, float sq, float S)
{
    const float fb = floorf(forced_bound(k, prior, N));
    const u32 f = fb >= (float)n ? n : (u32)fb;  // (no more than n visits can go: the cast stays in range for any k)
    const float q = W / (float)n;
    u32 m = n;
    for (u32 i = 0; i < f; i++) {
        if (m >= 1u && forced_score(prior, q, m - 1u, sq, c_puct) < S)
            m -= 1u;
        else
            break;
    }
    return (m < n && m <= 1u) ? 0u : m;
}
// The written visit counts of a whole root (out[j]; 0: edge j is left out of the record): the most visited edge, ties to
// the lowest index, keeps its visits and sets S; N is the sum of the visits.  Host and device restate the same rule: this
// is the host's (azh_forced_prune), advance_game holds the wave's.
__host__ __device__ inline void forced_prune_root(const float *prior, const float *W, const u32 *n, int M, float k, float c_puct,
                                                  u32 *out)
{
    u32 N = 0;
    int b = 0;
    for (int j = 0; j < M; j++) {
        N += n[j];
        if (n[j] > n[b])
            b = j;
    }
    if (M <= 0)
        return;
    const float sq = sqrtf((float)(1u + N));
    const float S = forced_score(fabsf(prior[b]), n[b] ? W[b] / (float)n[b] : 0.0f, n[b], sq, c_puct);
    for (int j = 0; j < M; j++)
        out[j] = (j == b || n[j] == 0u) ? n[j] : forced_prune_edge(fabsf(prior[j]), W[j], n[j], N, k, c_puct, sq, S);
}

// First-play urgency and the exploration rate of the leaf-parallel search (azh_engine_set_exploration; DESIGN.md, "First-play
// urgency and the exploration rate").  Host (azh_exploration_scores) and device (vl_select_game) share every function but the
// wave's two sums; every f32 operation is a single IEEE one in the order written.
// The mode is on while either knob is: fpu_reduction < 0 is FPU off, c_base == 0 the constant c_puct.
__host__ __device__ inline bool exploration_on(float fpu_reduction, float c_base) { return fpu_reduction >= 0.0f || c_base > 0.0f; }
// c of a node whose children hold N effective visits: AlphaZero's log((1 + N + c_base) / c_base) + c_init, or c_puct.
__host__ __device__ inline float exploration_c(u32 N, float c_puct, float c_base, float c_init)
{
#pragma clang fp contract(off)
    if (!(c_base > 0.0f))
        return c_puct;
    return det_logf(((float)(1u + N) + c_base) / c_base) + c_init;
}
// f, the Q of the node's unvisited children, from the 64-lane sums of W over all children and of P over the visited ones: the
// node's mean score less fpu_reduction * sqrt(visited policy mass), not below 0 (a NaN becomes 0); 0 with FPU off or N == 0.
__host__ __device__ inline float exploration_fpu(float Wsum, float Psum, u32 N, float fpu_reduction)
{
#pragma clang fp contract(off)
    if (!(fpu_reduction >= 0.0f) || N == 0u)
        return 0.0f;
    const float qX = Wsum / (float)N;
    const float f = qX - fpu_reduction * sqrtf(Psum);
    return f > 0.0f ? f : 0.0f;
}
// Q + U of an edge of that node (puct_score's operation order; prior without its mark): with c = c_puct and f = 0 puct_score itself.
__host__ __device__ inline float exploration_score(float prior, float W, u32 n, float sq, float c, float f)
{
#pragma clang fp contract(off)
    const float q = n ? W / (float)n : f;
    const float u = (sq / (1.0f + (float)n)) * (c * prior);
    return u + q;
}

// Search settings per side (azh_engine_set_search_sets; DESIGN.md, "Search settings per side"): the sets of x and of o in game
// `uid` among n sets, as x | o << 8.  With q = uid / 2 and t = q % (n (n - 1) / 2), (a, b), a < b, is the t-th unordered pair
// in lexicographic order; x plays a in an even uid and b in an odd one.  n < 2: both sides play set 0.  The host's
// azh_search_set_pairing and the kernels that write a slot's word (begin_game_key, k_slot_sets) run this one function.
__host__ __device__ inline u32 search_set_pairing(u32 uid, u32 n)
{
    if (n < 2u)
        return 0u;
    u32 t = (uid >> 1) % (n * (n - 1u) / 2u);
    u32 a = 0;
    while (t >= n - 1u - a) {  // row a holds the n - 1 - a pairs (a, a + 1) .. (a, n - 1)
        t -= n - 1u - a;
        a++;
    }
    const u32 b = a + 1u + t;
    return (uid & 1u) ? (b | (a << 8)) : (a | (b << 8));
}

// Temperature of the move played (azh_engine_set_temperature; DESIGN.md, "Temperature of the move and of the root policy").
// The fixed-point weight of a root edge with n visits when the most visited edge has exp(log_nmax) of them: (n / n_max)^(1/T)
// in units of 2^-20, from det_logf / det_expf and one IEEE f32 division, so host and device agree to the bit and the sum of
// the weights is an integer that no summation order changes.  The best edge weighs exactly 2^20 (det_expf(0) is 1).
constexpr u32 TEMPERATURE_ONE = 1048576u;
__host__ __device__ inline u32 temperature_weight(u32 n, float log_nmax, float T)
{
#pragma clang fp contract(off)
    if (n == 0u)
        return 0u;
    const float d = fminf(det_logf((float)n) - log_nmax, 0.0f);
    const float w = det_expf(d / T);
    const u32 q = (u32)(w * 1048576.0f);
    return q < TEMPERATURE_ONE ? q : TEMPERATURE_ONE;
}
// The choice of a whole root on the host (azh_temperature_pick): advance_game holds the wave's.  v0: word 0 of the ply's
// sampling block.  q (or null) receives the weights the choice was made on: T == 1 the raw counts (today's proportional draw),
// T == 0 2^20 at the first maximum and 0 elsewhere, else temperature_weight.  A root without a visit yields edge 0.
__host__ __device__ inline int temperature_pick_root(const u32 *n, int M, float T, u32 v0, u32 *q)
{
    int b = 0;
    for (int j = 1; j < M; j++)
        if (n[j] > n[b])
            b = j;
    const float lmax = M > 0 ? det_logf((float)n[b]) : 0.0f;
    u32 S = 0;
    for (int j = 0; j < M; j++)
        S += T == 1.0f ? n[j] : (T == 0.0f ? (j == b ? TEMPERATURE_ONE : 0u) : temperature_weight(n[j], lmax, T));
    const u32 r = (u32)(((u64)v0 * (u64)S) >> 32);
    int chosen = -1;
    u32 cum = 0;
    for (int j = 0; j < M; j++) {
        const u32 w = T == 1.0f ? n[j] : (T == 0.0f ? (j == b ? TEMPERATURE_ONE : 0u) : temperature_weight(n[j], lmax, T));
        if (q)
            q[j] = w;
        cum += w;
        if (chosen < 0 && cum > r)
            chosen = j;
    }
    return chosen < 0 ? 0 : chosen;
}

// ---------------------------------------------------------------- Gumbel root search with sequential halving
// azh_engine_set_gumbel ("Gumbel root search with sequential halving").  Every f32 operation is a single IEEE one in
// the order written, in whichever translation unit this is compiled (the pragmas keep a multiply and an add apart).  Host and
// device share every function but the wave's reductions: gumbel_root is the host's whole root (azh_gumbel_root), select_game
// and advance_game hold the wave's.
constexpr u32 STREAM_GUMBEL = 7u;
constexpr u32 STREAM_SAMPLE_DRAW = 8u;  // azh_samples_draw_gather: counter (step, sample, attempt, 8)
constexpr int GUMBEL_MAX_ACTIONS = 256;
constexpr int GUMBEL_MAX_TABLE = 1 << 20;  // entries of the considered-visits table: m * visits

// The sequence of considered visit counts for r considered actions and V simulations (the rule of the header), out [V].
inline void gumbel_considered_visits(int r, int V, u16 *out)
{
    if (r <= 1) {
        for (int i = 0; i < V; i++)
            out[i] = (u16)i;
        return;
    }
    int L = 0;
    while ((1 << L) < r)
        L++;
    u16 visits[GUMBEL_MAX_ACTIONS] = {};
    int k = r, len = 0;
    while (len < V) {
        const int d = V / (L * k), extra = d > 1 ? d : 1;
        for (int x = 0; x < extra && len < V; x++) {
            for (int i = 0; i < k && len < V; i++)
                out[len++] = visits[i];
            for (int i = 0; i < k; i++)
                visits[i]++;
        }
        k = k / 2 > 2 ? k / 2 : 2;
    }
}
// g_j: the Gumbel(0, 1) draw of root edge j of ply `ply` of game `uid`
__host__ __device__ inline float gumbel_noise(u32 k0, u32 k1, u32 uid, u32 ply, u32 j)
{
#pragma clang fp contract(off)
    const u32 x = philox(k0, k1, uid, ply, STREAM_GUMBEL, j).v[0];
    const float u = ((float)(x >> 9) + 0.5f) * 0x1p-23f;  // exact, in (0, 1)
    return -det_logf(-det_logf(u));
}
// l_j: the logit of a prior as stored (without its mark)
__host__ __device__ inline float gumbel_logit(float prior) { return prior > 0.0f ? det_logf(prior) : -INFINITY; }
// ks = (c_visit + n_max) * c_scale: what a [0, 1] score is multiplied by
__host__ __device__ inline float gumbel_ks(float c_visit, float c_scale, u32 n_max)
{
#pragma clang fp contract(off)
    return (c_visit + (float)n_max) * c_scale;
}
// s_j = a_j + ks * q_j of a visited edge, a_j of an unvisited one
__host__ __device__ inline float gumbel_score(float a, float W, u32 n, float ks)
{
#pragma clang fp contract(off)
    if (n == 0u)
        return a;
    const float t = ks * (W / (float)n);
    return a + t;
}
// Arg-max key of (score, edge): the greatest key is the greatest score, the lowest index among equal ones; 0 for a NaN, which
// never wins (any other score's key is > 0: the keys of -inf .. +inf ascend from 0x007FFFFF).
__host__ __device__ inline u64 gumbel_key(float s, u32 j)
{
    if (!(s == s))
        return 0ull;
    const u32 b = f2u(s + 0.0f);  // (-0 becomes +0: equal scores have equal bits)
    const u32 o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((u64)o << 32) | (u64)(0xFFFFFFFFu - j);
}
// x_j = l_j + ks * cq_j and the written count of an edge whose x is `x` when the greatest is x_max
__host__ __device__ inline float gumbel_target_logit(float prior, float cq, float ks)
{
#pragma clang fp contract(off)
    const float t = ks * cq;
    return gumbel_logit(prior) + t;
}
__host__ __device__ inline u32 gumbel_count(float x, float x_max)
{
#pragma clang fp contract(off)
    const float w = det_expf(x - x_max) * 65535.0f;
    const u32 c = (u32)w;
    return c < 65535u ? c : 65535u;
}
// v_mix from the root's own value, its visits N and the two 64-lane sums over the visited edges
__host__ __device__ inline float gumbel_v_mix(float v0, u32 N, float sp, float sw)
{
#pragma clang fp contract(off)
    if (!(sp > 0.0f))
        return v0;
    const float t = ((float)N / sp) * sw;
    return (v0 + t) / (1.0f + (float)N);
}
// The 64-lane sum on the host: lane l adds its terms l, l + 64, ... in that order from 0, then the xor butterfly 1 .. 32.
inline float gumbel_lane_sum(const float *v, int M)
{
    float lane[WAVE] = {};
    for (int j = 0; j < M; j++)
        lane[j & 63] = lane[j & 63] + v[j];
    for (int off = 1; off < WAVE; off <<= 1) {
        float nx[WAVE];
        for (int l = 0; l < WAVE; l++)
            nx[l] = lane[l] + lane[l ^ off];
        for (int l = 0; l < WAVE; l++)
            lane[l] = nx[l];
    }
    return lane[0];
}
// The whole root on the host (azh_gumbel_root): the move played and the written counts (counts [M]; 0: left out).  noise [M]:
// g_j (gumbel_noise).  Returns the edge of the move.  A root whose counts would all be 0 (no finite greatest x: every prior 0,
// every visited W a NaN, ks q out of range) writes 65535 at the move played and nothing else, so no record lacks a target.
inline int gumbel_root(const float *prior, const float *W, const u32 *n, int M, float v0, const float *noise, float c_visit,
                       float c_scale, u32 *counts)
{
#pragma clang fp contract(off)
    u32 N = 0, n_max = 0;
    for (int j = 0; j < M; j++) {
        N += n[j];
        n_max = n[j] > n_max ? n[j] : n_max;
    }
    const float ks = gumbel_ks(c_visit, c_scale, n_max);
    u64 key = 0;
    float tp[GUMBEL_MAX_ACTIONS], tw[GUMBEL_MAX_ACTIONS];
    for (int j = 0; j < M; j++) {
        const float p = fabsf(prior[j]);
        if (n[j] == n_max) {
            const u64 kk = gumbel_key(gumbel_score(noise[j] + gumbel_logit(p), W[j], n[j], ks), (u32)j);
            key = kk > key ? kk : key;
        }
        tp[j] = n[j] >= 1u ? p : 0.0f;
        tw[j] = n[j] >= 1u ? p * (W[j] / (float)n[j]) : 0.0f;
    }
    const float v_mix = gumbel_v_mix(v0, N, gumbel_lane_sum(tp, M), gumbel_lane_sum(tw, M));
    float x_max = -INFINITY;
    for (int j = 0; j < M; j++) {
        tp[j] = gumbel_target_logit(fabsf(prior[j]), n[j] >= 1u ? W[j] / (float)n[j] : v_mix, ks);
        if (tp[j] > x_max)
            x_max = tp[j];
    }
    u32 any = 0;
    for (int j = 0; j < M; j++) {
        counts[j] = gumbel_count(tp[j], x_max);
        any |= counts[j];
    }
    const int move = key ? (int)(0xFFFFFFFFu - (u32)key) : 0;
    // no count at all (x_max is -inf, +inf or every x a NaN, so every x - x_max is a NaN): the record is the move alone
    if (any == 0u && M > 0)
        counts[move] = 65535u;
    return move;
}

// ---------------------------------------------------------------- random symmetry per evaluation
// azh_engine_set_random_symmetry ("Random symmetry per evaluation"): every position goes to the evaluator as its
// image under one of the 8 dihedral symmetries of the board, and the logits come back through the same symmetry's move map.
// Symmetry s, as training._symmetry_bits (train.py:11-23): bit 0 mirrors x, bit 1 mirrors y, bit 2 then transposes, on the
// cells (x, y) = (sq % 7, 6 - sq / 7) of policy_index.  Host and device share every function but the wave's ballot form.

// image_s: where a stone on `sq` lies in the image
__host__ __device__ inline int symmetry_cell(int s, int sq)
{
    int x = sq % 7, y = 6 - sq / 7;
    if (s & 1) x = 6 - x;
    if (s & 2) y = 6 - y;
    if (s & 4) { const int t = x; x = y; y = t; }
    return x + 7 * (6 - y);
}
// the cell whose image is `sq` (the inverse: the transposition is undone first)
__host__ __device__ inline int symmetry_source_cell(int s, int sq)
{
    int x = sq % 7, y = 6 - sq / 7;
    if (s & 4) { const int t = x; x = y; y = t; }
    if (s & 1) x = 6 - x;
    if (s & 2) y = 6 - y;
    return x + 7 * (6 - y);
}
// T_s on a bitboard, one lane (or the host) on its own: a loop over the stones, registers only.
__host__ __device__ inline u64 symmetry_board(int s, u64 bb)
{
    u64 out = 0;
    for (u64 r = bb & BOARD_MASK; r; r &= r - 1ULL)
        out |= 1ULL << symmetry_cell(s, __builtin_ctzll(r));
    return out;
}
// T_s on a move: both squares by image_s — a clone stays a clone and policy_index finds the jump's layer from the squares.
// A value that is no board move (a pass) is returned as it is.
__host__ __device__ inline u32 symmetry_move(int s, u32 move)
{
    const u32 from = move & 0xFFu, to = (move >> 8) & 0xFFu;
    if (from >= 49u || to >= 49u)
        return move;
    return (u32)symmetry_cell(s, (int)from) | ((u32)symmetry_cell(s, (int)to) << 8);
}
// T_s on a flat policy index 119 x + 17 y + layer, real move or not: the destination cell by image_s, a jump layer by the image
// of its (dx, dy) = to - from, the clone layer as it is.  For a move m, symmetry_policy_index(s, policy_index(m)) =
// policy_index(symmetry_move(s, m)); over all 833 indices it is the permutation that brings the logits of the image back:
// logits_of_the_position[i] = logits_of_the_image[symmetry_policy_index(s, i)].
__host__ __device__ inline int symmetry_policy_index(int s, int index)
{
    // (the three bits enter as 0 / 1 factors, not as conditions: nothing of s has to be kept as a lane mask around the caller's loop)
    const int fx = s & 1, fy = (s >> 1) & 1, tr = (s >> 2) & 1;
    const int x0 = index / 119, rest = index - 119 * x0, y0 = rest / 17;
    int layer = rest - 17 * y0;
    if (layer != 16) {
        int dx, dy;
        if (layer < 5) { dx = -2; dy = layer - 2; }
        else if (layer >= 11) { dx = 2; dy = layer - 13; }
        else { dx = (layer - 5) / 2 - 1; dy = ((layer - 5) & 1) ? 2 : -2; }
        dx *= 1 - 2 * fx;
        dy *= 1 - 2 * fy;
        const int ex = dx + tr * (dy - dx), ey = dy + tr * (dx - dy);
        if (ex == -2) layer = ey + 2;
        else if (ex == 2) layer = 13 + ey;
        else layer = 5 + 2 * (ex + 1) + (ey > 0 ? 1 : 0);
    }
    const int x1 = x0 + fx * (6 - 2 * x0), y1 = y0 + fy * (6 - 2 * y0);
    const int x = x1 + tr * (y1 - x1), y = y1 + tr * (x1 - y1);
    return 119 * x + 17 * y + layer;
}
// The game's key word (one per game: written where the game begins) and the symmetry of a position of that game: a hash of the
// key and the UNTRANSFORMED leaf board (mover, opponent), u32 arithmetic — a pure function a host restates (azh_eval_symmetry).
__host__ __device__ inline u32 eval_symmetry_key(u32 k0, u32 k1, u32 uid)
{
    return philox(k0, k1, uid, 0u, STREAM_EVAL_SYMMETRY, 0u).v[0];
}
__host__ __device__ inline u32 eval_symmetry_mix(u32 a, u32 w)
{
    a = (a ^ w) * 0x9E3779B1u;
    return a ^ (a >> 15);
}
__host__ __device__ inline int eval_symmetry_of(u32 key, u64 mover, u64 opponent)
{
    u32 a = eval_symmetry_mix(key, (u32)mover);
    a = eval_symmetry_mix(a, (u32)(mover >> 32));
    a = eval_symmetry_mix(a, (u32)opponent);
    a = eval_symmetry_mix(a, (u32)(opponent >> 32));
    a = a * 0x85EBCA77u;
    a ^= a >> 13;
    return (int)(a >> 29);
}
// T_s on the two bitboards of a position the whole wave holds (s, mover, opponent wave-uniform): lane i < 49 tests the source
// cell of image cell i and a ballot assembles each word.  No LDS, no memory.
__device__ inline void wave_symmetry_boards(int s, u64 &mover, u64 &opponent)
{
    const int lane = lane_id();
    const int src = symmetry_source_cell(s, lane < 49 ? lane : 0);
    const u64 m = __ballot(lane < 49 && ((mover >> src) & 1ULL) != 0ULL);
    const u64 o = __ballot(lane < 49 && ((opponent >> src) & 1ULL) != 0ULL);
    mover = m;
    opponent = o;
}

constexpr u32 STREAM_GAMMA = 0x10000u;

// Gamma(alpha, 1), alpha < 1: Marsaglia-Tsang on alpha + 1 with a polar normal,
// boosted by U^(1/alpha); one Philox block per attempt.  Stands in for
// std::gamma_distribution at cpp/self_play_client.cpp:252-255.
__host__ __device__ inline float det_gamma(float alpha, u32 k0, u32 k1, u32 uid, u32 ply, u32 edge)
{
    float d = (alpha + 1.0f) - 0.333333343f;
    float c = 1.0f / sqrtf(9.0f * d);
    for (u32 attempt = 0; attempt < 64u; attempt++) {
        Philox4 r = philox(k0, k1, uid, ply, STREAM_GAMMA + edge, attempt);
        float u1 = (float)(r.v[0] >> 8) * 1.1920929e-7f - 1.0f;
        float u2 = (float)(r.v[1] >> 8) * 1.1920929e-7f - 1.0f;
        float s = u1 * u1 + u2 * u2;
        if (!(s < 1.0f) || s == 0.0f)
            continue;
        float x = u1 * sqrtf((-2.0f * det_logf(s)) / s);
        float v = 1.0f + c * x;
        if (!(v > 0.0f))
            continue;
        v = (v * v) * v;
        float U = (float)((r.v[2] >> 8) + 1u) * 5.9604645e-8f;
        float lhs = det_logf(U);
        float rhs = ((0.5f * x) * x + d) - d * v + d * det_logf(v);
        if (!(lhs < rhs))
            continue;
        float U2 = (float)((r.v[3] >> 8) + 1u) * 5.9604645e-8f;
        float boost = det_expf(det_logf(U2) / alpha);
        return (d * v) * boost;
    }
    return 0.0f;
}

}  // namespace azh
