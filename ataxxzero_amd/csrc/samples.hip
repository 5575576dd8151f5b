// Device-resident training samples (azh_samples_*; include/ataxxzero_hip.h, DESIGN.md "Device-resident samples"): finished
// games kept in HBM as bitboards and sparse policy targets, and one kernel that writes a minibatch — features [n][7][7][4],
// policy [n][7][7][17], value [n][1], f32 — straight into the trainer's tensors, bit for bit what
// training.make_minibatch_reference builds on the host (train.py:43-77 of the reference).  A game may carry a wall mask
// (DESIGN.md "Walls through the loop"): plane 3 of its samples shows it, and the surprise pass generates moves around it.
//
// Compiled with -ffp-contract=off: the value target's blend is three IEEE double operations in Python's order, and a
// lambda-return's step four (include/ataxxzero_hip.h, "lambda-returns as value targets").
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "alphabeta_search.h"
#include "azh_device.h"
#include "azh_host.h"

using namespace azh;

namespace {

constexpr int FEATURES = 196, POLICY = 833, SAMPLE_FLOATS = FEATURES + POLICY + 1;
constexpr int MAX_ATTEMPTS = 64;  // one per lane of the wave that draws the sample
constexpr u32 GAME_HAS_FULL = 1u << 8, GAME_HAS_VALUES = 1u << 9;
constexpr u32 PLY_ODD = 0x80u;  // in the device's targets_flags only: o is the mover (the surprise kernel sees no game)
constexpr u32 WEIGHT_ONE = 65536u;
constexpr u64 RETURN_ABSENT = ~0ULL;  // the bits of a ply's lambda-return that no pass has covered (a NaN no arithmetic yields)
constexpr int SURPRISE_CHUNK = 16384;
// auxiliary targets (include/ataxxzero_hip.h, "Auxiliary targets"): the aux kernels' LDS behind the sample's padded floats
constexpr int SAMPLE_LDS = (SAMPLE_FLOATS + 3) / 4 * 4;
constexpr int AUX_OWNERSHIP = SAMPLE_LDS, AUX_SCORE = AUX_OWNERSHIP + 49, AUX_WEIGHT = AUX_SCORE + 1, AUX_REPLY = AUX_WEIGHT + 2;
constexpr int AUX_LDS = (AUX_REPLY + POLICY + 3) / 4 * 4;

struct Ply {  // 32 bytes
    u64 x, o;      // bit = file + 7 * rank, the ring record's layout
    double value;  // the search's value for the mover in [-1, 1] (games with "values")
    u32 first_target;
    u32 targets_flags;  // targets << 8 | AZH_SAMPLES_PLY_*
};

struct View {  // what the kernels read
    const uint4 *games;  // {first ply, plies, result | GAME_HAS_*, random_ply + 1}
    const Ply *plies;
    const u16 *candidates;  // [first ply + k]: the k-th ply of the game a sample may be drawn from
    const u32 *candidate_count;
    const u16 *target_index;
    const float *target_weight;
    const u32 *cum;  // null: uniform ply draws; else [first ply + k]: the running sum of the game's candidate weights
    const u64 *blockers;  // null: no stored game has walls; else [game]: its wall mask, bit = file + 7 * rank
    const int16_t *proofs;  // null: azh_samples_prove was never called; else [ply]: the proven value of its mover, 0: none
    const double *returns;  // null: no lambda-returns (azh_samples_value_returns); else [ply]: G_p, RETURN_ABSENT: not covered
};

__host__ __device__ inline u64 f64_bits(double v)
{
    u64 bits;
    memcpy(&bits, &v, sizeof(bits));
    return bits;
}

struct NoAux {};  // the kernels without auxiliary targets: emit_sample is what it was
struct Aux {      // the four further outputs, and where the owners come from
    const u64 *owners;  // null: no stored game has owners; else [game][2]: the cells x and o own at the game's end
    float *ownership, *score, *reply, *weight;
};

// One wave builds sample `i` in LDS and writes it out with coalesced stores; g < 0: the sample is all zeros.
// A = Aux: also ownership [49], score [1], reply [833] and aux_weight [2], built in the LDS behind the sample.
template <class A>
__device__ void emit_sample(const View &v, float *lds, int i, int g, int p, int s, double blend, float *features,
                            float *policy, float *value, const A &aux)
{
    constexpr bool AUX = std::is_same<A, Aux>::value;
    const int lane = (int)threadIdx.x;
    for (int k = lane; k < (AUX ? AUX_LDS : SAMPLE_LDS) / 4; k += WAVE)
        reinterpret_cast<float4 *>(lds)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    if (g >= 0) {
        const uint4 game = v.games[g];
        const Ply ply = v.plies[game.x + (u32)p];
        const u64 walls = v.blockers ? v.blockers[g] : 0ULL;  // (wave-uniform)
        const int mover = 1 + (p & 1);  // x (1) moves on even plies
        const u64 mine = mover == 1 ? ply.x : ply.o, theirs = mover == 1 ? ply.o : ply.x;
        if (lane < 49) {  // cell [X][Y] of the image shows the cell its source was
            const int X = lane / 7, Y = lane - 7 * X;
            const int src = symmetry_source_cell(s, X + 7 * (6 - Y));
            reinterpret_cast<float4 *>(lds)[lane] =
                make_float4(1.f, (float)((mine >> src) & 1ULL), (float)((theirs >> src) & 1ULL), (float)((walls >> src) & 1ULL));
        }
        const u32 count = ply.targets_flags >> 8;
        for (u32 t = (u32)lane; t < count; t += WAVE) {
            const int index = v.target_index[ply.first_target + t];
            atomicAdd(&lds[FEATURES + symmetry_policy_index(s, index)], v.target_weight[ply.first_target + t]);
        }
        if (lane == 0) {
            const int z = (int)(game.z & 0xFFu) == mover ? 1 : -1;
            float out = (float)z;
            const double ret = v.returns ? v.returns[game.x + (u32)p] : 0.0;
            if (v.returns && f64_bits(ret) != RETURN_ABSENT)  // a covered ply: the lambda-return in place of z or the blend
                out = (float)ret;
            else if (blend != 0.0 && (game.z & GAME_HAS_VALUES))
                out = (float)((1.0 - blend) * (double)z + blend * ply.value);
            if (v.proofs) {  // a proven outcome stands above the game's result and the search's value
                const int proof = v.proofs[game.x + (u32)p];
                if (proof != 0)
                    out = proof > 0 ? 1.0f : -1.0f;
            }
            lds[FEATURES + POLICY] = out;
        }
        if constexpr (AUX) {
            const u64 own_x = aux.owners ? aux.owners[2 * g] : 0ULL, own_o = aux.owners ? aux.owners[2 * g + 1] : 0ULL;
            const u64 own_mine = mover == 1 ? own_x : own_o, own_theirs = mover == 1 ? own_o : own_x;
            if (lane < 49) {  // the same source cell as the feature planes
                const int X = lane / 7, Y = lane - 7 * X;
                const int src = symmetry_source_cell(s, X + 7 * (6 - Y));
                lds[AUX_OWNERSHIP + lane] = (float)(int)((own_mine >> src) & 1ULL) - (float)(int)((own_theirs >> src) & 1ULL);
            }
            // the reply: ply p + 1's target, where that ply is one a sample could have been drawn from
            bool reply = (u32)p + 1u < game.y;  // (wave-uniform)
            if (reply) {
                const Ply next = v.plies[game.x + (u32)p + 1u];
                const u32 f = next.targets_flags & 0xFFu;
                reply = !(f & (AZH_SAMPLES_PLY_PASS | AZH_SAMPLES_PLY_BAD)) && (!(game.z & GAME_HAS_FULL) || (f & AZH_SAMPLES_PLY_FULL));
                const u32 n_reply = reply ? next.targets_flags >> 8 : 0u;
                for (u32 t = (u32)lane; t < n_reply; t += WAVE) {
                    const int index = v.target_index[next.first_target + t];
                    atomicAdd(&lds[AUX_REPLY + symmetry_policy_index(s, index)], v.target_weight[next.first_target + t]);
                }
            }
            if (lane == 0) {
                lds[AUX_SCORE] = (float)((int)__popcll(own_mine) - (int)__popcll(own_theirs));
                lds[AUX_WEIGHT] = (own_x | own_o) ? 1.f : 0.f;
                lds[AUX_WEIGHT + 1] = reply ? 1.f : 0.f;
            }
        }
    }
    __syncthreads();
    if (lane < 49)
        reinterpret_cast<float4 *>(features + (size_t)i * FEATURES)[lane] = reinterpret_cast<const float4 *>(lds)[lane];
    float *row = policy + (size_t)i * POLICY;  // rows are 3332 bytes apart: four-byte stores, 256 contiguous bytes per wave
    for (int k = lane; k < POLICY; k += WAVE)
        row[k] = lds[FEATURES + k];
    if (lane == 0)
        value[i] = lds[FEATURES + POLICY];
    if constexpr (AUX) {
        if (lane < 49)
            aux.ownership[(size_t)i * 49 + lane] = lds[AUX_OWNERSHIP + lane];
        float *reply_row = aux.reply + (size_t)i * POLICY;
        for (int k = lane; k < POLICY; k += WAVE)
            reply_row[k] = lds[AUX_REPLY + k];
        if (lane == 0)
            aux.score[i] = lds[AUX_SCORE];
        if (lane < 2)
            aux.weight[2 * (size_t)i + lane] = lds[AUX_WEIGHT + lane];
    }
}

__global__ __launch_bounds__(WAVE) void k_samples_gather(View v, int n, const int *draws, double blend, float *features,
                                                         float *policy, float *value)
{
    __shared__ __attribute__((aligned(16))) float lds[SAMPLE_LDS];
    const int i = (int)blockIdx.x;
    if (i >= n)
        return;
    emit_sample(v, lds, i, draws[3 * i], draws[3 * i + 1], draws[3 * i + 2], blend, features, policy, value, NoAux{});
}

__global__ __launch_bounds__(WAVE) void k_samples_gather_aux(View v, int n, const int *draws, double blend, float *features,
                                                             float *policy, float *value, Aux aux)
{
    __shared__ __attribute__((aligned(16))) float lds[AUX_LDS];
    const int i = (int)blockIdx.x;
    if (i >= n)
        return;
    emit_sample(v, lds, i, draws[3 * i], draws[3 * i + 1], draws[3 * i + 2], blend, features, policy, value, aux);
}

// One attempt of sample `i`'s draw from the arrays of `v`, or of the host mirror: the same function on both sides.
struct Attempt {
    int game, ply, symmetry;
    bool ok;
};

// `weighted`: the ply is picked by cum_at (the running sums of the game's candidate weights) instead of uniformly.
template <class GameAt, class CountAt, class CandidateAt, class FlagsAt, class CumAt>
__host__ __device__ inline Attempt draw_attempt(u32 k0, u32 k1, u32 step, u32 i, u32 a, u32 first_game, u32 n_games,
                                                GameAt game_at, CountAt count_at, CandidateAt candidate_at, FlagsAt flags_at,
                                                bool weighted, CumAt cum_at)
{
    const Philox4 r = philox(k0, k1, step, i, a, STREAM_SAMPLE_DRAW);
    Attempt out;
    out.game = (int)(first_game + (u32)(((u64)r.v[0] * n_games) >> 32));
    out.symmetry = (int)(r.v[2] >> 29);
    const uint4 game = game_at(out.game);
    const u32 c = count_at(out.game);
    out.ply = 0;
    out.ok = c != 0;  // a game that carries "full" without one full ply gives no sample, whatever else it carries
    u32 k = 0;
    if (out.ok && weighted) {
        const u32 total = cum_at(game.x + c - 1u);
        out.ok = total != 0u;
        const u32 R = (u32)(((u64)r.v[1] * total) >> 32);
        u32 lo = 0, hi = c - 1u;  // the first k with cum[k] > R: cum[c - 1] = total > R
        while (lo < hi) {
            const u32 mid = (lo + hi) >> 1;
            if (cum_at(game.x + mid) > R)
                hi = mid;
            else
                lo = mid + 1u;
        }
        k = lo;
    } else if (out.ok) {
        k = (u32)(((u64)r.v[1] * c) >> 32);
    }
    if (out.ok) {
        out.ply = game.w ? (int)game.w : (int)candidate_at(game.x + k);
        out.ok = (u32)out.ply < game.y &&
                 !(flags_at(game.x + (u32)out.ply) & (AZH_SAMPLES_PLY_PASS | AZH_SAMPLES_PLY_BAD));
    }
    return out;
}

// Sample i's draw: lane a makes attempt a; the first one that succeeds is the draw.  -> (game, ply, symmetry) in every lane, -1
// each when all 64 attempts fail (counted in *errors).
struct Draw {
    int g, p, s;
};
__device__ __forceinline__ Draw draw_sample(const View &v, int i, u32 k0, u32 k1, u32 step, u32 first_game, u32 n_games,
                                            int *draws_out, u32 *errors)
{
    const int lane = (int)threadIdx.x;  // lane a makes attempt a; the first one that succeeds is the draw
    const Attempt mine = draw_attempt(
        k0, k1, step, (u32)i, (u32)lane, first_game, n_games, [&](int g) { return v.games[g]; },
        [&](int g) { return v.candidate_count[g]; }, [&](u32 at) { return (u32)v.candidates[at]; },
        [&](u32 at) { return v.plies[at].targets_flags & 0xFFu; }, v.cum != nullptr, [&](u32 at) { return v.cum[at]; });
    const u64 ok = __ballot(mine.ok);
    const int first = ok ? (int)__builtin_ctzll(ok) : 0;
    const int g = ok ? __shfl(mine.game, first) : -1;
    const int p = ok ? __shfl(mine.ply, first) : -1;
    const int s = ok ? __shfl(mine.symmetry, first) : -1;
    if (lane == 0) {
        if (!ok)
            atomicAdd(errors, 1u);
        if (draws_out) {
            draws_out[4 * i] = g;
            draws_out[4 * i + 1] = p;
            draws_out[4 * i + 2] = s;
            draws_out[4 * i + 3] = ok ? first + 1 : MAX_ATTEMPTS;
        }
    }
    return Draw{g, p, s};
}

__global__ __launch_bounds__(WAVE) void k_samples_draw_gather(View v, int n, u32 k0, u32 k1, u32 step, u32 first_game,
                                                              u32 n_games, double blend, float *features, float *policy,
                                                              float *value, int *draws_out, u32 *errors)
{
    __shared__ __attribute__((aligned(16))) float lds[SAMPLE_LDS];
    const int i = (int)blockIdx.x;
    if (i >= n)
        return;
    const Draw d = draw_sample(v, i, k0, k1, step, first_game, n_games, draws_out, errors);
    emit_sample(v, lds, i, d.g, d.p, d.s, blend, features, policy, value, NoAux{});
}

__global__ __launch_bounds__(WAVE) void k_samples_draw_gather_aux(View v, int n, u32 k0, u32 k1, u32 step, u32 first_game,
                                                                  u32 n_games, double blend, float *features, float *policy,
                                                                  float *value, int *draws_out, u32 *errors, Aux aux)
{
    __shared__ __attribute__((aligned(16))) float lds[AUX_LDS];
    const int i = (int)blockIdx.x;
    if (i >= n)
        return;
    const Draw d = draw_sample(v, i, k0, k1, step, first_game, n_games, draws_out, errors);
    emit_sample(v, lds, i, d.g, d.p, d.s, blend, features, policy, value, aux);
}

// ---------------------------------------------------------------- policy surprise (include/ataxxzero_hip.h)

// The stored value of a ply's KL: a negative, NaN or infinite sum reads 0.
__host__ __device__ inline float stored_surprise(float kl) { return (kl >= 0.0f && kl <= 3.40282347e38f) ? kl : 0.0f; }
// One target's term; lp = log p_t.
__host__ __device__ inline float surprise_term(float w, float lp) { return w * (det_logf(w) - lp); }

// The boards of plies [first, first + n) as the tower takes them: (mover, opponent).
__global__ __launch_bounds__(256) void k_samples_pack_boards(View v, u32 first, int n, u64 *boards)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n)
        return;
    const Ply ply = v.plies[first + (u32)i];
    const bool odd = (ply.targets_flags & PLY_ODD) != 0;
    boards[2 * i] = odd ? ply.o : ply.x;
    boards[2 * i + 1] = odd ? ply.x : ply.o;
}

// One wave per ply: movegen into LDS, the legal moves marked in an 833-cell map and their logits reduced to (mx, S) in the
// engine's lane order (apply_priors: move j in lane j % 64, ascending j, then the butterfly), then the targets 64 per step.
// logits: row i belongs to ply first + i.  A position has at most 49 * 16 jumps and 49 clones: the move list holds them all.
// blockers: the wall mask of the game(s) the plies belong to — one per launch: the host cuts its launches at mask changes.
__global__ __launch_bounds__(WAVE) void k_samples_surprise(View v, u32 first, int n, const float *__restrict__ logits,
                                                           float *__restrict__ kl_out, u32 *illegal, u64 blockers)
{
    __shared__ u16 moves[POLICY + 3];
    __shared__ u32 legal[(POLICY + 31) / 32];
    const int i = (int)blockIdx.x;
    if (i >= n)
        return;
    const int lane = (int)threadIdx.x;
    const Ply ply = v.plies[first + (u32)i];
    const u32 flags = ply.targets_flags & 0xFFu;
    float out = 0.0f;
    if (!(flags & (AZH_SAMPLES_PLY_PASS | AZH_SAMPLES_PLY_BAD))) {  // (wave-uniform)
        if (lane < (POLICY + 31) / 32)
            legal[lane] = 0u;
        Board b;
        b.x = ply.x;
        b.o = ply.o;
        b.turn = (flags & PLY_ODD) ? 1 : 0;
        const int M = wave_movegen(b, blockers, moves, nullptr);
        __syncthreads();
        const float *row = logits + (size_t)i * POLICY;
        float mx = -INFINITY;
        for (int j = lane; j < M; j += WAVE) {
            const int at = policy_index(moves[j]);
            atomicOr(&legal[at >> 5], 1u << (at & 31));
            const float l = row[at];
            if (l > mx)
                mx = l;
        }
        mx = wave_max_f32(mx);
        float part = 0.0f;
        for (int j = lane; j < M; j += WAVE)
            part = part + det_expf(row[policy_index(moves[j])] - mx);
        const float log_s = det_logf(wave_sum_f32(part));
        __syncthreads();
        const u32 count = ply.targets_flags >> 8;
        float acc = 0.0f;
        int missing = 0;
        for (u32 t = (u32)lane; t < count; t += WAVE) {
            const int at = v.target_index[ply.first_target + t];
            const float w = v.target_weight[ply.first_target + t];
            if (w > 0.0f) {
                if ((legal[at >> 5] >> (at & 31)) & 1u)
                    acc = acc + surprise_term(w, (row[at] - mx) - log_s);
                else
                    missing++;
            }
        }
        out = stored_surprise(wave_sum_f32(acc));
        missing = wave_sum_int(missing);
        if (lane == 0 && missing)
            atomicAdd(illegal, (u32)missing);
    }
    if (lane == 0)
        kl_out[first + (u32)i] = out;
}

template <class T>
struct DeviceArray {
    T *d = nullptr;
    int alloc(size_t n)
    {
        AZH_HIP(hipMalloc((void **)&d, std::max<size_t>(n, 1) * sizeof(T)));
        return 0;
    }
    void release()
    {
        if (d)
            (void)hipFree(d);
        d = nullptr;
    }
};

// |1 - sum| >= 1e-3 over the ply's weights added in f32 in ascending index order (equal indices in the order given)
bool bad_target(const uint16_t *index, const float *weight, size_t n)
{
    std::vector<size_t> order(n);
    for (size_t j = 0; j < n; j++)
        order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return index[a] < index[b]; });
    float sum = 0.f;
    for (size_t j : order)
        sum += weight[j];
    return fabsf(1.f - sum) >= 1e-3f;
}

bool board_move(uint32_t mv)  // a clone, or a jump over a distance of exactly two
{
    const int from = mv & 0xFF, to = (mv >> 8) & 0xFF;
    if (from >= 49 || to >= 49)
        return false;
    const int dx = abs(to % 7 - from % 7), dy = abs(to / 7 - from / 7);
    return from == to || std::max(dx, dy) == 2;
}

}  // namespace

struct azh_samples {
    int64_t cap_games = 0, cap_plies = 0, cap_targets = 0;
    int64_t games = 0, plies = 0, targets = 0, bad_plies = 0;
    DeviceArray<uint4> d_games;
    DeviceArray<Ply> d_plies;
    DeviceArray<u16> d_candidates;
    DeviceArray<u32> d_candidate_count;
    DeviceArray<u16> d_target_index;
    DeviceArray<float> d_target_weight;
    DeviceArray<u32> d_errors;
    DeviceArray<u64> d_blockers;      // [cap_games]: null until the first game with walls arrives
    std::vector<u64> h_blockers;      // [games]
    DeviceArray<u64> d_owners;        // [cap_games][2]: null until the first game with owners arrives
    std::vector<u64> h_owners;        // [games][2]
    // policy surprise weighting: all null until asked for
    DeviceArray<u32> d_cum;      // [cap_plies] beside d_candidates (azh_samples_set_ply_weights)
    DeviceArray<float> d_kl;     // [cap_plies]: the last surprise of every ply
    DeviceArray<u32> d_illegal;  // [1]
    std::vector<u32> h_cum;      // [plies] while d_cum is held
    int surprise_chunk = SURPRISE_CHUNK;
    float surprise_ms[2] = {0.f, 0.f};
    // reanalysis: scratch of azh_samples_read_plies and azh_samples_retarget, null until one of them is called
    DeviceArray<unsigned char> d_scratch;
    size_t scratch_bytes = 0;
    // proven outcomes (azh_samples_prove): all null until its first call that commits
    DeviceArray<int16_t> d_proofs;       // [cap_plies]: 0, or the search's value, |value| >= 1000
    DeviceArray<u16> d_proof_moves;      // [cap_plies]: the move of the ply's last search, 0xFFFF before one
    DeviceArray<uint8_t> d_proof_depths; // [cap_plies]: the iteration that search completed
    std::vector<int16_t> h_proofs;       // [plies at the last call]: the mirror of d_proofs
    // lambda-returns (azh_samples_value_returns): null until its first call, and again after azh_samples_clear_value_returns
    DeviceArray<double> d_returns;       // [cap_plies]: G_p, RETURN_ABSENT where no pass has covered the ply
    // the host mirror: what a draw is validated against
    std::vector<uint32_t> h_games;  // [games][4]
    std::vector<uint8_t> h_flags;   // [plies]
    std::vector<u16> h_candidates;  // [plies]
    std::vector<u32> h_count;       // [games]
    // draws on their way to the device: two pinned buffers and two device buffers taken in turn, each guarded by the event
    // recorded behind the kernel that read it, so the next call never waits for this one
    hipStream_t stream = nullptr;
    int *h_stage[2] = {nullptr, nullptr};
    int *d_stage[2] = {nullptr, nullptr};
    hipEvent_t used[2] = {nullptr, nullptr};
    int64_t stage_rows = 0;
    int turn = 0;

    View view() const
    {
        return View{d_games.d, d_plies.d, d_candidates.d, d_candidate_count.d, d_target_index.d, d_target_weight.d, d_cum.d,
                    d_blockers.d, d_proofs.d, d_returns.d};
    }
};

static void release_stage(azh_samples *s)
{
    for (int k = 0; k < 2; k++) {
        if (s->used[k]) {
            (void)hipEventSynchronize(s->used[k]);
            (void)hipEventDestroy(s->used[k]);
        }
        if (s->h_stage[k])
            (void)hipHostFree(s->h_stage[k]);
        if (s->d_stage[k])
            (void)hipFree(s->d_stage[k]);
        s->used[k] = nullptr;
        s->h_stage[k] = s->d_stage[k] = nullptr;
    }
    s->stage_rows = 0;
}

static int reserve_stage(azh_samples *s, int64_t rows)
{
    if (rows <= s->stage_rows)
        return 0;
    release_stage(s);
    for (int k = 0; k < 2; k++) {
        AZH_HIP(hipHostMalloc((void **)&s->h_stage[k], (size_t)rows * 3 * sizeof(int), hipHostMallocDefault));
        AZH_HIP(hipMalloc((void **)&s->d_stage[k], (size_t)rows * 3 * sizeof(int)));
        AZH_HIP(hipEventCreateWithFlags(&s->used[k], hipEventDisableTiming));
    }
    s->stage_rows = rows;
    return 0;
}

extern "C" void azh_samples_destroy(azh_samples *s)
{
    if (!s)
        return;
    if (s->stream)
        (void)hipStreamSynchronize(s->stream);
    release_stage(s);
    s->d_games.release();
    s->d_plies.release();
    s->d_candidates.release();
    s->d_candidate_count.release();
    s->d_target_index.release();
    s->d_target_weight.release();
    s->d_errors.release();
    s->d_blockers.release();
    s->d_owners.release();
    s->d_cum.release();
    s->d_kl.release();
    s->d_illegal.release();
    s->d_scratch.release();
    s->d_proofs.release();
    s->d_proof_moves.release();
    s->d_proof_depths.release();
    s->d_returns.release();
    if (s->stream)
        (void)hipStreamDestroy(s->stream);
    delete s;
}

extern "C" int azh_samples_create(int64_t cap_games, int64_t cap_plies, int64_t cap_targets, azh_samples **out)
{
    if (!out)
        return azh_fail(-1, "azh_samples_create: null argument");
    *out = nullptr;
    if (cap_games < 1 || cap_plies < 1 || cap_targets < 1 || cap_games > 0x7FFFFFFF || cap_plies > 0x7FFFFFFF ||
        cap_targets > 0x7FFFFFFF)
        return azh_fail(-1, "azh_samples_create: capacities must lie in [1, 2^31)");
    if (int rc = azh_require_device())
        return rc;
    azh_samples *s = new azh_samples;
    s->cap_games = cap_games;
    s->cap_plies = cap_plies;
    s->cap_targets = cap_targets;
    int rc = s->d_games.alloc((size_t)cap_games);
    rc = rc ? rc : s->d_plies.alloc((size_t)cap_plies);
    rc = rc ? rc : s->d_candidates.alloc((size_t)cap_plies);
    rc = rc ? rc : s->d_candidate_count.alloc((size_t)cap_games);
    rc = rc ? rc : s->d_target_index.alloc((size_t)cap_targets);
    rc = rc ? rc : s->d_target_weight.alloc((size_t)cap_targets);
    rc = rc ? rc : s->d_errors.alloc(1);
    if (!rc) {
        const hipError_t e1 = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
        const hipError_t e2 = e1 == hipSuccess ? hipMemset(s->d_errors.d, 0, sizeof(u32)) : e1;
        if (e2 != hipSuccess)
            rc = azh_fail(-100 - (int)e2, "azh_samples_create: %s", hipGetErrorString(e2));
    }
    if (rc) {
        azh_samples_destroy(s);
        return rc;
    }
    *out = s;
    return 0;
}

// A wall mask with bits beyond the 49 cells, or a stone of plies [0, n) on a wall cell: why, or null.
static const char *walls_refusal(uint64_t mask, const uint64_t *boards, int64_t n, int64_t *ply)
{
    *ply = -1;
    if (mask & ~BOARD_MASK)
        return "the blockers mask has bits beyond the 49 cells";
    for (int64_t q = 0; q < n; q++)
        if ((boards[2 * q] | boards[2 * q + 1]) & mask) {
            *ply = q;
            return "a stone stands on a wall cell";
        }
    return nullptr;
}

// A game's owner masks against its walls and its recorded result: why they are refused, or null.
static const char *owners_refusal(uint64_t own_x, uint64_t own_o, uint64_t walls, uint32_t result)
{
    if (!(own_x | own_o))
        return nullptr;
    if (own_x & own_o)
        return "the owner masks overlap";
    if ((own_x | own_o) & (walls | ~BOARD_MASK))
        return "an owner mask has bits on walls or beyond the 49 cells";
    if ((own_x | own_o | walls) != BOARD_MASK)
        return "the owner masks leave a cell that is no wall unowned";
    const int margin = __builtin_popcountll(own_x) - __builtin_popcountll(own_o);
    if (result != (margin < 0 ? 2u : 1u))
        return "the owners' margin contradicts the recorded result";
    return nullptr;
}

extern "C" int azh_samples_check_owners(uint64_t own_x, uint64_t own_o, uint64_t blockers, uint32_t result)
{
    if (const char *why = owners_refusal(own_x, own_o, blockers, result))
        return azh_fail(-2, "azh_samples_check_owners: owners %#llx, %#llx, walls %#llx, result %u: %s", (unsigned long long)own_x,
                        (unsigned long long)own_o, (unsigned long long)blockers, (unsigned)result, why);
    return 0;
}

extern "C" int azh_samples_add_games(azh_samples *s, const azh_sample_arrays *a)
{
    if (!s || !a)
        return azh_fail(-1, "azh_samples_add_games: null argument");
    const int64_t n_games = a->n_games, n_plies = a->n_plies, n_targets = a->n_targets;
    const uint32_t *games = a->games;
    const uint64_t *boards = a->boards, *game_blockers = a->game_blockers, *game_owners = a->game_owners;
    const uint8_t *ply_flags = a->ply_flags;
    const double *values = a->values;
    const int32_t *target_start = a->target_start;
    const uint16_t *target_index = a->target_index;
    const float *target_weight = a->target_weight;
    if (n_games < 0 || n_plies < 0 || (n_games && !games) || (n_plies && (!boards || !ply_flags || !values)) || !target_start)
        return azh_fail(-1, "azh_samples_add_games: null argument");
    if (target_start[0] != 0 || n_targets < 0 || (n_targets && (!target_index || !target_weight)))
        return azh_fail(-2, "azh_samples_add_games: target_start must begin at 0 and the targets must be given");
    if (n_targets != target_start[n_plies])
        return azh_fail(-2, "azh_samples_add_games: n_targets is %lld, target_start ends at %lld", (long long)n_targets,
                        (long long)target_start[n_plies]);
    // everything is checked and built on the host first: a refused call leaves the store exactly as it was
    std::vector<uint4> g_words((size_t)n_games);
    std::vector<u32> g_count((size_t)n_games);
    std::vector<Ply> p_words((size_t)n_plies);
    std::vector<u16> p_candidates((size_t)n_plies);
    std::vector<uint8_t> p_flags((size_t)n_plies);
    int64_t at = 0, bad = 0;
    bool walled = false, owned = false;
    for (int64_t g = 0; g < n_games; g++) {
        const uint32_t *w = games + 4 * g;
        const uint32_t result = w[2] & 0xFFu;
        if ((int64_t)w[0] != at || w[1] < 1 || w[1] > 0xFFFFu || at + w[1] > n_plies || result > 2 ||
            (w[2] & ~(0xFFu | GAME_HAS_FULL | GAME_HAS_VALUES)) || w[3] > 0xFFFFu)
            return azh_fail(-2, "azh_samples_add_games: game %lld: plies must follow each other (1 .. 65535 each), result "
                                "must be 0 .. 2 and the flags known ones", (long long)g);
        u32 c = 0;
        for (uint32_t p = 0; p < w[1]; p++) {
            const int64_t q = at + p;
            const int64_t lo = target_start[q], hi = target_start[q + 1];
            if (lo > hi || hi > n_targets || hi - lo > 0xFFFFFF || (ply_flags[q] & ~(AZH_SAMPLES_PLY_PASS | AZH_SAMPLES_PLY_FULL)))
                return azh_fail(-2, "azh_samples_add_games: ply %lld: targets out of order or unknown flags", (long long)q);
            for (int64_t t = lo; t < hi; t++)
                if (target_index[t] >= POLICY)
                    return azh_fail(-2, "azh_samples_add_games: policy index %u", (unsigned)target_index[t]);
            uint8_t f = ply_flags[q];
            if (bad_target(target_index + lo, target_weight + lo, (size_t)(hi - lo))) {
                f |= AZH_SAMPLES_PLY_BAD;
                bad += !(f & AZH_SAMPLES_PLY_PASS);  // (a pass has no target and is never a sample: not worth a warning)
            }
            p_flags[(size_t)q] = f;
            p_words[(size_t)q] = Ply{boards[2 * q] & BOARD_MASK, boards[2 * q + 1] & BOARD_MASK, values[q],
                                     (u32)(s->targets + lo), (u32)(hi - lo) << 8 | f | ((p & 1u) ? PLY_ODD : 0u)};
            if (!(w[2] & GAME_HAS_FULL) || (f & AZH_SAMPLES_PLY_FULL))
                p_candidates[(size_t)(at + c++)] = (u16)p;
        }
        if (game_blockers) {
            int64_t ply = -1;
            if (const char *why = walls_refusal(game_blockers[g], boards + 2 * at, (int64_t)w[1], &ply))
                return azh_fail(-2, "azh_samples_add_games: game %lld (blockers %#llx, ply %lld): %s", (long long)g,
                                (unsigned long long)game_blockers[g], (long long)ply, why);
            walled = walled || game_blockers[g] != 0;
        }
        if (game_owners) {
            const uint64_t own_x = game_owners[2 * g], own_o = game_owners[2 * g + 1];
            if (const char *why = owners_refusal(own_x, own_o, game_blockers ? game_blockers[g] : 0ULL, result))
                return azh_fail(-2, "azh_samples_add_games: game %lld (owners %#llx, %#llx, result %u): %s", (long long)g,
                                (unsigned long long)own_x, (unsigned long long)own_o, (unsigned)result, why);
            owned = owned || (own_x | own_o) != 0;
        }
        g_words[(size_t)g] = make_uint4((u32)(s->plies + at), w[1], w[2], w[3]);
        g_count[(size_t)g] = c;
        at += w[1];
    }
    if (at != n_plies)
        return azh_fail(-2, "azh_samples_add_games: the games hold %lld plies, %lld were given", (long long)at, (long long)n_plies);
    if (s->games + n_games > s->cap_games || s->plies + n_plies > s->cap_plies || s->targets + n_targets > s->cap_targets)
        return azh_fail(-6, "azh_samples_add_games: %lld games, %lld plies, %lld targets do not fit beside %lld, %lld, %lld "
                            "in capacities %lld, %lld, %lld", (long long)n_games, (long long)n_plies, (long long)n_targets,
                        (long long)s->games, (long long)s->plies, (long long)s->targets, (long long)s->cap_games,
                        (long long)s->cap_plies, (long long)s->cap_targets);
    // (the copies go behind whatever the store's stream still runs and are waited for: the vectors die with this call.  A
    // gather in flight on another stream reads only what lies below the counts it was launched with.)
    std::vector<u64> g_blockers((size_t)n_games, 0ULL);
    if (game_blockers)
        std::copy(game_blockers, game_blockers + n_games, g_blockers.begin());
    if (walled && !s->d_blockers.d) {  // the first walls: every game stored so far has none
        if (int rc = s->d_blockers.alloc((size_t)s->cap_games))
            return rc;
        AZH_HIP(hipMemsetAsync(s->d_blockers.d, 0, (size_t)s->cap_games * sizeof(u64), s->stream));
    }
    if (n_games && s->d_blockers.d)
        AZH_HIP(hipMemcpyAsync(s->d_blockers.d + s->games, g_blockers.data(), (size_t)n_games * sizeof(u64), hipMemcpyHostToDevice, s->stream));
    std::vector<u64> g_owners((size_t)n_games * 2, 0ULL);
    if (game_owners)
        std::copy(game_owners, game_owners + 2 * n_games, g_owners.begin());
    if (owned && !s->d_owners.d) {  // the first owners: every game stored so far has none
        if (int rc = s->d_owners.alloc((size_t)s->cap_games * 2))
            return rc;
        AZH_HIP(hipMemsetAsync(s->d_owners.d, 0, (size_t)s->cap_games * 2 * sizeof(u64), s->stream));
    }
    if (n_games && s->d_owners.d)
        AZH_HIP(hipMemcpyAsync(s->d_owners.d + 2 * s->games, g_owners.data(), (size_t)n_games * 2 * sizeof(u64), hipMemcpyHostToDevice, s->stream));
    if (n_games) {
        AZH_HIP(hipMemcpyAsync(s->d_games.d + s->games, g_words.data(), (size_t)n_games * sizeof(uint4), hipMemcpyHostToDevice, s->stream));
        AZH_HIP(hipMemcpyAsync(s->d_candidate_count.d + s->games, g_count.data(), (size_t)n_games * sizeof(u32), hipMemcpyHostToDevice, s->stream));
    }
    if (n_plies) {
        AZH_HIP(hipMemcpyAsync(s->d_plies.d + s->plies, p_words.data(), (size_t)n_plies * sizeof(Ply), hipMemcpyHostToDevice, s->stream));
        AZH_HIP(hipMemcpyAsync(s->d_candidates.d + s->plies, p_candidates.data(), (size_t)n_plies * sizeof(u16), hipMemcpyHostToDevice, s->stream));
    }
    if (n_targets) {
        AZH_HIP(hipMemcpyAsync(s->d_target_index.d + s->targets, target_index, (size_t)n_targets * sizeof(u16), hipMemcpyHostToDevice, s->stream));
        AZH_HIP(hipMemcpyAsync(s->d_target_weight.d + s->targets, target_weight, (size_t)n_targets * sizeof(float), hipMemcpyHostToDevice, s->stream));
    }
    std::vector<u32> p_cum;
    if (s->d_cum.d && n_plies) {  // weights are held: the new games' candidates weigh one each
        p_cum.resize((size_t)n_plies);
        for (int64_t g = 0; g < n_games; g++)
            for (u32 k = 0; k < games[4 * g + 1]; k++)
                p_cum[(size_t)games[4 * g] + k] = WEIGHT_ONE * (k + 1u);
        AZH_HIP(hipMemcpyAsync(s->d_cum.d + s->plies, p_cum.data(), (size_t)n_plies * sizeof(u32), hipMemcpyHostToDevice, s->stream));
    }
    AZH_HIP(hipStreamSynchronize(s->stream));
    s->h_cum.insert(s->h_cum.end(), p_cum.begin(), p_cum.end());
    s->h_candidates.insert(s->h_candidates.end(), p_candidates.begin(), p_candidates.end());
    s->h_count.insert(s->h_count.end(), g_count.begin(), g_count.end());
    for (int64_t g = 0; g < n_games; g++) {
        const uint4 w = g_words[(size_t)g];
        s->h_games.insert(s->h_games.end(), {w.x, w.y, w.z, w.w});
    }
    s->h_flags.insert(s->h_flags.end(), p_flags.begin(), p_flags.end());
    s->h_blockers.insert(s->h_blockers.end(), g_blockers.begin(), g_blockers.end());
    s->h_owners.insert(s->h_owners.end(), g_owners.begin(), g_owners.end());
    s->games += n_games;
    s->plies += n_plies;
    s->targets += n_targets;
    s->bad_plies += bad;
    return 0;
}

// A record's owners: azh_samples_final_owners of its last ply's boards and move word.
static int record_owners(const RecordView &r, uint64_t blockers, uint64_t *owners)
{
    PlyView ply = r.first_ply();
    for (uint32_t p = 0; p + 1 < r.plies(); p++)
        ply = ply.next();
    int32_t result = 0;
    return azh_samples_final_owners(ply.x(), ply.o(), blockers, (int)((r.plies() - 1u) & 1u), ply.move(), owners, &result);
}

// Ring records -> the arrays azh_samples_add_games takes.  Host code only.
extern "C" int azh_samples_pack_records(const uint32_t *rec, int64_t words, uint64_t blockers, const uint64_t *record_masks,
                                        int64_t n_masks, int aux, azh_sample_arrays *out)
{
    // record_masks: null, or one mask per record of the buffer in its order (markers of dropped and loaded games included),
    // in place of `blockers`: records of an engine with a start pool (azh_engine_uid_blockers of each record's uid)
    if (record_masks && blockers)
        return azh_fail(-1, "azh_samples_pack_records: walls are given by `blockers` or by record_masks, not both");
    if (record_masks && n_masks < 0)
        return azh_fail(-1, "azh_samples_pack_records: %lld masks", (long long)n_masks);
    int64_t ri = 0;
    for (int64_t i = 0; record_masks && i < n_masks; i++)
        if (record_masks[i] & ~BOARD_MASK)
            return azh_fail(-2, "azh_samples_pack_records: the blockers mask %#llx of record %lld has bits beyond the 49 cells",
                            (unsigned long long)record_masks[i], (long long)i);
    if (blockers & ~BOARD_MASK)
        return azh_fail(-2, "azh_samples_pack_records: the blockers mask %#llx has bits beyond the 49 cells",
                        (unsigned long long)blockers);
    if (!out || (words > 0 && !rec) || words < 0)
        return azh_fail(-1, "azh_samples_pack_records: null argument");
    const bool write = out->games != nullptr;
    if (write && (!out->boards || !out->ply_flags || !out->values || !out->target_start || !out->target_index ||
                  !out->target_weight))
        return azh_fail(-1, "azh_samples_pack_records: null output array");
    const int64_t cap_games = out->n_games, cap_plies = out->n_plies, cap_targets = out->n_targets;
    // the first walk counts and refuses; nothing is written before the whole buffer has been found well formed
    int64_t n_games = 0, n_plies = 0, n_targets = 0;
    for (int64_t pos = 0; pos < words;) {
        const char *why = nullptr;
        if (!azh_record_well_formed(rec + pos, (size_t)(words - pos), 0u, &why))
            return azh_fail(-2, "azh_samples_pack_records: word %lld: %s", (long long)pos, why ? why : "not a record");
        const RecordView r{rec + pos};
        pos += r.words();
        if (record_masks) {
            if (ri >= n_masks)
                return azh_fail(-2, "azh_samples_pack_records: %lld masks for a buffer of more records", (long long)n_masks);
            blockers = record_masks[ri++];
        }
        if (r.dropped() || r.loaded())  // a dropped game's marker; a game begun at a loaded position: neither has a line
            continue;
        if (r.plies() < 1 || r.plies() > 0xFFFFu || r.random_ply_plus_1() > 0xFFFFu)
            return azh_fail(-2, "azh_samples_pack_records: a game of %u plies with result %u and random_ply + 1 = %u", r.plies(),
                            r.result(), r.random_ply_plus_1());
        PlyView ply = r.first_ply();
        for (uint32_t p = 0; p < r.plies(); p++, ply = ply.next()) {
            if ((ply.x() | ply.o()) & blockers)
                return azh_fail(-2, "azh_samples_pack_records: word %lld, ply %u: a stone stands on a wall cell of the "
                                    "blockers mask %#llx", (long long)(r.w - rec), p, (unsigned long long)blockers);
            for (uint32_t j = 0; j < ply.targets(); j++)
                if (!board_move(ply.target(j) & 0xFFFFu))
                    return azh_fail(-2, "azh_samples_pack_records: target %#x is no clone and no jump", ply.target(j) & 0xFFFFu);
            n_targets += ply.targets();
        }
        if (aux) {
            uint64_t owners[2];
            if (record_owners(r, blockers, owners))
                return azh_fail(-2, "azh_samples_pack_records: word %lld: the last move of the game is not legal at its last "
                                    "board", (long long)(r.w - rec));
        }
        n_games++;
        n_plies += r.plies();
    }
    if (record_masks && ri != n_masks)
        return azh_fail(-2, "azh_samples_pack_records: %lld masks for a buffer of %lld records", (long long)n_masks, (long long)ri);
    out->n_games = n_games;
    out->n_plies = n_plies;
    out->n_targets = n_targets;
    if (!write)
        return 0;
    if (n_games > cap_games || n_plies > cap_plies || n_targets > cap_targets)
        return azh_fail(-6, "azh_samples_pack_records: %lld games, %lld plies, %lld targets, the arrays hold %lld, %lld, %lld",
                        (long long)n_games, (long long)n_plies, (long long)n_targets, (long long)cap_games,
                        (long long)cap_plies, (long long)cap_targets);
    int64_t g = 0, q = 0, t = 0;
    ri = 0;
    std::vector<std::pair<std::string, uint32_t>> ents;
    out->target_start[0] = 0;
    for (int64_t pos = 0; pos < words;) {
        const RecordView r{rec + pos};
        pos += r.words();
        if (record_masks)
            blockers = record_masks[ri++];
        if (r.dropped() || r.loaded())
            continue;
        const bool valued = r.valued(), capped = r.capped();
        uint32_t *game = out->games + 4 * g;
        game[0] = (uint32_t)q;
        game[1] = r.plies();
        game[2] = r.result() | (capped ? GAME_HAS_FULL : 0u) | (valued ? GAME_HAS_VALUES : 0u);
        game[3] = r.random_ply_plus_1();
        if (out->game_blockers)
            out->game_blockers[g] = blockers;
        if (aux && out->game_owners)
            (void)record_owners(r, blockers, out->game_owners + 2 * g);  // (legal: the first walk has made this call)
        g++;
        PlyView ply = r.first_ply();
        for (uint32_t p = 0; p < r.plies(); p++, q++, ply = ply.next()) {
            out->boards[2 * q] = ply.x();
            out->boards[2 * q + 1] = ply.o();
            out->ply_flags[q] = capped && ply.full(valued) ? AZH_SAMPLES_PLY_FULL : 0;  // (the device loop records no pass: a ply is a move)
            out->values[q] = ply.value(valued);
            const uint64_t total = azh_ply_target(ply, ents);  // in the order of the line's "dists"
            for (const auto &e : ents) {
                out->target_index[t] = (uint16_t)policy_index(e.second & 0xFFFFu);
                out->target_weight[t] = total ? (float)((double)(e.second >> 16) / (double)total) : 0.f;
                t++;
            }
            out->target_start[q + 1] = (int32_t)t;
        }
    }
    return 0;
}

extern "C" int azh_samples_add_records(azh_samples *s, const uint32_t *rec, int64_t words, uint64_t blockers,
                                       const uint64_t *record_masks, int64_t n_masks, int aux)
{
    if (!s)
        return azh_fail(-1, "azh_samples_add_records: null store");
    azh_sample_arrays a = {};  // no arrays: the counts only
    if (int rc = azh_samples_pack_records(rec, words, blockers, record_masks, n_masks, aux, &a))
        return rc;
    std::vector<uint64_t> masks((size_t)a.n_games + 1), owners((size_t)a.n_games * 2 + 1);
    std::vector<uint32_t> games((size_t)a.n_games * 4 + 1);
    std::vector<uint64_t> boards((size_t)a.n_plies * 2 + 1);
    std::vector<uint8_t> flags((size_t)a.n_plies + 1);
    std::vector<double> values((size_t)a.n_plies + 1);
    std::vector<int32_t> start((size_t)a.n_plies + 1);
    std::vector<uint16_t> index((size_t)a.n_targets + 1);
    std::vector<float> weight((size_t)a.n_targets + 1);
    a = azh_sample_arrays{a.n_games, a.n_plies, a.n_targets, games.data(), boards.data(), flags.data(), values.data(),
                          start.data(), index.data(), weight.data(), masks.data(), owners.data()};
    if (int rc = azh_samples_pack_records(rec, words, blockers, record_masks, n_masks, aux, &a))
        return rc;
    a.game_blockers = blockers || record_masks ? masks.data() : nullptr;
    a.game_owners = aux ? owners.data() : nullptr;
    return azh_samples_add_games(s, &a);
}

extern "C" int azh_samples_final_owners(uint64_t x, uint64_t o, uint64_t blockers, int o_to_move, uint32_t move,
                                        uint64_t *owners_out, int32_t *result_out)
{
    if (!owners_out || !result_out)
        return azh_fail(-1, "azh_samples_final_owners: null argument");
    owners_out[0] = owners_out[1] = 0;
    *result_out = 0;
    if ((x | o | blockers) & ~BOARD_MASK || (x & o) || ((x | o) & blockers))
        return azh_fail(-2, "azh_samples_final_owners: boards %#llx, %#llx, walls %#llx overlap or leave the 49 cells",
                        (unsigned long long)x, (unsigned long long)o, (unsigned long long)blockers);
    Board b;
    b.x = x;
    b.o = o;
    b.turn = o_to_move ? 1 : 0;
    uint16_t legal[POLICY];
    int32_t n_legal = 0;  // the position's moves as the surprise pass lists them: the one statement of the rules on the host
    if (int rc = azh_samples_legal(b.turn ? o : x, b.turn ? x : o, blockers, legal, &n_legal))
        return rc;
    if ((move & 0xFFFFu) == 0xFFFFu) {
        if (n_legal)
            return azh_fail(-2, "azh_samples_final_owners: a pass where the mover has %d moves", (int)n_legal);
        b.turn ^= 1;  // a pass only hands the turn over
    } else {
        if (!board_move(move & 0xFFFFu))
            return azh_fail(-2, "azh_samples_final_owners: move %#x is no clone and no jump", (unsigned)move);
        const uint16_t *begin = legal, *end = legal + n_legal;
        if (std::find(begin, end, (uint16_t)policy_index(move & 0xFFFFu)) == end)
            return azh_fail(-2, "azh_samples_final_owners: move %#x is not legal for %s on %#llx, %#llx, walls %#llx",
                            (unsigned)move, b.turn ? "o" : "x", (unsigned long long)x, (unsigned long long)o,
                            (unsigned long long)blockers);
        b = make_move(b, (int)(move & 0xFFu), (int)((move >> 8) & 0xFFu));
    }
    // the kernels' order of checks (wave_movegen): a side without stones, then a stuck mover, then a full board
    const u64 empty = BOARD_MASK & ~(b.x | b.o | blockers);
    u64 own_x = b.x, own_o = b.o;
    if (azh_samples_legal(b.turn ? b.o : b.x, b.turn ? b.x : b.o, blockers, legal, &n_legal))
        return -1;
    if (!b.x || !b.o) {
        if ((b.turn ? !b.x : !b.o) && !n_legal && empty)
            return azh_fail(-2, "azh_samples_final_owners: the mover is stuck and its opponent has no stones: the reference's "
                                "two orders of adjudication disagree here");
        (b.x ? own_x : own_o) |= empty;
    } else if (!n_legal) {
        (b.turn ? own_x : own_o) |= empty;  // the mover is stuck: the empty cells go to the side not to move
    } else if (empty) {
        return 0;  // the game goes on: no owners
    }
    owners_out[0] = own_x;
    owners_out[1] = own_o;
    *result_out = __builtin_popcountll(own_x) < __builtin_popcountll(own_o) ? 2 : 1;
    return 0;
}

extern "C" int azh_samples_game_owners(const azh_samples *s, uint64_t *owners)
{
    if (!s || !owners)
        return azh_fail(-1, "azh_samples_game_owners: null argument");
    if (!s->h_owners.empty())
        memcpy(owners, s->h_owners.data(), s->h_owners.size() * sizeof(uint64_t));
    return 0;
}

extern "C" int azh_samples_counts(const azh_samples *s, int64_t *out)
{
    if (!s || !out)
        return azh_fail(-1, "azh_samples_counts: null argument");
    out[0] = s->games;
    out[1] = s->plies;
    out[2] = s->targets;
    out[3] = s->bad_plies;
    return 0;
}

extern "C" int azh_samples_mirror(const azh_samples *s, uint32_t *games, uint8_t *ply_flags)
{
    if (!s || !games || !ply_flags)
        return azh_fail(-1, "azh_samples_mirror: null argument");
    if (!s->h_games.empty())
        memcpy(games, s->h_games.data(), s->h_games.size() * sizeof(uint32_t));
    if (!s->h_flags.empty())
        memcpy(ply_flags, s->h_flags.data(), s->h_flags.size());
    return 0;
}

extern "C" int azh_samples_game_blockers(const azh_samples *s, uint64_t *blockers)
{
    if (!s || !blockers)
        return azh_fail(-1, "azh_samples_game_blockers: null argument");
    if (!s->h_blockers.empty())
        memcpy(blockers, s->h_blockers.data(), s->h_blockers.size() * sizeof(uint64_t));
    return 0;
}

// The outputs of a minibatch call: 0 with *aux set when the four auxiliary arrays are given, 0 with it clear when none is.
static int check_outputs(const char *what, const azh_sample_outputs *out, bool *aux)
{
    if (!out || !out->features || !out->policy || !out->value)
        return azh_fail(-1, "%s: null argument", what);
    const int given = !!out->ownership + !!out->score + !!out->reply + !!out->aux_weight;
    if (given != 0 && given != 4)
        return azh_fail(-1, "%s: %d of the four auxiliary outputs are given: all or none", what, given);
    *aux = given == 4;
    return 0;
}

extern "C" int azh_samples_gather(azh_samples *s, int n, const int32_t *draws, double value_blend,
                                  const azh_sample_outputs *out, uintptr_t stream)
{
    bool aux = false;
    if (!s || !draws)
        return azh_fail(-1, "azh_samples_gather: null argument");
    if (int rc = check_outputs("azh_samples_gather", out, &aux))
        return rc;
    if (n < 1)
        return azh_fail(-1, "azh_samples_gather: n must be at least 1");
    if (!(value_blend == value_blend))
        return azh_fail(-1, "azh_samples_gather: value_blend is not a number");
    for (int i = 0; i < n; i++) {  // no kernel ever sees an index it cannot serve
        const int64_t g = draws[3 * i], p = draws[3 * i + 1], sym = draws[3 * i + 2];
        if (g < 0 || g >= s->games || p < 0 || p >= (int64_t)s->h_games[4 * g + 1] || sym < 0 || sym > 7)
            return azh_fail(-1, "azh_samples_gather: draw %d (game %lld, ply %lld, symmetry %lld) is out of range", i,
                            (long long)g, (long long)p, (long long)sym);
        const uint8_t f = s->h_flags[s->h_games[4 * g] + p];
        if (f & AZH_SAMPLES_PLY_PASS)
            return azh_fail(-1, "azh_samples_gather: draw %d (game %lld, ply %lld) is a pass", i, (long long)g, (long long)p);
        if (f & AZH_SAMPLES_PLY_BAD)
            return azh_fail(-2, "azh_samples_gather: draw %d (game %lld, ply %lld): policy target does not sum to one", i,
                            (long long)g, (long long)p);
    }
    if (int rc = reserve_stage(s, n))
        return rc;
    const int k = s->turn;
    s->turn ^= 1;
    AZH_HIP(hipEventSynchronize(s->used[k]));  // the call before the last one: long done in a training loop
    memcpy(s->h_stage[k], draws, (size_t)n * 3 * sizeof(int));
    hipStream_t st = stream ? (hipStream_t)stream : s->stream;
    AZH_HIP(hipMemcpyAsync(s->d_stage[k], s->h_stage[k], (size_t)n * 3 * sizeof(int), hipMemcpyHostToDevice, st));
    if (aux)
        hipLaunchKernelGGL(k_samples_gather_aux, dim3((unsigned)n), dim3(WAVE), 0, st, s->view(), n, s->d_stage[k], value_blend,
                           out->features, out->policy, out->value,
                           Aux{s->d_owners.d, out->ownership, out->score, out->reply, out->aux_weight});
    else
        hipLaunchKernelGGL(k_samples_gather, dim3((unsigned)n), dim3(WAVE), 0, st, s->view(), n, s->d_stage[k], value_blend,
                           out->features, out->policy, out->value);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipEventRecord(s->used[k], st));
    if (!stream)
        AZH_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int azh_samples_draw_gather(azh_samples *s, int n, uint64_t seed, uint32_t step, int64_t first_game,
                                       int64_t n_games, double value_blend, const azh_sample_outputs *out, int32_t *draws_out,
                                       uintptr_t stream)
{
    bool aux = false;
    if (!s)
        return azh_fail(-1, "azh_samples_draw_gather: null argument");
    if (int rc = check_outputs("azh_samples_draw_gather", out, &aux))
        return rc;
    if (n < 1 || first_game < 0 || n_games < 1 || first_game + n_games > s->games)
        return azh_fail(-1, "azh_samples_draw_gather: n = %d, games [%lld, %lld) of %lld", n, (long long)first_game,
                        (long long)(first_game + n_games), (long long)s->games);
    if (!(value_blend == value_blend))
        return azh_fail(-1, "azh_samples_draw_gather: value_blend is not a number");
    hipStream_t st = stream ? (hipStream_t)stream : s->stream;
    if (aux)
        hipLaunchKernelGGL(k_samples_draw_gather_aux, dim3((unsigned)n), dim3(WAVE), 0, st, s->view(), n, (u32)seed,
                           (u32)(seed >> 32), step, (u32)first_game, (u32)n_games, value_blend, out->features, out->policy,
                           out->value, draws_out, s->d_errors.d,
                           Aux{s->d_owners.d, out->ownership, out->score, out->reply, out->aux_weight});
    else
        hipLaunchKernelGGL(k_samples_draw_gather, dim3((unsigned)n), dim3(WAVE), 0, st, s->view(), n, (u32)seed,
                           (u32)(seed >> 32), step, (u32)first_game, (u32)n_games, value_blend, out->features, out->policy,
                           out->value, draws_out, s->d_errors.d);
    AZH_HIP(hipGetLastError());
    if (!stream)
        AZH_HIP(hipStreamSynchronize(st));
    return 0;
}

// One sample's draw restated on the host from mirror arrays: arithmetic only, no device and no store.
// cum == null: the uniform ply draw, the candidates found from the flags; else the weighted one from the mirrors of the
// store's candidates and cum arrays (azh_samples_ply_cum).
extern "C" int azh_samples_draw(uint64_t seed, uint32_t step, uint32_t sample, int64_t first_game, int64_t n_games,
                                const uint32_t *games, int64_t total_games, const uint8_t *ply_flags, const uint16_t *candidates,
                                const uint32_t *cum, int32_t *out)
{
    if (!games || !ply_flags || !out || (candidates != nullptr) != (cum != nullptr))
        return azh_fail(-1, "azh_samples_draw: null argument (candidates and cum go together)");
    if (first_game < 0 || n_games < 1 || first_game + n_games > total_games || total_games > 0x7FFFFFFF)
        return azh_fail(-1, "azh_samples_draw: games [%lld, %lld) of %lld", (long long)first_game,
                        (long long)(first_game + n_games), (long long)total_games);
    auto game_at = [&](int g) { return make_uint4(games[4 * g], games[4 * g + 1], games[4 * g + 2], games[4 * g + 3]); };
    auto candidate = [&](int g, uint32_t flag) {  // plies a sample may come from: all, or the full ones of a game with "full"
        return !(games[4 * g + 2] & GAME_HAS_FULL) || (flag & AZH_SAMPLES_PLY_FULL);
    };
    out[0] = out[1] = out[2] = -1;
    out[3] = MAX_ATTEMPTS;
    for (uint32_t a = 0; a < (uint32_t)MAX_ATTEMPTS; a++) {
        int drawn = -1;
        const Attempt t = draw_attempt(
            (u32)seed, (u32)(seed >> 32), step, sample, a, (u32)first_game, (u32)n_games, game_at,
            [&](int g) {
                drawn = g;
                u32 c = 0;
                for (uint32_t p = 0; p < games[4 * g + 1]; p++)
                    c += candidate(g, ply_flags[games[4 * g] + p]);
                return c;
            },
            [&](u32 at) {  // the k-th candidate of the drawn game, k = at - first ply
                if (candidates)
                    return (u32)candidates[at];
                u32 k = at - games[4 * drawn];
                for (uint32_t p = 0; p < games[4 * drawn + 1]; p++)
                    if (candidate(drawn, ply_flags[games[4 * drawn] + p]) && k-- == 0)
                        return p;
                return 0u;
            },
            [&](u32 at) { return (u32)ply_flags[at]; }, cum != nullptr, [&](u32 at) { return cum[at]; });
        if (t.ok) {
            out[0] = t.game;
            out[1] = t.ply;
            out[2] = t.symmetry;
            out[3] = (int32_t)a + 1;
            break;
        }
    }
    return 0;
}

extern "C" int azh_samples_status(azh_samples *s, int64_t *failed)
{
    if (!s || !failed)
        return azh_fail(-1, "azh_samples_status: null argument");
    u32 n = 0;  // (a blocking copy from the null stream: it waits for the kernels enqueued so far on every blocking stream)
    AZH_HIP(hipDeviceSynchronize());
    AZH_HIP(hipMemcpy(&n, s->d_errors.d, sizeof(u32), hipMemcpyDeviceToHost));
    *failed = (int64_t)n;
    return 0;
}

// ---------------------------------------------------------------- policy surprise weighting: entry points

static int reserve_surprise(azh_samples *s)
{
    if (!s->d_kl.d) {
        if (int rc = s->d_kl.alloc((size_t)s->cap_plies))
            return rc;
        AZH_HIP(hipMemset(s->d_kl.d, 0, (size_t)s->cap_plies * sizeof(float)));
    }
    if (!s->d_illegal.d)
        if (int rc = s->d_illegal.alloc(1))
            return rc;
    return 0;
}

namespace {
struct MaskRun {  // plies [first, end) of consecutive games that share one wall mask
    int64_t first, end;
    u64 blockers;
};
}  // namespace

// The stored plies [first, end) cut where the wall mask of their games changes: no launch of the tower or of the surprise kernel
// spans two masks.  From the host mirror.
static std::vector<MaskRun> mask_runs(const azh_samples *s, int64_t first, int64_t end)
{
    std::vector<MaskRun> runs;
    int64_t lo = 0, hi = s->games - 1;  // the game that holds ply `first`: the last one whose first ply is <= first
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)s->h_games[4 * mid] <= first)
            lo = mid;
        else
            hi = mid - 1;
    }
    for (int64_t g = lo; g < s->games && (int64_t)s->h_games[4 * g] < end; g++) {
        const int64_t a = std::max<int64_t>(first, s->h_games[4 * g]);
        const int64_t b = std::min<int64_t>(end, (int64_t)s->h_games[4 * g] + s->h_games[4 * g + 1]);
        const u64 mask = s->h_blockers[(size_t)g];
        if (!runs.empty() && runs.back().blockers == mask)
            runs.back().end = b;
        else
            runs.push_back(MaskRun{a, b, mask});
    }
    return runs;
}

extern "C" int azh_samples_surprise_logits(azh_samples *s, int64_t first_ply, int64_t n_plies, const float *d_logits,
                                           float *kl_out, int64_t *illegal_out, uintptr_t stream)
{
    if (!s || !d_logits || !kl_out || !illegal_out)
        return azh_fail(-1, "azh_samples_surprise_logits: null argument");
    if (first_ply < 0 || n_plies < 1 || first_ply + n_plies > s->plies)
        return azh_fail(-1, "azh_samples_surprise_logits: plies [%lld, %lld) of %lld", (long long)first_ply,
                        (long long)(first_ply + n_plies), (long long)s->plies);
    if (int rc = reserve_surprise(s))
        return rc;
    hipStream_t st = stream ? (hipStream_t)stream : s->stream;
    AZH_HIP(hipMemsetAsync(s->d_illegal.d, 0, sizeof(u32), st));
    for (const MaskRun &run : mask_runs(s, first_ply, first_ply + n_plies)) {
        hipLaunchKernelGGL(k_samples_surprise, dim3((unsigned)(run.end - run.first)), dim3(WAVE), 0, st, s->view(),
                           (u32)run.first, (int)(run.end - run.first), d_logits + (size_t)(run.first - first_ply) * POLICY,
                           s->d_kl.d, s->d_illegal.d, run.blockers);
        AZH_HIP(hipGetLastError());
    }
    u32 missing = 0;
    AZH_HIP(hipMemcpyAsync(kl_out, s->d_kl.d + first_ply, (size_t)n_plies * sizeof(float), hipMemcpyDeviceToHost, st));
    AZH_HIP(hipMemcpyAsync(&missing, s->d_illegal.d, sizeof(u32), hipMemcpyDeviceToHost, st));
    AZH_HIP(hipStreamSynchronize(st));
    *illegal_out = (int64_t)missing;
    return 0;
}

extern "C" int azh_samples_set_surprise_chunk(azh_samples *s, int plies)
{
    if (!s || plies < 0 || plies > SURPRISE_CHUNK)
        return azh_fail(-1, "azh_samples_set_surprise_chunk: 0 .. %d plies", SURPRISE_CHUNK);
    s->surprise_chunk = plies ? plies : SURPRISE_CHUNK;
    return 0;
}

extern "C" int azh_samples_surprise_ms(const azh_samples *s, float *ms)
{
    if (!s || !ms)
        return azh_fail(-1, "azh_samples_surprise_ms: null argument");
    ms[0] = s->surprise_ms[0];
    ms[1] = s->surprise_ms[1];
    return 0;
}

namespace {
struct SurpriseScratch {  // freed on every path out of azh_samples_surprise
    u64 *boards = nullptr;
    float *logits = nullptr, *values = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ~SurpriseScratch()
    {
        (void)hipFree(boards);
        (void)hipFree(logits);
        (void)hipFree(values);
        for (hipEvent_t e : ev)
            if (e)
                (void)hipEventDestroy(e);
    }
};
}  // namespace

extern "C" int azh_samples_surprise(azh_samples *s, azh_net *net, int dtype, int64_t first_game, int64_t n_games, float *kl_out,
                                    int64_t *illegal_out)
{
    if (!s || !net || !kl_out || !illegal_out)
        return azh_fail(-1, "azh_samples_surprise: null argument");
    if (first_game < 0 || n_games < 1 || first_game + n_games > s->games)
        return azh_fail(-1, "azh_samples_surprise: games [%lld, %lld) of %lld", (long long)first_game,
                        (long long)(first_game + n_games), (long long)s->games);
    if (int rc = reserve_surprise(s))
        return rc;
    const int64_t first = s->h_games[4 * first_game];
    const int64_t end = (int64_t)s->h_games[4 * (first_game + n_games - 1)] + s->h_games[4 * (first_game + n_games - 1) + 1];
    const int chunk = (int)std::min<int64_t>(s->surprise_chunk, end - first);
    SurpriseScratch sc;
    AZH_HIP(hipMalloc((void **)&sc.boards, (size_t)chunk * 2 * sizeof(u64)));
    AZH_HIP(hipMalloc((void **)&sc.logits, (size_t)chunk * POLICY * sizeof(float)));
    AZH_HIP(hipMalloc((void **)&sc.values, (size_t)chunk * sizeof(float)));
    for (hipEvent_t &e : sc.ev)
        AZH_HIP(hipEventCreate(&e));
    hipStream_t st = s->stream;
    AZH_HIP(hipMemsetAsync(s->d_illegal.d, 0, sizeof(u32), st));
    s->surprise_ms[0] = s->surprise_ms[1] = 0.f;
    // (each chunk is waited for before the next reuses the scratch and the events: the tower's time dwarfs the wait)
    // (a chunk never spans two wall masks: the tower takes one blocker plane per launch, the kernel one mask)
    std::vector<MaskRun> chunks;  // cut at mask changes as well as at `chunk` plies
    for (const MaskRun &r : mask_runs(s, first, end))
        for (int64_t at = r.first; at < r.end; at += chunk)
            chunks.push_back(MaskRun{at, std::min<int64_t>(at + chunk, r.end), r.blockers});
    for (const MaskRun &run : chunks) {
        const int64_t at = run.first;
        const int n = (int)(run.end - run.first);
        AZH_HIP(hipEventRecord(sc.ev[0], st));
        hipLaunchKernelGGL(k_samples_pack_boards, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->view(), (u32)at, n,
                           sc.boards);
        AZH_HIP(hipGetLastError());
        azh::NetBatch batch;
        batch.boards = sc.boards;
        batch.max_n = n;
        batch.blockers = run.blockers;
        batch.logits = sc.logits;
        batch.values = sc.values;
        if (int rc = azh_net_launch(net, dtype, batch, st))
            return rc;
        AZH_HIP(hipEventRecord(sc.ev[1], st));
        hipLaunchKernelGGL(k_samples_surprise, dim3((unsigned)n), dim3(WAVE), 0, st, s->view(), (u32)at, n, sc.logits,
                           s->d_kl.d, s->d_illegal.d, run.blockers);
        AZH_HIP(hipGetLastError());
        AZH_HIP(hipEventRecord(sc.ev[2], st));
        AZH_HIP(hipStreamSynchronize(st));
        float tower = 0.f, kernel = 0.f;
        AZH_HIP(hipEventElapsedTime(&tower, sc.ev[0], sc.ev[1]));
        AZH_HIP(hipEventElapsedTime(&kernel, sc.ev[1], sc.ev[2]));
        s->surprise_ms[0] += tower;
        s->surprise_ms[1] += kernel;
    }
    u32 missing = 0;
    AZH_HIP(hipMemcpy(kl_out, s->d_kl.d + first, (size_t)(end - first) * sizeof(float), hipMemcpyDeviceToHost));
    AZH_HIP(hipMemcpy(&missing, s->d_illegal.d, sizeof(u32), hipMemcpyDeviceToHost));
    *illegal_out = (int64_t)missing;
    return 0;
}

extern "C" int azh_samples_legal(uint64_t mover, uint64_t opponent, uint64_t blockers, uint16_t *index_out, int32_t *n_out)
{
    if (!index_out || !n_out)
        return azh_fail(-1, "azh_samples_legal: null argument");
    mover &= BOARD_MASK;
    opponent &= BOARD_MASK;
    const u64 empty = BOARD_MASK & ~(mover | opponent | blockers);
    int n = 0;
    for (int from = 0; from < 49; from++)  // wave_movegen's order: jumps by ascending (from, to), then clones ascending
        if ((mover >> from) & 1ULL)
            for (u64 to = double_jump_bb(1ULL << from) & empty; to; to &= to - 1ULL)
                index_out[n++] = (uint16_t)policy_index((u32)from | ((u32)__builtin_ctzll(to) << 8));
    for (u64 to = single_jump_bb(mover) & empty; to; to &= to - 1ULL) {
        const u32 sq = (u32)__builtin_ctzll(to);
        index_out[n++] = (uint16_t)policy_index(sq | (sq << 8));
    }
    *n_out = n;
    return 0;
}

extern "C" int azh_samples_surprise_host(const float *logits833, const uint16_t *legal_index, int n_legal,
                                         const uint16_t *target_index, const float *target_weight, int n_targets, float *kl_out,
                                         int32_t *illegal_out)
{
    if (!logits833 || !kl_out || n_legal < 0 || n_targets < 0 || (n_legal && !legal_index) ||
        (n_targets && (!target_index || !target_weight)))
        return azh_fail(-1, "azh_samples_surprise_host: bad argument");
    std::vector<uint8_t> legal(POLICY, 0);
    std::vector<float> term((size_t)std::max(n_legal, n_targets) + 1);
    float mx = -INFINITY;
    for (int j = 0; j < n_legal; j++) {
        if (legal_index[j] >= POLICY)
            return azh_fail(-1, "azh_samples_surprise_host: policy index %u", (unsigned)legal_index[j]);
        legal[legal_index[j]] = 1;
        const float l = logits833[legal_index[j]];
        if (l > mx)
            mx = l;
    }
    for (int j = 0; j < n_legal; j++)
        term[(size_t)j] = det_expf(logits833[legal_index[j]] - mx);
    const float log_s = det_logf(gumbel_lane_sum(term.data(), n_legal));
    int32_t missing = 0;
    for (int t = 0; t < n_targets; t++) {
        term[(size_t)t] = 0.0f;
        if (target_index[t] >= POLICY)
            return azh_fail(-1, "azh_samples_surprise_host: policy index %u", (unsigned)target_index[t]);
        if (!(target_weight[t] > 0.0f))
            continue;
        if (legal[target_index[t]])
            term[(size_t)t] = surprise_term(target_weight[t], (logits833[target_index[t]] - mx) - log_s);
        else
            missing++;
    }
    *kl_out = stored_surprise(gumbel_lane_sum(term.data(), n_targets));
    if (illegal_out)
        *illegal_out = missing;
    return 0;
}

extern "C" int azh_samples_surprise_host_blockers(const float *logits833, uint64_t mover, uint64_t opponent, uint64_t blockers,
                                                  const uint16_t *target_index, const float *target_weight, int n_targets,
                                                  float *kl_out, int32_t *illegal_out)
{
    uint16_t legal[POLICY];
    int32_t n_legal = 0;
    if (int rc = azh_samples_legal(mover, opponent, blockers, legal, &n_legal))
        return rc;
    return azh_samples_surprise_host(logits833, legal, n_legal, target_index, target_weight, n_targets, kl_out, illegal_out);
}

static void default_cum(const azh_samples *s, int64_t game, u32 *cum)  // cum: the store's whole array
{
    const u32 first = s->h_games[4 * game];
    for (u32 k = 0; k < s->h_count[(size_t)game]; k++)
        cum[first + k] = WEIGHT_ONE * (k + 1u);
}

extern "C" int azh_samples_set_ply_weights(azh_samples *s, int64_t first_game, int64_t n_games, const float *w)
{
    if (!s || !w)
        return azh_fail(-1, "azh_samples_set_ply_weights: null argument");
    if (first_game < 0 || n_games < 1 || first_game + n_games > s->games)
        return azh_fail(-1, "azh_samples_set_ply_weights: games [%lld, %lld) of %lld", (long long)first_game,
                        (long long)(first_game + n_games), (long long)s->games);
    // everything is checked and built on the host first: a refused call leaves the store exactly as it was
    std::vector<u32> cum(s->h_cum);
    if (cum.empty()) {
        cum.assign((size_t)s->plies, 0u);
        for (int64_t g = 0; g < s->games; g++)
            default_cum(s, g, cum.data());
    }
    const int64_t base = s->h_games[4 * first_game];
    for (int64_t g = first_game; g < first_game + n_games; g++) {
        const u32 first = s->h_games[4 * g], plies = s->h_games[4 * g + 1];
        for (u32 p = 0; p < plies; p++) {
            const float x = w[first - base + p];
            if (!(x >= 0.0f && x <= 3.40282347e38f))
                return azh_fail(-1, "azh_samples_set_ply_weights: game %lld, ply %u: a weight must be finite and >= 0",
                                (long long)g, p);
        }
        double total = 0.0;  // (sums of integers below 2^53: exact)
        for (u32 k = 0; k < s->h_count[(size_t)g]; k++) {
            const double q = floor((double)w[first - base + s->h_candidates[first + k]] * 65536.0 + 0.5);
            total = q > 4294967295.0 ? 4294967296.0 : total + q;
            if (total > 4294967295.0)
                return azh_fail(-1, "azh_samples_set_ply_weights: game %lld: the weights add up to more than 2^32 - 1 units "
                                    "of 1 / 65536", (long long)g);
            cum[first + k] = (u32)total;
        }
    }
    AZH_HIP(hipDeviceSynchronize());
    if (!s->d_cum.d)
        if (int rc = s->d_cum.alloc((size_t)s->cap_plies))
            return rc;
    const hipError_t e = cum.empty() ? hipSuccess : hipMemcpy(s->d_cum.d, cum.data(), cum.size() * sizeof(u32), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (s->h_cum.empty())
            s->d_cum.release();
        return azh_fail(-100 - (int)e, "azh_samples_set_ply_weights: %s", hipGetErrorString(e));
    }
    s->h_cum.swap(cum);
    return 0;
}

extern "C" int azh_samples_clear_ply_weights(azh_samples *s)
{
    if (!s)
        return azh_fail(-1, "azh_samples_clear_ply_weights: null store");
    AZH_HIP(hipDeviceSynchronize());
    s->d_cum.release();
    s->h_cum.clear();
    return 0;
}

extern "C" int azh_samples_ply_cum(const azh_samples *s, uint16_t *candidates, uint32_t *candidate_count, uint32_t *cum,
                                   int32_t *present)
{
    if (!s || !candidates || !candidate_count || !cum || !present)
        return azh_fail(-1, "azh_samples_ply_cum: null argument");
    if (s->plies)
        memcpy(candidates, s->h_candidates.data(), (size_t)s->plies * sizeof(u16));
    if (s->games)
        memcpy(candidate_count, s->h_count.data(), (size_t)s->games * sizeof(u32));
    *present = s->d_cum.d != nullptr;
    if (*present) {
        memcpy(cum, s->h_cum.data(), (size_t)s->plies * sizeof(u32));
    } else {
        memset(cum, 0, (size_t)s->plies * sizeof(u32));
        for (int64_t g = 0; g < s->games; g++)
            default_cum(s, g, cum);
    }
    return 0;
}

// ---------------------------------------------------------------- reanalysis of stored plies (include/ataxxzero_hip.h)

namespace {

constexpr int REPORT_WORDS = AZH_ROOT_REPORT_WORDS;
constexpr int SCAN_BLOCK = 256;

// One edge of a root report.  Records are AZH_ROOT_REPORT_WORDS words apart, so an edge is aligned to its words only: the
// 16-byte load is one that needs no more (global memory takes a dwordx4 load at any word address).
struct ReportEdge {
    u32 move, visits, w, prior;
};

// The definition's move test: a clone, or a jump over a distance of exactly two, between two of the 49 cells.
__host__ __device__ inline bool report_move(u32 mv)
{
    if (mv > 0xFFFFu)
        return false;
    const int from = (int)(mv & 0xFFu), to = (int)(mv >> 8);
    if (from >= 49 || to >= 49)
        return false;
    int dx = to % 7 - from % 7, dy = to / 7 - from / 7;
    dx = dx < 0 ? -dx : dx;
    dy = dy < 0 ? -dy : dy;
    return from == to || (dx > dy ? dx : dy) == 2;
}

__host__ __device__ inline double report_value(float w, u32 visits)
{
    const float q = w / (float)visits;  // (one IEEE division on both sides: no fast-math, no contraction)
    return (f2u(q) & 0x7F800000u) != 0x7F800000u ? 2.0 * (double)q - 1.0 : 0.0;
}

// The edges j = lane + 64 k, k < 4, of a record in this lane's registers; zero beyond M.
struct LaneEdges {
    ReportEdge e[4];
};
__device__ __forceinline__ LaneEdges load_edges(const u32 *rec, int M, int lane)
{
    LaneEdges L;
    const ReportEdge *edges = reinterpret_cast<const ReportEdge *>(rec + 4);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = lane + 64 * k;
        L.e[k] = j < M ? edges[j] : ReportEdge{0u, 0u, 0u, 0u};
    }
    return L;
}

// Phase 1: record i -> counts[i] = its new targets (0: unchanged), bad[i] = 1 for a malformed record.
__global__ __launch_bounds__(WAVE) void k_retarget_count(const u32 *__restrict__ reports, int n, u32 *__restrict__ counts,
                                                         u32 *__restrict__ bad)
{
    const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (i >= n)
        return;
    const u32 *rec = reports + (size_t)i * REPORT_WORDS;
    const u32 M = rec[1], finished = rec[3];
    bool malformed = M > (u32)AZH_MAX_MOVES;
    u32 count = 0;
    if (!malformed) {  // (wave-uniform)
        const LaneEdges L = load_edges(rec, (int)M, lane);
        bool wrong = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool visited = L.e[k].visits > 0u;
            wrong = wrong || (visited && !report_move(L.e[k].move));
            count += (u32)__popcll(__ballot(visited));
        }
        malformed = __ballot(wrong) != 0ULL;
    }
    if (lane == 0) {
        counts[i] = malformed || finished ? 0u : count;
        bad[i] = malformed ? 1u : 0u;
    }
}

__device__ __forceinline__ u64 block_sum_u64(u64 v, u64 *lds)  // SCAN_BLOCK threads; the sum in every thread
{
    const int t = (int)threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int step = SCAN_BLOCK / 2; step > 0; step >>= 1) {
        if (t < step)
            lds[t] += lds[t + step];
        __syncthreads();
    }
    const u64 out = lds[0];
    __syncthreads();
    return out;
}

// The scan's first pass: sums[2 b] = the counts of block b's SCAN_BLOCK records, sums[2 b + 1] = its malformed records.
__global__ __launch_bounds__(SCAN_BLOCK) void k_retarget_block_sums(const u32 *__restrict__ counts, const u32 *__restrict__ bad,
                                                                    int n, u64 *__restrict__ sums)
{
    __shared__ u64 lds[SCAN_BLOCK];
    const int i = (int)(blockIdx.x * SCAN_BLOCK + threadIdx.x);
    const u64 c = block_sum_u64(i < n ? counts[i] : 0u, lds);
    const u64 b = block_sum_u64(i < n ? bad[i] : 0u, lds);
    if (threadIdx.x == 0) {
        sums[2 * blockIdx.x] = c;
        sums[2 * blockIdx.x + 1] = b;
    }
}

// The second: offsets[i] = the counts of the records before i (exclusive, call order); the last block leaves the total and
// the number of malformed records in totals[0 .. 1].
__global__ __launch_bounds__(SCAN_BLOCK) void k_retarget_scan(const u32 *__restrict__ counts, int n, const u64 *__restrict__ sums,
                                                              u32 *__restrict__ offsets, u64 *__restrict__ totals)
{
    __shared__ u64 lds[SCAN_BLOCK];
    __shared__ u32 wave_total[SCAN_BLOCK / WAVE];
    const int t = (int)threadIdx.x, b = (int)blockIdx.x, i = b * SCAN_BLOCK + t;
    u64 before = 0, malformed = 0;
    for (int k = t; k < b; k += SCAN_BLOCK)
        before += sums[2 * k];
    before = block_sum_u64(before, lds);
    const u32 mine = i < n ? counts[i] : 0u;
    const u32 incl = (u32)wave_incl_scan((int)mine);
    if ((t & 63) == 63)
        wave_total[t >> 6] = incl;
    __syncthreads();
    u32 waves_before = 0;
    for (int w = 0; w < (t >> 6); w++)
        waves_before += wave_total[w];
    if (i < n)
        offsets[i] = (u32)before + waves_before + incl - mine;
    if (b == (int)gridDim.x - 1) {  // (block-uniform)
        for (int k = t; k < (int)gridDim.x; k += SCAN_BLOCK)
            malformed += sums[2 * k + 1];
        malformed = block_sum_u64(malformed, lds);
        if (t == 0) {
            totals[0] = before + sums[2 * b];
            totals[1] = malformed;
        }
    }
}

// The sum of one u64 per lane whose value is below 2^48, exactly: three 16-bit columns, each below 2^22 over the wave.
__device__ __forceinline__ u64 wave_sum_u48(u64 v)
{
    const u64 a = wave_sum_u32((u32)(v & 0xFFFFu)), b = wave_sum_u32((u32)((v >> 16) & 0xFFFFu)),
              c = wave_sum_u32((u32)((v >> 32) & 0xFFFFu));
    return a + (b << 16) + (c << 32);
}

// Phase 2: record i -> ply ply_at[i]: the visited edges compacted in edge order behind base + offsets[i], the value, and the
// ply's two target words.  Phase 1 has found every record well formed and the host has found the room.
__global__ __launch_bounds__(WAVE) void k_retarget_write(const u32 *__restrict__ reports, int n, const u32 *__restrict__ ply_at,
                                                         const u32 *__restrict__ offsets, u32 base, Ply *__restrict__ plies,
                                                         u16 *__restrict__ target_index, float *__restrict__ target_weight,
                                                         int *__restrict__ status)
{
    const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (i >= n)
        return;
    const u32 *rec = reports + (size_t)i * REPORT_WORDS;
    const int M = (int)min(rec[1], (u32)AZH_MAX_MOVES);
    const LaneEdges L = load_edges(rec, M, lane);
    u64 part = 0, key = 0;
    u32 best_w = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        part += L.e[k].visits;
        const u64 kj = ((u64)L.e[k].visits << 32) | (u64)(0xFFFFFFFFu - (u32)(lane + 64 * k));  // most visits, first on a tie
        if (kj > key) {
            key = kj;
            best_w = L.e[k].w;
        }
    }
    const u64 total = wave_sum_u48(part);
    const bool changed = total != 0ULL && rec[3] == 0u;  // (wave-uniform)
    if (changed) {
        key = wave_max_u64(key);
        const int bj = (int)(0xFFFFFFFFu - (u32)key);
        const u32 w_bits = (u32)read_lane((int)best_w, bj & 63);
        const u32 first = base + offsets[i];
        u32 at = first;
        const u64 below = (1ULL << lane) - 1ULL;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool visited = L.e[k].visits > 0u;
            const u64 mask = __ballot(visited);
            if (visited) {
                const u32 to = at + (u32)__popcll(mask & below);
                target_index[to] = (u16)policy_index(L.e[k].move);
                target_weight[to] = (float)((double)L.e[k].visits / (double)total);
            }
            at += (u32)__popcll(mask);
        }
        if (lane == 0) {
            Ply *ply = plies + ply_at[i];
            ply->value = report_value(u2f(w_bits), (u32)(key >> 32));
            ply->first_target = first;
            ply->targets_flags = (at - first) << 8 | (ply->targets_flags & 0xFFu);
        }
    }
    if (lane == 0)
        status[i] = changed ? 1 : 0;
}

// azh_samples_read_plies: ply ply_at[i] as it is stored.  (k_samples_pack_boards serves a run of consecutive plies in the
// tower's (mover, opponent) order; a scattered list in (x, o) order with the value and the target words is another kernel, not
// a branch in that one.)
__global__ __launch_bounds__(256) void k_samples_read_plies(View v, int n, const u32 *__restrict__ ply_at, Ply *__restrict__ out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n)
        out[i] = v.plies[ply_at[i]];
}

// One wave per ply: its targets, in stored order, to start[i] of the packed arrays.
__global__ __launch_bounds__(WAVE) void k_samples_read_targets(View v, int n, const u32 *__restrict__ ply_at,
                                                               const u32 *__restrict__ start, u16 *__restrict__ index,
                                                               float *__restrict__ weight)
{
    const int i = (int)blockIdx.x;
    if (i >= n)
        return;
    const Ply ply = v.plies[ply_at[i]];
    const u32 count = ply.targets_flags >> 8;
    for (u32 t = threadIdx.x; t < count; t += WAVE) {
        index[start[i] + t] = v.target_index[ply.first_target + t];
        weight[start[i] + t] = v.target_weight[ply.first_target + t];
    }
}

size_t round_up(size_t bytes) { return (bytes + 255) / 256 * 256; }

}  // namespace

// Device scratch of the two calls below, kept from call to call and grown on demand.
static int reserve_scratch(azh_samples *s, size_t bytes)
{
    if (bytes <= s->scratch_bytes)
        return 0;
    s->d_scratch.release();
    s->scratch_bytes = 0;
    if (int rc = s->d_scratch.alloc(bytes))
        return rc;
    s->scratch_bytes = bytes;
    return 0;
}

// (game, ply) pairs -> the plies' places in the store, from the mirror: -1 for a pair outside it.
static int ply_places(const azh_samples *s, const char *what, int n, const int32_t *plies, std::vector<u32> &at)
{
    at.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        const int64_t g = plies[2 * i], p = plies[2 * i + 1];
        if (g < 0 || g >= s->games || p < 0 || p >= (int64_t)s->h_games[4 * g + 1])
            return azh_fail(-1, "%s: pair %d (game %lld, ply %lld) is outside the store", what, i, (long long)g, (long long)p);
        at[(size_t)i] = s->h_games[4 * g] + (u32)p;
    }
    return 0;
}

// The plies at `at` as the device holds them -> got; waits for the store's stream.
static int fetch_plies(azh_samples *s, const std::vector<u32> &at, std::vector<Ply> &got)
{
    const size_t N = at.size(), at_bytes = round_up(N * sizeof(u32)), ply_bytes = round_up(N * sizeof(Ply));
    if (int rc = reserve_scratch(s, at_bytes + ply_bytes))
        return rc;
    u32 *d_at = reinterpret_cast<u32 *>(s->d_scratch.d);
    Ply *d_out = reinterpret_cast<Ply *>(s->d_scratch.d + at_bytes);
    got.resize(N);
    AZH_HIP(hipMemcpyAsync(d_at, at.data(), N * sizeof(u32), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_samples_read_plies, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, s->view(), (int)N, d_at,
                       d_out);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipMemcpyAsync(got.data(), d_out, N * sizeof(Ply), hipMemcpyDeviceToHost, s->stream));
    AZH_HIP(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int azh_samples_ply_targets(azh_samples *s, int n, const int32_t *plies, uint32_t *out)
{
    if (!s || !plies || !out || n < 1)
        return azh_fail(-1, "azh_samples_ply_targets: bad argument");
    std::vector<u32> at;
    if (int rc = ply_places(s, "azh_samples_ply_targets", n, plies, at))
        return rc;
    std::vector<Ply> got;
    if (int rc = fetch_plies(s, at, got))
        return rc;
    for (size_t i = 0; i < got.size(); i++) {
        out[2 * i] = got[i].first_target;
        out[2 * i + 1] = got[i].targets_flags >> 8;
    }
    return 0;
}

extern "C" int azh_samples_read_plies(azh_samples *s, int n, const int32_t *plies, uint64_t *boards_out, double *values_out,
                                      uint8_t *flags_out, int32_t *target_start_out, uint16_t *index_out, float *weight_out,
                                      int64_t cap_targets)
{
    if (!s || !plies || !boards_out || !values_out || !flags_out || !target_start_out || n < 1 ||
        (index_out != nullptr) != (weight_out != nullptr))
        return azh_fail(-1, "azh_samples_read_plies: bad argument (n >= 1; index_out and weight_out go together)");
    std::vector<u32> at;
    if (int rc = ply_places(s, "azh_samples_read_plies", n, plies, at))
        return rc;
    std::vector<Ply> got;
    if (int rc = fetch_plies(s, at, got))
        return rc;
    const size_t N = (size_t)n, at_bytes = round_up(N * sizeof(u32));
    std::vector<u32> start(N + 1, 0u);
    int64_t total = 0;
    target_start_out[0] = 0;
    for (size_t i = 0; i < N; i++) {
        boards_out[2 * i] = got[i].x;
        boards_out[2 * i + 1] = got[i].o;
        values_out[i] = got[i].value;
        flags_out[i] = (uint8_t)(got[i].targets_flags & (AZH_SAMPLES_PLY_PASS | AZH_SAMPLES_PLY_FULL | AZH_SAMPLES_PLY_BAD));
        total += got[i].targets_flags >> 8;
        if (total > 0x7FFFFFFF)
            return azh_fail(-6, "azh_samples_read_plies: the plies hold more than 2^31 - 1 targets");
        start[i + 1] = (u32)total;
        target_start_out[i + 1] = (int32_t)total;
    }
    if (!index_out || total == 0)
        return 0;
    if (total > cap_targets)
        return azh_fail(-6, "azh_samples_read_plies: the plies hold %lld targets, the arrays %lld", (long long)total,
                        (long long)cap_targets);
    const size_t T = (size_t)total, start_bytes = round_up((N + 1) * sizeof(u32)), weight_bytes = round_up(T * sizeof(float));
    if (int rc = reserve_scratch(s, at_bytes + start_bytes + weight_bytes + round_up(T * sizeof(u16))))
        return rc;
    u32 *d_at = reinterpret_cast<u32 *>(s->d_scratch.d);
    u32 *d_start = reinterpret_cast<u32 *>(s->d_scratch.d + at_bytes);
    float *d_weight = reinterpret_cast<float *>(s->d_scratch.d + at_bytes + start_bytes);
    u16 *d_index = reinterpret_cast<u16 *>(s->d_scratch.d + at_bytes + start_bytes + weight_bytes);
    AZH_HIP(hipMemcpyAsync(d_at, at.data(), N * sizeof(u32), hipMemcpyHostToDevice, s->stream));
    AZH_HIP(hipMemcpyAsync(d_start, start.data(), (N + 1) * sizeof(u32), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_samples_read_targets, dim3((unsigned)n), dim3(WAVE), 0, s->stream, s->view(), n, d_at, d_start, d_index,
                       d_weight);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipMemcpyAsync(index_out, d_index, T * sizeof(u16), hipMemcpyDeviceToHost, s->stream));
    AZH_HIP(hipMemcpyAsync(weight_out, d_weight, T * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    AZH_HIP(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int azh_samples_retarget_host(const uint32_t *report, uint16_t *index_out, float *weight_out, int32_t *n_out,
                                         double *value_out)
{
    if (!report || !index_out || !weight_out || !n_out || !value_out)
        return azh_fail(-1, "azh_samples_retarget_host: null argument");
    *n_out = 0;
    *value_out = 0.0;
    const uint32_t M = report[1];
    if (M > (uint32_t)AZH_MAX_MOVES)
        return azh_fail(-2, "azh_samples_retarget_host: a root of %u edges", (unsigned)M);
    uint64_t total = 0;
    uint32_t best = 0, best_visits = 0;
    for (uint32_t j = 0; j < M; j++) {
        const uint32_t *e = report + 4 + 4 * j;
        if (e[1] > 0u && !report_move(e[0]))
            return azh_fail(-2, "azh_samples_retarget_host: edge %u: move %#x is no clone and no jump", (unsigned)j, (unsigned)e[0]);
        total += e[1];
        if (e[1] > best_visits) {  // (the first in edge order on a tie)
            best_visits = e[1];
            best = j;
        }
    }
    if (total == 0 || report[3] != 0u)
        return 0;
    int32_t n = 0;
    for (uint32_t j = 0; j < M; j++) {
        const uint32_t *e = report + 4 + 4 * j;
        if (e[1] > 0u) {
            index_out[n] = (uint16_t)policy_index(e[0]);
            weight_out[n] = (float)((double)e[1] / (double)total);
            n++;
        }
    }
    *n_out = n;
    *value_out = report_value(u2f(report[6 + 4 * best]), best_visits);
    return 0;
}

extern "C" int azh_samples_retarget(azh_samples *s, int n, const int32_t *plies, const uint32_t *d_reports,
                                    uint64_t report_blockers, int32_t *status_out, uintptr_t stream)
{
    if (!s || !plies || !d_reports || !status_out || n < 1)
        return azh_fail(-1, "azh_samples_retarget: bad argument");
    // everything the mirror can tell is checked first: a refused call launches nothing
    std::vector<u32> at;
    if (int rc = ply_places(s, "azh_samples_retarget", n, plies, at))
        return rc;
    for (int i = 0; i < n; i++) {
        const int64_t g = plies[2 * i];
        const uint8_t f = s->h_flags[at[(size_t)i]];
        if (f & AZH_SAMPLES_PLY_PASS)
            return azh_fail(-1, "azh_samples_retarget: pair %d (game %lld, ply %d) is a pass", i, (long long)g, plies[2 * i + 1]);
        if ((s->h_games[4 * g + 2] & GAME_HAS_FULL) && !(f & AZH_SAMPLES_PLY_FULL))
            return azh_fail(-1, "azh_samples_retarget: pair %d (game %lld, ply %d) is not among its game's candidates", i,
                            (long long)g, plies[2 * i + 1]);
        if (f & AZH_SAMPLES_PLY_BAD)
            return azh_fail(-2, "azh_samples_retarget: pair %d (game %lld, ply %d): policy target does not sum to one", i,
                            (long long)g, plies[2 * i + 1]);
        if (s->h_blockers[(size_t)g] != report_blockers)
            return azh_fail(-2, "azh_samples_retarget: pair %d: game %lld is stored with walls %#llx, the reports were searched "
                                "on %#llx", i, (long long)g, (unsigned long long)s->h_blockers[(size_t)g],
                            (unsigned long long)report_blockers);
    }
    {
        std::vector<u32> sorted(at);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return azh_fail(-1, "azh_samples_retarget: a pair is given twice");
    }
    const size_t N = (size_t)n, blocks = (N + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const size_t sums_bytes = round_up((2 * blocks + 2) * sizeof(u64)), row_bytes = round_up(N * sizeof(u32));
    if (int rc = reserve_scratch(s, sums_bytes + 5 * row_bytes))
        return rc;
    u64 *d_sums = reinterpret_cast<u64 *>(s->d_scratch.d), *d_totals = d_sums + 2 * blocks;
    u32 *d_at = reinterpret_cast<u32 *>(s->d_scratch.d + sums_bytes);
    u32 *d_counts = d_at + row_bytes / 4, *d_bad = d_counts + row_bytes / 4, *d_offsets = d_bad + row_bytes / 4;
    int *d_status = reinterpret_cast<int *>(d_offsets + row_bytes / 4);
    AZH_HIP(hipStreamSynchronize(s->stream));
    if (stream)
        AZH_HIP(hipStreamSynchronize((hipStream_t)stream));
    hipStream_t st = s->stream;
    AZH_HIP(hipMemcpyAsync(d_at, at.data(), N * sizeof(u32), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_retarget_count, dim3((unsigned)n), dim3(WAVE), 0, st, d_reports, n, d_counts, d_bad);
    hipLaunchKernelGGL(k_retarget_block_sums, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, st, d_counts, d_bad, n, d_sums);
    hipLaunchKernelGGL(k_retarget_scan, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, st, d_counts, n, d_sums, d_offsets, d_totals);
    AZH_HIP(hipGetLastError());
    u64 totals[2] = {0, 0};
    AZH_HIP(hipMemcpyAsync(totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    AZH_HIP(hipStreamSynchronize(st));
    if (totals[1])
        return azh_fail(-2, "azh_samples_retarget: %llu of the %d records are malformed (more than %d edges, or a visited "
                            "move that is no clone and no jump)", (unsigned long long)totals[1], n, AZH_MAX_MOVES);
    if ((u64)s->targets + totals[0] > (u64)s->cap_targets)
        return azh_fail(-6, "azh_samples_retarget: %llu new targets do not fit beside %lld in a capacity of %lld",
                        (unsigned long long)totals[0], (long long)s->targets, (long long)s->cap_targets);
    hipLaunchKernelGGL(k_retarget_write, dim3((unsigned)n), dim3(WAVE), 0, st, d_reports, n, d_at, d_offsets, (u32)s->targets,
                       s->d_plies.d, s->d_target_index.d, s->d_target_weight.d, d_status);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipMemcpyAsync(status_out, d_status, N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AZH_HIP(hipStreamSynchronize(st));
    s->targets += (int64_t)totals[0];
    return 0;
}

// ---------------------------------------------------------------- proven outcomes for stored plies (include/ataxxzero_hip.h)

namespace {

constexpr int PROVE_CHUNK = SURPRISE_CHUNK;  // plies per launch: a launch runs no longer than this many searches under the budget

struct ProveItem {  // one eligible ply of a call
    u32 ply, game;  // its place in the store; its game, whose wall mask the search runs on
};
struct ProveResult {  // what azh_alphabeta_search reports for the ply's position
    int value;
    u32 move_depth;  // move | depth_done << 16
    u64 nodes;
};
struct ProofRow {  // azh_samples_proofs: one ply's three words
    int proof, move, depth_done;
};

// k_alphabeta's shape: one wave per ply, AB_WAVES of them per workgroup, each on its own stack in LDS; no wave waits for
// another.  The position is read where the store keeps it: the ply's record and its game's wall mask.
__global__ __launch_bounds__(AB_WAVES *WAVE) void k_samples_prove(View v, const ProveItem *__restrict__ items, int n, int depth,
                                                                  u64 budget, ProveResult *__restrict__ out)
{
    __shared__ AbStack stacks[AB_WAVES];
    const int wave = (int)(threadIdx.x >> 6);
    const int r = uni((int)blockIdx.x * AB_WAVES + wave);
    if (r >= n)
        return;  // the whole wave
    const ProveItem it = items[r];
    const Ply ply = v.plies[it.ply];
    Board root;
    root.x = ply.x;
    root.o = ply.o;
    root.turn = (ply.targets_flags & PLY_ODD) ? 1 : 0;
    const u64 bl = v.blockers ? v.blockers[it.game] : 0ULL;
    const AbAnswer a = ab_search_position(root, bl, &stacks[wave], depth, budget);
    if (lane_id() == 0)
        out[r] = ProveResult{a.value, a.move | ((u32)a.depth_done << 16), a.nodes};
}

// Phase 2: item i's result goes to its ply's three proof words (the proof only where the value is a proven one); slot[i] !=
// NONE: the ply also takes the single pair (its move, 1.0f) at target slot[i].  The host has found the room.
__global__ __launch_bounds__(256) void k_samples_prove_commit(const ProveItem *__restrict__ items, const ProveResult *__restrict__ res,
                                                              const u32 *__restrict__ slot, int n, Ply *__restrict__ plies,
                                                              int16_t *__restrict__ proofs, u16 *__restrict__ moves,
                                                              uint8_t *__restrict__ depths, u16 *__restrict__ target_index,
                                                              float *__restrict__ target_weight)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n)
        return;
    const u32 at = items[i].ply;
    const ProveResult r = res[i];
    if (r.value >= AB_WIN || r.value <= -AB_WIN)
        proofs[at] = (int16_t)r.value;
    moves[at] = (u16)(r.move_depth & 0xFFFFu);
    depths[at] = (uint8_t)(r.move_depth >> 16);
    if (slot && slot[i] != NONE) {
        target_index[slot[i]] = (u16)policy_index(r.move_depth & 0xFFFFu);
        target_weight[slot[i]] = 1.0f;
        plies[at].first_target = slot[i];
        plies[at].targets_flags = (1u << 8) | (plies[at].targets_flags & 0xFFu);
    }
}

__global__ __launch_bounds__(256) void k_samples_read_proofs(int n, const u32 *__restrict__ ply_at, const int16_t *__restrict__ proofs,
                                                             const u16 *__restrict__ moves, const uint8_t *__restrict__ depths,
                                                             ProofRow *__restrict__ out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n)
        out[i] = ProofRow{(int)proofs[ply_at[i]], (int)moves[ply_at[i]], (int)depths[ply_at[i]]};
}

}  // namespace

// The three proof arrays, all or none: no proof, no move (0xFFFF), no iteration for every ply the store can hold.
static int reserve_proofs(azh_samples *s)
{
    if (s->d_proofs.d)
        return 0;
    DeviceArray<int16_t> proofs;
    DeviceArray<u16> moves;
    DeviceArray<uint8_t> depths;
    const size_t cap = (size_t)s->cap_plies;
    int rc = proofs.alloc(cap);
    rc = rc ? rc : moves.alloc(cap);
    rc = rc ? rc : depths.alloc(cap);
    if (!rc) {
        hipError_t e = hipMemsetAsync(proofs.d, 0, cap * sizeof(int16_t), s->stream);
        e = e == hipSuccess ? hipMemsetAsync(moves.d, 0xFF, cap * sizeof(u16), s->stream) : e;
        e = e == hipSuccess ? hipMemsetAsync(depths.d, 0, cap, s->stream) : e;
        e = e == hipSuccess ? hipStreamSynchronize(s->stream) : e;
        if (e != hipSuccess)
            rc = azh_fail(-100 - (int)e, "azh_samples_prove: %s", hipGetErrorString(e));
    }
    if (rc) {
        proofs.release();
        moves.release();
        depths.release();
        return rc;
    }
    s->d_proofs = proofs;
    s->d_proof_moves = moves;
    s->d_proof_depths = depths;
    return 0;
}

extern "C" int azh_samples_prove(azh_samples *s, int64_t first_game, int64_t n_games, int depth, uint64_t node_budget,
                                 int retarget_wins, uint64_t *stats_out)
{
    if (!s || !stats_out)
        return azh_fail(-1, "azh_samples_prove: null argument");
    if (first_game < 0 || n_games < 1 || first_game + n_games > s->games)
        return azh_fail(-1, "azh_samples_prove: games [%lld, %lld) of %lld", (long long)first_game,
                        (long long)(first_game + n_games), (long long)s->games);
    if (const char *why = limits_refusal(depth, node_budget))
        return azh_fail(-2, "azh_samples_prove: %s", why);
    // the eligible plies in ascending (game, ply) order, from the mirrors: a game's candidates are kept in ply order
    std::vector<ProveItem> items;
    for (int64_t g = first_game; g < first_game + n_games; g++) {
        const u32 first = s->h_games[4 * g];
        for (u32 k = 0; k < s->h_count[(size_t)g]; k++) {
            const u32 at = first + s->h_candidates[first + k];
            if (s->h_flags[at] & (AZH_SAMPLES_PLY_PASS | AZH_SAMPLES_PLY_BAD))
                continue;
            if (at < s->h_proofs.size() && s->h_proofs[at] != 0)
                continue;
            items.push_back(ProveItem{at, (u32)g});
        }
    }
    uint64_t stats[AZH_SAMPLES_PROOF_STAT_COUNT] = {};
    const size_t N = items.size();
    if (N == 0) {
        memcpy(stats_out, stats, sizeof(stats));
        return 0;
    }
    // phase 1: every search into scratch, nothing of the store written
    const size_t item_bytes = round_up(N * sizeof(ProveItem)), result_bytes = round_up(N * sizeof(ProveResult));
    if (int rc = reserve_scratch(s, item_bytes + result_bytes + round_up(N * sizeof(u32))))
        return rc;
    ProveItem *d_items = reinterpret_cast<ProveItem *>(s->d_scratch.d);
    ProveResult *d_results = reinterpret_cast<ProveResult *>(s->d_scratch.d + item_bytes);
    u32 *d_slot = reinterpret_cast<u32 *>(s->d_scratch.d + item_bytes + result_bytes);
    hipStream_t st = s->stream;
    AZH_HIP(hipStreamSynchronize(st));
    AZH_HIP(hipMemcpyAsync(d_items, items.data(), N * sizeof(ProveItem), hipMemcpyHostToDevice, st));
    for (size_t at = 0; at < N; at += PROVE_CHUNK) {
        const int n = (int)std::min<size_t>(PROVE_CHUNK, N - at);
        hipLaunchKernelGGL(k_samples_prove, dim3((unsigned)((n + AB_WAVES - 1) / AB_WAVES)), dim3(AB_WAVES * WAVE), 0, st, s->view(),
                           d_items + at, n, depth, (u64)node_budget, d_results + at);
        AZH_HIP(hipGetLastError());
    }
    std::vector<ProveResult> results(N);
    AZH_HIP(hipMemcpyAsync(results.data(), d_results, N * sizeof(ProveResult), hipMemcpyDeviceToHost, st));
    AZH_HIP(hipStreamSynchronize(st));
    std::vector<u32> slot(N, NONE);
    stats[AZH_PROOF_VISITED] = N;
    for (size_t i = 0; i < N; i++) {
        const ProveResult &r = results[i];
        stats[AZH_PROOF_NODES] += r.nodes;
        if (r.value > -AB_WIN && r.value < AB_WIN)
            continue;
        const u32 p = items[i].ply - s->h_games[4 * (size_t)items[i].game];
        const bool mover_won = (s->h_games[4 * (size_t)items[i].game + 2] & 0xFFu) == 1u + (p & 1u);
        stats[r.value > 0 ? AZH_PROOF_WINS : AZH_PROOF_LOSSES]++;
        stats[AZH_PROOF_CONTRADICTED] += (r.value > 0) != mover_won;
        if (retarget_wins && r.value > 0 && (r.move_depth & 0xFFFFu) != 0xFFFFu)
            slot[i] = (u32)(s->targets + (int64_t)stats[AZH_PROOF_RETARGETED]++);
    }
    if ((u64)s->targets + stats[AZH_PROOF_RETARGETED] > (u64)s->cap_targets)
        return azh_fail(-6, "azh_samples_prove: %llu new targets do not fit beside %lld in a capacity of %lld",
                        (unsigned long long)stats[AZH_PROOF_RETARGETED], (long long)s->targets, (long long)s->cap_targets);
    // phase 2
    if (int rc = reserve_proofs(s))
        return rc;
    const bool pairs = stats[AZH_PROOF_RETARGETED] != 0;
    if (pairs)
        AZH_HIP(hipMemcpyAsync(d_slot, slot.data(), N * sizeof(u32), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_samples_prove_commit, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, d_items, d_results,
                       pairs ? d_slot : (const u32 *)nullptr, (int)N, s->d_plies.d, s->d_proofs.d, s->d_proof_moves.d,
                       s->d_proof_depths.d, s->d_target_index.d, s->d_target_weight.d);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipStreamSynchronize(st));
    s->h_proofs.resize((size_t)s->plies, 0);
    for (size_t i = 0; i < N; i++)
        if (results[i].value >= AB_WIN || results[i].value <= -AB_WIN)
            s->h_proofs[items[i].ply] = (int16_t)results[i].value;
    s->targets += (int64_t)stats[AZH_PROOF_RETARGETED];
    memcpy(stats_out, stats, sizeof(stats));
    return 0;
}

extern "C" int azh_samples_proofs(azh_samples *s, int n, const int32_t *plies, int32_t *proof_out, uint16_t *move_out,
                                  int32_t *depth_done_out)
{
    if (!s || !plies || !proof_out || !move_out || !depth_done_out || n < 1)
        return azh_fail(-1, "azh_samples_proofs: bad argument");
    std::vector<u32> at;
    if (int rc = ply_places(s, "azh_samples_proofs", n, plies, at))
        return rc;
    const size_t N = (size_t)n, at_bytes = round_up(N * sizeof(u32));
    std::vector<ProofRow> got(N, ProofRow{0, 0xFFFF, 0});
    if (s->d_proofs.d) {
        if (int rc = reserve_scratch(s, at_bytes + round_up(N * sizeof(ProofRow))))
            return rc;
        u32 *d_at = reinterpret_cast<u32 *>(s->d_scratch.d);
        ProofRow *d_out = reinterpret_cast<ProofRow *>(s->d_scratch.d + at_bytes);
        AZH_HIP(hipMemcpyAsync(d_at, at.data(), N * sizeof(u32), hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(k_samples_read_proofs, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, n, d_at, s->d_proofs.d,
                           s->d_proof_moves.d, s->d_proof_depths.d, d_out);
        AZH_HIP(hipGetLastError());
        AZH_HIP(hipMemcpyAsync(got.data(), d_out, N * sizeof(ProofRow), hipMemcpyDeviceToHost, s->stream));
        AZH_HIP(hipStreamSynchronize(s->stream));
    }
    for (size_t i = 0; i < N; i++) {
        proof_out[i] = got[i].proof;
        move_out[i] = (uint16_t)got[i].move;
        depth_done_out[i] = got[i].depth_done;
    }
    return 0;
}

// ---------------------------------------------------------------- lambda-returns as value targets (include/ataxxzero_hip.h)

namespace {

constexpr int RETURNS_WAVES = 4;  // games per workgroup, one wave each; no wave waits for another

// The definition's step: a = 1.0 - lambda comes in, four IEEE double operations in all, none fused (-ffp-contract=off).
__host__ __device__ inline double return_step(double b /* a * v_p */, double lambda, double next) { return b + lambda * next; }

__host__ __device__ inline double result_for_mover(u32 result, u32 ply) { return result == 1u + (ply & 1u) ? 1.0 : -1.0; }

__device__ __forceinline__ double read_lane_f64(double v, int src)
{
    const u64 bits = f64_bits(v);
    const u64 got = (u64)(u32)read_lane((int)(u32)bits, src) | ((u64)(u32)read_lane((int)(u32)(bits >> 32), src) << 32);
    double out;
    memcpy(&out, &got, sizeof(out));
    return out;
}

// One wave per game, from the game's end in chunks of 64 plies: lane l loads the value and the proof of ply lo + l (the
// independent part, a * v_p, is done there), the proofs become two wave-uniform masks, and the chunk's steps run in ply order on
// b read from lane j's register; lane j keeps G_j and stores it.  `next` is carried from chunk to chunk.
__global__ __launch_bounds__(RETURNS_WAVES *WAVE) void k_samples_value_returns(View v, u32 first_game, int n_games, double lambda,
                                                                              double *__restrict__ returns)
{
    const int lane = lane_id();
    const int r = uni((int)blockIdx.x * RETURNS_WAVES + (int)(threadIdx.x >> 6));
    if (r >= n_games)
        return;  // the whole wave
    const uint4 game = v.games[first_game + (u32)r];
    if (!(game.z & GAME_HAS_VALUES))
        return;  // (wave-uniform) its plies stay absent
    const int T = (int)game.y;
    const double a = 1.0 - lambda;
    double next = result_for_mover(game.z & 0xFFu, (u32)(T - 1));  // z of the last ply's mover
    for (int hi = T; hi > 0; hi -= WAVE) {
        const int lo = hi > WAVE ? hi - WAVE : 0, n = hi - lo;
        const u32 at = game.x + (u32)(lo + lane);
        double value = 0.0;
        int proof = 0;
        if (lane < n) {
            value = v.plies[at].value;
            proof = v.proofs ? (int)v.proofs[at] : 0;
        }
        const double b = a * value;
        const u64 won = __ballot(proof > 0), lost = __ballot(proof < 0);
        double mine = 0.0;
        for (int j = n - 1; j >= 0; j--) {  // (wave-uniform: every lane computes every step)
            double G = return_step(read_lane_f64(b, j), lambda, next);
            if ((won >> j) & 1ULL)
                G = 1.0;
            else if ((lost >> j) & 1ULL)
                G = -1.0;
            if (lane == j)
                mine = G;
            next = -G;
        }
        if (lane < n)
            returns[at] = mine;
    }
}

struct ReturnRow {
    double value;
    int present;
};

__global__ __launch_bounds__(256) void k_samples_read_returns(int n, const u32 *__restrict__ ply_at, const double *__restrict__ returns,
                                                              ReturnRow *__restrict__ out)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n)
        return;
    const double g = returns[ply_at[i]];
    const bool present = f64_bits(g) != RETURN_ABSENT;
    out[i] = ReturnRow{present ? g : 0.0, present ? 1 : 0};
}

const char *lambda_refusal(double lambda)
{
    return lambda >= 0.0 && lambda <= 1.0 ? nullptr : "lambda must be a number in [0, 1]";
}

}  // namespace

extern "C" int azh_samples_value_returns_host(const double *values, const int32_t *proofs, int64_t T, uint32_t result,
                                              double lambda, double *out)
{
    if (T < 0 || (T > 0 && (!values || !out)))
        return azh_fail(-1, "azh_samples_value_returns_host: null argument or a game of %lld plies", (long long)T);
    if (const char *why = lambda_refusal(lambda))
        return azh_fail(-2, "azh_samples_value_returns_host: %s", why);
    const double a = 1.0 - lambda;
    double next = 0.0;
    for (int64_t p = T - 1; p >= 0; p--) {
        if (p == T - 1)
            next = result_for_mover(result, (u32)p);
        const double b = a * values[p];
        double G = return_step(b, lambda, next);
        if (proofs && proofs[p] != 0)
            G = proofs[p] > 0 ? 1.0 : -1.0;
        out[p] = G;
        next = -G;
    }
    return 0;
}

extern "C" int azh_samples_value_returns(azh_samples *s, int64_t first_game, int64_t n_games, double lambda)
{
    if (!s)
        return azh_fail(-1, "azh_samples_value_returns: null store");
    if (first_game < 0 || n_games < 1 || first_game + n_games > s->games)
        return azh_fail(-1, "azh_samples_value_returns: games [%lld, %lld) of %lld", (long long)first_game,
                        (long long)(first_game + n_games), (long long)s->games);
    if (const char *why = lambda_refusal(lambda))
        return azh_fail(-2, "azh_samples_value_returns: %s", why);
    hipStream_t st = s->stream;
    AZH_HIP(hipStreamSynchronize(st));
    if (!s->d_returns.d) {  // every ply the store can hold: absent
        DeviceArray<double> fresh;
        if (int rc = fresh.alloc((size_t)s->cap_plies))
            return rc;
        hipError_t e = hipMemsetAsync(fresh.d, 0xFF, (size_t)s->cap_plies * sizeof(double), st);
        e = e == hipSuccess ? hipStreamSynchronize(st) : e;
        if (e != hipSuccess) {
            fresh.release();
            return azh_fail(-100 - (int)e, "azh_samples_value_returns: %s", hipGetErrorString(e));
        }
        s->d_returns = fresh;
    }
    hipLaunchKernelGGL(k_samples_value_returns, dim3((unsigned)((n_games + RETURNS_WAVES - 1) / RETURNS_WAVES)),
                       dim3(RETURNS_WAVES * WAVE), 0, st, s->view(), (u32)first_game, (int)n_games, lambda, s->d_returns.d);
    AZH_HIP(hipGetLastError());
    AZH_HIP(hipStreamSynchronize(st));
    return 0;
}

extern "C" int azh_samples_clear_value_returns(azh_samples *s)
{
    if (!s)
        return azh_fail(-1, "azh_samples_clear_value_returns: null store");
    AZH_HIP(hipDeviceSynchronize());
    s->d_returns.release();
    return 0;
}

extern "C" int azh_samples_read_value_returns(azh_samples *s, int n, const int32_t *plies, double *out, int32_t *present)
{
    if (!s || !plies || !out || !present || n < 1)
        return azh_fail(-1, "azh_samples_read_value_returns: bad argument");
    std::vector<u32> at;
    if (int rc = ply_places(s, "azh_samples_read_value_returns", n, plies, at))
        return rc;
    const size_t N = (size_t)n, at_bytes = round_up(N * sizeof(u32));
    std::vector<ReturnRow> got(N, ReturnRow{0.0, 0});
    if (s->d_returns.d) {
        if (int rc = reserve_scratch(s, at_bytes + round_up(N * sizeof(ReturnRow))))
            return rc;
        u32 *d_at = reinterpret_cast<u32 *>(s->d_scratch.d);
        ReturnRow *d_out = reinterpret_cast<ReturnRow *>(s->d_scratch.d + at_bytes);
        AZH_HIP(hipMemcpyAsync(d_at, at.data(), N * sizeof(u32), hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(k_samples_read_returns, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, n, d_at,
                           s->d_returns.d, d_out);
        AZH_HIP(hipGetLastError());
        AZH_HIP(hipMemcpyAsync(got.data(), d_out, N * sizeof(ReturnRow), hipMemcpyDeviceToHost, s->stream));
        AZH_HIP(hipStreamSynchronize(s->stream));
    }
    for (size_t i = 0; i < N; i++) {
        out[i] = got[i].value;
        present[i] = got[i].present;
    }
    return 0;
}
