// Host-side helpers shared by the translation units of libataxxzero_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#define AZH_NO_REFERENCE_ABI
#include "../../include/ataxxzero_hip.h"
#include "record.h"

// Record the message for azh_last_error() and return `code`.
int azh_fail(int code, const char *fmt, ...);
// 0 when a HIP device is usable; otherwise records why and returns non-zero.
// There is no CPU fallback: every compute entry point fails loudly without a GPU.
int azh_require_device(void);

#define AZH_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return azh_fail(-100 - (int)_e, "%s failed at %s:%d: %s", #expr, __FILE__,     \
                            __LINE__, hipGetErrorString(_e));                               \
    } while (0)

// json.cpp: finished-game records (record.h) -> game lines.  Only azh_record_well_formed takes words nobody has checked.
bool azh_record_well_formed(const uint32_t *rec, size_t avail, uint32_t max_plies, const char **why);
std::string azh_format_game_json(const uint32_t *rec, bool with_ids);
std::string azh_format_game_json_blockers(const uint32_t *rec, bool with_ids, uint64_t blockers);
uint64_t azh_ply_target(azh::PlyView ply, std::vector<std::pair<std::string, uint32_t>> &ents);

// net_kernels.hip: one tower launch over a batch of boards.  Every pointer is a device pointer.
namespace azh {
struct AdvanceHook;  // engine_device.h
struct NetBatch {
    const unsigned long long *boards = nullptr;  // (mover, opponent) per game
    const int *list = nullptr, *count = nullptr;  // dense list of the games to evaluate; both null: the first max_n boards
    int max_n = 0;                                // bound of *count (of count_a + count_b for a pair: a game has one leaf)
    unsigned long long blockers = 0;              // the wall mask of every board ...
    const unsigned long long *masks = nullptr;    // ... or, non-null, one mask per board, indexed as `boards`
    float *logits = nullptr, *values = nullptr;   // [.][833] and [.], indexed by game
};
struct NetOptions {
    int thin = 0;  // the caller expects a handful of boards (<= 512): one board per workgroup (Geo2Thin) where that kernel applies
    unsigned long long *stamps = nullptr;  // diagnostic: the stamped bf16 tower writes [wg][wave][128] clock values here
    const AdvanceHook *hook = nullptr;     // the device-resident search loop's queued moves are played by the first
                                           // `workers` workgroups of the launch
    // both non-null: the symmetry-averaged evaluation (nn_evals.py:48-62) — the tower runs 8 * max_n virtual boards into
    // this scratch ([8 max_n][833] and [8 max_n] floats), k_sym_reduce behind it writes the averages by game
    float *sym_logits = nullptr, *sym_values = nullptr;
};
}  // namespace azh
int azh_net_launch(azh_net *net, int dtype, const azh::NetBatch &batch, hipStream_t stream, const azh::NetOptions &options = {});
// two nets, two dense leaf lists (batch.list / batch.count are net_a's), one launch (arena); 1 = not applicable here, nothing
// launched (launch them one by one)
int azh_net_launch_pair(azh_net *net_a, azh_net *net_b, int dtype, const azh::NetBatch &batch, const int *list_b,
                        const int *count_b, hipStream_t stream, const azh::NetOptions &options);
