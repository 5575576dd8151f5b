// The finished-game record, stated once.  The device loop writes it into the ring (engine_device.h, advance_game); the host
// reads it back into game lines (json.cpp), into the trainer's sample store (samples.hip) and into the drain (engine.hip).
// ataxxzero_amd/link.py restates the constants under the same names and walks the same layout in link.records.
//
// 8-word header {magic, slot, uid, plies, result, words, random_ply + 1 (0 = none), kind}, then per ply 6 fixed words
// {x lo, x hi, o lo, o hi, move | nd << 16, full} and nd x (move | count << 16), nd <= REC_MAXD.  `words` counts the whole
// record, header included; the plies fill it exactly.
// kind, bits 0-1: 0 a whole game, 1 the marker a dropped game leaves (a header and nothing else), 2 a game begun at a loaded
// position (it lacks the plies before the start, so no line is written for it outside the arena).  Beside them:
//   | 4  the game was played with the playout cap on (azh_engine_set_playout_cap): word 5 of a ply is 1 where the ply was
//        searched in full, and the line carries "full";
//   | 8  forced playouts were on: the counts of the plies the mode acts on are the pruned ones — no reader depends on it;
//   | 16 the search value was recorded (azh_engine_set_resign): word 5 of a ply is the f32 bits of q = W_b / n_b of the most
//        visited root edge (in [0, 1], for the mover) with the sign bit = searched in full, and the line gains "values"
//        (2 q - 1 as a double; a q that is not finite reads 0);
//   | 32 the game ended by resignation: the line gains "resigned" (the side that resigned, 3 - result: the mover of the last
//        ply);
//   | 64 the Gumbel root search was on (azh_engine_set_gumbel): the counts are the improved policy in units of 1/65535 of
//        its greatest entry, over every root move — no reader depends on it.
// The views below name these words and nothing more: they check no bound.  azh_record_well_formed (json.cpp) is the one
// function that reads words nobody has checked; every other reader stands behind it.
#pragma once

#include <stdint.h>

namespace azh {

constexpr uint32_t RING_MAGIC = 0x415A4847u;  // "AZHG"
enum { REC_MAGIC, REC_SLOT, REC_UID, REC_PLIES, REC_RESULT, REC_WORDS, REC_RANDOM_PLY_PLUS_1, REC_KIND };  // header words
constexpr int REC_HDR_WORDS = 8;
constexpr int REC_PLY_WORDS = 6;
constexpr int REC_MAXD = 256;
constexpr uint32_t REC_KIND_MASK = 3u;  // bits 0-1 of header word 7
constexpr uint32_t REC_KIND_WHOLE = 0u;
constexpr uint32_t REC_KIND_DROPPED = 1u;
constexpr uint32_t REC_KIND_LOADED = 2u;
constexpr uint32_t REC_KIND_PLAYOUT_CAP = 4u;  // the mode bits beside them
constexpr uint32_t REC_KIND_FORCED = 8u;
constexpr uint32_t REC_KIND_VALUES = 16u;
constexpr uint32_t REC_KIND_RESIGNED = 32u;
constexpr uint32_t REC_KIND_GUMBEL = 64u;
constexpr uint32_t REC_KIND_MODES = REC_KIND_PLAYOUT_CAP | REC_KIND_FORCED | REC_KIND_VALUES | REC_KIND_RESIGNED | REC_KIND_GUMBEL;
constexpr uint32_t REC_PLY_FULL_BIT = 0x80000000u;  // ply word 5 under REC_KIND_VALUES: full << 31 | the bits of q
constexpr uint32_t REC_PLY_Q_BITS = 0x7FFFFFFFu;

struct PlyView {
    const uint32_t *w;
    uint64_t x() const { return (uint64_t)w[0] | ((uint64_t)w[1] << 32); }
    uint64_t o() const { return (uint64_t)w[2] | ((uint64_t)w[3] << 32); }
    uint32_t move() const { return w[4] & 0xFFFFu; }
    uint32_t targets() const { return w[4] >> 16; }
    bool full(bool valued) const { return (valued ? w[5] & REC_PLY_FULL_BIT : w[5]) != 0; }
    double value(bool valued) const  // 2 q - 1; 0 where no value was recorded or q is not finite
    {
        const uint32_t bits = w[5] & REC_PLY_Q_BITS;
        if (!valued || (bits & 0x7F800000u) == 0x7F800000u)
            return 0.0;
        float q;
        __builtin_memcpy(&q, &bits, 4);
        return 2.0 * (double)q - 1.0;
    }
    uint32_t target(uint32_t j) const { return w[REC_PLY_WORDS + j]; }  // move | count << 16
    PlyView next() const { return {w + REC_PLY_WORDS + targets()}; }
};

struct RecordView {
    const uint32_t *w;
    uint32_t slot() const { return w[REC_SLOT]; }
    uint32_t uid() const { return w[REC_UID]; }
    uint32_t plies() const { return w[REC_PLIES]; }
    uint32_t result() const { return w[REC_RESULT]; }
    uint32_t words() const { return w[REC_WORDS]; }
    uint32_t random_ply_plus_1() const { return w[REC_RANDOM_PLY_PLUS_1]; }
    bool dropped() const { return (w[REC_KIND] & REC_KIND_MASK) == REC_KIND_DROPPED; }
    bool loaded() const { return (w[REC_KIND] & REC_KIND_MASK) == REC_KIND_LOADED; }
    bool capped() const { return (w[REC_KIND] & REC_KIND_PLAYOUT_CAP) != 0; }
    bool valued() const { return (w[REC_KIND] & REC_KIND_VALUES) != 0; }
    bool resigned() const { return (w[REC_KIND] & REC_KIND_RESIGNED) != 0; }
    bool gumbel() const { return (w[REC_KIND] & REC_KIND_GUMBEL) != 0; }
    PlyView first_ply() const { return {w + REC_HDR_WORDS}; }
};

}  // namespace azh
