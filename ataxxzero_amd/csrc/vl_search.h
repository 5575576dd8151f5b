// Leaf-parallel search with virtual loss (azh_engine_set_leaf_batch): one tree selects up to K leaves per iteration, the
// leaves go to the net in the same tower launch, and the K paths are backed up before the next select.  Included by
// engine.hip (compiled -ffp-contract=off) after the one-leaf tree kernels, whose device functions it shares
// (apply_priors, mark_game, compact_leaves); none of those changes with it.  A level's score is exploration_score
// (azh_device.h): puct_score's operations with the node's c and the unvisited children's Q as arguments — c_puct and 0, i.e.
// puct_score itself, unless azh_engine_set_exploration switched first-play urgency or the growing exploration rate on.
//
// The definition (DESIGN.md "Leaf-parallel search"; tests/vl_reference.py restates it in numpy):
//   k = min(K, T - root_visits) paths per iteration (at least 1; T = visits, or the ply's own threshold under the playout cap), selected as if one after the other, each on the
//   tree the earlier paths of the batch left: an edge taken by c earlier paths scores with n + VL c visits and an
//   unchanged W (a virtual loss is a visit that scored 0 for the mover), N is the sum of the children's effective
//   counts.  A path ends at an edge without a child (EVAL: expanded exactly as select_game does, its node and edges
//   appended to the arena in path order), at a finished node (TERMINAL), or at a node an earlier path of this batch
//   created (COLLISION).  Every path keeps its virtual loss until the backup, which applies the EVAL and TERMINAL paths in
//   path order, each like one ordinary backup, and removes every virtual loss.
//
// The virtual loss lives in the tree itself: a path adds VL to the visit count of every edge it takes as it takes it
// (16-bit field: visits <= 60000, VL * K <= 1024), so the next path's PUCT reads the effective counts with select's own
// loads and arithmetic.  One wave descends the k paths one after the other; a path's stores are made visible to the
// next path's loads by a workgroup-scope fence (same wave, same CU).
#pragma once

namespace azh {

constexpr int VL_MAX_LEAVES = 64;    // paths per game and iteration: one lane each in the backup
constexpr int VL_MAX_LOSS = 16;      // 60000 visits + 16 * 64 stays inside the edge record's 16-bit visit field
constexpr int VL_WAVES = 4;          // waves per game: the priors of a batch's new nodes are computed four at a time

struct VlParams {
    int K, vl, path_cap;
    int *kind;        // [G * K] slot kinds (AZH_LEAF_*) of the current batch
    u32 *leaf_edge;   // [G * K] the last edge of the slot's path (NONE: no edge)
    int *leaf_node;   // [G * K] the node the path ended at
    int *path_len;    // [G * K] edges on the path
    int *path;        // [G * K][path_cap] the paths' edges, root first
    int solver;       // azh_engine_set_solver: the backup is followed by the proof pass (vl_prove)
    u64 *proofs;      // [G][2] counters of the proof pass: AZH_PROOF_STAT_NODES, _HITS (azh_engine_proof_stats)
};

// What the ply of a game searches with: the engine's own settings, or (azh_engine_set_search_sets) the set of the side to move
// at the root.  Wave-uniform, resolved once per game and launch by k_vl_tree.
struct PlySearch {
    int visits, leaves, vl;  // root visits at which the move is due; paths per iteration; the virtual loss
    float c_puct, fpu_reduction, c_base, c_init;
};

__device__ inline PlySearch engine_search(const EngineParams &P, const VlParams &V, u32 pk)
{
    PlySearch S;
    S.visits = ply_threshold(P, pk);
    S.leaves = V.K;
    S.vl = V.vl;
    S.c_puct = P.c_puct;
    S.fpu_reduction = P.fpu_reduction;
    S.c_base = P.c_base;
    S.c_init = P.c_init;
    return S;
}

// Search settings per side: the set of the root's mover — the root board's turn bit picks the byte of the slot's word, and the
// set's seven values come from the table on the device.  g, s: wave-uniform, and so is every load here (readfirstlane: the
// values live in scalar registers beside the engine's own, which they replace).  The root is the same for the backup, the
// mark and the select of one launch: a batch's backup removes the virtual loss its select put on.
__device__ inline void set_search(const EngineParams &P, int g, const azh_game_state &s, PlySearch &S)
{
    if (P.search_sets == nullptr)
        return;
    const u64 w0 = arena_of(P, s.arena, g).nb[0].x;
    const u32 word = P.slot_sets[g];
    const int i = __builtin_amdgcn_readfirstlane((int)((w0 & TURN_BIT) ? (word >> 8) & 0xFFu : word & 0xFFu));
    const azh_search_set &t = P.search_sets[i];
    S.visits = __builtin_amdgcn_readfirstlane(t.visits);
    S.leaves = __builtin_amdgcn_readfirstlane(t.leaves);
    S.vl = __builtin_amdgcn_readfirstlane(t.virtual_loss);
    S.c_puct = u2f((u32)__builtin_amdgcn_readfirstlane((int)f2u(t.c_puct)));
    S.fpu_reduction = u2f((u32)__builtin_amdgcn_readfirstlane((int)f2u(t.fpu_reduction)));
    S.c_base = u2f((u32)__builtin_amdgcn_readfirstlane((int)f2u(t.c_base)));
    S.c_init = u2f((u32)__builtin_amdgcn_readfirstlane((int)f2u(t.c_init)));
}

// Selects the game's batch: k paths in path order (phase 1), the root evaluation (phase 0, slot 0), or nothing.  `s` is
// the game's state in registers (uniform over the lanes); stored here.  Returns the slots that need the net (bit p: slot p).
// `S`: what the ply searches with (its visits are the T of k below, its leaves the K).
__device__ inline u64 vl_select_game(const EngineParams &P, const VlParams &V, int g, azh_game_state &s, u16 *s_moves, const PlySearch &S)
{
    const int lane = lane_id();
    const int K = V.K;
    const size_t base = (size_t)g * K;
    Arena A = arena_of(P, s.arena, g);
    const u32 tie_flip = (P.flags & AZH_FLAG_TIE_FIRST) ? 0xFFFFFFFFu : 0u;
    // first-play urgency and the exploration rate (azh_engine_set_exploration, or the ply's search set): wave-uniform
    const bool explore = exploration_on(S.fpu_reduction, S.c_base);
    // lane p collects slot p's result
    int r_kind = AZH_LEAF_NONE, r_node = 0, r_len = 0;
    u32 r_edge = NONE;
    u64 r_mover = 0, r_opp = 0;
    int over = 0, paths = 0;
    u64 st_steps = 0, st_evals = 0, st_levels = 0, st_children = 0, st_newmoves = 0, st_coll = 0;

    if (s.phase >= 2) {
        // move due (played after this select) or idle slot: no leaf
    } else if (s.phase == 0) {
        // the root's priors are (re)computed with noise: one leaf, slot 0
        const ulonglong2 w = A.nb[0];
        const Board b = unpack_board(w.x, w.y);
        if (lane == 0) {
            r_kind = AZH_LEAF_ROOT;
            r_mover = b.turn ? b.o : b.x;
            r_opp = b.turn ? b.x : b.o;
        }
        st_evals = 1;
        s.leaf_kind = AZH_LEAF_ROOT;
    } else {
        const int nodes0 = s.n_nodes;  // nodes from this id on were created by this batch (unevaluated until its backup)
        const int k = max(1, min(S.leaves, S.visits - s.root_visits));
        const uint4 rinfo = A.ni[0];
        const u32 root_kid = pack_kid(rinfo.x, rinfo.y & 0xFFFFu, (rinfo.y >> 16) != 0u);
        for (int p = 0; p < k; p++) {
            int *path = V.path + (base + (size_t)p) * V.path_cap;
            int kind = AZH_LEAF_NONE, depth = 0;
            u32 node = 0, kid = root_kid, leaf_e = NONE;
            u64 lm = 0, lo = 0;
            st_steps++;
            for (;;) {
                const int M = kid_count(kid);
                const u32 first = kid_first(kid);
                if (kid_finished(kid) || M == 0) {
                    kind = AZH_LEAF_TERMINAL;  // select_action -> NO_MOVE (:336-340)
                    break;
                }
                if ((int)node >= nodes0) {
                    kind = AZH_LEAF_COLLISION;  // an earlier path of this batch created it: still unevaluated
                    break;
                }
                st_levels += 1;
                st_children += (u64)M;
                const int rounds = (M + 63) >> 6;
                uint4 ev[4];
                u32 nsum = 0;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int j = lane + 64 * r;
                    ev[r] = fresh_edge(0u);
                    if (r < rounds && j < M) {
                        ev[r] = A.ed[first + j];
                        nsum += edge_visits(ev[r]);
                    }
                }
                // N = the sum of the children's effective counts, as the oracle sums them
                const u32 N = wave_sum_u32(nsum);
                const float sq = sqrtf((float)(1u + N));
                // c and the unvisited children's Q: c_puct and 0 unless the mode is on (exploration_score is then puct_score)
                float c = S.c_puct, fpu = 0.0f;
                if (explore) {
                    float wpart = 0.0f, ppart = 0.0f;  // the lane's terms j = lane, lane + 64, ... from +0 in that order
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (r < rounds && lane + 64 * r < M) {
                            wpart = wpart + u2f(ev[r].y);
                            ppart = ppart + (edge_visits(ev[r]) ? __builtin_fabsf(u2f(ev[r].x)) : 0.0f);
                        }
                    const float Wsum = wave_sum_f32(wpart), Psum = wave_sum_f32(ppart);
                    c = exploration_c(N, S.c_puct, S.c_base, S.c_init);
                    fpu = exploration_fpu(Wsum, Psum, N, S.fpu_reduction);
                }
                // arg-max with the engine's tie rule: (score bits << 32 | index or ~index), NaN and empty lanes key 0
                u64 key = 0;
                u32 mine = ev[0].z, mkid = ev[0].w;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int j = lane + 64 * r;
                    if (r < rounds && j < M) {
                        const float score = exploration_score(__builtin_fabsf(u2f(ev[r].x)), u2f(ev[r].y), edge_visits(ev[r]), sq, c, fpu);
                        const u64 kj = score >= 0.0f ? (((u64)f2u(score + 0.0f)) << 32) | (u64)((u32)j ^ tie_flip) : 0ull;
                        if (kj > key) {
                            key = kj;
                            mine = ev[r].z;
                            mkid = ev[r].w;
                        }
                    }
                }
                key = wave_max_u64(key);
                const int bj = key ? (int)((u32)key ^ tie_flip) : 0;
                const u32 eidx = first + (u32)bj;
                const u32 zsel = (u32)read_lane((int)mine, bj & 63);
                const u32 wsel = (u32)read_lane((int)mkid, bj & 63);
                if (lane == 0)
                    path[depth] = (int)eidx;
                depth++;
                leaf_e = eidx;
                const u32 child = zsel >> 16;
                if (child != ENONE) {
                    if (lane == 0)  // the path's virtual loss on this edge
                        reinterpret_cast<u32 *>(&A.ed[eidx])[2] = zsel + (u32)S.vl;
                    node = child;
                    kid = wsel;
                    continue;
                }
                // expand (:429-439), as select_game does
                const u32 mv = A.em[eidx];
                const ulonglong2 pw = A.nb[node];
                const Board cb = make_move(unpack_board(pw.x, pw.y), (int)(mv & 0xFF), (int)(mv >> 8));
                int res2;
                const int M2 = wave_movegen(cb, game_blockers(P, g), s_moves, &res2);
                wave_sync();
                if (s.n_nodes >= P.node_cap || (res2 == 0 && (s.n_edges + M2 > P.edge_cap || M2 > 255))) {
                    // arena full: this path is dropped (it keeps its virtual loss until the backup) and the batch ends
                    over = 1;
                    kind = AZH_LEAF_NONE;
                    if (lane == 0)
                        reinterpret_cast<u32 *>(&A.ed[eidx])[2] = zsel + (u32)S.vl;
                    break;
                }
                const u32 cid = (u32)s.n_nodes;
                s.n_nodes += 1;
                u32 nf = 0;
                if (res2 != 0) {
                    float tv = res2 == 1 ? 1.0f : -1.0f;
                    if (cb.turn == 1)
                        tv = -tv;
                    if (lane == 0)
                        A.ni[cid] = make_uint4(0u, (u32)res2 << 16, 0u, f2u(tv));
                    kind = AZH_LEAF_TERMINAL;
                } else {
                    nf = (u32)s.n_edges;
                    for (int j = lane; j < M2; j += WAVE) {
                        A.ed[nf + j] = fresh_edge(0u);
                        A.em[nf + j] = s_moves[j];
                    }
                    s.n_edges += M2;
                    if (lane == 0)
                        A.ni[cid] = make_uint4(nf, (u32)M2, 0u, 0u);
                    kind = AZH_LEAF_EVAL;
                    st_evals += 1;
                    st_newmoves += (u64)M2;
                    lm = cb.turn ? cb.o : cb.x;
                    lo = cb.turn ? cb.x : cb.o;
                }
                if (lane == 0) {
                    A.nb[cid] = make_ulonglong2(pack_word0(cb), cb.o);
                    // the edge gets its child, the child's range, and this path's virtual loss
                    reinterpret_cast<uint2 *>(&A.ed[eidx])[1] =
                        make_uint2((cid << 16) | (u32)S.vl, res2 != 0 ? pack_kid(0u, 0u, 1u) : pack_kid(nf, (u32)M2, 0u));
                }
                node = cid;
                break;
            }
            if (kind == AZH_LEAF_COLLISION)
                st_coll += 1;
            if (lane == p) {
                r_kind = kind;
                r_node = (int)node;
                r_len = depth;
                r_edge = leaf_e;
                r_mover = lm;
                r_opp = lo;
            }
            paths = p + 1;
            // this path's stores (virtual losses, the new node and its edges) before the next path's loads
            __threadfence_block();
            wave_sync();
            if (over)
                break;
        }
        s.leaf_kind = AZH_LEAF_EVAL;  // a batch is pending: s.path_len paths
    }
    s.leaf_node = 0;
    s.path_len = paths;
    const bool need = r_kind == AZH_LEAF_EVAL || r_kind == AZH_LEAF_ROOT;
    if (P.random_symmetry != 0u && lane < K && need) {
        // the evaluator sees the image of every slot's position; lane p owns slot p, so each lane transforms its own two
        // words in registers (symmetry_board: a loop over the stones; no LDS — the workgroup's other waves are at work)
        const int sy = eval_symmetry_of(P.eval_key[g], r_mover, r_opp);
        r_mover = symmetry_board(sy, r_mover);
        r_opp = symmetry_board(sy, r_opp);
    }
    if (lane < K) {
        V.kind[base + lane] = r_kind;
        V.leaf_edge[base + lane] = r_edge;
        V.leaf_node[base + lane] = r_node;
        V.path_len[base + lane] = r_len;
        P.need_eval[base + lane] = need ? 1 : 0;
        P.leaf_board[base + lane] = make_ulonglong2(r_mover, r_opp);
        if (P.pool)
            P.leaf_mask[base + lane] = P.slot_mask[g];
    }
    if (lane == 0) {
        P.gs[g] = s;
        if (over)
            P.force[g] = 1;
    }
    {
        const u64 inc = lane == AZH_STAT_STEPS ? st_steps
                      : lane == AZH_STAT_NN_EVALS ? st_evals
                      : lane == AZH_STAT_LEVELS ? st_levels
                      : lane == AZH_STAT_CHILDREN ? st_children
                      : lane == AZH_STAT_NEW_MOVES ? st_newmoves
                      : lane == AZH_STAT_EDGE_OVERFLOW ? (u64)over
                      : lane == AZH_STAT_COLLISIONS ? st_coll : 0ull;
        if (lane < NSTAT)
            add_stat(P, g, lane, inc);
    }
    return __ballot(lane < K && need);
}

// The priors of the batch's new nodes (wave w of the game's workgroup: paths w, w + VL_WAVES, ...) and of the root after
// its evaluation (wave 0).  Reads the state; changes nothing the other waves read.
__device__ inline void vl_backup_priors(const EngineParams &P, const VlParams &V, int g, const azh_game_state &s, int w, u32 pk)
{
    const size_t base = (size_t)g * V.K;
    Arena A = arena_of(P, s.arena, g);
    if (s.leaf_kind == AZH_LEAF_ROOT) {
        if (w == 0)
            apply_priors(P, A, 0, P.logits + base * AZH_POLICY_SIZE, (pk & PLY_FULL) != 0u, s.uid, (u32)s.ply,
                         eval_symmetry_at(P, A, g, 0));
        return;
    }
    if (s.leaf_kind != AZH_LEAF_EVAL)
        return;
    for (int p = w; p < s.path_len; p += VL_WAVES)
        if (V.kind[base + p] == AZH_LEAF_EVAL) {
            const int node = V.leaf_node[base + p];
            apply_priors(P, A, node, P.logits + (base + p) * AZH_POLICY_SIZE, false, 0u, 0u, eval_symmetry_at(P, A, g, node));
        }
}

// The proof pass (azh_engine_set_solver; DESIGN.md "Proven wins and losses"; tests/solver_reference.py restates it), run by
// the backup's wave after vl_backup_edges.  A node is DECIDED if it is a finished position or PROVEN; both are stored the
// same way — the node's value (the bits of +1.0f: its side to move wins, -1.0f: it loses) in node_info.w, and the
// "finished" bit of the range word of the edge that leads to it — so select ends a path there and the backup reads its
// value exactly as it does for a finished position; a proven node keeps its edge count in that word and its result bits 0
// (the game is not over: reroot_game copies both words as they are, and the root is descended from whatever its own mark).
// For every TERMINAL path whose last node became decided in this batch (`fresh`: a finished position the batch created; a
// hit of a position settled earlier proves nothing new, its parent was tested then) in path order, from the parent X of
// the path's last node upwards: X is a proven win if a child
// of X is decided with -1, a proven loss if every edge of X has a child decided with +1 (one 16-byte load per child,
// lane-striped like select's level, the decided children's values gathered behind it, one ballot each); when X becomes
// proven the walk goes on with X's parent, else — or when X was decided already — it stops.  A mark is made visible to the
// loads of the next step and of the next path by a workgroup-scope fence (same wave, same CU), like a path's virtual loss.
// `kind`, `len`, `leaf`, `fresh`: lane p's path.  W and n are never touched.
__device__ inline void vl_prove(const EngineParams &P, const VlParams &V, int g, const Arena &A, int k, int kind, int len, int leaf,
                                bool fresh)
{
    const int lane = lane_id();
    const size_t base = (size_t)g * V.K;
    const bool term = lane < k && kind == AZH_LEAF_TERMINAL && len > 0;
    const bool walk = term && fresh;
    bool hit = false;  // a path that ended at a proven node (not a finished position)
    if (term && !fresh)
        hit = (A.ni[leaf].y >> 16) == 0u;
    const u64 st_hits = (u64)__popcll(__ballot(hit));
    u64 st_nodes = 0;
    const uint4 rinfo = A.ni[0];
    const u32 root_kid = pack_kid(rinfo.x, rinfo.y & 0xFFFFu, 0u);
    bool root_decided = (rinfo.y >> 16) != 0u || (rinfo.w & 0x7FFFFFFFu) == 0x3F800000u;
    __threadfence_block();
    wave_sync();
    for (u64 todo = __ballot(walk); todo; todo &= todo - 1ull) {
        const int p = __ffsll((long long)todo) - 1;
        const int *path = V.path + (base + (size_t)p) * V.path_cap;
        for (int d = read_lane(len, p) - 1; d >= 0; d--) {
            // X: the node at depth d of the path — the root, or the child of the path's edge d - 1
            u32 x = 0, xkid = root_kid, pe = 0;
            if (d > 0) {
                pe = (u32)__builtin_amdgcn_readfirstlane(path[d - 1]);
                const uint2 pr = reinterpret_cast<const uint2 *>(&A.ed[pe])[1];
                x = (u32)__builtin_amdgcn_readfirstlane((int)(pr.x >> 16));
                xkid = (u32)__builtin_amdgcn_readfirstlane((int)pr.y);
                if (kid_finished(xkid))
                    break;  // proven by an earlier path of this batch
            } else if (root_decided) {
                break;
            }
            const int M = kid_count(xkid);
            const u32 first = kid_first(xkid);
            bool loses = false, open = false;  // among this lane's children: one decided with -1; one not decided with +1
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = lane + 64 * r;
                if (j < M) {
                    const uint4 ev = A.ed[first + j];
                    const u32 c = edge_child(ev);
                    if (c != ENONE && kid_finished(ev.w)) {
                        if (A.ni[c].w >> 31)
                            loses = true;
                    } else {
                        open = true;
                    }
                }
            }
            const bool win = __ballot(loses) != 0ull;
            if (!win && (M == 0 || __ballot(open) != 0ull))
                break;
            if (lane == 0) {
                reinterpret_cast<u32 *>(&A.ni[x])[3] = f2u(win ? 1.0f : -1.0f);
                if (d > 0)
                    reinterpret_cast<u32 *>(&A.ed[pe])[3] = xkid | 0x80000000u;
            }
            if (d == 0)
                root_decided = true;
            st_nodes += 1;
            __threadfence_block();
            wave_sync();
        }
    }
    if (lane == 0 && (st_nodes | st_hits)) {
        V.proofs[(size_t)g * 2 + AZH_PROOF_STAT_NODES] += st_nodes;
        V.proofs[(size_t)g * 2 + AZH_PROOF_STAT_HITS] += st_hits;
    }
}

// The batch's edge backup (one wave; lane p = path p).  Level by level — the paths that share an edge share it at the
// same depth — every edge gets ONE read-modify-write: W plus the scores of the EVAL and TERMINAL paths through it in path
// order (f32, the oracle's per-level inversion), visits plus those paths minus every path's virtual loss.
// `vl`: the virtual loss of the ply's search (the select that made the batch put it on).
__device__ inline void vl_backup_edges(const EngineParams &P, const VlParams &V, int g, azh_game_state &s, int vl)
{
    const int lane = lane_id();
    if (s.leaf_kind == AZH_LEAF_ROOT) {
        s.phase = 1;
        s.leaf_kind = AZH_LEAF_NONE;
        return;
    }
    if (s.leaf_kind != AZH_LEAF_EVAL)
        return;
    const int k = s.path_len;
    const size_t base = (size_t)g * V.K;
    Arena A = arena_of(P, s.arena, g);
    int kind = AZH_LEAF_NONE, len = 0, leaf = 0;
    float v = 0.0f;
    if (lane < k) {
        kind = V.kind[base + lane];
        len = V.path_len[base + lane];
        leaf = V.leaf_node[base + lane];
        if (kind == AZH_LEAF_EVAL)
            v = P.values[base + lane];
        else if (kind == AZH_LEAF_TERMINAL)
            v = u2f(A.ni[leaf].w);
    }
    const bool counted = kind == AZH_LEAF_EVAL || kind == AZH_LEAF_TERMINAL;
    // step() part 4 (:449-459), as backup_game: the score seen from the edge `flips` levels above the leaf
    const float sc0 = (v + 1.0f) * 0.5f;
    const float fa = 1.0f - sc0, fb = 1.0f - fa, fc = 1.0f - fb;
    const int *path = V.path + (base + (size_t)(lane < k ? lane : 0)) * V.path_cap;
    const int maxlen = (int)wave_max_u32((u32)len);
    bool fresh = false;  // the path's last edge had no visit before this batch: its child was created by the batch
    for (int d = 0; d < maxlen; d++) {
        const bool on = d < len;
        const u32 e = on ? (u32)path[d] : NONE;
        const int flips = len - d;
        const float val = flips == 1 ? fa : ((flips & 1) ? fc : fb);
        u32 *rec = reinterpret_cast<u32 *>(&A.ed[on ? e : 0u]);
        float W = 0.0f;
        u32 z = 0;
        if (on) {
            W = u2f(rec[1]);
            z = rec[2];
        }
        bool leader = on;
        u32 adds = 0, paths = 0;
        for (int q = 0; q < k; q++) {
            const u32 eq = (u32)read_lane((int)e, q);
            const int cq = read_lane((int)counted, q);
            const float vq = u2f((u32)read_lane((int)f2u(val), q));
            if (on && eq == e) {
                leader = leader && q >= lane;
                paths += 1;
                if (cq) {
                    W = W + vq;
                    adds += 1;
                }
            }
        }
        if (on && d == len - 1)
            fresh = (z & 0xFFFFu) == (u32)vl * paths;
        if (leader) {
            rec[1] = f2u(W);
            rec[2] = z + adds - (u32)vl * paths;  // (visits: the low half; never borrows from the child id)
        }
    }
    s.root_visits += (int)wave_sum_u32((counted && len > 0) ? 1u : 0u);
    if (V.solver)
        vl_prove(P, V, g, A, k, kind, len, leaf, fresh);
    s.leaf_kind = AZH_LEAF_NONE;
    s.path_len = 0;
}

// The tree phase of a leaf-parallel iteration as ONE launch, one workgroup of VL_WAVES waves per game: backup (priors by
// every wave, edges by wave 0) -> "is the move due?" -> the next batch's select (wave 0) -> need bits, and the workgroup
// that finishes last compacts the leaf list over the G * K slots.  mode bit 0: backup + mark, bit 1: select (+ compaction).
__global__ __launch_bounds__(VL_WAVES * WAVE) void k_vl_tree(EngineParams P, VlParams V, int mode)
{
    __shared__ u16 s_moves[MAX_MOVES];
    __shared__ int s_cnt[2 * VL_WAVES];
    __shared__ int s_last;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = blockIdx.x;
    azh_game_state s = P.gs[g];
    const int forced = P.force[g];
    const u32 pk = ply_kind_of(P, g);
    PlySearch S = engine_search(P, V, pk);
    if (w == 0)
        set_search(P, g, s, S);  // (the other waves compute priors: none of these values)
    if (mode & 1) {
        vl_backup_priors(P, V, g, s, w, pk);
        if (w == 0)
            vl_backup_edges(P, V, g, s, S.vl);
        __threadfence_block();
        __syncthreads();
    }
    u64 need = 0;
    if (w == 0) {
        if (mode & 1)
            mark_game_at(P, g, s, forced, S.visits);
        if (mode & 2)
            need = vl_select_game(P, V, g, s, s_moves, S);  // stores the state
        else if (lane_id() == 0)
            P.gs[g] = s;
    }
    if (!(mode & 2))
        return;
    if (threadIdx.x == 0) {
        // the game's need bits (slots g K .. g K + K - 1) into the mask, word by word
        const size_t b0 = (size_t)g * V.K;
        u32 seen = 0;
        for (int done = 0; done < V.K;) {
            const size_t bit = b0 + (size_t)done;
            const int off = (int)(bit & 31);
            const int take = min(32 - off, V.K - done);
            const u32 bits = (u32)(need >> done) & (take == 32 ? 0xFFFFFFFFu : ((1u << take) - 1u));
            if (bits)
                seen |= __hip_atomic_fetch_or(&P.need_mask[bit >> 5], bits << off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            done += take;
        }
        s_last = last_tree_workgroup(P, seen);
    }
    __syncthreads();
    if (s_last)
        compact_leaves<VL_WAVES>(P, 0, s_cnt);
}

}  // namespace azh
