/*
 * ataxxzero_hip.h — C ABI of the MI355X-native batched Ataxx self-play engine.
 *
 * Drop-in boundary for the reference's self-play hot path.  Plain C types only
 * (pointers, sizes, ints); no torch / Python objects cross this line.  All
 * `azh_*` functions return 0 on success and a negative code on failure, with a
 * message available from azh_last_error().  Host pointers are caller-owned and
 * are fully consumed (copied) before the call returns unless stated otherwise.
 *
 * Each entry point names the reference interface it replaces (file:line under
 * /root/reference).  The binding a maintainer of the reference would add is in
 * INTEGRATION.md; the Python side of this repo binds it in ataxxzero_amd/link.py.
 *
 * Bit conventions (cpp/bitboards.hpp:9-25, cpp/ataxx.hpp:28-34): square =
 * file + 7*rank0, a1 = bit 0.  A packed board is two u64: word0 = x stones with
 * the side to move in bit 63 (0 = x, 1 = o), word1 = o stones.  A "leaf board"
 * is (mover stones, opponent stones).  A move is u16 = from | to << 8, clone
 * <=> from == to (cpp/move.hpp:9-33).  Policy rows are the reference's
 * (7,7,17) f32 logits, flat index 119*to_x + 17*to_y + layer
 * (cpp/self_play_client.cpp:220-237); feature rows are (7,7,4) f32
 * (cpp/self_play_client.cpp:174-202).
 */
#ifndef ATAXXZERO_HIP_H
#define ATAXXZERO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZH_POLICY_SIZE 833
#define AZH_FEATURE_SIZE 196
#define AZH_MAX_MOVES 256
#define AZH_STAT_COUNT 16

enum { AZH_DTYPE_F32 = 0, AZH_DTYPE_BF16 = 1, AZH_DTYPE_F16 = 2 };
enum { AZH_LEAF_NONE = 0, AZH_LEAF_EVAL = 1, AZH_LEAF_TERMINAL = 2, AZH_LEAF_ROOT = 3, AZH_LEAF_DESCENT = 4,
       AZH_LEAF_COLLISION = 5 /* leaf-parallel search: the path met a node an earlier path of its batch created */ };

/* ------------------------------------------------------------------ errors */
const char *azh_last_error(void);
/* number of visible HIP devices, or a negative code when the runtime is unusable */
int azh_device_count(void);
/* select the device used by every later call from this process (one process per GPU) */
int azh_set_device(int device);
/* PCI bus id ("0000:05:00.0") of HIP device `device`: bench.py --gpus N prints it per rank, so that two ranks on one card
 * (or a straggling card) can be told from the aggregate line. */
int azh_device_pci_bus_id(int device, char *buf, int cap);

/* ------------------------------------------------------------------ rules
 * Replaces cpp/movegen.cpp:10-79 (movegen), cpp/makemove.cpp:56-76 (makemove),
 * cpp/self_play_client.cpp:109-144 (get_board_result) and perft.py:5-26. */

/* perft node count on the GPU with perft.py's "a position without a move has one
 * pass child" semantics. */
int azh_perft(uint64_t x, uint64_t o, uint64_t blockers, int turn, int depth, uint64_t *nodes_out);

/* For n packed boards: legal moves in the reference's movegen order
 * (moves_out [n][AZH_MAX_MOVES], zero past a row's count), their count, and
 * the adjudication 0 / 1 / 2.  Any output pointer may be NULL. */
int azh_rules_batch(int n, const uint64_t *boards, uint64_t blockers, uint16_t *moves_out,
                    int32_t *counts_out, int32_t *results_out);

/* boards_out[i] = makemove(boards[i], moves[i]); a move of 0xFFFF passes
 * (ataxx_rules.py:112-114). */
int azh_makemove_batch(int n, const uint64_t *boards, const uint16_t *moves, uint64_t *boards_out);

/* Reference feature rows (cpp/self_play_client.cpp:174-202, engine.py:53-73) for n
 * leaf boards (mover, opponent): out [n][7][7][4] f32. */
int azh_features_batch(int n, const uint64_t *leaf_boards, uint64_t blockers, float *out);

/* Uniform-random playouts (generate_games.py:16-75 with --random-play): plays
 * n_games games from the given start to the end or max_plies.  Outputs, all
 * optional: plies[n], results[n] (0 = unfinished), and the per-ply trace
 * boards_out [n][max_plies][2] (x, o), moves_out [n][max_plies]. */
int azh_random_play(int n_games, uint64_t seed, uint64_t x, uint64_t o, uint64_t blockers, int turn,
                    int max_plies, int32_t *plies, int32_t *results, uint64_t *boards_out,
                    uint16_t *moves_out);

/* ------------------------------------------------------------------ alpha-beta search
 * A depth-limited material search without a net: the teacher of generate_games.py --supervised-depth and the fixed
 * opponent of tools/anchor_match.py ("Alpha-beta search").  With result(p) the adjudication and moves(p) the
 * move order of azh_rules_batch, value(p, d), an integer seen from the side to move, is
 *   1. result(p) != 0: +(1000 + d) when the side to move has won, -(1000 + d) otherwise;
 *   2. d == 0: the stones of the side to move minus the opponent's;
 *   3. else the maximum over m in moves(p) of -value(makemove(p, m), d - 1),
 * and best(p, d) is the FIRST move of moves(p) that reaches value(p, d); a finished root has the move 0xFFFF and the value
 * of rule 1.  The search deepens d = 1 .. depth and counts nodes: the positions value was entered on, roots excluded,
 * summed over the iterations.  node_budget > 0: an iteration during which the count passes the budget is abandoned and the
 * last completed one is reported (depth 1 always completes: node_budget >= AZH_MAX_MOVES); node_budget == 0, no limit, is
 * accepted up to depth AZH_ALPHABETA_UNBOUNDED_DEPTH.  depth outside 1 .. AZH_ALPHABETA_MAX_DEPTH, a refused budget and a
 * board whose stones or walls overlap: -2. */
#define AZH_ALPHABETA_MAX_DEPTH 8
#define AZH_ALPHABETA_UNBOUNDED_DEPTH 3

/* n packed boards (as azh_rules_batch), one wave each, pruned; every root on `blockers`, or root i on
 * blockers_per_board[i] when that is not NULL.  Outputs, all optional: moves_out[n] = best, values_out[n] = value,
 * depth_done_out[n] = the iteration reported, nodes_out[n]. */
int azh_alphabeta_search(int n, const uint64_t *boards, uint64_t blockers, const uint64_t *blockers_per_board, int depth,
                         uint64_t node_budget, uint16_t *moves_out, int32_t *values_out, int32_t *depth_done_out,
                         uint64_t *nodes_out);

/* The same for one position as a plain negamax on the host: no pruning, no device.  Its node count is the definition's
 * own, so under a budget it may complete fewer iterations than the device does.  Outputs optional. */
int azh_alphabeta_host(uint64_t x, uint64_t o, uint64_t blockers, int turn, int depth, uint64_t node_budget,
                       uint16_t *move_out, int32_t *value_out, int32_t *depth_done_out, uint64_t *nodes_out);

/* Teacher games (generate_games.py:26-57 with --supervised, the engine being this search): n_games games from (x, o, turn)
 * on `blockers`, or game g from the packed board starts[2g .. 2g+1] and on blockers_per_game[g] where those are not NULL.
 * At every ply the training move is best(p, depth) under the budget; the move played is replaced by legal move number
 * (v[1] * M) >> 32 of the M legal moves when v[0] < random_per_2_32[ply], v = philox(seed; game, ply, 9, 0); plies from
 * n_schedule on are never replaced.  One launch per ply.  Outputs, all optional, as azh_random_play: plies[n], results[n]
 * (0 = unfinished at max_plies), boards_out [n][max_plies][2] (x, o), training_moves_out and played_moves_out
 * [n][max_plies]. */
int azh_alphabeta_play(int n_games, uint64_t seed, uint64_t x, uint64_t o, uint64_t blockers, int turn,
                       const uint64_t *starts, const uint64_t *blockers_per_game, int depth, uint64_t node_budget,
                       const uint32_t *random_per_2_32, int n_schedule, int max_plies, int32_t *plies, int32_t *results,
                       uint64_t *boards_out, uint16_t *training_moves_out, uint16_t *played_moves_out);

/* Test hook for the engine's deterministic f32 math / Philox4x32-10 (the arithmetic
 * the search's bit-exact contract with the CPU oracle rests on).  kind 0: exp(in[i]);
 * 1: log(in[i]); 2: gamma(alpha = in[0]) keyed (seed, aux[3i..3i+2] = uid, ply, edge);
 * 3: philox(seed; aux[4i..4i+3]) -> out[4i..4i+3].  out holds raw 32-bit patterns. */
int azh_probe_detmath(int kind, int n, const float *in, const uint32_t *aux, uint64_t seed, uint32_t *out);

/* ------------------------------------------------------------------ network
 * Replaces model.Network's forward pass (model.py:38-79,116-142) and
 * model.load_model (model.py:186-196). */
typedef struct azh_net azh_net;

/* conv_flat: the 2*blocks+5 parameter arrays of the .npy file's first list,
 * concatenated in file order: (3,3,4,F), 2*blocks x (3,3,F,F), (1,1,F,17),
 * (1,1,F,1), fc_w (49,1), fc_b (1,).  bn_flat: the 2*(2*blocks+1) arrays of the
 * second list, (moving_mean, moving_variance) per batch-norm in creation order.
 * gamma = 1, beta = 0 as after model.load_model;
 * bn_eps is TensorFlow's default 1e-3.  filters: 128 (model.py:16; the tuned towers), 64 or 256 (model.Network.FILTERS
 * is a class attribute that uai_interface.py:92-93 patches: these run on the width-templated 32x32 tower).
 * A tower whose numbers are not finite is refused, not run: -2, with a message that names the tower layer, when a tower
 * convolution weight, a batch-norm mean, or a derived batch-norm scale 1 / sqrt(var + eps) or shift -mean * scale is a NaN or
 * an infinity (var + eps <= 0 is the usual cause).  The check needs no device and comes before the device is asked for.  The
 * policy and value 1x1 heads, fc_w and fc_b are not restricted: an infinity there gives infinite logits, values of +-1 and
 * NaNs exactly where IEEE arithmetic puts them, in every tower. */
int azh_net_create(int blocks, int filters, const float *conv_flat, const float *bn_flat,
                   float bn_eps, azh_net **out);
void azh_net_destroy(azh_net *net);

/* The forward pass of n leaf boards (mover, opponent): logits_out [n][833] f32 (raw policy logits, model.py:66-69), values_out
 * [n] (tanh value, model.py:71-79).  Null arguments and n < 0: -1; a mode outside the enum: -2.
 * A net with a finite tower weight that `dtype` rounds to an infinity after the batch-norm scale is folded in (70000 in f16):
 * -2, the message names the layer; nothing is launched and nothing allocated, and the net goes on serving the dtypes that
 * hold it.  (The engine's launches pass the same refusal on.)  Activations may still overflow from finite weights: an f16
 * activation of 65520 or more is +inf, and the layers after it carry infinities and NaNs as IEEE arithmetic has them — ReLU
 * keeps a NaN and +inf and turns -inf into 0 — identically in every tower kernel (tests/test_gpu_net_edges.py) but one family:
 * the bf16 16x16x32 towers (k_tower2<bf16>, k_tower2_thin<bf16>, k_tower2_pair<bf16>: the default bf16 path at 128 filters)
 * take ReLU as an integer max on the bit pattern and turn a NaN activation into 0, so a bf16 net whose f32 accumulators
 * overflow goes on with finite numbers there where f32, f16 and the 32x32 towers (AZH_TOWER=1) report NaN.
 * mode: AZH_FORWARD_PLAIN, the ordinary tower, or
 *   AZH_FORWARD_THIN   THIN batches (a match's last games, a UAI engine's single position): the 16-bit towers with ONE board
 *     per workgroup — the latency of a launch of a handful of boards is one workgroup's time for the 25 layers, and a board
 *     alone in its workgroup needs 288 MFMAs per wave and layer instead of the 3-board workgroup's 720.  Same net, same boards
 *     -> the same logits and values up to the summation order (the last bits of the 16-bit towers differ from the 3-board
 *     kernel's); f32 and other widths run the ordinary tower.
 *   AZH_FORWARD_SYM    test-time symmetry averaging, nn_evals.evaluate (nn_evals.py:48-62): the tower runs the 8 dihedral
 *     images of every board in one launch; logits come back through the inverse symmetry (spatially) and are averaged,
 *     values are averaged.
 * Walls: `blockers` is the wall mask of every board, unless blockers_per_board [n] is given (bits beyond the 49 cells: -2, the
 * message names the board): then board i is evaluated with the wall plane of its own mask, in the same launch as the others —
 * what the engine's loop does under a start pool (azh_engine_set_start_pool).  A board's rows are bit for bit those of the
 * same launch with that board's mask for every board.  blockers_per_board = NULL and blockers = 0: no walls anywhere.  Both
 * given (a mask array and blockers != 0) is two sources for one plane: -2. */
enum { AZH_FORWARD_PLAIN = 0, AZH_FORWARD_THIN = 1, AZH_FORWARD_SYM = 2 };
int azh_net_forward(azh_net *net, int dtype, int mode, int n, const uint64_t *leaf_boards, uint64_t blockers,
                    const uint64_t *blockers_per_board, float *logits_out, float *values_out);
/* Measurement hook: average HIP-event milliseconds per launch of the tower kernel (mode: AZH_FORWARD_PLAIN or _THIN, else
 * -2) over n synthetic boards (iters launches on one stream, 3 untimed warm-up launches). */
int azh_net_bench(azh_net *net, int dtype, int mode, int n, int iters, float *ms_out);
/* Which tower kernel a launch runs (host arithmetic, no GPU needed): the library's one dispatch function, asked without a
 * launch.  stamped: azh_net_stamps; pair: the arena's two-net launch; variant1: AZH_TOWER=1; six_boards: AZH_TOWER_BOARDS=6;
 * lds_range_ok: what azh_net_create's probe of the device found (1 where the towers were built for, and with -DAZH_OOBZERO=0).
 * 0: *out is filled (the instantiation's name; boards, threads and dynamic LDS bytes per workgroup, workgroups per CU);
 * -2: the launch would be refused; 1 (pair only): no pair kernel here, the two nets are launched one after the other. */
typedef struct { char kernel[64]; int32_t boards, threads, lds_bytes, per_cu; } azh_tower_choice;
int azh_net_tower_choice(int filters, int dtype, int thin, int stamped, int pair, int variant1, int six_boards,
                         int lds_range_ok, azh_tower_choice *out);
/* Diagnostic build of the bf16 tower with s_memtime stamps per layer phase: copies the
 * stamps of the first `wgs` workgroups, [wg][wave][128] u64, to out (layout: net_kernels.hip). */
int azh_net_stamps(azh_net *net, int n, int wgs, uint64_t *out);

/* ------------------------------------------------------------------ engine
 * Replaces the worker threads of cpp/self_play_client.cpp: MCTS::step (:419-473),
 * Evaluations::populate (:153-272), MCTS::play (:475-492),
 * sample_proportionally_to_visits (:495-506), generate_game (:508-582). */
typedef struct azh_engine azh_engine;

typedef struct {
    int32_t games;           /* concurrent game slots ("threads" in the reference) */
    int32_t visits;          /* global_visits (:46,:522) */
    int32_t max_plies;       /* maximum_game_plies (:34) */
    int32_t edges_per_node;  /* edge arena per game = (visits + 8) * edges_per_node */
    float c_puct;            /* exploration_parameter (:31) */
    float dirichlet_alpha;   /* (:32) */
    float dirichlet_weight;  /* (:33) */
    int32_t start_turn;
    uint64_t seed;
    uint64_t start_x, start_o, blockers; /* STARTING_GAME_POSITION (:23) */
    uint32_t flags;          /* AZH_FLAG_*; 0 = the C++ self-play generator's behaviour */
    uint32_t select_budget;  /* 0 = every descent finishes inside one select; k > 0 = at most k tree levels per
                                select: a deeper descent parks (AZH_LEAF_DESCENT, no leaf this iteration) and
                                resumes next iteration where it stopped.  A parked game's tree does not change in
                                between, so each game plays bit for bit what it plays with budget 0; the launch no
                                longer lasts as long as the deepest descent of the batch */
} azh_config;

/* Behaviour switches that turn the self-play search into the arena search, i.e. the
 * Python engine the reference's uai_ringmaster.py drives (engine.py, uai_interface.py): */
enum {
    AZH_FLAG_NO_REUSE = 1,        /* fresh tree every ply: with per-ply "moves" messages engine.set_state
                                     (engine.py:452-472) never finds its grand-child and rebuilds the tree */
    AZH_FLAG_TIE_FIRST = 2,       /* python max(): first maximal move (engine.py:291), not the C++ last (:354) */
    AZH_FLAG_PY_POSTERIOR = 4,    /* 833-way softmax, gather, / (sum_legal + 1e-6) (engine.py:197-203) */
    AZH_FLAG_SAMPLE_POW5 = 8,     /* move ~ (n/N)^5 over edges with n >= max/2 (engine.py:532-548, exponent 5
                                     at uai_interface.py:76-79) */
    AZH_FLAG_KEEP_UNFINISHED = 16,/* games cut at max_plies are reported with result 0 ("invalid" ->
                                     annulled, uai_ringmaster.py:147-150) instead of dropped */
    AZH_FLAG_TWO_NETS = 32,       /* arena: the side to move alternates between two nets; slot parity picks
                                     which net plays x; records carry "slot" and "uid" */
    AZH_FLAG_ARENA = 1 | 2 | 4 | 8 | 16 | 32,
    AZH_FLAG_SYMMETRY_AVG = 128,  /* every evaluation is nn_evals.evaluate (nn_evals.py:48-62): the mean over the 8
                                     dihedral symmetries of the board, logits brought back spatially (move-type
                                     layers not permuted, as the reference), values averaged; 8x the tower work */
    AZH_FLAG_EVAL_CACHE = 256,    /* engine.py's NNEvaluator.cache (engine.py:127-234) for the device loop: a position this
                                     game's search has already evaluated (a transposition, a re-visited position: about
                                     a quarter of the leaves at 400 sims/move) takes its priors and value from the node
                                     that carries them instead of going to the net again.  Off by default: the C++
                                     generator evaluates every new node.  The net being deterministic, the trees are the
                                     ones the uncached search builds; AZH_STAT_NN_EVALS falls, AZH_STAT_CACHE_HITS counts */
    AZH_FLAG_ONE_RANDOM_MOVE = 64 /* the ONE_RANDOM_MOVE build of the client (cpp/self_play_client.cpp:515-552):
                                     per game one ply in 0..119 plays a uniformly random legal move, every later
                                     ply the most visited move; the entry gains "random_ply" (train.py:47-49) */
};

typedef struct {
    int32_t phase, arena, n_nodes, n_edges, ply, root_visits, leaf_kind, leaf_node, path_len;
    uint32_t uid;
} azh_game_state;

enum {
    AZH_STAT_STEPS = 0, AZH_STAT_NN_EVALS, AZH_STAT_LEVELS, AZH_STAT_CHILDREN, AZH_STAT_NEW_MOVES,
    AZH_STAT_PLIES, AZH_STAT_GAMES, AZH_STAT_DROPPED, AZH_STAT_EDGE_OVERFLOW, AZH_STAT_REROOT_NODES,
    AZH_STAT_REROOT_EDGES, AZH_STAT_RING_OVERFLOW, AZH_STAT_CACHE_HITS,
    AZH_STAT_PARKED,        /* (game, iteration) pairs in which a descent was parked by select_budget */
    AZH_STAT_REROOT_SPILLS, /* re-roots whose breadth-first frontier outgrew its LDS queue (the rest went through HBM) */
    AZH_STAT_COLLISIONS     /* leaf-parallel search: paths that ended at a node created earlier in their batch */
};

typedef struct {
    /* sums of HIP-event elapsed milliseconds over the iterations SAMPLED since the last azh_engine_timing_reset
     * (every `enable`-th iteration of the device loop, events on the engine's stream), and the number of samples */
    double select_ms, net_ms, backup_ms; /* select_ms: the fused tree launch of the run loop (backup + advance +
                                            select + compaction); backup_ms: 0 there */
    int64_t iterations;
    int64_t net_evals; /* leaves evaluated by the net in those iterations */
} azh_timing;

int azh_engine_create(const azh_config *cfg, azh_engine **out);
void azh_engine_destroy(azh_engine *e);
int azh_engine_node_cap(const azh_engine *e);
int azh_engine_edge_cap(const azh_engine *e);

/* One search iteration = select -> evaluate -> backup.
 * select: PUCT descent + expansion in every game (one new leaf per game). */
int azh_engine_select(azh_engine *e, int32_t *n_leaves_out);
/* need_eval [G], leaf_boards [G][2] (mover, opponent); either may be NULL */
int azh_engine_leaves(azh_engine *e, int32_t *need_eval, uint64_t *leaf_boards);
/* the reference's request_evaluation role (:648-681): feature rows of the current leaf
 * batch, dense, in game order: out [n_leaves][7][7][4] f32; games_out [n_leaves]
 * (optional) = the game each row belongs to */
int azh_engine_leaf_features(azh_engine *e, float *out, int32_t *games_out);
/* evaluate the leaf batch on the device with the built-in net */
int azh_engine_eval(azh_engine *e, azh_net *net, int dtype);
/* or supply evaluations from outside (the reference's complete_workload role,
 * :723-738): host arrays indexed by game, logits [G][833], values [G] */
int azh_engine_set_evals(azh_engine *e, const float *logits, const float *values);
/* priors (+ root Dirichlet), backup, and — once the root has `visits` visits —
 * sample the move, record the ply, re-root, finish/restart games */
int azh_engine_backup(azh_engine *e);

/* `iterations` full iterations with the built-in net, enqueued asynchronously */
int azh_engine_run(azh_engine *e, azh_net *net, int dtype, int iterations);
/* the same run for n engines of one GPU (half-batches: the reference's double buffer, cpp/self_play_client.cpp:593-600),
 * their iterations enqueued in turn, so that all of them start with the first launches enqueued */
int azh_engines_run(azh_engine *const *engines, int n, azh_net *net, int dtype, int iterations);
/* arena (AZH_FLAG_TWO_NETS): net_a plays x in even slots and o in odd slots, net_b the
 * other way round (uai_ringmaster.py:241-247 queues every pairing both ways).  Per iteration the leaves whose mover is net_a and
 * those whose mover is net_b are evaluated by ONE launch of the 16-bit tower (each workgroup picks its weight set from the list
 * it serves; the nets may differ in depth; f32, other widths and AZH_FLAG_SYMMETRY_AVG: one launch per net), with results bit
 * for bit those of separate launches.  A match is a fixed cohort under azh_engine_set_game_limit, and its last games want
 * azh_engine_set_thin_batches (below). */
int azh_engine_run_arena(azh_engine *e, azh_net *net_a, azh_net *net_b, int dtype, int iterations);
int azh_engine_sync(azh_engine *e);
/* change the root-visit threshold (global_visits) for the coming moves; 1 <= visits <= the
 * value the engine was created with */
int azh_engine_set_visits(azh_engine *e, int visits);
/* SEARCH MODES: WHO REFUSES WHOM.  Ten modes.  Nine modes are switched by setters below, each by values of its own, and the
 * tenth by a table of search sets (azh_engine_set_search_sets); all of them before the first select or between iterations.
 * A call that switches a mode on is a request for it; one that switches it off is not, and is never refused for a reason in
 * this table.  Every one of these setters checks in this order, and changes nothing unless every check passes: -1 a null
 * engine, -2 a value out of range, -3 a selected batch awaits its backup (requests and switching off alike), -4 the request
 * is refused by a row of this table.
 *
 *   mode            is on while                 refused on an engine created with                         refused beside
 *   playout cap     fast_visits != 0            TWO_NETS, ONE_RANDOM_MOVE                                 Gumbel, search sets
 *   forced playouts k != 0                      TWO_NETS, ONE_RANDOM_MOVE                                 Gumbel, leaf batch, solver,
 *                                                                                                         exploration, search sets
 *   Gumbel          m != 0                      TWO_NETS, ONE_RANDOM_MOVE, SAMPLE_POW5, EVAL_CACHE;       playout cap, forced playouts,
 *                                               without NO_REUSE; dirichlet_weight != 0                   temperature, leaf batch, solver,
 *                                                                                                         exploration, search sets
 *   temperature     either table is set         TWO_NETS, ONE_RANDOM_MOVE, SAMPLE_POW5, PY_POSTERIOR      Gumbel
 *   resign          consecutive != 0            TWO_NETS, ONE_RANDOM_MOVE                                 -
 *   random symmetry on != 0                     TWO_NETS, SYMMETRY_AVG; a blockers mask that is not its   -
 *                                               own image under all 8 symmetries
 *   leaf batch      leaves_per_game > 1         TWO_NETS, EVAL_CACHE, SYMMETRY_AVG; select_budget > 0     Gumbel, forced playouts
 *   solver          on != 0                     TWO_NETS, EVAL_CACHE, SYMMETRY_AVG; select_budget > 0     Gumbel, forced playouts
 *   exploration     fpu_reduction >= 0 ||       TWO_NETS, EVAL_CACHE, SYMMETRY_AVG; select_budget > 0     Gumbel, forced playouts
 *                   c_base > 0                                                                            (and search sets)
 *   search sets     n != 0                      TWO_NETS, ONE_RANDOM_MOVE, EVAL_CACHE, SYMMETRY_AVG;      Gumbel, forced playouts,
 *                                               select_budget > 0                                         playout cap, exploration
 *
 * The last column is symmetric: of two modes that exclude each other, whichever is asked for second is refused, and comes on
 * once the other is off.  Everything not listed composes.  The message (azh_last_error) is "<setter>: not supported with
 * <cause>", from azh_engine_set_leaf_batch and azh_engine_set_solver "<setter>: more than one leaf per game is not supported
 * with <cause>" / "<setter>: the solver is not supported with <cause>"; the cause is the flag (AZH_FLAG_...), "select_budget
 * > 0", the blockers mask, or the mode that is on with its setter: "the playout cap (azh_engine_set_playout_cap)", "forced
 * playouts (azh_engine_set_forced_playouts)", "the Gumbel root search (azh_engine_set_gumbel)", "a temperature table
 * (azh_engine_set_temperature)", "more than one leaf per game (azh_engine_set_leaf_batch)", "the solver", "first-play
 * urgency or a growing exploration rate (azh_engine_set_exploration)", "search settings per side
 * (azh_engine_set_search_sets)"; Gumbel on an engine
 * without NO_REUSE or with a dirichlet_weight says that the engine must have been created with both.  Where several causes
 * apply the message names one: a flag before anything else, in the order TWO_NETS, ONE_RANDOM_MOVE, SAMPLE_POW5, PY_POSTERIOR,
 * EVAL_CACHE, SYMMETRY_AVG, then the other create-time causes, then the modes, Gumbel first, the pairs of the search sets
 * last.  The paragraphs below say why. */
/* Leaf-parallel search (an extension; the reference searches one leaf per tree at a time): every game selects up to
 * `leaves_per_game` = K leaves per iteration (1 <= K <= 64), spread over different lines by a virtual loss of
 * `virtual_loss` visits (1 .. 16) on every edge an earlier path of the batch took; the leaves of all games are evaluated
 * in one tower launch (slots g K + p; the thin tower while G K <= AZH_THIN_MAX_GAMES) and every path is backed up before
 * the next select.  Definition: DESIGN.md, "Leaf-parallel search".  Call before the first select or between iterations;
 * K = 1 restores the one-leaf search exactly.  K > 1 is refused with AZH_FLAG_TWO_NETS, AZH_FLAG_EVAL_CACHE,
 * AZH_FLAG_SYMMETRY_AVG and select_budget > 0 (the table above).  With K > 1, azh_engine_select / _eval / _backup / _run work on the
 * batch, azh_engine_leaves / _set_evals / _leaf_features / _tree_stamps return an error (their buffers are G-sized): use
 * the two calls below. */
int azh_engine_set_leaf_batch(azh_engine *e, int leaves_per_game, int virtual_loss);
/* kind [G K] (AZH_LEAF_NONE for an empty slot, _EVAL, _TERMINAL, _ROOT, _COLLISION), leaf_boards [G K][2] (mover,
 * opponent; zero unless the slot needs the net), leaf_edge [G K] (the last edge of the slot's path, 0xFFFFFFFF: none);
 * any pointer may be NULL */
int azh_engine_batch_leaves(azh_engine *e, int32_t *kind, uint64_t *leaf_boards, uint32_t *leaf_edge);
/* evaluations of the batch from outside, by slot: logits [G K][833], values [G K] */
int azh_engine_set_batch_evals(azh_engine *e, const float *logits, const float *values);

/* Playout cap randomization (an extension, off by default; the reference searches every ply with `visits`): most plies of
 * a game get a cheap search, a random share the full one, and only those are training targets (KataGo).  While it is on,
 * every ply of every game is FAST or FULL — FULL iff (philox(seed; uid, ply, 4, 0).v[0] >> 16) < full_per_65536, a pure
 * function of the engine's seed, the game's uid and the ply (azh_playout_cap_kind restates it on the host; stream 4 is
 * drawn from by nothing else, so no other random number moves).  A FULL ply's move is due at `visits` root visits and its
 * root priors get the Dirichlet mix, bit for bit those of the uncapped engine at the same uid, ply and position; a FAST
 * ply's move is due at `fast_visits` and its root priors are the plain posterior.  The leaf-parallel search's
 * k = max(1, min(K, T - root_visits)) uses the ply's own threshold T.  Every ply still begins with the root's evaluation: a
 * root that inherits `fast_visits` visits or more plays its FAST move right after it.  Sampling, re-root, evaluation cache,
 * select budget and the K-leaf search are unchanged.  The record of a game finished while the mode is on says so (bit 2 of
 * header word 7) and word 5 of each ply is 1 for a FULL ply: the game's line gains "full": [0,1,...], one entry per ply,
 * between "dists" and "moves".  Lines of an engine with the mode off are byte for byte what they were.
 * fast_visits = 0 switches the mode off; else 1 <= fast_visits <= visits and 0 <= full_per_65536 <= 65536 (65536: every
 * ply FULL, 0: none).  Call before the first select or between iterations.  Refused with AZH_FLAG_TWO_NETS (match play
 * searches every move alike) and AZH_FLAG_ONE_RANDOM_MOVE (the table above); while it is on azh_engine_set_visits refuses values below
 * fast_visits.  Definition and measurements: DESIGN.md, "Playout cap randomization". */
int azh_engine_set_playout_cap(azh_engine *e, int fast_visits, int full_per_65536);
/* The kind of ply `ply` of game `uid` of an engine created with `seed`: 1 FULL, 0 FAST.  Host arithmetic only, usable
 * without a device (trainers, tests). */
int azh_playout_cap_kind(uint64_t seed, uint32_t uid, uint32_t ply, uint32_t full_per_65536);

/* Forced playouts and policy target pruning (an extension, off by default; KataGo, "Accelerating Self-Play Learning in Go",
 * section 3.2).  k = 0 switches the mode off (the state after create), k > 0 on (KataGo: 2); k < 0 or NaN is refused.  The
 * mode acts on the plies whose root priors get the Dirichlet mix: every ply while the playout cap is off, the FULL plies
 * while it is on; FAST plies are searched and recorded as ever.  All f32 operations below are single IEEE operations in the
 * order written, sqrtf the correctly rounded one.
 * FORCED PLAYOUTS, at the root level of a fresh descent (not of one the level budget parked and that resumes): with
 * N = root_visits, P_j the prior of root edge j after the noise mix and n_j its visits, edge j is OWED iff n_j >= 1 and
 * (float)n_j < sqrtf((k * P_j) * (float)N).  If an edge is owed the descent takes an owed edge — the last in edge order, the
 * first under AZH_FLAG_TIE_FIRST — else the level is the PUCT level.  Below the root nothing changes; the root level counts
 * in the level budget and the counters as any level.
 * POLICY TARGET PRUNING, when the ply is recorded: the move is sampled from the raw visits and the tree is re-rooted exactly
 * as with the mode off (the game's trajectory does not depend on pruning; the played move may be absent from the ply's
 * dists); only the visit counts written into the record, and so the line's dists, change.  With sq = sqrtf((float)(1 + N)),
 * b the root edge with the most visits (ties: the lowest index) and S = ((sq / (1 + n_b)) * (c_puct * P_b)) + W_b / n_b, edge
 * b keeps n_b, and for every other edge j with n_j >= 1: f_j = (u32)floorf(sqrtf((k * P_j) * (float)N)), q_j = W_j /
 * (float)n_j, m = n_j; up to f_j times: if m >= 1 and ((sq / (1.0f + (float)(m - 1))) * (c_puct * P_j)) + q_j < S then m -= 1,
 * else stop; if m < n_j and m <= 1 then m = 0.  Edges with m = 0 are left out of the record; nd counts the written ones.
 * The record of a game finished while the mode is on carries bit 3 (value 8) in header word 7; its line has the usual keys.
 * Refused (the engine stays as it was) with AZH_FLAG_TWO_NETS and AZH_FLAG_ONE_RANDOM_MOVE, with more than one leaf per
 * game and with the solver; while the mode is on azh_engine_set_leaf_batch (K > 1) and azh_engine_set_solver (on) refuse in
 * turn (the table above).  Call before the first select or between iterations.  Definition and measurements: DESIGN.md, "Forced playouts and
 * policy target pruning". */
int azh_engine_set_forced_playouts(azh_engine *e, float k);
/* The visit counts the pruning above writes for a root of M edges — prior [M] (after the noise mix), W [M] total scores,
 * n [M] visits, N their sum — into out [M] (0: the edge is left out of the record).  Host arithmetic only, usable without a
 * device: the same per-edge function the device's ply record uses. */
int azh_forced_prune(const float *prior, const float *W, const uint32_t *n, int M, float k, float c_puct, uint32_t *out);

/* Gumbel root search with sequential halving (an extension, off by default; Danihelka et al., "Policy improvement by
 * planning with Gumbel", ICLR 2022).  m = 0 switches the mode off (the state after create); 1 <= m <= 256 on, with a finite
 * c_visit >= 0, a finite c_scale > 0 (mctx: 16, 50, 1) and m * visits <= 2^20.  All f32 operations below are single IEEE
 * operations in the order written; logf / expf are the library's deterministic ones (azh_probe_detmath); a "64-lane sum" has
 * lane l add its terms l, l + 64, ... in that order from 0 and combines the lanes by the xor butterfly 1, 2, 4, 8, 16, 32.
 * SCHEDULE: seq(r, V), the considered visit counts for r considered actions and V simulations.  r <= 1: 0, 1, .., V - 1.
 * Otherwise L = ceil(log2 r), k = r, visits[0..r) = 0, and while the sequence is shorter than V: extra = max(1, V / (L k));
 * `extra` times append visits[0..k) and add 1 to each of them; then k = max(2, k / 2).  The result is cut to V entries
 * (azh_gumbel_considered_visits).  azh_engine_set_visits rebuilds the engine's rows while the mode is on.
 * AT THE ROOT'S EVALUATION, for every root edge j < M: x = word 0 of philox(seed; uid, ply, stream 7, j),
 * u = ((float)(x >> 9) + 0.5f) * 2^-23, g_j = -logf(-logf(u)) (azh_gumbel_noise), l_j = P_j > 0 ? logf(P_j) : -inf with P_j the
 * prior as stored, a_j = g_j + l_j; and v0 = (value + 1.0f) * 0.5f of the root's own evaluation.
 * THE ROOT LEVEL of a fresh descent (not of one the level budget parked and that resumes): t = root_visits, r = min(m, M),
 * cv = seq(r, visits)[t], n_max = max_j n_j, ks = (c_visit + (float)n_max) * c_scale, s_j = n_j >= 1 ? a_j + ks * (W_j /
 * (float)n_j) : a_j.  The descent takes the edge with n_j == cv and the greatest s_j; a NaN never wins and equal scores go to
 * the lowest edge index whatever AZH_FLAG_TIE_FIRST says.  If no edge qualifies (or t >= visits, after azh_engine_set_visits
 * lowered the threshold under a ply) the level is the PUCT level.  Below the root nothing changes; the root level counts in
 * the level budget and the counters as any level.  On a fresh tree a candidate always exists and no more than min(m, M) root
 * edges are ever visited.
 * WHEN THE MOVE IS PLAYED (N = root_visits; n_max, ks, s_j on the final counts): the move is the edge with n_j == n_max and
 * the greatest s_j, the lowest index among equal ones (edge 0 if every such score is a NaN); no random number is drawn.  The
 * record carries the improved policy: q_j = W_j / (float)n_j over the visited edges, sp / sw the 64-lane sums of P_j / of
 * P_j * q_j over them (an unvisited edge adds 0), v_mix = sp > 0 ? (v0 + ((float)N / sp) * sw) / (1.0f + (float)N) : v0,
 * cq_j = n_j >= 1 ? q_j : v_mix, x_j = l_j + ks * cq_j, x_max their maximum, c_j = min((u32)(expf(x_j - x_max) * 65535.0f),
 * 65535).  Every root edge with c_j >= 1, EXPANDED OR NOT, is written as move | c_j << 16 in edge order and nd counts them,
 * so the line's dists — the counts over their sum — are softmax(logits + sigma(completedQ)) to 16 bits; its keys do not
 * change.  NO RECORD IS WITHOUT A TARGET: when no c_j is >= 1 — there is no finite greatest x_j: every prior is zero (a +inf
 * logit in the root's row, or a row of NaN), every visited W_j is a NaN, or ks * cq_j overflows, so every x_j - x_max is a
 * NaN and expf of a NaN is 0 — the record carries the move played with the count 65535 and nothing else (nd = 1).  The record of a game finished while the mode is on carries bit 6 (value 64) in header word 7.  The value recorded
 * under azh_engine_set_resign stays W_b / n_b of the most visited edge.  q is the engine's [0, 1] score (no min-max
 * rescaling), and below the root the search stays PUCT.
 * A ply whose root was evaluated before the mode came on is searched with a_j = 0 and v0 = 0.5: switch it on before the first
 * select, or accept that for the plies in progress.
 * Refused (the engine stays as it was) unless the engine was created with AZH_FLAG_NO_REUSE and dirichlet_weight 0; with
 * AZH_FLAG_TWO_NETS, _ONE_RANDOM_MOVE, _SAMPLE_POW5, _EVAL_CACHE; and while the playout cap, forced playouts, a temperature
 * table, more than one leaf per game or the solver is on — their setters refuse in turn while this mode is on.  Random symmetry
 * and azh_engine_set_resign stay allowed (the table above).  Definition and measurements: DESIGN.md, "Gumbel root search with sequential
 * halving". */
int azh_engine_set_gumbel(azh_engine *e, int m, float c_visit, float c_scale);
/* seq(m, visits) above, out [visits] (1 <= m <= 256, 1 <= visits <= 60000).  Host arithmetic only, usable without a device. */
int azh_gumbel_considered_visits(int m, int visits, uint16_t *out);
/* g_j above for the root edges j < M of ply `ply` of game `uid` of an engine created with `seed`, out [M].  Host arithmetic
 * only: the function the root's backup calls. */
int azh_gumbel_noise(uint64_t seed, uint32_t uid, uint32_t ply, int M, float *out);
/* The move and the written counts above for a root of M edges — prior [M], W [M] total scores, n [M] visits, the root's own
 * score v0 and noise [M] = g_j: counts_out [M] (0: the edge is left out of the record), *move_out the edge played.  Host
 * arithmetic only: the per-edge functions the device's ply record uses. */
int azh_gumbel_root(const float *prior, const float *W, const uint32_t *n, int M, float v0, const float *noise, float c_visit,
                    float c_scale, uint32_t *counts_out, int32_t *move_out);

/* Random symmetry per evaluation (an extension, off by default; AlphaGo Zero / AlphaZero evaluate every leaf under a random
 * dihedral symmetry, and so does the reference's symmetry variant of its Python engine).  While it is on, every position
 * that goes to the evaluator — new leaves and the root's evaluation at the start of a ply — goes as its image T_s(mover),
 * T_s(opponent) under one symmetry s of the board, and the prior of every edge is gathered from the logit of T_s(move); the
 * value is used as it comes (under AZH_FLAG_PY_POSTERIOR the 833-way softmax sums the image's logits in the position's index
 * order, azh_symmetry_policy_index: the same f32 sum as over logits brought back).  No tower work is added (AZH_FLAG_SYMMETRY_AVG costs 8x).
 * Symmetry s in 0..7 as train.py:11-23: bit 0 mirrors x, bit 1 mirrors y, bit 2 then transposes, on the cells (x, y) =
 * (sq % 7, 6 - sq / 7) of the policy index: image_s(x, y) = x <- 6 - x if bit 0, y <- 6 - y if bit 1, then x <-> y if bit 2.
 * T_s(bitboard) has a stone at image_s(c) for every stone at c; T_s(move) maps from and to by image_s (a clone stays a clone,
 * a jump's layer follows from the transformed squares).
 * WHICH s is a pure function of the engine's seed, the game's uid and the position: key = philox(seed; uid, 0, 5, 0).v[0]
 * (stream 5 is drawn from by nothing else, so no other random number moves) and, over the UNTRANSFORMED leaf board, u32
 * arithmetic:  a = key;  for w in (lo32(mover), hi32(mover), lo32(opponent), hi32(opponent)): a = (a ^ w) * 0x9E3779B1,
 * a ^= a >> 15;  then a = a * 0x85EBCA77, a ^= a >> 13, s = a >> 29.  azh_eval_symmetry restates it on the host.  It does not
 * depend on iteration order, a parked descent or the evaluation cache: a position of a game is always seen the same way, so
 * the root's re-evaluation uses the symmetry of the node's first evaluation, and with AZH_FLAG_EVAL_CACHE a transposition
 * takes priors that were gathered under its own s — cache on still builds the trees of cache off.  (The reference's variant
 * draws a fresh symmetry per evaluation.)
 * azh_engine_leaves, _batch_leaves and _leaf_features return the image; azh_engine_set_evals and _set_batch_evals take the
 * logits of the image: an outside evaluator needs no change.  Node boards, records, game lines, the cache's keys, sampling,
 * the Dirichlet mix, re-roots and azh_engine_root_report are untouched, and with the mode off every engine behaves byte for
 * byte as before.  Composes with select_budget, the evaluation cache, the playout cap, forced playouts, ONE_RANDOM_MOVE, the
 * leaf-parallel search, the solver, thin batches, half-batches, azh_engine_play_moves and azh_engine_set_positions.
 * Refused (the engine stays as it was) with AZH_FLAG_TWO_NETS, with AZH_FLAG_SYMMETRY_AVG, and when the engine's blockers
 * mask is not its own image under all 8 symmetries (the tower takes the blocker plane once per launch; no blockers, the four
 * corners and the self-play start's diamond are); the table above.  Call before the first select or between iterations; off (0) is the state
 * after create.  Definition and measurements: DESIGN.md, "Random symmetry per evaluation". */
int azh_engine_set_random_symmetry(azh_engine *e, int on);
/* The symmetry, 0..7, under which an engine created with `seed` and the mode on evaluates the position (mover, opponent) of
 * game `uid`.  Host arithmetic only, usable without a device: the same function the kernels call. */
int azh_eval_symmetry(uint64_t seed, uint32_t uid, uint64_t mover, uint64_t opponent);
/* T_s on a bitboard (s is taken modulo 8, bits beyond the 49 cells are dropped) and on a move (u16 from | to << 8; a value that
 * is no board move, such as the pass 0xFFFF, comes back as it is; a negative code for s outside 0..7).  Host arithmetic only:
 * the same functions as the device's. */
uint64_t azh_symmetry_board(int s, uint64_t bitboard);
int azh_symmetry_move(int s, uint16_t move);
/* T_s on a flat policy index 119 x + 17 y + layer, for all 833 of them (the destination cell by image_s, a jump layer by the
 * image of its (dx, dy), the clone layer as it is): for a move m it is the index of T_s(m), and as a whole it is the
 * permutation that turns the logits of the image into logits of the position, position[i] = image[azh_symmetry_policy_index(s,
 * i)] — what a host needs to compare a mode-on engine with a mode-off one.  A negative code for s outside 0..7 or an index
 * outside 0..832.  Host arithmetic only. */
int azh_symmetry_policy_index(int s, int index);

/* The search's own value in the game record, and resignation of decided games (an extension, off by default; AlphaGo Zero /
 * AlphaZero resign decided self-play games and keep a share that never resigns, from which the threshold's false-positive
 * rate is measured).  consecutive = 0 switches the mode off (the state after create); else 1 <= consecutive <= 255,
 * 0 <= q_below < 1 and 0 <= playthrough_per_65536 <= 65536.
 * THE PLY'S VALUE q, when the device plays a move: b = the root edge with the most visits (ties: the lowest index),
 * q = W_b / (float)n_b, one IEEE f32 division of the edge's total score (azh_engine_root_report's W, in [0, 1] per visit for
 * the side to move) by its visits; a root without a visited edge has q = 0.5f, and such a ply neither counts nor resets.
 * q is never negative under a finite evaluator; its sign bit is dropped (the record has no room for it) before the rule
 * sees it, so the rule is a pure function of the record and no value that is not finite is ever below.
 * THE RULE: a ply COUNTS unless the playout cap is on and the ply is FAST.  Each side has a counter of its own consecutive
 * counted plies with q < q_below (the plain IEEE <: a NaN is never below; q_below = 0 records values and never resigns); a
 * counted ply with q >= q_below (or NaN) resets the mover's counter.  The rule FIRES at a ply after which the mover's
 * counter is >= consecutive (a counter stops at 255).
 * Game `uid` is a PLAY-THROUGH game iff (philox(seed; uid, 0, 6, 0).v[0] >> 16) < playthrough_per_65536 (stream 6 is drawn
 * from by nothing else, so no other random number moves; azh_resign_playthrough restates it): it runs to its real end
 * whatever the rule says.  In any other game the ply at which the rule fires is recorded as usual — board, visit
 * distribution, the sampled move, q — and the game ends there with result = 3 - mover (mover 1: x): the sampled move is not
 * played, no re-root is done, and the slot restarts exactly as after a finished game (ring record, AZH_STAT_GAMES, a fresh
 * game with uid + games).
 * THE RECORD of a game finished while the mode is on carries bit 4 (value 16) in header word 7, and word 5 of each ply is
 * (bits(q) & 0x7FFFFFFF) | (0x80000000 if the playout cap is on and the ply is FULL); a resigned game's carries bit 5
 * (value 32) too.  The line gains "values": [2 q - 1, ...] (the mover's expectation in [-1, 1], one per ply; a q that is not
 * finite reads 0) after "result" and, resigned, "resigned": 3 - result, the side that gave up.  Plies played before the
 * mode was switched on read q = 0.  Sampling, re-root, evaluation cache, select budget, the K-leaf search, the solver,
 * forced playouts and random symmetry are untouched, and with the mode off every state, tree and record word and every
 * output byte is what it was.
 * Refused (the engine stays as it was) with AZH_FLAG_TWO_NETS and AZH_FLAG_ONE_RANDOM_MOVE, and while a selected batch
 * awaits its backup (the table above).  Call before the first select or between iterations; setting it clears every slot's counters.
 * Definition and measurements: DESIGN.md, "Recorded search value and resignation". */
int azh_engine_set_resign(azh_engine *e, float q_below, int consecutive, int playthrough_per_65536);
/* Is game `uid` of an engine created with `seed` a play-through game?  1 / 0.  Host arithmetic only. */
int azh_resign_playthrough(uint64_t seed, uint32_t uid, uint32_t playthrough_per_65536);
/* Once-per-game counts since the engine was created: [0] games resigned, [1] play-through games finished, [2] of those, the
 * games in which the rule fired, [3] of those, the games the side it first fired for did NOT lose (the false positives). */
enum { AZH_RESIGN_STAT_RESIGNED = 0, AZH_RESIGN_STAT_PLAYTHROUGH = 1, AZH_RESIGN_STAT_FIRED = 2, AZH_RESIGN_STAT_FALSE = 3,
       AZH_RESIGN_STAT_COUNT = 4 };
int azh_engine_resign_stats(azh_engine *e, uint64_t *out /* [AZH_RESIGN_STAT_COUNT] */);

/* Temperature of the move played and of the root policy, per ply (an extension, off by default; AlphaZero plays
 * proportionally to the visits for 30 plies and then the most visited move, KataGo decays a temperature from 0.8 to 0.2 and
 * flattens the policy of the roots that get noise, 1.25 -> 1.1).  Each argument is a table of max_plies floats, copied, or
 * NULL: that part is off.  Both NULL is the state after create, and every byte the engine then produces is what it produced
 * before the call existed.
 * THE MOVE, when the device plays the move of ply p (azh_engine_run and the step-wise calls alike; not
 * azh_engine_play_moves), T = move_temperature[p]:
 *   T == 1: the proportional draw on the raw visit counts, untouched: a table of ones plays the games of no table.
 *   T == 0: the most visited root edge, the first one in edge order on a tie.
 *   else (1/64 <= T <= 64), in fixed point: n_max = the largest visit count of the root's edges; an edge with n_j >= 1 visits
 *     weighs q_j = min((uint32)(w * 1048576.0f), 1048576) with w = det_expf(d / T) (one IEEE f32 division) and
 *     d = min(det_logf((float)n_j) - det_logf((float)n_max), 0.0f); an edge without a visit weighs 0; the most visited edges
 *     weigh exactly 2^20.  S = sum of the q_j (<= 2^28), r = (uint32)(((uint64)v0 * S) >> 32) with v0 word 0 of
 *     philox(seed; uid, p, 1, 0) — the block of the proportional draw — and the move is the first edge j in edge order with
 *     q_0 + ... + q_j > r.  Integers throughout: no summation order changes the choice.
 * Everything after the choice is unchanged: the ply's record holds the search's visit counts (raw, or pruned under forced
 * playouts) — temperature changes the move, never the policy target — and the value, the resign rule and the re-root follow
 * as before.  FAST plies of the playout cap take their entry like any other ply.  While a move table is set the device loop
 * plays its queued moves in the move-playing launch of its own, as under forced playouts.
 * THE ROOT POLICY: where a root's priors are made on a ply that gets the Dirichlet noise (every ply, or the FULL ones under
 * the playout cap) and R = root_policy_temperature[ply] != 1, every legal move's logit is multiplied by 1.0f / R (one f32
 * division per node, one f32 multiply per edge) before the softmax over the legal moves; maximum, det_expf, sum, division
 * and the Dirichlet mix follow as before.  Other nodes, FAST plies and entries of 1 keep their priors bit for bit.  The
 * K-leaf search (azh_engine_set_leaf_batch) does the same.
 * Refused, the engine left as it was: an entry that is NaN or negative, a move temperature that is neither 0 nor in
 * [1/64, 64] (one in (0, 1/64) is refused, not rounded), a root policy temperature outside [1/4, 64]; tables on an engine
 * with AZH_FLAG_ONE_RANDOM_MOVE, AZH_FLAG_SAMPLE_POW5, AZH_FLAG_PY_POSTERIOR or AZH_FLAG_TWO_NETS; a call while a selected
 * batch awaits its backup; tables while the Gumbel root search is on (the table above).  Call before the first select or between iterations.
 * Definition and measurements: DESIGN.md, "Temperature of the move and of the root policy". */
int azh_engine_set_temperature(azh_engine *e, const float *move_temperature /* [max_plies] or NULL */,
                               const float *root_policy_temperature /* [max_plies] or NULL */);
/* The edge the rule above chooses from the visit counts visits[M] (1 <= M <= 256, in edge order) at `temperature` for ply
 * `ply` of game `uid` of an engine created with `seed`, restated on the host from the code the device runs; negative on a bad
 * argument (the temperature's range is azh_engine_set_temperature's).  q_out, unless NULL, receives the M weights the choice
 * was made on: the q_j above, at temperature 1 the visit counts themselves, at 0 2^20 for the chosen edge and 0 elsewhere.
 * Visit counts that are all 0 yield edge 0.  Host arithmetic only. */
int azh_temperature_pick(const uint32_t *visits, int M, float temperature, uint64_t seed, uint32_t uid, uint32_t ply,
                         uint32_t *q_out);

/* Proven wins and losses in the tree (MCTS-solver; an extension, off by default; DESIGN.md, "Proven wins and losses").
 * A node is DECIDED if it is a finished position or was PROVEN: after every batch's backup, for each path that ended at a
 * decided node, the node's parent is a proven win (+1 for its side to move) if one of its children is decided with -1, and
 * a proven loss (-1) if every one of its edges has a child decided with +1; a new proof is carried on towards the root.  A
 * path that reaches a decided node other than the root ends there (AZH_LEAF_TERMINAL) and backs up the node's value; the
 * root is always descended from.  Nothing else in the search changes: no move is pruned, W and n are the leaf-parallel
 * search's.  A proven node keeps its edges and result 0; its value is word 3 of its azh_engine_tree info row (the bits of
 * +-1.0f, as a finished position's terminal value) and the "finished" bit of the range word of the edge that leads to it
 * (azh_engine_tree_raw) is set; both are carried through re-roots (the device's own moves and azh_engine_play_moves).
 * While the solver is on, EVERY leaves_per_game — 1 included — runs through the leaf-parallel kernel: the step-wise calls
 * are azh_engine_batch_leaves / _set_batch_evals with K = leaves_per_game slots per game.  Call between iterations only.
 * Refused with AZH_FLAG_TWO_NETS, AZH_FLAG_EVAL_CACHE, AZH_FLAG_SYMMETRY_AVG and select_budget > 0 (the table above).  Turning it off
 * returns to the dispatch azh_engine_set_leaf_batch describes; marks already in the tree stay where they are (every tree
 * kernel ends a path at them as at a finished position). */
int azh_engine_set_solver(azh_engine *e, int on);
/* Counters of the proof pass, summed over the game slots since the engine was created: nodes proven, and paths that ended
 * at a proven node (a settled line hit again). */
enum { AZH_PROOF_STAT_NODES = 0, AZH_PROOF_STAT_HITS = 1, AZH_PROOF_STAT_COUNT = 2 };
int azh_engine_proof_stats(azh_engine *e, uint64_t *out /* [AZH_PROOF_STAT_COUNT] */);
/* For the slots first_game .. first_game + n_games - 1, one record of AZH_ROOT_PROOF_WORDS i32 each: [0] the decided value
 * of the root (0: not decided; +1 / -1: its side to move wins / loses — a finished root included), [1 + j], j < root edges,
 * in edge order as azh_engine_root_report: the decided value of edge j's child, seen from the side to move THERE (-1: the
 * move wins for the root's mover); 0 for an edge without a child, an undecided child and j >= root edges. */
enum { AZH_ROOT_PROOF_WORDS = 1 + AZH_MAX_MOVES };
int azh_engine_root_proofs(azh_engine *e, int first_game, int n_games, int32_t *out /* [n_games][AZH_ROOT_PROOF_WORDS] */);

/* First-play urgency and the exploration rate of the leaf-parallel search (an extension, off by default; the reference scores
 * an unvisited child with Q = 0 and explores with the constant c_puct; DESIGN.md, "First-play urgency and the exploration
 * rate").  The setter is azh_engine_set_exploration(e, fpu_reduction, c_base, c_init).
 *   - fpu_reduction < 0 means FPU off: an unvisited child's Q is 0, as today.
 *   - c_base == 0 means the constant cfg.c_puct, as today.  c_init is then ignored.
 *   - The mode is on while fpu_reduction >= 0 || c_base > 0.
 *   - Return -2 for a NaN or infinite argument, c_base < 0 or c_init < 0.
 * For one level of one path, at a node with children j = 0..M-1 in edge order:
 *   - n_j is the effective count: stored visits plus VL times the number of earlier paths of the batch.
 *   - W_j is unchanged.
 *   - P_j is |prior|.
 *   - N = sum of the n_j as u32.
 *   - sq = sqrtf((float)(1u + N)), as today.
 * All arithmetic is f32, every operation a single IEEE one, compiled -ffp-contract=off as the rest of engine.hip is.
 *   - c.  If c_base > 0, c = det_logf(((float)(1u + N) + c_base) / c_base) + c_init.  Otherwise c = c_puct.
 *   - f, with FPU on and N > 0.
 *       Wsum is the 64-lane sum of W_j over all j.  Unvisited edges add their stored +0.
 *       Psum is the 64-lane sum of (n_j > 0 ? P_j : +0.0f).
 *       Both sums are in the engine's canonical order: term j is added from +0 into lane j % 64 in ascending j, and the lanes
 *       are then folded by the xor butterfly 1, 2, 4, 8, 16, 32.  This is wave_sum_f32, restated in numpy by
 *       tests/priors_reference.wave_sum.
 *       qX = Wsum / (float)N, then f = qX - fpu_reduction * sqrtf(Psum), then f = f > 0.0f ? f : 0.0f.  A NaN becomes 0.
 *   - f, with FPU off or N == 0.  f = 0.
 *   - Score.  score_j = (sq / (1.0f + (float)n_j)) * (c * P_j) + (n_j ? W_j / (float)n_j : f), in puct_score's operation order.
 * Nothing else changes: a score is selectable only if score >= 0; ties follow the flags; path ends are unchanged (EVAL,
 * TERMINAL, COLLISION, dropped); the virtual loss, the backup, the solver's proofs and marks, re-roots, the root report and the
 * PV are all what they are today.  With the mode off, every byte of every arena is what it was before the mode existed.
 * While the mode is on, EVERY leaves_per_game — 1 included — runs through the leaf-parallel kernel, as under the solver: the
 * step-wise calls are azh_engine_batch_leaves / _set_batch_evals; off with K = 1 and no solver returns to the one-leaf kernels.
 * Call between iterations only.  Refused with AZH_FLAG_TWO_NETS, AZH_FLAG_EVAL_CACHE, AZH_FLAG_SYMMETRY_AVG and select_budget
 * > 0, and beside the Gumbel root search and forced playouts, which restate the root's PUCT with q = 0 and the constant c (the
 * table above); a refused call changes nothing.  AlphaZero's published c_base = 19652, c_init = 1.25 are a starting point;
 * nothing is tuned for Ataxx. */
int azh_engine_set_exploration(azh_engine *e, float fpu_reduction, float c_base, float c_init);
/* the three values in force: out [3] = fpu_reduction (-1: off), c_base (0: the constant c_puct), c_init */
int azh_engine_exploration(const azh_engine *e, float *out);
/* One node's M scores (1 <= M <= 256) under the rule above: prior [M], W [M] total scores, n [M] effective counts, into
 * scores_out [M].  With (-1, 0, 0) these are the reference's PUCT scores.  -2 for the arguments the setter refuses.  Host
 * arithmetic only, usable without a device: the functions the device's level uses, the two sums restated lane by lane. */
int azh_exploration_scores(const float *prior, const float *W, const uint32_t *n, int M, float c_puct, float fpu_reduction,
                           float c_base, float c_init, float *scores_out);

/* Search settings per side (an extension, off by default; DESIGN.md, "Search settings per side"): the two sides of a game
 * search with different settings inside the device-resident loop, every setting meets every other with the colours swapped,
 * and the device keeps the result table.  A SEARCH SET is what one side searches with: */
typedef struct azh_search_set {
    int32_t visits;          /* root visits at which this side's move is due */
    int32_t leaves;          /* paths per iteration: k = max(1, min(leaves, visits - root_visits)) */
    int32_t virtual_loss;
    float   c_puct;
    float   fpu_reduction;   /* < 0: off, as azh_engine_set_exploration */
    float   c_base, c_init;  /* c_base == 0: the constant c_puct */
} azh_search_set;
#define AZH_SEARCH_SETS_MAX 16
/* azh_engine_set_search_sets(e, n, sets), 0 <= n <= AZH_SEARCH_SETS_MAX: the sets are copied to the device, every slot learns
 * the pairing of the game it holds, and the tally (below) is zeroed.  n = 0 switches the mode off.
 * PAIRING.  For n >= 2 let q = uid / 2 and t = q % (n (n - 1) / 2); (a, b), a < b, is the t-th unordered pair in
 * lexicographic order.  In game uid x plays a and o plays b if uid is even, and the other way round if it is odd: uids 2q and
 * 2q + 1 are one pairing with the colours swapped (and share their opening under azh_engine_set_start_pool with stride 2), and
 * any n (n - 1) consecutive uids that start at a multiple of that number hold every ordered pair exactly once.  n = 1: (0, 0).
 * azh_search_set_pairing restates the rule on the host (out [2] = the set of x, the set of o); host and kernels run one function.
 * A PLY'S SET is the set of the side to move at the root (the root board's turn bit, not the ply's parity), whether the root
 * was reached by the engine's own move, by azh_engine_play_moves or loaded by azh_engine_set_positions.
 * While the mode is on every ply searches with its set: its move is due at the set's `visits`; a select takes up to the
 * set's `leaves` paths with the set's `virtual_loss`; a level scores with the set's c_puct, fpu_reduction, c_base and c_init
 * under the rule of azh_engine_set_exploration; a batch's backup removes the virtual loss of the set that selected it.  The
 * engine's own visits, c_puct and virtual loss are not used for the search of a ply; its leaves_per_game K stays the stride
 * of the leaf slots (g K + p), and no set may ask for more leaves.  Everything else is what it is without the mode: root
 * noise, the tie rule, expansion, backup, the move's draw, records, game lines, the re-root.  Every K, 1 included, runs
 * through the leaf-parallel kernel (the step-wise calls are azh_engine_batch_leaves / _set_batch_evals), and the device loop
 * plays the queued moves in a launch of their own.  With tree reuse a new root inherits the subtree the other side's settings
 * built; that is allowed, and a match tool wants AZH_FLAG_NO_REUSE.
 * -2, the first offending set named: visits outside 1 .. the engine's current visits; leaves outside 1 .. K in force;
 * virtual_loss outside 1 .. 16 (so leaves * virtual_loss <= 1024, the leaf batch's bound); c_puct not finite or < 0;
 * fpu_reduction, c_base, c_init as azh_engine_set_exploration checks them.  While sets are on azh_engine_set_visits below a
 * set's visits and azh_engine_set_leaf_batch below a set's leaves are refused with -2.  -3, -4: the table above.  A refused
 * call changes nothing.  Composes with the leaf batch, the solver, temperature, resign, random symmetry, the start pool, the
 * game limit, azh_engine_set_positions and azh_engine_play_moves.
 * TALLY.  azh_engine_search_set_stats: out [n][n][AZH_SET_STAT_COUNT], indexed [set of x][set of o], counted once per game
 * where AZH_STAT_GAMES or AZH_STAT_DROPPED is: GAMES every such game, X_WINS / O_WINS by the result (a resigned game by its
 * result), UNDECIDED a game cut at the ply limit (the rules know no draw), so GAMES = X_WINS + O_WINS + UNDECIDED. */
int azh_engine_set_search_sets(azh_engine *e, int n, const azh_search_set *sets);
/* the sets in force: *n_out their number (0: the mode is off), sets_out [AZH_SEARCH_SETS_MAX] or NULL */
int azh_engine_search_sets(const azh_engine *e, int32_t *n_out, azh_search_set *sets_out);
/* out [2] = the set of x, the set of o in game `uid` among n sets; -1 for a null out, -2 for n outside 1 ..
 * AZH_SEARCH_SETS_MAX.  Host arithmetic only, usable without a device. */
int azh_search_set_pairing(uint32_t uid, int n, int32_t *out);
enum { AZH_SET_STAT_GAMES = 0, AZH_SET_STAT_X_WINS = 1, AZH_SET_STAT_O_WINS = 2, AZH_SET_STAT_UNDECIDED = 3, AZH_SET_STAT_COUNT = 4 };
int azh_engine_search_set_stats(azh_engine *e, uint64_t *out /* [n][n][AZH_SET_STAT_COUNT] */);

/* Which tower the device-resident loop evaluates its leaves with: 0 the 3-board workgroups (throughput), 1 one board per
 * workgroup (latency: AZH_FORWARD_THIN's kernel), -1 (default) by the engine's size — thin for engines of at most
 * AZH_THIN_MAX_GAMES game slots.  A host that knows its batch has thinned out (a match under a game limit whose last games
 * are running, uai_ringmaster.py:221-262) switches at a drain; results of the 16-bit towers differ in the last bits between
 * the two kernels, so switch at points that do not depend on timing. */
#define AZH_THIN_MAX_GAMES 512
int azh_engine_set_thin_batches(azh_engine *e, int mode);

/* Measurement set-up hook: every slot restarts at a given position — boards [games][2] packed (x | turn << 63, o),
 * plies [games] — with a fresh tree.  Such games are played, counted (AZH_STAT_GAMES / _DROPPED), and their records are
 * assembled, drained and formatted like any other (the measured path does the same work per finished game), but no line is
 * handed out: the record lacks the plies before the start.  bench.py loads the positions a long-running generator would
 * be found at instead of waiting a game generation (about 70 s at 400 sims/move) for the steady state to form.
 * Under azh_engine_set_game_limit the slots g >= limit are loaded and left idle (they resume the loaded game when the limit
 * is raised): see there. */
int azh_engine_set_positions(azh_engine *e, const uint64_t *boards, const int32_t *plies);

/* A start position and wall map per game, drawn from a pool (an extension, off by default; DESIGN.md, "A start position per
 * game").  With a pool of n entries — x [n], o [n], blockers [n] bitboards, turn [n] (0: x to move, 1: o), copied — the game
 * with uid u starts from entry (u / stride) % n and is played on that entry's walls, instead of azh_config's start_x, start_o,
 * start_turn and blockers; azh_start_pool_entry restates the rule on the host.  Slot g plays uids g, g + games, ..., so a slot
 * changes map from one game to the next unless n divides games / stride.  stride 1: self-play; stride 2: a two-net match, whose
 * slots 2k and 2k + 1 play one map with the colours swapped as they share an opening.  Round robin keeps every prefix of a
 * uid-ordered games file balanced over the maps.  All games are evaluated in the same tower launches — each leaf goes to the
 * net with the wall plane of its own game, which the select that produced the leaf wrote beside it — and are written into the
 * same lines: with azh_engine_set_record_blockers every line's "blockers" is the mask of the line's game, and
 * azh_engine_uid_blockers gives a host the mask of any uid (the engine's one mask while no pool is set).
 * n = 0 takes the pool away: every game starts from the configured position again.  1 <= n <= AZH_START_POOL_MAX, stride >= 1.
 * Call before the engine's first select (the pool replaces the start position the engine was created with; every slot starts
 * its game again, so positions loaded by azh_engine_set_positions before the call are gone: load them after it).  Under a pool
 * azh_engine_set_positions checks slot g's position against the walls of uid g and plays it on them.
 * Checked in the setters' order, and a refused call changes nothing: -1 a null argument; -2 n or stride out of range, or an
 * entry (named in azh_last_error, the first one) with bits beyond the 49 cells, a cell with stones of both sides, a stone on
 * a wall, a side without a stone, a turn that is neither 0 nor 1, or a position the rules adjudicate as finished; -3 a
 * selected batch awaits its backup; -4 the engine has begun to search, or random symmetry is on and an entry's mask is not its
 * own image under all 8 symmetries ("azh_engine_set_start_pool: the random symmetry is not supported with a blockers mask (0x...)
 * that is not its own image under all 8 symmetries (...)").  With a pool set, azh_engine_set_random_symmetry refuses in the same
 * words when any entry's mask is not invariant (the table above reads "the engine's blockers mask" as "every mask games are
 * played on"). */
#define AZH_START_POOL_MAX 65536
int azh_engine_set_start_pool(azh_engine *e, int n, const uint64_t *x, const uint64_t *o, const uint64_t *blockers,
                              const int32_t *turn, int stride);
/* (uid / stride) % n, or a negative code for n < 1 or stride < 1.  Host arithmetic only, usable without a device. */
int azh_start_pool_entry(uint32_t uid, int n, int stride);
/* The walls game `uid` of this engine is played on: its pool entry's, or the engine's blockers while no pool is set. */
int azh_engine_uid_blockers(const azh_engine *e, uint32_t uid, uint64_t *out);

/* ------------------------------------------------------------------ moves named by the host (an extension)
 * A front-end that keeps its search tree across moves (uai_interface.py --reuse-tree; the reference's
 * MCTSEngine.set_state, engine.py:452-472, walks to the new root with MCTS.play, engine.py:411-424) tells the engine
 * which move was played instead of letting it sample one.
 *
 * azh_engine_play_moves: moves [games], one per slot, u16 = from | to << 8; 0xFFFF leaves the slot alone.  Per slot with
 * a move, status_out [games] is
 *   AZH_PLAY_KEPT      the root edge had a child: that child is the root now, with its subtree, visit counts, total scores
 *                      and priors (the re-root of the device's own moves: breadth-first compaction into the other arena)
 *   AZH_PLAY_FRESH     the edge had no child, or the engine was created with AZH_FLAG_NO_REUSE: a one-node tree at the
 *                      position after the move
 *   AZH_PLAY_FINISHED  the move was played (subtree kept or not) and the new root is a finished position: the slot goes idle
 *                      at that root (phase 3; azh_engine_set_positions starts it again)
 *   AZH_PLAY_ILLEGAL   the move is not among the root's edges: every byte of the slot's arenas and state is as before
 *   AZH_PLAY_BUSY      the slot is idle (phase 3): untouched
 *   AZH_PLAY_NONE      no move was given
 * After a move that was played the slot's ply is one higher (it stops at max_plies - 1: the ply cut belongs to the games
 * the device plays itself), its root is evaluated again by the next select (phase 0, as after a sampled move), no random
 * number has been drawn, no ply record written, AZH_STAT_PLIES has not moved (AZH_STAT_REROOT_* count the copy), and the
 * slot's game never becomes a game line (as after azh_engine_set_positions).  With AZH_FLAG_EVAL_CACHE the new arena's table
 * is rebuilt as after a sampled move.
 * A slot whose OWN move is due (phase 2: its root has reached `visits`; a leaf-parallel search that ran exactly to its
 * target ends there) is taken out of the move queue and the host's move is played IN PLACE of the sampled one: the device
 * never samples for a slot the host has moved in before the next select.
 * Refused with an error, nothing changed: while a batch selected with azh_engine_select awaits its azh_engine_backup, and
 * on AZH_FLAG_TWO_NETS engines.  Enqueued on the engine's stream; returns when status_out has been written. */
enum { AZH_PLAY_NONE = 0, AZH_PLAY_KEPT = 1, AZH_PLAY_FRESH = 2, AZH_PLAY_FINISHED = 3, AZH_PLAY_ILLEGAL = -1,
       AZH_PLAY_BUSY = -2 };
int azh_engine_play_moves(azh_engine *e, const uint16_t *moves /* [games] */, int32_t *status_out /* [games] */);

/* azh_engine_root_report: what a front-end prints about a search, without copying the tree (azh_engine_tree moves 16 B per
 * node twice and 18 B per edge: tens of MB at 60000 visits).  For the slots first_game .. first_game + n_games - 1, one
 * record of AZH_ROOT_REPORT_WORDS u32 each:
 *   [0] root visits   [1] root edges M (<= AZH_MAX_MOVES)   [2] root edges with a child   [3] the root's result (0: not
 *   finished, 1 / 2: as azh_rules_batch)
 *   [4 + 4 j .. 7 + 4 j], j < M, in edge (= move generation) order: move, visits, total score W (f32 bits, seen from the
 *   side to move at the root), prior (f32 bits); zero for j >= M
 *   [AZH_ROOT_REPORT_PV]  number of moves L of the principal variation, then L pairs (move, visits of its edge): from the
 *   root the edge with the most visits, the first one in edge order on a tie; the line ends before an edge with 0 visits,
 *   after an edge without a child or into a finished position, and after AZH_PV_MAX moves; zero beyond L pairs. */
#define AZH_PV_MAX 32
enum { AZH_ROOT_REPORT_PV = 4 + 4 * AZH_MAX_MOVES, AZH_ROOT_REPORT_WORDS = AZH_ROOT_REPORT_PV + 1 + 2 * AZH_PV_MAX };
int azh_engine_root_report(azh_engine *e, int first_game, int n_games, uint32_t *out /* [n_games][AZH_ROOT_REPORT_WORDS] */);
/* The same kernel and the same records written into a DEVICE array of the caller's, d_out [n_games][AZH_ROOT_REPORT_WORDS] (a
 * torch tensor's pointer): no device-to-host copy; returns when the kernel has completed.  What azh_samples_retarget reads. */
int azh_engine_root_report_device(azh_engine *e, int first_game, int n_games, uint32_t *d_out);

int azh_engine_game_state(azh_engine *e, int game, azh_game_state *out);
/* arena dump: boards [n_nodes][2] u64, info [n_nodes][4] u32
 * (first_edge, n_edges | result << 16, 0, terminal value bits), edges
 * [n_edges][4] u32 (prior bits, visits, total score bits, child), moves [n_edges] */
int azh_engine_tree(azh_engine *e, int game, uint64_t *boards, uint32_t *info, uint32_t *edges,
                    uint16_t *moves);
/* Diagnostic: the same edges as the 16-byte records the tree kernels read — edges [n_edges][4] u32 = prior bits (bit 31:
 * the mark of the child the last descent through the node chose — the early request of the next level, never part of a
 * decision), total score bits, visits | child << 16 (0xFFFF: none), the child's edge range (first | count << 23 |
 * finished << 31).  tests/test_gpu_engine.py checks the mark's invariants on it. */
int azh_engine_tree_raw(azh_engine *e, int game, uint32_t *edges);
int azh_engine_stats(azh_engine *e, uint64_t *out /* [AZH_STAT_COUNT] */);
/* enable = 0: off; n > 0: bracket every n-th iteration of the device loop with events (tower start / tower end /
 * next tower start); at most 8192 samples are kept */
/* Diagnostic: runs two iterations of the device loop with the tree launch between their towers stamped by
 * s_memrealtime (100 MHz): out [games][10] u64 = wave start, state loaded, backup done, move-due mark done, descent done,
 * expansion done, state stored, workgroup (its four games, one beyond 8192) done, then two counts: levels descended, children scanned —
 * tools/tree_stamps.py turns them into a breakdown. */
int azh_engine_tree_stamps(azh_engine *e, azh_net *net, int dtype, uint64_t *out);
int azh_engine_timing_reset(azh_engine *e, int enable);
int azh_engine_timing(azh_engine *e, azh_timing *out);

/* Finished games as JSON lines in the reference's format
 * (cpp/self_play_client.cpp:512,565-578,639-641: keys boards, dists, moves,
 * result; one compact object per line).  Writes whole lines only; *used = bytes
 * written, *n_games = lines written; call again while *n_games > 0. */
int azh_engine_drain_json(azh_engine *e, char *buf, int64_t cap, int64_t *used, int32_t *n_games);
/* Takes the finished games off the device without formatting them: waits for the work enqueued so far, copies the record
 * ring to the host and empties it; the next azh_engine_drain_json formats what was fetched and does not touch the device.
 * A host loop that calls fetch, enqueues its next azh_engine_run and only then drains has the formatting and its own file
 * writes running under that run instead of in front of it (the reference's workers write their games from their own
 * threads, cpp/self_play_client.cpp:637-642: there, too, nobody waits for a game to be written).  Optional: a drain with
 * nothing fetched fetches by itself whenever work has been enqueued since the last fetch (so a caller that never fetches gets
 * one fetch per round, whether it drains in a loop until *n_games == 0 or with one call per round) — except inside the
 * drain sequence that follows an explicit fetch (the calls up to and including the first one that returns *n_games == 0):
 * those never touch the device, whatever was enqueued meanwhile.  A fetch touches only its own engine's streams: with
 * several engines on one GPU (half-batches) fetching one does not wait for the others' runs. */
int azh_engine_fetch(azh_engine *e);
/* 1 while work enqueued on this engine's streams is still in flight, 0 when they are idle (< 0: error).  Never waits. */
int azh_engine_query(azh_engine *e);
/* How many times azh_engine_drain_json had to fetch by itself (and so waited for the device) since the engine was created:
 * 0 for a host loop that fetches explicitly before every drain sequence. */
long long azh_engine_implicit_fetches(const azh_engine *e);
/* Diagnostic: the records the last azh_engine_fetch took off the device and no drain has formatted yet, copied as they lie
 * in the ring (one after the other, each as azh_format_record_json describes; dropped games' 8-word markers included).
 * Nothing is consumed: the next azh_engine_drain_json formats them as usual.  *words = words staged; -6 if `cap` (in
 * words) is smaller (nothing written).  What a game line does not carry — uid, visit counts, the "full" words of the
 * plies — can be read here. */
int azh_engine_staged_records(azh_engine *e, uint32_t *buf, int64_t cap, int64_t *words);
/* The line of ONE finished-game record (the words between two ring headers, as the device loop leaves them: 8-word header
 * {magic, slot, uid, plies, result, words, random_ply + 1, kind}, then per ply {x lo, x hi, o lo, o hi, move | nd << 16, full,
 * nd x (move | visits << 16)}; kind | 4 and full: azh_engine_set_playout_cap) exactly as azh_engine_drain_json writes it, without the newline: what the reference's
 * `entry.dump()` gives (cpp/self_play_client.cpp:565-578,639-641: nlohmann::json — sorted keys, no whitespace, floats as
 * the digits its Grisu2 finds, plain decimals from 1e-4 up, d.ddde-XX below).  Host code only, usable without a device.
 * *used = bytes the line has; -6 if `cap` is smaller (nothing written), -2 if the words are not a well-formed record — or
 * carry kind bit 64 (azh_engine_set_gumbel): those records become lines in azh_engine_drain_json only.
 * with_ids: the arena's two extra keys (slot, uid).
 * The record's layout, every kind bit included, is defined once, in ataxxzero_amd/csrc/record.h; ataxxzero_amd/link.py
 * carries the same names (RECORD_MAGIC, REC_KIND_*) and walks it in link.records.  The kind bits are not part of this
 * header: a caller reads them there. */
int azh_format_record_json(const uint32_t *rec, int64_t words, int32_t with_ids, char *buf, int64_t cap, int64_t *used);
/* Order in which azh_engine_drain_json hands games out: 0 (default) as they finish; 1 by game uid (slot g plays
 * uids g, g + games, g + 2 games, ...): a finished game is held back until every game with a smaller uid has been
 * handed out or dropped.  The reference's workers write games as they finish (Worker::thread_main :637-642) and
 * looper.py:51-64 stops the generator at --game-count lines, i.e. keeps the games that finished FIRST — the short
 * ones; with thousands of games in flight that bias is no longer slight, and uid order removes it (the first N
 * lines are the first N games started).  Call before the first drain. */
int azh_engine_set_emit_order(azh_engine *e, int by_uid);
/* on != 0: every line azh_engine_drain_json writes gains one key in front, "blockers":[...] — the engine's blockers mask (under a
 * start pool: the mask of the line's game, azh_engine_uid_blockers of its uid) as
 * the ascending list of wall cells in the index the line's boards use, x + 7 y with y = 0 at rank 7 ([] for no walls; the
 * start position of the self-play generator gives [17,23,25,31]).  The ring record does not change, and a line with the key's
 * bytes taken out is the line written without it.  Off by default.  Takes effect for records fetched after the call. */
int azh_engine_set_record_blockers(azh_engine *e, int on);
/* azh_format_record_json with that key written from `blockers` (bit = file + 7 * rank; bits beyond the 49 cells: -1). */
int azh_format_record_json_blockers(const uint32_t *rec, int64_t words, int32_t with_ids, uint64_t blockers, char *buf,
                                    int64_t cap, int64_t *used);
/* Play at most `games` games (uids 0 .. games - 1) and then stop searching: a slot whose next game would be past the
 * limit goes idle, the batch thins out as the last games end.  For a generator that was given a target count: in uid
 * order line N appears once the slowest of the first N games has ended, and without a limit every other slot meanwhile
 * plays games nobody will read.  The limit may be raised later (dropped games leave the caller short of lines): idle
 * slots whose next game is now below it start it; games that have begun are never stopped.  (The reference's client has
 * no such notion: it is stopped from outside, looper.py:51-64.)
 * The contract, loaded positions included (tests/test_gpu_game_limit.py):
 *  - A slot HAS NOT BEGUN when it is in phase 0 with no leaf or root evaluation in flight, has one node and root_visits == 0,
 *    and no move of its current game has been played since the game was started, neither by the device nor through
 *    azh_engine_play_moves — started by the engine itself at ply 0, or by azh_engine_set_positions at the loaded ply.
 *  - The call idles every such slot whose uid is >= games (phase 3).  The slot keeps its uid, its loaded root, its ply and
 *    where its record starts.  azh_engine_set_positions under a limit already in force leaves the slots g >= games idle in
 *    the same way: both call orders give the same engine state, word for word.
 *  - Raised: a slot that was idled while it held a loaded position it had not begun resumes THAT game — same board, same
 *    ply, same record start; any other idle slot below the new limit starts a fresh game at the start position.
 *  - Begun games are never stopped: a loaded slot whose root evaluation is in flight or done, and a slot after a host-played
 *    move, the fresh one-node root of AZH_PLAY_FRESH included.  Idle slots add nothing to any counter.
 *  - With no limit, or a limit >= the slot count when positions are loaded, nothing differs from an engine without one. */
int azh_engine_set_game_limit(azh_engine *e, int64_t games);

/* ------------------------------------------------------------------ device-resident training samples
 * (an extension; nothing above changes).  A store keeps finished games in device memory — per game {first ply, plies,
 * result | AZH_SAMPLES_GAME_*, random_ply + 1 (0: none)}, per ply the two bitboards in the ring record's layout (bit
 * x + 7 (6 - y) is the cell boards[ply][x + 7 y] of the game line), its flags AZH_SAMPLES_PLY_*, the recorded value as a
 * double and its policy target as (flat index 119 x + 17 y + layer: u16, weight: f32) pairs — and one kernel writes a
 * minibatch from it straight into the trainer's tensors: features [n][7][7][4], policy [n][7][7][17], value [n][1], f32,
 * bit for bit what the host pipeline (training.make_minibatch_reference; the reference's train.py:43-77) builds from the
 * same games for the same draws: plane 0 ones, plane 1 the mover's stones (the mover is 1 + ply % 2), plane 2 the
 * opponent's, plane 3 zeros (the game's walls where it has a mask: "Walls" below), the board under symmetry s (bit 0 mirrors
 * x, bit 1 mirrors y, bit 2 then transposes); each
 * weight at azh_symmetry_policy_index(s, index); the value z = +-1 (result == mover), or with value_blend = L != 0 and a
 * game that has values (1 - L) * z + L * v in double, in that order, rounded once to f32.
 * The host keeps a mirror of the per-game words and the ply flags (a few bytes per ply) and checks every draw against it:
 * no kernel ever sees an index it cannot serve.
 * A ply is BAD when the f32 sum of its weights, added in ascending index order, is off from 1 by at least 1e-3: the host
 * finds that at ingest.  (The host pipeline sums the 833 cells pairwise: for a sum within an ulp or so of the edge the two
 * may disagree; agreement exactly at the edge is not claimed.)
 * Codes: -1 bad argument, -2 malformed input (azh_samples_gather: a draw on a bad ply), -6 capacity. */
typedef struct azh_samples azh_samples;
enum { AZH_SAMPLES_PLY_PASS = 1, AZH_SAMPLES_PLY_FULL = 2, AZH_SAMPLES_PLY_BAD = 4 };
enum { AZH_SAMPLES_GAME_HAS_FULL = 1 << 8, AZH_SAMPLES_GAME_HAS_VALUES = 1 << 9 };
int azh_samples_create(int64_t cap_games, int64_t cap_plies, int64_t cap_targets, azh_samples **out);
void azh_samples_destroy(azh_samples *s);
/* Games as host arrays, what azh_samples_add_games takes and azh_samples_pack_records fills: games [n_games][4] as above with
 * the first ply counted from these arrays; boards [n_plies][2] (x, o); ply_flags [n_plies] (PASS and FULL; BAD is found at
 * ingest); values [n_plies]; target_start [n_plies + 1] into target_index / target_weight [n_targets].  A game has 1 .. 65535
 * plies; result 1 or 2, or 0 for a game cut at the ply limit and kept (AZH_FLAG_KEEP_UNFINISHED), which is nobody's win: z = -1
 * for both sides, as the host pipeline has it.  The two optional arrays: "Walls" and "Auxiliary targets" below. */
typedef struct azh_sample_arrays {
    int64_t n_games, n_plies, n_targets;
    uint32_t *games;  uint64_t *boards;  uint8_t *ply_flags;  double *values;
    int32_t *target_start;  uint16_t *target_index;  float *target_weight;
    uint64_t *game_blockers;            /* [n_games], or NULL: no game has walls */
    uint64_t *game_owners;              /* [n_games][2] (x-owned, o-owned), or NULL: no game has owners */
} azh_sample_arrays;
/* The DEVICE arrays a minibatch is written into: features [n][7][7][4], policy [n][7][7][17], value [n][1], and either all
 * four or none of ownership [n][7][7], score [n][1], reply [n][7][7][17], aux_weight [n][2] ("Auxiliary targets" below). */
typedef struct azh_sample_outputs {
    float *features, *policy, *value;
    float *ownership, *score, *reply, *aux_weight; /* all four NULL: no auxiliary targets */
} azh_sample_outputs;
/* Appends the games of `a`.  -1 for a missing array, -2 when the arrays contradict each other (n_targets is not
 * target_start[n_plies] among it) or walls or owners are refused (below), -6 when a capacity would be exceeded: every time
 * the store is exactly what it was. */
int azh_samples_add_games(azh_samples *s, const azh_sample_arrays *a);
/* Ring records, one after the other as azh_engine_staged_records returns them, -> the arrays azh_samples_add_games takes,
 * holding what parsing each game's own line would give: the targets in the order of the line's sorted keys, weight
 * (float)((double)count / (double)total) over the written counts (0 when total is 0; the same rule for the Gumbel search's
 * 65535-unit counts), value isfinite(q) ? 2.0 * (double)q - 1.0 : 0.0 under kind & 16, FULL from word 5 (its sign bit under
 * kind & 16) under kind & 4, random_ply + 1 from header word 6, indices by the engine's own move -> policy index map.  Each
 * record must pass the walk azh_format_record_json makes; the markers of dropped games (kind & 1) and games begun at a loaded
 * position (kind & 3 == 2) have no line and are skipped; anything else — a record cut short, a word count that does not
 * match, a target that is no clone and no jump — returns -2 with nothing written.
 * Walls come one of two ways: `blockers`, the mask of the engine that wrote the records, with record_masks NULL; or, for an
 * engine with a start pool (azh_engine_set_start_pool), record_masks [n_masks], one mask per record of the buffer in its
 * order — the markers of dropped and loaded games included — each azh_engine_uid_blockers of the record's uid, with `blockers`
 * 0.  A non-zero `blockers` beside record_masks is -1; n_masks other than the number of records is -2.
 * aux != 0: each game's owners are computed too ("Auxiliary targets").
 * out: n_games, n_plies, n_targets hold the room of the arrays on entry and what the records hold on return; with
 * out->games == NULL only these counts are returned; game_blockers and game_owners are filled where they are not NULL (the
 * owners only under aux).  -6 when an array is too small.  Host code only, usable without a device. */
int azh_samples_pack_records(const uint32_t *rec, int64_t words, uint64_t blockers, const uint64_t *record_masks,
                             int64_t n_masks, int aux, azh_sample_arrays *out);
/* azh_samples_pack_records followed by azh_samples_add_games, the walls going along when `blockers` or record_masks is
 * given and the owners under aux: -1, -2 and -6 add nothing. */
int azh_samples_add_records(azh_samples *s, const uint32_t *rec, int64_t words, uint64_t blockers,
                            const uint64_t *record_masks, int64_t n_masks, int aux);
/* out [4]: games, plies, targets, bad plies that are no passes. */
int azh_samples_counts(const azh_samples *s, int64_t *out);
/* The host mirror: games [games][4] (first ply counted from the store's first), ply_flags [plies]. */
int azh_samples_mirror(const azh_samples *s, uint32_t *games, uint8_t *ply_flags);
/* A minibatch for host draws [n][3] of (game, ply, symmetry) into the arrays of `out`: with the four auxiliary arrays the
 * kernel that also writes them runs, for the same draws the same bytes in features, policy and value (a store in which no
 * game has owners is served: final weight 0 everywhere, reply as defined); with one to three of them -1.  Every draw is
 * checked first: out of range or a pass -> -1, a bad ply -> -2 ("policy target does not sum to one"), nothing launched.  `stream` is a
 * hipStream_t as a pointer-sized integer: the call enqueues on it and returns; the draws travel through pinned staging the
 * store owns, two buffers taken in turn, so the next call does not wait for this one.  stream = 0: the store's own stream,
 * and the call returns after completion — that stream is not ordered against any other, the null stream included: a caller
 * whose work runs on the null stream passes hipStreamLegacy (1), as link.SampleStore does for torch's default stream. */
int azh_samples_gather(azh_samples *s, int n, const int32_t *draws, double value_blend, const azh_sample_outputs *out,
                       uintptr_t stream);
/* The same with the draws made on the device.  Sample i makes at most 64 attempts; attempt a takes one Philox4x32-10 block
 * v keyed by `seed` with counter (step, i, a, 8) — stream 8 is drawn from by nothing else:
 *   game g = first_game + ((u64)v[0] * n_games >> 32);  c = the game's candidate plies: all of them, or the FULL ones of a
 *   game that has "full"; c == 0 fails the attempt;  ply = random_ply + 1 if the game has one, else candidate
 *   ((u64)v[1] * c >> 32);  a ply outside the game, a pass or a bad ply fails the attempt;  symmetry = v[2] >> 29.
 * The first attempt that succeeds is the draw: the host pipeline's distribution — uniform game, uniform ply, everything
 * redrawn on rejection.  (The multiply-shift picks each of r values with a probability within 2^-32 of 1 / r.)  A sample
 * whose 64 attempts all fail is written as zeros and counted (azh_samples_status).  draws_out: NULL, or a DEVICE array
 * [n][4] of (game, ply, symmetry, attempts used); (-1, -1, -1, 64) for a failed sample. */
int azh_samples_draw_gather(azh_samples *s, int n, uint64_t seed, uint32_t step, int64_t first_game, int64_t n_games,
                            double value_blend, const azh_sample_outputs *out, int32_t *draws_out, uintptr_t stream);
/* One sample's draw restated from mirror arrays (games [total_games][4], ply_flags with BAD set where it applies) -> out [4]
 * as a row of draws_out.  candidates and cum both NULL: the uniform ply draw above; both given (azh_samples_ply_cum's
 * mirrors): the weighted one ("Weighted ply draws" below); one of them: -1.  Host arithmetic only: no device, no store. */
int azh_samples_draw(uint64_t seed, uint32_t step, uint32_t sample, int64_t first_game, int64_t n_games,
                     const uint32_t *games, int64_t total_games, const uint8_t *ply_flags, const uint16_t *candidates,
                     const uint32_t *cum, int32_t *out);
/* Waits for the device and returns how many samples of azh_samples_draw_gather have failed since the store was created. */
int azh_samples_status(azh_samples *s, int64_t *failed);

/* Walls.  The store keeps one u64 blockers mask per game in the ring record's bit layout (bit = file + 7 * rank), 0 for a game
 * that came without one, in a device array [cap_games] that is allocated when the first game with walls arrives: until then
 * the kernels are handed a null pointer and every output is what it was.  With a mask, feature plane 3 of a sample holds 1.0
 * on the wall cells, under the sample's symmetry like planes 1 and 2 (training.make_minibatch_reference with an entry's
 * "blockers").
 *  - azh_samples_add_games: -2, nothing added, for a mask of game_blockers with bits beyond the 49 cells and for a game one of
 *    whose plies has a stone on a wall cell (the game is named).
 *  - azh_samples_pack_records / azh_samples_add_records: the same two refusals for `blockers` and for every mask of
 *    record_masks, before anything is written; game_blockers receives each game's mask.
 *  - azh_samples_game_blockers: the host mirror of the masks, blockers [games]. */
int azh_samples_game_blockers(const azh_samples *s, uint64_t *blockers);

/* ------------------------------------------------------------------ policy surprise weighting
 * (an extension of the store; with none of these called, every launch and every draw above is what it was.)
 *
 * The SURPRISE of a stored ply is KL(target || prior), the prior being a net's policy for the mover's view of the stored
 * position (the mover is 1 + ply % 2; the boards go to the tower as (mover, opponent), the orientation the engine feeds it).
 * With l the net's 833 f32 logits, `legal` the position's moves in the device movegen's order (jumps by ascending
 * (from, to), then clones ascending; no blockers) mapped by the engine's move -> policy index map — for a game stored with a
 * wall mask, `legal` = the position's moves from wave_movegen with the game's blockers, and the tower is shown that mask as
 * its blocker plane:
 *   mx = max of l over legal;  S = sum over legal of det_expf(l_j - mx);  log p_t = (l_t - mx) - det_logf(S);
 *   KL = sum over the ply's targets with weight w_t > 0 and t legal of  w_t * (det_logf(w_t) - log p_t).
 * Everything is f32, every operation a single IEEE one.  BOTH sums run in the engine's 64-lane order: term j (the j-th legal
 * move; the j-th target of the ply in stored order, a skipped target being a term of +0) is added, from +0, into lane j % 64
 * in ascending j, then the lanes are folded by the xor butterfly with offsets 1, 2, 4, 8, 16, 32.  The maximum starts at
 * -inf and a NaN never replaces it.  A result that is negative, NaN or infinite is stored as 0; a pass or a bad ply has KL 0.
 * A target with w_t > 0 whose index is not legal adds nothing and is counted (0 for games the engine wrote).
 *
 * azh_samples_surprise_logits: the surprise of plies [first_ply, first_ply + n_plies) (counted from the store's first ply) from
 * a DEVICE array of logits [n_plies][833], enqueued on `stream` (0: the store's own) and waited for; kl_out [n_plies] on the
 * host; *illegal_out the count above.  The values also stay in a device array the store owns, one f32 per ply. */
int azh_samples_surprise_logits(azh_samples *s, int64_t first_ply, int64_t n_plies, const float *d_logits, float *kl_out,
                                int64_t *illegal_out, uintptr_t stream);
/* The same for every ply of games [first_game, first_game + n_games), the logits coming from `net` in `dtype`: in chunks of
 * at most 16384 plies (azh_samples_set_surprise_chunk: another size, for tests; 0 restores the default) a small kernel packs
 * the boards, the tower runs, and the surprise kernel runs behind it on the store's stream.  kl_out: one f32 per ply of those
 * games.  A chunk never spans two wall masks: the chunks are cut where the mask changes from one game to the next as well as
 * at the chunk size (planned on the host from its mirror); azh_samples_surprise_logits cuts its kernel launches the same way. */
int azh_samples_surprise(azh_samples *s, azh_net *net, int dtype, int64_t first_game, int64_t n_games, float *kl_out,
                         int64_t *illegal_out);
int azh_samples_set_surprise_chunk(azh_samples *s, int plies);
/* ms [2]: HIP-event milliseconds of the last azh_samples_surprise, summed over its chunks: {board packing and tower,
 * surprise kernel}. */
int azh_samples_surprise_ms(const azh_samples *s, float *ms);
/* The legal moves of a position as policy indices in the order above -> index_out [up to 833], *n_out; no move goes onto a
 * cell of `blockers` (0: no walls).  Host arithmetic. */
int azh_samples_legal(uint64_t mover, uint64_t opponent, uint64_t blockers, uint16_t *index_out, int32_t *n_out);
/* One ply's surprise restated on the host: *kl_out is the stored value (the "stored as 0" rule applied), *illegal_out (or
 * NULL) this ply's count.  Host arithmetic only. */
int azh_samples_surprise_host(const float *logits833, const uint16_t *legal_index, int n_legal, const uint16_t *target_index,
                              const float *target_weight, int n_targets, float *kl_out, int32_t *illegal_out);
/* The same with `legal` found here: azh_samples_legal of the position. */
int azh_samples_surprise_host_blockers(const float *logits833, uint64_t mover, uint64_t opponent, uint64_t blockers,
                                       const uint16_t *target_index, const float *target_weight, int n_targets, float *kl_out,
                                       int32_t *illegal_out);

/* Weighted ply draws.  w [plies of games first_game .. first_game + n_games): one weight per ply, finite and >= 0.  Per
 * CANDIDATE ply the store keeps q = (u32)floor((double)w * 65536 + 0.5) as a running sum per game, cum[first ply + k] = q_0 +
 * ... + q_k over the game's candidates 0 .. k (a u32 beside the candidates array); the weights of other plies are checked and
 * otherwise unused.  -1, with nothing changed, for a weight that is NaN, infinite or negative, or a game whose total
 * exceeds 2^32 - 1.  Games never given weights, and games added later, have q = 65536 on every candidate.
 * With weights present an attempt of azh_samples_draw_gather picks its ply as
 *   total = the game's last cum; total == 0 fails the attempt (also for a game with random_ply);
 *   R = ((u64)v[1] * total) >> 32;  ply = the candidate at the first k with cum[k] > R (binary search, at most 16 steps);
 * everything else — game, random_ply + 1, the rejections, symmetry, the 64 attempts, the Philox counters — is unchanged.  With
 * every q = 65536 this is the uniform draw exactly: floor(floor(v c 2^16 / 2^32) / 2^16) = floor(v c / 2^32).
 * Neither call may run while a draw is in flight: both wait for the device first.
 * azh_samples_clear_ply_weights frees the array; the draw is again the one above. */
int azh_samples_set_ply_weights(azh_samples *s, int64_t first_game, int64_t n_games, const float *w);
int azh_samples_clear_ply_weights(azh_samples *s);
/* The draw's mirror: candidates [plies] (the k-th candidate of game g at [first ply + k]), candidate_count [games], cum
 * [plies] (valid below each game's count; 65536 (k + 1) throughout when the store holds no weights), *present: 1 when it
 * does.  azh_samples_draw restates the weighted draw from candidates and cum. */
int azh_samples_ply_cum(const azh_samples *s, uint16_t *candidates, uint32_t *candidate_count, uint32_t *cum, int32_t *present);

/* ------------------------------------------------------------------ auxiliary targets
 * (an extension of the store; with none of these called, every byte written above is what it was.)  Three further training
 * targets per sample — who ends up owning each cell, by how many stones the game is won, what the opponent answers — from what
 * the store already holds plus the end of each game.
 *
 * Final position.  The final position F of a stored game is the position after the move played at its last recorded ply.  The
 * side to move at ply p is x for even p, as everywhere in the store.  So F has x to move iff `plies` is even.  A last move of
 * "pass" only hands the turn over.
 * F is TERMINAL iff the kernels' adjudication gives a result there.  The order of checks is the one of wave_movegen:
 *   1. a side without stones loses;
 *   2. else a side to move without a move hands every empty cell to its opponent;
 *   3. a full board goes to the larger count, and a tie goes to x.
 *
 * Owners (two 49-bit masks per game).  Bit = file + 7 * rank, the ring record's layout.  Both masks are 0 when F is not
 * terminal.  That covers games cut at the ply limit, resigned games and truncated files.  When F is terminal, each cell is
 * assigned as follows:
 *   - a stone belongs to its colour;
 *   - a wall belongs to nobody;
 *   - an empty cell belongs to the only side that has stones, if one side has none;
 *   - otherwise an empty cell belongs to the side NOT to move in F (the mover is stuck).
 * The masks are therefore disjoint, disjoint from the walls, and together cover every non-wall cell.
 * Let margin_x = popcount(x-owned) - popcount(o-owned).  It must agree with the recorded result: > 0 => 1, < 0 => 2, = 0 => 1.
 * A game where it does not is refused at ingest (-2, the game named, nothing added).
 * The reference's Python result() differs from the kernels' order on one freak board: the mover is stuck and the opponent has
 * no stones (and a cell is empty).  Such a final position is refused: azh_samples_final_owners returns -2 there.
 *
 * Per-sample outputs.  Each sample is a (game g, ply p, symmetry s) with mover m = 1 + p % 2.  All outputs are f32.
 *   - ownership [n][7][7]: cell [X][Y] of the image under s, using the same source-cell map as feature planes 1-3.  It holds
 *     +1 where the source cell is owned by m, -1 where owned by the opponent, and 0 on walls.  It is all zeros when the game
 *     has no owners.
 *   - score [n][1]: popcount(owned by m) - popcount(owned by the opponent) as a float.  This is an exact integer in -49..49.
 *     It is 0 without owners.
 *   - reply [n][7][7][17]: the policy target of ply p + 1, each weight placed at azh_symmetry_policy_index(s, index), exactly
 *     as `policy` is built for ply p.  The row is all zeros unless the reply is present.
 *   - The reply is PRESENT iff all three hold: p + 1 < plies; ply p + 1 is neither PASS nor BAD; and the game either has no
 *     "full" or ply p + 1 is FULL.
 *   - aux_weight [n][2]: {1.0 if the game has owners else 0.0, 1.0 if the reply is present else 0.0}.
 *   - A failed device draw (g < 0) writes zeros everywhere, the weights included.
 * All values are exact: small integers, or single f32 weights landing on distinct cells.
 *
 * azh_samples_final_owners: host arithmetic only, no device and no store.  Applies the ring record's 16-bit move (from |
 * to << 8, a clone has from == to, PASS is 0xFFFF) for the side to move (o iff o_to_move) to the position (x, o) on a board with
 * walls `blockers`, and returns the owners of the position reached in owners_out [2] (x-owned, o-owned) and its result in
 * *result_out (0, with owners 0, when it is not terminal).  -2 for a move that is not legal there — a pass with a move
 * available, a source that is not the mover's, a destination that is not empty, a wrong distance, a stone or destination on a
 * wall — found with the move list of azh_samples_legal, and for the freak board above. */
int azh_samples_final_owners(uint64_t x, uint64_t o, uint64_t blockers, int o_to_move, uint32_t move, uint64_t *owners_out,
                             int32_t *result_out);
/* azh_samples_add_games with game_owners: the store keeps them in a device array [cap_games][2] that is allocated when the
 * first game with non-zero owners arrives.  -2, store unchanged, the game named, for: overlapping masks; bits on walls or
 * beyond the 49 cells; non-zero masks that leave a non-wall cell unowned; a margin that contradicts the result.
 * azh_samples_check_owners: that check of one game's owners against its walls and its recorded result, by itself: 0, or -2
 * with the reason in azh_last_error.  Masks that are both 0 pass.  Host arithmetic only: no device, no store. */
int azh_samples_check_owners(uint64_t own_x, uint64_t own_o, uint64_t blockers, uint32_t result);
/* azh_samples_pack_records / azh_samples_add_records under aux: each game's owners are azh_samples_final_owners of its last
 * ply's boards and move word with the record's walls.  A record whose last move is not legal at its last board is -2, with
 * nothing written (also when only the counts are asked for).
 * azh_samples_game_owners: the host mirror of the owners, owners [games][2]. */
int azh_samples_game_owners(const azh_samples *s, uint64_t *owners);

/* ------------------------------------------------------------------ reanalysis of stored plies
 * (an extension of the store; with none of these called, every call, launch and byte above is what it was.)  A stored ply's
 * policy target and value are replaced by what a fresh search of its position gives (MuZero's Reanalyse): the positions are read
 * back (azh_samples_read_plies), an engine searches them without playing a move (azh_engine_set_positions, AZH_FLAG_NO_REUSE,
 * visits + 1), its root reports stay on the device (azh_engine_root_report_device) and a kernel of the store turns them into
 * targets (azh_samples_retarget).  training.reanalyse drives the rounds; DESIGN.md section 4, "Reanalysis of stored plies".
 *
 * azh_samples_read_plies: a host read-back of n stored plies, plies [n][2] = (game, ply): boards_out [n][2] (x, o),
 * values_out [n], flags_out [n] (AZH_SAMPLES_PLY_*), target_start_out [n + 1] (the running sum of the plies' target counts
 * from 0) and, unless index_out and weight_out are both NULL, the targets in stored order behind one another, cap_targets
 * being the room of those two arrays.  A small gather kernel, then a copy; waits for the store's stream.  -1 for a pair
 * outside the store (checked against the mirror before any launch) or one of the two arrays without the other, -6 when
 * cap_targets is too small (the counts have been written by then: target_start_out [n] says how much room is needed). */
int azh_samples_read_plies(azh_samples *s, int n, const int32_t *plies /* [n][2] (game, ply) */,
                           uint64_t *boards_out /* [n][2] x, o */, double *values_out /* [n] */,
                           uint8_t *flags_out /* [n] */, int32_t *target_start_out /* [n + 1] */,
                           uint16_t *index_out, float *weight_out, int64_t cap_targets);
/* Diagnostic: where the targets of those plies lie, out [n][2] = (first target, counted from the store's first; targets), read
 * from the device like azh_samples_read_plies.  tests/reanalyse_gpu_checks.py checks azh_samples_retarget's placement on it. */
int azh_samples_ply_targets(azh_samples *s, int n, const int32_t *plies /* [n][2] */, uint32_t *out /* [n][2] */);
/* The definition, stated once; azh_samples_retarget (device) and azh_samples_retarget_host (host arithmetic) both follow it.
 * A RECORD r is one slot's AZH_ROOT_REPORT_WORDS words of azh_engine_root_report.  M = r[1]; edge j < M has move r[4 + 4 j],
 * visits r[5 + 4 j] and total score W = the f32 in r[6 + 4 j].
 *   MALFORMED: M > AZH_MAX_MOVES, or an edge j < M with visits > 0 whose move word is no clone and no jump over a distance of
 *     two between two of the 49 cells (from | to << 8, nothing above bit 15).
 *   total = the sum of the visits of the edges j < M, as a u64.
 *   UNCHANGED: total == 0 (M == 0 among it) or r[3] != 0 (a finished root): the ply stays exactly as it was, status 0.
 *   Otherwise the NEW TARGET is, for the edges j < M with visits_j > 0 in edge order, the pair
 *     index = the engine's move -> policy index map of move_j,  weight = (float)((double)visits_j / (double)total)
 *   — the rule azh_samples_pack_records applies to a game line's counts — and the NEW VALUE comes from the edge b with the most
 *   visits, the first in edge order on a tie: q = W_b / (float)visits_b, one IEEE f32 division, and
 *     value = isfinite(q) ? 2.0 * (double)q - 1.0 : 0.0,
 *   the record rule under kind & 16.  The value is always written; it is read, as before, only for games that have values.
 *
 * azh_samples_retarget_host: one record -> its new pairs in index_out / weight_out [up to AZH_MAX_MOVES], their number in
 * *n_out (0: unchanged, *value_out is then 0.0) and the value in *value_out.  -2 for a malformed record.  Host arithmetic only,
 * usable without a device.
 *
 * azh_samples_retarget: ply i of plies [n][2] = (game, ply) takes record i of d_reports, a DEVICE array
 * [n][AZH_ROOT_REPORT_WORDS].  status_out [n] on the host: 1 changed, 0 unchanged.
 * Placement.  New targets are appended: with T the store's target count before the call, changed ply i gets first_target =
 * T + (the sum of the new counts of the changed plies < i) and its new count; its flag byte is untouched, the old pairs stay
 * where they are, unreferenced; azh_samples_counts reports the new total and later azh_samples_add_games calls append behind it.
 * A reanalysed ply stays the candidate it was.
 * Checked on the host first, against the mirror, nothing launched: -1 for a pair out of range, a pass ply, a ply that is
 * not among its game's candidates (not FULL in a game that has "full") or a pair given twice; -2 for a BAD ply, and for
 * report_blockers (the walls the reports were searched on) differing from the game's stored mask (0 for a game without one).
 * Then two phases, so that a refused call changes nothing.  Phase 1, one wave per record, counts the new targets and marks
 * malformed records; an exclusive scan of the counts in call order follows and the host reads the total and the number of
 * malformed records: any malformed record -> -2, a total that does not fit beside T in the store's target capacity -> -6,
 * nothing written either time.  Phase 2, one wave per record, writes the pairs, the value and the ply's two target words.
 * The call waits for the store's own stream and for `stream` (0: none) before it writes, runs on the store's stream and
 * returns after completion.  It must not run while a minibatch call is in flight on another stream.  The per-ply surprise
 * kept by azh_samples_surprise is stale for changed plies: run the surprise pass afterwards. */
int azh_samples_retarget(azh_samples *s, int n, const int32_t *plies /* [n][2] */,
                         const uint32_t *d_reports /* DEVICE [n][AZH_ROOT_REPORT_WORDS] */, uint64_t report_blockers,
                         int32_t *status_out /* [n] */, uintptr_t stream);
int azh_samples_retarget_host(const uint32_t *report /* one record */, uint16_t *index_out, float *weight_out, int32_t *n_out,
                              double *value_out);

/* ------------------------------------------------------------------ proven outcomes for stored plies
 * (an extension of the store; with azh_samples_prove never called, every call, launch and byte above is what it was.)  The
 * alpha-beta search proves stored plies won or lost, and the minibatch kernels train a proven ply's value on the proven outcome
 * instead of the game's result (what tablebase rescoring does for lc0's training data).  training.train drives it under
 * train.py --prove-depth; DESIGN.md section 4, "Proven outcomes for stored plies".
 *
 * The definition, stated once.  The position of stored ply q of game g is (x, o, turn = q & 1, the game's stored wall mask, 0
 * for a game without one).  (move, value, depth_done, nodes) are exactly what azh_alphabeta_search reports for that position at
 * (depth, node_budget): the same iterative deepening, the same rule that abandons an iteration under a budget, the same node
 * count.
 *   proof(q) = value if |value| >= 1000, else 0.  Sound at any completed iteration: material scores are at most 49 in
 *   magnitude, so a value of 1000 or more is a forced adjudicated end.  A stored position that is already finished is proven by
 *   rule 1, and its move is 0xFFFF.
 *   ELIGIBLE are the plies training.reanalyse_plan calls eligible — the candidate plies (every ply, or the FULL ones of a game
 *   that has "full") of games [first_game, first_game + n_games) that are neither PASS nor BAD — which also have proof == 0.
 *   They are visited in ascending (game, ply) order.  A proof, once set, is never removed or changed: a later call skips the ply.
 *
 * azh_samples_prove searches every eligible ply, one wave per ply on the store's own records, and writes this call's counts to
 * stats_out: VISITED the eligible plies searched, WINS and LOSSES the new proofs by sign, CONTRADICTED the new proofs whose sign
 * differs from the mover's z ((game word 2 & 0xFF) == 1 + (ply & 1) -> +1, else -1), RETARGETED the policy targets replaced,
 * NODES the sum of the searches' node counts.
 * Storage.  Proofs live in an array of their own, one 16-bit word per ply the store can hold, allocated by the first call that
 * commits; beside it lie the move and the completed iteration of every ply's LAST search (0xFFFF and 0 before one), which
 * azh_samples_proofs reads back from the device like azh_samples_read_plies: proof_out, move_out, depth_done_out [n].
 * Minibatches.  Once the array exists, the four gather / draw-gather kernels write proof > 0 ? 1.0f : -1.0f as the value target
 * of a sample whose ply has proof != 0, whatever z, value_blend and the stored value say.  Features, policy, the auxiliary
 * outputs and the draws do not change; without the array the kernels write what they wrote.
 * retarget_wins != 0: each ply newly proven in this call with proof > 0 and move != 0xFFFF gets the single policy pair (the
 * engine's policy index of move, 1.0f), appended by azh_samples_retarget's placement rule in visiting order: first_target = T +
 * (the number of such plies before it), count 1, the old pairs stay unreferenced, flag byte and stored value untouched,
 * azh_samples_counts reports the new total.  Rule 1 scores 1000 + the remaining depth, so the quickest win is the move.  Proven
 * losses keep their recorded policy.
 * Refusals, in this order, each changing nothing: -1 a null argument or a game range outside the store; -2 the limits of
 * azh_alphabeta_search (depth 1 .. AZH_ALPHABETA_MAX_DEPTH, node_budget 0 up to AZH_ALPHABETA_UNBOUNDED_DEPTH only, else at
 * least AZH_MAX_MOVES); -6 with retarget_wins, the new pairs do not fit in the target capacity.  Hence two phases: every search
 * goes to scratch memory, in launches of 16384 plies, the host counts, and only then one kernel commits proofs and pairs.
 * Streams as azh_samples_retarget: the call waits for the store's stream, runs on it and returns after completion; it must not
 * run while a minibatch call is in flight on another stream; the surprise kept by azh_samples_surprise is stale for retargeted
 * plies. */
enum { AZH_PROOF_VISITED, AZH_PROOF_WINS, AZH_PROOF_LOSSES, AZH_PROOF_CONTRADICTED, AZH_PROOF_RETARGETED, AZH_PROOF_NODES,
       AZH_SAMPLES_PROOF_STAT_COUNT };
int azh_samples_prove(azh_samples *s, int64_t first_game, int64_t n_games, int depth, uint64_t node_budget, int retarget_wins,
                      uint64_t *stats_out /* [AZH_SAMPLES_PROOF_STAT_COUNT], this call's */);
int azh_samples_proofs(azh_samples *s, int n, const int32_t *plies /* [n][2] (game, ply) */, int32_t *proof_out,
                       uint16_t *move_out, int32_t *depth_done_out);

/* ------------------------------------------------------------------ lambda-returns as value targets
 * (an extension of the store; with azh_samples_value_returns never called, or after azh_samples_clear_value_returns, every call,
 * launch and byte above is what it was.)  The value target of a stored ply becomes the TD(lambda) return over the search values
 * of the plies that follow it, closed with the game's result (KataGo's short-term value targets; MuZero trains on n-step
 * returns).  training.train drives it under train.py --value-lambda; DESIGN.md section 4, "Lambda-returns as value targets".
 *
 * The definition, stated once; azh_samples_value_returns (device), azh_samples_value_returns_host (host arithmetic) and
 * tests/lambda_reference.py (Python floats) all follow it.  Take a stored game of T plies that carries values (game word 2 has
 * bit 9, "values") and lambda in [0, 1].  The mover of ply p is x for even p.  z_p = +1 when (game word 2 & 0xFF) == 1 + (p & 1),
 * else -1 — the integer the minibatch kernels compute, also for a game without a result.  v_p is the ply's stored value.  For
 * p = T - 1 down to 0:
 *     next = z_p          if p == T - 1
 *          = -G_{p+1}     otherwise
 *     G_p  = (1.0 - lambda) * v_p + lambda * next
 * in four IEEE double operations in exactly this order: a = 1.0 - lambda, b = a * v_p, c = lambda * next, G_p = b + c, none of them
 * fused.  Where the store has proofs and proof(p) != 0, G_p is exactly +1.0 or -1.0 by the proof's sign instead, and the
 * recursion goes on from that value: a proven ply corrects the targets of the plies before it.
 * Two identities follow from the arithmetic: lambda = 1 gives G_p = z_p bit for bit (for a game with a result: z alternates
 * with the mover; without one every z_p is -1 and G alternates from the last ply's), and lambda = 0 gives G_p = v_p bit for
 * bit (for v_p other than -0.0), the target of value_blend = 1.0.
 *
 * azh_samples_value_returns fills G_p for every ply of the games [first_game, first_game + n_games) that carry values, one wave
 * per game: the wave walks its game from the end in chunks of 64 plies, each lane loads one ply's value and proof, the chunk's
 * steps run in order on values read from the lanes' registers, and each lane stores its own ply's return.  Storage: one
 * double per ply the store can hold, allocated by the first call, every entry ABSENT until a call covers it (a game without
 * values is never covered).  A second call replaces the entries of its games and leaves every other entry as it was.
 * Minibatches.  While the array exists, the four gather / draw-gather kernels write (float)G_p as the value target of a sample
 * whose ply is covered, in place of z or the value_blend mix; a ply that is absent keeps its target.  Proofs stand above both,
 * as before; they already went into G_p, so a ply proven before the pass trains on +-1 either way.  Features, policy, the
 * auxiliary outputs and the draws do not change.
 * Order.  The pass reads the stored values and the proofs as they are when it runs.  azh_samples_retarget or azh_samples_prove
 * after it leave the returns stale: run the pass after them (training.train does: reanalysis, proofs, returns, surprise).
 * Calling it again recomputes.
 * azh_samples_clear_value_returns frees the array: minibatches are again what they were without it.
 * azh_samples_read_value_returns reads entries back from the device like azh_samples_proofs: out [n] (0.0 where absent) and
 * present [n] (1 covered, 0 absent; all 0 while there is no array).
 * Refusals, each changing nothing: -1 a null argument or a game range outside the store (n_games < 1 among them), -2 a lambda
 * that is not a number or lies outside [0, 1].
 * Streams as azh_samples_prove: the calls wait for the store's stream, run on it and return after completion; they must not
 * run while a minibatch call is in flight on another stream.
 *
 * azh_samples_value_returns_host: the definition itself for one game, host arithmetic only, usable without a device.  values
 * [T]; proofs [T] (azh_samples_proofs' proof words) or NULL; result the game's (0 .. 2); out [T].  -1 for a null argument or
 * T < 0, -2 for lambda as above. */
int azh_samples_value_returns(azh_samples *s, int64_t first_game, int64_t n_games, double lambda);
int azh_samples_clear_value_returns(azh_samples *s);
int azh_samples_read_value_returns(azh_samples *s, int n, const int32_t *plies /* [n][2] (game, ply) */, double *out /* [n] */,
                                   int32_t *present /* [n] */);
int azh_samples_value_returns_host(const double *values /* [T] */, const int32_t *proofs /* [T] or NULL */, int64_t T,
                                   uint32_t result, double lambda, double *out /* [T] */);

/* ------------------------------------------------------------------ reference ABI
 * The four symbols link.py:6-32 binds (cpp/self_play_client.cpp:683-749), with
 * the worker threads replaced by GPU game slots: `thread_count` concurrent
 * games are split into two halves of `buffer_entries` leaf rows; the host
 * evaluates a filled (buffer_entries,7,7,4) f32 buffer and hands back
 * (buffer_entries,7,7,17) posteriors (raw logits) + (buffer_entries,1) values.
 * (`shutdown` shadows the libc socket call of the same name exactly as the
 * reference's library does; define AZH_NO_REFERENCE_ABI to hide these.) */
#ifndef AZH_NO_REFERENCE_ABI
void launch_threads(char *output_path, int visits, float *fill_buffer1, float *fill_buffer2,
                    int buffer_entries, int thread_count);
int get_workload(void);
void complete_workload(int workload, float *posteriors, float *values);
void shutdown(void);
#endif

#ifdef __cplusplus
}
#endif
#endif
