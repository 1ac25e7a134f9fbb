/* alpharat_hip.h -- C-ABI of libalpharat_hip.so, the MI355X-native self-play MCTS sampler.
 *
 * These entry points are what the reference's FFI for the sampling hot path binds today through
 * PyO3 (module pyrat_engine._core, crates/alpharat-mcts-python/src/lib.rs:10-39). Each function
 * names the reference interface it replaces. Conventions kept from the reference: the callee owns
 * all game / tree memory, the caller passes scalars, plain pointers and UTF-8 paths, results are
 * returned by value in caller-owned structs; functions return 0 on success and a negative AR_E_*
 * code on failure (message via ar_last_error), and never throw across the boundary.
 * No torch types appear here; the library needs a HIP device and fails loudly without one.
 */
#ifndef ALPHARAT_HIP_H
#define ALPHARAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AR_ABI_VERSION 1

enum {
    AR_OK = 0,
    AR_E_INVALID = -1,  /* bad argument (reference: ValueError / panic on unknown maze_type) */
    AR_E_BACKEND = -2,  /* evaluator failure (reference: BackendError -> PyRuntimeError)       */
    AR_E_IO = -3,       /* bundle / weight file I/O (reference: SelfPlayError::Io -> PyIOError) */
    AR_E_DEVICE = -4,   /* no HIP device, HIP API error, kernel fault                           */
    AR_E_NOMEM = -5     /* device arena / host allocation failure                               */
};

/* crates/alpharat-mcts/src/search.rs:18-58  SearchConfig (same fields, same defaults) */
typedef struct ArSearchConfig {
    float c_puct;               /* 1.5   */
    float fpu_reduction;        /* 0.2   */
    float force_k;              /* 2.0   */
    float noise_epsilon;        /* 0.0   */
    float noise_concentration;  /* 10.83 */
    uint32_t collision_limit_min;     /* 1     */
    uint32_t collision_limit_max;     /* 256   */
    uint32_t collision_scaling_start; /* 800   */
    uint32_t collision_scaling_end;   /* 50000 */
    float collision_scaling_power;    /* 1.0; another power: the host tabulates the budgets, and
                                         collision_scaling_end - collision_scaling_start may be at most 4194304 */
} ArSearchConfig;

/* A full PyRat position: what `rust_mcts_search(game: PyRat, ...)` clones out of the engine
 * (crates/alpharat-mcts/src/bindings.rs:248). Cells are y-major, idx = y*width + x; directions
 * UP0 RIGHT1 DOWN2 LEFT3. cost[cell*4+dir]: 0 wall / board edge, 1 open, >=2 mud cost. */
typedef struct ArGameSpec {
    uint8_t width, height;
    uint16_t max_turns;
    uint16_t turn;
    uint8_t p1_x, p1_y, p2_x, p2_y;
    uint8_t p1_mud, p2_mud;
    float p1_score, p2_score;
    const uint8_t* cost;   /* [height*width*4]; NULL = open maze */
    const uint8_t* cheese; /* [height*width] 0/1 */
} ArGameSpec;

/* crates/alpharat-mcts/src/search.rs:304-325 SearchResult / bindings.rs:26-99 PySearchResult */
typedef struct ArSearchResult {
    float policy_p1[5], policy_p2[5];
    float value_p1, value_p2;
    float visit_counts_p1[5], visit_counts_p2[5];
    float prior_p1[5], prior_p2[5];
    uint32_t total_visits, nn_evals, terminals, collisions;
} ArSearchResult;

/* Leaf position handed to a host evaluator callback: what PyCallbackBackend wraps as PyRat
 * objects for `predict_fn(list[PyRat])` (crates/alpharat-mcts/src/bindings.rs:131-160). */
typedef struct ArLeaf {
    uint8_t p1_x, p1_y, p2_x, p2_y;
    uint8_t p1_mud, p2_mud;
    uint16_t turn;
    float p1_score, p2_score;
    uint64_t cheese_bits[4]; /* bit idx = y*width + x */
} ArLeaf;

/* predict_fn: fill policy_p1[n*5], policy_p2[n*5], value_p1[n], value_p2[n]; n <= batch_size.
 * Return 0, or non-zero to fail the search (-> AR_E_BACKEND, virtual losses reverted as in
 * search.rs:919-955). */
typedef int (*ArPredictFn)(void* user, const ArLeaf* leaves, uint32_t n, float* policy_p1, float* policy_p2,
                           float* value_p1, float* value_p2);

typedef struct ArNet ArNet; /* device-resident policy/value head (weights + workspace) */

const char* ar_version(void);
/* copies the calling thread's last error message; returns its length */
size_t ar_last_error(char* buf, size_t cap);
/* number of visible HIP devices, or AR_E_DEVICE */
int ar_device_count(void);
/* Game generation, host only (works without a device): the walls + mud (`cost_out[cells * 4]`: 0 wall / edge,
 * 1 open, >= 2 mud; directions UP RIGHT DOWN LEFT) and the cheese mask (`cheese_out[cells]`) that
 * ar_selfplay_run draws for the game seeded `seed` (= game_seed_base + game index). The reference leaves
 * both to the pyrat-rust engine (bindings.rs:502-532), which is not available: own generators, DESIGN.md
 * "game generation". Player cells are y * width + x. */
int ar_generate_maze(uint8_t width, uint8_t height, float wall_density, float mud_density, int symmetric, uint64_t seed,
                     uint8_t* cost_out);
int ar_generate_cheese(uint8_t width, uint8_t height, uint8_t p1_cell, uint8_t p2_cell, uint16_t count, int symmetric,
                       uint64_t seed, uint8_t* cheese_out);
/* hipDeviceSynchronize on `device` (benchmark bracketing) */
int ar_device_sync(int device);
/* The library keeps one tree-arena allocation per device between calls (the driver clears device
 * memory on allocation, seconds for a full MI355X; the reference's sampler likewise keeps its
 * thread pool and backend alive across play_games calls, selfplay.rs:600-660). This frees it, e.g.
 * before a training step that needs the HBM. AR_NO_ARENA_CACHE=1 in the environment disables the cache. */
int ar_release_device_memory(int device);

/* ---- evaluator: replaces OnnxBackend / TensorrtBackend (+ FlatEncoder) -----------------------
 * crates/alpharat-sampling/src/backends/onnx.rs:176-246, tensorrt.rs:423 ff., trt_shim.cpp:53-324.
 * `blob_path` is the weight blob written by alpharat_amd/weights.py from a .pt checkpoint. */
int ar_net_load(const char* blob_path, int device, ArNet** out);
void ar_net_free(ArNet* net);
/* Encode + forward `n` positions on the device. Outputs are host arrays:
 * policy_p1[n*5], policy_p2[n*5] (softmax), value_p1[n], value_p2[n] (softplus);
 * logits_p1/logits_p2 may be NULL. == model.predict(FlatObservationBuilder.build(...)) */
int ar_net_evaluate(ArNet* net, const ArGameSpec* games, uint32_t n, float* policy_p1, float* policy_p2,
                    float* value_p1, float* value_p2, float* logits_p1, float* logits_p2);
/* Device FlatEncoder (flat_encoder.rs:52-125): obs[n * (w*h*7+6)] on the host. */
int ar_encode(const ArGameSpec* games, uint32_t n, int device, float* obs);

/* ---- rust_mcts_search (crates/alpharat-mcts/src/bindings.rs:228-304) --------------------------
 * One search on a fresh tree. seed == NULL -> entropy. Evaluator: `net` if non-NULL, else
 * `predict_fn` if non-NULL (host callback per leaf batch), else SmartUniform. */
int ar_search(const ArGameSpec* game, const ArSearchConfig* cfg, uint32_t simulations, uint32_t batch_size,
              const uint64_t* seed, ArPredictFn predict_fn, void* user, ArNet* net, int device,
              ArSearchResult* out);
/* `n` independent searches in one launch set (evaluation-time callers: tournaments). seeds[n]. */
int ar_search_many(const ArGameSpec* games, uint32_t n, const ArSearchConfig* cfg, uint32_t simulations,
                   uint32_t batch_size, const uint64_t* seeds, ArNet* net, int device, ArSearchResult* out);

/* ---- rust_self_play (crates/alpharat-sampling/src/bindings.rs:268-483) ----------------------- */
typedef struct ArSelfPlayParams {
    /* game (make_games, bindings.rs:489-533) */
    uint8_t width, height;
    uint16_t cheese_count, max_turns;
    uint32_t num_games;
    int cheese_symmetric;       /* default 1 */
    const char* maze_type;      /* "open" | "classic" | "random" (generated mazes: our own seeded generator) */
    const char* positions;      /* "corners" | "random" */
    float wall_density, mud_density;
    int maze_symmetric;
    /* search */
    uint32_t simulations, batch_size;
    ArSearchConfig search;
    /* sampling */
    uint32_t num_threads;          /* accepted for drop-in compatibility; the device runs every game */
    const char* output_dir;        /* bundles go to output_dir/bundle_<uuid>.npz; NULL = keep in memory */
    uint32_t max_games_per_bundle; /* 32 */
    const char* weights_path;      /* NULL = SmartUniform; replaces onnx_model_path */
    const char* device;            /* "auto" | "hip" | "hip:N" | "mi355x"; anything else: AR_E_INVALID */
    uint32_t mux_max_batch_size;   /* accepted, unused: leaves are batched device-wide */
    uint64_t cache_size;           /* NN-eval cache entries, 0 = off */
    /* extensions (not in the reference signature) */
    int has_seed;                  /* 0: entropy (reference behaviour), 1: game i uses seeds below */
    uint64_t game_seed_base;       /* cheese layout of game i: game_seed_base + i */
    uint64_t rng_seed_base;        /* search/sampling stream of game i: rng_seed_base + i */
    uint32_t first_game_index;     /* shard offset: this call plays games first..first+num_games */
    uint32_t concurrent_games;     /* device-resident games (0 = choose from HBM size) */
    int device_index;              /* used when device == "auto"/"hip" */
} ArSelfPlayParams;

/* crates/alpharat-sampling/src/selfplay.rs:136-158 (+ derived rates computed by the caller) */
typedef struct ArSelfPlayStats {
    uint32_t total_games;
    uint64_t total_positions, total_simulations;
    double elapsed_secs;
    uint32_t p1_wins, p2_wins, draws;
    float total_cheese_collected;
    uint32_t total_cheese_available;
    uint32_t min_turns, max_turns;
    uint64_t total_nn_evals, total_terminals, total_collisions;
    uint64_t cache_hits, cache_misses;
    /* instrumentation for the roofline: tree levels traversed */
    uint64_t gather_node_visits, backup_node_visits, new_nodes;
    double device_secs; /* time inside step kernels (HIP events) */
    uint64_t steps;     /* batch steps launched */
    double gather_secs; /* time inside the gather kernel alone: HIP events around every launch, on its stream */
    uint64_t gather_launches;
} ArSelfPlayStats;

/* crates/alpharat-sampling/src/selfplay.rs:343-359: live counters in caller-owned memory, written
 * with relaxed atomic stores while ar_selfplay_run is blocking on another thread. */
typedef struct ArProgress {
    volatile uint32_t games_completed;
    volatile uint64_t positions_completed, simulations_completed, nn_evals_completed;
} ArProgress;

/* One finished game as the bundle writer sees it (selfplay.rs:80-132); arrays are only valid
 * during the callback. */
typedef struct ArGameRecordView {
    uint8_t width, height;
    uint16_t max_turns;
    uint32_t game_index, n_positions;
    const int8_t* maze;            /* [h*w*4] */
    const uint8_t* initial_cheese; /* [h*w]   */
    const uint8_t* cheese_outcomes;/* [h*w]   */
    float final_p1_score, final_p2_score;
    uint8_t result;                /* 0 draw 1 P1 2 P2 */
    uint16_t cheese_available;
    uint64_t total_simulations, total_nn_evals, total_terminals, total_collisions;
    /* position arrays, n_positions rows */
    const uint8_t* p1_pos;  /* [n*2] */
    const uint8_t* p2_pos;  /* [n*2] */
    const float* p1_score;  const float* p2_score;
    const uint8_t* p1_mud;  const uint8_t* p2_mud;
    const uint16_t* turn;
    const uint8_t* cheese_mask;   /* [n*h*w] */
    const float* value_p1;  const float* value_p2;
    const float* visit_counts_p1; const float* visit_counts_p2; /* [n*5] */
    const float* prior_p1;  const float* prior_p2;
    const float* policy_p1; const float* policy_p2;
    const uint8_t* action_p1; const uint8_t* action_p2;
} ArGameRecordView;
typedef void (*ArGameSink)(void* user, const ArGameRecordView* game);

/* Blocking. Plays params->num_games games, streams bundles to output_dir (atomic tmp->rename,
 * recording.rs:121-161) and/or hands each finished game to `sink`. */
int ar_selfplay_run(const ArSelfPlayParams* params, ArProgress* progress, ArGameSink sink, void* sink_user,
                    ArSelfPlayStats* out);

/* ---- the same run in slices (extension; the reference's worker pool lives for one call, selfplay.rs:721-808).
 * A session keeps the device engine, its resident games and the supply of new games alive between calls:
 *   ar_selfplay_open   sets up `concurrent_games` resident games (num_games == UINT32_MAX: the supply never
 *                      ends; game indices continue from first_game_index and wrap);
 *   ar_selfplay_step   runs `batch_steps` simulate_batch steps (search.rs:961) for every resident game
 *                      (UINT32_MAX: until all games are finished), with finished games drained to the sink /
 *                      bundle writer and their slots refilled, and reports in `window` what was done inside
 *                      this call: games finished, and positions / simulations / evaluations / node-visits per
 *                      finished MOVE (games still in flight count with the moves they completed);
 *                      *finished = 1 when no game is left;
 *   ar_selfplay_close  flushes the bundles, returns the totals of the finished games and frees everything.
 * ar_selfplay_run(p, ...) == open; step(UINT32_MAX); close. */
typedef struct ArSelfPlaySession ArSelfPlaySession;
int ar_selfplay_open(const ArSelfPlayParams* params, ArProgress* progress, ArGameSink sink, void* sink_user,
                     ArSelfPlaySession** out);
int ar_selfplay_step(ArSelfPlaySession* session, uint32_t batch_steps, ArSelfPlayStats* window, int* finished);
int ar_selfplay_close(ArSelfPlaySession* session, ArSelfPlayStats* total);

/* What the library chose for a session (the resident count may be smaller than `concurrent_games`: it is bounded by the
 * device memory the trees need). gather_kind: 0 one lane per game (k_gather), 1 eight lanes per game (k_gather8), 2 the
 * work queue over tree levels (k_gatherw), 3 fused SmartUniform step (k_step_uniform). */
typedef struct ArSessionInfo {
    uint32_t resident_games, groups, gather_kind;
    uint32_t gather_pass_limit; /* k_gatherw: passes per launch (UINT32_MAX: no limit) */
    uint64_t tree_region_bytes; /* device memory set aside for the trees */
    uint64_t host_grown_arenas; /* trees that outgrew a run of pages and were moved to an arena of their own */
    uint32_t idle_slots;        /* slots waiting for room in their zone of the tree region (resident games = resident_games - idle_slots) */
    float tree_pages_per_game;  /* what the resident set is sized by: pages a game of this run holds after a few moves */
} ArSessionInfo;
int ar_selfplay_info(const ArSelfPlaySession* session, ArSessionInfo* out);

/* ---- head-to-head matches (alpharat/eval/tournament.py:329-373 -> eval/game.py:47-87 play_game ->
 * ai/searcher_agent.py:40-56 SearcherAgent.get_move) --------------------------------------------
 * Two search agents play `num_games` games against each other, every game resident on the device from its first move
 * to its last. Game i is the game self-play generates for index first_game_index + i (board, maze, positions, cheese
 * from game_seed_base + index). Agent A plays P1, unless swap_sides != 0 and i is odd (tournament.py:397). Per turn each
 * agent searches the position on a fresh tree with its own evaluator, budget and configuration, drawing from its own
 * stream of this game (seeded rng_seed_base + index once per game, never re-seeded), and then samples its action from
 * the policy of the side it plays with one more draw from that stream (temperature 1.0, searcher_agent.py:53-54).
 * Neither agent's results depend on the other's stream, nor on how many games are resident.
 *
 * Agent kinds (alpharat/eval/benchmark.py:78-125, ai/config.py:64-137): besides a search agent, an agent can be
 *   AR_AGENT_RANDOM  ai/random_agent.py:17-19: one uniform draw over the five actions per move from its stream;
 *   AR_AGENT_GREEDY  ai/greedy_agent.py:23-84: the first step of the cheapest path (mud counted) to the nearest cheese,
 *                    directions tried UP, RIGHT, DOWN, LEFT, ties broken as the reference's (cost, push counter) heap does.
 * Both move at every turn, in mud or not. Neither has an evaluator, a tree or counters: weights_path must be NULL,
 * simulations / batch_size / search are ignored, and the agent's ArMatchSearchView rows and ArMatchStats counters are 0.
 * The reference's pure-network agent (ai/config.py:88-106) is a search agent with simulations = 1, batch_size = 1,
 * noise_epsilon = 0 and a temperature: the policy of such a search is the network's prior at the root. */
enum { AR_AGENT_SEARCH = 0, AR_AGENT_RANDOM = 1, AR_AGENT_GREEDY = 2 };

typedef struct ArMatchAgent {
    const char* weights_path; /* NULL = SmartUniform */
    uint32_t simulations, batch_size;
    ArSearchConfig search;
    uint64_t rng_seed_base;
    /* AR_AGENT_*; 0 (a search agent) is what every caller before these fields existed means */
    uint32_t kind;
    /* search agents only (ai/utils.py:26-40): 1.0 samples the policy of the side played as it is; 0.0 takes the first
     * index of its largest entry and draws nothing; any other value >= 0 samples exp(log(p + 1e-10) / temperature),
     * normalised, computed in double and rounded to float weights. Must be finite and >= 0. */
    float temperature;
} ArMatchAgent;

typedef struct ArMatchParams {
    /* game: as in ArSelfPlayParams */
    uint8_t width, height;
    uint16_t cheese_count, max_turns;
    int cheese_symmetric;
    const char* maze_type;
    const char* positions;
    float wall_density, mud_density;
    int maze_symmetric;
    uint32_t num_games, first_game_index;
    int has_seed;              /* 0: entropy for the games and both agents' streams */
    uint64_t game_seed_base;
    int swap_sides;            /* non-zero: agent B plays P1 in the odd games */
    uint32_t concurrent_games; /* device-resident games (0 = 4096) */
    const char* device;
    int device_index;
    ArMatchAgent a, b;
} ArMatchParams;

/* what one agent's searches returned, n_positions rows */
typedef struct ArMatchSearchView {
    const float* policy_p1; const float* policy_p2;             /* [n*5] */
    const float* value_p1;  const float* value_p2;              /* [n]   */
    const float* visit_counts_p1; const float* visit_counts_p2; /* [n*5] */
    const float* prior_p1;  const float* prior_p2;              /* [n*5] */
    const uint32_t* total_visits; const uint32_t* nn_evals;     /* [n]   */
    const uint32_t* terminals;    const uint32_t* collisions;   /* [n]   */
} ArMatchSearchView;

/* One finished game; arrays are only valid during the callback. */
typedef struct ArMatchGameView {
    uint8_t width, height;
    uint16_t max_turns;
    uint32_t game_index, n_positions;
    uint8_t a_is_p1;
    uint8_t result; /* 0 draw 1 P1 2 P2 */
    float final_p1_score, final_p2_score;
    const uint8_t* p1_pos;  /* [n*2] */
    const uint8_t* p2_pos;  /* [n*2] */
    const float* p1_score;  const float* p2_score;
    const uint8_t* p1_mud;  const uint8_t* p2_mud;
    const uint16_t* turn;
    const uint8_t* cheese_mask;   /* [n*h*w] */
    const uint8_t* action_p1; const uint8_t* action_p2;
    ArMatchSearchView a, b;
} ArMatchGameView;
typedef void (*ArMatchSink)(void* user, const ArMatchGameView* game);

/* tournament.py:61-72 MatchupResult as sums, plus the search counters per agent */
typedef struct ArMatchStats {
    uint32_t total_games, wins_a, wins_b, draws;
    float cheese_a, cheese_b; /* sums of the final scores */
    uint64_t total_positions;
    uint64_t simulations_a, simulations_b, nn_evals_a, nn_evals_b, terminals_a, terminals_b, collisions_a, collisions_b;
    double elapsed_secs;
} ArMatchStats;

/* Blocking. `sink` may be NULL. */
int ar_match_run(const ArMatchParams* params, ArMatchSink sink, void* sink_user, ArMatchStats* out);

/* Bundle writer on its own (recording.rs:23-162 write_bundle): used by the known-answer test. */
int ar_write_bundle(const ArGameRecordView* games, uint32_t n, const char* path);

/* ---- training rows (alpharat/data/sharding.py:513-595 _process_games_to_arrays: FlatObservationBuilder.build,
 * nn/builders/flat.py:142-197, and build_targets, nn/targets.py:19-70, once per position) -----------------------------
 * A row set keeps finished games on the device: their position records as the engine leaves them, a header per game and
 * the maze bytes; no observations. Its capacity in positions is fixed at open and allocated once; an append that does not
 * fit returns AR_E_NOMEM and changes nothing. Games come from host records (ar_rows_add_games) or, without visiting the
 * host, from a session the set is attached to. ar_rows_build writes output row i from stored position rows[i]: the
 * caller's order (a shuffle) is the gather index. The eight arrays are the BatchKey arrays of a shard
 * (nn/training/keys.py:52-62), n rows each, in host memory owned by the caller.
 * One caller at a time; an attached set outlives its session's last step and is closed after the session. */
typedef struct ArRowSet ArRowSet;
typedef struct ArTrainRows {
    float* observation;      /* [n][h*w*7 + 6]  as ar_encode                                                */
    float* policy_p1;        /* [n][5]                                                                      */
    float* policy_p2;        /* [n][5]                                                                      */
    float* value_p1;         /* [n]  final score - score at the position                                    */
    float* value_p2;         /* [n]                                                                         */
    int8_t* action_p1;       /* [n]                                                                         */
    int8_t* action_p2;       /* [n]                                                                         */
    int8_t* cheese_outcomes; /* [n][h][w]  the game's outcome where the position still has the cheese, else -1 */
} ArTrainRows;
int ar_rows_open(uint8_t width, uint8_t height, uint64_t capacity_positions, int device, ArRowSet** out);
/* host records, from bundles or a sink; the cheese outcomes are the view's. A game of another board size: AR_E_INVALID. */
int ar_rows_add_games(ArRowSet* set, const ArGameRecordView* games, uint32_t n);
/* before the session's first step: every game the session drains is appended on the device, cheese outcomes included.
 * A session that has stepped, a second attach, another board size or device: AR_E_INVALID. */
int ar_rows_attach(ArRowSet* set, ArSelfPlaySession* session);
int ar_rows_count(const ArRowSet* set, uint32_t* games, uint64_t* positions);
/* one entry per stored game, in append order (arrays of ar_rows_count's `games` entries; any may be NULL) */
int ar_rows_games(const ArRowSet* set, uint32_t* game_index, uint64_t* first_row, uint32_t* n_rows);
/* rows[n]: stored positions, each below ar_rows_count's `positions` (else AR_E_INVALID); n == 0 succeeds */
int ar_rows_build(ArRowSet* set, const uint64_t* rows, uint64_t n, const ArTrainRows* out);
/* time inside the kernels of the last ar_rows_build (HIP events), for measurements */
int ar_rows_build_time(const ArRowSet* set, double* kernel_ms);
/* ---- batches for a trainer, without the host copy (the reference's GPUDataset, nn/gpu_dataset.py, and its per-batch
 * PlayerSwapStrategy, nn/augmentation.py:86-184) ------------------------------------------------------------------------
 * The set keeps one order on the device: for every row of an epoch its stored position and whether the row is seen by P2
 * (swap[i] != 0: the planes, scalars, policies, actions and values of the two players exchanged, cheese outcome 0 <-> 3,
 * score difference negated). ar_rows_order_set checks every position (one beyond the set: AR_E_INVALID, the old order
 * stays), waits for the set's pending appends and for the last stream a batch was launched on, and replaces the order as
 * a whole; swap == NULL swaps no row. */
int ar_rows_order_set(ArRowSet* set, const uint64_t* rows, const uint8_t* swap, uint64_t n);
/* Rows first .. first + n of the order into `out_device`, whose eight arrays are the caller's device memory on the set's
 * device (n rows each, the float arrays 4-byte aligned), launched on `stream` (a hipStream_t; NULL: the null stream). It
 * only launches: no synchronisation, no copy, no allocation; the caller orders its reads behind `stream`. AR_E_INVALID
 * before any launch: no order set, first + n beyond the order, an array that is not device memory of the set's device
 * (hipPointerGetAttributes) or a misaligned float array. n == 0 succeeds and launches nothing. */
int ar_rows_build_device(ArRowSet* set, uint64_t first, uint64_t n, const ArTrainRows* out_device, void* stream);
/* forgets the games and drops the order */
int ar_rows_clear(ArRowSet* set);
void ar_rows_close(ArRowSet* set);

/* ---- validation of a checkpoint over stored positions (the validation pass of alpharat/nn/training/loop.py:306-361:
 * eval-mode forward, the loss of architectures/<arch>/loss.py, the detailed metrics of nn/metrics.py) --------------------
 * The request is walked in chunks: evaluator requests are written from the stored records, the evaluator runs with its
 * logits output, and one reduction sums the terms of every row; no observation and no target array is built. The sums
 * are additive over rows (two results over disjoint rows add to the result over their union) and are formed in double
 * from f32 terms without atomics: the same request gives the same bytes. For player p, with logits l, predicted value v
 * (softplus, as ar_net_evaluate), target policy t and target value y = final score - score at the position:
 *   ce          -sum_k t_k log_softmax(l)_k                      (F.cross_entropy with soft targets)
 *   sq_err      (v - y)^2                                        (F.mse_loss)
 *   ent_pred    -sum_k softmax(l)_k log_softmax(l)_k             (metrics.py:34-46)
 *   ent_target  -sum_k t_k log(max(t_k, 1e-8))                   (metrics.py:49-62)
 *   top1, top2  rank < 1, rank < 2, where a is the first index of the largest t_k and
 *               rank = #{k : l_k > l_a} + #{k < a : l_k == l_a}  (metrics.py:15-31; torch.topk leaves the order among
 *               equal logits open: taking the lower index first is this library's rule)
 *   sum_pred, sum_target, sum_pred2, sum_target2, sum_pred_target   v, y, v^2, y^2, v y (metrics.py:65-116) */
typedef struct ArValSums {
    uint64_t n;
    double ce[2], sq_err[2], ent_pred[2], ent_target[2];
    uint64_t top1[2], top2[2];
    double sum_pred[2], sum_target[2], sum_pred2[2], sum_target2[2], sum_pred_target[2];
} ArValSums;
/* per-row outputs in request order, host memory of n rows each; any array may be NULL */
typedef struct ArValRows {
    float* logits_p1; /* [n][5] */
    float* logits_p2; /* [n][5] */
    float* value_p1;  /* [n]    */
    float* value_p2;  /* [n]    */
} ArValRows;
/* rows[n]: stored positions as for ar_rows_build, in any order, repeats allowed. chunk_rows: rows per evaluator launch,
 * 0 = 65536 (a workspace of about 10 MB, kept in the set and grown to the largest chunk asked for). Blocks until the sums
 * are on the host; waits for the set's pending appends and batches first. n == 0 succeeds with zero sums. AR_E_INVALID,
 * with the set, the net and *sums untouched: a null set, net or sums; rows == NULL with n > 0; a row beyond the set's
 * positions; a net built for another board size; a net on another device. The net's maze constants are bound to the
 * set's mazes when they are not already; ar_net_evaluate binds its own again by itself. rows_out may be NULL. */
int ar_rows_validate(ArRowSet* set, ArNet* net, const uint64_t* rows, uint64_t n, uint32_t chunk_rows, ArValSums* sums,
                     const ArValRows* rows_out);

/* ---- validation of a local_value checkpoint (LocalValueMLP) with its ownership head ------------------------------------
 * The reference's val/loss for that architecture adds ownership_weight * loss_ownership
 * (architectures/local_value/loss.py:55-59): the cross-entropy of the head's per-cell logits [hw][4] against the game's
 * cheese outcomes over the cells that still hold their cheese (losses/ownership.py:26-46). The head is in an mlp blob that
 * alpharat_amd/weights.py wrote with keep_ownership (ownership_head.0 / .2, all four tensors or none; wrong shapes:
 * AR_E_BACKEND at load) and is built where the hidden width runs on the matrix cores (a multiple of 32, at most 256);
 * sampling, ar_net_evaluate and ar_rows_validate do with such a net exactly what they do with the plain blob.
 * 1 if `net` has the head, else 0 (a null net too). */
int ar_net_has_ownership(const ArNet* net);
/* ce and cells are additive over rows: the sum over active cells of logsumexp(l) - l[outcome], and their number. The
 * reference does not pool: per batch it takes ce_b / cells_b (0.0 for a batch without an active cell) and averages the
 * batches weighted by their size. With loss_batch_rows > 0 the request is cut into consecutive batches of that many rows,
 * the last one short: batch_weighted = sum_b B_b * (ce_b / cells_b), batch sums taken in row order. With
 * loss_batch_rows == 0, batch_weighted and batch_rows are 0. */
typedef struct ArOwnSums {
    uint64_t n, cells;
    double ce;
    double batch_weighted;
    uint64_t batch_rows;
} ArOwnSums;
/* per-row outputs in request order, host memory; any array may be NULL. A row's ce and value (the reference's
 * ownership_value under cheese_mask = cheese_outcomes >= 0) are sums over its active cells in increasing cell order,
 * accumulated in double from f32 terms. */
typedef struct ArOwnRows {
    double* ce;      /* [n]        */
    uint32_t* cells; /* [n]        */
    float* value;    /* [n]        */
    float* logits;   /* [n][hw][4] */
} ArOwnRows;
/* Everything ar_rows_validate does, with the same checks, refusals and waits; the evaluator also stores its trunk output,
 * from which the ownership head and the terms of every row are computed. chunk_rows is rounded up to a multiple of
 * loss_batch_rows. The workspace grows by chunk * H floats (64 MB at the default chunk and H = 256), 16 bytes a row and,
 * only when own_out->logits is asked for, chunk * hw * 16 bytes. *sums and rows_out are the bytes ar_rows_validate gives
 * for the same request in the same chunks. Additionally AR_E_INVALID with nothing touched: a net without an ownership
 * head, a null `own`. rows_out and own_out may be NULL. */
int ar_rows_validate_lv(ArRowSet* set, ArNet* net, const uint64_t* rows, uint64_t n, uint32_t chunk_rows,
                        uint32_t loss_batch_rows, ArValSums* sums, ArOwnSums* own, const ArValRows* rows_out,
                        const ArOwnRows* own_out);

/* ---- training gradients of PyRatMLP over stored rows (nn/models/mlp.py in training mode, the loss of
 * architectures/mlp/loss.py, loss.backward()) -----------------------------------------------------------------------------
 * The loss and the gradients of one batch -- rows first .. first + n of the order, with their swap flags, exactly the
 * rows ar_rows_build_device writes -- computed on the device in f32 and written into the caller's tensors. The
 * optimiser, the schedule and the checkpoints stay the caller's. Dropout is not applied here (the architecture's default
 * 0; with it: ar_rows_grad_mlp_dropout, below).
 * BatchNorm (both layers), over the batch: mu = mean(z), var = mean((z - mu)^2) (two passes), xhat = (z - mu) *
 * rsqrt(var + 1e-5), y = gamma * xhat + beta, then ReLU. Running statistics, when given: rm = 0.9 rm + 0.1 mu,
 * rv = 0.9 rv + 0.1 var * n / (n - 1). Heads: l1, l2 the policy logits, v = softplus(o) of the value head (v = o above 20).
 *   loss_pX       = mean(-sum_k t_k log_softmax(l)_k)       loss_value_pX = mean((v - y)^2)
 *   loss_value    = 0.5 (loss_value_p1 + loss_value_p2)     loss = policy_weight (loss_p1 + loss_p2) + value_weight loss_value
 * trunk0_b and trunk4_b sit in front of a BatchNorm, so their true gradient is zero: what is written is the column sum of
 * the layer's dz, rounding noise, as torch writes it. Sums over the batch use fixed partitions combined in a fixed order,
 * without atomics: the same request gives the same bytes. */
typedef struct ArMlpTensors { /* device pointers, f32, C order: PyRatMLP's state_dict tensors */
    float *trunk0_w, *trunk0_b;       /* [H][D], [H]      D = h*w*7 + 6 */
    float *bn1_w, *bn1_b;             /* [H]  trunk.1     */
    float *trunk4_w, *trunk4_b;       /* [H][H], [H]      */
    float *bn2_w, *bn2_b;             /* [H]  trunk.5     */
    float *p1_w, *p1_b, *p2_w, *p2_b; /* [5][H], [5]      */
    float *value_w, *value_b;         /* [2][H], [2]      */
} ArMlpTensors;
typedef struct ArMlpBnStats { /* running statistics [H], updated in place */
    float *mean1, *var1, *mean2, *var2;
} ArMlpBnStats;
typedef struct ArTrainOut { /* device memory of the caller's, any may be NULL */
    float* losses;                /* [6] loss_p1, loss_p2, loss_value_p1, loss_value_p2, loss_value, loss (batch means) */
    float *logits_p1, *logits_p2; /* [n][5] the training-mode outputs */
    float *value_p1, *value_p2;   /* [n] */
} ArTrainOut;
/* `grads` has the tensors of `params` and is overwritten, not accumulated into. running == NULL: no running statistic is
 * updated; out == NULL: nothing but the gradients is written. Launched on `stream` (a hipStream_t; NULL: the null stream)
 * with no synchronisation and no host copy; it allocates only when the set's training workspace must grow (the first
 * call, or a larger n or hidden_dim; about 30 MB at n = 4096, D = 349, H = 256). ar_rows_order_set, ar_rows_clear and
 * ar_rows_close wait for a pending step as they wait for pending batches. AR_E_INVALID before any launch, nothing
 * written: a null set, params or grads; no order set, or first + n beyond it; n < 2 (a training BatchNorm over one row
 * has no variance) or n > 65536; hidden_dim not a multiple of 32 or above 256; a null tensor in params, grads or
 * running; any given pointer that is not device memory of the set's device (hipPointerGetAttributes) or not 4-byte
 * aligned. */
int ar_rows_grad_mlp(ArRowSet* set, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArMlpTensors* params,
                     const ArMlpTensors* grads, const ArMlpBnStats* running, float policy_weight, float value_weight,
                     const ArTrainOut* out, void* stream);

/* ---- training gradients of SymmetricMLP over stored rows (nn/models/symmetric.py in training mode, the loss of
 * architectures/symmetric/loss.py, loss.backward()) -----------------------------------------------------------------------
 * ar_rows_grad_mlp for the second architecture: the same rows, the same loss (no third term), the same BatchNorm
 * arithmetic, ArTrainOut, streams, workspace (the two steps share the set's one workspace and wait for each other) and
 * refusals. With hw = h*w the inputs are columns of the flat row: shared_raw = [0, 4hw) + [6hw, 7hw) + scalar 1,
 * p1_raw = [4hw, 5hw) + scalars 2, 4, p2_raw = [5hw, 6hw) + scalars 3, 5. shared = se(shared_raw), p_i = pe(p_i_raw),
 * h_i = trunk(cat(shared, p_i)), agg = h_1 + h_2, logits_i = policy(cat(h_i, agg)), value_i = softplus(value(cat(h_i, agg))).
 * Seven BatchNorm applications over four modules: se1 sees the batch once; pe1, bn1 (trunk.1) and bn2 (trunk.5) are called
 * for P1's rows and then for P2's, each call with its own batch mean and variance, never pooled. Running statistics, when
 * given: P1's call updates first, P2's on top of it, rm = 0.9 (0.9 rm + 0.1 mu_1) + 0.1 mu_2, each variance with its own
 * n / (n - 1). The gradient of a shared tensor is the sum of its two calls' contributions, P1's before P2's. se0_b, pe0_b,
 * trunk0_b and trunk4_b sit in front of a BatchNorm: what is written there is the column sum of dz, rounding noise. */
typedef struct ArSymTensors { /* device pointers, f32, C order: SymmetricMLP's parameters in named_parameters() order */
    float *se0_w, *se0_b;       /* [H][5hw + 1], [H]   shared_encoder.0 */
    float *se1_w, *se1_b;       /* [H]                 shared_encoder.1 */
    float *pe0_w, *pe0_b;       /* [H][hw + 2], [H]    player_encoder.0 */
    float *pe1_w, *pe1_b;       /* [H]                 player_encoder.1 */
    float *trunk0_w, *trunk0_b; /* [H][2H], [H]        */
    float *bn1_w, *bn1_b;       /* [H]  trunk.1        */
    float *trunk4_w, *trunk4_b; /* [H][H], [H]         */
    float *bn2_w, *bn2_b;       /* [H]  trunk.5        */
    float *policy_w, *policy_b; /* [5][2H], [5]        */
    float *value_w, *value_b;   /* [1][2H], [1]        */
} ArSymTensors;
typedef struct ArSymBnStats { /* running statistics [H], updated in place */
    float *se_mean, *se_var, *pe_mean, *pe_var, *bn1_mean, *bn1_var, *bn2_mean, *bn2_var;
} ArSymBnStats;
/* As ar_rows_grad_mlp in every other respect: `grads` overwritten; running and out may be NULL; launched on `stream` with
 * no synchronisation; the workspace is about 151 MB at n = 4096, 7x7, H = 256 and about 2.2 GB at the cap of 65536 rows;
 * AR_E_INVALID before any launch, nothing written, for the same list (here twenty tensors, eight running statistics). */
int ar_rows_grad_symmetric(ArRowSet* set, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArSymTensors* params,
                           const ArSymTensors* grads, const ArSymBnStats* running, float policy_weight, float value_weight,
                           const ArTrainOut* out, void* stream);

/* ---- training gradients of LocalValueMLP over stored rows (nn/models/local_value.py in training mode, the loss of
 * architectures/local_value/loss.py, loss.backward()) ---------------------------------------------------------------------
 * ar_rows_grad_mlp for the third architecture of the family: the same rows, trunk, heads, BatchNorm arithmetic, streams,
 * workspace (the three steps share the set's one workspace and wait for each other) and refusals, plus the ownership head
 * on the trunk output A2 and its loss, over the window's cheese outcomes as ar_rows_build_device writes them (swapped rows:
 * classes 0 and 3 exchanged). With hw = h*w:
 *   Zo = A2 Wo0^T + bo0 [n][H]     Ao = relu(Zo)     L = Ao Wo2^T + bo2 [n][hw][4], class fastest
 *   a cell is active iff its cheese outcome is >= 0; C = the active cells of the window
 *   loss_ownership = (1/C) sum over active cells of logsumexp(l) - l[outcome]        (0 when C = 0)
 *   loss = policy_weight (loss_p1 + loss_p2) + value_weight loss_value + ownership_weight loss_ownership
 * The logits' gradient is (ownership_weight / C)(softmax(l) - onehot(outcome)) for an active cell and exactly 0 for any
 * other; C = 0 writes zeros into the head's four gradients (the reference's early return), and no NaN anywhere. The cells
 * are counted in integers, their terms added in double over a fixed partition in a fixed order: the same request gives the
 * same bytes. */
typedef struct ArLvTensors { /* device pointers, f32, C order: LocalValueMLP's parameters in named_parameters() order */
    float *trunk0_w, *trunk0_b;       /* ArMlpTensors' fourteen, as there */
    float *bn1_w, *bn1_b;
    float *trunk4_w, *trunk4_b;
    float *bn2_w, *bn2_b;
    float *p1_w, *p1_b, *p2_w, *p2_b;
    float *value_w, *value_b;
    float *own0_w, *own0_b;           /* [H][H], [H]        ownership_head.0 */
    float *own2_w, *own2_b;           /* [4hw][H], [4hw]    ownership_head.2 */
} ArLvTensors;
typedef struct ArLvTrainOut { /* device memory of the caller's, any may be NULL */
    float* losses;                /* [7] ArTrainOut's six (loss with the third term), then loss_ownership */
    float *logits_p1, *logits_p2; /* [n][5] the training-mode outputs */
    float *value_p1, *value_p2;   /* [n] */
    float* ownership_logits;      /* [n][h][w][4] the forward's L, copied out before dL takes its place */
} ArLvTrainOut;
/* As ar_rows_grad_mlp in every other respect: `grads` overwritten; running and out may be NULL; launched on `stream` with
 * no synchronisation (the copy of the logits is a device-to-device copy on that stream). hidden_dim a multiple of 32, at
 * most 256; 2 to 65536 rows; any board of the set. The workspace is the MLP step's plus 3 n H + 4 n hw floats and a few KB
 * of partial sums: about 46 MB at n = 4096, 7x7, H = 256, and at the cap of 65536 rows of 16x16 about 1.4 GB, of which L
 * is 268 MB. AR_E_INVALID before any launch, nothing written, for the same list (here eighteen tensors, four running
 * statistics, six outputs). */
int ar_rows_grad_local_value(ArRowSet* set, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArLvTensors* params,
                             const ArLvTensors* grads, const ArMlpBnStats* running, float policy_weight, float value_weight,
                             float ownership_weight, const ArLvTrainOut* out, void* stream);

/* ---- dropout in the three training steps (nn.Dropout in training mode behind every BatchNorm -> ReLU of the encoders and
 * the trunk) ----------------------------------------------------------------------------------------------------------------
 * Inverted dropout: a kept element of relu(bn(z)) is multiplied by scale = 1.0f / (float)(1.0 - (double)p), a dropped one is
 * exactly 0, and the backward multiplies the gradient of the kept elements by the same scale. No mask is stored (a dropped
 * element is 0 in the activation, which the backward already reads as its ReLU mask), so the workspace does not grow and no
 * launch is added. The mask is this library's own counter-based generator (alpharat_amd/csrc/dev_dropout.h), a pure function
 * of (seed, step, call, row, column) in wrapping 64-bit arithmetic, with G = 0x9e3779b97f4a7c15 and mix SplitMix64's finaliser:
 *   key  = mix(mix(mix(seed + G) + step * G + G) + call * G + G)         bits = mix(key + (row * H + column + 1) * G)
 *   thr  = floor(p * 2^32 + 0.5)                                          kept iff (bits >> 32) >= thr
 * `call` is the index of the BatchNorm call the dropout follows and `row` counts within that call's own n rows: PyRatMLP and
 * LocalValueMLP 0 = trunk.3, 1 = trunk.7 (the ownership head reads the trunk output behind the second); SymmetricMLP
 * 0 = shared_encoder, 1, 2 = player_encoder on P1's, P2's rows, 3, 4 = trunk.3 for P1, P2, 5, 6 = trunk.7 for P1, P2. It is
 * not torch's Philox stream: a step is reproducible from (seed, step) -- the same request gives the same bytes -- and is not
 * mask-for-mask equal to a torch run. The caller counts the steps. */
typedef struct ArTrainDropout { float p; uint64_t seed; uint64_t step; } ArTrainDropout;
/* The three steps with `dropout` in front of `stream`. dropout == NULL or p == 0: exactly the function without the suffix,
 * launch for launch (those are calls of these with NULL). AR_E_INVALID before any launch, nothing written, for that
 * function's list and for p < 0, p >= 1 or NaN. */
int ar_rows_grad_mlp_dropout(ArRowSet* set, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArMlpTensors* params,
                             const ArMlpTensors* grads, const ArMlpBnStats* running, float policy_weight, float value_weight,
                             const ArTrainOut* out, const ArTrainDropout* dropout, void* stream);
int ar_rows_grad_symmetric_dropout(ArRowSet* set, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArSymTensors* params,
                                   const ArSymTensors* grads, const ArSymBnStats* running, float policy_weight,
                                   float value_weight, const ArTrainOut* out, const ArTrainDropout* dropout, void* stream);
int ar_rows_grad_local_value_dropout(ArRowSet* set, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArLvTensors* params,
                                     const ArLvTensors* grads, const ArMlpBnStats* running, float policy_weight,
                                     float value_weight, float ownership_weight, const ArLvTrainOut* out,
                                     const ArTrainDropout* dropout, void* stream);
/* The mask of one call as the device's own generator gives it: keep_device [n][hidden_dim] bytes of device memory, 1 for a
 * kept element, 0 for a dropped one; launched on `stream` of the pointer's device, no synchronisation. AR_E_INVALID before any
 * launch: a null or non-device pointer; n == 0 or n > 65536; hidden_dim not a multiple of 32 or above 256; p < 0, p >= 1 or
 * NaN. */
int ar_train_dropout_mask(uint64_t seed, uint64_t step, uint32_t call, uint64_t n, uint32_t hidden_dim, float p,
                          uint8_t* keep_device, void* stream);

/* ---- training gradients of PyRatCNN over stored rows (nn/models/cnn/model.py in training mode as CNNModelConfig builds it by
 * default, the loss of architectures/cnn/loss.py, loss.backward()) ---------------------------------------------------------
 * ar_rows_grad_mlp for the fourth architecture: the same rows, the same loss (no third term), the same BatchNorm arithmetic
 * (BatchNorm2d over (N, H, W): R = n*hw values per channel, rv takes var * R / (R - 1)), ArTrainOut, streams, workspace and
 * refusals. With C = channels, PD = player_dim, HD = hidden_dim, B = n_blocks and hw = h*w:
 *   in = 5 planes of the flat row (channel d < 4 of a cell is column 4 cell + d, channel 4 is column 6hw + cell)
 *   x_0 = relu(stem_bn(stem(in))); per block x_b+1 = conv2(relu(bn2(conv1(relu(bn1(x_b)))))) + x_b; every convolution 3x3,
 *   padding 1, no bias, torch's cross-correlation with the weights in torch's [Cout][Cin][3][3] layout
 *   f_i = x_B at player i's cell (the 1 of columns [4hw, 5hw) for P1, [5hw, 6hw) for P2); side_i = [score, mud, progress],
 *   scalars 4, 2, 1 for P1 and 5, 3, 1 for P2; h_i = relu(comb(cat(f_i, relu(enc(side_i))))), agg = h_1 + h_2,
 *   logits_i = policy(cat(h_i, agg)), value_i = softplus(value(cat(h_i, agg))).
 * Every BatchNorm module is called once per step. The gradient of a tensor shared by both players is the sum of its two
 * calls' contributions, P1's before P2's. Not built, and refused by whoever fills these structs from a model
 * (alpharat_amd/train.py): PooledValueHead, KataGoCNN; GPoolResBlock and dropout are ar_rows_grad_cnn_gpool's, below. */
typedef struct ArCnnDims { uint32_t channels, player_dim, hidden_dim, n_blocks; } ArCnnDims;
typedef struct ArCnnBlock {     /* a ResBlock's parameters in named_parameters() order */
    float *bn1_w, *bn1_b;       /* [C]          */
    float* conv1_w;             /* [C][C][3][3] */
    float *bn2_w, *bn2_b;       /* [C]          */
    float* conv2_w;             /* [C][C][3][3] */
} ArCnnBlock;
typedef struct ArCnnTensors { /* device pointers, f32, C order: PyRatCNN's parameters in named_parameters() order */
    float* stem_w;              /* [C][5][3][3]        stem               */
    float *stem_bn_w, *stem_bn_b; /* [C]               stem_bn            */
    ArCnnBlock blocks[8];       /* the first n_blocks are read            */
    float *enc_w, *enc_b;       /* [PD][3], [PD]       player_encoder.0   */
    float *comb_w, *comb_b;     /* [HD][C + PD], [HD]  combiner.0         */
    float *policy_w, *policy_b; /* [5][2HD], [5]       policy_head.linear */
    float *value_w, *value_b;   /* [1][2HD], [1]       value_head.linear  */
} ArCnnTensors;
typedef struct ArCnnBlockStats { float *bn1_mean, *bn1_var, *bn2_mean, *bn2_var; } ArCnnBlockStats;
typedef struct ArCnnBnStats { /* running statistics [C], updated in place */
    float *stem_mean, *stem_var;
    ArCnnBlockStats blocks[8];
} ArCnnBnStats;
/* As ar_rows_grad_mlp in every other respect: `grads` overwritten; running and out may be NULL; launched on `stream` with
 * no synchronisation; the workspace holds 4 B + 5 activations of n*hw*C floats, about 0.9 GB at n = 4096, 7x7, C = 64,
 * B = 3. AR_E_INVALID before any launch, nothing written, for ar_rows_grad_mlp's list (here 11 + 6 B tensors
 * and 2 + 4 B running statistics, those of the first n_blocks blocks) and for: null dims; channels or hidden_dim not a
 * multiple of 32 or above 256; player_dim outside 1 .. 256; n_blocks above 8; a board of fewer than 2 or more than 256 cells;
 * n * hw above 2^22. */
int ar_rows_grad_cnn(ArRowSet* set, uint64_t first, uint64_t n, const ArCnnDims* dims, const ArCnnTensors* params,
                     const ArCnnTensors* grads, const ArCnnBnStats* running, float policy_weight, float value_weight,
                     const ArTrainOut* out, void* stream);

/* ---- PyRatCNN with GPoolResBlocks in its trunk and dropout (alpharat/nn/models/cnn/blocks.py; what
 * configs/train_cnn_7x7.yaml trains: res, res, gpool(32), dropout 0.1) --------------------------------------------------------
 * ar_rows_grad_cnn with any mix of ResBlock and GPoolResBlock among its blocks. A gpool block with G = gpool_channels has,
 * beside the ResBlock's regular path,
 *   ap = relu(pool_bn(x_b)); pz [n hw][G] = pool_conv(ap) (1x1, no bias); pool_cat [n][2G] = [mean | max over the hw cells];
 *   x_b+1 = (conv2(..) + pool_linear(pool_cat) broadcast over the cells) + x_b.
 * The mean is summed in cell order in double and rounded once; the maximum's gradient is shared evenly among the cells
 * that equal it, as torch's amax does. pool_bn is a BatchNorm module of its own with its own running statistics.
 * ArCnnPoolBlock holds a block's five further parameters in named_parameters() order, behind the block's six.
 * Dropout (p > 0): inverted dropout behind the ReLU of player_encoder and of combiner, from the generator described above.
 * Each module is called once per player on that player's n rows: call 0, 1 = player_encoder on P1's, P2's rows, call 2, 3 =
 * combiner on P1's, P2's rows; element e = row * H + column, row within the call's n rows, H = player_dim resp. hidden_dim.
 * The trunk has no dropout.
 * pool_dims == NULL or all zeros, and dropout == NULL or p == 0: ar_rows_grad_cnn launch for launch (that function is a call
 * of this one with NULLs). Per gpool block 21 launches more, and the workspace grows by ap [n hw][C], pz [n hw][G], pool_cat
 * [n][2G] and the tie counts [n][G]; with any gpool block once by one more array of n*hw*C floats, dpz [n hw][max G], po / dpo
 * [n][C] and dcat [n][2 max G]. AR_E_INVALID before any launch, nothing written, for ar_rows_grad_cnn's list and
 * for: a gpool_channels above 256; a null pool tensor (or, with `running`, a null pool statistic) of a block whose
 * gpool_channels != 0; n * hw above 65535 * 64 with a gpool block; p < 0, p >= 1 or NaN. */
typedef struct ArCnnPoolDims { uint32_t gpool_channels[8]; } ArCnnPoolDims; /* 0: a ResBlock; 1 .. 256: a GPoolResBlock */
typedef struct ArCnnPoolBlock {
    float *pool_bn_w, *pool_bn_b;         /* [C]           */
    float* pool_conv_w;                   /* [G][C][1][1]  */
    float *pool_linear_w, *pool_linear_b; /* [C][2G], [C]  */
} ArCnnPoolBlock;
typedef struct ArCnnPoolTensors { ArCnnPoolBlock blocks[8]; } ArCnnPoolTensors;
typedef struct ArCnnPoolStats { float *pool_bn_mean, *pool_bn_var; } ArCnnPoolStats; /* pool_running: an array of 8 */
int ar_rows_grad_cnn_gpool(ArRowSet* set, uint64_t first, uint64_t n, const ArCnnDims* dims, const ArCnnPoolDims* pool_dims,
                           const ArCnnTensors* params, const ArCnnPoolTensors* pool_params, const ArCnnTensors* grads,
                           const ArCnnPoolTensors* pool_grads, const ArCnnBnStats* running, const ArCnnPoolStats* pool_running,
                           float policy_weight, float value_weight, const ArTrainOut* out, const ArTrainDropout* dropout,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALPHARAT_HIP_H */
