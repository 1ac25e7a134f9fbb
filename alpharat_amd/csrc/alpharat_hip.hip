// libalpharat_hip.so -- HIP kernels + host runtime + C-ABI (include/alpharat_hip.h).
//
// Host runtime = the MI355X counterpart of crates/alpharat-sampling/src/selfplay.rs:609-808
// (game_worker_loop / run_self_play_to_disk): instead of N OS threads each walking one tree,
// every resident game advances one simulate_batch per kernel step; finished games are drained to
// a writer thread and their slots refilled from the pending game list.
//
// gfx950 only. No CPU path: every entry point needs a HIP device and fails with AR_E_DEVICE
// without one.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/alpharat_hip.h"
#include "nets.h"
#include "npz_writer.h"
#include "slot_layout.h"
#include "dev_gather8.h"
#include "dev_gatherw.h"
#include "dev_backup16.h"
#include "dev_advance.h"
#include "dev_match.h"
#include "dev_agents.h"
#include "dev_rows.h"
#include "dev_validate.h"
#include "train_mlp.h"
#include "train_sym.h"
#include "train_lv.h"
#include "train_cnn.h"
#include "train_gpool.h"
#include "host_games.h"
#include "zig_norm_tables.inc"

using namespace ar;

// ------------------------------------------------------------------------------------------------
// hardware queues
// ------------------------------------------------------------------------------------------------
// The step pipeline of a large run keeps four streams busy at once (two groups of games x {walk + evaluator, tree
// reuse}; group 0 runs on the engine's own stream). The HIP runtime maps streams onto its hardware queues (four by
// default, GPU_MAX_HW_QUEUES): streams that share a queue serialise, and the pipeline runs 1.1-1.7x slower than with
// one queue per stream (measured). The number of queues is the host's choice, made before the
// runtime initialises; the library never sets it. What is known about the queues is what the variable said when this
// library was loaded.
static int g_hw_queues_at_load = 0;
__attribute__((constructor)) static void ar_read_hw_queues() {
    const char* e = getenv("GPU_MAX_HW_QUEUES");
    g_hw_queues_at_load = e ? atoi(e) : 4;
}
static int hw_queues() { return g_hw_queues_at_load; }

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_error;
static int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}
static int nets_fail(int code, const std::string& msg) { return fail(code, msg); }
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(AR_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));           \
    } while (0)

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
template <int NW>
struct GameInit {
    Board board;
    State<NW> st;
    uint64_t rng_seed;
    uint32_t game_index;
    uint32_t slot;
    uint32_t single;
    uint32_t reset_arena;  // 1: the slot's grown arena was released, go back to its pool share
};

template <int NW>
struct DoneInfo {
    uint32_t slot, game_index, n_pos, error;
    State<NW> final_st;
    uint64_t t_sims, t_nn, t_term, t_coll, nv_gather, nv_backup, new_nodes;
    MoveResult last;
};

// Where the trees live. One allocation per device holds every game's arena, cut into PAGES of 768 nodes (243 KB with
// the nodes' share of the re-rooting table); a game owns one run of consecutive pages at a time, exactly as many as its
// kept tree plus one full search needs, and changes run when tree reuse re-roots the tree (k_advance rewrites every kept
// node anyway). A resident game so costs what its tree needs -- not a fixed first arena plus overflow blocks (rounds 1-2:
// 3.7 MB per game for 1.7 MB of live nodes, which capped the device at 65536 games).
// Which pages are taken is a bitmap, 64 pages to a word; a run lies inside one word (at most 64 pages = 49152 nodes;
// bigger trees get an arena from the host), so finding n free pages is bit arithmetic on one word and claiming them one
// atomic OR -- and pages that come back merge with their free neighbours by themselves (size classes with free lists
// were tried first: a session's games start in step, every class sees its peak demand once, and the region ends up
// cut into blocks of sizes nobody wants any more).
// Kernels only CLAIM pages and only APPEND runs they leave to the return lists; k_pool_merge (ordered after the kernels
// that could still read those pages) clears their bits -- so no page is handed out while an earlier kernel may read it.
// The region is cut into ZONES, one per 1024 consecutive slots, each with its own bitmap: a wavefront (and a CU) works on
// consecutive slots, and their trees then lie within a few GB of each other. With one pool for the whole device the
// trees of neighbouring slots ended up anywhere in 260 GB and every kernel that walks trees ran 2-3x slower, more so
// the longer the run (address translation: the big allocation is mapped with large fragments, and a CU that touches a
// few of them is served from its translation cache).
enum { POOL_PAGE_NODES = 768, POOL_WORD_PAGES = 64, POOL_ZONE_SLOTS = 1024 };
struct ArenaPool {
    unsigned long long* bits;   // [zones x zone_words] bit set: page taken
    unsigned long long* ret;    // [zones x ret_cap] runs left since the last merge: page index within the zone | pages << 32
    uint32_t* ret_n;            // [zones]
    uint32_t zone_words, zones, ret_cap;
    uint32_t page_nodes;        // nodes per page (768; the AR_ARENA_NODES test knob makes pages small)
    uint32_t fresh_pages;       // pages of a fresh game's arena
    unsigned long long page_bytes, zone_bytes;  // zone z is [z * zone_bytes, (z + 1) * zone_bytes) of the region
};

// The cost tables are read once or twice in every round of a gather (the step into the next child), in front of the
// round's record fetch: with one maze shared by all games (open mazes) -- or a handful, in batched searches -- the
// whole pool is copied into LDS at kernel start, which takes a dependent L2 round trip out of every round.
enum { MAZE_STAGE_BYTES = 4096 };

// the three bases every tree kernel receives; all per-game addresses derive from them
struct Bases {
    unsigned char* arena;    // pool of first arenas; grown arenas are addressed relative to it too
    unsigned char* scratch;  // S x layout.total
    const uint8_t* maze;     // cost tables
    uint32_t maze_stage;     // bytes of the whole maze pool when it is small enough to sit in LDS (else 0)
    SlotLayout L;
    ArenaPool pool;
};

// pages for `need` nodes; 0 when no run can hold them (more than one word of pages)
__device__ inline uint32_t pool_pages_for(const ArenaPool& P, uint32_t need) {
    const uint32_t n = (need + P.page_nodes - 1) / P.page_nodes;
    return n <= POOL_WORD_PAGES ? (n ? n : 1u) : 0u;
}
// A run of `n` free pages in the slot's zone: first fit from a start word that differs from slot to slot (games that
// look at the same time then look at different words). Returns the first page's index within the zone, NIL if none.
// Called by one thread.
__device__ inline uint32_t pool_claim(const ArenaPool& P, uint32_t slot, uint32_t n) {
    const uint32_t zone = slot / POOL_ZONE_SLOTS;
    unsigned long long* words = P.bits + (size_t)zone * P.zone_words;
    const unsigned long long run = n >= 64 ? ~0ULL : ((1ULL << n) - 1ULL);
    // (the start words cover the low end of the zone only: a zone that is far from full keeps its trees close together)
    uint32_t w = (slot * 7u) % (P.zone_words < 96u ? P.zone_words : 96u);
    for (uint32_t tries = 0; tries < P.zone_words; ++tries, w = w + 1 == P.zone_words ? 0 : w + 1) {
        for (int again = 0; again < 4; ++again) {  // (a few retries on a word others are claiming from too)
            const unsigned long long taken = __hip_atomic_load(&words[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            unsigned long long m = ~taken;  // bit p survives when pages p .. p + n - 1 are all free
            for (uint32_t len = 1; len < n && m;) {
                const uint32_t sh = len < n - len ? len : n - len;
                m &= m >> sh;
                len += sh;
            }
            if (!m) break;
            const uint32_t pos = (uint32_t)__ffsll((long long)m) - 1u;
            const unsigned long long mask = run << pos;
            const unsigned long long old = atomicOr(&words[w], mask);
            if ((old & mask) == 0) return w * POOL_WORD_PAGES + pos;
            atomicAnd(&words[w], ~(mask & ~old));  // someone was faster on part of it: give back what was ours, look again
        }
    }
    return NIL;
}
// where a slot's arena fields point when it owns `n` pages from page `first` of its zone
template <int NW>
__device__ inline void slot_at_pages(Slot<NW>& s, const Bases& B, uint32_t slot, uint32_t first, uint32_t n) {
    const uint32_t cap = n * B.pool.page_nodes;
    const long long base = (long long)((unsigned long long)(slot / POOL_ZONE_SLOTS) * B.pool.zone_bytes + (unsigned long long)first * B.pool.page_bytes);
    s.cap = cap;
    s.stats_off = base;
    s.fwd_off = base + (long long)cap * (long long)sizeof(NodeStats);
    s.pool_blk = n;
}
// the arena a slot leaves behind: pages go to the return list of their zone, host-grown arenas are flagged
// (in `s`, the slot as it will be written back; so is the error of a full return list)
template <int NW>
__device__ inline void leave_arena(const Slot<NW>& old, Slot<NW>& s, const Bases& B) {
    if (old.pool_blk) {
        const uint32_t zone = (uint32_t)((unsigned long long)old.stats_off / B.pool.zone_bytes);
        const uint32_t first = (uint32_t)(((unsigned long long)old.stats_off - (unsigned long long)zone * B.pool.zone_bytes) / B.pool.page_bytes);
        const uint32_t at = atomicAdd(&B.pool.ret_n[zone], 1u);
        if (at < B.pool.ret_cap) B.pool.ret[(size_t)zone * B.pool.ret_cap + at] = (unsigned long long)first | ((unsigned long long)old.pool_blk << 32);
        else s.error = 12;  // (the list holds a run per slot of the zone and then some: more cannot be left between two
                            // merges. A run that found it full would stay taken for good: the host's scan reports it)
    } else if (old.cap != 0) {
        s.release_grown = 1;
    }
}
// nodes a game needs room for when its kept tree has `cnt` nodes: the tree plus one full search
__device__ inline uint32_t arena_need(uint32_t cnt, const SearchCfg& cfg) { return cnt + cfg.n_sims + 2 * cfg.batch_size + 64; }

__global__ void k_pool_merge(ArenaPool P, uint32_t zone_first, uint32_t zone_count) {  // one block per zone
    if (blockIdx.x >= zone_count) return;
    const uint32_t zone = zone_first + blockIdx.x;
    if (zone >= P.zones) return;
    uint32_t n = P.ret_n[zone];
    if (n > P.ret_cap) n = P.ret_cap;
    unsigned long long* words = P.bits + (size_t)zone * P.zone_words;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const unsigned long long r = P.ret[(size_t)zone * P.ret_cap + i];
        const uint32_t first = (uint32_t)r, pages = (uint32_t)(r >> 32);
        const unsigned long long run = pages >= 64 ? ~0ULL : ((1ULL << pages) - 1ULL);
        atomicAnd(&words[first / POOL_WORD_PAGES], ~(run << (first % POOL_WORD_PAGES)));
    }
    __syncthreads();
    if (threadIdx.x == 0) P.ret_n[zone] = 0;
}

// Slot ownership across the two streams of a group. The tree walks (k_gather, k_backup) own a slot
// while it is ACTIVE; k_advance, on the side stream, owns it from the backup that ended a move (or the
// gather that stalled) until the compaction is done. No kernel may take over a slot from a kernel that
// is still running -- only a kernel boundary orders the writes (and writes back / invalidates the
// per-XCD L2s), and in-kernel agent-scope fences cost a full L2 write-back each. So every hand-off
// status carries the parity of the step that wrote it, and a kernel only accepts the parity whose
// writer the stream order has already completed:
//   backup(t) / gather(t) write ADVANCE / STALL tagged t&1  -> accepted by advance(t) only (launched after
//                                                             backup(t); advance(t-1) may still be running
//                                                             next to backup(t) and ignores this parity);
//   advance(t) writes READY tagged t&1                       -> accepted by gather(t+2), which waits for
//                                                             advance(t)'s event; gather(t+1) ignores it.
// Without the side stream everything runs in stream order with phase 0 and READY = ACTIVE.
enum { SLOT_STALL_B = 6, SLOT_ADVANCE_B = 7, SLOT_READY_A = 8, SLOT_READY_B = 9 };
__device__ inline uint32_t tag_status(uint32_t st, uint32_t phase) {
    if (phase == 0) return st;
    return st == SLOT_STALL ? (uint32_t)SLOT_STALL_B : st == SLOT_ADVANCE ? (uint32_t)SLOT_ADVANCE_B : st;
}

// per-game mazes (generated mazes): maze i of the upload goes to the pool entry of the slot game i starts in
template <int NW>
__global__ void k_place_mazes(const GameInit<NW>* init, uint32_t n, const uint8_t* stage, uint32_t stride, uint8_t* pool,
                              uint32_t* ids_out) {
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const uint32_t slot = init[i].slot;
    for (uint32_t b = threadIdx.x; b < stride; b += blockDim.x) pool[(size_t)slot * stride + b] = stage[(size_t)i * stride + b];
    if (threadIdx.x == 0) ids_out[i] = slot;
}

template <int NW>
__global__ void k_init_games(Slot<NW>* slots, const GameInit<NW>* init, uint32_t n, Bases B, SearchCfg cfg) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GameInit<NW> gi = init[i];
    Slot<NW> s = slots[gi.slot];
    // the block of the game that was here goes back (a host-grown arena was freed by the host already); the new game
    // takes one for a fresh tree
    if (s.pool_blk) {
        Slot<NW> unused = s;
        leave_arena(s, unused, B);
        if (unused.error) s.error = unused.error;
    }
    s.cap = 0;
    s.pool_blk = 0;
    s.board = gi.board;
    s.st = gi.st;
    rng_seed(s.rng, gi.rng_seed);
    s.game_index = gi.game_index;
    s.single_search = gi.single;
    const uint32_t off = pool_claim(B.pool, gi.slot, B.pool.fresh_pages);
    if (off != NIL) {
        slot_at_pages(s, B, gi.slot, off, B.pool.fresh_pages);
        const Mem<NW> m = resolve_mem<NW>(s, B.arena, B.scratch, gi.slot, B.L, B.maze);
        start_game(s, m, cfg);
    } else {
        // no block right now: the game waits as a tree to be re-rooted from nothing; k_advance gives it its arena
        // and its root when blocks have come back
        start_game_header(s, cfg);
        s.hi = 0;
        s.root = 0;
        s.node_count = 0;
        s.stats_off = s.fwd_off = 0;
        s.pending_root = NIL;
        s.status = (!s.single_search && st_over(s.board, s.st)) ? (uint32_t)SLOT_DONE : (uint32_t)SLOT_ADVANCE;
    }
    slots[gi.slot] = s;
}

// One lane walks one game's tree: `iters` x (gather -> evaluate -> backup [-> end of turn]).
// SmartUniform is evaluated inside the gather, so the whole simulate_batch is one pass. The slot
// header is copied to registers for the duration of the kernel.
template <int NW>
__global__ void __launch_bounds__(64) k_step_uniform(Slot<NW>* slots, uint32_t n_slots, SearchCfg cfg, Bases B,
                                                     const ZigTables* zt, int iters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    if (slots[i].status != SLOT_ACTIVE) return;
    Slot<NW> s = slots[i];
    const Mem<NW> m = resolve_mem<NW>(s, B.arena, B.scratch, i, B.L, B.maze);
    // (fused_machine -- lanes free-running across batch boundaries -- measured slower: it spreads the
    // wavefront over twice as many states per round)
    for (int it = 0; it < iters; ++it) {
        if (s.status != SLOT_ACTIVE) break;
        if (!gather_machine(s, m, cfg, EVAL_UNIFORM)) break;
        if (backup_machine(s, m, cfg, m.ev_local, zt)) finish_move(s, m, cfg);
    }
    slots[i] = s;
}

// Split form for evaluators that run outside the tree walk (networks, host callbacks).
template <int NW>
__global__ void __launch_bounds__(64) k_gather(Slot<NW>* slots, uint32_t n_slots, SearchCfg cfg, Bases B,
                                               LeafReq<NW>* queue, uint32_t* queue_count, uint32_t max_rounds,
                                               uint32_t first, uint32_t phase, uint32_t accept_ready) {
    // slots [first, n_slots) -- one group of games; one game per lane
    __shared__ uint32_t lds_maze[MAZE_STAGE_BYTES / 4];
    if (B.maze_stage) {
        for (uint32_t w = threadIdx.x; w < B.maze_stage / 4; w += blockDim.x) lds_maze[w] = ((const uint32_t*)B.maze)[w];
        __syncthreads();
    }
    const uint32_t i = first + blockIdx.x * 64u + threadIdx.x;
    if (i >= n_slots) return;
    {
        const uint32_t st = slots[i].status;
        if (st != SLOT_ACTIVE && st != accept_ready) return;
    }
    Slot<NW> s = slots[i];
    s.status = SLOT_ACTIVE;
    Mem<NW> m = resolve_mem<NW>(s, B.arena, B.scratch, i, B.L, B.maze);
    if (B.maze_stage) m.cost = (const uint8_t*)lds_maze + s.board.maze_off;
    // a batch that was already gathered and still waits for its backup is left alone
    const int got = s.batch_active ? GATHER_PENDING : gather_machine_limited(s, m, cfg, EVAL_STORE, max_rounds);
    if (got == GATHER_COMPLETE && queue != nullptr && s.b_nn > 0) {
        const uint32_t base = atomicAdd(queue_count, s.b_nn);
        s.eval_base = base;
        for (uint32_t j = 0; j < s.b_nn; ++j) {
            LeafReq<NW> r;
            r.st = m.leaf_local[j];
            r.slot = i;
            r.pad = 0;
            queue[base + j] = r;
        }
    }
    s.status = tag_status(s.status, phase);
    slots[i] = s;
}

// The same gather with eight lanes per game (dev_gather8.h): a wavefront holds eight games, an octet of lanes walks
// one tree together. Launched with ceil(n / 8) blocks of 64 threads. Trees, batch entries, counters and the leaf
// queue contents per game are identical to k_gather's; only the order in which games append to the queue differs.
template <int NW, int WPE>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) k_gather8(Slot<NW>* slots, uint32_t n_slots, SearchCfg cfg, Bases B,
                                                LeafReq<NW>* queue, uint32_t* queue_count, uint32_t first,
                                                uint32_t phase, uint32_t accept_ready) {
    const uint32_t ol = threadIdx.x & 7u;
    const uint32_t i = first + blockIdx.x * 8u + (threadIdx.x >> 3);
    __shared__ uint32_t lds_maze[MAZE_STAGE_BYTES / 4];
    bool run = i < n_slots;
    if (run) {
        const uint32_t st = slots[i].status;
        run = st == SLOT_ACTIVE || st == accept_ready;
    }
    const uint32_t ii = i < n_slots ? i : first;  // idle octets read a valid slot and store nothing
    Slot<NW>& S = slots[ii];
    OctMem<NW> m;
    m.stats = (NodeStats*)(B.arena + S.stats_off);
    m.scratch = B.scratch;
    m.maze = B.maze;
    if (B.maze_stage) {
        for (uint32_t w = threadIdx.x; w < B.maze_stage / 4; w += blockDim.x) lds_maze[w] = ((const uint32_t*)B.maze)[w];
        m.maze = (const uint8_t*)lds_maze;  // (the barrier below, in front of the rounds, orders these writes)
    }
    m.s_off = (uint32_t)((size_t)ii * B.L.total);  // (setup() keeps all games' scratch below 4 GB for this kernel)
    m.maze_off = S.board.maze_off;
    m.proc_off = (uint32_t)B.L.proc_off;
    m.coll_off = (uint32_t)B.L.coll_off;
    m.levels_off = (uint32_t)B.L.levels_off;
    m.leaf_off = (uint32_t)B.L.leaf_off;
    m.coll_cap = B.L.coll_cap;
    m.max_depth = B.L.max_depth;
    const Board board = S.board;
    __shared__ OctShared<NW> shared[8];
    __shared__ OutcomeTable otab;
    outcome_table_fill(otab);
    OctShared<NW>& sh = shared[threadIdx.x >> 3];
    Oct<NW> o;
    o.done = true;
    o.alloc_left = 0;
    o.error = 0;
    o.d_new = o.d_visits = 0;
    o.rounds = 0;
    o.batch_active = S.batch_active;
    bool stalled = false;
    // a batch that was already gathered and still waits for its backup is left alone
    const bool begin = run && o.batch_active == 0;
    if (begin) {
        // gather_begin (dev_search.h)
        o.hi = S.hi;
        o.cap = S.cap;
        o.root = S.root;
        o.node_count = S.node_count;
        const uint32_t remaining = S.remaining;
        o.batch = remaining < cfg.batch_size ? remaining : cfg.batch_size;
        if (o.hi + o.batch > o.cap) {
            stalled = true;
        } else {
            o.left = (long long)(int32_t)collisions_left(o.node_count, cfg);
            o.n_proc = o.n_coll = o.b_nn = o.b_term = o.b_coll = 0;
            o.depth = 0;
            o.node = 0;
            o.mask = 0;
            o.omap0 = o.omap1 = 0;
            o.pick_mv = 0;
            o.have_pick = false;
            o.work = S.st;
            sh.rng = S.rng;  // (all eight lanes store the same values: see best_of5)
            sh.root_st = S.st;
            o.n1 = o.n2 = 0;
            o.forced = 0;
            for (int k = 0; k < 2; ++k) {
                o.sc[k] = o.util[k] = o.num[k] = 0.0f;
                o.ns[k] = o.add[k] = o.nif0[k] = 0;
            }
            for (int k = 0; k < 4; ++k) {
                o.kid[k] = NIL;
                o.vtp[k] = 0;
            }
            o.done = false;
        }
    }
    __syncthreads();  // (one wavefront: the LDS writes above are visible to its other lanes)
    for (uint32_t guard = 0; guard < (1u << 22); ++guard) {  // (every game's gather ends; the bound is a fuse)
        if (!__any(!o.done)) break;
        gather8_round(o, sh, otab, board, m, cfg, ol);
    }
    __syncthreads();
    if (!run) return;
    if (begin && !stalled && !o.done) o.error = 8;  // the fuse blew
    uint32_t status = SLOT_ACTIVE;
    if (stalled) status = SLOT_STALL;
    if (begin && !stalled) {
        uint32_t base = 0;
        const bool complete = o.done && o.batch_active != 0;
        if (complete && queue != nullptr && o.b_nn > 0) {
            if (ol == 0) base = atomicAdd(queue_count, o.b_nn);
            base = oct_pick(base, 0);
            for (uint32_t j = ol; j < o.b_nn; j += 8) {
                LeafReq<NW> r;
                r.st = m.leaves()[j];
                r.slot = i;
                r.pad = 0;
                queue[base + j] = r;
            }
        }
        if (ol == 0) {
            S.hi = o.hi;
            S.node_count = o.node_count;
            S.new_nodes += o.d_new;
            S.nv_gather += o.d_visits;
            S.n_proc = o.n_proc;
            S.n_coll = o.n_coll;
            S.b_nn = o.b_nn;
            S.b_term = o.b_term;
            S.b_coll = o.b_coll;
            S.batch_active = o.batch_active;
            S.eval_base = base;
            S.rng = sh.rng;
            S.gather_pending = 0;
            S.g_rounds = o.rounds;
            if (o.error) S.error = o.error;
        }
    }
    if (ol == 0) {
        if (stalled) S.need_nodes = S.hi + cfg.n_sims + 2 * cfg.batch_size;
        S.status = tag_status(status, phase);
    }
}


// The gather as a work queue over tree levels (dev_gatherw.h): a wavefront serves G game contexts at once, every node
// a pick reaches is an item in the wavefront's LDS ring, and each pass the 64 lanes take the next 64 items -- of
// whichever games they are. The grid is persistent: context c of wavefront b walks game c of the sets (of G consecutive
// slots) j * gridDim.x + b, j = 0, 1, ... one after the other, so the lanes stay busy until the launch runs out of games.
// With a pass limit the sets of turn j >= 1 only get the passes their wavefront's first set leaves over, so the numbering of
// the sets is rotated from launch to launch (`rot`: set v of this launch is set (v + rot) mod n_sets; the host advances rot
// by n_sets - gridDim.x per launch, the width of the second turn): every game waits its share of the launches instead of
// the same eighth of the games waiting in all of them. Which wavefront walks a game never changes what its walk does.
// Leaves are left in the games' scratch (k_pack_leaves appends them to the evaluator queue).
// Ring item: context (bits 0..6), BEGIN flag (bit 7: the context wants a game), visit slot, siblings behind it.
// At most 168 VGPRs (the lane state takes 160-166, no scratch; the attribute is a guard): three wavefronts per SIMD. With
// G = 32 and two records per game the LDS (12 952 B + the maze stage) holds twelve per CU (profiles/r04_resource_usage.txt).
enum { GW_RECS = 2 };           // position records per game in LDS (R); a parent that finds them taken uses its game's scratch
enum { GW_WAVES_PER_CU = 11 };  // default persistent grid (AR_GW_WAVES overrides it)
template <int NW, int G, int R>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3)))
k_gatherw(Slot<NW>* slots, uint32_t n_slots, SearchCfg cfg, Bases B, uint32_t first, uint32_t phase, uint32_t accept_ready,
          uint32_t pass_limit, uint32_t rot) {
    static_assert((G & (G - 1)) == 0 && G <= 64, "the ring is a power of two; a context number fits a ring item");
    static_assert(sizeof(GwRec<NW>) == (sizeof(State<NW>) + 16 + 7) / 8 * 8, "slot_layout.h sizes the spill area");
    typedef GwShared<NW, G, R> Sh;
    __shared__ Sh sh;
    const uint32_t ring_mask = Sh::RING - 1;
    __shared__ OutcomeTable otab;
    extern __shared__ uint32_t lds_maze[];  // the shared maze (B.maze_stage bytes), if the run has one
    const uint32_t L = threadIdx.x;
    GwMem<NW> m;
    m.arena = B.arena;
    m.scratch = B.scratch;
    m.maze = B.maze;
    if (B.maze_stage) {
        for (uint32_t w = L; w < B.maze_stage / 4; w += 64) lds_maze[w] = ((const uint32_t*)B.maze)[w];
        m.maze = (const uint8_t*)lds_maze;
    }
    m.slot_bytes = B.L.total;
    m.proc_off = (uint32_t)B.L.proc_off;
    m.coll_off = (uint32_t)B.L.coll_off;
    m.leaf_off = (uint32_t)B.L.leaf_off;
    m.spill_off = (uint32_t)B.L.levels_off;
    m.coll_cap = B.L.coll_cap;
    if (L < 17) outcome_entry(L, otab.omap[L], otab.n[L]);
    if (L == 0) sh.tail = G;
    for (uint32_t c = L; c < (uint32_t)G; c += 64) {
        sh.game[c].slot = NIL;
        sh.game[c].running = 0;
        sh.game[c].next_game = 0;
        for (int j = 0; j < R; ++j) sh.rec_owner[c][j] = 0;
        sh.ring[c] = (uint16_t)(c | 0x80u);  // every context starts by asking for a game
    }
    uint32_t head = 0;
#if defined(AR_STATS)
    // per-wavefront counters (lane 0): passes, items, begins, pick ends, waits, interior, final, entries whose record came
    // from the game's scratch (no free record in LDS), passes with such an entry; 100 MHz clocks of the four phases
    unsigned long long gs_cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, gs_clk[5] = {0, 0, 0, 0, 0}, gs_hist[17] = {0}, gs_x[6] = {0, 0, 0, 0, 0, 0};
    const unsigned long long gs_t0 = wall_clock64();
#define GW_STAT(...) __VA_ARGS__
#else
#define GW_STAT(...)
#endif
    for (uint32_t guard = 0; guard < (1u << 24); ++guard) {  // (the queue drains; the bound is a fuse)
        __syncthreads();
        const uint32_t n = *(volatile uint32_t*)&sh.tail - head;
        if (n == 0) break;
        GW_STAT(const unsigned long long gs_a = wall_clock64();)
        uint32_t take = n < 64u ? n : 64u;
        const uint32_t item = L < take ? (uint32_t)sh.ring[(head + L) & ring_mask] : 0u;
        {
            // the children of one parent are taken in the same pass (they all read the parent's position first)
            const unsigned long long split = __ballot(L < take && L + ((item >> 12) & 15u) >= 64u);
            if (split) take = (uint32_t)__ffsll((long long)split) - 1u;
        }
        head += take;
        const bool mine = L < take;
        const bool begin = mine && (item & 0x80u);
        GW_STAT(gs_cnt[0] += 1; gs_cnt[1] += take; gs_cnt[2] += (unsigned long long)__popcll(__ballot(begin)); gs_hist[take / 4] += 1;)
        const uint32_t g = item & 0x7fu;
        GwLane<NW> ln;
        ln.active = mine && !begin;
        ln.g = g;
        // ---- phase 1
        uint32_t slot_i = NIL;
        bool skip = false;  // a context beyond the end of a ragged last set: nothing to walk this turn, but the next may have
        if (begin && guard < pass_limit) {  // (past the limit no game is begun: its turn comes with the next launch)
            const uint32_t turn = sh.game[g].next_game;
            sh.game[g].next_game = turn + 1u;
            const uint32_t n_sets = (n_slots - first + (uint32_t)G - 1u) / (uint32_t)G;
            const uint32_t v = turn * gridDim.x + blockIdx.x;
            if (v < n_sets) {
                uint32_t set = v + rot;
                if (set >= n_sets) set -= n_sets;
                slot_i = first + set * (uint32_t)G + g;
                skip = slot_i >= n_slots;
            }
        }
        if (ln.active) gw_fetch<NW, R>(ln, item, sh.game, &sh.rec[0][0], &sh.stub[0][0], &sh.stub_node[0][0], m);
        GW_STAT({
            const bool sp = ln.active && !ln.from_pick && ((sh.stub[g][(item >> 8) & 0xfu] >> 12) & 7u) == GW_SPILL;
            const unsigned long long b = __ballot(sp);
            gs_cnt[7] += (unsigned long long)__popcll(b);
            gs_cnt[8] += b ? 1ULL : 0ULL;
        })
        // ---- phase 2
        GW_STAT(const unsigned long long gs_b = wall_clock64();)
        bool started = false, retire = false;
        if (begin) {
            if (slot_i >= n_slots) {
                retire = !skip;
            } else {
                Slot<NW>& S = slots[slot_i];
                const uint32_t st = S.status;
                const bool run = st == SLOT_ACTIVE || st == accept_ready;
                if (run) {
                    uint32_t status = SLOT_ACTIVE;
                    if (S.batch_active == 0) {  // (a batch that still waits for its backup is left alone)
                        GwGame<NW>& Gm = sh.game[g];
                        gw_begin(Gm, S, slot_i, cfg);
                        started = Gm.began != 0;
                        GW_STAT(Gm.dbg_start = guard;)
                        if (Gm.stalled) {
                            gw_end(Gm, S, cfg);
                            status = SLOT_STALL;
                        }
                    }
                    if (!started) S.status = tag_status(status, phase);
                }
            }
        }
        if (ln.active) gw_visit(ln, sh.game[g], sh.rec_owner[g], m, cfg, &otab);
        __syncthreads();
        GW_STAT(const unsigned long long gs_c = wall_clock64();
                gs_cnt[4] += (unsigned long long)__popcll(__ballot(ln.active && ln.wait));
                gs_cnt[5] += (unsigned long long)__popcll(__ballot(ln.active && ln.interior));
                gs_cnt[6] += (unsigned long long)__popcll(__ballot(ln.active && ln.is_final));
                {
                    // the slowest lane of the pass: allocation steps; clocks from the start of the phase to record arrival /
                    // set-up / end of allocation (interior entries only)
                    const bool in = ln.active && ln.interior;
                    uint32_t st = in ? ln.dbg_steps : 0u, t0 = in ? (uint32_t)(ln.dbg_t[0] - gs_b) : 0u,
                             t1 = in ? (uint32_t)(ln.dbg_t[1] - gs_b) : 0u, t2 = in ? (uint32_t)(ln.dbg_t[2] - gs_b) : 0u;
                    uint32_t ssum = st;
                    for (int off = 32; off > 0; off >>= 1) {
                        st = max(st, (uint32_t)__shfl_xor((int)st, off, 64));
                        ssum += (uint32_t)__shfl_xor((int)ssum, off, 64);
                        t0 = max(t0, (uint32_t)__shfl_xor((int)t0, off, 64));
                        t1 = max(t1, (uint32_t)__shfl_xor((int)t1, off, 64));
                        t2 = max(t2, (uint32_t)__shfl_xor((int)t2, off, 64));
                    }
                    gs_x[0] += st; gs_x[1] += ssum; gs_x[2] += t0; gs_x[3] += t1; gs_x[4] += t2;
                    gs_x[5] += (unsigned long long)__popcll(__ballot(ln.active && ln.from_pick));
                })
        // ---- phase 3
        bool finisher = false;
        if (ln.active)
            finisher = gw_publish<NW, R>(ln, sh.game[g], sh.rec[g], sh.rec_owner[g], m.spill(sh.game[g]), sh.stub[g], sh.stub_node[g],
                                         sh.ring, ring_mask, &sh.tail);
        __syncthreads();
        GW_STAT(const unsigned long long gs_d = wall_clock64(); gs_cnt[3] += (unsigned long long)__popcll(__ballot(finisher));)
        // ---- phase 4: the end of a pick / the first pick of a new game / the next game for a context
        if (finisher) gw_finish_pick(sh.game[g], sh.stub[g], sh.ring, ring_mask, &sh.tail, g, guard + 1u < pass_limit);
        if (started) gw_next_pick(sh.game[g], sh.stub[g], sh.ring, ring_mask, &sh.tail, g);
        if (finisher || started) {
            GwGame<NW>& Gm = sh.game[g];
            if (!Gm.running) {  // the game's gather is complete (or parked): hand the slot back, ask for another game
                GW_STAT(atomicAdd(&g_gather_clk[64 + min((guard - Gm.dbg_start) / 8u, 47u)], 1ULL);)
                Slot<NW>& S = slots[Gm.slot];
                gw_end(Gm, S, cfg);
                S.status = tag_status(SLOT_ACTIVE, phase);
                Gm.slot = NIL;
                sh.ring[atomicAdd(&sh.tail, 1u) & ring_mask] = (uint16_t)(g | 0x80u);
            }
        } else if (begin && !retire) {
            sh.ring[atomicAdd(&sh.tail, 1u) & ring_mask] = (uint16_t)(g | 0x80u);  // not a game to walk: try the next one
        }
        GW_STAT(const unsigned long long gs_e = wall_clock64(); gs_clk[0] += gs_b - gs_a; gs_clk[1] += gs_c - gs_b;
                gs_clk[2] += gs_d - gs_c; gs_clk[3] += gs_e - gs_d;)
    }
#if defined(AR_STATS)
    if (L == 0) {
        gs_clk[4] = wall_clock64() - gs_t0;
        atomicAdd(&g_gather_clk[0], 1ULL);
        for (int k = 0; k < 7; ++k) atomicAdd(&g_gather_clk[1 + k], gs_cnt[k]);
        for (int k = 0; k < 5; ++k) atomicAdd(&g_gather_clk[8 + k], gs_clk[k]);
        atomicAdd(&g_gather_clk[13], gs_cnt[7]);
        atomicAdd(&g_gather_clk[14], gs_cnt[8]);
        for (int k = 0; k < 17; ++k) atomicAdd(&g_gather_clk[16 + k], gs_hist[k]);
        for (int k = 0; k < 6; ++k) atomicAdd(&g_gather_clk[40 + k], gs_x[k]);
    }
#endif
}

// The evaluation requests of the games that have just gathered a batch, appended to the device-wide leaf queue
// (replaces MuxBackend's request queue, mux.rs:170-289): one atomic per wavefront reserves the run, every lane copies its
// game's leaves. Only the order of games in the queue depends on the scheduling.
template <int NW>
__global__ void __launch_bounds__(64) k_pack_leaves(Slot<NW>* slots, uint32_t n_slots, Bases B, uint32_t first, LeafReq<NW>* queue,
                                                    uint32_t* queue_count) {
    const uint32_t i = first + blockIdx.x * 64u + threadIdx.x;
    uint32_t nn = 0;
    if (i < n_slots && slots[i].status == SLOT_ACTIVE && slots[i].batch_active != 0) nn = slots[i].b_nn;
    uint32_t incl = nn;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
        if ((threadIdx.x & 63u) >= (uint32_t)off) incl += up;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    uint32_t base = 0;
    if (threadIdx.x == 0 && total) base = atomicAdd(queue_count, total);
    base = (uint32_t)__shfl((int)base, 0, 64) + incl - nn;
    if (nn == 0) return;
    slots[i].eval_base = base;
    const State<NW>* leaves = (const State<NW>*)(B.scratch + (size_t)i * B.L.total + B.L.leaf_off);
    for (uint32_t j = 0; j < nn; ++j) {
        LeafReq<NW> r;
        r.st = leaves[j];
        r.slot = i;
        r.pad = 0;
        queue[base + j] = r;
    }
}

template <int NW>
__global__ void __launch_bounds__(64) k_backup(Slot<NW>* slots, uint32_t n_slots, SearchCfg cfg, Bases B,
                                               const ZigTables* zt, const EvalOut* ev_queue, uint32_t first,
                                               uint32_t phase) {
    const uint32_t i = first + blockIdx.x * 64u + threadIdx.x;
    if (i >= n_slots) return;
    if (slots[i].status != SLOT_ACTIVE || !slots[i].batch_active) return;
    Slot<NW> s = slots[i];
    const Mem<NW> m = resolve_mem<NW>(s, B.arena, B.scratch, i, B.L, B.maze);
    const EvalOut* ev = ev_queue ? ev_queue + s.eval_base : m.ev_local;
    if (backup_machine(s, m, cfg, ev, zt)) finish_move(s, m, cfg);
    s.status = tag_status(s.status, phase);
    slots[i] = s;
}

// The backup with sixteen lanes per game (dev_backup16.h): ceil(n / 4) blocks of 64 threads, dynamic LDS = the notes of
// 64 paths (BACKUP16_LDS_BYTES; `path_cap` = levels a path may have); four wavefronts per SIMD (128 registers) match the
// sixteen blocks a CU's LDS takes. Ends with batch_end; a search that is complete is left in the state (ACTIVE, no batch,
// remaining == 0) for k_finish.
template <int NW>
__global__ void __launch_bounds__(64, 4) k_backup16(Slot<NW>* slots, uint32_t n_slots, SearchCfg cfg, Bases B,
                                                 const ZigTables* zt, const EvalOut* ev_queue, uint32_t first,
                                                 uint32_t path_cap) {
    extern __shared__ uint32_t lds_path[];
    const uint32_t w = threadIdx.x & 15u;
    const uint32_t i = first + blockIdx.x * 4u + (threadIdx.x >> 4);
    bool active = i < n_slots && slots[i].status == SLOT_ACTIVE && slots[i].batch_active != 0;
    const uint32_t ii = i < n_slots ? i : first;
    Slot<NW>& S = slots[ii];
    const Mem<NW> m = resolve_mem<NW>(S, B.arena, B.scratch, ii, B.L, B.maze);
    active = active && backup16_wants(S, m, cfg);
    const EvalOut* ev = ev_queue ? ev_queue + S.eval_base : m.ev_local;
    (void)zt;
    backup16<NW>(active, S, m, cfg, ev, lds_path, path_cap, w);
    if (active && w == 0) batch_end(S);
}
// the end of a move (selfplay.rs:538-565 up to the tree reuse) for the games whose search k_backup16 completed
template <int NW>
__global__ void __launch_bounds__(64) k_finish(Slot<NW>* slots, uint32_t n_slots, SearchCfg cfg, Bases B, uint32_t first,
                                               uint32_t phase) {
    const uint32_t i = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    if (slots[i].status != SLOT_ACTIVE || slots[i].batch_active != 0 || slots[i].remaining != 0) return;
    Slot<NW> s = slots[i];
    const Mem<NW> m = resolve_mem<NW>(s, B.arena, B.scratch, i, B.L, B.maze);
    finish_move(s, m, cfg);
    s.status = tag_status(s.status, phase);
    slots[i] = s;
}

// Tree reuse (tree.rs:283-302): a workgroup per game that has to move re-roots the tree by the sliding compaction of
// dev_advance.h (advance_tree_scalar in dev_search.h is the one-lane statement of the same passes).
// The compaction is also where a game changes arena: once the kept tree is counted, the slot picks the run of pages
// that holds the kept tree plus one full search, and the move writes there. So a tree never runs out of room in the
// middle of a search, and a tree that shrank gives pages back. A slot that stalled anyway (pool empty at the time)
// is retried here on every launch: its nodes are copied unchanged into a bigger run.
// The slot header stays in memory: the block reads the few words it needs and its first thread writes the few that change.
template <int NW>
__device__ inline void adv_arena_fields(const Slot<NW>& from, Slot<NW>& to) {
    to.stats_off = from.stats_off;
    to.fwd_off = from.fwd_off;
    to.cap = from.cap;
    to.pool_blk = from.pool_blk;
    to.release_grown = from.release_grown;
    to.error = from.error;
}
// the block reads the same words in every lane: in scalar registers they cost the move none of its vector registers
__device__ inline uint32_t adv_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ inline long long adv_uniform(long long x) {
    return (long long)(((unsigned long long)adv_uniform((uint32_t)((unsigned long long)x >> 32)) << 32) | adv_uniform((uint32_t)x));
}
template <int NW>
__device__ inline void advance_slot(Slot<NW>* slots, uint32_t slot, const Bases& B, const SearchCfg& cfg, uint32_t phase,
                                    uint32_t ready_status, uint32_t fast_nodes, AdvLds& L) {
    const uint32_t tid = threadIdx.x;
    Slot<NW>& G = slots[slot];
    Slot<NW> s;  // the arena the slot has now (only the fields the arena helpers read and write)
    adv_arena_fields(G, s);
    s.stats_off = adv_uniform(s.stats_off);
    s.fwd_off = adv_uniform(s.fwd_off);
    s.cap = adv_uniform(s.cap);
    s.pool_blk = adv_uniform(s.pool_blk);
    s.release_grown = adv_uniform(s.release_grown);
    s.error = adv_uniform(s.error);
    const uint32_t status = adv_uniform(G.status), hi = adv_uniform(G.hi), keep_root = adv_uniform(G.pending_root),
                   need = adv_uniform(G.need_nodes);
    __syncthreads();  // (the first thread rewrites these words at the end: every thread has read them)
    NodeStats* stats = (NodeStats*)(B.arena + s.stats_off);
    uint32_t* fwd = (uint32_t*)(B.arena + s.fwd_off);

    if (status == tag_status(SLOT_STALL, phase)) {
        const uint32_t want = pool_pages_for(B.pool, need > s.cap + 1 ? need : s.cap + 1);
        if (tid == 0) L.pick = want ? pool_claim(B.pool, slot, want) : NIL;
        __syncthreads();
        const uint32_t idx = adv_uniform(L.pick);
        if (idx == NIL) return;  // nothing free: the host sees the stall and decides
        Slot<NW> d;
        adv_arena_fields(s, d);
        slot_at_pages(d, B, slot, idx, want);
        const uint4* ss = (const uint4*)stats;
        uint4* ds = (uint4*)(B.arena + d.stats_off);
        for (uint32_t w = tid; w < hi * (uint32_t)NODE_GROUPS; w += ADV_THREADS) ds[w] = ss[w];
        if (tid == 0) {
            leave_arena(s, d, B);
            adv_arena_fields(d, G);
            G.status = ready_status;
        }
        return;
    }

    if (keep_root == NIL) {  // fresh root: the pages a fresh tree wants (the run it is in, if that is as many)
        if (tid == 0) {
            Slot<NW> d;
            adv_arena_fields(s, d);
            const uint32_t want = B.pool.fresh_pages;
            bool ok = s.cap != 0;
            if (s.pool_blk != want) {  // (a bigger run, none, or an arena from the host)
                const uint32_t off = pool_claim(B.pool, slot, want);
                if (off != NIL) {
                    slot_at_pages(d, B, slot, off, want);
                    leave_arena(s, d, B);
                    ok = true;
                }
            }
            if (ok) {  // (an arena too small for a whole search stalls at its first gather and grows, like any other)
                adv_arena_fields(d, G);
                make_root(G, resolve_mem<NW>(G, B.arena, B.scratch, slot, B.L, B.maze));
                G.status = ready_status;
            }  // else: no arena yet; the slot stays as it is and the next launch of this parity tries again
        }
        return;
    }

    Slot<NW> d;
    adv_arena_fields(s, d);
    bool moved = false;
    const uint32_t cnt = advance_compact(stats, fwd, hi, keep_root, fast_nodes, L, [&](uint32_t kept) -> NodeStats* {
        // destination: the run that holds the kept tree plus one search (0 pages: beyond a run; the tree stays)
        const uint32_t want = pool_pages_for(B.pool, arena_need(kept, cfg));
        if (want != 0 && want != s.pool_blk) {  // (pool_blk 0: an arena from the host)
            if (tid == 0) L.pick = pool_claim(B.pool, slot, want);
            __syncthreads();
            const uint32_t idx = adv_uniform(L.pick);
            if (idx != NIL) {
                slot_at_pages(d, B, slot, idx, want);
                moved = true;
            }
        }
        return (NodeStats*)(B.arena + d.stats_off);
    });
    if (tid == 0) {
        if (moved) leave_arena(s, d, B);
        adv_arena_fields(d, G);
        G.root = 0;
        G.hi = cnt;
        G.node_count = cnt;
        G.status = ready_status;
    }
}

// Which slots: k_advance_scan lists the slots of [first_slot, n_slots) that wait for this phase's tree reuse, by the size
// of the job (a launch lasts as long as its largest trees, so those start first), and k_advance's blocks take the entries
// through a ticket, largest class first: a block's first ticket is its number, every later one comes from the counter.
// Games move in bursts (a session's games start in step, and so do the games that refill the slots of one host visit),
// in neighbouring slots: a block per range of slots serialises a burst (measured: as slow as one wavefront per game), a
// block per slot is 131072 blocks of eight wavefronts. `count` holds this launch's ADV_COUNTERS words (entries per
// class, then the ticket) and `count_next` the next launch's, which are cleared here: the launches of one stream
// alternate between two sets, so no launch needs a memset of its own. Class c's list is list + c * list_stride.
// ADV_BLOCKS: the grid. 256 (a block per CU, a tree at a time beside the CU's evaluator workgroups) gave the shortest batch
// step on the bench workload, ahead of 512 and 2048 (profiles/r08_advance_ab.txt).
enum { ADV_BLOCKS = 256, ADV_CLASSES = 4, ADV_TICKET = ADV_CLASSES, ADV_COUNTERS = 8 };
// nodes to look at: hi - pending_root of a re-root, hi of a stalled slot's copy, 0 for a fresh root. The bounds are an
// inference, not a histogram by nodes: tools/advance_stats.py sorts trees by time, and its two means (3175 nodes in 173 us
// for all trees, 7819 nodes in 550 us for those above 300 us, profiles/r08_advance_premise.txt) put about 15 nodes in a
// microsecond, so 8192 / 4096 / 1024 nodes stand for about 550 / 300 / 70 us of the parent's kernel. The order of the
// classes is what matters, not where exactly they part.
__device__ inline uint32_t adv_size_class(uint32_t nodes) { return nodes >= 8192u ? 0u : nodes >= 4096u ? 1u : nodes >= 1024u ? 2u : 3u; }
template <int NW>
__global__ void __launch_bounds__(256) k_advance_scan(const Slot<NW>* slots, uint32_t n_slots, uint32_t first_slot, uint32_t phase,
                                                      uint32_t* list, uint32_t list_stride, uint32_t* count, uint32_t* count_next) {
    const uint32_t slot = first_slot + blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t cls = ADV_CLASSES;  // (no work)
    if (slot < n_slots) {
        const Slot<NW>& G = slots[slot];
        const uint32_t status = G.status;
        if (status == tag_status(SLOT_ADVANCE, phase)) cls = adv_size_class(G.pending_root == NIL ? 0u : G.hi - G.pending_root);
        else if (status == tag_status(SLOT_STALL, phase)) cls = adv_size_class(G.hi);
    }
    if (__ballot(cls != (uint32_t)ADV_CLASSES) != 0ULL) {
        for (uint32_t c = 0; c < (uint32_t)ADV_CLASSES; ++c) {
            const unsigned long long bal = __ballot(cls == c);
            if (bal == 0ULL) continue;
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(count + c, (uint32_t)__popcll(bal));
            base = (uint32_t)__shfl((int)base, 0, 64);
            // (at most one entry per slot of the range, so a class's list never holds more than list_stride)
            if (cls == c) list[(size_t)c * list_stride + base + (uint32_t)__popcll(bal & ((1ULL << lane) - 1ULL))] = slot;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (uint32_t)ADV_COUNTERS) count_next[threadIdx.x] = 0;
}
template <int NW>
__global__ void __launch_bounds__(ADV_THREADS) k_advance(Slot<NW>* slots, Bases B, SearchCfg cfg, uint32_t phase, uint32_t ready_status,
                                                         const uint32_t* list, uint32_t list_stride, uint32_t* count, uint32_t fast_nodes) {
    __shared__ AdvLds L;
    for (uint32_t t = blockIdx.x;;) {
        uint32_t c = 0, at = t;  // entry `at` of class c: the classes one after the other (the counts are read again per
        for (; c < (uint32_t)ADV_CLASSES; ++c) {  // ticket: a few scalar loads, and no registers held across a tree)
            const uint32_t n = count[c];
            if (at < n) break;
            at -= n;
        }
        if (c == (uint32_t)ADV_CLASSES) break;
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[(size_t)c * list_stride + at]);
        __syncthreads();  // (the tables of the tree before are free, and every thread has read its ticket)
        advance_slot(slots, slot, B, cfg, phase, ready_status, fast_nodes, L);
        if (threadIdx.x == 0) L.ticket = gridDim.x + atomicAdd(count + ADV_TICKET, 1u);
        __syncthreads();
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.ticket);
    }
}

// evaluator failure: revert the gathered batch (search.rs:919-955)
template <int NW>
__global__ void k_cancel(Slot<NW>* slots, uint32_t n_slots, Bases B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    Slot<NW> s = slots[i];
    const Mem<NW> m = resolve_mem<NW>(s, B.arena, B.scratch, i, B.L, B.maze);
    if (s.batch_active || s.gather_pending) cancel_batch(s, m);  // (a parked gather holds claims and virtual losses too)
    s.gather_pending = 0;
    if (s.status == SLOT_ACTIVE) s.status = SLOT_FAILED;
    slots[i] = s;
}

// counts[0] done, [1] stalled, [2] active (incl. waiting for k_advance), [3] errors; lists hold slot ids.
// live[0..9): sums over the games that sit in a slot right now (finished-but-not-drained ones included) of
// positions, simulations, nn evals, terminals, collisions, gather / backup node-visits, new nodes, and the
// number of such games -- the host adds them to the totals of the games already drained, so a session can
// report the work done inside a window of steps (per finished move) without waiting for games to end.
enum { LIVE_N = 9 };
template <int NW>
__global__ void k_scan(const Slot<NW>* slots, uint32_t n_slots, uint32_t* counts, uint32_t* done_list,
                       uint32_t* stall_list, uint32_t* release_list, ArenaPool P, unsigned long long* live) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n_slots;
    if (in && P.bits && i < P.zones * P.zone_words) {  // for the host's bookkeeping: free pages of the region
        const uint32_t free_pages = (uint32_t)__popcll(~P.bits[i]);
        if (free_pages) atomicAdd(&counts[5], free_pages);
    }
    unsigned long long v[LIVE_N];
    for (int k = 0; k < LIVE_N; ++k) v[k] = 0;
    if (in) {
        const Slot<NW>& s = slots[i];
        const uint32_t st = s.status;
        if (s.error) atomicAdd(&counts[3], 1u);
        if (s.release_grown) release_list[atomicAdd(&counts[4], 1u)] = i;
        if (st == SLOT_DONE) done_list[atomicAdd(&counts[0], 1u)] = i;
        else if (st == SLOT_STALL || st == SLOT_STALL_B) stall_list[atomicAdd(&counts[1], 1u)] = i;
        else if (st == SLOT_ACTIVE || st == SLOT_ADVANCE || st == SLOT_ADVANCE_B || st == SLOT_READY_A || st == SLOT_READY_B)
            atomicAdd(&counts[2], 1u);
        if (st != SLOT_EMPTY && live != nullptr) {
            v[0] = s.n_pos;
            v[1] = s.t_sims;
            v[2] = s.t_nn;
            v[3] = s.t_term;
            v[4] = s.t_coll;
            v[5] = s.nv_gather;
            v[6] = s.nv_backup;
            v[7] = s.new_nodes;
            v[8] = 1;
        }
        // what a game that has been running for a while holds in tree pages (the host sizes the resident set by it)
        if (live != nullptr && st != SLOT_EMPTY && st != SLOT_DONE && s.pool_blk != 0 && s.n_pos >= 4) {
            atomicAdd(&live[12], (unsigned long long)s.pool_blk);
            atomicAdd(&live[13], 1ULL);
        }
    }
    if (live == nullptr) return;
    for (int k = 0; k < LIVE_N; ++k) {  // one atomic per wavefront and counter
        unsigned long long x = v[k];
        for (int off = 32; off > 0; off >>= 1) x += (unsigned long long)__shfl_xor((long long)x, off, 64);
        if ((threadIdx.x & 63u) == 0 && x) atomicAdd(&live[k], x);
    }
}

// one block per finished game: header by thread 0, position records copied by the whole block
template <int NW>
__global__ void k_pack_done(Slot<NW>* slots, const uint32_t* done_list, uint32_t n_done, DoneInfo<NW>* info,
                            PosRec<NW>* staging, uint32_t max_turns, Bases B) {
    const uint32_t d = blockIdx.x;
    if (d >= n_done) return;
    const uint32_t slot = done_list[d];
    Slot<NW>& s = slots[slot];
    const Mem<NW> m = resolve_mem<NW>(s, B.arena, B.scratch, slot, B.L, B.maze);
    if (threadIdx.x == 0) {
        DoneInfo<NW>& o = info[d];
        o.slot = slot;
        o.game_index = s.game_index;
        o.n_pos = s.n_pos;
        o.error = s.error;
        o.final_st = s.st;
        o.t_sims = s.t_sims;
        o.t_nn = s.t_nn;
        o.t_term = s.t_term;
        o.t_coll = s.t_coll;
        o.nv_gather = s.nv_gather;
        o.nv_backup = s.nv_backup;
        o.new_nodes = s.new_nodes;
        o.last = s.last;
    }
    const uint32_t n = s.n_pos < max_turns ? s.n_pos : max_turns;
    const uint32_t words = n * (uint32_t)(sizeof(PosRec<NW>) / 4);
    const uint32_t* src = (const uint32_t*)m.pos;
    uint32_t* dst = (uint32_t*)(staging + (size_t)d * max_turns);
    for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) dst[w] = src[w];
    __syncthreads();
    if (threadIdx.x == 0) {
        // the finished game's tree pages go back now (the slot may stay empty for a while: the host admits new games by
        // what the zone has free); an arena from the host is flagged for release
        Slot<NW> unused = s;
        leave_arena(s, unused, B);
        if (unused.error) s.error = unused.error;
        if (unused.release_grown) s.release_grown = 1;
        s.cap = 0;
        s.pool_blk = 0;
        s.status = SLOT_EMPTY;
    }
}

// ---- training rows (dev_rows.h) ------------------------------------------------------------------------------------
// Where the host puts a drained game in a row set: game `d` of the drain becomes stored game `game`, its positions the
// rows first_row .. first_row + n_rows.
struct RowPlace {
    uint64_t first_row;
    uint32_t game, n_rows, d, pad;
};

// Behind k_pack_done, one block per drained game: its staged records, its maze and its header go into the row set, and its
// cheese outcomes are computed here (the records of an attached run never visit the host for this).
template <int NW>
__global__ void k_rows_append(const DoneInfo<NW>* info, const PosRec<NW>* staging, uint32_t max_turns, const Slot<NW>* slots,
                              const uint8_t* maze_pool, const RowPlace* place, uint32_t n_place, PosRec<NW>* recs,
                              uint32_t* pos_game, RowGame* games, uint8_t* mazes, uint8_t* outcomes) {
    if (blockIdx.x >= n_place) return;
    const RowPlace pl = place[blockIdx.x];
    const DoneInfo<NW>& di = info[pl.d];
    const Board b = slots[di.slot].board;
    const uint32_t hw = (uint32_t)b.width * b.height;
    const PosRec<NW>* src_recs = staging + (size_t)pl.d * max_turns;
    const uint32_t words = pl.n_rows * (uint32_t)(sizeof(PosRec<NW>) / 4);
    const uint32_t* src = (const uint32_t*)src_recs;
    uint32_t* dst = (uint32_t*)(recs + pl.first_row);
    for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) dst[w] = src[w];
    for (uint32_t i = threadIdx.x; i < pl.n_rows; i += blockDim.x) pos_game[pl.first_row + i] = pl.game;
    const uint32_t* cost = (const uint32_t*)(maze_pool + b.maze_off);
    uint32_t* maze_dst = (uint32_t*)(mazes + (size_t)pl.game * hw * 4u);
    for (uint32_t c = threadIdx.x; c < hw; c += blockDim.x) maze_dst[c] = cost[c];
    rows_game_outcomes<NW>(threadIdx.x, blockDim.x, src_recs, pl.n_rows, di.final_st, (int)hw, outcomes + (size_t)pl.game * hw);
    if (threadIdx.x == 0) {
        RowGame g;
        g.width = b.width;
        g.height = b.height;
        g.max_turns = b.max_turns;
        g.pad = 0;
        g.final1 = di.final_st.s1;
        g.final2 = di.final_st.s2;
        g.game_index = di.game_index;
        g.n_rows = pl.n_rows;
        g.first_row = pl.first_row;
        games[pl.game] = g;
    }
}

// Output row row0 + i from stored position rows[row0 + i]: the caller's order is the gather index, so a shuffled training set
// is written once. One wavefront per row, four rows per block; every output array is contiguous over rows and a wavefront
// writes consecutive elements of its row (dword stores for the floats, byte stores for the i8 arrays, whose row stride of hw
// bytes is no multiple of four in general). The kernel is bound by its stores (1.5 KB per 7x7 row); no LDS.
enum { ROWS_PER_BLOCK = 4, ROWS_PER_LAUNCH = 262144 };
template <int NW>
__global__ void __launch_bounds__(ROWS_PER_BLOCK * ROWS_LANES)
k_rows_build(const PosRec<NW>* recs, const uint32_t* pos_game, const RowGame* games, const uint8_t* mazes,
             const uint8_t* outcomes, const uint64_t* rows, uint64_t row0, uint32_t n, RowOut out) {
    const uint32_t i = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint64_t r = row0 + i;
    const uint64_t src = rows[r];
    const uint32_t gi = pos_game[src];
    const RowGame& g = games[gi];
    const size_t hw = (size_t)g.width * g.height;
    rows_build_row<NW>(threadIdx.x & 63u, recs[src], g, mazes + (size_t)gi * hw * 4u, outcomes + (size_t)gi * hw, out, r);
}

// Output row row0 + i of a batch from stored position order_rows[first + row0 + i], seen by P2 where order_swap[...] is set
// (dev_rows.h rows_build_row_as): an epoch's shuffle and its player-swap mask sit on the device as the set's order, and a
// batch is a window of it, written once into the caller's tensors. The shape of k_rows_build: one wavefront per row, four
// rows per block, global loads and stores only, no LDS. The wavefront's number in the block is made a scalar, so the row's
// index, its flag and its game are read once per wavefront and the flag selects without divergence.
template <int NW>
__global__ void __launch_bounds__(ROWS_PER_BLOCK * ROWS_LANES)
k_rows_batch(const PosRec<NW>* recs, const uint32_t* pos_game, const RowGame* games, const uint8_t* mazes,
             const uint8_t* outcomes, const uint64_t* order_rows, const uint8_t* order_swap, uint64_t first, uint64_t row0,
             uint32_t n, RowOut out) {
    const uint32_t i = blockIdx.x * ROWS_PER_BLOCK + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= n) return;
    const uint64_t r = row0 + i;
    const uint64_t src = order_rows[first + r];
    const bool swap = order_swap[first + r] != 0;
    const uint32_t gi = pos_game[src];
    const RowGame& g = games[gi];
    const size_t hw = (size_t)g.width * g.height;
    rows_build_row_as<NW>(threadIdx.x & 63u, recs[src], g, mazes + (size_t)gi * hw * 4u, outcomes + (size_t)gi * hw, out, r, swap);
}

// ---- validation over stored rows (dev_validate.h) ------------------------------------------------------------------
// Evaluator requests from stored records, one lane per row: the position of row rows[i], and the number of its stored game
// as the index of its Board (one Board per stored game, maze_off = game * hw * 4: the set's mazes are the maze pool).
enum { VAL_BLOCK = 256, VAL_WAVES = VAL_BLOCK / 64, VAL_N_TERMS = VAL_N_DOUBLE + VAL_N_COUNT };
template <int NW>
__global__ void __launch_bounds__(VAL_BLOCK)
k_val_requests(const PosRec<NW>* recs, const uint32_t* pos_game, const uint64_t* rows, uint32_t n, LeafReq<NW>* req) {
    const uint32_t i = blockIdx.x * VAL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t src = rows[i];
    LeafReq<NW> q;
    q.st = recs[src].st;
    q.slot = pos_game[src];
    q.pad = 0;
    req[i] = q;
}

// The terms of row i (val_row_terms) from its record, its game, the evaluator's ten logits and two values, summed over the
// block: in double over the wavefront with __shfl_down (a fixed tree), then over the block's wavefronts through LDS in
// wavefront order. One partial vector per block, written with plain stores: no atomics, so the same request gives the same
// bytes. A lane beyond n adds zeros and takes part in every shuffle.
template <int NW>
__global__ void __launch_bounds__(VAL_BLOCK)
k_val_terms(const PosRec<NW>* recs, const uint32_t* pos_game, const RowGame* games, const uint64_t* rows, uint32_t n,
            const float* logits, const EvalOut* ev, ValAcc* partial) {
    __shared__ double s_d[VAL_WAVES][VAL_N_DOUBLE];
    __shared__ uint32_t s_c[VAL_WAVES][VAL_N_COUNT];
    const uint32_t i = blockIdx.x * VAL_BLOCK + threadIdx.x;
    ValAcc acc;
#pragma unroll
    for (int j = 0; j < VAL_N_DOUBLE; ++j) acc.d[j] = 0.0;
#pragma unroll
    for (int j = 0; j < VAL_N_COUNT; ++j) acc.c[j] = 0;
    if (i < n) {
        const uint64_t src = rows[i];
        float l[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) l[k] = logits[(size_t)i * 10 + k];
        const EvalOut& o = ev[i];
        val_accumulate(acc, val_row_terms<NW>(recs[src], games[pos_game[src]], l, o.v1, o.v2));
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < VAL_N_DOUBLE; ++j) {
        double v = acc.d[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s_d[wave][j] = v;
    }
#pragma unroll
    for (int j = 0; j < VAL_N_COUNT; ++j) {
        uint32_t c = (uint32_t)acc.c[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_down((int)c, off, 64);
        if (lane == 0) s_c[wave][j] = c;
    }
    __syncthreads();
    if (threadIdx.x < VAL_N_DOUBLE) {
        double v = s_d[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < VAL_WAVES; ++w) v += s_d[w][threadIdx.x];
        partial[blockIdx.x].d[threadIdx.x] = v;
    } else if (threadIdx.x < VAL_N_TERMS) {
        const uint32_t j = threadIdx.x - VAL_N_DOUBLE;
        uint64_t c = 0;
#pragma unroll
        for (int w = 0; w < VAL_WAVES; ++w) c += s_c[w][j];
        partial[blockIdx.x].c[j] = c;
    }
}

// One block adds the partial vectors of a chunk to the running total, in index order: thread j owns term j.
__global__ void __launch_bounds__(64) k_val_sum(const ValAcc* partial, uint32_t n_partial, ValAcc* total) {
    const uint32_t j = threadIdx.x;
    if (j < VAL_N_DOUBLE) {
        double v = total->d[j];
        for (uint32_t b = 0; b < n_partial; ++b) v += partial[b].d[j];
        total->d[j] = v;
    } else if (j < VAL_N_TERMS) {
        uint64_t c = total->c[j - VAL_N_DOUBLE];
        for (uint32_t b = 0; b < n_partial; ++b) c += partial[b].c[j - VAL_N_DOUBLE];
        total->c[j - VAL_N_DOUBLE] = c;
    }
}

// The ownership terms of a chunk's rows (k_own_mfma) added to the running total by one block, without atomics. ce and
// cells: thread t sums a contiguous segment of the rows in row order, thread 0 adds the 256 segment sums in order. With
// `batch` > 0 the chunk (a multiple of `batch` rows, but for the request's last) is cut into consecutive batches: a thread
// sums one batch's rows in row order and forms B_b * (ce_b / cells_b), 0 for a batch without an active cell
// (losses/ownership.py:35-37); thread 0 adds the batches' terms in batch order.
struct OwnAcc {
    double ce, batch_weighted;
    uint64_t cells;
};
enum { OWN_SUM_BLOCK = 256 };
__global__ void __launch_bounds__(OWN_SUM_BLOCK)
k_own_sum(const double* row_ce, const uint32_t* row_cells, uint32_t n, uint32_t batch, OwnAcc* total) {
    __shared__ double s_ce[OWN_SUM_BLOCK];
    __shared__ uint64_t s_cells[OWN_SUM_BLOCK];
    const uint32_t t = threadIdx.x;
    {
        const uint64_t per = ((uint64_t)n + OWN_SUM_BLOCK - 1) / OWN_SUM_BLOCK;
        const uint64_t lo = t * per, hi = lo + per < (uint64_t)n ? lo + per : (uint64_t)n;
        double ce = 0.0;
        uint64_t cells = 0;
        for (uint64_t i = lo; i < hi; ++i) {
            ce += row_ce[i];
            cells += row_cells[i];
        }
        s_ce[t] = ce;
        s_cells[t] = cells;
    }
    __syncthreads();
    if (t == 0) {
        double ce = total->ce;
        uint64_t cells = total->cells;
        for (int j = 0; j < OWN_SUM_BLOCK; ++j) {
            ce += s_ce[j];
            cells += s_cells[j];
        }
        total->ce = ce;
        total->cells = cells;
    }
    if (batch == 0) return;
    const uint32_t n_batches = (uint32_t)(((uint64_t)n + batch - 1) / batch);
    for (uint32_t b0 = 0; b0 < n_batches; b0 += OWN_SUM_BLOCK) {
        __syncthreads();  // thread 0 is done with s_ce
        double term = 0.0;
        if (b0 + t < n_batches) {
            const uint64_t lo = (uint64_t)(b0 + t) * batch, hi = lo + batch < (uint64_t)n ? lo + batch : (uint64_t)n;
            double ce = 0.0;
            uint64_t cells = 0;
            for (uint64_t i = lo; i < hi; ++i) {
                ce += row_ce[i];
                cells += row_cells[i];
            }
            term = cells ? (double)(hi - lo) * (ce / (double)cells) : 0.0;
        }
        s_ce[t] = term;
        __syncthreads();
        if (t == 0) {
            double v = total->batch_weighted;
            for (uint32_t j = 0; j < OWN_SUM_BLOCK && b0 + j < n_batches; ++j) v += s_ce[j];
            total->batch_weighted = v;
        }
    }
}

// arena growth: what a stalled slot reports, and its new home once the host has copied the nodes
struct StallInfo {
    uint32_t slot, cap, hi, need;
    long long stats_off;
};
struct GrowReq {
    uint32_t slot, cap;
    long long stats_off, fwd_off;
};
template <int NW>
__global__ void k_read_stall(const Slot<NW>* slots, const uint32_t* stall_list, uint32_t n, StallInfo* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Slot<NW>& s = slots[stall_list[i]];
    StallInfo o;
    o.slot = stall_list[i];
    o.cap = s.cap;
    o.hi = s.hi;
    o.need = s.need_nodes;
    o.stats_off = s.stats_off;
    out[i] = o;
}
template <int NW>
__global__ void k_clear_release(Slot<NW>* slots, const uint32_t* list, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) slots[list[i]].release_grown = 0;
}
template <int NW>
__global__ void k_apply_grow(Slot<NW>* slots, const GrowReq* req, uint32_t n, Bases B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Slot<NW>& s = slots[req[i].slot];
    if (s.pool_blk) {
        Slot<NW> unused = s;
        leave_arena(s, unused, B);
        if (unused.error) s.error = unused.error;
    }
    s.pool_blk = 0;
    s.cap = req[i].cap;
    s.stats_off = req[i].stats_off;
    s.fwd_off = req[i].fwd_off;
    s.status = SLOT_ACTIVE;
}

// ------------------------------------------------------------------------------------------------
// NN-evaluation cache (cached_backend.rs:70-130, nn_cache.rs): positions that were evaluated before
// skip the network. The reference keeps one FIFO table per worker thread keyed by a 64-bit FNV-1a
// hash of everything the network sees; here one device-wide open-addressing table serves all games,
// indexed by the same kind of hash but matched on the full position, so a hit is exact. A hit returns
// bit for bit what the network kernel would compute again (it is deterministic per leaf), so game
// records do not depend on the cache, only the work does.
//   k_cache_probe: every queued leaf looks itself up (<= CACHE_PROBES slots from its home slot); hits
//     get their result at once, misses are compacted into a second queue for the network;
//   k_cache_fill:  results of the misses go to their place in the batch and into the table (first empty
//     slot of the probe window, else the home slot is overwritten). Writers claim a slot by CAS on its
//     tag; readers only run in k_cache_probe, i.e. after a kernel boundary, and never see a slot mid-write
//     (the cache forces one group of games: one probe / fill pair in flight at a time).
// The maze is part of the key like in the reference (walls and mud are hashed, cached_backend.rs:130-199):
// with one shared maze the key is its pool offset; with generated mazes (one pool entry per slot, rewritten
// for every new game) it is the game the position belongs to -- only that game has that maze.
enum { CACHE_PROBES = 8, CACHE_EMPTY = 0, CACHE_VALID = 1, CACHE_BUSY = 2 };
template <int NW>
struct alignas(16) CacheEntry {
    State<NW> st;
    uint32_t maze_off;
    uint32_t tag;
    uint32_t maze_game;  // 0: shared maze; game index + 1 with one maze per game
    EvalOut ev;
};
template <int NW>
__device__ inline uint64_t position_hash(const State<NW>& st, uint32_t maze_off, uint32_t maze_game) {  // FNV-1a, cached_backend.rs:135-199
    uint64_t h = 0xcbf29ce484222325ULL;
    auto mix = [&](uint64_t v) {
        h ^= v;
        h *= 0x100000001b3ULL;
    };
    mix(st.p1);
    mix(st.p2);
    mix(__float_as_uint(st.s1));
    mix(__float_as_uint(st.s2));
    mix(st.m1);
    mix(st.m2);
    mix(st.turn);
    mix(maze_off);
    mix(maze_game);
    for (int w = 0; w < NW; ++w) mix(st.cheese[w]);
    return h;
}
template <int NW>
__device__ inline bool same_position(const State<NW>& a, const State<NW>& b) {
    bool eq = a.p1 == b.p1 && a.p2 == b.p2 && a.m1 == b.m1 && a.m2 == b.m2 && a.turn == b.turn &&
              __float_as_uint(a.s1) == __float_as_uint(b.s1) && __float_as_uint(a.s2) == __float_as_uint(b.s2);
    for (int w = 0; w < NW; ++w) eq = eq && a.cheese[w] == b.cheese[w];
    return eq;
}
template <int NW>
__global__ void k_cache_probe(const LeafReq<NW>* queue, const uint32_t* n_ptr, const Slot<NW>* slots,
                              const CacheEntry<NW>* table, uint64_t mask, EvalOut* ev_out, LeafReq<NW>* miss_queue,
                              uint32_t* miss_map, uint32_t* miss_count, unsigned long long* counters,
                              uint32_t maze_per_game) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < *n_ptr;
    LeafReq<NW> r = queue[in ? i : 0];
    bool hit = false;
    if (in) {
        const uint32_t maze_off = slots[r.slot].board.maze_off;
        const uint32_t maze_game = maze_per_game ? slots[r.slot].game_index + 1u : 0u;
        const uint64_t h = position_hash(r.st, maze_off, maze_game);
        for (int p = 0; p < CACHE_PROBES && !hit; ++p) {
            const CacheEntry<NW>& e = table[(h + (uint64_t)p) & mask];
            if (e.tag == CACHE_EMPTY) break;
            if (e.tag == CACHE_VALID && e.maze_off == maze_off && e.maze_game == maze_game && same_position(e.st, r.st)) {
                ev_out[i] = e.ev;
                hit = true;
            }
        }
    }
    // one atomic per wavefront for the counters and for the misses' places in the second queue
    const unsigned long long hits = __ballot(in && hit), misses = __ballot(in && !hit);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == 0) {
        if (hits) atomicAdd(&counters[0], (unsigned long long)__popcll(hits));
        if (misses) {
            atomicAdd(&counters[1], (unsigned long long)__popcll(misses));
            base = atomicAdd(miss_count, (uint32_t)__popcll(misses));
        }
    }
    base = (uint32_t)__shfl((int)base, 0, 64);
    if (in && !hit) {
        const uint32_t j = base + (uint32_t)__popcll(misses & ((1ULL << lane) - 1ULL));
        miss_queue[j] = r;
        miss_map[j] = i;
    }
}
template <int NW>
__global__ void k_cache_fill(const LeafReq<NW>* miss_queue, const uint32_t* miss_map, const uint32_t* miss_count,
                             const EvalOut* ev_miss, const Slot<NW>* slots, CacheEntry<NW>* table, uint64_t mask,
                             EvalOut* ev_out, uint32_t maze_per_game) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= *miss_count) return;
    const LeafReq<NW> r = miss_queue[j];
    const EvalOut ev = ev_miss[j];
    ev_out[miss_map[j]] = ev;
    const uint32_t maze_off = slots[r.slot].board.maze_off;
    const uint32_t maze_game = maze_per_game ? slots[r.slot].game_index + 1u : 0u;
    const uint64_t h = position_hash(r.st, maze_off, maze_game);
    // first empty slot of the window; a position that is already there (or being written by a twin in
    // this batch) is left alone; a full window overwrites the home slot
    for (int p = 0; p <= CACHE_PROBES; ++p) {
        const bool evict = p == CACHE_PROBES;
        CacheEntry<NW>& e = table[(h + (uint64_t)(evict ? 0 : p)) & mask];
        const uint32_t tag = e.tag;
        if (!evict && tag == CACHE_VALID) {
            if (e.maze_off == maze_off && e.maze_game == maze_game && same_position(e.st, r.st)) return;
            continue;
        }
        if (!evict && tag == CACHE_BUSY) continue;
        if (atomicCAS(&e.tag, evict ? (uint32_t)CACHE_VALID : (uint32_t)CACHE_EMPTY, (uint32_t)CACHE_BUSY) !=
            (evict ? (uint32_t)CACHE_VALID : (uint32_t)CACHE_EMPTY)) {
            if (evict) return;
            continue;
        }
        e.st = r.st;
        e.maze_off = maze_off;
        e.maze_game = maze_game;
        e.ev = ev;
        __threadfence();
        atomicExch(&e.tag, (uint32_t)CACHE_VALID);
        return;
    }
}

// SmartUniformBackend (backend.rs:92-103) as an evaluator of the leaf queue: the split pipeline (k_gather8 -> this ->
// k_backup16) then serves uniform-prior runs too; the values are what the fused k_step_uniform computes inline
// (emit_proc, EVAL_UNIFORM).
template <int NW>
__global__ void k_uniform_eval(const LeafReq<NW>* queue, const uint32_t* n_ptr, const Slot<NW>* slots, const uint8_t* maze,
                               EvalOut* ev_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *n_ptr) return;
    const LeafReq<NW> r = queue[i];
    const uint8_t* cost = maze + slots[r.slot].board.maze_off;
    EvalOut o;
    uniform_prior(eff_actions(cost, r.st.p1, r.st.m1), o.p1);
    uniform_prior(eff_actions(cost, r.st.p2, r.st.m2), o.p2);
    o.v1 = 0.0f;
    o.v2 = 0.0f;
    ev_out[i] = o;
}

// host-callback evaluator support: leaves out, results in (single-slot searches)
template <int NW>
__global__ void k_export_leaves(const Slot<NW>* slots, uint32_t slot, Bases B, State<NW>* out, uint32_t* n_out) {
    const Slot<NW>& s = slots[slot];
    const Mem<NW> m = resolve_mem<NW>(s, B.arena, B.scratch, slot, B.L, B.maze);
    if (threadIdx.x == 0) *n_out = s.batch_active ? s.b_nn : 0;
    for (uint32_t j = threadIdx.x; j < s.b_nn; j += blockDim.x) out[j] = m.leaf_local[j];
}
template <int NW>
__global__ void k_import_evals(const Slot<NW>* slots, uint32_t slot, Bases B, const EvalOut* in, uint32_t n) {
    const Mem<NW> m = resolve_mem<NW>(slots[slot], B.arena, B.scratch, slot, B.L, B.maze);
    for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) m.ev_local[j] = in[j];
}

// ---- head-to-head matches (dev_match.h): one slot set per searching agent, slot k of either holds game k ----------
// Replaces the host loop of eval/game.py:47-87 around SearcherAgent.get_move (searcher_agent.py:40-56).
// All of these run while the engines' streams are at rest on the slots they touch (the host orders them with events):
// ownership passes at kernel boundaries only, as everywhere else. (The kernels of the move itself follow below, with
// the agents that do not search.)
// counts[0] finished games (their slots in done_list), [1] games being played, [2] games with the bug guard set
template <int NW>
__global__ void k_match_scan(const MatchGame<NW>* games, uint32_t n, uint32_t* counts, uint32_t* done_list) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t st = games[i].status;
    if (st == MATCH_FINISHED) done_list[atomicAdd(&counts[0], 1u)] = i;
    else if (st == MATCH_PLAYING) atomicAdd(&counts[1], 1u);
    if (st != MATCH_EMPTY && games[i].error) atomicAdd(&counts[2], 1u);
}
// one block per finished game: header and position records to the staging buffers, the game leaves the match buffer
template <int NW>
__global__ void k_match_pack(MatchGame<NW>* games, const uint32_t* done_list, uint32_t n_done, MatchGame<NW>* info,
                             const MatchPos<NW>* recs, MatchPos<NW>* staging, uint32_t max_turns) {
    const uint32_t d = blockIdx.x;
    if (d >= n_done) return;
    const uint32_t slot = done_list[d];
    const MatchGame<NW> g = games[slot];
    const uint32_t n = g.n_pos < max_turns ? g.n_pos : max_turns;
    const uint32_t words = n * (uint32_t)(sizeof(MatchPos<NW>) / 4);
    const uint32_t* src = (const uint32_t*)(recs + (size_t)slot * max_turns);
    uint32_t* dst = (uint32_t*)(staging + (size_t)d * max_turns);
    for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) dst[w] = src[w];
    if (threadIdx.x == 0) {
        info[d] = g;
        info[d].pad[0] = slot;
        games[slot].status = MATCH_EMPTY;
    }
}
// the slots of the finished games, one engine at a time: tree pages go back, the slot is free (as k_pack_done leaves it)
template <int NW>
__global__ void k_match_release(Slot<NW>* slots, const uint32_t* done_list, uint32_t n_done, Bases B) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_done) return;
    Slot<NW>& s = slots[done_list[d]];
    Slot<NW> unused = s;
    leave_arena(s, unused, B);
    if (unused.error) s.error = unused.error;
    if (unused.release_grown) s.release_grown = 1;
    s.cap = 0;
    s.pool_blk = 0;
    s.status = SLOT_EMPTY;
}


// ---- matches with agents that do not search (dev_agents.h) --------------------------------------------------------
// The match keeps the position, the random agents' streams and the greedy agents' moves of game k in aux[k], and the
// mazes in a pool of its own (an agent without an engine has none). `sa` / `sb` are null for an agent that does not search.
template <int NW>
struct MatchAuxInit {
    uint32_t slot, game_index, a_is_p1, pad;
    Board board;
    State<NW> st;
    uint64_t seed_a, seed_b;
};
// one block per new game: its maze goes to the slot's pool entry (maze_stride != 0), lane 0 writes the game's records
template <int NW>
__global__ void __launch_bounds__(64) k_match_init_agents(MatchGame<NW>* games, MatchAux<NW>* aux, Slot<NW>* sa, Slot<NW>* sb,
                                                          const MatchAuxInit<NW>* init, uint32_t n, const uint8_t* maze_stage,
                                                          uint8_t* maze, uint32_t maze_stride) {
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const MatchAuxInit<NW> mi = init[i];
    if (maze_stride) {
        const uint32_t* src = (const uint32_t*)(maze_stage + (size_t)i * maze_stride);
        uint32_t* dst = (uint32_t*)(maze + (size_t)mi.slot * maze_stride);
        for (uint32_t w = threadIdx.x; w < maze_stride / 4u; w += blockDim.x) dst[w] = src[w];
    }
    if (threadIdx.x != 0) return;
    MatchAux<NW> x;
    x.board = mi.board;
    x.st = mi.st;
    rng_seed(x.rng[0], mi.seed_a);
    rng_seed(x.rng[1], mi.seed_b);
    x.greedy_act[0] = x.greedy_act[1] = DIR_STAY;
    x.pad[0] = x.pad[1] = 0;
    aux[mi.slot] = x;
    MatchGame<NW> g;
    g.status = MATCH_PLAYING;
    g.game_index = mi.game_index;
    g.n_pos = 0;
    g.a_is_p1 = mi.a_is_p1;
    g.error = 0;
    g.pad[0] = g.pad[1] = g.pad[2] = 0;
    g.final_st = mi.st;
    if (st_over(mi.board, mi.st)) {  // while not game.is_over(): nothing to play
        g.status = MATCH_FINISHED;
        if (sa) sa[mi.slot].status = SLOT_DONE;
        if (sb) sb[mi.slot].status = SLOT_DONE;
    }
    games[mi.slot] = g;
}

__device__ inline uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}
// greedy_agent.py:34-84 for the player on `start`, by the whole wavefront (dev_agents.h: levels of increasing distance,
// pop order inside a level from the keys). At most `hw` levels: every level settles a cell. `bound_hit`: the loop ran out.
template <int NW>
__device__ uint32_t greedy_move_wave(GreedyShared& sh, const uint8_t* cost, const Board& board, const State<NW>& st,
                                     uint32_t start, bool& bound_hit) {
    const uint32_t lane = threadIdx.x, hw = (uint32_t)board.width * board.height;
    const int w = board.width, h = board.height;
    bound_hit = false;
    __syncthreads();  // (the block of a previous call is no longer read)
    greedy_load(sh, lane, cost, st, hw, start);
    __syncthreads();
    if (sh.cheese[start]) return DIR_STAY;
    uint32_t settled = 1;
    for (uint32_t round = 0; round < hw; ++round) {
        const uint32_t level = wave_min_u32(greedy_tent(sh, lane, hw, w, h));
        if (level == GREEDY_NONE) return DIR_STAY;  // the heap ran empty: no cheese can be reached
        greedy_key(sh, lane, level, hw, w, h);
        __syncthreads();
        uint32_t cheese;
        const uint32_t n = wave_sum_u32(greedy_rank(sh, lane, level, settled, hw, cheese));
        cheese = wave_min_u32(cheese);
        if (cheese != GREEDY_NO_CHEESE) return cheese & 0xffu;
        settled += n;
        __syncthreads();
    }
    bound_hit = true;
    return DIR_STAY;
}
// One wavefront per resident game: the moves of the greedy agents of every game that is ready to move, left in aux for
// k_match_move_agents behind it on the same stream.
template <int NW>
__global__ void __launch_bounds__(64) k_match_greedy(const Slot<NW>* sa, const Slot<NW>* sb, MatchGame<NW>* games,
                                                     MatchAux<NW>* aux, uint32_t n, const uint8_t* maze, uint32_t kind_a,
                                                     uint32_t kind_b) {
    __shared__ GreedyShared sh;
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    if (!match_ready_agents(games[i], sa ? sa + i : nullptr, sb ? sb + i : nullptr)) return;  // (uniform over the block)
    const Board board = aux[i].board;
    const State<NW> st = aux[i].st;
    if ((uint32_t)board.width * board.height > GREEDY_CELLS) return;
    const uint8_t* cost = maze + board.maze_off;
    const int side_a = games[i].a_is_p1 ? 0 : 1;
    for (int which = 0; which < 2; ++which) {
        if ((which == 0 ? kind_a : kind_b) != AGENT_GREEDY) continue;
        const int side = which == 0 ? side_a : 1 - side_a;
        bool bound_hit;
        const uint32_t mv = greedy_move_wave<NW>(sh, cost, board, st, side == 0 ? st.p1 : st.p2, bound_hit);
        if (threadIdx.x == 0) {
            aux[i].greedy_act[which] = mv;
            if (bound_hit) games[i].error = 8;
        }
    }
}
// One lane per game: the move of every game that is ready (dev_agents.h match_move_agents), as k_match_move
template <int NW>
__global__ void __launch_bounds__(64) k_match_move_agents(Slot<NW>* sa, Slot<NW>* sb, MatchGame<NW>* games, MatchAux<NW>* aux,
                                                          MatchPos<NW>* recs, uint32_t n, uint32_t max_turns,
                                                          const uint8_t* maze, AgentDesc da, AgentDesc db) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Slot<NW>* a = sa ? sa + i : nullptr;
    Slot<NW>* b = sb ? sb + i : nullptr;
    if (!match_ready_agents(games[i], a, b)) return;
    match_move_agents(games[i], aux[i], a, b, da, db, maze + aux[i].board.maze_off, recs + (size_t)i * max_turns,
                      tag_status(SLOT_ADVANCE, 0u));
}

// ------------------------------------------------------------------------------------------------
// host (game generation and the supply of a run's games: host_games.h)
// ------------------------------------------------------------------------------------------------
namespace {

// a new game's record for k_init_games; the caller sets rng_seed and single
template <int NW>
GameInit<NW> game_init(const HostGame& g, uint32_t slot, uint32_t index, uint32_t maze_off) {
    GameInit<NW> gi;
    memset(&gi, 0, sizeof gi);
    fill_state<NW>(g, gi.board, gi.st, maze_off);
    gi.game_index = index;
    gi.slot = slot;
    return gi;
}

SearchCfg to_cfg(const ArSearchConfig& c, uint32_t sims, uint32_t batch) {
    SearchCfg s;
    s.c_puct = c.c_puct;
    s.fpu_reduction = c.fpu_reduction;
    s.force_k = c.force_k;
    s.noise_epsilon = c.noise_epsilon;
    s.noise_concentration = c.noise_concentration;
    s.coll_min = c.collision_limit_min;
    s.coll_max = c.collision_limit_max;
    s.coll_start = c.collision_scaling_start;
    s.coll_end = c.collision_scaling_end;
    s.coll_power = c.collision_scaling_power;
    s.n_sims = sims;
    s.batch_size = batch;
    s.alloc_per_round = 1;  // measured best on the bench workload; results do not depend on it
    if (const char* e = getenv("AR_ALLOC_PER_ROUND"))
        if (atoi(e) >= 1) s.alloc_per_round = (uint32_t)atoi(e);
    return s;
}

// The most node counts a budget table holds (16 MiB of device memory): check_cfg refuses wider scaling ranges when the
// power is not 1.
enum { COLL_TABLE_MAX = 1 << 22 };

int check_cfg(const SearchCfg& c) {
    if (c.n_sims == 0) return fail(AR_E_INVALID, "simulations must be > 0");
    static_assert(MAX_BATCH_SIZE == 4096, "the message below states the limit");
    if (c.batch_size == 0 || c.batch_size > MAX_BATCH_SIZE) return fail(AR_E_INVALID, "batch_size must be in 1..4096");
    if (c.coll_max > 65536) return fail(AR_E_INVALID, "collision_limit_max must be <= 65536");
    if (c.coll_min > c.coll_max) return fail(AR_E_INVALID, "collision_limit_min must be <= collision_limit_max");
    static_assert(COLL_TABLE_MAX == 4194304, "the message below states the limit");
    if (coll_table_size(c) >= (uint32_t)COLL_TABLE_MAX)
        return fail(AR_E_INVALID, "collision_scaling_power != 1 needs collision_scaling_end - collision_scaling_start <= 4194304");
    if (c.noise_epsilon > 0.0f && !(c.noise_concentration / 5.0f > 1.0f))
        return fail(AR_E_INVALID, "noise_concentration must exceed 5 (Gamma shape >= 1 path only)");
    return AR_OK;
}

// ------------------------------------------------------------------------------------------------
// host: the engine -- device-resident slots and the step loop
// ------------------------------------------------------------------------------------------------
// A game's positions and moves as the columns of its record (self-play and match records share them)
struct PosColumns {
    std::vector<uint8_t> p1_pos, p2_pos, p1_mud, p2_mud, cheese_mask, a1, a2;
    std::vector<float> p1_score, p2_score;
    std::vector<uint16_t> turn;
    void resize(size_t n, int hw) {
        for (auto* v : {&p1_pos, &p2_pos}) v->resize(n * 2);
        for (auto* v : {&p1_mud, &p2_mud, &a1, &a2}) v->resize(n);
        for (auto* v : {&p1_score, &p2_score}) v->resize(n);
        turn.resize(n);
        cheese_mask.resize(n * hw);
    }
    template <int NW>
    void set(size_t i, const State<NW>& s, uint32_t act1, uint32_t act2, int w, int hw) {
        p1_pos[i * 2] = s.p1 % w;
        p1_pos[i * 2 + 1] = s.p1 / w;
        p2_pos[i * 2] = s.p2 % w;
        p2_pos[i * 2 + 1] = s.p2 / w;
        p1_mud[i] = s.m1;
        p2_mud[i] = s.m2;
        turn[i] = s.turn;
        p1_score[i] = s.s1;
        p2_score[i] = s.s2;
        for (int c = 0; c < hw; ++c) cheese_mask[i * hw + c] = st_has_cheese(s, c) ? 1 : 0;
        a1[i] = (uint8_t)act1;
        a2[i] = (uint8_t)act2;
    }
    template <typename View>
    void point(View& v) const {  // ArGameRecordView / ArMatchGameView
        v.p1_pos = p1_pos.data();
        v.p2_pos = p2_pos.data();
        v.p1_score = p1_score.data();
        v.p2_score = p2_score.data();
        v.p1_mud = p1_mud.data();
        v.p2_mud = p2_mud.data();
        v.turn = turn.data();
        v.cheese_mask = cheese_mask.data();
        v.action_p1 = a1.data();
        v.action_p2 = a2.data();
    }
};

struct GameRecordHost : PosColumns {  // owning twin of ArGameRecordView
    uint8_t width, height;
    uint16_t max_turns;
    uint32_t game_index, n;
    std::vector<int8_t> maze;
    std::vector<uint8_t> initial_cheese, cheese_outcomes;
    float final_p1, final_p2;
    uint8_t result;
    uint16_t cheese_available;
    uint64_t sims, nn, term, coll;
    std::vector<float> v1, v2, vc1, vc2, pr1, pr2, po1, po2;
    ArGameRecordView view() const {
        ArGameRecordView v;
        memset(&v, 0, sizeof v);
        v.width = width;
        v.height = height;
        v.max_turns = max_turns;
        v.game_index = game_index;
        v.n_positions = n;
        v.maze = maze.data();
        v.initial_cheese = initial_cheese.data();
        v.cheese_outcomes = cheese_outcomes.data();
        v.final_p1_score = final_p1;
        v.final_p2_score = final_p2;
        v.result = result;
        v.cheese_available = cheese_available;
        v.total_simulations = sims;
        v.total_nn_evals = nn;
        v.total_terminals = term;
        v.total_collisions = coll;
        point(v);
        v.value_p1 = v1.data();
        v.value_p2 = v2.data();
        v.visit_counts_p1 = vc1.data();
        v.visit_counts_p2 = vc2.data();
        v.prior_p1 = pr1.data();
        v.prior_p2 = pr2.data();
        v.policy_p1 = po1.data();
        v.policy_p2 = po2.data();
        return v;
    }
};

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count) {
        n = count;
        return hipMalloc((void**)&p, sizeof(T) * (count ? count : 1));
    }
    ~DevBuf() {
        if (p) hipFree(p);
    }
};
// The collision budgets of a configuration whose power is not 1, computed here with the host's powf (the one the
// reference's budgets come from) and kept on the current device for collisions_left to look up: c.coll_table points into
// `buf`, which must live as long as kernels run with `c`. A power of 1 needs no table and leaves c.coll_table null.
static int make_coll_table(SearchCfg& c, DevBuf<uint32_t>& buf) {
    c.coll_table = nullptr;
    const uint32_t n = coll_table_size(c);
    if (n == 0) return AR_OK;
    std::vector<uint32_t> host(n);
    for (uint32_t k = 0; k < n; ++k) host[k] = collisions_left(c.coll_start + 1 + k, c);  // (the host's)
    HIP_TRY(buf.alloc(n));
    HIP_TRY(hipMemcpy(buf.p, host.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    c.coll_table = buf.p;
    return AR_OK;
}

template <typename T>
struct PinBuf {
    T* p = nullptr;
    hipError_t alloc(size_t count) { return hipHostMalloc((void**)&p, sizeof(T) * (count ? count : 1)); }
    ~PinBuf() {
        if (p) hipHostFree(p);
    }
};

// The arena allocation (first arenas + overflow pool) is by far the largest one, and the driver
// clears device memory when it hands it out (~30 ms per GB measured, 6-7 s for a full MI355X). One
// block per device is therefore kept between calls: a training loop that calls ar_selfplay_run once
// per iteration pays for it once. ar_release_device_memory() (or AR_NO_ARENA_CACHE=1) gives it back.
struct ArenaBlock {
    unsigned char* p = nullptr;
    size_t bytes = 0;
};
enum { MAX_DEVICES = 64 };
static std::mutex g_arena_mu;
static ArenaBlock g_arena_cache[MAX_DEVICES];

static size_t arena_cached_bytes(int dev) {
    std::lock_guard<std::mutex> lk(g_arena_mu);
    return dev >= 0 && dev < MAX_DEVICES ? g_arena_cache[dev].bytes : 0;
}
static hipError_t arena_acquire(int dev, size_t bytes, ArenaBlock& out) {
    {
        std::lock_guard<std::mutex> lk(g_arena_mu);
        if (dev >= 0 && dev < MAX_DEVICES) {
            ArenaBlock& c = g_arena_cache[dev];
            if (c.p && c.bytes >= bytes) {
                out = c;
                c = ArenaBlock();
                return hipSuccess;
            }
            if (c.p) {  // too small for this call: make room for the new one
                hipFree(c.p);
                c = ArenaBlock();
            }
        }
    }
    out.bytes = bytes;
    return hipMalloc((void**)&out.p, bytes);
}
static void arena_release(int dev, ArenaBlock b) {
    if (!b.p) return;
    if (!getenv("AR_NO_ARENA_CACHE") && dev >= 0 && dev < MAX_DEVICES) {
        std::lock_guard<std::mutex> lk(g_arena_mu);
        ArenaBlock& c = g_arena_cache[dev];
        if (!c.p) {
            c = b;
            return;
        }
        if (c.bytes < b.bytes) std::swap(c, b);  // keep the bigger of the two
    }
    hipFree(b.p);
}
struct ArenaHold {
    unsigned char* p = nullptr;
    ArenaBlock blk;
    int dev = -1;
    hipError_t alloc(int device, size_t bytes) {
        dev = device;
        const hipError_t e = arena_acquire(device, bytes, blk);
        p = blk.p;
        return e;
    }
    ~ArenaHold() { arena_release(dev, blk); }
};

// The kernel that walks the trees of the split pipeline (results are identical; Engine::choose_gather):
// - Wide: the work queue over tree levels (k_gatherw, dev_gatherw.h), the default of network runs whose batches it serves.
// - Octet2 / Octet3: eight lanes per game (k_gather8). Measured on the bench workload (DESIGN.md section 7,
//   profiles/r02_gather_ab.md) it is faster per launch than one lane per game at every size -- 1.9x / 1.7x at 1024 /
//   8192 resident games, where its eight-fold wavefront count fills SIMDs the lane-per-game kernel leaves to one
//   wavefront or none, and still ahead at 65536 once the shared maze sits in LDS and three wavefronts share a SIMD.
//   Its register budget: two wavefronts per SIMD without spills up to 32768 games (Octet2), three (168 VGPRs) above.
// - Lane: one lane per game (k_gather).
enum class GatherKernel { Lane, Octet2, Octet3, Wide };
// measured (BASELINE config 2: 5x5, 1000 sims, 4096 games: 71.1 M vs 41.5 M simulations/s through the split pipeline;
// 7x7 / 1897 sims at 65536 games: 1180 M vs 1251 M): few games want k_gather8's wavefront count, many the fused kernel
static bool default_uniform_queue(uint32_t resident_games) { return resident_games <= 16384u; }

// ar_debug_advance: the compaction of dev_advance.h on trees the caller made up, one block per tree; a tree either stays
// on its records or moves to the same place of a second buffer
struct DbgAdvTree {
    uint32_t first, hi, keep_root, moves;
};
__global__ void __launch_bounds__(ADV_THREADS) k_dbg_advance(NodeStats* recs, NodeStats* other, uint32_t* fwd, const DbgAdvTree* trees,
                                                             uint32_t n, uint32_t fast_nodes, uint32_t* counts) {
    __shared__ AdvLds L;
    if (blockIdx.x >= n) return;
    const DbgAdvTree t = trees[blockIdx.x];
    NodeStats* src = recs + t.first;
    NodeStats* dst = t.moves ? other + t.first : src;
    const uint32_t cnt = advance_compact(src, fwd + t.first, t.hi, t.keep_root, fast_nodes, L, [&](uint32_t) { return dst; });
    if (threadIdx.x == 0) counts[blockIdx.x] = cnt;
}

// the ziggurat tables every engine copies to its device (zig.p); ar_debug_draws copies the same object
static const ZigTables g_host_zig = {AR_ZIG_NORM_X_INIT, AR_ZIG_NORM_F_INIT};

// ar_debug_budgets / ar_debug_draws: the scalar routines of dev_search.h and dev_rng.h by themselves, one thread per item,
// so that what the device's math library and code generation return can be compared with the host's, call by call
__global__ void k_dbg_budgets(const uint32_t* node_counts, uint32_t n, SearchCfg cfg, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = collisions_left(node_counts[i], cfg);
}

enum { DBG_DRAW_U64 = 0, DBG_DRAW_BELOW = 1, DBG_DRAW_WEIGHTED5 = 2, DBG_DRAW_NORMAL = 3, DBG_DRAW_GAMMA = 4, DBG_DRAW_DIRICHLET = 5, DBG_DRAW_KINDS = 6 };
// kind; draws per stream; n: the range of rng_below, the outcome count of dirichlet_mix; w: the weights of rng_weighted5,
// the prior every dirichlet_mix starts from; shape: of rng_gamma; epsilon, concentration: of dirichlet_mix
struct DbgDraw {
    uint32_t kind, count, n;
    float w[5];
    double shape;
    float epsilon, concentration;
};
static size_t dbg_draw_bytes(uint32_t kind) { return kind == DBG_DRAW_BELOW || kind == DBG_DRAW_WEIGHTED5 ? 4 : kind == DBG_DRAW_DIRICHLET ? 20 : 8; }
// stream s: rng_seed(seeds[s]), then d.count draws; draw i of stream s is item s * d.count + i of `out` (u64: rng_u64 and
// the bits of the f64 draws; u32: rng_below, rng_weighted5 with -1 as 0xFFFFFFFF; five f32: the mixed prior); states:
// the four words of the stream after its last draw
__global__ void k_dbg_draws(const uint64_t* seeds, uint32_t n_streams, DbgDraw d, const ZigTables* zt, void* out, uint64_t* states) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    Rng r;
    rng_seed(r, seeds[s]);
    const size_t first = (size_t)s * d.count;
    for (uint32_t i = 0; i < d.count; ++i) {
        const size_t at = first + i;
        if (d.kind == DBG_DRAW_U64) {
            ((uint64_t*)out)[at] = rng_u64(r);
        } else if (d.kind == DBG_DRAW_BELOW) {
            ((uint32_t*)out)[at] = rng_below(r, d.n);
        } else if (d.kind == DBG_DRAW_WEIGHTED5) {
            ((uint32_t*)out)[at] = (uint32_t)rng_weighted5(r, d.w);
        } else if (d.kind == DBG_DRAW_NORMAL) {
            ((double*)out)[at] = rng_normal(r, zt);
        } else if (d.kind == DBG_DRAW_GAMMA) {
            ((double*)out)[at] = rng_gamma(r, d.shape, zt);
        } else {
            float prior[5];
            for (int k = 0; k < 5; ++k) prior[k] = d.w[k];
            dirichlet_mix(prior, d.n, d.epsilon, d.concentration, r, zt);
            for (int k = 0; k < 5; ++k) ((float*)out)[at * 5 + k] = prior[k];
        }
    }
    states[4 * (size_t)s + 0] = r.a;
    states[4 * (size_t)s + 1] = r.b;
    states[4 * (size_t)s + 2] = r.c;
    states[4 * (size_t)s + 3] = r.d;
}

#if defined(AR_STATS)
static void* g_dbg_slots;
static uint32_t g_dbg_S, g_dbg_nw;
template <int NW>
__global__ void k_dbg_tree_hist(const Slot<NW>* slots, uint32_t n, unsigned long long* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Slot<NW>& s = slots[i];
    if (s.status == SLOT_EMPTY || s.status == SLOT_DONE) return;
    atomicAdd(&out[min(s.hi / 512u, 63u)], 1ULL);
    atomicAdd(&out[64 + min(s.cap / 512u, 63u)], 1ULL);
    atomicAdd(&out[128], (unsigned long long)s.hi);
    atomicAdd(&out[129], (unsigned long long)s.cap);
    atomicAdd(&out[130], 1ULL);
}
#endif
template <int NW>
struct Engine {
    int dev = 0;
    hipStream_t stream = nullptr;
    uint32_t S = 0;
    SearchCfg cfg;
    SlotLayout L;
    uint32_t max_turns = 0, cap0 = 0;
    DevBuf<Slot<NW>> slots;
    DevBuf<unsigned char> scratch;
    ArenaHold arena;
    DevBuf<uint8_t> maze;
    DevBuf<ZigTables> zig;
    DevBuf<uint32_t> coll_table;  // cfg.coll_table
    DevBuf<uint32_t> counts, done_list, stall_list, release_list;
    DevBuf<StallInfo> stall_info;
    DevBuf<GameInit<NW>> init;
    DevBuf<DoneInfo<NW>> info;
    DevBuf<PosRec<NW>> staging;
    DevBuf<GrowReq> grow;
    DevBuf<LeafReq<NW>> queue;
    DevBuf<EvalOut> ev_queue;
    DevBuf<uint32_t> queue_count;
    PinBuf<uint32_t> h_counts, h_release;
    DevBuf<unsigned long long> live;  // k_scan's sums over the resident games (LIVE_N values)
    PinBuf<unsigned long long> h_live;
    PinBuf<StallInfo> h_stall;
    PinBuf<DoneInfo<NW>> h_info;
    PinBuf<PosRec<NW>> h_staging;
    std::vector<void*> slot_grown;  // per slot: the arena the host allocated after a stall (nullptr = none)
    // host-allocated arenas are recycled by size instead of going back to the driver (hipMalloc + hipFree of
    // a few MB cost ~0.3 ms together, thousands of times per run when the overflow pool runs dry)
    std::vector<uint32_t> slot_grown_cap;
    std::multimap<uint32_t, void*> spare_arenas;  // cap -> block
    void retire_arena(uint32_t slot) {
        if (slot_grown[slot]) spare_arenas.emplace(slot_grown_cap[slot], slot_grown[slot]);
        slot_grown[slot] = nullptr;
    }
    // generated mazes: one pool entry per slot, rewritten when a new game starts there (open mazes: one shared entry)
    bool per_slot_maze = false;
    uint32_t maze_stride = 0;
    DevBuf<uint8_t> maze_stage;
    DevBuf<uint32_t> maze_ids;
    // NN-evaluation cache (k_cache_probe / k_cache_fill); cache_entries == 0: off
    uint64_t cache_entries = 0;
    DevBuf<CacheEntry<NW>> cache_table;
    DevBuf<LeafReq<NW>> miss_queue;
    DevBuf<uint32_t> miss_map, miss_count;
    DevBuf<EvalOut> ev_miss;
    DevBuf<unsigned long long> cache_counters;
    ArenaPool pool = {};            // overflow blocks handed out by the kernels themselves
    bool backup16 = false;       // network path: the sixteen-lanes-per-game backup (k_backup16 + k_finish) instead of k_backup
    bool uniform_queue = false;  // SmartUniform through the split pipeline (leaf queue + k_uniform_eval) instead of k_step_uniform
    bool use_queue() const { return net != nullptr || uniform_queue; }
    GatherKernel gather = GatherKernel::Lane;  // the split pipeline's gather (setup() chooses it)
    // k_gatherw runs as a persistent grid of `gatherw_waves`
    uint32_t gatherw_waves = 2048;
    // passes one launch may run; gathers that are not complete then are parked between two picks and go on in the next
    // launch. A game needs 50 passes in the median, 110 at the 90th and 160 at the 99th percentile, a few need 300+
    // (profiles/r03_gw_stats.txt): without a limit every launch lasts as long as its slowest game. Measured at 131072
    // resident games: 64 / 80 / 96 / 128 / 192 passes -> 638 / 646 / 643 / 615 / 598 M simulations/s; with the faster
    // evaluator and the late tree reuse of the round's end, over windows of five generations of games: 32 / 48 / 64 / 96 ->
    // 726 / 732 / 730 / 721 M (profiles/r03_sweeps.md; shorter windows sample one phase of the games and mislead).
    uint32_t gatherw_passes = 64;
    uint32_t gather_rounds = 0xFFFFFFFFu;  // rounds one k_gather launch may run per lane (set before setup())
    size_t region_bytes = 0;
    uint32_t region_low_mb = 0xFFFFFFFFu;  // least the region had left: MB never carved + MB in free blocks
    DevBuf<unsigned long long> pool_bits;
    DevBuf<int> pool_ctr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_order = nullptr;  // ev_order: side streams start after the main stream's refills
    double device_ms = 0.0;
    uint64_t steps = 0;
    uint64_t grows = 0;
    bool timed = false;
    ArNet* net = nullptr;

    ~Engine() {
        if (stream) hipStreamSynchronize(stream);
        for (Group& g : groups) {
            if (g.stream && g.stream != stream) {
                hipStreamSynchronize(g.stream);
                hipStreamDestroy(g.stream);
            }
            if (g.adv_stream) {
                hipStreamSynchronize(g.adv_stream);
                hipStreamDestroy(g.adv_stream);
            }
            if (g.done) hipEventDestroy(g.done);
            if (g.backed_up) hipEventDestroy(g.backed_up);
            if (g.gathered) hipEventDestroy(g.gathered);
            if (g.adv_ev[0]) hipEventDestroy(g.adv_ev[0]);
            if (g.adv_ev[1]) hipEventDestroy(g.adv_ev[1]);
            if (g.adv_done) hipEventDestroy(g.adv_done);
        }
        for (void* p : slot_grown)
            if (p) hipFree(p);
        for (auto& kv : spare_arenas) hipFree(kv.second);
        for (hipEvent_t e : gather_ev) hipEventDestroy(e);
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
        if (ev_order) hipEventDestroy(ev_order);
        if (stream) hipStreamDestroy(stream);
    }

    Bases bases() const {
        Bases b;
        b.arena = arena.p;
        b.scratch = scratch.p;
        b.maze = maze.p;
        b.maze_stage = (!per_slot_maze && maze.n > 0 && maze.n <= MAZE_STAGE_BYTES && maze.n % 4 == 0) ? (uint32_t)maze.n : 0u;
        b.L = L;
        b.pool = pool;
        return b;
    }

    // bytes of device memory setup() takes besides the arenas, per resident game
    static size_t per_game_overhead(const SearchCfg& c, uint32_t mt, bool need_queue) {
        size_t b = make_layout<NW>(c, mt).total + sizeof(Slot<NW>) + sizeof(PosRec<NW>) * mt + sizeof(GameInit<NW>) +
                   sizeof(DoneInfo<NW>) + sizeof(StallInfo) + sizeof(GrowReq) + 16;
        if (need_queue) b += (size_t)c.batch_size * (sizeof(LeafReq<NW>) + sizeof(EvalOut));
        return b;
    }

    // The gather of the split pipeline, from S, L, cfg, net and gather_rounds; AR_GATHER = wide | octet | octet2 | octet3 |
    // lane asks for one (results are identical).
    GatherKernel choose_gather(bool need_queue) const {
        // the work-queue gather serves batches of up to GW_SLOTS descents and GW_MAX_PICKS picks (batch_size + collision
        // budget: its entries carry a 12-bit pick number); with uniform priors nearly every allocation step draws a tie
        // break, which puts its items in sequence again: those runs keep the eight-lane kernel
        const bool fits = need_queue && cfg.batch_size <= GW_SLOTS &&
                          cfg.batch_size + std::max(cfg.coll_min, cfg.coll_max) <= (uint32_t)GW_MAX_PICKS;
        const bool big = (size_t)S * L.total >= ((size_t)1 << 32);  // k_gather8 addresses scratch with 32-bit offsets
        const GatherKernel octet = big ? GatherKernel::Lane : S <= 32768u ? GatherKernel::Octet2 : GatherKernel::Octet3;
        const char* e = getenv("AR_GATHER");
        const std::string want = e ? e : "";
        if (gather_rounds != 0xFFFFFFFFu) return GatherKernel::Lane;  // the round limit parks the walk: lane kernel only
        if (!e) return net != nullptr && fits ? GatherKernel::Wide : octet;
        if (want == "wide") return fits ? GatherKernel::Wide : octet;
        if (want == "octet2") return big ? GatherKernel::Lane : GatherKernel::Octet2;
        if (want == "octet3") return big ? GatherKernel::Lane : GatherKernel::Octet3;
        if (want.rfind("octet", 0) == 0) return octet;
        return GatherKernel::Lane;
    }

    // What a driver decides before setup(). `n`: the evaluator, nullptr = SmartUniform; `host_eval`: the leaves go to the
    // caller's predict_fn instead. SmartUniform runs in the fused step kernel, or in the split pipeline of the network path
    // with k_uniform_eval as its evaluator: the default for `games` resident games, or AR_UNIFORM=fused | queue (results
    // are identical). `slot_maze_cells` != 0: generated mazes, one pool entry of that many cells per slot, filled when a
    // game starts there. `arena_knob`: the run honours the AR_ARENA_NODES test knob (small arenas: trees stall and grow).
    uint32_t arena_nodes = 0;
    void configure(ArNet* n, uint32_t games, uint32_t slot_maze_cells, bool arena_knob = true, bool host_eval = false) {
        net = host_eval ? nullptr : n;
        const char* e = getenv("AR_UNIFORM");
        uniform_queue = !host_eval && net == nullptr && (e ? std::string(e) == "queue" : default_uniform_queue(games));
        per_slot_maze = slot_maze_cells != 0;
        maze_stride = slot_maze_cells * 4u;
        arena_nodes = arena_knob && getenv("AR_ARENA_NODES") ? (uint32_t)atoi(getenv("AR_ARENA_NODES")) : 0u;
    }

    // After configure(). `shared_maze`: the maze pool of a run without generated mazes.
    // `tree_bytes`: device memory for the trees (0 = one smallest block per game: every growth goes through the host)
    int setup(int device, uint32_t n_slots, const SearchCfg& c, uint32_t mt, const std::vector<uint8_t>& shared_maze,
              size_t tree_bytes = 0) {
        const std::vector<uint8_t> slot_mazes(per_slot_maze ? (size_t)n_slots * maze_stride : 0, (uint8_t)0);
        const std::vector<uint8_t>& maze_bytes = per_slot_maze ? slot_mazes : shared_maze;
        const bool need_queue = use_queue();
        dev = device;
        S = n_slots;
        cfg = c;
        max_turns = mt;
        HIP_TRY(hipSetDevice(dev));
        if (int rc = make_coll_table(cfg, coll_table)) return rc;
        HIP_TRY(hipStreamCreate(&stream));
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventCreateWithFlags(&ev_order, hipEventDisableTiming));
        L = make_layout<NW>(cfg, max_turns);
        static_assert(sizeof(LevelO<NW>) <= (16 + 112 + sizeof(State<NW>) + 15) / 16 * 16, "slot_layout.h sizes the level stack");
        // which backup kernel (results are identical): AR_BACKUP=lane | group; the group kernel keeps 64 paths in LDS
        // (the deep part of its paths lives in the level-stack scratch, which make_layout sizes for it too)
        backup16 = true;
        if (backup16_deep_bytes(L.max_depth) > L.ev_off - L.levels_off)
            return fail(AR_E_BACKEND, "slot layout: the level stack is smaller than k_backup16's path notes");
        if (const char* e = getenv("AR_BACKUP")) backup16 = backup16 && std::string(e) != "lane";
        gather = choose_gather(need_queue);
        if (gather == GatherKernel::Wide) {
            int cus = 0;
            HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
            // one wavefront per CU fewer than fit (twelve), 32 (16 on boards above 64 cells) games each: a full CU leaves no
            // room for the small kernels beside the gather (profiles/r04_ab.txt: 705 M simulations/s at 11, 651 M at 12)
            gatherw_waves = (uint32_t)(cus > 0 ? cus : 256) * GW_WAVES_PER_CU;
            if (const char* e = getenv("AR_GW_WAVES"))
                if (atoi(e) > 0) gatherw_waves = (uint32_t)atoi(e);
            if (const char* e = getenv("AR_GW_PASSES")) gatherw_passes = atoi(e) > 0 ? (uint32_t)atoi(e) : 0xFFFFFFFFu;  // 0: no limit
        }
        cap0 = arena_nodes ? (uint32_t)align_up(arena_nodes, 64) : initial_arena_nodes(cfg);  // (arenas are whole 256-byte units)
        if (const char* e = getenv("AR_ADV_NODES"))  // test knob, like AR_ARENA_NODES: small trees reach the slow path
            if (atoi(e) >= 0) adv_fast_nodes = (uint32_t)atoi(e) < (uint32_t)ADV_MAX_NODES ? (uint32_t)atoi(e) : (uint32_t)ADV_MAX_NODES;
        if (const char* e = getenv("AR_ADV_BLOCKS"))  // test knob: a smaller k_advance grid, so that a block takes several entries
            if (atoi(e) > 0) adv_blocks = (uint32_t)atoi(e) < (uint32_t)ADV_BLOCKS ? (uint32_t)atoi(e) : (uint32_t)ADV_BLOCKS;
        slot_grown.assign(S, nullptr);
        slot_grown_cap.assign(S, 0u);
        HIP_TRY(slots.alloc(S));
        HIP_TRY(hipMemsetAsync(slots.p, 0, sizeof(Slot<NW>) * S, stream));
        HIP_TRY(adv_list.alloc((size_t)ADV_CLASSES * S));
        HIP_TRY(adv_count.alloc(2 * ADV_CTXS * ADV_COUNTERS));
        HIP_TRY(hipMemsetAsync(adv_count.p, 0, sizeof(uint32_t) * 2 * ADV_CTXS * ADV_COUNTERS, stream));
#if defined(AR_STATS)
        g_dbg_slots = slots.p;
        g_dbg_S = S;
        g_dbg_nw = NW;
#endif
        HIP_TRY(scratch.alloc((size_t)S * L.total));
        // the tree region: pages, a bitmap per zone of 1024 slots; at least a fresh game's pages for every slot
        size_t region = tree_bytes;
        {
            pool.page_nodes = arena_nodes ? cap0 : (uint32_t)POOL_PAGE_NODES;  // (test knob: small pages, fresh games on a single one)
            pool.fresh_pages = arena_nodes ? 1u : (initial_arena_nodes(cfg) + POOL_PAGE_NODES - 1) / POOL_PAGE_NODES;
            // (initial_arena_nodes carries 2 * batch_size + 64 nodes of slack. A search adds at most one node per simulation
            // and a gather stalls only when hi + min(remaining, batch_size) > cap, so 1 + n_sims nodes are what a fresh game
            // needs: where the slack alone goes past the longest run -- batch sizes in the thousands -- the run is taken whole)
            if (pool.fresh_pages > POOL_WORD_PAGES &&
                (uint64_t)1 + cfg.n_sims + cfg.batch_size <= (uint64_t)POOL_WORD_PAGES * POOL_PAGE_NODES)
                pool.fresh_pages = POOL_WORD_PAGES;
            if (pool.fresh_pages > POOL_WORD_PAGES) return fail(AR_E_INVALID, "simulations per move beyond what one run of tree pages holds");
            cap0 = pool.fresh_pages * pool.page_nodes;
            pool.page_bytes = arena_bytes(pool.page_nodes);
            const size_t word_bytes = (size_t)POOL_WORD_PAGES * pool.page_bytes;
            pool.zones = (S + POOL_ZONE_SLOTS - 1) / POOL_ZONE_SLOTS;
            {
                // (every zone holds a fresh arena per slot of a full zone, with room for runs that do not pack a word)
                const size_t floor_b = (size_t)(S < POOL_ZONE_SLOTS ? S : (uint32_t)POOL_ZONE_SLOTS) * pool.fresh_pages * pool.page_bytes * 5 / 4 + word_bytes;
                const size_t share = region / pool.zones;
                const size_t zb = share > floor_b ? share : floor_b;
                pool.zone_words = (uint32_t)((zb + word_bytes - 1) / word_bytes);
            }
            pool.zone_bytes = (unsigned long long)pool.zone_words * word_bytes;
            region = (size_t)pool.zone_bytes * pool.zones;
            region_bytes = region;
            pool.ret_cap = 2 * POOL_ZONE_SLOTS + 64;
            HIP_TRY(pool_bits.alloc((size_t)pool.zones * pool.zone_words + (size_t)pool.zones * pool.ret_cap));
            HIP_TRY(hipMemsetAsync(pool_bits.p, 0, 8 * (size_t)pool.zones * pool.zone_words, stream));
            HIP_TRY(pool_ctr.alloc(pool.zones + 2));
            HIP_TRY(hipMemsetAsync(pool_ctr.p, 0, sizeof(int) * (pool.zones + 2), stream));
            pool.bits = pool_bits.p;
            pool.ret = pool_bits.p + (size_t)pool.zones * pool.zone_words;
            pool.ret_n = (uint32_t*)pool_ctr.p;
        }
        const size_t pool_end = region;
        HIP_TRY(arena.alloc(dev, pool_end + 256));
        HIP_TRY(maze.alloc(maze_bytes.size()));
        HIP_TRY(hipMemcpyAsync(maze.p, maze_bytes.data(), maze_bytes.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(zig.alloc(1));
        HIP_TRY(hipMemcpyAsync(zig.p, &g_host_zig, sizeof g_host_zig, hipMemcpyHostToDevice, stream));
        HIP_TRY(counts.alloc(8));
        HIP_TRY(release_list.alloc(S));
        HIP_TRY(h_release.alloc(S));
        HIP_TRY(done_list.alloc(S));
        HIP_TRY(stall_list.alloc(S));
        HIP_TRY(stall_info.alloc(S));
        HIP_TRY(init.alloc(S));
        HIP_TRY(info.alloc(S));
        HIP_TRY(staging.alloc((size_t)S * max_turns));
        HIP_TRY(grow.alloc(S));
        HIP_TRY(h_counts.alloc(8));
        HIP_TRY(live.alloc(16));
        HIP_TRY(h_live.alloc(16));
        HIP_TRY(h_stall.alloc(S));
        HIP_TRY(h_info.alloc(S));
        HIP_TRY(h_staging.alloc((size_t)S * max_turns));
        if (need_queue) {
            HIP_TRY(queue.alloc((size_t)S * cfg.batch_size));
            HIP_TRY(ev_queue.alloc((size_t)S * cfg.batch_size));
            HIP_TRY(queue_count.alloc(64));
        }
        if (need_queue && cache_entries) {
            HIP_TRY(cache_table.alloc(cache_entries));
            HIP_TRY(hipMemsetAsync(cache_table.p, 0, sizeof(CacheEntry<NW>) * cache_entries, stream));
            HIP_TRY(miss_queue.alloc((size_t)S * cfg.batch_size));
            HIP_TRY(miss_map.alloc((size_t)S * cfg.batch_size));
            HIP_TRY(ev_miss.alloc((size_t)S * cfg.batch_size));
            HIP_TRY(miss_count.alloc(64));
            HIP_TRY(cache_counters.alloc(2));
            HIP_TRY(hipMemsetAsync(cache_counters.p, 0, 16, stream));
        }
        if (net != nullptr) {
            const size_t per = (size_t)net->dev.hw * 4;
            if (maze_bytes.size() % per != 0) return fail(AR_E_INVALID, "maze pool does not match the network's board size");
            if (int rc = net_bind_mazes(net, maze.p, (int)(maze_bytes.size() / per), stream)) return rc;
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return AR_OK;
    }

    uint32_t grid(uint32_t n) const { return (n + 63) / 64; }

    // `mazes`: games.size() x maze_stride bytes when per_slot_maze
    int start_games(std::vector<GameInit<NW>>& games, const std::vector<uint8_t>* mazes = nullptr) {
        if (games.empty()) return AR_OK;
        for (GameInit<NW>& g : games) {  // a new game starts in the slot's first arena again
            g.reset_arena = 0;
            if (slot_grown[g.slot]) {
                retire_arena(g.slot);  // the slot was drained: no kernel touches that arena any more
                g.reset_arena = 1;
            }
        }
        HIP_TRY(hipMemcpyAsync(init.p, games.data(), sizeof(GameInit<NW>) * games.size(), hipMemcpyHostToDevice, stream));
        if (per_slot_maze) {
            if (!mazes || mazes->size() != games.size() * (size_t)maze_stride) return fail(AR_E_INVALID, "internal: mazes missing");
            if (!maze_stage.p) {
                HIP_TRY(maze_stage.alloc((size_t)S * maze_stride));
                HIP_TRY(maze_ids.alloc(S));
            }
            HIP_TRY(hipMemcpyAsync(maze_stage.p, mazes->data(), mazes->size(), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(k_place_mazes<NW>, dim3((uint32_t)games.size()), dim3(64), 0, stream, init.p,
                               (uint32_t)games.size(), maze_stage.p, maze_stride, maze.p, maze_ids.p);
            if (net != nullptr)
                if (int rc = net_rebind_mazes(net, maze_ids.p, (int)games.size(), stream)) return rc;
        }
        hipLaunchKernelGGL(k_init_games<NW>, dim3(grid((uint32_t)games.size())), dim3(64), 0, stream, slots.p, init.p,
                           (uint32_t)games.size(), bases(), cfg);
        HIP_TRY(hipGetLastError());
        // init.p is reused by the next call: wait for the copy + kernel
        HIP_TRY(hipStreamSynchronize(stream));
        return AR_OK;
    }

    // Games are split into `n_groups` contiguous slot ranges, each with its own stream and evaluator
    // queue. The groups run the same gather -> evaluate -> backup -> advance sequence independently, so
    // the compute-bound network kernel of one group overlaps the latency-bound tree walks of the others.
    // Tree reuse (k_advance) runs on a side stream per group: its duration is that of the one slowest
    // compaction, and the games it works on sit out the next step anyway, so the next gather does not
    // wait for it (ownership of a slot passes through its status word, see tag_status).
    struct Group {
        hipStream_t stream = nullptr, adv_stream = nullptr;
        hipEvent_t done = nullptr, backed_up = nullptr, adv_done = nullptr, adv_ev[2] = {nullptr, nullptr};
        hipEvent_t gathered = nullptr;  // the group's last gather launch is complete
        uint32_t first = 0, end = 0;  // slots [first, end)
        uint64_t step = 0;
        bool adv_pending = false;  // (late tree reuse) the last step's k_advance has not been launched yet
        uint32_t adv_phase = 0;
    };
    // HIP events around every k_gather launch of group 0 (on the stream it runs on); read back in scan()
    std::vector<hipEvent_t> gather_ev;
    size_t gather_ev_used = 0;
    double gather_ms = 0.0;
    uint64_t gather_launches = 0;
    bool overlap_advance = true;
    bool merge_per_group = false;
    std::vector<Group> groups;
    int make_groups(uint32_t n) {
        if (n < 1) n = 1;
        if (n > S) n = S;
        groups.resize(n);
        // groups of whole pool zones when there are enough games: a group's tree reuse then hands blocks out and takes
        // them back in its own zones only, and can put returned blocks back on the free stacks at every step
        merge_per_group = S / n >= POOL_ZONE_SLOTS;
        auto cut = [&](uint32_t g) {
            uint32_t at = (uint32_t)((uint64_t)S * g / n);
            if (merge_per_group && g > 0 && g < n) at = at / POOL_ZONE_SLOTS * POOL_ZONE_SLOTS;
            return at;
        };
        for (uint32_t g = 0; g < n; ++g) {
            groups[g].first = cut(g);
            groups[g].end = cut(g + 1);
            // group 0 runs on the engine's own stream: with two groups that makes four streams (two step streams, two
            // tree-reuse side streams), which is what the runtime maps to hardware queues by default (GPU_MAX_HW_QUEUES
            // = 4); a fifth stream shares a queue with another and the pipeline collapses (measured: 321 M against
            // 565 M simulations/s)
            HIP_TRY(hipEventCreateWithFlags(&groups[g].gathered, hipEventDisableTiming));
            if (g > 0) {
                HIP_TRY(hipStreamCreateWithFlags(&groups[g].stream, hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&groups[g].done, hipEventDisableTiming));
            } else {
                groups[g].stream = stream;
            }
            if (overlap_advance) {
                HIP_TRY(hipStreamCreateWithFlags(&groups[g].adv_stream, hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&groups[g].backed_up, hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&groups[g].adv_done, hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&groups[g].adv_ev[0], hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&groups[g].adv_ev[1], hipEventDisableTiming));
            }
        }
        return AR_OK;
    }
    int group_step(Group& g) {
        const uint32_t n = g.end - g.first, gi = (uint32_t)(&g - groups.data());
        const bool side = g.adv_stream != nullptr;
        const uint32_t phase = side ? (uint32_t)(g.step & 1) : 0u;
        const uint32_t ready = side ? (uint32_t)SLOT_READY_A + phase : (uint32_t)SLOT_ACTIVE;
        if (side) HIP_TRY(hipStreamWaitEvent(g.stream, g.adv_ev[phase], 0));  // advance(step - 2) is complete
        LeafReq<NW>* q = queue.p + (size_t)g.first * cfg.batch_size;
        EvalOut* ev = ev_queue.p + (size_t)g.first * cfg.batch_size;
        uint32_t* qc = queue_count.p + gi;
        HIP_TRY(hipMemsetAsync(qc, 0, 4, g.stream));
        while (gather_ev.size() < gather_ev_used + 2) {  // every group's gather launch is timed on its own stream
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreate(&e));
            gather_ev.push_back(e);
        }
        HIP_TRY(hipEventRecord(gather_ev[gather_ev_used], g.stream));
        switch (gather) {
        case GatherKernel::Wide: {
            // a persistent grid: at most gatherw_waves wavefronts, and at small sizes about four games per wavefront
            constexpr int GWG = NW == 1 ? 32 : 16;
            uint32_t waves = (n + 3) / 4;
            if (waves > gatherw_waves) waves = gatherw_waves;
            const uint32_t n_sets = (n + GWG - 1) / GWG, second_turn = n_sets > waves ? n_sets - waves : 0u;
            const uint32_t rot = second_turn ? (uint32_t)((g.step * (uint64_t)second_turn) % n_sets) : 0u;
            hipLaunchKernelGGL((k_gatherw<NW, GWG, GW_RECS>), dim3(waves), dim3(64), (size_t)bases().maze_stage, g.stream, slots.p, g.end, cfg,
                               bases(), g.first, phase, ready, gatherw_passes, rot);
            break;
        }
        case GatherKernel::Octet2:
            hipLaunchKernelGGL((k_gather8<NW, 2>), dim3((n + 7) / 8), dim3(64), 0, g.stream, slots.p, g.end, cfg, bases(), q,
                               qc, g.first, phase, ready);
            break;
        case GatherKernel::Octet3:
            hipLaunchKernelGGL((k_gather8<NW, 3>), dim3((n + 7) / 8), dim3(64), 0, g.stream, slots.p, g.end, cfg, bases(), q,
                               qc, g.first, phase, ready);
            break;
        case GatherKernel::Lane:
            hipLaunchKernelGGL(k_gather<NW>, dim3(grid(n)), dim3(64), 0, g.stream, slots.p, g.end, cfg, bases(), q, qc,
                               gather_rounds, g.first, phase, ready);
            break;
        }
        HIP_TRY(hipEventRecord(gather_ev[gather_ev_used + 1], g.stream));
        gather_ev_used += 2;
        HIP_TRY(hipEventRecord(g.gathered, g.stream));
        if (g.adv_pending)
            if (int rc = launch_late_advance(g)) return rc;
        if (gather == GatherKernel::Wide)
            hipLaunchKernelGGL(k_pack_leaves<NW>, dim3((n + 63) / 64), dim3(64), 0, g.stream, slots.p, g.end, bases(), g.first, q, qc);
        const uint32_t n_max = (uint32_t)((size_t)n * cfg.batch_size);
        if (cache_entries && net != nullptr) {
            LeafReq<NW>* mq = miss_queue.p + (size_t)g.first * cfg.batch_size;
            uint32_t* mm = miss_map.p + (size_t)g.first * cfg.batch_size;
            EvalOut* em = ev_miss.p + (size_t)g.first * cfg.batch_size;
            uint32_t* mc = miss_count.p + gi;
            HIP_TRY(hipMemsetAsync(mc, 0, 4, g.stream));
            hipLaunchKernelGGL(k_cache_probe<NW>, dim3((n_max + 255) / 256), dim3(256), 0, g.stream, q, qc, slots.p,
                               cache_table.p, cache_entries - 1, ev, mq, mm, mc, cache_counters.p, per_slot_maze ? 1u : 0u);
            if (int rc = net_forward_queue<NW>(net, mq, mc, n_max, slots.p, maze.p, em, g.stream)) return rc;
            hipLaunchKernelGGL(k_cache_fill<NW>, dim3((n_max + 255) / 256), dim3(256), 0, g.stream, mq, mm, mc, em, slots.p,
                               cache_table.p, cache_entries - 1, ev, per_slot_maze ? 1u : 0u);
        } else if (net == nullptr) {
            hipLaunchKernelGGL(k_uniform_eval<NW>, dim3((n_max + 255) / 256), dim3(256), 0, g.stream, q, qc, slots.p, maze.p, ev);
        } else if (int rc = net_forward_queue<NW>(net, q, qc, n_max, slots.p, maze.p, ev, g.stream)) {
            return rc;
        }
        if (backup16) {
            const uint32_t path_cap = L.max_depth + 2;
            hipLaunchKernelGGL(k_backup16<NW>, dim3((n + 3) / 4), dim3(64), (size_t)BACKUP16_LDS_BYTES,
                               g.stream, slots.p, g.end, cfg, bases(), zig.p, ev, g.first, path_cap);
            hipLaunchKernelGGL(k_finish<NW>, dim3(grid(n)), dim3(64), 0, g.stream, slots.p, g.end, cfg, bases(), g.first, phase);
            // (fresh roots that draw Dirichlet noise were left alone above; k_finish ignores a slot with a batch pending)
            if (cfg.noise_epsilon > 0.0f)
                hipLaunchKernelGGL(k_backup<NW>, dim3(grid(n)), dim3(64), 0, g.stream, slots.p, g.end, cfg, bases(), zig.p, ev,
                                   g.first, phase);
        } else
            hipLaunchKernelGGL(k_backup<NW>, dim3(grid(n)), dim3(64), 0, g.stream, slots.p, g.end, cfg, bases(), zig.p, ev,
                               g.first, phase);
        if (side) {
            // The tree reuse of this step is launched behind the NEXT gather of the group (launch_late_advance),
            // so that it runs beside the evaluator, which leaves the memory system alone, instead of beside the tree walk,
            // which it slows down by a fifth (profiles/r03_sweeps.md: the gather launch with and without k_advance beside it)
            HIP_TRY(hipEventRecord(g.backed_up, g.stream));
            g.adv_pending = true;
            g.adv_phase = phase;
        } else {
            // blocks the group's trees left at the last step go back on the free stacks (nothing reads them any more, and
            // this stream is the only one that pops or returns in the group's zones)
            if (merge_per_group && pool.bits) {
                const uint32_t z0 = g.first / POOL_ZONE_SLOTS, z1 = (g.end + POOL_ZONE_SLOTS - 1) / POOL_ZONE_SLOTS;
                hipLaunchKernelGGL(k_pool_merge, dim3(z1 - z0), dim3(64), 0, g.stream, pool, z0, z1 - z0);
            }
            launch_k_advance(g.stream, g.first, g.end, 0u, (uint32_t)SLOT_ACTIVE, gi);
        }
        g.step += 1;
        return AR_OK;
    }

    // tree reuse of slots [first, end) on `st`: every launch site goes through here
    uint32_t adv_fast_nodes = ADV_MAX_NODES;  // (AR_ADV_NODES, a test knob: trees above it take the compaction's slow path)
    // `ctx`: which sequence of launches this one belongs to (a group's, or ADV_CTX_ALL for the launches over all slots):
    // the launches of a sequence are in stream order and alternate between the sequence's two counters
    enum { ADV_CTX_ALL = 64, ADV_CTXS = 65 };
    DevBuf<uint32_t> adv_list, adv_count;  // [ADV_CLASSES][S] slots that wait, grouped as the slots are; [ADV_CTXS][2][ADV_COUNTERS]
    uint64_t adv_seq[ADV_CTXS] = {};
    uint32_t adv_blocks = ADV_BLOCKS;  // (AR_ADV_BLOCKS, a test knob: a smaller grid, so that a block takes several entries)
    void launch_k_advance(hipStream_t st, uint32_t first, uint32_t end, uint32_t phase, uint32_t ready, uint32_t ctx) {
        const uint32_t n = end - first;
        uint32_t* cnt = adv_count.p + (2 * ctx + (uint32_t)(adv_seq[ctx] & 1)) * ADV_COUNTERS;
        uint32_t* cnt_next = adv_count.p + (2 * ctx + (uint32_t)((adv_seq[ctx] + 1) & 1)) * ADV_COUNTERS;
        adv_seq[ctx] += 1;
        hipLaunchKernelGGL(k_advance_scan<NW>, dim3((n + 255) / 256), dim3(256), 0, st, slots.p, end, first, phase, adv_list.p + first,
                           S, cnt, cnt_next);
        hipLaunchKernelGGL(k_advance<NW>, dim3(n < adv_blocks ? n : adv_blocks), dim3(ADV_THREADS), 0, st, slots.p,
                           bases(), cfg, phase, ready, adv_list.p + first, S, cnt, adv_fast_nodes);
    }

    // tree reuse of the group's previous step, on the side stream: after that step's backup and (when a gather has been
    // launched since) after that gather
    int launch_late_advance(Group& g) {
        HIP_TRY(hipStreamWaitEvent(g.adv_stream, g.backed_up, 0));
        HIP_TRY(hipStreamWaitEvent(g.adv_stream, g.gathered, 0));
        if (merge_per_group && pool.bits) {
            const uint32_t z0 = g.first / POOL_ZONE_SLOTS, z1 = (g.end + POOL_ZONE_SLOTS - 1) / POOL_ZONE_SLOTS;
            hipLaunchKernelGGL(k_pool_merge, dim3(z1 - z0), dim3(64), 0, g.adv_stream, pool, z0, z1 - z0);
        }
        launch_k_advance(g.adv_stream, g.first, g.end, g.adv_phase, (uint32_t)SLOT_READY_A + g.adv_phase, (uint32_t)(&g - groups.data()));
        HIP_TRY(hipEventRecord(g.adv_ev[g.adv_phase], g.adv_stream));
        g.adv_pending = false;
        return AR_OK;
    }

    void launch_gather(bool to_queue) {
        hipLaunchKernelGGL(k_gather<NW>, dim3(grid(S)), dim3(64), 0, stream, slots.p, S, cfg, bases(),
                           to_queue ? queue.p : (LeafReq<NW>*)nullptr, to_queue ? queue_count.p : (uint32_t*)nullptr,
                           gather_rounds, 0u, 0u, (uint32_t)SLOT_ACTIVE);
    }
    void launch_backup(bool from_queue) {
        hipLaunchKernelGGL(k_backup<NW>, dim3(grid(S)), dim3(64), 0, stream, slots.p, S, cfg, bases(), zig.p,
                           from_queue ? ev_queue.p : (const EvalOut*)nullptr, 0u, 0u);
    }
    void launch_advance() {
        if (pool.bits) hipLaunchKernelGGL(k_pool_merge, dim3(pool.zones), dim3(64), 0, stream, pool, 0u, pool.zones);
        launch_k_advance(stream, 0u, S, 0u, (uint32_t)SLOT_ACTIVE, (uint32_t)ADV_CTX_ALL);
    }
    void launch_cancel() { hipLaunchKernelGGL(k_cancel<NW>, dim3(grid(S)), dim3(64), 0, stream, slots.p, S, bases()); }

    // `n_launch` rounds of {`iters` simulate_batch per game, then tree reuse for the games that moved},
    // timed with HIP events on our stream
    int run_steps(int n_launch, int iters) {
        if (!timed) HIP_TRY(hipEventRecord(ev0, stream));  // several calls between two scans are timed as one interval
        for (int k = 0; k < n_launch; ++k) {
            if (!use_queue()) {
                hipLaunchKernelGGL(k_step_uniform<NW>, dim3(grid(S)), dim3(64), 0, stream, slots.p, S, cfg, bases(), zig.p,
                                   iters);
                launch_advance();
                steps += (uint64_t)iters;
            } else {
                steps += (uint64_t)iters;
            }
        }
        if (use_queue()) {
            if (groups.empty())
                if (int rc = make_groups(1)) return rc;
            HIP_TRY(hipEventRecord(ev_order, stream));
            for (const Group& g : groups) {
                if (g.stream != stream) HIP_TRY(hipStreamWaitEvent(g.stream, ev_order, 0));
                if (g.adv_stream) HIP_TRY(hipStreamWaitEvent(g.adv_stream, ev_order, 0));
            }
            for (int k = 0; k < n_launch * iters; ++k)
                for (Group& g : groups)
                    if (int rc = group_step(g)) return rc;
            for (Group& g : groups)
                if (g.adv_pending)
                    if (int rc = launch_late_advance(g)) return rc;
            for (const Group& g : groups) {
                if (g.stream != stream) {
                    HIP_TRY(hipEventRecord(g.done, g.stream));
                    HIP_TRY(hipStreamWaitEvent(stream, g.done, 0));
                }
                if (g.adv_stream) {  // the host's scan sees every slot at rest
                    HIP_TRY(hipEventRecord(g.adv_done, g.adv_stream));
                    HIP_TRY(hipStreamWaitEvent(stream, g.adv_done, 0));
                }
            }
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev1, stream));
        timed = true;
        return AR_OK;
    }

    // after run_steps: status lists on the host. Also accumulates device time.
    int scan(uint32_t out_counts[4]) {
        if (pool.bits) hipLaunchKernelGGL(k_pool_merge, dim3(pool.zones), dim3(64), 0, stream, pool, 0u, pool.zones);
        HIP_TRY(hipMemsetAsync(counts.p, 0, 32, stream));
        HIP_TRY(hipMemsetAsync(live.p, 0, 8 * 16, stream));
        hipLaunchKernelGGL(k_scan<NW>, dim3(grid(S)), dim3(64), 0, stream, slots.p, S, counts.p, done_list.p,
                           stall_list.p, release_list.p, pool, live.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_counts.p, counts.p, 32, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(h_live.p, live.p, 8 * 16, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (const uint32_t n_rel = h_counts.p[4]) {  // slots that moved back to their pool share
            HIP_TRY(hipMemcpyAsync(h_release.p, release_list.p, 4 * n_rel, hipMemcpyDeviceToHost, stream));
            hipLaunchKernelGGL(k_clear_release<NW>, dim3(grid(n_rel)), dim3(64), 0, stream, slots.p, release_list.p, n_rel);
            HIP_TRY(hipStreamSynchronize(stream));
            for (uint32_t i = 0; i < n_rel; ++i) retire_arena(h_release.p[i]);
        }
        if (timed) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) device_ms += ms;
            timed = false;
        }
        for (size_t i = 0; i + 1 < gather_ev_used; i += 2) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, gather_ev[i], gather_ev[i + 1]) == hipSuccess) {
                gather_ms += ms;
                gather_launches += 1;
            }
        }
        gather_ev_used = 0;
        for (int i = 0; i < 4; ++i) out_counts[i] = h_counts.p[i];
        {
            const uint32_t left_mb = (uint32_t)(((unsigned long long)h_counts.p[5] * pool.page_bytes) >> 20);
            if (left_mb < region_low_mb) region_low_mb = left_mb;
        }
        return AR_OK;
    }

    // stalled games get a doubled arena: live nodes are copied across unchanged (ids are arena-relative)
    // `may_wait`: other games are still running, so a stalled game that cannot be given memory now
    // simply stays stalled (k_advance retries it from the overflow pool on every launch)
    int handle_stalls(uint32_t n_stall, bool may_wait = false) {
        if (n_stall == 0) return AR_OK;
        hipLaunchKernelGGL(k_read_stall<NW>, dim3(grid(n_stall)), dim3(64), 0, stream, slots.p, stall_list.p, n_stall,
                           stall_info.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_stall.p, stall_info.p, sizeof(StallInfo) * n_stall, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        std::vector<GrowReq> reqs(n_stall);
        std::vector<std::pair<uint32_t, void*>> old_arenas;
        for (uint32_t i = 0; i < n_stall; ++i) {
            const StallInfo& si = h_stall.p[i];
            uint32_t ncap = si.cap * 2;
            while (ncap < si.need) ncap *= 2;
            unsigned char* na = nullptr;
            const auto spare = spare_arenas.find(ncap);
            if (spare != spare_arenas.end()) {
                na = (unsigned char*)spare->second;
                spare_arenas.erase(spare);
            }
            // keep a reserve: the runtime allocates kernel scratch and queues from the same memory
            size_t free_b = 0, total_b = 0;
            const bool room = na != nullptr || (hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
                                                free_b > arena_bytes(ncap) + ((size_t)3 << 30));
            if (!room || (na == nullptr && hipMalloc((void**)&na, arena_bytes(ncap) + 256) != hipSuccess)) {
                (void)hipGetLastError();
                if (may_wait) {
                    n_stall = i;  // the rest waits for blocks to come back
                    reqs.resize(i);
                    break;
                }
                return fail(AR_E_NOMEM, "out of device memory while growing a tree arena to " + std::to_string(ncap) +
                                            " nodes");
            }
            if (slot_grown[si.slot]) old_arenas.emplace_back(slot_grown_cap[si.slot], slot_grown[si.slot]);
            slot_grown[si.slot] = na;
            slot_grown_cap[si.slot] = ncap;
            GrowReq r;
            r.slot = si.slot;
            r.cap = ncap;
            r.stats_off = (long long)(na - arena.p);
            r.fwd_off = r.stats_off + (long long)ncap * (long long)sizeof(NodeStats);
            HIP_TRY(hipMemcpyAsync(na, arena.p + si.stats_off, (size_t)si.hi * sizeof(NodeStats), hipMemcpyDeviceToDevice,
                                   stream));
            reqs[i] = r;
        }
        if (n_stall == 0) return AR_OK;
        HIP_TRY(hipMemcpyAsync(grow.p, reqs.data(), sizeof(GrowReq) * n_stall, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_apply_grow<NW>, dim3(grid(n_stall)), dim3(64), 0, stream, slots.p, grow.p, n_stall, bases());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        for (auto& kv : old_arenas) spare_arenas.emplace(kv.first, kv.second);  // the copies are done (sync above)
        grows += n_stall;
        return AR_OK;
    }

    // What the host does after a run of steps: the scan (`c` as scan() fills it), the guard of the tree kernels, and room
    // for the stalled trees. `may_wait`: a tree that cannot grow now may wait while other games are active (c[2]).
    // `secs`, when given, gains the wall time of the scan in [0] and of the rest in [1] (the AR_TIMING line).
    int visit(uint32_t c[4], bool may_wait = false, double* secs = nullptr) {
        const auto t0 = std::chrono::steady_clock::now();
        int rc = scan(c);
        const auto t1 = std::chrono::steady_clock::now();
        if (rc == AR_OK && c[3] != 0) rc = fail(AR_E_DEVICE, "internal capacity guard tripped in a tree kernel (slot.error != 0)");
        if (rc == AR_OK) rc = handle_stalls(c[1], may_wait && c[2] > 0);
        if (secs) {
            secs[0] += std::chrono::duration<double>(t1 - t0).count();
            secs[1] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        }
        return rc;
    }

    // copies the finished games' headers + positions to pinned host memory and frees their slots
    int drain(uint32_t n_done) {
        if (n_done == 0) return AR_OK;
        hipLaunchKernelGGL(k_pack_done<NW>, dim3(n_done), dim3(128), 0, stream, slots.p, done_list.p, n_done, info.p,
                           staging.p, max_turns, bases());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_info.p, info.p, sizeof(DoneInfo<NW>) * n_done, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(h_staging.p, staging.p, sizeof(PosRec<NW>) * (size_t)n_done * max_turns,
                               hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return AR_OK;
    }
};

std::vector<int8_t> maze_array(const std::vector<uint8_t>& cost) {
    std::vector<int8_t> m(cost.size());
    for (size_t i = 0; i < cost.size(); ++i) m[i] = cost[i] ? (int8_t)cost[i] : (int8_t)-1;
    return m;
}

template <int NW>
void record_from_device(const DoneInfo<NW>& d, const PosRec<NW>* pos, const HostGame& g0,
                        const std::vector<uint8_t>& cost, GameRecordHost& r) {
    const int w = g0.width, hw = g0.width * g0.height;
    r.width = g0.width;
    r.height = g0.height;
    r.max_turns = g0.max_turns;
    r.game_index = d.game_index;
    r.n = d.n_pos;
    r.maze = maze_array(cost);
    r.initial_cheese = g0.cheese;
    r.cheese_available = g0.total_cheese;
    r.final_p1 = d.final_st.s1;
    r.final_p2 = d.final_st.s2;
    r.result = r.final_p1 > r.final_p2 ? 1 : r.final_p2 > r.final_p1 ? 2 : 0;
    r.sims = d.t_sims;
    r.nn = d.t_nn;
    r.term = d.t_term;
    r.coll = d.t_coll;
    const size_t n = r.n;
    r.resize(n, hw);
    r.v1.resize(n);
    r.v2.resize(n);
    r.vc1.resize(n * 5);
    r.vc2.resize(n * 5);
    r.pr1.resize(n * 5);
    r.pr2.resize(n * 5);
    r.po1.resize(n * 5);
    r.po2.resize(n * 5);
    for (size_t i = 0; i < n; ++i) {
        const PosRec<NW>& p = pos[i];
        r.set(i, p.st, p.a1, p.a2, w, hw);
        r.v1[i] = p.res.value[0];
        r.v2[i] = p.res.value[1];
        memcpy(&r.vc1[i * 5], p.res.visit_counts[0], 20);
        memcpy(&r.vc2[i * 5], p.res.visit_counts[1], 20);
        memcpy(&r.pr1[i * 5], p.res.prior[0], 20);
        memcpy(&r.pr2[i * 5], p.res.prior[1], 20);
        memcpy(&r.po1[i * 5], p.res.policy[0], 20);
        memcpy(&r.po2[i * 5], p.res.policy[1], 20);
    }
    // selfplay.rs:415-471 compute_cheese_outcomes: the rule is dev_rows.h rows_cell_outcome, which an attached row set runs on
    // the device for the same records
    r.cheese_outcomes.resize(hw);
    for (int c = 0; c < hw; ++c) r.cheese_outcomes[c] = rows_cell_outcome<NW>(pos, (uint32_t)n, d.final_st, c);
}

std::string uuid4() {
    static std::mutex m;
    static std::mt19937_64 gen{std::random_device{}()};
    std::lock_guard<std::mutex> lk(m);
    uint64_t a = gen(), b = gen();
    a = (a & 0xFFFFFFFFFFFF0FFFULL) | 0x0000000000004000ULL;
    b = (b & 0x3FFFFFFFFFFFFFFFULL) | 0x8000000000000000ULL;
    char buf[40];
    snprintf(buf, sizeof buf, "%08x-%04x-%04x-%04x-%012llx", (uint32_t)(a >> 32), (uint32_t)((a >> 16) & 0xFFFF),
             (uint32_t)(a & 0xFFFF), (uint32_t)(b >> 48), (unsigned long long)(b & 0xFFFFFFFFFFFFULL));
    return buf;
}

// writer thread: recording.rs:170-224 BundleWriter behind an unbounded queue (selfplay.rs:742-757)
struct BundleSink {
    std::string dir;
    uint32_t max_games = 32;
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::shared_ptr<GameRecordHost>> q;
    bool closed = false;
    std::string error;
    std::thread th;
    std::vector<std::shared_ptr<GameRecordHost>> buf;
    std::vector<std::string> paths;

    void start() {
        th = std::thread([this]() {
            for (;;) {
                std::shared_ptr<GameRecordHost> g;
                {
                    std::unique_lock<std::mutex> lk(m);
                    cv.wait(lk, [this] { return closed || !q.empty(); });
                    if (q.empty()) break;
                    g = q.front();
                    q.pop_front();
                }
                buf.push_back(g);
                if (buf.size() >= max_games) flush();
            }
            flush();
        });
    }
    void flush() {
        if (buf.empty() || !error.empty()) {
            buf.clear();
            return;
        }
        std::vector<ArGameRecordView> views;
        for (auto& g : buf) views.push_back(g->view());
        std::string path = dir + "/bundle_" + uuid4() + ".npz", err;
        if (!write_bundle(views.data(), (uint32_t)views.size(), path, err)) error = err;
        else paths.push_back(path);
        buf.clear();
    }
    void push(std::shared_ptr<GameRecordHost> g) {
        {
            std::lock_guard<std::mutex> lk(m);
            q.push_back(std::move(g));
        }
        cv.notify_one();
    }
    void finish() {
        {
            std::lock_guard<std::mutex> lk(m);
            closed = true;
        }
        cv.notify_one();
        if (th.joinable()) th.join();
    }
};

int parse_device(const char* device, int device_index, int& out) {
    std::string d = device ? device : "auto";
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(AR_E_DEVICE, "no HIP device visible: libalpharat_hip has no CPU path");
    if (d == "auto" || d == "hip" || d == "mi355x" || d == "cuda" || d == "rocm") out = device_index;
    else if (d.rfind("hip:", 0) == 0) out = atoi(d.c_str() + 4);
    else return fail(AR_E_INVALID, "device '" + d + "' is not available in the HIP sampler (use auto | hip | hip:N)");
    if (out < 0 || out >= n) return fail(AR_E_INVALID, "device index " + std::to_string(out) + " out of range");
    return AR_OK;
}

// ------------------------------------------------------------------------------------------------
// row set: finished games kept on the device until their training rows are built (dev_rows.h)
// ------------------------------------------------------------------------------------------------
// Position records as the engine leaves them, one RowGame header per game, the game's maze bytes and its cheese outcomes,
// and the game of every position. Everything is allocated once at open for `capacity` positions (a game has at least one
// position, so `capacity` games at most); an append that does not fit is refused and changes nothing. The observations are
// not stored: k_rows_build writes them when rows are asked for. Not thread-safe: one caller at a time, as a session.
static std::atomic<uint64_t> g_rows_stamp{1};  // a value per state of a set's mazes that an evaluator may be bound to
struct RowStore {
    int device = 0, nw = 1;
    uint8_t width = 0, height = 0;
    uint32_t hw = 0;
    uint64_t capacity = 0, n_pos = 0;
    bool attached = false;
    DevBuf<uint8_t> recs, mazes, outcomes;  // PosRec<nw>[capacity], [capacity][hw * 4], [capacity][hw]
    DevBuf<uint32_t> pos_game;
    DevBuf<RowGame> games;
    std::vector<RowGame> h_games;
    // attached appends: placements of one drain
    PinBuf<RowPlace> h_place;
    DevBuf<RowPlace> d_place;
    uint32_t place_cap = 0;
    // ar_rows_build: row indices and output rows on the device (kept between calls, grown to the largest request)
    DevBuf<uint64_t> d_rows;
    DevBuf<uint8_t> d_out;
    uint64_t out_rows = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double build_kernel_ms = 0.0;
    hipEvent_t ev_append = nullptr;  // behind the last k_rows_append of an attached session, on its stream
    bool has_append = false;
    // ar_rows_build_device: the order (stored position and perspective of every row of an epoch), replaced as a whole by
    // ar_rows_order_set; ev_batch sits behind the last k_rows_batch, on the caller's stream
    DevBuf<uint64_t> ord_rows;
    DevBuf<uint8_t> ord_swap;
    uint64_t ord_cap = 0, ord_n = 0;
    bool has_order = false;
    hipEvent_t ev_batch = nullptr;
    bool has_batch = false;
    hipError_t wait_batches() const { return has_batch ? hipEventSynchronize(ev_batch) : hipSuccess; }
    // ar_rows_validate: one Board per stored game (the evaluator's `boards`; games only ever append, so the first
    // val_boards_n entries stay right until a clear), and the workspace of one chunk, grown to the largest chunk asked for
    uint64_t stamp = 0;  // changes when the games are forgotten: the same pool and count may then hold other mazes
    DevBuf<Board> val_boards;
    size_t val_boards_n = 0;
    DevBuf<uint64_t> val_rows;
    DevBuf<uint8_t> val_req;
    DevBuf<EvalOut> val_out;
    DevBuf<float> val_logits;
    DevBuf<ValAcc> val_partial, val_total;
    uint32_t val_chunk = 0;
    // ar_rows_validate_lv: the trunk output of a chunk ([chunk][H]), its rows' ownership terms and, when the caller asks
    // for them, the head's logits ([chunk][hw][4]); grown like the workspace above
    DevBuf<float> own_feat, own_value, own_logits;
    DevBuf<double> own_ce;
    DevBuf<uint32_t> own_cells;
    DevBuf<OwnAcc> own_total;
    size_t own_feat_n = 0, own_logits_n = 0;
    uint32_t own_chunk = 0;
    // ar_rows_grad_*: the workspace of one training step (train_mlp.h), one allocation grown to the largest request
    DevBuf<uint8_t> train_ws;
    size_t train_ws_bytes = 0;
    // uploads and builds run on the null stream: they wait for the attached session's last append, nothing else
    hipError_t wait_appends() const { return has_append ? hipEventSynchronize(ev_append) : hipSuccess; }

    size_t rec_bytes() const { return nw == 1 ? sizeof(PosRec<1>) : sizeof(PosRec<4>); }
    ~RowStore() {
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
        if (ev_append) hipEventDestroy(ev_append);
        if (ev_batch) hipEventDestroy(ev_batch);
    }
    int open(uint8_t w, uint8_t h, uint64_t cap, int dev) {
        device = dev;
        width = w;
        height = h;
        hw = (uint32_t)w * h;
        nw = hw <= 64 ? 1 : 4;
        capacity = cap;
        stamp = g_rows_stamp++;
        HIP_TRY(hipSetDevice(device));
        if (recs.alloc(cap * rec_bytes()) != hipSuccess || pos_game.alloc(cap) != hipSuccess || games.alloc(cap) != hipSuccess ||
            mazes.alloc(cap * hw * 4) != hipSuccess || outcomes.alloc(cap * hw) != hipSuccess) {
            (void)hipGetLastError();
            return fail(AR_E_NOMEM, "not enough device memory for a row set of " + std::to_string(cap) + " positions");
        }
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventCreateWithFlags(&ev_append, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_batch, hipEventDisableTiming));
        return AR_OK;
    }
    bool fits(uint64_t positions, uint64_t n_games) const {
        return n_pos + positions <= capacity && h_games.size() + n_games <= capacity;
    }
};

// one host record as the engine's position records (the fields a row is built from, and the search results beside them)
template <int NW>
void rows_records_from_view(const ArGameRecordView& v, PosRec<NW>* out) {
    const uint32_t hw = (uint32_t)v.width * v.height;
    for (uint32_t i = 0; i < v.n_positions; ++i) {
        PosRec<NW>& p = out[i];
        memset(&p, 0, sizeof p);
        const uint8_t* mask = v.cheese_mask + (size_t)i * hw;
        for (uint32_t c = 0; c < hw; ++c)
            if (mask[c]) {
                p.st.cheese[c >> 6] |= 1ULL << (c & 63u);
                p.st.remaining += 1;
            }
        p.st.s1 = v.p1_score[i];
        p.st.s2 = v.p2_score[i];
        p.st.turn = v.turn[i];
        p.st.p1 = (uint8_t)(v.p1_pos[i * 2 + 1] * v.width + v.p1_pos[i * 2]);
        p.st.p2 = (uint8_t)(v.p2_pos[i * 2 + 1] * v.width + v.p2_pos[i * 2]);
        p.st.m1 = v.p1_mud[i];
        p.st.m2 = v.p2_mud[i];
        memcpy(p.res.policy[0], v.policy_p1 + (size_t)i * 5, 20);
        memcpy(p.res.policy[1], v.policy_p2 + (size_t)i * 5, 20);
        if (v.value_p1) p.res.value[0] = v.value_p1[i];
        if (v.value_p2) p.res.value[1] = v.value_p2[i];
        if (v.visit_counts_p1) memcpy(p.res.visit_counts[0], v.visit_counts_p1 + (size_t)i * 5, 20);
        if (v.visit_counts_p2) memcpy(p.res.visit_counts[1], v.visit_counts_p2 + (size_t)i * 5, 20);
        if (v.prior_p1) memcpy(p.res.prior[0], v.prior_p1 + (size_t)i * 5, 20);
        if (v.prior_p2) memcpy(p.res.prior[1], v.prior_p2 + (size_t)i * 5, 20);
        p.a1 = v.action_p1[i];
        p.a2 = v.action_p2[i];
    }
}

// ar_rows_add_games: host records (bundles read back, or a sink's) go to the tail of the store with plain copies; the
// games' cheese outcomes are the view's
template <int NW>
int rows_add_games(RowStore& R, const ArGameRecordView* gs, uint32_t n) {
    uint64_t positions = 0, n_games = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const ArGameRecordView& v = gs[k];
        if (v.width != R.width || v.height != R.height)
            return fail(AR_E_INVALID, "the row set holds " + std::to_string(R.width) + "x" + std::to_string(R.height) +
                                          " games, this one is " + std::to_string(v.width) + "x" + std::to_string(v.height));
        if (v.n_positions == 0) continue;
        if (!v.maze || !v.cheese_outcomes || !v.cheese_mask || !v.p1_pos || !v.p2_pos || !v.p1_score || !v.p2_score ||
            !v.p1_mud || !v.p2_mud || !v.turn || !v.policy_p1 || !v.policy_p2 || !v.action_p1 || !v.action_p2)
            return fail(AR_E_INVALID, "a game record lacks an array the rows are built from");
        positions += v.n_positions;
        n_games += 1;
    }
    if (!R.fits(positions, n_games))
        return fail(AR_E_NOMEM, "the row set is full: " + std::to_string(R.n_pos) + " + " + std::to_string(positions) +
                                    " positions, capacity " + std::to_string(R.capacity));
    if (positions == 0) return AR_OK;
    const uint32_t hw = R.hw;
    std::vector<PosRec<NW>> recs(positions);
    std::vector<uint32_t> pos_game(positions);
    std::vector<RowGame> hdr;
    std::vector<uint8_t> mazes(n_games * hw * 4), outcomes(n_games * hw);
    uint64_t at = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const ArGameRecordView& v = gs[k];
        if (v.n_positions == 0) continue;
        const size_t j = hdr.size();
        rows_records_from_view<NW>(v, recs.data() + at);
        for (uint32_t i = 0; i < v.n_positions; ++i) pos_game[at + i] = (uint32_t)(R.h_games.size() + j);
        for (uint32_t b = 0; b < hw * 4; ++b) mazes[j * hw * 4 + b] = v.maze[b] > 0 ? (uint8_t)v.maze[b] : (uint8_t)0;
        memcpy(&outcomes[j * hw], v.cheese_outcomes, hw);
        RowGame g;
        g.width = v.width;
        g.height = v.height;
        g.max_turns = v.max_turns;
        g.pad = 0;
        g.final1 = v.final_p1_score;
        g.final2 = v.final_p2_score;
        g.game_index = v.game_index;
        g.n_rows = v.n_positions;
        g.first_row = R.n_pos + at;
        hdr.push_back(g);
        at += v.n_positions;
    }
    HIP_TRY(hipSetDevice(R.device));
    HIP_TRY(R.wait_appends());
    const size_t g0 = R.h_games.size();
    HIP_TRY(hipMemcpy(R.recs.p + R.n_pos * sizeof(PosRec<NW>), recs.data(), positions * sizeof(PosRec<NW>), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(R.pos_game.p + R.n_pos, pos_game.data(), positions * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(R.games.p + g0, hdr.data(), hdr.size() * sizeof(RowGame), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(R.mazes.p + g0 * hw * 4, mazes.data(), mazes.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(R.outcomes.p + g0 * hw, outcomes.data(), outcomes.size(), hipMemcpyHostToDevice));
    R.h_games.insert(R.h_games.end(), hdr.begin(), hdr.end());
    R.n_pos += positions;
    return AR_OK;
}

// the drained games of an attached session, in the order of the drain: k_rows_append on the engine's stream, behind
// k_pack_done and in front of whatever overwrites the staging buffers next
template <int NW>
int rows_append_done(RowStore& R, const DoneInfo<NW>* h_info, const DoneInfo<NW>* d_info, const PosRec<NW>* staging,
                     uint32_t n_done, uint32_t max_turns, const Slot<NW>* slots, const uint8_t* maze_pool, hipStream_t stream) {
    uint64_t positions = 0;
    uint32_t n_place = 0;
    if (n_done > R.place_cap) return fail(AR_E_INVALID, "more games drained than the session has slots");
    for (uint32_t d = 0; d < n_done; ++d) {
        const uint32_t n = h_info[d].n_pos < max_turns ? h_info[d].n_pos : max_turns;
        if (n == 0) continue;
        RowPlace& pl = R.h_place.p[n_place];
        pl.first_row = R.n_pos + positions;
        pl.game = (uint32_t)R.h_games.size() + n_place;
        pl.n_rows = n;
        pl.d = d;
        pl.pad = 0;
        positions += n;
        n_place += 1;
    }
    if (!R.fits(positions, n_place))
        return fail(AR_E_NOMEM, "the attached row set is full: " + std::to_string(R.n_pos) + " + " + std::to_string(positions) +
                                    " positions, capacity " + std::to_string(R.capacity));
    if (n_place == 0) return AR_OK;
    HIP_TRY(hipMemcpyAsync(R.d_place.p, R.h_place.p, sizeof(RowPlace) * n_place, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_rows_append<NW>, dim3(n_place), dim3(128), 0, stream, d_info, staging, max_turns, slots, maze_pool,
                       (const RowPlace*)R.d_place.p, n_place, (PosRec<NW>*)R.recs.p, R.pos_game.p, R.games.p, R.mazes.p,
                       R.outcomes.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(R.ev_append, stream));
    R.has_append = true;
    for (uint32_t j = 0; j < n_place; ++j) {
        const RowPlace& pl = R.h_place.p[j];
        const DoneInfo<NW>& di = h_info[pl.d];
        RowGame g;
        g.width = R.width;
        g.height = R.height;
        g.max_turns = (uint16_t)max_turns;
        g.pad = 0;
        g.final1 = di.final_st.s1;
        g.final2 = di.final_st.s2;
        g.game_index = di.game_index;
        g.n_rows = pl.n_rows;
        g.first_row = pl.first_row;
        R.h_games.push_back(g);
    }
    R.n_pos += positions;
    // the placements are read by the copy above when the stream gets there: the pinned buffer is written again only after
    // the next drain, which waits for the stream
    return AR_OK;
}

template <int NW>
int rows_build(RowStore& R, const uint64_t* rows, uint64_t n, const ArTrainRows& o) {
    for (uint64_t i = 0; i < n; ++i)
        if (rows[i] >= R.n_pos)
            return fail(AR_E_INVALID, "row " + std::to_string(i) + " asks for position " + std::to_string(rows[i]) +
                                          ", the set holds " + std::to_string(R.n_pos));
    R.build_kernel_ms = 0.0;
    if (n == 0) return AR_OK;
    HIP_TRY(hipSetDevice(R.device));
    HIP_TRY(R.wait_appends());
    const size_t hw = R.hw, obs = rows_obs_dim(R.hw);
    // the eight arrays behind each other in one allocation, the float arrays first (4-byte aligned)
    const size_t off_obs = 0, off_p1 = off_obs + n * obs * 4, off_p2 = off_p1 + n * 20, off_v1 = off_p2 + n * 20,
                 off_v2 = off_v1 + n * 4, off_a1 = off_v2 + n * 4, off_a2 = off_a1 + n, off_co = off_a2 + n,
                 total = off_co + n * hw;
    if (n > R.out_rows) {
        if (R.d_rows.p) HIP_TRY(hipFree(R.d_rows.p));
        if (R.d_out.p) HIP_TRY(hipFree(R.d_out.p));
        R.d_rows.p = nullptr;
        R.d_out.p = nullptr;
        R.out_rows = 0;
        if (R.d_rows.alloc(n) != hipSuccess || R.d_out.alloc(total) != hipSuccess) {
            (void)hipGetLastError();
            return fail(AR_E_NOMEM, "not enough device memory for " + std::to_string(n) + " output rows");
        }
        R.out_rows = n;
    }
    uint8_t* base = R.d_out.p;
    RowOut out;
    out.observation = (float*)(base + off_obs);
    out.policy_p1 = (float*)(base + off_p1);
    out.policy_p2 = (float*)(base + off_p2);
    out.value_p1 = (float*)(base + off_v1);
    out.value_p2 = (float*)(base + off_v2);
    out.action_p1 = (int8_t*)(base + off_a1);
    out.action_p2 = (int8_t*)(base + off_a2);
    out.cheese_outcomes = (int8_t*)(base + off_co);
    HIP_TRY(hipMemcpy(R.d_rows.p, rows, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipEventRecord(R.ev0, nullptr));
    for (uint64_t row0 = 0; row0 < n; row0 += ROWS_PER_LAUNCH) {
        const uint32_t cnt = (uint32_t)(n - row0 < (uint64_t)ROWS_PER_LAUNCH ? n - row0 : (uint64_t)ROWS_PER_LAUNCH);
        hipLaunchKernelGGL(k_rows_build<NW>, dim3((cnt + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), dim3(ROWS_PER_BLOCK * ROWS_LANES), 0,
                           nullptr, (const PosRec<NW>*)R.recs.p, (const uint32_t*)R.pos_game.p, (const RowGame*)R.games.p,
                           (const uint8_t*)R.mazes.p, (const uint8_t*)R.outcomes.p, (const uint64_t*)R.d_rows.p, row0, cnt, out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(R.ev1, nullptr));
    HIP_TRY(hipEventSynchronize(R.ev1));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, R.ev0, R.ev1));
    R.build_kernel_ms = ms;
    HIP_TRY(hipMemcpy(o.observation, out.observation, n * obs * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(o.policy_p1, out.policy_p1, n * 20, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(o.policy_p2, out.policy_p2, n * 20, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(o.value_p1, out.value_p1, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(o.value_p2, out.value_p2, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(o.action_p1, out.action_p1, n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(o.action_p2, out.action_p2, n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(o.cheese_outcomes, out.cheese_outcomes, n * hw, hipMemcpyDeviceToHost));
    return AR_OK;
}

// ar_rows_order_set: the order is checked on the host, then replaces the old one on the device. Nothing may still read the
// old one: the appends of an attached session and the last stream a batch was launched on are waited for first.
int rows_order_set(RowStore& R, const uint64_t* rows, const uint8_t* swap, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (rows[i] >= R.n_pos)
            return fail(AR_E_INVALID, "order entry " + std::to_string(i) + " asks for position " + std::to_string(rows[i]) +
                                          ", the set holds " + std::to_string(R.n_pos));
    HIP_TRY(hipSetDevice(R.device));
    HIP_TRY(R.wait_appends());
    HIP_TRY(R.wait_batches());
    if (n > R.ord_cap) {
        DevBuf<uint64_t> nr;
        DevBuf<uint8_t> ns;
        if (nr.alloc(n) != hipSuccess || ns.alloc(n) != hipSuccess) {
            (void)hipGetLastError();
            return fail(AR_E_NOMEM, "not enough device memory for an order of " + std::to_string(n) + " rows");
        }
        std::swap(R.ord_rows.p, nr.p);  // (the old buffers are freed with nr and ns)
        std::swap(R.ord_swap.p, ns.p);
        R.ord_cap = n;
    }
    R.has_order = false;
    if (n) {
        HIP_TRY(hipMemcpy(R.ord_rows.p, rows, n * 8, hipMemcpyHostToDevice));
        if (swap)
            HIP_TRY(hipMemcpy(R.ord_swap.p, swap, n, hipMemcpyHostToDevice));
        else
            HIP_TRY(hipMemset(R.ord_swap.p, 0, n));
        HIP_TRY(hipStreamSynchronize(nullptr));  // the batches run on other streams: the order is complete before any is launched
    }
    R.ord_n = n;
    R.has_order = true;
    return AR_OK;
}

// an output array of ar_rows_build_device: device memory of the set's device
int rows_check_device_ptr(const RowStore& R, const void* p, size_t align, const char* what) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(AR_E_INVALID, std::string(what) + " is not device memory");
    }
    if (a.type != hipMemoryTypeDevice || a.device != R.device)
        return fail(AR_E_INVALID, std::string(what) + " is not device memory of device " + std::to_string(R.device));
    if ((uintptr_t)p % align) return fail(AR_E_INVALID, std::string(what) + " is not aligned to " + std::to_string(align) + " bytes");
    return AR_OK;
}

// ar_rows_build_device: rows first .. first + n of the order into the caller's device arrays, on the caller's stream. It
// only launches: no synchronisation, no copy, no allocation.
template <int NW>
int rows_build_device(RowStore& R, uint64_t first, uint64_t n, const ArTrainRows& o, hipStream_t stream) {
    if (!R.has_order) return fail(AR_E_INVALID, "the row set has no order: ar_rows_order_set comes first");
    if (first > R.ord_n || n > R.ord_n - first)
        return fail(AR_E_INVALID, "rows " + std::to_string(first) + " + " + std::to_string(n) + " go beyond the order of " +
                                      std::to_string(R.ord_n));
    if (n == 0) return AR_OK;
    const struct { const void* p; size_t align; const char* what; } arrays[8] = {
        {o.observation, 4, "observation"}, {o.policy_p1, 4, "policy_p1"}, {o.policy_p2, 4, "policy_p2"},
        {o.value_p1, 4, "value_p1"},       {o.value_p2, 4, "value_p2"},   {o.action_p1, 1, "action_p1"},
        {o.action_p2, 1, "action_p2"},     {o.cheese_outcomes, 1, "cheese_outcomes"}};
    for (const auto& a : arrays)
        if (int rc = rows_check_device_ptr(R, a.p, a.align, a.what)) return rc;
    int before = 0;
    HIP_TRY(hipGetDevice(&before));  // the caller's framework keeps its own current device
    if (before != R.device) HIP_TRY(hipSetDevice(R.device));
    RowOut out;
    out.observation = o.observation;
    out.policy_p1 = o.policy_p1;
    out.policy_p2 = o.policy_p2;
    out.value_p1 = o.value_p1;
    out.value_p2 = o.value_p2;
    out.action_p1 = o.action_p1;
    out.action_p2 = o.action_p2;
    out.cheese_outcomes = o.cheese_outcomes;
    hipError_t err = hipSuccess;
    for (uint64_t row0 = 0; row0 < n && err == hipSuccess; row0 += ROWS_PER_LAUNCH) {
        const uint32_t cnt = (uint32_t)(n - row0 < (uint64_t)ROWS_PER_LAUNCH ? n - row0 : (uint64_t)ROWS_PER_LAUNCH);
        hipLaunchKernelGGL(k_rows_batch<NW>, dim3((cnt + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), dim3(ROWS_PER_BLOCK * ROWS_LANES), 0,
                           stream, (const PosRec<NW>*)R.recs.p, (const uint32_t*)R.pos_game.p, (const RowGame*)R.games.p,
                           (const uint8_t*)R.mazes.p, (const uint8_t*)R.outcomes.p, (const uint64_t*)R.ord_rows.p,
                           (const uint8_t*)R.ord_swap.p, first, row0, cnt, out);
        err = hipGetLastError();
    }
    if (err == hipSuccess) {
        err = hipEventRecord(R.ev_batch, stream);
        R.has_batch = true;
    }
    if (before != R.device) (void)hipSetDevice(before);
    HIP_TRY(err);
    return AR_OK;
}

// free and allocate again (DevBuf::alloc on its own would leak the old block)
template <typename T>
static hipError_t regrow(DevBuf<T>& b, size_t count) {
    if (b.p) {
        const hipError_t e = hipFree(b.p);
        b.p = nullptr;
        b.n = 0;
        if (e != hipSuccess) return e;
    }
    return b.alloc(count);
}

// What the training steps of a row set share (ar_rows_grad_mlp, ar_rows_grad_symmetric, ar_rows_grad_local_value): the
// refusals, the workspace, the stream rule and the launches that the chains are made of. One rule for the workspace and
// the stream, stated here only: a set has one workspace, grown to the largest request; a step waits on ev_batch before it touches it, so a step on
// another stream starts behind the last one; growth first waits for the pending batches, which may still use the old
// block; and ev_batch is recorded behind the step's last launch, so whatever waits for pending batches waits for a
// pending step too. Everything is checked before the first launch; a step then only launches, and allocates only to grow.
// `err` is sticky: after the first failure every member returns without launching, and end() reports it.
static const char* const kMlpTensorNames[14] = {"trunk0_w", "trunk0_b", "bn1_w",  "bn1_b",  "trunk4_w", "trunk4_b", "bn2_w",
                                                "bn2_b",    "p1_w",     "p1_b",   "p2_w",   "p2_b",     "value_w",  "value_b"};
static const char* const kSymTensorNames[20] = {"se0_w",    "se0_b",    "se1_w",  "se1_b",  "pe0_w",    "pe0_b",    "pe1_w",
                                                "pe1_b",    "trunk0_w", "trunk0_b", "bn1_w", "bn1_b",    "trunk4_w", "trunk4_b",
                                                "bn2_w",    "bn2_b",    "policy_w", "policy_b", "value_w", "value_b"};
static const char* const kLvTensorNames[18] = {"trunk0_w", "trunk0_b", "bn1_w", "bn1_b", "trunk4_w", "trunk4_b", "bn2_w", "bn2_b", "p1_w",
                                               "p1_b",     "p2_w",     "p2_b",  "value_w", "value_b", "own0_w",  "own0_b", "own2_w",
                                               "own2_b"};
struct TrainStep {
    RowStore& R;
    hipStream_t stream;
    int n = 0, H = 0, head_blocks = 0;
    TrainCols tc{};
    size_t total = 0;     // bytes of workspace taken so far
    size_t o_rows[8]{};   // the row targets: x, t1, t2, y1, y2, a1, a2, co
    size_t o_lpart = 0, o_loss = 0;
    uint8_t* ws = nullptr;
    float *wpart = nullptr, *bpart = nullptr;  // grad_w's partial products and column sums: the driver sizes and sets them
    RowOut ro{};
    hipError_t err = hipSuccess;
    int before = 0;  // the caller's framework keeps its own current device
    // dropout (dev_dropout.h): off unless check_dropout saw a p above 0
    bool dropping = false;
    float drop_p = 0.0f;
    uint64_t drop_seed = 0, drop_step = 0;

    // the dropout's refusal, before any launch; NULL or p == 0: the step without dropout, launch for launch
    int check_dropout(const ArTrainDropout* dr) {
        if (!dr) return AR_OK;
        if (!(dr->p >= 0.0f) || !(dr->p < 1.0f))  // (NaN fails both)
            return fail(AR_E_INVALID, "dropout p must be in [0, 1) (got " + std::to_string(dr->p) + ")");
        dropping = dr->p > 0.0f;
        drop_p = dr->p;
        drop_seed = dr->seed;
        drop_step = dr->step;
        return AR_OK;
    }
    // (key, thr, scale) of the dropout behind BatchNorm call `call`, formed once per call on the host; without dropout
    // nothing is hashed: keep everything at scale 1, which no kernel of that path reads
    TrainDrop drop_of(int call) const {
        TrainDrop d{0, 0, 1.0f};
        if (!dropping) return d;
        d.key = dropout_key(drop_seed, drop_step, (uint64_t)call);
        d.thr = dropout_thr(drop_p);
        d.scale = dropout_scale(drop_p);
        return d;
    }

    // the refusals; `params`, `grads`: `count` pointers named by `names`; `running`: n_running pointers (0: none given)
    int check(uint64_t first, uint64_t n64, uint32_t H_, const char* const* names, float* const* params, float* const* grads,
              int count, float* const* running, int n_running, const ArTrainOut* out) {
        if (!R.has_order) return fail(AR_E_INVALID, "the row set has no order: ar_rows_order_set comes first");
        if (first > R.ord_n || n64 > R.ord_n - first)
            return fail(AR_E_INVALID, "rows " + std::to_string(first) + " + " + std::to_string(n64) + " go beyond the order of " +
                                          std::to_string(R.ord_n));
        if (n64 < 2) return fail(AR_E_INVALID, "a training BatchNorm needs at least two rows");
        if (n64 > (uint64_t)TRAIN_MAX_ROWS) return fail(AR_E_INVALID, "at most 65536 rows a step");
        if (H_ == 0 || H_ % 32 != 0 || H_ > 256)
            return fail(AR_E_INVALID, "hidden_dim must be a multiple of 32, at most 256 (got " + std::to_string(H_) + ")");
        for (int i = 0; i < count; ++i) {
            if (!params[i] || !grads[i]) return fail(AR_E_INVALID, std::string("null tensor: ") + names[i]);
            if (int rc = rows_check_device_ptr(R, params[i], 4, names[i])) return rc;
            if (int rc = rows_check_device_ptr(R, grads[i], 4, names[i])) return rc;
        }
        for (int i = 0; i < n_running; ++i) {
            if (!running[i]) return fail(AR_E_INVALID, "null running statistic");
            if (int rc = rows_check_device_ptr(R, running[i], 4, "running statistic")) return rc;
        }
        if (out) {
            float* const os[5] = {out->losses, out->logits_p1, out->logits_p2, out->value_p1, out->value_p2};
            for (float* q : os)
                if (q)
                    if (int rc = rows_check_device_ptr(R, q, 4, "output")) return rc;
        }
        n = (int)n64;
        H = (int)H_;
        tc = train_cols(n, H);
        head_blocks = (n + TRAIN_HEAD_ROWS - 1) / TRAIN_HEAD_ROWS;
        return AR_OK;
    }

    // the workspace: offsets into one allocation, every array 256-byte aligned
    size_t take(size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    }
    void take_rows() {
        const size_t N = (size_t)n, bytes[8] = {N * rows_obs_dim(R.hw) * 4, N * 20, N * 20, N * 4, N * 4, N, N, N * R.hw};
        for (int i = 0; i < 8; ++i) o_rows[i] = take(bytes[i]);
    }
    void take_losses() {
        o_lpart = take((size_t)head_blocks * 32);
        o_loss = take(6 * 4);
    }
    float* f(size_t at) const { return (float*)(ws + at); }
    double* d(size_t at) const { return (double*)(ws + at); }

    // the set's device current, `total` bytes of workspace behind `ws`, the stream behind the last batch or step
    int begin() {
        HIP_TRY(hipGetDevice(&before));
        if (before != R.device) HIP_TRY(hipSetDevice(R.device));
        if (total > R.train_ws_bytes) {
            hipError_t e = R.wait_batches();
            if (e == hipSuccess) e = regrow(R.train_ws, total);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                R.train_ws_bytes = 0;
                if (before != R.device) (void)hipSetDevice(before);
                return fail(AR_E_NOMEM, "not enough device memory for a training workspace of " + std::to_string(total) + " bytes");
            }
            R.train_ws_bytes = total;
        }
        ws = R.train_ws.p;
        if (R.has_batch) err = hipStreamWaitEvent(stream, R.ev_batch, 0);
        return AR_OK;
    }
    bool ok() const { return err == hipSuccess; }
    void launched() {
        if (err == hipSuccess) err = hipGetLastError();
    }
    int end() {
        if (err == hipSuccess) {
            err = hipEventRecord(R.ev_batch, stream);
            R.has_batch = true;
        }
        if (before != R.device) (void)hipSetDevice(before);
        HIP_TRY(err);
        return AR_OK;
    }
    static dim3 blocks(size_t count) { return dim3((unsigned)((count + 255) / 256)); }
    dim3 cgrid() const { return dim3((H + 63) / 64, tc.P); }

    // X and the targets of the window, by the row routine the batches use
    template <int NW>
    void rows(uint64_t first) {
        ro.observation = f(o_rows[0]);
        ro.policy_p1 = f(o_rows[1]);
        ro.policy_p2 = f(o_rows[2]);
        ro.value_p1 = f(o_rows[3]);
        ro.value_p2 = f(o_rows[4]);
        ro.action_p1 = (int8_t*)(ws + o_rows[5]);
        ro.action_p2 = (int8_t*)(ws + o_rows[6]);
        ro.cheese_outcomes = (int8_t*)(ws + o_rows[7]);
        if (err != hipSuccess) return;
        hipLaunchKernelGGL(k_rows_batch<NW>, dim3((n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), dim3(ROWS_PER_BLOCK * ROWS_LANES), 0,
                           stream, (const PosRec<NW>*)R.recs.p, (const uint32_t*)R.pos_game.p, (const RowGame*)R.games.p,
                           (const uint8_t*)R.mazes.p, (const uint8_t*)R.outcomes.p, (const uint64_t*)R.ord_rows.p,
                           (const uint8_t*)R.ord_swap.p, first, (uint64_t)0, (uint32_t)n, ro);
        launched();
    }
    // C[M][N] = sum_k A(m, k) B(k, n)
    void gemm(const float* a, long sam, long sak, int a_kfast, const float* b, long sbk, long sbn, int b_kfast, float* c, int M,
              int N, int K, const float* bias, int splits, int k_per_split, float* colsum) {
        if (err != hipSuccess) return;
        TrainGemm t;
        t.a = a;
        t.b = b;
        t.bias = bias;
        t.c = c;
        t.colsum = colsum;
        t.M = M;
        t.N = N;
        t.K = K;
        t.k_per_split = k_per_split;
        t.ldc = N;
        t.sam = sam;
        t.sak = sak;
        t.sbk = sbk;
        t.sbn = sbn;
        t.c_split = (size_t)M * N;
        t.a_kfast = a_kfast;
        t.b_kfast = b_kfast;
        hipLaunchKernelGGL(k_train_gemm, dim3((N + TG_TILE - 1) / TG_TILE, (M + TG_TILE - 1) / TG_TILE, splits), dim3(TG_THREADS), 0,
                           stream, t);
        launched();
    }
    // Z[rows][H] = In[rows][K] W[H][K]^T + b
    void linear(const float* in, int rows, int K, const float* w, const float* b, float* z) {
        gemm(in, K, 1, 1, w, 1, K, 1, z, rows, H, K, b, 1, K, nullptr);
    }
    // dIn[rows][N] = d[rows][K] W[K][N], K = H unless given (the ownership head's last layer has 4 hw outputs)
    void grad_in(const float* d, int rows, const float* w, int N, float* din, int K = 0) {
        if (K == 0) K = H;
        gemm(d, K, 1, 1, w, N, 1, 0, din, rows, N, K, nullptr, 1, K, nullptr);
    }
    // dW[M][N] = d[rows][M]^T In[rows][N] and db = colsum(d): per row range of `sp`, then the ranges added in order into up
    // to three destinations, consecutive segments of dW's rows (the MLP's three heads; one segment otherwise)
    struct Seg {
        float *w, *b;
        int rows;
    };
    void grad_w(const float* d, int M, const float* in, int N, int rows, TrainSplit sp, Seg s0, Seg s1 = {nullptr, nullptr, 0},
                Seg s2 = {nullptr, nullptr, 0}) {
        gemm(d, 1, M, 0, in, N, 1, 0, wpart, M, N, rows, nullptr, sp.S, sp.kps, bpart);
        if (err != hipSuccess) return;
        TrainReduce t;
        t.wpart = wpart;
        t.bpart = bpart;
        t.S = sp.S;
        t.M = M;
        t.N = N;
        t.w[0] = s0.w, t.w[1] = s1.w, t.w[2] = s2.w;
        t.b[0] = s0.b, t.b[1] = s1.b, t.b[2] = s2.b;
        t.rows[0] = s0.rows, t.rows[1] = s1.rows, t.rows[2] = s2.rows;
        hipLaunchKernelGGL(k_train_reduce, blocks((size_t)M * N + M), dim3(256), 0, stream, t);
        launched();
    }
    // act = relu(bn(z)) over n rows at z with the batch's statistics (two passes over z); mu and rstd kept for the backward
    // `dr`: the dropout behind it (null: none)
    void bn_forward(const float* z, const float* gamma, const float* beta, float* act, double* mu, float* rstd, float* run_mean,
                    float* run_var, double* part_sum, double* part_sq, const TrainDrop* dr = nullptr) {
        if (err != hipSuccess) return;
        TrainColArgs a;
        memset(&a, 0, sizeof a);
        a.z = z;
        a.part0 = part_sum;
        hipLaunchKernelGGL(k_train_colsum<TC_SUM>, cgrid(), dim3(256), 0, stream, tc, a);
        a.sum_in = part_sum;
        a.part0 = part_sq;
        hipLaunchKernelGGL(k_train_colsum<TC_SQ>, cgrid(), dim3(256), 0, stream, tc, a);
        if (dr)
            hipLaunchKernelGGL(k_train_bn_apply_drop, cgrid(), dim3(256), 0, stream, tc, z, (const double*)part_sum,
                               (const double*)part_sq, gamma, beta, act, mu, rstd, run_mean, run_var, *dr);
        else
            hipLaunchKernelGGL(k_train_bn_apply, cgrid(), dim3(256), 0, stream, tc, z, (const double*)part_sum,
                               (const double*)part_sq, gamma, beta, act, mu, rstd, run_mean, run_var);
        launched();
    }
    // the backward of one BatchNorm call: a column kernel leaves the masked dy in a.d and its two column sums in a.part0,
    // a.part1 (bn_backward_trunk: from dA already in a.d; a head's own kernel is its driver's), then bn_bwd puts dz there.
    // `dr`: the dropout behind the call's activation (null: none); its scale goes with the arguments.
    static TrainColArgs backward_args(const float* z, const float* act, float* d, const double* mu, const float* rstd,
                                      double* part0, double* part1, const TrainDrop* dr = nullptr) {
        TrainColArgs a;
        memset(&a, 0, sizeof a);
        a.z = z;
        a.act = act;
        a.d = d;
        a.mu = mu;
        a.rstd = rstd;
        a.part0 = part0;
        a.part1 = part1;
        a.scale = dr ? dr->scale : 1.0f;
        return a;
    }
    void bn_bwd(const float* z, float* d, const double* part0, const double* part1, const double* mu, const float* rstd,
                const float* gamma, float* dgamma, float* dbeta) {
        hipLaunchKernelGGL(k_train_bn_bwd, cgrid(), dim3(256), 0, stream, tc, z, d, part0, part1, mu, rstd, gamma, dgamma, dbeta);
        launched();
    }
    void bn_backward_trunk(const TrainColArgs& a, const float* gamma, float* dgamma, float* dbeta) {
        if (err != hipSuccess) return;
        if (dropping) hipLaunchKernelGGL((k_train_colsum<TC_DTRUNK, true>), cgrid(), dim3(256), 0, stream, tc, a);
        else hipLaunchKernelGGL(k_train_colsum<TC_DTRUNK>, cgrid(), dim3(256), 0, stream, tc, a);
        bn_bwd(a.z, a.d, a.part0, a.part1, a.mu, a.rstd, gamma, dgamma, dbeta);
    }
    // the six losses from the heads' partial sums (called behind the driver's heads launch)
    void loss_sum(float pw, float vw, const ArTrainOut* out) {
        hipLaunchKernelGGL(k_train_loss_sum, dim3(1), dim3(256), 0, stream, (const double*)d(o_lpart), (uint32_t)head_blocks,
                           (uint32_t)n, pw, vw, f(o_loss), out ? out->losses : nullptr);
        launched();
    }
};

// What ar_rows_grad_local_value adds to a call of rows_grad_mlp: the eighteen tensors (their first fourteen are the `p` and
// `g` of the call), the third weight and the caller's outputs (the first five of them are the `out` of the call).
struct LvStep {
    const ArLvTensors *p, *g;
    float ow;
    const ArLvTrainOut* out;
};

// ar_rows_grad_mlp: the loss and the gradients of PyRatMLP over rows first .. first + n of the order, on the caller's
// stream: train_mlp.h's chain, under TrainStep's rules. With `lv`, ar_rows_grad_local_value: the same chain issued by the
// same lines, and between them what train_lv.h lists for the ownership head.
template <int NW>
int rows_grad_mlp(RowStore& R, uint64_t first, uint64_t n64, uint32_t H, const ArMlpTensors& p, const ArMlpTensors& g,
                  const ArMlpBnStats* run, float pw, float vw, const ArTrainOut* out, hipStream_t stream,
                  const LvStep* lv = nullptr, const ArTrainDropout* dropout = nullptr) {
    static_assert(sizeof(ArMlpTensors) == 14 * sizeof(float*), "fourteen pointers");
    static_assert(sizeof(ArMlpBnStats) == 4 * sizeof(float*), "four pointers");
    static_assert(sizeof(ArLvTensors) == 18 * sizeof(float*) && offsetof(ArLvTensors, own0_w) == sizeof(ArMlpTensors),
                  "ArMlpTensors' fourteen pointers, then four");
    static_assert(sizeof(ArLvTrainOut) == 6 * sizeof(float*) && offsetof(ArLvTrainOut, ownership_logits) == sizeof(ArTrainOut),
                  "ArTrainOut's five pointers, then one");
    TrainStep T{R, stream};
    if (int rc = lv ? T.check(first, n64, H, kLvTensorNames, (float* const*)lv->p, (float* const*)lv->g, 18, (float* const*)run,
                              run ? 4 : 0, out)
                    : T.check(first, n64, H, kMlpTensorNames, (float* const*)&p, (float* const*)&g, 14, (float* const*)run,
                              run ? 4 : 0, out))
        return rc;
    if (int rc = T.check_dropout(dropout)) return rc;
    if (lv && lv->out && lv->out->ownership_logits)
        if (int rc = rows_check_device_ptr(R, lv->out->ownership_logits, 4, "output")) return rc;
    const int n = T.n, D = (int)rows_obs_dim(R.hw), Hi = T.H, hw4 = 4 * (int)R.hw;
    const LvCells lc = lv_cells(n, (int)R.hw);
    const TrainSplit sp = train_split(n);
    const size_t nH = (size_t)n * H * 4;
    T.take_rows();
    const size_t o_z1 = T.take(nH), o_act1 = T.take(nH), o_z2 = T.take(nH), o_act2 = T.take(nH), o_dout = T.take((size_t)n * 48),
                 o_dz2 = T.take(nH), o_dz1 = T.take(nH), o_parts = T.take((size_t)6 * TRAIN_MAX_PARTS * H * 8),
                 o_mean = T.take((size_t)2 * H * 8), o_rstd = T.take((size_t)2 * H * 4),
                 o_wpart = T.take((size_t)sp.S * H * std::max(D, Hi) * 4),  // (D > 4 hw: dWo2's [S][4 hw][H] fits as well)
                 o_bpart = T.take((size_t)sp.S * (lv ? std::max(Hi, hw4) : Hi) * 4);
    T.take_losses();
    // the ownership head's: Zo, Ao, dAo [n][H], L [n][4 hw], the row parts' counts and ce sums, the seven losses
    size_t o_zo = 0, o_ao = 0, o_dao = 0, o_l = 0, o_cnt = 0, o_ce = 0, o_loss7 = 0;
    if (lv) {
        o_zo = T.take(nH), o_ao = T.take(nH), o_dao = T.take(nH), o_l = T.take((size_t)n * hw4 * 4);
        o_cnt = T.take((size_t)lc.B * 4), o_ce = T.take((size_t)lc.B * 8), o_loss7 = T.take(7 * 4);
    }
    if (int rc = T.begin()) return rc;
    float *Z1 = T.f(o_z1), *A1 = T.f(o_act1), *Z2 = T.f(o_z2), *A2 = T.f(o_act2), *dOut = T.f(o_dout), *dZ2 = T.f(o_dz2),
          *dZ1 = T.f(o_dz1), *rstds = T.f(o_rstd);
    double *parts = T.d(o_parts), *means = T.d(o_mean);
    T.wpart = T.f(o_wpart);
    T.bpart = T.f(o_bpart);
    auto part = [&](int i) { return parts + (size_t)i * TRAIN_MAX_PARTS * H; };
    // z -> relu(bn(z)), layer 0 / 1, which is the BatchNorm call's index for the dropout behind it
    auto bn_forward = [&](int layer, const float* z, const float* gamma, const float* beta, float* act, float* rm, float* rv) {
        const TrainDrop dr = T.drop_of(layer);
        T.bn_forward(z, gamma, beta, act, means + (size_t)layer * H, rstds + (size_t)layer * H, rm, rv, part(2 * layer),
                     part(2 * layer + 1), T.dropping ? &dr : nullptr);
    };
    auto bn_backward = [&](int layer, bool head, const float* z, const float* act, float* d, const float* gamma, float* dgamma,
                           float* dbeta) {
        if (!T.ok()) return;
        const TrainDrop dr = T.drop_of(layer);
        TrainColArgs a = TrainStep::backward_args(z, act, d, means + (size_t)layer * H, rstds + (size_t)layer * H, part(4), part(5),
                                                  T.dropping ? &dr : nullptr);
        a.dout = dOut;
        a.w_p1 = p.p1_w;
        a.w_p2 = p.p2_w;
        a.w_v = p.value_w;
        if (!head) return T.bn_backward_trunk(a, gamma, dgamma, dbeta);
        if (lv && T.dropping) hipLaunchKernelGGL((k_train_colsum<TC_DHEAD_ADD, true>), T.cgrid(), dim3(256), 0, stream, T.tc, a);
        else if (lv) hipLaunchKernelGGL(k_train_colsum<TC_DHEAD_ADD>, T.cgrid(), dim3(256), 0, stream, T.tc, a);  // d holds dZo Wo0
        else if (T.dropping) hipLaunchKernelGGL((k_train_colsum<TC_DHEAD, true>), T.cgrid(), dim3(256), 0, stream, T.tc, a);
        else hipLaunchKernelGGL(k_train_colsum<TC_DHEAD>, T.cgrid(), dim3(256), 0, stream, T.tc, a);
        T.bn_bwd(z, d, part(4), part(5), a.mu, a.rstd, gamma, dgamma, dbeta);
    };
    const float* X = T.f(T.o_rows[0]);
    T.rows<NW>(first);
    // forward
    T.linear(X, n, D, p.trunk0_w, p.trunk0_b, Z1);
    bn_forward(0, Z1, p.bn1_w, p.bn1_b, A1, run ? run->mean1 : nullptr, run ? run->var1 : nullptr);
    T.linear(A1, n, Hi, p.trunk4_w, p.trunk4_b, Z2);
    bn_forward(1, Z2, p.bn2_w, p.bn2_b, A2, run ? run->mean2 : nullptr, run ? run->var2 : nullptr);
    if (T.ok()) {
        TrainHeads t;
        t.act = A2;
        t.w_p1 = p.p1_w, t.b_p1 = p.p1_b, t.w_p2 = p.p2_w, t.b_p2 = p.p2_b, t.w_v = p.value_w, t.b_v = p.value_b;
        t.t1 = T.ro.policy_p1, t.t2 = T.ro.policy_p2, t.y1 = T.ro.value_p1, t.y2 = T.ro.value_p2;
        t.dout = dOut;
        t.loss_part = T.d(T.o_lpart);
        t.logits_p1 = out ? out->logits_p1 : nullptr;
        t.logits_p2 = out ? out->logits_p2 : nullptr;
        t.value_p1 = out ? out->value_p1 : nullptr;
        t.value_p2 = out ? out->value_p2 : nullptr;
        t.n = n;
        t.H = Hi;
        t.pw_n = pw / (float)n;
        t.vw_n = vw / (float)n;
        hipLaunchKernelGGL(k_train_heads, dim3(T.head_blocks), dim3(256), (size_t)12 * H * 4, stream, t);
        if (!lv) T.loss_sum(pw, vw, out);
    }
    float *Zo = nullptr, *Ao = nullptr, *dAo = nullptr, *L = nullptr;
    if (lv) {  // the ownership head's forward, its cells' terms and dL in place of L, the seven losses
        Zo = T.f(o_zo), Ao = T.f(o_ao), dAo = T.f(o_dao), L = T.f(o_l);
        const size_t nH4 = (size_t)n * H / 4;
        T.linear(A2, n, Hi, lv->p->own0_w, lv->p->own0_b, Zo);
        if (T.ok()) {
            hipLaunchKernelGGL(k_train_lv_relu, TrainStep::blocks(nH4), dim3(256), 0, stream, (const float4*)Zo, (float4*)Ao, nH4);
            T.launched();
        }
        T.gemm(Ao, Hi, 1, 1, lv->p->own2_w, 1, Hi, 1, L, n, hw4, Hi, lv->p->own2_b, 1, Hi, nullptr);
        if (T.ok()) {
            uint32_t* cnt = (uint32_t*)(T.ws + o_cnt);
            hipLaunchKernelGGL(k_train_own_count, dim3(lc.B), dim3(256), 0, stream, lc, (const int8_t*)T.ro.cheese_outcomes, cnt);
            T.launched();
            if (T.ok() && lv->out && lv->out->ownership_logits)
                T.err = hipMemcpyAsync(lv->out->ownership_logits, L, (size_t)n * hw4 * 4, hipMemcpyDeviceToDevice, stream);
        }
        if (T.ok()) {
            uint32_t* cnt = (uint32_t*)(T.ws + o_cnt);
            LvOwn a;
            a.l = L;
            a.co = T.ro.cheese_outcomes;
            a.count_part = cnt;
            a.ce_part = T.d(o_ce);
            a.ow = lv->ow;
            hipLaunchKernelGGL(k_train_own_cells, dim3(lc.B), dim3(256), 0, stream, lc, a);
            hipLaunchKernelGGL(k_train_lv_loss_sum, dim3(1), dim3(320), 0, stream, (const double*)T.d(T.o_lpart),
                               (uint32_t)T.head_blocks, (uint32_t)n, (const double*)T.d(o_ce), (const uint32_t*)cnt, (uint32_t)lc.B,
                               pw, vw, lv->ow, T.f(o_loss7), out ? out->losses : nullptr);
            T.launched();
        }
    }
    // backward
    T.grad_w(dOut, 12, A2, Hi, n, sp, {g.p1_w, g.p1_b, 5}, {g.p2_w, g.p2_b, 5}, {g.value_w, g.value_b, 2});
    if (lv) {  // the ownership head's: its four gradients, and dZo Wo0 where the trunk's backward adds the three heads' part
        const size_t nH4 = (size_t)n * H / 4;
        T.grad_w(L, hw4, Ao, Hi, n, sp, {lv->g->own2_w, lv->g->own2_b, hw4});
        T.grad_in(L, n, lv->p->own2_w, Hi, dAo, hw4);
        if (T.ok()) {
            hipLaunchKernelGGL(k_train_lv_relu_bwd, TrainStep::blocks(nH4), dim3(256), 0, stream, (const float4*)Zo, (float4*)dAo, nH4);
            T.launched();
        }
        T.grad_w(dAo, Hi, A2, Hi, n, sp, {lv->g->own0_w, lv->g->own0_b, Hi});
        T.grad_in(dAo, n, lv->p->own0_w, Hi, dZ2);
    }
    bn_backward(1, true, Z2, A2, dZ2, p.bn2_w, g.bn2_w, g.bn2_b);
    T.grad_w(dZ2, Hi, A1, Hi, n, sp, {g.trunk4_w, g.trunk4_b, Hi});
    T.grad_in(dZ2, n, p.trunk4_w, Hi, dZ1);
    bn_backward(0, false, Z1, A1, dZ1, p.bn1_w, g.bn1_w, g.bn1_b);
    T.grad_w(dZ1, Hi, X, D, n, sp, {g.trunk0_w, g.trunk0_b, Hi});
    return T.end();
}

// ar_rows_grad_symmetric: the loss and the gradients of SymmetricMLP over rows first .. first + n of the order, on the
// caller's stream: train_sym.h's chain, under TrainStep's rules. P1's and P2's rows are stacked: an array of [2n] rows holds
// P1's n, then P2's.
template <int NW>
int rows_grad_symmetric(RowStore& R, uint64_t first, uint64_t n64, uint32_t H, const ArSymTensors& p, const ArSymTensors& g,
                        const ArSymBnStats* run, float pw, float vw, const ArTrainOut* out, hipStream_t stream,
                        const ArTrainDropout* dropout = nullptr) {
    static_assert(sizeof(ArSymTensors) == 20 * sizeof(float*), "twenty pointers");
    static_assert(sizeof(ArSymBnStats) == 8 * sizeof(float*), "eight pointers");
    float* const* rs = (float* const*)run;  // se mean, var; pe; trunk.1; trunk.5
    TrainStep T{R, stream};
    if (int rc = T.check(first, n64, H, kSymTensorNames, (float* const*)&p, (float* const*)&g, 20, rs, run ? 8 : 0, out)) return rc;
    if (int rc = T.check_dropout(dropout)) return rc;
    const int n = T.n, n2 = 2 * n, hw = (int)R.hw, Hi = T.H, H2 = 2 * Hi;
    const int Ds = sym_shared_dim(hw), Dp = sym_player_dim(hw);
    // a product is reduced over the n rows of the shared encoder or the 2n of everything else
    const TrainSplit sp1 = train_split(n), sp2 = train_split(n2);
    const size_t nH = (size_t)n * H * 4;
    T.take_rows();
    const size_t o_xs = T.take((size_t)n * Ds * 4), o_xp = T.take((size_t)n2 * Dp * 4), o_zs = T.take(nH), o_as = T.take(nH),
                 o_zp = T.take(2 * nH), o_ap = T.take(2 * nH), o_cat = T.take(4 * nH), o_zt0 = T.take(2 * nH),
                 o_at0 = T.take(2 * nH), o_zt4 = T.take(2 * nH), o_at4 = T.take(2 * nH), o_d12 = T.take((size_t)n2 * 48),
                 o_dt4 = T.take(2 * nH), o_dt0 = T.take(2 * nH), o_dcat = T.take(4 * nH), o_dp = T.take(2 * nH), o_ds = T.take(nH),
                 o_parts = T.take((size_t)6 * TRAIN_MAX_PARTS * H * 8), o_mean = T.take((size_t)7 * H * 8),
                 o_rstd = T.take((size_t)7 * H * 4), o_wpart = T.take((size_t)sp2.S * H * std::max(std::max(Ds, Dp), H2) * 4),
                 o_bpart = T.take((size_t)sp2.S * H * 4);
    T.take_losses();
    const size_t o_bnscr = T.take((size_t)2 * H * 4);
    if (int rc = T.begin()) return rc;
    float *Xs = T.f(o_xs), *Xp = T.f(o_xp), *Zs = T.f(o_zs), *As = T.f(o_as), *Zp = T.f(o_zp), *Ap = T.f(o_ap), *Cat = T.f(o_cat),
          *Zt0 = T.f(o_zt0), *At0 = T.f(o_at0), *Zt4 = T.f(o_zt4), *At4 = T.f(o_at4), *D12 = T.f(o_d12), *dT4 = T.f(o_dt4),
          *dT0 = T.f(o_dt0), *dCat = T.f(o_dcat), *dP = T.f(o_dp), *dS = T.f(o_ds), *rstds = T.f(o_rstd), *bnscr = T.f(o_bnscr);
    double *parts = T.d(o_parts), *means = T.d(o_mean);
    T.wpart = T.f(o_wpart);
    T.bpart = T.f(o_bpart);
    auto part = [&](int i) { return parts + (size_t)i * TRAIN_MAX_PARTS * H; };
    const size_t half = (size_t)n * H;  // P2's rows of a [2n][H] array
    // one BatchNorm call (0: shared; 1, 2: player_encoder.1 of P1, P2; 3, 4: trunk.1; 5, 6: trunk.5) over n rows at z
    auto bn_forward = [&](int call, const float* z, const float* gamma, const float* beta, float* act, float* rm, float* rv) {
        const TrainDrop dr = T.drop_of(call);
        T.bn_forward(z, gamma, beta, act, means + (size_t)call * H, rstds + (size_t)call * H, rm, rv, part(0), part(1),
                     T.dropping ? &dr : nullptr);
    };
    // a module called for both players: P1's call, then P2's on top of it
    auto bn_forward2 = [&](int call, const float* z, const float* gamma, const float* beta, float* act, float* rm, float* rv) {
        bn_forward(call, z, gamma, beta, act, rm, rv);
        bn_forward(call + 1, z + half, gamma, beta, act + half, rm, rv);
    };
    // dz in place of d for one call; its column sums stay in part(2 + 2 * slot), part(3 + 2 * slot)
    auto bn_backward = [&](int call, int slot, bool head, const float* z, const float* act, float* d, const float* d12,
                           const float* gamma, float* dgamma, float* dbeta) {
        if (!T.ok()) return;
        double *p0 = part(2 + 2 * slot), *p1 = part(3 + 2 * slot);
        const double* mu = means + (size_t)call * H;
        const float* rstd = rstds + (size_t)call * H;
        const TrainDrop dr = T.drop_of(call);
        const TrainDrop* drp = T.dropping ? &dr : nullptr;
        if (!head) return T.bn_backward_trunk(TrainStep::backward_args(z, act, d, mu, rstd, p0, p1, drp), gamma, dgamma, dbeta);
        SymDHead a;
        a.z = z;
        a.act = act;
        a.d = d;
        a.d12 = d12;
        a.w_p = p.policy_w;
        a.w_v = p.value_w;
        a.mu = mu;
        a.rstd = rstd;
        a.part0 = p0;
        a.part1 = p1;
        a.scale = drp ? drp->scale : 1.0f;
        if (T.dropping) hipLaunchKernelGGL(k_sym_dhead<true>, T.cgrid(), dim3(256), 0, stream, T.tc, a);
        else hipLaunchKernelGGL(k_sym_dhead<false>, T.cgrid(), dim3(256), 0, stream, T.tc, a);
        T.bn_bwd(z, d, p0, p1, mu, rstd, gamma, dgamma, dbeta);
    };
    // both calls of a shared module; the module's two gradients from both calls' column sums (k_train_bn_bwd's own go to bnscr)
    auto bn_backward2 = [&](int call, bool head, const float* z, const float* act, float* d, const float* gamma, float* dgamma,
                            float* dbeta) {
        bn_backward(call, 0, head, z, act, d, D12, gamma, bnscr, bnscr + H);
        bn_backward(call + 1, 1, head, z + half, act + half, d + half, D12 + (size_t)n * 12, gamma, bnscr, bnscr + H);
        if (!T.ok()) return;
        hipLaunchKernelGGL(k_sym_bn_grad, dim3((H + 255) / 256), dim3(256), 0, stream, T.tc.P, Hi, (const double*)part(2),
                           (const double*)part(3), (const double*)part(4), (const double*)part(5), dgamma, dbeta);
        T.launched();
    };
    auto rstat = [&](int i) { return run ? rs[i] : (float*)nullptr; };
    T.rows<NW>(first);
    if (T.ok()) {
        hipLaunchKernelGGL(k_sym_split, T.blocks((size_t)n * (Ds + 2 * Dp)), dim3(256), 0, stream, (const float*)T.ro.observation, Xs,
                           Xp, n, hw);
        T.launched();
    }
    // forward
    T.linear(Xs, n, Ds, p.se0_w, p.se0_b, Zs);
    bn_forward(0, Zs, p.se1_w, p.se1_b, As, rstat(0), rstat(1));
    T.linear(Xp, n2, Dp, p.pe0_w, p.pe0_b, Zp);
    bn_forward2(1, Zp, p.pe1_w, p.pe1_b, Ap, rstat(2), rstat(3));
    if (T.ok()) {
        hipLaunchKernelGGL(k_sym_cat, T.blocks((size_t)4 * n * H), dim3(256), 0, stream, (const float*)As, (const float*)Ap, Cat, n, Hi);
        T.launched();
    }
    T.linear(Cat, n2, H2, p.trunk0_w, p.trunk0_b, Zt0);
    bn_forward2(3, Zt0, p.bn1_w, p.bn1_b, At0, rstat(4), rstat(5));
    T.linear(At0, n2, Hi, p.trunk4_w, p.trunk4_b, Zt4);
    bn_forward2(5, Zt4, p.bn2_w, p.bn2_b, At4, rstat(6), rstat(7));
    if (T.ok()) {
        SymHeads t;
        t.h = At4;
        t.w_p = p.policy_w, t.b_p = p.policy_b, t.w_v = p.value_w, t.b_v = p.value_b;
        t.t1 = T.ro.policy_p1, t.t2 = T.ro.policy_p2, t.y1 = T.ro.value_p1, t.y2 = T.ro.value_p2;
        t.d12 = D12;
        t.loss_part = T.d(T.o_lpart);
        t.logits_p1 = out ? out->logits_p1 : nullptr;
        t.logits_p2 = out ? out->logits_p2 : nullptr;
        t.value_p1 = out ? out->value_p1 : nullptr;
        t.value_p2 = out ? out->value_p2 : nullptr;
        t.n = n;
        t.H = Hi;
        t.pw_n = pw / (float)n;
        t.vw_n = vw / (float)n;
        hipLaunchKernelGGL(k_sym_heads, dim3(T.head_blocks), dim3(256), (size_t)12 * H * 4, stream, t);
        T.loss_sum(pw, vw, out);
    }
    // backward: the heads
    T.gemm(D12, 1, 12, 0, At4, Hi, 1, 0, T.wpart, 12, Hi, n2, nullptr, sp2.S, sp2.kps, T.bpart);
    if (T.ok()) {
        hipLaunchKernelGGL(k_sym_head_reduce, T.blocks((size_t)12 * H + 6), dim3(256), 0, stream, (const float*)T.wpart,
                           (const float*)T.bpart, sp2.S, Hi, g.policy_w, g.policy_b, g.value_w, g.value_b);
        T.launched();
    }
    // the trunk
    bn_backward2(5, true, Zt4, At4, dT4, p.bn2_w, g.bn2_w, g.bn2_b);
    T.grad_w(dT4, Hi, At0, Hi, n2, sp2, {g.trunk4_w, g.trunk4_b, Hi});
    T.grad_in(dT4, n2, p.trunk4_w, Hi, dT0);
    bn_backward2(3, false, Zt0, At0, dT0, p.bn1_w, g.bn1_w, g.bn1_b);
    T.grad_w(dT0, Hi, Cat, H2, n2, sp2, {g.trunk0_w, g.trunk0_b, Hi});
    T.grad_in(dT0, n2, p.trunk0_w, H2, dCat);
    if (T.ok()) {
        hipLaunchKernelGGL(k_sym_uncat, T.blocks((size_t)2 * n * H), dim3(256), 0, stream, (const float*)dCat, dS, dP, n, Hi);
        T.launched();
    }
    // the encoders
    bn_backward2(1, false, Zp, Ap, dP, p.pe1_w, g.pe1_w, g.pe1_b);
    T.grad_w(dP, Hi, Xp, Dp, n2, sp2, {g.pe0_w, g.pe0_b, Hi});
    bn_backward(0, 0, false, Zs, As, dS, nullptr, p.se1_w, g.se1_w, g.se1_b);
    T.grad_w(dS, Hi, Xs, Ds, n, sp1, {g.se0_w, g.se0_b, Hi});
    return T.end();
}

// ar_rows_grad_cnn_gpool: the loss and the gradients of PyRatCNN over rows first .. first + n of the order, on the caller's
// stream: train_cnn.h's chain, under TrainStep's rules. A trunk activation is [R][C] with R = n hw; the heads' arrays hold
// P1's n rows, then P2's, as in rows_grad_symmetric. A block b with pd->gpool_channels[b] != 0 is a GPoolResBlock, whose pool
// path train_gpool.h lists; with `dropout` the four kernels around the player cells are their masked forms. Without either
// (ar_rows_grad_cnn) the launches and their arguments are train_cnn.h's.
template <int NW>
int rows_grad_cnn(RowStore& R, uint64_t first, uint64_t n64, const ArCnnDims& dims, const ArCnnTensors& p, const ArCnnTensors& g,
                  const ArCnnBnStats* run, float pw, float vw, const ArTrainOut* out, hipStream_t stream,
                  const ArCnnPoolDims* pd = nullptr, const ArCnnPoolTensors* pp = nullptr, const ArCnnPoolTensors* pg = nullptr,
                  const ArCnnPoolStats* prun = nullptr, const ArTrainDropout* dropout = nullptr) {
    static_assert(sizeof(ArCnnPoolTensors) == 40 * sizeof(float*) && sizeof(ArCnnPoolBlock) == 5 * sizeof(float*), "8 * 5 pointers");
    static_assert(sizeof(ArCnnPoolStats) == 2 * sizeof(float*), "2 pointers a block");
    static_assert(sizeof(ArCnnTensors) == 59 * sizeof(float*) && sizeof(ArCnnBlock) == 6 * sizeof(float*), "3 + 8 * 6 + 8 pointers");
    static_assert(sizeof(ArCnnBnStats) == 34 * sizeof(float*), "2 + 8 * 4 pointers");
    const uint32_t Cu = dims.channels, PDu = dims.player_dim, HDu = dims.hidden_dim, Bu = dims.n_blocks;
    if (Cu == 0 || Cu % 32 != 0 || Cu > 256)
        return fail(AR_E_INVALID, "channels must be a multiple of 32, at most 256 (got " + std::to_string(Cu) + ")");
    if (PDu == 0 || PDu > 256) return fail(AR_E_INVALID, "player_dim must be 1 to 256 (got " + std::to_string(PDu) + ")");
    if (Bu > (uint32_t)CNN_MAX_BLOCKS_TRAIN) return fail(AR_E_INVALID, "at most 8 residual blocks (got " + std::to_string(Bu) + ")");
    if (R.hw < 2 || R.hw > 256)  // (k_cnn_split's 5 n hw threads also fill the 6n side elements)
        return fail(AR_E_INVALID, "boards of 2 to 256 cells (this one has " + std::to_string(R.hw) + ")");
    if (n64 <= (uint64_t)TRAIN_MAX_ROWS && n64 * R.hw > (uint64_t)CNN_MAX_TRUNK_ROWS)  // (more rows than that: check's refusal)
        return fail(AR_E_INVALID, "n * h * w is " + std::to_string(n64 * R.hw) + ": at most 2^22 trunk rows a step");
    // the gpool blocks among the first n_blocks: Gs[b] = gpool_channels, 0 for a ResBlock
    int Gs[CNN_MAX_BLOCKS_TRAIN] = {}, n_pool = 0, Gmax = 0;
    for (uint32_t b = 0; pd && b < Bu; ++b) {
        const uint32_t Gu = pd->gpool_channels[b];
        if (Gu > (uint32_t)CNN_MAX_GPOOL)
            return fail(AR_E_INVALID, "gpool_channels must be at most 256 (block " + std::to_string(b) + " has " + std::to_string(Gu) + ")");
        if (Gu == 0) continue;
        if (!pp || !pg) return fail(AR_E_INVALID, "null tensor: the pool tensors of block " + std::to_string(b));
        if (run && !prun) return fail(AR_E_INVALID, "null running statistic: pool_bn of block " + std::to_string(b));
        Gs[b] = (int)Gu;
        Gmax = std::max(Gmax, (int)Gu);
        ++n_pool;
    }
    // (the products over the trunk rows put their row tiles on blockIdx.y)
    if (n_pool && n64 <= (uint64_t)TRAIN_MAX_ROWS && n64 * R.hw > (uint64_t)65535 * TG_TILE)
        return fail(AR_E_INVALID, "n * h * w is " + std::to_string(n64 * R.hw) + ": at most 65535 * 64 trunk rows with a gpool block");
    // the tensors that B blocks use, under their names
    std::vector<std::string> names = {"stem_w", "stem_bn_w", "stem_bn_b"};
    std::vector<float*> ps = {p.stem_w, p.stem_bn_w, p.stem_bn_b}, gs = {g.stem_w, g.stem_bn_w, g.stem_bn_b}, rs;
    if (run) rs = {run->stem_mean, run->stem_var};
    for (uint32_t b = 0; b < Bu; ++b) {
        static const char* const kBlock[6] = {"bn1_w", "bn1_b", "conv1_w", "bn2_w", "bn2_b", "conv2_w"};
        const ArCnnBlock &pb = p.blocks[b], &gb = g.blocks[b];
        float* const pk[6] = {pb.bn1_w, pb.bn1_b, pb.conv1_w, pb.bn2_w, pb.bn2_b, pb.conv2_w};
        float* const gk[6] = {gb.bn1_w, gb.bn1_b, gb.conv1_w, gb.bn2_w, gb.bn2_b, gb.conv2_w};
        for (int k = 0; k < 6; ++k) {
            names.push_back("blocks[" + std::to_string(b) + "]." + kBlock[k]);
            ps.push_back(pk[k]);
            gs.push_back(gk[k]);
        }
        if (run) {
            const ArCnnBlockStats& rb = run->blocks[b];
            rs.insert(rs.end(), {rb.bn1_mean, rb.bn1_var, rb.bn2_mean, rb.bn2_var});
        }
        if (Gs[b]) {
            static const char* const kPool[5] = {"pool_bn_w", "pool_bn_b", "pool_conv_w", "pool_linear_w", "pool_linear_b"};
            const ArCnnPoolBlock &qb = pp->blocks[b], &hb = pg->blocks[b];
            float* const pk[5] = {qb.pool_bn_w, qb.pool_bn_b, qb.pool_conv_w, qb.pool_linear_w, qb.pool_linear_b};
            float* const gk[5] = {hb.pool_bn_w, hb.pool_bn_b, hb.pool_conv_w, hb.pool_linear_w, hb.pool_linear_b};
            for (int k = 0; k < 5; ++k) {
                names.push_back("blocks[" + std::to_string(b) + "]." + kPool[k]);
                ps.push_back(pk[k]);
                gs.push_back(gk[k]);
            }
            if (run) rs.insert(rs.end(), {prun[b].pool_bn_mean, prun[b].pool_bn_var});
        }
    }
    {
        static const char* const kTail[8] = {"enc_w", "enc_b", "comb_w", "comb_b", "policy_w", "policy_b", "value_w", "value_b"};
        float* const pk[8] = {p.enc_w, p.enc_b, p.comb_w, p.comb_b, p.policy_w, p.policy_b, p.value_w, p.value_b};
        float* const gk[8] = {g.enc_w, g.enc_b, g.comb_w, g.comb_b, g.policy_w, g.policy_b, g.value_w, g.value_b};
        for (int k = 0; k < 8; ++k) {
            names.push_back(kTail[k]);
            ps.push_back(pk[k]);
            gs.push_back(gk[k]);
        }
    }
    std::vector<const char*> name_ptrs;
    for (const std::string& s : names) name_ptrs.push_back(s.c_str());
    TrainStep T{R, stream};
    if (int rc = T.check(first, n64, HDu, name_ptrs.data(), ps.data(), gs.data(), (int)ps.size(), rs.data(), (int)rs.size(), out))
        return rc;
    if (int rc = T.check_dropout(dropout)) return rc;
    const int n = T.n, n2 = 2 * n, hw = (int)R.hw, C = (int)Cu, PD = (int)PDu, HD = (int)HDu, B = (int)Bu, W = C + PD;
    const int Rr = n * hw;
    const TrainCols tcR = cnn_cols(n, hw, C);
    TrainCols tc1 = tcR;  // what the column kernels see once the parts are collapsed: the same rows per part, one row of totals
    tc1.P = 1;
    const TrainSplit spR = cnn_split(n, hw), sp2 = train_split(n2), spN = train_split(n);
    const int n_calls = 2 * B + 1 + (n_pool ? B : 0);  // pool_bn of block b is BatchNorm call 2 B + 1 + b
    const size_t act = (size_t)Rr * C * 4;
    T.take_rows();
    const size_t o_x5 = T.take((size_t)Rr * 5 * 4), o_side = T.take((size_t)n2 * 3 * 4), o_cells = T.take((size_t)n2 * 4),
                 o_zs = T.take(act), o_x = T.take((size_t)(B + 1) * act), o_blk = T.take((size_t)3 * B * act), o_g = T.take(act),
                 o_d = T.take(act), o_e = T.take(act), o_ze = T.take((size_t)n2 * PD * 4), o_cat = T.take((size_t)n2 * W * 4),
                 o_zc = T.take((size_t)n2 * HD * 4), o_h = T.take((size_t)n2 * HD * 4), o_d12 = T.take((size_t)n2 * 48),
                 o_dzc = T.take((size_t)n2 * HD * 4), o_dcat = T.take((size_t)n2 * W * 4), o_dze = T.take((size_t)n2 * PD * 4),
                 o_parts = T.take((size_t)2 * CNN_MAX_PARTS * C * 8), o_tot = T.take((size_t)2 * C * 8),
                 o_mean = T.take((size_t)n_calls * C * 8), o_rstd = T.take((size_t)n_calls * C * 4),
                 o_wpart = T.take(std::max({(size_t)spR.S * C * 9 * C, (size_t)sp2.S * std::max(HD * W, 12 * HD),
                                            n_pool ? (size_t)spN.S * C * 2 * Gmax : (size_t)0}) * 4),
                 o_bpart = T.take((size_t)(n_pool ? std::max({sp2.S, spN.S, spR.S}) : sp2.S) * 256 * 4), o_scr = T.take((size_t)256 * 4);
    T.take_losses();
    // what the gpool blocks add: per block ap, pz, pool_cat and the tie counts; once c2 / the third gradient array, po, dpo,
    // dcat and dpz
    size_t o_ap[CNN_MAX_BLOCKS_TRAIN] = {}, o_pz[CNN_MAX_BLOCKS_TRAIN] = {}, o_pcat[CNN_MAX_BLOCKS_TRAIN] = {},
           o_pcnt[CNN_MAX_BLOCKS_TRAIN] = {}, o_pe = 0, o_po = 0, o_dpcat = 0, o_dpz = 0;
    if (n_pool) {
        for (int b = 0; b < B; ++b)
            if (Gs[b]) {
                o_ap[b] = T.take(act);
                o_pz[b] = T.take((size_t)Rr * Gs[b] * 4);
                o_pcat[b] = T.take((size_t)n * 2 * Gs[b] * 4);
                o_pcnt[b] = T.take((size_t)n * Gs[b] * 4);
            }
        o_pe = T.take(act);
        o_po = T.take((size_t)n * C * 4);
        o_dpcat = T.take((size_t)n * 2 * Gmax * 4);
        o_dpz = T.take((size_t)Rr * Gmax * 4);
    }
    if (int rc = T.begin()) return rc;
    float *X5 = T.f(o_x5), *Side = T.f(o_side), *Zs = T.f(o_zs), *G = T.f(o_g), *Dd = T.f(o_d), *E = T.f(o_e), *Ze = T.f(o_ze),
          *Cat = T.f(o_cat), *Zc = T.f(o_zc), *Hh = T.f(o_h), *D12 = T.f(o_d12), *dZc = T.f(o_dzc), *dCat = T.f(o_dcat),
          *dZe = T.f(o_dze), *rstds = T.f(o_rstd), *scr = T.f(o_scr);
    int* cells = (int*)(T.ws + o_cells);
    double *parts = T.d(o_parts), *tots = T.d(o_tot), *means = T.d(o_mean);
    T.wpart = T.f(o_wpart);
    T.bpart = T.f(o_bpart);
    auto xs = [&](int b) { return T.f(o_x) + (size_t)b * Rr * C; };                 // the residual stream x_b
    auto blk = [&](int b, int i) { return T.f(o_blk) + (size_t)(3 * b + i) * Rr * C; };  // a block's a, z, a'
    double *part0 = parts, *part1 = parts + (size_t)CNN_MAX_PARTS * C, *tot0 = tots, *tot1 = tots + C;
    const dim3 cgrid((C + 63) / 64, tcR.P), colgrid((C + 255) / 256);
    // one BatchNorm call over the R rows at z (0: stem_bn; 1 + 2 b, 2 + 2 b: block b's bn1, bn2)
    auto bn_forward = [&](int call, const float* z, const float* gamma, const float* beta, float* a, float* rm, float* rv) {
        if (!T.ok()) return;
        TrainColArgs ca;
        memset(&ca, 0, sizeof ca);
        ca.z = z;
        ca.part0 = part0;
        hipLaunchKernelGGL(k_train_colsum<TC_SUM>, cgrid, dim3(256), 0, stream, tcR, ca);
        hipLaunchKernelGGL(k_cnn_collapse, colgrid, dim3(256), 0, stream, tcR.P, C, (const double*)part0, tot0, (const double*)nullptr,
                           (double*)nullptr);
        ca.sum_in = tot0;
        ca.part0 = part1;
        hipLaunchKernelGGL(k_train_colsum<TC_SQ>, cgrid, dim3(256), 0, stream, tc1, ca);
        hipLaunchKernelGGL(k_cnn_collapse, colgrid, dim3(256), 0, stream, tcR.P, C, (const double*)part1, tot1, (const double*)nullptr,
                           (double*)nullptr);
        hipLaunchKernelGGL(k_train_bn_apply, cgrid, dim3(256), 0, stream, tc1, z, (const double*)tot0, (const double*)tot1, gamma, beta,
                           a, means + (size_t)call * C, rstds + (size_t)call * C, rm, rv);
        T.launched();
    };
    // dz in place of dA at d, through the ReLU whose output is a
    auto bn_backward = [&](int call, const float* z, const float* a, float* d, const float* gamma, float* dgamma, float* dbeta) {
        if (!T.ok()) return;
        const double* mu = means + (size_t)call * C;
        const float* rstd = rstds + (size_t)call * C;
        const TrainColArgs ca = TrainStep::backward_args(z, a, d, mu, rstd, part0, part1);
        hipLaunchKernelGGL(k_train_colsum<TC_DTRUNK>, cgrid, dim3(256), 0, stream, tcR, ca);
        hipLaunchKernelGGL(k_cnn_collapse, colgrid, dim3(256), 0, stream, tcR.P, C, (const double*)part0, tot0, (const double*)part1, tot1);
        hipLaunchKernelGGL(k_train_bn_bwd, cgrid, dim3(256), 0, stream, tc1, z, d, (const double*)tot0, (const double*)tot1, mu, rstd,
                           gamma, dgamma, dbeta);
        T.launched();
    };
    auto conv_args = [&](const float* x, const float* w, const float* d, const float* add, float* c, int Cin) {
        TrainConv t;
        t.x = x, t.w = w, t.d = d, t.add = add, t.c = c;
        t.R = Rr, t.hw = hw, t.bw = (int)R.width, t.bh = (int)R.height, t.Cin = Cin, t.Cout = C;
        t.k_per_split = 9 * C;  // (FWD, DIN: one range, and K is at most this)
        t.c_split = 0;
        return t;
    };
    const unsigned mtiles = (unsigned)((Rr + TG_TILE - 1) / TG_TILE), ctiles = (unsigned)((C + TG_TILE - 1) / TG_TILE);
    auto conv = [&](const float* in, int Cin, const float* w, const float* add, float* o) {
        if (!T.ok()) return;
        hipLaunchKernelGGL(k_train_conv3<CV_FWD>, dim3(mtiles, ctiles, 1), dim3(TG_THREADS), 0, stream, conv_args(in, w, nullptr, add, o, Cin));
        T.launched();
    };
    auto conv_din = [&](const float* dout, const float* w, float* din) {
        if (!T.ok()) return;
        hipLaunchKernelGGL(k_train_conv3<CV_DIN>, dim3(mtiles, ctiles, 1), dim3(TG_THREADS), 0, stream,
                           conv_args(dout, w, nullptr, nullptr, din, C));
        T.launched();
    };
    auto conv_dw = [&](const float* dout, const float* in, int Cin, float* dw) {
        if (!T.ok()) return;
        TrainConv t = conv_args(in, nullptr, dout, nullptr, T.wpart, Cin);
        t.k_per_split = spR.kps;
        t.c_split = (size_t)C * 9 * Cin;
        hipLaunchKernelGGL(k_train_conv3<CV_DW>, dim3((unsigned)((9 * Cin + TG_TILE - 1) / TG_TILE), ctiles, spR.S), dim3(TG_THREADS), 0,
                           stream, t);
        TrainReduce tr;
        tr.wpart = T.wpart;
        // A convolution here has no bias, and k_train_reduce always reduces M bias lanes beside the M x N weights. They are
        // given something harmless to do: bpart = wpart, so lane j adds wpart[k * M + j], k < S -- inside the S * M * N floats of
        // the partial products -- and writes the sum to scr[j], j < C <= 256, a scratch row nobody reads (train_mlp.h TrainReduce).
        tr.bpart = T.wpart;
        tr.S = spR.S, tr.M = C, tr.N = 9 * Cin;
        tr.w[0] = dw, tr.w[1] = tr.w[2] = nullptr;
        tr.b[0] = scr, tr.b[1] = tr.b[2] = nullptr;
        tr.rows[0] = C, tr.rows[1] = tr.rows[2] = 0;
        hipLaunchKernelGGL(k_train_reduce, TrainStep::blocks((size_t)C * 9 * Cin + C), dim3(256), 0, stream, tr);
        T.launched();
    };
    T.rows<NW>(first);
    if (T.ok()) {
        hipLaunchKernelGGL(k_cnn_split, TrainStep::blocks((size_t)Rr * 5), dim3(256), 0, stream, (const float*)T.ro.observation, X5, Side,
                           cells, n, hw);
        T.launched();
    }
    // forward: the trunk
    conv(X5, 5, p.stem_w, nullptr, Zs);
    bn_forward(0, Zs, p.stem_bn_w, p.stem_bn_b, xs(0), run ? run->stem_mean : nullptr, run ? run->stem_var : nullptr);
    for (int b = 0; b < B; ++b) {
        const ArCnnBlock& q = p.blocks[b];
        bn_forward(1 + 2 * b, xs(b), q.bn1_w, q.bn1_b, blk(b, 0), run ? run->blocks[b].bn1_mean : nullptr,
                   run ? run->blocks[b].bn1_var : nullptr);
        conv(blk(b, 0), C, q.conv1_w, nullptr, blk(b, 1));
        bn_forward(2 + 2 * b, blk(b, 1), q.bn2_w, q.bn2_b, blk(b, 2), run ? run->blocks[b].bn2_mean : nullptr,
                   run ? run->blocks[b].bn2_var : nullptr);
        if (!Gs[b]) {
            conv(blk(b, 2), C, q.conv2_w, xs(b), xs(b + 1));
            continue;
        }
        // a gpool block: conv2 without the skip, the pool path, and the three terms joined in torch's order
        const int Gp = Gs[b];
        const ArCnnPoolBlock& qp = pp->blocks[b];
        float *Pe = T.f(o_pe), *Ap = T.f(o_ap[b]), *Pz = T.f(o_pz[b]), *Pcat = T.f(o_pcat[b]), *Po = T.f(o_po);
        conv(blk(b, 2), C, q.conv2_w, nullptr, Pe);
        bn_forward(2 * B + 1 + b, xs(b), qp.pool_bn_w, qp.pool_bn_b, Ap, run ? prun[b].pool_bn_mean : nullptr,
                   run ? prun[b].pool_bn_var : nullptr);
        T.gemm(Ap, C, 1, 1, qp.pool_conv_w, 1, C, 1, Pz, Rr, Gp, C, nullptr, 1, C, nullptr);
        if (T.ok()) {
            hipLaunchKernelGGL(k_gpool_reduce, TrainStep::blocks((size_t)n * Gp), dim3(256), 0, stream, (const float*)Pz, Pcat,
                               (int*)(T.ws + o_pcnt[b]), n, hw, Gp);
            T.launched();
        }
        T.gemm(Pcat, 2 * Gp, 1, 1, qp.pool_linear_w, 1, 2 * Gp, 1, Po, n, C, 2 * Gp, qp.pool_linear_b, 1, 2 * Gp, nullptr);
        if (T.ok()) {
            const size_t c4 = (size_t)Rr * C / 4;
            hipLaunchKernelGGL(k_gpool_join, TrainStep::blocks(c4), dim3(256), 0, stream, (const float4*)Pe, (const float*)Po,
                               (const float4*)xs(b), (float4*)xs(b + 1), c4, hw, C);
            T.launched();
        }
    }
    // the player cells and the heads
    const TrainDrop dr_e1 = T.drop_of(0), dr_e2 = T.drop_of(1), dr_c1 = T.drop_of(2), dr_c2 = T.drop_of(3);
    T.gemm(Side, 3, 1, 1, p.enc_w, 1, 3, 1, Ze, n2, PD, 3, p.enc_b, 1, 3, nullptr);
    if (T.ok()) {
        if (T.dropping)
            hipLaunchKernelGGL(k_cnn_gather_drop, TrainStep::blocks((size_t)n2 * W), dim3(256), 0, stream, (const float*)xs(B),
                               (const int*)cells, (const float*)Ze, Cat, n, hw, C, PD, dr_e1, dr_e2);
        else
            hipLaunchKernelGGL(k_cnn_gather, TrainStep::blocks((size_t)n2 * W), dim3(256), 0, stream, (const float*)xs(B), (const int*)cells,
                               (const float*)Ze, Cat, n, hw, C, PD);
        T.launched();
    }
    T.gemm(Cat, W, 1, 1, p.comb_w, 1, W, 1, Zc, n2, HD, W, p.comb_b, 1, W, nullptr);
    if (T.ok()) {
        const size_t c4 = (size_t)n2 * HD / 4;
        if (T.dropping)
            hipLaunchKernelGGL(k_cnn_relu_drop, TrainStep::blocks((size_t)n2 * HD), dim3(256), 0, stream, (const float*)Zc, Hh, n, HD,
                               dr_c1, dr_c2);
        else
            hipLaunchKernelGGL(k_train_lv_relu, TrainStep::blocks(c4), dim3(256), 0, stream, (const float4*)Zc, (float4*)Hh, c4);
        SymHeads t;
        t.h = Hh;
        t.w_p = p.policy_w, t.b_p = p.policy_b, t.w_v = p.value_w, t.b_v = p.value_b;
        t.t1 = T.ro.policy_p1, t.t2 = T.ro.policy_p2, t.y1 = T.ro.value_p1, t.y2 = T.ro.value_p2;
        t.d12 = D12;
        t.loss_part = T.d(T.o_lpart);
        t.logits_p1 = out ? out->logits_p1 : nullptr;
        t.logits_p2 = out ? out->logits_p2 : nullptr;
        t.value_p1 = out ? out->value_p1 : nullptr;
        t.value_p2 = out ? out->value_p2 : nullptr;
        t.n = n;
        t.H = HD;
        t.pw_n = pw / (float)n;
        t.vw_n = vw / (float)n;
        hipLaunchKernelGGL(k_sym_heads, dim3(T.head_blocks), dim3(256), (size_t)12 * HD * 4, stream, t);
        T.loss_sum(pw, vw, out);
    }
    // backward: the heads, the combiner, the encoder
    T.gemm(D12, 1, 12, 0, Hh, HD, 1, 0, T.wpart, 12, HD, n2, nullptr, sp2.S, sp2.kps, T.bpart);
    if (T.ok()) {
        hipLaunchKernelGGL(k_sym_head_reduce, TrainStep::blocks((size_t)12 * HD + 6), dim3(256), 0, stream, (const float*)T.wpart,
                           (const float*)T.bpart, sp2.S, HD, g.policy_w, g.policy_b, g.value_w, g.value_b);
        if (T.dropping)
            hipLaunchKernelGGL(k_cnn_dhead_drop, TrainStep::blocks((size_t)n2 * HD), dim3(256), 0, stream, (const float*)D12,
                               (const float*)p.policy_w, (const float*)p.value_w, (const float*)Hh, dZc, n2, HD, dr_c1.scale);
        else
            hipLaunchKernelGGL(k_cnn_dhead, TrainStep::blocks((size_t)n2 * HD), dim3(256), 0, stream, (const float*)D12,
                               (const float*)p.policy_w, (const float*)p.value_w, (const float*)Hh, dZc, n2, HD);
        T.launched();
    }
    T.grad_w(dZc, HD, Cat, W, n2, sp2, {g.comb_w, g.comb_b, HD});
    T.grad_in(dZc, n2, p.comb_w, W, dCat, HD);
    if (T.ok()) {
        if (T.dropping)
            hipLaunchKernelGGL(k_cnn_enc_bwd_drop, TrainStep::blocks((size_t)n2 * PD), dim3(256), 0, stream, (const float*)dCat,
                               (const float*)Cat, dZe, n2, C, PD, dr_e1.scale);
        else
            hipLaunchKernelGGL(k_cnn_enc_bwd, TrainStep::blocks((size_t)n2 * PD), dim3(256), 0, stream, (const float*)dCat,
                               (const float*)Ze, dZe, n2, C, PD);
        T.launched();
    }
    T.grad_w(dZe, PD, Side, 3, n2, sp2, {g.enc_w, g.enc_b, PD});
    if (T.ok()) {
        hipLaunchKernelGGL(k_cnn_scatter, TrainStep::blocks((size_t)Rr * C), dim3(256), 0, stream, (const float*)dCat, (const int*)cells, G,
                           n, hw, C, PD);
        T.launched();
    }
    // the trunk, G the gradient of the residual stream
    for (int b = B - 1; b >= 0; --b) {
        const ArCnnBlock &q = p.blocks[b], &gq = g.blocks[b];
        conv_dw(G, blk(b, 2), C, gq.conv2_w);
        conv_din(G, q.conv2_w, Dd);
        bn_backward(2 + 2 * b, blk(b, 1), blk(b, 2), Dd, q.bn2_w, gq.bn2_w, gq.bn2_b);
        conv_dw(Dd, blk(b, 0), C, gq.conv1_w);
        conv_din(Dd, q.conv1_w, E);
        bn_backward(1 + 2 * b, xs(b), blk(b, 0), E, q.bn1_w, gq.bn1_w, gq.bn1_b);
        float* Pe = nullptr;
        if (Gs[b]) {  // the pool path, from the same G = d x_b+1, into Pe
            const int Gp = Gs[b];
            const ArCnnPoolBlock &qp = pp->blocks[b], &gp = pg->blocks[b];
            float *Ap = T.f(o_ap[b]), *Pz = T.f(o_pz[b]), *Pcat = T.f(o_pcat[b]), *dPo = T.f(o_po), *dPcat = T.f(o_dpcat),
                  *dPz = T.f(o_dpz);
            Pe = T.f(o_pe);
            if (T.ok()) {
                hipLaunchKernelGGL(k_gpool_rowsum, TrainStep::blocks((size_t)n * C), dim3(256), 0, stream, (const float*)G, dPo, n, hw, C);
                T.launched();
            }
            T.grad_w(dPo, C, Pcat, 2 * Gp, n, spN, {gp.pool_linear_w, gp.pool_linear_b, C});
            T.grad_in(dPo, n, qp.pool_linear_w, 2 * Gp, dPcat, C);
            if (T.ok()) {
                hipLaunchKernelGGL(k_gpool_dpz, TrainStep::blocks((size_t)Rr * Gp), dim3(256), 0, stream, (const float*)Pz,
                                   (const float*)Pcat, (const int*)(T.ws + o_pcnt[b]), (const float*)dPcat, dPz, n, hw, Gp);
                T.launched();
            }
            // over cnn_split's ranges of the trunk rows, as CV_DW (no bias: the column sums go to the scratch row)
            T.grad_w(dPz, Gp, Ap, C, Rr, spR, {gp.pool_conv_w, scr, Gp});
            T.grad_in(dPz, Rr, qp.pool_conv_w, C, Pe, Gp);
            bn_backward(2 * B + 1 + b, xs(b), Ap, Pe, qp.pool_bn_w, gp.pool_bn_w, gp.pool_bn_b);
        }
        if (T.ok()) {
            const size_t c4 = (size_t)Rr * C / 4;
            hipLaunchKernelGGL(k_cnn_add, TrainStep::blocks(c4), dim3(256), 0, stream, (float4*)G, (const float4*)E, c4);
            T.launched();
        }
        if (Pe && T.ok()) {
            const size_t c4 = (size_t)Rr * C / 4;
            hipLaunchKernelGGL(k_cnn_add, TrainStep::blocks(c4), dim3(256), 0, stream, (float4*)G, (const float4*)Pe, c4);
            T.launched();
        }
    }
    bn_backward(0, Zs, xs(0), G, p.stem_bn_w, g.stem_bn_w, g.stem_bn_b);
    conv_dw(G, X5, 5, g.stem_w);
    return T.end();
}

// ar_rows_validate: the request in chunks of `chunk` rows -- requests from the stored records (k_val_requests), the
// evaluator with its logits output (net_launch), the terms of every row summed per block (k_val_terms) and added to the
// running total (k_val_sum) -- all on the null stream; blocks until the sums are on the host. No observation, no target
// array and, without `ro`, no per-row output leaves the device.
//
// ar_rows_validate_lv (`own` set): the evaluator launch is the one that also stores its trunk output, and behind it run the
// ownership head with its row terms (k_own_mfma) and their reduction (k_own_sum, batches of `loss_batch` rows); the
// launches that ar_rows_validate makes are the same ones with the same arguments, so `sums` and `ro` get the same bytes.
enum { VAL_DEFAULT_CHUNK = 65536 };
template <int NW>
int rows_validate(RowStore& R, ArNet* net, const uint64_t* rows, uint64_t n, uint32_t chunk, ArValSums& sums, const ArValRows* ro,
                  uint32_t loss_batch = 0, ArOwnSums* own = nullptr, const ArOwnRows* oro = nullptr) {
    for (uint64_t i = 0; i < n; ++i)
        if (rows[i] >= R.n_pos)
            return fail(AR_E_INVALID, "row " + std::to_string(i) + " asks for position " + std::to_string(rows[i]) +
                                          ", the set holds " + std::to_string(R.n_pos));
    if (net->dev.width != R.width || net->dev.height != R.height)
        return fail(AR_E_INVALID, "the network was built for a " + std::to_string(net->dev.width) + "x" +
                                      std::to_string(net->dev.height) + " board, the row set holds " + std::to_string(R.width) +
                                      "x" + std::to_string(R.height) + " games");
    if (net->device != R.device)
        return fail(AR_E_INVALID, "the network is on device " + std::to_string(net->device) + ", the row set on device " +
                                      std::to_string(R.device));
    const size_t n_games = R.h_games.size();
    if ((uint64_t)n_games * R.hw * 4u > 0xFFFFFFFFull)  // Board::maze_off is 32 bits wide
        return fail(AR_E_INVALID, "the row set holds more games than an evaluator's maze pool can address");
    if (own) own->batch_rows = loss_batch;
    if (n == 0) return AR_OK;
    if (chunk == 0) chunk = VAL_DEFAULT_CHUNK;
    if (own && loss_batch) {  // no batch straddles two chunks
        uint64_t c = ((uint64_t)chunk + loss_batch - 1) / loss_batch * loss_batch;
        if (c > n) c = n;
        if (c > 0xFFFFFFFFull) return fail(AR_E_INVALID, "loss_batch_rows does not fit a chunk of the request");
        chunk = (uint32_t)c;
    }
    if ((uint64_t)chunk > n) chunk = (uint32_t)n;
    HIP_TRY(hipSetDevice(R.device));
    HIP_TRY(R.wait_appends());
    HIP_TRY(R.wait_batches());
    const uint32_t max_blocks = (chunk + VAL_BLOCK - 1) / VAL_BLOCK;
    if (own) {
        const size_t feat_n = (size_t)chunk * net->dev.H, logits_n = oro && oro->logits ? (size_t)chunk * R.hw * 4 : 0;
        bool ok = true;
        if (feat_n > R.own_feat_n) {
            R.own_feat_n = 0;
            ok = regrow(R.own_feat, feat_n) == hipSuccess;
            if (ok) R.own_feat_n = feat_n;
        }
        if (ok && chunk > R.own_chunk) {
            R.own_chunk = 0;
            ok = regrow(R.own_ce, chunk) == hipSuccess && regrow(R.own_cells, chunk) == hipSuccess &&
                 regrow(R.own_value, chunk) == hipSuccess && (R.own_total.p || R.own_total.alloc(1) == hipSuccess);
            if (ok) R.own_chunk = chunk;
        }
        if (ok && logits_n > R.own_logits_n) {
            R.own_logits_n = 0;
            ok = regrow(R.own_logits, logits_n) == hipSuccess;
            if (ok) R.own_logits_n = logits_n;
        }
        if (!ok) {
            (void)hipGetLastError();
            return fail(AR_E_NOMEM, "not enough device memory to validate " + std::to_string(chunk) +
                                        " rows at a time with the ownership head");
        }
    }
    if (chunk > R.val_chunk) {
        R.val_chunk = 0;
        if (regrow(R.val_rows, chunk) != hipSuccess || regrow(R.val_req, (size_t)chunk * sizeof(LeafReq<NW>)) != hipSuccess ||
            regrow(R.val_out, chunk) != hipSuccess || regrow(R.val_logits, (size_t)chunk * 10) != hipSuccess ||
            regrow(R.val_partial, max_blocks) != hipSuccess || (!R.val_total.p && R.val_total.alloc(1) != hipSuccess)) {
            (void)hipGetLastError();
            return fail(AR_E_NOMEM, "not enough device memory to validate " + std::to_string(chunk) + " rows at a time");
        }
        R.val_chunk = chunk;
    }
    // the boards of the games appended since the last call
    if (n_games > R.val_boards.n || !R.val_boards.p) {
        if (regrow(R.val_boards, n_games + n_games / 2 + 64) != hipSuccess) {
            (void)hipGetLastError();
            return fail(AR_E_NOMEM, "not enough device memory for the boards of " + std::to_string(n_games) + " games");
        }
        R.val_boards_n = 0;
    }
    if (R.val_boards_n < n_games) {
        std::vector<Board> boards(n_games - R.val_boards_n);
        for (size_t g = R.val_boards_n; g < n_games; ++g) {
            Board& b = boards[g - R.val_boards_n];
            b.width = R.h_games[g].width;
            b.height = R.h_games[g].height;
            b.max_turns = R.h_games[g].max_turns;
            b.total_cheese = 0;  // (the evaluators read the size, max_turns and maze_off)
            b.maze_off = (uint32_t)(g * R.hw * 4u);
        }
        HIP_TRY(hipMemcpy(R.val_boards.p + R.val_boards_n, boards.data(), boards.size() * sizeof(Board), hipMemcpyHostToDevice));
        R.val_boards_n = n_games;
    }
    if (net->bound_pool != R.mazes.p || net->bound_mazes != (int)n_games || net->bound_stamp != R.stamp) {
        if (int rc = net_bind_mazes(net, R.mazes.p, (int)n_games, nullptr)) return rc;
        net->bound_stamp = R.stamp;
    }
    HIP_TRY(hipMemsetAsync(R.val_total.p, 0, sizeof(ValAcc), nullptr));
    if (own) HIP_TRY(hipMemsetAsync(R.own_total.p, 0, sizeof(OwnAcc), nullptr));
    std::vector<EvalOut> h_out;
    std::vector<float> h_logits;
    if (ro) {
        h_out.resize(chunk);
        h_logits.resize((size_t)chunk * 10);
    }
    float* own_logits = own && oro && oro->logits ? R.own_logits.p : nullptr;
    const PosRec<NW>* recs = (const PosRec<NW>*)R.recs.p;
    LeafReq<NW>* req = (LeafReq<NW>*)R.val_req.p;
    for (uint64_t row0 = 0; row0 < n; row0 += chunk) {
        const uint32_t cnt = (uint32_t)(n - row0 < (uint64_t)chunk ? n - row0 : (uint64_t)chunk);
        const uint32_t blocks = (cnt + VAL_BLOCK - 1) / VAL_BLOCK;
        HIP_TRY(hipMemcpy(R.val_rows.p, rows + row0, (size_t)cnt * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_val_requests<NW>, dim3(blocks), dim3(VAL_BLOCK), 0, nullptr, recs, (const uint32_t*)R.pos_game.p,
                           (const uint64_t*)R.val_rows.p, cnt, req);
        HIP_TRY(hipGetLastError());
        if (int rc = net_launch<NW>(net, req, nullptr, cnt, (const char*)R.val_boards.p, sizeof(Board), R.val_out.p,
                                    R.val_logits.p, nullptr, own ? R.own_feat.p : nullptr))
            return rc;
        if (own) {
            if (int rc = net_launch_own<NW>(net, R.own_feat.p, req, R.outcomes.p, cnt, R.own_ce.p, R.own_cells.p, R.own_value.p,
                                            own_logits, nullptr))
                return rc;
            hipLaunchKernelGGL(k_own_sum, dim3(1), dim3(OWN_SUM_BLOCK), 0, nullptr, (const double*)R.own_ce.p,
                               (const uint32_t*)R.own_cells.p, cnt, loss_batch, R.own_total.p);
            HIP_TRY(hipGetLastError());
            if (oro) {
                if (oro->ce) HIP_TRY(hipMemcpy(oro->ce + row0, R.own_ce.p, (size_t)cnt * 8, hipMemcpyDeviceToHost));
                if (oro->cells) HIP_TRY(hipMemcpy(oro->cells + row0, R.own_cells.p, (size_t)cnt * 4, hipMemcpyDeviceToHost));
                if (oro->value) HIP_TRY(hipMemcpy(oro->value + row0, R.own_value.p, (size_t)cnt * 4, hipMemcpyDeviceToHost));
                if (oro->logits)
                    HIP_TRY(hipMemcpy(oro->logits + row0 * R.hw * 4, own_logits, (size_t)cnt * R.hw * 16, hipMemcpyDeviceToHost));
            }
        }
        hipLaunchKernelGGL(k_val_terms<NW>, dim3(blocks), dim3(VAL_BLOCK), 0, nullptr, recs, (const uint32_t*)R.pos_game.p,
                           (const RowGame*)R.games.p, (const uint64_t*)R.val_rows.p, cnt, (const float*)R.val_logits.p,
                           (const EvalOut*)R.val_out.p, R.val_partial.p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_val_sum, dim3(1), dim3(64), 0, nullptr, (const ValAcc*)R.val_partial.p, blocks, R.val_total.p);
        HIP_TRY(hipGetLastError());
        if (ro) {
            HIP_TRY(hipMemcpy(h_out.data(), R.val_out.p, sizeof(EvalOut) * cnt, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(h_logits.data(), R.val_logits.p, (size_t)cnt * 40, hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < cnt; ++i) {
                if (ro->logits_p1) memcpy(ro->logits_p1 + (row0 + i) * 5, &h_logits[(size_t)i * 10], 20);
                if (ro->logits_p2) memcpy(ro->logits_p2 + (row0 + i) * 5, &h_logits[(size_t)i * 10 + 5], 20);
                if (ro->value_p1) ro->value_p1[row0 + i] = h_out[i].v1;
                if (ro->value_p2) ro->value_p2[row0 + i] = h_out[i].v2;
            }
        }
    }
    ValAcc total;
    HIP_TRY(hipMemcpy(&total, R.val_total.p, sizeof total, hipMemcpyDeviceToHost));  // (waits for the null stream)
    if (own) {
        OwnAcc ot;
        HIP_TRY(hipMemcpy(&ot, R.own_total.p, sizeof ot, hipMemcpyDeviceToHost));
        own->n = n;
        own->cells = ot.cells;
        own->ce = ot.ce;
        own->batch_weighted = ot.batch_weighted;
    }
    sums.n = n;
    for (int p = 0; p < 2; ++p) {
        const double* d = total.d + VAL_D_PER_PLAYER * p;
        sums.ce[p] = d[0];
        sums.sq_err[p] = d[1];
        sums.ent_pred[p] = d[2];
        sums.ent_target[p] = d[3];
        sums.sum_pred[p] = d[4];
        sums.sum_target[p] = d[5];
        sums.sum_pred2[p] = d[6];
        sums.sum_target2[p] = d[7];
        sums.sum_pred_target[p] = d[8];
        sums.top1[p] = total.c[p];
        sums.top2[p] = total.c[2 + p];
    }
    return AR_OK;
}

// ------------------------------------------------------------------------------------------------
// self-play driver
// ------------------------------------------------------------------------------------------------
// A self-play run as an object that outlives one call: the engine, its resident games and the supply of
// new games stay alive between ar_selfplay_step calls, so a caller can run the sampler in bounded slices
// (the benchmark's "step") or to the end (ar_selfplay_run = open + step until finished + close).
// The counterpart in the reference is the worker pool of run_self_play_to_disk (selfplay.rs:721-808), which
// lives for one call only; the slicing is an extension.
struct SessionBase {
    virtual ~SessionBase() {}
    virtual void info(ArSessionInfo* out) const = 0;
    virtual int step(uint32_t batch_steps, ArSelfPlayStats* window, int* finished_out) = 0;
    virtual int close(ArSelfPlayStats* total) = 0;
    virtual int attach_rows(RowStore* rows) = 0;
};

template <int NW>
struct SelfPlaySession : SessionBase {
    ArSelfPlayParams p;  // strings are copied below; the pointers in here are not used after open()
    SearchCfg cfg;
    GameSupply supply;
    std::vector<uint8_t> cost;
    uint64_t rseed = 0;
    bool unbounded = false;
    uint32_t S = 0;
    Engine<NW> eng;
    ArNet* net = nullptr;  // owned by the ArSelfPlaySession wrapper (freed after the engine)
    BundleSink writer;
    bool to_disk = false;
    ArProgress* progress = nullptr;
    ArGameSink sink = nullptr;
    void* sink_user = nullptr;
    ArSelfPlayStats st;  // finished games
    unsigned long long live[LIVE_N] = {0};  // resident games at the last scan, minus the ones drained since
    std::vector<HostGame> slot_game;
    uint64_t next_game = 0, finished = 0;
    std::chrono::steady_clock::time_point t0;
    std::string err;
    bool timing = false, failed = false;
    double tm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    RowStore* rows = nullptr;  // attached row set: every drained game is appended to it on the device
    int device_id = 0;

    int attach_rows(RowStore* r) override {
        if (rows) return fail(AR_E_INVALID, "the session already has a row set");
        if (r->attached) return fail(AR_E_INVALID, "the row set is already attached to a session");
        if (eng.steps != 0 || finished != 0) return fail(AR_E_INVALID, "a row set is attached before the session's first step");
        if (r->width != p.width || r->height != p.height)
            return fail(AR_E_INVALID, "the row set holds " + std::to_string(r->width) + "x" + std::to_string(r->height) +
                                          " games, the session plays " + std::to_string(p.width) + "x" + std::to_string(p.height));
        if (r->device != device_id) return fail(AR_E_INVALID, "the row set and the session are on different devices");
        if (S > r->place_cap) {  // (kept from an earlier session when large enough)
            HIP_TRY(hipSetDevice(device_id));
            if (r->h_place.p) HIP_TRY(hipHostFree(r->h_place.p));
            if (r->d_place.p) HIP_TRY(hipFree(r->d_place.p));
            r->h_place.p = nullptr;
            r->d_place.p = nullptr;
            r->place_cap = 0;
            if (r->h_place.alloc(S) != hipSuccess || r->d_place.alloc(S) != hipSuccess) {
                (void)hipGetLastError();
                return fail(AR_E_NOMEM, "no memory for the row set's placement buffers");
            }
            r->place_cap = S;
        }
        r->attached = true;
        rows = r;
        return AR_OK;
    }

    void info(ArSessionInfo* out) const override {
        out->resident_games = S;
        out->groups = (uint32_t)(eng.groups.empty() ? 1 : eng.groups.size());
        out->gather_kind = !eng.use_queue() ? 3u : eng.gather == GatherKernel::Wide ? 2u : eng.gather == GatherKernel::Lane ? 0u : 1u;
        out->gather_pass_limit = eng.gather == GatherKernel::Wide ? eng.gatherw_passes : 0xFFFFFFFFu;
        out->tree_region_bytes = eng.region_bytes;
        out->host_grown_arenas = eng.grows;
        out->idle_slots = (uint32_t)idle_slots.size();
        out->tree_pages_per_game = (float)pages_per_game;
    }
    ~SelfPlaySession() override {
        if (to_disk) writer.finish();
        if (eng.stream) hipStreamSynchronize(eng.stream);
        // the evaluator outlives every kernel that reads its weights: ~Engine synchronises its streams, so
        // the engine has to go first -- done explicitly in close(); here only as a last resort
    }

    bool supply_left() const { return unbounded || next_game < p.num_games; }
    bool all_finished() const { return !unbounded && finished >= p.num_games; }

    // How many games are resident is bounded by what their trees need, and that depends on the run (the network's priors
    // decide how much of a tree survives a move): a slot is only given a new game while its zone of the tree region would
    // stay under 88 % with every resident game at the size games of this run have after a few moves (measured by k_scan;
    // four fresh arenas per game until there is a measurement). Slots that have to wait are tried again at every visit.
    // Without this, 131072 games with a network that keeps big subtrees fill the region before the first generation has
    // finished, nothing can grow any more, and the run crawls (24 M instead of 370 M simulations/s, measured).
    std::vector<uint8_t> slot_busy;
    std::vector<uint32_t> zone_busy, idle_slots;
    double pages_per_game = 0.0;
    bool admit(uint32_t slot) const {
        const uint32_t z = slot / POOL_ZONE_SLOTS;
        const double zone_pages = (double)eng.pool.zone_words * POOL_WORD_PAGES;
        return ((double)zone_busy[z] + 1.0) * pages_per_game <= 0.88 * zone_pages || zone_busy[z] == 0;
    }
    void leave_slot(uint32_t slot) {
        if (slot < slot_busy.size() && slot_busy[slot]) {
            slot_busy[slot] = 0;
            zone_busy[slot / POOL_ZONE_SLOTS] -= 1;
        }
    }
    int refill(const std::vector<uint32_t>& free_slots) {
        std::vector<GameInit<NW>> inits;
        std::vector<uint8_t> mazes;
        std::vector<uint32_t> candidates;
        candidates.swap(idle_slots);
        candidates.insert(candidates.end(), free_slots.begin(), free_slots.end());
        for (uint32_t sl : candidates) {
            if (!supply_left()) break;
            if (!admit(sl)) {
                idle_slots.push_back(sl);
                continue;
            }
            slot_busy[sl] = 1;
            zone_busy[sl / POOL_ZONE_SLOTS] += 1;
            const uint32_t index = supply.index(next_game);
            HostGame g;
            if (!supply.make_game(index, g, err)) return fail(AR_E_INVALID, err);
            GameInit<NW> gi = game_init<NW>(g, sl, index, sl * eng.maze_stride);
            mazes.insert(mazes.end(), g.cost.begin(), g.cost.end());
            gi.rng_seed = rseed + index;
            gi.single = 0;
            inits.push_back(gi);
            slot_game[sl] = std::move(g);
            ++next_game;
        }
        return eng.start_games(inits, supply.gen_maze ? &mazes : nullptr);
    }

    int open(const ArSelfPlayParams& params, const GameSupply& games, int device, ArNet* owned_net, ArProgress* prog,
             ArGameSink sk, void* sk_user) {
        p = params;
        supply = games;
        net = owned_net;
        progress = prog;
        sink = sk;
        sink_user = sk_user;
        device_id = device;
        memset(&st, 0, sizeof st);
        st.min_turns = 0xFFFFFFFFu;
        cfg = to_cfg(p.search, p.simulations, p.batch_size);
        if (int rc = check_cfg(cfg)) return rc;
        cost = open_maze_cost(p.width, p.height);
        unbounded = p.num_games == 0xFFFFFFFFu;
        rseed = p.has_seed ? p.rng_seed_base : entropy_seed();
        to_disk = p.output_dir != nullptr;
        if (to_disk) {
            writer.dir = p.output_dir;
            writer.max_games = p.max_games_per_bundle ? p.max_games_per_bundle : 32;
        }
        p.maze_type = p.positions = p.output_dir = p.weights_path = p.device = nullptr;  // caller-owned strings

        // resident games: bounded by the request, the caller's hint and the arena footprint
        S = p.concurrent_games ? p.concurrent_games : 16384;
        if (S > p.num_games) S = p.num_games;
        size_t pool_bytes = 0;
        t0 = std::chrono::steady_clock::now();
        if (S == 0) return AR_OK;
        eng.configure(net, S, supply.gen_maze ? (uint32_t)supply.hw : 0u);
        {
            size_t free_b = 0, total_b = 0;
            if (hipSetDevice(device) != hipSuccess) return fail(AR_E_DEVICE, "hipSetDevice failed");
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            free_b += arena_cached_bytes(device);  // the block kept from the previous call is ours to reuse
            if (const char* e = getenv("AR_MEM_FRACTION"))  // several processes on one device (bench rehearsals): each
                if (atof(e) > 0.0 && atof(e) <= 1.0) free_b = (size_t)((double)free_b * atof(e));  // takes its share
            // device memory per resident game: its scratch and queue share, and its tree. A tree lives in a block of the
            // smallest size class (4/3 apart) that holds it plus one full search; averaged over a game's life that is about
            // twice a fresh game's block at the tuned 7x7 configuration (measured: mean tree top 2150 nodes at 1897
            // simulations per move), which is what the resident count is sized by -- games beyond what the region can
            // serve would only wait for blocks.
            const size_t fresh = arena_bytes(eng.arena_nodes ? eng.arena_nodes : initial_arena_nodes(cfg));
            const size_t overhead = Engine<NW>::per_game_overhead(cfg, p.max_turns, eng.use_queue());
            const size_t reserve = (size_t)4 << 30;  // the evaluator's buffers, arenas beyond the largest class (host-allocated)
            const size_t usable = free_b > reserve ? free_b - reserve : 0;
            const size_t per_game = 2 * fresh + overhead;
            if ((size_t)S * per_game > usable) S = (uint32_t)(usable / per_game);
            if (S == 0) return fail(AR_E_NOMEM, "not enough device memory for a single game arena");
            pool_bytes = (usable - (size_t)S * overhead) / 100 * 95;
        }

        // AR_TIMING=1 prints where the host wall time of this run went (stderr)
        timing = getenv("AR_TIMING") != nullptr;
        auto tp = std::chrono::steady_clock::now();
        auto since = [](std::chrono::steady_clock::time_point a) {
            return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count();
        };
        if (p.cache_size && net != nullptr) {
            // the reference sizes one table per worker thread (capacity x 1.9 slots, nn_cache.rs:49); one table
            // serves every game here, so it gets the threads' worth, rounded up to a power of two
            const uint64_t want = (uint64_t)((double)p.cache_size * (p.num_threads ? p.num_threads : 1) * 1.9) + 1;
            uint64_t e = 1u << 16;
            while (e < want && e < (1ULL << 26)) e <<= 1;
            eng.cache_entries = e;
        }
        if (getenv("AR_NO_POOL")) pool_bytes = 0;  // test knob: one smallest block per game, every growth goes through the host path
        if (const char* e = getenv("AR_TREE_GB"))  // test knob: a small tree region (games wait for blocks, trees move between classes)
            if (atof(e) > 0.0) pool_bytes = (size_t)(atof(e) * 1073741824.0);
        // rounds per gather launch (dev_search.h gather_machine_limited): no limit unless AR_GATHER_ROUNDS sets one
        // (0 = no limit); a limit keeps the walk on the lane kernel
        if (const char* e = getenv("AR_GATHER_ROUNDS")) eng.gather_rounds = atoi(e) > 0 ? (uint32_t)atoi(e) : 0xFFFFFFFFu;
        if (int rc = eng.setup(device, S, cfg, p.max_turns, cost, pool_bytes)) return rc;
        tm[0] = since(tp);
        {
            // groups of games pipelined against each other (Engine::group_step); AR_GROUPS overrides
            // two groups from 8192 games up (one group's evaluator runs beside the other group's tree walks: +6..18 %,
            // DESIGN.md section 7) -- when every stream can have a hardware queue of its own
            uint32_t ng = (S >= 8192u && hw_queues() >= 8) ? 2u : 1u;
            if (const char* e = getenv("AR_GROUPS"))
                if (atoi(e) >= 1 && atoi(e) <= 64) ng = (uint32_t)atoi(e);
            if (eng.cache_entries) ng = 1;  // one probe/fill pair in flight at a time: a reader never overlaps an eviction
            if (getenv("AR_NO_ADVANCE_OVERLAP")) eng.overlap_advance = false;
            if (int rc = eng.make_groups(ng)) return rc;
        }
        if (to_disk) writer.start();
        slot_game.resize(S);
        slot_busy.assign(S, 0);
        zone_busy.assign(eng.pool.zones, 0u);
        pages_per_game = 4.0 * (double)eng.pool.fresh_pages;
        t0 = std::chrono::steady_clock::now();
        tp = t0;
        std::vector<uint32_t> all(S);
        for (uint32_t i = 0; i < S; ++i) all[i] = i;
        if (int rc = refill(all)) return rc;
        tm[1] = since(tp);
        return AR_OK;
    }

    // `c` simulate_batch steps for every resident game
    int run_chunk(uint32_t c) {
        const uint32_t iters = 4;  // batches one k_step_uniform launch runs per lane before the tree reuse
        if (c / iters)
            if (int rc = eng.run_steps((int)(c / iters), (int)iters)) return rc;
        if (c % iters)
            if (int rc = eng.run_steps(1, (int)(c % iters))) return rc;
        return AR_OK;
    }

    // one finished game: stats, progress, sink, writer (SelfPlayStats::add_game, selfplay.rs:190-210)
    void account(const DoneInfo<NW>& di, const PosRec<NW>* pos) {
        const float f1 = di.final_st.s1, f2 = di.final_st.s2;
        const HostGame& hg = slot_game[di.slot];
        st.total_games += 1;
        st.total_positions += di.n_pos;
        st.total_simulations += di.t_sims;
        st.total_nn_evals += di.t_nn;
        st.total_terminals += di.t_term;
        st.total_collisions += di.t_coll;
        st.total_cheese_collected += f1 + f2;
        st.total_cheese_available += hg.total_cheese;
        if (di.n_pos < st.min_turns) st.min_turns = di.n_pos;
        if (di.n_pos > st.max_turns) st.max_turns = di.n_pos;
        if (f1 > f2) st.p1_wins += 1;
        else if (f2 > f1) st.p2_wins += 1;
        else st.draws += 1;
        st.gather_node_visits += di.nv_gather;
        st.backup_node_visits += di.nv_backup;
        st.new_nodes += di.new_nodes;
        // the game leaves the resident set: its part of the last scan's sums moves to the finished totals
        const unsigned long long part[LIVE_N] = {di.n_pos, di.t_sims, di.t_nn, di.t_term, di.t_coll, di.nv_gather,
                                                di.nv_backup, di.new_nodes, 1};
        for (int k = 0; k < LIVE_N; ++k) live[k] = live[k] >= part[k] ? live[k] - part[k] : 0;
        if (progress) {  // selfplay.rs:637-645
            __atomic_fetch_add(&progress->positions_completed, (uint64_t)di.n_pos, __ATOMIC_RELAXED);
            __atomic_fetch_add(&progress->simulations_completed, (uint64_t)di.t_sims, __ATOMIC_RELAXED);
            __atomic_fetch_add(&progress->nn_evals_completed, (uint64_t)di.t_nn, __ATOMIC_RELAXED);
            __atomic_fetch_add(&progress->games_completed, 1u, __ATOMIC_RELAXED);
        }
        if (sink || to_disk) {  // the record itself is only built for someone who wants it
            auto rec = std::make_shared<GameRecordHost>();
            record_from_device<NW>(di, pos, hg, hg.cost.empty() ? cost : hg.cost, *rec);
            if (sink) {
                ArGameRecordView v = rec->view();
                sink(sink_user, &v);
            }
            if (to_disk && rec->n > 0) writer.push(rec);
        }
    }

    // cumulative figures: finished games + what the resident games have done so far (per finished move)
    void totals(ArSelfPlayStats& o) const {
        o = st;
        o.total_positions += live[0];
        o.total_simulations += live[1];
        o.total_nn_evals += live[2];
        o.total_terminals += live[3];
        o.total_collisions += live[4];
        o.gather_node_visits += live[5];
        o.backup_node_visits += live[6];
        o.new_nodes += live[7];
        o.device_secs = eng.device_ms / 1000.0;
        o.steps = eng.steps;
        o.gather_secs = eng.gather_ms / 1000.0;
        o.gather_launches = eng.gather_launches;
    }
    int read_cache_counters(ArSelfPlayStats& o) {
        if (!eng.cache_entries) return AR_OK;
        unsigned long long hm[2] = {0, 0};
        HIP_TRY(hipMemcpy(hm, eng.cache_counters.p, sizeof hm, hipMemcpyDeviceToHost));
        o.cache_hits = hm[0];
        o.cache_misses = hm[1];
        return AR_OK;
    }

    int step(uint32_t batch_steps, ArSelfPlayStats* window, int* finished_out) override {
        if (failed) return fail(AR_E_INVALID, "the session has failed earlier; close it");
        if (unbounded && batch_steps == 0xFFFFFFFFu)
            return fail(AR_E_INVALID, "a session with an endless supply of games cannot be run to its end: pass a number of batch steps");
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto since = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(now() - a).count(); };
        const auto w0 = now();
        ArSelfPlayStats before;
        totals(before);
        if (int rc = read_cache_counters(before)) return rc;
        uint32_t win_min = 0xFFFFFFFFu, win_max = 0;
        const ArSelfPlayStats st_before = st;
        int rc = AR_OK;
        // steps between host visits: a game needs ~n_sims/batch steps per move, so a few dozen steps of
        // latency on refills and arena growth costs little
        const uint32_t visit_every = 32;
        uint64_t left = batch_steps;
        while (S > 0 && !all_finished() && left > 0) {
            const uint32_t chunk = left < visit_every ? (uint32_t)left : visit_every;
            if (batch_steps != 0xFFFFFFFFu) left -= chunk;
            auto tp = now();
            if ((rc = run_chunk(chunk)) != AR_OK) break;
            tm[2] += since(tp);
            uint32_t c[4];
            if ((rc = eng.visit(c, true, &tm[3])) != AR_OK) break;  // (tm[3] scan-wait, tm[4] grow)
            for (int k = 0; k < LIVE_N; ++k) live[k] = eng.h_live.p[k];
            if (eng.h_live.p[13] >= 256)  // tree pages of a game that has played a few moves, in this run
                pages_per_game = std::max((double)eng.pool.fresh_pages, 1.1 * (double)eng.h_live.p[12] / (double)eng.h_live.p[13]);
            tp = now();
            if (c[0]) {
                const uint32_t n_done = c[0];
                if ((rc = eng.drain(n_done)) != AR_OK) break;
                if (rows && (rc = rows_append_done<NW>(*rows, eng.h_info.p, eng.info.p, eng.staging.p, n_done, eng.max_turns,
                                                       eng.slots.p, eng.maze.p, eng.stream)) != AR_OK)
                    break;
                tm[5] += since(tp);
                tp = now();
                std::vector<uint32_t> free_slots;
                for (uint32_t d = 0; d < n_done; ++d) {
                    const DoneInfo<NW>& di = eng.h_info.p[d];
                    account(di, eng.h_staging.p + (size_t)d * p.max_turns);
                    if (di.n_pos < win_min) win_min = di.n_pos;
                    if (di.n_pos > win_max) win_max = di.n_pos;
                    free_slots.push_back(di.slot);
                    leave_slot(di.slot);
                    ++finished;
                }
                tm[6] += since(tp);
                tp = now();
                if ((rc = refill(free_slots)) != AR_OK) break;
                tm[7] += since(tp);
            } else if (!idle_slots.empty() && supply_left()) {
                if ((rc = refill(std::vector<uint32_t>())) != AR_OK) break;  // (slots that waited for room in their zone)
            }
            if (c[0] == 0 && c[1] == 0 && c[2] == 0 && !all_finished() && !supply_left()) {
                rc = fail(AR_E_DEVICE, "self-play stalled: no active games left but not all games finished");
                break;
            }
        }
        if (rc != AR_OK) failed = true;
        if (window) {
            ArSelfPlayStats a;
            totals(a);
            if (rc == AR_OK) rc = read_cache_counters(a);
            ArSelfPlayStats& w = *window;
            memset(&w, 0, sizeof w);
            w.total_games = a.total_games - before.total_games;
            w.total_positions = a.total_positions - before.total_positions;
            w.total_simulations = a.total_simulations - before.total_simulations;
            w.total_nn_evals = a.total_nn_evals - before.total_nn_evals;
            w.total_terminals = a.total_terminals - before.total_terminals;
            w.total_collisions = a.total_collisions - before.total_collisions;
            w.gather_node_visits = a.gather_node_visits - before.gather_node_visits;
            w.backup_node_visits = a.backup_node_visits - before.backup_node_visits;
            w.new_nodes = a.new_nodes - before.new_nodes;
            w.p1_wins = st.p1_wins - st_before.p1_wins;
            w.p2_wins = st.p2_wins - st_before.p2_wins;
            w.draws = st.draws - st_before.draws;
            w.total_cheese_collected = st.total_cheese_collected - st_before.total_cheese_collected;
            w.total_cheese_available = st.total_cheese_available - st_before.total_cheese_available;
            w.min_turns = w.total_games ? win_min : 0;
            w.max_turns = win_max;
            w.cache_hits = a.cache_hits - before.cache_hits;
            w.cache_misses = a.cache_misses - before.cache_misses;
            w.device_secs = a.device_secs - before.device_secs;
            w.steps = a.steps - before.steps;
            w.gather_secs = a.gather_secs - before.gather_secs;
            w.gather_launches = a.gather_launches - before.gather_launches;
            w.elapsed_secs = since(w0);
        }
        if (finished_out) *finished_out = (S == 0 || all_finished()) ? 1 : 0;
        return rc;
    }

    // Ends the run: bundles flushed, totals of the FINISHED games returned (an unbounded session that is
    // closed with games in flight simply drops them, like a sampler that is interrupted).
    int close(ArSelfPlayStats* total) override {
        int rc = AR_OK;
        if (rows) {  // the row set is the caller's again (its appends are done: it may be attached to the next session)
            if (eng.stream) (void)hipStreamSynchronize(eng.stream);
            rows->attached = false;
            rows = nullptr;
        }
        if (to_disk) {
            writer.finish();
            to_disk = false;
            if (!writer.error.empty()) rc = fail(AR_E_IO, writer.error);
        }
        ArSelfPlayStats o = st;
        o.elapsed_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (o.total_games == 0) o.min_turns = 0;
        o.device_secs = eng.device_ms / 1000.0;
        o.steps = eng.steps;
        o.gather_secs = eng.gather_ms / 1000.0;
        o.gather_launches = eng.gather_launches;
        if (S > 0 && rc == AR_OK) rc = read_cache_counters(o);
        if (timing)
            fprintf(stderr,
                    "[ar timing] games=%llu resident=%u wall=%.3fs device=%.3fs | setup %.3f first-fill %.3f launch %.3f "
                    "scan-wait %.3f grow %.3f (%llu) drain %.3f records %.3f refill %.3f | tree region %.1f GB, least left "
                    "%.1f GB\n",
                    (unsigned long long)finished, S, o.elapsed_secs, o.device_secs, tm[0], tm[1], tm[2], tm[3], tm[4],
                    (unsigned long long)eng.grows, tm[5], tm[6], tm[7], (double)eng.region_bytes / 1073741824.0,
                    eng.region_low_mb == 0xFFFFFFFFu ? -1.0 : (double)eng.region_low_mb / 1024.0);
        if (total) *total = o;
        return rc;
    }
};

// ------------------------------------------------------------------------------------------------
// single searches
// ------------------------------------------------------------------------------------------------
bool host_game_from_spec(const ArGameSpec& g, HostGame& h, std::vector<uint8_t>& cost, std::string& err) {
    const int hw = g.width * g.height;
    if (g.width == 0 || g.height == 0 || hw > 256) {
        err = "board must have 1..256 cells";
        return false;
    }
    if (g.p1_x >= g.width || g.p2_x >= g.width || g.p1_y >= g.height || g.p2_y >= g.height) {
        err = "player position outside the board";
        return false;
    }
    if (!g.cheese) {
        err = "cheese mask is required";
        return false;
    }
    h.width = g.width;
    h.height = g.height;
    h.max_turns = g.max_turns;
    h.turn = g.turn;
    h.p1 = (uint8_t)(g.p1_y * g.width + g.p1_x);
    h.p2 = (uint8_t)(g.p2_y * g.width + g.p2_x);
    h.m1 = g.p1_mud;
    h.m2 = g.p2_mud;
    h.s1 = g.p1_score;
    h.s2 = g.p2_score;
    h.cheese.assign(g.cheese, g.cheese + hw);
    uint32_t rem = 0;
    for (int i = 0; i < hw; ++i) rem += h.cheese[i] ? 1 : 0;
    h.total_cheese = (uint16_t)(g.p1_score + g.p2_score + (float)rem);
    if (g.cost) cost.assign(g.cost, g.cost + (size_t)hw * 4);
    else cost = open_maze_cost(g.width, g.height);
    return true;
}

void fill_result(const MoveResult& m, ArSearchResult* o) {
    memcpy(o->policy_p1, m.policy[0], 20);
    memcpy(o->policy_p2, m.policy[1], 20);
    o->value_p1 = m.value[0];
    o->value_p2 = m.value[1];
    memcpy(o->visit_counts_p1, m.visit_counts[0], 20);
    memcpy(o->visit_counts_p2, m.visit_counts[1], 20);
    memcpy(o->prior_p1, m.prior[0], 20);
    memcpy(o->prior_p2, m.prior[1], 20);
    o->total_visits = m.total_visits;
    o->nn_evals = m.nn_evals;
    o->terminals = m.terminals;
    o->collisions = m.collisions;
}

template <int NW>
int search_impl(const ArGameSpec* games, uint32_t n, const SearchCfg& cfg, const uint64_t* seeds,
                ArPredictFn predict_fn, void* user, ArNet* net, int device, ArSearchResult* out) {
    std::string err;
    std::vector<HostGame> hg(n);
    std::vector<uint8_t> mazes;
    std::vector<uint32_t> maze_off(n);
    uint16_t max_turns = 1;
    for (uint32_t i = 0; i < n; ++i) {
        std::vector<uint8_t> c;
        if (!host_game_from_spec(games[i], hg[i], c, err)) return fail(AR_E_INVALID, err);
        maze_off[i] = (uint32_t)mazes.size();
        mazes.insert(mazes.end(), c.begin(), c.end());
        if (hg[i].max_turns > max_turns) max_turns = hg[i].max_turns;
    }
    Engine<NW> eng;
    eng.configure(net, n, 0u, /*arena_knob=*/false, /*host_eval=*/predict_fn != nullptr);
    if (eng.net != nullptr)
        for (uint32_t i = 0; i < n; ++i)
            if (games[i].width != net->dev.width || games[i].height != net->dev.height)
                return fail(AR_E_INVALID, "game size does not match the network's board size");
    if (int rc = eng.setup(device, n, cfg, max_turns, mazes)) return rc;
    std::vector<GameInit<NW>> inits(n);
    for (uint32_t i = 0; i < n; ++i) {
        inits[i] = game_init<NW>(hg[i], i, i, maze_off[i]);
        inits[i].rng_seed = seeds ? seeds[i] : entropy_seed();
        inits[i].single = 1;
    }
    if (int rc = eng.start_games(inits)) return rc;

    if (predict_fn) {
        // host evaluator per leaf batch (PyCallbackBackend, bindings.rs:119-161); n == 1
        DevBuf<State<NW>> d_leaves;
        DevBuf<EvalOut> d_ev;
        DevBuf<uint32_t> d_n;
        HIP_TRY(d_leaves.alloc(cfg.batch_size));
        HIP_TRY(d_ev.alloc(cfg.batch_size));
        HIP_TRY(d_n.alloc(1));
        std::vector<State<NW>> leaves(cfg.batch_size);
        std::vector<ArLeaf> al(cfg.batch_size);
        std::vector<EvalOut> ev(cfg.batch_size);
        std::vector<float> pp1(cfg.batch_size * 5), pp2(cfg.batch_size * 5), pv1(cfg.batch_size), pv2(cfg.batch_size);
        const int w = hg[0].width;
        for (;;) {
            uint32_t c[4];
            if (int rc = eng.visit(c)) return rc;
            if (c[1]) continue;
            if (c[2] == 0) break;
            eng.launch_gather(false);
            hipLaunchKernelGGL(k_export_leaves<NW>, dim3(1), dim3(64), 0, eng.stream, eng.slots.p, 0u, eng.bases(),
                               d_leaves.p, d_n.p);
            uint32_t nl = 0;
            HIP_TRY(hipMemcpyAsync(&nl, d_n.p, 4, hipMemcpyDeviceToHost, eng.stream));
            HIP_TRY(hipMemcpyAsync(leaves.data(), d_leaves.p, sizeof(State<NW>) * cfg.batch_size, hipMemcpyDeviceToHost,
                                   eng.stream));
            HIP_TRY(hipStreamSynchronize(eng.stream));
            if (nl > 0) {
                for (uint32_t j = 0; j < nl; ++j) {
                    const State<NW>& s = leaves[j];
                    ArLeaf& a = al[j];
                    memset(&a, 0, sizeof a);
                    a.p1_x = s.p1 % w;
                    a.p1_y = s.p1 / w;
                    a.p2_x = s.p2 % w;
                    a.p2_y = s.p2 / w;
                    a.p1_mud = s.m1;
                    a.p2_mud = s.m2;
                    a.turn = s.turn;
                    a.p1_score = s.s1;
                    a.p2_score = s.s2;
                    for (int k = 0; k < NW; ++k) a.cheese_bits[k] = s.cheese[k];
                }
                if (predict_fn(user, al.data(), nl, pp1.data(), pp2.data(), pv1.data(), pv2.data()) != 0) {
                    eng.launch_cancel();
                    hipStreamSynchronize(eng.stream);
                    return fail(AR_E_BACKEND, "predict_fn raised an exception");
                }
                for (uint32_t j = 0; j < nl; ++j) {
                    memcpy(ev[j].p1, &pp1[j * 5], 20);
                    memcpy(ev[j].p2, &pp2[j * 5], 20);
                    ev[j].v1 = pv1[j];
                    ev[j].v2 = pv2[j];
                }
                HIP_TRY(hipMemcpyAsync(d_ev.p, ev.data(), sizeof(EvalOut) * nl, hipMemcpyHostToDevice, eng.stream));
                hipLaunchKernelGGL(k_import_evals<NW>, dim3(1), dim3(64), 0, eng.stream, eng.slots.p, 0u, eng.bases(),
                                   d_ev.p, nl);
            }
            eng.launch_backup(false);
            HIP_TRY(hipGetLastError());
        }
    } else {
        for (;;) {
            if (int rc = eng.run_steps(4, 8)) return rc;
            uint32_t c[4];
            if (int rc = eng.visit(c)) return rc;
            if (c[2] == 0 && c[1] == 0) break;
        }
    }
    uint32_t c[4];
    if (int rc = eng.scan(c)) return rc;
    if (c[0] != n) return fail(AR_E_DEVICE, "search ended with unfinished slots");
    if (int rc = eng.drain(n)) return rc;
    for (uint32_t d = 0; d < n; ++d) fill_result(eng.h_info.p[d].last, &out[eng.h_info.p[d].game_index]);
    return AR_OK;
}

// ------------------------------------------------------------------------------------------------
// head-to-head matches
// ------------------------------------------------------------------------------------------------
struct MatchSideHost {  // owning twin of ArMatchSearchView
    std::vector<float> po1, po2, v1, v2, vc1, vc2, pr1, pr2;
    std::vector<uint32_t> tv, nn, term, coll;
    void resize(size_t n) {
        for (auto* v : {&po1, &po2, &vc1, &vc2, &pr1, &pr2}) v->resize(n * 5);
        v1.resize(n);
        v2.resize(n);
        for (auto* v : {&tv, &nn, &term, &coll}) v->resize(n);
    }
    void set(size_t i, const MoveResult& m) {
        memcpy(&po1[i * 5], m.policy[0], 20);
        memcpy(&po2[i * 5], m.policy[1], 20);
        v1[i] = m.value[0];
        v2[i] = m.value[1];
        memcpy(&vc1[i * 5], m.visit_counts[0], 20);
        memcpy(&vc2[i * 5], m.visit_counts[1], 20);
        memcpy(&pr1[i * 5], m.prior[0], 20);
        memcpy(&pr2[i * 5], m.prior[1], 20);
        tv[i] = m.total_visits;
        nn[i] = m.nn_evals;
        term[i] = m.terminals;
        coll[i] = m.collisions;
    }
    ArMatchSearchView view() const {
        ArMatchSearchView v;
        v.policy_p1 = po1.data();
        v.policy_p2 = po2.data();
        v.value_p1 = v1.data();
        v.value_p2 = v2.data();
        v.visit_counts_p1 = vc1.data();
        v.visit_counts_p2 = vc2.data();
        v.prior_p1 = pr1.data();
        v.prior_p2 = pr2.data();
        v.total_visits = tv.data();
        v.nn_evals = nn.data();
        v.terminals = term.data();
        v.collisions = coll.data();
        return v;
    }
};

// The match driver: tournament.py:329-373 (one game per worker) and eval/game.py:47-87 (the turn loop) for every
// resident game at once. Every agent that searches has an engine; two engines hold the same game in the same slot number
// and each runs its own step pipeline on its own stream (no side streams: two streams in all, what a self-play session
// of one group uses), so one agent's evaluator runs beside the other's tree walk. An agent that does not search
// (ArMatchAgent::kind random / greedy) has no engine: no slots, no arenas, no leaf queue, no network. After every step of
// the engines, k_match_greedy and k_match_move_agents (on the match's stream: A's, else B's, else one of its own; behind
// an event of B's when both search) move the games in which every searching agent's search is complete, and each engine's
// re-rooting kernel gives the re-armed slots their fresh roots. The host visits every few steps, as in self-play: stalls,
// finished games, refills.
template <int NW>
struct MatchRun {
    ArMatchParams p;
    SearchCfg cfg_a, cfg_b;
    Engine<NW> ea, eb;  // set up only for an agent that searches (has_a / has_b)
    bool has_a = true, has_b = true;
    AgentDesc da, db;
    hipStream_t own_stream = nullptr, ms = nullptr;  // ms: the stream the match's own kernels run on
    GameSupply supply;
    std::vector<uint8_t> cost;
    uint32_t S = 0;
    uint64_t seed_a = 0, seed_b = 0;
    DevBuf<MatchGame<NW>> games, info;
    DevBuf<MatchPos<NW>> recs, staging;
    DevBuf<MatchAux<NW>> aux;
    DevBuf<MatchAuxInit<NW>> init;
    DevBuf<uint8_t> maze, maze_stage;  // the match's own maze pool: one entry, or one per slot for generated mazes
    uint32_t maze_stride = 0;
    DevBuf<uint32_t> counts, done_list;
    PinBuf<uint32_t> h_counts;
    PinBuf<MatchGame<NW>> h_info;
    PinBuf<MatchPos<NW>> h_staging;
    hipEvent_t ev_b = nullptr, ev_m = nullptr;
    ArMatchSink sink = nullptr;
    void* sink_user = nullptr;
    ArMatchStats st;
    uint32_t next_game = 0, finished = 0;
    std::string err;

    ~MatchRun() {
        if (ea.stream) hipStreamSynchronize(ea.stream);
        if (eb.stream) hipStreamSynchronize(eb.stream);
        if (own_stream) {
            hipStreamSynchronize(own_stream);
            hipStreamDestroy(own_stream);
        }
        if (ev_b) hipEventDestroy(ev_b);
        if (ev_m) hipEventDestroy(ev_m);
    }

    int setup_engine(Engine<NW>& e, const SearchCfg& cfg, ArNet* net, int device) {
        e.configure(net, S, supply.gen_maze ? (uint32_t)supply.hw : 0u);
        e.overlap_advance = false;  // one stream per engine: every hand-off is in stream order (phase 0)
        return e.setup(device, S, cfg, p.max_turns, cost);
    }

    int open(const ArMatchParams& params, const GameSupply& match_games, int device, ArNet* net_a, ArNet* net_b, ArMatchSink sk,
             void* sk_user) {
        p = params;
        supply = match_games;
        sink = sk;
        sink_user = sk_user;
        memset(&st, 0, sizeof st);
        has_a = p.a.kind == AR_AGENT_SEARCH;
        has_b = p.b.kind == AR_AGENT_SEARCH;
        cfg_a = to_cfg(p.a.search, has_a ? p.a.simulations : 0u, has_a ? p.a.batch_size : 1u);
        cfg_b = to_cfg(p.b.search, has_b ? p.b.simulations : 0u, has_b ? p.b.batch_size : 1u);
        da = AgentDesc{p.a.kind, p.a.temperature, cfg_a.n_sims, 0u};
        db = AgentDesc{p.b.kind, p.b.temperature, cfg_b.n_sims, 0u};
        cost = open_maze_cost(p.width, p.height);
        seed_a = p.has_seed ? p.a.rng_seed_base : entropy_seed();
        seed_b = p.has_seed ? p.b.rng_seed_base : entropy_seed();
        const int hw = supply.hw;
        const bool gen_maze = supply.gen_maze;
        p.maze_type = p.positions = p.device = p.a.weights_path = p.b.weights_path = nullptr;  // caller-owned strings

        S = p.concurrent_games ? p.concurrent_games : 4096u;
        if (S > p.num_games) S = p.num_games;
        if (S == 0) return AR_OK;
        {
            // what a resident game takes on the device: per agent a fresh tree (with the region's slack) and the slot's
            // scratch and queue share, plus its match records
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipSetDevice(device));
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            free_b += arena_cached_bytes(device);
            size_t per_game = 2 * sizeof(MatchPos<NW>) * p.max_turns + 2 * sizeof(MatchGame<NW>) + sizeof(MatchAux<NW>) +
                              sizeof(MatchAuxInit<NW>) + 2 * (size_t)hw * 4;
            if (has_a) per_game += arena_bytes(initial_arena_nodes(cfg_a)) * 5 / 4 + Engine<NW>::per_game_overhead(cfg_a, p.max_turns, true);
            if (has_b) per_game += arena_bytes(initial_arena_nodes(cfg_b)) * 5 / 4 + Engine<NW>::per_game_overhead(cfg_b, p.max_turns, true);
            const size_t reserve = (size_t)4 << 30;
            const size_t usable = free_b > reserve ? free_b - reserve : 0;
            if ((size_t)S * per_game > usable) S = (uint32_t)(usable / per_game);
            if (S == 0) return fail(AR_E_NOMEM, "not enough device memory for a single match game");
        }
        if (has_a)
            if (int rc = setup_engine(ea, cfg_a, net_a, device)) return rc;
        if (has_b)
            if (int rc = setup_engine(eb, cfg_b, net_b, device)) return rc;
        if (!has_a && !has_b) HIP_TRY(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
        ms = has_a ? ea.stream : has_b ? eb.stream : own_stream;
        maze_stride = gen_maze ? (uint32_t)hw * 4u : 0u;
        HIP_TRY(maze.alloc(gen_maze ? (size_t)S * maze_stride : cost.size()));
        if (gen_maze) HIP_TRY(maze_stage.alloc((size_t)S * maze_stride));
        else HIP_TRY(hipMemcpy(maze.p, cost.data(), cost.size(), hipMemcpyHostToDevice));
        HIP_TRY(aux.alloc(S));
        HIP_TRY(hipMemset(aux.p, 0, sizeof(MatchAux<NW>) * S));
        HIP_TRY(hipEventCreateWithFlags(&ev_b, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_m, hipEventDisableTiming));
        const size_t mt = p.max_turns > 0 ? p.max_turns : 1;
        HIP_TRY(games.alloc(S));
        HIP_TRY(hipMemset(games.p, 0, sizeof(MatchGame<NW>) * S));
        HIP_TRY(info.alloc(S));
        HIP_TRY(recs.alloc((size_t)S * mt));
        HIP_TRY(staging.alloc((size_t)S * mt));
        HIP_TRY(init.alloc(S));
        HIP_TRY(counts.alloc(8));
        HIP_TRY(done_list.alloc(S));
        HIP_TRY(h_counts.alloc(8));
        HIP_TRY(h_info.alloc(S));
        HIP_TRY(h_staging.alloc((size_t)S * mt));
        std::vector<uint32_t> all(S);
        for (uint32_t i = 0; i < S; ++i) all[i] = i;
        return refill(all);
    }

    int refill(const std::vector<uint32_t>& free_slots) {
        std::vector<GameInit<NW>> ia, ib;
        std::vector<MatchAuxInit<NW>> mi;
        std::vector<uint8_t> mazes;
        for (uint32_t sl : free_slots) {
            if (next_game >= p.num_games) break;
            const uint32_t index = supply.index(next_game);
            HostGame g;
            if (!supply.make_game(index, g, err)) return fail(AR_E_INVALID, err);
            GameInit<NW> gi = game_init<NW>(g, sl, index, sl * maze_stride);
            mazes.insert(mazes.end(), g.cost.begin(), g.cost.end());
            gi.single = 1;  // the search stops in SLOT_DONE; the move is the match's
            gi.rng_seed = seed_a + index;
            ia.push_back(gi);
            gi.rng_seed = seed_b + index;
            ib.push_back(gi);
            MatchAuxInit<NW> m;
            memset(&m, 0, sizeof m);
            m.slot = sl;
            m.game_index = index;
            m.a_is_p1 = (p.swap_sides && (index & 1u)) ? 0u : 1u;  // tournament.py:397
            m.board = gi.board;
            m.st = gi.st;
            m.seed_a = seed_a + index;
            m.seed_b = seed_b + index;
            mi.push_back(m);
            ++next_game;
        }
        if (mi.empty()) return AR_OK;
        if (has_a)
            if (int rc = ea.start_games(ia, supply.gen_maze ? &mazes : nullptr)) return rc;
        if (has_b)
            if (int rc = eb.start_games(ib, supply.gen_maze ? &mazes : nullptr)) return rc;
        // (the engines' streams are at rest: start_games waits for its kernel)
        HIP_TRY(hipMemcpyAsync(init.p, mi.data(), sizeof(MatchAuxInit<NW>) * mi.size(), hipMemcpyHostToDevice, ms));
        if (supply.gen_maze) HIP_TRY(hipMemcpyAsync(maze_stage.p, mazes.data(), mazes.size(), hipMemcpyHostToDevice, ms));
        hipLaunchKernelGGL(k_match_init_agents<NW>, dim3((uint32_t)mi.size()), dim3(64), 0, ms, games.p, aux.p, slots_a(), slots_b(),
                           (const MatchAuxInit<NW>*)init.p, (uint32_t)mi.size(), (const uint8_t*)maze_stage.p, maze.p, maze_stride);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ms));
        return AR_OK;
    }

    Slot<NW>* slots_a() { return has_a ? ea.slots.p : nullptr; }
    Slot<NW>* slots_b() { return has_b ? eb.slots.p : nullptr; }
    static uint32_t grid(uint32_t n) { return (n + 63) / 64; }

    // one simulate_batch step of every searching agent, then the moves of the games whose searches are complete (with no
    // searching agent: one move of every resident game)
    int tick() {
        if (has_a)
            if (int rc = ea.run_steps(1, 1)) return rc;
        if (has_b)
            if (int rc = eb.run_steps(1, 1)) return rc;
        if (has_a && has_b) {
            HIP_TRY(hipEventRecord(ev_b, eb.stream));
            HIP_TRY(hipStreamWaitEvent(ea.stream, ev_b, 0));
        }
        if (da.kind == AGENT_GREEDY || db.kind == AGENT_GREEDY)
            hipLaunchKernelGGL(k_match_greedy<NW>, dim3(S), dim3(64), 0, ms, (const Slot<NW>*)slots_a(), (const Slot<NW>*)slots_b(),
                               games.p, aux.p, S, (const uint8_t*)maze.p, da.kind, db.kind);
        hipLaunchKernelGGL(k_match_move_agents<NW>, dim3(grid(S)), dim3(64), 0, ms, slots_a(), slots_b(), games.p, aux.p, recs.p, S,
                           (uint32_t)p.max_turns, (const uint8_t*)maze.p, da, db);
        HIP_TRY(hipGetLastError());
        if (has_a && has_b) {
            HIP_TRY(hipEventRecord(ev_m, ea.stream));
            HIP_TRY(hipStreamWaitEvent(eb.stream, ev_m, 0));  // B's stream leaves its slots alone until the moves are made
        }
        if (has_a) ea.launch_advance();
        if (has_b) eb.launch_advance();
        HIP_TRY(hipGetLastError());
        return AR_OK;
    }

    void account(const MatchGame<NW>& g, const MatchPos<NW>* pos) {
        const float f1 = g.final_st.s1, f2 = g.final_st.s2;
        const uint8_t result = f1 > f2 ? 1 : f2 > f1 ? 2 : 0;
        st.total_games += 1;
        st.total_positions += g.n_pos;
        if (result == 0) st.draws += 1;
        else if ((result == 1) == (g.a_is_p1 != 0)) st.wins_a += 1;
        else st.wins_b += 1;
        st.cheese_a += g.a_is_p1 ? f1 : f2;
        st.cheese_b += g.a_is_p1 ? f2 : f1;
        const size_t n = g.n_pos;
        for (size_t i = 0; i < n; ++i) {
            st.simulations_a += pos[i].a.total_visits;
            st.simulations_b += pos[i].b.total_visits;
            st.nn_evals_a += pos[i].a.nn_evals;
            st.nn_evals_b += pos[i].b.nn_evals;
            st.terminals_a += pos[i].a.terminals;
            st.terminals_b += pos[i].b.terminals;
            st.collisions_a += pos[i].a.collisions;
            st.collisions_b += pos[i].b.collisions;
        }
        if (!sink) return;
        PosColumns col;
        col.resize(n, supply.hw);
        MatchSideHost sa, sb;
        sa.resize(n);
        sb.resize(n);
        for (size_t i = 0; i < n; ++i) {
            const MatchPos<NW>& q = pos[i];
            col.set(i, q.st, q.a1, q.a2, p.width, supply.hw);
            sa.set(i, q.a);
            sb.set(i, q.b);
        }
        ArMatchGameView v;
        memset(&v, 0, sizeof v);
        v.width = p.width;
        v.height = p.height;
        v.max_turns = p.max_turns;
        v.game_index = g.game_index;
        v.n_positions = g.n_pos;
        v.a_is_p1 = (uint8_t)g.a_is_p1;
        v.result = result;
        v.final_p1_score = f1;
        v.final_p2_score = f2;
        col.point(v);
        v.a = sa.view();
        v.b = sb.view();
        sink(sink_user, &v);
    }

    // stalls, finished games, refills: everything the host does between two runs of ticks
    int visit() {
        uint32_t ca[4] = {0, 0, 0, 0}, cb[4] = {0, 0, 0, 0};
        if (has_a)
            if (int rc = ea.visit(ca, true)) return rc;
        if (has_b)
            if (int rc = eb.visit(cb, true)) return rc;
        HIP_TRY(hipMemsetAsync(counts.p, 0, 32, ms));
        hipLaunchKernelGGL(k_match_scan<NW>, dim3(grid(S)), dim3(64), 0, ms, (const MatchGame<NW>*)games.p, S, counts.p,
                           done_list.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_counts.p, counts.p, 32, hipMemcpyDeviceToHost, ms));
        HIP_TRY(hipStreamSynchronize(ms));
        const uint32_t n_done = h_counts.p[0], playing = h_counts.p[1];
        if (h_counts.p[2])
            return fail(AR_E_DEVICE, "a match game recorded more positions than max_turns, or a greedy move ran past its bound");
        if (n_done) {
            const size_t mt = p.max_turns > 0 ? p.max_turns : 1;
            hipLaunchKernelGGL(k_match_pack<NW>, dim3(n_done), dim3(128), 0, ms, games.p, (const uint32_t*)done_list.p, n_done,
                               info.p, (const MatchPos<NW>*)recs.p, staging.p, (uint32_t)p.max_turns);
            if (has_a)
                hipLaunchKernelGGL(k_match_release<NW>, dim3(grid(n_done)), dim3(64), 0, ea.stream, ea.slots.p,
                                   (const uint32_t*)done_list.p, n_done, ea.bases());
            if (has_b)
                hipLaunchKernelGGL(k_match_release<NW>, dim3(grid(n_done)), dim3(64), 0, eb.stream, eb.slots.p,
                                   (const uint32_t*)done_list.p, n_done, eb.bases());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_info.p, info.p, sizeof(MatchGame<NW>) * n_done, hipMemcpyDeviceToHost, ms));
            HIP_TRY(hipMemcpyAsync(h_staging.p, staging.p, sizeof(MatchPos<NW>) * (size_t)n_done * mt, hipMemcpyDeviceToHost, ms));
            HIP_TRY(hipStreamSynchronize(ms));
            if (has_b) HIP_TRY(hipStreamSynchronize(eb.stream));
            std::vector<uint32_t> free_slots;
            for (uint32_t d = 0; d < n_done; ++d) {
                account(h_info.p[d], h_staging.p + (size_t)d * mt);
                free_slots.push_back(h_info.p[d].pad[0]);
                ++finished;
            }
            if (int rc = refill(free_slots)) return rc;
        } else if (playing == 0 && finished < p.num_games) {
            return fail(AR_E_DEVICE, "match stalled: no game is being played but not all games are finished");
        }
        return AR_OK;
    }

    int run(ArMatchStats* out) {
        const auto t0 = std::chrono::steady_clock::now();
        // steps between host visits: a move takes n_sims / batch_size steps of the slower agent, so a visit every few
        // moves costs little and keeps refills timely
        const uint32_t visit_every = 16;
        // (bug guard: every batch step of a search produces at least one simulation, so a generation of games is over
        // after max_turns moves of at most n_sims steps each; stalls and refills wait for a visit -- four times that)
        const uint64_t per_generation = ((uint64_t)p.max_turns + 1) * ((uint64_t)std::max(cfg_a.n_sims, cfg_b.n_sims) + visit_every) * 4;
        const uint64_t max_ticks = S ? ((uint64_t)p.num_games / S + 2) * per_generation : 0;
        uint64_t ticks = 0;
        while (S > 0 && finished < p.num_games) {
            for (uint32_t k = 0; k < visit_every; ++k)
                if (int rc = tick()) return rc;
            if (int rc = visit()) return rc;
            ticks += visit_every;
            if (ticks > max_ticks) return fail(AR_E_DEVICE, "match made no progress: games left unfinished after every step they could need");
        }
        st.elapsed_secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *out = st;
        return AR_OK;
    }
};

template <int NW>
int match_impl(const ArMatchParams& p, const GameSupply& games, int dev, ArNet* net_a, ArNet* net_b, ArMatchSink sink, void* user,
               ArMatchStats* out) {
    MatchRun<NW> run;  // (destroyed before the caller frees the evaluators: ~Engine synchronises its streams)
    if (int rc = run.open(p, games, dev, net_a, net_b, sink, user)) return rc;
    return run.run(out);
}

// the reference fails on the ONNX input shape when the model was trained for another board (`who`: "" or "agent A: ")
int check_net_board(const ArNet* net, int width, int height, const std::string& who = "") {
    if (net->dev.width == width && net->dev.height == height) return AR_OK;
    return fail(AR_E_INVALID, who + "the network was built for a " + std::to_string(net->dev.width) + "x" +
                                  std::to_string(net->dev.height) + " board, the games are " + std::to_string(width) + "x" +
                                  std::to_string(height));
}

}  // namespace

// the evaluator must outlive the engine's streams: the session is destroyed first, then the net
struct ArSelfPlaySession {
    SessionBase* impl = nullptr;
    ArNet* net = nullptr;
    ~ArSelfPlaySession() {
        delete impl;
        if (net) ar_net_free(net);
    }
};

struct ArRowSet {
    RowStore* impl = nullptr;
    ~ArRowSet() { delete impl; }
};

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* ar_version(void) { return "alpharat_hip 0.1.0 (gfx950)"; }

size_t ar_last_error(char* buf, size_t cap) {
    if (buf && cap) {
        size_t n = g_error.size() < cap - 1 ? g_error.size() : cap - 1;
        memcpy(buf, g_error.data(), n);
        buf[n] = 0;
    }
    return g_error.size();
}

int ar_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return fail(AR_E_DEVICE, "hipGetDeviceCount failed (no HIP device?)");
    return n;
}

// ---- game generation, host only (no device needed): what ar_selfplay_run draws for game `seed` ----------
int ar_generate_maze(uint8_t width, uint8_t height, float wall_density, float mud_density, int symmetric, uint64_t seed,
                     uint8_t* cost_out) {
    if (!cost_out || width == 0 || height == 0 || (int)width * height > 256) return fail(AR_E_INVALID, "bad board");
    const std::vector<uint8_t> c = generate_maze(width, height, wall_density, mud_density, symmetric != 0, seed);
    memcpy(cost_out, c.data(), c.size());
    return AR_OK;
}
int ar_generate_cheese(uint8_t width, uint8_t height, uint8_t p1_cell, uint8_t p2_cell, uint16_t count, int symmetric,
                       uint64_t seed, uint8_t* cheese_out) {
    if (!cheese_out || width == 0 || height == 0 || (int)width * height > 256) return fail(AR_E_INVALID, "bad board");
    HostGame g;
    g.width = width;
    g.height = height;
    g.p1 = p1_cell;
    g.p2 = p2_cell;
    std::string err;
    if (!place_cheese(g, count, symmetric != 0, seed, err)) return fail(AR_E_INVALID, err);
    memcpy(cheese_out, g.cheese.data(), g.cheese.size());
    return AR_OK;
}

// Test entry (not in the public header): re-roots `n` made-up trees in one launch with the routine k_advance uses.
// records: all trees' node records back to back, tree t being nodes [first[t], first[t] + hi[t]); keep_root[t] is the
// node to keep; moves[t] != 0: the kept tree is written to a second buffer (which starts out as bytes of 0xEE), else in
// place. fast_nodes: the fast path's limit as AR_ADV_NODES sets it (0xFFFFFFFF: the default). Out: both buffers
// (in_place_out, moved_out: as many records as came in) and the kept count per tree.
int ar_debug_advance(const void* records, uint64_t n_records, const uint32_t* first, const uint32_t* hi, const uint32_t* keep_root,
                     const uint32_t* moves, uint32_t n, uint32_t fast_nodes, void* in_place_out, void* moved_out, uint32_t* counts_out) {
    if (!records || !first || !hi || !keep_root || !moves || !in_place_out || !moved_out || !counts_out || n == 0 || n_records == 0)
        return fail(AR_E_INVALID, "ar_debug_advance: null argument");
    std::vector<DbgAdvTree> trees(n);
    for (uint32_t t = 0; t < n; ++t) {
        if (hi[t] == 0 || keep_root[t] >= hi[t] || (uint64_t)first[t] + hi[t] > n_records) return fail(AR_E_INVALID, "ar_debug_advance: bad tree");
        trees[t] = DbgAdvTree{first[t], hi[t], keep_root[t], moves[t]};
    }
    const size_t bytes = (size_t)n_records * sizeof(NodeStats);
    DevBuf<NodeStats> a, b;
    DevBuf<uint32_t> fwd, cnt;
    DevBuf<DbgAdvTree> tr;
    HIP_TRY(a.alloc(n_records));
    HIP_TRY(b.alloc(n_records));
    HIP_TRY(fwd.alloc(n_records));
    HIP_TRY(cnt.alloc(n));
    HIP_TRY(tr.alloc(n));
    HIP_TRY(hipMemcpy(a.p, records, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b.p, 0xEE, bytes));
    HIP_TRY(hipMemcpy(tr.p, trees.data(), sizeof(DbgAdvTree) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_dbg_advance, dim3(n), dim3(ADV_THREADS), 0, 0, a.p, b.p, fwd.p, tr.p, n,
                       fast_nodes < (uint32_t)ADV_MAX_NODES ? fast_nodes : (uint32_t)ADV_MAX_NODES, cnt.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(in_place_out, a.p, bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(moved_out, b.p, bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts_out, cnt.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return AR_OK;
}

// Test entries (not in the public header): the device's scalar arithmetic, item by item.
// ar_debug_budgets: out[i] = collisions_left(node_counts[i], cfg) as the gathers compute it at the start of a batch.
int ar_debug_budgets(const ArSearchConfig* cfg, const uint32_t* node_counts, uint32_t n, uint32_t* out) {
    if (!cfg || !node_counts || !out || n == 0) return fail(AR_E_INVALID, "ar_debug_budgets: null argument");
    SearchCfg sc = to_cfg(*cfg, 1, 1);
    if (int rc = check_cfg(sc)) return rc;
    DevBuf<uint32_t> in, res, table;
    if (int rc = make_coll_table(sc, table)) return rc;  // as Engine::setup does
    HIP_TRY(in.alloc(n));
    HIP_TRY(res.alloc(n));
    HIP_TRY(hipMemcpy(in.p, node_counts, 4 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_dbg_budgets, dim3((n + 255) / 256), dim3(256), 0, 0, in.p, n, sc, res.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, res.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return AR_OK;
}

// ar_debug_draws: `n_streams` random streams, stream s seeded with seeds[s], each making draw->count draws of one kind
// (DbgDraw and k_dbg_draws above say which, with what parameters and in what format). out: n_streams * count items;
// states_out: four words per stream, the generator after the stream's last draw.
int ar_debug_draws(const uint64_t* seeds, uint32_t n_streams, const DbgDraw* draw, void* out, uint64_t* states_out) {
    if (!seeds || !draw || !out || !states_out || n_streams == 0) return fail(AR_E_INVALID, "ar_debug_draws: null argument");
    const DbgDraw d = *draw;
    if (d.kind >= DBG_DRAW_KINDS || d.count == 0 || (uint64_t)n_streams * d.count > (1ull << 26))
        return fail(AR_E_INVALID, "ar_debug_draws: unknown kind, no draws or more than 2^26 of them");
    if (d.kind == DBG_DRAW_BELOW && d.n == 0) return fail(AR_E_INVALID, "ar_debug_draws: rng_below needs n >= 1");
    if (d.kind == DBG_DRAW_GAMMA && !(d.shape >= 1.0 && d.shape <= 1e300))
        return fail(AR_E_INVALID, "ar_debug_draws: rng_gamma needs a finite shape >= 1");
    if (d.kind == DBG_DRAW_DIRICHLET && (d.n > 5 || !(d.concentration <= 3e38f)))
        return fail(AR_E_INVALID, "ar_debug_draws: dirichlet_mix needs n <= 5 and a finite concentration");
    const size_t bytes = (size_t)n_streams * d.count * dbg_draw_bytes(d.kind);
    DevBuf<uint64_t> sd, st;
    DevBuf<unsigned char> res;
    DevBuf<ZigTables> zig;
    HIP_TRY(sd.alloc(n_streams));
    HIP_TRY(st.alloc(4 * (size_t)n_streams));
    HIP_TRY(res.alloc(bytes));
    HIP_TRY(zig.alloc(1));
    HIP_TRY(hipMemcpy(sd.p, seeds, 8 * (size_t)n_streams, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(zig.p, &g_host_zig, sizeof g_host_zig, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_dbg_draws, dim3((n_streams + 63) / 64), dim3(64), 0, 0, sd.p, n_streams, d, zig.p, (void*)res.p, st.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, res.p, bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(states_out, st.p, 32 * (size_t)n_streams, hipMemcpyDeviceToHost));
    return AR_OK;
}

#if defined(AR_STATS)
// sizes of the resident trees: [0..64) games by live-tree top (hi) / 512, [64..128) by arena capacity / 512,
// [128] sum of hi, [129] sum of cap, [130] games
int ar_debug_tree_hist(unsigned long long* out131) {
    HIP_TRY(hipDeviceSynchronize());
    if (!g_dbg_slots) return fail(AR_E_INVALID, "no session");
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, 131 * 8));
    HIP_TRY(hipMemset(d, 0, 131 * 8));
    if (g_dbg_nw == 1) hipLaunchKernelGGL(k_dbg_tree_hist<1>, dim3((g_dbg_S + 255) / 256), dim3(256), 0, 0, (const Slot<1>*)g_dbg_slots, g_dbg_S, d);
    else hipLaunchKernelGGL(k_dbg_tree_hist<4>, dim3((g_dbg_S + 255) / 256), dim3(256), 0, 0, (const Slot<4>*)g_dbg_slots, g_dbg_S, d);
    HIP_TRY(hipMemcpy(out131, d, 131 * 8, hipMemcpyDeviceToHost));
    hipFree(d);
    return AR_OK;
}
int ar_debug_advance_clk(unsigned long long* out32) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out32, HIP_SYMBOL(ar::g_adv_clk), sizeof(unsigned long long) * 32));
    unsigned long long z[32] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(ar::g_adv_clk), z, sizeof z));
    return AR_OK;
}
int ar_debug_backup16_clk(unsigned long long* out32) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out32, HIP_SYMBOL(ar::g_bk16_clk), sizeof(unsigned long long) * 32));
    unsigned long long z[32] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(ar::g_bk16_clk), z, sizeof z));
    return AR_OK;
}
int ar_debug_round_stats(unsigned long long* out32) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out32, HIP_SYMBOL(ar::g_round_stats), sizeof(unsigned long long) * 32));
    unsigned long long z[32] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(ar::g_round_stats), z, sizeof z));
    return AR_OK;
}
int ar_debug_gather_hist(unsigned long long* out136) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out136, HIP_SYMBOL(ar::g_gather_hist), sizeof(unsigned long long) * 136));
    unsigned long long z[136] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(ar::g_gather_hist), z, sizeof z));
    return AR_OK;
}
int ar_debug_gather_clk(unsigned long long* out128) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out128, HIP_SYMBOL(ar::g_gather_clk), sizeof(unsigned long long) * 128));
    unsigned long long z[128] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(ar::g_gather_clk), z, sizeof z));
    return AR_OK;
}
#endif

int ar_release_device_memory(int device) {
    int dev = 0;
    if (int rc = parse_device("hip", device, dev)) return rc;
    HIP_TRY(hipSetDevice(dev));
    ArenaBlock b;
    {
        std::lock_guard<std::mutex> lk(g_arena_mu);
        if (dev < MAX_DEVICES) std::swap(b, g_arena_cache[dev]);
    }
    if (b.p) HIP_TRY(hipFree(b.p));
    return AR_OK;
}

int ar_device_sync(int device) {
    int dev = 0;
    if (int rc = parse_device("hip", device, dev)) return rc;
    HIP_TRY(hipSetDevice(dev));
    HIP_TRY(hipDeviceSynchronize());
    return AR_OK;
}

int ar_search_many(const ArGameSpec* games, uint32_t n, const ArSearchConfig* cfg, uint32_t simulations,
                   uint32_t batch_size, const uint64_t* seeds, ArNet* net, int device, ArSearchResult* out) {
    if (!games || !cfg || !out || n == 0) return fail(AR_E_INVALID, "null argument");
    int dev = 0;
    if (int rc = parse_device("hip", device, dev)) return rc;
    SearchCfg c = to_cfg(*cfg, simulations, batch_size);
    if (int rc = check_cfg(c)) return rc;
    bool small = true;
    for (uint32_t i = 0; i < n; ++i) small = small && (int)games[i].width * games[i].height <= 64;
    return small ? search_impl<1>(games, n, c, seeds, nullptr, nullptr, net, dev, out)
                 : search_impl<4>(games, n, c, seeds, nullptr, nullptr, net, dev, out);
}

int ar_search(const ArGameSpec* game, const ArSearchConfig* cfg, uint32_t simulations, uint32_t batch_size,
              const uint64_t* seed, ArPredictFn predict_fn, void* user, ArNet* net, int device, ArSearchResult* out) {
    if (!game || !cfg || !out) return fail(AR_E_INVALID, "null argument");
    int dev = 0;
    if (int rc = parse_device("hip", device, dev)) return rc;
    SearchCfg c = to_cfg(*cfg, simulations, batch_size);
    if (int rc = check_cfg(c)) return rc;
    const bool small = (int)game->width * game->height <= 64;
    return small ? search_impl<1>(game, 1, c, seed, predict_fn, user, net, dev, out)
                 : search_impl<4>(game, 1, c, seed, predict_fn, user, net, dev, out);
}

int ar_selfplay_open(const ArSelfPlayParams* p, ArProgress* progress, ArGameSink sink, void* sink_user,
                     ArSelfPlaySession** out) {
    if (!p || !out) return fail(AR_E_INVALID, "null argument");
    *out = nullptr;
    GameSupply games;
    std::string err;
    if (!games.init(*p, err)) return fail(AR_E_INVALID, err);
    int dev = 0;
    if (int rc = parse_device(p->device, p->device_index, dev)) return rc;
    std::unique_ptr<ArSelfPlaySession> s(new ArSelfPlaySession());
    if (p->weights_path) {
        if (int rc = ar_net_load(p->weights_path, dev, &s->net)) return rc;
        if (int rc = check_net_board(s->net, p->width, p->height)) return rc;
    }
    int rc;
    if (games.hw <= 64) {
        auto* impl = new SelfPlaySession<1>();
        s->impl = impl;
        rc = impl->open(*p, games, dev, s->net, progress, sink, sink_user);
    } else {
        auto* impl = new SelfPlaySession<4>();
        s->impl = impl;
        rc = impl->open(*p, games, dev, s->net, progress, sink, sink_user);
    }
    if (rc != AR_OK) return rc;
    *out = s.release();
    return AR_OK;
}

int ar_selfplay_step(ArSelfPlaySession* s, uint32_t batch_steps, ArSelfPlayStats* window, int* finished) {
    if (!s || !s->impl) return fail(AR_E_INVALID, "null session");
    return s->impl->step(batch_steps, window, finished);
}

int ar_selfplay_info(const ArSelfPlaySession* s, ArSessionInfo* out) {
    if (!s || !s->impl || !out) return fail(AR_E_INVALID, "null argument");
    s->impl->info(out);
    return AR_OK;
}

int ar_selfplay_close(ArSelfPlaySession* s, ArSelfPlayStats* total) {
    if (!s) return AR_OK;
    const int rc = s->impl ? s->impl->close(total) : AR_OK;
    delete s;
    return rc;
}

int ar_selfplay_run(const ArSelfPlayParams* p, ArProgress* progress, ArGameSink sink, void* sink_user,
                    ArSelfPlayStats* out) {
    if (!p || !out) return fail(AR_E_INVALID, "null argument");
    if (p->num_games == 0xFFFFFFFFu) return fail(AR_E_INVALID, "num_games = UINT32_MAX (unbounded) needs a session");
    memset(out, 0, sizeof *out);
    ArSelfPlaySession* s = nullptr;
    if (int rc = ar_selfplay_open(p, progress, sink, sink_user, &s)) return rc;
    int finished = 0;
    const int rc = ar_selfplay_step(s, 0xFFFFFFFFu, nullptr, &finished);
    const std::string msg = g_error;
    const int rc2 = ar_selfplay_close(s, out);
    if (rc != AR_OK) return fail(rc, msg);
    return rc2;
}

// ---- training rows: alpharat/data/sharding.py:513-595 on the device (dev_rows.h) --------------------------------
int ar_rows_open(uint8_t width, uint8_t height, uint64_t capacity_positions, int device, ArRowSet** out) {
    if (!out) return fail(AR_E_INVALID, "null argument");
    *out = nullptr;
    if (width == 0 || height == 0 || (int)width * height > 256) return fail(AR_E_INVALID, "board must have 1..256 cells");
    if (capacity_positions > 0xFFFFFFFFull) return fail(AR_E_INVALID, "a row set holds at most 2^32 - 1 positions");
    int dev = 0;
    if (int rc = parse_device("hip", device, dev)) return rc;
    std::unique_ptr<ArRowSet> s(new ArRowSet());
    s->impl = new RowStore();
    if (int rc = s->impl->open(width, height, capacity_positions, dev)) return rc;
    *out = s.release();
    return AR_OK;
}

int ar_rows_add_games(ArRowSet* s, const ArGameRecordView* games, uint32_t n) {
    if (!s || !s->impl || (!games && n)) return fail(AR_E_INVALID, "null argument");
    return s->impl->nw == 1 ? rows_add_games<1>(*s->impl, games, n) : rows_add_games<4>(*s->impl, games, n);
}

int ar_rows_attach(ArRowSet* s, ArSelfPlaySession* session) {
    if (!s || !s->impl || !session || !session->impl) return fail(AR_E_INVALID, "null argument");
    return session->impl->attach_rows(s->impl);
}

int ar_rows_count(const ArRowSet* s, uint32_t* games, uint64_t* positions) {
    if (!s || !s->impl) return fail(AR_E_INVALID, "null argument");
    if (games) *games = (uint32_t)s->impl->h_games.size();
    if (positions) *positions = s->impl->n_pos;
    return AR_OK;
}

int ar_rows_games(const ArRowSet* s, uint32_t* game_index, uint64_t* first_row, uint32_t* n_rows) {
    if (!s || !s->impl) return fail(AR_E_INVALID, "null argument");
    const std::vector<RowGame>& g = s->impl->h_games;
    for (size_t i = 0; i < g.size(); ++i) {
        if (game_index) game_index[i] = g[i].game_index;
        if (first_row) first_row[i] = g[i].first_row;
        if (n_rows) n_rows[i] = g[i].n_rows;
    }
    return AR_OK;
}

int ar_rows_build(ArRowSet* s, const uint64_t* rows, uint64_t n, const ArTrainRows* out) {
    if (!s || !s->impl) return fail(AR_E_INVALID, "null argument");
    if (n == 0) {
        s->impl->build_kernel_ms = 0.0;
        return AR_OK;
    }
    if (!rows || !out || !out->observation || !out->policy_p1 || !out->policy_p2 || !out->value_p1 || !out->value_p2 ||
        !out->action_p1 || !out->action_p2 || !out->cheese_outcomes)
        return fail(AR_E_INVALID, "null argument");
    return s->impl->nw == 1 ? rows_build<1>(*s->impl, rows, n, *out) : rows_build<4>(*s->impl, rows, n, *out);
}

int ar_rows_build_time(const ArRowSet* s, double* kernel_ms) {
    if (!s || !s->impl || !kernel_ms) return fail(AR_E_INVALID, "null argument");
    *kernel_ms = s->impl->build_kernel_ms;
    return AR_OK;
}

int ar_rows_order_set(ArRowSet* s, const uint64_t* rows, const uint8_t* swap, uint64_t n) {
    if (!s || !s->impl || (!rows && n)) return fail(AR_E_INVALID, "null argument");
    return rows_order_set(*s->impl, rows, swap, n);
}

int ar_rows_build_device(ArRowSet* s, uint64_t first, uint64_t n, const ArTrainRows* out, void* stream) {
    if (!s || !s->impl) return fail(AR_E_INVALID, "null argument");
    if (n && (!out || !out->observation || !out->policy_p1 || !out->policy_p2 || !out->value_p1 || !out->value_p2 ||
              !out->action_p1 || !out->action_p2 || !out->cheese_outcomes))
        return fail(AR_E_INVALID, "null argument");
    static const ArTrainRows none = {};
    return s->impl->nw == 1 ? rows_build_device<1>(*s->impl, first, n, out ? *out : none, (hipStream_t)stream)
                            : rows_build_device<4>(*s->impl, first, n, out ? *out : none, (hipStream_t)stream);
}

int ar_rows_grad_mlp_dropout(ArRowSet* s, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArMlpTensors* params,
                             const ArMlpTensors* grads, const ArMlpBnStats* running, float policy_weight, float value_weight,
                             const ArTrainOut* out, const ArTrainDropout* dropout, void* stream) {
    if (!s || !s->impl || !params || !grads) return fail(AR_E_INVALID, "null argument");
    return s->impl->nw == 1 ? rows_grad_mlp<1>(*s->impl, first, n, hidden_dim, *params, *grads, running, policy_weight, value_weight,
                                               out, (hipStream_t)stream, nullptr, dropout)
                            : rows_grad_mlp<4>(*s->impl, first, n, hidden_dim, *params, *grads, running, policy_weight, value_weight,
                                               out, (hipStream_t)stream, nullptr, dropout);
}

int ar_rows_grad_mlp(ArRowSet* s, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArMlpTensors* params,
                     const ArMlpTensors* grads, const ArMlpBnStats* running, float policy_weight, float value_weight,
                     const ArTrainOut* out, void* stream) {
    return ar_rows_grad_mlp_dropout(s, first, n, hidden_dim, params, grads, running, policy_weight, value_weight, out, nullptr,
                                    stream);
}

int ar_rows_grad_local_value_dropout(ArRowSet* s, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArLvTensors* params,
                                     const ArLvTensors* grads, const ArMlpBnStats* running, float policy_weight,
                                     float value_weight, float ownership_weight, const ArLvTrainOut* out,
                                     const ArTrainDropout* dropout, void* stream) {
    if (!s || !s->impl || !params || !grads) return fail(AR_E_INVALID, "null argument");
    const LvStep lv{params, grads, ownership_weight, out};
    const ArMlpTensors &p = *(const ArMlpTensors*)params, &g = *(const ArMlpTensors*)grads;
    return s->impl->nw == 1 ? rows_grad_mlp<1>(*s->impl, first, n, hidden_dim, p, g, running, policy_weight, value_weight,
                                               (const ArTrainOut*)out, (hipStream_t)stream, &lv, dropout)
                            : rows_grad_mlp<4>(*s->impl, first, n, hidden_dim, p, g, running, policy_weight, value_weight,
                                               (const ArTrainOut*)out, (hipStream_t)stream, &lv, dropout);
}

int ar_rows_grad_local_value(ArRowSet* s, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArLvTensors* params,
                             const ArLvTensors* grads, const ArMlpBnStats* running, float policy_weight, float value_weight,
                             float ownership_weight, const ArLvTrainOut* out, void* stream) {
    return ar_rows_grad_local_value_dropout(s, first, n, hidden_dim, params, grads, running, policy_weight, value_weight,
                                            ownership_weight, out, nullptr, stream);
}

int ar_rows_grad_symmetric_dropout(ArRowSet* s, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArSymTensors* params,
                                   const ArSymTensors* grads, const ArSymBnStats* running, float policy_weight, float value_weight,
                                   const ArTrainOut* out, const ArTrainDropout* dropout, void* stream) {
    if (!s || !s->impl || !params || !grads) return fail(AR_E_INVALID, "null argument");
    return s->impl->nw == 1 ? rows_grad_symmetric<1>(*s->impl, first, n, hidden_dim, *params, *grads, running, policy_weight,
                                                     value_weight, out, (hipStream_t)stream, dropout)
                            : rows_grad_symmetric<4>(*s->impl, first, n, hidden_dim, *params, *grads, running, policy_weight,
                                                     value_weight, out, (hipStream_t)stream, dropout);
}

int ar_rows_grad_symmetric(ArRowSet* s, uint64_t first, uint64_t n, uint32_t hidden_dim, const ArSymTensors* params,
                           const ArSymTensors* grads, const ArSymBnStats* running, float policy_weight, float value_weight,
                           const ArTrainOut* out, void* stream) {
    return ar_rows_grad_symmetric_dropout(s, first, n, hidden_dim, params, grads, running, policy_weight, value_weight, out,
                                          nullptr, stream);
}

int ar_rows_grad_cnn_gpool(ArRowSet* s, uint64_t first, uint64_t n, const ArCnnDims* dims, const ArCnnPoolDims* pool_dims,
                           const ArCnnTensors* params, const ArCnnPoolTensors* pool_params, const ArCnnTensors* grads,
                           const ArCnnPoolTensors* pool_grads, const ArCnnBnStats* running, const ArCnnPoolStats* pool_running,
                           float policy_weight, float value_weight, const ArTrainOut* out, const ArTrainDropout* dropout,
                           void* stream) {
    if (!s || !s->impl || !dims || !params || !grads) return fail(AR_E_INVALID, "null argument");
    return s->impl->nw == 1 ? rows_grad_cnn<1>(*s->impl, first, n, *dims, *params, *grads, running, policy_weight, value_weight, out,
                                               (hipStream_t)stream, pool_dims, pool_params, pool_grads, pool_running, dropout)
                            : rows_grad_cnn<4>(*s->impl, first, n, *dims, *params, *grads, running, policy_weight, value_weight, out,
                                               (hipStream_t)stream, pool_dims, pool_params, pool_grads, pool_running, dropout);
}

int ar_rows_grad_cnn(ArRowSet* s, uint64_t first, uint64_t n, const ArCnnDims* dims, const ArCnnTensors* params,
                     const ArCnnTensors* grads, const ArCnnBnStats* running, float policy_weight, float value_weight,
                     const ArTrainOut* out, void* stream) {
    return ar_rows_grad_cnn_gpool(s, first, n, dims, nullptr, params, nullptr, grads, nullptr, running, nullptr, policy_weight,
                                  value_weight, out, nullptr, stream);
}

int ar_train_dropout_mask(uint64_t seed, uint64_t step, uint32_t call, uint64_t n, uint32_t hidden_dim, float p,
                          uint8_t* keep_device, void* stream) {
    if (!keep_device) return fail(AR_E_INVALID, "null argument");
    if (!(p >= 0.0f) || !(p < 1.0f)) return fail(AR_E_INVALID, "dropout p must be in [0, 1) (got " + std::to_string(p) + ")");
    if (n == 0 || n > (uint64_t)TRAIN_MAX_ROWS) return fail(AR_E_INVALID, "1 to 65536 rows a mask");
    if (hidden_dim == 0 || hidden_dim % 32 != 0 || hidden_dim > 256)
        return fail(AR_E_INVALID, "hidden_dim must be a multiple of 32, at most 256 (got " + std::to_string(hidden_dim) + ")");
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, keep_device) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(AR_E_INVALID, "keep_device is not device memory");
    }
    int before = 0;
    HIP_TRY(hipGetDevice(&before));
    if (before != at.device) HIP_TRY(hipSetDevice(at.device));
    TrainDrop dr;
    dr.key = dropout_key(seed, step, (uint64_t)call);
    dr.thr = dropout_thr(p);
    dr.scale = dropout_scale(p);
    const uint64_t count = n * hidden_dim;
    hipLaunchKernelGGL(k_train_dropout_mask, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dr, count,
                       keep_device);
    const hipError_t e = hipGetLastError();
    if (before != at.device) (void)hipSetDevice(before);
    HIP_TRY(e);
    return AR_OK;
}

int ar_rows_clear(ArRowSet* s) {
    if (!s || !s->impl) return fail(AR_E_INVALID, "null argument");
    if (s->impl->has_batch) {  // the positions may be overwritten next: no batch may still read them
        HIP_TRY(hipSetDevice(s->impl->device));
        HIP_TRY(s->impl->wait_batches());
    }
    s->impl->h_games.clear();
    s->impl->n_pos = 0;
    s->impl->val_boards_n = 0;
    s->impl->stamp = g_rows_stamp++;
    s->impl->has_order = false;
    s->impl->ord_n = 0;
    return AR_OK;
}

void ar_rows_close(ArRowSet* s) { delete s; }

int ar_rows_validate(ArRowSet* s, ArNet* net, const uint64_t* rows, uint64_t n, uint32_t chunk_rows, ArValSums* sums,
                     const ArValRows* rows_out) {
    if (!s || !s->impl || !net || !sums || (!rows && n)) return fail(AR_E_INVALID, "null argument");
    ArValSums out;
    memset(&out, 0, sizeof out);
    const int rc = s->impl->nw == 1 ? rows_validate<1>(*s->impl, net, rows, n, chunk_rows, out, rows_out)
                                    : rows_validate<4>(*s->impl, net, rows, n, chunk_rows, out, rows_out);
    if (rc == AR_OK) *sums = out;
    return rc;
}

int ar_rows_validate_lv(ArRowSet* s, ArNet* net, const uint64_t* rows, uint64_t n, uint32_t chunk_rows, uint32_t loss_batch_rows,
                        ArValSums* sums, ArOwnSums* own, const ArValRows* rows_out, const ArOwnRows* own_out) {
    if (!s || !s->impl || !net || !sums || !own || (!rows && n)) return fail(AR_E_INVALID, "null argument");
    if (!net->has_own)
        return fail(AR_E_INVALID, "the network has no ownership head (an mlp blob written with keep_ownership, hidden width a "
                                  "multiple of 32 up to 256)");
    ArValSums out;
    ArOwnSums oout;
    memset(&out, 0, sizeof out);
    memset(&oout, 0, sizeof oout);
    const int rc = s->impl->nw == 1
                       ? rows_validate<1>(*s->impl, net, rows, n, chunk_rows, out, rows_out, loss_batch_rows, &oout, own_out)
                       : rows_validate<4>(*s->impl, net, rows, n, chunk_rows, out, rows_out, loss_batch_rows, &oout, own_out);
    if (rc == AR_OK) {
        *sums = out;
        *own = oout;
    }
    return rc;
}

// ---- matches: tournament.py:329-373 / eval/game.py:47-87 / searcher_agent.py:40-56 on the device --------------
int ar_match_run(const ArMatchParams* p, ArMatchSink sink, void* sink_user, ArMatchStats* out) {
    if (!p || !out) return fail(AR_E_INVALID, "null argument");
    memset(out, 0, sizeof *out);
    GameSupply games;
    std::string err;
    if (!games.init(*p, err)) return fail(AR_E_INVALID, err);
    const ArMatchAgent* agents[2] = {&p->a, &p->b};
    for (int k = 0; k < 2; ++k) {
        const ArMatchAgent& ag = *agents[k];
        const std::string who = std::string("agent ") + (k ? "B" : "A") + ": ";
        if (ag.kind != AR_AGENT_SEARCH && ag.kind != AR_AGENT_RANDOM && ag.kind != AR_AGENT_GREEDY)
            return fail(AR_E_INVALID, who + "unknown kind " + std::to_string(ag.kind));
        if (!std::isfinite(ag.temperature) || ag.temperature < 0.0f)
            return fail(AR_E_INVALID, who + "temperature must be finite and >= 0");
        if (ag.kind != AR_AGENT_SEARCH) {
            if (ag.weights_path) return fail(AR_E_INVALID, who + "weights_path given for a random or greedy agent, which has no evaluator");
            continue;  // (simulations, batch_size and search are not read)
        }
        if (int rc = check_cfg(to_cfg(ag.search, ag.simulations, ag.batch_size))) return rc;
    }
    int dev = 0;
    if (int rc = parse_device(p->device, p->device_index, dev)) return rc;
    struct Nets {
        ArNet* n[2] = {nullptr, nullptr};
        ~Nets() {
            for (ArNet* x : n)
                if (x) ar_net_free(x);
        }
    } nets;
    for (int k = 0; k < 2; ++k) {
        if (!agents[k]->weights_path) continue;
        if (int rc = ar_net_load(agents[k]->weights_path, dev, &nets.n[k])) return rc;
        if (int rc = check_net_board(nets.n[k], p->width, p->height, k ? "agent B: " : "agent A: ")) return rc;
    }
    return games.hw <= 64 ? match_impl<1>(*p, games, dev, nets.n[0], nets.n[1], sink, sink_user, out)
                          : match_impl<4>(*p, games, dev, nets.n[0], nets.n[1], sink, sink_user, out);
}

int ar_net_load(const char* blob_path, int device, ArNet** out) {
    if (!blob_path || !out) return fail(AR_E_INVALID, "null argument");
    *out = nullptr;
    int dev = 0;
    if (int rc = parse_device("hip", device, dev)) return rc;
    HIP_TRY(hipSetDevice(dev));
    arnet::Blob blob;
    std::string err;
    if (!blob.load(blob_path, err)) return fail(AR_E_IO, err);
    std::unique_ptr<ArNet> net(new ArNet());
    net->device = dev;
    if (int rc = net_build(blob, net.get())) return rc;
    *out = net.release();
    return AR_OK;
}

void ar_net_free(ArNet* net) { delete net; }

int ar_net_has_ownership(const ArNet* net) { return net && net->has_own ? 1 : 0; }

}  // extern "C"

namespace {
template <int NW>
int specs_to_device(const ArGameSpec* games, uint32_t n, std::vector<LeafReq<NW>>& reqs, std::vector<Board>& boards,
                    std::vector<uint8_t>& mazes) {
    std::string err;
    reqs.resize(n);
    boards.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        HostGame hg;
        std::vector<uint8_t> c;
        if (!host_game_from_spec(games[i], hg, c, err)) return fail(AR_E_INVALID, err);
        memset(&reqs[i], 0, sizeof reqs[i]);
        fill_state<NW>(hg, boards[i], reqs[i].st, (uint32_t)mazes.size());
        reqs[i].slot = i;
        mazes.insert(mazes.end(), c.begin(), c.end());
    }
    return AR_OK;
}

// grow-only device buffer kept inside the ArNet between ar_net_evaluate calls (callers such as a predict_fn
// adaptor evaluate a handful of positions thousands of times: five allocations per call cost more than the network)
static int scratch_reserve(ArNet* net, int which, size_t bytes, void** out) {
    ArNet::Scratch& sc = net->scratch[which];
    if (sc.bytes < bytes) {
        if (sc.p) hipFree(sc.p);
        sc.p = nullptr;
        sc.bytes = 0;
        const size_t want = bytes < 4096 ? 4096 : bytes + bytes / 2;
        if (hipMalloc(&sc.p, want) != hipSuccess) return fail(AR_E_NOMEM, "device allocation failed (evaluator scratch)");
        sc.bytes = want;
    }
    *out = sc.p;
    return AR_OK;
}

template <int NW>
int net_evaluate_impl(ArNet* net, const ArGameSpec* games, uint32_t n, float* pp1, float* pp2, float* pv1, float* pv2,
                      float* lg1, float* lg2) {
    std::vector<LeafReq<NW>> reqs;
    std::vector<Board> boards;
    std::vector<uint8_t> mazes;
    for (uint32_t i = 0; i < n; ++i)
        if (games[i].width != net->dev.width || games[i].height != net->dev.height)
            return fail(AR_E_INVALID, "game size does not match the network's board size");
    if (int rc = specs_to_device<NW>(games, n, reqs, boards, mazes)) return rc;
    // positions on the same maze share one pool entry (the usual case: a batch of leaves of one game)
    const size_t per = (size_t)net->dev.hw * 4;
    bool one_maze = true;
    for (uint32_t i = 1; i < n && one_maze; ++i) one_maze = memcmp(&mazes[i * per], &mazes[0], per) == 0;
    if (one_maze) {
        mazes.resize(per);
        for (uint32_t i = 0; i < n; ++i) boards[i].maze_off = 0;
    }
    const int n_mazes = one_maze ? 1 : (int)n;
    HIP_TRY(hipSetDevice(net->device));
    LeafReq<NW>* d_req = nullptr;
    Board* d_boards = nullptr;
    uint8_t* d_maze = nullptr;
    EvalOut* d_out = nullptr;
    float* d_logits = nullptr;
    if (int rc = scratch_reserve(net, 0, sizeof(LeafReq<NW>) * n, (void**)&d_req)) return rc;
    if (int rc = scratch_reserve(net, 1, sizeof(Board) * n, (void**)&d_boards)) return rc;
    if (int rc = scratch_reserve(net, 2, mazes.size(), (void**)&d_maze)) return rc;
    if (int rc = scratch_reserve(net, 3, sizeof(EvalOut) * n, (void**)&d_out)) return rc;
    if (int rc = scratch_reserve(net, 4, (size_t)n * 40, (void**)&d_logits)) return rc;
    HIP_TRY(hipMemcpy(d_req, reqs.data(), sizeof(LeafReq<NW>) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_boards, boards.data(), sizeof(Board) * n, hipMemcpyHostToDevice));
    // the maze constants are only recomputed when the mazes' bytes (not just their address) differ from the last call's
    if (net->scratch_mazes != mazes || net->bound_pool != d_maze || net->bound_mazes != n_mazes) {
        HIP_TRY(hipMemcpy(d_maze, mazes.data(), mazes.size(), hipMemcpyHostToDevice));
        if (int rc = net_bind_mazes(net, d_maze, n_mazes, nullptr)) return rc;
        net->scratch_mazes = mazes;
    }
    int rc = net_launch<NW>(net, d_req, nullptr, n, (const char*)d_boards, sizeof(Board), d_out, d_logits, nullptr);
    if (rc != AR_OK) return rc;
    std::vector<EvalOut> out(n);
    std::vector<float> logits((size_t)n * 10);
    HIP_TRY(hipMemcpy(out.data(), d_out, sizeof(EvalOut) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(logits.data(), d_logits, logits.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) {
        memcpy(pp1 + (size_t)i * 5, out[i].p1, 20);
        memcpy(pp2 + (size_t)i * 5, out[i].p2, 20);
        pv1[i] = out[i].v1;
        pv2[i] = out[i].v2;
        if (lg1) memcpy(lg1 + (size_t)i * 5, &logits[(size_t)i * 10], 20);
        if (lg2) memcpy(lg2 + (size_t)i * 5, &logits[(size_t)i * 10 + 5], 20);
    }
    return AR_OK;
}

template <int NW>
int encode_impl(const ArGameSpec* games, uint32_t n, float* obs) {
    std::vector<LeafReq<NW>> reqs;
    std::vector<Board> boards;
    std::vector<uint8_t> mazes;
    if (int rc = specs_to_device<NW>(games, n, reqs, boards, mazes)) return rc;
    int dim = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const int d = games[i].width * games[i].height * 7 + 6;
        if (i && d != dim) return fail(AR_E_INVALID, "ar_encode: all games must have the same board size");
        dim = d;
    }
    DevBuf<LeafReq<NW>> d_req;
    DevBuf<Board> d_boards;
    DevBuf<uint8_t> d_maze;
    DevBuf<float> d_obs;
    HIP_TRY(d_req.alloc(n));
    HIP_TRY(d_boards.alloc(n));
    HIP_TRY(d_maze.alloc(mazes.size()));
    HIP_TRY(d_obs.alloc((size_t)n * dim));
    HIP_TRY(hipMemcpy(d_req.p, reqs.data(), sizeof(LeafReq<NW>) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_boards.p, boards.data(), sizeof(Board) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_maze.p, mazes.data(), mazes.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(arnet::k_encode<NW>, dim3(n), dim3(128), 0, nullptr, d_req.p, n, d_boards.p, d_maze.p, d_obs.p, dim);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(obs, d_obs.p, (size_t)n * dim * 4, hipMemcpyDeviceToHost));
    return AR_OK;
}
}  // namespace

extern "C" {

int ar_net_evaluate(ArNet* net, const ArGameSpec* games, uint32_t n, float* policy_p1, float* policy_p2,
                    float* value_p1, float* value_p2, float* logits_p1, float* logits_p2) {
    if (!net || !games || !policy_p1 || !policy_p2 || !value_p1 || !value_p2) return fail(AR_E_INVALID, "null argument");
    if (n == 0) return AR_OK;
    return net->dev.hw <= 64
               ? net_evaluate_impl<1>(net, games, n, policy_p1, policy_p2, value_p1, value_p2, logits_p1, logits_p2)
               : net_evaluate_impl<4>(net, games, n, policy_p1, policy_p2, value_p1, value_p2, logits_p1, logits_p2);
}

int ar_encode(const ArGameSpec* games, uint32_t n, int device, float* obs) {
    if (!games || !obs) return fail(AR_E_INVALID, "null argument");
    if (n == 0) return AR_OK;
    int dev = 0;
    if (int rc = parse_device("hip", device, dev)) return rc;
    HIP_TRY(hipSetDevice(dev));
    bool small = true;
    for (uint32_t i = 0; i < n; ++i) small = small && (int)games[i].width * games[i].height <= 64;
    return small ? encode_impl<1>(games, n, obs) : encode_impl<4>(games, n, obs);
}

int ar_write_bundle(const ArGameRecordView* games, uint32_t n, const char* path) {
    if (!games || !path) return fail(AR_E_INVALID, "null argument");
    std::string err;
    if (!write_bundle(games, n, path, err)) return fail(AR_E_IO, err);
    return AR_OK;
}

}  // extern "C"
