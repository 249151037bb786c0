// Engine state shared by the ABI layer and the kernel launchers (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <map>
#include <utility>

#include "../../include/m2d.h"

struct m2d_train_state;   // csrc/m2d_train.hip
struct m2d_engine;

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- engine-owned memory ----
// Everything the engine allocates lives in one of the owner types below: pointer and capacity travel together, and the block is
// freed when its owner goes (with the engine, or with the state it is built into) -- nothing is freed by hand anywhere else.
#define M2D_HIP_TRY(h, expr)                                                                   \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return m2d_hip_failed(h, #expr, e_);                             \
    } while (0)
int m2d_hip_failed(m2d_engine *h, const char *expr, hipError_t e);   // sets last_error, returns M2D_ERR_HIP

// A device block of T (capacity in units of UNIT bytes: sizeof(T), or 1 for blocks that are carved up by hand).  It converts to T *,
// so launchers read it like the plain pointer it replaces.
template <typename T> struct m2d_unit { static constexpr size_t bytes = sizeof(T); };
template <> struct m2d_unit<void> { static constexpr size_t bytes = 1; };
template <typename T, size_t UNIT = m2d_unit<T>::bytes>
struct m2d_dev_buf {
    T *p = nullptr;
    size_t cap = 0;
    m2d_dev_buf() = default;
    m2d_dev_buf(m2d_dev_buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    m2d_dev_buf &operator=(m2d_dev_buf &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~m2d_dev_buf() { reset(); }
    operator T *() const { return p; }
    T *get() const { return p; }
    hipError_t release()                // null with capacity 0 afterwards, whatever hipFree says
    {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr; cap = 0;
        return e;
    }
    void reset() { (void)release(); }
    // Grow to `need` units; nothing happens while the capacity suffices.  `inside` are the engine's pointers into the old block:
    // they are null before it is freed and stay null when the allocation fails -- m2d_get_option reads through them -- and the
    // buffer is then null with capacity 0.
    template <typename... Inside> int grow(m2d_engine *h, const size_t need, Inside *&...inside)
    {
        if (cap >= need) return M2D_OK;
        ((inside = nullptr), ...);
        M2D_HIP_TRY(h, release());
        M2D_HIP_TRY(h, hipMalloc((void **)&p, need * UNIT));
        cap = need;
        return M2D_OK;
    }
};

// the same for a pinned host block, allocated once
template <typename T> struct m2d_host_buf {
    T *p = nullptr;
    m2d_host_buf() = default;
    m2d_host_buf(const m2d_host_buf &) = delete;
    m2d_host_buf &operator=(const m2d_host_buf &) = delete;
    ~m2d_host_buf() { reset(); }
    operator T *() const { return p; }
    void reset()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
    int alloc(m2d_engine *h, const size_t count, const unsigned flags = hipHostMallocDefault)
    {
        reset();
        M2D_HIP_TRY(h, hipHostMalloc((void **)&p, count * sizeof(T), flags));
        return M2D_OK;
    }
};

// an event, created on first use
struct m2d_event {
    hipEvent_t e = nullptr;
    m2d_event() = default;
    m2d_event(const m2d_event &) = delete;
    m2d_event &operator=(const m2d_event &) = delete;
    ~m2d_event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

// A table the caller handed over: `p` is what the launchers read -- the caller's own array (M2D_TABLES_DEVICE: borrowed, `own` is
// empty) or the engine's copy of it (M2D_TABLES_HOST: `own`).  Filled by adopt() in m2d_abi.hip; a setter builds its tables aside
// and moves them in when everything has passed.
template <typename T> struct m2d_table {
    const T *p = nullptr;
    m2d_dev_buf<T> own;
    operator const T *() const { return p; }
    void reset() { p = nullptr; own.reset(); }
};

struct m2d_engine {
    // tables in HBM, row-major, float32 (Model_Recommender.py:45-53)
    m2d_table<float> pm;         // [U, C+1, E]
    m2d_table<float> re;         // [I, E]
    m2d_table<float> ce;         // [C, E]
    m2d_table<float> dish_cats;  // [I, C] or null
    int64_t U = 0, I = 0;
    int32_t C = 0, E = 0;
    int64_t user_base = 0;
    float a = 0.f;  // float32(coef)             Model_Recommender.py:17
    float b = 0.f;  // 1.0f - a, taken in float32 Model_Recommender.py:96
    int device = 0;
    int num_cu = 256;

    // id-error latch: {code, bad value, index lo, index hi}; cleared by m2d_check (kernels write it with m2d_latch_error below)
    m2d_dev_buf<int32_t> err_dev;
    m2d_host_buf<int32_t> err_host;

    // "some value of Personal_Memory / Recipe_Embedding / Category_Embedding is not finite, or some H[d] of the ingredient table is
    // +-inf" (device word, sticky until the next full scan).  Model_Recommender.py:82-90 multiplies the row of a category a dish does not have by 0, and
    // 0 * inf = NaN: every kernel that leaves such rows out (option skip_masked, the pattern-grouped forms) reads this
    // word and fetches / multiplies everything when it is set.  Set by m2d_scan_tables (queued by m2d_create and
    // m2d_tables_updated, run by the next scoring call on its stream) and by the engine's own writers (training step,
    // Write_Memory) on the values they write.
    int32_t *nonfinite_dev = nullptr;
    bool finite_scan_pending = true;

    // build-defined extension: multi-hot ingredient table
    m2d_table<float> ing;              // [R, E]
    m2d_table<int32_t> ing_off;        // [I+1] CSR offsets per dish
    m2d_table<int32_t> ing_ids;        // [nnz]
    m2d_table<float> ing_w;            // [nnz] or null (all ones)
    int64_t ing_rows = 0, ing_nnz = 0;
    m2d_dev_buf<float> dish_high;      // [I, E]  H[d] = sum_j w_j ING[id_j] / sum_j w_j

    // build-defined extension: 3-layer scoring head
    m2d_table<float> mlp_w1, mlp_b1, mlp_w2, mlp_b2, mlp_w3;   // "the head is set" is mlp_w1 != null
    float mlp_b3 = 0.f;
    int32_t mlp_h1 = 0, mlp_h2 = 0;
    m2d_dev_buf<void> mlp_w1x3;         // split-bf16 image of W1 for the bf16x3 layer-1 path (built lazily)
    m2d_dev_buf<float> mlp_w1pad;       // W1 zero-padded to a multiple of 64 rows, for K = (C + 1) E that is not one (built lazily)
    m2d_dev_buf<void> mlp_w1pc;         // W1 | W2 image of the producer / consumer kernel (built lazily)
    m2d_dev_buf<int32_t> mlp_pg;        // per-launch pair grouping of that kernel: histogram | tile count | tile blocks | slot -> pair
    m2d_dev_buf<uint8_t> mlp_pat8;      // [I] a dish's pattern of non-zero mask weights (all blocks for n = 0 / NaN): what the grouping reads per pair
    uint64_t mlp_pat8_gen = 0;          // the dish-vector build it belongs to (dish_vec_gen)

    // m2d_topk_users_mlp (m2d_topk_mlp.hip): a chunk's pair ids (users | items), its head scores and, in the two-stage form, stage 1's
    // candidate ids (with exclusions: the whole call's, ids [nU, K1] | stage 1's scores [nU, K1]) -- buffers of their own: stage 1
    // writes `scratch`, the head's pair grouping writes mlp_pg
    m2d_dev_buf<int32_t> topk_mlp_ids;
    m2d_dev_buf<float> topk_mlp_scores;
    m2d_dev_buf<int32_t> topk_mlp_cand;
    m2d_dev_buf<float> topk_mlp_held;             // m2d_catalogue_rank_mlp: the held-out pairs' scores when the caller takes none
    int64_t opt_topk_mlp_chunk_pairs = 1 << 22;   // pairs per head launch of that call (diagnostic: the lists do not depend on it)
    int64_t topk_mlp_launches = 0;                // head launches of the last call

    // m2d_score_slate / m2d_topk_slate (m2d_slate.hip): the call's slate vectors Dt_s -- rows of K rounded up to the kernel's k chunk
    // floats, zero beyond K: the slate's nD rows, zero rows up to the dish-tile multiple and one more zero row that pads the
    // user operand -- rebuilt by every call (they hang on the call's slate and on every table); and a user block's scores of m2d_topk_slate
    m2d_dev_buf<float> slate_dt;
    m2d_dev_buf<float> slate_scores;
    int64_t opt_slate_chunk_pairs = 1 << 22;         // pairs of score scratch per m2d_topk_slate pass (the lists do not depend on it)
    int64_t opt_deep_chunk_pairs = 1 << 22;          // the same for m2d_topk_users_deep: ranges of min(I, P, 65536) dishes, blocks of P / W users

    // m2d_topk_groups / m2d_*_groups_slate (m2d_groups.hip): the call's dense member array i32[nG * M] (valid ids only) | cnt i32[nG]
    // (m2d_plan_groups: | the folded caps i32[nG, C] | the folded plan caps i32[nG, C]); the members' score rows go to slate_scores above
    m2d_dev_buf<int32_t> group_ids;

    // m2d_topk_menu (m2d_menu.hip): the signature index of the dish masks -- perm i32[I], the dish ids by (signature, id) | seg_off
    // i32[65] behind it, with seg_off's host copy (menu_seg; read once per build through the pinned block) -- built by the first call
    // after a mask write; the build's scratch (sig u8[I] | block counts i32[nb, 64] | block bases i32[nb, 64], in words); and a user
    // block's candidate lists [S', Ub, k] (S' non-empty segments).  The score rows go to slate_scores above
    m2d_dev_buf<int32_t> menu_perm;
    m2d_dev_buf<int32_t> menu_work;
    m2d_host_buf<int32_t> menu_seg_host;
    int32_t menu_seg[65] = {};
    bool menu_valid = false;
    m2d_dev_buf<float> menu_list_scores;
    m2d_dev_buf<int32_t> menu_list_ids;
    int opt_menu_select = 0;           // the per-segment selection: 0 = the list across a wave's lanes (m2d_topk_mlp_select), 1 = the radix select (A/B: same words)
    // m2d_topk_menu_filtered with a slate: the call's own index -- slate_perm i32[nD], the slate's ids by (signature, id) | seg_off i32[65]
    // behind it -- and its build's scratch (sig u8[nD] | block counts | block bases, in words); rebuilt by every call with a slate
    m2d_dev_buf<int32_t> menu_slate_perm;
    m2d_dev_buf<int32_t> menu_slate_work;

    // m2d_set_recipes / m2d_cookable_dishes (m2d_market.hip): every dish's ingredient list, CSR, validated once by the setter (CSR
    // shape, every id in [0, R)); lists only -- no table, no weights, nothing the scoring path reads, and no tie to `ing` above.
    // market_buf: the call's scratch -- bitmap of R bits | missing[I] (unless the caller gives a buffer) | kept dishes per block |
    // their exclusive scan | the total (8 bytes)
    m2d_table<int32_t> rcp_off;        // [I+1]
    m2d_table<int32_t> rcp_ids;        // [nnz]
    bool rcp_set = false;
    int64_t rcp_rows = 0, rcp_nnz = 0;
    m2d_dev_buf<int32_t> market_buf;
    m2d_host_buf<int64_t> market_count_host;   // the count of the last call

    // m2d_topk_markets (m2d_market_requests.hip): the shares' partial lists, ids [nQ, S k] | score words [nQ, S k], and in the
    // through-L2 form (R > 65 536) one bitmap of ceil(R / 32) words per request behind them
    m2d_dev_buf<int32_t> markets_buf;
    int opt_market_shares = 0;         // shares of the catalogue per request: 0 = the launcher's rule, 1 ... 64 forced (A/B: same words)
    int market_shares_used = 0;        // what the last call used

    // m2d_*_profiles (m2d_profiles.hip): the call's composed rows [n, C+1, E] and, behind them, the ids 0 .. n-1 its launchers are
    // handed as users (m2d_rows_view below)
    m2d_dev_buf<float> profile_buf;

    // derived table for pair scoring: <U_high[u], CE_c> per user and category (built lazily by large m2d_score_pairs calls;
    // stale after any write to Personal_Memory / Category_Embedding: the engine's own writers and m2d_tables_updated reset it)
    m2d_dev_buf<float> user_high;  // [U, 4]
    bool user_high_valid = false;

    // serving mirror of Personal_Memory (option "pm_bf16"): its round-to-nearest-even bf16 image, rows indexed like the table's own
    // (u - user_base); built lazily by m2d_ensure_pm_bf16, stale after any write to Personal_Memory.  Rounding can make an inf the
    // f32 table does not hold, so the mirror has a non-finite word of its own: the builder sets it from what it writes, and the
    // mirror kernels leave out weight-0 rows only while this word and nonfinite_dev are both 0
    m2d_dev_buf<uint16_t> pm_bf16;        // [U, C+1, E]
    bool pm_bf16_valid = false;
    int32_t *pm_bf16_nonfinite = nullptr; // device word (inside err_dev's allocation)

    // factored dish vectors for catalogue retrieval (built lazily by m2d_topk_users)
    m2d_dev_buf<float> dish_vec;  // [I_pad, (C+1)*E]
    int64_t dish_vec_rows = 0;
    bool dish_vec_valid = false;
    uint64_t dish_vec_gen = 0;          // counts m2d_ensure_dish_vectors' rebuilds (what hangs on the dish masks rebuilds with it)

    // pattern-grouped retrieval tables (0/1 masks only; built lazily by m2d_topk_users)
    m2d_dev_buf<float> grp_rs;          // [grp_cap_rows, E] Recipe_Embedding rows sorted by (mask pattern, dish id)
    m2d_dev_buf<void> grp_rs16;         // the same rows split into bf16 hi | lo blocks per 32-row tile
    m2d_dev_buf<int32_t> grp_perm;      // [grp_cap_rows]    slot -> dish id, -1 = padding
    m2d_dev_buf<int32_t> grp_tile_info; // [tiles]           pattern | valid rows << 8
    m2d_dev_buf<int32_t, 1> grp_work;   // block histograms / group offsets / flags (bytes)
    int64_t grp_tiles = 0, grp_cap_rows = 0;
    int grp_ew = 0;                     // row width of grp_rs: E, or 2 E with the ingredient extension ([H[d] | RE[d]])
    bool grp_valid = false, grp_binary = false;
    bool grp_nonfinite = false;         // *nonfinite_dev as last read by the retrieval launcher (with the table build, or again
    bool grp_nonfinite_known = false;   //  after a writer that leaves the sorted dish rows alone: m2d_write_memory on Personal_Memory)
    uint64_t grp_gen = 0;               // counts the sorted table's builds (what is derived from it rebuilds with it)

    // m2d_catalogue_rank (m2d_catalogue_rank.hip): per-query records | sort | counters, and the per-tile row-norm table
    m2d_dev_buf<float> rank_buf;
    unsigned long long *rank_counters = nullptr;   // [0] tiles multiplied, [1] (query, dish) pairs decided exactly, of the last call
    m2d_dev_buf<float> rank_tnorm;      // [tiles] largest row norm of each 32-row tile of the sorted table
    uint64_t rank_tnorm_gen = ~0ull;    // the grp_gen it was built for

    // m2d_topk_users_excluding (m2d_catalogue_excl.hip): unfiltered lists | short users | records | sort | counters | partial lists
    m2d_dev_buf<float> excl_buf;
    unsigned long long *excl_counters = nullptr;   // [0] tiles the exact scan multiplied in the last call
    int32_t *excl_short = nullptr;      // [0] users the last call's filter sent to the exact scan
    int64_t excl_all_short = -1;        // >= 0: the last call sent every user there (this many), the device word is not used
    int opt_topk_excl_tier = 0;         // 0 = filter m2d_topk_users' lists where they are index-exact, exact scan for the rest; 2 = exact scan for all (A/B)

    // training step: optimizer slots and gradient scratch, created by m2d_train_begin
    m2d_train_state *train = nullptr;

    // staging for m2d_score_pairs_host: one pinned block and its device twin
    m2d_host_buf<unsigned char> stage_host;
    m2d_dev_buf<unsigned char> stage_dev;  // its capacity is the size of both
    m2d_event stage_ev[2];              // chunked host feeds: a block's chunk has been delivered
    uint32_t stage_ticket = 0;          // completion word of the last m2d_score_pairs_host call (wraps)

    // scratch for rank_candidates
    m2d_dev_buf<float, 1> scratch;      // (bytes)
    m2d_dev_buf<float> topk_flags;      // pattern-grouped retrieval: tie values per (user, split) / per user (NaN: no tie at the k-th score)
    float *topk_tie_final = nullptr;    // the per-user values of the last call, inside topk_flags
    m2d_dev_buf<float> topk_plan;       // pipelined retrieval kernel: per-user plan records | launch order | sort histogram | tile counter
    unsigned long long *topk_tiles_counter = nullptr;   // tiles the blocks of the last pipelined launch stepped through (inside topk_plan)
    bool topk_apx_last = false;         // the last pipelined retrieval launch took the hi x hi first form (see "topk_tiles_completed")
    int64_t topk_tiles_full = 0;        // ... and what they would have stepped through without pattern pruning
    int32_t *topk_tie_list = nullptr;   // [0] users the tie repair re-ranked in the last pattern-grouped call (get_option "topk_repaired")

    // benchmarking knobs
    int opt_prefetch = 2;
    int opt_nt = 1;
    int opt_blocks_per_cu = 8;
    int opt_variant = 0;
    int opt_user_high = 0;              // opt-in: batches of >= 2^18 pairs take the high-level sum from the derived <U_high, CE_c> table
    int opt_pm_bf16 = 0;                // opt-in: the C = 4 pair kernels read Personal_Memory's rows from the bf16 mirror (any batch size)
    int opt_host_zero_copy = 2;         // m2d_score_pairs_host, <= 65536 pairs: 1 = the kernel reads / writes the pinned staging block itself,
                                        // 2 = and the host spins on a completion word in that block before falling back to a stream wait; 0 = staged copies
    int opt_skip_masked = 1;            // pair kernels: rows of categories with mask weight 0 are not fetched (their products are 0)
    int opt_mlp_form = 0;               // split-bf16 MLP head: 0 = matrix waves fed by gather / DMA waves (m2d_mlp_pc), 1 = every wave gathers its own rows
    int opt_mlp_bf16x3 = 1;             // MLP head layer 1 (build-defined) on split-bf16 MFMA; 0 = exact-f32 MFMA
    int opt_topk_bf16x3 = 1;            // retrieval (build-defined) on split-bf16 MFMA; 0 = exact-f32 MFMA
    int opt_topk_grouped = 1;           // 0/1-mask catalogues: pattern-grouped retrieval (contraction over E); 0 = dense kernel
    int opt_topk_form = 0;              // split-bf16 retrieval kernel: 0 / 2 = pipelined form, 1 = first form; 3 / 4 = hi x hi first form always / never
    int opt_topk_refine = 1;            // near-tied lists are finished in the tie repair's plain-f32 arithmetic (m2d_topk_refine): 0 = off (A/B)
    m2d_dev_buf<float> topk_ex;         // what the lists leave out, per (user, dish range) / (user, group) / user: 4 floats each
    int32_t *topk_refine_counter = nullptr;   // [2] users refined, users sent on to the repair (inside topk_ex's allocation)
    int opt_topk_block = 0;             // users per block of a pruned split-bf16 launch: 0 = the launcher's choice, 128 / 256 forced (A/B)
    int topk_block_users = 256;         // what the last pattern-grouped launch used (the tile counters count tiles of blocks this size)
    int opt_topk_prune = 1;             // pipelined form: blocks step through the tiles of their users' relevant mask patterns only (0 = every tile)

    std::string last_error;
    const char *last_kernel = "";

    m2d_engine() = default;
    ~m2d_engine();                      // m2d_train.hip (the training state's type lives there); the engine's device is current
};

// the id-error latch (m2d_engine::err_dev): the first error of a call wins -- its code, the bad value, where it stood
__device__ __forceinline__ void m2d_latch_error(int32_t *err, int code, int32_t value, int64_t index)
{
    if (atomicCAS(&err[0], 0, code) == 0) {
        err[1] = value;
        err[2] = (int32_t)(index & 0xffffffff);
        err[3] = (int32_t)(index >> 32);
    }
}

// a pair's id error: the user id is looked at first (ul = uid - user_base, U rows), the caller has found one of the two out of range
__device__ __forceinline__ void m2d_latch_bad_pair(int32_t *err, int64_t ul, int64_t U, int32_t uid, int32_t did, int64_t index)
{
    const bool user = ul < 0 || ul >= U;
    m2d_latch_error(err, user ? M2D_ERR_BAD_USER_ID : M2D_ERR_BAD_ITEM_ID, user ? uid : did, index);
}

// floats of table 0 / 1 / 2: Personal_Memory [U, C+1, E], Recipe_Embedding [I, E], Category_Embedding [C, E]
static inline int64_t m2d_table_floats(const m2d_engine *h, int table)
{
    return table == 0 ? h->U * (int64_t)(h->C + 1) * h->E : table == 1 ? h->I * (int64_t)h->E : (int64_t)h->C * h->E;
}

// grid of a grid-stride launch: one block per `per_block` items, at least one, at most `per_cu` (eight) per CU
static inline unsigned m2d_blocks_for(const m2d_engine *h, int64_t items, int64_t per_block, int per_cu = 8)
{
    const int64_t b = (items + per_block - 1) / per_block, cap = (int64_t)h->num_cu * per_cu;
    return (unsigned)(b > cap ? cap : b < 1 ? 1 : b);
}

// What a write makes stale.  Every writer of something the derived state is built from says WHICH tables it wrote and what is
// known about the new VALUES; the dependencies are here and nowhere else:
//   user_high (<U_high, CE_c>)                                  hangs on Personal_Memory, Category_Embedding;
//   pm_bf16 (the bf16 mirror) and its non-finite word           hang on Personal_Memory (rebuilt as a whole, word included);
//   dish_vec and the sorted retrieval tables (grp_*)            hang on Recipe_Embedding, Category_Embedding, the dish masks and
//                                                               the ingredient table (H[d] rides in the sorted rows);
//   the menu call's signature index (menu_*)                    hangs on the dish masks (m2d_tables_updated names them too: a
//                                                               borrowed mask table may have been rewritten in place);
//   the non-finite word (nonfinite_dev)                         covers every table value and H[d]:
//     M2D_BY_ENGINE  one of the engine's own kernels wrote, and looked at what it wrote: the word is up to date on the device, but
//                    the retrieval launcher's host copy of it (grp_nonfinite) is not -- it reads the word again;
//     M2D_BY_CALLER  the caller wrote: nobody looked, the full scan is queued again (it resets the host copy when it runs);
//     M2D_NO_VALUES  nothing the word covers changed (the dish masks).
// State that follows a generation counter (mlp_pat8_gen, rank_tnorm_gen) rebuilds with what it was derived from.
enum : unsigned { M2D_TAB_PM = 1, M2D_TAB_RE = 2, M2D_TAB_CE = 4, M2D_TAB_MASKS = 8, M2D_TAB_ING = 16 };
enum m2d_written_by { M2D_BY_ENGINE, M2D_BY_CALLER, M2D_NO_VALUES };
static inline void m2d_mark_written(m2d_engine *h, unsigned tables, m2d_written_by who)
{
    if (tables & (M2D_TAB_PM | M2D_TAB_CE)) h->user_high_valid = false;
    if (tables & M2D_TAB_PM) h->pm_bf16_valid = false;
    if (tables & (M2D_TAB_RE | M2D_TAB_CE | M2D_TAB_MASKS | M2D_TAB_ING)) h->dish_vec_valid = h->grp_valid = false;
    if (tables & M2D_TAB_MASKS) h->menu_valid = false;
    if (who == M2D_BY_ENGINE) h->grp_nonfinite_known = false;
    if (who == M2D_BY_CALLER) h->finite_scan_pending = true;
}

// Scoped view (m2d_profiles.hip): while it lives, every launcher serves `rows` [n, C+1, E] in place of Personal_Memory -- users are
// 0 .. n-1, no shard base, neither the <U_high, CE_c> table nor the bf16 mirror (both belong to the real table).  The destructor
// puts the engine's own values back on every exit path; kernels and launcher signatures are what they were.  Rules:
//   m2d_ensure_finite_scan runs BEFORE the view is entered (inside, a queued scan would walk `rows` instead of the table);
//   user_high, pm_bf16, their validity flags and m2d_mark_written are neither read, rebuilt nor touched inside it -- with both
//   options at 0 no launcher asks for them; the rows are finite while the engine's non-finite word is 0 (the composer sees to it).
// Only the table's plain pointer is swapped (pm.p): what the engine owns stays where it is, and the pointer goes back as found.
struct m2d_rows_view {
    m2d_engine *const h;
    const float *const pm;
    const int64_t U, user_base;
    const int opt_user_high, opt_pm_bf16;
    m2d_rows_view(m2d_engine *e, const float *rows, int64_t n)
        : h(e), pm(e->pm.p), U(e->U), user_base(e->user_base), opt_user_high(e->opt_user_high), opt_pm_bf16(e->opt_pm_bf16)
    {
        e->pm.p = rows; e->U = n; e->user_base = 0; e->opt_user_high = 0; e->opt_pm_bf16 = 0;
    }
    ~m2d_rows_view()
    {
        h->pm.p = pm; h->U = U; h->user_base = user_base; h->opt_user_high = opt_user_high; h->opt_pm_bf16 = opt_pm_bf16;
    }
    m2d_rows_view(const m2d_rows_view &) = delete;
    m2d_rows_view &operator=(const m2d_rows_view &) = delete;
};

inline int m2d_hip_failed(m2d_engine *h, const char *expr, const hipError_t e)
{
    h->last_error = std::string(expr) + ": " + hipGetErrorString(e);
    return M2D_ERR_HIP;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and size: a retrieval call makes six such calls, each a
// trip into the runtime, for a value that does not change (8 us of a 50 us host-side call)
// (The attribute belongs to the function ON A DEVICE, and a process may hold engines on several -- m2d_create(device): the
// cache is keyed by the current device as well; every entry point has already made the engine's device current.)
static inline hipError_t m2d_lds_limit(const void *fn, int bytes)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, int> seen;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_pair(dev, fn);
    auto it = seen.find(key);
    if (it != seen.end() && it->second >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) seen[key] = bytes;
    return e;
}

// a * x + b * y as TF's Mul, Mul, Add compute Model_Recommender.py:95-96: two rounded products, one rounded sum.
// __fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)) does not guarantee that -- the device library's bodies carry the `contract` flag,
// and hipcc 7.2 fused the second product into the add (v_fmac, one rounding fewer) in SOME copies of an unrolled loop: the same
// (user, dish) then scored one ulp apart depending on the slot it was computed in (m2d_catalogue_repair.hip, repair scan).  Plain
// operators under `fp contract(off)` carry no such flag, also after inlining.
__device__ __forceinline__ float m2d_blend_unfused(const float a, const float x, const float b, const float y)
{
#pragma clang fp contract(off)
    const float p = a * x;
    const float q = b * y;
    return p + q;
}

// One wave, one (user, dish) pair, any C and E: Model_Recommender.py:67-96 as written -- every product of every category, the rows
// of weight-0 categories included unless `skipm` (0 * inf = NaN, :82) -- lanes striding over e, one xor butterfly per sum.  Every
// lane returns the score.  um: the user's (C + 1) E floats, it: RE[d], mrow: the pair's C weights, hv: H[d] of the ingredient
// table or null.  Shared by m2d_score_pairs_generic (m2d_score.hip) and m2d_topk_literal (m2d_catalogue_dense.hip): the same
// (user, dish, mask) scores the same bits in both.
__device__ __forceinline__ float m2d_pair_score_wave(const float *um, const float *it, const float *mrow, const float *ce, const float *hv,
                                                     const int C, const int E, const float a, const float b, const bool skipm, const int lane)
{
    float hs = 0.f, ls = 0.f, n = 0.f;
    for (int c = 0; c < C; ++c) {
        const float mc = mrow[c];
        n += mc;                               // :77
        if (skipm && mc == 0.f) continue;      // 0 * row = 0: the row is not fetched
        for (int e = lane; e < E; e += 64) {
            if (!hv) hs = fmaf(um[e], mc * ce[(size_t)c * E + e], hs);          // :67, :71, :75
            ls = fmaf(it[e], mc * um[(size_t)(c + 1) * E + e], ls);             // :82, :86, :90
        }
    }
    if (hv)
        for (int e = lane; e < E; e += 64) hs = fmaf(um[e], hv[e], hs);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) hs += __shfl_xor(hs, off, 64);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ls += __shfl_xor(ls, off, 64);
    return m2d_blend_unfused(a, hv ? hs : hs / n, b, ls / n);                   // :79, :92, :95-96
}

// m2d_topk_users' order as ONE unsigned comparison: a smaller key comes earlier in the list.  High word: NaN -> all ones (after
// every -inf), otherwise the complement of the float's ascending-orderable image, -0 folded onto +0 (they tie); low word: the
// dish id.  Ids of a row are distinct, so the order is strict: whatever way a row's candidates are cut into ranges, waves and
// lanes, the first k of it are the same.  TKM_NONE (NaN, id -1) is "no entry": it loses against everything a launch can score.
constexpr uint64_t TKM_NONE = ~0ull;

__device__ __forceinline__ uint64_t tkm_key(const float s, const int32_t id)
{
    uint32_t hi = 0xFFFFFFFFu;
    if (s == s) {
        const uint32_t b = s == 0.f ? 0u : __float_as_uint(s);
        hi = (b & 0x80000000u) ? b : ~(b | 0x80000000u);      // ~(negative ? ~b : b | sign)
    }
    return ((uint64_t)hi << 32) | (uint32_t)id;
}

// ---- device helpers shared by the LDS-DMA kernels (m2d_catalogue_*.hip, m2d_mlp.hip) ----
// vmcnt(0) twice over: the builtin is an s_waitcnt the compiler's own counter model sees (so it stops assuming that
// loads from a previous loop trip are still in flight), the asm one cannot be optimised away on the grounds that
// the compiler knows of nothing outstanding (the DMA ops below are hidden from it).
static __device__ __forceinline__ void wait_all_vmem()
{
    __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0), expcnt / lgkmcnt untouched
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// LDS-DMA of 64 x 16 B: lane l's 16 bytes at `src` land at lds_base + 16 l.  Written as asm on purpose: after the
// builtin the compiler puts s_waitcnt vmcnt(0) in front of the next ds_read (it must assume the read aliases the
// DMA'd bytes), which serialises the NEXT stage's fill with the CURRENT stage's multiply.  Here a stage is
// published by an explicit vmcnt(0) + barrier before anyone reads it, so that wait is never needed.  The hidden
// VMEM op only makes the compiler's own vmcnt(N) waits more conservative (returns are in order), never less.
static __device__ __forceinline__ void lds_dma16(const void *src, const void *lds_base_uniform)
{
    const uint32_t m0v = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)lds_base_uniform);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(m0v) : "memory", "m0");
}

// the same through the compiler's builtin (the inline-asm form takes its 64-bit address in any VGPR pair; where the
// allocator picks an odd one hipcc 7.2 stops with "Subtarget requires even aligned vector registers")
static __device__ __forceinline__ void lds_dma16_b(const void *src, void *lds_base_uniform)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)lds_base_uniform, 16, 0, 0);
}

// launchers (m2d_score.hip / m2d_topk.hip); all enqueue on `stream` and return a status
int m2d_launch_score_pairs(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats,
                           bool by_dish, int64_t B, float *out, hipStream_t stream,
                           bool use_ingredients = false, bool may_use_mirror = true);   // false: exact f32 rows whatever "pm_bf16" says
int m2d_ensure_finite_scan(m2d_engine *h, hipStream_t stream);   // m2d_abi.hip: runs the queued table scan, if any
int m2d_launch_rows_finite_check(m2d_engine *h, const int32_t *users, int64_t B, hipStream_t stream);   // Personal_Memory rows of a batch
// m2d_ingredients.hip: H[d] of an ingredient table that is not the engine's yet (m2d_set_ingredients builds it aside) into `high` [I, E]
int m2d_launch_build_dish_high(m2d_engine *h, const float *ing, const int32_t *off, const int32_t *ids, const float *w, int64_t R,
                               float *high, hipStream_t stream);
int m2d_ensure_user_high(m2d_engine *h, hipStream_t stream);
int m2d_ensure_pm_bf16(m2d_engine *h, hipStream_t stream);
int m2d_launch_check_csr(m2d_engine *h, const int32_t *off, int64_t nnz, hipStream_t stream);        // a row pointer of I + 1 entries
// m2d_market.hip: latches the first recipe id outside [0, R); the filter behind m2d_cookable_dishes
int m2d_launch_check_recipe_ids(m2d_engine *h, const int32_t *ids, int64_t nnz, int64_t R, hipStream_t stream);
int m2d_launch_cookable(m2d_engine *h, const int32_t *market, int64_t nM, int32_t max_missing, int32_t *out_ids, int32_t *out_missing,
                        int64_t *out_count, hipStream_t stream);
// m2d_market_requests.hip: one (user, market) per request -- filter, score and list in one launch per batch; with `excl_off` the
// exclusion form of the kernel, with `out_missing` (and max_missing > 0) m2d_markets_missing after the rows are final
int m2d_launch_topk_markets(m2d_engine *h, const int32_t *users, int64_t nQ, const int64_t *market_off, const int32_t *market_ids,
                            int64_t nnzM, int32_t k, int32_t max_missing, float *out_scores, int32_t *out_ids, int32_t *out_counts,
                            hipStream_t stream, const int64_t *excl_off = nullptr, const int32_t *excl_ids = nullptr,
                            int32_t *out_missing = nullptr);
int m2d_ensure_dish_vectors(m2d_engine *h, hipStream_t stream);
int m2d_launch_write_memory(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats,
                            const float *sign, const float *labels, int64_t B, int32_t L, float *gm, float beta_1,
                            float beta_2, float alpha, int32_t which, double *out_sums, hipStream_t stream);
int m2d_train_setup(m2d_engine *h, int32_t learner, float lr, float clip_norm, hipStream_t stream);
void m2d_train_release(m2d_engine *h);   // deletes h->train, which frees what it owns
int m2d_launch_train_step(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats, const float *labels,
                          int64_t B, int32_t apply, float *out, hipStream_t stream);
int m2d_train_get_slot(m2d_engine *h, int32_t table, int32_t slot, float **dev, int64_t *count);
int m2d_train_step_count(m2d_engine *h, int64_t *steps, int32_t set);
int m2d_launch_score_pairs_mlp(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t B, float *out,
                               hipStream_t stream);
// m2d_mlp.hip: frees what is derived from the head's weights (mlp_w1x3, mlp_w1pad, mlp_w1pc: a new head rebuilds them)
void m2d_mlp_free_derived(m2d_engine *h);
int m2d_launch_rank_candidates(m2d_engine *h, const int32_t *users, const int32_t *items,
                               const int32_t *lens, int64_t nseg, int32_t L, int32_t k, float *out_scores,
                               int32_t *out_items, int32_t *out_flags, hipStream_t stream, bool head = false);
// m2d_topk_mlp.hip, the chunked head loop of m2d_topk_users_mlp (deep = false: m2d_topk_mlp_select, k <= 64) and m2d_topk_users_mlp_deep
// (deep = true: m2d_select_deep, k <= 1024).  excl_off: the exclusion forms -- the exact mode strikes each row's ids inside the selection;
// the two-stage mode takes its candidates from m2d_topk_users_excluding, once per call, or under `deep` from m2d_launch_deep_lists per
// user block
int m2d_launch_topk_users_mlp(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates, const int64_t *excl_off,
                              const int32_t *excl_ids, float *out_scores, int32_t *out_ids, bool deep, hipStream_t stream);
int m2d_launch_catalogue_rank_mlp(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t n, const int64_t *excl_off,
                                  const int32_t *excl_ids, int32_t *out_rank, float *out_scores, hipStream_t stream);
int m2d_launch_topk_users(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, float *out_scores,
                          int32_t *out_ids, hipStream_t stream);
// One selection request (m2d_select.hip): the k best of each of `rows` score rows of W columns, in tkm_key's order, as (score, id) lists
// in out_scores / out_ids [rows, k].  It is the kernels' one argument, by value.
struct SelectJob {
    const float *scores;                // column e of row r at scores[r * rs + e * es]
    int64_t rs, es;
    const int32_t *ids;                 // row r's ids at ids + r * ids_stride (0: one id row shared by all); null: column e is dish d0 + e
    int64_t ids_stride;
    int64_t rows, W;
    int32_t d0, k;
    int32_t first;                      // 1: the lists start with this block; 0: the k entries the outputs hold take part as k more candidates
    float *out_scores;
    int32_t *out_ids;
    // row r leaves out the ascending dish ids xids[xoff[r] .. xoff[r + 1]), *xend = the array's length (null: none).  With `ids` the id
    // row must be ascending (m2d_topk_menu_filtered); without, the strike works on the dish range d0 + e
    const int64_t *xoff;
    const int32_t *xids;
    const int64_t *xend;
    bool holes;                         // an id below 0 in `ids` is no entry whatever its score (candidates of a retrieval with exclusions)

    // the two layouts in use; k, the outputs and the exclusions are the caller's to name
    // dish-major range, as the head's pair generator leaves it: the `rows` scores of dish d0 + e are neighbours
    static SelectJob dish_major(const float *scores, const int64_t rows, const int64_t W, const int32_t d0)
    {
        SelectJob j{};
        j.scores = scores; j.rs = 1; j.es = rows;
        j.rows = rows; j.W = W; j.d0 = d0; j.first = d0 == 0 ? 1 : 0;
        return j;
    }
    // row-major [rows, W] with an id table (ids_stride W or 0), or without one: the dish range d0 + e
    static SelectJob row_major(const float *scores, const int64_t rows, const int64_t W, const int32_t *ids, const int64_t ids_stride,
                               const int32_t d0 = 0)
    {
        SelectJob j{};
        j.scores = scores; j.rs = W; j.es = 1;
        j.ids = ids; j.ids_stride = ids_stride;
        j.rows = rows; j.W = W; j.d0 = d0; j.first = d0 == 0 ? 1 : 0;
        return j;
    }
};
// m2d_select.hip: the one selection launcher.  deep = false: m2d_topk_mlp_select, a sorted list across a wave's lanes (k <= 64);
// deep = true: m2d_select_deep, a radix select on the key (1 <= k <= 1024).  Which one is the caller's choice.
int m2d_launch_select(m2d_engine *h, const SelectJob &job, bool deep, hipStream_t stream);
// threads of a selection / count block: a wave for the reranker's short rows, sixteen for a catalogue-wide range (few rows then share
// the device: a block of P / W rows)
static inline int select_threads(const int64_t W) { return W <= 256 ? 64 : W <= 16384 ? 256 : 1024; }
// the block rule of every call that scores blocks of rows into P pairs of scratch, W columns a row: max(1, P / W) rows, no more than n
static inline int64_t m2d_block_rows(const int64_t P, const int64_t W, const int64_t n)
{
    const int64_t R0 = P / W > 1 ? P / W : 1;
    return R0 < n ? R0 : n;
}
// m2d_slate.hip, the deep catalogue lists (m2d_topk_users_deep).  m2d_deep_conditions: the slate launcher's table conditions without its
// head refusal, under the name `entry`.  m2d_launch_deep_lists: the blocks and ranges of `nU` users whose conditions and exclusion
// lists the caller has checked -- excl_off: these users' offsets (null: none), excl_end: where the array's length stands,
// index_base: the position of users[0] in the call's array, for the error latch
int m2d_deep_conditions(m2d_engine *h, const char *entry, hipStream_t stream);
int m2d_launch_deep_lists(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int64_t *excl_off, const int32_t *excl_ids,
                          const int64_t *excl_end, int64_t index_base, float *out_scores, int32_t *out_ids, hipStream_t stream);
int m2d_launch_topk_users_deep(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int64_t *excl_off, const int32_t *excl_ids,
                               float *out_scores, int32_t *out_ids, hipStream_t stream);
// m2d_slate.hip: what the slate score kernels take, by value
struct SlateArgs {
    const float *pm;        // [U, K]
    const float *dt;        // Dt_s [rows, Kp]
    const float *zero;      // Dt_s's last row: Kp zeros
    const int32_t *users;   // [nU] global ids
    int64_t nU, U, user_base;
    int64_t index_base;     // position of users[0] in the caller's array (m2d_topk_slate's user blocks), for the error latch
    int64_t nD;
    int64_t utiles, dtiles;
    int32_t K, Kp;
    float *out;             // [nU, nD]
    int32_t *err;
};
// m2d_slate.hip's slate_prepare / launch_scores for other launchers: the call's slate vectors in slate_dt (`slate` null: the dishes
// d0 .. d0 + nD - 1) and everything of `a` but users, nU, index_base and out; then one score launch of a.nU rows into a.out [nU, nD]
int m2d_slate_prepare(m2d_engine *h, const int32_t *slate, int32_t d0, int64_t nD, SlateArgs &a, bool &mfma, hipStream_t stream);
int m2d_launch_slate_scores(m2d_engine *h, SlateArgs &a, bool mfma, hipStream_t stream);
// m2d_groups.hip: one launcher behind m2d_topk_groups (slate == null), m2d_topk_groups_slate (out == null) and m2d_score_groups_slate
// (out: f32[nG, nD]); the arguments are checked by the ABI layer
int m2d_launch_groups(m2d_engine *h, const char *entry, const int32_t *members, int64_t nG, int32_t M, int32_t mode, const int32_t *slate,
                      int64_t nD, int32_t k, const int64_t *excl_off, const int32_t *excl_ids, float *out, float *out_scores,
                      int32_t *out_ids, hipStream_t stream);
// m2d_groups.hip, for m2d_plan_groups' walk (m2d_menu.hip).  m2d_launch_group_prepare: the member check and, with member_caps, the cap
// fold (m2d_group_caps) -- *dense i32[nG M] valid ids, *cnt i32[nG], *group_caps / *group_plan_caps i32[nG, C] (written only with
// member_caps; the latter null without member_plan_caps).  m2d_launch_group_reduce: groups' first cnt rows of src [groups, M, W] folded
// into dst + g dst_rs under `mode`
int m2d_launch_group_prepare(m2d_engine *h, const int32_t *members, int64_t nG, int32_t M, const int32_t *member_caps,
                             const int32_t *member_plan_caps, const int32_t **dense, const int32_t **cnt, const int32_t **group_caps,
                             const int32_t **group_plan_caps, hipStream_t stream);
int m2d_launch_group_reduce(m2d_engine *h, int mode, const float *src, const int32_t *cnt, int64_t groups, int M, int64_t W, float *dst,
                            int64_t dst_rs, hipStream_t stream);
// m2d_menu.hip: m2d_topk_menu behind the ABI layer's argument checks -- caps i32[nU, C], C <= M2D_MENU_MAX_CATEGORIES
int m2d_launch_topk_menu(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int32_t *caps, float *out_scores,
                         int32_t *out_ids, hipStream_t stream);
// m2d_topk_menu_filtered: the same loop over slate \ exclusions (excl_off null: no exclusions; slate null: the whole catalogue; both
// null: m2d_launch_topk_menu's launches under the name `entry`)
int m2d_launch_topk_menu_filtered(m2d_engine *h, const char *entry, const int32_t *users, int64_t nU, int32_t k, const int32_t *caps,
                                  const int64_t *excl_off, const int32_t *excl_ids, const int32_t *slate, int64_t nD, float *out_scores,
                                  int32_t *out_ids, hipStream_t stream);
// m2d_plan_menus: the same loop with lists of days * k and m2d_plan_merge behind it (plan_caps null: no cap over the plan); the
// outputs are [nU, days, k]
int m2d_launch_plan_menus(m2d_engine *h, const int32_t *users, int64_t nU, int32_t days, int32_t k, const int32_t *caps,
                          const int32_t *plan_caps, const int64_t *excl_off, const int32_t *excl_ids, const int32_t *slate, int64_t nD,
                          float *out_scores, int32_t *out_ids, hipStream_t stream);
// m2d_plan_groups: the same loop with a group of M member slots per row -- the members' rows scored, reduced under `mode` into the
// group's row 0 and listed from there; caps_per_member: both cap tables are [nG, M, C] and are folded first; the outputs are [nG, days, k]
int m2d_launch_plan_groups(m2d_engine *h, const int32_t *members, int64_t nG, int32_t M, int32_t mode, int32_t days, int32_t k,
                           const int32_t *caps, const int32_t *plan_caps, bool caps_per_member, const int64_t *excl_off,
                           const int32_t *excl_ids, const int32_t *slate, int64_t nD, float *out_scores, int32_t *out_ids, hipStream_t stream);
// m2d_slate.hip: out == null: the scores of user blocks go to scratch and the lists of k to out_scores / out_ids
int m2d_launch_slate(m2d_engine *h, const char *entry, const int32_t *users, int64_t nU, const int32_t *slate, int64_t nD, int32_t k,
                     float *out, float *out_scores, int32_t *out_ids, hipStream_t stream);
// m2d_catalogue_plan.hip: the host's copy of the "a table value is not finite" word (grp_nonfinite), read again if a writer made it stale
int m2d_refresh_nonfinite(m2d_engine *h, hipStream_t stream);
int m2d_launch_catalogue_rank(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t n, const int64_t *excl_off,
                              const int32_t *excl_ids, int32_t *out_rank, float *out_scores, hipStream_t stream);
// entry: the name its refusals carry; under_head: the caller ranks the lists under the MLP head afterwards (m2d_topk_users_mlp_excluding)
int m2d_launch_topk_users_excluding(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int64_t *excl_off,
                                    const int32_t *excl_ids, float *out_scores, int32_t *out_ids, hipStream_t stream,
                                    const char *entry = "m2d_topk_users_excluding", bool under_head = false);
// m2d_catalogue_excl.hip: the one whole-list check of a call's exclusion lists (n rows: offsets off[0 .. n], ids[off[n]]) -- what it
// finds goes to the id-error latch
int m2d_launch_check_exclusions(m2d_engine *h, const int64_t *off, const int32_t *ids, int64_t n, hipStream_t stream);
