// The launch policy of a pattern-grouped retrieval call (launch_grouped, m2d_catalogue_plan.hip): everything the launcher decides
// before it touches memory, as one function of plain values -- no HIP, no engine -- so that the measured rules below can be run on a
// CPU (tests/c_abi/grouped_policy_table.cpp, tests/test_grouped_policy_cpu.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

// "variant" >= 100, test hook: force the number of dish-range splits of a retrieval launch (variant - 100, within 1 .. max_splits)
inline int topk_split_hook(const int variant, int nsplit, const int max_splits)
{
    if (variant >= 100) {
        nsplit = variant - 100;
        if (nsplit < 1) nsplit = 1;
        if (nsplit > max_splits) nsplit = max_splits;
    }
    return nsplit;
}

struct GroupedPolicyIn {
    int E;                     // the tables' embedding size
    int E8;                    // the scan kernel's row width / 8 (E, or the next instantiated width when PAD; 2 E / 8 with HV)
    int KR;                    // list slots per lane (10 or 16 >= k)
    bool BF16X3;               // split-bf16 MFMA, else exact f32
    bool HV;                   // rows [H[d] | RE[d]] of the ingredient table (pipelined split-bf16 kernel only)
    bool PAD;                  // zero-padded rows (exact f32 only)
    int k;
    int64_t nU;
    int64_t tiles;             // 32-dish tiles of the sorted table
    int num_cu;
    int topk_form, topk_prune, topk_block, topk_refine, variant;   // the options of those names
    // what the kernels' header fixes (m2d_catalogue.h, m2d_catalogue_plan.hip), passed in so that this file includes neither
    int tiles_per_stage;       // grouped_tiles_per_stage(8 E8): tiles of a stage of an eight-wave block
    bool half_blocks;          // M2D_TOPK_HALF_BLOCKS: the launcher's own choice of 128-user blocks is compiled in
    int max_probes;            // PLAN_PROBES
    int repair_cap;            // REPAIR_CAP
};

struct GroupedPolicy {
    bool pipe;                 // split bf16: the pipelined form (else the first form)
    bool apx;                  // hi x hi product first, cross products for the tiles with a candidate
    bool half;                 // blocks of 128 users (four waves)
    int WV;                    // waves per block
    int TPS;                   // tiles per stage
    size_t lds;                // bytes of LDS of the scan
    int64_t ublocks;           // user blocks
    int nsplit;                // dish ranges
    bool planned;              // the scan takes a plan (all but the first-form bf16 kernel)
    bool ext;                  // the lists' left-out records are kept for m2d_topk_refine
    bool sorted;               // users sorted by pattern mask
    int pmode;                 // the plan kernel's mode: 1 = no pruning, 2 / 4 = "topk_prune" 2 / 4, 0 = the default bound
    int nprobe;                // probe rows per user of the plan kernel
    int plan_quads;            // the plan kernel's instantiation: 1 / 2 / 4 for E <= 64 / <= 128 / beyond
    bool share_thresholds;     // dish ranges of a user share their thresholds
    bool deal_items;           // (user block, dish range) items are handed out longest first
    int prog_limit;            // polls of the progress words before a wave gives up
    int all_patterns;          // 1: the repair reads every pattern's dishes
    int cap;                   // listed users the repair's scan / merge pair handles
};

constexpr int GROUPED_WAVES = 8;                           // waves per block unless the launcher takes blocks of 128 users (`half`)

// shared tail of every MFMA retrieval launch: dish-range splits -> partial lists in scratch.  The grouped kernels run
// ONE block per CU (128 KiB of LDS), so the grid is ublocks x nsplit blocks dealt out in rounds of num_cu: the fewest
// splits whose last round is at least 90 % full are taken (each split repeats the early, insertion-heavy part of a
// scan and adds a merge pass: 65 536 users x 100 k dishes ran 3.69 ms with 2 splits and 2.91 ms with 1).  Few users:
// up to max_splits blocks per user block, so that a single query still uses the whole chip.
inline int grouped_pick_splits(const int num_cu, const int variant, const int64_t ublocks, const int64_t tiles, const int64_t min_tiles_per_split,
                               const int max_splits)
{
    const int64_t cus = num_cu;
    int64_t cap = tiles / min_tiles_per_split > 1 ? tiles / min_tiles_per_split : 1;
    if (cap > max_splits) cap = max_splits;
    int64_t lim = (2 * cus + ublocks - 1) / ublocks;        // beyond two rounds' worth of blocks nothing is gained
    if (lim < 1) lim = 1;
    if (lim > cap) lim = cap;
    int nsplit = 1;
    double best = 0.0;
    for (int64_t ns = 1; ns <= lim; ++ns) {
        const int64_t blocks = ublocks * ns, rounds = (blocks + cus - 1) / cus;
        const double fill = (double)blocks / (double)(rounds * cus);
        if (fill > best + 1e-9) { best = fill; nsplit = (int)ns; }
        if (fill >= 0.9) break;
    }
    nsplit = topk_split_hook(variant, nsplit, max_splits);
    if (nsplit > 64) nsplit &= ~63;    // two-pass merge: whole groups of 64
    return nsplit;
}

inline GroupedPolicy grouped_policy(const GroupedPolicyIn &in)
{
    GroupedPolicy p;
    const int E = in.E8 * 8;
    const bool BF16X3 = in.BF16X3, HV = in.HV;
    // "topk_form" (split-bf16 kernels): 0 or 2 = pipelined form (E = 64: 2.55 ms against 3.3 at 100 k dishes; E = 128:
    // 38.3 ms against 45.4 at 1 M dishes), 1 = first form (kept as the A/B reference; it takes no plan)
    p.pipe = HV || in.topk_form != 1;
    p.planned = !BF16X3 || p.pipe;
    // Blocks of 128 users (four waves, half-size stages, two blocks per CU) for pruned launches of the pipelined kernel at
    // E = 64: a stage barrier holds up four waves instead of eight, the CU's other block runs meanwhile, and 128 users share
    // fewer patterns than 256 (tiles stepped through 0.109 -> 0.100 of the catalogue).  Measured, k = 10: 65 536 users x 100 k
    // dishes 0.629 -> 0.584 ms, 262 144 users 2.10 -> 1.99 ms, 16 384 users 0.384 -> 0.376 ms; but every block streams its own
    // copy of the tiles, and once the catalogue image (8 KiB a tile) no longer sits in the Infinity Cache that costs more than
    // the barriers did -- 1 M dishes: 65 536 users 3.19 -> 3.24 ms, 262 144 users 10.7 -> 11.4 ms -- so: catalogues up to 8 192
    // tiles (64 MiB of image).  "topk_block" = 128 / 256 forces either.
    const bool half_ok = BF16X3 && !HV && E == 64 && p.pipe;
    // (k > 10 with the left-out bookkeeping: 232 registers since the launch bounds say two waves per SIMD -- it took 261 and one
    //  wave per SIMD before, and the launcher kept eight-wave blocks for it: 65 536 users x 100 k dishes, k = 16: 0.764 -> 0.666 ms)
    // The hi x hi first form of that kernel (APX in m2d_catalogue_scan_bf16.hip) for the catalogues where a tile with a candidate is
    // the exception.  It pays once fewer than about a quarter (E = 64) / a half (E = 128) of the (wave, tile) pairs still need their
    // cross products -- 65 536 users, pruned, three-product form against it: E = 64 200 k dishes 0.73 / 0.88 ms, 500 k 1.51 / 1.63,
    // 1 M 2.81 / 2.63; E = 128 300 k 1.94 / 1.94, 500 k 2.96 / 2.75, 1 M 6.16 / 4.95 -- so: more than 24 576 tiles at E = 64, more
    // than 10 240 at E = 128.  The rule looks at the catalogue alone: that form's scores are not the three-product kernels' bits, and
    // every launch shape of one problem must return the same lists (blocks of 256 users there: "topk_block" = 128 is not
    // honoured).  "topk_form" 3 / 4 (diagnostic): that form for any catalogue / never.
    // (The ingredient form multiplies every tile -- no pattern can be pruned -- so tiles with a candidate are the exception from
    //  small catalogues on: 65 536 users x 20 k dishes 0.89 -> 0.64 ms, 100 k 3.79 -> 2.09 ms, 1 M 36.3 -> 18.5; more than 256 tiles.)
    p.apx = BF16X3 && p.pipe && (E == 64 || E == 128) && in.topk_form != 4 &&
            (in.tiles > (HV ? 256 : (E == 64 ? 24576 : 10240)) || in.topk_form == 3);
    p.half = half_ok && !p.apx && (in.topk_block == 128 || (in.topk_block == 0 && in.half_blocks && in.topk_prune != 0 &&
                                                            in.variant < 100 && in.nU >= 16384 && in.tiles <= 8192));
    p.WV = p.half ? 4 : GROUPED_WAVES;
    p.TPS = in.tiles_per_stage * p.WV / GROUPED_WAVES;
    p.lds = (size_t)2 * p.TPS * 32 * E * sizeof(float);
    p.prog_limit = in.variant == 15 ? 0 : (1 << 24);      // "variant" 15: test hook of the progress-word timeout
    const int64_t ublocks = p.ublocks = (in.nU + 32 * p.WV - 1) / (32 * p.WV);
    int nsplit = grouped_pick_splits(in.num_cu, in.variant, ublocks, in.tiles, 2 * p.TPS, 512);
    if ((!BF16X3 || (!HV && in.topk_form != 1)) && in.topk_prune != 0 && in.variant < 100) {
        // Pattern pruning makes the blocks unequal -- a block of users with one relevant pattern steps through a fifteenth of
        // the catalogue, one whose users need most patterns through all of it -- so a launch with many user blocks is cut into
        // dish ranges and the (block, range) items are handed out longest first (m2d_plan_items_*).  The longest item bounds
        // the launch, every piece starts its lists from the scan-start bound again (more pieces re-insert more): measured
        // best at 100 k dishes, E = 64 -- 16 / 32 user blocks: 32 ranges (0.30 / 0.33 ms; 8 ranges 0.56), 64 blocks: 16
        // (0.42 ms; 8: 0.59, 32: 0.49), 128 blocks: 12 (0.58 ms; 8: 0.62, 24: 0.68), 256 blocks: 8 (0.85 ms; 16: 1.0).
        // 8 blocks: 64 (0.21 ms; 32: 0.25).  A handful of blocks (serving): most ranges hold no tile of the users' patterns and
        // return at once, the others are short -- 1 user: 512 ranges 0.056 ms (192, the unpruned launch's count: 0.066), 32
        // users 0.068 (0.091), 256 users: 256 ranges 0.101 (0.113), 1 024 users: 128 ranges 0.167 (0.185).
        if (ublocks >= 6) {
            nsplit = ublocks >= 192 ? 8 : (ublocks >= 96 ? 12 : (ublocks >= 48 ? 16 : (ublocks >= 24 ? 32 : (int)(512 / ublocks))));
            // long catalogues: since a user's ranges share their thresholds, twice the ranges cost little and balance better
            // (65 536 users x 1 M dishes: 8 ranges 3.41 ms, 16 ranges 3.19 ms, 24: 3.32; 262 144 users: 8 ranges 10.7, 16: 11.2)
            if (BF16X3 && E == 64 && in.tiles >= 16384 && ublocks >= 192 && ublocks < 768) nsplit = 16;
            // blocks of 128 users, many of them: about 4 096 items is what balances (8 rounds of the 512 block slots); more only
            // adds item prologues, partial stages and merge work -- 131 072 users x 100 k dishes: 4 ranges 0.87 ms (3: 0.95, 6:
            // 0.90, 8: 0.95); 262 144 users: 2 ranges 1.59 (1: 2.11, 3: 1.65, 4: 1.66, 8: 1.85); 524 288 users: 1 range 2.86
            // (2: 2.99, 4: 3.24, 8: 3.67).  (Blocks of 256 users over 1 M dishes: 8 stays -- 262 144 users 10.2 ms against 10.6
            // with 3 ... 6; 524 288 users 19.3 ... 20.2 for 2 ... 8, within the noise.)
            if (p.half && ublocks >= 768) nsplit = ublocks >= 3072 ? 1 : (ublocks >= 1536 ? 2 : 4);
            const int64_t most = in.tiles / (4 * p.TPS);     // at least four stages per range
            if (most < nsplit) nsplit = most > 1 ? (int)most : 1;
        } else {
            nsplit = ublocks == 1 ? (in.nU <= 64 ? 512 : 256) : (int)(512 / ublocks);
            const int64_t most = in.tiles / 4;               // at least four tiles per range
            if (most < nsplit) nsplit = most > 1 ? (int)most : 1;
        }
        if (nsplit > 64) nsplit &= ~63;                      // two-pass merge: whole groups of 64 (6 or 7 blocks: 85 / 73 -> 64)
    }
    p.nsplit = nsplit;
    // what the lists leave out, for m2d_topk_refine (kernels that keep it: see EXT in the scan kernels)
    // (a user's word is its position in the call | left-out dishes to take along << 30: calls of 2^30 users or more go without)
    p.ext = p.planned && in.topk_refine != 0 && !HV && !in.PAD && in.nU < ((int64_t)1 << 30) &&
            (BF16X3 ? (p.pipe && !(E == 128 && in.KR == 16)) : in.E8 <= 16);
    // the call's plan: per user the scan-start bound, <U_high, CE_c> and the mask of patterns that can reach the
    // top-k; users sorted by mask so that a block's 256 users share their patterns (a single block: no sort)
    const bool prune = in.topk_prune != 0;
    p.sorted = p.planned && prune && !HV && in.nU > 32 * p.WV;
    p.pmode = (HV || !prune) ? 1 : (in.topk_prune == 2 ? 2 : (in.topk_prune == 4 ? 4 : 0));
    // probe rows per user: each costs a row read per user (16: +18 us for 65 536 users) and buys a tighter bound -- 16 rows
    // at 100 k dishes (0.71 ms; 32: 0.73), 32 at 1 M (3.83 ms; 16: 4.02)
    p.nprobe = in.tiles < 8192 ? 16 : (in.tiles < 65536 ? 32 : in.max_probes);
    p.plan_quads = in.E <= 64 ? 1 : (in.E <= 128 ? 2 : 4);
    // dish ranges of a user share their thresholds (pipelined kernel; "topk_prune" = 7 keeps them apart: A/B)
    p.share_thresholds = BF16X3 && p.pipe && !HV && E == 64 && nsplit > 1 && in.topk_prune != 7;
    p.deal_items = p.sorted && ublocks * nsplit > (int64_t)in.num_cu && in.topk_prune != 5;      // 5: grid order (A/B)
    p.all_patterns = in.topk_prune == 9 ? 1 : 0;             // "topk_prune" = 9: the repair reads every pattern (A/B)
    p.cap = in.variant == 13 ? 2 : in.repair_cap;           // test hook: send all but two listed users to the one-block-per-user kernel
    return p;
}
