// Build-defined extension (no reference counterpart): m2d_topk_menu, the k best dishes of the whole catalogue
// under per-category caps -- at most cap[u][c] listed dishes of category c.
//
//   sig(d)  = the C-bit mask of dish d's categories (cats[d][c] != 0.0f; C <= 6: at most 64 signatures, one per lane of a wave)
//   menu(u) = the greedy walk of m2d_topk_users' order that takes a dish iff none of its categories is at its cap
//
// The identity the call rests on (tests/test_menu_cases_cpu.py): a category that is at its cap stays there, so a signature that
// stops being admissible never returns, and while it is admissible the walk takes its dishes in the order's own sequence -- the walk
// never reaches past the k best dishes OF A SIGNATURE.  The menu over the full order is therefore the menu over the merge of each
// signature's own top-k list, and those lists are what the engine already computes: a signature's dishes, ascending, are a slate.
//
// Signature index (once per mask table): perm[I], the dish ids by (signature, id), and seg_off[65].  The market filter's three passes,
// ascending by construction -- no sort, no atomic cursor, no block waits for another:
//   m2d_menu_flag    a lane per dish: sig[d], and per block of 256 dishes the number of dishes of each signature (six ballots give
//                    lane s the wave's dishes of signature s)
//   m2d_menu_scan    one block: per signature the exclusive scan of the block counts, offset by the signatures in front: every
//                    (block, signature) base, and seg_off
//   m2d_menu_write   each dish lands at its block's base for its signature + the waves in front + the popcount of its signature's
//                    ballot below its lane
// The build reads seg_off to the host (ONE stream synchronisation per mask table); the calls after it do not synchronise.
//
// A call (m2d_launch_topk_menu): per block of Ub users and non-empty segment, ranges of W = min(n_s, P, 65536) dishes go through
// m2d_slate_prepare / m2d_launch_slate_scores / m2d_launch_select (ids = the range of perm, one id row for all) into list scratch
// [S', Ub, k]; m2d_menu_merge then walks the S' lists of a user in one wave.
//
// m2d_topk_menu_filtered: the same walk over the dishes of a slate, less each user's exclusion segment.
// Removing dishes leaves the identity intact -- the menu over the allowed order is the menu over the merge of each signature's first
// k ALLOWED dishes.  Exclusions: a range of a segment is an ascending id table, so the selection strikes the row's ascending exclusion
// segment against it (SelectJob::xoff with ids; ExclCursor::strike_ids).  Slate: its own index (menu_slate_index: the three passes
// over the slate, reading the resident signature bytes), ONE STREAM SYNCHRONISATION PER CALL WITH A SLATE for the 64 segment sizes.
// One loop (menu_walk) serves both forms; with null filters it is m2d_topk_menu's launches.
//
// m2d_plan_menus: `days` menus with no dish twice, day caps and caps over the whole plan.  A walk takes a
// signature's dishes as a prefix of its own order, so the days are one walk over lists of L = days k with cursors that persist:
// menu_walk with lists of L (above 64: the radix selection) and m2d_plan_merge behind them; days == 1 without plan caps is
// m2d_topk_menu_filtered's launches.
//
// m2d_plan_groups: the same plan for a GROUP of users.  A row of the walk is a group of M member slots:
// m2d_group_members / m2d_group_caps run first (m2d_groups.hip), a block's Gb M member rows are scored into [Gb M, W],
// m2d_group_reduce folds each group's rows into its row 0 and the selection lists that row (row stride M W).  Everything behind the
// lists -- the prefix argument, the merges -- sees score words per row and dish and nothing of where they came from.
#include "m2d_engine.h"

namespace {

constexpr int MN_WAVES = 4;                    // waves per block of the index passes
constexpr int MN_DB = 64 * MN_WAVES;           // dishes per block (one per lane)
constexpr int MN_SIGS = 64;                    // signatures: 2^M2D_MENU_MAX_CATEGORIES
constexpr int MN_SCAN_WAVES = 16;

// The live lanes of the wave whose signature is `t` (t may differ per lane): six ballots, one per category bit.  Every lane of the
// wave calls it (full EXEC).
__device__ __forceinline__ unsigned long long menu_same_sig(const unsigned sig, const bool live, const unsigned t)
{
    unsigned long long m = __ballot(live);
#pragma unroll
    for (int c = 0; c < M2D_MENU_MAX_CATEGORIES; ++c) {
        const unsigned long long b = __ballot(live && ((sig >> c) & 1u));
        m &= ((t >> c) & 1u) ? b : ~b;
    }
    return m;
}

__global__ __launch_bounds__(MN_DB) void m2d_menu_flag(const float *cats, int64_t I, int C, uint8_t *sig, int32_t *counts)
{
    __shared__ int32_t wave_cnt[MN_WAVES][MN_SIGS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t d = ((int64_t)blockIdx.x * MN_WAVES + wave) * 64 + lane;
    const bool live = d < I;
    unsigned s = 0;
    if (live) {
        const float *row = cats + (size_t)d * C;
        for (int c = 0; c < C; ++c) s |= row[c] != 0.0f ? 1u << c : 0u;      // -0.0 is no member, a NaN weight is one
        sig[d] = (uint8_t)s;
    }
    wave_cnt[wave][lane] = __popcll(menu_same_sig(s, live, (unsigned)lane));
    __syncthreads();
    if (threadIdx.x < MN_SIGS) {
        int32_t n = 0;
        for (int w = 0; w < MN_WAVES; ++w) n += wave_cnt[w][threadIdx.x];
        counts[(size_t)blockIdx.x * MN_SIGS + threadIdx.x] = n;
    }
}

// one block of 16 waves: lane s of wave w owns signature s over the w-th share of the blocks
__global__ __launch_bounds__(64 * MN_SCAN_WAVES) void m2d_menu_scan(const int32_t *counts, int64_t nb, int32_t *base, int32_t *seg_off)
{
    __shared__ int32_t part[MN_SCAN_WAVES][MN_SIGS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t per = (nb + MN_SCAN_WAVES - 1) / MN_SCAN_WAVES;
    const int64_t b0 = wave * per < nb ? wave * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
    int32_t s = 0;
    for (int64_t b = b0; b < b1; ++b) s += counts[(size_t)b * MN_SIGS + lane];
    part[wave][lane] = s;
    __syncthreads();
    int32_t total = 0, before = 0;
    for (int w = 0; w < MN_SCAN_WAVES; ++w) {
        const int32_t v = part[w][lane];
        before += w < wave ? v : 0;
        total += v;
    }
    int32_t upto = total;                       // inclusive scan of the signatures' sizes over the lanes (every lane takes part)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t v = __shfl_up(upto, o, 64);
        upto += lane >= o ? v : 0;
    }
    if (wave == 0) {
        seg_off[lane] = upto - total;
        if (lane == 63) seg_off[MN_SIGS] = upto;
    }
    int32_t run = upto - total + before;
    for (int64_t b = b0; b < b1; ++b) {
        base[(size_t)b * MN_SIGS + lane] = run;
        run += counts[(size_t)b * MN_SIGS + lane];
    }
}

// `src` (the slate form): entry d of the index is the slate's d-th id, not d itself
__global__ __launch_bounds__(MN_DB) void m2d_menu_write(const uint8_t *sig, const int32_t *base, int64_t I, const int32_t *src, int32_t *perm)
{
    __shared__ int32_t wave_cnt[MN_WAVES][MN_SIGS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t d = ((int64_t)blockIdx.x * MN_WAVES + wave) * 64 + lane;
    const bool live = d < I;
    const unsigned s = live ? sig[d] & (MN_SIGS - 1) : 0u;
    const unsigned long long mine = menu_same_sig(s, live, s);
    wave_cnt[wave][lane] = __popcll(menu_same_sig(s, live, (unsigned)lane));
    __syncthreads();
    if (live) {
        int64_t at = base[(size_t)blockIdx.x * MN_SIGS + s];
        for (int w = 0; w < wave; ++w) at += wave_cnt[w][s];
        at += __popcll(mine & ((1ull << lane) - 1ull));
        if (at >= 0 && at < I) perm[at] = src ? src[d] : (int32_t)d;       // (the counts make it so: perm cannot be overrun whatever they are)
    }
}

// The flag pass over a slate (m2d_topk_menu_filtered): lane i reads sig[slate[i]] from the catalogue index's resident signature bytes
// into ssig[i], and checks the caller's slate by m2d_topk_slate's convention -- an id outside [0, I) is M2D_ERR_BAD_ITEM_ID at its
// index (it indexes nothing: signature 0), an entry not above its predecessor M2D_ERR_INVALID_ARG at its index (a predecessor that is
// itself out of range is reported by its own lane).
__global__ __launch_bounds__(MN_DB) void m2d_menu_flag_slate(const int32_t *slate, int64_t nD, int64_t I, const uint8_t *sig, uint8_t *ssig,
                                                             int32_t *counts, int32_t *err)
{
    __shared__ int32_t wave_cnt[MN_WAVES][MN_SIGS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = ((int64_t)blockIdx.x * MN_WAVES + wave) * 64 + lane;
    const bool live = i < nD;
    unsigned s = 0;
    if (live) {
        const int32_t d = slate[i];
        if (d < 0 || (int64_t)d >= I) {
            m2d_latch_error(err, M2D_ERR_BAD_ITEM_ID, d, i);
        } else {
            s = sig[d] & (MN_SIGS - 1);
            if (i > 0) {
                const int32_t prev = slate[i - 1];
                if (prev >= 0 && (int64_t)prev < I && prev >= d) m2d_latch_error(err, M2D_ERR_INVALID_ARG, d, i);
            }
        }
        ssig[i] = (uint8_t)s;
    }
    wave_cnt[wave][lane] = __popcll(menu_same_sig(s, live, (unsigned)lane));
    __syncthreads();
    if (threadIdx.x < MN_SIGS) {
        int32_t n = 0;
        for (int w = 0; w < MN_WAVES; ++w) n += wave_cnt[w][threadIdx.x];
        counts[(size_t)blockIdx.x * MN_SIGS + threadIdx.x] = n;
    }
}

// ---- the constrained merge -----------------------------------------------------------------------------------------------------
// One wave per user.  Lane s is signature s: a cursor into segment s's list of k (the j-th list of the scratch, j = the non-empty
// segments in front of s) and the tkm_key of the entry under it.  `full` -- wave-uniform -- holds the categories at their cap; a lane
// is admissible while its signature shares no bit with it and its list has an entry left.  A step takes the least key over the
// admissible lanes (a butterfly of 64-bit minima), lane t of the wave keeps the t-th entry taken, the winner moves on, the winner's
// categories count.  Ids are distinct across segments, so the minimum names one lane.  The row is written once, k lanes side by
// side; what no step filled is id -1 / the fill NaN.  A cap below 0 is latched (value: the cap, position: u C + c) and counts as 0.
struct MenuMergeArgs {
    const float *list_scores;           // [S', Ub, k]
    const int32_t *list_ids;
    const int32_t *seg_off;             // [65]
    const int32_t *caps;                // [n, C]: the block's rows
    int64_t n, Ub, index_base;
    int32_t k, C;
    float *out_scores;                  // [n, k]: the block's rows
    int32_t *out_ids;
    int32_t *err;
};

__global__ __launch_bounds__(256) void m2d_menu_merge(const MenuMergeArgs p)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + wave;
    if (r >= p.n) return;                       // wave-uniform
    const int k = p.k;

    const bool have = p.seg_off[lane + 1] > p.seg_off[lane];
    const int j = __popcll(__ballot(have) & ((1ull << lane) - 1ull));

    int32_t capv = 0;
    if (lane < p.C) {
        capv = p.caps[(size_t)r * p.C + lane];
        if (capv < 0) m2d_latch_error(p.err, M2D_ERR_INVALID_ARG, capv, (p.index_base + r) * p.C + lane);
    }
    int32_t cap[M2D_MENU_MAX_CATEGORIES], cnt[M2D_MENU_MAX_CATEGORIES];
    unsigned full = 0;
#pragma unroll
    for (int c = 0; c < M2D_MENU_MAX_CATEGORIES; ++c) {
        cap[c] = __builtin_amdgcn_readlane(capv, c);
        cnt[c] = 0;
        if (c < p.C && cap[c] <= 0) full |= 1u << c;
    }

    const size_t lrow = ((size_t)j * p.Ub + r) * k;
    int cur = 0;
    uint64_t key = TKM_NONE;
    uint32_t word = 0x7FC00000u;
    const auto load = [&]() {                   // the entry under the cursor, or no entry: the list's end, an id below 0
        key = TKM_NONE;
        if (have && cur < k) {
            const int32_t id = p.list_ids[lrow + cur];
            if (id >= 0) {
                const float s = p.list_scores[lrow + cur];
                word = __float_as_uint(s);
                key = tkm_key(s, id);
            }
        }
    };
    load();

    int32_t oid = -1;
    uint32_t ow = 0x7FC00000u;
    for (int t = 0; t < k; ++t) {               // wave-uniform: best, win and full are the same in every lane
        const bool adm = key != TKM_NONE && ((unsigned)lane & full) == 0u;
        uint64_t best = adm ? key : TKM_NONE;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint64_t o = __shfl_xor((unsigned long long)best, off, 64);
            best = o < best ? o : best;
        }
        if (best == TKM_NONE) break;
        const int win = __ffsll((unsigned long long)__ballot(adm && key == best)) - 1;
        const uint32_t bw = (uint32_t)__shfl((int)word, win, 64);
        if (lane == t) {
            oid = (int32_t)(uint32_t)(best & 0xFFFFFFFFu);
            ow = bw;
        }
#pragma unroll
        for (int c = 0; c < M2D_MENU_MAX_CATEGORIES; ++c)
            if ((win >> c) & 1) {
                cnt[c] += 1;
                if (cnt[c] >= cap[c]) full |= 1u << c;
            }
        if (lane == win) {
            ++cur;
            load();
        }
    }
    if (lane < k) {
        p.out_ids[(size_t)r * k + lane] = oid;
        p.out_scores[(size_t)r * k + lane] = __uint_as_float(ow);
    }
}

// ---- the plan merge (m2d_plan_menus) ---------------------------------------------------------------------
// D days of the constrained merge in one wave per user, over lists of L = D k.  The walk takes a signature's dishes as a PREFIX of its
// own order (a cursor moves only on a take), so day d + 1 over the order less the dishes of days 1 .. d is the same walk with the
// cursors where day d left them and the day counters back at 0.  `full` = the categories at their day cap | those at their plan cap:
// the first come back the next morning, the second never.  Lane t keeps the day's t-th entry; a day's row is stored once, k lanes
// side by side, and every row of [days, k] is written (id -1 / the fill NaN where no step filled it).
// The window: the menu merge makes one dependent 8-byte load by one lane per step; over up to 1 024 steps with few waves in flight
// that latency is the kernel.  A lane therefore holds its next PM_WIN entries (key and score word) in registers, filled by PM_WIN
// independent pairs of loads in one go; a take shifts the window (static indices: registers), and only an empty window loads
// again.  Lists have row stride L, any alignment: the loads are dwords.  A list ends at an id below 0 or at L (key TKM_NONE: such
// a lane is never taken from, so it never shifts).  No LDS, no atomics but the error latch.
constexpr int PM_WIN = 8;

struct PlanMergeArgs {
    const float *list_scores;           // [S', Ub, L]
    const int32_t *list_ids;
    const int32_t *seg_off;             // [65]
    const int32_t *caps;                // [n, C]: the block's rows, per day
    const int32_t *plan_caps;           // [n, C]: the block's rows, over the plan; null: none
    int64_t n, Ub, index_base, nU;      // nU: the call's rows (a plan cap's position is nU C + u C + c)
    int32_t days, k, L, C;
    float *out_scores;                  // [n, days, k]: the block's rows
    int32_t *out_ids;
    int32_t *err;
};

__global__ __launch_bounds__(256) void m2d_plan_merge(const PlanMergeArgs p)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + wave;
    if (r >= p.n) return;                       // wave-uniform
    const int k = p.k, L = p.L;

    const bool have = p.seg_off[lane + 1] > p.seg_off[lane];
    const int j = __popcll(__ballot(have) & ((1ull << lane) - 1ull));

    int32_t capv = 0, planv = 0x7FFFFFFF;
    if (lane < p.C) {
        capv = p.caps[(size_t)r * p.C + lane];
        if (capv < 0) m2d_latch_error(p.err, M2D_ERR_INVALID_ARG, capv, (p.index_base + r) * p.C + lane);
        if (p.plan_caps) {
            planv = p.plan_caps[(size_t)r * p.C + lane];
            if (planv < 0) m2d_latch_error(p.err, M2D_ERR_INVALID_ARG, planv, (p.nU + p.index_base + r) * p.C + lane);
        }
    }
    int32_t cap[M2D_MENU_MAX_CATEGORIES], pcap[M2D_MENU_MAX_CATEGORIES], cnt[M2D_MENU_MAX_CATEGORIES], pcnt[M2D_MENU_MAX_CATEGORIES];
#pragma unroll
    for (int c = 0; c < M2D_MENU_MAX_CATEGORIES; ++c) {
        cap[c] = __builtin_amdgcn_readlane(capv, c);
        pcap[c] = __builtin_amdgcn_readlane(planv, c);      // no plan caps: INT32_MAX, which no count reaches
        pcnt[c] = 0;
    }

    const size_t lrow = ((size_t)j * p.Ub + r) * L;
    int next = 0, held = 0;                     // the list position behind the window; the window's entries not yet taken
    uint64_t wkey[PM_WIN];
    uint32_t wword[PM_WIN];
    const auto refill = [&]() {                 // PM_WIN entries from `next` on: the loads do not depend on one another
        int32_t id[PM_WIN];
        float sc[PM_WIN];
#pragma unroll
        for (int i = 0; i < PM_WIN; ++i) {
            const bool in = have && next + i < L;
            id[i] = in ? p.list_ids[lrow + next + i] : -1;
            sc[i] = in ? p.list_scores[lrow + next + i] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < PM_WIN; ++i) {
            wkey[i] = id[i] >= 0 ? tkm_key(sc[i], id[i]) : TKM_NONE;
            wword[i] = __float_as_uint(sc[i]);
        }
        next += PM_WIN;
        held = PM_WIN;
    };
    refill();

    bool done = false;                          // a day took nothing: so will every day after it (wave-uniform)
    for (int d = 0; d < p.days; ++d) {
        unsigned full = 0;
#pragma unroll
        for (int c = 0; c < M2D_MENU_MAX_CATEGORIES; ++c) {
            cnt[c] = 0;
            if (c < p.C && (cap[c] <= 0 || pcnt[c] >= pcap[c])) full |= 1u << c;
        }
        int32_t oid = -1;
        uint32_t ow = 0x7FC00000u;
        int t = 0;
        for (; t < k && !done; ++t) {           // wave-uniform: best, win and full are the same in every lane
            const uint64_t key = wkey[0];
            const bool adm = key != TKM_NONE && ((unsigned)lane & full) == 0u;
            uint64_t best = adm ? key : TKM_NONE;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const uint64_t o = __shfl_xor((unsigned long long)best, off, 64);
                best = o < best ? o : best;
            }
            if (best == TKM_NONE) break;
            const int win = __ffsll((unsigned long long)__ballot(adm && key == best)) - 1;
            const uint32_t bw = (uint32_t)__shfl((int)wword[0], win, 64);
            if (lane == t) {
                oid = (int32_t)(uint32_t)(best & 0xFFFFFFFFu);
                ow = bw;
            }
#pragma unroll
            for (int c = 0; c < M2D_MENU_MAX_CATEGORIES; ++c)
                if ((win >> c) & 1) {
                    cnt[c] += 1;
                    pcnt[c] += 1;
                    if (cnt[c] >= cap[c] || pcnt[c] >= pcap[c]) full |= 1u << c;
                }
            if (lane == win) {
#pragma unroll
                for (int i = 0; i + 1 < PM_WIN; ++i) {
                    wkey[i] = wkey[i + 1];
                    wword[i] = wword[i + 1];
                }
                wkey[PM_WIN - 1] = TKM_NONE;
                if (--held == 0) refill();
            }
        }
        if (t == 0) done = true;
        if (lane < k) {
            const size_t at = ((size_t)r * p.days + d) * k + lane;
            p.out_ids[at] = oid;
            p.out_scores[at] = __uint_as_float(ow);
        }
    }
}

// the signature index of the resident masks, built when they changed: perm | seg_off behind it, and seg_off's host copy
int menu_ensure_index(m2d_engine *h, hipStream_t st)
{
    if (h->menu_valid) return M2D_OK;
    const int64_t I = h->I, nb = (I + MN_DB - 1) / MN_DB;
    const size_t o_counts = ((size_t)I + 3) / 4, o_base = o_counts + (size_t)nb * MN_SIGS;      // in words: sig u8[I] | counts | bases
    int rc;
    if ((rc = h->menu_perm.grow(h, (size_t)I + MN_SIGS + 1)) != M2D_OK) return rc;
    if ((rc = h->menu_work.grow(h, o_base + (size_t)nb * MN_SIGS)) != M2D_OK) return rc;
    if (!h->menu_seg_host && (rc = h->menu_seg_host.alloc(h, MN_SIGS + 1)) != M2D_OK) return rc;
    uint8_t *sig = reinterpret_cast<uint8_t *>(h->menu_work.get());
    int32_t *counts = h->menu_work + o_counts, *base = h->menu_work + o_base, *seg_off = h->menu_perm + I;

    hipLaunchKernelGGL(m2d_menu_flag, dim3((unsigned)nb), dim3(MN_DB), 0, st, h->dish_cats, I, h->C, sig, counts);
    hipLaunchKernelGGL(m2d_menu_scan, dim3(1), dim3(64 * MN_SCAN_WAVES), 0, st, counts, nb, base, seg_off);
    hipLaunchKernelGGL(m2d_menu_write, dim3((unsigned)nb), dim3(MN_DB), 0, st, sig, base, I, nullptr, h->menu_perm);
    M2D_HIP_TRY(h, hipGetLastError());
    // the build's one synchronisation: the 64 segment sizes decide the launches of every call that follows
    M2D_HIP_TRY(h, hipMemcpyAsync(h->menu_seg_host, seg_off, (MN_SIGS + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    M2D_HIP_TRY(h, hipStreamSynchronize(st));
    bool ok = h->menu_seg_host[0] == 0 && (int64_t)h->menu_seg_host[MN_SIGS] == I;
    for (int s = 0; s < MN_SIGS; ++s) {
        h->menu_seg[s] = h->menu_seg_host[s];
        ok = ok && h->menu_seg_host[s] <= h->menu_seg_host[s + 1];
    }
    h->menu_seg[MN_SIGS] = h->menu_seg_host[MN_SIGS];
    if (!ok) {
        h->last_error = "m2d_topk_menu: the signature index does not cover the catalogue";
        return M2D_ERR_HIP;
    }
    h->menu_valid = true;
    return M2D_OK;
}

// What a call walks: the dish ids by (signature, id), the 65 offsets on the device (the merge reads them) and on the host (they
// decide the launches).  The catalogue's index, or a slate's own.
struct MenuIndex {
    const int32_t *perm;
    const int32_t *seg_off;             // device [65]
    const int32_t *seg;                 // host [65]
};

// The signature index of a strictly ascending slate i32[nD]: slate_perm[nD], the slate's ids by (signature, id), | seg_off[65] -- the
// catalogue index's three passes, the flag pass reading the resident signature bytes (menu_ensure_index has run) and checking the
// caller's slate, the write pass storing slate[i].  The 64 segment sizes decide the launches: they are read to the host HERE, ONE
// STREAM SYNCHRONISATION PER CALL WITH A SLATE.
int menu_slate_index(m2d_engine *h, const int32_t *slate, const int64_t nD, int32_t (&seg)[MN_SIGS + 1], hipStream_t st)
{
    const int64_t nb = (nD + MN_DB - 1) / MN_DB;
    const size_t o_counts = ((size_t)nD + 3) / 4, o_base = o_counts + (size_t)nb * MN_SIGS;     // in words: ssig u8[nD] | counts | bases
    int rc;
    if ((rc = h->menu_slate_perm.grow(h, (size_t)nD + MN_SIGS + 1)) != M2D_OK) return rc;
    if ((rc = h->menu_slate_work.grow(h, o_base + (size_t)nb * MN_SIGS)) != M2D_OK) return rc;
    const uint8_t *sig = reinterpret_cast<const uint8_t *>(h->menu_work.get());
    uint8_t *ssig = reinterpret_cast<uint8_t *>(h->menu_slate_work.get());
    int32_t *counts = h->menu_slate_work + o_counts, *base = h->menu_slate_work + o_base, *seg_off = h->menu_slate_perm + nD;

    hipLaunchKernelGGL(m2d_menu_flag_slate, dim3((unsigned)nb), dim3(MN_DB), 0, st, slate, nD, h->I, sig, ssig, counts, h->err_dev);
    hipLaunchKernelGGL(m2d_menu_scan, dim3(1), dim3(64 * MN_SCAN_WAVES), 0, st, counts, nb, base, seg_off);
    hipLaunchKernelGGL(m2d_menu_write, dim3((unsigned)nb), dim3(MN_DB), 0, st, ssig, base, nD, slate, h->menu_slate_perm);
    M2D_HIP_TRY(h, hipGetLastError());
    M2D_HIP_TRY(h, hipMemcpyAsync(h->menu_seg_host, seg_off, (MN_SIGS + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    M2D_HIP_TRY(h, hipStreamSynchronize(st));
    bool ok = h->menu_seg_host[0] == 0 && (int64_t)h->menu_seg_host[MN_SIGS] == nD;
    for (int s = 0; s <= MN_SIGS; ++s) {
        seg[s] = h->menu_seg_host[s];
        ok = ok && (s == MN_SIGS || h->menu_seg_host[s] <= h->menu_seg_host[s + 1]);
    }
    if (!ok) {
        h->last_error = "m2d_topk_menu_filtered: the signature index does not cover the slate";
        return M2D_ERR_HIP;
    }
    return M2D_OK;
}

// The rows of a walk that are groups (null: users): M member slots per row, `users` is then the dense member array i32[nU M] and cnt
// i32[nU] the rows' member counts (m2d_launch_group_prepare).  members: the caller's matrix, for menu_call.
struct MenuGroups {
    const int32_t *members;
    const int32_t *cnt;
    int32_t M, mode;
    bool caps_per_member;
};

// One loop for both forms: per block of Ub users and non-empty segment of `ix`, ranges of W dishes -- vectors, scores, selection into
// the segment's lists (excl_off: each row's exclusion segment is struck on the range's ascending ids; a later range merges into the
// list of the ranges before it, whose entries were struck when they were listed) -- then the merge under the caps.
// m2d_plan_menus: the lists are L = days k long (above 64 the selection is the radix form whatever the option says) and the merge is
// m2d_plan_merge into [nU, days, k]; with days == 1 and no plan caps L = k and every launch is the menu call's.
// m2d_plan_groups (grp): a row is a group -- its M member rows are scored (fillers too: 4.12's known cost), reduced into the first of
// them and listed from there; blocks hold whole groups, score scratch [Ub M, W].  With grp == null M is 1 and nothing here differs from
// the per-user launches.  The order stays blocks outside, ranges inside (m2d_launch_groups has it the other way round): a block's lists
// live in list scratch [S', Ub, L] until its merge, so ranges outside would need the lists of ALL rows at once, [S', nU, L], which no
// option bounds.  The price: a range's dish vectors are rebuilt per block (m2d_slate_prepare, W K floats against the block's Ub M W K
// products).
int menu_walk(m2d_engine *h, const MenuIndex &ix, const int32_t *users, int64_t nU, int32_t days, int32_t k, const int32_t *caps,
              const int32_t *plan_caps, const int64_t *excl_off, const int32_t *excl_ids, float *out_scores, int32_t *out_ids, hipStream_t st,
              const MenuGroups *grp = nullptr)
{
    int rc;
    const int32_t L = days * k;
    const int64_t M = grp ? grp->M : 1;
    const bool plan = days != 1 || plan_caps;
    const int64_t P = h->opt_deep_chunk_pairs;
    const auto range_of = [&](const int64_t n_s) {
        const int64_t W0 = n_s < P ? n_s : P;
        return W0 < 65536 ? W0 : 65536;
    };
    int64_t S = 0, Wmax = 1;
    for (int s = 0; s < MN_SIGS; ++s) {
        const int64_t n_s = ix.seg[s + 1] - ix.seg[s];
        if (n_s <= 0) continue;
        ++S;
        if (range_of(n_s) > Wmax) Wmax = range_of(n_s);
    }
    // user blocks: score scratch [Ub M, W] and list scratch [S', Ub, L] both within P words (a block holds one row at least)
    const int64_t Ub = m2d_block_rows(P, M * Wmax > S * L ? M * Wmax : S * L, nU);
    if ((rc = h->slate_scores.grow(h, (size_t)Ub * M * Wmax)) != M2D_OK) return rc;
    if ((rc = h->menu_list_scores.grow(h, (size_t)S * Ub * L)) != M2D_OK) return rc;
    if ((rc = h->menu_list_ids.grow(h, (size_t)S * Ub * L)) != M2D_OK) return rc;
    const bool deep = L > 64 || h->opt_menu_select != 0;

    for (int64_t u0 = 0; u0 < nU; u0 += Ub) {
        const int64_t n = nU - u0 < Ub ? nU - u0 : Ub;
        int64_t j = 0;
        for (int s = 0; s < MN_SIGS; ++s) {
            const int64_t n_s = ix.seg[s + 1] - ix.seg[s];
            if (n_s <= 0) continue;
            const int64_t W = range_of(n_s);
            for (int64_t r0 = 0; r0 < n_s; r0 += W) {
                const int64_t Wc = n_s - r0 > W ? W : n_s - r0;
                const int32_t *ids = ix.perm + ix.seg[s] + r0;                   // ascending: a slate
                SlateArgs a;
                bool mfma;
                if ((rc = m2d_slate_prepare(h, ids, 0, Wc, a, mfma, st)) != M2D_OK) return rc;
                a.users = users + u0 * M; a.nU = n * M; a.index_base = u0 * M; a.out = h->slate_scores;
                if ((rc = m2d_launch_slate_scores(h, a, mfma, st)) != M2D_OK) return rc;
                if (grp && (rc = m2d_launch_group_reduce(h, grp->mode, h->slate_scores, grp->cnt + u0, n, (int)M, Wc, h->slate_scores,
                                                         M * Wc, st)) != M2D_OK)
                    return rc;
                SelectJob job = SelectJob::row_major(h->slate_scores, n, Wc, ids, 0);
                job.rs = M * Wc;                                                 // a group's list is read from its row 0
                job.first = r0 == 0 ? 1 : 0;
                job.k = L;
                job.out_scores = h->menu_list_scores + (size_t)j * Ub * L;
                job.out_ids = h->menu_list_ids + (size_t)j * Ub * L;
                if (excl_off) {
                    job.xoff = excl_off + u0; job.xids = excl_ids; job.xend = excl_off + nU;
                }
                if ((rc = m2d_launch_select(h, job, deep, st)) != M2D_OK) return rc;
            }
            ++j;
        }
        if (plan) {
            PlanMergeArgs m;
            m.list_scores = h->menu_list_scores; m.list_ids = h->menu_list_ids; m.seg_off = ix.seg_off;
            m.caps = caps + (size_t)u0 * h->C; m.plan_caps = plan_caps ? plan_caps + (size_t)u0 * h->C : nullptr;
            m.n = n; m.Ub = Ub; m.index_base = u0; m.nU = nU; m.days = days; m.k = k; m.L = L; m.C = h->C;
            m.out_scores = out_scores + (size_t)u0 * L; m.out_ids = out_ids + (size_t)u0 * L; m.err = h->err_dev;
            hipLaunchKernelGGL(m2d_plan_merge, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, m);
        } else {
            MenuMergeArgs m;
            m.list_scores = h->menu_list_scores; m.list_ids = h->menu_list_ids; m.seg_off = ix.seg_off;
            m.caps = caps + (size_t)u0 * h->C; m.n = n; m.Ub = Ub; m.index_base = u0; m.k = k; m.C = h->C;
            m.out_scores = out_scores + (size_t)u0 * k; m.out_ids = out_ids + (size_t)u0 * k; m.err = h->err_dev;
            hipLaunchKernelGGL(m2d_menu_merge, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, m);
        }
        M2D_HIP_TRY(h, hipGetLastError());
    }
    h->last_kernel = plan ? "m2d_plan_merge" : "m2d_menu_merge";
    return M2D_OK;
}

// what every entry does in front of the loop: the table conditions, the catalogue's index, the callers' lists, the slate's index
int menu_call(m2d_engine *h, const char *entry, const int32_t *users, int64_t nU, int32_t days, int32_t k, const int32_t *caps,
              const int32_t *plan_caps, const int64_t *excl_off, const int32_t *excl_ids, const int32_t *slate, int64_t nD, float *out_scores,
              int32_t *out_ids, hipStream_t st, const MenuGroups *groups = nullptr)
{
    int rc;
    if ((rc = m2d_deep_conditions(h, entry, st)) != M2D_OK) return rc;
    // groups: `users` is null and nU counts groups.  The member check is the call's first launch, the cap fold its second: their
    // latches come before every other, and from here on users / caps / plan_caps are the dense members and one cap row per group
    MenuGroups g;
    if (groups) {
        g = *groups;
        if ((rc = m2d_launch_group_prepare(h, g.members, nU, g.M, g.caps_per_member ? caps : nullptr, g.caps_per_member ? plan_caps : nullptr,
                                           &users, &g.cnt, &caps, &plan_caps, st)) != M2D_OK)
            return rc;
    }
    if ((rc = menu_ensure_index(h, st)) != M2D_OK) return rc;
    // the callers' lists are checked before any scoring launch in stream order: the positions the latch reports are the caller's
    if (excl_off && (rc = m2d_launch_check_exclusions(h, excl_off, excl_ids, nU, st)) != M2D_OK) return rc;
    MenuIndex ix{h->menu_perm, h->menu_perm + h->I, h->menu_seg};
    int32_t seg[MN_SIGS + 1];
    if (slate) {
        if ((rc = menu_slate_index(h, slate, nD, seg, st)) != M2D_OK) return rc;
        ix = MenuIndex{h->menu_slate_perm, h->menu_slate_perm + nD, seg};
    }
    return menu_walk(h, ix, users, nU, days, k, caps, plan_caps, excl_off, excl_ids, out_scores, out_ids, st, groups ? &g : nullptr);
}

}  // namespace

int m2d_launch_topk_menu_filtered(m2d_engine *h, const char *entry, const int32_t *users, int64_t nU, int32_t k, const int32_t *caps,
                                  const int64_t *excl_off, const int32_t *excl_ids, const int32_t *slate, int64_t nD, float *out_scores,
                                  int32_t *out_ids, hipStream_t st)
{
    return menu_call(h, entry, users, nU, 1, k, caps, nullptr, excl_off, excl_ids, slate, nD, out_scores, out_ids, st);
}

int m2d_launch_plan_menus(m2d_engine *h, const int32_t *users, int64_t nU, int32_t days, int32_t k, const int32_t *caps,
                          const int32_t *plan_caps, const int64_t *excl_off, const int32_t *excl_ids, const int32_t *slate, int64_t nD,
                          float *out_scores, int32_t *out_ids, hipStream_t st)
{
    return menu_call(h, "m2d_plan_menus", users, nU, days, k, caps, plan_caps, excl_off, excl_ids, slate, nD, out_scores, out_ids, st);
}

int m2d_launch_plan_groups(m2d_engine *h, const int32_t *members, int64_t nG, int32_t M, int32_t mode, int32_t days, int32_t k,
                           const int32_t *caps, const int32_t *plan_caps, bool caps_per_member, const int64_t *excl_off,
                           const int32_t *excl_ids, const int32_t *slate, int64_t nD, float *out_scores, int32_t *out_ids, hipStream_t st)
{
    const MenuGroups g{members, nullptr, M, mode, caps_per_member};
    return menu_call(h, "m2d_plan_groups", nullptr, nG, days, k, caps, plan_caps, excl_off, excl_ids, slate, nD, out_scores, out_ids, st, &g);
}

int m2d_launch_topk_menu(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int32_t *caps, float *out_scores,
                         int32_t *out_ids, hipStream_t st)
{
    return m2d_launch_topk_menu_filtered(h, "m2d_topk_menu", users, nU, k, caps, nullptr, nullptr, nullptr, 0, out_scores, out_ids, st);
}

