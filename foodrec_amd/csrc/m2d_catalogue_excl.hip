// m2d_topk_users_excluding: the k best dishes of the catalogue for each user, leaving out an ascending list of dish ids per user
// (the dishes the user has had).  Order and arithmetic are m2d_catalogue_rank's (m2d_catalogue.h: rank_exact_score16 and its
// one-lane form), so for the same excluded set the j-th listed dish has rank j, as integers.
//
// Tier 1 (default options, E = 32 / 64 / 128, k <= K1 = 16 / 16 / 10: where m2d_topk_users' lists are index-exact)
//   m2d_launch_topk_users   the unfiltered top K1 into engine scratch, kernels as they are
//   m2d_topk_excl_filter    16 lanes per user: listed ids found in the user's segment are dropped, the survivors compacted in order,
//                           the first k re-scored in the ranking arithmetic and written.  The unfiltered top K1 holds every dish that
//                           can precede its own last entry, so k survivors ARE the filtered top k; a user with fewer is `short` and
//                           appended to a device list (one atomic counter).
// Tier 2 (the short users; every user when tier 1 does not apply or "topk_excl_tier" = 2)
//   m2d_topk_excl_plan      16 lanes per short user: the bound sums, the 15 pattern bounds, the seed -- the largest lower bound over
//                           patterns that hold at least k + |X| rows (k of them are not excluded and score at least that) -- and
//                           the patterns whose upper bound reaches it; records past the short users carry an empty mask
//   m2d_plan_sort_launch    the records sorted by pattern mask (the retrieval plan's own sort)
//   m2d_topk_excl_scan      E <= 128: a wave per 64 sorted records and share of the tiles of their patterns, best upper bound first,
//                           on m2d_rank_count's walk (walk_tiles, m2d_catalogue.h); a lane's k-entry list in registers.  A tile is skipped when
//                           its bound is strictly below every lane's k-th score (the seed while a list is not full); a row that
//                           precedes a lane's k-th entry -- (score, id) compared explicitly: rows inside a pattern are stored by
//                           norm bucket, not by id -- is looked up in the lane's segment and inserted if absent
//   m2d_topk_excl_scan16    E > 128: 16 lanes per (record, share), the list held by all 16; of the walk, the shares and the clipping
//   m2d_topk_excl_merge     the shares' partial lists merged with the same comparison; a list still not full takes the empty-mask
//                           dishes (NaN scores, ranked last) that are not excluded in id order, then id -1 / NaN
//   m2d_check_exclusions    the offsets and ids themselves: out-of-range ids, segments not ascending, offsets not non-decreasing --
//                           the one whole-list check, also of the calls under the MLP head (m2d_launch_check_exclusions)
#include "m2d_catalogue.h"
#include "m2d_exclusions.h"

#pragma clang fp contract(off)

namespace {

constexpr int EXCL_KR = 16;                                  // list slots per lane (k <= 16)
constexpr int EXCL_XS = 60;                                  // excluded ids per user the one-lane scan keeps in LDS (longer segments: searched in HBM)
constexpr int32_t EXCL_NONE = 0x7fffffff;                    // id of an empty slot: (NaN, EXCL_NONE) is preceded by every dish

struct ExclArgs {
    RankTables t;
    const int32_t *users;
    const int64_t *excl_off;
    const int32_t *excl_ids;
    int64_t nU;
    int32_t k, K1, all_short;
    int64_t want;                    // waves (E <= 128) / 16-lane groups (E > 128) the scan should at least fill the device with
    const int32_t *list_i;           // [nU, K1] the unfiltered lists (tier 1)
    int32_t *short_list;             // [0] short users, [4 + s] their positions in the call
    float *plan, *bnd;               // the records (m2d_catalogue.h, RankRecord): the seed, the relevant patterns, the user's position in the call
    const int32_t *order;            // sorted position -> record: the records with users are the last `live` ones (an empty mask sorts first)
    float *part_s;                   // [shares, live users, k] partial lists (excl_shape)
    int32_t *part_i;
    float *out_scores;
    int32_t *out_ids;
    unsigned long long *counters;    // [0] tiles multiplied, [1] records with users (`live`)
};

// The scan's shape, worked out on the device from the number of records with users -- the host never learns how many users are
// short: `nsplit` shares of the tiles per wave of 64 users (E <= 128) / per user (E > 128), enough to fill the device when the
// users are few.  At most want + units items in all, which is what the launch and the partial lists are sized for.
__device__ __forceinline__ int excl_shape(const ExclArgs &p, const int64_t live, int64_t &units)
{
    units = p.t.E <= 128 ? (live + 63) >> 6 : live;
    return units <= 0 ? 0 : share_count(p.want, units);
}

// user i's segment of excl_ids, kept inside [0, excl_off[nU]] whatever the offsets hold (m2d_check_exclusions reports them); no
// lists, or a negative total: an empty window
__device__ __forceinline__ void excl_segment(const ExclArgs &p, const int64_t i, int64_t &x0, int64_t &x1)
{
    x0 = x1 = 0;
    if (!p.excl_off) return;
    const int64_t nnz = p.excl_off[p.nU];
    bool bad;
    csr_segment(p.excl_off, i, nnz < 0 ? 0 : nnz, x0, x1, bad);
}

// (x, id) into a list sorted by rank_before, in place from the last slot up (slot i - 1 still holds its old entry when slot i is
// written); the caller has established that it precedes the last entry
__device__ __forceinline__ void excl_insert(float (&ls)[EXCL_KR], int32_t (&li)[EXCL_KR], const float x, const int32_t id)
{
#pragma unroll
    for (int i = EXCL_KR - 1; i >= 0; --i) {
        const bool here = rank_before(x, id, ls[i], li[i]);
        const bool above = i > 0 ? rank_before(x, id, ls[i > 0 ? i - 1 : 0], li[i > 0 ? i - 1 : 0]) : false;
        ls[i] = above ? ls[i > 0 ? i - 1 : 0] : (here ? x : ls[i]);
        li[i] = above ? li[i > 0 ? i - 1 : 0] : (here ? id : li[i]);
    }
}

// a list of k entries in EXCL_KR slots: the first EXCL_KR - k hold (+inf, -1), which precedes every dish and is never moved, so
// that the k-th entry is always the last slot
__device__ __forceinline__ void excl_list_init(float (&ls)[EXCL_KR], int32_t (&li)[EXCL_KR], const int k)
{
#pragma unroll
    for (int i = 0; i < EXCL_KR; ++i) {
        ls[i] = i < EXCL_KR - k ? INFINITY : __builtin_nanf("");
        li[i] = i < EXCL_KR - k ? -1 : EXCL_NONE;
    }
}

__device__ __forceinline__ void excl_list_store(const float (&ls)[EXCL_KR], const int32_t (&li)[EXCL_KR], const int k, float *os, int32_t *oi)
{
#pragma unroll
    for (int i = 0; i < EXCL_KR; ++i) {
        if (i >= EXCL_KR - k) {
            os[i - (EXCL_KR - k)] = ls[i];
            oi[i - (EXCL_KR - k)] = li[i];
        }
    }
}

// ---- the lists themselves ------------------------------------------------------------------------------------------------------------
// The lists of a call, looked at once: offsets non-decreasing from 0 (so none reaches past the array, whose length is the last of
// them), every id a dish of the catalogue and not below the id in front of it in its segment -- m2d_catalogue_rank's checks and
// latch values (m2d_exclusions.h).  A grid-stride walk: with a single malformed entry the latch is the same whatever the grid (with
// several, the first thread to reach the latch wins, as in every kernel that writes it).
__global__ __launch_bounds__(256) void m2d_check_exclusions(const int64_t *off, const int32_t *ids, int64_t n, int64_t I, int32_t *err)
{
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
    for (int64_t q = t0; q <= n; q += nt) csr_check_offset(off, q, err);
    const int64_t nnz = off[n];
    int32_t x;
    int64_t row;
    for (int64_t i = t0; i < nnz; i += nt) csr_check_id(off, ids, n, I, i, true, err, x, row);      // (a thread per id)
}

// ---- tier 1: the unfiltered top K1 without the listed ids ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void m2d_topk_excl_filter(ExclArgs p)
{
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (u >= p.nU) return;                                  // (16-lane groups are whole)
    const RankTables &t = p.t;
    const int E4 = t.E >> 2, k = p.k;
    const int32_t uid = p.users[u];
    const int64_t ul = (int64_t)uid - t.user_base;
    if (ul < 0 || ul >= t.U) {
        if (j == 0) m2d_latch_error(t.err, M2D_ERR_BAD_USER_ID, uid, u);
        return;                                             // (the rows of a call with a latched error are unspecified)
    }
    int64_t x0, x1;
    excl_segment(p, u, x0, x1);
    int32_t id = j < p.K1 ? p.list_i[(size_t)u * p.K1 + j] : -1;
    if ((int64_t)id >= t.I) id = -1;
    const bool keep = id >= 0 && !sorted_contains(p.excl_ids, x0, x1, id);
    const uint32_t bal = (uint32_t)((__ballot(keep) >> (lane & 48)) & 0xffffull);
    if (__builtin_popcount(bal) < k) {
        if (j == 0) p.short_list[4 + atomicAdd(&p.short_list[0], 1)] = (int32_t)u;
        return;
    }
    const v4f *pmu = user_block(t, uid);
    float hc[4], ha[4], G[10];
    rank_user_sums16(pmu, t.ce, E4, j, hc, ha, G);
    uint32_t m = bal;
    for (int o = 0; o < k; ++o, m &= m - 1) {               // the o-th survivor sits in the lane of m's lowest bit
        const int32_t d = __shfl(id, (lane & 48) + (__ffs(m) - 1), 64);
        const float s = rank_exact_score16(pmu, t.re, E4, j, d, dish_pattern(t.cats, d), t.a, t.b, hc);
        if (j == 0) {
            p.out_scores[(size_t)u * k + o] = s;
            p.out_ids[(size_t)u * k + o] = d;
        }
    }
}

// ---- tier 2: per short user the bounds, the seed, the relevant patterns --------------------------------------------------------------
__global__ __launch_bounds__(256) void m2d_topk_excl_plan(ExclArgs p)
{
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (s >= p.nU) return;                                  // (16-lane groups are whole)
    const RankTables &t = p.t;
    const int64_t nshort = p.all_short ? p.nU : (int64_t)p.short_list[0];
    int64_t u = -1;
    if (s < nshort) u = p.all_short ? s : (int64_t)p.short_list[4 + s];
    int32_t uid = 0;
    if (u >= 0) {
        uid = p.users[u];
        const int64_t ul = (int64_t)uid - t.user_base;
        if (ul < 0 || ul >= t.U) {
            if (j == 0) m2d_latch_error(t.err, M2D_ERR_BAD_USER_ID, uid, u);
            u = -1;
        }
    }
    if (u < 0) {                                            // no user in this record: an empty mask, nothing scanned or written
        record_store_none(p.plan, s, j);
        return;
    }
    const v4f *pmu = user_block(t, uid);
    float hc[4], ha[4], G[10];
    rank_user_sums16(pmu, t.ce, t.E >> 2, j, hc, ha, G);
    int64_t x0, x1;
    excl_segment(p, u, x0, x1);
    const int64_t rows_needed = (int64_t)p.k + (x1 - x0);   // (repeated ids only make it larger: still a bound)
    float seed, lo, hi;
    grouped_pattern_bounds_lanes(hc, ha, G, t.grp, (int)(rows_needed > 0x7fffffff ? 0x7fffffff : rows_needed), t.a, t.b, t.E, j, seed, lo, hi);
    const uint32_t mask = grouped_mask_lanes(hi, seed, j);
    if (j == 0) atomicAdd(&p.counters[1], 1ull);
    record_store(p.plan, p.bnd, s, j, seed, hc, mask, (int32_t)u, 0, ha, G);
}

// ---- tier 2, E <= 128: one lane per user -----------------------------------------------------------------------------------------------
template <int E4MAX>
__global__ __launch_bounds__(256) void m2d_topk_excl_scan(ExclArgs p)
{
    const RankTables &t = p.t;
    const int lane = threadIdx.x & 63;
    const int64_t g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nlive = (int64_t)p.counters[1];
    int64_t nqw;
    const int nsplit = excl_shape(p, nlive, nqw);
    if (g >= nqw * nsplit) return;
    const int64_t qw = g % nqw;
    const int split = (int)(g / nqw);
    const int k = p.k;
    const bool valid = qw * 64 + lane < nlive;
    const int64_t si = valid ? (int64_t)p.order[p.nU - nlive + qw * 64 + lane] : 0;
    const RankRecord rec = record_load(p.plan, p.bnd, si);
    const float seed = rec.s;
    const int32_t u = valid ? rec.id : -1;
    const bool live = u >= 0;
    const uint32_t mask = live ? rec.mask : 0u;
    uint32_t um = mask;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) um |= __shfl_xor(um, off, 64);
    um = __builtin_amdgcn_readfirstlane(um);
    if (um == 0u) return;                                   // a wave of records without users
    // (a bad id: latched by m2d_topk_excl_plan, which leaves such a record without a user)
    const v4f *pmu = user_block(t, live ? (int64_t)p.users[u] : t.user_base);
    int64_t x0 = 0, x1 = 0;
    if (live) excl_segment(p, u, x0, x1);
    // the lane's segment in its own LDS column: a candidate's lookup is then a few LDS reads instead of a chain of dependent loads
    // from HBM (with a list that is still filling, some lane of the wave has a candidate in every third row)
    __shared__ int32_t xs[4][EXCL_XS][64];
    const int wv = threadIdx.x >> 6;
    const int xn = x1 - x0 <= EXCL_XS ? (int)(x1 - x0) : -1;
    for (int i = 0; i < xn; ++i) xs[wv][i][lane] = p.excl_ids[x0 + i];
    // the wave's patterns, best upper bound first: the lists fill early and the thresholds rise early
    float key[GRP_MAXPAT];
#pragma unroll
    for (int q = 1; q < GRP_MAXPAT; ++q) {
        float lo, hi;
        pattern_bound(pattern_bound_terms(rec.hc, rec.ha, rec.G, q, t.a, t.b, t.E), __int_as_float(t.grp[GRP_RMAX + q]), lo, hi);
        float v = ((mask >> q) & 1u) ? fmaxf(hi, -INFINITY) : -INFINITY;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
        key[q] = v;
    }
    int64_t t0, t1;
    share_of(pattern_set_tiles(t.grp, um), nsplit, split, t0, t1);
    float ls[EXCL_KR];
    int32_t li[EXCL_KR];
    excl_list_init(ls, li, k);
    const unsigned long long multiplied = walk_tiles<E4MAX>(
        t, pmu, rec, um, t0, t1,
        [&](const uint32_t avail) {
            int best = -1;
            float bk = 0.f;
#pragma unroll
            for (int q = 1; q < GRP_MAXPAT; ++q) {
                if (((avail >> q) & 1u) && (best < 0 || key[q] > bk)) {
                    best = q;
                    bk = key[q];
                }
            }
            return __builtin_amdgcn_readfirstlane(best);    // (the keys are wave-uniform)
        },
        [&](const int, const float, const float bhi, const int) {
            // the lane's k-th score, the seed while its list is not full; strict: a row equal to either must reach the insertion
            const float thr = li[EXCL_KR - 1] != EXCL_NONE ? ls[EXCL_KR - 1] : seed;
            return live && !(bhi < thr);
        },
        [&](const float sc, const int32_t id, const bool) {
            const bool cand = live && !(sc < seed) && rank_before(sc, id, ls[EXCL_KR - 1], li[EXCL_KR - 1]);
            if (__ballot(cand) != 0ull) {                   // rare once the lists are full
                if (cand) {
                    const bool found = xn >= 0 ? sorted_contains(0, xn, id, [&](const int i) { return xs[wv][i][lane]; })
                                               : sorted_contains(p.excl_ids, x0, x1, id);
                    if (!found) excl_insert(ls, li, sc, id);
                }
            }
        });
    if (live) excl_list_store(ls, li, k, p.part_s + ((size_t)g * 64 + lane) * k, p.part_i + ((size_t)g * 64 + lane) * k);
    if (lane == 0 && multiplied) atomicAdd(&p.counters[0], multiplied);
}

// ---- tier 2, E > 128: 16 lanes per (record, share of its patterns' tiles), every lane holding the list ---------------------------------
__global__ __launch_bounds__(256) void m2d_topk_excl_scan16(ExclArgs p)
{
    const RankTables &t = p.t;
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int64_t nlive = (int64_t)p.counters[1];
    int64_t units;
    const int nsplit = excl_shape(p, nlive, units);
    if (g >= nlive * nsplit) return;                        // (whole 16-lane groups)
    const int64_t si = p.order[p.nU - nlive + g % nlive];
    const int split = (int)(g / nlive);
    const int E4 = t.E >> 2, k = p.k;
    const RankRecord rec = record_load(p.plan, p.bnd, si);
    const int32_t u = rec.id;
    if (u < 0) return;
    const float seed = rec.s;
    const v4f *pmu = user_block(t, p.users[u]);
    int64_t x0, x1;
    excl_segment(p, u, x0, x1);
    int64_t t0, t1;
    share_of(pattern_set_tiles(t.grp, rec.mask), nsplit, split, t0, t1);
    float ls[EXCL_KR];
    int32_t li[EXCL_KR];
    excl_list_init(ls, li, k);
    unsigned long long multiplied = 0ull;
    int64_t cum = 0;
    for (int q = 1; q < GRP_MAXPAT && cum < t1; ++q) {
        if (!((rec.mask >> q) & 1u)) continue;
        int64_t tile, tile1;
        if (!pattern_span(t.grp, q, t0, t1, cum, tile, tile1)) continue;
        const PatternBoundTerms rb = pattern_bound_terms(rec.hc, rec.ha, rec.G, q, t.a, t.b, t.E);
        for (; tile < tile1; ++tile) {
            const int nrows = t.tile_info[tile] >> 8;
            float blo, bhi;
            pattern_bound(rb, t.tnorm[tile], blo, bhi);
            const float thr = li[EXCL_KR - 1] != EXCL_NONE ? ls[EXCL_KR - 1] : seed;
            if (bhi < thr) continue;                        // (the same in all 16 lanes)
            multiplied += 1ull;
            for (int r = 0; r < nrows; ++r) {
                const int32_t id = t.perm[tile * 32 + r];
                const float sc = rank_exact_score16(pmu, t.re, E4, j, id, q, t.a, t.b, rec.hc);
                if (!(sc < seed) && rank_before(sc, id, ls[EXCL_KR - 1], li[EXCL_KR - 1]) && !sorted_contains(p.excl_ids, x0, x1, id))
                    excl_insert(ls, li, sc, id);
            }
        }
    }
    if (j == 0) {
        excl_list_store(ls, li, k, p.part_s + (size_t)g * k, p.part_i + (size_t)g * k);
        if (multiplied) atomicAdd(&p.counters[0], multiplied);
    }
}

// ---- tier 2: the shares' lists into the user's row ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void m2d_topk_excl_merge(ExclArgs p)
{
    __shared__ float ms[EXCL_KR][256];
    __shared__ int32_t mi[EXCL_KR][256];
    const int tx = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * 256 + tx;       // the t-th record with a user, in sorted order
    const int64_t nlive = (int64_t)p.counters[1];
    if (t >= nlive) return;
    int64_t units;
    const int nsplit = excl_shape(p, nlive, units);
    const int32_t u = record_id(p.plan, p.order[p.nU - nlive + t]);
    if (u < 0) return;
    const int k = p.k;
    int cnt = 0;
    for (int sp = 0; sp < nsplit; ++sp) {
        // where the scan kernels put share sp of this record: (wave, lane) of the one-lane form, the group of the 16-lane form
        const size_t slot = p.t.E <= 128 ? ((size_t)sp * units + (size_t)(t >> 6)) * 64 + (size_t)(t & 63) : (size_t)sp * nlive + (size_t)t;
        const float *ps = p.part_s + slot * k;
        const int32_t *pi = p.part_i + slot * k;
        for (int e = 0; e < k; ++e) {
            const int32_t id = pi[e];
            const float s = ps[e];
            if (id == EXCL_NONE) break;
            if (cnt == k && !rank_before(s, id, ms[k - 1][tx], mi[k - 1][tx])) break;     // (a share's list is sorted: nor can the rest)
            int i = cnt < k ? cnt : k - 1;
            for (; i > 0 && rank_before(s, id, ms[i - 1][tx], mi[i - 1][tx]); --i) {
                ms[i][tx] = ms[i - 1][tx];
                mi[i][tx] = mi[i - 1][tx];
            }
            ms[i][tx] = s;
            mi[i][tx] = id;
            cnt += cnt < k ? 1 : 0;
        }
    }
    if (cnt < k) {                                          // every dish with a mask that is not excluded is listed: the empty-mask ones follow
        int64_t x0, x1;
        excl_segment(p, u, x0, x1);
        for (int64_t d = 0; d < p.t.I && cnt < k; ++d) {
            if (dish_pattern(p.t.cats, d) == 0 && !sorted_contains(p.excl_ids, x0, x1, (int32_t)d)) {
                ms[cnt][tx] = __builtin_nanf("");
                mi[cnt][tx] = (int32_t)d;
                ++cnt;
            }
        }
    }
    for (int e = 0; e < k; ++e) {
        p.out_scores[(size_t)u * k + e] = e < cnt ? ms[e][tx] : __builtin_nanf("");
        p.out_ids[(size_t)u * k + e] = e < cnt ? mi[e][tx] : -1;
    }
}

}  // namespace

int m2d_launch_check_exclusions(m2d_engine *h, const int64_t *off, const int32_t *ids, int64_t n, hipStream_t st)
{
    hipLaunchKernelGGL(m2d_check_exclusions, dim3((unsigned)(h->num_cu * 4)), dim3(256), 0, st, off, ids, n, h->I, h->err_dev);
    M2D_HIP_TRY(h, hipGetLastError());
    return M2D_OK;
}

int m2d_launch_topk_users_excluding(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int64_t *excl_off,
                                    const int32_t *excl_ids, float *out_scores, int32_t *out_ids, hipStream_t st, const char *entry,
                                    bool under_head)
{
    int rc;
    if ((rc = m2d_rank_prepare(h, entry, st, under_head)) != M2D_OK) return rc;

    // tier 1 where m2d_topk_users' lists are index-exact against the ranking arithmetic (include/m2d.h), under the default options
    const int K1 = h->E == 128 ? 10 : 16;
    const bool tier1 = h->opt_topk_excl_tier != 2 && (h->E == 32 || h->E == 64 || h->E == 128) && k <= K1 && (int64_t)K1 <= h->I &&
                       h->grp_tiles > 0 && h->opt_topk_refine == 1 && h->opt_topk_grouped == 1 && h->opt_topk_form == 0 &&
                       h->opt_topk_prune == 1 && h->opt_topk_block == 0 && h->opt_variant == 0;
    // waves in flight, 8 per SIMD (E > 128: four 16-lane groups each).  The scan's items -- (wave of 64 users, share of its tiles), or
    // (user, share) -- are counted on the device (excl_shape): at most want + units of them, units <= those of nU users
    const int64_t want = (int64_t)h->num_cu * 32 * (h->E <= 128 ? 1 : 4);
    const int64_t items = want + (h->E <= 128 ? (nU + 63) / 64 : nU);

    // K1 lists: scores [nU, 16] | ids [nU, 16] | short list [4 + nU] | the records' scratch (rank_scratch) | partial lists: scores,
    // ids [items, k]
    const size_t n4 = ((size_t)nU + 3) & ~(size_t)3;
    const size_t part = (size_t)items * (h->E <= 128 ? 64 : 1) * k;
    const size_t need = (size_t)nU * 32 + (4 + n4) + rank_scratch(nullptr, nU).floats + 2 * part;
    if ((rc = h->excl_buf.grow(h, need, h->excl_counters, h->excl_short)) != M2D_OK) return rc;
    ExclArgs a;
    a.t = rank_tables(h);
    a.users = users; a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.nU = nU; a.k = k; a.want = want; a.K1 = K1;
    a.all_short = tier1 ? 0 : 1;
    float *list_s = h->excl_buf;
    int32_t *list_i = reinterpret_cast<int32_t *>(list_s + (size_t)nU * 16);
    a.list_i = list_i;
    a.short_list = list_i + (size_t)nU * 16;
    const RankScratch sc = rank_scratch(reinterpret_cast<float *>(a.short_list + 4 + n4), nU);
    a.plan = sc.plan; a.bnd = sc.bnd; a.order = sc.order; a.counters = sc.counters;
    a.part_s = sc.plan + sc.floats;
    a.part_i = reinterpret_cast<int32_t *>(a.part_s + part);
    a.out_scores = out_scores; a.out_ids = out_ids;
    h->excl_counters = a.counters;
    h->excl_short = a.short_list;
    h->excl_all_short = tier1 ? -1 : nU;
    M2D_HIP_TRY(h, hipMemsetAsync(a.counters, 0, 8 * sizeof(int32_t), st));
    M2D_HIP_TRY(h, hipMemsetAsync(a.short_list, 0, 4 * sizeof(int32_t), st));
    if (excl_off && (rc = m2d_launch_check_exclusions(h, excl_off, excl_ids, nU, st)) != M2D_OK) return rc;
    const dim3 g16((unsigned)((nU * 16 + 255) / 256));
    if (tier1) {
        if ((rc = m2d_launch_topk_users(h, users, nU, K1, list_s, list_i, st)) != M2D_OK) return rc;
        hipLaunchKernelGGL(m2d_topk_excl_filter, g16, dim3(256), 0, st, a);
        M2D_HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(m2d_topk_excl_plan, g16, dim3(256), 0, st, a);
    M2D_HIP_TRY(h, hipGetLastError());
    // records with users last (an empty mask is key 0), grouped by pattern mask so that the 64 users of a wave share patterns
    if ((rc = m2d_plan_sort_launch(h, a.plan, nU, sc.hist, sc.order, st)) != M2D_OK) return rc;
    const dim3 grid(h->E <= 128 ? (unsigned)((items + 3) / 4) : (unsigned)((items * 16 + 255) / 256));
    with_rank_width(h->E, [&](auto w) {
        constexpr int W = decltype(w)::value;
        if constexpr (W != 0) hipLaunchKernelGGL(m2d_topk_excl_scan<W>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(m2d_topk_excl_scan16, grid, dim3(256), 0, st, a);
    });
    M2D_HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(m2d_topk_excl_merge, dim3((unsigned)((nU + 255) / 256)), dim3(256), 0, st, a);
    M2D_HIP_TRY(h, hipGetLastError());
    h->last_kernel = "m2d_topk_excl_scan";
    return M2D_OK;
}
