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
//   m2d_topk_excl_scan      E <= 128: a wave per 64 sorted records and share of the tiles of their patterns, best upper bound first;
//                           one lane per user, its k-entry list in registers, the dish row wave-uniform.  A tile is skipped when
//                           its bound is strictly below every lane's k-th score (the seed while a list is not full); a row that
//                           precedes a lane's k-th entry -- (score, id) compared explicitly: rows inside a pattern are stored by
//                           norm bucket, not by id -- is looked up in the lane's segment and inserted if absent
//   m2d_topk_excl_scan16    E > 128: 16 lanes per (record, share), the list held by all 16
//   m2d_topk_excl_merge     the shares' partial lists merged with the same comparison; a list still not full takes the empty-mask
//                           dishes (NaN scores, ranked last) that are not excluded in id order, then id -1 / NaN
//   m2d_topk_excl_check     the offsets and ids themselves: out-of-range ids, segments not ascending, offsets not non-decreasing
#include "m2d_catalogue.h"

#pragma clang fp contract(off)

namespace {

constexpr int EXCL_KR = 16;                                  // list slots per lane (k <= 16)
constexpr int EXCL_XS = 60;                                  // excluded ids per user the one-lane scan keeps in LDS (longer segments: searched in HBM)
constexpr int32_t EXCL_NONE = 0x7fffffff;                    // id of an empty slot: (NaN, EXCL_NONE) is preceded by every dish

struct ExclArgs {
    const float *pm, *re, *ce, *cats;
    const float *rs, *tnorm;         // the pattern-sorted f32 dish table (row stride ew floats), per-tile largest row norm
    const int32_t *perm, *tile_info, *grp;
    const int32_t *users;
    const int64_t *excl_off;
    const int32_t *excl_ids;
    int64_t nU, U, I, user_base;
    int32_t E, ew, k, K1, all_short;
    int64_t want;                    // waves (E <= 128) / 16-lane groups (E > 128) the scan should at least fill the device with
    float a, b;
    const int32_t *list_i;           // [nU, K1] the unfiltered lists (tier 1)
    int32_t *short_list;             // [0] short users, [4 + s] their positions in the call
    float *plan;                     // [nU, 8]  seed, <U_high, CE_c> x 4, relevant-pattern mask, position in the call (-1: none), 0
    float *bnd;                      // [nU, 16] the bound sums (m2d_catalogue_rank's layout)
    const int32_t *order;            // sorted position -> record: the records with users are the last `live` ones (an empty mask sorts first)
    float *part_s;                   // [shares, live users, k] partial lists (excl_shape)
    int32_t *part_i;
    float *out_scores;
    int32_t *out_ids;
    int32_t *err;
    unsigned long long *counters;    // [0] tiles multiplied, [1] records with users (`live`)
};

// The scan's shape, worked out on the device from the number of records with users -- the host never learns how many users are
// short: `nsplit` shares of the tiles per wave of 64 users (E <= 128) / per user (E > 128), enough to fill the device when the
// users are few.  At most want + units items in all, which is what the launch and the partial lists are sized for.
__device__ __forceinline__ int excl_shape(const ExclArgs &p, const int64_t live, int64_t &units)
{
    units = p.E <= 128 ? (live + 63) >> 6 : live;
    if (units <= 0) return 0;
    const int64_t ns = (p.want + units - 1) / units;
    return (int)(ns < 1 ? 1 : (ns > 512 ? 512 : ns));
}

// (s, d) before (t, p) in the ranking: score descending, NaN last, equal scores (NaN included) to the lower id
__device__ __forceinline__ bool excl_before(const float s, const int32_t d, const float t, const int32_t p)
{
    if (t != t) return s == s || d < p;
    return s > t || (s == t && d < p);
}

// user i's segment of excl_ids, kept inside [0, excl_off[nU]] whatever the offsets hold (m2d_topk_excl_check reports them)
__device__ __forceinline__ void excl_segment(const ExclArgs &p, const int64_t i, int64_t &x0, int64_t &x1)
{
    x0 = x1 = 0;
    if (!p.excl_off) return;
    int64_t nnz = p.excl_off[p.nU];
    nnz = nnz < 0 ? 0 : nnz;
    const int64_t a = p.excl_off[i], b = p.excl_off[i + 1];
    x0 = a < 0 ? 0 : (a > nnz ? nnz : a);
    x1 = b < x0 ? x0 : (b > nnz ? nnz : b);
}

__device__ __forceinline__ bool excl_contains(const int32_t *ids, int64_t lo, int64_t hi, const int32_t d)
{
    const int64_t end = hi;
    while (lo < hi) {                                       // first position with ids[pos] >= d
        const int64_t mid = (lo + hi) >> 1;
        if (ids[mid] < d) lo = mid + 1; else hi = mid;
    }
    return lo < end && ids[lo] == d;
}

// (x, id) into a list sorted by excl_before, in place from the last slot up (slot i - 1 still holds its old entry when slot i is
// written); the caller has established that it precedes the last entry
__device__ __forceinline__ void excl_insert(float (&ls)[EXCL_KR], int32_t (&li)[EXCL_KR], const float x, const int32_t id)
{
#pragma unroll
    for (int i = EXCL_KR - 1; i >= 0; --i) {
        const bool here = excl_before(x, id, ls[i], li[i]);
        const bool above = i > 0 ? excl_before(x, id, ls[i > 0 ? i - 1 : 0], li[i > 0 ? i - 1 : 0]) : false;
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
__global__ __launch_bounds__(256) void m2d_topk_excl_check(ExclArgs p)
{
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
    for (int64_t q = t0; q <= p.nU; q += nt) csr_check_offset(p.excl_off, q, p.err);
    const int64_t nnz = p.excl_off[p.nU];
    int32_t x;
    int64_t user;
    for (int64_t i = t0; i < nnz; i += nt) csr_check_id(p.excl_off, p.excl_ids, p.nU, p.I, i, true, p.err, x, user);      // (a thread per id)
}

// ---- tier 1: the unfiltered top K1 without the listed ids ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void m2d_topk_excl_filter(ExclArgs p)
{
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (u >= p.nU) return;                                  // (16-lane groups are whole)
    const int E4 = p.E >> 2, k = p.k;
    const int32_t uid = p.users[u];
    int64_t ul = (int64_t)uid - p.user_base;
    if (ul < 0 || ul >= p.U) {
        if (j == 0) m2d_latch_error(p.err, M2D_ERR_BAD_USER_ID, uid, u);
        return;                                             // (the rows of a call with a latched error are unspecified)
    }
    int64_t x0, x1;
    excl_segment(p, u, x0, x1);
    int32_t id = j < p.K1 ? p.list_i[(size_t)u * p.K1 + j] : -1;
    if ((int64_t)id >= p.I) id = -1;
    const bool keep = id >= 0 && !excl_contains(p.excl_ids, x0, x1, id);
    const uint32_t bal = (uint32_t)((__ballot(keep) >> (lane & 48)) & 0xffffull);
    if (__builtin_popcount(bal) < k) {
        if (j == 0) p.short_list[4 + atomicAdd(&p.short_list[0], 1)] = (int32_t)u;
        return;
    }
    const v4f *pmu = reinterpret_cast<const v4f *>(p.pm) + (size_t)ul * (5 * E4);
    float hc[4], ha[4], G[10];
    rank_user_sums16(pmu, p.ce, E4, j, hc, ha, G);
    uint32_t m = bal;
    for (int o = 0; o < k; ++o, m &= m - 1) {               // the o-th survivor sits in the lane of m's lowest bit
        const int32_t d = __shfl(id, (lane & 48) + (__ffs(m) - 1), 64);
        const float s = rank_exact_score16(pmu, p.re, E4, j, d, dish_pattern(p.cats, d), p.a, p.b, hc);
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
    const int E4 = p.E >> 2;
    const int64_t nshort = p.all_short ? p.nU : (int64_t)p.short_list[0];
    float *o = p.plan + (size_t)s * 8;
    int64_t u = -1;
    if (s < nshort) u = p.all_short ? s : (int64_t)p.short_list[4 + s];
    int64_t ul = 0;
    if (u >= 0) {
        const int32_t uid = p.users[u];
        ul = (int64_t)uid - p.user_base;
        if (ul < 0 || ul >= p.U) {
            if (j == 0) m2d_latch_error(p.err, M2D_ERR_BAD_USER_ID, uid, u);
            u = -1;
        }
    }
    if (u < 0) {                                            // no user in this record: an empty mask, nothing scanned or written
        if (j < 8) o[j] = j == 6 ? __int_as_float(-1) : 0.f;
        return;
    }
    const v4f *pmu = reinterpret_cast<const v4f *>(p.pm) + (size_t)ul * (5 * E4);
    float hc[4], ha[4], G[10];
    rank_user_sums16(pmu, p.ce, E4, j, hc, ha, G);
    int64_t x0, x1;
    excl_segment(p, u, x0, x1);
    const int64_t rows_needed = (int64_t)p.k + (x1 - x0);   // (repeated ids only make it larger: still a bound)
    float seed, lo, hi;
    grouped_pattern_bounds_lanes(hc, ha, G, p.grp, (int)(rows_needed > 0x7fffffff ? 0x7fffffff : rows_needed), p.a, p.b, p.E, j, seed, lo, hi);
    const uint32_t mask = grouped_mask_lanes(hi, seed, j);
    if (j == 0) {
        atomicAdd(&p.counters[1], 1ull);
        o[0] = seed; o[1] = hc[0]; o[2] = hc[1]; o[3] = hc[2]; o[4] = hc[3]; o[5] = __uint_as_float(mask);
        o[6] = __int_as_float((int32_t)u); o[7] = 0.f;
    }
    if (j < 4) p.bnd[(size_t)s * 16 + j] = ha[j];
    if (j < 10) p.bnd[(size_t)s * 16 + 4 + j] = G[j];
}

// ---- tier 2, E <= 128: one lane per user -----------------------------------------------------------------------------------------------
template <int E4MAX>
__global__ __launch_bounds__(256) void m2d_topk_excl_scan(ExclArgs p)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nlive = (int64_t)p.counters[1];
    int64_t nqw;
    const int nsplit = excl_shape(p, nlive, nqw);
    if (g >= nqw * nsplit) return;
    const int64_t qw = g % nqw;
    const int split = (int)(g / nqw);
    const int E4 = p.E >> 2, k = p.k;
    const bool valid = qw * 64 + lane < nlive;
    const int64_t si = valid ? (int64_t)p.order[p.nU - nlive + qw * 64 + lane] : 0;
    const float *rec = p.plan + (size_t)si * 8;
    const float seed = rec[0];
    const float hc[4] = {rec[1], rec[2], rec[3], rec[4]};
    const int32_t u = valid ? __float_as_int(rec[6]) : -1;
    const bool live = u >= 0;
    const uint32_t mask = live ? __float_as_uint(rec[5]) : 0u;
    uint32_t um = mask;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) um |= __shfl_xor(um, off, 64);
    um = __builtin_amdgcn_readfirstlane(um);
    if (um == 0u) return;                                   // a wave of records without users
    float ha[4], G[10];
#pragma unroll
    for (int i = 0; i < 4; ++i) ha[i] = p.bnd[(size_t)si * 16 + i];
#pragma unroll
    for (int i = 0; i < 10; ++i) G[i] = p.bnd[(size_t)si * 16 + 4 + i];
    int64_t ul = live ? (int64_t)p.users[u] - p.user_base : 0;
    if (ul < 0 || ul >= p.U) ul = 0;                        // (latched by m2d_topk_excl_plan, which leaves such a record without a user)
    const v4f *pmu = reinterpret_cast<const v4f *>(p.pm) + (size_t)ul * (5 * E4);
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
    int64_t T = 0;
#pragma unroll
    for (int q = 1; q < GRP_MAXPAT; ++q) {
        float lo, hi;
        pattern_bound(pattern_bound_terms(hc, ha, G, q, p.a, p.b, p.E), __int_as_float(p.grp[GRP_RMAX + q]), lo, hi);
        float v = ((mask >> q) & 1u) ? fmaxf(hi, -INFINITY) : -INFINITY;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
        key[q] = v;
        T += ((um >> q) & 1u) ? (p.grp[40 + q] + 31) >> 5 : 0;
    }
    const int64_t per = (T + nsplit - 1) / nsplit, t0 = (int64_t)split * per, t1 = t0 + per < T ? t0 + per : T;
    const v4f *rows4 = reinterpret_cast<const v4f *>(p.rs);
    const int EW4 = p.ew >> 2;
    float ls[EXCL_KR];
    int32_t li[EXCL_KR];
    excl_list_init(ls, li, k);
    unsigned long long multiplied = 0ull;
    uint32_t avail = um;
    int64_t cum = 0;
    for (int it = 1; it < GRP_MAXPAT && cum < t1; ++it) {
        int best = -1;
        float bk = 0.f;
#pragma unroll
        for (int q = 1; q < GRP_MAXPAT; ++q) {
            if (((avail >> q) & 1u) && (best < 0 || key[q] > bk)) {
                best = q;
                bk = key[q];
            }
        }
        if (best < 0) break;
        const int q = __builtin_amdgcn_readfirstlane(best);   // (the keys are wave-uniform)
        avail &= ~(1u << q);
        const int64_t nt = (p.grp[40 + q] + 31) >> 5;
        const int64_t lo_t = t0 > cum ? t0 : cum, hi_t = t1 < cum + nt ? t1 : cum + nt;
        const int64_t tfirst = p.grp[q] >> 5;
        const int64_t c0 = cum;
        cum += nt;
        if (lo_t >= hi_t) continue;
        const PatternBoundTerms rb = pattern_bound_terms(hc, ha, G, q, p.a, p.b, p.E);
        const float alpha = repair_alpha(p.a, hc, q);
        const float npat = (float)__builtin_popcount(q);
        v4f w[E4MAX];
        rank_pattern_weights<E4MAX>(w, pmu, E4, q);
        for (int64_t t = lo_t; t < hi_t; ++t) {
            const int64_t tile = tfirst + (t - c0);
            const int nrows = p.tile_info[tile] >> 8;
            float blo, bhi;
            pattern_bound(rb, p.tnorm[tile], blo, bhi);
            // the lane's k-th score, the seed while its list is not full; strict: a row equal to either must reach the insertion
            const float thr = li[EXCL_KR - 1] != EXCL_NONE ? ls[EXCL_KR - 1] : seed;
            if (__ballot(live && !(bhi < thr)) == 0ull) continue;
            multiplied += 1ull;
            for (int r = 0; r < nrows; ++r) {
                const int64_t slot = tile * 32 + r;
                const int32_t id = __builtin_amdgcn_readfirstlane(p.perm[slot]);
                const v4f *row = rows4 + (size_t)slot * EW4;
                const float sc = rank_exact_score_lane<E4MAX>(w, row, E4, alpha, p.b, npat);
                const bool cand = live && !(sc < seed) && excl_before(sc, id, ls[EXCL_KR - 1], li[EXCL_KR - 1]);
                if (__ballot(cand) != 0ull) {               // rare once the lists are full
                    if (cand) {
                        bool found;
                        if (xn >= 0) {
                            int lo = 0, hi = xn;
                            while (lo < hi) {
                                const int mid = (lo + hi) >> 1;
                                if (xs[wv][mid][lane] < id) lo = mid + 1; else hi = mid;
                            }
                            found = lo < xn && xs[wv][lo][lane] == id;
                        } else {
                            found = excl_contains(p.excl_ids, x0, x1, id);
                        }
                        if (!found) excl_insert(ls, li, sc, id);
                    }
                }
            }
        }
    }
    if (live) excl_list_store(ls, li, k, p.part_s + ((size_t)g * 64 + lane) * k, p.part_i + ((size_t)g * 64 + lane) * k);
    if (lane == 0 && multiplied) atomicAdd(&p.counters[0], multiplied);
}

// ---- tier 2, E > 128: 16 lanes per (record, share of its patterns' tiles), every lane holding the list ---------------------------------
__global__ __launch_bounds__(256) void m2d_topk_excl_scan16(ExclArgs p)
{
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const int64_t nlive = (int64_t)p.counters[1];
    int64_t units;
    const int nsplit = excl_shape(p, nlive, units);
    if (g >= nlive * nsplit) return;                        // (whole 16-lane groups)
    const int64_t si = p.order[p.nU - nlive + g % nlive];
    const int split = (int)(g / nlive);
    const int E4 = p.E >> 2, k = p.k;
    const float *rec = p.plan + (size_t)si * 8;
    const int32_t u = __float_as_int(rec[6]);
    if (u < 0) return;
    const float seed = rec[0];
    const float hc[4] = {rec[1], rec[2], rec[3], rec[4]};
    const uint32_t mask = __float_as_uint(rec[5]);
    float ha[4], G[10];
#pragma unroll
    for (int i = 0; i < 4; ++i) ha[i] = p.bnd[(size_t)si * 16 + i];
#pragma unroll
    for (int i = 0; i < 10; ++i) G[i] = p.bnd[(size_t)si * 16 + 4 + i];
    int64_t ul = (int64_t)p.users[u] - p.user_base;
    if (ul < 0 || ul >= p.U) ul = 0;
    const v4f *pmu = reinterpret_cast<const v4f *>(p.pm) + (size_t)ul * (5 * E4);
    int64_t x0, x1;
    excl_segment(p, u, x0, x1);
    int64_t T = 0;
    for (int q = 1; q < GRP_MAXPAT; ++q) T += ((mask >> q) & 1u) ? (p.grp[40 + q] + 31) >> 5 : 0;
    const int64_t per = (T + nsplit - 1) / nsplit, t0 = (int64_t)split * per, t1 = t0 + per < T ? t0 + per : T;
    float ls[EXCL_KR];
    int32_t li[EXCL_KR];
    excl_list_init(ls, li, k);
    unsigned long long multiplied = 0ull;
    int64_t cum = 0;
    for (int q = 1; q < GRP_MAXPAT && cum < t1; ++q) {
        if (!((mask >> q) & 1u)) continue;
        const int64_t nt = (p.grp[40 + q] + 31) >> 5;
        const int64_t lo_t = t0 > cum ? t0 : cum, hi_t = t1 < cum + nt ? t1 : cum + nt;
        const int64_t tfirst = p.grp[q] >> 5;
        const int64_t c0 = cum;
        cum += nt;
        if (lo_t >= hi_t) continue;
        const PatternBoundTerms rb = pattern_bound_terms(hc, ha, G, q, p.a, p.b, p.E);
        for (int64_t t = lo_t; t < hi_t; ++t) {
            const int64_t tile = tfirst + (t - c0);
            const int nrows = p.tile_info[tile] >> 8;
            float blo, bhi;
            pattern_bound(rb, p.tnorm[tile], blo, bhi);
            const float thr = li[EXCL_KR - 1] != EXCL_NONE ? ls[EXCL_KR - 1] : seed;
            if (bhi < thr) continue;                        // (the same in all 16 lanes)
            multiplied += 1ull;
            for (int r = 0; r < nrows; ++r) {
                const int32_t id = p.perm[tile * 32 + r];
                const float sc = rank_exact_score16(pmu, p.re, E4, j, id, q, p.a, p.b, hc);
                if (!(sc < seed) && excl_before(sc, id, ls[EXCL_KR - 1], li[EXCL_KR - 1]) && !excl_contains(p.excl_ids, x0, x1, id))
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
    const int32_t u = __float_as_int(p.plan[(size_t)p.order[p.nU - nlive + t] * 8 + 6]);
    if (u < 0) return;
    const int k = p.k;
    int cnt = 0;
    for (int sp = 0; sp < nsplit; ++sp) {
        // where the scan kernels put share sp of this record: (wave, lane) of the one-lane form, the group of the 16-lane form
        const size_t slot = p.E <= 128 ? ((size_t)sp * units + (size_t)(t >> 6)) * 64 + (size_t)(t & 63) : (size_t)sp * nlive + (size_t)t;
        const float *ps = p.part_s + slot * k;
        const int32_t *pi = p.part_i + slot * k;
        for (int e = 0; e < k; ++e) {
            const int32_t id = pi[e];
            const float s = ps[e];
            if (id == EXCL_NONE) break;
            if (cnt == k && !excl_before(s, id, ms[k - 1][tx], mi[k - 1][tx])) break;     // (a share's list is sorted: nor can the rest)
            int i = cnt < k ? cnt : k - 1;
            for (; i > 0 && excl_before(s, id, ms[i - 1][tx], mi[i - 1][tx]); --i) {
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
        for (int64_t d = 0; d < p.I && cnt < k; ++d) {
            if (dish_pattern(p.cats, d) == 0 && !excl_contains(p.excl_ids, x0, x1, (int32_t)d)) {
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

int m2d_launch_topk_users_excluding(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int64_t *excl_off,
                                    const int32_t *excl_ids, float *out_scores, int32_t *out_ids, hipStream_t st)
{
    int rc;
    if ((rc = m2d_rank_prepare(h, "m2d_topk_users_excluding", st)) != M2D_OK) return rc;

    // tier 1 where m2d_topk_users' lists are index-exact against the ranking arithmetic (include/m2d.h), under the default options
    const int K1 = h->E == 128 ? 10 : 16;
    const bool tier1 = h->opt_topk_excl_tier != 2 && (h->E == 32 || h->E == 64 || h->E == 128) && k <= K1 && (int64_t)K1 <= h->I &&
                       h->grp_tiles > 0 && h->opt_topk_refine == 1 && h->opt_topk_grouped == 1 && h->opt_topk_form == 0 &&
                       h->opt_topk_prune == 1 && h->opt_topk_block == 0 && h->opt_variant == 0;
    // waves in flight, 8 per SIMD (E > 128: four 16-lane groups each).  The scan's items -- (wave of 64 users, share of its tiles), or
    // (user, share) -- are counted on the device (excl_shape): at most want + units of them, units <= those of nU users
    const int64_t want = (int64_t)h->num_cu * 32 * (h->E <= 128 ? 1 : 4);
    const int64_t items = want + (h->E <= 128 ? (nU + 63) / 64 : nU);

    // K1 lists: scores [nU, 16] | ids [nU, 16] | short list [4 + nU] | records [nU, 8] | bound sums [nU, 16] | order | sort histogram |
    // counters | partial lists: scores, ids [items, k]
    const size_t n4 = ((size_t)nU + 3) & ~(size_t)3;
    const size_t part = (size_t)items * (h->E <= 128 ? 64 : 1) * k;
    const size_t need = (size_t)nU * 32 + (4 + n4) + (size_t)nU * 24 + n4 + PLAN_KEYS + 8 + 2 * part;
    if ((rc = m2d_grow(h, h->excl_buf, h->excl_cap, need, sizeof(float), h->excl_counters, h->excl_short)) != M2D_OK) return rc;
    ExclArgs a;
    a.pm = h->pm; a.re = h->re; a.ce = h->ce; a.cats = h->dish_cats; a.rs = h->grp_rs; a.tnorm = h->rank_tnorm;
    a.perm = h->grp_perm; a.tile_info = h->grp_tile_info;
    a.grp = grouped_grp(h);
    a.users = users; a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.nU = nU; a.U = h->U; a.I = h->I; a.user_base = h->user_base; a.E = h->E; a.ew = h->grp_ew; a.k = k; a.want = want; a.K1 = K1;
    a.all_short = tier1 ? 0 : 1; a.a = h->a; a.b = h->b;
    float *list_s = h->excl_buf;
    int32_t *list_i = reinterpret_cast<int32_t *>(list_s + (size_t)nU * 16);
    a.list_i = list_i;
    a.short_list = list_i + (size_t)nU * 16;
    a.plan = reinterpret_cast<float *>(a.short_list + 4 + n4);
    a.bnd = a.plan + (size_t)nU * 8;
    int32_t *order = reinterpret_cast<int32_t *>(a.bnd + (size_t)nU * 16);
    int32_t *hist = order + n4;
    a.counters = reinterpret_cast<unsigned long long *>(hist + PLAN_KEYS);
    a.part_s = reinterpret_cast<float *>(hist + PLAN_KEYS + 8);
    a.part_i = reinterpret_cast<int32_t *>(a.part_s + part);
    a.order = order;
    a.out_scores = out_scores; a.out_ids = out_ids; a.err = h->err_dev;
    h->excl_counters = a.counters;
    h->excl_short = a.short_list;
    h->excl_all_short = tier1 ? -1 : nU;
    M2D_HIP_TRY(h, hipMemsetAsync(a.counters, 0, 8 * sizeof(int32_t), st));
    M2D_HIP_TRY(h, hipMemsetAsync(a.short_list, 0, 4 * sizeof(int32_t), st));
    if (excl_off) {
        hipLaunchKernelGGL(m2d_topk_excl_check, dim3((unsigned)(h->num_cu * 4)), dim3(256), 0, st, a);
        M2D_HIP_TRY(h, hipGetLastError());
    }
    const dim3 g16((unsigned)((nU * 16 + 255) / 256));
    if (tier1) {
        if ((rc = m2d_launch_topk_users(h, users, nU, K1, list_s, list_i, st)) != M2D_OK) return rc;
        hipLaunchKernelGGL(m2d_topk_excl_filter, g16, dim3(256), 0, st, a);
        M2D_HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(m2d_topk_excl_plan, g16, dim3(256), 0, st, a);
    M2D_HIP_TRY(h, hipGetLastError());
    // records with users last (an empty mask is key 0), grouped by pattern mask so that the 64 users of a wave share patterns
    if ((rc = m2d_plan_sort_launch(h, a.plan, nU, hist, order, st)) != M2D_OK) return rc;
    if (h->E <= 128) {
        const dim3 grid((unsigned)((items + 3) / 4));
        if (h->E <= 32) hipLaunchKernelGGL(m2d_topk_excl_scan<8>, grid, dim3(256), 0, st, a);
        else if (h->E <= 64) hipLaunchKernelGGL(m2d_topk_excl_scan<16>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(m2d_topk_excl_scan<32>, grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(m2d_topk_excl_scan16, dim3((unsigned)((items * 16 + 255) / 256)), dim3(256), 0, st, a);
    }
    M2D_HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(m2d_topk_excl_merge, dim3((unsigned)((nU + 255) / 256)), dim3(256), 0, st, a);
    M2D_HIP_TRY(h, hipGetLastError());
    h->last_kernel = "m2d_topk_excl_scan";
    return M2D_OK;
}
