// m2d_catalogue_rank: for queries (user u, held-out dish p), the number of dishes that precede p in m2d_topk_users' order
// (score descending, NaN last, equal scores to the lower id), leaving out an optional ascending list of dish ids per query.
//
// The score is the tie repair's plain-f32 arithmetic (m2d_topk_repair_scan, m2d_topk_refine): alpha_P from <U_high, CE_c> summed
// exactly as m2d_topk_user_plan sums it, low = a float4 column per lane of 16 in fmaf chains, combined by row16_sum, then
// repair_score_planned(alpha_P, b, low / n_P).  Wherever retrieval lists are index-exact the two calls then agree as integers:
// rank(u, ids[u][j]) == j.
//
//   m2d_rank_plan      16 lanes per query: the id checks, <U_high, CE_c> and the bound sums, s* = the score of p, the 15 patterns
//                      classified by grouped_pattern_terms -- ahead (lo > s*: every row counts), behind (hi < s*), straddling (word 5
//                      of the record, the key m2d_plan_hist / _scan / _scatter sort the queries by)
//   m2d_rank_count     a wave per 64 sorted queries and share of the tiles of their straddling patterns: a tile whose bound (the
//                      pattern's, with the tile's largest row norm in place of the pattern's) settles a lane is counted without
//                      multiplying; the others are scored in the exact arithmetic, one lane per query, the dish row wave-uniform
//   m2d_rank_exclude   16 lanes per (query, excluded id): the id's exact score against (s*, p); one less if it precedes
#include "m2d_catalogue.h"

#pragma clang fp contract(off)

namespace {

struct RankArgs {
    const float *pm, *re, *ce, *cats;
    const float *rs;                 // the pattern-sorted f32 dish table (row stride ew floats) and per-tile largest row norm
    const float *tnorm;
    const int32_t *perm, *tile_info, *grp, *blk_hist;
    const int32_t *users, *items;
    const int64_t *excl_off;
    const int32_t *excl_ids;
    int64_t n, U, I, user_base;
    int32_t E, ew, nsplit;
    float a, b;
    float *plan;                     // [n, 8]  s*, <U_high, CE_c> x 4, straddling-pattern mask, p, p's pattern
    float *bnd;                      // [n, 16] the bound sums: sum |U_high CE_c| x 4, the Gram matrix of the U_low rows (10)
    const int32_t *order;            // sorted position -> query, or null
    int32_t *out_rank;
    float *out_scores;
    int32_t *err;
    unsigned long long *counters;    // [0] tiles multiplied, [1] pairs decided in the exact arithmetic
};

// ---- per query: checks, sums, s*, the patterns' classes ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void m2d_rank_plan(RankArgs p)
{
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, q = gid >> 4;
    const int E = p.E, E4 = E >> 2;
    if (gid == 0) { p.counters[0] = 0ull; p.counters[1] = 0ull; }
    if (q >= p.n) return;                                   // (16-lane groups are whole: row operations below see a full row)
    bool bad = false;
    const int32_t uid = p.users[q];
    int64_t ul = (int64_t)uid - p.user_base;
    if (ul < 0 || ul >= p.U) {
        if (j == 0) m2d_latch_error(p.err, M2D_ERR_BAD_USER_ID, uid, q);
        ul = 0;
        bad = true;
    }
    int32_t it = p.items[q];
    if (it < 0 || (int64_t)it >= p.I) {
        if (j == 0) m2d_latch_error(p.err, M2D_ERR_BAD_ITEM_ID, it, q);
        it = 0;
        bad = true;
    }
    const v4f *pmu = reinterpret_cast<const v4f *>(p.pm) + (size_t)ul * (5 * E4);
    float hc[4], ha[4], G[10];
    rank_user_sums16(pmu, p.ce, E4, j, hc, ha, G);
    const int ppt = dish_pattern(p.cats, it);
    const float s = rank_exact_score16(pmu, p.re, E4, j, it, ppt, p.a, p.b, hc);
    // lane j >= 1 classifies pattern j
    int ahead = 0;
    uint32_t mask = 0u;
    if (j >= 1) {
        const int rows = p.grp[40 + j];
        float lo, hi;
        grouped_pattern_terms(hc, ha, G, p.grp, j, 1, p.a, p.b, E, lo, hi);
        if (ppt == 0) ahead = rows;                         // p scores NaN: every dish with a mask precedes it
        else if (lo > s) ahead = rows;
        else if (!(hi < s) && rows > 0) mask = 1u << j;
    }
    // NaN s*: the empty-mask dishes (NaN too) with a lower id precede p -- those of the 256-dish blocks in front of p's (the table
    // build's block histogram, pattern 0's keys) and those of its own block in front of it
    int empt = 0;
    if (s != s) {
        const int64_t blk = it >> 8;
        empt = p.blk_hist[(size_t)blk * GRP_KEYS + j];      // keys 0 ... 15: pattern 0, every norm bucket
        for (int64_t d = (blk << 8) + j; d < it; d += 16) empt += dish_pattern(p.cats, d) == 0 ? 1 : 0;
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
        ahead += __shfl_xor(ahead, off, 64);
        empt += __shfl_xor(empt, off, 64);
        mask |= __shfl_xor(mask, off, 64);
    }
    if (bad) mask = 0u;
    if (j == 0) {
        float *o = p.plan + (size_t)q * 8;
        o[0] = s; o[1] = hc[0]; o[2] = hc[1]; o[3] = hc[2]; o[4] = hc[3]; o[5] = __uint_as_float(mask);
        o[6] = __int_as_float(it); o[7] = __int_as_float(ppt);
        p.out_rank[q] = ahead + empt;
        if (p.out_scores) p.out_scores[q] = s;
    }
    if (j < 4) p.bnd[(size_t)q * 16 + j] = ha[j];
    if (j < 10) p.bnd[(size_t)q * 16 + 4 + j] = G[j];
}

// ---- the count: one lane per query, E <= 128 ---------------------------------------------------------------------------------------
// A wave takes 64 sorted queries and one of `nsplit` shares of the tiles of their straddling patterns (the union over the wave).
// Per tile each lane's bound -- alpha_P +- the pattern's reach with the tile's largest row norm -- settles it (ahead: the tile's
// rows count; behind: nothing) or not; a tile some lane needs is multiplied for all, a row at a time: the row and its id are
// wave-uniform (scalar loads), the lane's w_P sits in registers.  The score is the repair's arithmetic: lane j's chain of the
// 16-lane form is the chain of part[j] here (float4 columns j, j + 16, ... in order), row16_sum's rotations are the pairs
// (i, i + 8), (i, i + 4), (i, i + 2), (i, i + 1) -- float addition commutes, so every order of a pair gives the same bits.
template <int E4MAX>
__global__ __launch_bounds__(256) void m2d_rank_count(RankArgs p)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nqw = (p.n + 63) >> 6;
    if (g >= nqw * p.nsplit) return;
    const int64_t qw = g % nqw;
    const int split = (int)(g / nqw);
    const int E4 = p.E >> 2;
    const int64_t pos = qw * 64 + lane;
    const bool valid = pos < p.n;
    const int64_t qi = valid ? (p.order ? (int64_t)p.order[pos] : pos) : 0;
    const float *rec = p.plan + (size_t)qi * 8;
    const float s = rec[0];
    const float hc[4] = {rec[1], rec[2], rec[3], rec[4]};
    const uint32_t mask = valid ? __float_as_uint(rec[5]) : 0u;
    const int32_t pd = __float_as_int(rec[6]);
    float ha[4], G[10];
#pragma unroll
    for (int i = 0; i < 4; ++i) ha[i] = p.bnd[(size_t)qi * 16 + i];
#pragma unroll
    for (int i = 0; i < 10; ++i) G[i] = p.bnd[(size_t)qi * 16 + 4 + i];
    uint32_t um = mask;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) um |= __shfl_xor(um, off, 64);
    um = __builtin_amdgcn_readfirstlane(um);
    int64_t T = 0;
    for (int q = 1; q < GRP_MAXPAT; ++q) T += ((um >> q) & 1u) ? (p.grp[40 + q] + 31) >> 5 : 0;
    const int64_t per = (T + p.nsplit - 1) / p.nsplit, t0 = (int64_t)split * per, t1 = t0 + per < T ? t0 + per : T;
    if (t0 >= t1) return;
    int64_t ul = valid ? (int64_t)p.users[qi] - p.user_base : 0;
    if (ul < 0 || ul >= p.U) ul = 0;                        // (latched by m2d_rank_plan)
    const v4f *pmu = reinterpret_cast<const v4f *>(p.pm) + (size_t)ul * (5 * E4);
    const v4f *rows4 = reinterpret_cast<const v4f *>(p.rs);
    const int EW4 = p.ew >> 2;
    int count = 0;
    unsigned long long multiplied = 0ull, resolved = 0ull;
    int64_t cum = 0;
    for (int q = 1; q < GRP_MAXPAT; ++q) {                  // wave-uniform
        if (!((um >> q) & 1u)) continue;
        const int64_t nt = (p.grp[40 + q] + 31) >> 5;
        const int64_t lo_t = t0 > cum ? t0 : cum, hi_t = t1 < cum + nt ? t1 : cum + nt;
        const int64_t tfirst = p.grp[q] >> 5;
        const int64_t c0 = cum;
        cum += nt;
        if (lo_t >= hi_t) continue;
        const bool straddle = (mask >> q) & 1u;
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
            const bool ahead_t = straddle && blo > s;
            const bool need = straddle && !ahead_t && !(bhi < s);
            count += ahead_t ? nrows : 0;
            const unsigned long long ball = __ballot(need);
            if (ball == 0ull) continue;
            multiplied += 1ull;
            resolved += (unsigned long long)__builtin_popcountll(ball) * (unsigned long long)nrows;
            for (int r = 0; r < nrows; ++r) {
                const int64_t slot = tile * 32 + r;
                const int32_t id = __builtin_amdgcn_readfirstlane(p.perm[slot]);
                const v4f *row = rows4 + (size_t)slot * EW4;
                const float sc = rank_exact_score_lane<E4MAX>(w, row, E4, alpha, p.b, npat);
                count += (need && rank_precedes(sc, id, s, pd)) ? 1 : 0;
            }
        }
    }
    if (valid && count) atomicAdd(&p.out_rank[qi], count);
    if (lane == 0 && multiplied) {
        atomicAdd(&p.counters[0], multiplied);
        atomicAdd(&p.counters[1], resolved);
    }
}

// ---- the count, E > 128: 16 lanes per (query, share of its straddling rows), the repair's own layout -------------------------------
__global__ __launch_bounds__(256) void m2d_rank_count16(RankArgs p)
{
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (g >= p.n * p.nsplit) return;                        // (whole 16-lane groups)
    const int64_t qi = g % p.n;
    const int split = (int)(g / p.n);
    const int E4 = p.E >> 2;
    const float *rec = p.plan + (size_t)qi * 8;
    const float s = rec[0];
    const float hc[4] = {rec[1], rec[2], rec[3], rec[4]};
    const uint32_t mask = __float_as_uint(rec[5]);
    const int32_t pd = __float_as_int(rec[6]);
    int64_t R = 0;
    for (int q = 1; q < GRP_MAXPAT; ++q) R += ((mask >> q) & 1u) ? p.grp[40 + q] : 0;
    const int64_t per = (R + p.nsplit - 1) / p.nsplit, i0 = (int64_t)split * per, i1 = i0 + per < R ? i0 + per : R;
    if (i0 >= i1) return;
    int64_t ul = (int64_t)p.users[qi] - p.user_base;
    if (ul < 0 || ul >= p.U) ul = 0;
    const v4f *pmu = reinterpret_cast<const v4f *>(p.pm) + (size_t)ul * (5 * E4);
    int count = 0;
    int64_t cum = 0;
    for (int q = 1; q < GRP_MAXPAT; ++q) {
        const int64_t rq = ((mask >> q) & 1u) ? p.grp[40 + q] : 0;
        const int64_t a0 = i0 > cum ? i0 : cum, a1 = i1 < cum + rq ? i1 : cum + rq;
        for (int64_t i = a0; i < a1; ++i) {
            const int32_t id = p.perm[p.grp[q] + (i - cum)];
            const float sc = rank_exact_score16(pmu, p.re, E4, j, id, q, p.a, p.b, hc);
            count += rank_precedes(sc, id, s, pd) ? 1 : 0;
        }
        cum += rq;
    }
    if (j == 0) {
        if (count) atomicAdd(&p.out_rank[qi], count);
        atomicAdd(&p.counters[1], (unsigned long long)(i1 - i0));
    }
}

// ---- exclusions: 16 lanes per (query, excluded id) -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void m2d_rank_exclude(RankArgs p)
{
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t g0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4, ng = ((int64_t)gridDim.x * 256) >> 4;
    const int E4 = p.E >> 2;
    // the offsets themselves: non-decreasing from 0
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q <= p.n; q += (int64_t)gridDim.x * 256) csr_check_offset(p.excl_off, q, p.err);
    const int64_t nnz = p.excl_off[p.n];
    for (int64_t i = g0; i < nnz; i += ng) {                // 16-lane-uniform
        int32_t x;
        int64_t q;                                          // the query
        if (csr_check_id(p.excl_off, p.excl_ids, p.n, p.I, i, j == 0, p.err, x, q) != 1) continue;     // (a repeated id counts once)
        const float *rec = p.plan + (size_t)q * 8;
        const int32_t pd = __float_as_int(rec[6]);
        if (x == pd) continue;                              // p in its own list: ignored
        const float hc[4] = {rec[1], rec[2], rec[3], rec[4]};
        int64_t ul = (int64_t)p.users[q] - p.user_base;
        if (ul < 0 || ul >= p.U) ul = 0;
        const v4f *pmu = reinterpret_cast<const v4f *>(p.pm) + (size_t)ul * (5 * E4);
        const int pt = dish_pattern(p.cats, x);
        const bool empty_p = __float_as_int(rec[7]) == 0;
        bool prec;
        if (pt == 0) prec = rec[0] != rec[0] && x < pd;    // NaN: after every score, before a NaN p of higher id
        else if (empty_p) prec = true;                      // p scores NaN (m2d_rank_plan counted every dish with a mask)
        else prec = rank_precedes(rank_exact_score16(pmu, p.re, E4, j, x, pt, p.a, p.b, hc), x, rec[0], pd);
        if (j == 0 && prec) atomicSub(&p.out_rank[q], 1);
    }
}

// one wave per 32-row tile of the sorted table: its largest row norm (a NaN norm counts as +inf; padding rows are zeros)
__global__ __launch_bounds__(256) void m2d_rank_tile_norms(const float *rs, int64_t tiles, int E, int ew, float *tnorm)
{
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= tiles) return;
    float mx = 0.f;
    for (int r = 0; r < 32; ++r) {
        float q = 0.f;
        for (int e = lane; e < E; e += 64) {
            const float x = rs[(size_t)(t * 32 + r) * ew + e];
            q = fmaf(x, x, q);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
        const float nr = sqrtf(q);
        mx = fmaxf(mx, nr == nr ? nr : INFINITY);
    }
    if (lane == 0) tnorm[t] = mx * (1.0f + 1e-6f);           // (a few ulp over this loop's f32 sum: the bound's row norms are upper bounds)
}

}  // namespace

// What m2d_catalogue_rank and m2d_topk_users_excluding (`entry`: the name their refusals carry) need before they launch: a model
// the ranking arithmetic covers, the sorted dish table, and h->rank_tnorm for that table as it stands (rebuilt when the table
// was: grp_gen)
int m2d_rank_prepare(m2d_engine *h, const char *entry, hipStream_t st)
{
    auto refuse = [&](const char *why) {
        h->last_error = std::string(entry) + ": " + why;
        return M2D_ERR_UNSUPPORTED;
    };
    if (h->C != 4) return refuse("needs C = 4 categories");
    if (h->E % 4 != 0 || h->E > 256) return refuse("needs E a multiple of 4 up to 256");
    if (h->ing || h->dish_high) return refuse("the ingredient table is set (not supported)");
    if (h->mlp_w1) return refuse("the MLP head is set (not supported)");
    int rc;
    if ((rc = m2d_ensure_finite_scan(h, st)) != M2D_OK) return rc;
    if ((rc = m2d_grouped_tables(h, st)) != M2D_OK) return rc;
    if (!h->grp_binary) return refuse("needs 0/1 dish masks (a mask weight is neither 0 nor 1)");
    if (h->grp_nonfinite) return refuse("needs finite tables (a table value is inf or NaN)");
    const int64_t tiles = h->grp_tiles;
    if (h->rank_tnorm_gen != h->grp_gen) {
        if ((rc = m2d_grow(h, h->rank_tnorm, h->rank_tnorm_cap, (size_t)(tiles + 1), sizeof(float))) != M2D_OK) return rc;
        if (tiles > 0)
            hipLaunchKernelGGL(m2d_rank_tile_norms, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, st, h->grp_rs, tiles, h->E, h->grp_ew, h->rank_tnorm);
        M2D_HIP_TRY(h, hipGetLastError());
        h->rank_tnorm_gen = h->grp_gen;
    }
    return M2D_OK;
}

int m2d_launch_catalogue_rank(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t n, const int64_t *excl_off,
                              const int32_t *excl_ids, int32_t *out_rank, float *out_scores, hipStream_t st)
{
    int rc;
    if ((rc = m2d_rank_prepare(h, "m2d_catalogue_rank", st)) != M2D_OK) return rc;
    // records [n, 8] | bound sums [n, 16] | order [n] | sort histogram | counters
    const size_t n4 = ((size_t)n + 3) & ~(size_t)3;
    const size_t need = (size_t)n * 24 + n4 + PLAN_KEYS + 8;
    if ((rc = m2d_grow(h, h->rank_buf, h->rank_cap, need, sizeof(float), h->rank_counters)) != M2D_OK) return rc;
    RankArgs a;
    a.pm = h->pm; a.re = h->re; a.ce = h->ce; a.cats = h->dish_cats; a.rs = h->grp_rs; a.tnorm = h->rank_tnorm;
    a.perm = h->grp_perm; a.tile_info = h->grp_tile_info;
    a.blk_hist = h->grp_work;                                // per 256-dish block: dishes of each key in the blocks before it
    a.grp = grouped_grp(h);
    a.users = users; a.items = items; a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.n = n; a.U = h->U; a.I = h->I; a.user_base = h->user_base; a.E = h->E; a.ew = h->grp_ew; a.a = h->a; a.b = h->b;
    a.plan = h->rank_buf;
    a.bnd = a.plan + (size_t)n * 8;
    int32_t *order = reinterpret_cast<int32_t *>(a.bnd + (size_t)n * 16);
    int32_t *hist = order + n4;
    a.counters = reinterpret_cast<unsigned long long *>(hist + PLAN_KEYS);
    h->rank_counters = a.counters;
    a.order = nullptr;
    a.out_rank = out_rank; a.out_scores = out_scores; a.err = h->err_dev;
    a.nsplit = 1;
    hipLaunchKernelGGL(m2d_rank_plan, dim3((unsigned)((n * 16 + 255) / 256)), dim3(256), 0, st, a);
    M2D_HIP_TRY(h, hipGetLastError());
    const int64_t want = (int64_t)h->num_cu * 32;            // waves in flight: 8 per SIMD
    if (h->E <= 128) {
        if (n > 64) {
            if ((rc = m2d_plan_sort_launch(h, a.plan, n, hist, order, st)) != M2D_OK) return rc;
            a.order = order;
        }
        const int64_t nqw = (n + 63) / 64;
        int64_t ns = (want + nqw - 1) / nqw;
        a.nsplit = (int)(ns < 1 ? 1 : (ns > 512 ? 512 : ns));
        const int64_t waves = nqw * a.nsplit;
        const dim3 grid((unsigned)((waves + 3) / 4));
        if (h->E <= 32) hipLaunchKernelGGL(m2d_rank_count<8>, grid, dim3(256), 0, st, a);
        else if (h->E <= 64) hipLaunchKernelGGL(m2d_rank_count<16>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(m2d_rank_count<32>, grid, dim3(256), 0, st, a);
    } else {
        int64_t ns = (want * 4 + n - 1) / n;
        a.nsplit = (int)(ns < 1 ? 1 : (ns > 512 ? 512 : ns));
        hipLaunchKernelGGL(m2d_rank_count16, dim3((unsigned)((n * a.nsplit * 16 + 255) / 256)), dim3(256), 0, st, a);
    }
    M2D_HIP_TRY(h, hipGetLastError());
    if (excl_off) {
        hipLaunchKernelGGL(m2d_rank_exclude, dim3((unsigned)(h->num_cu * 8)), dim3(256), 0, st, a);
        M2D_HIP_TRY(h, hipGetLastError());
    }
    h->last_kernel = "m2d_rank_count";
    return M2D_OK;
}
