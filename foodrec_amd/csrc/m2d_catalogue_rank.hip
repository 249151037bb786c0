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
//   m2d_rank_count     a wave per 64 sorted queries and share of the tiles of their straddling patterns, ascending, on the walk it
//                      shares with m2d_topk_excl_scan (walk_tiles, m2d_catalogue.h): a tile whose bound settles a lane is counted
//                      without multiplying (ahead: its rows count; behind: nothing), a scored row counts where it precedes (s*, p)
//   m2d_rank_count16   E > 128: 16 lanes per (query, share of its straddling ROWS), every row decided -- no tile bound, so no walk
//   m2d_rank_exclude   16 lanes per (query, excluded id): the id's exact score against (s*, p); one less if it precedes
#include "m2d_catalogue.h"
#include "m2d_exclusions.h"   // (m2d_rank_exclude's fused check-and-count: csr_check_offset / csr_check_id)

#pragma clang fp contract(off)

namespace {

struct RankArgs {
    RankTables t;
    const int32_t *blk_hist;         // per 256-dish block: dishes of each key in the blocks before it (the table build's histogram)
    const int32_t *users, *items;
    const int64_t *excl_off;
    const int32_t *excl_ids;
    int64_t n;
    int32_t nsplit;
    float *plan, *bnd;               // the records (m2d_catalogue.h, RankRecord): s*, the straddling patterns, p, p's pattern
    const int32_t *order;            // sorted position -> query, or null
    int32_t *out_rank;
    float *out_scores;
    unsigned long long *counters;    // [0] tiles multiplied, [1] pairs decided in the exact arithmetic
};

// ---- per query: checks, sums, s*, the patterns' classes ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void m2d_rank_plan(RankArgs p)
{
    const RankTables &t = p.t;
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, q = gid >> 4;
    const int E = t.E, E4 = E >> 2;
    if (gid == 0) { p.counters[0] = 0ull; p.counters[1] = 0ull; }
    if (q >= p.n) return;                                   // (16-lane groups are whole: row operations below see a full row)
    bool bad = false;
    const int32_t uid = p.users[q];
    const int64_t ul = (int64_t)uid - t.user_base;
    if (ul < 0 || ul >= t.U) {
        if (j == 0) m2d_latch_error(t.err, M2D_ERR_BAD_USER_ID, uid, q);
        bad = true;
    }
    int32_t it = p.items[q];
    if (it < 0 || (int64_t)it >= t.I) {
        if (j == 0) m2d_latch_error(t.err, M2D_ERR_BAD_ITEM_ID, it, q);
        it = 0;
        bad = true;
    }
    const v4f *pmu = user_block(t, uid);
    float hc[4], ha[4], G[10];
    rank_user_sums16(pmu, t.ce, E4, j, hc, ha, G);
    const int ppt = dish_pattern(t.cats, it);
    const float s = rank_exact_score16(pmu, t.re, E4, j, it, ppt, t.a, t.b, hc);
    // lane j >= 1 classifies pattern j
    int ahead = 0;
    uint32_t mask = 0u;
    if (j >= 1) {
        const int rows = t.grp[40 + j];
        float lo, hi;
        grouped_pattern_terms(hc, ha, G, t.grp, j, 1, t.a, t.b, E, lo, hi);
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
        for (int64_t d = (blk << 8) + j; d < it; d += 16) empt += dish_pattern(t.cats, d) == 0 ? 1 : 0;
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
        ahead += __shfl_xor(ahead, off, 64);
        empt += __shfl_xor(empt, off, 64);
        mask |= __shfl_xor(mask, off, 64);
    }
    if (bad) mask = 0u;
    record_store(p.plan, p.bnd, q, j, s, hc, mask, it, ppt, ha, G);
    if (j == 0) {
        p.out_rank[q] = ahead + empt;
        if (p.out_scores) p.out_scores[q] = s;
    }
}

// ---- the count: one lane per query, E <= 128 ---------------------------------------------------------------------------------------
template <int E4MAX>
__global__ __launch_bounds__(256) void m2d_rank_count(RankArgs p)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t nqw = (p.n + 63) >> 6;
    if (g >= nqw * p.nsplit) return;
    const int64_t qw = g % nqw;
    const int split = (int)(g / nqw);
    const int64_t pos = qw * 64 + lane;
    const bool valid = pos < p.n;
    const int64_t qi = valid ? (p.order ? (int64_t)p.order[pos] : pos) : 0;
    const RankRecord rec = record_load(p.plan, p.bnd, qi);
    const uint32_t mask = valid ? rec.mask : 0u;
    uint32_t um = mask;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) um |= __shfl_xor(um, off, 64);
    um = __builtin_amdgcn_readfirstlane(um);
    int64_t t0, t1;
    share_of(pattern_set_tiles(p.t.grp, um), p.nsplit, split, t0, t1);
    if (t0 >= t1) return;
    const v4f *pmu = user_block(p.t, valid ? (int64_t)p.users[qi] : p.t.user_base);      // (a bad id: latched by m2d_rank_plan)
    int count = 0;
    unsigned long long resolved = 0ull;
    const unsigned long long multiplied = walk_tiles<E4MAX>(
        p.t, pmu, rec, um, t0, t1, [](const uint32_t avail) { return __ffs(avail) - 1; },
        [&](const int q, const float blo, const float bhi, const int nrows) {
            const bool straddle = (mask >> q) & 1u;
            const bool ahead_t = straddle && blo > rec.s;
            const bool need = straddle && !ahead_t && !(bhi < rec.s);
            count += ahead_t ? nrows : 0;
            resolved += (unsigned long long)__builtin_popcountll(__ballot(need)) * (unsigned long long)nrows;
            return need;
        },
        [&](const float sc, const int32_t id, const bool need) { count += (need && rank_precedes(sc, id, rec.s, rec.id)) ? 1 : 0; });
    if (valid && count) atomicAdd(&p.out_rank[qi], count);
    if (lane == 0 && multiplied) {
        atomicAdd(&p.counters[0], multiplied);
        atomicAdd(&p.counters[1], resolved);
    }
}

// ---- the count, E > 128: 16 lanes per (query, share of its straddling rows), the repair's own layout -------------------------------
// It stands apart from the walk: a group has one query and cuts that query's ROWS into shares, not the tiles of a wave's patterns,
// and decides every row (no tile bound).  It shares the record and the user block only.
__global__ __launch_bounds__(256) void m2d_rank_count16(RankArgs p)
{
    const RankTables &t = p.t;
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (g >= p.n * p.nsplit) return;                        // (whole 16-lane groups)
    const int64_t qi = g % p.n;
    const int split = (int)(g / p.n);
    const int E4 = t.E >> 2;
    const RankRecord rec = record_load(p.plan, p.bnd, qi);
    const uint32_t mask = rec.mask;
    int64_t R = 0;
    for (int q = 1; q < GRP_MAXPAT; ++q) R += ((mask >> q) & 1u) ? t.grp[40 + q] : 0;
    const int64_t per = (R + p.nsplit - 1) / p.nsplit, i0 = (int64_t)split * per, i1 = i0 + per < R ? i0 + per : R;
    if (i0 >= i1) return;
    const v4f *pmu = user_block(t, p.users[qi]);
    int count = 0;
    int64_t cum = 0;
    for (int q = 1; q < GRP_MAXPAT; ++q) {
        const int64_t rq = ((mask >> q) & 1u) ? t.grp[40 + q] : 0;
        const int64_t a0 = i0 > cum ? i0 : cum, a1 = i1 < cum + rq ? i1 : cum + rq;
        for (int64_t i = a0; i < a1; ++i) {
            const int32_t id = t.perm[t.grp[q] + (i - cum)];
            const float sc = rank_exact_score16(pmu, t.re, E4, j, id, q, t.a, t.b, rec.hc);
            count += rank_precedes(sc, id, rec.s, rec.id) ? 1 : 0;
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
    const RankTables &t = p.t;
    const int lane = threadIdx.x & 63, j = lane & 15;
    const int64_t g0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4, ng = ((int64_t)gridDim.x * 256) >> 4;
    const int E4 = t.E >> 2;
    // the offsets themselves: non-decreasing from 0
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q <= p.n; q += (int64_t)gridDim.x * 256) csr_check_offset(p.excl_off, q, t.err);
    const int64_t nnz = p.excl_off[p.n];
    for (int64_t i = g0; i < nnz; i += ng) {                // 16-lane-uniform
        int32_t x;
        int64_t q;                                          // the query
        if (csr_check_id(p.excl_off, p.excl_ids, p.n, t.I, i, j == 0, t.err, x, q) != 1) continue;     // (a repeated id counts once)
        const RankRecord rec = record_load(p.plan, p.bnd, q);
        if (x == rec.id) continue;                          // p in its own list: ignored
        const int pt = dish_pattern(t.cats, x);
        bool prec;
        if (pt == 0) prec = rec.s != rec.s && x < rec.id;   // NaN: after every score, before a NaN p of higher id
        else if (rec.tag == 0) prec = true;                 // p scores NaN (m2d_rank_plan counted every dish with a mask)
        else prec = rank_precedes(rank_exact_score16(user_block(t, p.users[q]), t.re, E4, j, x, pt, t.a, t.b, rec.hc), x, rec.s, rec.id);
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
int m2d_rank_prepare(m2d_engine *h, const char *entry, hipStream_t st, bool under_head)
{
    auto refuse = [&](const char *why) {
        h->last_error = std::string(entry) + ": " + why;
        return M2D_ERR_UNSUPPORTED;
    };
    if (h->C != 4) return refuse("needs C = 4 categories");
    if (h->E % 4 != 0 || h->E > 256) return refuse("needs E a multiple of 4 up to 256");
    if (h->ing || h->dish_high) return refuse("the ingredient table is set (not supported)");
    if (h->mlp_w1 && !under_head) return refuse("the MLP head is set (not supported)");
    int rc;
    if ((rc = m2d_ensure_finite_scan(h, st)) != M2D_OK) return rc;
    if ((rc = m2d_grouped_tables(h, st)) != M2D_OK) return rc;
    if (!h->grp_binary) return refuse("needs 0/1 dish masks (a mask weight is neither 0 nor 1)");
    if (h->grp_nonfinite) return refuse("needs finite tables (a table value is inf or NaN)");
    const int64_t tiles = h->grp_tiles;
    if (h->rank_tnorm_gen != h->grp_gen) {
        if ((rc = h->rank_tnorm.grow(h, (size_t)(tiles + 1))) != M2D_OK) return rc;
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
    if ((rc = h->rank_buf.grow(h, rank_scratch(nullptr, n).floats, h->rank_counters)) != M2D_OK) return rc;
    const RankScratch sc = rank_scratch(h->rank_buf, n);
    RankArgs a;
    a.t = rank_tables(h);
    a.blk_hist = h->grp_work;
    a.users = users; a.items = items; a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.n = n;
    a.plan = sc.plan; a.bnd = sc.bnd; a.counters = sc.counters;
    h->rank_counters = a.counters;
    a.order = nullptr;
    a.out_rank = out_rank; a.out_scores = out_scores;
    a.nsplit = 1;
    hipLaunchKernelGGL(m2d_rank_plan, dim3((unsigned)((n * 16 + 255) / 256)), dim3(256), 0, st, a);
    M2D_HIP_TRY(h, hipGetLastError());
    const int64_t want = (int64_t)h->num_cu * 32;            // waves in flight: 8 per SIMD
    dim3 grid;
    if (h->E <= 128) {                                       // a wave per (64 sorted queries, share of their tiles)
        if (n > 64) {
            if ((rc = m2d_plan_sort_launch(h, a.plan, n, sc.hist, sc.order, st)) != M2D_OK) return rc;
            a.order = sc.order;
        }
        const int64_t nqw = (n + 63) / 64;
        a.nsplit = share_count(want, nqw);
        grid = dim3((unsigned)((nqw * a.nsplit + 3) / 4));
    } else {                                                 // a 16-lane group per (query, share of its rows)
        a.nsplit = share_count(want * 4, n);
        grid = dim3((unsigned)((n * a.nsplit * 16 + 255) / 256));
    }
    with_rank_width(h->E, [&](auto w) {
        constexpr int W = decltype(w)::value;
        if constexpr (W != 0) hipLaunchKernelGGL(m2d_rank_count<W>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(m2d_rank_count16, grid, dim3(256), 0, st, a);
    });
    M2D_HIP_TRY(h, hipGetLastError());
    if (excl_off) {
        hipLaunchKernelGGL(m2d_rank_exclude, dim3((unsigned)(h->num_cu * 8)), dim3(256), 0, st, a);
        M2D_HIP_TRY(h, hipGetLastError());
    }
    h->last_kernel = "m2d_rank_count";
    return M2D_OK;
}
