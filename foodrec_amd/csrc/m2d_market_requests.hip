// Build-defined extension (no reference counterpart): m2d_topk_markets, one (user, market) per request --
// the cookable-dish filter of m2d_market.hip, the literal pair score and the list of k, in one launch per batch.
//
//   request q  = (users[q], market_ids[market_off[q] .. market_off[q + 1]))
//   cookable   = m2d_cookable_dishes' definition: a non-empty list with at most max_missing ENTRIES absent from the market
//   row q      = the first min(k, count_q) cookable dishes in m2d_topk_users' order (tkm_key), NaN / -1 from count_q on
//
// m2d_markets_topk<LDS>: a block of MQ_WAVES waves serves one (request, share); a share is a contiguous range of MQ_DB-dish blocks of
// the catalogue.  The block builds its market's bitmap (LDS up to MQ_LDS_BITS bits; beyond, m2d_markets_bitmap has written one bitmap per
// request into scratch and the block reads its own through L2), its waves walk the share's 64-dish groups as m2d_market_flag does,
// score every kept dish with m2d_pair_score_wave -- the whole wave on one dish -- and keep the k best as a sorted list across lanes,
// the insertion of m2d_topk_mlp_select.  The four lists meet in LDS; with one share the block writes the row, with S > 1 it writes k
// (score, id) words into scratch [nQ, S k] and m2d_topk_mlp_select merges the shares.  The order is strict and tkm_key(NaN, -1) is
// TKM_NONE, so the words do not depend on S.  Nothing synchronises: no block waits for another, the stream orders the launches.
// The setter has validated the recipe lists (m2d_set_recipes), so no kernel here range-checks a recipe id or a recipe offset; the
// call's own inputs -- market ids, user ids, market offsets -- are checked where they are read.
//
// m2d_topk_markets_excluding is the same call with two additions.  m2d_markets_topk<LDS, true> takes an ascending
// CSR of dish ids per request and drops them from the `kept` ballot of each 64-dish group before anything is scored or counted; the
// instantiations without it are the code above, unchanged.  m2d_markets_missing<LDS> runs after the rows are final and writes, for every
// listed dish, the ids of its list entries that are absent from the request's market, in list order.
#include "m2d_exclusions.h"   // (csr_segment: a request's market; ExclCursor: its excluded dishes)

namespace {

constexpr int MQ_DW = 64;                      // dishes per group (one per lane)
constexpr int MQ_WAVES = 4;                    // waves per block
constexpr int MQ_DB = MQ_DW * MQ_WAVES;        // dishes per catalogue block: what a share is counted in
constexpr int MQ_EB = 64;                      // entries per batch (one per lane)
constexpr int MQ_BF = 4;                       // batches loaded before the first of them is tested
constexpr int MQ_LDS_BITS = 1 << 16;           // the bitmap lives in LDS up to this many bits (8 KiB a block)
constexpr int MQ_KMAX = 64;                    // k <= 64: one wave holds a whole list
constexpr int MQ_MAX_SHARES = 64;

struct MarketsArgs {
    const float *pm, *re, *ce, *cats;
    const int32_t *rcp_off, *rcp_ids;
    const int32_t *users;
    const int64_t *moff;
    const int32_t *mids;
    const uint32_t *bitmaps;   // through-L2 form: [nQ, ceil(R / 32)]
    int64_t nnzM, U, I, user_base;
    int32_t C, E, R, k, max_missing, S;
    float a, b;
    int32_t skip_masked;
    const int32_t *nonfinite;
    float *out_scores;         // [nQ, k]
    int32_t *out_ids;
    int32_t *counts;           // [nQ] or null
    uint32_t *part_scores;     // S > 1: [nQ, S k] score words
    int32_t *part_ids;
    int32_t *err;
    // exclusion form (m2d_markets_topk<LDS, true>): request q leaves out xids[xoff[q] .. xoff[q + 1]), ascending dish ids
    const int64_t *xoff;
    const int32_t *xids;
    int64_t nQ;
};

// Wave-uniform values are carried in SGPRs: every loop with a ballot or a shuffle in it is scalar control flow, no cross-lane
// operation executes under a partial EXEC mask.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// through-L2 form: block q sets request q's bits in its own bitmap (zeroed by a memset in front)
__global__ __launch_bounds__(256) void m2d_markets_bitmap(const int64_t *moff, const int32_t *mids, int64_t nnzM, int32_t R, int64_t words,
                                                          uint32_t *bitmaps, int32_t *err)
{
    const int64_t q = blockIdx.x;
    int64_t m0, m1;
    bool bad;
    csr_segment(moff, q, nnzM, m0, m1, bad);
    uint32_t *bm = bitmaps + q * words;
    for (int64_t i = m0 + threadIdx.x; i < m1; i += 256) {
        const int32_t id = mids[i];
        if (id < 0 || id >= R) m2d_latch_error(err, M2D_ERR_BAD_INGREDIENT, id, i);
        else atomicOr(&bm[id >> 5], 1u << (id & 31));
    }
}

template <bool LDS, bool EXCL = false>
__global__ __launch_bounds__(256) void m2d_markets_topk(MarketsArgs p)
{
    __shared__ uint32_t bm[LDS ? MQ_LDS_BITS / 32 : 1];
    __shared__ uint64_t mk[MQ_WAVES * MQ_KMAX];
    __shared__ uint32_t ms[MQ_WAVES * MQ_KMAX];
    __shared__ int32_t wave_kept[MQ_WAVES];
    const int wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int k = p.k, C = p.C, E = p.E, S = p.S;
    const int64_t q = blockIdx.x / S;
    const int s = (int)(blockIdx.x - q * S);

    int64_t m0, m1;
    bool bad_seg;
    csr_segment(p.moff, q, p.nnzM, m0, m1, bad_seg);
    const int32_t uid = p.users[q];
    const int64_t ul = (int64_t)uid - p.user_base;
    const bool bad_user = ul < 0 || ul >= p.U;               // block-uniform: nothing is read for that user
    if (threadIdx.x == 0 && s == 0) {
        if (bad_seg) m2d_latch_error(p.err, M2D_ERR_INVALID_ARG, (int32_t)p.moff[q + 1], q);
        if (bad_user) m2d_latch_error(p.err, M2D_ERR_BAD_USER_ID, uid, q);
    }
    const int words = (p.R + 31) >> 5;
    if (LDS) {                                               // words <= MQ_LDS_BITS / 32: the launcher picks this form by R
        for (int i = threadIdx.x; i < words; i += MQ_WAVES * 64) bm[i] = 0u;
        __syncthreads();
        for (int64_t i = m0 + threadIdx.x; i < m1; i += MQ_WAVES * 64) {
            const int32_t id = p.mids[i];
            if (id < 0 || id >= p.R) {
                if (s == 0) m2d_latch_error(p.err, M2D_ERR_BAD_INGREDIENT, id, i);
            } else atomicOr(&bm[id >> 5], 1u << (id & 31));
        }
        __syncthreads();
    }
    const uint32_t *bits = LDS ? bm : p.bitmaps + q * (int64_t)words;

    // exclusion form: the request's segment, clamped into the array (its length is the last offset, as m2d_catalogue_rank takes it)
    // before anything is read; the share-0 block checks every id once -- a dish of the catalogue, not below the id in front of it
    // (these latch values are this call's own, not csr_check_offset's); the cursor then walks the window group by group
    ExclCursor xc;
    if (EXCL) {
        const bool bad_x = xc.open(p.xoff, p.xids, p.xids ? p.xoff[p.nQ] : 0, q);     // (no array: its length is 0, a non-empty segment is bad)
        const int64_t x0 = xc.xw, x1 = xc.x1;
        if (s == 0) {
            if (threadIdx.x == 0 && bad_x) m2d_latch_error(p.err, M2D_ERR_INVALID_ARG, (int32_t)p.xoff[q + 1], q + 1);
            for (int64_t i = x0 + threadIdx.x; i < x1; i += MQ_WAVES * 64) {
                const int32_t x = p.xids[i];
                if (x < 0 || x >= p.I) m2d_latch_error(p.err, M2D_ERR_BAD_ITEM_ID, x, i);
                else if (i > x0 && p.xids[i - 1] > x) m2d_latch_error(p.err, M2D_ERR_INVALID_ARG, x, i);
            }
        }
    }

    // the share: catalogue blocks [s nb / S, (s + 1) nb / S), S <= nb
    const int64_t nb = (p.I + MQ_DB - 1) / MQ_DB;
    const int64_t b0 = (int64_t)s * nb / S, b1 = (int64_t)(s + 1) * nb / S;
    const int64_t groups = (b1 - b0) * MQ_WAVES;
    const float *um = p.pm + (size_t)(bad_user ? 0 : ul) * (size_t)(C + 1) * E;
    const bool skipm = p.skip_masked != 0 && uni(*p.nonfinite) == 0;        // as skip_rows() decides it (m2d_score.hip)

    uint64_t lk = TKM_NONE, thr = TKM_NONE;      // this lane's list entry; lane k - 1's: what a candidate has to beat
    uint32_t ls = 0x7FC00000u;
    int cnt = 0;                                  // kept dishes of this wave (wave-uniform)
    for (int64_t g = wave; g < groups; g += MQ_WAVES) {                     // scalar bounds
        const int64_t d0 = b0 * MQ_DB + g * MQ_DW;
        const int64_t left = p.I - d0;
        const int dn = uni((int)(left < 0 ? 0 : left < MQ_DW ? left : MQ_DW));
        int my_begin = 0, my_end = 0;                                       // this lane's dish: entries [my_begin, my_end)
        if (lane < dn) {
            my_begin = p.rcp_off[d0 + lane];
            my_end = p.rcp_off[d0 + lane + 1];
        }
        // (entry positions are below 2^31 -- m2d_set_recipes -- so they and a step past the end fit 32 unsigned bits)
        const uint32_t e_begin = dn > 0 ? __builtin_amdgcn_readlane(my_begin, 0) : 0;
        const uint32_t e_end = dn > 0 ? __builtin_amdgcn_readlane(my_end, dn - 1) : 0;
        int miss = 0;
        for (uint32_t pos = e_begin; pos < e_end; pos += MQ_BF * MQ_EB) {   // scalar bounds
            int32_t id[MQ_BF];
#pragma unroll
            for (int f = 0; f < MQ_BF; ++f) {                               // MQ_BF batches in flight: the walk waits for memory, not for ALUs
                const uint32_t e = pos + f * MQ_EB + lane;
                id[f] = e < e_end ? p.rcp_ids[e] : -1;                      // (recipe ids are >= 0: the setter has checked them)
            }
#pragma unroll
            for (int f = 0; f < MQ_BF; ++f) {
                const int64_t at = pos + (uint32_t)(f * MQ_EB);
                const int32_t v = id[f] < 0 ? 0 : id[f];                    // the bitmap read is in bounds for a lane without an entry too
                const bool absent = id[f] >= 0 && ((bits[v >> 5] >> (v & 31)) & 1u) == 0;
                const unsigned long long word = __ballot(absent);           // bit j: entry at + j is not in the market
                const int64_t lo = my_begin > at ? my_begin - at : 0, hi = my_end - at < MQ_EB ? my_end - at : MQ_EB;
                if (hi > lo) {
                    const unsigned long long run = hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1;
                    miss += __popcll(word & (run << lo));
                }
            }
        }
        unsigned long long kept = __ballot(lane < dn && my_end != my_begin && miss <= p.max_missing);
        if (EXCL) {                                                         // the segment's window for [d0, d0 + 64): an empty one costs a compare
            bool in[1] = {true};
            xc.strike(p.xids, d0, lane, in, false);
            kept &= __ballot(in[0]);
        }
        cnt += __popcll(kept);
        if (bad_user) continue;
        while (kept) {                                                      // wave-uniform: one dish, the whole wave
            const int j = __ffsll(kept) - 1;
            kept &= kept - 1;
            const int64_t d = d0 + j;
            // every lane holds the same score (the butterflies are symmetric); lane 0's word makes the branch below a scalar one
            const float sc = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(
                m2d_pair_score_wave(um, p.re + (size_t)d * E, p.cats + (size_t)d * C, p.ce, nullptr, C, E, p.a, p.b, skipm, lane))));
            const uint64_t c = tkm_key(sc, (int32_t)d);
            if (c >= thr) continue;
            const int at = __popcll(__ballot(lk < c));                      // sorted: the lanes in front of c
            const uint64_t upk = __shfl_up(lk, 1, 64);
            const uint32_t ups = __shfl_up(ls, 1, 64);
            if (lane == at) { lk = c; ls = __float_as_uint(sc); }
            else if (lane > at) { lk = upk; ls = ups; }
            thr = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(lk >> 32), k - 1) << 32) |
                  (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)lk, k - 1);
        }
    }
    if (lane < k) {
        mk[wave * k + lane] = lk;
        ms[wave * k + lane] = ls;
    }
    if (lane == 0) wave_kept[wave] = cnt;
    __syncthreads();
    // every entry counts the entries in front of it; the first k write themselves out (MQ_WAVES k <= 256 entries: one per thread)
    const int M = MQ_WAVES * k;
    const int64_t row = S == 1 ? q * k : ((int64_t)q * S + s) * k;
    if ((int)threadIdx.x < M) {
        const int i = threadIdx.x;
        const uint64_t ki = mk[i];
        int rank = 0;
        for (int j = 0; j < M; ++j) {
            const uint64_t kj = mk[j];
            rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
        }
        if (rank < k) {
            const uint32_t w = ki == TKM_NONE ? 0x7FC00000u : ms[i];
            const int32_t id = ki == TKM_NONE ? -1 : (int32_t)(uint32_t)(ki & 0xFFFFFFFFu);
            if (S == 1) {
                p.out_scores[row + rank] = __uint_as_float(w);
                p.out_ids[row + rank] = id;
            } else {
                p.part_scores[row + rank] = w;
                p.part_ids[row + rank] = id;
            }
        }
    }
    if (threadIdx.x == 0 && p.counts) {
        int32_t n = 0;
        for (int w = 0; w < MQ_WAVES; ++w) n += wave_kept[w];
        if (S == 1) p.counts[q] = n;
        else if (n) atomicAdd(&p.counts[q], n);                             // zeroed in front: an integer sum, any order
    }
}

// m2d_markets_missing<LDS>: block q, after row q is final.  It has the request's bitmap as m2d_markets_topk has it (rebuilt in LDS, or the
// one m2d_markets_bitmap left in scratch, still valid in stream order); wave w takes the listed dishes j = w, w + MQ_WAVES, ... and walks
// the dish's list MQ_EB entries a batch.  An absent entry's place is the running total plus the absent entries below its lane in the
// batch's ballot, so the words come out in list order without an atomic or a sort.  Every word of [nQ, k, max_missing] is written.
template <bool LDS>
__global__ __launch_bounds__(256) void m2d_markets_missing(MarketsArgs p, int32_t *out_missing)
{
    __shared__ uint32_t bm[LDS ? MQ_LDS_BITS / 32 : 1];
    const int wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t q = blockIdx.x;
    const int k = p.k, mm = p.max_missing;
    const int words = (p.R + 31) >> 5;
    if (LDS) {                                               // (the ids have been reported by m2d_markets_topk: a bad one is skipped)
        int64_t m0, m1;
        bool bad_seg;
        csr_segment(p.moff, q, p.nnzM, m0, m1, bad_seg);
        for (int i = threadIdx.x; i < words; i += MQ_WAVES * 64) bm[i] = 0u;
        __syncthreads();
        for (int64_t i = m0 + threadIdx.x; i < m1; i += MQ_WAVES * 64) {
            const int32_t id = p.mids[i];
            if (id >= 0 && id < p.R) atomicOr(&bm[id >> 5], 1u << (id & 31));
        }
        __syncthreads();
    }
    const uint32_t *bits = LDS ? bm : p.bitmaps + q * (int64_t)words;
    for (int j = wave; j < k; j += MQ_WAVES) {                               // scalar bounds
        const int32_t d = uni(p.out_ids[q * k + j]);
        int32_t *row = out_missing + (q * k + j) * (int64_t)mm;
        int total = 0;                                                       // absent entries so far (wave-uniform)
        if (d >= 0 && d < p.I) {
            const uint32_t e_begin = uni(p.rcp_off[d]), e_end = uni(p.rcp_off[d + 1]);
            for (uint32_t pos = e_begin; pos < e_end; pos += MQ_EB) {        // scalar bounds
                const uint32_t e = pos + lane;
                const int32_t id = e < e_end ? p.rcp_ids[e] : -1;
                const int32_t v = id < 0 ? 0 : id;
                const bool absent = id >= 0 && ((bits[v >> 5] >> (v & 31)) & 1u) == 0;
                const unsigned long long word = __ballot(absent);
                const int at = total + __popcll(word & ((1ull << lane) - 1));
                if (absent && at < mm) row[at] = id;                         // (more than max_missing only if the row is wrong: capped)
                total += __popcll(word);
            }
        }
        for (int i = (total < mm ? total : mm) + lane; i < mm; i += 64) row[i] = -1;
    }
}

}  // namespace

int m2d_launch_topk_markets(m2d_engine *h, const int32_t *users, int64_t nQ, const int64_t *market_off, const int32_t *market_ids,
                            int64_t nnzM, int32_t k, int32_t max_missing, float *out_scores, int32_t *out_ids, int32_t *out_counts,
                            hipStream_t st, const int64_t *excl_off, const int32_t *excl_ids, int32_t *out_missing)
{
    int rc;
    if ((rc = m2d_ensure_finite_scan(h, st)) != M2D_OK) return rc;
    const int64_t I = h->I, R = h->rcp_rows;
    const int64_t words = (R + 31) / 32, nb = (I + MQ_DB - 1) / MQ_DB;
    const bool lds = R <= MQ_LDS_BITS;
    // shares: a lone request is spread over the device, a thousand requests take one block each
    int64_t S = h->opt_market_shares > 0 ? h->opt_market_shares : 4 * (int64_t)h->num_cu / nQ;
    const int64_t smax = nb < MQ_MAX_SHARES ? nb : MQ_MAX_SHARES;
    S = S > smax ? smax : S;
    S = S < 1 ? 1 : S;
    h->market_shares_used = (int)S;
    if (nQ * S > 0x7FFFFFFF) {
        h->last_error = "m2d_topk_markets: nQ x shares exceeds the grid limit";
        return M2D_ERR_INVALID_ARG;
    }
    // partial ids | partial score words | bitmaps
    const int64_t part = S > 1 ? nQ * S * k : 0, o_bm = 2 * part;
    const int64_t need = o_bm + (lds ? 0 : nQ * words);
    if ((rc = h->markets_buf.grow(h, (size_t)(need > 1 ? need : 1))) != M2D_OK) return rc;

    MarketsArgs a;
    a.pm = h->pm; a.re = h->re; a.ce = h->ce; a.cats = h->dish_cats;
    a.rcp_off = h->rcp_off; a.rcp_ids = h->rcp_ids;
    a.users = users; a.moff = market_off; a.mids = market_ids;
    a.bitmaps = reinterpret_cast<const uint32_t *>(h->markets_buf + o_bm);
    a.nnzM = nnzM; a.U = h->U; a.I = I; a.user_base = h->user_base;
    a.C = h->C; a.E = h->E; a.R = (int32_t)R; a.k = k; a.max_missing = max_missing; a.S = (int32_t)S;
    a.a = h->a; a.b = h->b;
    a.skip_masked = h->opt_skip_masked; a.nonfinite = h->nonfinite_dev;
    a.out_scores = out_scores; a.out_ids = out_ids; a.counts = out_counts;
    a.part_ids = h->markets_buf; a.part_scores = reinterpret_cast<uint32_t *>(h->markets_buf + part);
    a.err = h->err_dev;
    a.xoff = excl_off; a.xids = excl_ids; a.nQ = nQ;

    if (S > 1 && out_counts) M2D_HIP_TRY(h, hipMemsetAsync(out_counts, 0, (size_t)nQ * sizeof(int32_t), st));
    if (!lds) {
        M2D_HIP_TRY(h, hipMemsetAsync(h->markets_buf + o_bm, 0, (size_t)(nQ * words) * sizeof(uint32_t), st));
        hipLaunchKernelGGL(m2d_markets_bitmap, dim3((unsigned)nQ), dim3(256), 0, st, market_off, market_ids, nnzM, (int32_t)R, words,
                           reinterpret_cast<uint32_t *>(h->markets_buf + o_bm), h->err_dev);
    }
    h->last_kernel = lds ? "m2d_markets_topk_lds" : "m2d_markets_topk_l2";
    if (excl_off) {
        h->last_kernel = lds ? "m2d_markets_topk_excl_lds" : "m2d_markets_topk_excl_l2";
        if (lds) hipLaunchKernelGGL((m2d_markets_topk<true, true>), dim3((unsigned)(nQ * S)), dim3(MQ_WAVES * 64), 0, st, a);
        else hipLaunchKernelGGL((m2d_markets_topk<false, true>), dim3((unsigned)(nQ * S)), dim3(MQ_WAVES * 64), 0, st, a);
    } else if (lds) hipLaunchKernelGGL(m2d_markets_topk<true>, dim3((unsigned)(nQ * S)), dim3(MQ_WAVES * 64), 0, st, a);
    else hipLaunchKernelGGL(m2d_markets_topk<false>, dim3((unsigned)(nQ * S)), dim3(MQ_WAVES * 64), 0, st, a);
    M2D_HIP_TRY(h, hipGetLastError());
    if (S > 1) {                                             // the shares' partial lists, [nQ, S k] words and ids, become the rows
        SelectJob job = SelectJob::row_major(reinterpret_cast<const float *>(a.part_scores), nQ, S * k, a.part_ids, S * k);
        job.k = k; job.out_scores = out_scores; job.out_ids = out_ids;
        if ((rc = m2d_launch_select(h, job, /*deep=*/false, st)) != M2D_OK) return rc;
    }
    if (out_missing && max_missing > 0) {                    // the rows are final; the bitmaps in markets_buf have not moved (one growth, above)
        if (lds) hipLaunchKernelGGL(m2d_markets_missing<true>, dim3((unsigned)nQ), dim3(MQ_WAVES * 64), 0, st, a, out_missing);
        else hipLaunchKernelGGL(m2d_markets_missing<false>, dim3((unsigned)nQ), dim3(MQ_WAVES * 64), 0, st, a, out_missing);
        M2D_HIP_TRY(h, hipGetLastError());
    }
    return M2D_OK;
}
