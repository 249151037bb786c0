// Retrieval under the 3-layer head (build-defined extension): full-catalogue top-k and the two-stage
// retrieve-then-rerank form.  The head arithmetic is m2d_launch_score_pairs_mlp's (m2d_mlp.hip), whichever kernel family the
// shape selects; this file is what stands around it: the pair generators, the selection kernel and the chunked launcher.
// With exclusions: m2d_topk_mlp_select<true, false> strikes a row's excluded dishes from every step before its
// ballots, m2d_topk_mlp_count counts the dishes in front of a held-out one (m2d_catalogue_rank_mlp), m2d_launch_check_exclusions
// (m2d_catalogue_excl.hip) looks at the lists once per call.
#include "m2d_exclusions.h"   // (ExclCursor: a row's exclusion window)

namespace {

// ---- pair generators ----------------------------------------------------------------------------------------------------
// rows x W pairs, dish-major: pair c * rows + r is (users[r], d0 + c), so the `rows` pairs of a dish are neighbours -- a tile of
// the head kernel shares Dt rows, and a dish range's Dt rows are read once per user block.  (Measured against user-major, where a
// tile shares one Personal_Memory block: DESIGN.md section 8.5.)
__global__ __launch_bounds__(256) void m2d_topk_mlp_pairs(const int32_t *users, int64_t rows, int64_t W, int32_t d0,
                                                          int32_t *users_x, int32_t *items_x)
{
    const int64_t total = rows * W, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t c = t / rows;
        users_x[t] = users[t - c * rows];
        items_x[t] = d0 + (int32_t)c;
    }
}

// stage 2 of the two-stage form: pair r * W + j is (users[r], cand[r][j]), cand i32[rows, W] as stage 1 left it (user-major: every
// user has candidates of its own).  FILL: a slot stage 1 left empty (id -1: fewer than W dishes remained) becomes a pair on dish 0, so
// that the head launch stays in bounds; the selection reads the ids from `cand` and drops the slot whatever it scored.
template <bool FILL = false>
__global__ __launch_bounds__(256) void m2d_topk_mlp_pairs_cand(const int32_t *users, const int32_t *cand, int64_t rows, int64_t W,
                                                               int32_t *users_x, int32_t *items_x)
{
    const int64_t total = rows * W, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        users_x[t] = users[t / W];
        items_x[t] = FILL && cand[t] < 0 ? 0 : cand[t];
    }
}

// ---- selection ------------------------------------------------------------------------------------------------------------
// (the order's key -- TKM_NONE, tkm_key -- is m2d_engine.h's: m2d_market_requests.hip lists by it as well)
// One workgroup per user row: the row's W scores -- column e at scores[row * rs + e * es]: rs = 1, es = rows behind the dish-major
// generator, rs = W, es = 1 behind the candidate form; ids: ids[row * ids_stride + e] (ids_stride = W: a row of ids per user, 0: one row
// shared by all, the slate of m2d_topk_slate), or d0 + e when null -- merged into the row's list of k
// (score, id) in out_scores / out_ids -- `first`: the list starts with this range, otherwise it takes part as k more candidates.
// Every wave keeps the k best of the 64-wide slices it reads as a sorted list ACROSS its lanes (lane j: the j-th best, k <= 64
// is why one wave holds a whole list): a slice is compared with lane k - 1's key in one ballot, and the few candidates that
// pass are inserted one by one -- a ballot for the position, a one-lane shift for the tail.  After the first slices about
// k ln(W / k) candidates pass per wave, the rest costs a load, a compare and a ballot per 64 scores.  The waves' lists and the
// running list meet in LDS ((waves + 1) k keys of 8 B and score words of 4 B), where every entry counts the entries in front of
// it and the first k write themselves out.  No atomics; the score written is the word that was read (a NaN's payload, a -0).
// EXCL (dish-major form only: ids == null): row r leaves out xids[xoff[r] .. xoff[r + 1]), ascending dish ids, the array's length at
// *xend -- struck by ExclCursor::strike between a step's loads and its ballots.  HOLES (candidate form behind the exclusion
// retrieval): an id below 0 in `ids` is no entry (TKM_NONE), whatever its score.  <false, false> is the kernel as it stood.
template <bool EXCL, bool HOLES>
__global__ __launch_bounds__(1024) void m2d_topk_mlp_select(const float *scores, const int32_t *ids, int64_t W, int32_t d0, int32_t k,
                                                            int32_t first, float *out_scores, int32_t *out_ids, int64_t rs, int64_t es,
                                                            int64_t ids_stride, const int64_t *xoff, const int32_t *xids,
                                                            const int64_t *xend)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int nw = blockDim.x >> 6, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x;
    const float *sc = scores + row * rs;
    const int32_t *idr = ids ? ids + row * ids_stride : nullptr;
    uint64_t *mk = reinterpret_cast<uint64_t *>(smem);                          // [(nw + 1) k]
    uint32_t *ms = reinterpret_cast<uint32_t *>(mk + (size_t)(nw + 1) * k);     // [(nw + 1) k]

    uint64_t lk = TKM_NONE, thr = TKM_NONE;      // this lane's list entry; lane k - 1's: what a candidate has to beat
    uint32_t ls = 0x7FC00000u;
    ExclCursor xc;
    if (EXCL) xc.open(xoff, xids, xend, row);    // (a bad segment is the call's check to report)
    for (int64_t base = (int64_t)wave * 256; base < W; base += (int64_t)nw * 256) {
        uint64_t ck[4];
        uint32_t cs[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {            // four slices in flight
            const int64_t e = base + q * 64 + lane;
            ck[q] = TKM_NONE;
            cs[q] = 0u;
            if (e < W) {
                const float s = sc[e * es];
                cs[q] = __float_as_uint(s);
                const int32_t id = idr ? idr[e] : d0 + (int32_t)e;
                ck[q] = tkm_key(s, id);
                if (HOLES) ck[q] |= (uint64_t)(int64_t)(id >> 31);          // an id below 0: all ones, TKM_NONE (no branch)
            }
        }
        if (EXCL) xc.strike(xids, (int64_t)d0 + base, lane, ck, TKM_NONE);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned long long m = __ballot(ck[q] < thr);
            while (m) {                          // wave-uniform: m, c and thr are the same in every lane
                const int src = __ffsll(m) - 1;
                m &= m - 1;
                const uint64_t c = __shfl(ck[q], src, 64);
                if (c >= thr) continue;          // the list moved on since the ballot
                const uint32_t cb = __shfl(cs[q], src, 64);
                const int pos = __popcll(__ballot(lk < c));                    // sorted: the lanes in front of c
                const uint64_t upk = __shfl_up(lk, 1, 64);
                const uint32_t ups = __shfl_up(ls, 1, 64);
                if (lane == pos) { lk = c; ls = cb; }
                else if (lane > pos) { lk = upk; ls = ups; }
                thr = __shfl(lk, k - 1, 64);
            }
        }
    }
    if (lane < k) {
        mk[wave * k + lane] = lk;
        ms[wave * k + lane] = ls;
    }
    if (!first && (int)threadIdx.x < k) {
        const float s = out_scores[row * k + threadIdx.x];
        mk[nw * k + threadIdx.x] = tkm_key(s, out_ids[row * k + threadIdx.x]);
        ms[nw * k + threadIdx.x] = __float_as_uint(s);
    }
    __syncthreads();                             // the running list has been read: from here on it is written
    const int M = (nw + (first ? 0 : 1)) * k;
    for (int i = threadIdx.x; i < M; i += blockDim.x) {
        const uint64_t ki = mk[i];
        int rank = 0;
        for (int j = 0; j < M; ++j) {            // every lane reads the same word: a broadcast
            const uint64_t kj = mk[j];
            rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
        }
        if (rank < k) {
            out_scores[row * k + rank] = __uint_as_float(ki == TKM_NONE ? 0x7FC00000u : ms[i]);
            out_ids[row * k + rank] = ki == TKM_NONE ? -1 : (int32_t)(uint32_t)(ki & 0xFFFFFFFFu);
        }
    }
}

// ---- the rank of a held-out dish ---------------------------------------------------------------------------------------------
// One workgroup per query row (user, held-out dish p): the row's W scores in the dish-major layout (column e at scores[row + e *
// rows], dish d0 + e), read in the selection's steps.  A lane counts the dishes whose key is in front of p's -- held[row] is p's
// score word, from the same launcher --, p itself and the row's excluded dishes (ExclCursor) left out; one full-wave reduction, the
// waves' sums meet in LDS, and thread 0 stores the count (`first`: the first dish range) or adds it to out_rank[row].  No atomics:
// a row has one block per range and the ranges are stream-ordered.
__global__ __launch_bounds__(1024) void m2d_topk_mlp_count(const float *scores, int64_t rows, int64_t W, int32_t d0, int32_t first,
                                                           const int32_t *items, const float *held, int32_t *out_rank,
                                                           const int64_t *xoff, const int32_t *xids, const int64_t *xend)
{
    __shared__ int32_t wsum[16];
    const int nw = blockDim.x >> 6, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x;
    const float *sc = scores + row;
    const int32_t p = items[row];
    const uint64_t pk = tkm_key(held[row], p);
    ExclCursor xc;
    xc.open(xoff, xids, xend, row);
    int32_t cnt = 0;
    for (int64_t base = (int64_t)wave * 256; base < W; base += (int64_t)nw * 256) {
        uint64_t ck[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {            // four slices in flight
            const int64_t e = base + q * 64 + lane;
            ck[q] = TKM_NONE;
            if (e < W) ck[q] = tkm_key(sc[e * rows], d0 + (int32_t)e);
        }
        if (xoff) xc.strike(xids, (int64_t)d0 + base, lane, ck, TKM_NONE);   // scalar: a kernel argument
#pragma unroll
        for (int q = 0; q < 4; ++q) cnt += (ck[q] < pk && (uint32_t)ck[q] != (uint32_t)p) ? 1 : 0;   // (TKM_NONE is in front of no key)
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) wsum[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t total = first ? 0 : out_rank[row];
        for (int w = 0; w < nw; ++w) total += wsum[w];
        out_rank[row] = total;
    }
}

}  // namespace

int m2d_launch_topk_select(m2d_engine *h, const float *scores, const int32_t *ids, int64_t ids_stride, int64_t rows, int64_t W, int32_t d0,
                           int32_t k, int32_t first, float *out_scores, int32_t *out_ids, int64_t rs, int64_t es, hipStream_t stream,
                           const int64_t *xoff, const int32_t *xids, const int64_t *xend, bool holes)
{
    const int threads = select_threads(W);
    const size_t lds = (size_t)(threads / 64 + 1) * k * (sizeof(uint64_t) + sizeof(uint32_t));
    const auto launch = [&](auto kernel) -> int {
        M2D_HIP_TRY(h, m2d_lds_limit((const void *)kernel, (int)lds));
        hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(threads), lds, stream, scores, ids, W, d0, k, first, out_scores, out_ids, rs, es,
                           ids_stride, xoff, xids, xend);
        M2D_HIP_TRY(h, hipGetLastError());
        return M2D_OK;
    };
    return xoff ? launch(m2d_topk_mlp_select<true, false>) : holes ? launch(m2d_topk_mlp_select<false, true>) : launch(m2d_topk_mlp_select<false, false>);
}

namespace {

// the chunk geometry of both calls: dish ranges of W dishes, blocks of R rows, n pairs of scratch a chunk
struct ChunkShape {
    int64_t W, R;
    size_t n;
};

ChunkShape chunk_shape(const m2d_engine *h, const int64_t rows, const int64_t width)
{
    const int64_t P = h->opt_topk_mlp_chunk_pairs;
    ChunkShape c;
    c.W = width < P ? width : P;
    const int64_t R0 = P / c.W > 1 ? P / c.W : 1;
    c.R = R0 < rows ? R0 : rows;
    c.n = ((size_t)c.R * c.W + 3) & ~(size_t)3;                     // (the id halves stay 16-byte aligned)
    return c;
}

}  // namespace

int m2d_launch_topk_users_mlp(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates, float *out_scores,
                              int32_t *out_ids, hipStream_t stream, const int64_t *excl_off, const int32_t *excl_ids)
{
    h->topk_mlp_launches = 0;
    if (nU == 0) return M2D_OK;
    const bool two = candidates > 0;
    const ChunkShape cs = chunk_shape(h, nU, two ? candidates : h->I);   // dish range (two-stage: the K1 candidates), user rows of a block
    const int64_t W = cs.W, R = cs.R;
    const size_t n = cs.n;                                          // pairs of a chunk
    int rc;
    if ((rc = m2d_grow(h, h->topk_mlp_ids, h->topk_mlp_ids_cap, 2 * n, sizeof(int32_t))) != M2D_OK) return rc;
    if ((rc = m2d_grow(h, h->topk_mlp_scores, h->topk_mlp_scores_cap, n, sizeof(float))) != M2D_OK) return rc;
    // two-stage with exclusions: stage 1 runs once for the whole call (its offsets are the call's), ids [nU, K1] | scores [nU, K1]
    const bool two_x = two && excl_off;
    const size_t ncand = two_x ? 2 * (size_t)nU * candidates : n;
    if (two && (rc = m2d_grow(h, h->topk_mlp_cand, h->topk_mlp_cand_cap, ncand, sizeof(int32_t))) != M2D_OK) return rc;
    int32_t *users_x = h->topk_mlp_ids, *items_x = users_x + n;
    float *scores = h->topk_mlp_scores;
    if (two_x) {      // the K1 best by the reference score among the dishes left, -1 where fewer are (its checks are the lists' checks)
        if ((rc = m2d_launch_topk_users_excluding(h, users, nU, candidates, excl_off, excl_ids,
                                                  reinterpret_cast<float *>(h->topk_mlp_cand + (size_t)nU * candidates), h->topk_mlp_cand, stream,
                                                  "m2d_topk_users_mlp_excluding", /*under_head=*/true)) != M2D_OK)
            return rc;
    } else if (excl_off && (rc = m2d_launch_check_exclusions(h, excl_off, excl_ids, nU, stream)) != M2D_OK)
        return rc;
    for (int64_t u0 = 0; u0 < nU; u0 += R) {
        const int64_t rows = nU - u0 < R ? nU - u0 : R;
        // stage 1, as m2d_topk_users runs it: the K1 best by the reference / ingredient score (its scores are not kept: the
        // head's land on them)
        if (two && !two_x && (rc = m2d_launch_topk_users(h, users + u0, rows, candidates, scores, h->topk_mlp_cand, stream)) != M2D_OK) return rc;
        const int32_t *cand = two_x ? h->topk_mlp_cand + u0 * candidates : h->topk_mlp_cand;
        for (int64_t d0 = 0; d0 < (two ? W : h->I); d0 += W) {
            const int64_t Wc = two || h->I - d0 > W ? W : h->I - d0;
            const unsigned gb = m2d_blocks_for(h, rows * Wc, 1024);
            if (two_x)
                hipLaunchKernelGGL(m2d_topk_mlp_pairs_cand<true>, dim3(gb), dim3(256), 0, stream, users + u0, cand, rows, Wc, users_x, items_x);
            else if (two)
                hipLaunchKernelGGL(m2d_topk_mlp_pairs_cand<>, dim3(gb), dim3(256), 0, stream, users + u0, cand, rows, Wc, users_x, items_x);
            else
                hipLaunchKernelGGL(m2d_topk_mlp_pairs, dim3(gb), dim3(256), 0, stream, users + u0, rows, Wc, (int32_t)d0, users_x, items_x);
            M2D_HIP_TRY(h, hipGetLastError());
            if ((rc = m2d_launch_score_pairs_mlp(h, users_x, items_x, rows * Wc, scores, stream)) != M2D_OK) return rc;
            ++h->topk_mlp_launches;
            const int32_t *ids = two_x ? cand : two ? (const int32_t *)items_x : nullptr;
            const bool strike = excl_off && !two;
            if ((rc = m2d_launch_topk_select(h, scores, ids, Wc, rows, Wc, (int32_t)d0, k, d0 == 0 ? 1 : 0, out_scores + u0 * k, out_ids + u0 * k,
                                             two ? Wc : (int64_t)1, two ? (int64_t)1 : rows, stream, strike ? excl_off + u0 : nullptr, excl_ids,
                                             strike ? excl_off + nU : nullptr, two_x)) != M2D_OK)
                return rc;
        }
    }
    return M2D_OK;
}

// m2d_topk_users_mlp_deep: the loop above with m2d_select_deep for every k up to 1024.  Exact form: the same
// chunk geometry, dish-major, a row's excluded dishes struck inside the selection.  Two-stage form: blocks of max(1, P / K1) users;
// per block stage 1 is m2d_launch_deep_lists' K1 dishes (exclusions already left out; its conditions and the lists' check are
// looked at once, in front of the loop), then the candidate generator, the head and the selection with HOLES.
int m2d_launch_topk_users_mlp_deep(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates, const int64_t *excl_off,
                                   const int32_t *excl_ids, float *out_scores, int32_t *out_ids, hipStream_t stream)
{
    h->topk_mlp_launches = 0;
    if (nU == 0) return M2D_OK;
    const bool two = candidates > 0;
    ChunkShape cs = chunk_shape(h, nU, h->I);
    if (two) {                                                      // (K1 may exceed the smallest P: a block is whole candidate rows)
        const int64_t R0 = h->opt_topk_mlp_chunk_pairs / candidates > 1 ? h->opt_topk_mlp_chunk_pairs / candidates : 1;
        cs.W = candidates;
        cs.R = R0 < nU ? R0 : nU;
        cs.n = ((size_t)cs.R * cs.W + 3) & ~(size_t)3;
    }
    const int64_t W = cs.W, R = cs.R;
    const size_t n = cs.n;
    int rc;
    if (two && (rc = m2d_deep_conditions(h, "m2d_topk_users_mlp_deep", stream)) != M2D_OK) return rc;
    if ((rc = m2d_grow(h, h->topk_mlp_ids, h->topk_mlp_ids_cap, 2 * n, sizeof(int32_t))) != M2D_OK) return rc;
    if ((rc = m2d_grow(h, h->topk_mlp_scores, h->topk_mlp_scores_cap, n, sizeof(float))) != M2D_OK) return rc;
    if (two && (rc = m2d_grow(h, h->topk_mlp_cand, h->topk_mlp_cand_cap, n, sizeof(int32_t))) != M2D_OK) return rc;
    int32_t *users_x = h->topk_mlp_ids, *items_x = users_x + n;
    float *scores = h->topk_mlp_scores;
    if (excl_off && (rc = m2d_launch_check_exclusions(h, excl_off, excl_ids, nU, stream)) != M2D_OK) return rc;
    const int64_t *xend = excl_off ? excl_off + nU : nullptr;
    for (int64_t u0 = 0; u0 < nU; u0 += R) {
        const int64_t rows = nU - u0 < R ? nU - u0 : R;
        const int64_t *xoff = excl_off ? excl_off + u0 : nullptr;
        if (two) {
            if ((rc = m2d_launch_deep_lists(h, users + u0, rows, candidates, xoff, excl_ids, xend, u0, scores, h->topk_mlp_cand, stream)) != M2D_OK)
                return rc;
            hipLaunchKernelGGL(m2d_topk_mlp_pairs_cand<true>, dim3(m2d_blocks_for(h, rows * W, 1024)), dim3(256), 0, stream, users + u0,
                               h->topk_mlp_cand, rows, W, users_x, items_x);
            M2D_HIP_TRY(h, hipGetLastError());
            if ((rc = m2d_launch_score_pairs_mlp(h, users_x, items_x, rows * W, scores, stream)) != M2D_OK) return rc;
            ++h->topk_mlp_launches;
            if ((rc = m2d_launch_select_deep(h, scores, h->topk_mlp_cand, W, rows, W, 0, k, 1, out_scores + u0 * k, out_ids + u0 * k, W, 1, stream,
                                             nullptr, nullptr, nullptr, true)) != M2D_OK)
                return rc;
            continue;
        }
        for (int64_t d0 = 0; d0 < h->I; d0 += W) {
            const int64_t Wc = h->I - d0 > W ? W : h->I - d0;
            hipLaunchKernelGGL(m2d_topk_mlp_pairs, dim3(m2d_blocks_for(h, rows * Wc, 1024)), dim3(256), 0, stream, users + u0, rows, Wc, (int32_t)d0,
                               users_x, items_x);
            M2D_HIP_TRY(h, hipGetLastError());
            if ((rc = m2d_launch_score_pairs_mlp(h, users_x, items_x, rows * Wc, scores, stream)) != M2D_OK) return rc;
            ++h->topk_mlp_launches;
            if ((rc = m2d_launch_select_deep(h, scores, nullptr, 0, rows, Wc, (int32_t)d0, k, d0 == 0 ? 1 : 0, out_scores + u0 * k, out_ids + u0 * k, 1,
                                             rows, stream, xoff, excl_ids, xend)) != M2D_OK)
                return rc;
        }
    }
    return M2D_OK;
}

int m2d_launch_catalogue_rank_mlp(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t n, const int64_t *excl_off,
                                  const int32_t *excl_ids, int32_t *out_rank, float *out_scores, hipStream_t stream)
{
    h->topk_mlp_launches = 0;
    if (n == 0) return M2D_OK;
    const ChunkShape cs = chunk_shape(h, n, h->I);
    const int64_t W = cs.W, R = cs.R;
    int rc;
    if ((rc = m2d_grow(h, h->topk_mlp_ids, h->topk_mlp_ids_cap, 2 * cs.n, sizeof(int32_t))) != M2D_OK) return rc;
    if ((rc = m2d_grow(h, h->topk_mlp_scores, h->topk_mlp_scores_cap, cs.n, sizeof(float))) != M2D_OK) return rc;
    if (!out_scores && (rc = m2d_grow(h, h->topk_mlp_held, h->topk_mlp_held_cap, (size_t)n, sizeof(float))) != M2D_OK) return rc;
    int32_t *users_x = h->topk_mlp_ids, *items_x = users_x + cs.n;
    float *scores = h->topk_mlp_scores, *held = out_scores ? out_scores : h->topk_mlp_held;
    // the held-out pairs' words (and the call's id checks: a bad user or held-out id is latched at its query)
    if ((rc = m2d_launch_score_pairs_mlp(h, users, items, n, held, stream)) != M2D_OK) return rc;
    ++h->topk_mlp_launches;
    if (excl_off && (rc = m2d_launch_check_exclusions(h, excl_off, excl_ids, n, stream)) != M2D_OK) return rc;
    for (int64_t q0 = 0; q0 < n; q0 += R) {
        const int64_t rows = n - q0 < R ? n - q0 : R;
        for (int64_t d0 = 0; d0 < h->I; d0 += W) {
            const int64_t Wc = h->I - d0 > W ? W : h->I - d0;
            hipLaunchKernelGGL(m2d_topk_mlp_pairs, dim3(m2d_blocks_for(h, rows * Wc, 1024)), dim3(256), 0, stream, users + q0, rows, Wc, (int32_t)d0,
                               users_x, items_x);
            M2D_HIP_TRY(h, hipGetLastError());
            if ((rc = m2d_launch_score_pairs_mlp(h, users_x, items_x, rows * Wc, scores, stream)) != M2D_OK) return rc;
            ++h->topk_mlp_launches;
            hipLaunchKernelGGL(m2d_topk_mlp_count, dim3((unsigned)rows), dim3(select_threads(Wc)), 0, stream, scores, rows, Wc, (int32_t)d0,
                               d0 == 0 ? 1 : 0, items + q0, held + q0, out_rank + q0, excl_off ? excl_off + q0 : nullptr, excl_ids,
                               excl_off ? excl_off + n : nullptr);
            M2D_HIP_TRY(h, hipGetLastError());
        }
    }
    return M2D_OK;
}
