// Retrieval under the 3-layer head (build-defined extension): full-catalogue top-k and the two-stage
// retrieve-then-rerank form.  The head arithmetic is m2d_launch_score_pairs_mlp's (m2d_mlp.hip), whichever kernel family the
// shape selects; this file is what stands around it: the pair generators, the selection kernel and the chunked launcher.
#include "m2d_engine.h"

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
// user has candidates of its own)
__global__ __launch_bounds__(256) void m2d_topk_mlp_pairs_cand(const int32_t *users, const int32_t *cand, int64_t rows, int64_t W,
                                                               int32_t *users_x, int32_t *items_x)
{
    const int64_t total = rows * W, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        users_x[t] = users[t / W];
        items_x[t] = cand[t];
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
__global__ __launch_bounds__(1024) void m2d_topk_mlp_select(const float *scores, const int32_t *ids, int64_t W, int32_t d0, int32_t k,
                                                            int32_t first, float *out_scores, int32_t *out_ids, int64_t rs, int64_t es,
                                                            int64_t ids_stride)
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
                ck[q] = tkm_key(s, idr ? idr[e] : d0 + (int32_t)e);
            }
        }
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

// threads of a selection block: a wave for the reranker's short rows, sixteen for a catalogue-wide range (few rows then share
// the device: a block of P / W rows)
int select_threads(const int64_t W) { return W <= 256 ? 64 : W <= 16384 ? 256 : 1024; }

}  // namespace

int m2d_launch_topk_select(m2d_engine *h, const float *scores, const int32_t *ids, int64_t ids_stride, int64_t rows, int64_t W, int32_t d0,
                           int32_t k, int32_t first, float *out_scores, int32_t *out_ids, int64_t rs, int64_t es, hipStream_t stream)
{
    const int threads = select_threads(W);
    const size_t lds = (size_t)(threads / 64 + 1) * k * (sizeof(uint64_t) + sizeof(uint32_t));
    M2D_HIP_TRY(h, m2d_lds_limit((const void *)m2d_topk_mlp_select, (int)lds));
    hipLaunchKernelGGL(m2d_topk_mlp_select, dim3((unsigned)rows), dim3(threads), lds, stream, scores, ids, W, d0, k, first, out_scores, out_ids,
                       rs, es, ids_stride);
    M2D_HIP_TRY(h, hipGetLastError());
    return M2D_OK;
}

int m2d_launch_topk_users_mlp(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates, float *out_scores,
                              int32_t *out_ids, hipStream_t stream)
{
    h->topk_mlp_launches = 0;
    if (nU == 0) return M2D_OK;
    const bool two = candidates > 0;
    const int64_t P = h->opt_topk_mlp_chunk_pairs;
    const int64_t W = two ? candidates : (h->I < P ? h->I : P);     // dish range (two-stage: the K1 candidates)
    const int64_t R0 = P / W > 1 ? P / W : 1, R = R0 < nU ? R0 : nU; // user rows of a block
    const size_t n = ((size_t)R * W + 3) & ~(size_t)3;              // pairs of a chunk (the id halves stay 16-byte aligned)
    int rc;
    if ((rc = m2d_grow(h, h->topk_mlp_ids, h->topk_mlp_ids_cap, 2 * n, sizeof(int32_t))) != M2D_OK) return rc;
    if ((rc = m2d_grow(h, h->topk_mlp_scores, h->topk_mlp_scores_cap, n, sizeof(float))) != M2D_OK) return rc;
    if (two && (rc = m2d_grow(h, h->topk_mlp_cand, h->topk_mlp_cand_cap, n, sizeof(int32_t))) != M2D_OK) return rc;
    int32_t *users_x = h->topk_mlp_ids, *items_x = users_x + n;
    float *scores = h->topk_mlp_scores;
    for (int64_t u0 = 0; u0 < nU; u0 += R) {
        const int64_t rows = nU - u0 < R ? nU - u0 : R;
        // stage 1, as m2d_topk_users runs it: the K1 best by the reference / ingredient score (its scores are not kept: the
        // head's land on them)
        if (two && (rc = m2d_launch_topk_users(h, users + u0, rows, candidates, scores, h->topk_mlp_cand, stream)) != M2D_OK) return rc;
        for (int64_t d0 = 0; d0 < (two ? W : h->I); d0 += W) {
            const int64_t Wc = two || h->I - d0 > W ? W : h->I - d0;
            const unsigned gb = m2d_blocks_for(h, rows * Wc, 1024);
            if (two)
                hipLaunchKernelGGL(m2d_topk_mlp_pairs_cand, dim3(gb), dim3(256), 0, stream, users + u0, h->topk_mlp_cand, rows, Wc, users_x, items_x);
            else
                hipLaunchKernelGGL(m2d_topk_mlp_pairs, dim3(gb), dim3(256), 0, stream, users + u0, rows, Wc, (int32_t)d0, users_x, items_x);
            M2D_HIP_TRY(h, hipGetLastError());
            if ((rc = m2d_launch_score_pairs_mlp(h, users_x, items_x, rows * Wc, scores, stream)) != M2D_OK) return rc;
            ++h->topk_mlp_launches;
            if ((rc = m2d_launch_topk_select(h, scores, two ? (const int32_t *)items_x : nullptr, Wc, rows, Wc, (int32_t)d0, k, d0 == 0 ? 1 : 0,
                                             out_scores + u0 * k, out_ids + u0 * k, two ? Wc : (int64_t)1, two ? (int64_t)1 : rows, stream)) != M2D_OK)
                return rc;
        }
    }
    return M2D_OK;
}
