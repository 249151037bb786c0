// Retrieval under the 3-layer head (build-defined extension): full-catalogue top-k and the two-stage
// retrieve-then-rerank form.  The head arithmetic is m2d_launch_score_pairs_mlp's (m2d_mlp.hip), whichever kernel family the
// shape selects; this file is what stands around it: the pair generators, the count kernel and the one chunked launcher of
// m2d_topk_users_mlp, its exclusion form and m2d_topk_users_mlp_deep.  The selection is m2d_launch_select's (m2d_select.hip), either
// kernel.  With exclusions: the selection strikes a row's excluded dishes from every step of its walk,
// m2d_topk_mlp_count counts the dishes in front of a held-out one (m2d_catalogue_rank_mlp) on the same walk, m2d_launch_check_exclusions
// (m2d_catalogue_excl.hip) looks at the lists once per call.
#include "m2d_select.h"   // (select_walk: a row of a SelectJob in the selection's steps)

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

// ---- the rank of a held-out dish ---------------------------------------------------------------------------------------------
// One workgroup per query row (user, held-out dish p): the row's W scores -- `job`: a dish-major range as the selection takes it, its
// k and outputs unused --, read in the selection's steps (select_walk).  A lane counts the dishes whose key is in front of p's --
// held[row] is p's score word, from the same launcher --, p itself and the row's excluded dishes left out (null offsets: none); one
// full-wave reduction, the waves' sums meet in LDS, and thread 0 stores the count (`first`: the first dish range) or adds it to
// out_rank[row].  No atomics: a row has one block per range and the ranges are stream-ordered.
__global__ __launch_bounds__(1024) void m2d_topk_mlp_count(SelectJob job, const int32_t *items, const float *held, int32_t *out_rank)
{
    job.ids = nullptr;                           // a dish range has no id table: the walk's branch on it folds away
    __shared__ int32_t wsum[16];
    const int nw = blockDim.x >> 6, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x;
    const int32_t p = items[row];
    const uint64_t pk = tkm_key(held[row], p);
    int32_t cnt = 0;
    select_walk<true, false>(job, row, wave, nw, lane, [&](const uint64_t key, uint32_t) {
        cnt += (key < pk && (uint32_t)key != (uint32_t)p) ? 1 : 0;   // (TKM_NONE is in front of no key)
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) wsum[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t total = job.first ? 0 : out_rank[row];
        for (int w = 0; w < nw; ++w) total += wsum[w];
        out_rank[row] = total;
    }
}

// ---- what the launchers share ---------------------------------------------------------------------------------------------------
// the chunk geometry: ranges of W columns, blocks of R rows, n pairs of scratch a chunk.  Exact form: dish ranges of W = min(I, P);
// two-stage form: W = the K1 candidates (K1 may exceed the smallest P: a block is whole candidate rows)
struct ChunkShape {
    int64_t W, R;
    size_t n;
};

ChunkShape chunk_shape(const m2d_engine *h, const int64_t rows, const int32_t candidates)
{
    const int64_t P = h->opt_topk_mlp_chunk_pairs;
    ChunkShape c;
    c.W = candidates > 0 ? candidates : h->I < P ? h->I : P;
    c.R = m2d_block_rows(P, c.W, rows);
    c.n = ((size_t)c.R * c.W + 3) & ~(size_t)3;                     // (the id halves stay 16-byte aligned)
    return c;
}

// the head scratch of a chunk of n pairs: pair ids (users | items) and head scores; ncand > 0: stage 1's candidates as well, nheld > 0:
// the held-out pairs' scores
struct HeadScratch {
    int32_t *users_x, *items_x;
    float *scores;
};

int head_scratch(m2d_engine *h, const size_t n, const size_t ncand, const size_t nheld, HeadScratch &s)
{
    int rc;
    if ((rc = h->topk_mlp_ids.grow(h, 2 * n)) != M2D_OK) return rc;
    if ((rc = h->topk_mlp_scores.grow(h, n)) != M2D_OK) return rc;
    if (ncand && (rc = h->topk_mlp_cand.grow(h, ncand)) != M2D_OK) return rc;
    if (nheld && (rc = h->topk_mlp_held.grow(h, nheld)) != M2D_OK) return rc;
    s.users_x = h->topk_mlp_ids;
    s.items_x = s.users_x + n;
    s.scores = h->topk_mlp_scores;
    return M2D_OK;
}

// the head's scores of the pairs the generator has just written to s.users_x / s.items_x
int score_chunk(m2d_engine *h, const int64_t pairs, const HeadScratch &s, hipStream_t stream)
{
    M2D_HIP_TRY(h, hipGetLastError());
    int rc;
    if ((rc = m2d_launch_score_pairs_mlp(h, s.users_x, s.items_x, pairs, s.scores, stream)) != M2D_OK) return rc;
    ++h->topk_mlp_launches;
    return M2D_OK;
}

// an exact dish-major range: the head's scores of (users[r], d0 + c), r < rows, c < Wc, at s.scores[c * rows + r]
int score_range(m2d_engine *h, const int32_t *users, const int64_t rows, const int64_t Wc, const int64_t d0, const HeadScratch &s,
                hipStream_t stream)
{
    hipLaunchKernelGGL(m2d_topk_mlp_pairs, dim3(m2d_blocks_for(h, rows * Wc, 1024)), dim3(256), 0, stream, users, rows, Wc, (int32_t)d0,
                       s.users_x, s.items_x);
    return score_chunk(h, rows * Wc, s, stream);
}

}  // namespace

// m2d_topk_users_mlp, m2d_topk_users_mlp_excluding (deep = false: m2d_topk_mlp_select) and m2d_topk_users_mlp_deep (deep = true:
// m2d_select_deep for every k up to 1024): user blocks of R rows, per block the exact form's dish ranges -- a
// row's excluded dishes struck inside the selection -- or the two-stage form's one chunk of K1 candidates a row.  Stage 1 of the
// two-stage form: m2d_launch_topk_users per block; with exclusions m2d_launch_topk_users_excluding once for the whole call (its offsets
// are the call's, its checks are the lists' checks); under `deep` m2d_launch_deep_lists per block (exclusions already left out; its
// conditions and the lists' check are looked at once, in front of the loop).  Both exclusion forms of stage 1 can leave holes (id -1:
// fewer than K1 dishes remained): the FILL generator and the selection with HOLES behind them.
int m2d_launch_topk_users_mlp(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates, const int64_t *excl_off,
                              const int32_t *excl_ids, float *out_scores, int32_t *out_ids, const bool deep, hipStream_t stream)
{
    h->topk_mlp_launches = 0;
    if (nU == 0) return M2D_OK;
    const bool two = candidates > 0;
    const ChunkShape cs = chunk_shape(h, nU, candidates);
    const int64_t W = cs.W, R = cs.R;
    int rc;
    if (deep && two && (rc = m2d_deep_conditions(h, "m2d_topk_users_mlp_deep", stream)) != M2D_OK) return rc;
    // stage 1 once for the whole call: ids [nU, K1] | scores [nU, K1]
    const bool once = two && excl_off && !deep;
    const bool holes = two && (deep || once);
    HeadScratch s;
    if ((rc = head_scratch(h, cs.n, !two ? 0 : once ? 2 * (size_t)nU * candidates : cs.n, 0, s)) != M2D_OK) return rc;
    if (once) {       // the K1 best by the reference score among the dishes left, -1 where fewer are
        if ((rc = m2d_launch_topk_users_excluding(h, users, nU, candidates, excl_off, excl_ids,
                                                  reinterpret_cast<float *>(h->topk_mlp_cand + (size_t)nU * candidates), h->topk_mlp_cand, stream,
                                                  "m2d_topk_users_mlp_excluding", /*under_head=*/true)) != M2D_OK)
            return rc;
    } else if (excl_off && (rc = m2d_launch_check_exclusions(h, excl_off, excl_ids, nU, stream)) != M2D_OK)
        return rc;
    const int64_t *xend = excl_off ? excl_off + nU : nullptr;
    for (int64_t u0 = 0; u0 < nU; u0 += R) {
        const int64_t rows = nU - u0 < R ? nU - u0 : R;
        const int64_t *xoff = excl_off ? excl_off + u0 : nullptr;
        if (two) {
            // stage 1 of a block, as m2d_topk_users / m2d_topk_users_deep run it: the K1 best by the reference / ingredient score (its
            // scores are not kept: the head's land on them)
            if (deep)
                rc = m2d_launch_deep_lists(h, users + u0, rows, candidates, xoff, excl_ids, xend, u0, s.scores, h->topk_mlp_cand, stream);
            else if (!once)
                rc = m2d_launch_topk_users(h, users + u0, rows, candidates, s.scores, h->topk_mlp_cand, stream);
            if (rc != M2D_OK) return rc;
            const int32_t *cand = h->topk_mlp_cand + (once ? u0 * candidates : 0);
            const unsigned gb = m2d_blocks_for(h, rows * W, 1024);
            if (holes) hipLaunchKernelGGL(m2d_topk_mlp_pairs_cand<true>, dim3(gb), dim3(256), 0, stream, users + u0, cand, rows, W, s.users_x, s.items_x);
            else hipLaunchKernelGGL(m2d_topk_mlp_pairs_cand<>, dim3(gb), dim3(256), 0, stream, users + u0, cand, rows, W, s.users_x, s.items_x);
            if ((rc = score_chunk(h, rows * W, s, stream)) != M2D_OK) return rc;
            SelectJob job = SelectJob::row_major(s.scores, rows, W, holes ? cand : s.items_x, W);
            job.k = k; job.out_scores = out_scores + u0 * k; job.out_ids = out_ids + u0 * k;
            job.holes = holes;
            if ((rc = m2d_launch_select(h, job, deep, stream)) != M2D_OK) return rc;
            continue;
        }
        for (int64_t d0 = 0; d0 < h->I; d0 += W) {
            const int64_t Wc = h->I - d0 > W ? W : h->I - d0;
            if ((rc = score_range(h, users + u0, rows, Wc, d0, s, stream)) != M2D_OK) return rc;
            SelectJob job = SelectJob::dish_major(s.scores, rows, Wc, (int32_t)d0);
            job.k = k; job.out_scores = out_scores + u0 * k; job.out_ids = out_ids + u0 * k;
            job.xoff = xoff; job.xids = excl_ids; job.xend = xend;
            if ((rc = m2d_launch_select(h, job, deep, stream)) != M2D_OK) return rc;
        }
    }
    return M2D_OK;
}

int m2d_launch_catalogue_rank_mlp(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t n, const int64_t *excl_off,
                                  const int32_t *excl_ids, int32_t *out_rank, float *out_scores, hipStream_t stream)
{
    h->topk_mlp_launches = 0;
    if (n == 0) return M2D_OK;
    const ChunkShape cs = chunk_shape(h, n, 0);
    const int64_t W = cs.W, R = cs.R;
    int rc;
    HeadScratch s;
    if ((rc = head_scratch(h, cs.n, 0, out_scores ? 0 : (size_t)n, s)) != M2D_OK) return rc;
    float *held = out_scores ? out_scores : h->topk_mlp_held;
    // the held-out pairs' words (and the call's id checks: a bad user or held-out id is latched at its query)
    if ((rc = m2d_launch_score_pairs_mlp(h, users, items, n, held, stream)) != M2D_OK) return rc;
    ++h->topk_mlp_launches;
    if (excl_off && (rc = m2d_launch_check_exclusions(h, excl_off, excl_ids, n, stream)) != M2D_OK) return rc;
    for (int64_t q0 = 0; q0 < n; q0 += R) {
        const int64_t rows = n - q0 < R ? n - q0 : R;
        for (int64_t d0 = 0; d0 < h->I; d0 += W) {
            const int64_t Wc = h->I - d0 > W ? W : h->I - d0;
            if ((rc = score_range(h, users + q0, rows, Wc, d0, s, stream)) != M2D_OK) return rc;
            SelectJob job = SelectJob::dish_major(s.scores, rows, Wc, (int32_t)d0);
            job.xoff = excl_off ? excl_off + q0 : nullptr; job.xids = excl_ids; job.xend = excl_off ? excl_off + n : nullptr;
            hipLaunchKernelGGL(m2d_topk_mlp_count, dim3((unsigned)rows), dim3(select_threads(Wc)), 0, stream, job, items + q0, held + q0,
                               out_rank + q0);
            M2D_HIP_TRY(h, hipGetLastError());
        }
    }
    return M2D_OK;
}

