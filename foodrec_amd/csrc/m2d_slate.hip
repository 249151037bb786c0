// Slate scoring for gfx950 (m2d_score_slate, m2d_topk_slate; build-defined, no reference counterpart): many users against ONE shared,
// ascending list of dishes -- the [nU, nD] score matrix, or the k best dishes of the slate per user.
//
// By the algebra of m2d_catalogue_dense.hip's header, score(u, d) = <flatten(PM[u]), Dt[d]> with K = (C + 1) E, so the call is a dense
// [nU x K] . [K x nD] contraction of GATHERED rows on both sides: the user rows come straight from Personal_Memory, the dish rows
// from a per-call table Dt_s that holds the slate's dish vectors only (m2d_build_slate_vectors; the full-catalogue table of
// m2d_ensure_dish_vectors is neither built nor read here).  Exact f32 on v_mfma_f32_32x32x2_f32: one accumulator per (user, dish)
// that starts at +0 and takes one fused multiply-add per k, in an order of k that depends on E alone -- so a score's bits do not
// depend on nU, nD, where its row or column stands, or how the launcher cuts the work.
//
// m2d_score_slate_mfma<TN>.  A block of 4 waves owns a tile of BM = 128 users x BN = 64 TN dishes (TN = 2; TN = 1 for slates of up to
// 64 dishes); wave (wm, wn) owns 64 users x 32 TN dishes of it as 2 x TN accumulator tiles of 32 x 32 that live in registers across
// the whole K loop.  Users are the MFMA's A side (rows), dishes its B side (columns): in the 32 x 32 C/D layout register r of lanes
// 0-31 then holds 32 CONSECUTIVE dishes of one user row, and the epilogue stores whole 128-byte segments of `out` from the
// accumulators.  K is stepped through LDS in chunks of KC = 32 floats, two stage buffers: LDS-DMA (global_load_lds_dwordx4, 16 B
// per lane) fills one stage while the other is multiplied.  A stage image is [row][8 slots of 16 B]; the 16-byte slot q of row r
// sits at slot q ^ ((r >> 1) & 7) -- the swizzle is on the DMA's per-lane SOURCE address, the LDS side stays lane-linear -- so the
// 16 lanes ds_read_b128 serves together (8 row pairs of one slot column) touch 16 different 16-byte bank groups.  Both operands are
// ZERO past K and past the last user / dish: Dt_s rows are K rounded up to KC floats wide with zeros behind K and zero rows up to
// the tile multiple; a user-side lane whose slot lies past K, or whose row lies past nU (or holds a bad id), reads Dt_s's last row,
// which is all zeros.  fma(0, 0, acc) leaves acc as it is.
//
// LDS: 2 stages x (128 + 64 TN) rows x 128 B = 64 KiB (TN = 2) / 48 KiB (TN = 1): two blocks per CU.  Registers: 32 TN accumulator
// words, 8 + 4 TN source pointers of the DMA pieces (a lane's pieces are the same rows in every stage), 4 swizzled read offsets.
#include "m2d_catalogue.h"

#pragma clang fp contract(off)

namespace {

constexpr int SL_BM = 128;                       // users of a block's tile
constexpr int SL_KC = 32;                        // floats of K per LDS stage
constexpr int SL_DPAD = 128;                     // Dt_s holds zero rows up to this multiple of dishes (the largest BN)

// ---- slate vectors ------------------------------------------------------------------------------------------------------------------
// One wave per row of Dt_s: rows [0, nD) are the slate's dish vectors -- dish_vector_row, the expressions of m2d_build_dish_vectors --
// zero behind K; rows [nD, rows) are zero.  The wave of entry j checks it: an id outside [0, I) is latched as M2D_ERR_BAD_ITEM_ID (its
// row stays zero: nothing is read for it), an id not above its predecessor as M2D_ERR_INVALID_ARG (a predecessor that is itself out
// of range is reported by its own wave).  The d0 form (slate == null: a dish range of m2d_topk_users_deep): entry j is dish d0 + j.
__global__ __launch_bounds__(256) void m2d_build_slate_vectors(const float *re, const float *ce, const float *dish_cats, const int32_t *slate,
                                                               int32_t d0, int64_t nD, int64_t rows, int64_t I, int C, int E, float a, float b,
                                                               float *dt, int Kp, int32_t *err)
{
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= rows) return;
    const int K = (C + 1) * E;
    float *o = dt + (size_t)j * Kp;
    bool ok = false;
    if (j < nD) {
        const int32_t d = slate ? slate[j] : d0 + (int32_t)j;
        ok = d >= 0 && (int64_t)d < I;
        if (!ok) {
            if (lane == 0) m2d_latch_error(err, M2D_ERR_BAD_ITEM_ID, d, j);
        } else if (slate && j > 0) {
            const int32_t prev = slate[j - 1];
            if (prev >= 0 && (int64_t)prev < I && prev >= d && lane == 0) m2d_latch_error(err, M2D_ERR_INVALID_ARG, d, j);
        }
        if (ok) dish_vector_row(re, ce, dish_cats, nullptr, d, C, E, a, b, lane, o);
    }
    for (int k = (ok ? K : 0) + lane; k < Kp; k += 64) o[k] = 0.f;
}

// (SlateArgs: m2d_engine.h)

// a user's row in Personal_Memory, or -1 (past nU, or a bad id -- latched by `report`)
__device__ __forceinline__ int64_t slate_user_row(const SlateArgs &p, const int64_t ui, const bool report)
{
    if (ui >= p.nU) return -1;
    const int32_t uid = p.users[ui];
    const int64_t ul = (int64_t)uid - p.user_base;
    if (ul < 0 || ul >= p.U) {
        if (report) m2d_latch_error(p.err, M2D_ERR_BAD_USER_ID, uid, p.index_base + ui);
        return -1;
    }
    return ul;
}

template <int TN>
__global__ __launch_bounds__(256) void m2d_score_slate_mfma(SlateArgs p)
{
    constexpr int BM = SL_BM, BN = 64 * TN, KC = SL_KC;
    constexpr int APW = BM * (KC / 4) / 64 / 4;  // 1-KiB DMA pieces (8 rows x 128 B) per wave and stage: user side 4 ...
    constexpr int BPW = BN * (KC / 4) / 64 / 4;  // ... dish side 2 TN
    constexpr int STAGE = (BM + BN) * KC;        // floats
    extern __shared__ __align__(16) float smem[];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int j = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int nst = p.Kp / KC;
    int rd_off[KC / 8];                          // float offset of fragment T in the lane's image row: slot (2 T + h) ^ ((row >> 1) & 7)
#pragma unroll
    for (int T = 0; T < KC / 8; ++T) rd_off[T] = ((2 * T + h) ^ ((j >> 1) & 7)) * 4;

    const int64_t tiles = p.utiles * p.dtiles;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t ut = tile / p.dtiles;
        const int64_t u0 = ut * BM, d0 = (tile - ut * p.dtiles) * BN;

        // ---- the rows this lane's DMA pieces carry: piece pc = wave + 4 i is image rows 8 pc .. 8 pc + 7, lane l its row 8 pc + (l >> 3),
        //      physical slot l & 7 -- which must receive logical slot (l & 7) ^ ((row >> 1) & 7)
        const float *asrc[APW], *bsrc[BPW];
        int aoff[APW];
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            const int r = (wave + 4 * i) * 8 + (lane >> 3);
            const int64_t ul = slate_user_row(p, u0 + r, (lane & 7) == 0);
            aoff[i] = ((lane & 7) ^ ((r >> 1) & 7)) * 4;
            asrc[i] = ul >= 0 ? p.pm + (size_t)ul * p.K + aoff[i] : nullptr;
        }
#pragma unroll
        for (int i = 0; i < BPW; ++i) {
            const int r = (wave + 4 * i) * 8 + (lane >> 3);
            bsrc[i] = p.dt + (size_t)(d0 + r) * p.Kp + ((lane & 7) ^ ((r >> 1) & 7)) * 4;
        }
        auto issue_stage = [&](const int s, const int buf) {
            float *dst = smem + (size_t)buf * STAGE;
#pragma unroll
            for (int i = 0; i < APW; ++i) {
                const bool live = asrc[i] != nullptr && s * KC + aoff[i] < p.K;      // (K is a multiple of 4: a slot is inside or outside)
                lds_dma16(live ? asrc[i] + s * KC : p.zero, dst + (wave + 4 * i) * 256);
            }
#pragma unroll
            for (int i = 0; i < BPW; ++i) lds_dma16(bsrc[i] + s * KC, dst + BM * KC + (wave + 4 * i) * 256);
        };

        v16f acc[2][TN];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

        issue_stage(0, 0);
        wait_all_vmem();
        __syncthreads();
        for (int s = 0; s < nst; ++s) {
            const int buf = s & 1;
            if (s + 1 < nst) issue_stage(s + 1, buf ^ 1);
            const float *imgA = smem + (size_t)buf * STAGE + (size_t)(wm * 64 + j) * KC;
            const float *imgB = smem + (size_t)buf * STAGE + BM * KC + (size_t)(wn * 32 * TN + j) * KC;
#pragma unroll
            for (int T = 0; T < KC / 8; ++T) {
                v4f av[2], bv[TN];
#pragma unroll
                for (int tm = 0; tm < 2; ++tm) av[tm] = *reinterpret_cast<const v4f *>(imgA + tm * 32 * KC + rd_off[T]);
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) bv[tn] = *reinterpret_cast<const v4f *>(imgB + tn * 32 * KC + rd_off[T]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                        for (int tn = 0; tn < TN; ++tn)
                            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm][q], bv[tn][q], acc[tm][tn], 0, 0, 0);
            }
            wait_all_vmem();
            __syncthreads();
        }

        // ---- epilogue: register r of lane (j, h) is user row (r & 3) + 8 (r >> 2) + 4 h, dish column j of its 32 x 32 tile
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int64_t col = d0 + wn * 32 * TN + tn * 32 + j;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = u0 + wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (row < p.nU && col < p.nD) p.out[(size_t)row * p.nD + col] = acc[tm][tn][r];
                }
            }
    }
}

// Every other shape (C != 4, E no multiple of 4, E > 256; "variant" = 9): one output per thread, the same Dt_s, an fmaf chain in
// increasing k from +0.  Correct and untuned: it makes the calls total over shapes, as m2d_topk_generic does.
__global__ __launch_bounds__(256) void m2d_score_slate_generic(SlateArgs p)
{
    const int64_t total = p.nU * p.nD, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t ui = t / p.nD, c = t - ui * p.nD;
        const int64_t ul = slate_user_row(p, ui, c == 0);
        float s = __builtin_nanf("");
        if (ul >= 0) {
            const float *um = p.pm + (size_t)ul * p.K, *dv = p.dt + (size_t)c * p.Kp;
            s = 0.f;
            for (int k = 0; k < p.K; ++k) s = fmaf(um[k], dv[k], s);
        }
        p.out[t] = s;
    }
}

int launch_scores(m2d_engine *h, SlateArgs &a, const bool mfma, hipStream_t st)
{
    if (!mfma) {
        hipLaunchKernelGGL(m2d_score_slate_generic, dim3(m2d_blocks_for(h, a.nU * a.nD, 256, 16)), dim3(256), 0, st, a);
        M2D_HIP_TRY(h, hipGetLastError());
        return M2D_OK;
    }
    const int TN = a.nD <= 64 ? 1 : 2, BN = 64 * TN;
    a.utiles = (a.nU + SL_BM - 1) / SL_BM;
    a.dtiles = (a.nD + BN - 1) / BN;
    const int64_t tiles = a.utiles * a.dtiles;
    const unsigned grid = (unsigned)(tiles < 0x7fffffff ? tiles : 0x7fffffff);
    const size_t lds = (size_t)2 * (SL_BM + BN) * SL_KC * sizeof(float);
    if (TN == 1) {
        M2D_HIP_TRY(h, m2d_lds_limit((const void *)m2d_score_slate_mfma<1>, (int)lds));
        hipLaunchKernelGGL(m2d_score_slate_mfma<1>, dim3(grid), dim3(256), lds, st, a);
    } else {
        M2D_HIP_TRY(h, m2d_lds_limit((const void *)m2d_score_slate_mfma<2>, (int)lds));
        hipLaunchKernelGGL(m2d_score_slate_mfma<2>, dim3(grid), dim3(256), lds, st, a);
    }
    M2D_HIP_TRY(h, hipGetLastError());
    return M2D_OK;
}

// the call's slate vectors in slate_dt (`slate` null: the dishes d0 .. d0 + nD - 1) and what the score kernels take but users, rows and out
int slate_prepare(m2d_engine *h, const int32_t *slate, int32_t d0, int64_t nD, SlateArgs &a, bool &mfma, hipStream_t st)
{
    const int K = (h->C + 1) * h->E, Kp = (K + SL_KC - 1) / SL_KC * SL_KC;
    const int64_t rows = (nD + SL_DPAD - 1) / SL_DPAD * SL_DPAD + 1;          // the slate, zero rows up to the tile multiple, the zero row
    int rc;
    if ((rc = h->slate_dt.grow(h, (size_t)rows * Kp)) != M2D_OK) return rc;
    hipLaunchKernelGGL(m2d_build_slate_vectors, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, h->re, h->ce, h->dish_cats, slate, d0, nD,
                       rows, h->I, h->C, h->E, h->a, h->b, h->slate_dt, Kp, h->err_dev);
    M2D_HIP_TRY(h, hipGetLastError());
    mfma = h->C == 4 && h->E % 4 == 0 && h->E <= 256 && h->opt_variant != 9;
    a.pm = h->pm; a.dt = h->slate_dt; a.zero = h->slate_dt + (size_t)(rows - 1) * Kp;
    a.U = h->U; a.user_base = h->user_base; a.nD = nD; a.utiles = a.dtiles = 0; a.K = K; a.Kp = Kp; a.err = h->err_dev;
    h->last_kernel = mfma ? "m2d_score_slate_mfma" : "m2d_score_slate_generic";
    return M2D_OK;
}

}  // namespace

// what every call on the slate kernels needs of the tables (the head refusal is the public slate entries' own)
int m2d_deep_conditions(m2d_engine *h, const char *entry, hipStream_t st)
{
    auto refuse = [&](const char *why) {
        h->last_error = std::string(entry) + ": " + why;
        return M2D_ERR_UNSUPPORTED;
    };
    if (h->ing || h->dish_high) return refuse("the ingredient table is set (not supported)");
    int rc;
    if ((rc = m2d_ensure_finite_scan(h, st)) != M2D_OK) return rc;
    if ((rc = m2d_refresh_nonfinite(h, st)) != M2D_OK) return rc;
    if (h->grp_nonfinite) return refuse("needs finite tables (a table value is not finite)");
    return M2D_OK;
}

int m2d_launch_slate(m2d_engine *h, const char *entry, const int32_t *users, int64_t nU, const int32_t *slate, int64_t nD, int32_t k,
                     float *out, float *out_scores, int32_t *out_ids, hipStream_t st)
{
    if (h->mlp_w1 && !(h->ing || h->dish_high)) {
        h->last_error = std::string(entry) + ": the MLP head is set (not supported)";
        return M2D_ERR_UNSUPPORTED;
    }
    int rc;
    if ((rc = m2d_deep_conditions(h, entry, st)) != M2D_OK) return rc;

    SlateArgs a;
    bool mfma;
    if ((rc = slate_prepare(h, slate, 0, nD, a, mfma, st)) != M2D_OK) return rc;
    if (out) {
        a.users = users; a.nU = nU; a.index_base = 0; a.out = out;
        return launch_scores(h, a, mfma, st);
    }
    // m2d_topk_slate: user blocks of max(1, P / nD) rows are scored into scratch and selected from there
    const int64_t R = m2d_block_rows(h->opt_slate_chunk_pairs, nD, nU);
    if ((rc = h->slate_scores.grow(h, (size_t)R * nD)) != M2D_OK) return rc;
    for (int64_t u0 = 0; u0 < nU; u0 += R) {
        const int64_t n = nU - u0 < R ? nU - u0 : R;
        a.users = users + u0; a.nU = n; a.index_base = u0; a.out = h->slate_scores;
        if ((rc = launch_scores(h, a, mfma, st)) != M2D_OK) return rc;
        SelectJob job = SelectJob::row_major(h->slate_scores, n, nD, slate, 0);      // one id row for all: the slate
        job.k = k; job.out_scores = out_scores + u0 * k; job.out_ids = out_ids + u0 * k;
        if ((rc = m2d_launch_select(h, job, /*deep=*/false, st)) != M2D_OK) return rc;
    }
    return M2D_OK;
}

// m2d_topk_users_deep: dish ranges of W = min(I, P, 65536) dishes, user blocks of max(1, P / W) rows; per block
// and range the range's vectors (the builder's d0 form), the score kernel into scratch, m2d_select_deep over the block's rows -- the
// first range starts a row's list, the others merge into it where it stands in the outputs.
int m2d_launch_deep_lists(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int64_t *excl_off, const int32_t *excl_ids,
                          const int64_t *excl_end, int64_t index_base, float *out_scores, int32_t *out_ids, hipStream_t st)
{
    const int64_t P = h->opt_deep_chunk_pairs;
    const int64_t W0 = h->I < P ? h->I : P, W = W0 < 65536 ? W0 : 65536;
    const int64_t R = m2d_block_rows(P, W, nU);
    int rc;
    if ((rc = h->slate_scores.grow(h, (size_t)R * W)) != M2D_OK) return rc;
    for (int64_t u0 = 0; u0 < nU; u0 += R) {
        const int64_t n = nU - u0 < R ? nU - u0 : R;
        for (int64_t d0 = 0; d0 < h->I; d0 += W) {
            const int64_t Wc = h->I - d0 > W ? W : h->I - d0;
            SlateArgs a;
            bool mfma;
            if ((rc = slate_prepare(h, nullptr, (int32_t)d0, Wc, a, mfma, st)) != M2D_OK) return rc;
            a.users = users + u0; a.nU = n; a.index_base = index_base + u0; a.out = h->slate_scores;
            if ((rc = launch_scores(h, a, mfma, st)) != M2D_OK) return rc;
            SelectJob job = SelectJob::row_major(h->slate_scores, n, Wc, nullptr, 0, (int32_t)d0);
            job.k = k; job.out_scores = out_scores + u0 * k; job.out_ids = out_ids + u0 * k;
            job.xoff = excl_off ? excl_off + u0 : nullptr; job.xids = excl_ids; job.xend = excl_end;
            if ((rc = m2d_launch_select(h, job, /*deep=*/true, st)) != M2D_OK) return rc;
        }
    }
    return M2D_OK;
}

int m2d_launch_topk_users_deep(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int64_t *excl_off, const int32_t *excl_ids,
                               float *out_scores, int32_t *out_ids, hipStream_t st)
{
    int rc;
    if ((rc = m2d_deep_conditions(h, "m2d_topk_users_deep", st)) != M2D_OK) return rc;
    if (excl_off && (rc = m2d_launch_check_exclusions(h, excl_off, excl_ids, nU, st)) != M2D_OK) return rc;
    return m2d_launch_deep_lists(h, users, nU, k, excl_off, excl_ids, excl_off ? excl_off + nU : nullptr, 0, out_scores, out_ids, st);
}

// the two steps above for launchers outside this file (m2d_groups.hip): the same kernels, the same words
int m2d_slate_prepare(m2d_engine *h, const int32_t *slate, int32_t d0, int64_t nD, SlateArgs &a, bool &mfma, hipStream_t st)
{
    return slate_prepare(h, slate, d0, nD, a, mfma, st);
}

int m2d_launch_slate_scores(m2d_engine *h, SlateArgs &a, bool mfma, hipStream_t st) { return launch_scores(h, a, mfma, st); }
