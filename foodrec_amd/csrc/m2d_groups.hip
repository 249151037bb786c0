// Household retrieval for gfx950 (m2d_topk_groups, m2d_score_groups_slate, m2d_topk_groups_slate; build-defined, no reference
// counterpart): ONE list of dishes for a GROUP of users.  A call takes nG groups as a padded matrix
// members i32[nG, M], 1 <= M <= M2D_GROUP_MAX_MEMBERS: row g's leading entries >= 0 are its members (global ids, repeats allowed), -1
// fills the rest.  With s_j the word m2d_score_slate writes for (member j, dish d), the group's word for d is
//   M2D_GROUP_LEAST  the word of the member that ranks WORST under tkm_key's high half (lowest score, -0 = +0, NaN worst),
//   M2D_GROUP_MOST   the word of the member that ranks best (NaN only if every member's word is NaN),
//                    -- the first member in member order among equals, in both --
//   M2D_GROUP_MEAN   acc = s_0; acc = acc + s_j for j = 1 .. cnt - 1 in member order, then one division by (float)cnt (cnt >= 2):
//                    plain float32 operators under fp contract(off) -- no fma, no reciprocal, no tree.
// A group of one returns its member's word in every mode.  The words depend on the members and the dish alone: not on nG, the
// group's position, M, or how the launcher cuts the work.
//
// Three steps per block of whole groups and per dish range (m2d_launch_groups):
//   m2d_group_members   once per call, first in stream order (its latch is the call's): checks every slot, writes a dense user array
//                       of VALID ids (a filler or bad slot holds the group's first valid member) and cnt[g];
//   the slate kernels   (m2d_slate.hip, through m2d_slate_prepare / m2d_launch_slate_scores) score the block's Gb M rows -- fillers
//                       included: their cost grows with the padding, compaction is not part of this file -- into scratch [Gb M, W];
//   m2d_group_reduce    folds each group's first cnt[g] rows into its row 0 (or into the caller's matrix), after which
//                       m2d_select_deep lists row 0 of every group: a SelectJob with row stride M W.
//
// m2d_plan_groups (the walk is m2d_menu.hip's) takes the first and the third step from here
// (m2d_launch_group_prepare, m2d_launch_group_reduce) and one kernel more:
//   m2d_group_caps      once per call, right behind m2d_group_members: folds the members' cap rows i32[nG, M, C] into one row per group,
//                       the minimum over the group's first cnt[g] members of max(cap, 0); a cap below 0 is latched with its position.
#include "m2d_engine.h"

#pragma clang fp contract(off)

namespace {

constexpr int GR_COLS = 4;                       // consecutive columns a thread of m2d_group_reduce owns: one 16-byte load per member row

__device__ __forceinline__ bool group_user_ok(const int32_t id, const int64_t U, const int64_t user_base)
{
    const int64_t ul = (int64_t)id - user_base;
    return id >= 0 && ul >= 0 && ul < U;
}

// One thread per slot t = g M + j.  An id that is neither -1 nor in the engine's range: M2D_ERR_BAD_USER_ID (id, t); an id >= 0 right
// behind a -1: M2D_ERR_INVALID_ARG (id, t); a row that starts with -1 (an empty group): M2D_ERR_INVALID_ARG (-1, g M)
// -- of a row with several defects ONE is latched, whichever thread comes first.  dense[t]: the
// slot's id where it is valid, else the row's first valid id, else user_base -- the score kernels see valid ids only.  cnt[g]: the
// row's leading entries >= 0 (thread j = 0 walks the row: M loads).  Cost: a filler slot's search for the first valid id ends at the
// row's first entry in a well-formed row -- one load; it walks further only behind bad leading entries, M loads a slot at most and
// only in a row that is latched anyway.
__global__ __launch_bounds__(256) void m2d_group_members(const int32_t *members, const int64_t nG, const int M, const int64_t U,
                                                         const int64_t user_base, int32_t *dense, int32_t *cnt, int32_t *err)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nG * M) return;
    const int64_t g = t / M;
    const int j = (int)(t - g * M);
    const int32_t *row = members + g * M;
    const int32_t id = row[j];
    const bool ok = group_user_ok(id, U, user_base);
    if (id != -1) {
        if (!ok) m2d_latch_error(err, M2D_ERR_BAD_USER_ID, id, t);
        else if (j > 0 && row[j - 1] == -1) m2d_latch_error(err, M2D_ERR_INVALID_ARG, id, t);
    } else if (j == 0) {
        m2d_latch_error(err, M2D_ERR_INVALID_ARG, -1, t);
    }
    int32_t v = id;
    if (!ok) {
        v = (int32_t)user_base;
        for (int q = 0; q < M; ++q)
            if (group_user_ok(row[q], U, user_base)) { v = row[q]; break; }
    }
    dense[t] = v;
    if (j == 0) {
        int c = 0;
        while (c < M && row[c] >= 0) ++c;
        cnt[g] = c;
    }
}

// One thread per (group g, category c), both tables in one walk of the group's first cnt[g] slots -- a filler slot's row is never
// read.  A cap below 0 of a real member: M2D_ERR_INVALID_ARG with the cap and its position (g M + j) C + c in `caps`, nG M C further
// on in `plan_caps` (the two tables as one array, caps first); it counts as 0.  What is written is >= 0, so the merge that reads the
// folded tables latches nothing.  cnt[g] = 0 (a latched call) leaves INT32_MAX: unspecified, in bounds.
// The split: the tables are nG M C words -- 65 536 groups of 4 at C = 6 are 6 MB for both, read once, against a scoring pass of
// nG M I products behind it.  A thread's loads are C words apart from its neighbour's within a group and M C words between groups, so
// a wave's loads of one step fall into 64 / C groups' rows; nothing here is worth a wave per group (6 of 64 lanes live) or LDS.
__global__ __launch_bounds__(256) void m2d_group_caps(const int32_t *caps, const int32_t *plan_caps, const int32_t *cnt, const int64_t nG,
                                                      const int M, const int C, int32_t *gcaps, int32_t *gplan, int32_t *err)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nG * C) return;
    const int64_t g = t / C;
    const int c = (int)(t - g * C);
    const int n = cnt[g] < M ? cnt[g] : M;
    int32_t lo = 0x7FFFFFFF, plo = 0x7FFFFFFF;
    for (int j = 0; j < n; ++j) {
        const int64_t at = ((int64_t)g * M + j) * C + c;
        int32_t v = caps[at];
        if (v < 0) {
            m2d_latch_error(err, M2D_ERR_INVALID_ARG, v, at);
            v = 0;
        }
        lo = v < lo ? v : lo;
        if (plan_caps) {
            int32_t w = plan_caps[at];
            if (w < 0) {
                m2d_latch_error(err, M2D_ERR_INVALID_ARG, w, nG * M * C + at);
                w = 0;
            }
            plo = w < plo ? w : plo;
        }
    }
    gcaps[t] = lo;
    if (plan_caps) gplan[t] = plo;
}

struct GroupReduceArgs {
    const float *src;       // [groups, M, W]: group g's member rows
    const int32_t *cnt;     // [groups]
    float *dst;             // group g's row at dst + g * dst_rs (in place: src, M W)
    int64_t dst_rs;
    int64_t W, chunks;      // chunks: blocks per group
    int32_t M;
};

// tkm_key's high half: the order of a score word, a SMALLER value ranks better; NaN is all ones
__device__ __forceinline__ uint32_t group_rank(const float s) { return (uint32_t)(tkm_key(s, 0) >> 32); }

template <bool VEC>
__device__ __forceinline__ void group_load(const float *p, const int n, float (&v)[GR_COLS])
{
    if (VEC) {
        const v4f x = *reinterpret_cast<const v4f *>(p);
#pragma unroll
        for (int q = 0; q < GR_COLS; ++q) v[q] = x[q];
    } else {
#pragma unroll
        for (int q = 0; q < GR_COLS; ++q) v[q] = q < n ? p[q] : 0.f;
    }
}

// Block (group g, column chunk): thread t owns columns 4 (chunk * blockDim + t) .. + 3 and walks the group's cnt[g] rows in member order
// -- row 0 always (cnt = 0 is a latched call: unspecified, in bounds), rows >= cnt never.  VEC: W % 4 == 0 and both bases 16-byte
// aligned -- one 16-byte load per row, one 16-byte store; otherwise scalar accesses, the row's tail bounded by W.
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void m2d_group_reduce(const GroupReduceArgs p)
{
    const int64_t g = blockIdx.x / p.chunks, chunk = blockIdx.x - g * p.chunks;
    const int c = __builtin_amdgcn_readfirstlane(p.cnt[g]);
    const int64_t col = (chunk * blockDim.x + threadIdx.x) * GR_COLS;
    if (col >= p.W) return;
    const int n = p.W - col < GR_COLS ? (int)(p.W - col) : GR_COLS;
    const float *row = p.src + (size_t)g * p.M * p.W + col;

    float acc[GR_COLS];
    uint32_t rank[GR_COLS];
    group_load<VEC>(row, n, acc);
    if (MODE != M2D_GROUP_MEAN) {
#pragma unroll
        for (int q = 0; q < GR_COLS; ++q) rank[q] = group_rank(acc[q]);
    }
#pragma unroll 4
    for (int j = 1; j < c; ++j) {
        float s[GR_COLS];
        group_load<VEC>(row + (size_t)j * p.W, n, s);
#pragma unroll
        for (int q = 0; q < GR_COLS; ++q) {
            if (MODE == M2D_GROUP_MEAN) {
                acc[q] = acc[q] + s[q];
            } else {
                const uint32_t r = group_rank(s[q]);
                const bool take = MODE == M2D_GROUP_LEAST ? r > rank[q] : r < rank[q];      // strict: the first member wins among equals
                acc[q] = take ? s[q] : acc[q];
                rank[q] = take ? r : rank[q];
            }
        }
    }
    if (MODE == M2D_GROUP_MEAN && c > 1) {
        const float d = (float)c;
#pragma unroll
        for (int q = 0; q < GR_COLS; ++q) acc[q] = acc[q] / d;
    }
    float *o = p.dst + (size_t)g * p.dst_rs + col;
    if (VEC) {
        v4f x;
#pragma unroll
        for (int q = 0; q < GR_COLS; ++q) x[q] = acc[q];
        *reinterpret_cast<v4f *>(o) = x;
    } else {
#pragma unroll
        for (int q = 0; q < GR_COLS; ++q)
            if (q < n) o[q] = acc[q];
    }
}

}  // namespace

int m2d_launch_group_reduce(m2d_engine *h, const int mode, const float *src, const int32_t *cnt, const int64_t groups, const int M,
                            const int64_t W, float *dst, const int64_t dst_rs, hipStream_t st)
{
    const int threads = W <= 64 * GR_COLS ? 64 : 256;
    GroupReduceArgs p;
    p.src = src; p.cnt = cnt; p.dst = dst; p.dst_rs = dst_rs; p.W = W; p.M = M;
    p.chunks = (W + (int64_t)threads * GR_COLS - 1) / ((int64_t)threads * GR_COLS);
    const bool vec = W % 4 == 0 && dst_rs % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const dim3 grid((unsigned)(groups * p.chunks));
    const auto launch = [&](auto scalar, auto vector) {
        if (vec) hipLaunchKernelGGL(vector, grid, dim3(threads), 0, st, p);
        else hipLaunchKernelGGL(scalar, grid, dim3(threads), 0, st, p);
    };
    if (mode == M2D_GROUP_LEAST) launch(m2d_group_reduce<M2D_GROUP_LEAST, false>, m2d_group_reduce<M2D_GROUP_LEAST, true>);
    else if (mode == M2D_GROUP_MEAN) launch(m2d_group_reduce<M2D_GROUP_MEAN, false>, m2d_group_reduce<M2D_GROUP_MEAN, true>);
    else launch(m2d_group_reduce<M2D_GROUP_MOST, false>, m2d_group_reduce<M2D_GROUP_MOST, true>);
    M2D_HIP_TRY(h, hipGetLastError());
    return M2D_OK;
}

// What m2d_plan_groups runs in front of its walk: m2d_group_members, first in stream order, and -- member_caps != null -- m2d_group_caps
// right behind it.  group_ids: dense i32[nG M] | cnt i32[nG] | folded caps i32[nG, C] | folded plan caps i32[nG, C].
int m2d_launch_group_prepare(m2d_engine *h, const int32_t *members, const int64_t nG, const int32_t M, const int32_t *member_caps,
                             const int32_t *member_plan_caps, const int32_t **dense, const int32_t **cnt, const int32_t **group_caps,
                             const int32_t **group_plan_caps, hipStream_t st)
{
    int rc;
    const int64_t slots = nG * M, table = nG * h->C;
    if ((rc = h->group_ids.grow(h, (size_t)(slots + nG + 2 * table))) != M2D_OK) return rc;
    int32_t *d = h->group_ids, *n = d + slots, *gc = n + nG, *gp = gc + table;
    hipLaunchKernelGGL(m2d_group_members, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, members, nG, M, h->U, h->user_base, d, n,
                       h->err_dev);
    M2D_HIP_TRY(h, hipGetLastError());
    *dense = d;
    *cnt = n;
    if (member_caps) {
        hipLaunchKernelGGL(m2d_group_caps, dim3((unsigned)((table + 255) / 256)), dim3(256), 0, st, member_caps, member_plan_caps, n, nG, M,
                           h->C, gc, gp, h->err_dev);
        M2D_HIP_TRY(h, hipGetLastError());
        *group_caps = gc;
        *group_plan_caps = member_plan_caps ? gp : nullptr;
    }
    return M2D_OK;
}

// Blocks of Gb = max(1, P / (M W)) whole groups, P = option "deep_chunk_pairs"; catalogue form (slate == null): dish ranges of
// W = min(I, P, 65536) dishes, the first range starts a row's list and the others merge into it (m2d_launch_deep_lists' rule); slate
// forms: W = nD, one range (d0 = 0) -- their scratch, M nD floats a group, is NOT bounded by the option.
int m2d_launch_groups(m2d_engine *h, const char *entry, const int32_t *members, const int64_t nG, const int32_t M, const int32_t mode,
                      const int32_t *slate, const int64_t nD, const int32_t k, const int64_t *excl_off, const int32_t *excl_ids, float *out,
                      float *out_scores, int32_t *out_ids, hipStream_t st)
{
    int rc;
    if ((rc = m2d_deep_conditions(h, entry, st)) != M2D_OK) return rc;
    const int64_t slots = nG * M;
    if ((rc = h->group_ids.grow(h, (size_t)(slots + nG))) != M2D_OK) return rc;
    int32_t *dense = h->group_ids, *cnt = h->group_ids + slots;
    hipLaunchKernelGGL(m2d_group_members, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, members, nG, M, h->U, h->user_base, dense,
                       cnt, h->err_dev);
    M2D_HIP_TRY(h, hipGetLastError());
    if (excl_off && (rc = m2d_launch_check_exclusions(h, excl_off, excl_ids, nG, st)) != M2D_OK) return rc;

    const int64_t P = h->opt_deep_chunk_pairs, total = slate ? nD : h->I;
    const int64_t W0 = total < P ? total : P, W = slate ? nD : W0 < 65536 ? W0 : 65536;
    const int64_t Gb = m2d_block_rows(P, (int64_t)M * W, nG);
    if ((rc = h->slate_scores.grow(h, (size_t)Gb * M * W)) != M2D_OK) return rc;
    // ranges outside, blocks inside: a range's dish vectors are built ONCE for all blocks (a row's list lives in the outputs between
    // its ranges, so the order of the two loops does not show in it)
    for (int64_t d0 = 0; d0 < total; d0 += W) {
        const int64_t Wc = total - d0 > W ? W : total - d0;
        SlateArgs a;
        bool mfma = false;
        if ((rc = m2d_slate_prepare(h, slate, (int32_t)d0, Wc, a, mfma, st)) != M2D_OK) return rc;
        for (int64_t g0 = 0; g0 < nG; g0 += Gb) {
            const int64_t n = nG - g0 < Gb ? nG - g0 : Gb;
            a.users = dense + g0 * M; a.nU = n * M; a.index_base = g0 * M; a.out = h->slate_scores;
            if ((rc = m2d_launch_slate_scores(h, a, mfma, st)) != M2D_OK) return rc;
            if (out) {                                       // m2d_score_groups_slate: straight into the caller's matrix
                if ((rc = m2d_launch_group_reduce(h, mode, h->slate_scores, cnt + g0, n, M, Wc, out + g0 * nD, nD, st)) != M2D_OK) return rc;
                continue;
            }
            if ((rc = m2d_launch_group_reduce(h, mode, h->slate_scores, cnt + g0, n, M, Wc, h->slate_scores, (int64_t)M * Wc, st)) != M2D_OK)
                return rc;
            SelectJob job = SelectJob::row_major(h->slate_scores, n, Wc, slate, 0, (int32_t)d0);
            job.rs = (int64_t)M * Wc;                        // a group's list is read from its row 0
            job.k = k; job.out_scores = out_scores + g0 * k; job.out_ids = out_ids + g0 * k;
            job.xoff = excl_off ? excl_off + g0 : nullptr; job.xids = excl_ids; job.xend = excl_off ? excl_off + nG : nullptr;
            if ((rc = m2d_launch_select(h, job, /*deep=*/true, st)) != M2D_OK) return rc;
        }
    }
    return M2D_OK;
}
