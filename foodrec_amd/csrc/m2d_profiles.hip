// Build-defined extension (no reference counterpart): serving from health labels.
//
// The reference reads General_Memory only while it writes: Write_Memory (Model_Recommender.py:170-198) adds
// alpha * (sum_l y_l GM[l]) / (sum_l y_l) to the user's block of Personal_Memory.  A profile q = (u_q, y_q) is that block BY VALUE,
//
//   ysum = sum_l y_l                     label order, weights != 0 only, plain adds
//   g_k  = fmaf(y_l, GM[l][k], g_k)      label order, weights != 0 only, from 0
//   M_k  = base_k + alpha * (g_k / ysum) true division, one rounded product, one rounded sum
//   base = PM[u_q - user_base] for u_q >= 0, zeros for a guest (u_q == -1, or no user array at all)
//
// -- m2d_write_memory_kernel<0>'s g, ysum and alpha * (g / ysum) (m2d_write.hip) and the add its atomicAdd performs -- and nothing is
// written to any table.  m2d_compose_profiles_kernel makes the rows; the serving calls compose into engine scratch and run the
// launchers that exist against those rows through m2d_rows_view (m2d_engine.h): the pattern-grouped retrieval, the exclusion tiers,
// the pair kernels and the market-request kernel are the code for the heavy part, there is no second scan here.
//
// Containment.  The fast scans leave products with weight-0 rows out on the engine's word "every table value is finite": rows they
// may see have to be finite while that word is 0.  The composer reads the word: while it is 0 a request whose row would hold an
// inf / NaN gets a row of zeros and latches M2D_ERR_INVALID_ARG (number of non-zero labels, q); while it is 1 the rows are written
// as computed and retrieval takes the literal kernels anyway.  A label of weight 0 is not read (the write kernel's rule), so an inf
// in a General_Memory row nobody addresses does not matter.
#include <math.h>
#include <string.h>

#include <type_traits>

#include "m2d_engine.h"

namespace {

struct ProfileArgs {
    const float *pm;         // [U, W]
    const float *gm;         // [L, W]
    const float *labels;     // [n, L]
    const int32_t *users;    // [n] or null
    float *out;              // [n, W]
    int32_t *ids;            // [n] := 0 .. n-1, or null
    int64_t n, U, user_base;
    int32_t W, L;            // W = (C + 1) E
    float alpha;
    int32_t *err;
    const int32_t *nonfinite;
};

// Wave-uniform values are carried in SGPRs, every ballot below runs under a full EXEC mask (m2d_market_requests.hip's convention)
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ float compose_one(const float base, const float g, const float ysum, const float alpha)
{
#pragma clang fp contract(off)
    const float t = alpha * (g / ysum);      // Model_Recommender.py:184-186
    return base + t;                         // :198 -- two roundings, as the write kernel's product and its atomic add
}

__device__ __forceinline__ float col_zero(float) { return 0.f; }
__device__ __forceinline__ v4f col_zero(v4f) { return v4f{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ float col_fma(const float w, const float r, const float g) { return fmaf(w, r, g); }
__device__ __forceinline__ v4f col_fma(const float w, const v4f r, const v4f g)
{
    return v4f{fmaf(w, r.x, g.x), fmaf(w, r.y, g.y), fmaf(w, r.z, g.z), fmaf(w, r.w, g.w)};
}
__device__ __forceinline__ float col_compose(const float b, const float g, const float ysum, const float alpha)
{
    return compose_one(b, g, ysum, alpha);
}
__device__ __forceinline__ v4f col_compose(const v4f b, const v4f g, const float ysum, const float alpha)
{
    return v4f{compose_one(b.x, g.x, ysum, alpha), compose_one(b.y, g.y, ysum, alpha), compose_one(b.z, g.z, ysum, alpha),
               compose_one(b.w, g.w, ysum, alpha)};
}
// x * 0 is 0 for every finite x and NaN for inf / NaN
__device__ __forceinline__ bool col_nonfinite(const float v) { return v * 0.f != 0.f; }
__device__ __forceinline__ bool col_nonfinite(const v4f v) { return (v.x * 0.f + v.y * 0.f) + (v.z * 0.f + v.w * 0.f) != 0.f; }

constexpr int MAXM = 4;       // mask words of 64 labels: the lane-mask form serves L <= 256
constexpr int KEEP = 5;       // columns a lane keeps in registers between the non-finite test and the store, at most

// A request's labels of non-zero weight, in label order, wave-uniform: the write kernel's two forms.  L <= 256: lane l of word w holds
// y[64 w + l], a ballot per word gives the lane mask and a weight comes out of its lane's register -- nothing is loaded twice; beyond:
// a plain loop over y.
struct LabelCursor {
    int w = 0, l = 0;
    unsigned long long bits = 0ull;
};

// One wave per request, grid-stride.  VEC: a float4 column per lane (E a multiple of 4, 16-byte aligned rows), else a float.  NK: the
// columns a lane keeps -- every column of rows up to 64 NK columns ((C + 1) E <= 1280 floats with VEC and NK = 5); wider rows compute
// the rest again for the store, from rows that are in L2 by then.  A request is a chain of dependent memory trips -- its labels, then
// the General_Memory rows they name -- and a wave has one request in flight: the base row is asked for before the labels are walked,
// the labels are taken two at a time, and all of a lane's columns of both rows are asked for before the first of them is used.
template <bool VEC, int NK>
__global__ __launch_bounds__(256, (VEC && NK > 2) ? 4 : 8) void m2d_compose_profiles_kernel(ProfileArgs p)
{
    using T = typename std::conditional<VEC, v4f, float>::type;
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + uni(threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const int L = p.L, cols = VEC ? p.W >> 2 : p.W;
    const bool masks = L <= 64 * MAXM;
    const bool literal = uni(*p.nonfinite) != 0;
    const float alpha = p.alpha;
    const T *gm = reinterpret_cast<const T *>(p.gm);
    for (int64_t q = wave0; q < p.n; q += nwaves) {
        T *orow = reinterpret_cast<T *>(p.out) + (size_t)q * cols;
        if (p.ids && lane == 0) p.ids[q] = (int32_t)q;
        const int32_t uid = p.users ? uni(p.users[q]) : -1;
        const int64_t ul = (int64_t)uid - p.user_base;
        const bool guest = uid == -1;
        if (!guest && (ul < 0 || ul >= p.U)) {               // wave-uniform: nothing is read for that user
            if (lane == 0) m2d_latch_error(p.err, M2D_ERR_BAD_USER_ID, uid, q);
            for (int j = lane; j < cols; j += 64) orow[j] = col_zero(T{});
            continue;
        }
        const T *brow = reinterpret_cast<const T *>(p.pm) + (size_t)(guest ? 0 : ul) * cols;
        const float *y = p.labels + (size_t)q * L;
        float yv[MAXM];
        unsigned long long am[MAXM];
#pragma unroll
        for (int w = 0; w < MAXM; ++w) {
            const int l = w * 64 + lane;
            yv[w] = (masks && l < L) ? y[l] : 0.f;
            am[w] = (masks && w * 64 < L) ? __ballot(yv[w] != 0.f) : 0ull;
        }
        T base[NK];
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            const int j = c * 64 + lane;
            base[c] = (!guest && j < cols) ? brow[j] : col_zero(T{});
        }
        // the next label of non-zero weight and its weight; false: none is left
        auto next = [&](LabelCursor &k, int &l, float &wt) __attribute__((always_inline)) {
            if (masks) {
#pragma unroll
                for (int w = 0; w < MAXM; ++w)
                    if (k.bits == 0ull && k.w <= w) { k.w = w + 1; k.bits = am[w]; }      // k.w: one past the word `bits` came from
                if (k.bits == 0ull) return false;
                const int b = __builtin_ctzll(k.bits);
                k.bits &= k.bits - 1;
                const float v = k.w == 1 ? yv[0] : k.w == 2 ? yv[1] : k.w == 3 ? yv[2] : yv[3];
                l = (k.w - 1) * 64 + b;
                wt = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), b));
                return true;
            }
            while (k.l < L) {
                const float v = __builtin_bit_cast(float, uni(__builtin_bit_cast(int, y[k.l])));
                ++k.l;
                if (v != 0.f) { l = k.l - 1; wt = v; return true; }
            }
            return false;
        };
        float ysum = 0.f;
        int32_t m = 0;
        {
            LabelCursor k;
            int l;
            float wt;
            while (next(k, l, wt)) { ysum += wt; ++m; }                      // :180 -- the zero weights add nothing
        }
        // g of the lane's kept columns: two labels a trip, every column of both rows in flight before the first fma
        T g[NK];
#pragma unroll
        for (int c = 0; c < NK; ++c) g[c] = col_zero(T{});
        {
            LabelCursor k;
            int l0, l1;
            float w0, w1;
            while (next(k, l0, w0)) {
                const bool two = next(k, l1, w1);
                if (!two) l1 = l0;                                           // (loaded again, not used)
                const T *r0 = gm + (size_t)l0 * cols, *r1 = gm + (size_t)l1 * cols;
                T a0[NK], a1[NK];
#pragma unroll
                for (int c = 0; c < NK; ++c) {
                    const int j = c * 64 + lane;
                    a0[c] = j < cols ? r0[j] : col_zero(T{});
                    a1[c] = j < cols ? r1[j] : col_zero(T{});
                }
#pragma unroll
                for (int c = 0; c < NK; ++c) {
                    g[c] = col_fma(w0, a0[c], g[c]);                         // :172-176
                    if (two) g[c] = col_fma(w1, a1[c], g[c]);
                }
            }
        }
        // a column past the kept ones, start to end
        auto column = [&](const int j) __attribute__((always_inline)) {
            T gj = col_zero(T{});
            LabelCursor k;
            int l;
            float wt;
            while (next(k, l, wt)) gj = col_fma(wt, gm[(size_t)l * cols + j], gj);
            return col_compose(guest ? col_zero(T{}) : brow[j], gj, ysum, alpha);
        };
        T keep[NK];
        bool notfin = false;
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            keep[c] = col_compose(base[c], g[c], ysum, alpha);
            notfin = notfin || (c * 64 + lane < cols && col_nonfinite(keep[c]));
        }
        // (wave-uniform trips with the column clamped, the guard on the result: the cursor's readlane runs under a full EXEC mask)
        for (int j0 = NK * 64; j0 < cols; j0 += 64) {
            const int j = j0 + lane;
            const T v = column(j < cols ? j : cols - 1);
            notfin = notfin || (j < cols && col_nonfinite(v));
        }
        // wave-uniform, before the first store: a row is wholly composed or wholly zero
        const bool zero_row = !literal && __ballot(notfin) != 0ull;
        if (zero_row && lane == 0) m2d_latch_error(p.err, M2D_ERR_INVALID_ARG, m, q);
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            const int j = c * 64 + lane;
            if (j < cols) orow[j] = zero_row ? col_zero(T{}) : keep[c];
        }
        for (int j0 = NK * 64; j0 < cols; j0 += 64) {
            const int j = j0 + lane;
            const T v = column(j < cols ? j : cols - 1);
            if (j < cols) orow[j] = zero_row ? col_zero(T{}) : v;
        }
    }
}

int fail(m2d_engine *h, int code, const std::string &msg)
{
    h->last_error = msg;
    return code;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the refusals every profile call shares; n == 0 is the caller's to return on
int check_batch(m2d_engine *h, const char *entry, const m2d_profile_batch *p)
{
    const std::string e(entry);
    if (!p) return fail(h, M2D_ERR_INVALID_ARG, e + ": null batch");
    if (p->n < 0 || p->n > (int64_t)INT32_MAX || p->L < 1) return fail(h, M2D_ERR_INVALID_ARG, e + ": need 0 <= n < 2^31 and L >= 1");
    if (!p->labels || !p->general_memory) return fail(h, M2D_ERR_INVALID_ARG, e + ": null labels or general_memory");
    if (!isfinite(p->alpha)) return fail(h, M2D_ERR_INVALID_ARG, e + ": alpha is not finite");
    return M2D_OK;
}

// rows [n, W] into `out` (and 0 .. n-1 into `ids` unless null); the table scan, if one is queued, runs first: the kernel reads its word
int launch_compose(m2d_engine *h, const m2d_profile_batch *p, float *out, int32_t *ids, hipStream_t st)
{
    const int rc = m2d_ensure_finite_scan(h, st);
    if (rc != M2D_OK) return rc;
    ProfileArgs a;
    a.pm = h->pm; a.gm = p->general_memory; a.labels = p->labels; a.users = p->users; a.out = out; a.ids = ids;
    a.n = p->n; a.U = h->U; a.user_base = h->user_base; a.W = (h->C + 1) * h->E; a.L = p->L; a.alpha = p->alpha;
    a.err = h->err_dev; a.nonfinite = h->nonfinite_dev;
    const dim3 grid(m2d_blocks_for(h, p->n, 4));
    const bool vec = h->E % 4 == 0 && aligned16(a.gm) && aligned16(out);           // (Personal_Memory is aligned: m2d_create)
    const bool narrow = (vec ? a.W / 4 : a.W) <= 128;                              // two kept columns a lane cover the row
    if (vec && narrow) hipLaunchKernelGGL((m2d_compose_profiles_kernel<true, 2>), grid, dim3(256), 0, st, a);
    else if (vec) hipLaunchKernelGGL((m2d_compose_profiles_kernel<true, KEEP>), grid, dim3(256), 0, st, a);
    else if (narrow) hipLaunchKernelGGL((m2d_compose_profiles_kernel<false, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((m2d_compose_profiles_kernel<false, KEEP>), grid, dim3(256), 0, st, a);
    M2D_HIP_TRY(h, hipGetLastError());
    return M2D_OK;
}

// the serving calls' first half: scan, scratch, rows and ids.  `ids` are the users of the view.
int compose_to_scratch(m2d_engine *h, const m2d_profile_batch *p, const int32_t *&ids, hipStream_t st)
{
    const size_t rows = (size_t)p->n * (h->C + 1) * h->E;
    int rc = h->profile_buf.grow(h, rows + (size_t)p->n);
    if (rc != M2D_OK) return rc;
    int32_t *made = reinterpret_cast<int32_t *>(h->profile_buf + rows);
    if ((rc = launch_compose(h, p, h->profile_buf, made, st)) != M2D_OK) return rc;
    ids = made;
    return M2D_OK;
}

// a refusal of the launcher behind a profile call names the profile call
int renamed(m2d_engine *h, const int rc, const char *from, const char *to)
{
    const size_t len = strlen(from);
    if (rc != M2D_OK && h->last_error.compare(0, len, from) == 0 && (h->last_error.size() == len || h->last_error[len] == ':'))
        h->last_error.replace(0, len, to);
    return rc;
}

}  // namespace

extern "C" {

int m2d_compose_profiles(m2d_engine *h, const m2d_profile_batch *p, float *out_rows, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    const int rc = check_batch(h, "m2d_compose_profiles", p);
    if (rc != M2D_OK) return rc;
    if (!out_rows) return fail(h, M2D_ERR_INVALID_ARG, "m2d_compose_profiles: null buffer");
    if (p->n == 0) return M2D_OK;
    M2D_HIP_TRY(h, hipSetDevice(h->device));
    return launch_compose(h, p, out_rows, nullptr, (hipStream_t)stream);
}

int m2d_topk_profiles(m2d_engine *h, const m2d_profile_batch *p, int32_t k, const int64_t *excl_off, const int32_t *excl_ids,
                      float *out_scores, int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    int rc = check_batch(h, "m2d_topk_profiles", p);
    if (rc != M2D_OK) return rc;
    const int kmax = excl_off ? 16 : 64;
    if (k < 1 || k > kmax || (int64_t)k > h->I)
        return fail(h, M2D_ERR_INVALID_ARG, excl_off ? "m2d_topk_profiles: with exclusions need 1 <= k <= min(16, I)"
                                                     : "m2d_topk_profiles: need 1 <= k <= min(64, I)");
    if (!out_scores || !out_ids || (excl_off && !excl_ids)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_topk_profiles: null buffer");
    if (p->n == 0) return M2D_OK;
    if (!h->dish_cats) return fail(h, M2D_ERR_NOT_CONFIGURED, "m2d_topk_profiles: call m2d_set_dish_categories first");
    M2D_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)stream;
    const int32_t *ids = nullptr;
    if ((rc = compose_to_scratch(h, p, ids, st)) != M2D_OK) return rc;
    m2d_rows_view view(h, h->profile_buf, p->n);
    if (excl_off)
        return m2d_launch_topk_users_excluding(h, ids, p->n, k, excl_off, excl_ids, out_scores, out_ids, st, "m2d_topk_profiles");
    return renamed(h, m2d_launch_topk_users(h, ids, p->n, k, out_scores, out_ids, st), "m2d_topk_users", "m2d_topk_profiles");
}

int m2d_score_profiles(m2d_engine *h, const m2d_profile_batch *p, const int32_t *rows, const int32_t *items, int64_t B, float *out,
                       void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    int rc = check_batch(h, "m2d_score_profiles", p);
    if (rc != M2D_OK) return rc;
    if (B < 0) return fail(h, M2D_ERR_INVALID_ARG, "m2d_score_profiles: negative batch");
    if (B > 0 && (!rows || !items || !out)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_score_profiles: null buffer");
    if (p->n == 0 || B == 0) return M2D_OK;
    if (!h->dish_cats) return fail(h, M2D_ERR_NOT_CONFIGURED, "m2d_score_profiles: call m2d_set_dish_categories first");
    M2D_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)stream;
    const int32_t *ids = nullptr;
    if ((rc = compose_to_scratch(h, p, ids, st)) != M2D_OK) return rc;
    m2d_rows_view view(h, h->profile_buf, p->n);
    return m2d_launch_score_pairs(h, rows, items, h->dish_cats, true, B, out, st);
}

int m2d_topk_markets_profiles(m2d_engine *h, const m2d_profile_batch *p, const int64_t *market_off, const int32_t *market_ids,
                              int64_t nnzM, const int64_t *excl_off, const int32_t *excl_ids, int32_t k, int32_t max_missing,
                              float *out_scores, int32_t *out_ids, int32_t *out_counts, int32_t *out_missing, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    int rc = check_batch(h, "m2d_topk_markets_profiles", p);
    if (rc != M2D_OK) return rc;
    if (nnzM < 0 || k < 1 || k > 64 || max_missing < 0)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_topk_markets_profiles: need nnzM >= 0, 1 <= k <= 64 and max_missing >= 0");
    if (!market_off || (!market_ids && nnzM > 0) || !out_scores || !out_ids)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_topk_markets_profiles: null buffer");
    if (p->n == 0) return M2D_OK;
    if (!h->rcp_set) return fail(h, M2D_ERR_NOT_CONFIGURED, "m2d_topk_markets_profiles: call m2d_set_recipes first");
    if (!h->dish_cats) return fail(h, M2D_ERR_NOT_CONFIGURED, "m2d_topk_markets_profiles: call m2d_set_dish_categories first");
    if (h->ing) return fail(h, M2D_ERR_UNSUPPORTED, "m2d_topk_markets_profiles: the ingredient table is set");
    if (h->mlp_w1) return fail(h, M2D_ERR_UNSUPPORTED, "m2d_topk_markets_profiles: the MLP head is set");
    M2D_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)stream;
    const int32_t *ids = nullptr;
    if ((rc = compose_to_scratch(h, p, ids, st)) != M2D_OK) return rc;
    m2d_rows_view view(h, h->profile_buf, p->n);
    return renamed(h, m2d_launch_topk_markets(h, ids, p->n, market_off, market_ids, nnzM, k, max_missing, out_scores, out_ids, out_counts,
                                              st, excl_off, excl_ids, out_missing),
                   "m2d_topk_markets", "m2d_topk_markets_profiles");
}

}  // extern "C"
