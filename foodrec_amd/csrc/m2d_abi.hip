// extern "C" surface of libm2d.so -- see include/m2d.h for the contract and the reference
// interfaces each entry point replaces.  No exceptions cross this boundary.
#include <string.h>
#include <time.h>

#include <new>

#include "m2d_engine.h"

namespace {

// plain streaming read: 4 x 16 B in flight per lane, non-temporal, the four loads a whole grid stride apart, TWO workgroups per CU.
// Round 6 sweep on MI355X over the 1.28 GB Personal_Memory (profiles/r06_stream_probe_sweep.txt):
// this form 6 970-7 000 GB/s at 2-3 workgroups per CU against 5 560-5 840 at 4-16 (round 1-5's launch: 8 per CU), 6 250 at 32;
// plain loads 6 310 at 2 per CU; block-contiguous slices (4 or 8 x 16 B per lane) 6 610-6 740 at 2 per CU.
__global__ __launch_bounds__(256) void m2d_stream_read(const v4f *p, int64_t n4, float *sink)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const v4f a = __builtin_nontemporal_load(p + i);
        const v4f b = __builtin_nontemporal_load(p + i + stride);
        const v4f c = __builtin_nontemporal_load(p + i + 2 * stride);
        const v4f d = __builtin_nontemporal_load(p + i + 3 * stride);
        acc += (a + b) + (c + d);
    }
    for (; i < n4; i += stride) acc += __builtin_nontemporal_load(p + i);
    const float s = (acc.x + acc.y) + (acc.z + acc.w);
    if (s == 123456.789f) sink[0] = s;   // keeps the loads live; practically never true
}

// x * 0 is 0 for every finite x and NaN for inf / NaN: one fma per value, the lane's sum is NaN iff it met one
__global__ __launch_bounds__(256) void m2d_scan_nonfinite(const float *p, int64_t n, int32_t *flag)
{
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    const v4f *p4 = reinterpret_cast<const v4f *>(p);
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const v4f a = __builtin_nontemporal_load(p4 + i);
        const v4f b = __builtin_nontemporal_load(p4 + i + stride);
        const v4f c = __builtin_nontemporal_load(p4 + i + 2 * stride);
        const v4f d = __builtin_nontemporal_load(p4 + i + 3 * stride);
        acc += (a * 0.f + b * 0.f) + (c * 0.f + d * 0.f);
    }
    for (; i < n4; i += stride) acc += __builtin_nontemporal_load(p4 + i) * 0.f;
    float s = (acc.x + acc.y) + (acc.z + acc.w);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) s += p[(n4 << 2) + threadIdx.x] * 0.f;
    if (s != s) *flag = 1;
}

// H[d] of the ingredient table: +-inf only.  A NaN row (a dish without ingredients, 0 / 0) is NaN in every form of every kernel;
// an inf is not -- the split-bf16 retrieval rows hold hi = inf and lo = inf - inf = NaN where the product with U_high is +-inf
__global__ __launch_bounds__(256) void m2d_scan_inf(const float *p, int64_t n, int32_t *flag)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool hit = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) hit = hit || __builtin_isinf(p[i]);
    if (hit) *flag = 1;
}

// the Personal_Memory blocks of a batch's users (after a writer that adds into them with atomics)
__global__ __launch_bounds__(256) void m2d_rows_nonfinite(const float *pm, const int32_t *users, int64_t B, int64_t U, int64_t user_base,
                                                          int32_t W, int32_t *flag)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    float s = 0.f;
    for (int64_t b = wave0; b < B; b += nwaves) {
        const int64_t ul = (int64_t)users[b] - user_base;
        if (ul < 0 || ul >= U) continue;                     // reported by the writer itself
        const float *row = pm + (size_t)ul * W;
        for (int e = lane; e < W; e += 64) s += row[e] * 0.f;
    }
    if (s != s) *flag = 1;
}

std::string g_create_error;

int fail(m2d_engine *h, int code, const char *msg)
{
    if (h) h->last_error = msg; else g_create_error = msg;
    return code;
}
int fail(m2d_engine *h, int code, const std::string &msg) { return fail(h, code, msg.c_str()); }

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool table_flags_ok(const int flags) { return flags == M2D_TABLES_HOST || flags == M2D_TABLES_DEVICE; }
// what a setter can judge before it replaces anything: a BORROWED array that the kernels read 16 bytes at a time must be aligned
// (the engine's own copies are hipMalloc's, checked after they are made)
bool borrowed_misaligned(const void *p, const int flags) { return flags == M2D_TABLES_DEVICE && !aligned16(p); }

// copy a host table to HBM (engine-owned) or borrow a device pointer; a null `src` or no entries: no copy
template <typename T> int adopt(m2d_engine *h, const T *src, const size_t count, const int flags, m2d_table<T> &t)
{
    t.reset();
    if (flags == M2D_TABLES_DEVICE || !src) {
        t.p = src;
        return M2D_OK;
    }
    if (int rc = t.own.grow(h, count)) return rc;
    const hipError_t e = hipMemcpy(t.own, src, count * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        t.reset();
        return fail(h, M2D_ERR_HIP, std::string("hipMemcpy(table): ") + hipGetErrorString(e));
    }
    t.p = t.own;
    return M2D_OK;
}

// ---- what the entry points ask for before they launch, each check named once.  enter() runs them in the one order every entry
// point uses -- recipes, head, dish masks, "plain scores only", then the engine's device -- and returns the refusal, if any.
#define M2D_REQUIRE(expr)                                                                      \
    do {                                                                                       \
        if (const int rc_ = (expr)) return rc_;                                                \
    } while (0)

enum : unsigned { NEEDS_MASKS = 1, NEEDS_HEAD = 2, NEEDS_RECIPES = 4, PLAIN_SCORES_ONLY = 8 };

int enter(m2d_engine *h, const unsigned needs = 0, const char *entry = "")
{
    if ((needs & NEEDS_RECIPES) && !h->rcp_set) return fail(h, M2D_ERR_NOT_CONFIGURED, "call m2d_set_recipes first");
    if ((needs & NEEDS_HEAD) && !h->mlp_w1) return fail(h, M2D_ERR_NOT_CONFIGURED, "call m2d_set_mlp_head first");
    if ((needs & NEEDS_MASKS) && !h->dish_cats) return fail(h, M2D_ERR_NOT_CONFIGURED, "call m2d_set_dish_categories first");
    if ((needs & PLAIN_SCORES_ONLY) && h->ing) return fail(h, M2D_ERR_UNSUPPORTED, std::string(entry) + ": the ingredient table is set");
    if ((needs & PLAIN_SCORES_ONLY) && h->mlp_w1) return fail(h, M2D_ERR_UNSUPPORTED, std::string(entry) + ": the MLP head is set");
    M2D_HIP_TRY(h, hipSetDevice(h->device));
    return M2D_OK;
}

int null_buffer(m2d_engine *h, const char *entry) { return fail(h, M2D_ERR_INVALID_ARG, std::string(entry) + ": null buffer"); }
int negative_batch(m2d_engine *h, const char *entry) { return fail(h, M2D_ERR_INVALID_ARG, std::string(entry) + ": negative batch"); }

// "need nU >= 0 and 1 <= k <= min(limit, I)" of the catalogue top-k calls
int topk_range(m2d_engine *h, const char *entry, const int64_t nU, const int32_t k, const int limit)
{
    if (nU >= 0 && k >= 1 && k <= limit && (int64_t)k <= h->I) return M2D_OK;
    return fail(h, M2D_ERR_INVALID_ARG, std::string(entry) + ": need nU >= 0 and 1 <= k <= min(" + std::to_string(limit) + ", I)");
}

// "candidates must be 0 (exact) or k <= candidates <= min(limit, I)" of the calls under the head
int candidates_range(m2d_engine *h, const char *entry, const int32_t k, const int32_t candidates, const int limit, const char *when = "")
{
    if (candidates == 0 || (candidates >= k && candidates <= limit && (int64_t)candidates <= h->I)) return M2D_OK;
    return fail(h, M2D_ERR_INVALID_ARG, std::string(entry) + ": " + when + "candidates must be 0 (exact) or k <= candidates <= min(" +
                                            std::to_string(limit) + ", I)");
}

}  // namespace

// The scan queued by m2d_create / m2d_tables_updated / m2d_set_ingredients / m2d_clear_ingredients: one streaming pass over the
// three tables, and over H[d] when the ingredient table is set, on the caller's stream, in front of the launch that needs its
// answer (1.28 GB of Personal_Memory: 0.2 ms, once per table change).
int m2d_ensure_finite_scan(m2d_engine *h, hipStream_t st)
{
    if (!h->finite_scan_pending) return M2D_OK;
    M2D_HIP_TRY(h, hipMemsetAsync(h->nonfinite_dev, 0, sizeof(int32_t), st));
    const float *t[3] = {h->pm, h->re, h->ce};
    for (int i = 0; i < 3; ++i) {
        const int64_t n = m2d_table_floats(h, i);
        hipLaunchKernelGGL(m2d_scan_nonfinite, dim3(m2d_blocks_for(h, n / 4, 1024)), dim3(256), 0, st, t[i], n, h->nonfinite_dev);
    }
    if (h->dish_high) {                 // (set / cleared by m2d_set_ingredients / m2d_clear_ingredients, which queue this scan again)
        const int64_t nh = h->I * (int64_t)h->E;
        hipLaunchKernelGGL(m2d_scan_inf, dim3(m2d_blocks_for(h, nh, 1024)), dim3(256), 0, st, h->dish_high, nh, h->nonfinite_dev);
    }
    M2D_HIP_TRY(h, hipGetLastError());
    h->grp_nonfinite_known = false;     // the retrieval launcher's host copy of the word
    h->finite_scan_pending = false;
    return M2D_OK;
}

int m2d_launch_rows_finite_check(m2d_engine *h, const int32_t *users, int64_t B, hipStream_t st)
{
    if (B <= 0) return M2D_OK;
    hipLaunchKernelGGL(m2d_rows_nonfinite, dim3(m2d_blocks_for(h, B, 4)), dim3(256), 0, st, h->pm, users, B, h->U, h->user_base,
                       (h->C + 1) * h->E, h->nonfinite_dev);
    M2D_HIP_TRY(h, hipGetLastError());
    return M2D_OK;
}

extern "C" {

int m2d_abi_version(void) { return 2; }

int m2d_create(const float *pm, const float *re, const float *ce, int64_t U, int64_t I, int32_t C, int32_t E,
               float coef, int device, int table_flags, m2d_engine **out)
{
    if (!out) return fail(nullptr, M2D_ERR_INVALID_ARG, "m2d_create: out is null");
    *out = nullptr;
    if (!pm || !re || !ce) return fail(nullptr, M2D_ERR_INVALID_ARG, "m2d_create: null table pointer");
    if (U <= 0 || I <= 0 || C <= 0 || E <= 0)
        return fail(nullptr, M2D_ERR_INVALID_ARG, "m2d_create: U, I, C, E must be positive");
    if (I > INT32_MAX || U > (int64_t)INT32_MAX)
        return fail(nullptr, M2D_ERR_UNSUPPORTED, "m2d_create: ids are int32 (Model_Recommender.py:26-29)");
    if (!table_flags_ok(table_flags)) return fail(nullptr, M2D_ERR_INVALID_ARG, "m2d_create: bad table_flags");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, M2D_ERR_NO_DEVICE,
                    "m2d_create: no HIP device visible (this engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, M2D_ERR_INVALID_ARG, "m2d_create: bad device index");
    m2d_engine *h = new (std::nothrow) m2d_engine();
    if (!h) return fail(nullptr, M2D_ERR_HIP, "m2d_create: out of host memory");
    h->U = U; h->I = I; h->C = C; h->E = E; h->device = device;
    h->a = coef;            // float32(coef)               Model_Recommender.py:17
    h->b = 1.0f - h->a;     // evaluated in float32        Model_Recommender.py:96
    int rc = M2D_OK;
    auto bail = [&](int code) {         // (the engine's device is current, or no device call has succeeded)
        g_create_error = h->last_error;
        delete h;
        return code;
    };
    if (hipSetDevice(device) != hipSuccess) { h->last_error = "hipSetDevice failed"; return bail(M2D_ERR_HIP); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        h->num_cu = prop.multiProcessorCount;
    if ((rc = adopt(h, pm, (size_t)U * (C + 1) * E, table_flags, h->pm)) != M2D_OK) return bail(rc);
    if ((rc = adopt(h, re, (size_t)I * E, table_flags, h->re)) != M2D_OK) return bail(rc);
    if ((rc = adopt(h, ce, (size_t)C * E, table_flags, h->ce)) != M2D_OK) return bail(rc);
    if (!aligned16(h->pm) || !aligned16(h->re) || !aligned16(h->ce)) {
        h->last_error = "m2d_create: device tables must be 16-byte aligned";
        return bail(M2D_ERR_INVALID_ARG);
    }
    if (h->err_dev.grow(h, 8) != M2D_OK ||                                          // id-error latch [4] | non-finite word | the bf16 mirror's | pad
        hipMemset(h->err_dev, 0, 8 * sizeof(int32_t)) != hipSuccess || h->err_host.alloc(h, 4) != M2D_OK) {
        h->last_error = "m2d_create: could not allocate the error latch";
        return bail(M2D_ERR_HIP);
    }
    h->nonfinite_dev = h->err_dev + 4;
    h->pm_bf16_nonfinite = h->err_dev + 5;
    h->finite_scan_pending = true;      // the first scoring call scans the tables on its stream
    *out = h;
    return M2D_OK;
}

int m2d_destroy(m2d_engine *h)
{
    if (!h) return M2D_OK;
    (void)hipSetDevice(h->device);
    delete h;
    return M2D_OK;
}

const char *m2d_last_error(const m2d_engine *h) { return h ? h->last_error.c_str() : g_create_error.c_str(); }

const char *m2d_last_kernel(const m2d_engine *h) { return h ? h->last_kernel : ""; }

int m2d_set_user_base(m2d_engine *h, int64_t user_base)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (user_base < 0 || user_base + h->U > (int64_t)INT32_MAX + 1)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_set_user_base: shard range leaves int32");
    h->user_base = user_base;
    return M2D_OK;
}

// (failure contract: m2d.h, "Setters")
int m2d_set_dish_categories(m2d_engine *h, const float *cats, int table_flags)
{
    if (!h || !cats) return fail(h, M2D_ERR_INVALID_ARG, "m2d_set_dish_categories: null argument");
    if (!table_flags_ok(table_flags)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_set_dish_categories: bad table_flags");
    if (borrowed_misaligned(cats, table_flags)) return fail(h, M2D_ERR_INVALID_ARG, "dish categories must be 16-byte aligned");
    M2D_REQUIRE(enter(h));
    h->dish_cats.reset();               // replacement begins: from here on a failure leaves no table
    m2d_mark_written(h, M2D_TAB_MASKS, M2D_NO_VALUES);
    m2d_table<float> t;
    M2D_REQUIRE(adopt(h, cats, (size_t)h->I * h->C, table_flags, t));
    if (!aligned16(t)) return fail(h, M2D_ERR_INVALID_ARG, "dish categories must be 16-byte aligned");
    h->dish_cats = std::move(t);
    return M2D_OK;
}

int m2d_score_pairs(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats, int64_t B,
                    float *out, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (B < 0) return negative_batch(h, "m2d_score_pairs");
    if (B == 0) return M2D_OK;
    if (!users || !items || !cats || !out) return null_buffer(h, "m2d_score_pairs");
    if (h->C == 4 && !aligned16(cats)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_score_pairs: cats must be 16-byte aligned");
    M2D_REQUIRE(enter(h));
    return m2d_launch_score_pairs(h, users, items, cats, false, B, out, (hipStream_t)stream);
}

// Host-buffer form of m2d_score_pairs: what the reference's own call site hands over (numpy / lists, 51 pairs per
// sess.run, evaluate.py:55-59).  One pinned staging block [users | items | cats | out | err], one H2D copy, the
// kernel, one D2H copy that brings the scores AND the id-error latch back, one synchronisation.
namespace {
__global__ void m2d_copy_latch(const int32_t *latch, int32_t *dst, int32_t *done, int32_t ticket)
{
    if (threadIdx.x < 4) dst[threadIdx.x] = latch[threadIdx.x];
    if (done) {                         // host-visible completion word, written after the latch (and after the scores,
        __threadfence_system();         // which the kernel before this one on the stream wrote)
        if (threadIdx.x == 0) __hip_atomic_store(done, ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
}  // namespace

namespace {
constexpr int64_t HOST_CHUNK = 1 << 18;

int ensure_stage(m2d_engine *h, size_t total, hipStream_t st)
{
    if (total <= h->stage_dev.cap) return M2D_OK;
    M2D_HIP_TRY(h, hipStreamSynchronize(st));
    h->stage_host.reset();
    h->stage_dev.reset();
    // the kernel writes scores, the id-error latch and the completion word into this block and the host polls the word:
    // host-coherent (fine-grained) and mapped, stated rather than left to the runtime's default / HIP_HOST_COHERENT
    M2D_REQUIRE(h->stage_host.alloc(h, total * 2, hipHostMallocCoherent | hipHostMallocMapped));
    return h->stage_dev.grow(h, total * 2);
}

// Feeds of more than HOST_CHUNK pairs: chunks through two pinned blocks, so that the host's copy of chunk k + 1 into its
// block runs while chunk k is on the link and in the kernel (one block: the five steps of a call run one after another
// and the host-side copies are the longest of them).  Chunks retire in order; an id error is reported with the position
// in the whole feed, and the scores of the chunks before the offending one have then been delivered.
int score_pairs_host_chunked(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats, int64_t B,
                             float *out, hipStream_t st)
{
    const int C = h->C;
    const size_t in_b = (size_t)HOST_CHUNK * C * 4 + 2 * (size_t)HOST_CHUNK * 4, out_b = (size_t)HOST_CHUNK * 4 + 16;
    const size_t blk = in_b + out_b;
    // an id error latched by an earlier, unchecked launch is reported as what it is -- with that call's position -- before
    // anything of this feed is queued (the latch keeps the first error; a chunk's position arithmetic below must only
    // ever see an error of its own chunk)
    int rc = m2d_check(h, (void *)st, nullptr, nullptr);
    if (rc != M2D_OK) return rc;
    if ((rc = ensure_stage(h, 2 * blk, st)) != M2D_OK) return rc;
// a HIP error inside the loop: nothing may stay in flight on the two pinned blocks when the call returns
#define M2D_CHUNK_TRY(expr)                                                                    \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            h->last_error = std::string(#expr) + ": " + hipGetErrorString(e_);                 \
            (void)hipStreamSynchronize(st);                                                    \
            return M2D_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)
    for (m2d_event &ev : h->stage_ev)
        if (!ev.e) M2D_HIP_TRY(h, hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
    const int64_t nch = (B + HOST_CHUNK - 1) / HOST_CHUNK;
    auto retire = [&](int64_t k) -> int {
        unsigned char *hs = h->stage_host + (size_t)(k & 1) * blk;
        M2D_CHUNK_TRY(hipEventSynchronize(h->stage_ev[k & 1]));
        const int32_t *err = reinterpret_cast<const int32_t *>(hs + in_b + (size_t)HOST_CHUNK * 4);
        if (err[0] != 0) {
            // the kernel latched a position inside its chunk: put the position in the feed there before reporting it
            const int64_t idx = (((int64_t)(uint32_t)err[3] << 32) | (uint32_t)err[2]) + k * HOST_CHUNK;
            int32_t *fixed = reinterpret_cast<int32_t *>(hs);                   // pinned; the block is not in use any more
            fixed[0] = err[0]; fixed[1] = err[1]; fixed[2] = (int32_t)(idx & 0xffffffff); fixed[3] = (int32_t)(idx >> 32);
            M2D_CHUNK_TRY(hipMemcpyAsync(h->err_dev, fixed, 16, hipMemcpyHostToDevice, st));
            return m2d_check(h, (void *)st, nullptr, nullptr);                  // synchronises, formats, clears the latch
        }
        const int64_t n = B - k * HOST_CHUNK < HOST_CHUNK ? B - k * HOST_CHUNK : HOST_CHUNK;
        memcpy(out + k * HOST_CHUNK, hs + in_b, (size_t)n * 4);
        return M2D_OK;
    };
    for (int64_t k = 0; k < nch; ++k) {
        if (k >= 2 && (rc = retire(k - 2)) != M2D_OK) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
        unsigned char *hs = h->stage_host + (size_t)(k & 1) * blk, *ds = h->stage_dev + (size_t)(k & 1) * blk;
        const int64_t o = k * HOST_CHUNK, n = B - o < HOST_CHUNK ? B - o : HOST_CHUNK;
        const size_t o_u = (size_t)HOST_CHUNK * C * 4, o_i = o_u + (size_t)HOST_CHUNK * 4;
        memcpy(hs, cats + o * C, (size_t)n * C * 4);
        memcpy(hs + o_u, users + o, (size_t)n * 4);
        memcpy(hs + o_i, items + o, (size_t)n * 4);
        M2D_CHUNK_TRY(hipMemcpyAsync(ds, hs, (size_t)n * C * 4, hipMemcpyHostToDevice, st));
        M2D_CHUNK_TRY(hipMemcpyAsync(ds + o_u, hs + o_u, (size_t)n * 4, hipMemcpyHostToDevice, st));
        M2D_CHUNK_TRY(hipMemcpyAsync(ds + o_i, hs + o_i, (size_t)n * 4, hipMemcpyHostToDevice, st));
        rc = m2d_launch_score_pairs(h, reinterpret_cast<const int32_t *>(ds + o_u), reinterpret_cast<const int32_t *>(ds + o_i),
                                    reinterpret_cast<const float *>(ds), false, n, reinterpret_cast<float *>(ds + in_b), st);
        if (rc != M2D_OK) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
        hipLaunchKernelGGL(m2d_copy_latch, dim3(1), dim3(64), 0, st, h->err_dev,
                           reinterpret_cast<int32_t *>(ds + in_b + (size_t)HOST_CHUNK * 4), (int32_t *)nullptr, 0);
        M2D_CHUNK_TRY(hipGetLastError());
        M2D_CHUNK_TRY(hipMemcpyAsync(hs + in_b, ds + in_b, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        M2D_CHUNK_TRY(hipMemcpyAsync(hs + in_b + (size_t)HOST_CHUNK * 4, ds + in_b + (size_t)HOST_CHUNK * 4, 16, hipMemcpyDeviceToHost, st));
        M2D_CHUNK_TRY(hipEventRecord(h->stage_ev[k & 1], st));
    }
    for (int64_t k = nch >= 2 ? nch - 2 : 0; k < nch; ++k)
        if ((rc = retire(k)) != M2D_OK) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
    return M2D_OK;
#undef M2D_CHUNK_TRY
}
}  // namespace

int m2d_score_pairs_host(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats, int64_t B,
                         float *out, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (B < 0) return negative_batch(h, "m2d_score_pairs_host");
    if (B == 0) return M2D_OK;
    if (!users || !items || !cats || !out) return null_buffer(h, "m2d_score_pairs_host");
    hipStream_t st = (hipStream_t)stream;
    M2D_REQUIRE(enter(h));
    if (B > HOST_CHUNK && h->opt_host_zero_copy != 0) return score_pairs_host_chunked(h, users, items, cats, B, out, st);
    const int C = h->C;
    // layout (16-byte aligned sections): cats [B, C] | users [B] | items [B] || out [B] | err [4] | completion word
    const size_t nb = ((size_t)B + 3) & ~(size_t)3;
    const size_t in_bytes = nb * C * 4 + 2 * nb * 4, out_bytes = nb * 4 + 16, total = in_bytes + out_bytes + 16;
    M2D_REQUIRE(ensure_stage(h, total, st));
    unsigned char *hs = h->stage_host, *ds = h->stage_dev;
    memcpy(hs, cats, (size_t)B * C * 4);
    memcpy(hs + nb * C * 4, users, (size_t)B * 4);
    memcpy(hs + nb * C * 4 + nb * 4, items, (size_t)B * 4);
    // Small feeds (the reference's 51 pairs per call, evaluate.py:55-59): the kernel reads the pinned block and writes the
    // scores into it over the host link -- two launches and one synchronisation, no copy engine round trips.
    unsigned char *ws = ds;
    if (h->opt_host_zero_copy && B <= 65536) {
        void *mapped = nullptr;
        M2D_HIP_TRY(h, hipHostGetDevicePointer(&mapped, hs, 0));
        ws = static_cast<unsigned char *>(mapped);
    } else {
        M2D_HIP_TRY(h, hipMemcpyAsync(ds, hs, in_bytes, hipMemcpyHostToDevice, st));
    }
    const int rc = m2d_launch_score_pairs(h, reinterpret_cast<const int32_t *>(ws + nb * C * 4),
                                          reinterpret_cast<const int32_t *>(ws + nb * C * 4 + nb * 4),
                                          reinterpret_cast<const float *>(ws), false, B, reinterpret_cast<float *>(ws + in_bytes), st);
    if (rc != M2D_OK) return rc;
    // the latch rides back behind the scores: put it next to them first (16 B, same stream)
    const bool poll = ws != ds && h->opt_host_zero_copy >= 2;
    int32_t *done_dev = poll ? reinterpret_cast<int32_t *>(ws + in_bytes + nb * 4 + 16) : nullptr;
    volatile int32_t *done_host = reinterpret_cast<volatile int32_t *>(hs + in_bytes + nb * 4 + 16);
    const int32_t ticket = (int32_t)++h->stage_ticket;
    if (poll) *done_host = (int32_t)(h->stage_ticket - 1u);
    hipLaunchKernelGGL(m2d_copy_latch, dim3(1), dim3(64), 0, st, h->err_dev, reinterpret_cast<int32_t *>(ws + in_bytes + nb * 4),
                       done_dev, ticket);
    M2D_HIP_TRY(h, hipGetLastError());
    if (ws == ds) M2D_HIP_TRY(h, hipMemcpyAsync(hs + in_bytes, ds + in_bytes, out_bytes, hipMemcpyDeviceToHost, st));
    bool seen = false;
    if (poll) {
        // spin on the completion word (a stream synchronisation costs more than the two kernels), for at most 250 us of
        // wall time -- a 65 536-pair feed, the largest that takes this path, is done in ~0.1 ms -- then wait on the stream
        timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (;;) {
            for (int spin = 0; spin < 256 && !seen; ++spin)
                seen = __atomic_load_n(const_cast<const int32_t *>(done_host), __ATOMIC_ACQUIRE) == ticket;
            if (seen) break;
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec) > 250000ll) break;
        }
    }
    if (!seen) M2D_HIP_TRY(h, hipStreamSynchronize(st));
    const int32_t *err = reinterpret_cast<const int32_t *>(hs + in_bytes + nb * 4);
    if (err[0] != 0) return m2d_check(h, stream, nullptr, nullptr);     // formats the message, clears the latch
    memcpy(out, hs + in_bytes, (size_t)B * 4);
    return M2D_OK;
}

int m2d_score_pairs_bydish(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t B, float *out,
                           void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (B < 0) return negative_batch(h, "m2d_score_pairs_bydish");
    if (B == 0) return M2D_OK;
    if (!users || !items || !out) return null_buffer(h, "m2d_score_pairs_bydish");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    return m2d_launch_score_pairs(h, users, items, h->dish_cats, true, B, out, (hipStream_t)stream);
}

// m2d_rank_candidates and m2d_rank_candidates_mlp
static int rank_candidates(m2d_engine *h, const char *entry, const bool head, const int32_t *users, const int32_t *items, const int32_t *lens,
                           int64_t nseg, int32_t L, int32_t k, float *out_scores, int32_t *out_items, int32_t *out_flags, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (nseg < 0 || L < 1 || L > 1024 || k < 1 || k > 64)
        return fail(h, M2D_ERR_INVALID_ARG, std::string(entry) + ": need nseg >= 0, 1 <= L <= 1024, 1 <= k <= 64");
    if (nseg == 0) return M2D_OK;
    if (!users || !items || !out_scores || !out_items || !out_flags) return null_buffer(h, entry);
    M2D_REQUIRE(enter(h, head ? NEEDS_HEAD | NEEDS_MASKS : NEEDS_MASKS));
    return m2d_launch_rank_candidates(h, users, items, lens, nseg, L, k, out_scores, out_items, out_flags, (hipStream_t)stream, head);
}

int m2d_rank_candidates(m2d_engine *h, const int32_t *users, const int32_t *items, const int32_t *lens,
                        int64_t nseg, int32_t L, int32_t k, float *out_scores, int32_t *out_items,
                        int32_t *out_flags, void *stream)
{
    return rank_candidates(h, "m2d_rank_candidates", false, users, items, lens, nseg, L, k, out_scores, out_items, out_flags, stream);
}

int m2d_topk_users(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, float *out_scores,
                   int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    M2D_REQUIRE(topk_range(h, "m2d_topk_users", nU, k, 64));
    if (nU == 0) return M2D_OK;
    if (!users || !out_scores || !out_ids) return null_buffer(h, "m2d_topk_users");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    return m2d_launch_topk_users(h, users, nU, k, out_scores, out_ids, (hipStream_t)stream);
}

int m2d_catalogue_rank(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t n, const int64_t *excl_off,
                       const int32_t *excl_ids, int32_t *out_rank, float *out_scores, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (n < 0) return fail(h, M2D_ERR_INVALID_ARG, "m2d_catalogue_rank: need n >= 0");
    if (n == 0) return M2D_OK;
    if (!users || !items || !out_rank || (excl_off && !excl_ids)) return null_buffer(h, "m2d_catalogue_rank");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    return m2d_launch_catalogue_rank(h, users, items, n, excl_off, excl_ids, out_rank, out_scores, (hipStream_t)stream);
}

int m2d_topk_users_excluding(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int64_t *excl_off,
                             const int32_t *excl_ids, float *out_scores, int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    M2D_REQUIRE(topk_range(h, "m2d_topk_users_excluding", nU, k, 16));
    if (nU == 0) return M2D_OK;
    if (!users || !out_scores || !out_ids || (excl_off && !excl_ids)) return null_buffer(h, "m2d_topk_users_excluding");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    return m2d_launch_topk_users_excluding(h, users, nU, k, excl_off, excl_ids, out_scores, out_ids, (hipStream_t)stream);
}

int m2d_score_slate(m2d_engine *h, const int32_t *users, int64_t nU, const int32_t *slate, int64_t nD, float *out, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (nU < 0 || nD < 1 || nD > h->I) return fail(h, M2D_ERR_INVALID_ARG, "m2d_score_slate: need nU >= 0 and 1 <= nD <= I");
    if (nU == 0) return M2D_OK;
    if (!users || !slate || !out) return null_buffer(h, "m2d_score_slate");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    return m2d_launch_slate(h, "m2d_score_slate", users, nU, slate, nD, 0, out, nullptr, nullptr, (hipStream_t)stream);
}

int m2d_topk_slate(m2d_engine *h, const int32_t *users, int64_t nU, const int32_t *slate, int64_t nD, int32_t k, float *out_scores,
                   int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (nU < 0 || nD < 1 || nD > h->I || k < 1 || k > 64 || (int64_t)k > nD)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_topk_slate: need nU >= 0, 1 <= nD <= I and 1 <= k <= min(64, nD)");
    if (nU == 0) return M2D_OK;
    if (!users || !slate || !out_scores || !out_ids) return null_buffer(h, "m2d_topk_slate");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    return m2d_launch_slate(h, "m2d_topk_slate", users, nU, slate, nD, k, nullptr, out_scores, out_ids, (hipStream_t)stream);
}

int m2d_clear_ingredients(m2d_engine *h)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    h->ing.reset(); h->ing_off.reset(); h->ing_ids.reset(); h->ing_w.reset(); h->dish_high.reset();
    h->ing_rows = 0; h->ing_nnz = 0;
    m2d_mark_written(h, M2D_TAB_ING, M2D_BY_CALLER);       // H[d] was part of the scan
    return M2D_OK;
}

// (failure contract: m2d.h, "Setters".  None of the four arrays has an alignment rule, so nothing of a borrowed one is refused.)
int m2d_set_ingredients(m2d_engine *h, const float *ing, int64_t R, const int32_t *off, const int32_t *ids,
                        const float *w, int64_t nnz, int table_flags)
{
    if (!h || !ing || !off || (!ids && nnz > 0) || R <= 0 || nnz < 0 || nnz > INT32_MAX)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_set_ingredients: bad argument");
    if (!table_flags_ok(table_flags)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_set_ingredients: bad table_flags");
    // an id error latched by an earlier launch is reported as what it is, before the CSR check can mislabel it
    M2D_REQUIRE(m2d_check(h, nullptr, nullptr, nullptr));
    M2D_REQUIRE(m2d_clear_ingredients(h));      // replacement begins: from here on a failure leaves no ingredient table
    M2D_REQUIRE(enter(h));
    m2d_table<float> t_ing, t_w;
    m2d_table<int32_t> t_off, t_ids;
    m2d_dev_buf<float> high;
    M2D_REQUIRE(adopt(h, ing, (size_t)R * h->E, table_flags, t_ing));
    M2D_REQUIRE(adopt(h, off, (size_t)h->I + 1, table_flags, t_off));
    M2D_REQUIRE(adopt(h, ids, (size_t)nnz, table_flags, t_ids));
    M2D_REQUIRE(adopt(h, w, (size_t)nnz, table_flags, t_w));
    M2D_REQUIRE(high.grow(h, (size_t)h->I * h->E));
    if (!aligned16(high)) return fail(h, M2D_ERR_HIP, "dish_high not aligned");
    M2D_REQUIRE(m2d_launch_check_csr(h, t_off, nnz, nullptr));
    if (m2d_check(h, nullptr, nullptr, nullptr) != M2D_OK)
        return fail(h, M2D_ERR_BAD_INGREDIENT,
                    "m2d_set_ingredients: offsets are not a CSR row pointer (off[0] = 0, non-decreasing, off[I] = nnz)");
    M2D_REQUIRE(m2d_launch_build_dish_high(h, t_ing, t_off, t_ids, t_w, R, high, nullptr));
    if (m2d_check(h, nullptr, nullptr, nullptr) != M2D_OK) return fail(h, M2D_ERR_BAD_INGREDIENT, "m2d_set_ingredients: " + h->last_error);
    h->ing = std::move(t_ing); h->ing_off = std::move(t_off); h->ing_ids = std::move(t_ids); h->ing_w = std::move(t_w);
    h->dish_high = std::move(high);
    h->ing_rows = R;
    h->ing_nnz = nnz;
    m2d_mark_written(h, M2D_TAB_ING, M2D_BY_CALLER);       // H[d] is part of the scan
    return M2D_OK;
}

int m2d_clear_recipes(m2d_engine *h)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    h->rcp_off.reset(); h->rcp_ids.reset();
    h->rcp_set = false; h->rcp_rows = 0; h->rcp_nnz = 0;
    return M2D_OK;
}

// (failure contract: m2d.h, "Setters")
int m2d_set_recipes(m2d_engine *h, int64_t R, const int32_t *off, const int32_t *ids, int64_t nnz, int32_t flags)
{
    if (!h || !off || (!ids && nnz > 0) || R < 1 || R > INT32_MAX || nnz < 0 || nnz > INT32_MAX)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_set_recipes: bad argument (need 1 <= R, 0 <= nnz, both within int32, offsets, and ids where nnz > 0)");
    if (!table_flags_ok(flags)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_set_recipes: bad flags");
    // an id error latched by an earlier launch is reported as what it is, before the checks below can mislabel it
    M2D_REQUIRE(m2d_check(h, nullptr, nullptr, nullptr));
    M2D_REQUIRE(m2d_clear_recipes(h));          // replacement begins: from here on a failure leaves no recipes
    M2D_REQUIRE(enter(h));
    m2d_table<int32_t> t_off, t_ids;
    M2D_REQUIRE(adopt(h, off, (size_t)h->I + 1, flags, t_off));
    M2D_REQUIRE(adopt(h, ids, (size_t)nnz, flags, t_ids));
    // the row pointer first: the id pass reads ids[0, nnz) only, but nothing may call the lists valid before both have passed
    // (a failure that is not the check's own finding -- a HIP error -- keeps its code)
    auto refused = [&](int code, const std::string &msg) { return fail(h, code, "m2d_set_recipes: " + msg); };
    int rc;
    if ((rc = m2d_launch_check_csr(h, t_off, nnz, nullptr)) != M2D_OK) return refused(rc, h->last_error);
    if ((rc = m2d_check(h, nullptr, nullptr, nullptr)) != M2D_OK)
        return rc == M2D_ERR_BAD_INGREDIENT ? refused(rc, "offsets are not a CSR row pointer (off[0] = 0, non-decreasing, off[I] = nnz)")
                                            : refused(rc, h->last_error);
    if ((rc = m2d_launch_check_recipe_ids(h, t_ids, nnz, R, nullptr)) != M2D_OK) return refused(rc, h->last_error);
    if ((rc = m2d_check(h, nullptr, nullptr, nullptr)) != M2D_OK) return refused(rc, h->last_error);
    h->rcp_off = std::move(t_off); h->rcp_ids = std::move(t_ids);
    h->rcp_rows = R;
    h->rcp_nnz = nnz;
    h->rcp_set = true;
    return M2D_OK;
}

int m2d_cookable_dishes(m2d_engine *h, const int32_t *market, int64_t nM, int32_t max_missing, int32_t *out_ids, int32_t *out_missing,
                        int64_t *out_count, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (nM < 0 || nM > INT32_MAX || max_missing < 0)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_cookable_dishes: need 0 <= nM < 2^31 and max_missing >= 0");
    if ((!market && nM > 0) || !out_ids || !out_count) return null_buffer(h, "m2d_cookable_dishes");
    M2D_REQUIRE(enter(h, NEEDS_RECIPES));
    return m2d_launch_cookable(h, market, nM, max_missing, out_ids, out_missing, out_count, (hipStream_t)stream);
}

// m2d_topk_markets and m2d_topk_markets_excluding (excl_off, excl_ids, out_missing: the latter's)
static int topk_markets(m2d_engine *h, const char *entry, const int32_t *users, int64_t nQ, const int64_t *market_off, const int32_t *market_ids,
                        int64_t nnzM, const int64_t *excl_off, const int32_t *excl_ids, int32_t k, int32_t max_missing, float *out_scores,
                        int32_t *out_ids, int32_t *out_counts, int32_t *out_missing, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (nQ < 0 || nnzM < 0 || k < 1 || k > 64 || max_missing < 0)
        return fail(h, M2D_ERR_INVALID_ARG, std::string(entry) + ": need nQ >= 0, nnzM >= 0, 1 <= k <= 64 and max_missing >= 0");
    if (nQ == 0) return M2D_OK;
    if (!users || !market_off || (!market_ids && nnzM > 0) || !out_scores || !out_ids) return null_buffer(h, entry);
    M2D_REQUIRE(enter(h, NEEDS_RECIPES | NEEDS_MASKS | PLAIN_SCORES_ONLY, entry));
    return m2d_launch_topk_markets(h, users, nQ, market_off, market_ids, nnzM, k, max_missing, out_scores, out_ids, out_counts,
                                   (hipStream_t)stream, excl_off, excl_ids, out_missing);
}

int m2d_topk_markets(m2d_engine *h, const int32_t *users, int64_t nQ, const int64_t *market_off, const int32_t *market_ids, int64_t nnzM,
                     int32_t k, int32_t max_missing, float *out_scores, int32_t *out_ids, int32_t *out_counts, void *stream)
{
    return topk_markets(h, "m2d_topk_markets", users, nQ, market_off, market_ids, nnzM, nullptr, nullptr, k, max_missing, out_scores, out_ids,
                        out_counts, nullptr, stream);
}

int m2d_topk_markets_excluding(m2d_engine *h, const int32_t *users, int64_t nQ, const int64_t *market_off, const int32_t *market_ids,
                               int64_t nnzM, const int64_t *excl_off, const int32_t *excl_ids, int32_t k, int32_t max_missing,
                               float *out_scores, int32_t *out_ids, int32_t *out_counts, int32_t *out_missing, void *stream)
{
    return topk_markets(h, "m2d_topk_markets_excluding", users, nQ, market_off, market_ids, nnzM, excl_off, excl_ids, k, max_missing,
                        out_scores, out_ids, out_counts, out_missing, stream);
}

int m2d_score_pairs_ingredients(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats,
                                int64_t B, float *out, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (B < 0) return negative_batch(h, "m2d_score_pairs_ingredients");
    if (B == 0) return M2D_OK;
    if (!users || !items || !out) return null_buffer(h, "m2d_score_pairs_ingredients");
    if (!h->dish_high) return fail(h, M2D_ERR_NOT_CONFIGURED, "call m2d_set_ingredients first");
    if (!cats && !h->dish_cats) return fail(h, M2D_ERR_NOT_CONFIGURED, "cats == NULL needs m2d_set_dish_categories");
    if (cats && h->C == 4 && !aligned16(cats)) return fail(h, M2D_ERR_INVALID_ARG, "cats must be 16-byte aligned");
    M2D_REQUIRE(enter(h));
    return m2d_launch_score_pairs(h, users, items, cats ? cats : h->dish_cats, cats == nullptr, B, out,
                                  (hipStream_t)stream, /*use_ingredients=*/true);
}

int m2d_write_memory(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats,
                     const float *write_sign, const float *labels, int64_t B, int32_t L, float *general_memory,
                     float beta_1, float beta_2, float alpha, int32_t which, double *out_sums, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (B < 0 || L <= 0) return fail(h, M2D_ERR_INVALID_ARG, "m2d_write_memory: need B >= 0 and L > 0");
    if (which <= 0 || (which & ~(M2D_WRITE_PERSONAL | M2D_WRITE_GENERAL)))
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_write_memory: which must be M2D_WRITE_PERSONAL, M2D_WRITE_GENERAL or both");
    if (!general_memory || (B > 0 && (!users || !items || !cats || !write_sign || !labels)))
        return null_buffer(h, "m2d_write_memory");
    M2D_REQUIRE(enter(h));
    return m2d_launch_write_memory(h, users, items, cats, write_sign, labels, B, L, general_memory, beta_1, beta_2,
                                   alpha, which, out_sums, (hipStream_t)stream);
}

int m2d_clear_mlp_head(m2d_engine *h)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    h->mlp_w1.reset(); h->mlp_b1.reset(); h->mlp_w2.reset(); h->mlp_b2.reset(); h->mlp_w3.reset();
    m2d_mlp_free_derived(h);
    h->mlp_h1 = h->mlp_h2 = 0;
    return M2D_OK;
}

// (failure contract: m2d.h, "Setters")
int m2d_set_mlp_head(m2d_engine *h, const float *W1, const float *b1, const float *W2, const float *b2,
                     const float *w3, float b3, int32_t H1, int32_t H2, int table_flags)
{
    if (!h || !W1 || !b1 || !W2 || !b2 || !w3 || H1 <= 0 || H2 <= 0)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_set_mlp_head: bad argument");
    if (!table_flags_ok(table_flags)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_set_mlp_head: bad table_flags");
    if (borrowed_misaligned(W1, table_flags) || borrowed_misaligned(W2, table_flags))
        return fail(h, M2D_ERR_INVALID_ARG, "MLP weights must be 16-byte aligned");
    M2D_REQUIRE(m2d_clear_mlp_head(h));         // replacement begins: from here on a failure leaves no head
    M2D_REQUIRE(enter(h));
    const size_t K = (size_t)(h->C + 1) * h->E;
    m2d_table<float> t_w1, t_b1, t_w2, t_b2, t_w3;
    M2D_REQUIRE(adopt(h, W1, K * H1, table_flags, t_w1));
    M2D_REQUIRE(adopt(h, b1, (size_t)H1, table_flags, t_b1));
    M2D_REQUIRE(adopt(h, W2, (size_t)H1 * H2, table_flags, t_w2));
    M2D_REQUIRE(adopt(h, b2, (size_t)H2, table_flags, t_b2));
    M2D_REQUIRE(adopt(h, w3, (size_t)H2, table_flags, t_w3));
    if (!aligned16(t_w1) || !aligned16(t_w2)) return fail(h, M2D_ERR_INVALID_ARG, "MLP weights must be 16-byte aligned");
    h->mlp_w1 = std::move(t_w1); h->mlp_b1 = std::move(t_b1); h->mlp_w2 = std::move(t_w2); h->mlp_b2 = std::move(t_b2);
    h->mlp_w3 = std::move(t_w3);
    h->mlp_b3 = b3;
    h->mlp_h1 = H1;
    h->mlp_h2 = H2;
    return M2D_OK;
}

int m2d_score_pairs_mlp(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t B, float *out,
                        void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (B < 0) return negative_batch(h, "m2d_score_pairs_mlp");
    if (B == 0) return M2D_OK;
    if (!users || !items || !out) return null_buffer(h, "m2d_score_pairs_mlp");
    M2D_REQUIRE(enter(h, NEEDS_HEAD | NEEDS_MASKS));
    return m2d_launch_score_pairs_mlp(h, users, items, B, out, (hipStream_t)stream);
}

int m2d_topk_users_mlp(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates, float *out_scores,
                       int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    M2D_REQUIRE(topk_range(h, "m2d_topk_users_mlp", nU, k, 64));
    M2D_REQUIRE(candidates_range(h, "m2d_topk_users_mlp", k, candidates, 64));
    if (nU == 0) return M2D_OK;
    if (!users || !out_scores || !out_ids) return null_buffer(h, "m2d_topk_users_mlp");
    M2D_REQUIRE(enter(h, NEEDS_HEAD | NEEDS_MASKS));
    return m2d_launch_topk_users_mlp(h, users, nU, k, candidates, nullptr, nullptr, out_scores, out_ids, /*deep=*/false, (hipStream_t)stream);
}

int m2d_topk_users_mlp_excluding(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates, const int64_t *excl_off,
                                 const int32_t *excl_ids, float *out_scores, int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (!excl_off)                                  // no exclusions: m2d_topk_users_mlp's launches and words, its argument rules
        return m2d_topk_users_mlp(h, users, nU, k, candidates, out_scores, out_ids, stream);
    M2D_REQUIRE(topk_range(h, "m2d_topk_users_mlp_excluding", nU, k, 64));
    M2D_REQUIRE(candidates_range(h, "m2d_topk_users_mlp_excluding", k, candidates, 16, "with exclusions "));
    if (nU == 0) return M2D_OK;
    if (!users || !out_scores || !out_ids || !excl_ids) return null_buffer(h, "m2d_topk_users_mlp_excluding");
    M2D_REQUIRE(enter(h, NEEDS_HEAD | NEEDS_MASKS));
    return m2d_launch_topk_users_mlp(h, users, nU, k, candidates, excl_off, excl_ids, out_scores, out_ids, /*deep=*/false, (hipStream_t)stream);
}

int m2d_topk_users_deep(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int64_t *excl_off, const int32_t *excl_ids,
                        float *out_scores, int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    M2D_REQUIRE(topk_range(h, "m2d_topk_users_deep", nU, k, 1024));
    if (nU == 0) return M2D_OK;
    if (!users || !out_scores || !out_ids || (excl_off && !excl_ids)) return null_buffer(h, "m2d_topk_users_deep");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    return m2d_launch_topk_users_deep(h, users, nU, k, excl_off, excl_ids, out_scores, out_ids, (hipStream_t)stream);
}

// ---- household retrieval (m2d_groups.hip): the three calls share their group arguments' rules
static const char *group_args_wrong(const int64_t nG, const int32_t M, const int32_t mode)
{
    if (nG < 0) return "need nG >= 0";
    if (M < 1 || M > M2D_GROUP_MAX_MEMBERS) return "need 1 <= M <= 64";
    if (mode != M2D_GROUP_LEAST && mode != M2D_GROUP_MEAN && mode != M2D_GROUP_MOST) return "mode must be M2D_GROUP_LEAST, _MEAN or _MOST";
    return nullptr;
}

int m2d_topk_groups(m2d_engine *h, const int32_t *members, int64_t nG, int32_t M, int32_t mode, int32_t k, const int64_t *excl_off,
                    const int32_t *excl_ids, float *out_scores, int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (const char *why = group_args_wrong(nG, M, mode)) return fail(h, M2D_ERR_INVALID_ARG, std::string("m2d_topk_groups: ") + why);
    if (k < 1 || k > 1024 || (int64_t)k > h->I) return fail(h, M2D_ERR_INVALID_ARG, "m2d_topk_groups: need 1 <= k <= min(1024, I)");
    if (nG == 0) return M2D_OK;
    if (!members || !out_scores || !out_ids || (excl_off && !excl_ids)) return null_buffer(h, "m2d_topk_groups");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    return m2d_launch_groups(h, "m2d_topk_groups", members, nG, M, mode, nullptr, 0, k, excl_off, excl_ids, nullptr, out_scores, out_ids,
                             (hipStream_t)stream);
}

int m2d_score_groups_slate(m2d_engine *h, const int32_t *members, int64_t nG, int32_t M, int32_t mode, const int32_t *slate, int64_t nD,
                           float *out, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (const char *why = group_args_wrong(nG, M, mode)) return fail(h, M2D_ERR_INVALID_ARG, std::string("m2d_score_groups_slate: ") + why);
    if (nD < 1 || nD > h->I) return fail(h, M2D_ERR_INVALID_ARG, "m2d_score_groups_slate: need 1 <= nD <= I");
    if (nG == 0) return M2D_OK;
    if (!members || !slate || !out) return null_buffer(h, "m2d_score_groups_slate");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    return m2d_launch_groups(h, "m2d_score_groups_slate", members, nG, M, mode, slate, nD, 0, nullptr, nullptr, out, nullptr, nullptr,
                             (hipStream_t)stream);
}

int m2d_topk_groups_slate(m2d_engine *h, const int32_t *members, int64_t nG, int32_t M, int32_t mode, const int32_t *slate, int64_t nD,
                          int32_t k, float *out_scores, int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (const char *why = group_args_wrong(nG, M, mode)) return fail(h, M2D_ERR_INVALID_ARG, std::string("m2d_topk_groups_slate: ") + why);
    if (nD < 1 || nD > h->I || k < 1 || k > 1024 || (int64_t)k > nD)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_topk_groups_slate: need 1 <= nD <= I and 1 <= k <= min(1024, nD)");
    if (nG == 0) return M2D_OK;
    if (!members || !slate || !out_scores || !out_ids) return null_buffer(h, "m2d_topk_groups_slate");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    return m2d_launch_groups(h, "m2d_topk_groups_slate", members, nG, M, mode, slate, nD, k, nullptr, nullptr, nullptr, out_scores, out_ids,
                             (hipStream_t)stream);
}

int m2d_topk_menu(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int32_t *caps, float *out_scores, int32_t *out_ids,
                  void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    M2D_REQUIRE(topk_range(h, "m2d_topk_menu", nU, k, 64));
    if (nU == 0) return M2D_OK;
    if (!users || !caps || !out_scores || !out_ids) return null_buffer(h, "m2d_topk_menu");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    if (h->C > M2D_MENU_MAX_CATEGORIES)
        return fail(h, M2D_ERR_UNSUPPORTED, "m2d_topk_menu: more than 6 categories (one signature per lane of a wave: C <= M2D_MENU_MAX_CATEGORIES)");
    return m2d_launch_topk_menu(h, users, nU, k, caps, out_scores, out_ids, (hipStream_t)stream);
}

int m2d_topk_menu_filtered(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, const int32_t *caps, const int64_t *excl_off,
                           const int32_t *excl_ids, const int32_t *slate, int64_t nD, float *out_scores, int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    M2D_REQUIRE(topk_range(h, "m2d_topk_menu_filtered", nU, k, 64));
    if (slate && (nD < 1 || nD > h->I)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_topk_menu_filtered: with a slate need 1 <= nD <= I");
    if (excl_off && !excl_ids) return fail(h, M2D_ERR_INVALID_ARG, "m2d_topk_menu_filtered: excl_off without excl_ids");
    if (nU == 0) return M2D_OK;
    if (!users || !caps || !out_scores || !out_ids) return null_buffer(h, "m2d_topk_menu_filtered");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    if (h->C > M2D_MENU_MAX_CATEGORIES)
        return fail(h, M2D_ERR_UNSUPPORTED,
                    "m2d_topk_menu_filtered: more than 6 categories (one signature per lane of a wave: C <= M2D_MENU_MAX_CATEGORIES)");
    return m2d_launch_topk_menu_filtered(h, "m2d_topk_menu_filtered", users, nU, k, caps, excl_off, excl_ids, slate, nD, out_scores, out_ids,
                                         (hipStream_t)stream);
}

int m2d_plan_menus(m2d_engine *h, const int32_t *users, int64_t nU, int32_t days, int32_t k, const int32_t *caps, const int32_t *plan_caps,
                   const int64_t *excl_off, const int32_t *excl_ids, const int32_t *slate, int64_t nD, float *out_scores, int32_t *out_ids,
                   void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    M2D_REQUIRE(topk_range(h, "m2d_plan_menus", nU, k, 64));
    if (days < 1 || (int64_t)days * k > M2D_PLAN_MAX_LIST)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_plan_menus: need days >= 1 and days * k <= M2D_PLAN_MAX_LIST = 1024");
    if (slate && (nD < 1 || nD > h->I)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_plan_menus: with a slate need 1 <= nD <= I");
    if (excl_off && !excl_ids) return fail(h, M2D_ERR_INVALID_ARG, "m2d_plan_menus: excl_off without excl_ids");
    if (nU == 0) return M2D_OK;
    if (!users || !caps || !out_scores || !out_ids) return null_buffer(h, "m2d_plan_menus");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    if (h->C > M2D_MENU_MAX_CATEGORIES)
        return fail(h, M2D_ERR_UNSUPPORTED, "m2d_plan_menus: more than 6 categories (one signature per lane of a wave: C <= M2D_MENU_MAX_CATEGORIES)");
    return m2d_launch_plan_menus(h, users, nU, days, k, caps, plan_caps, excl_off, excl_ids, slate, nD, out_scores, out_ids,
                                 (hipStream_t)stream);
}

int m2d_plan_groups(m2d_engine *h, const int32_t *members, int64_t nG, int32_t M, int32_t mode, int32_t days, int32_t k, const int32_t *caps,
                    const int32_t *plan_caps, int32_t caps_per_member, const int64_t *excl_off, const int32_t *excl_ids, const int32_t *slate,
                    int64_t nD, float *out_scores, int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (const char *why = group_args_wrong(nG, M, mode)) return fail(h, M2D_ERR_INVALID_ARG, std::string("m2d_plan_groups: ") + why);
    if (k < 1 || k > 64 || (int64_t)k > h->I) return fail(h, M2D_ERR_INVALID_ARG, "m2d_plan_groups: need 1 <= k <= min(64, I)");
    if (days < 1 || (int64_t)days * k > M2D_PLAN_MAX_LIST)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_plan_groups: need days >= 1 and days * k <= M2D_PLAN_MAX_LIST = 1024");
    if (caps_per_member != 0 && caps_per_member != 1) return fail(h, M2D_ERR_INVALID_ARG, "m2d_plan_groups: caps_per_member must be 0 or 1");
    if (slate && (nD < 1 || nD > h->I)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_plan_groups: with a slate need 1 <= nD <= I");
    if (excl_off && !excl_ids) return fail(h, M2D_ERR_INVALID_ARG, "m2d_plan_groups: excl_off without excl_ids");
    if (nG == 0) return M2D_OK;
    if (!members || !caps || !out_scores || !out_ids) return null_buffer(h, "m2d_plan_groups");
    M2D_REQUIRE(enter(h, NEEDS_MASKS));
    if (h->C > M2D_MENU_MAX_CATEGORIES)
        return fail(h, M2D_ERR_UNSUPPORTED, "m2d_plan_groups: more than 6 categories (one signature per lane of a wave: C <= M2D_MENU_MAX_CATEGORIES)");
    return m2d_launch_plan_groups(h, members, nG, M, mode, days, k, caps, plan_caps, caps_per_member == 1, excl_off, excl_ids, slate, nD,
                                  out_scores, out_ids, (hipStream_t)stream);
}

int m2d_topk_users_mlp_deep(m2d_engine *h, const int32_t *users, int64_t nU, int32_t k, int32_t candidates, const int64_t *excl_off,
                            const int32_t *excl_ids, float *out_scores, int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    M2D_REQUIRE(topk_range(h, "m2d_topk_users_mlp_deep", nU, k, 1024));
    M2D_REQUIRE(candidates_range(h, "m2d_topk_users_mlp_deep", k, candidates, 1024));
    if (nU == 0) return M2D_OK;
    if (!users || !out_scores || !out_ids || (excl_off && !excl_ids)) return null_buffer(h, "m2d_topk_users_mlp_deep");
    M2D_REQUIRE(enter(h, NEEDS_HEAD | NEEDS_MASKS));
    return m2d_launch_topk_users_mlp(h, users, nU, k, candidates, excl_off, excl_ids, out_scores, out_ids, /*deep=*/true, (hipStream_t)stream);
}

int m2d_select_probe(m2d_engine *h, const float *scores, int64_t rows, int64_t W, int32_t k, int32_t form, float *out_scores,
                     int32_t *out_ids, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (rows < 1 || rows > 0x7fffffff || W < 1 || W > 0x7fffffff || k < 1 || (int64_t)k > W || k > (form ? 64 : 1024) || form < 0 || form > 1)
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_select_probe: need rows >= 1, 1 <= k <= min(W, 1024) (form 1: 64), form 0 / 1");
    if (!scores || !out_scores || !out_ids) return null_buffer(h, "m2d_select_probe");
    M2D_REQUIRE(enter(h));
    SelectJob job = SelectJob::row_major(scores, rows, W, nullptr, 0);
    job.k = k; job.out_scores = out_scores; job.out_ids = out_ids;
    return m2d_launch_select(h, job, /*deep=*/form == 0, (hipStream_t)stream);
}

int m2d_catalogue_rank_mlp(m2d_engine *h, const int32_t *users, const int32_t *items, int64_t n, const int64_t *excl_off,
                           const int32_t *excl_ids, int32_t *out_rank, float *out_scores, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (n < 0) return fail(h, M2D_ERR_INVALID_ARG, "m2d_catalogue_rank_mlp: need n >= 0");
    if (n == 0) return M2D_OK;
    if (!users || !items || !out_rank || (excl_off && !excl_ids)) return null_buffer(h, "m2d_catalogue_rank_mlp");
    M2D_REQUIRE(enter(h, NEEDS_HEAD | NEEDS_MASKS));
    return m2d_launch_catalogue_rank_mlp(h, users, items, n, excl_off, excl_ids, out_rank, out_scores, (hipStream_t)stream);
}

int m2d_rank_candidates_mlp(m2d_engine *h, const int32_t *users, const int32_t *items, const int32_t *lens, int64_t nseg, int32_t L,
                            int32_t k, float *out_scores, int32_t *out_items, int32_t *out_flags, void *stream)
{
    return rank_candidates(h, "m2d_rank_candidates_mlp", true, users, items, lens, nseg, L, k, out_scores, out_items, out_flags, stream);
}

// (failure contract: m2d.h, "Setters" -- m2d_train_setup builds the state aside)
int m2d_train_begin(m2d_engine *h, int32_t learner, float lr, float clip_norm, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (learner < M2D_LEARNER_SGD || learner > M2D_LEARNER_ADAM) return fail(h, M2D_ERR_INVALID_ARG, "m2d_train_begin: unknown learner");
    if (!(clip_norm > 0.f)) return fail(h, M2D_ERR_INVALID_ARG, "m2d_train_begin: clip_norm must be positive");
    if (h->ing) return fail(h, M2D_ERR_UNSUPPORTED, "m2d_train_begin: the ingredient extension has no training step");
    M2D_REQUIRE(enter(h));
    return m2d_train_setup(h, learner, lr, clip_norm, (hipStream_t)stream);
}

int m2d_train_step(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats, const float *labels,
                   int64_t B, int32_t apply, float *out, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (!h->train) return fail(h, M2D_ERR_NOT_CONFIGURED, "m2d_train_step: call m2d_train_begin first");
    if (B <= 0) return fail(h, M2D_ERR_INVALID_ARG, "m2d_train_step: need B > 0 (the mean of an empty batch is NaN)");
    if (!users || !items || !cats || !labels) return null_buffer(h, "m2d_train_step");
    M2D_REQUIRE(enter(h));
    return m2d_launch_train_step(h, users, items, cats, labels, B, apply, out, (hipStream_t)stream);
}

int m2d_train_slot(m2d_engine *h, int32_t table, int32_t slot, float *buf, int32_t restore, void *stream)
{
    if (!h || !buf) return M2D_ERR_INVALID_ARG;
    if (!h->train) return fail(h, M2D_ERR_NOT_CONFIGURED, "m2d_train_slot: call m2d_train_begin first");
    if (table < 0 || table > 2 || slot < 0 || slot > 1) return fail(h, M2D_ERR_INVALID_ARG, "m2d_train_slot: table 0..2, slot 0..1");
    float *dev = nullptr;
    int64_t count = 0;
    (void)m2d_train_get_slot(h, table, slot, &dev, &count);
    if (!dev) return fail(h, M2D_ERR_INVALID_ARG, "m2d_train_slot: this learner has no such slot");
    M2D_REQUIRE(enter(h));
    M2D_HIP_TRY(h, hipMemcpyAsync(restore ? dev : buf, restore ? buf : dev, (size_t)count * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return M2D_OK;
}

int m2d_pm_bf16(m2d_engine *h, uint16_t *buf, void *stream)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    if (!buf) return null_buffer(h, "m2d_pm_bf16");
    M2D_REQUIRE(enter(h));
    M2D_REQUIRE(m2d_ensure_pm_bf16(h, (hipStream_t)stream));
    M2D_HIP_TRY(h, hipMemcpyAsync(buf, h->pm_bf16, (size_t)m2d_table_floats(h, 0) * sizeof(uint16_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return M2D_OK;
}

int m2d_tables_updated(m2d_engine *h)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    // "every table value is finite" has to be established again; the masks are named for what hangs on them alone (the menu call's
    // signature index): a borrowed mask table may have been rewritten in place
    m2d_mark_written(h, M2D_TAB_PM | M2D_TAB_RE | M2D_TAB_CE | M2D_TAB_MASKS, M2D_BY_CALLER);
    return M2D_OK;
}

int m2d_train_steps(m2d_engine *h, int64_t *steps, int32_t set)
{
    if (!h || !steps) return M2D_ERR_INVALID_ARG;
    if (!h->train) return fail(h, M2D_ERR_NOT_CONFIGURED, "m2d_train_steps: call m2d_train_begin first");
    if (set && *steps < 0) return fail(h, M2D_ERR_INVALID_ARG, "m2d_train_steps: negative step count");
    return m2d_train_step_count(h, steps, set);
}

int m2d_train_end(m2d_engine *h)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    m2d_train_release(h);
    return M2D_OK;
}

int m2d_check(m2d_engine *h, void *stream, int64_t *bad_value, int64_t *bad_index)
{
    if (!h) return M2D_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    M2D_REQUIRE(enter(h));
    M2D_HIP_TRY(h, hipMemcpyAsync(h->err_host, h->err_dev, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    M2D_HIP_TRY(h, hipStreamSynchronize(st));
    const int code = h->err_host[0];
    if (code == 0) return M2D_OK;
    const int64_t value = h->err_host[1];
    const int64_t index = ((int64_t)(uint32_t)h->err_host[3] << 32) | (uint32_t)h->err_host[2];
    if (bad_value) *bad_value = value;
    if (bad_index) *bad_index = index;
    M2D_HIP_TRY(h, hipMemsetAsync(h->err_dev, 0, 4 * sizeof(int32_t), st));
    M2D_HIP_TRY(h, hipStreamSynchronize(st));
    if (code == M2D_ERR_KERNEL_TIMEOUT) {
        h->last_error = "m2d_topk_users: a wave of workgroup " + std::to_string(h->err_host[2]) + " gave up waiting for its workgroup's progress "
                        "words (stage " + std::to_string(value) + "): that call's lists are invalid";
        return code;
    }
    if (code == M2D_ERR_INVALID_ARG) {              // the exclusion lists of m2d_catalogue_rank / m2d_topk_users_excluding, the slate of m2d_*_slate
        h->last_error = "m2d_catalogue_rank / m2d_topk_users_excluding / m2d_score_slate / m2d_topk_slate: id list not ascending: value " +
                        std::to_string(value) + " at position " + std::to_string(index) +
                        " (an id below its predecessor in excl_ids, an offset below its predecessor in excl_off, or a slate id not above its predecessor;"
                        " m2d_topk_markets: the end offset of a market segment that decreases or reaches outside [0, nnzM], at its request;"
                        " m2d_topk_markets_excluding: also an excluded id below its predecessor, at its index in excl_ids, or the end offset of an"
                        " exclusion segment that decreases or reaches outside the array, at its index in excl_off;"
                        " m2d_topk_users_mlp_excluding / m2d_catalogue_rank_mlp: the exclusion lists as m2d_catalogue_rank reports them;"
                        " m2d_topk_menu: a cap below 0, at its position u * C + c in caps)";
        return code;
    }
    const char *what = code == M2D_ERR_BAD_USER_ID ? "user" : code == M2D_ERR_BAD_ITEM_ID ? "item" : "ingredient";
    h->last_error = std::string(what) + " id " + std::to_string(value) + " at position " +
                    std::to_string(code == M2D_ERR_BAD_INGREDIENT ? (int64_t)h->err_host[2] : index) + " is out of range";
    return code;
}

int m2d_stream_read_probe(m2d_engine *h, const void *buf, int64_t bytes, float *sink, void *stream)
{
    if (!h || !buf || !sink || bytes <= 0 || (bytes & 15) || !aligned16(buf))
        return fail(h, M2D_ERR_INVALID_ARG, "m2d_stream_read_probe: need a 16-byte aligned buffer and size");
    M2D_REQUIRE(enter(h));
    hipLaunchKernelGGL(m2d_stream_read, dim3(h->num_cu * 2), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const v4f *>(buf), bytes / 16, sink);
    M2D_HIP_TRY(h, hipGetLastError());
    return M2D_OK;
}

}  // extern "C"

// ---- options: one table serves m2d_set_option and m2d_get_option (include/m2d.h lists values and defaults) ----
// The variant option carries unrelated switches, each read where it acts:
//     7   retrieval on the dense MFMA kernel (the choice: m2d_catalogue_plan.hip; the kernel: m2d_catalogue_dense.hip)
//     9   retrieval on the one-block-per-user kernel (same places); also the generic pair, head and slate kernels (m2d_score.hip,
//         m2d_mlp.hip, m2d_slate.hip)
//    11 / 12   the pair kernel's throughput / latency form whatever the batch size (m2d_score.hip)
//    13   the tie repair's one-block-per-user tier from the third listed user on (m2d_grouped_policy.h)
//    14   the nine-launch training step (m2d_train.hip)
//    15   the retrieval scan's progress-word wait gives up at once: M2D_ERR_KERNEL_TIMEOUT, a test hook (m2d_grouped_policy.h)
//    16   the MLP head's row offsets in 16-byte units, the instantiation of tables of 4 GiB and more (m2d_mlp.hip)
//   100 + n   n dish-range splits in retrieval, 1 <= n <= 64; also switches the pruned launch off (topk_split_hook,
//         m2d_grouped_policy.h)
//   any value but 0 keeps m2d_topk_users_excluding off its filtered first tier (m2d_catalogue_excl.hip)
namespace {

// two device words of T behind `p` after a device synchronisation (the diagnostics' way to read a counter); null: zeros
template <typename T> int read_words(const m2d_engine *h, const T *p, T (&v)[2], const int n = 2)
{
    v[0] = v[1] = 0;
    if (!p) return M2D_OK;
    if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(v, p, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess)
        return M2D_ERR_HIP;
    return M2D_OK;
}

template <typename T> int read_word(const m2d_engine *h, const T *p, const int word, int64_t *value)
{
    T v[2];
    M2D_REQUIRE(read_words(h, p, v, word + 1));
    *value = (int64_t)v[word];
    return M2D_OK;
}

// the hi x hi first form's count of (wave, tile) pairs whose cross products were multiplied; -1: another form ran
int read_tiles_completed(const m2d_engine *h, int64_t *value)
{
    M2D_REQUIRE(read_word(h, h->topk_tiles_counter, 1, value));
    if (!h->topk_tiles_counter || !h->topk_apx_last) *value = -1;
    return M2D_OK;
}

// users the last m2d_topk_users_excluding call sent to the exact scan: a host count when it sent all of them
int read_excl_short(const m2d_engine *h, int64_t *value)
{
    if (h->excl_all_short < 0) return read_word(h, h->excl_short, 0, value);
    *value = h->excl_all_short;
    return M2D_OK;
}

// One option: an int or int64 member of the engine, or a reader (the diagnostics; they synchronise the device).  Writable members
// with lo <= hi refuse values outside [lo, hi] with "m2d_set_option: <name> takes <takes>"; the others store what they are given.
struct m2d_option {
    const char *name;
    int m2d_engine::*i;
    int64_t m2d_engine::*l;
    int (*read)(const m2d_engine *, int64_t *);
    bool writable;
    int64_t lo, hi;
    const char *takes;
};
constexpr m2d_option opt(const char *name, int m2d_engine::*m, int64_t lo = 1, int64_t hi = 0, const char *takes = "")
{
    return {name, m, nullptr, nullptr, true, lo, hi, takes};
}
constexpr m2d_option opt(const char *name, int64_t m2d_engine::*m, int64_t lo, int64_t hi, const char *takes)
{
    return {name, nullptr, m, nullptr, true, lo, hi, takes};
}
constexpr m2d_option read_only(const char *name, int m2d_engine::*m) { return {name, m, nullptr, nullptr, false, 1, 0, ""}; }
constexpr m2d_option read_only(const char *name, int64_t m2d_engine::*m) { return {name, nullptr, m, nullptr, false, 1, 0, ""}; }
constexpr m2d_option read_only(const char *name, int (*read)(const m2d_engine *, int64_t *))
{
    return {name, nullptr, nullptr, read, false, 1, 0, ""};
}

const m2d_option OPTIONS[] = {
    opt("prefetch", &m2d_engine::opt_prefetch),
    opt("nt_loads", &m2d_engine::opt_nt),
    opt("blocks_per_cu", &m2d_engine::opt_blocks_per_cu),
    opt("variant", &m2d_engine::opt_variant),
    opt("topk_bf16x3", &m2d_engine::opt_topk_bf16x3),
    opt("topk_form", &m2d_engine::opt_topk_form),
    opt("topk_prune", &m2d_engine::opt_topk_prune),
    opt("topk_block", &m2d_engine::opt_topk_block),
    opt("topk_refine", &m2d_engine::opt_topk_refine),
    opt("topk_grouped", &m2d_engine::opt_topk_grouped),
    opt("topk_excl_tier", &m2d_engine::opt_topk_excl_tier),
    opt("market_shares", &m2d_engine::opt_market_shares, 0, 64, "0 ... 64"),
    opt("topk_mlp_chunk_pairs", &m2d_engine::opt_topk_mlp_chunk_pairs, 256, 1 << 24, "256 ... 2^24"),
    opt("slate_chunk_pairs", &m2d_engine::opt_slate_chunk_pairs, 256, 1 << 24, "256 ... 2^24"),
    opt("deep_chunk_pairs", &m2d_engine::opt_deep_chunk_pairs, 256, 1 << 24, "256 ... 2^24"),
    opt("menu_select", &m2d_engine::opt_menu_select, 0, 1, "0 or 1"),
    opt("mlp_bf16x3", &m2d_engine::opt_mlp_bf16x3),
    opt("mlp_form", &m2d_engine::opt_mlp_form),
    opt("skip_masked", &m2d_engine::opt_skip_masked),
    opt("user_high_table", &m2d_engine::opt_user_high),
    opt("pm_bf16", &m2d_engine::opt_pm_bf16, 0, 1, "0 or 1"),
    opt("host_zero_copy", &m2d_engine::opt_host_zero_copy),
    read_only("num_cu", &m2d_engine::num_cu),
    read_only("topk_block_users", &m2d_engine::topk_block_users),
    read_only("market_shares_used", &m2d_engine::market_shares_used),
    read_only("topk_mlp_launches", &m2d_engine::topk_mlp_launches),
    // of the last pattern-grouped m2d_topk_users call: users the refinement finished / sent on to the tie repair, users the repair
    // re-ranked, 32-dish tiles the blocks of the pipelined launch stepped through and would have stepped through without pruning
    read_only("topk_refined", [](const m2d_engine *h, int64_t *v) { return read_word(h, h->topk_refine_counter, 0, v); }),
    read_only("topk_refine_repaired", [](const m2d_engine *h, int64_t *v) { return read_word(h, h->topk_refine_counter, 1, v); }),
    read_only("topk_repaired", [](const m2d_engine *h, int64_t *v) { return read_word(h, h->topk_tie_list, 0, v); }),
    read_only("topk_tiles_scanned", [](const m2d_engine *h, int64_t *v) { return read_word(h, h->topk_tiles_counter, 0, v); }),
    read_only("topk_tiles_full", &m2d_engine::topk_tiles_full),
    read_only("topk_tiles_completed", read_tiles_completed),
    // of the last m2d_catalogue_rank call: tiles the count kernel multiplied, (query, dish) pairs decided in the exact arithmetic
    read_only("rank_tiles_scanned", [](const m2d_engine *h, int64_t *v) { return read_word(h, h->rank_counters, 0, v); }),
    read_only("rank_resolved", [](const m2d_engine *h, int64_t *v) { return read_word(h, h->rank_counters, 1, v); }),
    // of the last m2d_topk_users_excluding call: users sent to the exact scan, tiles that scan multiplied
    read_only("topk_excl_short", read_excl_short),
    read_only("topk_excl_tiles_scanned", [](const m2d_engine *h, int64_t *v) { return read_word(h, h->excl_counters, 0, v); }),
};

const m2d_option *find_option(const char *name)
{
    for (const m2d_option &o : OPTIONS)
        if (!strcmp(name, o.name)) return &o;
    return nullptr;
}

}  // namespace

extern "C" {

int m2d_set_option(m2d_engine *h, const char *name, int64_t value)
{
    if (!h || !name) return M2D_ERR_INVALID_ARG;
    const m2d_option *o = find_option(name);
    if (!o || !o->writable) return fail(h, M2D_ERR_INVALID_ARG, "m2d_set_option: unknown option");
    if (o->lo <= o->hi && (value < o->lo || value > o->hi))
        return fail(h, M2D_ERR_INVALID_ARG, std::string("m2d_set_option: ") + name + " takes " + o->takes);
    if (o->i) h->*(o->i) = (int)value; else h->*(o->l) = value;
    return M2D_OK;
}

int m2d_get_option(const m2d_engine *h, const char *name, int64_t *value)
{
    if (!h || !name || !value) return M2D_ERR_INVALID_ARG;
    const m2d_option *o = find_option(name);
    if (!o) return M2D_ERR_INVALID_ARG;
    if (o->read) return o->read(h, value);
    *value = o->i ? (int64_t)(h->*(o->i)) : h->*(o->l);
    return M2D_OK;
}

}  // extern "C"
