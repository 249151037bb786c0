// Build-defined extension (no reference counterpart): the cookable-dish filter behind m2d_cookable_dishes.
//
//   market  = a set of ingredient ids (any order, repeats allowed)
//   missing[d] = the entries of dish d's recipe list whose id is not in the market, every occurrence counted
//   cookable   = the dishes with a non-empty list and missing[d] <= max_missing, as an ascending id list: a legal slate
//
// Four launches on the caller's stream, ordered by the stream and by nothing else -- no block ever waits for another:
//   m2d_market_bitmap   the market as R bits (cleared by a memset in front of it), atomicOr on 32-bit words; bad ids latched, not set
//   m2d_market_flag     a wave owns MK_DW consecutive dishes = one contiguous run of the CSR stream, one dish per lane.  Lanes read
//                       the run's ids coalesced, MK_EB entries a batch, and test the bitmap (a copy in LDS up to MK_LDS_BITS bits,
//                       through L2 beyond); one ballot turns the batch into a 64-bit "absent" word, and every lane counts the bits
//                       of ITS dish's entry range in it.  A list longer than a batch simply meets several words.  Writes missing[d]
//                       and the block's number of kept dishes.
//   m2d_market_scan     exclusive scan of the block counts (one block), and the total
//   m2d_market_write    each block ranks its kept dishes -- ballot / popcount inside a wave, wave bases through LDS -- and stores
//                       their ids from its base on: the output is ascending by construction.  No atomic cursor, no sort.
// The setter has validated the lists (m2d_check_csr: off[0] = 0, non-decreasing, off[I] = nnz; m2d_check_recipe_ids: every id in
// [0, R)), so no kernel here range-checks a recipe id or an offset.
#include "m2d_engine.h"

namespace {

constexpr int MK_DW = 64;                      // dishes per wave (one per lane)
constexpr int MK_WAVES = 4;                    // waves per block
constexpr int MK_DB = MK_DW * MK_WAVES;        // dishes per block
constexpr int MK_EB = 64;                      // entries per batch (one per lane)
constexpr int MK_LDS_BITS = 1 << 16;           // the bitmap is staged in LDS up to this many bits (8 KiB a block)

// Wave-uniform values are carried in SGPRs (readfirstlane): every loop with a ballot in it is scalar control flow, no cross-lane
// operation ever executes under a partial EXEC mask.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ __launch_bounds__(256) void m2d_check_recipe_ids(const int32_t *ids, int64_t nnz, int32_t R, int32_t *err)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += stride) {
        const int32_t id = ids[i];
        if (id < 0 || id >= R) m2d_latch_error(err, M2D_ERR_BAD_INGREDIENT, id, i);
    }
}

__global__ __launch_bounds__(256) void m2d_market_bitmap(const int32_t *market, int64_t nM, int32_t R, uint32_t *bitmap, int32_t *err)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nM; i += stride) {
        const int32_t id = market[i];
        if (id < 0 || id >= R) m2d_latch_error(err, M2D_ERR_BAD_INGREDIENT, id, i);
        else atomicOr(&bitmap[id >> 5], 1u << (id & 31));
    }
}

template <bool LDS>
__global__ __launch_bounds__(256) void m2d_market_flag(const int32_t *off, const int32_t *ids, const uint32_t *bitmap, int64_t I, int32_t R,
                                                       int32_t max_missing, int32_t *missing, int32_t *block_counts)
{
    __shared__ uint32_t bm[LDS ? MK_LDS_BITS / 32 : 1];
    __shared__ int32_t wave_kept[MK_WAVES];
    const int wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (LDS) {
        const int words = (R + 31) >> 5;                        // <= MK_LDS_BITS / 32: the launcher picks this form by R
        for (int i = threadIdx.x; i < words; i += MK_WAVES * 64) bm[i] = bitmap[i];
        __syncthreads();
    }
    const uint32_t *bits = LDS ? bm : bitmap;
    const int64_t d0 = ((int64_t)blockIdx.x * MK_WAVES + wave) * MK_DW;
    const int64_t left = I - d0;
    const int dn = uni((int)(left < 0 ? 0 : left < MK_DW ? left : MK_DW));   // a wave past the catalogue owns no dish, it still meets the barrier
    int my_begin = 0, my_end = 0;                               // this lane's dish: entries [my_begin, my_end)
    if (lane < dn) {
        my_begin = off[d0 + lane];
        my_end = off[d0 + lane + 1];
    }
    const int64_t e_begin = dn > 0 ? __builtin_amdgcn_readlane(my_begin, 0) : 0;
    const int64_t e_end = dn > 0 ? __builtin_amdgcn_readlane(my_end, dn - 1) : 0;

    int miss = 0;
    for (int64_t pos = e_begin; pos < e_end; pos += MK_EB) {    // scalar bounds
        const int64_t e = pos + lane;
        bool absent = false;
        if (e < e_end) {
            const int32_t id = ids[e];
            absent = ((bits[id >> 5] >> (id & 31)) & 1u) == 0;
        }
        const unsigned long long word = __ballot(absent);       // bit j: entry pos + j is not in the market
        const int64_t lo = my_begin > pos ? my_begin - pos : 0, hi = my_end - pos < MK_EB ? my_end - pos : MK_EB;
        if (hi > lo) {
            const unsigned long long run = hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1;
            miss += __popcll(word & (run << lo));
        }
    }
    const bool live = lane < dn, empty = my_end == my_begin;
    if (live) missing[d0 + lane] = empty ? -1 : miss;
    const unsigned long long kept = __ballot(live && !empty && miss <= max_missing);
    if (lane == 0) wave_kept[wave] = __popcll(kept);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t n = 0;
        for (int w = 0; w < MK_WAVES; ++w) n += wave_kept[w];
        block_counts[blockIdx.x] = n;
    }
}

// one block: thread t sums a contiguous share of the counts; the 256 shares are scanned with shuffles inside a wave and the four
// wave totals through LDS; then every thread writes its share's bases
__global__ __launch_bounds__(256) void m2d_market_scan(const int32_t *counts, int64_t n, int32_t *base, int64_t *total)
{
    __shared__ int32_t wave_sum[MK_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t per = (n + 255) / 256, b = threadIdx.x * per, e = b + per < n ? b + per : n;
    int32_t s = 0;
    for (int64_t i = b; i < e; ++i) s += counts[i];
    int32_t upto = s;                                           // inclusive scan over the wave's lanes (every lane takes part)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t v = __shfl_up(upto, o, 64);
        upto += lane >= o ? v : 0;
    }
    if (lane == 63) wave_sum[wave] = upto;
    __syncthreads();
    int32_t run = upto - s;
    for (int w = 0; w < wave; ++w) run += wave_sum[w];
    if (threadIdx.x == 255) *total = (int64_t)run + s;
    for (int64_t i = b; i < e; ++i) {
        base[i] = run;
        run += counts[i];
    }
}

__global__ __launch_bounds__(256) void m2d_market_write(const int32_t *missing, const int32_t *base, int64_t I, int32_t max_missing,
                                                        int32_t *out_ids)
{
    __shared__ int32_t wave_kept[MK_WAVES];
    const int wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t d = ((int64_t)blockIdx.x * MK_WAVES + wave) * MK_DW + lane;
    bool keep = false;
    if (d < I) {
        const int32_t m = missing[d];
        keep = m >= 0 && m <= max_missing;
    }
    const unsigned long long kept = __ballot(keep);
    if (lane == 0) wave_kept[wave] = __popcll(kept);
    __syncthreads();
    if (keep) {
        int32_t at = base[blockIdx.x];
        for (int w = 0; w < wave; ++w) at += wave_kept[w];
        out_ids[at + __popcll(kept & ((1ull << lane) - 1))] = (int32_t)d;
    }
}

}  // namespace

int m2d_launch_check_recipe_ids(m2d_engine *h, const int32_t *ids, int64_t nnz, int64_t R, hipStream_t stream)
{
    if (nnz == 0) return M2D_OK;
    hipLaunchKernelGGL(m2d_check_recipe_ids, dim3(m2d_blocks_for(h, nnz, 1024)), dim3(256), 0, stream, ids, nnz, (int32_t)R, h->err_dev);
    M2D_HIP_TRY(h, hipGetLastError());
    return M2D_OK;
}

int m2d_launch_cookable(m2d_engine *h, const int32_t *market, int64_t nM, int32_t max_missing, int32_t *out_ids, int32_t *out_missing,
                        int64_t *out_count, hipStream_t st)
{
    const int64_t I = h->I, R = h->rcp_rows;
    const int64_t words = (R + 31) / 32, nb = (I + MK_DB - 1) / MK_DB;
    auto even = [](int64_t n) { return (n + 1) & ~(int64_t)1; };            // the total is 8 bytes: it stands on an even word
    // bitmap | missing | block counts | block bases | total
    const int64_t o_missing = even(words), o_counts = o_missing + even(out_missing ? 0 : I), o_base = o_counts + even(nb),
                  o_total = o_base + even(nb);
    int rc;
    if ((rc = h->market_buf.grow(h, (size_t)(o_total + 2))) != M2D_OK) return rc;
    if (!h->market_count_host && (rc = h->market_count_host.alloc(h, 1)) != M2D_OK) return rc;
    uint32_t *bitmap = reinterpret_cast<uint32_t *>(h->market_buf.get());
    int32_t *missing = out_missing ? out_missing : h->market_buf + o_missing;
    int32_t *counts = h->market_buf + o_counts, *base = h->market_buf + o_base;
    int64_t *total = reinterpret_cast<int64_t *>(h->market_buf + o_total);

    M2D_HIP_TRY(h, hipMemsetAsync(bitmap, 0, (size_t)words * sizeof(uint32_t), st));
    if (nM > 0)
        hipLaunchKernelGGL(m2d_market_bitmap, dim3(m2d_blocks_for(h, nM, 256)), dim3(256), 0, st, market, nM, (int32_t)R, bitmap, h->err_dev);
    const bool lds = R <= MK_LDS_BITS;
    h->last_kernel = lds ? "m2d_market_flag_lds" : "m2d_market_flag_l2";
    if (lds)
        hipLaunchKernelGGL(m2d_market_flag<true>, dim3((unsigned)nb), dim3(MK_WAVES * 64), 0, st, h->rcp_off, h->rcp_ids, bitmap, I, (int32_t)R,
                           max_missing, missing, counts);
    else
        hipLaunchKernelGGL(m2d_market_flag<false>, dim3((unsigned)nb), dim3(MK_WAVES * 64), 0, st, h->rcp_off, h->rcp_ids, bitmap, I, (int32_t)R,
                           max_missing, missing, counts);
    hipLaunchKernelGGL(m2d_market_scan, dim3(1), dim3(256), 0, st, counts, nb, base, total);
    hipLaunchKernelGGL(m2d_market_write, dim3((unsigned)nb), dim3(MK_WAVES * 64), 0, st, missing, base, I, max_missing, out_ids);
    M2D_HIP_TRY(h, hipGetLastError());
    // the one synchronisation: the count, and with it the id-error latch (m2d_check's own copy and wait)
    M2D_HIP_TRY(h, hipMemcpyAsync(h->market_count_host, total, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    rc = m2d_check(h, st, nullptr, nullptr);
    *out_count = *h->market_count_host;
    return rc;
}
