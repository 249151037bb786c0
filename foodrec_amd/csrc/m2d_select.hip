// Selection: the k best of every row of a score block, as (score, id) lists in tkm_key's order (m2d_engine.h).  One request record
// (SelectJob, m2d_engine.h), one row walk (select_walk, m2d_select.h), two kernels and the one launcher in front of them:
//   m2d_topk_mlp_select   k <= 64: a sorted list across a wave's lanes, an insertion per candidate that passes
//   m2d_select_deep       1 <= k <= 1024: a radix select on the key, O(W) work per row for any k
// Both: one workgroup per score row -- column e at scores[row * rs + e * es], its id ids[row * ids_stride + e] or d0 + e when `ids` is
// null -- merged into the row's list of k (score, id) in out_scores / out_ids (`first`: the list starts with this block, otherwise its k
// entries take part as k more candidates: they were struck when they were listed).  EXCL: row r leaves out xids[xoff[r] .. xoff[r + 1]),
// ascending dish ids, the array's length at *xend -- 1 (ids == null): struck on the dish range d0 + e; 2 (ids != null, the id row
// ASCENDING: m2d_topk_menu_filtered's ranges of a signature's segment): struck on the id table.  HOLES (the candidate form behind a retrieval with exclusions): an id below 0 in `ids` is no entry,
// whatever its score.  Both make a candidate TKM_NONE, which takes part in nothing.  No global atomics, no block waits for another; the
// score written is the word that was read (a NaN's payload, a -0).
#include "m2d_select.h"

namespace {

// ---- the list across lanes ------------------------------------------------------------------------------------------------------
// Every wave keeps the k best of the 64-wide slices it reads as a sorted list ACROSS its lanes (lane j: the j-th best, k <= 64
// is why one wave holds a whole list): a slice is compared with lane k - 1's key in one ballot, and the few candidates that
// pass are inserted one by one -- a ballot for the position, a one-lane shift for the tail.  After the first slices about
// k ln(W / k) candidates pass per wave, the rest costs a load, a compare and a ballot per 64 scores.  The waves' lists and the
// running list meet in LDS ((waves + 1) k keys of 8 B and score words of 4 B), where every entry counts the entries in front of
// it and the first k write themselves out.  <false, false> is the kernel as it stood before exclusions.
template <int EXCL, bool HOLES>
__global__ __launch_bounds__(1024) void m2d_topk_mlp_select(const SelectJob job)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int nw = blockDim.x >> 6, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t row = blockIdx.x;
    const int k = job.k;
    float *out_scores = job.out_scores;
    int32_t *out_ids = job.out_ids;
    uint64_t *mk = reinterpret_cast<uint64_t *>(smem);                          // [(nw + 1) k]
    uint32_t *ms = reinterpret_cast<uint32_t *>(mk + (size_t)(nw + 1) * k);     // [(nw + 1) k]

    uint64_t lk = TKM_NONE, thr = TKM_NONE;      // this lane's list entry; lane k - 1's: what a candidate has to beat
    uint32_t ls = 0x7FC00000u;
    select_walk<EXCL, HOLES>(job, row, wave, nw, lane, [&](const uint64_t key, const uint32_t word) {
        unsigned long long m = __ballot(key < thr);
        while (m) {                              // wave-uniform: m, c and thr are the same in every lane
            const int src = __ffsll(m) - 1;
            m &= m - 1;
            const uint64_t c = __shfl(key, src, 64);
            if (c >= thr) continue;              // the list moved on since the ballot
            const uint32_t cb = __shfl(word, src, 64);
            const int pos = __popcll(__ballot(lk < c));                        // sorted: the lanes in front of c
            const uint64_t upk = __shfl_up(lk, 1, 64);
            const uint32_t ups = __shfl_up(ls, 1, 64);
            lk = lane == pos ? c : lane > pos ? upk : lk;                       // (selects: as if / else if the compiler branches here,
            ls = lane == pos ? cb : lane > pos ? ups : ls;                      //  now that the list is reached through the walk's body)
            thr = __shfl(lk, k - 1, 64);
        }
    });
    if (lane < k) {
        mk[wave * k + lane] = lk;
        ms[wave * k + lane] = ls;
    }
    if (!job.first && (int)threadIdx.x < k) {
        const float s = out_scores[row * k + threadIdx.x];
        mk[nw * k + threadIdx.x] = tkm_key(s, out_ids[row * k + threadIdx.x]);
        ms[nw * k + threadIdx.x] = __float_as_uint(s);
    }
    __syncthreads();                             // the running list has been read: from here on it is written
    const int M = (nw + (job.first ? 0 : 1)) * k;
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

// ---- the radix select -----------------------------------------------------------------------------------------------------------
// The list L (np2(k) keys of 8 B and score words of 4 B in LDS) starts as the running list, or as TKM_NONE throughout.  A digit pass
// histograms the next 11 bits (the last pass: 9) of every key that matches the prefix found so far -- the row, read again from L2,
// and L -- into 2 048 LDS bins; a wave adds once per distinct digit for the first four digits of a slice (ballot, one add of the
// popcount), so a row of equal scores costs one add per wave and slice.  A block-wide scan of the bins finds the digit of the k-th
// key, the count in front of it (`less`) and the keys that share it (`m`).  The passes end when less + m == k (everything that
// shares the prefix is listed: the usual exit is m == 1), when all 64 bits are fixed (only equal keys are left), or after the first
// pass when the row holds no more than k real keys (all are listed).  The gather then works on L IN PLACE: entries of L that stay
// keep their slot, the slots of the others go to a free list (in the bins' space), the row's listed keys take free slots in arrival
// order from an LDS counter, what is left of the free list becomes TKM_NONE.  A bitonic sort of L on the key, and the row is written
// once: the result is a function of the key set alone.
// LDS: 8 KiB of bins + 12 B x np2(k) + 128 B: 20.1 KiB at k = 1 024.
constexpr int SD_BITS = 11, SD_BINS = 1 << SD_BITS;
constexpr int SD_PEEL = 4;                       // distinct digits of a slice a wave adds once each; the lanes left add for themselves
enum { SD_WSUM = 0, SD_BIN = 16, SD_BEFORE, SD_COUNT, SD_TAKEN, SD_FREE, SD_EQ, SD_MISC = 32 };

__host__ __device__ __forceinline__ int sd_np2(const int k)
{
    int n = 1;
    while (n < k) n <<= 1;
    return n;
}

// one slice's adds to the bins: `on` lanes hold digit d
__device__ __forceinline__ void sd_hist_add(uint32_t *hist, bool on, const uint32_t d, const int lane)
{
    unsigned long long rem = __ballot(on);
    for (int round = 0; round < SD_PEEL && rem; ++round) {          // wave-uniform
        const int leader = __ffsll(rem) - 1;
        const uint32_t dl = (uint32_t)__shfl((int)d, leader, 64);
        const unsigned long long grp = __ballot(on && d == dl);
        if (lane == leader) atomicAdd(&hist[dl], (uint32_t)__popcll(grp));
        on = on && d != dl;
        rem &= ~grp;
    }
    if (on) atomicAdd(&hist[d], 1u);
}

// what the passes found: a key is listed when its top `bits` bits are below `prefix`, or equal to it while `need_eq` lasts;
// bits == 0: every real key is listed
struct SdCut {
    uint64_t prefix;
    int bits;
    int need_eq;
    __device__ __forceinline__ int side(const uint64_t key) const   // 0: in front, 1: shares the prefix, 2: behind (or no entry)
    {
        if (key == TKM_NONE) return 2;
        if (bits == 0) return 0;
        const uint64_t hi = key >> (64 - bits);
        return hi < prefix ? 0 : hi == prefix ? 1 : 2;
    }
};

template <int EXCL, bool HOLES>
__global__ __launch_bounds__(1024) void m2d_select_deep(const SelectJob job)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int T = blockDim.x, nw = T >> 6, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int k = job.k;
    const int32_t first = job.first;
    float *out_scores = job.out_scores;
    int32_t *out_ids = job.out_ids;
    const int n2 = sd_np2(k);
    uint64_t *lk = reinterpret_cast<uint64_t *>(smem);                  // [n2]
    uint32_t *ls = reinterpret_cast<uint32_t *>(lk + n2);               // [n2]
    uint32_t *hist = ls + n2;                                           // [SD_BINS]; the free list after the passes
    uint32_t *misc = hist + SD_BINS;                                    // [SD_MISC]

    // ---- L: the running list, or no entries (read before anything is written: the outputs are written at the very end) ----
    for (int i = tid; i < n2; i += T) {
        uint64_t key = TKM_NONE;
        uint32_t w = 0x7FC00000u;
        if (!first && i < k) {
            const float s = out_scores[row * k + i];
            key = tkm_key(s, out_ids[row * k + i]);
            w = __float_as_uint(s);
        }
        lk[i] = key;
        ls[i] = w;
    }

    // ---- the digit passes ----
    SdCut cut;
    cut.prefix = 0; cut.bits = 0; cut.need_eq = 0;
    int less = 0;                                    // keys in front of the prefix
    for (;;) {
        const int nb = 64 - cut.bits < SD_BITS ? 64 - cut.bits : SD_BITS, sh = 64 - cut.bits - nb;
        const uint32_t dmask = (1u << nb) - 1u;
        for (int i = tid; i < SD_BINS; i += T) hist[i] = 0u;
        if (tid == 0) misc[SD_BIN] = 0xFFFFFFFFu;
        __syncthreads();                             // (also: L is complete)
        const auto add = [&](const uint64_t key, uint32_t) {
            const bool on = key != TKM_NONE && (cut.bits == 0 || (key >> (64 - cut.bits)) == cut.prefix);
            sd_hist_add(hist, on, (uint32_t)(key >> sh) & dmask, lane);
        };
        select_walk<EXCL, HOLES>(job, row, wave, nw, lane, add);
        if (!first)
            for (int i0 = wave * 64; i0 < n2; i0 += T) add(i0 + lane < n2 ? lk[i0 + lane] : TKM_NONE, 0u);
        __syncthreads();
        // scan: thread t owns SD_BINS / T neighbouring bins
        const int per = SD_BINS / T;
        uint32_t own = 0;
        for (int j = 0; j < per; ++j) own += hist[tid * per + j];
        uint32_t incl = own;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) misc[SD_WSUM + wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += misc[SD_WSUM + w];
        const uint32_t want = (uint32_t)(k - less);                  // the k-th key is the want-th (1-based) of the keys counted
        uint32_t acc = incl - own;
        if (acc < want && want <= incl) {            // one thread at most
            for (int j = 0; j < per; ++j) {
                const uint32_t c = hist[tid * per + j];
                if (acc + c >= want) {
                    misc[SD_BIN] = (uint32_t)(tid * per + j);
                    misc[SD_BEFORE] = acc;
                    misc[SD_COUNT] = c;
                    break;
                }
                acc += c;
            }
        }
        __syncthreads();
        const uint32_t bin = misc[SD_BIN], before = misc[SD_BEFORE];
        const int m = (int)misc[SD_COUNT];
        __syncthreads();                             // everyone has read the pass's result: the next pass may reset it
        if (bin == 0xFFFFFFFFu) break;               // no more than k real keys (first pass only): bits == 0, all are listed
        less += (int)before;
        cut.prefix = (cut.prefix << nb) | bin;
        cut.bits += nb;
        cut.need_eq = k - less;
        if (less + m == k || cut.bits == 64) break;
    }

    // ---- gather, in place ----
    uint32_t *freel = hist;                          // [<= k] slots of L that are up for taking (the bins are done with)
    if (tid == 0) misc[SD_TAKEN] = misc[SD_FREE] = misc[SD_EQ] = 0u;
    __syncthreads();
    const auto listed = [&](const uint64_t key) {
        const int sd = cut.side(key);
        return sd == 0 || (sd == 1 && (int)atomicAdd(&misc[SD_EQ], 1u) < cut.need_eq);
    };
    for (int i = tid; i < k; i += T)
        if (!listed(lk[i])) freel[atomicAdd(&misc[SD_FREE], 1u)] = (uint32_t)i;
    __syncthreads();
    const uint32_t nfree = misc[SD_FREE];
    select_walk<EXCL, HOLES>(job, row, wave, nw, lane, [&](const uint64_t key, const uint32_t word) {
        const bool take = listed(key);
        const unsigned long long mk = __ballot(take);
        if (mk) {                                    // wave-uniform: one add per slice
            const int leader = __ffsll(mk) - 1;
            uint32_t at = 0;
            if (lane == leader) at = atomicAdd(&misc[SD_TAKEN], (uint32_t)__popcll(mk));
            at = (uint32_t)__shfl((int)at, leader, 64) + (uint32_t)__popcll(mk & ((1ull << lane) - 1ull));
            if (take && at < nfree) {                // (the counts make at < nfree: the list cannot be overrun whatever they are)
                const uint32_t slot = freel[at];
                lk[slot] = key;
                ls[slot] = word;
            }
        }
    });
    __syncthreads();
    const uint32_t ntaken = misc[SD_TAKEN];
    for (uint32_t j = ntaken + tid; j < nfree; j += T) {             // slots nobody took: no entry
        lk[freel[j]] = TKM_NONE;
        ls[freel[j]] = 0x7FC00000u;
    }
    __syncthreads();

    // ---- bitonic sort of L on the key, ascending ----
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            for (int p = tid; p < (n2 >> 1); p += T) {
                const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1)), j = i | stride;
                const bool up = (i & size) == 0;
                const uint64_t a = lk[i], b = lk[j];
                if ((a > b) == up && a != b) {
                    const uint32_t wa = ls[i], wb = ls[j];
                    lk[i] = b; lk[j] = a;
                    ls[i] = wb; ls[j] = wa;
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < k; i += T) {
        const uint64_t key = lk[i];
        out_scores[row * k + i] = __uint_as_float(key == TKM_NONE ? 0x7FC00000u : ls[i]);
        out_ids[row * k + i] = key == TKM_NONE ? -1 : (int32_t)(uint32_t)(key & 0xFFFFFFFFu);
    }
}

}  // namespace

int m2d_launch_select(m2d_engine *h, const SelectJob &job, const bool deep, hipStream_t stream)
{
    const int threads = select_threads(job.W);
    const size_t entry = sizeof(uint64_t) + sizeof(uint32_t);        // a list entry in LDS: key, score word
    const size_t lds = deep ? (size_t)sd_np2(job.k) * entry + (size_t)(SD_BINS + SD_MISC) * sizeof(uint32_t)
                            : (size_t)(threads / 64 + 1) * job.k * entry;
    const auto launch = [&](auto kernel) -> int {
        M2D_HIP_TRY(h, m2d_lds_limit((const void *)kernel, (int)lds));
        hipLaunchKernelGGL(kernel, dim3((unsigned)job.rows), dim3(threads), lds, stream, job);
        M2D_HIP_TRY(h, hipGetLastError());
        return M2D_OK;
    };
    const auto form = [&](auto list, auto radix) { return deep ? launch(radix) : launch(list); };
    return job.xoff  ? (job.ids ? form(m2d_topk_mlp_select<SELECT_EXCL_IDS, false>, m2d_select_deep<SELECT_EXCL_IDS, false>)
                                : form(m2d_topk_mlp_select<true, false>, m2d_select_deep<true, false>))
         : job.holes ? form(m2d_topk_mlp_select<false, true>, m2d_select_deep<false, true>)
                     : form(m2d_topk_mlp_select<false, false>, m2d_select_deep<false, false>);
}
