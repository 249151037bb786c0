// CSR lists per row on the device: what every call that takes "leave out these dishes per row" shares (m2d_catalogue_rank,
// m2d_topk_users_excluding, m2d_topk_markets_excluding, m2d_topk_users_mlp_excluding, m2d_catalogue_rank_mlp) -- the segment clamp,
// the lower bound, the whole-list checks and the forward-only strike cursor.  A list is int64 offsets off[0 .. n] and ascending int32
// ids; the array's length is the last offset.  Nothing here trusts an offset or an id: segments are clamped before anything is read,
// ids are only ever compared.
#pragma once

#include "m2d_engine.h"

// Row `row`'s segment [x0, x1), clamped into [0, total] before anything is read; `bad`: it decreases or reaches outside.  A market of
// m2d_topk_markets is a CSR segment like any other: m2d_markets_bitmap, m2d_markets_topk and m2d_markets_missing take a request's
// market with this function, and the exclusion forms a row's excluded dishes.
__device__ __forceinline__ void csr_segment(const int64_t *off, int64_t row, int64_t total, int64_t &x0, int64_t &x1, bool &bad)
{
    const int64_t lo = off[row], hi = off[row + 1];
    bad = hi < lo || lo < 0 || hi > total;
    x0 = lo < 0 ? 0 : lo > total ? total : lo;
    x1 = hi < x0 ? x0 : hi > total ? total : hi;
}

// First position in [lo, hi) whose id is not below d, the ids ascending; `at` says where they live (a segment in HBM, a lane's column
// of LDS).  The one binary search over ids.
template <typename Pos, typename Key, typename At>
__device__ __forceinline__ Pos csr_lower_bound(Pos lo, Pos hi, const Key d, At &&at)
{
    while (lo < hi) {
        const Pos mid = (lo + hi) >> 1;
        if (at(mid) < d) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t csr_lower_bound(const int32_t *ids, const int64_t lo, const int64_t hi, const int64_t d)
{
    return csr_lower_bound(lo, hi, d, [ids](const int64_t i) { return ids[i]; });
}

// is `d` among the ascending ids at(lo) ... at(hi - 1)?
template <typename Pos, typename At>
__device__ __forceinline__ bool sorted_contains(const Pos lo, const Pos hi, const int32_t d, At &&at)
{
    const Pos i = csr_lower_bound(lo, hi, d, at);
    return i < hi && at(i) == d;
}

__device__ __forceinline__ bool sorted_contains(const int32_t *ids, const int64_t lo, const int64_t hi, const int32_t d)
{
    return sorted_contains(lo, hi, d, [ids](const int64_t i) { return ids[i]; });
}

// ---- the whole-list checks -------------------------------------------------------------------------------------------------------
// A CSR exclusion list -- offsets off[0 .. n], ascending dish ids per segment -- as every call checks it.  Offset q: non-decreasing from 0.
__device__ __forceinline__ void csr_check_offset(const int64_t *off, const int64_t q, int32_t *err)
{
    const int64_t o = off[q];
    if ((q == 0 && o != 0) || (q > 0 && o < off[q - 1])) m2d_latch_error(err, M2D_ERR_INVALID_ARG, (int32_t)o, q);
}

// the segment position i lies in: the last q with off[q] <= i
__device__ __forceinline__ int64_t csr_owner(const int64_t *off, const int64_t n, const int64_t i)
{
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// The id x at position i: a dish of the catalogue, and not below the id before it in its segment q (set once x is in range).  Returns 0
// for an id that is neither, 2 for one that repeats the id before it, else 1; `report`: whether this thread latches the violation -- the
// callers' threads per id differ.
__device__ __forceinline__ int csr_check_id(const int64_t *off, const int32_t *ids, const int64_t n, const int64_t I, const int64_t i,
                                            const bool report, int32_t *err, int32_t &x, int64_t &q)
{
    x = ids[i];
    int r = 1;
    if (x < 0 || (int64_t)x >= I) {
        if (report) m2d_latch_error(err, M2D_ERR_BAD_ITEM_ID, x, i);
        r = 0;
    } else {
        q = csr_owner(off, n, i);
        if (i > off[q] && i > 0) {                          // (i > 0: a negative first offset must not reach in front of the array)
            const int32_t prev = ids[i - 1];
            if (prev > x && report) m2d_latch_error(err, M2D_ERR_INVALID_ARG, x, i);
            r = prev > x ? 0 : (prev == x ? 2 : 1);
        }
    }
    return r;
}

// ---- a row's exclusion window ---------------------------------------------------------------------------------------------
// The row's segment of ascending dish ids, clamped into the array before anything is read, and a cursor into it that only moves
// forward: a wave's steps cover consecutive ids [id0, id0 + 64 N) and ascend.  Everything here is wave-uniform and carried in SGPRs
// (readfirstlane), so the branches around the window are scalar ones; the per-lane search inside has no cross-lane operation.
// The ids are only ever compared: a bad one (reported by the call's check) indexes nothing.
__device__ __forceinline__ int64_t uni64(const int64_t v)
{
    return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)((uint64_t)v >> 32)) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v));
}

struct ExclCursor {
    int64_t xw = 0, x1 = 0;          // the next step's window starts at xw or behind it; the segment's end
    int32_t xv = INT32_MAX;          // the id at xw: a step that ends at or below it has an empty window and pays one compare

    // row's segment of xids, `total` ids long.  Returns what csr_segment says of the offsets (`bad`: reporting it is the caller's
    // business)
    __device__ __forceinline__ bool open(const int64_t *xoff, const int32_t *xids, const int64_t total, const int64_t row)
    {
        int64_t x0;
        bool bad;
        csr_segment(xoff, row, total, x0, x1, bad);
        xw = uni64(x0);
        x1 = uni64(x1);
        if (xw < x1) xv = __builtin_amdgcn_readfirstlane(xids[xw]);
        return bad;
    }

    // the same for lists that may be absent, their length at *xend: no offsets, nothing is read and the window stays empty
    __device__ __forceinline__ void open(const int64_t *xoff, const int32_t *xids, const int64_t *xend, const int64_t row)
    {
        if (xoff) open(xoff, xids, *xend, row);
    }

    // one step of N 64-wide slices (slice q, lane l: id id0 + 64 q + l): slot[q] becomes `none` where the slice's id is in the segment
    // (the head's kernels strike keys with TKM_NONE, m2d_markets_topk clears a `kept` flag)
    template <int N, typename T>
    __device__ __forceinline__ void strike(const int32_t *xids, const int64_t id0, const int lane, T (&slot)[N], const T none)
    {
        if ((int64_t)xv >= id0 + 64 * N) return;             // scalar: xv is the smallest id the wave has not passed
        const int64_t w0 = uni64(csr_lower_bound(xids, xw, x1, id0)), w1 = uni64(csr_lower_bound(xids, w0, x1, id0 + 64 * N));
        xw = w1;
        xv = w1 < x1 ? __builtin_amdgcn_readfirstlane(xids[w1]) : INT32_MAX;
        if (w1 == w0) return;                                // scalar: nothing of the segment in this step
#pragma unroll
        for (int q = 0; q < N; ++q) {
            const int64_t id = id0 + q * 64 + lane;
            const int64_t at = csr_lower_bound(xids, w0, w1, id);
            if (at < w1 && xids[at] == id) slot[q] = none;
        }
    }

    // The same step over an ASCENDING ID TABLE (m2d_topk_menu_filtered: a range of a signature's segment of the index): slice q, lane l
    // holds id[q] where live[q].  The step's ids lie in [id_lo, id_hi] -- the ids under its first and its last live column, wave-uniform
    // -- and the ids of the steps behind it are above id_hi, so the window is [lower bound of id_lo, lower bound of id_hi + 1) and the
    // cursor moves to its end: what lies between two of the table's ids (the row's excluded dishes of OTHER signatures) is passed over
    // by the bounds, never counted off.  Ids are only compared; a table that is not ascending gives an empty or a wrong window, and
    // nothing outside [xw, x1) is read.
    template <int N, typename T>
    __device__ __forceinline__ void strike_ids(const int32_t *xids, const int32_t id_lo, const int32_t id_hi, const int32_t (&id)[N],
                                               const bool (&live)[N], T (&slot)[N], const T none)
    {
        if (xv > id_hi) return;                              // scalar: xv is the smallest id the wave has not passed
        const int64_t w0 = uni64(csr_lower_bound(xids, xw, x1, (int64_t)id_lo)),
                      w1 = uni64(csr_lower_bound(xids, w0, x1, (int64_t)id_hi + 1));
        xw = w1;
        xv = w1 < x1 ? __builtin_amdgcn_readfirstlane(xids[w1]) : INT32_MAX;
        if (w1 == w0) return;                                // scalar: nothing of the segment in this step
#pragma unroll
        for (int q = 0; q < N; ++q) {
            if (!live[q]) continue;
            const int64_t at = csr_lower_bound(xids, w0, w1, (int64_t)id[q]);
            if (at < w1 && xids[at] == id[q]) slot[q] = none;
        }
    }
};
