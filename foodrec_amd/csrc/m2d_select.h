// The row walk of everything that reads a SelectJob's score block (m2d_engine.h): m2d_topk_mlp_select and both passes of m2d_select_deep
// (m2d_select.hip), m2d_topk_mlp_count (m2d_topk_mlp.hip).  How a column becomes a key is written here and nowhere else.
#pragma once

#include "m2d_exclusions.h"   // (ExclCursor: a row's exclusion window)

// A wave's share of row `row`: steps of four 64-wide slices (wave w of nw takes the columns from 256 w, then 256 nw further on).  A step
// loads its four slices, makes every column its key -- TKM_NONE past W; tkm_key of the score and the column's id (m2d_engine.h); HOLES:
// an id below 0 is no entry, whatever its score --, strikes the row's excluded dishes (EXCL: ExclCursor::strike at dish d0 + base, between
// the loads and the bodies; with null offsets the window is empty and the strike is one scalar compare), then calls
// body(key, score word) once per slice, in slice order.  Every lane of the wave calls every body: a body may ballot and shuffle.
// EXCL == SELECT_EXCL_IDS: the row's ids are an ASCENDING table (a range of a signature's segment, m2d_menu.hip) and the strike is
// ExclCursor::strike_ids between the ids under the step's first and last live column.
constexpr int SELECT_EXCL_NONE = 0, SELECT_EXCL_RANGE = 1, SELECT_EXCL_IDS = 2;      // (0 / 1: the former false / true)

template <int EXCL, bool HOLES, typename Body>
__device__ __forceinline__ void select_walk(const SelectJob &job, const int64_t row, const int wave, const int nw, const int lane, Body &&body)
{
    const float *sc = job.scores + row * job.rs;
    const int32_t *idr = job.ids ? job.ids + row * job.ids_stride : nullptr;
    ExclCursor xc;
    if (EXCL) xc.open(job.xoff, job.xids, job.xend, row);    // (a bad segment is the call's check to report)
    for (int64_t base = (int64_t)wave * 256; base < job.W; base += (int64_t)nw * 256) {
        uint64_t ck[4];
        uint32_t cs[4];
        int32_t cid[4];                          // (SELECT_EXCL_IDS only: the other forms never read them)
        bool live[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {            // four slices in flight
            const int64_t e = base + q * 64 + lane;
            ck[q] = TKM_NONE;
            cs[q] = 0u;
            cid[q] = 0;
            live[q] = e < job.W;
            if (e < job.W) {
                const float s = sc[e * job.es];
                cs[q] = __float_as_uint(s);
                int32_t id = job.d0 + (int32_t)e;
                if (idr) id = idr[e];            // (one scalar branch around the load; as `idr ? :` it became two a slice)
                ck[q] = tkm_key(s, id);
                cid[q] = id;
                if (HOLES) ck[q] |= (uint64_t)(int64_t)(id >> 31);          // an id below 0: all ones, TKM_NONE (no branch)
            }
        }
        if (EXCL == SELECT_EXCL_RANGE) xc.strike(job.xids, (int64_t)job.d0 + base, lane, ck, TKM_NONE);
        if (EXCL == SELECT_EXCL_IDS) {           // base < W: the step's first column is live; its last live one is wave-uniform too
            const int64_t last = base + 255 < job.W ? base + 255 : job.W - 1;
            xc.strike_ids(job.xids, __builtin_amdgcn_readfirstlane(idr[base]), __builtin_amdgcn_readfirstlane(idr[last]), cid, live, ck,
                          TKM_NONE);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) body(ck[q], cs[q]);
    }
}
