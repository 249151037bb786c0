// Fused pair-score kernels for gfx950 (MI355X): one pass over
//   gather PM[user] ((C+1)*E floats, contiguous)      Model_Recommender.py:57-62
//   gather RE[item] (E floats)                        Model_Recommender.py:63-66
//   masked category dot (high level)                  Model_Recommender.py:67-80
//   masked low-level dot                              Model_Recommender.py:82-93
//   blend                                             Model_Recommender.py:95-97
// with none of the [B, C, E] temporaries the TF graph materialises.
//
// Mapping (wave64).  A wave owns 64 consecutive pairs ("chunk"): lane i reads pair i's two ids and
// its mask with coalesced loads and finally stores pair i's score, so every id/mask/score access is
// one full 256-B (or 1-KiB) wave transaction.  Inside the chunk the wave is cut into 64/LPP groups
// of LPP lanes; a group walks its LPP pairs one per step, lane j of the group holding float4 column
// j of every row, so each row read is LPP*16 contiguous bytes (256 B at E = 64).  The Category_Embedding
// fragment a lane needs (C float4) never changes and lives in registers.  PF steps of row loads
// are kept in flight ahead of the arithmetic; the rows of Personal_Memory are read once and can
// be marked non-temporal so they do not evict the (re-used) dish rows from L2 / Infinity Cache.
//
// HBM-bound: ~1 flop per byte.  Algorithmic bytes per pair = (C+2)*E*4 + C*4 + 12.
//
// Layout of the file.  Four entry points -- throughput C = 4 (m2d_score_pairs_c4), latency C = 4 (_c4_small), throughput C <= 8
// (_cn), any shape (_generic) -- are put together from pieces that are each written once: pair_ids (id check, error latch, clamp),
// LaneGroup (a lane's place in its group, the idle-lane mask, the Category_Embedding fragment), fetch_pair (one pair's rows into
// a slot), pair_partial (a lane's share of the two dot products), walk_pairs (a group's steps over its pairs, PF in flight) and
// store_score (divisions, blend, NaN of a bad id, store).  The lane-group forms share every fmaf and its order, so the same pair
// scores the same bits in all of them.  The launcher turns the width into (LPP, FULL) in one place (with_width).
#include <type_traits>

#include "m2d_engine.h"

namespace {

struct ScoreArgs {
    const float *pm;
    const float *re;
    const float *ce;
    const int32_t *users;
    const int32_t *items;
    const float *cats;  // [B, C] (explicit feed) or [I, C] (by dish)
    const float *hv;    // extension: per-dish high-level vectors [I, E] (ingredient table), or null
    float *out;
    int64_t B;
    int64_t U;
    int64_t I;
    int64_t user_base;
    int32_t E;
    int32_t C;
    float a;
    float b;
    int32_t *err;
    int32_t skip_masked;   // do not fetch the Personal_Memory rows of categories whose mask weight is 0 (their products are 0)
    const int32_t *nonfinite;   // device word: some table value is inf / NaN -> 0 * row is not 0 (:82), every row is fetched
    const float *uh;       // [U, 4] derived table <U_high[u], CE_c> (m2d_build_user_high), or null: read U_high and multiply
    const uint16_t *pmh;   // [U, C+1, E] bf16 mirror of Personal_Memory (m2d_build_pm_bf16), or null: the BF kernel forms read it instead of pm
    const int32_t *nonfinite_bf;   // device word: some value of the mirror is inf / NaN (rounding makes inf of finite values)
};

// Rows of weight-0 categories may be left out only while every table value is finite: 0 * inf = NaN at
// Model_Recommender.py:82-90.  One scalar load per wave (the word is set by the table scan / the engine's writers).
template <bool BF = false>
__device__ __forceinline__ bool skip_rows(const ScoreArgs &p)
{
    bool skip = p.skip_masked != 0 && __builtin_amdgcn_readfirstlane(*p.nonfinite) == 0;
    if constexpr (BF) skip = skip && __builtin_amdgcn_readfirstlane(*p.nonfinite_bf) == 0;   // the mirror's own word as well
    return skip;
}

template <bool NT>
__device__ __forceinline__ v4f ld4(const v4f *p)
{
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

// A lane's four columns of a Personal_Memory row as they are loaded: a float4, or in the mirror forms (BF) the four bf16 halves in
// one 8-byte word, kept packed until they are used (the row buffers are half the registers) and widened by shifts, which is exact.
typedef uint32_t v2u __attribute__((ext_vector_type(2)));
template <bool BF> struct pm_row { typedef v4f type; };
template <> struct pm_row<true> { typedef v2u type; };

template <bool NT>
__device__ __forceinline__ v2u ld4(const v2u *p)
{
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

__device__ __forceinline__ v4f widen(const v4f &x) { return x; }
__device__ __forceinline__ v4f widen(const v2u &w)
{
    return v4f{__builtin_bit_cast(float, w.x << 16), __builtin_bit_cast(float, w.x & 0xffff0000u),
               __builtin_bit_cast(float, w.y << 16), __builtin_bit_cast(float, w.y & 0xffff0000u)};
}

__device__ __forceinline__ float dot4(const v4f &x, const v4f &y, float acc)
{
    acc = fmaf(x.x, y.x, acc);
    acc = fmaf(x.y, y.y, acc);
    acc = fmaf(x.z, y.z, acc);
    acc = fmaf(x.w, y.w, acc);
    return acc;
}

__device__ __forceinline__ v4f scale4(float s, const v4f &x) { return s * x; }

// Sum over the LPP lanes of a group; every lane of the group ends with the total.
template <int LPP>
__device__ __forceinline__ float group_sum(float v)
{
#pragma unroll
    for (int off = LPP / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// A pair's ids as the kernels use them: the user's row in this engine's block of users, the dish, both clamped to row 0 when out
// of range (the loads stay in bounds, the score becomes NaN: `bad`).  The user error is latched before the item error; `report`
// says whether this lane writes the latch (the lanes of a group that share a pair report once), EVERY: each lane has a pair of its own.
struct PairIds {
    int64_t ul;
    int32_t did;
    bool bad;
};

template <bool EVERY>
__device__ __forceinline__ PairIds pair_ids(const ScoreArgs &p, const int64_t pi, const bool valid, const bool report = true)
{
    const int32_t uid = valid ? p.users[pi] : (int32_t)p.user_base;
    PairIds r;
    r.did = valid ? p.items[pi] : 0;
    r.ul = (int64_t)uid - p.user_base;
    r.bad = false;
    if (r.ul < 0 || r.ul >= p.U) {
        if (EVERY || report) m2d_latch_error(p.err, M2D_ERR_BAD_USER_ID, uid, pi);
        r.ul = 0;
        r.bad = true;
    }
    if (r.did < 0 || (int64_t)r.did >= p.I) {
        if (EVERY || report) m2d_latch_error(p.err, M2D_ERR_BAD_ITEM_ID, r.did, pi);
        r.did = 0;
        r.bad = true;
    }
    return r;
}

// The score of pair `pi`: NaN when one of its ids was out of range.
__device__ __forceinline__ void put_score(const ScoreArgs &p, const int64_t pi, const bool bad, float score)
{
    if (bad) score = __builtin_nanf("");
    p.out[pi] = score;
}

// From a pair's two group sums to its stored score.  HV: `high` is <U_high, H[d]>, H[d] is already normalised.
template <bool HV>
__device__ __forceinline__ void store_score(const ScoreArgs &p, const int64_t pi, const bool bad, const float n, const float hs, const float ls)
{
    const float high = HV ? hs : hs / n;                                       // :79
    const float low = ls / n;                                                  // :92
    put_score(p, pi, bad, m2d_blend_unfused(p.a, high, p.b, low));             // :95-96, no fma contraction
}

// The same for the four weights of a C = 4 pair; use_uh: the high-level sum is sum_c m_c <U_high, CE_c> from the derived table
template <bool HV, bool use_uh>
__device__ __forceinline__ void store_score(const ScoreArgs &p, const int64_t pi, const bool bad, const v4f &m, float hs, const float ls,
                                            const v4f &uhv = v4f{0.f, 0.f, 0.f, 0.f})
{
    const float n = (m.x + m.y) + (m.z + m.w);                                 // :77
    if constexpr (use_uh) hs = fmaf(m.w, uhv.w, fmaf(m.z, uhv.z, fmaf(m.y, uhv.y, m.x * uhv.x)));
    store_score<HV>(p, pi, bad, n, hs, ls);
}

// A lane's place in its group of LPP lanes: lane j holds float4 column j of every row, E / 4 <= LPP columns.  FULL: E / 4 == LPP,
// no idle lanes.  cef: the lane's column of the C <= NC rows of Category_Embedding.  MASK: how an idle lane's `hs` is dropped, see `keep`.
template <int LPP, bool FULL, int NC, bool MASK = true>
struct LaneGroup {
    int j, E4, jc;
    bool col_ok;
    int32_t keep;
    v4f cef[NC];

    __device__ __forceinline__ LaneGroup(const float *ce, const int E, const int C)
    {
        j = threadIdx.x & (LPP - 1);
        E4 = FULL ? LPP : (E >> 2);
        col_ok = FULL || (j < E4);
        jc = col_ok ? j : 0;  // idle lanes re-read column 0 (in bounds), contribution zeroed
        // Idle lanes hold U_high's column 0 and cef = 0: 0 * inf would be NaN, so their `hs` is dropped like their `ls`.  As an AND
        // with a lane mask the compiler cannot see through: written as a select, it moved the whole high-level chain under the lane
        // condition and the default instantiations took 10 to 60 more VGPRs (LPP 16, PF 2: 144 -> 204); this form takes 2.
        // (m2d_score_pairs_cn keeps the select it always had, MASK = false: its chain sits under the wave-uniform c < C branches,
        // the select moves nothing there and the AND costs 1-2 VGPRs more, LPP 32: 176 against 174.)
        keep = col_ok ? -1 : 0;
        asm volatile("" : "+v"(keep));
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            cef[c] = v4f{0.f, 0.f, 0.f, 0.f};
            if (c < C) {
                cef[c] = reinterpret_cast<const v4f *>(ce)[(size_t)c * E4 + jc];
                if (!col_ok) cef[c] = v4f{0.f, 0.f, 0.f, 0.f};
            }
        }
    }

    __device__ __forceinline__ float drop_idle(const float v) const
    {
        if constexpr (FULL) return v;
        else if constexpr (!MASK) return col_ok ? v : 0.f;
        else return __builtin_bit_cast(float, __builtin_bit_cast(int32_t, v) & keep);
    }
};

// Issue the loads of the pair that lane s of the group holds (its user row, dish and row bits: ul, did, act) into one slot of row
// buffers: ub = U_high and the NB - 1 category rows, ib the dish row, hb H[d].  act: bit c set = category c's row is fetched (bits >= C
// are never set); use_uh: the U_high row is not fetched at all.  row_t v2u: the user rows come from the bf16 mirror.
// The shuffles stand here, next to their uses: passed in as arguments they were all placed ahead of the row loads and the default
// mirror instantiation took 10 more VGPRs.
template <int LPP, bool NT, bool HV, bool use_uh, int NB, typename row_t, typename G>
__device__ __forceinline__ void fetch_pair(row_t (&ub)[NB], v4f &ib, v4f &hb, const ScoreArgs &p, const G &g, const int C, const int32_t ul, const int32_t did,
                                           const int32_t act, const int s)
{
    const int32_t us = __shfl(ul, s, LPP);
    const int32_t ds = __shfl(did, s, LPP);
    const int32_t as = __shfl(act, s, LPP);
    constexpr bool BF = std::is_same<row_t, v2u>::value;
    const row_t *pm4 = BF ? reinterpret_cast<const row_t *>(p.pmh) : reinterpret_cast<const row_t *>(p.pm);
    const size_t urow4 = (size_t)(C + 1) * g.E4;  // float4 (mirror: 8-byte words) per user block
    const row_t *pu = pm4 + (size_t)us * urow4 + g.jc;
    if constexpr (use_uh) ub[0] = row_t{};
    else ub[0] = ld4<NT>(pu);
#pragma unroll
    for (int r = 1; r < NB; ++r) {
        ub[r] = row_t{};
        if ((as >> (r - 1)) & 1) ub[r] = ld4<NT>(pu + (size_t)r * g.E4);
    }
    ib = reinterpret_cast<const v4f *>(p.re)[(size_t)ds * g.E4 + g.jc];
    if constexpr (HV) hb = reinterpret_cast<const v4f *>(p.hv)[(size_t)ds * g.E4 + g.jc];
}

// A lane's share of a pair's two dot products; weight(c) is the pair's mask weight of category c, asked for only under the
// wave-uniform c < C.  HV (build-defined extension): the high-level operand sum_c m_c CE_c / n of
// Model_Recommender.py:67-79 is replaced by a resident per-dish vector H[d] (the normalised multi-hot ingredient sum), i.e.
// high = <U_high, H[d]>; the low-level path is unchanged.  The order of the fmaf chain is the scores' bits: every form shares it.
template <bool HV, bool use_uh, int NB, typename row_t, typename G, typename W>
__device__ __forceinline__ void pair_partial(const row_t (&ub)[NB], const v4f &ib, const v4f &hb, const G &g, const int C, const W weight, float &hs, float &ls)
{
    hs = 0.f;
    ls = 0.f;
    const v4f uhigh = widen(ub[0]);
#pragma unroll
    for (int c = 0; c < NB - 1; ++c) {
        if (c < C) {
            const float mc = weight(c);
            if constexpr (!HV && !use_uh) {
                const v4f dish_category = scale4(mc, g.cef[c]);           // :67
                hs = dot4(uhigh, dish_category, hs);                      // :71, :75
            }
            const v4f dish_memory = scale4(mc, widen(ub[c + 1]));     // :82
            ls = dot4(ib, dish_memory, ls);                           // :86, :90
        }
    }
    if constexpr (HV) hs = dot4(uhigh, hb, hs);
    if (!g.col_ok) ls = 0.f;
    hs = g.drop_idle(hs);
}

// A group's walk over its LPP pairs (lane s of the group holds pair s's ids, row bits and weights), the rows of PF pairs in flight
// ahead of the arithmetic; lane s ends with pair s's two sums.  No shuffle here runs under a partial EXEC mask.
template <int LPP, int PF, bool NT, bool HV, bool use_uh, int NR, typename row_t, typename G, typename W>
__device__ __forceinline__ void walk_pairs(const ScoreArgs &p, const G &g, const int C, const int32_t ul, const int32_t did, const int32_t act,
                                           const W weight, float &my_high, float &my_low)
{
    row_t ub[PF][NR + 1];
    v4f ib[PF], hb[PF];
    auto issue = [&](const int s, const int k) { fetch_pair<LPP, NT, HV, use_uh>(ub[k], ib[k], hb[k], p, g, C, ul, did, act, s); };
#pragma unroll
    for (int k = 0; k < PF; ++k) issue(k, k);
    for (int s0 = 0; s0 < LPP; s0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int s = s0 + k;
            float hs, ls, mc[NR];
#pragma unroll
            for (int c = 0; c < NR; ++c) {
                mc[c] = 0.f;
                if (c < C) mc[c] = weight(s, c);           // pair s's weights: shuffled ahead of the arithmetic
            }
            pair_partial<HV, use_uh>(ub[k], ib[k], hb[k], g, C, [&](const int c) { return mc[c]; }, hs, ls);
            if (s + PF < LPP) issue(s + PF, k);
            if constexpr (HV || !use_uh) hs = group_sum<LPP>(hs);
            ls = group_sum<LPP>(ls);
            if (g.j == s) {
                my_high = hs;
                my_low = ls;
            }
        }
    }
}

// C == 4 categories, E % 4 == 0, E / 4 <= LPP.
// UH is its own instantiation: the literal kernel's code, and with it its bits, stay what they were.
// BF (option "pm_bf16"): the Personal_Memory rows come from the bf16 mirror; everything after the load is the same code, so the
// scores are the f32 form's on the rounded table, bit for bit.
template <int LPP, int PF, bool BYDISH, bool NT, bool FULL, bool HV, bool UH = false, bool BF = false>
__global__ __launch_bounds__(256) void m2d_score_pairs_c4(ScoreArgs p)
{
    static_assert(!(UH && BF), "the mirror forms read U_high from the mirror");
    constexpr bool use_uh = UH && !HV;
    const int lane = threadIdx.x & 63;
    const int64_t nchunks = (p.B + 63) >> 6;
    // wave-uniform loop control lives in SGPRs
    const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const bool skipm = skip_rows<BF>(p);
    const LaneGroup<LPP, FULL, 4> g(p.ce, p.E, 4);

    for (int64_t chunk = wave0; chunk < nchunks; chunk += nwaves) {
        const int64_t pi = (chunk << 6) + lane;
        const bool valid = pi < p.B;
        const PairIds id = pair_ids<true>(p, pi, valid);
        v4f m = {0.f, 0.f, 0.f, 0.f};
        if (valid) m = reinterpret_cast<const v4f *>(p.cats)[BYDISH ? id.did : pi];
        v4f uhv = {0.f, 0.f, 0.f, 0.f};
        if constexpr (use_uh) uhv = reinterpret_cast<const v4f *>(p.uh)[id.ul];
        float my_high = 0.f, my_low = 0.f;
        // categories whose weight is exactly 0 contribute 0 * U_low[c] = 0 to :82-:90: their rows are not fetched
        // (a NaN weight compares unequal to 0 and keeps its row)
        const int32_t act = skipm ? ((m.x != 0.f ? 1 : 0) | (m.y != 0.f ? 2 : 0) | (m.z != 0.f ? 4 : 0) | (m.w != 0.f ? 8 : 0)) : 15;
        walk_pairs<LPP, PF, NT, HV, use_uh, 4, typename pm_row<BF>::type>(p, g, 4, (int32_t)id.ul, id.did, act,
                                                                          [&](const int s, const int c) { return __shfl(m[c], s, LPP); }, my_high, my_low);
        if (valid) store_score<HV, use_uh>(p, pi, id.bad, m, my_high, my_low, uhv);
    }
}

// Derived table for serving: uh[u][c] = <U_high[u], CE_c>, c < 4.  The high-level sum of Model_Recommender.py:67-79 is
// sum_c m_c uh[u][c] / n -- the same products in another order -- so a pair reads 16 bytes of this table (16 B x U: it
// lives in L2 / the Infinity Cache) instead of the E x 4-byte U_high row from HBM.  One group of E/4 lanes per user.
template <int LPP>
__global__ __launch_bounds__(256) void m2d_build_user_high(const float *pm, const float *ce, int64_t U, int32_t E, float *out)
{
    constexpr int C = 4;
    const LaneGroup<LPP, false, C> g(ce, E, C);
    const int64_t gpw = 64 / LPP;
    const int64_t g0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * gpw + (threadIdx.x & 63) / LPP;
    for (int64_t u = g0; u < ((U + gpw - 1) / gpw) * gpw; u += (int64_t)gridDim.x * 4 * gpw) {   // whole groups: full-wave shuffles
        const bool ok = u < U;
        const v4f x = reinterpret_cast<const v4f *>(pm)[(size_t)(ok ? u : 0) * (C + 1) * g.E4 + g.jc];
        float h[C];
#pragma unroll
        for (int c = 0; c < C; ++c) h[c] = group_sum<LPP>(g.drop_idle(dot4(x, g.cef[c], 0.f)));   // idle lanes: not 0 * U_high[u][0..3]
        if (ok && g.j == 0) reinterpret_cast<v4f *>(out)[u] = v4f{h[0], h[1], h[2], h[3]};
    }
}

// Serving mirror (option "pm_bf16"): out[i] = bf16(pm[i]), round to nearest even in the integer form -- add 0x7fff and the kept
// part's lowest bit, shift -- which rounds subnormals, keeps -0 and +-inf and turns finite values past the bf16 range into +-inf; a NaN
// becomes the quiet NaN 0x7fc0 (what torch's float32 -> bfloat16 returns).  A grid-stride stream of 16-byte loads and 8-byte stores; the
// n % 4 floats behind the last whole float4 go one by one.  *nonfinite (zeroed by the launcher) is set when a written value is inf / NaN.
__device__ __forceinline__ uint32_t bf16_rne(const float x)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__global__ __launch_bounds__(256) void m2d_build_pm_bf16(const float *pm, int64_t n, uint16_t *out, int32_t *nonfinite)
{
    const int64_t n4 = n >> 2, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    uint32_t bad = 0;
    for (int64_t i = t0; i < n4; i += stride) {
        const v4f x = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(pm) + i);
        const uint32_t h0 = bf16_rne(x.x), h1 = bf16_rne(x.y), h2 = bf16_rne(x.z), h3 = bf16_rne(x.w);
        bad |= (h0 & 0x7f80u) == 0x7f80u || (h1 & 0x7f80u) == 0x7f80u || (h2 & 0x7f80u) == 0x7f80u || (h3 & 0x7f80u) == 0x7f80u;
        reinterpret_cast<v2u *>(out)[i] = v2u{h0 | (h1 << 16), h2 | (h3 << 16)};
    }
    for (int64_t i = (n4 << 2) + t0; i < n; i += stride) {
        const uint32_t hh = bf16_rne(pm[i]);
        bad |= (hh & 0x7f80u) == 0x7f80u;
        out[i] = (uint16_t)hh;
    }
    if (bad) atomicOr(nonfinite, 1);
}

// Latency form of m2d_score_pairs_c4 for small batches (serving calls, the reference's own 51 pairs per sess.run):
// a group of LPP lanes takes ONE pair per pass instead of walking LPP pairs one after another, so a batch of B
// pairs is spread over B * LPP / 64 waves and finishes in about one row-gather latency instead of up to 64 of
// them in sequence.  The same pair_partial and the same group reduction: bit-identical scores.
template <int LPP, bool BYDISH, bool FULL, bool HV, bool BF = false>
__global__ __launch_bounds__(256) void m2d_score_pairs_c4_small(ScoreArgs p)
{
    typedef typename pm_row<BF>::type row_t;                // BF: rows from the bf16 mirror, see m2d_score_pairs_c4
    constexpr int GPW = 64 / LPP;                           // pairs per wave per pass
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const bool skipm = skip_rows<BF>(p);
    const LaneGroup<LPP, FULL, 4> g(p.ce, p.E, 4);
    for (int64_t base = wave0 * GPW; base < p.B; base += nwaves * GPW) {
        const int64_t pi = base + lane / LPP;
        const bool valid = pi < p.B;
        const PairIds id = pair_ids<false>(p, pi, valid, g.j == 0);
        v4f m = {0.f, 0.f, 0.f, 0.f};
        if (valid) m = reinterpret_cast<const v4f *>(p.cats)[BYDISH ? id.did : pi];
        // plain loads of the pair's own rows (no shuffle, no slot): fetch_pair's form of them cost this kernel occupancy
        const row_t *pu = (BF ? reinterpret_cast<const row_t *>(p.pmh) : reinterpret_cast<const row_t *>(p.pm)) + (size_t)id.ul * ((size_t)5 * g.E4) + g.jc;
        row_t ub[5];
        v4f ib, hb = {0.f, 0.f, 0.f, 0.f};
        ub[0] = pu[0];
#pragma unroll
        for (int r = 1; r <= 4; ++r) {                     // a category of weight 0 contributes 0: its row is not fetched
            ub[r] = row_t{};
            if (!skipm || m[r - 1] != 0.f) ub[r] = pu[(size_t)r * g.E4];
        }
        ib = reinterpret_cast<const v4f *>(p.re)[(size_t)id.did * g.E4 + g.jc];
        if constexpr (HV) hb = reinterpret_cast<const v4f *>(p.hv)[(size_t)id.did * g.E4 + g.jc];
        float hs, ls;
        pair_partial<HV, false>(ub, ib, hb, g, 4, [&](const int c) { return m[c]; }, hs, ls);
        hs = group_sum<LPP>(hs);
        ls = group_sum<LPP>(ls);
        if (valid && g.j == 0) store_score<HV, false>(p, pi, id.bad, m, hs, ls);
    }
}

// The throughput form for category counts other than 4 (1 <= C <= 8, E % 4 == 0, E / 4 <= LPP): the walk of
// m2d_score_pairs_c4, two pairs' rows in flight, with the category loop unrolled to 8 and every c >= C step skipped by
// a wave-uniform branch (no 0 * row products are added for categories the model does not have).  Mask weights are read
// as scalars (a pair's C weights are not a float4) and n is their sum in category order.  One wave per pair, as
// m2d_score_pairs_generic does it, reaches 1.3-2.1 G pairs/s on config-2 sized tables where this form reaches the rate
// of the C = 4 kernel.
template <int LPP, bool BYDISH, bool NT>
__global__ __launch_bounds__(256) void m2d_score_pairs_cn(ScoreArgs p)
{
    constexpr int CM = 8, PF = 2;
    const int C = p.C;
    const int lane = threadIdx.x & 63;
    const int64_t nchunks = (p.B + 63) >> 6;
    const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const bool skipm = skip_rows(p);
    const LaneGroup<LPP, false, CM, false> g(p.ce, p.E, C);

    for (int64_t chunk = wave0; chunk < nchunks; chunk += nwaves) {
        const int64_t pi = (chunk << 6) + lane;
        const bool valid = pi < p.B;
        const PairIds id = pair_ids<true>(p, pi, valid);
        float mk[CM];
        int32_t act = 0;
        float n = 0.f;
        const float *mrow = p.cats + (BYDISH ? (size_t)id.did : (size_t)pi) * C;
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            mk[c] = 0.f;
            if (c < C) {
                if (valid) mk[c] = mrow[c];
                n += mk[c];                                                // :77
                // weight exactly 0: 0 * U_low[c] = 0 at :82-:90, the row is not fetched (a NaN weight keeps its row)
                act |= (!skipm || mk[c] != 0.f) ? (1 << c) : 0;
            }
        }
        float my_high = 0.f, my_low = 0.f;
        walk_pairs<LPP, PF, NT, false, false, CM, v4f>(p, g, C, (int32_t)id.ul, id.did, act,
                                                       [&](const int s, const int c) { return __shfl(mk[c], s, LPP); }, my_high, my_low);
        if (valid) store_score<false>(p, pi, id.bad, n, my_high, my_low);
    }
}

// Any C (<= 64), any E: one wave per pair, lanes stride over e.  Slow path for shapes the
// vectorised kernels do not cover (E % 4 != 0, E > 256, C > 8) and the latency path of C != 4.
template <bool BYDISH>
__global__ __launch_bounds__(256) void m2d_score_pairs_generic(ScoreArgs p)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int C = p.C, E = p.E;
    const bool skipm = skip_rows(p);
    for (int64_t pi = wave0; pi < p.B; pi += nwaves) {
        const PairIds id = pair_ids<false>(p, pi, true, lane == 0);
        const float *um = p.pm + (size_t)id.ul * (size_t)(C + 1) * E;
        const float *it = p.re + (size_t)id.did * E;
        const float *mrow = p.cats + (BYDISH ? (size_t)id.did * C : (size_t)pi * C);
        const float score = m2d_pair_score_wave(um, it, mrow, p.ce, p.hv ? p.hv + (size_t)id.did * E : nullptr, C, E, p.a, p.b, skipm, lane);
        if (lane == 0) put_score(p, pi, id.bad, score);
    }
}

// ---- launcher ----

// Run-time values as compile-time ones: f gets std::integral_constant<int, v> for the v among V... (false: none of them), or
// std::bool_constant<b>.
template <int... V, typename F>
bool pick(const int v, F &&f)
{
    return ((v == V && (f(std::integral_constant<int, V>{}), true)) || ...);
}

template <typename F>
void pick_flag(const bool b, F &&f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// lanes per pair (and pairs per group step) of the lane-group kernels: the power of two that holds the E / 4 columns
constexpr int lpp_for(const int E4) { return E4 <= 8 ? 8 : E4 <= 16 ? 16 : E4 <= 32 ? 32 : 64; }

// f(LPP, FULL) for a row of E4 float4 columns, E4 <= 64
template <typename F>
void with_width(const int E4, F &&f)
{
    pick<8, 16, 32, 64>(lpp_for(E4), [&](auto lpp) { pick_flag(E4 == lpp(), [&](auto full) { f(lpp, full); }); });
}

// the vectorised C = 4 kernels (m2d_score_pairs_c4, _c4_small) serve this engine
bool serves_c4(const m2d_engine *h) { return h->C == 4 && h->E % 4 == 0 && h->E <= 256 && h->opt_variant != 9; }

// what m2d_last_kernel reports: the kernel form, "_bf16" behind the forms that read the mirror
const char *kernel_name(const bool c4, const bool cn, const bool small, const bool hv, const bool uh, const bool bf)
{
    static const char *const c4_names[2][2][2] = {
        {{"m2d_score_pairs_c4", "m2d_score_pairs_c4_bf16"}, {"m2d_score_pairs_c4_hv", "m2d_score_pairs_c4_hv_bf16"}},
        {{"m2d_score_pairs_c4_small", "m2d_score_pairs_c4_small_bf16"}, {"m2d_score_pairs_c4_small_hv", "m2d_score_pairs_c4_small_hv_bf16"}}};
    if (!c4) return cn ? "m2d_score_pairs_cn" : "m2d_score_pairs_generic";
    return uh ? "m2d_score_pairs_c4_uh" : c4_names[small][hv][bf];
}

template <bool BYDISH>
int launch_any(m2d_engine *h, const ScoreArgs &a, hipStream_t st)
{
    const int64_t nchunks = (a.B + 63) >> 6;
    const int pf = h->opt_prefetch == 1 || h->opt_prefetch == 4 ? h->opt_prefetch : 2;
    const bool nt = h->opt_nt != 0, hv = a.hv != nullptr, bf = a.pmh != nullptr;
    const int E4 = a.E >> 2, per_cu = h->opt_blocks_per_cu > 0 ? h->opt_blocks_per_cu : 8;
    const bool c4 = serves_c4(h);
    // up to 8192 pairs: the latency form (option "variant" = 11 forces the throughput form, 12 the latency form)
    const bool small = c4 && ((a.B <= 8192 && h->opt_variant != 11) || h->opt_variant == 12);
    const bool cn = !c4 && a.C <= 8 && (a.E % 4 == 0) && E4 <= 64 && !hv && a.B > 8192 && h->opt_variant != 9;
    // the derived table serves the throughput form without the ingredient table: PF 2 / 4, non-temporal user rows (m2d_launch_score_pairs)
    const bool uh = c4 && !small && !hv && a.uh != nullptr;
    if (!c4 && !cn && a.C > 64) {
        h->last_error = "num_categories > 64 is not supported";
        return M2D_ERR_UNSUPPORTED;
    }
    h->last_kernel = kernel_name(c4, cn, small, hv, uh, bf);
    // work per block of 4 waves: 4 chunks of 64 pairs; latency form: 4 waves' worth of groups and one block more; generic: 4 pairs
    const dim3 grid(m2d_blocks_for(h, small ? a.B * lpp_for(E4) / 64 + 4 : c4 || cn ? nchunks : a.B, 4, per_cu));
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a); };
    if (c4)
        with_width(E4, [&](auto lpp, auto full) {
            pick_flag(bf, [&](auto mirror) {
                constexpr int LPP = decltype(lpp)::value;
                constexpr bool FULL = decltype(full)::value, BF = decltype(mirror)::value;
                if (small) pick_flag(hv, [&](auto v) { launch(m2d_score_pairs_c4_small<LPP, BYDISH, FULL, decltype(v)::value, BF>); });
                else if (hv) launch(m2d_score_pairs_c4<LPP, 2, BYDISH, true, FULL, true, false, BF>);   // one configuration: PF 2, non-temporal
                else if (uh) {
                    if constexpr (!BF) pick<2, 4>(pf, [&](auto d) { launch(m2d_score_pairs_c4<LPP, decltype(d)::value, BYDISH, true, FULL, false, true>); });
                } else
                    pick<1, 2, 4>(pf, [&](auto d) {
                        pick_flag(nt, [&](auto t) { launch(m2d_score_pairs_c4<LPP, decltype(d)::value, BYDISH, decltype(t)::value, FULL, false, false, BF>); });
                    });
            });
        });
    else if (cn)
        with_width(E4, [&](auto lpp, auto) { pick_flag(nt, [&](auto t) { launch(m2d_score_pairs_cn<decltype(lpp)::value, BYDISH, decltype(t)::value>); }); });
    else
        launch(m2d_score_pairs_generic<BYDISH>);
    M2D_HIP_TRY(h, hipGetLastError());
    return M2D_OK;
}

}  // namespace

int m2d_ensure_user_high(m2d_engine *h, hipStream_t stream)
{
    if (h->user_high_valid) return M2D_OK;
    if (int rc = h->user_high.grow(h, (size_t)h->U * 4)) return rc;
    const int E4 = h->E >> 2;
    const dim3 grid(m2d_blocks_for(h, h->U * lpp_for(E4) / 64 + 4, 4, 16));
    with_width(E4, [&](auto lpp, auto) {
        hipLaunchKernelGGL((m2d_build_user_high<decltype(lpp)::value>), grid, dim3(256), 0, stream, h->pm, h->ce, h->U, h->E, h->user_high);
    });
    M2D_HIP_TRY(h, hipGetLastError());
    h->user_high_valid = true;
    return M2D_OK;
}

// The bf16 mirror of Personal_Memory, current: built on first use and again after a write (m2d_mark_written), a whole pass over the
// table.  Its non-finite word is zeroed and set again with every build.
int m2d_ensure_pm_bf16(m2d_engine *h, hipStream_t stream)
{
    if (h->pm_bf16_valid) return M2D_OK;
    const int64_t n = m2d_table_floats(h, 0);
    if (int rc = h->pm_bf16.grow(h, (size_t)n)) return rc;
    M2D_HIP_TRY(h, hipMemsetAsync(h->pm_bf16_nonfinite, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(m2d_build_pm_bf16, dim3(m2d_blocks_for(h, n / 4, 256)), dim3(256), 0, stream, h->pm, n, h->pm_bf16, h->pm_bf16_nonfinite);
    M2D_HIP_TRY(h, hipGetLastError());
    h->pm_bf16_valid = true;
    return M2D_OK;
}

int m2d_launch_score_pairs(m2d_engine *h, const int32_t *users, const int32_t *items, const float *cats,
                           bool by_dish, int64_t B, float *out, hipStream_t stream, bool use_ingredients, bool may_use_mirror)
{
    if (B == 0) return M2D_OK;
    {
        const int rc = m2d_ensure_finite_scan(h, stream);
        if (rc != M2D_OK) return rc;
    }
    ScoreArgs a;
    a.nonfinite = h->nonfinite_dev;
    a.hv = use_ingredients ? h->dish_high : nullptr;
    a.pm = h->pm; a.re = h->re; a.ce = h->ce;
    a.users = users; a.items = items; a.cats = cats; a.out = out;
    a.B = B; a.U = h->U; a.I = h->I; a.user_base = h->user_base;
    a.E = h->E; a.C = h->C; a.a = h->a; a.b = h->b; a.err = h->err_dev;
    a.skip_masked = h->opt_skip_masked;
    a.uh = nullptr;
    a.pmh = nullptr;
    a.nonfinite_bf = h->pm_bf16_nonfinite;
    // opt-in ("pm_bf16"): whenever the vectorised C = 4 kernels run, they read the user rows from the bf16 mirror -- whatever the
    // batch size, so a call's scores depend on its inputs and options only.  The mirror wins over "user_high_table".
    // (m2d_rank_candidates passes may_use_mirror = false: the evaluator's lists stay the f32 table's.)
    if (may_use_mirror && h->opt_pm_bf16 && serves_c4(h)) {
        const int rc = m2d_ensure_pm_bf16(h, stream);
        if (rc != M2D_OK) return rc;
        a.pmh = h->pm_bf16;
    }
    // opt-in ("user_high_table"): batches large enough to pay for a pass over U_high take the high-level sum from the derived
    // table (rebuilt when Personal_Memory / Category_Embedding changed); smaller ones never do, so a call's scores depend
    // on its inputs and its size only, not on what ran before
    if (!a.pmh && !use_ingredients && h->opt_user_high && serves_c4(h) && (h->opt_prefetch == 2 || h->opt_prefetch == 4) && h->opt_nt != 0 &&
        B >= (1 << 18)) {
        int rc = m2d_ensure_user_high(h, stream);
        if (rc != M2D_OK) return rc;
        a.uh = h->user_high;
    }
    return by_dish ? launch_any<true>(h, a, stream) : launch_any<false>(h, a, stream);
}
