// Device core of the matcher kernels (match.hip, match_knn.hip): the top-2 and
// key arithmetic, the gate policies, the fp16 block, the LDS staging of train
// tiles, the integer fold, the split rule and the split merge.  The
// bit-exactness rules -- the tie order, INT_MIN against kPadBias, rows past nt
// losing -- live here and nowhere else.  Function boundaries in these kernels
// decide the instruction stream (the note above block_queries): the functions
// are what the kernels measured in profiles/ were compiled from.
#pragma once
#include <float.h>
#include <limits.h>

#include <type_traits>

#include "sift_epipolar.h"
#include "sift_kernels.h"
#include "sift_match.h"
#include "sift_math.h"

namespace sift_amd {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kNone = 0x7fffffff;
// Row keys: key = 512 dot - (256 |c_t|^2 + r) orders (d^2, train row) in
// reverse for one query, where r < 256 is the row's index inside its group of
// kGroupTiles tiles: 256 (2 dot - |c_t|^2) = 256 (|c_q|^2 - d^2) lies in
// [-2^31 + 2^24, 2^29] for any codes (d^2 <= 128 * 255^2 < 2^23), so every key
// is an exact int32.  A padding row has zero codes and key kPadBias, below
// every valid key.
constexpr int kGroupTiles = 8;
constexpr int kPadBias = kMatchPadKey;
constexpr int kInvalidKey = kPadBias;  // keys <= this are padding rows (or none)

struct Top2 {
    float d1, d2;
    int i1, i2;
};

__device__ __forceinline__ bool better(float da, int ia, float db, int ib) {
    return da < db || (da == db && ia < ib);
}

// Top-2 of the union of two disjoint sorted pairs, (distance, index) order.
// Written with value selects only (no struct-reference selects -> no scratch).
__device__ __forceinline__ Top2 merge_top2(const Top2 a, const Top2 b) {
    const bool bfirst = better(b.d1, b.i1, a.d1, a.i1);
    // winner w, loser-head l (first of the other list), runner-up of the winner's list wn.
    const float wd = bfirst ? b.d1 : a.d1, ld = bfirst ? a.d1 : b.d1, wnd = bfirst ? b.d2 : a.d2;
    const int wi = bfirst ? b.i1 : a.i1, li = bfirst ? a.i1 : b.i1, wni = bfirst ? b.i2 : a.i2;
    const bool lsecond = better(ld, li, wnd, wni);
    Top2 r;
    r.d1 = wd;
    r.i1 = wi;
    r.d2 = lsecond ? ld : wnd;
    r.i2 = lsecond ? li : wni;
    return r;
}

__device__ __forceinline__ Top2 shfl_top2(const Top2& t, int mask) {
    Top2 r;
    r.d1 = __shfl_xor(t.d1, mask);
    r.d2 = __shfl_xor(t.d2, mask);
    r.i1 = __shfl_xor(t.i1, mask);
    r.i2 = __shfl_xor(t.i2, mask);
    return r;
}

// 16 fp16 descriptor values -> int8 codes c = v - 128 (4 dwords), adding
// sum c^2 to nrm; bad is set by a value that is not an integer 0..255 (NaN,
// infinities and -0 included), whose code is then meaningless (the caller
// falls back to the fp16 path).  Packed: v + 1024 puts an integer 0..1023 in
// the mantissa bits exactly (0x6400 | v for v < 256), one v_perm gathers four
// such low bytes, and v ^ 0x80 is v - 128 as int8; v_dot4 adds the squares.
__device__ __forceinline__ i32x4 codes16(const uint4 a, const uint4 b, int& nrm, bool& bad) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned y[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const h2 yv = __builtin_bit_cast(h2, w[e]) + (h2){(_Float16)1024.f, (_Float16)1024.f};
        const h2 back = yv - (h2){(_Float16)1024.f, (_Float16)1024.f};
        y[e] = __builtin_bit_cast(unsigned, yv);
        bad |= (y[e] & 0xff00ff00u) != 0x64006400u || __builtin_bit_cast(unsigned, back) != w[e];
    }
    i32x4 pk;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        pk[k] = (int)(__builtin_amdgcn_perm(y[2 * k + 1], y[2 * k], 0x06040200u) ^ 0x80808080u);
        nrm = __builtin_amdgcn_sdot4(pk[k], pk[k], nrm, false);
    }
    return pk;
}

// ---------------------------------------------------------------------------
// Integer path helpers.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int med3_i32(int a, int b, int c) {
    int r;
    __asm__("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ int max3_i32(int a, int b, int c) {
    int r;
    __asm__("v_max3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

struct Best {
    int e1, i1, e2, i2;  // e = d^2 - |c_q|^2 (kNone: no entry), i = train index
};

// Merge a key group's top-2 (max-keys m1 >= m2 of the group starting at train
// row t0) into the running pair.  The running entries come from earlier groups
// (lower train indices), so they win ties.
__device__ __forceinline__ Best fold_group(const Best b, int m1, int m2, int t0) {
    const int be1 = b.e1, bi1 = b.i1, be2 = b.e2, bi2 = b.i2;  // values: no member-address selects (scratch)
    const bool v1 = m1 > kInvalidKey, v2 = m2 > kInvalidKey;
    const int s1 = v1 ? -m1 : 0, s2 = v2 ? -m2 : 0;  // 256 e + r
    const int te1 = v1 ? (s1 >> 8) : kNone, ti1 = t0 + (s1 & 255);
    const int te2 = v2 ? (s2 >> 8) : kNone, ti2 = t0 + (s2 & 255);
    const bool c1 = te1 < be1;
    const bool c2 = c1 ? te2 < be1 : te1 < be2;
    Best r;
    r.e2 = c1 ? (c2 ? te2 : be1) : (c2 ? te1 : be2);
    r.i2 = c1 ? (c2 ? ti2 : bi1) : (c2 ? ti1 : bi2);
    r.e1 = c1 ? te1 : be1;
    r.i1 = c1 ? ti1 : bi1;
    return r;
}

__device__ __forceinline__ bool lt_ei(int ea, int ia, int eb, int ib) { return ea < eb || (ea == eb && ia < ib); }

__device__ __forceinline__ Best merge_best(const Best a, const Best b) {
    const bool bf = lt_ei(b.e1, b.i1, a.e1, a.i1);
    const int we = bf ? b.e1 : a.e1, wi = bf ? b.i1 : a.i1;
    const int le = bf ? a.e1 : b.e1, li = bf ? a.i1 : b.i1;  // head of the other list
    const int ne = bf ? b.e2 : a.e2, ni = bf ? b.i2 : a.i2;  // runner-up of the winner's list
    const bool ls = lt_ei(le, li, ne, ni);
    return Best{we, wi, ls ? le : ne, ls ? li : ni};
}

// ---------------------------------------------------------------------------
// General (fp16) path helpers.
// ---------------------------------------------------------------------------
__device__ __forceinline__ half8 load_frag(const uint16_t* row, int koff) {
    return *reinterpret_cast<const half8*>(row + koff);
}

// |v|^2 over a lane's eight 8-element fragments: v_dot2_f32_f16 in four chains.
__device__ __forceinline__ float sumsq8(const half8 (&v)[8]) {
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    float c[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 8; s++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const half2v x = {v[s][2 * j], v[s][2 * j + 1]};
            c[j] = __builtin_amdgcn_fdot2(x, x, c[j], false);
        }
    return (c[0] + c[1]) + (c[2] + c[3]);
}

// ---------------------------------------------------------------------------
// The gate (guided matching, k_match_guided) as a compile-time policy of the
// two match cores, chunk_top2 and match_f16_block.  Train row t is a candidate
// of query i when fabsf(tx - qx) <= radius && fabsf(ty - qy) <= radius
// (float32, one subtraction per axis, inclusive; a NaN coordinate is a
// candidate of nothing).  The distance matrix still lives in the accumulator
// only: the gate is a per-key predicate in the top-2 fold.  Instantiated with
// NoGate a core carries no position, query position or radius at all.
// ---------------------------------------------------------------------------
struct NoGate {};
template <class Gate>
constexpr bool kGated = !std::is_same<Gate, NoGate>::value;

__device__ __forceinline__ bool in_gate(float tx, float ty, float qx, float qy, float radius) {
    return __builtin_fabsf(tx - qx) <= radius && __builtin_fabsf(ty - qy) <= radius;
}

// The epipolar gate (k_match_epipolar): epi_query / epi_row / epi_pass / epi_pass2 of
// sift_epipolar.h, the one statement of the rule in include/sift_hip.h.

template <class Gate>
constexpr bool kEpipolar = std::is_same<Gate, EpipolarGate>::value;

// One wave's 32 queries (rows q0 + col of the pair) against train tiles
// [tbeg, tend): f16 MFMA (train rows as A, queries as B, so the accumulator's
// lane is the query and its 16 registers are train rows in increasing order),
// float top-2 with a strict '<' insert.  Returns the full d^2.  Under a gate
// (Gate = MatchGate) the insert also requires the row to lie in the query's
// window; lane col carries the position of train row t0 + col, as it carries
// its norm -- and under the epipolar gate the row's nr, computed once per
// tile row and shuffled with the position.
template <class Gate>
__device__ Top2 match_f16_block(const MatchPair& pr, const Gate& g, int q0, int tbeg, int tend, int col, int h) {
    const int qrow = q0 + col;
    const bool qvalid = qrow < pr.nq;
    half8 bq[8];
#pragma unroll
    for (int s = 0; s < 8; s++) bq[s] = qvalid ? load_frag(pr.q + (size_t)qrow * 128, 16 * s + 8 * h) : half8{};
    float qx = NAN, qy = NAN;
    if constexpr (kGated<Gate>) {
        qx = qvalid ? g.qxy[(size_t)qrow * g.qstride] : NAN;
        qy = qvalid ? g.qxy[(size_t)qrow * g.qstride + 1] : NAN;
    }
    // |q|^2: under the epipolar gate after the tile loop (bq lives across it
    // anyway), one register less inside it -- the budget of k_match_epipolar.
    float qn = 0.f;
    if constexpr (!kEpipolar<Gate>) {
        qn = sumsq8(bq);
        qn += __shfl_xor(qn, 32);
    }
    EpiQuery eq{};
    if constexpr (kEpipolar<Gate>) eq = epi_query(g.F, qx, qy);
    Top2 best{INFINITY, INFINITY, kNone, kNone};
    for (int tile = tbeg; tile < tend; tile++) {
        const int t0 = tile * kMatchTileRows, trow = t0 + col;
        const bool tvalid = trow < pr.nt;
        half8 a[8];
#pragma unroll
        for (int s = 0; s < 8; s++) a[s] = tvalid ? load_frag(pr.t + (size_t)trow * 128, 16 * s + 8 * h) : half8{};
        float tx = NAN, ty = NAN;
        if constexpr (kGated<Gate>) {
            tx = tvalid ? g.txy[(size_t)trow * g.tstride] : NAN;
            ty = tvalid ? g.txy[(size_t)trow * g.tstride + 1] : NAN;
        }
        float tn = sumsq8(a);
        tn += __shfl_xor(tn, 32);
        float tv = 0.f;  // epipolar only
        if constexpr (kEpipolar<Gate>) tv = epi_row(g.F, tx, ty);
        f32x16 acc = {}, acc2 = {};
#pragma unroll
        for (int s = 0; s < 8; s += 2) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], bq[s], acc, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s + 1], bq[s + 1], acc2, 0, 0, 0);
        }
        acc += acc2;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
            const float d = __shfl(tn, row) - 2.f * acc[i];
            bool cand = true;
            if constexpr (kEpipolar<Gate>)
                cand = epi_pass(eq, __shfl(tx, row), __shfl(ty, row), __shfl(tv, row), g.e2, g.radius);
            else if constexpr (kGated<Gate>)
                cand = in_gate(__shfl(tx, row), __shfl(ty, row), qx, qy, g.radius);
            if (t0 + row < pr.nt && cand && d < best.d2) {
                if (d < best.d1) {
                    best.d2 = best.d1;
                    best.i2 = best.i1;
                    best.d1 = d;
                    best.i1 = t0 + row;
                } else {
                    best.d2 = d;
                    best.i2 = t0 + row;
                }
            }
        }
    }
    best = merge_top2(best, shfl_top2(best, 32));
    if constexpr (kEpipolar<Gate>) {
        qn = sumsq8(bq);
        qn += __shfl_xor(qn, 32);
    }
    best.d1 += qn;
    best.d2 += qn;
    // tn, qn and the dot product are three fp32 sums rounded apart, so a d^2 near 0 (a duplicate row) can come out
    // below it: clamp (include/sift_hip.h, general path, item 1).  Every candidate of the query carries the same qn,
    // so no selection changes, and match_key's bit order needs d^2 >= 0.  A query row holding NaN or an infinity
    // (the only way to a qn that is not finite) has no neighbour: +Inf makes d = -Inf above, which would win.
    if (!(qn < INFINITY)) best = Top2{INFINITY, INFINITY, kNone, kNone};
    best.d1 = fmaxf(best.d1, 0.f);
    best.d2 = fmaxf(best.d2, 0.f);
    return best;
}

__device__ __forceinline__ unsigned long long match_key(float d2, int idx) {
    return idx == kNone ? ~0ull : ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)idx;
}

__device__ __forceinline__ void write_match(int i1, float e1, int i2, float e2, size_t o, const MatchOut& out) {
    if (out.idx2) {
        out.idx2[2 * o] = i1;
        out.idx2[2 * o + 1] = i2;
    }
    if (out.d2) {
        out.d2[2 * o] = e1;
        out.d2[2 * o + 1] = e2;
    }
    if (out.match) {
        int m = -1;
        if (i1 >= 0) {
            if (i2 < 0)
                m = i1;
            else if (out.ratio_on_squared)
                m = e1 < out.ratio * e2 ? i1 : -1;
            else
                m = __builtin_sqrtf(e1) < out.ratio * __builtin_sqrtf(e2) ? i1 : -1;
        }
        out.match[o] = m;
    }
}

// ---------------------------------------------------------------------------
// Integer-path building blocks shared by both kernels.
//
// Train tiles are staged in LDS a chunk (<= one key group of kGroupTiles
// tiles) at a time.  Code rows are stored unpadded (128 B) with their 16-byte
// pieces XOR-swizzled by (row >> 1) & 7, so a wave's ds_read_b128 of 32 rows x
// one piece covers the 64 banks once per 16-lane group; the swizzle also lets
// prepared codes go global -> LDS by LDS-DMA (a lane's source address is free,
// its LDS slot is lane x 16 B).
// ---------------------------------------------------------------------------
constexpr int kTileBytes = kMatchTileRows * 128;
// Waves per k_match_batch workgroup and 32-query blocks per wave (512 queries
// per workgroup).  (Measured alternative, round 3: 16 waves x 1 block, 42.1
// vs 39.1 us per C5 launch.)
constexpr int kMatchBatchNW = 8;
constexpr int kMatchBatchQBW = 2;
constexpr int kMatchBatchQB = 32 * kMatchBatchQBW * kMatchBatchNW;
constexpr int kMatchBatchWgPerCu = 2 * 8 / kMatchBatchNW > 0 ? 2 * 8 / kMatchBatchNW : 1;  // register budget: 16 waves per CU
constexpr int kChunkRows = kChunkTiles * kMatchTileRows;
static_assert(kChunkTiles == kGroupTiles, "a staged chunk is at most one key group");

__device__ __forceinline__ int piece_swz(int row, int piece) { return piece ^ ((row >> 1) & 7); }

// A wave's QBW 32-query B operands: lane (col, h) holds bytes [64h, 64h + 64)
// of query row q0w + 32 qb + col, one 16-byte fragment per MFMA; the A
// fragments take the same bytes of the train rows, so both sides pair the same
// descriptor dimensions in every K slot.  qn = |c_q|^2.
template <int QBW>
__device__ __forceinline__ void load_queries(const int8_t* __restrict__ qc, const int* __restrict__ qkeys, int nq,
                                             int q0w, int col, int h, i32x4 (&bq)[QBW][4], int (&qn)[QBW]) {
#pragma unroll
    for (int qb = 0; qb < QBW; qb++) {
        const int row = min(q0w + 32 * qb + col, nq - 1);
        const i32x4* src = reinterpret_cast<const i32x4*>(qc + (size_t)row * 128 + 64 * h);
#pragma unroll
        for (int kb = 0; kb < 4; kb++) bq[qb][kb] = src[kb];
        qn[qb] = (-qkeys[row]) >> 8;
    }
}

// Stage prepared train rows [row0, row0 + 32 nc) of a set (codes tc, key
// biases tk) into one LDS chunk by LDS-DMA; rows past nt read the zero
// sentinel row (zc, zk).  Codes: wave w fills 8-row blocks w, w + NW, ...
// (1 KiB each); lane l lands at slot (row 8b + l / 8, piece l & 7) and loads
// the global piece the swizzle puts there.  Keys: 64 rows per 4-byte-per-lane
// instruction.  Completion is this wave's vmcnt.
template <int NW>
__device__ __forceinline__ void stage_dma(const int8_t* __restrict__ tc, const int* __restrict__ tk, int nt, int row0,
                                          int nc, const int8_t* __restrict__ zc, const int* __restrict__ zk,
                                          int8_t* sc, int* sk, int w, int lane) {
    const int wv = __builtin_amdgcn_readfirstlane(w);
    for (int b = wv; b < nc * (kMatchTileRows / 8); b += NW) {
        const int r = 8 * b + (lane >> 3), gr = row0 + r;
        const int8_t* src = (gr < nt ? tc + (size_t)gr * 128 : zc) + 16 * piece_swz(r, lane & 7);
        __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)(sc + 1024 * b), 16,
                                         0, 0);
    }
    for (int b = wv; b < (nc * kMatchTileRows + 63) / 64; b += NW) {
        const int gr = row0 + 64 * b + lane;
        const int* src = gr < nt ? tk + gr : zk;
        __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)(sk + 64 * b), 4, 0,
                                         0);
    }
}

// The positions of train rows [row0, row0 + 32 nc) into the chunk's two float
// planes by 4-byte LDS-DMA, 64 rows per instruction as the keys.  Rows past nt
// read row nt - 1 (their padding key loses whatever the gate says): nothing
// past the caller's nt rows is touched.
template <int NW>
__device__ __forceinline__ void stage_pos_dma(const float* __restrict__ txy, int tstride, int nt, int row0, int nc,
                                              float* sx, float* sy, int w, int lane) {
    const int wv = __builtin_amdgcn_readfirstlane(w);
    for (int b = wv; b < (nc * kMatchTileRows + 63) / 64; b += NW) {
        const float* src = txy + (size_t)min(row0 + 64 * b + lane, nt - 1) * tstride;
        __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)(sx + 64 * b), 4, 0,
                                         0);
        __builtin_amdgcn_global_load_lds((const void*)(src + 1), (__attribute__((address_space(3))) void*)(sy + 64 * b),
                                         4, 0, 0);
    }
}

// A lane's side of the gate in the integer fold: the positions of its queries.
template <int QBW>
struct LaneGate {
    float qx[QBW], qy[QBW], radius;
};
template <int QBW>
__device__ __forceinline__ LaneGate<QBW> lane_gate(const MatchGate& g, int nq, int q0w, int col) {
    LaneGate<QBW> lg;
    lg.radius = g.radius;
#pragma unroll
    for (int qb = 0; qb < QBW; qb++) {
        const float* p = g.qxy + (size_t)min(q0w + 32 * qb + col, nq - 1) * g.qstride;
        lg.qx[qb] = p[0];
        lg.qy[qb] = p[1];
    }
    return lg;
}
template <int QBW>
__device__ __forceinline__ NoGate lane_gate(const NoGate&, int, int, int) {
    return {};
}

// A lane's side of the epipolar gate: the lines of its queries (and their
// positions, for the window); e2 and the radius are wave-uniform.  sn is the
// current chunk's third plane, the rows' nr beside their positions (match_pair
// fills it from the staged px / py once the chunk has landed).
template <int QBW>
struct LaneEpipolar {
    EpiQuery q[QBW];
    float radius, e2;
    const float* sn;
};
template <class Gate>
constexpr bool kLaneEpipolar = false;
template <int QBW>
constexpr bool kLaneEpipolar<LaneEpipolar<QBW>> = true;
template <int QBW>
__device__ __forceinline__ LaneEpipolar<QBW> lane_gate(const EpipolarGate& g, int nq, int q0w, int col) {
    LaneEpipolar<QBW> lg;
    lg.radius = g.radius;
    lg.e2 = g.e2;
    lg.sn = nullptr;
#pragma unroll
    for (int qb = 0; qb < QBW; qb++) {
        const float* p = g.qxy + (size_t)min(q0w + 32 * qb + col, nq - 1) * g.qstride;
        lg.q[qb] = epi_query(g.F, p[0], p[1]);
    }
    return lg;
}

// One staged chunk of nc tiles (rows t0 ...) against a wave's two query
// blocks: per tile 8 MFMAs from LDS fragments, then each lane folds its 32
// keys into a per-block running key top-2 -- two at a time: for a pair (x, y)
// of new keys and the running m1 >= m2 the new second is max(med3(m1, x, y),
// m2) and the new first max3(m1, x, y), 3 VALU per 2 keys, in two chains per
// block (accumulator registers 0-7 / 8-15).  The chunk lies in one key group
// (r = row - t0 < 256), so its top-2 is decoded once into (e, train index) and
// merged into the running pair (earlier groups win ties).
// Under a gate (Gate = LaneGate or LaneEpipolar, planes sx / sy) the key of a
// (query, row) that fails the gate becomes INT_MIN before the fold -- below
// kInvalidKey, so fold_group reads it as "none".  The positions are read as
// the keys are (the same address across the lanes of a half: broadcast reads).
template <int QBW, class Gate>
__device__ __forceinline__ void chunk_top2(const int8_t* sc, const int* sk, const float* sx, const float* sy, int nc,
                                           int t0, int col, int h, const i32x4 (&bq)[QBW][4], const Gate& g,
                                           Best (&best)[QBW]) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    int m1e[QBW], m2e[QBW], m1o[QBW], m2o[QBW];  // registers 0-7 / 8-15
#pragma unroll
    for (int qb = 0; qb < QBW; qb++) m1e[qb] = m2e[qb] = m1o[qb] = m2o[qb] = INT_MIN;
    const int sw = (col >> 1) & 7;
    const int8_t* const ta0 = sc + col * 128;
    const int* const tk1 = sk + 4 * h;
#pragma unroll
    for (int j = 0; j < kChunkTiles; j++) {
        if (j < nc) {
            i32x4 a[4], tk[4];
            f32x4 px[4], py[4];  // the window gate only
#pragma unroll
            for (int kb = 0; kb < 4; kb++)
                a[kb] = *reinterpret_cast<const i32x4*>(ta0 + j * kTileBytes + 16 * ((4 * h + kb) ^ sw));
            // accumulator register i holds train row (i & 3) + 8 (i >> 2) + 4 h
#pragma unroll
            for (int r = 0; r < 4; r++) {
                if constexpr (kLaneEpipolar<Gate>) continue;  // loads its planes in the fold, below
                tk[r] = *reinterpret_cast<const i32x4*>(tk1 + j * kMatchTileRows + 8 * r);
                if constexpr (kGated<Gate>) {
                    px[r] = *reinterpret_cast<const f32x4*>(sx + 4 * h + j * kMatchTileRows + 8 * r);
                    py[r] = *reinterpret_cast<const f32x4*>(sy + 4 * h + j * kMatchTileRows + 8 * r);
                }
            }
            i32x16 acc[QBW] = {};
#pragma unroll
            for (int qb = 0; qb < QBW; qb++)
#pragma unroll
                for (int kb = 0; kb < 4; kb++)
                    acc[qb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[kb], bq[qb][kb], acc[qb], 0, 0, 0);
#pragma unroll
            for (int qb = 0; qb < QBW; qb++) {
                if constexpr (kLaneEpipolar<Gate>) {
                    // The epipolar gate reads four planes (keys, px, py, nr): one
                    // row group at a time, loaded as the fold reaches it and not
                    // all four up front (the register budget of two workgroups per
                    // CU), its two pairs of adjacent rows into the two chains.  The
                    // top-2 of the chunk does not depend on which chain a key enters.
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int o = 4 * h + j * kMatchTileRows + 8 * r;
                        const i32x4 kr = *reinterpret_cast<const i32x4*>(sk + o);
                        const f32x4 xr = *reinterpret_cast<const f32x4*>(sx + o);
                        const f32x4 yr = *reinterpret_cast<const f32x4*>(sy + o);
                        const f32x4 nr = *reinterpret_cast<const f32x4*>(g.sn + o);
                        int x0 = (acc[qb][4 * r] << 9) + kr[0], y0 = (acc[qb][4 * r + 1] << 9) + kr[1];
                        int x1 = (acc[qb][4 * r + 2] << 9) + kr[2], y1 = (acc[qb][4 * r + 3] << 9) + kr[3];
                        bool p0, p1, p2, p3;
                        epi_pass2(g.q[qb], f32x2{xr[0], xr[1]}, f32x2{yr[0], yr[1]}, f32x2{nr[0], nr[1]}, g.e2, g.radius,
                                  p0, p1);
                        epi_pass2(g.q[qb], f32x2{xr[2], xr[3]}, f32x2{yr[2], yr[3]}, f32x2{nr[2], nr[3]}, g.e2, g.radius,
                                  p2, p3);
                        x0 = p0 ? x0 : INT_MIN, y0 = p1 ? y0 : INT_MIN, x1 = p2 ? x1 : INT_MIN, y1 = p3 ? y1 : INT_MIN;
                        m2e[qb] = max(med3_i32(m1e[qb], x0, y0), m2e[qb]);
                        m1e[qb] = max3_i32(m1e[qb], x0, y0);
                        m2o[qb] = max(med3_i32(m1o[qb], x1, y1), m2o[qb]);
                        m1o[qb] = max3_i32(m1o[qb], x1, y1);
                    }
                } else {
                    auto key = [&](int i) {
                        const int k = (acc[qb][i] << 9) + tk[i >> 2][i & 3];
                        if constexpr (kGated<Gate>)
                            return in_gate(px[i >> 2][i & 3], py[i >> 2][i & 3], g.qx[qb], g.qy[qb], g.radius) ? k : INT_MIN;
                        else
                            return k;
                    };
#pragma unroll
                    for (int i = 0; i < 8; i += 2) {
                        const int x0 = key(i), y0 = key(i + 1), x1 = key(i + 8), y1 = key(i + 9);
                        m2e[qb] = max(med3_i32(m1e[qb], x0, y0), m2e[qb]);
                        m1e[qb] = max3_i32(m1e[qb], x0, y0);
                        m2o[qb] = max(med3_i32(m1o[qb], x1, y1), m2o[qb]);
                        m1o[qb] = max3_i32(m1o[qb], x1, y1);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int qb = 0; qb < QBW; qb++) {
        const int a1 = m1e[qb], a2 = m2e[qb], b1 = m1o[qb], b2 = m2o[qb];
        best[qb] = fold_group(best[qb], max(a1, b1), max(min(a1, b1), max(a2, b2)), t0);
    }
}

// A lane's two halves of the train rows (lane, lane ^ 32) -> the query's
// (d^2, index) top-2 (d^2 = e + |c_q|^2).
__device__ __forceinline__ Top2 finish_best(const Best b, int qn) {
    Best o;
    o.e1 = __shfl_xor(b.e1, 32);
    o.i1 = __shfl_xor(b.i1, 32);
    o.e2 = __shfl_xor(b.e2, 32);
    o.i2 = __shfl_xor(b.i2, 32);
    const Best r = merge_best(b, o);
    Top2 t;
    t.d1 = r.e1 == kNone ? INFINITY : (float)(r.e1 + qn);
    t.i1 = r.e1 == kNone ? kNone : r.i1;
    t.d2 = r.e2 == kNone ? INFINITY : (float)(r.e2 + qn);
    t.i2 = r.e2 == kNone ? kNone : r.i2;
    return t;
}

__device__ __forceinline__ void write_top2(const Top2 r, size_t o, const MatchOut& out) {
    const int i1 = r.i1 == kNone ? -1 : r.i1, i2 = r.i2 == kNone ? -1 : r.i2;
    write_match(i1, i1 >= 0 ? r.d1 : FLT_MAX, i2, i2 >= 0 ? r.d2 : FLT_MAX, o, out);
}

// Global top-2 of a query over several contributions (train ranges):
// 64-bit atomicMin on keys (d^2 bits << 32 | train index).  A contribution
// min's its best into K1; whatever that displaced (or its best, if it lost)
// and its runner-up are candidates for K2, of which the smaller is min'ed in
// (the larger can never be second).  Every key except the final K1 reaches K2
// this way, so K2 ends as the true second.  Device-scope atomics only
// (coherent across XCDs, no cache write-back fences).  The contribution that
// completes the count (`units` of `total`, counted on *cnt) reads and
// restores the keys and the counter and writes the outputs.  Called by every
// thread of the workgroup, thread t for query q0 + t (s_res[t]).
__device__ __forceinline__ void merge_contribution(const Top2* s_res, unsigned* s_last, unsigned long long* K0,
                                                   unsigned* cnt, unsigned units, unsigned total, bool qv, size_t o,
                                                   const MatchOut& out) {
    const int tid = threadIdx.x;
    unsigned long long* K = K0 + 2 * tid;
    if (qv) {
        const Top2 r = s_res[tid];
        const unsigned long long a1 = match_key(r.d1, r.i1), a2 = match_key(r.d2, r.i2);
        if (a1 != ~0ull) {
            const unsigned long long o1 = atomicMin(&K[0], a1);
            const unsigned long long c = a1 < o1 ? o1 : a1;
            const unsigned long long o2 = atomicMin(&K[1], c < a2 ? c : a2);
            __asm__ volatile("" ::"v"(o2));  // returned: the min is performed before the count below
        }
    }
    __syncthreads();
    if (tid == 0) *s_last = atomicAdd(cnt, units) + units == total;
    __syncthreads();
    if (!*s_last) return;
    if (qv) {
        const unsigned long long k1 = atomicExch(&K[0], ~0ull), k2 = atomicExch(&K[1], ~0ull);
        const int i1 = k1 == ~0ull ? -1 : (int)(unsigned)k1, i2 = k2 == ~0ull ? -1 : (int)(unsigned)k2;
        const float e1 = i1 >= 0 ? __uint_as_float((unsigned)(k1 >> 32)) : FLT_MAX;
        const float e2 = i2 >= 0 ? __uint_as_float((unsigned)(k2 >> 32)) : FLT_MAX;
        write_match(i1, e1, i2, e2, o, out);
    }
    if (tid == 0) atomicExch(cnt, 0u);
}

// Splits of whole key groups: S splits of ntiles train tiles, split s owning
// tiles [begin(s), end(s)).  The one rule that keeps a kernel's tile range and
// the host's split count in agreement (tps rounded up can leave trailing
// splits empty: count() is the number that are not).
struct GroupSplit {
    int ntiles, tps;  // tiles per split
    __host__ __device__ GroupSplit(int ntiles, int S)
        : ntiles(ntiles), tps(((ntiles + S - 1) / S + kGroupTiles - 1) / kGroupTiles * kGroupTiles) {}
    __host__ __device__ int begin(int s) const { return min(ntiles, s * tps); }
    __host__ __device__ int end(int s) const { return min(ntiles, begin(s) + tps); }
    int count() const { return tps > 0 ? max(1, (ntiles + tps - 1) / tps) : 1; }
};
__host__ __device__ inline int match_tiles(int nt) { return (nt + kMatchTileRows - 1) / kMatchTileRows; }

// Queries per workgroup of NW waves with QBW 32-query blocks each.  Every match
// kernel ends the same way: each wave's h == 0 half parks the top-2 of its
// queries (over the workgroup's split) in s_res, which aliases the code tiles;
// thread t then owns query q0 + t and, with one split, writes its outputs,
// else merges them into the query block's keys (merge_contribution).  That
// ending and the LDS-DMA streaming loop before it are written out in
// k_match_single, k_match_batch and match_pair: as shared functions both
// compile to other instructions than the kernels measured in profiles/.
template <int NW, int QBW>
constexpr int block_queries() {
    constexpr int QB = 32 * QBW * NW;
    static_assert(QB <= 64 * NW, "the write-out gives each thread one query: at most 2 query blocks per wave");
    static_assert(sizeof(Top2) * QB <= kChunkTiles * kTileBytes, "results alias the code tiles");
    return QB;
}

}  // namespace sift_amd
