// Brute-force L2 matcher on MFMA for gfx950.
//
// Replaces /root/reference/sift_cuda/sift_func/Match.cu:8-177 (32 lanes per
// query, half2 diff^2, an N x M fp32 score matrix written to and re-read from
// HBM and allocated per call).  Here the distance matrix never leaves the
// register file.  Two launches per batched call, one for a single pair:
//
//  k_match_prep    every distinct descriptor set of the call (fp16 rows)
//                  becomes int8 codes c = v - 128 (128 B per row) and a key
//                  bias -(256 |c|^2 + (row mod 256)) per row, once per set (the
//                  8-way match: 8 sets for 56 pairs).  A set holding a value
//                  that is not an integer 0..255 is flagged.
//  k_match_batch   the distance GEMM on v_mfma_i32_32x32x32_i8 for prepared
//                  sets: a workgroup owns 512 queries (8 waves x 64; a wave
//                  keeps its two 32-query B operands in registers) and one
//                  split of the train tiles, which it streams through two LDS
//                  chunk buffers of 8 tiles by LDS-DMA (the next chunk lands
//                  while this one computes: one barrier per 8 tiles instead
//                  of one per tile); per 32-row tile 8 MFMAs per wave.
//  k_match_single  one pair without the prep launch: each workgroup (256
//                  queries) converts its own query rows and train tiles.
//  k_match_direct  one pair of ready code sets (detector sidecars): the
//                  integer path of k_match_batch with no prep and no flags.
//  k_match_guided  one pair of ready code sets under a search window: the
//                  direct kernel with the train positions staged beside the
//                  keys and a per-key gate in the top-2 fold.  Both are
//                  wrappers around one body, match_pair.
//  k_match_epipolar the same body under the gate of two-view geometry: a row is
//                  a candidate when its Sampson distance to the pair's
//                  fundamental matrix is within a bound (and it lies in the
//                  window); a third plane holds the rows' side of that test.
//  k_match_guided_batch / k_match_epipolar_batch  the two gated kernels with a
//                  pair dimension: P pairs of one code set per launch, the
//                  epipolar geometry read from device memory per pair.
//  k_match_select  match lists: the top-2 arrays of both directions filtered
//                  (ratio test, distance cap, cross check) and compacted in
//                  query order into cv::DMatch records, one workgroup per pair.
//  k_match_knn     k nearest neighbours (k <= 8) of every query of every pair:
//                  k_match_batch's streaming loop with a K-entry fold, and
//                  k_knn_select, the capped radius list of its table (the
//                  section at the end of this file).  The gate is a template
//                  parameter: k_match_knn<K, MatchGate / EpipolarGate> is the
//                  k-NN inside the window or the epipolar band, single or batched.
//
// Exactness: d^2 = sum (t - q)^2 = |c_t|^2 + |c_q|^2 - 2 c_t.c_q for the
// shifted codes (translation invariant), so the int32 accumulator and every
// key below are exact.  A lane folds the 16 train rows of its accumulator
// into a running top-2 of keys key = 512 dot - (256 |c_t|^2 + r) (one
// v_lshl_add_u32 each), where r is the row's index inside its group of 8
// tiles; keys order (e = d^2 - |c_q|^2, train row) in reverse, and two new
// keys at a time enter the top-2 with v_med3 + v_max3 (3 VALU per 2 keys).
// Each staged chunk is one key group: its top-2 is decoded into (e, train
// index) and merged into the running pair.  Ties keep the lower train index
// -- OpenCV's batchDistance / knnMatch order and the oracle's
// (sift_oracle_knn2).
//
// A pair with a flagged set (non-integer or out-of-range fp16 values, e.g. the
// reference's own unrounded x512 descriptors) runs the general path in the
// same launch: v_mfma_f32_32x32x16_f16 dot products (exact products, fp32
// sums), fp32 norms, a float top-2 in train order; d^2 is clamped at 0 and a
// query row holding NaN or an infinity has no neighbour (the contract: the
// general-path paragraph of include/sift_hip.h).
//
// Shared core: one integer fold (chunk_top2) and one fp16 block
// (match_f16_block), both templates on a gate policy (NoGate, the window of
// guided matching -- in_gate is its rule -- or the epipolar gate, epi_pass);
// one split rule for the kernels
// that split by whole key groups (GroupSplit, host and device); one merge
// (merge_contribution).  The bit-exactness rules -- the tie order, INT_MIN
// against kPadBias, rows past nt losing -- live there and nowhere else.
//
// Splits of the train rows merge through 64-bit atomicMin keys (d^2 bits << 32 |
// train index) in the matcher's scratch; the last split of a query block (a
// counter) writes the outputs and restores the scratch.  With one split the
// workgroup writes the outputs itself.
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
// Set preparation: 8 threads per row (16 halves each); per row the int8
// codes and the key bias -(256 |c|^2 + (row & 255)) (the norm is -bias >> 8).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_match_prep(MatchSets sets, int8_t* __restrict__ codes,
                                                    int* __restrict__ rowkeys, unsigned* __restrict__ flags,
                                                    unsigned epoch) {
    const MatchSet& st = sets.set[blockIdx.y];
    if ((int)blockIdx.x * 32 >= st.n) return;
    const int row = blockIdx.x * 32 + (threadIdx.x >> 3), part = threadIdx.x & 7;
    const bool in = row < st.n;
    const uint4* src = reinterpret_cast<const uint4*>(st.src + (size_t)min(row, st.n - 1) * 128 + part * 16);
    int nrm = 0;
    bool bad = false;
    const i32x4 pk = codes16(src[0], src[1], nrm, bad);  // codes of a flagged set are never used
    nrm += __shfl_xor(nrm, 1);
    nrm += __shfl_xor(nrm, 2);
    nrm += __shfl_xor(nrm, 4);
    if (in) {
        *reinterpret_cast<i32x4*>(codes + ((size_t)st.row0 + row) * 128 + part * 16) = pk;
        if (part == 0) rowkeys[st.row0 + row] = -(256 * nrm + (row & 255));  // the row's key bias (r = row mod 256)
        if (bad) flags[blockIdx.y] = epoch;  // every writer stores the same word
    }
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

// ---------------------------------------------------------------------------
// k_match_single: one pair, fp16 rows converted in the kernel (no prep
// launch).  grid = (query blocks of 64 NW, train splits S), 64 NW threads; a
// workgroup converts its query rows and its split's train rows as it stages
// them (8 threads per row: two 16-byte fp16 loads -> one swizzled 16-byte code
// piece; the row norm by three shuffles) and takes the fp16 path itself if
// any of them holds a non-integer value.  Mixing paths across workgroups is
// exact: on integer values 0..255 the fp16 path's dot products and norms are
// exact integers below 2^24, so both paths return the same (d^2, index) pairs
// with the same tie order.  The splits are plain ceil(ntiles / S) tile ranges,
// not GroupSplit's whole key groups: the workgroup computes the key biases
// itself, so its key groups start at the split's first tile, wherever that is,
// and the split may be as small as the conversion cost allows (match_plan).
// ---------------------------------------------------------------------------
template <int NW, int QBW>
__global__ __launch_bounds__(64 * NW, (kMatchWgPerCu * NW) / 4) void k_match_single(
    MatchPair pr, int S, unsigned long long* __restrict__ keys, unsigned* __restrict__ done, float ratio,
    int ratio_on_squared, int* __restrict__ idx2, float* __restrict__ d2out, int* __restrict__ match) {
    constexpr int NT = 64 * NW, QB = block_queries<NW, QBW>();  // threads, queries per workgroup
    __shared__ __attribute__((aligned(16))) int8_t s_codes[2][kChunkTiles * kTileBytes];
    __shared__ __attribute__((aligned(16))) int s_key[2][kChunkRows];
    __shared__ unsigned s_last;
    const int q0 = blockIdx.x * QB;
    if (q0 >= pr.nq) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 31, h = lane >> 5;
    const int ntiles = match_tiles(pr.nt), tps = (ntiles + S - 1) / S;
    const int tbeg = min(ntiles, (int)blockIdx.y * tps), tend = min(ntiles, tbeg + tps);
    const int q0w = q0 + 32 * QBW * w;
    Top2 res[QBW];
    bool bad = false;  // a non-integer value among this workgroup's rows
    {
        i32x4 bq[QBW][4];
        int qn[QBW];
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) {
            const int row = min(q0w + 32 * qb + col, pr.nq - 1);
            const uint4* src = reinterpret_cast<const uint4*>(pr.q + (size_t)row * 128 + 64 * h);
            int nrm = 0;
#pragma unroll
            for (int kb = 0; kb < 4; kb++) bq[qb][kb] = codes16(src[2 * kb], src[2 * kb + 1], nrm, bad);
            qn[qb] = nrm + __shfl_xor(nrm, 32);
        }
        auto stage = [&](int c0, int buf) {
            const int nc = min(kChunkTiles, tend - c0);
            int8_t* const sc = s_codes[buf];
            int* const sk = s_key[buf];
            constexpr int U = 2;  // loads go out U pieces at a time
            const int npieces = nc * kMatchTileRows * 8;
            for (int base = 0; base < npieces; base += NT * U) {
                uint4 hv[U][2];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int idx = min(base + tid + NT * u, npieces - 1), r = idx >> 3;
                    const uint4* src = reinterpret_cast<const uint4*>(
                        pr.t + (size_t)min(c0 * kMatchTileRows + r, pr.nt - 1) * 128 + 16 * (idx & 7));
                    hv[u][0] = src[0];
                    hv[u][1] = src[1];
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int idx = base + tid + NT * u, r = idx >> 3, part = idx & 7;
                    const int gr = c0 * kMatchTileRows + r;
                    int nrm = 0;
                    const i32x4 pk = codes16(hv[u][0], hv[u][1], nrm, bad);
                    nrm += __shfl_xor(nrm, 1);
                    nrm += __shfl_xor(nrm, 2);
                    nrm += __shfl_xor(nrm, 4);
                    if (idx < npieces) {  // whole rows of 8 lanes: the shuffles above stay inside a row
                        *reinterpret_cast<i32x4*>(sc + r * 128 + 16 * piece_swz(r, part)) =
                            gr < pr.nt ? pk : (i32x4){0, 0, 0, 0};
                        if (part == 0)
                            sk[r] = gr < pr.nt ? -(256 * nrm + ((gr - tbeg * kMatchTileRows) & 255)) : kPadBias;
                    }
                }
            }
        };
        Best best[QBW];
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) best[qb] = Best{kNone, kNone, kNone, kNone};
        if (tbeg < tend) stage(tbeg, 0);
        int buf = 0;
        for (int c0 = tbeg; c0 < tend; c0 += kChunkTiles, buf ^= 1) {
            __syncthreads();  // chunk c0 is staged; every wave is done with the other buffer
            if (c0 + kChunkTiles < tend) stage(c0 + kChunkTiles, buf ^ 1);
            chunk_top2(s_codes[buf], s_key[buf], nullptr, nullptr, min(kChunkTiles, tend - c0), c0 * kMatchTileRows, col,
                       h, bq, NoGate{}, best);
        }
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) res[qb] = finish_best(best[qb], qn[qb]);
    }
    if (__syncthreads_or(bad)) {
        // ---- general path: fp16 values that are not integers 0..255 ----
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) res[qb] = match_f16_block(pr, NoGate{}, q0w + 32 * qb, tbeg, tend, col, h);
    }
    Top2* const s_res = reinterpret_cast<Top2*>(&s_codes[0][0]);
    const MatchOut out{ratio, ratio_on_squared, idx2, d2out, match};
    __syncthreads();  // s_res aliases the code tiles
    if (h == 0) {
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) s_res[32 * QBW * w + 32 * qb + col] = res[qb];
    }
    __syncthreads();
    const int q = q0 + tid;
    const bool qv = tid < QB && q < pr.nq;
    const size_t o = (size_t)pr.out_off + q;
    if (S == 1) {
        if (qv) write_top2(s_res[tid], o, out);
        return;
    }
    merge_contribution(s_res, &s_last, keys + 2 * (size_t)q0, done + blockIdx.x, 1u, (unsigned)S, qv, o, out);
}

// ---------------------------------------------------------------------------
// k_match_batch: prepared sets (k_match_prep), any number of pairs.
// grid = (query blocks of 64 NW, train splits S, pairs), 64 NW threads.  A
// split is whole key groups of the pair's train tiles; the workgroup loads
// each wave's query operands once and streams its split through two LDS chunk
// buffers (the next group by LDS-DMA while this one computes: one barrier per
// 8 tiles).  With S > 1 the splits merge through the keys scratch and the one
// that completes the query block's count writes the outputs.
// ---------------------------------------------------------------------------
template <int NW, int QBW>
__global__ __launch_bounds__(64 * NW, (kMatchBatchWgPerCu * NW) / 4) void k_match_batch(
    MatchBatch batch, int S, int nq_stride, const int8_t* __restrict__ codes, const int* __restrict__ rowkeys,
    const int8_t* __restrict__ zc, const int* __restrict__ zk, const unsigned* __restrict__ flags, unsigned epoch,
    unsigned long long* __restrict__ keys,
    unsigned* __restrict__ done, float ratio, int ratio_on_squared, int* __restrict__ idx2, float* __restrict__ d2out,
    int* __restrict__ match) {
    constexpr int QB = block_queries<NW, QBW>();
    __shared__ __attribute__((aligned(16))) int8_t s_codes[2][kChunkTiles * kTileBytes];
    __shared__ __attribute__((aligned(16))) int s_key[2][kChunkRows];
    __shared__ unsigned s_last;
    const int p = blockIdx.z;
    const MatchPair& pr = batch.pair[p];
    const int q0 = blockIdx.x * QB;
    if (q0 >= pr.nq) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 31, h = lane >> 5;
    const GroupSplit split(match_tiles(pr.nt), S);
    const int tb = split.begin(blockIdx.y), te = split.end(blockIdx.y);
    const int q0w = q0 + 32 * QBW * w;
    Top2 res[QBW];
    // flags == nullptr: code sets handed over ready (sift_hip_match_codes_batched), integers by construction.
    if (!flags || (flags[pr.qset] != epoch && flags[pr.tset] != epoch)) {
        // ---- integer path (zc / zk: the zero code row and padding key) ----
        const int8_t* __restrict__ tc = codes + (size_t)pr.trow0 * 128;
        const int* __restrict__ tk = rowkeys + pr.tkrow0;
        auto stage = [&](int c0, int buf) {
            stage_dma<NW>(tc, tk, pr.nt, c0 * kMatchTileRows, min(kChunkTiles, te - c0), zc, zk, s_codes[buf], s_key[buf],
                          w, lane);
        };
        i32x4 bq[QBW][4];
        int qn[QBW];
        load_queries<QBW>(codes + (size_t)pr.qrow0 * 128, rowkeys + pr.qkrow0, pr.nq, q0w, col, h, bq, qn);
        Best best[QBW];
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) best[qb] = Best{kNone, kNone, kNone, kNone};
        if (tb < te) stage(tb, 0);
        int buf = 0;
        for (int c0 = tb; c0 < te; c0 += kChunkTiles, buf ^= 1) {
            // LDS-DMA writes are counted by vmcnt: this wave's copies of the
            // chunk have landed; the barrier publishes every wave's, and every
            // wave is done with the other buffer.
            __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (c0 + kChunkTiles < te) stage(c0 + kChunkTiles, buf ^ 1);
            chunk_top2(s_codes[buf], s_key[buf], nullptr, nullptr, min(kChunkTiles, te - c0), c0 * kMatchTileRows, col, h,
                       bq, NoGate{}, best);
        }
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) res[qb] = finish_best(best[qb], qn[qb]);
    } else {
        // ---- general path: fp16 values that are not integers 0..255 ----
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) res[qb] = match_f16_block(pr, NoGate{}, q0w + 32 * qb, tb, te, col, h);
    }
    const MatchOut out{ratio, ratio_on_squared, idx2, d2out, match};
    Top2* const s_res = reinterpret_cast<Top2*>(&s_codes[0][0]);
    __syncthreads();  // s_res aliases the code tiles
    if (h == 0) {
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) s_res[32 * QBW * w + 32 * qb + col] = res[qb];
    }
    __syncthreads();
    const int q = q0 + tid;
    const bool qv = tid < QB && q < pr.nq;
    const size_t o = (size_t)pr.out_off + q;
    if (S == 1) {
        if (qv) write_top2(s_res[tid], o, out);
        return;
    }
    merge_contribution(s_res, &s_last, keys + 2 * ((size_t)p * nq_stride + q0), done + (size_t)p * gridDim.x + blockIdx.x,
                       1u, (unsigned)S, qv, o, out);
}

// ---------------------------------------------------------------------------
// match_pair: the body of the three kernels on one pair of ready code sets,
// k_match_direct (Gate = NoGate), k_match_guided (Gate = MatchGate) and
// k_match_epipolar (Gate = EpipolarGate; s_pn: its third plane).  The
// integer path of k_match_batch with the codes and keys addressed directly:
// query operands from the query set, the split's train key groups streamed
// through the two LDS chunks by LDS-DMA -- under a gate with the train
// positions beside the keys and the queries' positions in registers.  A
// flagged set (flags != nullptr: the matcher's prepared sets) sends the pair
// down the fp16 path; with flags == nullptr that branch folds away.
// ---------------------------------------------------------------------------
template <int NW, int QBW, class Gate>
__device__ __forceinline__ void match_pair(int8_t (&s_codes)[2][kChunkTiles * kTileBytes], int (&s_key)[2][kChunkRows],
                                           float (*s_px)[kChunkRows], float (*s_py)[kChunkRows],
                                           float (*s_pn)[kChunkRows], unsigned* s_last,
                                           const MatchPair& pr, const Gate& g, const CodeSet& qs, const CodeSet& ts,
                                           const CodeSet& zero, const unsigned* flags, unsigned epoch, int S,
                                           unsigned long long* keys, unsigned* done, const MatchOut& out) {
    constexpr int QB = block_queries<NW, QBW>();
    const int q0 = blockIdx.x * QB;
    if (q0 >= pr.nq) return;
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, h = lane >> 5;
    // The wave's index: under the epipolar gate as a scalar, the one VGPR that
    // keeps k_match_epipolar inside 128 registers without scratch.
    const int w = kEpipolar<Gate> ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    const GroupSplit split(match_tiles(pr.nt), S);
    const int tb = split.begin(blockIdx.y), te = split.end(blockIdx.y);
    const int q0w = q0 + 32 * QBW * w;
    Top2 res[QBW];
    if (!flags || (flags[pr.qset] != epoch && flags[pr.tset] != epoch)) {
        // ---- integer path ----
        auto stage = [&](int c0, int buf) {
            const int nc = min(kChunkTiles, te - c0);
            stage_dma<NW>(ts.codes, ts.keys, pr.nt, c0 * kMatchTileRows, nc, zero.codes, zero.keys, s_codes[buf],
                          s_key[buf], w, lane);
            if constexpr (kGated<Gate>)
                stage_pos_dma<NW>(g.txy, g.tstride, pr.nt, c0 * kMatchTileRows, nc, s_px[buf], s_py[buf], w, lane);
        };
        if (tb < te) stage(tb, 0);  // the first chunk's DMA before the query loads: both round trips overlap
        i32x4 bq[QBW][4];
        int qn[QBW];
        load_queries<QBW>(qs.codes, qs.keys, pr.nq, q0w, col, h, bq, qn);
        auto lg = lane_gate<QBW>(g, pr.nq, q0w, col);
        Best best[QBW];
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) best[qb] = Best{kNone, kNone, kNone, kNone};
        int buf = 0;
        for (int c0 = tb; c0 < te; c0 += kChunkTiles, buf ^= 1) {
            __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // as in k_match_batch
            __syncthreads();
            if (c0 + kChunkTiles < te) stage(c0 + kChunkTiles, buf ^ 1);
            const float *sx = nullptr, *sy = nullptr;
            if constexpr (kGated<Gate>) sx = s_px[buf], sy = s_py[buf];
            if constexpr (kEpipolar<Gate>) {
                // The third plane: row r's nr from its landed position, once per
                // chunk instead of once per lane that folds the row.
                for (int r = tid; r < kChunkRows; r += 64 * NW) s_pn[buf][r] = epi_row(g.F, sx[r], sy[r]);
                lg.sn = s_pn[buf];
                __syncthreads();
            }
            chunk_top2(s_codes[buf], s_key[buf], sx, sy, min(kChunkTiles, te - c0), c0 * kMatchTileRows, col, h, bq, lg,
                       best);
        }
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) res[qb] = finish_best(best[qb], qn[qb]);
    } else {
        // ---- general path: fp16 values that are not integers 0..255 ----
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) res[qb] = match_f16_block(pr, g, q0w + 32 * qb, tb, te, col, h);
    }
    Top2* const s_res = reinterpret_cast<Top2*>(&s_codes[0][0]);
    __syncthreads();  // s_res aliases the code tiles
    if (h == 0) {
#pragma unroll
        for (int qb = 0; qb < QBW; qb++) s_res[32 * QBW * w + 32 * qb + col] = res[qb];
    }
    __syncthreads();
    const int q = q0 + tid;
    const bool qv = tid < QB && q < pr.nq;
    const size_t o = (size_t)pr.out_off + q;
    if (S == 1) {
        if (qv) write_top2(s_res[tid], o, out);
        return;
    }
    merge_contribution(s_res, s_last, keys + 2 * (size_t)q0, done + blockIdx.x, 1u, (unsigned)S, qv, o, out);
}

// k_match_direct: one pair of detector-produced descriptor sets, read through
// their sidecars (int8 codes + key bias, written by the descriptor kernels:
// no conversion, no prep launch).  No gate, no flags, no position planes.
// grid = (query blocks of 32 QBW NW, splits S of whole key groups).
template <int NW, int QBW>
__global__ __launch_bounds__(64 * NW) void k_match_direct(
    MatchPair pr, const int8_t* __restrict__ qc, const int* __restrict__ qk, const int8_t* __restrict__ tc,
    const int* __restrict__ tk, const int8_t* __restrict__ zc, const int* __restrict__ zk, int S,
    unsigned long long* __restrict__ keys, unsigned* __restrict__ done, float ratio, int ratio_on_squared,
    int* __restrict__ idx2, float* __restrict__ d2out, int* __restrict__ match) {
    __shared__ __attribute__((aligned(16))) int8_t s_codes[2][kChunkTiles * kTileBytes];
    __shared__ __attribute__((aligned(16))) int s_key[2][kChunkRows];
    __shared__ unsigned s_last;
    match_pair<NW, QBW>(s_codes, s_key, nullptr, nullptr, nullptr, &s_last, pr, NoGate{}, CodeSet{qc, qk},
                        CodeSet{tc, tk}, CodeSet{zc, zk}, nullptr, 0u, S, keys, done,
                        MatchOut{ratio, ratio_on_squared, idx2, d2out, match});
}

// k_match_guided: one pair of ready code sets (sidecars, or the matcher's
// prepared codes) under a gate.  match_pair with the train positions of each
// chunk staged beside its keys (two float planes of kChunkRows per buffer:
// 70 KiB of LDS per workgroup, still two per CU) and the gated cores; a pair
// with a flagged set takes the gated fp16 path.
// grid = (query blocks of 32 QBW NW, splits S of whole key groups).
template <int NW, int QBW>
__global__ __launch_bounds__(64 * NW, (2 * NW) / 4) void k_match_guided(  // registers for two workgroups per CU
    MatchPair pr, MatchGate g, const int8_t* __restrict__ qc, const int* __restrict__ qk,
    const int8_t* __restrict__ tc, const int* __restrict__ tk, const int8_t* __restrict__ zc,
    const int* __restrict__ zk, const unsigned* __restrict__ flags, unsigned epoch, int S,
    unsigned long long* __restrict__ keys, unsigned* __restrict__ done, float ratio, int ratio_on_squared,
    int* __restrict__ idx2, float* __restrict__ d2out, int* __restrict__ match) {
    __shared__ __attribute__((aligned(16))) int8_t s_codes[2][kChunkTiles * kTileBytes];
    __shared__ __attribute__((aligned(16))) int s_key[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_px[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_py[2][kChunkRows];
    __shared__ unsigned s_last;
    match_pair<NW, QBW>(s_codes, s_key, s_px, s_py, nullptr, &s_last, pr, g, CodeSet{qc, qk}, CodeSet{tc, tk},
                        CodeSet{zc, zk}, flags, epoch, S, keys, done,
                        MatchOut{ratio, ratio_on_squared, idx2, d2out, match});
}

// k_match_epipolar: k_match_guided with the epipolar gate -- the same staging,
// LDS and launch shape; the gate's extra work is VALU per key.
template <int NW, int QBW>
__global__ __launch_bounds__(64 * NW, (2 * NW) / 4) void k_match_epipolar(  // registers for two workgroups per CU
    MatchPair pr, EpipolarGate g, const int8_t* __restrict__ qc, const int* __restrict__ qk,
    const int8_t* __restrict__ tc, const int* __restrict__ tk, const int8_t* __restrict__ zc,
    const int* __restrict__ zk, const unsigned* __restrict__ flags, unsigned epoch, int S,
    unsigned long long* __restrict__ keys, unsigned* __restrict__ done, float ratio, int ratio_on_squared,
    int* __restrict__ idx2, float* __restrict__ d2out, int* __restrict__ match) {
    __shared__ __attribute__((aligned(16))) int8_t s_codes[2][kChunkTiles * kTileBytes];
    __shared__ __attribute__((aligned(16))) int s_key[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_px[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_py[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_pn[2][kChunkRows];
    __shared__ unsigned s_last;
    match_pair<NW, QBW>(s_codes, s_key, s_px, s_py, s_pn, &s_last, pr, g, CodeSet{qc, qk}, CodeSet{tc, tk},
                        CodeSet{zc, zk}, flags, epoch, S, keys, done,
                        MatchOut{ratio, ratio_on_squared, idx2, d2out, match});
}

// k_match_guided_batch / k_match_epipolar_batch: the two gated kernels with a
// pair dimension.  grid = (query blocks of 32 QBW NW, splits S of whole key
// groups, pairs); pair p = blockIdx.z runs match_pair on its rows of the
// launch's code set, with its own slice of the scratch keys (p * nq_stride) and
// of the done counters, as k_match_batch does.  The pair's record (kernarg) and
// everything derived from it are wave-uniform: the strides of a reverse pair
// are the launch's swapped.  LDS and registers are the single-pair kernels'.
template <int NW, int QBW>
__global__ __launch_bounds__(64 * NW, (2 * NW) / 4) void k_match_guided_batch(  // registers for two workgroups per CU
    GatedBatch batch, int qstride, int tstride, float radius, int S, int nq_stride, const int8_t* __restrict__ codes,
    const int* __restrict__ rowkeys, const int8_t* __restrict__ zc, const int* __restrict__ zk,
    const unsigned* __restrict__ flags, unsigned epoch, unsigned long long* __restrict__ keys,
    unsigned* __restrict__ done, float ratio, int ratio_on_squared, int* __restrict__ idx2, float* __restrict__ d2out,
    int* __restrict__ match) {
    __shared__ __attribute__((aligned(16))) int8_t s_codes[2][kChunkTiles * kTileBytes];
    __shared__ __attribute__((aligned(16))) int s_key[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_px[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_py[2][kChunkRows];
    __shared__ unsigned s_last;
    const int p = blockIdx.z;
    const GatedPair& gp = batch.pair[p];
    const MatchGate g{gp.qxy, gp.txy, gp.swapped ? tstride : qstride, gp.swapped ? qstride : tstride, radius};
    match_pair<NW, QBW>(s_codes, s_key, s_px, s_py, nullptr, &s_last, gp.pr, g,
                        CodeSet{codes + (size_t)gp.pr.qrow0 * 128, rowkeys + gp.pr.qkrow0},
                        CodeSet{codes + (size_t)gp.pr.trow0 * 128, rowkeys + gp.pr.tkrow0}, CodeSet{zc, zk}, flags, epoch,
                        S, keys + 2 * (size_t)p * nq_stride, done + (size_t)p * gridDim.x,
                        MatchOut{ratio, ratio_on_squared, idx2, d2out, match});
}

// The epipolar twin reads pair p's nine floats from device memory (geometry +
// geom * geometry_stride bytes: one wave-uniform load per workgroup, kept in
// scalar registers), transposed for a reverse pair.  A record that holds a
// value that is not finite, or nine zeros (the empty verify result), has no
// candidates: its e2 becomes NaN, which fails every compare of the gate (the
// device-side rule of include/sift_hip.h; a zero F would otherwise pass every
// row, 0 <= e2 * 0).
template <int NW, int QBW>
__global__ __launch_bounds__(64 * NW, (2 * NW) / 4) void k_match_epipolar_batch(  // registers for two workgroups per CU
    GatedBatch batch, int qstride, int tstride, float radius, float e2, const char* __restrict__ geometry,
    int geometry_stride, int S, int nq_stride, const int8_t* __restrict__ codes, const int* __restrict__ rowkeys,
    const int8_t* __restrict__ zc, const int* __restrict__ zk, const unsigned* __restrict__ flags, unsigned epoch,
    unsigned long long* __restrict__ keys, unsigned* __restrict__ done, float ratio, int ratio_on_squared,
    int* __restrict__ idx2, float* __restrict__ d2out, int* __restrict__ match) {
    __shared__ __attribute__((aligned(16))) int8_t s_codes[2][kChunkTiles * kTileBytes];
    __shared__ __attribute__((aligned(16))) int s_key[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_px[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_py[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_pn[2][kChunkRows];
    __shared__ unsigned s_last;
    const int p = blockIdx.z;
    const GatedPair& gp = batch.pair[p];
    const unsigned* const G = reinterpret_cast<const unsigned*>(geometry + (size_t)gp.geom * geometry_stride);
    float f[9];
    bool usable = true, zero = true;
#pragma unroll
    for (int e = 0; e < 9; e++) {
        f[e] = __uint_as_float(__builtin_amdgcn_readfirstlane(G[e]));
        usable = usable && __builtin_fabsf(f[e]) < INFINITY;
        zero = zero && f[e] == 0.f;
    }
    usable = usable && !zero;
    EpipolarGate g{gp.qxy, gp.txy, gp.swapped ? tstride : qstride, gp.swapped ? qstride : tstride, radius,
                   usable ? e2 : NAN, {}};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) g.F[3 * r + c] = gp.swapped ? f[3 * c + r] : f[3 * r + c];
    match_pair<NW, QBW>(s_codes, s_key, s_px, s_py, s_pn, &s_last, gp.pr, g,
                        CodeSet{codes + (size_t)gp.pr.qrow0 * 128, rowkeys + gp.pr.qkrow0},
                        CodeSet{codes + (size_t)gp.pr.trow0 * 128, rowkeys + gp.pr.tkrow0}, CodeSet{zc, zk}, flags, epoch,
                        S, keys + 2 * (size_t)p * nq_stride, done + (size_t)p * gridDim.x,
                        MatchOut{ratio, ratio_on_squared, idx2, d2out, match});
}

// Direct single pairs: 8 waves x 1 query block (256 queries per workgroup),
// one key group (256 train rows) per split up to kDirectWgTarget workgroups.
// 2000 x 2000 on detector buffers (tools/match_direct_time.py, two passes):
// 7.71 / 7.78 us; 4 waves 8.06 / 7.90; 4 waves x 2 blocks 8.97 / 8.98; two key
// groups per split (target 64) 9.65 / 9.72; the converting k_match_single
// on the same pair 11.2-11.4 (profiles/round5/match_direct_ab.jsonl).
constexpr int kDirectNW = 8, kDirectQBW = 1, kDirectQB = 32 * kDirectNW * kDirectQBW, kDirectWgTarget = 256;

int match_direct_splits(int nq, int nt) {
    const int ntiles = match_tiles(nt), groups = (ntiles + kGroupTiles - 1) / kGroupTiles;
    const int qblocks = (max(nq, 1) + kDirectQB - 1) / kDirectQB;
    return GroupSplit(ntiles, max(1, min(groups, kDirectWgTarget / max(qblocks, 1)))).count();
}

// The gated kernel takes the direct kernel's shape: the gate adds VALU work
// per key, not traffic, so the split that balances the one balances the other.
void launch_match_pair(const MatchPair& pr, const MatchGate* gate, const CodeSet& q, const CodeSet& t,
                       const SetFlags& flags, const MatchScratch& sc, const MatchOut& out, hipStream_t s) {
    const int S = match_direct_splits(pr.nq, pr.nt);
    const dim3 g((max(pr.nq, 1) + kDirectQB - 1) / kDirectQB, S, 1), b(64 * kDirectNW);
    if (gate)
        hipLaunchKernelGGL((k_match_guided<kDirectNW, kDirectQBW>), g, b, 0, s, pr, *gate, q.codes, q.keys, t.codes,
                           t.keys, sc.zero.codes, sc.zero.keys, flags.flags, flags.epoch, S, sc.keys, sc.done, out.ratio,
                           out.ratio_on_squared, out.idx2, out.d2, out.match);
    else
        hipLaunchKernelGGL((k_match_direct<kDirectNW, kDirectQBW>), g, b, 0, s, pr, q.codes, q.keys, t.codes, t.keys,
                           sc.zero.codes, sc.zero.keys, S, sc.keys, sc.done, out.ratio, out.ratio_on_squared, out.idx2,
                           out.d2, out.match);
}

void launch_match_pair(const MatchPair& pr, const EpipolarGate& gate, const CodeSet& q, const CodeSet& t,
                       const SetFlags& flags, const MatchScratch& sc, const MatchOut& out, hipStream_t s) {
    const int S = match_direct_splits(pr.nq, pr.nt);
    const dim3 g((max(pr.nq, 1) + kDirectQB - 1) / kDirectQB, S, 1), b(64 * kDirectNW);
    hipLaunchKernelGGL((k_match_epipolar<kDirectNW, kDirectQBW>), g, b, 0, s, pr, gate, q.codes, q.keys, t.codes, t.keys,
                       sc.zero.codes, sc.zero.keys, flags.flags, flags.epoch, S, sc.keys, sc.done, out.ratio,
                       out.ratio_on_squared, out.idx2, out.d2, out.match);
}

// Gated batches take the direct shape per pair (8 waves x 1 query block: the
// epipolar body has no registers for a second block) and split each pair's
// train rows into whole key groups until the launch fills two workgroups per CU
// of a 256-CU device once.  One pair gets the single-pair kernels' split.
constexpr int kGatedBatchWgTarget = 512;

int match_gated_splits(int max_nq, int max_nt, int P) {
    const int ntiles = match_tiles(max_nt), groups = (ntiles + kGroupTiles - 1) / kGroupTiles;
    const int units = (max(max_nq, 1) + kDirectQB - 1) / kDirectQB * max(P, 1);
    return GroupSplit(ntiles, max(1, min(groups, kGatedBatchWgTarget / units))).count();
}

void launch_match_gated(const GatedBatch& batch, const GatedCall& call, const CodeSet& set, const SetFlags& flags,
                        const MatchScratch& sc, const MatchOut& out, hipStream_t s) {
    int max_nq = 1, max_nt = 1;
    for (int p = 0; p < batch.P; p++) {
        max_nq = max(max_nq, batch.pair[p].pr.nq);
        max_nt = max(max_nt, batch.pair[p].pr.nt);
    }
    const int S = match_gated_splits(max_nq, max_nt, batch.P);
    const dim3 g((max_nq + kDirectQB - 1) / kDirectQB, S, batch.P), b(64 * kDirectNW);
    if (call.geometry)
        hipLaunchKernelGGL((k_match_epipolar_batch<kDirectNW, kDirectQBW>), g, b, 0, s, batch, call.qstride, call.tstride,
                           call.radius, call.e2, reinterpret_cast<const char*>(call.geometry), call.geometry_stride, S,
                           sc.nq_stride, set.codes, set.keys, sc.zero.codes, sc.zero.keys, flags.flags, flags.epoch,
                           sc.keys, sc.done, out.ratio, out.ratio_on_squared, out.idx2, out.d2, out.match);
    else
        hipLaunchKernelGGL((k_match_guided_batch<kDirectNW, kDirectQBW>), g, b, 0, s, batch, call.qstride, call.tstride,
                           call.radius, S, sc.nq_stride, set.codes, set.keys, sc.zero.codes, sc.zero.keys, flags.flags,
                           flags.epoch, sc.keys, sc.done, out.ratio, out.ratio_on_squared, out.idx2, out.d2, out.match);
}

void launch_match_prep(const MatchSets& sets, int8_t* codes, int* rowkeys, const SetFlags& flags, hipStream_t s) {
    if (sets.maxn > 0)
        hipLaunchKernelGGL(k_match_prep, dim3((sets.maxn + 31) / 32, sets.nsets), dim3(256), 0, s, sets, codes, rowkeys,
                           flags.flags, flags.epoch);
}

// Single pairs of foreign buffers (k_match_single): workgroups a launch aims
// for when choosing train splits (64-1024 measured equal, round 2), waves per
// workgroup and 32-query blocks per wave (4 x 2: 256 queries per workgroup;
// 128-query workgroups measured equal, round 4), and no prep launch (the
// prep + batch kernel path: host-synchronous calls 32-42 vs 25-28 us, round 2).
constexpr int kMatchWgTargetSingle = 256;
constexpr int kMatchNWSingle = 4;
constexpr int kMatchQBWSingle = 2;
constexpr int kMatchSingleQB = 32 * kMatchQBWSingle * kMatchNWSingle;
// The matcher's done counters are sized per (pair, kMatchQB-query block)
// (sift_hip_matcher_create); a launch indexes them by its own block, which must
// therefore hold at least kMatchQB queries.
static_assert(kMatchSingleQB >= kMatchQB, "single-pair blocks smaller than the done-counter block");
static_assert(kMatchBatchQB >= kMatchQB, "batched blocks smaller than the done-counter block");
static_assert(kDirectQB >= kMatchQB, "direct blocks smaller than the done-counter block");

static int device_cus() {
    static int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        return n;
    }();
    return cus;
}

MatchPlan match_plan(int max_nq, int max_nt, int P) {
    MatchPlan pl;
    const int ntiles = match_tiles(max_nt);
    if (P == 1) {
        pl.nw = kMatchNWSingle;
        const int qblocks = (max_nq + kMatchSingleQB - 1) / kMatchSingleQB;
        int S = (kMatchWgTargetSingle + qblocks - 1) / qblocks;
        // >= 4 tiles per split: every split converts its workgroup's query rows
        // again (C3, 2000 x 2000: 4 tiles 11.5 us per call, 3 tiles 11.9, 2 12.4,
        // 1 15.8, 6 12.3, 8 13.4; tools/r3_c3_dma.sh).
        constexpr int kMinTilesSingle = 4;
        const int maxS = (ntiles + kMinTilesSingle - 1) / kMinTilesSingle;
        S = S < maxS ? S : maxS;
        S = S < 1 ? 1 : S;
        // No empty splits (tps rounded up can leave trailing ones empty).
        const int tps = (ntiles + S - 1) / S;
        pl.S = tps > 0 ? (ntiles + tps - 1) / tps : 1;
    } else {
        // Splits (whole key groups each) that minimise the busiest CU's work
        // within one round of workgroups: a CU's tile rate is the same with
        // one workgroup (2 waves per SIMD) or two (4), so the time is
        // (workgroups on the busiest CU) x (tiles per split), plus the split
        // merge (~2.8 us, kMergeTiles tile-times) when S > 1.  C5 (224 query
        // blocks on 256 CUs): S = 1, 64 tiles and no merge, instead of S = 2
        // (two workgroups of 32 tiles on 192 CUs, then the merge).
        pl.nw = kMatchBatchNW;
        const int qblocks = (max_nq + kMatchBatchQB - 1) / kMatchBatchQB;
        const int groups = (ntiles + kGroupTiles - 1) / kGroupTiles;
        const int cus = device_cus(), units = qblocks * P;
        constexpr int kMergeTiles = 6;
        int best = 1;
        long best_cost = -1;
        for (int S = 1; S <= groups; S++) {
            const GroupSplit split(ntiles, S);
            if (split.count() != S) continue;  // same split sizes as a smaller S
            const long wgs = (long)units * S;
            if (S > 1 && wgs > (long)kMatchBatchWgPerCu * cus) break;  // one round only
            const long cost = (wgs + cus - 1) / cus * split.tps + (S > 1 ? kMergeTiles : 0);
            if (best_cost < 0 || cost < best_cost) {
                best_cost = cost;
                best = S;
            }
        }
        pl.S = best;
    }
    return pl;
}

void launch_match_single(const MatchPair& pr, int S, const MatchScratch& sc, const MatchOut& out, hipStream_t s) {
    const dim3 g((max(pr.nq, 1) + kMatchSingleQB - 1) / kMatchSingleQB, S, 1);
    hipLaunchKernelGGL((k_match_single<kMatchNWSingle, kMatchQBWSingle>), g, dim3(64 * kMatchNWSingle), 0, s, pr, S,
                       sc.keys, sc.done, out.ratio, out.ratio_on_squared, out.idx2, out.d2, out.match);
}

void launch_match_codes(const MatchBatch& batch, int S, const CodeSet& set, const SetFlags& flags,
                        const MatchScratch& sc, const MatchOut& out, hipStream_t s) {
    int max_nq = 1;
    for (int p = 0; p < batch.P; p++) max_nq = max(max_nq, batch.pair[p].nq);
    const dim3 g((max_nq + kMatchBatchQB - 1) / kMatchBatchQB, S, batch.P);
    hipLaunchKernelGGL((k_match_batch<kMatchBatchNW, kMatchBatchQBW>), g, dim3(64 * kMatchBatchNW), 0, s, batch, S,
                       sc.nq_stride, set.codes, set.keys, sc.zero.codes, sc.zero.keys, flags.flags, flags.epoch, sc.keys,
                       sc.done, out.ratio, out.ratio_on_squared, out.idx2, out.d2, out.match);
}

// ---------------------------------------------------------------------------
// k_match_select: match lists (sift_hip_match_list_*).  The match kernels above
// have written the forward top-2 of every query of every pair, and -- when the
// filter needs it -- the reverse top-2 of every train row (the same kernels
// with the roles swapped), into the matcher's select scratch.  One workgroup
// per pair (1024 threads, 16 waves) walks the pair's queries in chunks of 1024:
// a lane evaluates the keep rule of its query (include/sift_hip.h) -- the
// ratio test of write_match on the forward pair, the distance cap, and for the
// cross check / two-way ratio test a gather of row i1 of the reverse arrays --
// and the kept queries take consecutive slots in query order: a 64-bit ballot
// and popcount inside the wave, the wave totals through LDS, a running base
// across chunks.  No atomics: the slot of a query depends on the keep bits of
// the queries before it only, so the output bytes are the same in every run.
// ---------------------------------------------------------------------------
constexpr int kSelectThreads = 1024, kSelectWaves = kSelectThreads / 64;

__device__ __forceinline__ bool ratio_pass(int a1, float d1, int a2, float d2, float ratio, int ratio_on_squared) {
    if (a1 < 0) return false;
    if (a2 < 0 || !(ratio > 0.f)) return true;
    if (ratio_on_squared) return d1 < ratio * d2;
    return __builtin_sqrtf(d1) < ratio * __builtin_sqrtf(d2);
}

__global__ __launch_bounds__(kSelectThreads) void k_match_select(SelectBatch batch, const int* __restrict__ idx2,
                                                                 const float* __restrict__ d2, MatchFilter f,
                                                                 MatchRecord* __restrict__ out,
                                                                 int* __restrict__ counts) {
    __shared__ int s_wave[kSelectWaves];
    const int p = blockIdx.x;
    const SelectPair pr = batch.pair[p];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const bool reverse = f.cross_check || f.ratio_both_ways;
    const int2* const fi = reinterpret_cast<const int2*>(idx2) + pr.fwd;
    const float2* const fd = reinterpret_cast<const float2*>(d2) + pr.fwd;
    const int2* const ri = reinterpret_cast<const int2*>(idx2) + pr.rev;
    const float2* const rd = reinterpret_cast<const float2*>(d2) + pr.rev;
    MatchRecord* const o = out + pr.out_off;
    int base = 0;
    for (int c0 = 0; c0 < pr.nq; c0 += kSelectThreads) {  // workgroup-uniform
        const int i = c0 + tid;
        bool keep = false;
        MatchRecord rec{i, -1, p, 0.f};
        if (i < pr.nq) {
            const int2 a = fi[i];
            const float2 e = fd[i];
            rec.trainIdx = a.x;
            rec.distance = __builtin_sqrtf(e.x);
            keep = a.x >= 0 && a.x < pr.nt && ratio_pass(a.x, e.x, a.y, e.y, f.ratio, f.ratio_on_squared) &&
                   (!(f.max_distance > 0.f) || rec.distance <= f.max_distance);
            if (keep && reverse) {
                const int2 b = ri[a.x];
                const float2 g = rd[a.x];
                if (f.cross_check) keep = b.x == i;
                if (keep && f.ratio_both_ways) keep = ratio_pass(b.x, g.x, b.y, g.y, f.ratio, f.ratio_on_squared);
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_wave[w] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kSelectWaves; k++) {
            const int c = s_wave[k];
            before += k < w ? c : 0;
            total += c;
        }
        if (keep) o[base + before + __popcll(mask & lt_mask)] = rec;
        base += total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    if (tid == 0) counts[p] = base;
}

void launch_match_select(const SelectBatch& batch, int P, const int* idx2, const float* d2, const MatchFilter& filter,
                         MatchRecord* out, int* counts, hipStream_t s) {
    hipLaunchKernelGGL(k_match_select, dim3(P), dim3(kSelectThreads), 0, s, batch, idx2, d2, filter, out, counts);
}

// ---------------------------------------------------------------------------
// k nearest neighbours (sift_hip_match_knn_*; the rule: include/sift_hip.h).
//
// k_match_knn<K> is k_match_batch's streaming loop (the same code sets, LDS-DMA
// chunks and key biases, v_mfma_i32_32x32x32_i8) with a K-entry fold in place
// of the top-2 one, 8 waves x 1 query block (256 queries per workgroup: the
// lists take the registers of a second block).  Per lane:
//   L[K]  the K largest keys of the current key group, descending.  A new key x
//         enters with L[j] = med3(L[j-1], L[j], x), L[0] = max(L[0], x): one
//         VALU per slot (keys of a group are unique; padding keys and anything
//         at or below the tail drop off the end).  The chain runs only when
//         some lane of the wave holds x > tail = max(L[K-1], thr).
//   thr   the key bound of the running K-th entry, -256 e_K: a key of a later
//         group enters only with e < e_K (earlier groups win ties), so settled
//         lists skip the chain across groups too.
//   R[K]  the running entries, ascending, one u64 each: (e ^ 2^31) << 32 | train
//         index -- unsigned order is (e, index) order.  At a group's end its
//         keys are decoded and merged in (knn_merge; the index of a later
//         group is larger, so the full-key compare is the tie rule).
// The two lane halves merge by shuffle; the entries become output keys
// (d^2 bits << 32 | index, match_key's layout) in LDS, one thread per query.
// A pair with a flagged set runs knn_f16_block: match_f16_block's arithmetic
// with a K-entry insertion.
//
// Splits: split s of pair p writes the K output keys of query i to
// lists[((p S + s) nq_stride + i) K ..]; the split that completes the query
// block's counter merges the S sorted lists in key order, writes the outputs
// and restores the counter.  The lists need no restoring.
// ---------------------------------------------------------------------------
constexpr unsigned long long kKnnNone = ~0ull;
constexpr int kKnnNW = 8, kKnnQB = 32 * kKnnNW, kKnnWgTarget = 256;
static_assert(kKnnQB >= kMatchQB, "k-NN blocks smaller than the done-counter block");

__device__ __forceinline__ unsigned long long knn_entry(int e, int idx) {
    return ((unsigned long long)((unsigned)e ^ 0x80000000u) << 32) | (unsigned)idx;
}

// The K smallest of two ascending K-lists (kKnnNone pads both) into R, ascending: C[j] = min(R[j], X[K-1-j]) holds
// them as a bitonic sequence, which log2(K) rounds of K/2 compare-exchanges sort -- K + K log2(K) selects, against
// K^2 for K insertions.
template <int K>
__device__ __forceinline__ void knn_merge(unsigned long long (&R)[K], const unsigned long long (&X)[K]) {
    static_assert((K & (K - 1)) == 0, "a bitonic network");
#pragma unroll
    for (int j = 0; j < K; j++) R[j] = R[j] < X[K - 1 - j] ? R[j] : X[K - 1 - j];
#pragma unroll
    for (int step = K / 2; step >= 1; step /= 2)
#pragma unroll
        for (int i = 0; i < K; i++)
            if ((i & step) == 0) {
                const unsigned long long a = R[i], b = R[i + step];
                R[i] = a < b ? a : b;
                R[i + step] = a < b ? b : a;
            }
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int mask) {
    const unsigned lo = __shfl_xor((unsigned)v, mask), hi = __shfl_xor((unsigned)(v >> 32), mask);
    return ((unsigned long long)hi << 32) | lo;
}

// One staged chunk (a key group, nc tiles) against a wave's query block: the
// keys of each tile into the lane's descending list L.
// Under a gate (Gate = LaneGate<1> or LaneEpipolar<1>, planes sx / sy and the
// gate's sn) the key of a (query, row) that fails the gate becomes INT_MIN
// before the ballot: below kInvalidKey and every thr, so it never enters L (in
// a chain that runs for another lane it is a no-op: med3(a, b, INT_MIN) = b for
// a >= b).  The gated fold reads its planes one row group at a time, as
// chunk_top2 does under the epipolar gate, in place of the four key loads up
// front: the registers of the K-entry lists leave no room for both.
template <int K, class Gate>
__device__ __forceinline__ void chunk_topk(const int8_t* sc, const int* sk, const float* sx, const float* sy, int nc,
                                           int col, int h, const i32x4 (&bq)[4], const Gate& g, int (&L)[K], int& tail,
                                           int thr) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int sw = (col >> 1) & 7;
    const int8_t* const ta0 = sc + col * 128;
    const int* const tk1 = sk + 4 * h;
    for (int j = 0; j < nc; j++) {  // not unrolled: 16 insertion sites per tile
        i32x4 a[4], tk[4];
#pragma unroll
        for (int kb = 0; kb < 4; kb++)
            a[kb] = *reinterpret_cast<const i32x4*>(ta0 + j * kTileBytes + 16 * ((4 * h + kb) ^ sw));
        // accumulator register i holds train row (i & 3) + 8 (i >> 2) + 4 h
        if constexpr (!kGated<Gate>) {
#pragma unroll
            for (int r = 0; r < 4; r++) tk[r] = *reinterpret_cast<const i32x4*>(tk1 + j * kMatchTileRows + 8 * r);
        }
        i32x16 acc = {};
#pragma unroll
        for (int kb = 0; kb < 4; kb++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[kb], bq[kb], acc, 0, 0, 0);
        if constexpr (kGated<Gate>) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = 4 * h + j * kMatchTileRows + 8 * r;
                const i32x4 kr = *reinterpret_cast<const i32x4*>(sk + o);
                const f32x4 xr = *reinterpret_cast<const f32x4*>(sx + o);
                const f32x4 yr = *reinterpret_cast<const f32x4*>(sy + o);
                bool pass[4];
                if constexpr (kLaneEpipolar<Gate>) {
                    const f32x4 nr = *reinterpret_cast<const f32x4*>(g.sn + o);
                    epi_pass2(g.q[0], f32x2{xr[0], xr[1]}, f32x2{yr[0], yr[1]}, f32x2{nr[0], nr[1]}, g.e2, g.radius,
                              pass[0], pass[1]);
                    epi_pass2(g.q[0], f32x2{xr[2], xr[3]}, f32x2{yr[2], yr[3]}, f32x2{nr[2], nr[3]}, g.e2, g.radius,
                              pass[2], pass[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++) pass[e] = in_gate(xr[e], yr[e], g.qx[0], g.qy[0], g.radius);
                }
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int x = pass[e] ? (acc[4 * r + e] << 9) + kr[e] : INT_MIN;
                    if (__builtin_amdgcn_ballot_w64(x > tail) != 0) {  // wave-uniform
#pragma unroll
                        for (int s = K - 1; s >= 1; s--) L[s] = med3_i32(L[s - 1], L[s], x);
                        L[0] = max(L[0], x);
                        tail = max(L[K - 1], thr);
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int x = (acc[i] << 9) + tk[i >> 2][i & 3];
                if (__builtin_amdgcn_ballot_w64(x > tail) != 0) {  // wave-uniform
#pragma unroll
                    for (int s = K - 1; s >= 1; s--) L[s] = med3_i32(L[s - 1], L[s], x);
                    L[0] = max(L[0], x);
                    tail = max(L[K - 1], thr);
                }
            }
        }
    }
}

// match_f16_block with a K-entry list: the same loads, norms, MFMA sequence and
// d = |t|^2 - 2 q.t; a strict '<' insertion in train order, the halves merged
// in (d, index) order, then + |q|^2, the non-finite query rule and the clamp.
// Under a gate the insertion also requires the row to be a candidate of the
// query, evaluated as match_f16_block does (lane col carries the position of
// train row t0 + col, under the epipolar gate its nr too, and |q|^2 is formed
// after the tile loop).  res: output keys, kKnnNone where there is no entry.
template <int K, class Gate>
__device__ void knn_f16_block(const MatchPair& pr, const Gate& g, int q0, int tbeg, int tend, int col, int h,
                              unsigned long long (&res)[K]) {
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
    float qn = 0.f;
    if constexpr (!kEpipolar<Gate>) {
        qn = sumsq8(bq);
        qn += __shfl_xor(qn, 32);
    }
    EpiQuery eq{};
    if constexpr (kEpipolar<Gate>) eq = epi_query(g.F, qx, qy);
    float dl[K];
    int il[K];
#pragma unroll
    for (int j = 0; j < K; j++) dl[j] = INFINITY, il[j] = kNone;
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
            if (t0 + row < pr.nt && cand && d < dl[K - 1]) {
#pragma unroll
                for (int j = K - 1; j >= 1; j--) {
                    const bool sh = d < dl[j - 1], here = d < dl[j];
                    il[j] = sh ? il[j - 1] : (here ? t0 + row : il[j]);
                    dl[j] = sh ? dl[j - 1] : (here ? d : dl[j]);
                }
                if (d < dl[0]) dl[0] = d, il[0] = t0 + row;
            }
        }
    }
    float od[K];
    int oi[K];
#pragma unroll
    for (int j = 0; j < K; j++) od[j] = __shfl_xor(dl[j], 32), oi[j] = __shfl_xor(il[j], 32);
#pragma unroll
    for (int e = 0; e < K; e++) {
        const float d = od[e];
        const int ix = oi[e];
#pragma unroll
        for (int j = K - 1; j >= 1; j--) {
            const bool sh = better(d, ix, dl[j - 1], il[j - 1]), here = better(d, ix, dl[j], il[j]);
            il[j] = sh ? il[j - 1] : (here ? ix : il[j]);
            dl[j] = sh ? dl[j - 1] : (here ? d : dl[j]);
        }
        if (better(d, ix, dl[0], il[0])) dl[0] = d, il[0] = ix;
    }
    if constexpr (kEpipolar<Gate>) {
        qn = sumsq8(bq);
        qn += __shfl_xor(qn, 32);
    }
    // As match_f16_block ends: every candidate carries the same qn, so no selection changes.
    const bool none = !(qn < INFINITY);
#pragma unroll
    for (int j = 0; j < K; j++) res[j] = none ? kKnnNone : match_key(fmaxf(dl[j] + qn, 0.f), il[j]);
}

__device__ __forceinline__ void write_knn(unsigned long long x, int j, int k, size_t o, int* __restrict__ idx,
                                          float* __restrict__ d2) {
    const bool v = x != kKnnNone;
    if (idx) idx[o * k + j] = v ? (int)(unsigned)x : -1;
    if (d2) d2[o * k + j] = v ? __uint_as_float((unsigned)(x >> 32)) : FLT_MAX;
}

// The gate of a k-NN launch (Gate = NoGate, MatchGate or EpipolarGate): the
// batch record the kernel takes and the gate of its pair p.  An ungated launch
// takes k_match_batch's pairs; a gated one pairs with their position arrays and
// the call-wide gate fields (KnnGatedBatch).
template <class Gate>
struct KnnBatchOf {
    typedef KnnGatedBatch type;
};
template <>
struct KnnBatchOf<NoGate> {
    typedef MatchBatch type;
};
__device__ __forceinline__ MatchGate knn_gate(const KnnGatedBatch& b, int p, const MatchGate*) {
    return MatchGate{b.qxy[p], b.txy[p], b.call.qstride, b.call.tstride, b.call.radius};
}
// Pair p's nine floats: from device memory as k_match_epipolar_batch reads them
// (one wave-uniform load, kept in scalar registers), or -- geometry == nullptr,
// the single-pair calls, whose F the host has checked -- from the kernel
// arguments.  An unusable record (a value that is not finite, or nine zeros)
// makes e2 NaN, which fails every compare of the gate: no candidates.
__device__ __forceinline__ EpipolarGate knn_gate(const KnnGatedBatch& b, int p, const EpipolarGate*) {
    float f[9];
    if (b.call.geometry) {
        const unsigned* const G = reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(b.call.geometry) +
                                                                    (size_t)b.geom[p] * b.call.geometry_stride);
#pragma unroll
        for (int e = 0; e < 9; e++) f[e] = __uint_as_float(__builtin_amdgcn_readfirstlane(G[e]));
    } else {
#pragma unroll
        for (int e = 0; e < 9; e++) f[e] = b.F[e];
    }
    bool usable = true, zero = true;
#pragma unroll
    for (int e = 0; e < 9; e++) {
        usable = usable && __builtin_fabsf(f[e]) < INFINITY;
        zero = zero && f[e] == 0.f;
    }
    usable = usable && !zero;
    EpipolarGate g{b.qxy[p], b.txy[p], b.call.qstride, b.call.tstride, b.call.radius, usable ? b.call.e2 : NAN, {}};
#pragma unroll
    for (int e = 0; e < 9; e++) g.F[e] = f[e];
    return g;
}

// grid = (query blocks of kKnnQB, splits S of whole key groups, pairs).  Pair p
// reads code rows qrow0.. of qs and trow0.. of ts (one buffer for prepared or
// gathered sets, two for a pair of sidecars).  Under a gate the train positions
// of each chunk are staged beside its keys (two float planes per buffer, under
// the epipolar gate a third for the rows' nr, filled once per chunk as
// match_pair does) and the lane keeps its query's side in registers; the group
// decode, the merges and the split lists do not know the gate.
//
// Registers: the integer path of every instantiation fits two workgroups per CU (128 registers), and so does all of
// the ungated kernel and of <4, MatchGate>.  The general path of the other three gated instantiations does not (the
// K-entry lists, two operand sets and the gate's state: 20-76 B of scratch at that bound), so those three are built
// for one workgroup per CU instead of spilling (profiles/knn_gated/resources.json).
template <int K, class Gate>
constexpr int knn_wg_per_cu() {
    return kGated<Gate> && !(K == 4 && std::is_same<Gate, MatchGate>::value) ? 1 : 2;
}
template <int K, class Gate = NoGate>
__global__ __launch_bounds__(64 * kKnnNW, (knn_wg_per_cu<K, Gate>() * kKnnNW) / 4) void k_match_knn(
    typename KnnBatchOf<Gate>::type batch, int S, int k, int nq_stride, const int8_t* __restrict__ qcodes,
    const int* __restrict__ qkeys, const int8_t* __restrict__ tcodes, const int* __restrict__ tkeys,
    const int8_t* __restrict__ zc, const int* __restrict__ zk, const unsigned* __restrict__ flags, unsigned epoch,
    unsigned long long* __restrict__ lists, unsigned* __restrict__ done, int* __restrict__ idx,
    float* __restrict__ d2out) {
    constexpr int NW = kKnnNW, QB = kKnnQB;
    static_assert(sizeof(unsigned long long) * K * QB <= kChunkTiles * kTileBytes, "results alias the code tiles");
    __shared__ __attribute__((aligned(16))) int8_t s_codes[2][kChunkTiles * kTileBytes];
    __shared__ __attribute__((aligned(16))) int s_key[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_px[2][kChunkRows];  // the planes: gated instantiations only
    __shared__ __attribute__((aligned(16))) float s_py[2][kChunkRows];
    __shared__ __attribute__((aligned(16))) float s_pn[2][kChunkRows];  // the epipolar gate only
    __shared__ unsigned s_last;
    const int p = blockIdx.z;
    const MatchPair& pr = batch.pair[p];
    const int q0 = blockIdx.x * QB;
    if (q0 >= pr.nq) return;
    // The wave's index w: under a gate as a scalar (match_pair: the register that keeps the epipolar body in budget).
    const int tid = threadIdx.x, lane = tid & 63, w = kGated<Gate> ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6,
              col = lane & 31, h = lane >> 5;
    const GroupSplit split(match_tiles(pr.nt), S);
    const int tb = split.begin(blockIdx.y), te = split.end(blockIdx.y);
    const int q0w = q0 + 32 * w;
    Gate g{};
    if constexpr (kGated<Gate>) g = knn_gate(batch, p, static_cast<const Gate*>(nullptr));
    unsigned long long res[K];
    if (!flags || (flags[pr.qset] != epoch && flags[pr.tset] != epoch)) {
        // ---- integer path ----
        const int8_t* __restrict__ tc = tcodes + (size_t)pr.trow0 * 128;
        const int* __restrict__ tk = tkeys + pr.tkrow0;
        auto stage = [&](int c0, int buf) {
            stage_dma<NW>(tc, tk, pr.nt, c0 * kMatchTileRows, min(kChunkTiles, te - c0), zc, zk, s_codes[buf], s_key[buf],
                          w, lane);
            if constexpr (kGated<Gate>)
                stage_pos_dma<NW>(g.txy, g.tstride, pr.nt, c0 * kMatchTileRows, min(kChunkTiles, te - c0), s_px[buf],
                                  s_py[buf], w, lane);
        };
        if (tb < te) stage(tb, 0);
        i32x4 bq[1][4];
        int qn[1];
        load_queries<1>(qcodes + (size_t)pr.qrow0 * 128, qkeys + pr.qkrow0, pr.nq, q0w, col, h, bq, qn);
        auto lg = lane_gate<1>(g, pr.nq, q0w, col);
        unsigned long long R[K];
#pragma unroll
        for (int j = 0; j < K; j++) R[j] = kKnnNone;
        int buf = 0;
        for (int c0 = tb; c0 < te; c0 += kChunkTiles, buf ^= 1) {
            __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // as in k_match_batch
            __syncthreads();
            if (c0 + kChunkTiles < te) stage(c0 + kChunkTiles, buf ^ 1);
            // key > thr <=> e < e_K (256 e_K fits: the key range above); no K-th entry yet: every valid key.
            const int eK = (int)((unsigned)(R[K - 1] >> 32) ^ 0x80000000u);
            const int thr = R[K - 1] == kKnnNone ? kInvalidKey : max(kInvalidKey, (int)(0u - 256u * (unsigned)eK));
            int L[K], tail = thr;
#pragma unroll
            for (int j = 0; j < K; j++) L[j] = INT_MIN;
            const float *sx = nullptr, *sy = nullptr;
            if constexpr (kGated<Gate>) sx = s_px[buf], sy = s_py[buf];
            if constexpr (kEpipolar<Gate>) {
                for (int r = tid; r < kChunkRows; r += 64 * NW) s_pn[buf][r] = epi_row(g.F, sx[r], sy[r]);
                lg.sn = s_pn[buf];
                __syncthreads();
            }
            chunk_topk<K>(s_codes[buf], s_key[buf], sx, sy, min(kChunkTiles, te - c0), col, h, bq[0], lg, L, tail, thr);
            const int t0 = c0 * kMatchTileRows;
            if (__builtin_amdgcn_ballot_w64(L[0] > thr) != 0) {  // some lane's group holds a new entry
                unsigned long long X[K];  // ascending: L descends, and what does not beat thr pads the end
#pragma unroll
                for (int j = 0; j < K; j++) {
                    const int s = -L[j];  // 256 e + r
                    X[j] = L[j] > thr ? knn_entry(s >> 8, t0 + (s & 255)) : kKnnNone;
                }
                knn_merge(R, X);
            }
        }
        unsigned long long O[K];
#pragma unroll
        for (int j = 0; j < K; j++) O[j] = shfl_xor_u64(R[j], 32);
        knn_merge(R, O);
#pragma unroll
        for (int j = 0; j < K; j++) {
            const int e = (int)((unsigned)(R[j] >> 32) ^ 0x80000000u);
            res[j] = R[j] == kKnnNone ? kKnnNone : match_key((float)(e + qn[0]), (int)(unsigned)R[j]);
        }
    } else {
        // ---- general path: fp16 values that are not integers 0..255 ----
        knn_f16_block<K>(pr, g, q0w, tb, te, col, h, res);
    }
    unsigned long long* const s_res = reinterpret_cast<unsigned long long*>(&s_codes[0][0]);
    __syncthreads();  // s_res aliases the code tiles
    if (h == 0) {
#pragma unroll
        for (int j = 0; j < K; j++) s_res[(32 * w + col) * K + j] = res[j];
    }
    __syncthreads();
    const int q = q0 + tid;
    const bool qv = tid < QB && q < pr.nq;
    const size_t o = (size_t)pr.out_off + q;
    if (S == 1) {
        if (qv) {
#pragma unroll
            for (int j = 0; j < K; j++)
                if (j < k) write_knn(s_res[tid * K + j], j, k, o, idx, d2out);
        }
        return;
    }
    // Agent-scope atomic stores and loads of the lists: they bypass the caches that are not coherent across XCDs, so
    // no cache write-back or invalidate is needed, only their completion (vmcnt) before the count.
    unsigned long long* const pl = lists + (size_t)p * S * nq_stride * K;
    if (qv) {
        unsigned long long* dst = pl + ((size_t)blockIdx.y * nq_stride + q) * K;
#pragma unroll
        for (int j = 0; j < K; j++)
            __hip_atomic_store(dst + j, s_res[tid * K + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* const cnt = done + (size_t)p * gridDim.x + blockIdx.x;
    if (tid == 0) s_last = atomicAdd(cnt, 1u) + 1u == (unsigned)S;
    __syncthreads();
    if (!s_last) return;
    if (qv) {
        unsigned long long M[K];
#pragma unroll
        for (int j = 0; j < K; j++) M[j] = kKnnNone;
        for (int s = 0; s < S; s++) {
            // The K loads of a list go out together (one round trip per list, not per key).
            const unsigned long long* src = pl + ((size_t)s * nq_stride + q) * K;
            unsigned long long x[K];
#pragma unroll
            for (int j = 0; j < K; j++) x[j] = __hip_atomic_load(src + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            knn_merge(M, x);
        }
#pragma unroll
        for (int j = 0; j < K; j++)
            if (j < k) write_knn(M[j], j, k, o, idx, d2out);
    }
    if (tid == 0) atomicExch(cnt, 0u);
}

int match_knn_splits(int max_nq, int max_nt, int P) {
    const int ntiles = match_tiles(max_nt), groups = (ntiles + kGroupTiles - 1) / kGroupTiles;
    const int units = (max(max_nq, 1) + kKnnQB - 1) / kKnnQB * max(P, 1);
    return GroupSplit(ntiles, max(1, min(min(groups, kKnnMaxSplits), kKnnWgTarget / units))).count();
}

void launch_match_knn(const MatchBatch& batch, int S, int k, const CodeSet& q, const CodeSet& t, const SetFlags& flags,
                      const KnnScratch& sc, int* idx, float* d2, hipStream_t s) {
    int max_nq = 1;
    for (int p = 0; p < batch.P; p++) max_nq = max(max_nq, batch.pair[p].nq);
    const dim3 g((max_nq + kKnnQB - 1) / kKnnQB, S, batch.P), b(64 * kKnnNW);
    if (k <= 4)
        hipLaunchKernelGGL(k_match_knn<4>, g, b, 0, s, batch, S, k, sc.nq_stride, q.codes, q.keys, t.codes, t.keys,
                           sc.zero.codes, sc.zero.keys, flags.flags, flags.epoch, sc.lists, sc.done, idx, d2);
    else
        hipLaunchKernelGGL(k_match_knn<8>, g, b, 0, s, batch, S, k, sc.nq_stride, q.codes, q.keys, t.codes, t.keys,
                           sc.zero.codes, sc.zero.keys, flags.flags, flags.epoch, sc.lists, sc.done, idx, d2);
}

// Gated k-NN: the pairs of `batch` (at most kMaxGatedPairs) under its gate, the window's or (epipolar) the epipolar
// one.  The launch shape, the splits and the scratch are the ungated launch's.
void launch_match_knn_gated(const KnnGatedBatch& batch, bool epipolar, int S, int k, const CodeSet& q, const CodeSet& t,
                            const SetFlags& flags, const KnnScratch& sc, int* idx, float* d2, hipStream_t s) {
    int max_nq = 1;
    for (int p = 0; p < batch.P; p++) max_nq = max(max_nq, batch.pair[p].nq);
    const dim3 g((max_nq + kKnnQB - 1) / kKnnQB, S, batch.P), b(64 * kKnnNW);
#define SIFT_KNN_GATED(K, Gate)                                                                                         \
    hipLaunchKernelGGL((k_match_knn<K, Gate>), g, b, 0, s, batch, S, k, sc.nq_stride, q.codes, q.keys, t.codes, t.keys, \
                       sc.zero.codes, sc.zero.keys, flags.flags, flags.epoch, sc.lists, sc.done, idx, d2)
    if (epipolar) {
        if (k <= 4)
            SIFT_KNN_GATED(4, EpipolarGate);
        else
            SIFT_KNN_GATED(8, EpipolarGate);
    } else {
        if (k <= 4)
            SIFT_KNN_GATED(4, MatchGate);
        else
            SIFT_KNN_GATED(8, MatchGate);
    }
#undef SIFT_KNN_GATED
}

// k_knn_select: the capped radius list.  One workgroup per pair walks the
// pair's nq k table entries in (query, rank) order, 1024 at a time; an entry is
// kept when it holds a neighbour within max_distance, and the kept entries take
// consecutive slots by the ballot / popcount / LDS prefix of k_match_select.
__global__ __launch_bounds__(kSelectThreads) void k_knn_select(SelectBatch batch, int k, const int* __restrict__ idx,
                                                               const float* __restrict__ d2, float max_distance,
                                                               MatchRecord* __restrict__ out,
                                                               int* __restrict__ counts) {
    __shared__ int s_wave[kSelectWaves];
    const int p = blockIdx.x;
    const SelectPair pr = batch.pair[p];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const int* const ti = idx + (size_t)pr.fwd * k;
    const float* const td = d2 + (size_t)pr.fwd * k;
    MatchRecord* const o = out + pr.out_off;
    const int n = pr.nq * k;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += kSelectThreads) {  // workgroup-uniform
        const int e = c0 + tid;
        bool keep = false;
        MatchRecord rec{0, -1, p, 0.f};
        if (e < n) {
            rec.queryIdx = e / k;
            rec.trainIdx = ti[e];
            rec.distance = __builtin_sqrtf(td[e]);
            keep = rec.trainIdx >= 0 && (!(max_distance > 0.f) || rec.distance <= max_distance);
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_wave[w] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < kSelectWaves; j++) {
            const int c = s_wave[j];
            before += j < w ? c : 0;
            total += c;
        }
        if (keep) o[base + before + __popcll(mask & lt_mask)] = rec;
        base += total;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    if (tid == 0) counts[p] = base;
}

void launch_knn_select(const SelectBatch& batch, int P, int k, const int* idx, const float* d2, float max_distance,
                       MatchRecord* out, int* counts, hipStream_t s) {
    hipLaunchKernelGGL(k_knn_select, dim3(P), dim3(kSelectThreads), 0, s, batch, k, idx, d2, max_distance, out, counts);
}

}  // namespace sift_amd
