// k nearest neighbours (k <= 8) on MFMA for gfx950: k_match_batch's streaming
// loop (match.hip) with a K-entry fold.  The gate is a template parameter:
// k_match_knn<K, MatchGate / EpipolarGate> is the k-NN inside the window or the
// epipolar band, single or batched.  The capped radius list of its table is
// k_knn_select (match_select.hip).
#include "sift_match_dev.h"

namespace sift_amd {

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

}  // namespace sift_amd
