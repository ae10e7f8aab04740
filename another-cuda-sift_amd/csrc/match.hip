// Brute-force L2 matcher on MFMA for gfx950.
//
// Replaces the reference's sift_cuda/sift_func/Match.cu:8-177 (32 lanes per
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
//  k_match_select / k_knn_select  match lists from the top-2 arrays and the
//                  capped radius list of the k-NN table: match_select.hip.
//  k_match_knn     k nearest neighbours (k <= 8) of every query of every pair,
//                  with or without a gate: match_knn.hip.
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
// Shared core (sift_match_dev.h): one integer fold (chunk_top2) and one fp16 block
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
#include "sift_match_dev.h"

namespace sift_amd {

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

}  // namespace sift_amd
