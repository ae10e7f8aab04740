// Matcher launch interface: the launchers of match.hip, match_select.hip and match_knn.hip as matcher_api.hip's host path (the C ABI) calls them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sift_amd {

constexpr int kMaxMatchPairs = 64;
constexpr int kMatchQB = 128;       // queries per workgroup, smallest plan (done counters are sized per kMatchQB block)
constexpr int kMatchTileRows = 32;  // train rows per MFMA tile
constexpr int kChunkTiles = 8;      // train tiles per LDS chunk (32 KiB of codes + 1 KiB of keys, double buffered)
constexpr int kMatchWgPerCu = 2;    // workgroups per CU the kernel is register-budgeted for
constexpr int kMatchPadKey = -2140000000;  // key bias of a padding row (below every valid key)

struct MatchPair {
    const uint16_t* q;  // nq x 128 half, row-major
    const uint16_t* t;  // nt x 128 half, row-major
    int nq, nt;
    int out_off;        // output row offset of this pair
    int qset, tset;     // this call's prepared sets (k_match_prep) holding q and t
    int qrow0, trow0;   // their first int8 code row
    int qkrow0, tkrow0; // their first key bias (prepared sets: = qrow0 / trow0; gathered code buffers may differ)
};
static_assert(sizeof(MatchPair) == 56, "kernarg layout");

// Passed by value: lives in the kernarg segment (64 x 56 B = 3.5 KiB).
struct MatchBatch {
    MatchPair pair[kMaxMatchPairs];
    int P;
};

// A distinct descriptor set of one call (sets are deduplicated by pointer: the
// 8-way match has 8 sets for 56 pairs): n rows at src -> codes row0 ...
struct MatchSet {
    const uint16_t* src;
    int n, row0;
};
struct MatchSets {
    MatchSet set[2 * kMaxMatchPairs];
    int nsets, maxn;
};

// Launch plan: waves per workgroup (64 queries per wave) and, for the fused
// single-pair kernel, train splits S (the train tiles are cut into S
// contiguous ranges, one workgroup per (query block, range), merged through
// the keys scratch); batched splits are whole key groups.
struct MatchPlan {
    int nw, S;
};
MatchPlan match_plan(int max_nq, int max_nt, int P);
int match_direct_splits(int nq, int nt);  // splits of launch_match_pair

// --- Launch records.  What travels together through the launchers travels as
// one record; the launchers unpack them into the kernels' parameter lists.
//
// A code set: int8 code rows (128 B) and per row the key bias
// -(256 |code|^2 + (row mod 256)).  A detector buffer's sidecar (sift_kernels.h
// Sidecar), rows of the matcher's prepared codes (k_match_prep), or a caller's
// gathered code buffer.
struct CodeSet {
    const int8_t* codes;
    const int* keys;
};
// The flags of prepared sets: one word per set slot of the call, == epoch when
// that set holds a value that is not an integer 0..255 (its pairs take the
// general f16 path on pr.q / pr.t).  flags == nullptr: ready code sets,
// integers by construction.
struct SetFlags {
    unsigned* flags;
    unsigned epoch;
};
// The matcher's scratch (filled from a sift_hip_matcher in one place,
// matcher_api.hip).  keys: 2 x u64 per (pair, query), pair p at row p *
// nq_stride, all ones between calls; done: a counter per (pair, kMatchQB-query
// block), zero between calls (the merging workgroup resets both, so launches
// ordered on a stream may share them).  zero: the sentinel row, a zero code row
// with the padding key (written once at allocation, never by a call), read in
// place of rows past a set's end.
struct MatchScratch {
    unsigned long long* keys;
    unsigned* done;
    int nq_stride;
    CodeSet zero;
};
// What a call asks for: per query the top-2 indices (idx2) and squared
// distances (d2), two entries each, and the ratio-tested match; a null pointer
// skips that output.
struct MatchOut {
    float ratio;
    int ratio_on_squared;
    int* idx2;
    float* d2;
    int* match;
};

// The gate of guided matching as the kernel takes it (sift_hip_match_gate; the
// window rule is in include/sift_hip.h): row i of a set has its position at
// xy[i * stride + {0, 1}].
struct MatchGate {
    const float* qxy;
    const float* txy;
    int qstride, tstride;
    float radius;
};

// The gate of guided matching under a fundamental matrix
// (sift_hip_match_epipolar_gate; the rule is in include/sift_hip.h): the
// positions as MatchGate's, F row-major with x_train^T F x_query = 0, and
// e2 = max_error * max_error (one float32 product, formed on the host).  The
// reverse direction of a pair takes the positions swapped and F transposed.
struct EpipolarGate {
    const float* qxy;
    const float* txy;
    int qstride, tstride;
    float radius;
    float e2;
    float F[9];
};

// One pair of fp16 sets, converted in the kernel (k_match_single), S =
// match_plan(nq, nt, 1).S splits.
void launch_match_single(const MatchPair& pr, int S, const MatchScratch& sc, const MatchOut& out, hipStream_t s);

// k_match_prep: the call's distinct sets into codes / rowkeys (capacity for the
// call's sets) and their flags.
void launch_match_prep(const MatchSets& sets, int8_t* codes, int* rowkeys, const SetFlags& flags, hipStream_t s);

// Pairs of code sets (k_match_batch, S = match_plan(.., P >= 2).S splits):
// pair p reads code rows qrow0.. / trow0.. and key biases qkrow0.. / tkrow0..
// of `set` -- what launch_match_prep wrote (with its flags), or ready codes
// with no prep launch and no flags (e.g. the sidecars of every rank
// all-gathered: C5).
void launch_match_codes(const MatchBatch& batch, int S, const CodeSet& set, const SetFlags& flags,
                        const MatchScratch& sc, const MatchOut& out, hipStream_t s);

// One pair of ready code sets q / t, match_direct_splits(nq, nt) splits.
// gate == nullptr: k_match_direct, for sets that are integers by construction
// (sidecars; the kernel reads no flags).  Under a gate: k_match_guided, on
// sidecars (no flags) or on what launch_match_prep wrote, where a flagged set
// (flags[pr.qset], flags[pr.tset]) sends the pair down the gated fp16 path.
void launch_match_pair(const MatchPair& pr, const MatchGate* gate, const CodeSet& q, const CodeSet& t,
                       const SetFlags& flags, const MatchScratch& sc, const MatchOut& out, hipStream_t s);
// The same pair under an epipolar gate: k_match_epipolar, the guided kernel's
// launch shape and flag rule.
void launch_match_pair(const MatchPair& pr, const EpipolarGate& gate, const CodeSet& q, const CodeSet& t,
                       const SetFlags& flags, const MatchScratch& sc, const MatchOut& out, hipStream_t s);

// --- Gated batches (sift_hip_match_*_guided_batched / *_epipolar_batched): pairs of code sets under a gate in one
// launch (k_match_guided_batch, k_match_epipolar_batch).
//
// Pair p of a gated launch: the pair as k_match_batch takes it (rows of the launch's code set, its fp16 rows for the
// general path) and the two position arrays of its direction.  swapped marks the reverse direction of a cross check:
// the pair reads the launch's strides swapped and, under the epipolar gate, its geometry transposed; geom is the
// index of its geometry record (a reverse pair shares its forward pair's).
struct GatedPair {
    MatchPair pr;
    const float* qxy;
    const float* txy;
    int geom, swapped;
};
static_assert(sizeof(GatedPair) == 80, "kernarg layout");

// Passed by value, like MatchBatch, so a launch holds at most kMaxGatedPairs pairs (32 x 80 B = 2.5 KiB of kernarg
// beside the other arguments; 64 would not fit the 4 KiB segment).  A call of more pairs is several launches ordered
// on the stream: the scratch is restored when each ends, and the bytes do not depend on the cut.
constexpr int kMaxGatedPairs = 32;
struct GatedBatch {
    GatedPair pair[kMaxGatedPairs];
    int P;
};

// What is uniform over a gated call: the strides of the forward direction, the radius, and under the epipolar gate
// e2 = max_error * max_error (formed on the host) and the geometry records in device memory -- pair p's nine floats
// at geometry + geom * geometry_stride bytes, read by the kernel and never by the host.  geometry == nullptr: the
// window gate.
struct GatedCall {
    int qstride, tstride;
    float radius, e2;
    const void* geometry;
    int geometry_stride;
};

// The pairs of `batch` on rows of `set` (what launch_match_prep wrote, with its flags, or ready codes without), S =
// match_gated_splits(max nq, max nt, batch.P) splits.
int match_gated_splits(int max_nq, int max_nt, int P);
void launch_match_gated(const GatedBatch& batch, const GatedCall& call, const CodeSet& set, const SetFlags& flags,
                        const MatchScratch& sc, const MatchOut& out, hipStream_t s);

// --- Match lists (sift_hip_match_list_*): filter + ordered compaction of the
// top-2 arrays the launchers above wrote (k_match_select).
//
// One record per kept query, cv::DMatch's layout (sift_hip_dmatch).
struct MatchRecord {
    int queryIdx, trainIdx, imgIdx;
    float distance;
};
static_assert(sizeof(MatchRecord) == 16, "cv::DMatch layout");

// The keep rule's parameters (sift_hip_match_filter; the rule is in include/sift_hip.h).
struct MatchFilter {
    float ratio;
    int ratio_on_squared, ratio_both_ways;
    float max_distance;
    int cross_check;
};

// Pair p of a select launch: the forward top-2 of its query i is row fwd + i of
// idx2 / d2, the reverse top-2 of its train row t is row rev + t (read only when
// the filter needs the reverse direction), its records go to out + out_off.
struct SelectPair {
    int nq, nt, fwd, rev, out_off;
};
// Passed by value (64 x 20 B of kernarg).
struct SelectBatch {
    SelectPair pair[kMaxMatchPairs];
};

// One 1024-thread workgroup per pair: records of the kept queries in ascending
// query order at out + out_off, their number in counts[p].
void launch_match_select(const SelectBatch& batch, int P, const int* idx2, const float* d2, const MatchFilter& filter,
                         MatchRecord* out, int* counts, hipStream_t s);

// --- k nearest neighbours (sift_hip_match_knn_*): k_match_knn, k_knn_select.
constexpr int kKnnMax = 8;        // SIFT_HIP_KNN_MAX; the kernel is instantiated for 4 and 8 entries
constexpr int kKnnMaxSplits = 8;  // train splits of a k-NN launch at most

// The k-NN scratch of a matcher (allocated at its first k-NN call).  lists: a
// sorted list of u64 output keys per (pair, split, query) -- P S nq_stride lists
// of at most kKnnMax keys must fit; nothing in it outlives a launch.  done: the
// matcher's done counters (MatchScratch), zero between calls.
struct KnnScratch {
    unsigned long long* lists;
    unsigned* done;
    int nq_stride;
    CodeSet zero;
};

// Splits (whole key groups) of a k-NN launch of this shape, before the cap of
// the matcher's list scratch.
int match_knn_splits(int max_nq, int max_nt, int P);

// The k nearest neighbours of every query of every pair: idx / d2 rows of k
// entries, pair p at row out_off.  Pair p reads code rows qrow0.. of q and
// trow0.. of t (the same buffer for prepared or gathered sets; two sidecars for
// one pair of detector buffers); a flagged set sends its pair down the fp16
// path.
void launch_match_knn(const MatchBatch& batch, int S, int k, const CodeSet& q, const CodeSet& t, const SetFlags& flags,
                      const KnnScratch& sc, int* idx, float* d2, hipStream_t s);

// --- Gated k-NN (sift_hip_match_knn_guided_* / *_epipolar_*): k_match_knn under the window or the epipolar gate.
//
// The pairs of one launch as k_match_knn takes them (MatchPair), beside them their position arrays and the index of
// their geometry record (k-NN has no reverse direction, so nothing is swapped), and what is uniform over the call
// (GatedCall).  Under the epipolar gate pair p's nine floats are read from device memory at call.geometry + geom[p] *
// geometry_stride, or -- call.geometry == nullptr, the single-pair calls -- F, checked on the host, travels in the
// kernel arguments: no host-to-device copy.  Passed by value (2.5 KiB of kernarg), at most kMaxGatedPairs pairs.
struct KnnGatedBatch {
    MatchPair pair[kMaxGatedPairs];
    const float* qxy[kMaxGatedPairs];
    const float* txy[kMaxGatedPairs];
    int geom[kMaxGatedPairs];
    int P;
    GatedCall call;
    float F[9];
};

// S splits as launch_match_knn takes them; the scratch, the code sets and the flag rule are launch_match_knn's.
void launch_match_knn_gated(const KnnGatedBatch& batch, bool epipolar, int S, int k, const CodeSet& q, const CodeSet& t,
                            const SetFlags& flags, const KnnScratch& sc, int* idx, float* d2, hipStream_t s);

// One workgroup per pair: the table entries (rows fwd.. of idx / d2, k per row)
// that hold a neighbour within max_distance, in (query, rank) order at out +
// out_off, their number in counts[p].
void launch_knn_select(const SelectBatch& batch, int P, int k, const int* idx, const float* d2, float max_distance,
                       MatchRecord* out, int* counts, hipStream_t s);

}  // namespace sift_amd
