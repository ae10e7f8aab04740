// Matcher handle (sift_hip_matcher_*, sift_hip_match_*) and the descriptor
// sidecar registry of libsift_hip.so; the kernels are match.hip, match_select.hip
// and match_knn.hip.  Replaces
// /root/reference/sift_cuda/sift_func/Match.cu:8-33 (matchBruteForce).
//
// Every match entry point fills one MatchCall and hands it to run(): one
// checker, one staging function for fp16 sets, one reverse-pair builder and
// direction policy ("The matcher's host path: one call record").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <initializer_list>
#include <string>

#include "detector_state.h"
#include "sift_match.h"

namespace sift_amd {
namespace det {

// Matcher sidecars of the descriptor buffers the detector handles hand out
// (one per results slot and frame of every lane): exact buffer base -> its
// int8 codes and key biases (sift_kernels.h Sidecar).  sift_hip_match_* look
// the query and train pointers up and, when both are detector buffers, match
// their codes directly (k_match_direct) instead of converting the fp16 rows.
// A caller that writes into a detector descriptor buffer declares it
// (sift_hip_descriptors_written, DeviceBuffer::mutable_data): the entry is
// then stale -- matches on the buffer convert its fp16 rows -- until the
// detector launches a frame into that buffer again (sidecar_refreshed).
struct SidecarReg {
    const uint16_t* desc;
    Sidecar side;
    int cap;
    const void* owner;
    bool stale;
};
std::mutex g_side_mu;
std::vector<SidecarReg> g_side;
std::atomic<int> g_side_stale{0};  // stale entries (the per-frame refresh is free while 0)

void register_sidecar(const void* owner, const uint16_t* desc, Sidecar side, int cap) {
    std::lock_guard<std::mutex> g(g_side_mu);
    g_side.push_back(SidecarReg{desc, side, cap, owner, false});
}
void unregister_sidecars(const void* owner) {
    std::lock_guard<std::mutex> g(g_side_mu);
    for (const SidecarReg& r : g_side)
        if (r.owner == owner && r.stale) g_side_stale--;
    g_side.erase(std::remove_if(g_side.begin(), g_side.end(), [&](const SidecarReg& r) { return r.owner == owner; }),
                 g_side.end());
}
bool find_sidecar(const uint16_t* desc, int n, Sidecar* out) {
    std::lock_guard<std::mutex> g(g_side_mu);
    for (const SidecarReg& r : g_side)
        if (r.desc == desc && n <= r.cap && !r.stale) {
            *out = r.side;
            return true;
        }
    return false;
}
bool sidecar_written(const uint16_t* desc) {
    std::lock_guard<std::mutex> g(g_side_mu);
    bool found = false;
    for (SidecarReg& r : g_side)
        if (r.desc == desc) {
            found = true;
            if (!r.stale) {
                r.stale = true;
                g_side_stale++;
            }
        }
    return found;
}
void sidecar_refreshed(const uint16_t* desc) {
    if (g_side_stale.load() == 0) return;
    std::lock_guard<std::mutex> g(g_side_mu);
    for (SidecarReg& r : g_side)
        if (r.desc == desc && r.stale) {
            r.stale = false;
            g_side_stale--;
        }
}

}  // namespace det
}  // namespace sift_amd

struct sift_hip_matcher {
    int device = 0;
    int maxQ = 0, maxT = 0, maxP = 0;
    unsigned long long* dKeys = nullptr;  // running top-2 keys per (pair, query), all ones between calls
    unsigned* dDone = nullptr;            // finished splits per (pair, 256-query block), zero between calls
    int* dMatch = nullptr;
    int8_t* dCodes = nullptr;             // int8 codes of a call's distinct sets (k_match_prep)
    int* dRowKeys = nullptr;              // key bias per code row; row codeRows: the zero/padding sentinel
    unsigned* dFlags = nullptr;           // per set slot: == epoch if the set is not all integers 0..255
    long codeRows = 0;
    unsigned epoch = 0;
    bool sidecars = true;  // single pairs of detector buffers: match their sidecar codes (k_match_direct)
    // Match lists (sift_hip_match_list_*), allocated at the first such call: the top-2 arrays of the forward pairs
    // (rows 0 .. sum nq) and of the reverse pairs (after them), 2 maxP maxQ rows of two entries each; the records
    // and the count of sift_hip_match_list_host.
    int* dSelIdx = nullptr;
    float* dSelD = nullptr;
    MatchRecord* dList = nullptr;
    int* dCount = nullptr;
    // k nearest neighbours (sift_hip_match_knn_*), allocated at the first such call: the split lists (knn_lists()
    // lists of kKnnMax keys), and for the list and host forms the k-NN table of maxP maxQ rows of kKnnMax entries,
    // the records of one pair and its count.
    unsigned long long* dKnnLists = nullptr;
    int* dKnnIdx = nullptr;
    float* dKnnD = nullptr;
    MatchRecord* dKnnRec = nullptr;
    int* dKnnCount = nullptr;
    ~sift_hip_matcher() {
        (void)hipSetDevice(device);
        for (void* p : {(void*)dKeys, (void*)dDone, (void*)dMatch, (void*)dCodes, (void*)dRowKeys, (void*)dFlags,
                        (void*)dSelIdx, (void*)dSelD, (void*)dList, (void*)dCount, (void*)dKnnLists, (void*)dKnnIdx,
                        (void*)dKnnD, (void*)dKnnRec, (void*)dKnnCount})
            if (p) (void)hipFree(p);
    }
    // Split lists of the k-NN scratch: max_query * max(8, 2 max_pairs) (the formula of include/sift_hip.h).
    size_t knn_lists() const { return (size_t)maxQ * std::max(kKnnMaxSplits, 2 * maxP); }
    // The sentinel row (row codeRows of dCodes / dRowKeys): zero codes with the padding key, written at creation.
    CodeSet sentinel() const { return CodeSet{dCodes + (size_t)codeRows * 128, dRowKeys + codeRows}; }
    MatchScratch scratch() const { return MatchScratch{dKeys, dDone, maxQ, sentinel()}; }
    // The prepared sets of a call get a new epoch: flags from earlier calls never equal it.
    SetFlags next_epoch() {
        epoch = epoch + 1 == 0 ? 1 : epoch + 1;
        return SetFlags{dFlags, epoch};
    }
};

static_assert(sizeof(sift_hip_dmatch) == sizeof(MatchRecord) && sizeof(sift_hip_dmatch) == 16, "cv::DMatch layout");
static_assert(sizeof(sift_hip_match_filter) == sizeof(MatchFilter), "the filter is passed to the kernel as it is");
static_assert(sizeof(sift_hip_match_positions) == 2 * sizeof(void*), "two device pointers per pair");
static_assert(SIFT_HIP_KNN_MAX == kKnnMax, "the kernel's largest instantiation");

// --- One call record ------------------------------------------------------------
namespace {

const SetFlags kNoFlags{nullptr, 0u};  // ready code sets: integers by construction

enum class Op { Top2, List, KnnTable, KnnList };
enum class Gate { None, Window, Epipolar };

// How an entry family words the rules every family has: a null matcher, P outside 1..max_pairs, a null size array,
// a null descriptor array.  (Null code arrays are "bad code batch", null positions "bad gated batch", everywhere.)
struct Wording {
    const char *matcher, *pairs, *sizes, *sets;
};
const Wording kBatchWords{"bad batch", "bad batch", "bad batch", "bad batch"};
const Wording kCodeWords{"bad code batch", "bad code batch", "bad code batch", "bad code batch"};
const Wording kListWords{"bad match list arguments", "bad match list arguments", "bad match list arguments",
                         "bad match list arguments"};
const Wording kKnnWords{"null matcher", "k-NN: P outside 1..max_pairs", "k-NN: null size array",
                        "k-NN: null descriptor array"};
const Wording kGatedWords{"null matcher", "bad gated batch", "bad gated batch", "bad gated batch"};
const Wording kGatedKnnWords{"null matcher", "bad gated batch", "bad gated batch", "k-NN: null descriptor array"};

// What a match entry point asks for.  The entry points fill one and hand it to run().
struct MatchCall {
    Op op;
    const Wording* words;
    Gate gate = Gate::None;
    bool single = false;  // a single-pair entry point: its pair is a one-pair table in the entry point's frame
    bool host = false;    // a _host form: the outputs are the matcher's own buffers (run() fills them in)
    // The pair table: sizes, and the sets as fp16 pointers or (ready) as rows of a caller's code buffer.
    int P = 0;
    const int *nq = nullptr, *nt = nullptr;
    const uint16_t* const* q = nullptr;
    const uint16_t* const* t = nullptr;
    bool ready = false;
    const int8_t* codes = nullptr;
    const int* keys = nullptr;
    const int *qrow0 = nullptr, *qkey0 = nullptr, *trow0 = nullptr, *tkey0 = nullptr;
    // The gate: positions per pair and the call-wide fields; the epipolar geometry is the host's F (single-pair
    // calls, checked here, a kernel argument) or a device table the kernel reads (batched calls).
    bool has_gate = true;  // single-pair calls: the gate record is not null
    const sift_hip_match_positions* pos = nullptr;
    int qstride = 0, tstride = 0;
    float radius = 0.f, max_error = 0.f;
    const float* F = nullptr;
    const void* geometry = nullptr;
    int geometry_stride = 0;
    // The operation's parameters and outputs.
    float ratio = 0.f;
    int ratio_on_squared = 0;
    const sift_hip_match_filter* filter = nullptr;
    int k = 0;
    float max_distance = 0.f;
    int* idx = nullptr;  // top-2: idx2
    float* d2 = nullptr;
    int* match = nullptr;
    sift_hip_dmatch* out = nullptr;
    int* counts = nullptr;
    hipStream_t stream = nullptr;

    bool knn() const { return op == Op::KnnTable || op == Op::KnnList; }
    const char* gate_name() const { return gate == Gate::Epipolar ? "epipolar gate" : "match gate"; }
};

// The pair of a single-pair entry point as a one-pair table (and its gate's positions) on that entry point's stack.
struct OnePair {
    const uint16_t *q, *t;
    int nq, nt;
    sift_hip_match_positions pos;
};

MatchCall fp16_call(Op op, const Wording& w, int P, const uint16_t* const* q, const int* nq, const uint16_t* const* t,
                    const int* nt, void* stream) {
    MatchCall c{op, &w};
    c.P = P, c.q = q, c.nq = nq, c.t = t, c.nt = nt, c.stream = (hipStream_t)stream;
    return c;
}
MatchCall codes_call(Op op, const Wording& w, const int8_t* codes, const int* keys, int P, const int* qrow0,
                     const int* qkey0, const int* nq, const int* trow0, const int* tkey0, const int* nt, void* stream) {
    MatchCall c{op, &w};
    c.ready = true, c.codes = codes, c.keys = keys, c.P = P, c.nq = nq, c.nt = nt;
    c.qrow0 = qrow0, c.qkey0 = qkey0, c.trow0 = trow0, c.tkey0 = tkey0, c.stream = (hipStream_t)stream;
    return c;
}
MatchCall single_call(Op op, const Wording& w, const OnePair& o, void* stream) {
    MatchCall c = fp16_call(op, w, 1, &o.q, &o.nq, &o.t, &o.nt, stream);
    c.single = true;
    return c;
}
void set_gate(MatchCall& c, OnePair& o, const sift_hip_match_gate* g) {
    c.gate = Gate::Window, c.has_gate = g != nullptr;
    if (!g) return;
    o.pos = {g->query_xy, g->train_xy};
    c.pos = &o.pos, c.qstride = g->query_stride, c.tstride = g->train_stride, c.radius = g->radius;
}
void set_gate(MatchCall& c, OnePair& o, const sift_hip_match_epipolar_gate* g) {
    c.gate = Gate::Epipolar, c.has_gate = g != nullptr;
    if (!g) return;
    o.pos = {g->query_xy, g->train_xy};
    c.pos = &o.pos, c.qstride = g->query_stride, c.tstride = g->train_stride, c.radius = g->radius;
    c.max_error = g->max_error, c.F = g->F;
}
// The gate of a batched call: geometry == nullptr and epipolar == false is the window.
void set_gate(MatchCall& c, bool epipolar, const sift_hip_match_positions* pos, int qstride, int tstride, float radius,
              const void* geometry, int geometry_stride, float max_error) {
    c.gate = epipolar ? Gate::Epipolar : Gate::Window;
    c.pos = pos, c.qstride = qstride, c.tstride = tstride, c.radius = radius;
    c.geometry = geometry, c.geometry_stride = geometry_stride, c.max_error = max_error;
}

bool needs_reverse(const sift_hip_match_filter& f) { return f.cross_check || f.ratio_both_ways; }

// --- One checker.  The rules in the order of include/sift_hip.h ("Gated k nearest neighbours", which covers every
// family's): what needs no matcher (k, a NaN max_distance, the gate's fields), the matcher, P and the arrays, the
// pairs' sizes, the pointers of non-empty sets, the outputs.  The first broken rule is reported, in the family's
// wording; nothing is launched or written.
int check(const sift_hip_matcher* m, const MatchCall& c) {
    auto bad = [](const std::string& msg) { return fail(SIFT_HIP_ERR_INVALID, msg); };
    if (c.knn() && (c.k < 1 || c.k > kKnnMax)) return bad("k-NN: k outside 1..SIFT_HIP_KNN_MAX");
    if (c.op == Op::KnnList && std::isnan(c.max_distance)) return bad("k-NN list: max_distance is NaN");
    if (c.gate != Gate::None) {
        const std::string what = c.gate_name();
        if (!c.has_gate) return bad("null " + what);
        if (c.qstride < 2 || c.tstride < 2) return bad(what + ": a position stride below 2 floats");
        if (!(c.radius > 0.f)) return bad(what + ": the radius must be > 0");
    }
    if (c.gate == Gate::Epipolar) {
        if (!(c.max_error > 0.f) || !std::isfinite(c.max_error))
            return bad("epipolar gate: max_error must be > 0 and finite");
        if (c.single) {
            bool zero = true;
            for (int i = 0; i < 9; i++) {
                if (!std::isfinite(c.F[i])) return bad("epipolar gate: a non-finite entry of F");
                zero = zero && c.F[i] == 0.f;
            }
            if (zero) return bad("epipolar gate: F is all zero");
        } else {
            // The nine floats themselves are on the device: the kernel applies the usable-geometry rule to them.
            if (!c.geometry) return bad("epipolar gate: null geometry");
            if (c.geometry_stride < 36 || c.geometry_stride % 4)
                return bad("epipolar gate: geometry_stride_bytes must be >= 36 and a multiple of 4");
        }
    }
    if (!m) return bad(c.words->matcher);
    if (c.P <= 0 || c.P > m->maxP) return bad(c.words->pairs);
    if (!c.nq || !c.nt) return bad(c.words->sizes);
    if (c.gate != Gate::None && !c.pos) return bad("bad gated batch");
    if (c.op == Op::List && !c.filter) return bad("bad match list arguments");
    if (c.ready) {
        if (!c.codes || !c.keys || !c.qrow0 || !c.qkey0 || !c.trow0 || !c.tkey0) return bad("bad code batch");
    } else if (!c.q || !c.t) {
        return bad(c.words->sets);
    }
    const bool rev = c.op == Op::List && needs_reverse(*c.filter);
    for (int p = 0; p < c.P; p++) {
        if (c.nq[p] < 0 || c.nt[p] < 0 || c.nq[p] > m->maxQ || c.nt[p] > m->maxT)
            return bad("pair size exceeds matcher limits");
        if (rev && (c.nt[p] > m->maxQ || c.nq[p] > m->maxT))
            return bad("the reverse pair (roles swapped) exceeds matcher limits");
    }
    for (int p = 0; p < c.P; p++) {
        if (c.ready) {
            if (c.qrow0[p] < 0 || c.trow0[p] < 0 || c.qkey0[p] < 0 || c.tkey0[p] < 0) return bad("negative set row");
        } else if ((c.nq[p] && !c.q[p]) || (c.nt[p] && !c.t[p])) {
            return bad("null descriptor pointer");
        }
        if (c.gate != Gate::None && ((c.nq[p] && !c.pos[p].query_xy) || (c.nt[p] && !c.pos[p].train_xy)))
            return bad(std::string(c.gate_name()) + ": null position pointer");
    }
    if (!c.host && c.op == Op::List && (!c.out || !c.counts)) return bad("bad match list arguments");
    if (!c.host && c.op == Op::KnnList && (!c.out || !c.counts)) return bad("k-NN list: null out or count");
    return SIFT_HIP_OK;
}

// Whether the matching stage of a call has an output row to write; the rule is the family's (include/sift_hip.h).  The
// plain top-2 always launches.  A list of plain or single-pair gated pairs needs a pair with rows on both sides.
// Everything else -- gated batches, every k-NN form, the single-pair gated top-2 -- needs a query row, or with `rev`
// a train row (a query without train rows still gets its -1 / FLT_MAX row).
bool has_output_row(const MatchCall& c, bool rev) {
    if (c.op == Op::Top2 && c.gate == Gate::None) return true;
    const bool both = c.op == Op::List && (c.gate == Gate::None || c.single);
    for (int p = 0; p < c.P; p++)
        if (both ? c.nq[p] > 0 && c.nt[p] > 0 : c.nq[p] > 0 || (rev && c.nt[p] > 0)) return true;
    return false;
}

// --- The matcher's scratch of the list and the k-NN calls, at the first such call (not under stream capture).
struct Alloc {
    void** p;
    size_t bytes;
};
int ensure_scratch(sift_hip_matcher* m, std::initializer_list<Alloc> bufs, const char* what) {
    if (*bufs.begin()->p) return SIFT_HIP_OK;
    HIPCHK(hipSetDevice(m->device));
    for (const Alloc& b : bufs)
        if (hipMalloc(b.p, b.bytes) != hipSuccess) {
            for (const Alloc& f : bufs) {
                if (*f.p) (void)hipFree(*f.p);
                *f.p = nullptr;
            }
            return fail(SIFT_HIP_ERR_NOMEM, what);
        }
    return SIFT_HIP_OK;
}
int ensure_select_scratch(sift_hip_matcher* m) {
    const size_t rows = 2 * (size_t)m->maxP * m->maxQ;
    return ensure_scratch(m,
                          {{(void**)&m->dSelIdx, sizeof(int) * 2 * rows},
                           {(void**)&m->dSelD, sizeof(float) * 2 * rows},
                           {(void**)&m->dList, sizeof(MatchRecord) * (size_t)m->maxQ},
                           {(void**)&m->dCount, sizeof(int) * (size_t)m->maxP}},
                          "match list scratch allocation failed");
}
int ensure_knn_scratch(sift_hip_matcher* m) {
    const size_t rows = (size_t)m->maxP * m->maxQ * kKnnMax;
    return ensure_scratch(m,
                          {{(void**)&m->dKnnLists, sizeof(unsigned long long) * kKnnMax * m->knn_lists()},
                           {(void**)&m->dKnnIdx, sizeof(int) * rows},
                           {(void**)&m->dKnnD, sizeof(float) * rows},
                           {(void**)&m->dKnnRec, sizeof(MatchRecord) * (size_t)m->maxQ * kKnnMax},
                           {(void**)&m->dKnnCount, sizeof(int) * (size_t)m->maxP}},
                          "k-NN scratch allocation failed");
}

// --- The pairs of a call as the launchers take them: the forward pairs [0, P) with their output rows at
// sum_{r<p} nq[r], and -- when a filter needs them -- the reverse pairs [P, 2P) with the roles swapped, output rows at
// sum nq + sum_{r<p} nt[r] (select_lists' layout).  A reverse pair shares its forward pair's geometry record.
struct Pairs {
    GatedPair pair[2 * kMaxMatchPairs];
    int n;
};
void build_pairs(const MatchCall& c, bool rev, Pairs& g) {
    int off = 0;
    for (int p = 0; p < c.P; p++) {
        const MatchPair pr = c.ready ? MatchPair{nullptr, nullptr, c.nq[p], c.nt[p], off, 0, 0, c.qrow0[p], c.trow0[p],
                                                 c.qkey0[p], c.tkey0[p]}
                                     : MatchPair{c.q[p], c.t[p], c.nq[p], c.nt[p], off, 0, 0, 0, 0, 0, 0};
        g.pair[p] = GatedPair{pr, c.pos ? c.pos[p].query_xy : nullptr, c.pos ? c.pos[p].train_xy : nullptr, p, 0};
        off += c.nq[p];
    }
    for (int p = 0; rev && p < c.P; p++) {
        const GatedPair& f = g.pair[p];
        const MatchPair& a = f.pr;
        g.pair[c.P + p] = GatedPair{MatchPair{a.t, a.q, a.nt, a.nq, off, 0, 0, a.trow0, a.qrow0, a.tkrow0, a.qkrow0},
                                    f.txy, f.qxy, p, 1};
        off += a.nt;
    }
    g.n = rev ? 2 * c.P : c.P;
}

// The direction policy: forward and reverse pairs in one pass over 2P pairs when the matcher holds that many (and
// `one_pass`: the launch takes more than one pair), else in two passes of P.  The bytes are the same either way; the
// matcher's scratch is restored when a launch ends, so launches ordered on the stream may share it.
template <class Pass>
int directions(const sift_hip_matcher* m, int P, bool rev, bool one_pass, Pass pass) {
    if (rev && one_pass && 2 * P <= m->maxP) return pass(0, 2 * P);
    if (int rc = pass(0, P)) return rc;
    return rev ? pass(P, P) : SIFT_HIP_OK;
}

// n pairs in launches of at most kMaxGatedPairs (the gated launch records), ordered on the stream.
template <class Launch>
int chunked(const GatedPair* pairs, int n, Launch launch) {
    for (int p0 = 0; p0 < n; p0 += kMaxGatedPairs)
        if (int rc = launch(pairs + p0, std::min(kMaxGatedPairs, n - p0))) return rc;
    return SIFT_HIP_OK;
}

// --- One staging function: what the pairs of a launch read their codes from.
enum class Route {
    Ready,     // a caller's code buffer: no conversion, no flags
    Sidecars,  // one pair of detector buffers with fresh sidecars: q and t are separate code sets, no flags
    Fused,     // one plain pair of foreign buffers: k_match_single converts as it goes (rows laid out, no prep launch)
    Prepared,  // the distinct sets converted once by k_match_prep, with their flags
};
struct Staged {
    CodeSet q, t;
    SetFlags flags;
};

// The sidecar decision: a single pair -- of a plain call, or of a single-pair gated entry point; the batched gated
// forms never -- with sidecars enabled, both sets non-empty and both detector buffers with fresh sidecars.
bool sidecar_route(const sift_hip_matcher* m, const MatchCall& c, Staged* st) {
    if (c.ready || c.P != 1 || !(c.single || c.gate == Gate::None) || !m->sidecars || c.nq[0] <= 0 || c.nt[0] <= 0)
        return false;
    Sidecar sq{}, stt{};
    if (!find_sidecar(c.q[0], c.nq[0], &sq) || !find_sidecar(c.t[0], c.nt[0], &stt)) return false;
    *st = Staged{CodeSet{sq.codes, sq.keys}, CodeSet{stt.codes, stt.keys}, kNoFlags};
    return true;
}

// Checked pairs in, their set slots and rows filled in, and the code sets and flags to launch with out.  Ready and
// Sidecars: st is the call's already.  Otherwise the distinct sets by pointer (a set used by several pairs is
// prepared once, n = the largest use) are laid out in order of first appearance, get a new epoch, and -- Prepared --
// are converted.
int stage(sift_hip_matcher* m, const MatchCall& c, Route route, GatedPair* pairs, int n, Staged* st) {
    if (route == Route::Ready) *st = Staged{CodeSet{c.codes, c.keys}, CodeSet{c.codes, c.keys}, kNoFlags};
    if (route == Route::Ready || route == Route::Sidecars) return SIFT_HIP_OK;
    MatchSets sets{};
    auto set_of = [&](const uint16_t* ptr, int rows) {
        for (int s = 0; s < sets.nsets; s++)
            if (sets.set[s].src == ptr) {
                sets.set[s].n = std::max(sets.set[s].n, rows);
                return s;
            }
        sets.set[sets.nsets] = MatchSet{ptr, rows, 0};
        return sets.nsets++;
    };
    for (int p = 0; p < n; p++) {
        MatchPair& pr = pairs[p].pr;
        pr.qset = set_of(pr.q, pr.nq);
        pr.tset = set_of(pr.t, pr.nt);
    }
    long row = 0;
    for (int s = 0; s < sets.nsets; s++) {
        sets.set[s].row0 = (int)row;
        row += sets.set[s].n;
        sets.maxn = std::max(sets.maxn, sets.set[s].n);
    }
    if (row > m->codeRows) return fail(SIFT_HIP_ERR_INVALID, "descriptor sets exceed the matcher's code buffer");
    for (int p = 0; p < n; p++) {
        MatchPair& pr = pairs[p].pr;
        pr.qrow0 = pr.qkrow0 = sets.set[pr.qset].row0;
        pr.trow0 = pr.tkrow0 = sets.set[pr.tset].row0;
    }
    const CodeSet set{m->dCodes, m->dRowKeys};
    *st = Staged{set, set, m->next_epoch()};
    if (route == Route::Prepared) {
        launch_match_prep(sets, m->dCodes, m->dRowKeys, st->flags, c.stream);
        HIPCHK(hipGetLastError());
    }
    return SIFT_HIP_OK;
}

// --- The launches.
struct Shape {
    int maxq = 1, maxt = 1;
    bool queries = false;
    Shape(const GatedPair* pairs, int n) {
        for (int p = 0; p < n; p++) {
            maxq = std::max(maxq, pairs[p].pr.nq);
            maxt = std::max(maxt, pairs[p].pr.nt);
            queries = queries || pairs[p].pr.nq > 0;
        }
    }
};

// The plain launch records take a pass relative to its first output row: the pairs' offsets from it, the outputs at it.
MatchBatch batch_of(const GatedPair* pairs, int n, int base) {
    MatchBatch b{};
    b.P = n;
    for (int p = 0; p < n; p++) {
        b.pair[p] = pairs[p].pr;
        b.pair[p].out_off -= base;
    }
    return b;
}
MatchOut out_at(const MatchOut& o, int base) {
    return MatchOut{o.ratio, o.ratio_on_squared, o.idx2 ? o.idx2 + 2 * (size_t)base : nullptr,
                    o.d2 ? o.d2 + 2 * (size_t)base : nullptr, o.match ? o.match + base : nullptr};
}

// One pair on code sets of its own (k_match_direct, k_match_guided, k_match_epipolar): the sets start at the pair's
// rows (sidecars: row 0) and the outputs at its row; a reverse pair reads the sets, the strides and F swapped.
void launch_one(const sift_hip_matcher* m, const MatchCall& c, const GatedPair& g, const Staged& st, const MatchOut& out) {
    const MatchPair& a = g.pr;
    const MatchPair pr{a.q, a.t, a.nq, a.nt, 0, a.qset, a.tset, 0, 0, 0, 0};
    const CodeSet &qs = g.swapped ? st.t : st.q, &ts = g.swapped ? st.q : st.t;
    const CodeSet qc{qs.codes + (size_t)a.qrow0 * 128, qs.keys + a.qkrow0};
    const CodeSet tc{ts.codes + (size_t)a.trow0 * 128, ts.keys + a.tkrow0};
    const int qstride = g.swapped ? c.tstride : c.qstride, tstride = g.swapped ? c.qstride : c.tstride;
    const MatchOut o = out_at(out, a.out_off);
    if (c.gate == Gate::Epipolar) {
        // e2 = max_error^2 is formed here, one float32 product.
        EpipolarGate eg{g.qxy, g.txy, qstride, tstride, c.radius, c.max_error * c.max_error, {}};
        for (int r = 0; r < 3; r++)
            for (int col = 0; col < 3; col++) eg.F[3 * r + col] = c.F[g.swapped ? 3 * col + r : 3 * r + col];
        launch_match_pair(pr, eg, qc, tc, st.flags, m->scratch(), o, c.stream);
    } else {
        const MatchGate mg{g.qxy, g.txy, qstride, tstride, c.radius};
        launch_match_pair(pr, c.gate == Gate::Window ? &mg : nullptr, qc, tc, st.flags, m->scratch(), o, c.stream);
    }
}

// A pass of the plain top-2 (sift_hip_match_batched / _codes_batched on n pairs): staged by itself, since a pass of
// one pair goes through its sidecars or the fused kernel.  Ready codes keep the batched kernel's plan for one pair.
int plain_pass(sift_hip_matcher* m, const MatchCall& c, bool direct, Staged& st, GatedPair* pairs, int n,
               const MatchOut& out) {
    const Route route = c.ready ? Route::Ready : direct ? Route::Sidecars : n == 1 ? Route::Fused : Route::Prepared;
    if (int rc = stage(m, c, route, pairs, n, &st)) return rc;
    const int base = pairs[0].pr.out_off;
    const Shape sh(pairs, n);
    if (route == Route::Sidecars)
        launch_one(m, c, pairs[0], st, out);
    else if (route == Route::Fused) {
        MatchPair pr = pairs[0].pr;
        pr.out_off = 0;
        launch_match_single(pr, match_plan(sh.maxq, sh.maxt, 1).S, m->scratch(), out_at(out, base), c.stream);
    } else
        launch_match_codes(batch_of(pairs, n, base), match_plan(sh.maxq, sh.maxt, c.ready ? std::max(n, 2) : n).S, st.q,
                           st.flags, m->scratch(), out_at(out, base), c.stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

// What is uniform over a gated call as the launchers take it; e2 = max_error^2 is formed here, one float32 product.
GatedCall gated_call(const MatchCall& c) {
    const bool epi = c.gate == Gate::Epipolar;
    return GatedCall{c.qstride, c.tstride, c.radius, epi ? c.max_error * c.max_error : 0.f, epi ? c.geometry : nullptr,
                     epi ? c.geometry_stride : 0};
}

// The plan's splits of a k-NN launch, lowered to what the list scratch holds.
int knn_splits(const sift_hip_matcher* m, const Shape& sh, int P) {
    const size_t fit = m->knn_lists() / ((size_t)P * sh.maxq);  // >= 2: P <= maxP, maxq <= maxQ
    return (int)std::min<size_t>(match_knn_splits(sh.maxq, sh.maxt, P), fit);
}

// The top-2 of a call's pairs (forward, and with `rev` reverse) into `out`.
int top2(sift_hip_matcher* m, const MatchCall& c, bool rev, const MatchOut& out) {
    Pairs g;
    build_pairs(c, rev, g);
    Staged st{};
    const bool direct = sidecar_route(m, c, &st);
    if (c.gate == Gate::None)
        return directions(m, c.P, rev, !direct,
                          [&](int p0, int n) { return plain_pass(m, c, direct, st, g.pair + p0, n, out); });
    // Under a gate the call is staged once; a single-pair entry point launches pair by pair, a batch in chunks.
    if (int rc = stage(m, c, c.ready ? Route::Ready : direct ? Route::Sidecars : Route::Prepared, g.pair, g.n, &st))
        return rc;
    const GatedCall call = gated_call(c);
    return directions(m, c.P, rev, !c.single, [&](int p0, int n) {
        if (c.single) {
            launch_one(m, c, g.pair[p0], st, out);
            HIPCHK(hipGetLastError());
            return SIFT_HIP_OK;
        }
        return chunked(g.pair + p0, n, [&](const GatedPair* pairs, int np) {
            GatedBatch b{};
            b.P = np;
            std::copy(pairs, pairs + np, b.pair);
            launch_match_gated(b, call, st.q, st.flags, m->scratch(), out, c.stream);
            HIPCHK(hipGetLastError());
            return SIFT_HIP_OK;
        });
    });
}

// The k-NN table of a call's pairs into idx / d2, pair p at row sum_{r<p} nq[r]: one launch of the plain kernel, or
// under a gate launches of at most kMaxGatedPairs pairs, each with the splits of its own pairs.
int knn_table(sift_hip_matcher* m, const MatchCall& c, int* idx, float* d2) {
    Pairs g;
    build_pairs(c, false, g);
    Staged st{};
    const bool direct = sidecar_route(m, c, &st);
    if (int rc = stage(m, c, c.ready ? Route::Ready : direct ? Route::Sidecars : Route::Prepared, g.pair, g.n, &st))
        return rc;
    if (c.gate == Gate::None) {
        const Shape sh(g.pair, g.n);
        launch_match_knn(batch_of(g.pair, g.n, 0), knn_splits(m, sh, g.n), c.k, st.q, st.t, st.flags,
                         KnnScratch{m->dKnnLists, m->dDone, sh.maxq, m->sentinel()}, idx, d2, c.stream);
        HIPCHK(hipGetLastError());
        return SIFT_HIP_OK;
    }
    return chunked(g.pair, g.n, [&](const GatedPair* pairs, int np) {
        const Shape sh(pairs, np);
        if (!sh.queries) return SIFT_HIP_OK;
        KnnGatedBatch b{};
        b.P = np;
        b.call = gated_call(c);
        if (c.F) std::copy(c.F, c.F + 9, b.F);  // the single-pair epipolar call: the host's F is a kernel argument
        for (int i = 0; i < np; i++)
            b.pair[i] = pairs[i].pr, b.qxy[i] = pairs[i].qxy, b.txy[i] = pairs[i].txy, b.geom[i] = pairs[i].geom;
        launch_match_knn_gated(b, c.gate == Gate::Epipolar, knn_splits(m, sh, np), c.k, st.q, st.t, st.flags,
                               KnnScratch{m->dKnnLists, m->dDone, sh.maxq, m->sentinel()}, idx, d2, c.stream);
        HIPCHK(hipGetLastError());
        return SIFT_HIP_OK;
    });
}

// Filter and compact the top-2 arrays in the select scratch: forward pair p at row sum_{r<p} nq[r], reverse pair p at
// row sum nq + sum_{r<p} nt[r].
int select_lists(sift_hip_matcher* m, const MatchCall& c) {
    SelectBatch sb{};
    int totq = 0;
    for (int p = 0; p < c.P; p++) totq += c.nq[p];
    int fwd = 0, rev = totq;
    for (int p = 0; p < c.P; p++) {
        // a pair without train rows keeps nothing (its top-2 rows hold no entry)
        sb.pair[p] = SelectPair{c.nt[p] > 0 ? c.nq[p] : 0, c.nt[p], fwd, rev, fwd};
        fwd += c.nq[p];
        rev += c.nt[p];
    }
    const sift_hip_match_filter& f = *c.filter;
    launch_match_select(sb, c.P, m->dSelIdx, m->dSelD,
                        MatchFilter{f.ratio, f.ratio_on_squared, f.ratio_both_ways, f.max_distance, f.cross_check},
                        reinterpret_cast<MatchRecord*>(c.out), c.counts, c.stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

// The list of the matcher's k-NN table (pair p at row sum_{r<p} nq[r]): pair p's records from row k sum_{r<p} nq[r].
int knn_select(sift_hip_matcher* m, const MatchCall& c) {
    SelectBatch sb{};
    int row = 0;
    for (int p = 0; p < c.P; p++) {
        sb.pair[p] = SelectPair{c.nq[p], 0, row, 0, c.k * row};
        row += c.nq[p];
    }
    launch_knn_select(sb, c.P, c.k, m->dKnnIdx, m->dKnnD, c.max_distance, reinterpret_cast<MatchRecord*>(c.out),
                      c.counts, c.stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

// --- One host path: check, the matching stage where the call has an output row, then a list's selection.
int run(sift_hip_matcher* m, MatchCall c) {
    if (int rc = check(m, c)) return rc;
    const bool rev = c.op == Op::List && needs_reverse(*c.filter), rows = has_output_row(c, rev);
    // The operation's scratch, at the matcher's first such call; a table into the caller's buffers needs it to launch.
    if (c.op == Op::List)
        if (int rc = ensure_select_scratch(m)) return rc;
    if (c.op == Op::KnnList || (c.op == Op::KnnTable && (c.host || rows)))
        if (int rc = ensure_knn_scratch(m)) return rc;
    if (c.op == Op::KnnList || (c.op == Op::KnnTable && c.host)) c.idx = m->dKnnIdx, c.d2 = m->dKnnD;
    if (c.host) {
        c.match = m->dMatch;
        c.out = reinterpret_cast<sift_hip_dmatch*>(c.op == Op::List ? m->dList : m->dKnnRec);
        c.counts = c.op == Op::List ? m->dCount : m->dKnnCount;
    }
    if (rows) {
        HIPCHK(hipSetDevice(m->device));
        if (c.knn()) {
            if (int rc = knn_table(m, c, c.idx, c.d2)) return rc;
        } else {
            const MatchOut out = c.op == Op::List ? MatchOut{0.f, 0, m->dSelIdx, m->dSelD, nullptr}
                                                  : MatchOut{c.ratio, c.ratio_on_squared, c.idx, c.d2, c.match};
            if (int rc = top2(m, c, rev, out)) return rc;
        }
    }
    if (c.op == Op::Top2 || c.op == Op::KnnTable) return SIFT_HIP_OK;
    HIPCHK(hipSetDevice(m->device));
    return c.op == Op::List ? select_lists(m, c) : knn_select(m, c);
}

// The _host forms: run into the matcher's own buffers, synchronously, then one read-back each for the lists (the
// count, then min(count, cap) records) and the k-NN tables.  The host outputs are judged first (the count is zeroed
// before anything else can refuse); the plain list call words a null matcher or filter with them.
int run_list_host(sift_hip_matcher* m, MatchCall c, sift_hip_dmatch* out_host, int cap, int* count) {
    const bool list = c.op == Op::List;
    if ((list && (!c.filter || (!m && c.gate == Gate::None))) || !count || cap < 0 || (cap > 0 && !out_host))
        return fail(SIFT_HIP_ERR_INVALID, list ? "null argument" : "k-NN list: null out or count");
    *count = 0;
    c.host = true;
    if (int rc = run(m, c)) return rc;
    HIPCHK(hipMemcpy(count, list ? m->dCount : m->dKnnCount, sizeof(int), hipMemcpyDeviceToHost));
    const int n = std::min(*count, cap);
    if (n > 0)
        HIPCHK(hipMemcpy(out_host, list ? m->dList : m->dKnnRec, sizeof(sift_hip_dmatch) * (size_t)n,
                         hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}
int run_knn_host(sift_hip_matcher* m, MatchCall c, int* idx_host, float* d2_host) {
    c.host = true;
    if (int rc = run(m, c)) return rc;
    const size_t n = (size_t)c.nq[0] * c.k;
    if (n && idx_host) HIPCHK(hipMemcpy(idx_host, m->dKnnIdx, sizeof(int) * n, hipMemcpyDeviceToHost));
    if (n && d2_host) HIPCHK(hipMemcpy(d2_host, m->dKnnD, sizeof(float) * n, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

// The call records of the entry families.
MatchCall top2_call(MatchCall c, float ratio, int ratio_on_squared, int* idx2, float* d2, int* match) {
    c.ratio = ratio, c.ratio_on_squared = ratio_on_squared, c.idx = idx2, c.d2 = d2, c.match = match;
    return c;
}
MatchCall list_call(MatchCall c, const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* counts) {
    c.filter = filter, c.out = out, c.counts = counts;
    return c;
}
MatchCall knn_call(MatchCall c, int k, int* idx, float* d2) {
    c.k = k, c.idx = idx, c.d2 = d2;
    return c;
}
MatchCall knn_list_call(MatchCall c, int k, float max_distance, sift_hip_dmatch* out, int* counts) {
    c.k = k, c.max_distance = max_distance, c.out = out, c.counts = counts;
    return c;
}
template <class G>
MatchCall gated_single(Op op, OnePair& o, const G* gate, void* stream) {
    MatchCall c = single_call(op, kGatedWords, o, stream);
    set_gate(c, o, gate);
    return c;
}
MatchCall gated_batch(Op op, bool epipolar, int P, const uint16_t* const* q, const int* nq, const uint16_t* const* t,
                      const int* nt, const sift_hip_match_positions* pos, int qstride, int tstride, float radius,
                      const void* geometry, int geometry_stride, float max_error, void* stream) {
    MatchCall c = fp16_call(op, op == Op::KnnTable || op == Op::KnnList ? kGatedKnnWords : kGatedWords, P, q, nq, t, nt,
                            stream);
    set_gate(c, epipolar, pos, qstride, tstride, radius, geometry, geometry_stride, max_error);
    return c;
}

}  // namespace

extern "C" {

int sift_hip_matcher_create(int device, int max_query, int max_train, int max_pairs, sift_hip_matcher_t* out) {
    if (!out || max_query <= 0 || max_train <= 0 || max_pairs <= 0 || max_pairs > kMaxMatchPairs)
        return fail(SIFT_HIP_ERR_INVALID, "bad matcher limits");
    *out = nullptr;
    auto* m = new sift_hip_matcher();
    if (device < 0) {
        if (hipGetDevice(&m->device) != hipSuccess) m->device = 0;
    } else {
        m->device = device;
    }
    m->maxQ = max_query;
    m->maxT = max_train;
    m->maxP = max_pairs;
    // Distinct sets of a call: at most 2 per pair, each at most max(maxQ, maxT) rows.
    m->codeRows = 2L * max_pairs * std::max(max_query, max_train);
    const size_t nkeys = 2 * (size_t)max_pairs * max_query;
    const size_t nblk = (size_t)max_pairs * ((max_query + kMatchQB - 1) / kMatchQB);
    if (hipSetDevice(m->device) != hipSuccess ||
        hipMalloc((void**)&m->dKeys, sizeof(unsigned long long) * nkeys) != hipSuccess ||
        hipMalloc((void**)&m->dDone, sizeof(unsigned) * nblk) != hipSuccess ||
        hipMalloc((void**)&m->dMatch, sizeof(int) * (size_t)max_pairs * max_query) != hipSuccess ||
        hipMalloc((void**)&m->dCodes, (size_t)(m->codeRows + 1) * 128) != hipSuccess ||
        hipMalloc((void**)&m->dRowKeys, sizeof(int) * (size_t)(m->codeRows + 1)) != hipSuccess ||
        hipMemset((void*)m->sentinel().codes, 0, 128) != hipSuccess ||
        hipMemcpy((void*)m->sentinel().keys, &kMatchPadKey, sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc((void**)&m->dFlags, sizeof(unsigned) * 2 * kMaxMatchPairs) != hipSuccess ||
        hipMemset(m->dKeys, 0xff, sizeof(unsigned long long) * nkeys) != hipSuccess ||
        hipMemset(m->dDone, 0, sizeof(unsigned) * nblk) != hipSuccess ||
        hipMemset(m->dFlags, 0, sizeof(unsigned) * 2 * kMaxMatchPairs) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        delete m;
        return fail(SIFT_HIP_ERR_NOMEM, "matcher allocation failed");
    }
    *out = m;
    return SIFT_HIP_OK;
}

int sift_hip_matcher_set_sidecars(sift_hip_matcher_t m, int enable) {
    if (!m) return fail(SIFT_HIP_ERR_INVALID, "null matcher");
    m->sidecars = enable != 0;
    return SIFT_HIP_OK;
}

int sift_hip_matcher_destroy(sift_hip_matcher_t m) {
    delete m;
    return SIFT_HIP_OK;
}

int sift_hip_descriptors_written(const uint16_t* desc) {
    if (!desc) return fail(SIFT_HIP_ERR_INVALID, "null descriptor buffer");
    (void)sidecar_written(desc);  // a foreign buffer has no sidecar: nothing to drop
    return SIFT_HIP_OK;
}

int sift_hip_match_plan(int max_query, int max_train, int pairs, int* splits, int* waves) {
    if (max_query < 0 || max_train < 0 || pairs < 1 || !splits) return fail(SIFT_HIP_ERR_INVALID, "bad match shape");
    const MatchPlan pl = match_plan(max_query, max_train, pairs);
    *splits = pl.S;
    if (waves) *waves = pl.nw;
    return SIFT_HIP_OK;
}

int sift_hip_match_guided_plan(int nq, int nt, int* splits) {
    if (nq < 0 || nt < 0 || !splits) return fail(SIFT_HIP_ERR_INVALID, "bad match shape");
    *splits = match_direct_splits(nq, nt);
    return SIFT_HIP_OK;
}

int sift_hip_match_knn_plan(int nq, int nt, int pairs, int k, int* splits) {
    if (nq < 0 || nt < 0 || pairs < 1 || k < 1 || k > kKnnMax || !splits)
        return fail(SIFT_HIP_ERR_INVALID, "bad k-NN shape");
    *splits = match_knn_splits(nq, nt, pairs);
    return SIFT_HIP_OK;
}

void sift_hip_default_match_filter(sift_hip_match_filter* f) {
    if (!f) return;
    f->ratio = 0.8f;
    f->ratio_on_squared = 0;
    f->ratio_both_ways = 0;
    f->max_distance = 0.f;
    f->cross_check = 1;
}

// --- Top-2 ----------------------------------------------------------------------
int sift_hip_match_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                           const uint16_t* const* t, const int* nt, float ratio, int ratio_on_squared, int* idx2,
                           float* d2, int* match, void* stream) {
    return run(m, top2_call(fp16_call(Op::Top2, kBatchWords, P, q, nq, t, nt, stream), ratio, ratio_on_squared, idx2, d2,
                            match));
}

int sift_hip_match_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P, const int* qrow0,
                                 const int* qkey0, const int* nq, const int* trow0, const int* tkey0, const int* nt,
                                 float ratio, int ratio_on_squared, int* idx2, float* d2, int* match, void* stream) {
    return run(m, top2_call(codes_call(Op::Top2, kCodeWords, codes, keys, P, qrow0, qkey0, nq, trow0, tkey0, nt, stream),
                            ratio, ratio_on_squared, idx2, d2, match));
}

int sift_hip_match_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, float ratio,
                          int ratio_on_squared, int* idx2, float* d2, int* match, void* stream) {
    const OnePair o{q, t, nq, nt, {}};
    return run(m, top2_call(single_call(Op::Top2, kBatchWords, o, stream), ratio, ratio_on_squared, idx2, d2, match));
}

int sift_hip_match_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, float ratio,
                        int ratio_on_squared, int* out) {
    if (!m || !out) return fail(SIFT_HIP_ERR_INVALID, "null argument");
    if (nq <= 0) return SIFT_HIP_OK;
    const OnePair o{q, t, nq, nt, {}};
    MatchCall c = top2_call(single_call(Op::Top2, kBatchWords, o, nullptr), ratio, ratio_on_squared, nullptr, nullptr,
                            nullptr);
    c.host = true;
    if (int rc = run(m, c)) return rc;
    HIPCHK(hipMemcpy(out, m->dMatch, sizeof(int) * nq, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

int sift_hip_match_guided_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                 const sift_hip_match_gate* gate, float ratio, int ratio_on_squared, int* idx2,
                                 float* d2, int* match, void* stream) {
    OnePair o{q, t, nq, nt, {}};
    return run(m, top2_call(gated_single(Op::Top2, o, gate, stream), ratio, ratio_on_squared, idx2, d2, match));
}

int sift_hip_match_epipolar_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                   const sift_hip_match_epipolar_gate* gate, float ratio, int ratio_on_squared,
                                   int* idx2, float* d2, int* match, void* stream) {
    OnePair o{q, t, nq, nt, {}};
    return run(m, top2_call(gated_single(Op::Top2, o, gate, stream), ratio, ratio_on_squared, idx2, d2, match));
}

int sift_hip_match_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                  const uint16_t* const* t, const int* nt, const sift_hip_match_positions* positions,
                                  int query_stride, int train_stride, float radius, float ratio, int ratio_on_squared,
                                  int* idx2, float* d2, int* match, void* stream) {
    return run(m, top2_call(gated_batch(Op::Top2, false, P, q, nq, t, nt, positions, query_stride, train_stride, radius,
                                        nullptr, 0, 0.f, stream),
                            ratio, ratio_on_squared, idx2, d2, match));
}

int sift_hip_match_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                    const uint16_t* const* t, const int* nt, const sift_hip_match_positions* positions,
                                    int query_stride, int train_stride, float radius, const void* geometry,
                                    int geometry_stride_bytes, float max_error, float ratio, int ratio_on_squared,
                                    int* idx2, float* d2, int* match, void* stream) {
    return run(m, top2_call(gated_batch(Op::Top2, true, P, q, nq, t, nt, positions, query_stride, train_stride, radius,
                                        geometry, geometry_stride_bytes, max_error, stream),
                            ratio, ratio_on_squared, idx2, d2, match));
}

// --- Match lists ----------------------------------------------------------------
int sift_hip_match_list_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                const uint16_t* const* t, const int* nt, const sift_hip_match_filter* filter,
                                sift_hip_dmatch* out, int* counts, void* stream) {
    return run(m, list_call(fp16_call(Op::List, kListWords, P, q, nq, t, nt, stream), filter, out, counts));
}

int sift_hip_match_list_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                      const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                      const int* tkey0, const int* nt, const sift_hip_match_filter* filter,
                                      sift_hip_dmatch* out, int* counts, void* stream) {
    return run(m, list_call(codes_call(Op::List, kListWords, codes, keys, P, qrow0, qkey0, nq, trow0, tkey0, nt, stream),
                            filter, out, counts));
}

int sift_hip_match_list_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                               const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* count, void* stream) {
    const OnePair o{q, t, nq, nt, {}};
    return run(m, list_call(single_call(Op::List, kListWords, o, stream), filter, out, count));
}

int sift_hip_match_list_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                             const sift_hip_match_filter* filter, sift_hip_dmatch* out_host, int cap, int* count) {
    const OnePair o{q, t, nq, nt, {}};
    return run_list_host(m, list_call(single_call(Op::List, kListWords, o, nullptr), filter, nullptr, nullptr), out_host,
                         cap, count);
}

int sift_hip_match_list_guided_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                      const sift_hip_match_gate* gate, const sift_hip_match_filter* filter,
                                      sift_hip_dmatch* out, int* count, void* stream) {
    OnePair o{q, t, nq, nt, {}};
    return run(m, list_call(gated_single(Op::List, o, gate, stream), filter, out, count));
}

int sift_hip_match_list_guided_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                    const sift_hip_match_gate* gate, const sift_hip_match_filter* filter,
                                    sift_hip_dmatch* out_host, int cap, int* count) {
    OnePair o{q, t, nq, nt, {}};
    return run_list_host(m, list_call(gated_single(Op::List, o, gate, nullptr), filter, nullptr, nullptr), out_host, cap,
                         count);
}

int sift_hip_match_list_epipolar_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                        const sift_hip_match_epipolar_gate* gate, const sift_hip_match_filter* filter,
                                        sift_hip_dmatch* out, int* count, void* stream) {
    OnePair o{q, t, nq, nt, {}};
    return run(m, list_call(gated_single(Op::List, o, gate, stream), filter, out, count));
}

int sift_hip_match_list_epipolar_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                      const sift_hip_match_epipolar_gate* gate, const sift_hip_match_filter* filter,
                                      sift_hip_dmatch* out_host, int cap, int* count) {
    OnePair o{q, t, nq, nt, {}};
    return run_list_host(m, list_call(gated_single(Op::List, o, gate, nullptr), filter, nullptr, nullptr), out_host, cap,
                         count);
}

int sift_hip_match_list_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                       const uint16_t* const* t, const int* nt,
                                       const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                       float radius, const sift_hip_match_filter* filter, sift_hip_dmatch* out,
                                       int* counts, void* stream) {
    return run(m, list_call(gated_batch(Op::List, false, P, q, nq, t, nt, positions, query_stride, train_stride, radius,
                                        nullptr, 0, 0.f, stream),
                            filter, out, counts));
}

int sift_hip_match_list_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                         const uint16_t* const* t, const int* nt,
                                         const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                         float radius, const void* geometry, int geometry_stride_bytes, float max_error,
                                         const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* counts,
                                         void* stream) {
    return run(m, list_call(gated_batch(Op::List, true, P, q, nq, t, nt, positions, query_stride, train_stride, radius,
                                        geometry, geometry_stride_bytes, max_error, stream),
                            filter, out, counts));
}

int sift_hip_match_list_guided_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                             const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                             const int* tkey0, const int* nt,
                                             const sift_hip_match_positions* positions, int query_stride,
                                             int train_stride, float radius, const sift_hip_match_filter* filter,
                                             sift_hip_dmatch* out, int* counts, void* stream) {
    MatchCall c = codes_call(Op::List, kGatedWords, codes, keys, P, qrow0, qkey0, nq, trow0, tkey0, nt, stream);
    set_gate(c, false, positions, query_stride, train_stride, radius, nullptr, 0, 0.f);
    return run(m, list_call(c, filter, out, counts));
}

int sift_hip_match_list_epipolar_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                               const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                               const int* tkey0, const int* nt,
                                               const sift_hip_match_positions* positions, int query_stride,
                                               int train_stride, float radius, const void* geometry,
                                               int geometry_stride_bytes, float max_error,
                                               const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* counts,
                                               void* stream) {
    MatchCall c = codes_call(Op::List, kGatedWords, codes, keys, P, qrow0, qkey0, nq, trow0, tkey0, nt, stream);
    set_gate(c, true, positions, query_stride, train_stride, radius, geometry, geometry_stride_bytes, max_error);
    return run(m, list_call(c, filter, out, counts));
}

// --- k nearest neighbours and capped radius lists ----------------------------------
int sift_hip_match_knn_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                               const uint16_t* const* t, const int* nt, int k, int* idx, float* d2, void* stream) {
    return run(m, knn_call(fp16_call(Op::KnnTable, kKnnWords, P, q, nq, t, nt, stream), k, idx, d2));
}

int sift_hip_match_knn_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, int k,
                              int* idx, float* d2, void* stream) {
    const OnePair o{q, t, nq, nt, {}};
    return run(m, knn_call(single_call(Op::KnnTable, kKnnWords, o, stream), k, idx, d2));
}

int sift_hip_match_knn_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                     const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                     const int* tkey0, const int* nt, int k, int* idx, float* d2, void* stream) {
    return run(m, knn_call(codes_call(Op::KnnTable, kKnnWords, codes, keys, P, qrow0, qkey0, nq, trow0, tkey0, nt, stream),
                           k, idx, d2));
}

int sift_hip_match_knn_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, int k,
                            int* idx_host, float* d2_host) {
    const OnePair o{q, t, nq, nt, {}};
    return run_knn_host(m, knn_call(single_call(Op::KnnTable, kKnnWords, o, nullptr), k, nullptr, nullptr), idx_host,
                        d2_host);
}

int sift_hip_match_knn_list_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                    const uint16_t* const* t, const int* nt, int k, float max_distance,
                                    sift_hip_dmatch* out, int* counts, void* stream) {
    return run(m, knn_list_call(fp16_call(Op::KnnList, kKnnWords, P, q, nq, t, nt, stream), k, max_distance, out, counts));
}

int sift_hip_match_knn_list_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, int k,
                                   float max_distance, sift_hip_dmatch* out, int* count, void* stream) {
    const OnePair o{q, t, nq, nt, {}};
    return run(m, knn_list_call(single_call(Op::KnnList, kKnnWords, o, stream), k, max_distance, out, count));
}

int sift_hip_match_knn_list_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, int k,
                                 float max_distance, sift_hip_dmatch* out_host, int cap, int* count) {
    const OnePair o{q, t, nq, nt, {}};
    return run_list_host(m, knn_list_call(single_call(Op::KnnList, kKnnWords, o, nullptr), k, max_distance, nullptr, nullptr),
                         out_host, cap, count);
}

// --- Gated k nearest neighbours ---------------------------------------------------
int sift_hip_match_knn_guided_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                     const sift_hip_match_gate* gate, int k, int* idx, float* d2, void* stream) {
    OnePair o{q, t, nq, nt, {}};
    return run(m, knn_call(gated_single(Op::KnnTable, o, gate, stream), k, idx, d2));
}
int sift_hip_match_knn_epipolar_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                       const sift_hip_match_epipolar_gate* gate, int k, int* idx, float* d2,
                                       void* stream) {
    OnePair o{q, t, nq, nt, {}};
    return run(m, knn_call(gated_single(Op::KnnTable, o, gate, stream), k, idx, d2));
}
int sift_hip_match_knn_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                      const uint16_t* const* t, const int* nt, const sift_hip_match_positions* positions,
                                      int query_stride, int train_stride, float radius, int k, int* idx, float* d2,
                                      void* stream) {
    return run(m, knn_call(gated_batch(Op::KnnTable, false, P, q, nq, t, nt, positions, query_stride, train_stride, radius,
                                       nullptr, 0, 0.f, stream),
                           k, idx, d2));
}
int sift_hip_match_knn_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                        const uint16_t* const* t, const int* nt,
                                        const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                        float radius, const void* geometry, int geometry_stride_bytes, float max_error,
                                        int k, int* idx, float* d2, void* stream) {
    return run(m, knn_call(gated_batch(Op::KnnTable, true, P, q, nq, t, nt, positions, query_stride, train_stride, radius,
                                       geometry, geometry_stride_bytes, max_error, stream),
                           k, idx, d2));
}
int sift_hip_match_knn_list_guided_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                          const sift_hip_match_gate* gate, int k, float max_distance,
                                          sift_hip_dmatch* out, int* count, void* stream) {
    OnePair o{q, t, nq, nt, {}};
    return run(m, knn_list_call(gated_single(Op::KnnList, o, gate, stream), k, max_distance, out, count));
}
int sift_hip_match_knn_list_epipolar_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                            const sift_hip_match_epipolar_gate* gate, int k, float max_distance,
                                            sift_hip_dmatch* out, int* count, void* stream) {
    OnePair o{q, t, nq, nt, {}};
    return run(m, knn_list_call(gated_single(Op::KnnList, o, gate, stream), k, max_distance, out, count));
}
int sift_hip_match_knn_list_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                           const uint16_t* const* t, const int* nt,
                                           const sift_hip_match_positions* positions, int query_stride,
                                           int train_stride, float radius, int k, float max_distance,
                                           sift_hip_dmatch* out, int* counts, void* stream) {
    return run(m, knn_list_call(gated_batch(Op::KnnList, false, P, q, nq, t, nt, positions, query_stride, train_stride,
                                            radius, nullptr, 0, 0.f, stream),
                                k, max_distance, out, counts));
}
int sift_hip_match_knn_list_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                             const uint16_t* const* t, const int* nt,
                                             const sift_hip_match_positions* positions, int query_stride,
                                             int train_stride, float radius, const void* geometry,
                                             int geometry_stride_bytes, float max_error, int k, float max_distance,
                                             sift_hip_dmatch* out, int* counts, void* stream) {
    return run(m, knn_list_call(gated_batch(Op::KnnList, true, P, q, nq, t, nt, positions, query_stride, train_stride,
                                            radius, geometry, geometry_stride_bytes, max_error, stream),
                                k, max_distance, out, counts));
}
int sift_hip_match_knn_guided_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                   const sift_hip_match_gate* gate, int k, int* idx_host, float* d2_host) {
    OnePair o{q, t, nq, nt, {}};
    return run_knn_host(m, knn_call(gated_single(Op::KnnTable, o, gate, nullptr), k, nullptr, nullptr), idx_host, d2_host);
}
int sift_hip_match_knn_epipolar_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                     const sift_hip_match_epipolar_gate* gate, int k, int* idx_host, float* d2_host) {
    OnePair o{q, t, nq, nt, {}};
    return run_knn_host(m, knn_call(gated_single(Op::KnnTable, o, gate, nullptr), k, nullptr, nullptr), idx_host, d2_host);
}
int sift_hip_match_knn_list_guided_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                        const sift_hip_match_gate* gate, int k, float max_distance,
                                        sift_hip_dmatch* out_host, int cap, int* count) {
    OnePair o{q, t, nq, nt, {}};
    return run_list_host(m, knn_list_call(gated_single(Op::KnnList, o, gate, nullptr), k, max_distance, nullptr, nullptr),
                         out_host, cap, count);
}
int sift_hip_match_knn_list_epipolar_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                          const sift_hip_match_epipolar_gate* gate, int k, float max_distance,
                                          sift_hip_dmatch* out_host, int cap, int* count) {
    OnePair o{q, t, nq, nt, {}};
    return run_list_host(m, knn_list_call(gated_single(Op::KnnList, o, gate, nullptr), k, max_distance, nullptr, nullptr),
                         out_host, cap, count);
}

// --- Plain device memory for callers without a HIP runtime of their own -------------
int sift_hip_device_count(int* n) {
    if (!n) return fail(SIFT_HIP_ERR_INVALID, "null argument");
    if (hipGetDeviceCount(n) != hipSuccess) *n = 0;
    return SIFT_HIP_OK;
}
int sift_hip_malloc(void** p, size_t bytes) {
    HIPCHK(hipMalloc(p, bytes));
    return SIFT_HIP_OK;
}
int sift_hip_free(void* p) {
    HIPCHK(hipFree(p));
    return SIFT_HIP_OK;
}
int sift_hip_memcpy_h2d(void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return SIFT_HIP_OK;
}
int sift_hip_memcpy_d2h(void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}
int sift_hip_device_sync(void) {
    HIPCHK(hipDeviceSynchronize());
    return SIFT_HIP_OK;
}

}  // extern "C"
