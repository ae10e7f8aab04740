// Matcher handle (sift_hip_matcher_*, sift_hip_match_*) and the descriptor
// sidecar registry of libsift_hip.so; the kernels are match.hip.  Replaces
// /root/reference/sift_cuda/sift_func/Match.cu:8-33 (matchBruteForce).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
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

namespace {
const SetFlags kNoFlags{nullptr, 0u};  // ready code sets: integers by construction
}

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

int sift_hip_match_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                           const uint16_t* const* t, const int* nt, float ratio, int ratio_on_squared, int* idx2,
                           float* d2, int* match, void* stream) {
    if (!m || P <= 0 || P > m->maxP || !q || !nq || !t || !nt) return fail(SIFT_HIP_ERR_INVALID, "bad batch");
    const MatchOut out{ratio, ratio_on_squared, idx2, d2, match};
    Sidecar sq{}, st{};
    if (P == 1 && m->sidecars && nq[0] > 0 && nt[0] > 0 && nq[0] <= m->maxQ && nt[0] <= m->maxT &&
        find_sidecar(q[0], nq[0], &sq) && find_sidecar(t[0], nt[0], &st)) {
        // Both sets are detector buffers: their codes are ready (no conversion).
        HIPCHK(hipSetDevice(m->device));
        const MatchPair pr{q[0], t[0], nq[0], nt[0], 0, 0, 0, 0, 0, 0, 0};
        launch_match_pair(pr, nullptr, CodeSet{sq.codes, sq.keys}, CodeSet{st.codes, st.keys}, kNoFlags, m->scratch(), out,
                          (hipStream_t)stream);
        HIPCHK(hipGetLastError());
        return SIFT_HIP_OK;
    }
    MatchBatch b{};
    MatchSets sets{};
    b.P = P;
    // Distinct sets by pointer (a set used by several pairs is prepared once).
    auto set_of = [&](const uint16_t* ptr, int n) {
        for (int k = 0; k < sets.nsets; k++)
            if (sets.set[k].src == ptr) {
                sets.set[k].n = std::max(sets.set[k].n, n);
                return k;
            }
        sets.set[sets.nsets] = MatchSet{ptr, n, 0};
        return sets.nsets++;
    };
    int off = 0, maxq = 1, maxt = 1;
    for (int p = 0; p < P; p++) {
        if (nq[p] < 0 || nt[p] < 0 || nq[p] > m->maxQ || nt[p] > m->maxT)
            return fail(SIFT_HIP_ERR_INVALID, "pair size exceeds matcher limits");
        if ((nq[p] && !q[p]) || (nt[p] && !t[p])) return fail(SIFT_HIP_ERR_INVALID, "null descriptor pointer");
        const int qs = set_of(q[p], nq[p]), ts = set_of(t[p], nt[p]);
        b.pair[p] = MatchPair{q[p], t[p], nq[p], nt[p], off, qs, ts, 0, 0, 0, 0};
        off += nq[p];
        maxq = std::max(maxq, nq[p]);
        maxt = std::max(maxt, nt[p]);
    }
    long row = 0;
    for (int k = 0; k < sets.nsets; k++) {
        sets.set[k].row0 = (int)row;
        row += sets.set[k].n;
        sets.maxn = std::max(sets.maxn, sets.set[k].n);
    }
    if (row > m->codeRows) return fail(SIFT_HIP_ERR_INVALID, "descriptor sets exceed the matcher's code buffer");
    for (int p = 0; p < P; p++) {
        b.pair[p].qrow0 = b.pair[p].qkrow0 = sets.set[b.pair[p].qset].row0;
        b.pair[p].trow0 = b.pair[p].tkrow0 = sets.set[b.pair[p].tset].row0;
    }
    const SetFlags flags = m->next_epoch();
    HIPCHK(hipSetDevice(m->device));
    const int S = match_plan(maxq, maxt, P).S;
    if (P == 1) {
        // One pair of foreign buffers: the fused kernel converts as it goes (no prep launch).
        launch_match_single(b.pair[0], S, m->scratch(), out, (hipStream_t)stream);
    } else {
        launch_match_prep(sets, m->dCodes, m->dRowKeys, flags, (hipStream_t)stream);
        launch_match_codes(b, S, CodeSet{m->dCodes, m->dRowKeys}, flags, m->scratch(), out, (hipStream_t)stream);
    }
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

int sift_hip_match_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P, const int* qrow0,
                                 const int* qkey0, const int* nq, const int* trow0, const int* tkey0, const int* nt,
                                 float ratio, int ratio_on_squared, int* idx2, float* d2, int* match, void* stream) {
    if (!m || P <= 0 || P > m->maxP || !codes || !keys || !qrow0 || !qkey0 || !nq || !trow0 || !tkey0 || !nt)
        return fail(SIFT_HIP_ERR_INVALID, "bad code batch");
    MatchBatch b{};
    b.P = P;
    int off = 0, maxq = 1, maxt = 1;
    for (int p = 0; p < P; p++) {
        if (nq[p] < 0 || nt[p] < 0 || nq[p] > m->maxQ || nt[p] > m->maxT)
            return fail(SIFT_HIP_ERR_INVALID, "pair size exceeds matcher limits");
        if (qrow0[p] < 0 || trow0[p] < 0 || qkey0[p] < 0 || tkey0[p] < 0)
            return fail(SIFT_HIP_ERR_INVALID, "negative set row");
        b.pair[p] = MatchPair{nullptr, nullptr, nq[p], nt[p], off, 0, 0, qrow0[p], trow0[p], qkey0[p], tkey0[p]};
        off += nq[p];
        maxq = std::max(maxq, nq[p]);
        maxt = std::max(maxt, nt[p]);
    }
    HIPCHK(hipSetDevice(m->device));
    const int S = match_plan(maxq, maxt, std::max(P, 2)).S;  // the batched kernel's plan, also for one pair
    launch_match_codes(b, S, CodeSet{codes, keys}, kNoFlags, m->scratch(),
                       MatchOut{ratio, ratio_on_squared, idx2, d2, match}, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

int sift_hip_descriptors_written(const uint16_t* desc) {
    if (!desc) return fail(SIFT_HIP_ERR_INVALID, "null descriptor buffer");
    (void)sidecar_written(desc);  // a foreign buffer has no sidecar: nothing to drop
    return SIFT_HIP_OK;
}

int sift_hip_match_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, float ratio,
                          int ratio_on_squared, int* idx2, float* d2, int* match, void* stream) {
    return sift_hip_match_batched(m, 1, &q, &nq, &t, &nt, ratio, ratio_on_squared, idx2, d2, match, stream);
}

int sift_hip_match_plan(int max_query, int max_train, int pairs, int* splits, int* waves) {
    if (max_query < 0 || max_train < 0 || pairs < 1 || !splits) return fail(SIFT_HIP_ERR_INVALID, "bad match shape");
    const MatchPlan pl = match_plan(max_query, max_train, pairs);
    *splits = pl.S;
    if (waves) *waves = pl.nw;
    return SIFT_HIP_OK;
}

int sift_hip_match_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, float ratio,
                        int ratio_on_squared, int* out) {
    if (!m || !out) return fail(SIFT_HIP_ERR_INVALID, "null argument");
    if (nq <= 0) return SIFT_HIP_OK;
    int rc = sift_hip_match_device(m, q, nq, t, nt, ratio, ratio_on_squared, nullptr, nullptr, m->dMatch, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(out, m->dMatch, sizeof(int) * nq, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

}  // extern "C"

// --- Match lists -------------------------------------------------------------
static_assert(sizeof(sift_hip_dmatch) == sizeof(MatchRecord) && sizeof(sift_hip_dmatch) == 16, "cv::DMatch layout");
static_assert(sizeof(sift_hip_match_filter) == sizeof(MatchFilter), "the filter is passed to the kernel as it is");

namespace {

bool needs_reverse(const sift_hip_match_filter& f) { return f.cross_check || f.ratio_both_ways; }

// The select scratch, at the first list call of a matcher (not under stream capture).
int ensure_select_scratch(sift_hip_matcher* m) {
    if (m->dSelIdx) return SIFT_HIP_OK;
    const size_t rows = 2 * (size_t)m->maxP * m->maxQ;
    HIPCHK(hipSetDevice(m->device));
    if (hipMalloc((void**)&m->dSelIdx, sizeof(int) * 2 * rows) != hipSuccess ||
        hipMalloc((void**)&m->dSelD, sizeof(float) * 2 * rows) != hipSuccess ||
        hipMalloc((void**)&m->dList, sizeof(MatchRecord) * (size_t)m->maxQ) != hipSuccess ||
        hipMalloc((void**)&m->dCount, sizeof(int) * (size_t)m->maxP) != hipSuccess) {
        for (void** p : {(void**)&m->dSelIdx, (void**)&m->dSelD, (void**)&m->dList, (void**)&m->dCount}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        return fail(SIFT_HIP_ERR_NOMEM, "match list scratch allocation failed");
    }
    return SIFT_HIP_OK;
}

// Argument rules shared by the list entry points (nothing is launched on a failure).
int check_list_args(sift_hip_matcher* m, int P, const int* nq, const int* nt, const sift_hip_match_filter* filter,
                    const void* out, const void* counts) {
    if (!m || !filter || !out || !counts || P <= 0 || P > m->maxP || !nq || !nt)
        return fail(SIFT_HIP_ERR_INVALID, "bad match list arguments");
    const bool rev = needs_reverse(*filter);
    for (int p = 0; p < P; p++) {
        if (nq[p] < 0 || nt[p] < 0 || nq[p] > m->maxQ || nt[p] > m->maxT)
            return fail(SIFT_HIP_ERR_INVALID, "pair size exceeds matcher limits");
        if (rev && (nt[p] > m->maxQ || nq[p] > m->maxT))
            return fail(SIFT_HIP_ERR_INVALID, "the reverse pair (roles swapped) exceeds matcher limits");
    }
    return SIFT_HIP_OK;
}

// Filter and compact the top-2 arrays in the select scratch: forward pair p at row sum_{r<p} nq[r], reverse pair p at
// row sum nq + sum_{r<p} nt[r].
int select_lists(sift_hip_matcher* m, int P, const int* nq, const int* nt, const sift_hip_match_filter& filter,
                 sift_hip_dmatch* out, int* counts, hipStream_t stream) {
    SelectBatch sb{};
    int totq = 0;
    for (int p = 0; p < P; p++) totq += nq[p];
    int fwd = 0, rev = totq;
    for (int p = 0; p < P; p++) {
        // a pair without train rows keeps nothing (its top-2 rows hold no entry)
        sb.pair[p] = SelectPair{nt[p] > 0 ? nq[p] : 0, nt[p], fwd, rev, fwd};
        fwd += nq[p];
        rev += nt[p];
    }
    const MatchFilter f{filter.ratio, filter.ratio_on_squared, filter.ratio_both_ways, filter.max_distance,
                        filter.cross_check};
    launch_match_select(sb, P, m->dSelIdx, m->dSelD, f, reinterpret_cast<MatchRecord*>(out), counts, stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

bool any_pair(int P, const int* nq, const int* nt) {
    for (int p = 0; p < P; p++)
        if (nq[p] > 0 && nt[p] > 0) return true;
    return false;
}

// The matcher's own list (dList, dCount: one pair) back to the host: the count, then min(count, cap) records.
int read_list(sift_hip_matcher* m, sift_hip_dmatch* out_host, int cap, int* count) {
    HIPCHK(hipMemcpy(count, m->dCount, sizeof(int), hipMemcpyDeviceToHost));
    const int n = std::min(*count, cap);
    if (n > 0) HIPCHK(hipMemcpy(out_host, m->dList, sizeof(sift_hip_dmatch) * (size_t)n, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

}  // namespace

extern "C" {

void sift_hip_default_match_filter(sift_hip_match_filter* f) {
    if (!f) return;
    f->ratio = 0.8f;
    f->ratio_on_squared = 0;
    f->ratio_both_ways = 0;
    f->max_distance = 0.f;
    f->cross_check = 1;
}

int sift_hip_match_list_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                const uint16_t* const* t, const int* nt, const sift_hip_match_filter* filter,
                                sift_hip_dmatch* out, int* counts, void* stream) {
    if (int rc = check_list_args(m, P, nq, nt, filter, out, counts)) return rc;
    if (!q || !t) return fail(SIFT_HIP_ERR_INVALID, "bad match list arguments");
    for (int p = 0; p < P; p++)
        if ((nq[p] && !q[p]) || (nt[p] && !t[p])) return fail(SIFT_HIP_ERR_INVALID, "null descriptor pointer");
    if (int rc = ensure_select_scratch(m)) return rc;
    const bool rev = needs_reverse(*filter);
    if (any_pair(P, nq, nt)) {
        int totq = 0;
        for (int p = 0; p < P; p++) totq += nq[p];
        Sidecar sq{}, st{};
        // A single pair of detector buffers goes through its sidecars in both directions (two direct launches).
        const bool direct = P == 1 && m->sidecars && find_sidecar(q[0], nq[0], &sq) && find_sidecar(t[0], nt[0], &st);
        if (rev && 2 * P <= m->maxP && !direct) {
            // Forward and reverse pairs in one launch; the sets are deduplicated by pointer, so each is converted once.
            const uint16_t *q2[kMaxMatchPairs], *t2[kMaxMatchPairs];
            int nq2[kMaxMatchPairs], nt2[kMaxMatchPairs];
            for (int p = 0; p < P; p++) {
                q2[p] = q[p], t2[p] = t[p], nq2[p] = nq[p], nt2[p] = nt[p];
                q2[P + p] = t[p], t2[P + p] = q[p], nq2[P + p] = nt[p], nt2[P + p] = nq[p];
            }
            if (int rc = sift_hip_match_batched(m, 2 * P, q2, nq2, t2, nt2, 0.f, 0, m->dSelIdx, m->dSelD, nullptr, stream))
                return rc;
        } else {
            // The matcher's scratch is restored when a launch ends, so launches ordered on the stream may share it.
            if (int rc = sift_hip_match_batched(m, P, q, nq, t, nt, 0.f, 0, m->dSelIdx, m->dSelD, nullptr, stream))
                return rc;
            if (rev)
                if (int rc = sift_hip_match_batched(m, P, t, nt, q, nq, 0.f, 0, m->dSelIdx + 2 * (size_t)totq,
                                                    m->dSelD + 2 * (size_t)totq, nullptr, stream))
                    return rc;
        }
    }
    HIPCHK(hipSetDevice(m->device));
    return select_lists(m, P, nq, nt, *filter, out, counts, (hipStream_t)stream);
}

int sift_hip_match_list_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                      const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                      const int* tkey0, const int* nt, const sift_hip_match_filter* filter,
                                      sift_hip_dmatch* out, int* counts, void* stream) {
    if (int rc = check_list_args(m, P, nq, nt, filter, out, counts)) return rc;
    if (!codes || !keys || !qrow0 || !qkey0 || !trow0 || !tkey0) return fail(SIFT_HIP_ERR_INVALID, "bad code batch");
    for (int p = 0; p < P; p++)
        if (qrow0[p] < 0 || trow0[p] < 0 || qkey0[p] < 0 || tkey0[p] < 0)
            return fail(SIFT_HIP_ERR_INVALID, "negative set row");
    if (int rc = ensure_select_scratch(m)) return rc;
    const bool rev = needs_reverse(*filter);
    if (any_pair(P, nq, nt)) {
        int totq = 0;
        for (int p = 0; p < P; p++) totq += nq[p];
        if (rev && 2 * P <= m->maxP) {
            int a[6][kMaxMatchPairs];  // qrow0, qkey0, nq, trow0, tkey0, nt of the 2P pairs
            for (int p = 0; p < P; p++) {
                a[0][p] = qrow0[p], a[1][p] = qkey0[p], a[2][p] = nq[p], a[3][p] = trow0[p], a[4][p] = tkey0[p], a[5][p] = nt[p];
                a[0][P + p] = trow0[p], a[1][P + p] = tkey0[p], a[2][P + p] = nt[p];
                a[3][P + p] = qrow0[p], a[4][P + p] = qkey0[p], a[5][P + p] = nq[p];
            }
            if (int rc = sift_hip_match_codes_batched(m, codes, keys, 2 * P, a[0], a[1], a[2], a[3], a[4], a[5], 0.f, 0,
                                                      m->dSelIdx, m->dSelD, nullptr, stream))
                return rc;
        } else {
            if (int rc = sift_hip_match_codes_batched(m, codes, keys, P, qrow0, qkey0, nq, trow0, tkey0, nt, 0.f, 0,
                                                      m->dSelIdx, m->dSelD, nullptr, stream))
                return rc;
            if (rev)
                if (int rc = sift_hip_match_codes_batched(m, codes, keys, P, trow0, tkey0, nt, qrow0, qkey0, nq, 0.f, 0,
                                                          m->dSelIdx + 2 * (size_t)totq, m->dSelD + 2 * (size_t)totq,
                                                          nullptr, stream))
                    return rc;
        }
    }
    HIPCHK(hipSetDevice(m->device));
    return select_lists(m, P, nq, nt, *filter, out, counts, (hipStream_t)stream);
}

int sift_hip_match_list_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                               const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* count, void* stream) {
    return sift_hip_match_list_batched(m, 1, &q, &nq, &t, &nt, filter, out, count, stream);
}

int sift_hip_match_list_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                             const sift_hip_match_filter* filter, sift_hip_dmatch* out_host, int cap, int* count) {
    if (!m || !filter || !count || cap < 0 || (cap > 0 && !out_host)) return fail(SIFT_HIP_ERR_INVALID, "null argument");
    *count = 0;
    if (int rc = check_list_args(m, 1, &nq, &nt, filter, m, m)) return rc;  // the device outputs are the matcher's own
    if (int rc = ensure_select_scratch(m)) return rc;
    if (int rc = sift_hip_match_list_device(m, q, nq, t, nt, filter, reinterpret_cast<sift_hip_dmatch*>(m->dList),
                                            m->dCount, nullptr))
        return rc;
    return read_list(m, out_host, cap, count);
}

}  // extern "C"

// --- k nearest neighbours and capped radius lists ----------------------------------
static_assert(SIFT_HIP_KNN_MAX == kKnnMax, "the kernel's largest instantiation");

namespace {

// The k-NN scratch, at the first k-NN call of a matcher (not under stream capture).
int ensure_knn_scratch(sift_hip_matcher* m) {
    if (m->dKnnLists) return SIFT_HIP_OK;
    const size_t rows = (size_t)m->maxP * m->maxQ * kKnnMax;
    HIPCHK(hipSetDevice(m->device));
    if (hipMalloc((void**)&m->dKnnLists, sizeof(unsigned long long) * kKnnMax * m->knn_lists()) != hipSuccess ||
        hipMalloc((void**)&m->dKnnIdx, sizeof(int) * rows) != hipSuccess ||
        hipMalloc((void**)&m->dKnnD, sizeof(float) * rows) != hipSuccess ||
        hipMalloc((void**)&m->dKnnRec, sizeof(MatchRecord) * (size_t)m->maxQ * kKnnMax) != hipSuccess ||
        hipMalloc((void**)&m->dKnnCount, sizeof(int) * (size_t)m->maxP) != hipSuccess) {
        for (void** p : {(void**)&m->dKnnLists, (void**)&m->dKnnIdx, (void**)&m->dKnnD, (void**)&m->dKnnRec,
                         (void**)&m->dKnnCount}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        return fail(SIFT_HIP_ERR_NOMEM, "k-NN scratch allocation failed");
    }
    return SIFT_HIP_OK;
}

// The refusals, judged before any device call: k (and for a list max_distance) need nothing else, then the matcher,
// then the pairs.
int check_knn(const sift_hip_matcher* m, int k) {
    if (k < 1 || k > kKnnMax) return fail(SIFT_HIP_ERR_INVALID, "k-NN: k outside 1..SIFT_HIP_KNN_MAX");
    if (!m) return fail(SIFT_HIP_ERR_INVALID, "null matcher");
    return SIFT_HIP_OK;
}
int check_knn_list(const sift_hip_matcher* m, int k, float max_distance, const void* out, const void* count) {
    if (std::isnan(max_distance)) return fail(SIFT_HIP_ERR_INVALID, "k-NN list: max_distance is NaN");
    if (int rc = check_knn(m, k)) return rc;
    if (!out || !count) return fail(SIFT_HIP_ERR_INVALID, "k-NN list: null out or count");
    return SIFT_HIP_OK;
}
int check_knn_pairs(const sift_hip_matcher* m, int P, const int* nq, const int* nt) {
    if (P <= 0 || P > m->maxP) return fail(SIFT_HIP_ERR_INVALID, "k-NN: P outside 1..max_pairs");
    if (!nq || !nt) return fail(SIFT_HIP_ERR_INVALID, "k-NN: null size array");
    for (int p = 0; p < P; p++)
        if (nq[p] < 0 || nt[p] < 0 || nq[p] > m->maxQ || nt[p] > m->maxT)
            return fail(SIFT_HIP_ERR_INVALID, "pair size exceeds matcher limits");
    return SIFT_HIP_OK;
}
int check_knn_sets(int P, const uint16_t* const* q, const int* nq, const uint16_t* const* t, const int* nt) {
    if (!q || !t) return fail(SIFT_HIP_ERR_INVALID, "k-NN: null descriptor array");
    for (int p = 0; p < P; p++)
        if ((nq[p] && !q[p]) || (nt[p] && !t[p])) return fail(SIFT_HIP_ERR_INVALID, "null descriptor pointer");
    return SIFT_HIP_OK;
}
int check_knn_codes(int P, const int8_t* codes, const int* keys, const int* qrow0, const int* qkey0, const int* trow0,
                    const int* tkey0) {
    if (!codes || !keys || !qrow0 || !qkey0 || !trow0 || !tkey0) return fail(SIFT_HIP_ERR_INVALID, "bad code batch");
    for (int p = 0; p < P; p++)
        if (qrow0[p] < 0 || trow0[p] < 0 || qkey0[p] < 0 || tkey0[p] < 0)
            return fail(SIFT_HIP_ERR_INVALID, "negative set row");
    return SIFT_HIP_OK;
}

bool any_queries(int P, const int* nq) {
    for (int p = 0; p < P; p++)
        if (nq[p] > 0) return true;
    return false;
}

// One k-NN launch on the pairs of b: the plan's splits, lowered to what the list scratch holds.
int knn_launch(sift_hip_matcher* m, const MatchBatch& b, int k, const CodeSet& q, const CodeSet& t, const SetFlags& flags,
               int* idx, float* d2, hipStream_t stream) {
    int maxq = 1, maxt = 1;
    for (int p = 0; p < b.P; p++) {
        maxq = std::max(maxq, b.pair[p].nq);
        maxt = std::max(maxt, b.pair[p].nt);
    }
    const size_t fit = m->knn_lists() / ((size_t)b.P * maxq);  // >= 2: P <= maxP, maxq <= maxQ
    const int S = (int)std::min<size_t>(match_knn_splits(maxq, maxt, b.P), fit);
    launch_match_knn(b, S, k, q, t, flags, KnnScratch{m->dKnnLists, m->dDone, maxq, m->sentinel()}, idx, d2, stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

// The table of checked fp16 pairs, pair p at row sum_{r<p} nq[r].  A single pair of detector buffers with fresh
// sidecars matches their codes; otherwise the call's distinct sets are converted once (k_match_prep).
int knn_fp16(sift_hip_matcher* m, int P, const uint16_t* const* q, const int* nq, const uint16_t* const* t,
             const int* nt, int k, int* idx, float* d2, hipStream_t stream) {
    if (!any_queries(P, nq)) return SIFT_HIP_OK;
    MatchBatch b{};
    MatchSets sets{};
    b.P = P;
    auto set_of = [&](const uint16_t* ptr, int n) {
        for (int s = 0; s < sets.nsets; s++)
            if (sets.set[s].src == ptr) {
                sets.set[s].n = std::max(sets.set[s].n, n);
                return s;
            }
        sets.set[sets.nsets] = MatchSet{ptr, n, 0};
        return sets.nsets++;
    };
    int off = 0;
    for (int p = 0; p < P; p++) {
        const int qs = set_of(q[p], nq[p]), ts = set_of(t[p], nt[p]);
        b.pair[p] = MatchPair{q[p], t[p], nq[p], nt[p], off, qs, ts, 0, 0, 0, 0};
        off += nq[p];
    }
    long row = 0;
    for (int s = 0; s < sets.nsets; s++) {
        sets.set[s].row0 = (int)row;
        row += sets.set[s].n;
        sets.maxn = std::max(sets.maxn, sets.set[s].n);
    }
    if (row > m->codeRows) return fail(SIFT_HIP_ERR_INVALID, "descriptor sets exceed the matcher's code buffer");
    if (int rc = ensure_knn_scratch(m)) return rc;
    HIPCHK(hipSetDevice(m->device));
    Sidecar sq{}, st{};
    if (P == 1 && m->sidecars && nq[0] > 0 && nt[0] > 0 && find_sidecar(q[0], nq[0], &sq) &&
        find_sidecar(t[0], nt[0], &st))
        return knn_launch(m, b, k, CodeSet{sq.codes, sq.keys}, CodeSet{st.codes, st.keys}, kNoFlags, idx, d2, stream);
    for (int p = 0; p < P; p++) {
        b.pair[p].qrow0 = b.pair[p].qkrow0 = sets.set[b.pair[p].qset].row0;
        b.pair[p].trow0 = b.pair[p].tkrow0 = sets.set[b.pair[p].tset].row0;
    }
    const SetFlags flags = m->next_epoch();
    launch_match_prep(sets, m->dCodes, m->dRowKeys, flags, stream);
    HIPCHK(hipGetLastError());
    const CodeSet set{m->dCodes, m->dRowKeys};
    return knn_launch(m, b, k, set, set, flags, idx, d2, stream);
}

// The list of a table in idx / d2 (pair p at row sum_{r<p} nq[r]): pair p's records from row k sum_{r<p} nq[r].
int knn_select(sift_hip_matcher* m, int P, const int* nq, int k, const int* idx, const float* d2, float max_distance,
               sift_hip_dmatch* out, int* counts, hipStream_t stream) {
    SelectBatch sb{};
    int row = 0;
    for (int p = 0; p < P; p++) {
        sb.pair[p] = SelectPair{nq[p], 0, row, 0, k * row};
        row += nq[p];
    }
    HIPCHK(hipSetDevice(m->device));
    launch_knn_select(sb, P, k, idx, d2, max_distance, reinterpret_cast<MatchRecord*>(out), counts, stream);
    HIPCHK(hipGetLastError());
    return SIFT_HIP_OK;
}

}  // namespace

extern "C" {

int sift_hip_match_knn_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                               const uint16_t* const* t, const int* nt, int k, int* idx, float* d2, void* stream) {
    if (int rc = check_knn(m, k)) return rc;
    if (int rc = check_knn_pairs(m, P, nq, nt)) return rc;
    if (int rc = check_knn_sets(P, q, nq, t, nt)) return rc;
    return knn_fp16(m, P, q, nq, t, nt, k, idx, d2, (hipStream_t)stream);
}

int sift_hip_match_knn_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, int k,
                              int* idx, float* d2, void* stream) {
    return sift_hip_match_knn_batched(m, 1, &q, &nq, &t, &nt, k, idx, d2, stream);
}

int sift_hip_match_knn_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                     const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                     const int* tkey0, const int* nt, int k, int* idx, float* d2, void* stream) {
    if (int rc = check_knn(m, k)) return rc;
    if (int rc = check_knn_pairs(m, P, nq, nt)) return rc;
    if (int rc = check_knn_codes(P, codes, keys, qrow0, qkey0, trow0, tkey0)) return rc;
    if (!any_queries(P, nq)) return SIFT_HIP_OK;
    MatchBatch b{};
    b.P = P;
    int off = 0;
    for (int p = 0; p < P; p++) {
        b.pair[p] = MatchPair{nullptr, nullptr, nq[p], nt[p], off, 0, 0, qrow0[p], trow0[p], qkey0[p], tkey0[p]};
        off += nq[p];
    }
    if (int rc = ensure_knn_scratch(m)) return rc;
    HIPCHK(hipSetDevice(m->device));
    const CodeSet set{codes, keys};
    return knn_launch(m, b, k, set, set, kNoFlags, idx, d2, (hipStream_t)stream);
}

int sift_hip_match_knn_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, int k,
                            int* idx_host, float* d2_host) {
    if (int rc = check_knn(m, k)) return rc;
    if (int rc = check_knn_pairs(m, 1, &nq, &nt)) return rc;
    if (int rc = check_knn_sets(1, &q, &nq, &t, &nt)) return rc;
    if (nq == 0) return SIFT_HIP_OK;
    if (int rc = ensure_knn_scratch(m)) return rc;
    if (int rc = knn_fp16(m, 1, &q, &nq, &t, &nt, k, m->dKnnIdx, m->dKnnD, nullptr)) return rc;
    if (idx_host) HIPCHK(hipMemcpy(idx_host, m->dKnnIdx, sizeof(int) * (size_t)nq * k, hipMemcpyDeviceToHost));
    if (d2_host) HIPCHK(hipMemcpy(d2_host, m->dKnnD, sizeof(float) * (size_t)nq * k, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

int sift_hip_match_knn_list_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                    const uint16_t* const* t, const int* nt, int k, float max_distance,
                                    sift_hip_dmatch* out, int* counts, void* stream) {
    if (int rc = check_knn_list(m, k, max_distance, out, counts)) return rc;
    if (int rc = check_knn_pairs(m, P, nq, nt)) return rc;
    if (int rc = check_knn_sets(P, q, nq, t, nt)) return rc;
    if (int rc = ensure_knn_scratch(m)) return rc;
    if (int rc = knn_fp16(m, P, q, nq, t, nt, k, m->dKnnIdx, m->dKnnD, (hipStream_t)stream)) return rc;
    return knn_select(m, P, nq, k, m->dKnnIdx, m->dKnnD, max_distance, out, counts, (hipStream_t)stream);
}

int sift_hip_match_knn_list_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, int k,
                                   float max_distance, sift_hip_dmatch* out, int* count, void* stream) {
    return sift_hip_match_knn_list_batched(m, 1, &q, &nq, &t, &nt, k, max_distance, out, count, stream);
}

int sift_hip_match_knn_list_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt, int k,
                                 float max_distance, sift_hip_dmatch* out_host, int cap, int* count) {
    if (!count || cap < 0 || (cap > 0 && !out_host)) return fail(SIFT_HIP_ERR_INVALID, "k-NN list: null out or count");
    *count = 0;
    if (int rc = check_knn_list(m, k, max_distance, m, m)) return rc;  // the device outputs are the matcher's own
    if (int rc = check_knn_pairs(m, 1, &nq, &nt)) return rc;
    if (int rc = check_knn_sets(1, &q, &nq, &t, &nt)) return rc;
    if (int rc = ensure_knn_scratch(m)) return rc;
    if (int rc = sift_hip_match_knn_list_device(m, q, nq, t, nt, k, max_distance,
                                                reinterpret_cast<sift_hip_dmatch*>(m->dKnnRec), m->dKnnCount, nullptr))
        return rc;
    HIPCHK(hipMemcpy(count, m->dKnnCount, sizeof(int), hipMemcpyDeviceToHost));
    const int n = std::min(*count, cap);
    if (n > 0) HIPCHK(hipMemcpy(out_host, m->dKnnRec, sizeof(sift_hip_dmatch) * (size_t)n, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

int sift_hip_match_knn_plan(int nq, int nt, int pairs, int k, int* splits) {
    if (nq < 0 || nt < 0 || pairs < 1 || k < 1 || k > kKnnMax || !splits)
        return fail(SIFT_HIP_ERR_INVALID, "bad k-NN shape");
    *splits = match_knn_splits(nq, nt, pairs);
    return SIFT_HIP_OK;
}

}  // extern "C"

// --- Guided matching -----------------------------------------------------------
namespace {

// The rules both gates share (`what` names the gate in the message): the position fields, which need no matcher ...
int check_gate_positions(const char* what, int query_stride, int train_stride, float radius) {
    if (query_stride < 2 || train_stride < 2)
        return fail(SIFT_HIP_ERR_INVALID, std::string(what) + ": a position stride below 2 floats");
    if (!(radius > 0.f)) return fail(SIFT_HIP_ERR_INVALID, std::string(what) + ": the radius must be > 0");
    return SIFT_HIP_OK;
}
// ... then the matcher's and the sets'.
int check_gated_sets(const char* what, const sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                     const float* query_xy, const float* train_xy) {
    if (!m) return fail(SIFT_HIP_ERR_INVALID, "null matcher");
    if (nq < 0 || nt < 0 || nq > m->maxQ || nt > m->maxT)
        return fail(SIFT_HIP_ERR_INVALID, "pair size exceeds matcher limits");
    if ((nq && !q) || (nt && !t)) return fail(SIFT_HIP_ERR_INVALID, "null descriptor pointer");
    if ((nq && !query_xy) || (nt && !train_xy))
        return fail(SIFT_HIP_ERR_INVALID, std::string(what) + ": null position pointer");
    return SIFT_HIP_OK;
}

// The gate's own rules first (they need no matcher), then the matcher's.  Nothing is launched on a failure.
int check_guided_args(const sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                      const sift_hip_match_gate* g) {
    if (!g) return fail(SIFT_HIP_ERR_INVALID, "null match gate");
    if (int rc = check_gate_positions("match gate", g->query_stride, g->train_stride, g->radius)) return rc;
    return check_gated_sets("match gate", m, q, nq, t, nt, g->query_xy, g->train_xy);
}

int check_epipolar_args(const sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                        const sift_hip_match_epipolar_gate* g) {
    if (!g) return fail(SIFT_HIP_ERR_INVALID, "null epipolar gate");
    if (int rc = check_gate_positions("epipolar gate", g->query_stride, g->train_stride, g->radius)) return rc;
    if (!(g->max_error > 0.f) || !std::isfinite(g->max_error))
        return fail(SIFT_HIP_ERR_INVALID, "epipolar gate: max_error must be > 0 and finite");
    bool zero = true;
    for (float f : g->F) {
        if (!std::isfinite(f)) return fail(SIFT_HIP_ERR_INVALID, "epipolar gate: a non-finite entry of F");
        zero = zero && f == 0.f;
    }
    if (zero) return fail(SIFT_HIP_ERR_INVALID, "epipolar gate: F is all zero");
    return check_gated_sets("epipolar gate", m, q, nq, t, nt, g->query_xy, g->train_xy);
}

// The two directions of a pair under a gate, as the kernels take it: the forward gate, and the reverse direction's
// with the roles swapped (the epipolar gate: and F transposed; e2 = max_error^2 is formed here, one float32 product).
struct WindowGates {
    MatchGate fwd, rev;
    explicit WindowGates(const sift_hip_match_gate& g)
        : fwd{g.query_xy, g.train_xy, g.query_stride, g.train_stride, g.radius},
          rev{g.train_xy, g.query_xy, g.train_stride, g.query_stride, g.radius} {}
};
struct EpipolarGates {
    EpipolarGate fwd, rev;
    explicit EpipolarGates(const sift_hip_match_epipolar_gate& g) {
        const float e2 = g.max_error * g.max_error;
        fwd = EpipolarGate{g.query_xy, g.train_xy, g.query_stride, g.train_stride, g.radius, e2, {}};
        rev = EpipolarGate{g.train_xy, g.query_xy, g.train_stride, g.query_stride, g.radius, e2, {}};
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) fwd.F[3 * r + c] = rev.F[3 * c + r] = g.F[3 * r + c];
    }
};
void launch_gated_pair(const MatchPair& pr, const MatchGate& g, const CodeSet& q, const CodeSet& t, const SetFlags& flags,
                       const MatchScratch& sc, const MatchOut& out, hipStream_t s) {
    launch_match_pair(pr, &g, q, t, flags, sc, out, s);
}
void launch_gated_pair(const MatchPair& pr, const EpipolarGate& g, const CodeSet& q, const CodeSet& t,
                       const SetFlags& flags, const MatchScratch& sc, const MatchOut& out, hipStream_t s) {
    launch_match_pair(pr, g, q, t, flags, sc, out, s);
}

// The guided top-2 of (q, t) into idx2 / d2 / match and, with rev_idx2, of (t, q) under the reverse gate into
// rev_idx2 / rev_d2 (Gates: WindowGates or EpipolarGates).  Arguments are checked by the caller; nq > 0.  Detector
// buffers with fresh sidecars: one launch per direction on their codes.  Otherwise k_match_prep once for both sets,
// then one launch per direction.
template <class Gates>
int guided_top2(sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt, const Gates& g, float ratio,
                int ratio_on_squared, int* idx2, float* d2, int* match, int* rev_idx2, float* rev_d2,
                hipStream_t stream) {
    CodeSet qc, tc;
    SetFlags flags = kNoFlags;
    int qs = 0, ts = 0;
    Sidecar sq{}, st{};
    HIPCHK(hipSetDevice(m->device));
    if (m->sidecars && nt > 0 && find_sidecar(q, nq, &sq) && find_sidecar(t, nt, &st)) {
        qc = CodeSet{sq.codes, sq.keys}, tc = CodeSet{st.codes, st.keys};
    } else {
        MatchSets sets{};
        sets.set[sets.nsets++] = MatchSet{q, nq, 0};
        if (t == q)
            sets.set[0].n = std::max(nq, nt);
        else
            sets.set[ts = sets.nsets++] = MatchSet{t, nt, nq};
        sets.maxn = std::max(nq, nt);
        if ((long)nq + nt > m->codeRows)
            return fail(SIFT_HIP_ERR_INVALID, "descriptor sets exceed the matcher's code buffer");
        flags = m->next_epoch();
        launch_match_prep(sets, m->dCodes, m->dRowKeys, flags, stream);
        HIPCHK(hipGetLastError());
        const int trow0 = sets.set[ts].row0;
        qc = CodeSet{m->dCodes, m->dRowKeys}, tc = CodeSet{m->dCodes + (size_t)trow0 * 128, m->dRowKeys + trow0};
    }
    const MatchPair fwd{q, t, nq, nt, 0, qs, ts, 0, 0, 0, 0};
    launch_gated_pair(fwd, g.fwd, qc, tc, flags, m->scratch(), MatchOut{ratio, ratio_on_squared, idx2, d2, match},
                      stream);
    HIPCHK(hipGetLastError());
    if (rev_idx2 && nt > 0) {
        // The matcher's scratch is restored when a launch ends, so launches ordered on the stream may share it.
        const MatchPair rev{t, q, nt, nq, 0, ts, qs, 0, 0, 0, 0};
        launch_gated_pair(rev, g.rev, tc, qc, flags, m->scratch(), MatchOut{0.f, 0, rev_idx2, rev_d2, nullptr}, stream);
        HIPCHK(hipGetLastError());
    }
    return SIFT_HIP_OK;
}

// The guided match list of a checked pair: the guided top-2 of the directions the filter needs into the select
// scratch, then the filter and the compaction.
template <class Gates>
int guided_list(sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt, const Gates& g,
                const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* count, hipStream_t stream) {
    if (int rc = check_list_args(m, 1, &nq, &nt, filter, out, count)) return rc;
    if (int rc = ensure_select_scratch(m)) return rc;
    if (nq > 0 && nt > 0) {
        const bool rev = needs_reverse(*filter);
        if (int rc = guided_top2(m, q, nq, t, nt, g, 0.f, 0, m->dSelIdx, m->dSelD, nullptr,
                                 rev ? m->dSelIdx + 2 * (size_t)nq : nullptr, m->dSelD + 2 * (size_t)nq, stream))
            return rc;
    }
    HIPCHK(hipSetDevice(m->device));
    return select_lists(m, 1, &nq, &nt, *filter, out, count, stream);
}

// The same into the matcher's own list, synchronously, and back to the host.
template <class Gates>
int guided_list_host(sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt, const Gates& g,
                     const sift_hip_match_filter* filter, sift_hip_dmatch* out_host, int cap, int* count) {
    if (int rc = check_list_args(m, 1, &nq, &nt, filter, m, m)) return rc;  // the device outputs are the matcher's own
    if (int rc = ensure_select_scratch(m)) return rc;
    if (int rc = guided_list(m, q, nq, t, nt, g, filter, reinterpret_cast<sift_hip_dmatch*>(m->dList), m->dCount, nullptr))
        return rc;
    return read_list(m, out_host, cap, count);
}

}  // namespace

extern "C" {

int sift_hip_match_guided_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                 const sift_hip_match_gate* gate, float ratio, int ratio_on_squared, int* idx2,
                                 float* d2, int* match, void* stream) {
    if (int rc = check_guided_args(m, q, nq, t, nt, gate)) return rc;
    if (nq == 0) return SIFT_HIP_OK;
    return guided_top2(m, q, nq, t, nt, WindowGates(*gate), ratio, ratio_on_squared, idx2, d2, match, nullptr, nullptr,
                       (hipStream_t)stream);
}

int sift_hip_match_guided_plan(int nq, int nt, int* splits) {
    if (nq < 0 || nt < 0 || !splits) return fail(SIFT_HIP_ERR_INVALID, "bad match shape");
    *splits = match_direct_splits(nq, nt);
    return SIFT_HIP_OK;
}

int sift_hip_match_list_guided_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                      const sift_hip_match_gate* gate, const sift_hip_match_filter* filter,
                                      sift_hip_dmatch* out, int* count, void* stream) {
    if (int rc = check_guided_args(m, q, nq, t, nt, gate)) return rc;
    return guided_list(m, q, nq, t, nt, WindowGates(*gate), filter, out, count, (hipStream_t)stream);
}

int sift_hip_match_list_guided_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                    const sift_hip_match_gate* gate, const sift_hip_match_filter* filter,
                                    sift_hip_dmatch* out_host, int cap, int* count) {
    if (!filter || !count || cap < 0 || (cap > 0 && !out_host)) return fail(SIFT_HIP_ERR_INVALID, "null argument");
    *count = 0;
    if (int rc = check_guided_args(m, q, nq, t, nt, gate)) return rc;
    return guided_list_host(m, q, nq, t, nt, WindowGates(*gate), filter, out_host, cap, count);
}

int sift_hip_match_epipolar_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                   const sift_hip_match_epipolar_gate* gate, float ratio, int ratio_on_squared,
                                   int* idx2, float* d2, int* match, void* stream) {
    if (int rc = check_epipolar_args(m, q, nq, t, nt, gate)) return rc;
    if (nq == 0) return SIFT_HIP_OK;
    return guided_top2(m, q, nq, t, nt, EpipolarGates(*gate), ratio, ratio_on_squared, idx2, d2, match, nullptr,
                       nullptr, (hipStream_t)stream);
}

int sift_hip_match_list_epipolar_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                        const sift_hip_match_epipolar_gate* gate, const sift_hip_match_filter* filter,
                                        sift_hip_dmatch* out, int* count, void* stream) {
    if (int rc = check_epipolar_args(m, q, nq, t, nt, gate)) return rc;
    return guided_list(m, q, nq, t, nt, EpipolarGates(*gate), filter, out, count, (hipStream_t)stream);
}

int sift_hip_match_list_epipolar_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                      const sift_hip_match_epipolar_gate* gate, const sift_hip_match_filter* filter,
                                      sift_hip_dmatch* out_host, int cap, int* count) {
    if (!filter || !count || cap < 0 || (cap > 0 && !out_host)) return fail(SIFT_HIP_ERR_INVALID, "null argument");
    *count = 0;
    if (int rc = check_epipolar_args(m, q, nq, t, nt, gate)) return rc;
    return guided_list_host(m, q, nq, t, nt, EpipolarGates(*gate), filter, out_host, cap, count);
}

}  // extern "C"

// --- Batched guided matching ------------------------------------------------------
static_assert(sizeof(sift_hip_match_positions) == 2 * sizeof(void*), "two device pointers per pair");

namespace {

// The call-wide rules of a gated batch, which need no matcher: the position fields, then under the epipolar gate
// (epipolar: geometry, its stride and max_error are looked at) the geometry's.  The nine floats themselves are on the
// device: the kernel applies the usable-geometry rule to them.
int check_gated_call(bool epipolar, int query_stride, int train_stride, float radius, const void* geometry,
                     int geometry_stride, float max_error) {
    const char* what = epipolar ? "epipolar gate" : "match gate";
    if (int rc = check_gate_positions(what, query_stride, train_stride, radius)) return rc;
    if (!epipolar) return SIFT_HIP_OK;
    if (!(max_error > 0.f) || !std::isfinite(max_error))
        return fail(SIFT_HIP_ERR_INVALID, "epipolar gate: max_error must be > 0 and finite");
    if (!geometry) return fail(SIFT_HIP_ERR_INVALID, "epipolar gate: null geometry");
    if (geometry_stride < 36 || geometry_stride % 4)
        return fail(SIFT_HIP_ERR_INVALID, "epipolar gate: geometry_stride_bytes must be >= 36 and a multiple of 4");
    return SIFT_HIP_OK;
}

// ... then the matcher's and the pairs'.
int check_gated_pairs(bool epipolar, const sift_hip_matcher* m, int P, const int* nq, const int* nt,
                      const sift_hip_match_positions* positions) {
    if (!m) return fail(SIFT_HIP_ERR_INVALID, "null matcher");
    if (P <= 0 || P > m->maxP || !nq || !nt || !positions) return fail(SIFT_HIP_ERR_INVALID, "bad gated batch");
    for (int p = 0; p < P; p++) {
        if (nq[p] < 0 || nt[p] < 0 || nq[p] > m->maxQ || nt[p] > m->maxT)
            return fail(SIFT_HIP_ERR_INVALID, "pair size exceeds matcher limits");
        if ((nq[p] && !positions[p].query_xy) || (nt[p] && !positions[p].train_xy))
            return fail(SIFT_HIP_ERR_INVALID,
                        std::string(epipolar ? "epipolar gate" : "match gate") + ": null position pointer");
    }
    return SIFT_HIP_OK;
}

// A gated call as the launcher takes it; e2 = max_error^2 is formed here, one float32 product.
GatedCall gated_call(bool epipolar, int query_stride, int train_stride, float radius, const void* geometry,
                     int geometry_stride, float max_error) {
    return GatedCall{query_stride, train_stride, radius, epipolar ? max_error * max_error : 0.f,
                     epipolar ? geometry : nullptr, epipolar ? geometry_stride : 0};
}

// The pairs of a call: the forward pairs [0, P) with their rows at sum_{r<p} nq[r], and -- when a filter needs them --
// the reverse pairs [P, 2P) with the roles swapped, rows at sum nq + sum_{r<p} nt[r] (select_lists' layout).
struct GatedPairs {
    GatedPair pair[2 * kMaxMatchPairs];
    void fill(int P, bool rev, const sift_hip_match_positions* pos) {
        int totq = 0;
        for (int p = 0; p < P; p++) totq += pair[p].pr.nq;
        int fwd = 0, roff = totq;
        for (int p = 0; p < P; p++) {
            GatedPair& f = pair[p];
            f.pr.out_off = fwd;
            f.qxy = pos[p].query_xy, f.txy = pos[p].train_xy, f.geom = p, f.swapped = 0;
            fwd += f.pr.nq;
            if (!rev) continue;
            const MatchPair& a = f.pr;
            pair[P + p] = GatedPair{MatchPair{a.t, a.q, a.nt, a.nq, roff, a.tset, a.qset, a.trow0, a.qrow0, a.tkrow0,
                                              a.qkrow0},
                                    f.txy, f.qxy, p, 1};
            roff += a.nt;
        }
    }
};

// Whether a call has an output row to write at all (a query without train rows still gets its -1 / FLT_MAX row).
bool any_rows(int P, const int* nq, const int* nt, bool rev) {
    for (int p = 0; p < P; p++)
        if (nq[p] > 0 || (rev && nt[p] > 0)) return true;
    return false;
}

// n pairs in launches of at most kMaxGatedPairs, ordered on the stream (the scratch is restored when each ends).
int launch_gated(sift_hip_matcher* m, const GatedPair* pairs, int n, const GatedCall& call, const CodeSet& set,
                 const SetFlags& flags, const MatchOut& out, hipStream_t stream) {
    for (int p0 = 0; p0 < n; p0 += kMaxGatedPairs) {
        GatedBatch b{};
        b.P = std::min(kMaxGatedPairs, n - p0);
        std::copy(pairs + p0, pairs + p0 + b.P, b.pair);
        launch_match_gated(b, call, set, flags, m->scratch(), out, stream);
        HIPCHK(hipGetLastError());
    }
    return SIFT_HIP_OK;
}

// Forward pairs, and with `rev` the reverse pairs: in one pass over 2P pairs when the matcher holds that many,
// else in two of P.  The bytes are the same either way.
int launch_gated_directions(sift_hip_matcher* m, const GatedPairs& g, int P, bool rev, const GatedCall& call,
                            const CodeSet& set, const SetFlags& flags, const MatchOut& out, hipStream_t stream) {
    if (rev && 2 * P <= m->maxP) return launch_gated(m, g.pair, 2 * P, call, set, flags, out, stream);
    if (int rc = launch_gated(m, g.pair, P, call, set, flags, out, stream)) return rc;
    return rev ? launch_gated(m, g.pair + P, P, call, set, flags, out, stream) : SIFT_HIP_OK;
}

// fp16 sets: always converted (k_match_prep, distinct sets once, as sift_hip_match_batched does for P > 1), then the
// gated launches on the prepared codes with their flags.  Arguments are checked by the caller.
int gated_batch_fp16(sift_hip_matcher* m, int P, const uint16_t* const* q, const int* nq, const uint16_t* const* t,
                     const int* nt, const sift_hip_match_positions* pos, bool rev, const GatedCall& call,
                     const MatchOut& out, hipStream_t stream) {
    if (!q || !t) return fail(SIFT_HIP_ERR_INVALID, "bad gated batch");
    for (int p = 0; p < P; p++)
        if ((nq[p] && !q[p]) || (nt[p] && !t[p])) return fail(SIFT_HIP_ERR_INVALID, "null descriptor pointer");
    if (!any_rows(P, nq, nt, rev)) return SIFT_HIP_OK;
    MatchSets sets{};
    auto set_of = [&](const uint16_t* ptr, int n) {
        for (int k = 0; k < sets.nsets; k++)
            if (sets.set[k].src == ptr) {
                sets.set[k].n = std::max(sets.set[k].n, n);
                return k;
            }
        sets.set[sets.nsets] = MatchSet{ptr, n, 0};
        return sets.nsets++;
    };
    GatedPairs g{};
    for (int p = 0; p < P; p++) {
        const int qs = set_of(q[p], nq[p]), ts = set_of(t[p], nt[p]);
        g.pair[p].pr = MatchPair{q[p], t[p], nq[p], nt[p], 0, qs, ts, 0, 0, 0, 0};
    }
    long row = 0;
    for (int k = 0; k < sets.nsets; k++) {
        sets.set[k].row0 = (int)row;
        row += sets.set[k].n;
        sets.maxn = std::max(sets.maxn, sets.set[k].n);
    }
    if (row > m->codeRows) return fail(SIFT_HIP_ERR_INVALID, "descriptor sets exceed the matcher's code buffer");
    for (int p = 0; p < P; p++) {
        MatchPair& pr = g.pair[p].pr;
        pr.qrow0 = pr.qkrow0 = sets.set[pr.qset].row0;
        pr.trow0 = pr.tkrow0 = sets.set[pr.tset].row0;
    }
    g.fill(P, rev, pos);
    const SetFlags flags = m->next_epoch();
    HIPCHK(hipSetDevice(m->device));
    launch_match_prep(sets, m->dCodes, m->dRowKeys, flags, stream);
    HIPCHK(hipGetLastError());
    return launch_gated_directions(m, g, P, rev, call, CodeSet{m->dCodes, m->dRowKeys}, flags, out, stream);
}

// Ready code sets (sift_hip_match_list_codes_batched's arguments): no conversion, no flags.
int gated_batch_codes(sift_hip_matcher* m, const int8_t* codes, const int* keys, int P, const int* qrow0,
                      const int* qkey0, const int* nq, const int* trow0, const int* tkey0, const int* nt,
                      const sift_hip_match_positions* pos, bool rev, const GatedCall& call, const MatchOut& out,
                      hipStream_t stream) {
    if (!codes || !keys || !qrow0 || !qkey0 || !trow0 || !tkey0) return fail(SIFT_HIP_ERR_INVALID, "bad code batch");
    for (int p = 0; p < P; p++)
        if (qrow0[p] < 0 || trow0[p] < 0 || qkey0[p] < 0 || tkey0[p] < 0)
            return fail(SIFT_HIP_ERR_INVALID, "negative set row");
    if (!any_rows(P, nq, nt, rev)) return SIFT_HIP_OK;
    GatedPairs g{};
    for (int p = 0; p < P; p++)
        g.pair[p].pr = MatchPair{nullptr, nullptr, nq[p], nt[p], 0, 0, 0, qrow0[p], trow0[p], qkey0[p], tkey0[p]};
    g.fill(P, rev, pos);
    HIPCHK(hipSetDevice(m->device));
    return launch_gated_directions(m, g, P, rev, call, CodeSet{codes, keys}, kNoFlags, out, stream);
}

}  // namespace

extern "C" {

int sift_hip_match_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                  const uint16_t* const* t, const int* nt, const sift_hip_match_positions* positions,
                                  int query_stride, int train_stride, float radius, float ratio, int ratio_on_squared,
                                  int* idx2, float* d2, int* match, void* stream) {
    if (int rc = check_gated_call(false, query_stride, train_stride, radius, nullptr, 0, 0.f)) return rc;
    if (int rc = check_gated_pairs(false, m, P, nq, nt, positions)) return rc;
    return gated_batch_fp16(m, P, q, nq, t, nt, positions, false,
                            gated_call(false, query_stride, train_stride, radius, nullptr, 0, 0.f),
                            MatchOut{ratio, ratio_on_squared, idx2, d2, match}, (hipStream_t)stream);
}

int sift_hip_match_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                    const uint16_t* const* t, const int* nt, const sift_hip_match_positions* positions,
                                    int query_stride, int train_stride, float radius, const void* geometry,
                                    int geometry_stride_bytes, float max_error, float ratio, int ratio_on_squared,
                                    int* idx2, float* d2, int* match, void* stream) {
    if (int rc = check_gated_call(true, query_stride, train_stride, radius, geometry, geometry_stride_bytes, max_error))
        return rc;
    if (int rc = check_gated_pairs(true, m, P, nq, nt, positions)) return rc;
    return gated_batch_fp16(m, P, q, nq, t, nt, positions, false,
                            gated_call(true, query_stride, train_stride, radius, geometry, geometry_stride_bytes,
                                       max_error),
                            MatchOut{ratio, ratio_on_squared, idx2, d2, match}, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// The four list forms: the gated top-2 of the directions the filter needs into the select scratch, then the filter
// and the compaction (select_lists: sift_hip_match_list_batched's layout, imgIdx = p, counts on the device).
template <class Top2>
int gated_list(bool epipolar, sift_hip_matcher* m, int P, const int* nq, const int* nt,
               const sift_hip_match_positions* positions, int query_stride, int train_stride, float radius,
               const void* geometry, int geometry_stride, float max_error, const sift_hip_match_filter* filter,
               sift_hip_dmatch* out, int* counts, hipStream_t stream, Top2 top2) {
    if (int rc = check_gated_call(epipolar, query_stride, train_stride, radius, geometry, geometry_stride, max_error))
        return rc;
    if (int rc = check_gated_pairs(epipolar, m, P, nq, nt, positions)) return rc;
    if (int rc = check_list_args(m, P, nq, nt, filter, out, counts)) return rc;
    if (int rc = ensure_select_scratch(m)) return rc;
    const GatedCall call = gated_call(epipolar, query_stride, train_stride, radius, geometry, geometry_stride, max_error);
    if (int rc = top2(needs_reverse(*filter), call, MatchOut{0.f, 0, m->dSelIdx, m->dSelD, nullptr})) return rc;
    HIPCHK(hipSetDevice(m->device));
    return select_lists(m, P, nq, nt, *filter, out, counts, stream);
}

}  // namespace

extern "C" {

int sift_hip_match_list_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                       const uint16_t* const* t, const int* nt,
                                       const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                       float radius, const sift_hip_match_filter* filter, sift_hip_dmatch* out,
                                       int* counts, void* stream) {
    return gated_list(false, m, P, nq, nt, positions, query_stride, train_stride, radius, nullptr, 0, 0.f, filter, out,
                      counts, (hipStream_t)stream, [&](bool rev, const GatedCall& call, const MatchOut& o) {
                          return gated_batch_fp16(m, P, q, nq, t, nt, positions, rev, call, o, (hipStream_t)stream);
                      });
}

int sift_hip_match_list_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                         const uint16_t* const* t, const int* nt,
                                         const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                         float radius, const void* geometry, int geometry_stride_bytes, float max_error,
                                         const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* counts,
                                         void* stream) {
    return gated_list(true, m, P, nq, nt, positions, query_stride, train_stride, radius, geometry, geometry_stride_bytes,
                      max_error, filter, out, counts, (hipStream_t)stream,
                      [&](bool rev, const GatedCall& call, const MatchOut& o) {
                          return gated_batch_fp16(m, P, q, nq, t, nt, positions, rev, call, o, (hipStream_t)stream);
                      });
}

int sift_hip_match_list_guided_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                             const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                             const int* tkey0, const int* nt,
                                             const sift_hip_match_positions* positions, int query_stride,
                                             int train_stride, float radius, const sift_hip_match_filter* filter,
                                             sift_hip_dmatch* out, int* counts, void* stream) {
    return gated_list(false, m, P, nq, nt, positions, query_stride, train_stride, radius, nullptr, 0, 0.f, filter, out,
                      counts, (hipStream_t)stream, [&](bool rev, const GatedCall& call, const MatchOut& o) {
                          return gated_batch_codes(m, codes, keys, P, qrow0, qkey0, nq, trow0, tkey0, nt, positions, rev,
                                                   call, o, (hipStream_t)stream);
                      });
}

int sift_hip_match_list_epipolar_codes_batched(sift_hip_matcher_t m, const int8_t* codes, const int* keys, int P,
                                               const int* qrow0, const int* qkey0, const int* nq, const int* trow0,
                                               const int* tkey0, const int* nt,
                                               const sift_hip_match_positions* positions, int query_stride,
                                               int train_stride, float radius, const void* geometry,
                                               int geometry_stride_bytes, float max_error,
                                               const sift_hip_match_filter* filter, sift_hip_dmatch* out, int* counts,
                                               void* stream) {
    return gated_list(true, m, P, nq, nt, positions, query_stride, train_stride, radius, geometry, geometry_stride_bytes,
                      max_error, filter, out, counts, (hipStream_t)stream,
                      [&](bool rev, const GatedCall& call, const MatchOut& o) {
                          return gated_batch_codes(m, codes, keys, P, qrow0, qkey0, nq, trow0, tkey0, nt, positions, rev,
                                                   call, o, (hipStream_t)stream);
                      });
}

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
// --- Gated k nearest neighbours ---------------------------------------------------
namespace {

// What a gated k-NN call passes beside its pairs: which gate, the call-wide fields and -- the single-pair epipolar
// call, geometry == nullptr -- the host's F, which travels as a kernel argument.
struct KnnGate {
    bool epipolar;
    GatedCall call;
    float F[9];
};
KnnGate knn_gate_of(const sift_hip_match_gate& g) {
    return KnnGate{false, gated_call(false, g.query_stride, g.train_stride, g.radius, nullptr, 0, 0.f), {}};
}
KnnGate knn_gate_of(const sift_hip_match_epipolar_gate& g) {
    KnnGate kg{true, GatedCall{g.query_stride, g.train_stride, g.radius, g.max_error * g.max_error, nullptr, 0}, {}};
    std::copy(g.F, g.F + 9, kg.F);
    return kg;
}
sift_hip_match_positions positions_of(const sift_hip_match_gate& g) { return {g.query_xy, g.train_xy}; }
sift_hip_match_positions positions_of(const sift_hip_match_epipolar_gate& g) { return {g.query_xy, g.train_xy}; }
int check_gate_args(const sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                    const sift_hip_match_gate* g) {
    return check_guided_args(m, q, nq, t, nt, g);
}
int check_gate_args(const sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                    const sift_hip_match_epipolar_gate* g) {
    return check_epipolar_args(m, q, nq, t, nt, g);
}

// The refusals that need no matcher, in the order of include/sift_hip.h: k, a list's max_distance (list: the call
// has one), then the gate's own.
int check_knn_k(int k, bool list, float max_distance) {
    if (k < 1 || k > kKnnMax) return fail(SIFT_HIP_ERR_INVALID, "k-NN: k outside 1..SIFT_HIP_KNN_MAX");
    if (list && std::isnan(max_distance)) return fail(SIFT_HIP_ERR_INVALID, "k-NN list: max_distance is NaN");
    return SIFT_HIP_OK;
}

// Launches of at most kMaxGatedPairs pairs, ordered on the stream; each takes the plan's splits for its own pairs,
// lowered to what the list scratch holds, and restores the counters it used.
int knn_gated_launch(sift_hip_matcher* m, const MatchPair* pairs, const sift_hip_match_positions* pos, int P,
                     const KnnGate& kg, int k, const CodeSet& q, const CodeSet& t, const SetFlags& flags, int* idx,
                     float* d2, hipStream_t stream) {
    for (int p0 = 0; p0 < P; p0 += kMaxGatedPairs) {
        KnnGatedBatch b{};
        b.P = std::min(kMaxGatedPairs, P - p0);
        b.call = kg.call;
        std::copy(kg.F, kg.F + 9, b.F);
        int maxq = 1, maxt = 1;
        bool rows = false;
        for (int i = 0; i < b.P; i++) {
            b.pair[i] = pairs[p0 + i];
            b.qxy[i] = pos[p0 + i].query_xy;
            b.txy[i] = pos[p0 + i].train_xy;
            b.geom[i] = p0 + i;
            maxq = std::max(maxq, b.pair[i].nq);
            maxt = std::max(maxt, b.pair[i].nt);
            rows = rows || b.pair[i].nq > 0;
        }
        if (!rows) continue;
        const size_t fit = m->knn_lists() / ((size_t)b.P * maxq);  // >= 2: P <= maxP, maxq <= maxQ
        const int S = (int)std::min<size_t>(match_knn_splits(maxq, maxt, b.P), fit);
        launch_match_knn_gated(b, kg.epipolar, S, k, q, t, flags, KnnScratch{m->dKnnLists, m->dDone, maxq, m->sentinel()},
                               idx, d2, stream);
        HIPCHK(hipGetLastError());
    }
    return SIFT_HIP_OK;
}

// The gated table of checked fp16 pairs, pair p at row sum_{r<p} nq[r] (knn_fp16 under a gate).  sidecars: the
// single-pair calls, where two detector buffers with fresh sidecars match their codes; the batched forms convert.
int knn_gated_fp16(sift_hip_matcher* m, int P, const uint16_t* const* q, const int* nq, const uint16_t* const* t,
                   const int* nt, const sift_hip_match_positions* pos, const KnnGate& kg, bool sidecars, int k, int* idx,
                   float* d2, hipStream_t stream) {
    if (!any_queries(P, nq)) return SIFT_HIP_OK;
    MatchPair pairs[kMaxMatchPairs];
    MatchSets sets{};
    auto set_of = [&](const uint16_t* ptr, int n) {
        for (int s = 0; s < sets.nsets; s++)
            if (sets.set[s].src == ptr) {
                sets.set[s].n = std::max(sets.set[s].n, n);
                return s;
            }
        sets.set[sets.nsets] = MatchSet{ptr, n, 0};
        return sets.nsets++;
    };
    int off = 0;
    for (int p = 0; p < P; p++) {
        const int qs = set_of(q[p], nq[p]), ts = set_of(t[p], nt[p]);
        pairs[p] = MatchPair{q[p], t[p], nq[p], nt[p], off, qs, ts, 0, 0, 0, 0};
        off += nq[p];
    }
    long row = 0;
    for (int s = 0; s < sets.nsets; s++) {
        sets.set[s].row0 = (int)row;
        row += sets.set[s].n;
        sets.maxn = std::max(sets.maxn, sets.set[s].n);
    }
    if (row > m->codeRows) return fail(SIFT_HIP_ERR_INVALID, "descriptor sets exceed the matcher's code buffer");
    if (int rc = ensure_knn_scratch(m)) return rc;
    HIPCHK(hipSetDevice(m->device));
    Sidecar sq{}, st{};
    if (sidecars && P == 1 && m->sidecars && nq[0] > 0 && nt[0] > 0 && find_sidecar(q[0], nq[0], &sq) &&
        find_sidecar(t[0], nt[0], &st))
        return knn_gated_launch(m, pairs, pos, P, kg, k, CodeSet{sq.codes, sq.keys}, CodeSet{st.codes, st.keys}, kNoFlags,
                                idx, d2, stream);
    for (int p = 0; p < P; p++) {
        pairs[p].qrow0 = pairs[p].qkrow0 = sets.set[pairs[p].qset].row0;
        pairs[p].trow0 = pairs[p].tkrow0 = sets.set[pairs[p].tset].row0;
    }
    const SetFlags flags = m->next_epoch();
    launch_match_prep(sets, m->dCodes, m->dRowKeys, flags, stream);
    HIPCHK(hipGetLastError());
    const CodeSet set{m->dCodes, m->dRowKeys};
    return knn_gated_launch(m, pairs, pos, P, kg, k, set, set, flags, idx, d2, stream);
}

// The single-pair forms under either gate (Gate: sift_hip_match_gate or sift_hip_match_epipolar_gate).
template <class Gate>
int knn_gated_device(sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt, const Gate* gate, int k,
                     int* idx, float* d2, hipStream_t stream) {
    if (int rc = check_knn_k(k, false, 0.f)) return rc;
    if (int rc = check_gate_args(m, q, nq, t, nt, gate)) return rc;
    const sift_hip_match_positions pos = positions_of(*gate);
    return knn_gated_fp16(m, 1, &q, &nq, &t, &nt, &pos, knn_gate_of(*gate), true, k, idx, d2, stream);
}
template <class Gate>
int knn_gated_list_device(sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt, const Gate* gate,
                          int k, float max_distance, sift_hip_dmatch* out, int* count, hipStream_t stream) {
    if (int rc = check_knn_k(k, true, max_distance)) return rc;
    if (int rc = check_gate_args(m, q, nq, t, nt, gate)) return rc;
    if (!out || !count) return fail(SIFT_HIP_ERR_INVALID, "k-NN list: null out or count");
    if (int rc = ensure_knn_scratch(m)) return rc;
    const sift_hip_match_positions pos = positions_of(*gate);
    if (int rc = knn_gated_fp16(m, 1, &q, &nq, &t, &nt, &pos, knn_gate_of(*gate), true, k, m->dKnnIdx, m->dKnnD, stream))
        return rc;
    return knn_select(m, 1, &nq, k, m->dKnnIdx, m->dKnnD, max_distance, out, count, stream);
}
template <class Gate>
int knn_gated_host(sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt, const Gate* gate, int k,
                   int* idx_host, float* d2_host) {
    if (int rc = check_knn_k(k, false, 0.f)) return rc;
    if (int rc = check_gate_args(m, q, nq, t, nt, gate)) return rc;
    if (nq == 0) return SIFT_HIP_OK;
    if (int rc = ensure_knn_scratch(m)) return rc;
    if (int rc = knn_gated_device(m, q, nq, t, nt, gate, k, m->dKnnIdx, m->dKnnD, nullptr)) return rc;
    if (idx_host) HIPCHK(hipMemcpy(idx_host, m->dKnnIdx, sizeof(int) * (size_t)nq * k, hipMemcpyDeviceToHost));
    if (d2_host) HIPCHK(hipMemcpy(d2_host, m->dKnnD, sizeof(float) * (size_t)nq * k, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}
template <class Gate>
int knn_gated_list_host(sift_hip_matcher* m, const uint16_t* q, int nq, const uint16_t* t, int nt, const Gate* gate,
                        int k, float max_distance, sift_hip_dmatch* out_host, int cap, int* count) {
    if (!count || cap < 0 || (cap > 0 && !out_host)) return fail(SIFT_HIP_ERR_INVALID, "k-NN list: null out or count");
    *count = 0;
    if (int rc = check_knn_k(k, true, max_distance)) return rc;
    if (int rc = check_gate_args(m, q, nq, t, nt, gate)) return rc;
    if (int rc = ensure_knn_scratch(m)) return rc;
    if (int rc = knn_gated_list_device(m, q, nq, t, nt, gate, k, max_distance,
                                       reinterpret_cast<sift_hip_dmatch*>(m->dKnnRec), m->dKnnCount, nullptr))
        return rc;
    HIPCHK(hipMemcpy(count, m->dKnnCount, sizeof(int), hipMemcpyDeviceToHost));
    const int n = std::min(*count, cap);
    if (n > 0) HIPCHK(hipMemcpy(out_host, m->dKnnRec, sizeof(sift_hip_dmatch) * (size_t)n, hipMemcpyDeviceToHost));
    return SIFT_HIP_OK;
}

// The batched forms: the table into idx / d2, or (out != nullptr or list) into the matcher's own table and then the
// list.  The checks in the header's order: k, max_distance, the call's gate fields, then the matcher's and the pairs'.
int knn_gated_batched(bool epipolar, bool list, sift_hip_matcher* m, int P, const uint16_t* const* q, const int* nq,
                      const uint16_t* const* t, const int* nt, const sift_hip_match_positions* positions,
                      int query_stride, int train_stride, float radius, const void* geometry, int geometry_stride,
                      float max_error, int k, float max_distance, int* idx, float* d2, sift_hip_dmatch* out, int* counts,
                      hipStream_t stream) {
    if (int rc = check_knn_k(k, list, max_distance)) return rc;
    if (int rc = check_gated_call(epipolar, query_stride, train_stride, radius, geometry, geometry_stride, max_error))
        return rc;
    if (int rc = check_gated_pairs(epipolar, m, P, nq, nt, positions)) return rc;
    if (int rc = check_knn_sets(P, q, nq, t, nt)) return rc;
    if (list && (!out || !counts)) return fail(SIFT_HIP_ERR_INVALID, "k-NN list: null out or count");
    const KnnGate kg{epipolar,
                     gated_call(epipolar, query_stride, train_stride, radius, geometry, geometry_stride, max_error),
                     {}};
    if (!list) return knn_gated_fp16(m, P, q, nq, t, nt, positions, kg, false, k, idx, d2, stream);
    if (int rc = ensure_knn_scratch(m)) return rc;
    if (int rc = knn_gated_fp16(m, P, q, nq, t, nt, positions, kg, false, k, m->dKnnIdx, m->dKnnD, stream)) return rc;
    return knn_select(m, P, nq, k, m->dKnnIdx, m->dKnnD, max_distance, out, counts, stream);
}

}  // namespace

extern "C" {

int sift_hip_match_knn_guided_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                     const sift_hip_match_gate* gate, int k, int* idx, float* d2, void* stream) {
    return knn_gated_device(m, q, nq, t, nt, gate, k, idx, d2, (hipStream_t)stream);
}
int sift_hip_match_knn_epipolar_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                       const sift_hip_match_epipolar_gate* gate, int k, int* idx, float* d2,
                                       void* stream) {
    return knn_gated_device(m, q, nq, t, nt, gate, k, idx, d2, (hipStream_t)stream);
}
int sift_hip_match_knn_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                      const uint16_t* const* t, const int* nt, const sift_hip_match_positions* positions,
                                      int query_stride, int train_stride, float radius, int k, int* idx, float* d2,
                                      void* stream) {
    return knn_gated_batched(false, false, m, P, q, nq, t, nt, positions, query_stride, train_stride, radius, nullptr, 0,
                             0.f, k, 0.f, idx, d2, nullptr, nullptr, (hipStream_t)stream);
}
int sift_hip_match_knn_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                        const uint16_t* const* t, const int* nt,
                                        const sift_hip_match_positions* positions, int query_stride, int train_stride,
                                        float radius, const void* geometry, int geometry_stride_bytes, float max_error,
                                        int k, int* idx, float* d2, void* stream) {
    return knn_gated_batched(true, false, m, P, q, nq, t, nt, positions, query_stride, train_stride, radius, geometry,
                             geometry_stride_bytes, max_error, k, 0.f, idx, d2, nullptr, nullptr, (hipStream_t)stream);
}
int sift_hip_match_knn_list_guided_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                          const sift_hip_match_gate* gate, int k, float max_distance,
                                          sift_hip_dmatch* out, int* count, void* stream) {
    return knn_gated_list_device(m, q, nq, t, nt, gate, k, max_distance, out, count, (hipStream_t)stream);
}
int sift_hip_match_knn_list_epipolar_device(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                            const sift_hip_match_epipolar_gate* gate, int k, float max_distance,
                                            sift_hip_dmatch* out, int* count, void* stream) {
    return knn_gated_list_device(m, q, nq, t, nt, gate, k, max_distance, out, count, (hipStream_t)stream);
}
int sift_hip_match_knn_list_guided_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                           const uint16_t* const* t, const int* nt,
                                           const sift_hip_match_positions* positions, int query_stride,
                                           int train_stride, float radius, int k, float max_distance,
                                           sift_hip_dmatch* out, int* counts, void* stream) {
    return knn_gated_batched(false, true, m, P, q, nq, t, nt, positions, query_stride, train_stride, radius, nullptr, 0,
                             0.f, k, max_distance, nullptr, nullptr, out, counts, (hipStream_t)stream);
}
int sift_hip_match_knn_list_epipolar_batched(sift_hip_matcher_t m, int P, const uint16_t* const* q, const int* nq,
                                             const uint16_t* const* t, const int* nt,
                                             const sift_hip_match_positions* positions, int query_stride,
                                             int train_stride, float radius, const void* geometry,
                                             int geometry_stride_bytes, float max_error, int k, float max_distance,
                                             sift_hip_dmatch* out, int* counts, void* stream) {
    return knn_gated_batched(true, true, m, P, q, nq, t, nt, positions, query_stride, train_stride, radius, geometry,
                             geometry_stride_bytes, max_error, k, max_distance, nullptr, nullptr, out, counts,
                             (hipStream_t)stream);
}
int sift_hip_match_knn_guided_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                   const sift_hip_match_gate* gate, int k, int* idx_host, float* d2_host) {
    return knn_gated_host(m, q, nq, t, nt, gate, k, idx_host, d2_host);
}
int sift_hip_match_knn_epipolar_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                     const sift_hip_match_epipolar_gate* gate, int k, int* idx_host, float* d2_host) {
    return knn_gated_host(m, q, nq, t, nt, gate, k, idx_host, d2_host);
}
int sift_hip_match_knn_list_guided_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                        const sift_hip_match_gate* gate, int k, float max_distance,
                                        sift_hip_dmatch* out_host, int cap, int* count) {
    return knn_gated_list_host(m, q, nq, t, nt, gate, k, max_distance, out_host, cap, count);
}
int sift_hip_match_knn_list_epipolar_host(sift_hip_matcher_t m, const uint16_t* q, int nq, const uint16_t* t, int nt,
                                          const sift_hip_match_epipolar_gate* gate, int k, float max_distance,
                                          sift_hip_dmatch* out_host, int cap, int* count) {
    return knn_gated_list_host(m, q, nq, t, nt, gate, k, max_distance, out_host, cap, count);
}

}  // extern "C"
