// 3x3x3 scale-space extrema of the DoG pyramid for gfx950.
//
// Replaces the reference's sift_cuda/image_func/MatOps.cu.  Semantics follow
// OpenCV 4.x; the tests are the oracle's
// (oracle/sift_oracle.cpp isExtremum), so candidate lists are bit-exact.
#include "sift_kernels.h"
#include "sift_math.h"

namespace sift_amd {

// ---------------------------------------------------------------------------
// DoG + 3x3x3 extremum scan for one octave.  DoG planes D_d = G_{d+1} - G_d are
// formed in LDS for a 64 x 16 tile plus a 1-pixel halo (never written to HBM);
// every (layer 1..L, r, c) with border 5 is tested exactly as OpenCV's
// findScaleSpaceExtremaComputer: |v| > threshold and v >= (<=) all 26
// neighbours.  Hits are compacted with a wave ballot and one atomic per wave.
// Reference: MatOps.cu:39-181 (mask + full-volume CUB scan + scatter).
// ---------------------------------------------------------------------------
constexpr int EX_TW = 64;
constexpr int EX_TH = 16;
constexpr int EX_SW = EX_TW + 2;
constexpr int EX_SH = EX_TH + 2;
constexpr int EX_LIST = 512;  // per-workgroup candidate list (LDS)

// FLAT: the launches with thr = 0 (extrema_block's test_row).
template <bool FLAT>
__global__ __launch_bounds__(256) void k_extrema(OctGeom g, int L, int o, float thr, uint2* __restrict__ cand,
                                                 Counters* __restrict__ ctr, unsigned cap, long fs) {
    extern __shared__ float dog[];  // (L+2) planes of EX_SH x EX_SW
    g.base = fptr(g.base, blockIdx.z * fs);  // frame blockIdx.z
    cand = fptr(cand, blockIdx.z * fs);
    ctr = fptr(ctr, blockIdx.z * fs);
    const int tid = threadIdx.x;
    const int tile = xcd_tile(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
    const int x0 = (tile % gridDim.x) * EX_TW, y0 = (tile / gridDim.x) * EX_TH;
    const int W = g.W, H = g.H, pitch = g.pitch;
    constexpr int PS = EX_SH * EX_SW;
    __shared__ unsigned s_cnt, s_base;
    __shared__ uint2 s_list[EX_LIST];
    if (tid == 0) s_cnt = 0;

    for (int i = tid; i < PS; i += 256) {
        const int ly = i / EX_SW, lx = i - ly * EX_SW;
        const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float* p = g.base + (size_t)gy * pitch + gx;
            float prev = p[0];
            for (int d = 0; d < L + 2; d++) {
                const float next = p[(size_t)(d + 1) * g.planeStride];
                dog[d * PS + i] = next - prev;
                prev = next;
            }
        } else {
            for (int d = 0; d < L + 2; d++) dog[d * PS + i] = 0.f;
        }
    }
    __syncthreads();

    const int lane = tid & 63;
    const int total = EX_TH * EX_TW * L;
    for (int base = 0; base < total; base += 256) {
        const int i = base + tid;
        bool hit = false;
        int layer = 0, r = 0, c = 0;
        if (i < total) {
            layer = 1 + i / (EX_TH * EX_TW);
            const int rem = i - (layer - 1) * (EX_TH * EX_TW);
            const int ly = rem >> 6, lx = rem & 63;
            r = y0 + ly;
            c = x0 + lx;
            if (r >= 5 && r < H - 5 && c >= 5 && c < W - 5) {
                const float* cur = dog + layer * PS + (ly + 1) * EX_SW + (lx + 1);
                const float val = cur[0];
                if (fabsf(val) > thr) {
                    hit = true;
                    if constexpr (FLAT) {  // a constant in-layer 3x3 block is no candidate
                        hit = false;
#pragma unroll
                        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                            for (int dx = -1; dx <= 1; dx++) hit |= val != cur[dy * EX_SW + dx];
                    }
                    if (val > 0) {
#pragma unroll
                        for (int d = -1; d <= 1; d++)
#pragma unroll
                            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                                for (int dx = -1; dx <= 1; dx++) hit &= val >= cur[d * PS + dy * EX_SW + dx];
                    } else {
#pragma unroll
                        for (int d = -1; d <= 1; d++)
#pragma unroll
                            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                                for (int dx = -1; dx <= 1; dx++) hit &= val <= cur[d * PS + dy * EX_SW + dx];
                    }
                }
            }
        }
        // Hits go to a workgroup-local LDS list (wave ballot + one LDS atomic
        // per wave); the list is flushed with ONE global atomic per workgroup.
        const unsigned long long mask = __ballot(hit);
        if (mask) {
            unsigned basepos = 0;
            if (lane == 0) basepos = atomicAdd(&s_cnt, (unsigned)__popcll(mask));
            basepos = __shfl(basepos, 0);
            if (hit) {
                const unsigned pos = basepos + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
                const uint2 q = make_uint2((unsigned)(o << 8 | layer), (unsigned)(r << 16 | c));
                if (pos < EX_LIST) {
                    s_list[pos] = q;
                } else {  // plateau-heavy tile: spill straight to the global list
                    const unsigned gp = atomicAdd(&ctr->cand, 1u);
                    if (gp < cap)
                        cand[gp] = q;
                    else
                        atomicOr(&ctr->overflow, 1u);
                }
            }
        }
    }
    __syncthreads();
    const unsigned nl = min(s_cnt, (unsigned)EX_LIST);
    if (tid == 0) s_base = nl ? atomicAdd(&ctr->cand, nl) : 0u;
    __syncthreads();
    for (unsigned k = tid; k < nl; k += 256) {
        const unsigned pos = s_base + k;
        if (pos < cap)
            cand[pos] = s_list[k];
        else
            atomicOr(&ctr->overflow, 1u);
    }
}

// ---------------------------------------------------------------------------
// Register-streaming extrema for L = 1..6 (the common case; k_extrema above
// serves larger L).  Four columns per lane: one wave covers a 256-column x
// EX4_TR-row strip, rows streaming top to bottom with EX4_AHEAD rows' loads in
// flight, with
// 16-byte loads (one buffer_load_dwordx4 per row and plane), plus one dword
// per row and plane for the strip's outer neighbours (lane 0: column x0-1,
// lane 63: column x0+256).  Only the planes G1 .. G(L+1) are streamed: per row
// the L inner DoG layers D1 .. DL are formed in registers
// and kept in a 3-row ring; a tested row takes the vertical max/min of its
// three rows per column, then the horizontal 3-max in-lane, with the columns
// across lane boundaries brought in by one DPP move each (lane 0 / 63 keep
// their own outer column as the DPP's old value).  "v >= all 26 neighbours"
// is exactly "v == max of the 3x3x3 block" (the block contains v), so the
// decision per pixel is OpenCV's and the oracle's: |v| > threshold and
// v >= (<=) all 26, with no LDS staging.
//
// The outer DoG layers D0 = G1 - G0 and D(L+1) = G(L+2) - G(L+1) are compared
// against by layer 1 and layer L alone, so G0 and G(L+2) are not streamed (a
// third of the bytes at L = 3).  The stream tests layers 1 and L against the
// inner layers only: such a hit is provisional (~0.6 % of the pixels), and the
// nine outer values it still has to dominate are loaded and compared when the
// workgroup's list is flushed (outer_ok) -- the same float subtraction and the
// same comparisons as in the stream, so the candidate set is the same.
// ---------------------------------------------------------------------------
constexpr int EX4_LIST = 2048;  // per-workgroup candidate list (LDS): a 256 x 32 x L block can hold
                                // ~7 % extrema on textured frames; overflow spills to HBM
// Columns per lane of the extrema strips.  (Measured alternative, round 3: 2
// columns per lane, 137 VGPRs / 3 waves per SIMD: 266-268 vs 252 us per
// 16-frame launch.)
constexpr int kExCpl = 4;
constexpr int EX4_COLS = 64 * kExCpl;  // columns per wave

// One workgroup = 4 waves stacked vertically over a 256-column strip: block
// `tile` of the octave (strips across; the caller picks the XCD order).
// A wave tests NB * EX4_TR consecutive rows as one stream (the 3-row DoG ring
// and the loads ahead carry across its EX4_TR-row steps), so the two halo
// rows above and below are read once per NB * EX4_TR rows instead of once per
// EX4_TR: strips of 6 rows read 8 (1.20x algorithmic HBM bytes measured at
// 16 frames, round-3 verdict), 24-row streams read 26.
template <int LT, bool FLAT, int EX4_TR, int EX4_AHEAD, int NB = 1, int CPL = kExCpl>
__device__ __forceinline__ void extrema_block(const OctGeom& g, int o, float thr, uint2* __restrict__ cand,
                                              Counters* __restrict__ ctr, unsigned cap, int tile, int strips,
                                              uint2* s_list, unsigned& s_cnt, unsigned& s_keep, unsigned& s_base) {
    // NG planes in the octave; the stream reads NP of them (G1 .. G(LT+1)) and
    // forms the ND inner DoG layers (index d: layer d + 1).
    constexpr int NG = LT + 3, NP = LT + 1, ND = LT;
    static_assert(CPL * LT <= 31 && (CPL == 2 || CPL == 4), "hit bits per row");
    static_assert(NB == 1 || (EX4_TR % 3 == 0 && EX4_TR % (EX4_AHEAD + 1) == 0),
                  "multi-step streams: the ring and the load sets repeat every EX4_TR rows");
    typedef float f4 __attribute__((ext_vector_type(CPL)));  // CPL columns of one lane
    constexpr int EX4_COLS = 64 * CPL;                          // columns per wave
    constexpr int TR = EX4_TR * NB;                             // rows per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (tile % strips) * EX4_COLS, y0 = ((tile / strips) * 4 + wave) * TR;
    const int W = g.W, H = g.H, pitch = g.pitch;
    const int xl = x0 + CPL * lane;
    const int xe = min(max(lane == 0 ? x0 - 1 : x0 + EX4_COLS, 0), W - 1);
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        g.base, 0, (int)min((long)NG * g.planeStride * 4, 0x7fffffffL), 0x00020000);
    if (tid == 0) s_cnt = s_keep = 0;
    __syncthreads();

    bool colOK[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) colOK[c] = xl + c >= 5 && xl + c < W - 5;

    // Ring slot: DoG of the lane's 4 columns and of its outer column, per plane.
    f4 rd[3][ND];
    float re[3][ND];
    // Raw rows in flight: EX4_AHEAD + 1 register sets, loads issued EX4_AHEAD
    // rows ahead of the row being formed.
    f4 rv[EX4_AHEAD + 1][NP];
    float rev[EX4_AHEAD + 1][NP];
    // Lanes whose columns start past the octave's width (the last strip of a
    // row overhangs it: 1920 = 7.5 strips) and the lanes that do not use the
    // outer column (all but lanes 0 and 63) load from an offset past the
    // buffer: the hardware returns 0 without a memory request.
#if defined(SIFT_EX_DIAG) && (SIFT_EX_DIAG == 1 || SIFT_EX_DIAG == 3)  // traffic variants (wrong results): no outer-column loads
    const bool l4 = xl < W, le = false;
#else
    const bool l4 = xl < W, le = lane == 0 || lane == 63;
#endif
    auto issue_row = [&](int y, f4 (&v)[NP], float (&e)[NP]) {
#if defined(SIFT_EX_DIAG) && (SIFT_EX_DIAG == 2 || SIFT_EX_DIAG == 3)  // traffic variants: halo rows -> the wave's own rows
        y = min(max(y, y0), y0 + TR - 1);
#endif
        const int yc = min(max(y, 0), H - 1);
        const unsigned off4 = l4 ? (unsigned)(yc * pitch + xl) * 4u : 0x80000000u;
        const unsigned offe = le ? (unsigned)(yc * pitch + xe) * 4u : 0x80000000u;
#pragma unroll
        for (int d = 0; d < NP; d++) {
            const int so = (int)((long)(d + 1) * g.planeStride * 4);
            if constexpr (CPL == 4)
                v[d] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off4, so, 0));
            else
                v[d] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b64(rsrc, off4, so, 0));
            e[d] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, offe, so, 0));
        }
    };
    // The outer-layer half of the test for a provisional hit (layer 1: against
    // D0; layer LT: against D(LT+1); LT = 1: both): v > 0 stays iff v >= the
    // nine outer values, v < 0 iff v <= them.  A hit is >= 5 pixels from every
    // border, so the 3x3 patches are inside the planes.  Every row of a patch
    // is a cache line of its own in both planes, and by now the rows the block
    // streamed have left the L2, so the test goes in two steps: the centre row
    // first (with v: three lines; it rejects 57 % of the C2 frame's provisional
    // hits, the whole patch 77 %), then the rows above and below for the lanes
    // still in.  The loads of a step are all issued before the first is used
    // and none is conditional (a conditional load is a branch plus a full
    // wait): a lane with nothing to test loads from past the buffer (0, no
    // memory request).  Returns `true` for a hit that is not provisional.
    auto outer_ok = [&](bool have, int l, unsigned rc) -> bool {
        const unsigned ps4 = (unsigned)(g.planeStride * 4);
        const unsigned at = (unsigned)((int)(rc >> 16) * pitch + (int)(rc & 0xffffu)) * 4u;
        constexpr unsigned kPast = 0x90000000u;  // stays past the buffer with the patch and plane offsets added
        constexpr int NO = LT == 1 ? 2 : 1;      // outer layers to compare against
        const bool prov = have && (l == 1 || l == LT);
        unsigned lo[NO];  // byte offset of (r, c) in the lower plane of each outer DoG layer
        if constexpr (LT == 1) {
            lo[0] = at;
            lo[1] = at + 2u * ps4;
        } else {
            lo[0] = at + (l == 1 ? 0u : (unsigned)(LT + 1) * ps4);
        }
        auto ld = [&](unsigned off) {
            return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0));
        };
        // Rows r + dy (dy in DY) of the outer layers, as `form` makes them: one float subtraction.
        auto rows = [&](bool on, const int (&DY)[2], int ndy, float& mx, float& mn) {
            float a[NO][2][3], b[NO][2][3];
#pragma unroll
            for (int n = 0; n < NO; n++)
#pragma unroll
                for (int j = 0; j < ndy; j++)
#pragma unroll
                    for (int dx = 0; dx < 3; dx++) {
                        const unsigned off = on ? lo[n] + (unsigned)(DY[j] * pitch + dx - 1) * 4u : kPast;
                        a[n][j][dx] = ld(off);
                        b[n][j][dx] = ld(off + ps4);
                    }
            mx = mn = b[0][0][0] - a[0][0][0];
#pragma unroll
            for (int n = 0; n < NO; n++)
#pragma unroll
                for (int j = 0; j < ndy; j++)
#pragma unroll
                    for (int dx = 0; dx < 3; dx++) {
                        const float dv = b[n][j][dx] - a[n][j][dx];
                        mx = fmaxf(mx, dv);
                        mn = fminf(mn, dv);
                    }
        };
        const unsigned vo = prov ? at + (unsigned)l * ps4 : kPast;
        const float v0 = ld(vo), v1 = ld(vo + ps4);
        float mx, mn;
        rows(prov, {0, 0}, 1, mx, mn);
        const float v = v1 - v0;
        const bool in = prov && (v > 0 ? mx <= v : mn >= v);
        rows(in, {-1, 1}, 2, mx, mn);
        return !prov || (in && (v > 0 ? mx <= v : mn >= v));
    };
    // Candidates of one tested row: one LDS reservation per row with hits;
    // each lane's slot offset is the exclusive prefix of the per-lane hit
    // counts, taken from ballots of the count's bits (count <= 4 * LT < 32).
    auto emit_row = [&](int r, unsigned hits) {
        if (!__ballot(hits != 0)) return;  // wave-uniform
        const unsigned cnt = (unsigned)__popc(hits);
        unsigned excl = 0, tot = 0;
#pragma unroll
        for (int b = 0; b < 5; b++) {
            const unsigned long long bm = __ballot((cnt >> b) & 1u);
            excl += __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u)) << b;
            tot += (unsigned)__popcll(bm) << b;
        }
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&s_cnt, tot);
        unsigned pos = __builtin_amdgcn_readfirstlane(base) + excl;
        for (unsigned m = hits; m; m &= m - 1u, pos++) {
            const int f = __builtin_ctz(m), l = f / CPL + 1, c = f % CPL;
            const uint2 q = make_uint2((unsigned)(o << 8 | l), (unsigned)(r << 16 | (xl + c)));
            if (pos < EX4_LIST) {
                s_list[pos] = q;
            } else if (outer_ok(true, l, q.y)) {  // plateau-heavy tile: spill straight to the global list
                const unsigned gp = atomicAdd(&ctr->cand, 1u);
                if (gp < cap)
                    cand[gp] = q;
                else
                    atomicOr(&ctr->overflow, 1u);
            }
        }
    };
    auto test_row = [&](int r, int A, int B, int C) -> unsigned {
        const bool rowOK = r >= 5 && r < H - 5;
        f4 hx[ND], hn[ND];
#pragma unroll
        for (int d = 0; d < ND; d++) {
            f4 vx, vn;
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                vx[c] = fmaxf(fmaxf(rd[A][d][c], rd[B][d][c]), rd[C][d][c]);
                vn[c] = fminf(fminf(rd[A][d][c], rd[B][d][c]), rd[C][d][c]);
            }
            const float ex = fmaxf(fmaxf(re[A][d], re[B][d]), re[C][d]);
            const float en = fminf(fminf(re[A][d], re[B][d]), re[C][d]);
            const float lx = dpp_left_or(ex, vx[CPL - 1]), ln = dpp_left_or(en, vn[CPL - 1]);
            const float rx = dpp_right_or(ex, vx[0]), rn = dpp_right_or(en, vn[0]);
            // Column c's horizontal neighbours: c-1 and c+1 (across the lane
            // edges: the DPP values), max/min in the same operation order.
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                const float xa = c == 0 ? lx : vx[c - 1], xb = c == CPL - 1 ? rx : vx[c + 1];
                const float na = c == 0 ? ln : vn[c - 1], nb = c == CPL - 1 ? rn : vn[c + 1];
                hx[d][c] = fmaxf(fmaxf(xa, vx[c]), xb);
                hn[d][c] = fminf(fminf(na, vn[c]), nb);
            }
        }
        unsigned hits = 0;  // bit (l - 1) * CPL + c
#pragma unroll
        for (int l = 1; l <= LT; l++)
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                // Layer l is index l - 1; its neighbours among the inner layers
                // (layers 1 and LT lack one: provisional, outer_ok has the rest).
                const float v = rd[B][l - 1][c];
                float M = hx[l - 1][c], m = hn[l - 1][c];
                if (l > 1) M = fmaxf(M, hx[l - 2][c]), m = fminf(m, hn[l - 2][c]);
                if (l < LT) M = fmaxf(M, hx[l][c]), m = fminf(m, hn[l][c]);
                // M >= v >= m always (v is one of them), so "v >= all" is v == M;
                // |v| > thr >= 0 excludes v == 0, and the sign picks the test.
                bool h = rowOK && colOK[c] && fabsf(v) > thr && v == (v > 0 ? M : m);
                // FLAT (the launches with thr = 0): a hit whose in-layer 3x3 block
                // is constant (hx == hn) is dropped.  At thr = 0 every sample of a
                // flat non-zero region is such a plateau of rounding residue
                // (OpenCV makes them candidates), and adjustLocalExtrema can keep
                // none -- dxx = dyy = dxy = 0 and dx = dy = 0, so the 3x3 system is
                // singular (solve returns 0, the iteration stays in place) and the
                // 2-D det = 0 fails det > 0.  They only filled the candidate list
                // (overflow bit 0).  One compare per sample: 242 -> 250-254 us per
                // 16-frame C2 launch when always on, so launches with thr >= 1,
                // where such a block would have to be constant at |v| > 1, run
                // without it.
                if constexpr (FLAT) h = h && hx[l - 1][c] != hn[l - 1][c];
                hits |= (unsigned)h << ((l - 1) * CPL + c);
            }
        return hits;
    };

    if (y0 < H) {
        // Strip row m = 0 .. TR + 1 (image row y0 - 1 + m) is loaded into raw
        // set m % NS; once formed, its set is reloaded with strip row m + NS
        // (rows past the image: clamped reads, never tested).
        constexpr int NS = EX4_AHEAD + 1;
        // Streams end at the image's last tested row (H - 6): no load or test
        // past it (uniform).
        const int nsteps = NB == 1 ? 1 : min(NB, (min(H - 5, y0 + TR) - y0 + EX4_TR - 1) / EX4_TR);
        const int nr = nsteps * EX4_TR + 2, yb = y0 + nsteps * EX4_TR;
        // Odd waves stream bottom to top.  Vertically adjacent waves share
        // two rows (each one's halo row is the other's edge row), and a row
        // a wave loads at the start of its stream was loaded by a same-way
        // neighbour at the end of its stream: by then the XCD's L2 (4 MiB
        // against ~20 MB streamed meanwhile) had dropped it, and the halo
        // rows came back over the fabric -- 1.19x the algorithmic bytes (the
        // Infinity Cache served them, FETCH_SIZE counted them).  With
        // alternating directions every shared row is loaded by both waves at
        // the same end of their streams.  The 3x3x3 test is symmetric in
        // the rows (exact max / min), so candidates are unchanged.
        const bool up = (wave & 1) != 0;
        auto strip_row = [&](int m) { return up ? yb - m : y0 - 1 + m; };   // image row of strip row m
        auto tested_row = [&](int k) { return up ? yb - 1 - k : y0 + k; };  // image row of tested row k
        auto form = [&](int m, int km, f4 (&d4)[ND], float (&de)[ND]) {  // km = m % NS (compile-time)
#pragma unroll
            for (int d = 0; d < ND; d++) {
                d4[d] = rv[km][d + 1] - rv[km][d];
                de[d] = rev[km][d + 1] - rev[km][d];
            }
            if (m + NS < nr) issue_row(strip_row(m + NS), rv[km], rev[km]);
        };
#pragma unroll
        for (int m = 0; m < NS; m++) issue_row(strip_row(m), rv[m], rev[m]);
        form(0, 0, rd[0], re[0]);
        form(1, 1 % NS, rd[1], re[1]);
        // Strip row k + 2 enters ring slot (k + 2) % 3, tested row k is tested.
#pragma unroll 1
        for (int kb = 0; kb < nsteps * EX4_TR; kb += EX4_TR) {
#pragma unroll
            for (int k6 = 0; k6 < EX4_TR; k6++) {
                const int k = kb + k6;
                const int A = k6 % 3, B = (k6 + 1) % 3, C = (k6 + 2) % 3;
                form(k + 2, (k6 + 2) % NS, rd[C], re[C]);
                const int r = tested_row(k);
                emit_row(r, test_row(r, A, B, C));
            }
        }
    }
    __syncthreads();
    // Flush.  Pass 1 resolves the provisional entries: a survivor takes its
    // slot among the workgroup's survivors (ballot per wave, one LDS add) into
    // the free upper half of its first word (o << 8 | l < 2^16, slot <
    // EX4_LIST <= 2^16); a rejected entry becomes ~0.  Then one global atomic
    // reserves the survivors' run, and pass 2 writes them.
    static_assert(EX4_LIST <= 65536 && kMaxOctaves <= 256, "slot and o << 8 | l share a word");
    const unsigned nl = min(s_cnt, (unsigned)EX4_LIST);
    for (unsigned k0 = 0; k0 < nl; k0 += 256) {  // uniform
        const unsigned k = k0 + tid;
        const bool have = k < nl;
        const uint2 q = have ? s_list[k] : make_uint2(0u, 0u);
        const bool keep = outer_ok(have, (int)(q.x & 0xffu), q.y) && have;
        const unsigned long long km = __ballot(keep);
        unsigned base = 0;
        if (lane == 0 && km) base = atomicAdd(&s_keep, (unsigned)__popcll(km));
        const unsigned slot = __builtin_amdgcn_readfirstlane(base) +
                              __builtin_amdgcn_mbcnt_hi((unsigned)(km >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)km, 0u));
        if (have) s_list[k].x = keep ? q.x | slot << 16 : ~0u;
    }
    __syncthreads();
    if (tid == 0) s_base = s_keep ? atomicAdd(&ctr->cand, s_keep) : 0u;
    __syncthreads();
    for (unsigned k = tid; k < nl; k += 256) {
        const uint2 q = s_list[k];
        if (q.x == ~0u) continue;
        const unsigned pos = s_base + (q.x >> 16);
        if (pos < cap)
            cand[pos] = make_uint2(q.x & 0xffffu, q.y);
        else
            atomicOr(&ctr->overflow, 1u);
    }
}

// All octaves of the frame in one launch (L = 1..6): blocks [start[o],
// start[o+1]) take octave o, with tall strips (6 rows per wave) where they
// still give >= 1024 waves, else 2 rows per wave (small octaves are
// latency-bound and want waves; tools/kernel_bench: 1920x1200 16.7 us at 6
// rows vs 19.8 at 2; 960x600 9.2 us at 2 rows vs 10.8 at 6).
constexpr int kExTallMin = 2048;  // single frames: 6-row wave strips from this many strips per launch, else 2-row (1920x1200: 1600 -> 2-row, 26.4 -> 25.5 us); batches: 1024
constexpr int kExStream = 2;  // 6-row steps per tall wave stream (12 rows: 247 vs 251 us per 16-frame launch; 18, 24 rows slower)
struct ExtremaPlan {
    int start[kMaxOctaves + 1];  // start[nOct] = blocks per frame
    int strips[kMaxOctaves];
    int tall[kMaxOctaves];
};

template <int LT, bool FLAT>
__global__ __launch_bounds__(256) void k_extrema_all(PyrDesc pyr, ExtremaPlan plan, float thr,
                                                     uint2* __restrict__ cand, Counters* __restrict__ ctr,
                                                     unsigned cap, long fs) {
    __shared__ unsigned s_cnt, s_keep, s_base;
    __shared__ uint2 s_list[EX4_LIST];
    // Frame-major block order over all frames, XCD-aware: each XCD takes a
    // contiguous run of (frame, octave, strip block), so vertically adjacent
    // blocks (shared halo rows) meet in the same L2.
    const int per = plan.start[pyr.nOct];
    const int t = xcd_tile(blockIdx.x, gridDim.x);
    const int f = t / per, b = t - f * per;
    int o = 0;
    while (o + 1 < pyr.nOct && b >= plan.start[o + 1]) o++;
    OctGeom g = pyr.oct[o];
    g.base = fptr(g.base, f * fs);
    cand = fptr(cand, f * fs);
    ctr = fptr(ctr, f * fs);
    const int blk = b - plan.start[o];
    if (plan.tall[o])
        extrema_block<LT, FLAT, 6, 2, kExStream>(g, o, thr, cand, ctr, cap, blk, plan.strips[o], s_list, s_cnt, s_keep, s_base);
    else
        extrema_block<LT, FLAT, 2, 2>(g, o, thr, cand, ctr, cap, blk, plan.strips[o], s_list, s_cnt, s_keep, s_base);
}

// Octave o alone, for L > 6 (LDS-staged k_extrema).
void launch_extrema(const PyrDesc& pyr, int o, float threshold, uint2* cand, Counters* ctr, unsigned cap,
                    const Frames& fr, hipStream_t s) {
    const OctGeom& g = pyr.oct[o];
    dim3 grid((g.W + EX_TW - 1) / EX_TW, (g.H + EX_TH - 1) / EX_TH, fr.nf);
    const size_t lds = sizeof(float) * (size_t)(pyr.L + 2) * EX_SH * EX_SW;
    if (threshold == 0.f)
        hipLaunchKernelGGL((k_extrema<true>), grid, dim3(256), lds, s, g, pyr.L, o, threshold, cand, ctr, cap,
                           fr.stride);
    else
        hipLaunchKernelGGL((k_extrema<false>), grid, dim3(256), lds, s, g, pyr.L, o, threshold, cand, ctr, cap,
                           fr.stride);
}

bool launch_extrema_all(const PyrDesc& pyr, float threshold, uint2* cand, Counters* ctr, unsigned cap,
                        const Frames& fr, hipStream_t s) {
    if (pyr.L < 1 || pyr.L > 6) return false;
    ExtremaPlan plan{};
    int total = 0;
    for (int o = 0; o < pyr.nOct; o++) {
        const OctGeom& g = pyr.oct[o];
        const int strips = (g.W + EX4_COLS - 1) / EX4_COLS;
        // Frames of a batch count too: each brings its own strips.
        // (8, 12 or 20 rows per wave for batches: 147, 149, 582 us vs 131 at 6.)
        const bool tall = strips * ((g.H + 5) / 6) * fr.nf >= (fr.nf > 1 ? 1024 : kExTallMin);
        const int tr = tall ? 6 * kExStream : 2;
        plan.start[o] = total;
        plan.strips[o] = strips;
        plan.tall[o] = tall;
        total += strips * ((g.H + 4 * tr - 1) / (4 * tr));
    }
    plan.start[pyr.nOct] = total;
    const bool flat = threshold == 0.f;  // drop in-layer-flat hits (extrema_block's test_row)
    switch (pyr.L) {
#define SIFT_EX_CASE(LV) \
    case LV: {                                                                                                      \
        if (flat)                                                                                                   \
            hipLaunchKernelGGL((k_extrema_all<LV, true>), dim3(total * fr.nf), dim3(256), 0, s, pyr, plan, threshold, \
                               cand, ctr, cap, fr.stride);                                                          \
        else                                                                                                        \
            hipLaunchKernelGGL((k_extrema_all<LV, false>), dim3(total * fr.nf), dim3(256), 0, s, pyr, plan,         \
                               threshold, cand, ctr, cap, fr.stride);                                               \
        break;                                                                                                      \
    }
        SIFT_EX_CASE(1)
        SIFT_EX_CASE(2)
        SIFT_EX_CASE(3)
        SIFT_EX_CASE(4)
        SIFT_EX_CASE(5)
        SIFT_EX_CASE(6)
#undef SIFT_EX_CASE
    }
    return true;
}

}  // namespace sift_amd
