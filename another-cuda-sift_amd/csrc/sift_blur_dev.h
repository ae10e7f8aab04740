// ---------------------------------------------------------------------------
// Device side of the blur tile kernels (blur.hip): the tile's constants and
// switches, the job record and blur_tile, the body every k_blur / k_blur2
// instantiation inlines.
//
// Separable Gaussian blur, one 64 x BLUR_TH output tile per workgroup of
// BLUR_NW waves (each BLUR_TH / BLUR_NW rows of the column pass),
// instantiated per radius R (taps 2R+1) so every tap loop is fully unrolled.
// The (BLUR_TH+2R) x (64+2R) input tile (reflect-101 borders) is staged once
// in LDS; the blur of an octave's plane L also writes the next octave's base
// plane (its even rows and columns, OpenCV's INTER_NEAREST half-size resize).
// Row pass: 16 threads per row, each keeps a (2R+4)-float register window
// (ds_read_b128) and runs 4 independent fma chains (4 adjacent outputs).
// Column pass: one column per lane, 8 rows per thread, (2R+8)-float window.
// Row:    s = 0; s = fma(in[x-R+k], w[k], s), k = 0..2R          (2R+1 > 5)
//         s = in[x]*w[R]; s = fma(in[x-k]+in[x+k], w[R+k], s)      (2R+1 <= 5)
// Column: s = fma(mid[y], w[R], 0); s = fma(mid[y+k]+mid[y-k], w[R+k], s)
// Reference: Filter.cu:8-51 (no LDS, vertical first, modulo per tap).
// ---------------------------------------------------------------------------
#pragma once
#include "sift_kernels.h"
#include "sift_math.h"

namespace sift_amd {

// (a.y, b.x) in one v_pk_mov_b32 (the compiler otherwise emits two v_mov).
__device__ __forceinline__ f32x2 pk_mov_hi_lo(f32x2 a, f32x2 b) {
    f32x2 r;
    __asm__("v_pk_mov_b32 %0, %1, %2 op_sel:[1,0]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
constexpr int BLUR_TW = 64;
constexpr int BLUR_TH = 64;  // tile height: 64 (8 waves) beat 32 by 3-5 % of frame time (round 1)
// Waves per workgroup NW (a template parameter): 4 for launches of >= 2048
// tiles (octave-0 launches of frame batches: 2-8 % faster per launch, and a
// workgroup pair holds half of a CU's wave slots, so the other stream's
// keypoint kernels co-reside), 8 for the small launches (more waves per tile
// hide their latency better).
constexpr int kBlurBigTiles = 2048;
static_assert(BLUR_TH % 32 == 0, "blur tile height: 8-row column blocks for 4 or 8 waves");
inline int blur_waves(int tiles) { return tiles >= kBlurBigTiles ? 4 : 8; }

// One blur launch's job: plane src -> dst, optionally the next octave's base
// plane (dec), the pixel range and the frame counters.
struct BlurJob {
    const void* src;  // float, or uint8_t for the frame's first blur of an 8-bit frame
    float* dst;
    DecOut dec;
    unsigned* range_keys;
    Counters* zero_ctr;
    int spitch, W, H, dpitch, tilesX, ntiles;
    int nf;         // frames; the launch has nf * ntiles tiles of this job
    long sfs, dfs;  // byte strides between frames: source; dst / dec / range_keys / zero_ctr
    Taps taps;
};

// LDS row pitch of a blur tile (floats).  The row pass stores each lane's 4
// outputs with ds_write_b128, whose 8-lane groups put blocks of one row
// beside the same blocks of the next row: conflict-free exactly when the pitch
// is 16 mod 32 dwords (the old pitch, 64 + 2R rounded up to 4, was only for
// R = 8: SQ_LDS_BANK_CONFLICT 16-21 % of the LDS cycles at R = 5, 6, 10, 13).
// A multiple-of-16 pitch also lets the column pass fetch (y, y + 4) pairs with
// one ds_read2st64_b32.
constexpr bool kBlurIW16 = true;
// Tiles with every input in the image read their staging rows as aligned
// 16-byte loads of columns x0 - ORG .. x0 + 63 + ORG, ORG = 8 for radius <= 8
// and R rounded up to a multiple of 4 above (12 at R = 10, 16 at R = 13): a
// quarter of the load instructions of the per-column dword staging.  The LDS
// tile starts at column x0 - ORG whichever staging ran.
// (Measured alternative, round 3: the per-column dword staging for R > 8 --
// the paired R = 13 launch 115.7 vs 113.0 us per 16 frames.)
constexpr bool kBlurX4Ld = true;
constexpr bool kBlurX4LdBig = true;  // the 16-byte staging for radii > 8 too
constexpr int kBlurX4LdMaxR = 24;
// Full tiles store their output rows as 16-byte stores (each wave's 8-row
// blocks transposed through the freed LDS tile) instead of one dword per
// lane and row: a quarter of the store instructions.
constexpr bool kBlurX4St = true;
// Interior-tile staging by LDS-DMA (global_load_lds_dwordx4) instead of
// 16-byte loads into VGPRs + ds_write_b128.
// (Measured alternative, round 2: VGPR staging -- the x4 launches 1-3 % slower.)
constexpr bool kBlurDma = true;
template <int R>
constexpr int blur_org() {  // tile column 0 = image column x0 - ORG
    return kBlurX4Ld && R <= 8 ? 8 : kBlurX4Ld && kBlurX4LdBig && R <= kBlurX4LdMaxR ? (R + 3) & ~3 : R;
}
// Radius 11..24 with the dword staging: pitch 112 (16 mod 32, conflict-free
// row-pass stores).  With the 16-byte staging (default) the rows stay unpadded
// (R = 13: 96 floats) so the interior tiles stage by LDS-DMA: the paired
// R = 13 launch 115.7 -> 113.0 us per 16 frames (tools/r3_blur_x4_ab.sh).
constexpr bool kBlurIW112 = false;
template <int R>
constexpr int blur_iw() {  // radius 9, 10: the next 16-mod-32 pitch (112) costs a workgroup per CU -- kept at 64 + 2R
    return kBlurIW16 && R <= 8 ? ((BLUR_TW + 2 * blur_org<R>() + 15) / 32) * 32 + 16
           : kBlurIW112 && R >= 11 && R <= 24 ? 112
                                                   : (BLUR_TW + 2 * blur_org<R>() + 3) & ~3;
}
template <int R>
constexpr int blur_lds_floats() {
    return blur_iw<R>() * (BLUR_TH + 2 * R) + 4;
}

// Tile `blk` of job J's nf * ntiles (64 x 32 outputs; frame-major, XCD order)
// with LDS `in`.  T = float, or uint8_t
// for a caller's 8-bit frame read by the frame's first blur (OpenCV converts
// CV_8U to float exactly, so the planes are those of the float frame with the
// same values).

template <int R, typename T, int NWAVES>
__device__ __forceinline__ void blur_tile(const BlurJob& J, int blk, float* __restrict__ in) {
    constexpr int BLUR_NW = NWAVES;                   // waves per workgroup
    constexpr int BLUR_CB = BLUR_TH / (8 * BLUR_NW);  // 8-row column-pass blocks per wave
    constexpr int IW = blur_iw<R>();                 // LDS row stride (floats)
    constexpr int IH = BLUR_TH + 2 * R;
    constexpr int ORG = blur_org<R>();               // LDS column 0 = image column x0 - ORG
    constexpr int SA = (ORG - R) & ~3, SS = (ORG - R) & 3;  // row window: aligned start, shift
    constexpr int NW = (SS + 2 * R + 4 + 3) / 4;     // float4 reads per row window
    static_assert(BLUR_TW - 4 + SA + 4 * NW <= IW, "row window inside the LDS row");
    const int t = xcd_tile(blk, J.ntiles * J.nf);
    const int f = t / J.ntiles, tile = t - f * J.ntiles;
    const T* __restrict__ src = fptr(static_cast<const T*>(J.src), f * J.sfs);
    float* __restrict__ dst = fptr(J.dst, f * J.dfs);
    float* __restrict__ dec_out = J.dec.p ? fptr(J.dec.p, f * J.dfs) : nullptr;
    unsigned* __restrict__ range_keys = J.range_keys ? fptr(J.range_keys, f * J.dfs) : nullptr;
    Counters* __restrict__ zero_ctr = J.zero_ctr ? fptr(J.zero_ctr, f * J.dfs) : nullptr;
    const int spitch = J.spitch, W = J.W, H = J.H, dpitch = J.dpitch;
    const Taps& taps = J.taps;
    // Row-pass results (`mid`, pitch IW) overwrite their own input row of
    // `in` in place: a row is read and written only by the same 16 lanes of
    // one wave, whose LDS reads complete before its writes (in-order LDS per
    // wave), so one tile of LDS serves both passes (more workgroups per CU).
    float* const mid = in;
    const int x0 = (tile % J.tilesX) * BLUR_TW, y0 = (tile / J.tilesX) * BLUR_TH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // The frame's first blur also zeroes the frame counters (no memset node).
    // (Counters.pad[1] keeps its host-results request half: set by a host
    // frame's staging copy before this kernel, HostOut.)
    if (zero_ctr && tile == 0 && tid < (int)(sizeof(Counters) / 4))
        reinterpret_cast<unsigned*>(zero_ctr)[tid] =
            tid == offsetof(Counters, pad[1]) / 4 ? zero_ctr->pad[1] & ~((1u << kHostReqShift) - 1) : 0u;

    // Stage the input tile row by row: wave w takes rows w, w+4, ...; lane l
    // columns l and 64+l.  A row's source offset is wave-uniform (SGPR,
    // reflected in scalar code) and a lane's column offset is the same for
    // every row, so a staging load costs no vector address arithmetic.  All
    // loads are issued before the first LDS store.
    {
        constexpr int RW = BLUR_TW + 2 * R;  // <= 128: two column chunks
        constexpr int RPW = (IH + BLUR_NW - 1) / BLUR_NW;  // rows per wave
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        const bool single = W > R + 1 && H > R + 1;  // one reflection suffices
        auto refl = [&](int p, int len) {
            if (single) {
                // One bounce is exact for every input of an in-image output
                // (|offset| <= R < len); tile positions past the image edge feed
                // only discarded outputs, so clamping them just keeps the read
                // in bounds.
                p = p < 0 ? -p : (p >= len ? 2 * len - 2 - p : p);
                return min(max(p, 0), len - 1);
            }
            return reflect101(p, len);
        };
        const int gx0 = refl(x0 - R + lane, W), gx1 = refl(x0 - R + 64 + min(lane, RW - 65), W);
        constexpr int ES = (int)sizeof(T);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<T*>(src), 0, (int)min((long)spitch * H * ES, 0x7fffffffL), 0x00020000);
        const unsigned c0 = (unsigned)gx0 * ES, c1 = (unsigned)gx1 * ES;
        const int rowB = spitch * ES;  // bytes per source row
        float v0[RPW], v1[RPW];
        auto ld = [&](int i, int roff) {
            if constexpr (ES == 1) {
                v0[i] = (float)__builtin_amdgcn_raw_buffer_load_b8(rsrc, c0, roff, 0);
                v1[i] = (float)__builtin_amdgcn_raw_buffer_load_b8(rsrc, c1, roff, 0);
            } else {
                v0[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, c0, roff, 0));
                v1[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, c1, roff, 0));
            }
        };
        constexpr int QW = (BLUR_TW + 2 * ORG) / 4;  // float4s per staged row
        const bool x4 = ES == 4 && ORG % 4 == 0 && ORG >= R && x0 >= ORG &&
                        x0 + BLUR_TW + ORG <= W && y0 - R >= 0 && y0 - R + IH <= H;  // uniform
        if (x4) {
            // Interior tile: 16-byte loads of the QW-float4 rows, all in
            // flight before the first LDS store.
            static_assert(!(ES == 4 && ORG % 4 == 0) || 4 * QW <= IW, "x4 staging row inside the LDS row");
            constexpr int NQ = QW * IH, NT = 64 * BLUR_NW, QPT = (NQ + NT - 1) / NT;
            const int rb0 = (y0 - R) * spitch + x0 - ORG;
            if constexpr (kBlurDma && IW == 4 * QW) {
                // LDS-DMA (the LDS rows are unpadded: float4 q of the tile goes
                // to LDS float4 q; global_load_lds_dwordx4: a wave's 64 lanes
                // fill 1 KiB at M0), no VGPR round trip and no ds_write_b128.
                const float* fsrc = reinterpret_cast<const float*>(src);  // ES == 4 here
#pragma unroll
                for (int u = 0; u < QPT; u++) {
                    const int idx = tid + NT * u;
                    if (u < QPT - 1 || idx < NQ) {
                        const int row = idx / QW, qq = idx - row * QW;
                        __builtin_amdgcn_global_load_lds(
                            (const void*)(fsrc + rb0 + row * spitch + 4 * qq),
                            (__attribute__((address_space(3))) void*)(in + 4 * (NT * u + 64 * (tid >> 6))), 16, 0, 0);
                    }
                }
                // LDS-DMA writes are counted by vmcnt, not lgkmcnt: wait for this
                // wave's copies explicitly so the staging barrier below publishes
                // them whatever fence the compiler gives __syncthreads().
                __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else {
                // Padded LDS rows (R = 13: 96 floats staged in a 112-float pitch):
                // 16-byte loads into VGPRs, then ds_write_b128 per float4.
                typedef unsigned u32x4s __attribute__((ext_vector_type(4)));
                u32x4s q4[QPT];
#pragma unroll
                for (int u = 0; u < QPT; u++) {
                    const int idx = min(tid + NT * u, NQ - 1), row = idx / QW, qq = idx - row * QW;
                    q4[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (unsigned)(rb0 + row * spitch + 4 * qq) * 4u, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < QPT; u++) {
                    const int idx = tid + NT * u, row = idx / QW, qq = idx - row * QW;
                    if (u < QPT - 1 || idx < NQ) *reinterpret_cast<u32x4s*>(in + row * IW + 4 * qq) = q4[u];
                }
            }
        } else if (y0 - R >= 0 && y0 - R + IH <= H) {
            // Interior rows (most tiles): the row offset advances by a constant,
            // one s_add per row.  Rows past IH of the last step read in-range
            // data (or 0 past the buffer end) and are never stored.
            const int rb = __builtin_amdgcn_readfirstlane((y0 - R + wv) * rowB), rs = BLUR_NW * rowB;
#pragma unroll
            for (int i = 0; i < RPW; i++) ld(i, rb + i * rs);
        } else {
#pragma unroll
            for (int i = 0; i < RPW; i++) {
                const int ly = min(wv + BLUR_NW * i, IH - 1);
                ld(i, __builtin_amdgcn_readfirstlane(refl(y0 - R + ly, H) * rowB));
            }
        }
        // LDS row of step i: one base address + an immediate offset per row;
        // only the last step can fall past IH.
        float* const irow = in + wv * IW + lane + (ORG - R);
        if (!x4) {
#pragma unroll
            for (int i = 0; i < RPW; i++)
                if (i < RPW - 1 || wv + BLUR_NW * i < IH) irow[BLUR_NW * i * IW] = v0[i];
            if (lane < RW - 64) {
#pragma unroll
                for (int i = 0; i < RPW; i++)
                    if (i < RPW - 1 || wv + BLUR_NW * i < IH) irow[BLUR_NW * i * IW + 64] = v1[i];
            }
        }
    }
    __syncthreads();

    {
        // ds_read_b128 serves a wave in four 16-lane groups {0-3,12-15,20-27},
        // {4-11,16-19,28-31} (+32): give each group one row's 16 float4 blocks
        // so every group covers the 64 banks exactly once (conflict-free for
        // any row pitch).
        const int l = lane & 31;
        const bool grpB = (l >= 4 && l < 12) || (l >= 16 && l < 20) || l >= 28;
        const int blk = grpB ? (l < 12 ? l - 4 : (l < 20 ? l - 8 : l - 16)) : (l < 4 ? l : (l < 16 ? l - 8 : l - 12));
        const int xq = blk * 4;
        for (int ly = wave * 4 + (lane >> 5) * 2 + (grpB ? 1 : 0); ly < IH; ly += 4 * BLUR_NW) {
            float win[4 * NW];
            // The row's window starts at LDS column xq + ORG - R: read from the
            // aligned column xq + SA, the first SS values are skipped.
            const f32x4* p = reinterpret_cast<const f32x4*>(in + ly * IW + xq + SA);
#pragma unroll
            for (int v = 0; v < NW; v++) {
                f32x4 f = p[v];
                // Opaque use of all four lanes: otherwise the compiler narrows
                // the partly used last vector and splits the row into
                // misaligned ds_read2_b32/b64 pieces (bank conflicts).
                __asm__ volatile("" : "+v"(f));
                win[4 * v] = f[0];
                win[4 * v + 1] = f[1];
                win[4 * v + 2] = f[2];
                win[4 * v + 3] = f[3];
            }
            // Packed FP32: outputs (q, q+1) for q = 0, 2 share one v_pk_fma_f32
            // per tap (each lane an IEEE fma, so the chain is OpenCV's).  Their
            // operand (win[q+k], win[q+k+1]) is an even-aligned pair for even
            // q+k and an odd-aligned pair (built once per window) otherwise.
            f32x2 pe[2 * NW], po[2 * NW - 1];
#pragma unroll
            for (int j = 0; j < 2 * NW; j++) pe[j] = (f32x2){win[2 * j], win[2 * j + 1]};
#pragma unroll
            for (int j = 0; j < 2 * NW - 1; j++) po[j] = pk_mov_hi_lo(pe[j], pe[j + 1]);
            auto pr = [&](int i) -> f32x2 {  // (window[i], window[i+1]) = (win[SS+i], win[SS+i+1])
                i += SS;
                return (i & 1) ? po[i >> 1] : pe[i >> 1];
            };
            f32x2 s2[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int q = 2 * h;
                if constexpr (2 * R + 1 > 5) {
                    f32x2 a = {0.f, 0.f};
#pragma unroll
                    for (int k = 0; k <= 2 * R; k++) a = __builtin_elementwise_fma(pr(q + k), (f32x2)taps.w[k], a);
                    s2[h] = a;
                } else {
                    f32x2 a = pr(q + R) * (f32x2)taps.w[R];
#pragma unroll
                    for (int k = 1; k <= R; k++)
                        a = __builtin_elementwise_fma(pr(q + R - k) + pr(q + R + k), (f32x2)taps.w[R + k], a);
                    s2[h] = a;
                }
            }
            *reinterpret_cast<float4*>(mid + ly * IW + xq) = make_float4(s2[0][0], s2[0][1], s2[1][0], s2[1][1]);
        }
    }
    __syncthreads();

    float mx = -FLT_MAX, nmn = -FLT_MAX;  // pixel range (range_keys only)
    const int gx = x0 + lane;
    const bool full = y0 + BLUR_TH <= H && x0 + BLUR_TW <= W;  // uniform
    float outs[BLUR_CB][8];  // kBlurX4St: full-tile rows kept for the widened stores
#pragma unroll
    for (int cbk = 0; cbk < BLUR_CB; cbk++) {
        const int lx = lane, yb = (wave + cbk * BLUR_NW) * 8;
        // Column pairs (c[i], c[i+4]), one ds_read2st64_b32 each: output rows
        // (q, q+4) share every v_pk_add/v_pk_fma_f32 and no pair is assembled
        // from two loads.
        // (volatile: every element is loaded twice, into both pairs it belongs
        // to, instead of being loaded once and copied with v_mov.)
        const volatile __attribute__((address_space(3))) float* vmid =
            (const volatile __attribute__((address_space(3))) float*)(mid + yb * IW + lx);
        f32x2 cp[4 + 2 * R];
#pragma unroll
        for (int j = 0; j < 4 + 2 * R; j++) cp[j] = (f32x2){vmid[j * IW], vmid[(j + 4) * IW]};
        float out[8];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            f32x2 a = __builtin_elementwise_fma(cp[q + R], (f32x2)taps.w[R], (f32x2){0.f, 0.f});
#pragma unroll
            for (int k = 1; k <= R; k++) a = __builtin_elementwise_fma(cp[q + R + k] + cp[q + R - k], (f32x2)taps.w[R + k], a);
            out[q] = a[0];
            out[q + 4] = a[1];
        }
        if (kBlurX4St && full) {
#pragma unroll
            for (int q = 0; q < 8; q++) outs[cbk][q] = out[q];
        } else if (full) {
            // Full tile: unconditional buffer stores, the row step in the
            // scalar offset (no per-row address arithmetic or exec masking).
            const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(
                dst, 0, (int)min((long)dpitch * H * 4, 0x7fffffffL), 0x00020000);
            const unsigned voff = (unsigned)((y0 + yb) * dpitch + gx) * 4u;
#pragma unroll
            for (int q = 0; q < 8; q++)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, out[q]), drs, voff, q * dpitch * 4, 0);
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int gy = y0 + yb + q;
                if (gy < H && gx < W) dst[(size_t)gy * dpitch + gx] = out[q];
            }
        }
        if (dec_out && !(kBlurX4St && full)) {
            // The next octave's base plane (edge tiles; full tiles store it
            // from the LDS image below): even rows and columns of this plane
            // (y0, yb even), stored by the even lanes; other lanes get an
            // offset past the buffer, which the hardware drops (no branch).
            const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(
                dec_out, 0, (int)min((long)J.dec.pitch * J.dec.H * 4, 0x7fffffffL), 0x00020000);
            const bool cx = (gx & 1) == 0 && (gx >> 1) < J.dec.W;
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                const int dy = (y0 + yb + q) >> 1;
                const unsigned off = cx && dy < J.dec.H ? (unsigned)(dy * J.dec.pitch + (gx >> 1)) * 4u : 0x80000000u;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, out[q]), drs, off, 0, 0);
            }
        }
        if (range_keys) {
#pragma unroll
            for (int q = 0; q < 8; q++) {
                if (y0 + yb + q < H && gx < W) {
                    mx = fmaxf(mx, out[q]);
                    nmn = fmaxf(nmn, -out[q]);
                }
            }
        }
    }
    if (kBlurX4St && full) {
        // Widened stores: every wave's column pass has read `mid` (barrier);
        // each wave writes its 8-row blocks into the free LDS tile as a plain
        // 64-float-pitch image and reads back its own rows as float4s (the
        // same wave, in-order LDS: no second barrier), one 16-byte store per
        // 4 columns.  ds_read_b128 groups then cover 64 distinct banks.
        __syncthreads();
#pragma unroll
        for (int cbk = 0; cbk < BLUR_CB; cbk++) {
            const int yb = (wave + cbk * BLUR_NW) * 8;
#pragma unroll
            for (int q = 0; q < 8; q++) in[(yb + q) * BLUR_TW + lane] = outs[cbk][q];
        }
        typedef unsigned u32x4t __attribute__((ext_vector_type(4)));
        const __amdgpu_buffer_rsrc_t drs =
            __builtin_amdgcn_make_buffer_rsrc(dst, 0, (int)min((long)dpitch * H * 4, 0x7fffffffL), 0x00020000);
#pragma unroll
        for (int cbk = 0; cbk < BLUR_CB; cbk++) {
            const int yb = (wave + cbk * BLUR_NW) * 8;
#pragma unroll
            for (int hh = 0; hh < 2; hh++) {
                const int row = yb + 4 * hh + (lane >> 4), c4 = 4 * (lane & 15);
                const u32x4t v = *reinterpret_cast<const u32x4t*>(in + row * BLUR_TW + c4);
                __builtin_amdgcn_raw_buffer_store_b128(v, drs, (unsigned)((y0 + row) * dpitch + x0 + c4) * 4u, 0, 0);
            }
        }
        if (dec_out) {
            // The next octave's base plane from the same LDS image: an 8-row
            // block gives 4 rows x 8 float4s of even rows and columns; lane l
            // takes block 2 it + l / 32, row (l % 32) / 8, float4 l % 8 (two
            // 16-byte LDS reads, the even elements, one 16-byte store).
            const __amdgpu_buffer_rsrc_t ers = __builtin_amdgcn_make_buffer_rsrc(
                dec_out, 0, (int)min((long)J.dec.pitch * J.dec.H * 4, 0x7fffffffL), 0x00020000);
            const int r4 = (lane & 31) >> 3, c8 = 8 * (lane & 7);
#pragma unroll
            for (int it = 0; it < (BLUR_CB + 1) / 2; it++) {
                const int cbk = 2 * it + (lane >> 5);
                const int yb = (wave + min(cbk, BLUR_CB - 1) * BLUR_NW) * 8;
                const f32x4* rp = reinterpret_cast<const f32x4*>(in + (yb + 2 * r4) * BLUR_TW + c8);
                const f32x4 a = rp[0], b = rp[1];
                const u32x4t v = __builtin_bit_cast(u32x4t, (f32x4){a[0], a[2], b[0], b[2]});
                const unsigned off =
                    cbk < BLUR_CB ? (unsigned)(((y0 + yb) / 2 + r4) * J.dec.pitch + x0 / 2 + c8 / 2) * 4u : 0x80000000u;
                __builtin_amdgcn_raw_buffer_store_b128(v, ers, off, 0, 0);
            }
        }
    }
    {
        // Pixel range of the plane (requested for octave 0 / plane 0 only: every
        // later plane is a convex combination of it).  The descriptor sizes its
        // fixed-point histogram scale from it.
        if (range_keys) {
            for (int off = 32; off > 0; off >>= 1) {
                mx = fmaxf(mx, __shfl_xor(mx, off));
                nmn = fmaxf(nmn, __shfl_xor(nmn, off));
            }
            __syncthreads();  // reuse `mid` for the per-wave partials
            if (lane == 0) {
                mid[wave] = mx;
                mid[BLUR_NW + wave] = nmn;
            }
            __syncthreads();
            if (tid == 0) {  // spread over kRangeSlots address pairs: no single hot atomic
                unsigned* slot = range_keys + 2 * (tile % kRangeSlots);
                float a = mid[0], b = mid[BLUR_NW];
                for (int w = 1; w < BLUR_NW; w++) {
                    a = fmaxf(a, mid[w]);
                    b = fmaxf(b, mid[BLUR_NW + w]);
                }
                atomicMax(slot, range_key(a));
                atomicMax(slot + 1, range_key(b));
            }
        }
    }
}

inline BlurJob make_job(const void* src, int spitch, int W, int H, float* dst, int dpitch, const DecOut& dec,
                        const Taps& taps, unsigned* range_keys, Counters* zero_ctr, const Frames& fr, long sfs) {
    BlurJob j;
    j.nf = fr.nf;
    j.sfs = sfs;
    j.dfs = fr.stride;
    j.src = src;
    j.dst = dst;
    j.dec = dec;
    j.range_keys = range_keys;
    j.zero_ctr = zero_ctr;
    j.spitch = spitch;
    j.W = W;
    j.H = H;
    j.dpitch = dpitch;
    j.tilesX = (W + BLUR_TW - 1) / BLUR_TW;
    j.ntiles = j.tilesX * ((H + BLUR_TH - 1) / BLUR_TH);
    j.taps = taps;
    return j;
}

}  // namespace sift_amd
