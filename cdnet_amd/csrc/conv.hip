// Implicit-GEMM convolutions on the gfx950 matrix cores (v_mfma_f32_32x32x16_bf16), NHWC bf16 activations,
// fp32 accumulation.  One kernel family serves
//   3x3 pad 1 convolution   (models/dam/model_unet_rev1.py: VGG16-BN encoder :40-41, UpsampleBlock.conv2 :112-114,
//                            ResidualUnit :146-170; models/unet.py encoder/decoder :8-50)
//   1x1 convolution         (ResidualUnit.conv_1x1 :158)
//   ConvTranspose2d k4 s2 p1 as four 2x2 sub-pixel convolutions (UpsampleBlock.up :100-101)
//   ConvTranspose2d k2 s2   as four 1x1 sub-pixel convolutions  (models/unet.py decoder.up :30)
// and, with transposed/flipped weight packs, their backward-data passes.
//
// Tiling: one workgroup (4 waves) = TH x TW output pixels x BN output channels.  The (TH+2)x(TW+2) input halo of a
// CK-channel chunk is staged through LDS once and reused by all taps; the chunk's weights are staged in the exact
// MFMA B-fragment order (a linear copy of the host-side pack).  While staging, the producer layer's BatchNorm+ReLU
// (per-channel scale/shift), an optional residual add, a 2x2 max-pool and the decoder's zero-pad + concat are
// applied on the fly, so none of those ever makes its own pass over HBM.  The epilogue either applies a folded
// eval-mode BN (+ReLU) or emits the raw convolution output together with per-tile channel sums / sums of squares
// (training-mode BN statistics, reduced deterministically by bn_finalize).
#include <type_traits>
#include "common.h"
#include "conv_args.h"
#include "launch.h"
#include "xform.h"
#include "stage16.h"
#include <stdlib.h>

using namespace cdnet;

namespace {

__device__ int g_dbg_dummy;

// ------------------------------------------------------------------------------------------------------
// input staging
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ V16 max8(V16 a, V16 b, bool nonneg) {
    V16 o;
    if (nonneg) {                                // post-ReLU values: integer order == float order
        o.u = __builtin_bit_cast(uint4, xf_max_nonneg_bf8(__builtin_bit_cast(u32x4, a.u), __builtin_bit_cast(u32x4, b.u)));
        return o;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) o.h[j] = bf2f(a.h[j]) >= bf2f(b.h[j]) ? a.h[j] : b.h[j];
    return o;
}

// the 8 channels' scale / shift of one thread; `xf` is the LDS copy of the source's tables ([0] scale, [xfs] shift) made
// once per workgroup (a global load here would sit in front of the chunk pipeline: vmcnt retires in order), or null
// for callers without one
constexpr int XF_MAX = 2048;      // source channels (both concat sources) whose scale/shift fit the LDS table

__device__ __forceinline__ void load_chan_xf(ChanXf &t, const ConvSrc &s, const float *xf, int xfs, int c) {
    t.on = s.scale != nullptr;
    if (!t.on) return;
    const float4 *ps = reinterpret_cast<const float4 *>(xf ? xf + c : s.scale + c);
    const float4 *ph = reinterpret_cast<const float4 *>(xf ? xf + xfs + c : s.shift + c);
    float4 a = ps[0], b = ps[1], cc = ph[0], d = ph[1];
    t.sc[0] = a.x; t.sc[1] = a.y; t.sc[2] = a.z; t.sc[3] = a.w; t.sc[4] = b.x; t.sc[5] = b.y; t.sc[6] = b.z; t.sc[7] = b.w;
    t.sh[0] = cc.x; t.sh[1] = cc.y; t.sh[2] = cc.z; t.sh[3] = cc.w; t.sh[4] = d.x; t.sh[5] = d.y; t.sh[6] = d.z; t.sh[7] = d.w;
}

// Halo image of one K chunk in LDS.  16x16-pixel tiles with 16-channel chunks: 32 B per pixel, unpadded, the two 16-byte k-halves of
// a pixel at (half ^ (halo row & 1)) * 16 - an A-fragment ds_read_b128 serves 16 lanes per LDS cycle (8 pixels of one tile row and 8
// of the next, same k-half), and the row-parity swizzle puts them on 16 distinct 16-byte bank groups (tools/micro/lds_read_patterns.hip:
// 4 LDS cycles per read against 7-8 for 48-byte padded pixels).  Other tile shapes keep padded pixels (CK * 2 + 16 bytes).
template <int TH, int CK>
struct HaloImg {
    static constexpr bool SWZ = (TH == 16 && CK == 16);
    static constexpr int PSTR = SWZ ? CK * 2 : CK * 2 + 16;
    // byte offset of 16-byte slot `slot` of halo pixel `pix` in halo row `hy`
    __device__ __forceinline__ static int off(int pix, int hy, int slot) { return pix * PSTR + (SWZ ? ((slot ^ (hy & 1)) * 16) : slot * 16); }
};

template <int TH, int TW, int CK>
__device__ __forceinline__ void stage_input(const ConvSrc &s, int cc0, int n, int y0, int x0, int H, int W,
                                            unsigned char *lds_a, int tid, const float *xf = nullptr, int xfs = 0) {
    constexpr int VPP = CK / 8;                  // 16-byte vectors per pixel
    constexpr int HW_ = TW + 2, NPIX = (TH + 2) * (TW + 2);
    const int slot = tid % VPP;                  // constant per thread because 256 % VPP == 0
    ChanXf t;
    load_chan_xf(t, s, xf, xfs, cc0 + slot * 8);
    const bool relu = s.relu != 0;
    const bool f16 = s.f16 != 0;
    const bool plain = !t.on && !relu && s.res == nullptr && !f16;
    // logical source extent (after the optional 2x2 pool)
    // pool: 1 = floor mode (torchvision VGG 'M'), 2 = ceil mode (models/unet.py:19, partial windows at the edge)
    const int Hl = s.pool ? (s.Hs + (s.pool == 2)) / 2 : s.Hs, Wl = s.pool ? (s.Ws + (s.pool == 2)) / 2 : s.Ws;
    const size_t rs = s.row_stride ? (size_t)s.row_stride : (size_t)s.Ws * s.C;      // elements per row
    const size_t img = (size_t)n * s.Hs * rs;
    for (int v = tid; v < NPIX * VPP; v += 256) {
        const int pix = v / VPP;
        const int hy = pix / HW_, hx = pix - hy * HW_;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        V16 val;
        val.u = make_uint4(0, 0, 0, 0);
        const int ys = y - s.off_y, xs = x - s.off_x;
        if (y >= 0 && y < H && x >= 0 && x < W && ys >= 0 && ys < Hl && xs >= 0 && xs < Wl) {
            if (!s.pool) {
                const size_t e = img + (size_t)ys * rs + (size_t)xs * s.C + cc0 + slot * 8;
                V16 raw;
                raw.u = *reinterpret_cast<const uint4 *>(s.x + e);
                if (plain) val = raw;
                else if (s.res) { V16 r; r.u = *reinterpret_cast<const uint4 *>(s.res + e); val = xform8(raw, &r, t, relu, f16); }
                else val = xform8(raw, nullptr, t, relu, f16);
            } else {
                // maxpool 2x2 stride 2 of the transformed source (torchvision VGG 'M' layers / unet.py :19)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int yy = 2 * ys + (q >> 1), xx = 2 * xs + (q & 1);
                    if (q != 0 && (yy >= s.Hs || xx >= s.Ws)) continue;          // ceil-mode partial window
                    const size_t e = img + (size_t)yy * rs + (size_t)xx * s.C + cc0 + slot * 8;
                    V16 raw;
                    raw.u = *reinterpret_cast<const uint4 *>(s.x + e);
                    V16 tv = plain ? raw : xform8(raw, nullptr, t, relu, f16);
                    val = q == 0 ? tv : max8(val, tv, relu);
                }
            }
        }
        *reinterpret_cast<uint4 *>(lds_a + HaloImg<TH, CK>::off(pix, hy, slot)) = val.u;
    }
}

// ------------------------------------------------------------------------------------------------------
// software pipeline: the global loads of chunk c+1 (input halo + weights) are ISSUED before the MFMA loop of chunk c
// and only transformed / written to LDS after it, so their HBM/L2 latency hides under the matrix work (guide T14).
// Pooled sources (4 loads + max per element) keep the synchronous path.
// ------------------------------------------------------------------------------------------------------
#ifndef CDNET_CONV_XCD
#define CDNET_CONV_XCD 1
#endif
#ifndef CDNET_CONV_GLDS
#define CDNET_CONV_GLDS 1
#endif
#ifndef CDNET_CONV_ADEPTH
#define CDNET_CONV_ADEPTH 1
#endif
// LDS layout of conv_fwd_kernel (dynamic): [A halo tile][B chunk (x2 when the weights arrive by LDS-DMA)] aliased by the
// out tile + the BatchNorm partial sums, followed by the scale|shift table of the source channels.
template <int TH, int TW, int CK, int BN, int TAPS>
struct ConvLds {
    static constexpr bool DEEP = (CK == 16 && TH == 16);      // 16-channel chunks: prefetch ring of ADEPTH halo chunks
    static constexpr bool GLDS = CDNET_CONV_GLDS && DEEP;     // weights by global_load_lds into a double buffer
    static constexpr int ADEPTH = DEEP ? CDNET_CONV_ADEPTH : 1;
    static constexpr int PSTR = HaloImg<TH, CK>::PSTR;
    static constexpr int A_BYTES = (TH + 2) * (TW + 2) * PSTR;
    static constexpr int B_BYTES = TAPS * CK * BN * 2;
    static constexpr int STAGE = A_BYTES + (GLDS ? 2 : 1) * B_BYTES;
    static constexpr int OUT_BYTES = TH * TW * (BN * 2 + 8);
    static constexpr int STATS_BYTES = 4 * 2 * BN * 4;
    static constexpr int MAIN = ((STAGE > OUT_BYTES + STATS_BYTES ? STAGE : OUT_BYTES + STATS_BYTES) + 15) / 16 * 16;
    static int bytes(int ctot) { return MAIN + 2 * ((ctot + 7) / 8 * 8) * 4; }
};

template <int TH, int TW, int CK, int BN, int TAPS>
struct Prefetch {
    static constexpr int VPP = CK / 8;
    static constexpr int NPIX = (TH + 2) * (TW + 2);
    static constexpr int NA = (NPIX * VPP + 255) / 256;
    static constexpr bool GLDS = ConvLds<TH, TW, CK, BN, TAPS>::GLDS;
    static constexpr int NB = (TAPS * CK * BN * 2 / 16 + 255) / 256;
    static constexpr int ADEPTH = ConvLds<TH, TW, CK, BN, TAPS>::ADEPTH;
    struct ASlot {
        uint4 a[NA];
        unsigned valid;      // snapshot of the source's tvalid taken at issue time
        bool pooled;         // synchronous path at commit time
    };
    ASlot s[ADEPTH];         // ring of halo-chunk prefetches: chunk c lives in slot c % ADEPTH
    uint4 b[GLDS ? 1 : NB];
    // per (tile, source) staging geometry, computed once by prep_source and reused by every chunk of that source:
    int eoff[2][NA];         // element offset of the thread's i-th vector inside the image (channel 0 of its slot), -1 = zero fill
    unsigned tvalid[2];      // bit i: eoff[i] >= 0
};

template <int SI, int TH, int TW, int CK, int BN, int TAPS>
__device__ __forceinline__ void prep_source(Prefetch<TH, TW, CK, BN, TAPS> &P, const ConvSrc &s, int y0, int x0, int H, int W, int tid) {
    using PF = Prefetch<TH, TW, CK, BN, TAPS>;
    constexpr int HW_ = TW + 2;
    const int slot = tid % PF::VPP;
    const int rs = s.row_stride ? s.row_stride : s.Ws * s.C;
    P.tvalid[SI] = 0;
#pragma unroll
    for (int i = 0; i < PF::NA; ++i) {
        const int v = tid + i * 256;
        const int pix = v / PF::VPP;
        const int hy = pix / HW_, hx = pix - hy * HW_;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        const int ys = y - s.off_y, xs = x - s.off_x;
        const bool inr = v < PF::NPIX * PF::VPP;
        const bool ok = inr && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W && (unsigned)ys < (unsigned)s.Hs && (unsigned)xs < (unsigned)s.Ws;
        P.eoff[SI][i] = ok ? ys * rs + xs * s.C + slot * 8 : -1;
        P.tvalid[SI] |= (ok ? 1u : 0u) << i;
    }
}

template <int TH, int TW, int CK, int BN, int TAPS>
__device__ __forceinline__ void issue_b(Prefetch<TH, TW, CK, BN, TAPS> &P, const unsigned short *wchunk, int tid, unsigned char *lds_b_next) {
    using PF = Prefetch<TH, TW, CK, BN, TAPS>;
    if (PF::GLDS) {
        // weights: the packed chunk is the LDS image - LDS-DMA, one 1 KB wave-instruction per 64 vectors, no registers.
        // (destination = wave-uniform base + lane * 16; drained by the vmcnt(0) of the barrier before the next commit)
        constexpr int NVEC = TAPS * CK * BN * 2 / 16;
        static_assert(NVEC % 64 == 0, "whole wave-instructions");
        const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int i = 0; i < PF::NB; ++i) {
            const int v0 = (i * 4 + wave) * 64;                          // first vector of this wave-instruction
            if (v0 < NVEC)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(wchunk + (size_t)(v0 + lane) * 8),
                                                 (__attribute__((address_space(3))) void *)(lds_b_next + v0 * 16), 16, 0, 0);
        }
    } else {   // weights: linear, through registers
        const uint4 *src = reinterpret_cast<const uint4 *>(wchunk);
#pragma unroll
        for (int i = 0; i < PF::NB; ++i) {
            const int v = tid + i * 256;
            if (v < TAPS * CK * BN * 2 / 16) P.b[i] = src[v];
        }
    }
}

// halo chunk of source `si` (channels cc0..cc0+CK) -> the registers of one ring slot
template <typename PF>
__device__ __forceinline__ void issue_a(PF &P, typename PF::ASlot &S, const ConvSrc &s, int si, int cc0, int n) {
    S.pooled = s.pool != 0;
    S.valid = 0;
    if (S.pooled) return;
    const size_t rs = s.row_stride ? (size_t)s.row_stride : (size_t)s.Ws * s.C;
    const unsigned short *base = s.x + (size_t)n * s.Hs * rs + cc0;
    S.valid = si ? P.tvalid[1] : P.tvalid[0];
#pragma unroll
    for (int i = 0; i < PF::NA; ++i) {
        const int e = si ? P.eoff[1][i] : P.eoff[0][i];
        if (e >= 0) S.a[i] = *reinterpret_cast<const uint4 *>(base + e);
    }
}

template <int TH, int TW, int CK, int BN, int TAPS>
__device__ __forceinline__ void commit_chunk(const Prefetch<TH, TW, CK, BN, TAPS> &P, const typename Prefetch<TH, TW, CK, BN, TAPS>::ASlot &S,
                                             const ConvSrc &s, int si, int cc0, int n, int y0,
                                             int x0, int H, int W, unsigned char *lds_a, unsigned char *lds_b, int tid,
                                             const float *xf, int xfs) {
    using PF = Prefetch<TH, TW, CK, BN, TAPS>;
    if (!PF::GLDS) {
        uint4 *dst = reinterpret_cast<uint4 *>(lds_b);
#pragma unroll
        for (int i = 0; i < PF::NB; ++i) {
            const int v = tid + i * 256;
            if (v < TAPS * CK * BN * 2 / 16) dst[v] = P.b[i];
        }
    }
    if (S.pooled) { stage_input<TH, TW, CK>(s, cc0, n, y0, x0, H, W, lds_a, tid, xf, xfs); return; }
    const int slot = tid % PF::VPP;
    ChanXf t;
    load_chan_xf(t, s, xf, xfs, cc0 + slot * 8);
    const bool relu = s.relu != 0, f16 = s.f16 != 0;
    const bool plain = !t.on && !relu && s.res == nullptr && !f16;
    const size_t rs = s.row_stride ? (size_t)s.row_stride : (size_t)s.Ws * s.C;
    // the residual operand is read here (not prefetched: registers are better spent on more waves per SIMD); the
    // loads of all vectors are issued before the first use
    V16 rr[PF::NA];
    if (s.res) {
        const unsigned short *rbase = s.res + (size_t)n * s.Hs * rs + cc0;
#pragma unroll
        for (int i = 0; i < PF::NA; ++i) rr[i].u = *reinterpret_cast<const uint4 *>(rbase + ((S.valid & (1u << i)) ? (si ? P.eoff[1][i] : P.eoff[0][i]) : 0));
    }
    // LDS address of vector i: pixel (tid / VPP + i * 256 / VPP), slot tid % VPP
#pragma unroll
    for (int i = 0; i < PF::NA; ++i) {
        if (tid + i * 256 >= PF::NPIX * PF::VPP) continue;
        V16 val;
        val.u = make_uint4(0, 0, 0, 0);
        if (S.valid & (1u << i)) {
            V16 raw;
            raw.u = S.a[i];
            if (plain) val = raw;
            else if (s.res) val = xform8(raw, &rr[i], t, relu, f16);
            else val = xform8(raw, nullptr, t, relu, f16);
        }
        const int pix = (tid + i * 256) / PF::VPP;
        *reinterpret_cast<uint4 *>(lds_a + HaloImg<TH, CK>::off(pix, pix / (TW + 2), slot)) = val.u;
    }
}

// ------------------------------------------------------------------------------------------------------
// the kernel
// ------------------------------------------------------------------------------------------------------
template <int TH, int TW, int CK, int BN, int WM, int WN, int TAPS>
__global__ __launch_bounds__(256, (BN <= 64 ? (CK == 16 && TH == 16 && CDNET_CONV_ADEPTH <= 2 ? 3 : 2) : 1)) void conv_fwd_kernel(ConvArgs A) {
    constexpr int PSTR = HaloImg<TH, CK>::PSTR;
    constexpr bool SWZ = HaloImg<TH, CK>::SWZ;
    constexpr int HW_ = TW + 2;
    constexpr int KC = CK / 16;
    constexpr int MT = TH * TW / 32, NT = BN / 32;
    constexpr int MPW = MT / WM, NPW = NT / WN;
    using LDS = ConvLds<TH, TW, CK, BN, TAPS>;
    constexpr bool GLDS = LDS::GLDS;
    constexpr int A_BYTES = LDS::A_BYTES;
    constexpr int B_BYTES = LDS::B_BYTES;
    constexpr int OSTR = BN * 2 + 8;             // out staging row stride (bytes)
    static_assert(MT % WM == 0 && NT % WN == 0 && WM * WN == 4, "wave tiling");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *lds_a = smem;
    unsigned char *lds_b0 = smem + A_BYTES;
    float (*s_stats)[2][BN] = reinterpret_cast<float (*)[2][BN]>(smem + LDS::OUT_BYTES);      // epilogue only
    float *s_xf = reinterpret_cast<float *>(smem + LDS::MAIN);          // scale | shift of source 0 then source 1

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;
    const int xfs = ((A.src[0].C + (A.nsrc > 1 ? A.src[1].C : 0)) + 7) / 8 * 8;      // table stride (floats)
    {
        const int c0n = A.src[0].C, ctot = c0n + (A.nsrc > 1 ? A.src[1].C : 0);
        for (int c = tid; c < ctot; c += 256) {
            const ConvSrc &S = c < c0n ? A.src[0] : A.src[1];
            const int cc = c < c0n ? c : c - c0n;
            s_xf[c] = S.scale ? S.scale[cc] : 1.f;
            s_xf[xfs + c] = S.shift ? S.shift[cc] : 0.f;
        }
        // (published by the barrier in front of the first commit)
    }

    // one workgroup per (image, parity, tile_y, tile_x) tile
    const int tiles_x = (A.W + TW - 1) / TW, tiles_y = (A.H + TH - 1) / TH;
    const int tiles_img = tiles_x * tiles_y;
    const int total_tiles = A.N * A.npar * tiles_img;
    const int nchunk_total = A.nchunk;
    // XCD-aware order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2) in dispatch order (x fastest).  XCD k takes
    // the k-th contiguous eighth of the (tile, cout block) sequence with the cout blocks of one tile next to each other: neighbouring
    // tiles - which share halo rows / columns - and the cout blocks of one tile - which read the same input - sit behind one L2 at about
    // the same time (a 64 -> 256 1x1 layer read its input from HBM four times when the cout blocks were dealt a whole grid apart)
#if CDNET_CONV_XCD
    int tile, cout_tile;
    {
        const int NC = (int)gridDim.y, lin = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
        const int T = (int)gridDim.x * NC, q = T >> 3, rem = T & 7;
        const int xcd = lin & 7, idx = lin >> 3;
        const int seq = xcd < rem ? xcd * (q + 1) + idx : rem * (q + 1) + (xcd - rem) * q + idx;
        tile = seq / NC;
        cout_tile = seq - tile * NC;
        if (A.debug & 16) { tile = blockIdx.x; cout_tile = blockIdx.y; }          // ablation (CDNET_CONV_DEBUG=16): dispatch order
    }
#else
    const int tile = blockIdx.x, cout_tile = blockIdx.y;
#endif

    // per-lane A base for each of this wave's M tiles
    // (swizzled image: the k-half position follows the parity of the halo row = tile row + the tap's row offset)
    int abase[MPW][SWZ ? 2 : 1];
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
        const int m = (wm * MPW + mi) * 32 + l31;
        const int py = m / TW, px = m % TW;
#pragma unroll
        for (int rp = 0; rp < (SWZ ? 2 : 1); ++rp) abase[mi][rp] = (py * HW_ + px) * PSTR + (SWZ ? ((half ^ ((py + rp) & 1)) * 16) : half * 16);
    }
    const int bbase = half * BN * 16 + (wn * NPW * 32 + l31) * 16;

    // chunk c -> (source, first channel)
    auto chunk_src = [&](int c, int &si, int &cc0) {
        const int n0 = A.src[0].C / CK;
        if (c < n0) { si = 0; cc0 = c * CK; } else { si = 1; cc0 = (c - n0) * CK; }
    };
    auto decode = [&](int tile, int &n, int &par, int &y0, int &x0) {
        const int z = tile / tiles_img, r = tile - z * tiles_img;
        n = z / A.npar; par = z - n * A.npar;
        const int ty_ = r / tiles_x;
        y0 = ty_ * TH; x0 = (r - ty_ * tiles_x) * TW;
    };
    auto wchunk = [&](int par, int chunk) {
        return A.w + ((size_t)(par * gridDim.y + cout_tile) * nchunk_total + chunk) * (B_BYTES / 2);
    };

    Prefetch<TH, TW, CK, BN, TAPS> P;
    (void)total_tiles;
    {
        int n, par, y0, x0;
        decode(tile, n, par, y0, x0);
        using PF = Prefetch<TH, TW, CK, BN, TAPS>;
        constexpr int AD = PF::ADEPTH;
        prep_source<0>(P, A.src[0], y0, x0, A.H, A.W, tid);
        if (A.nsrc > 1) prep_source<1>(P, A.src[1], y0, x0, A.H, A.W, tid);
        // prologue: the first AD halo chunks and the first weight chunk
        issue_b(P, wchunk(par, 0), tid, lds_b0);
#pragma unroll
        for (int k = 0; k < AD; ++k)
            if (k < nchunk_total) {
                int si, cc0;
                chunk_src(k, si, cc0);
                issue_a(P, P.s[k], A.src[si], si, cc0, n);
            }
        // tap offsets inside the halo tile (rows, cols): 3x3 / 1x1 fixed, sub-pixel 2x2 depends on the parity
        int toff[TAPS], tpar[TAPS];
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            int r, c;
            if (TAPS == 9) { r = t / 3; c = t % 3; }
            else if (TAPS == 4) {
                const int a = par >> 1, b = par & 1, ty = t >> 1, tx = t & 1;
                r = a == 0 ? (ty == 0 ? 1 : 0) : (ty == 0 ? 2 : 1);
                c = b == 0 ? (tx == 0 ? 1 : 0) : (tx == 0 ? 2 : 1);
            } else { r = 1; c = 1; }
            toff[t] = (r * HW_ + c) * PSTR;
            tpar[t] = SWZ ? (r & 1) : 0;
        }
        f32x16 acc[MPW][NPW];
#pragma unroll
        for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
            for (int ni = 0; ni < NPW; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

        // one chunk step; K = ring slot of this chunk (compile-time so that the prefetch registers stay registers)
        auto step = [&](auto kc_, int chunk) {
            constexpr int K = decltype(kc_)::value;
            int si, cc0;
            chunk_src(chunk, si, cc0);
            __syncthreads();                               // previous chunk's fragment reads / previous tile's out-tile reads are done
            unsigned char *lds_b = lds_b0 + (GLDS ? (chunk & 1) * B_BYTES : 0);
            commit_chunk<TH, TW, CK, BN, TAPS>(P, P.s[K], A.src[si], si, cc0, n, y0, x0, A.H, A.W, lds_a, lds_b, tid, s_xf + (si ? A.src[0].C : 0), xfs);
            __syncthreads();
            // refill: the weights of the next chunk and the halo chunk AD steps ahead fly during the MFMA loops
            if (chunk + 1 < nchunk_total) issue_b(P, wchunk(par, chunk + 1), tid, lds_b0 + ((chunk + 1) & 1) * B_BYTES);
            if (chunk + AD < nchunk_total) {
                int sj, cj;
                chunk_src(chunk + AD, sj, cj);
                issue_a(P, P.s[K], A.src[sj], sj, cj, n);
            }
            if (A.debug & 4) return;
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) {
                    bf16x8 af[MPW], bfr[NPW];
#pragma unroll
                    for (int mi = 0; mi < MPW; ++mi)
                        af[mi] = *reinterpret_cast<const bf16x8 *>(lds_a + (SWZ ? (tpar[t] ? abase[mi][SWZ ? 1 : 0] : abase[mi][0]) : abase[mi][0]) + toff[t] + kc * 32);
#pragma unroll
                    for (int ni = 0; ni < NPW; ++ni)
                        bfr[ni] = *reinterpret_cast<const bf16x8 *>(lds_b + bbase + ((t * KC + kc) * 2) * BN * 16 + ni * 512);
#pragma unroll
                    for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NPW; ++ni)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
                }
            }
        };
        for (int c0 = 0; c0 < nchunk_total; c0 += AD) {
            step(std::integral_constant<int, 0>{}, c0);
            if (AD > 1 && c0 + 1 < nchunk_total) step(std::integral_constant<int, (AD > 1 ? 1 : 0)>{}, c0 + 1);
            if (AD > 2 && c0 + 2 < nchunk_total) step(std::integral_constant<int, (AD > 2 ? 2 : 0)>{}, c0 + 2);
            if (AD > 3 && c0 + 3 < nchunk_total) step(std::integral_constant<int, (AD > 3 ? 3 : 0)>{}, c0 + 3);
        }
        static_assert(AD <= 4, "ring depth");
        __syncthreads();

        // ---------------- epilogue ----------------
        if (A.debug & 8) { if (acc[0][0][0] == 123.456f) g_dbg_dummy = 1; return; }
        const int cout0 = cout_tile * BN;
        unsigned char *s_out = smem;
        const bool full = (y0 + TH <= A.H) && (x0 + TW <= A.W);
        float ssum[NPW], ssq[NPW];
#pragma unroll
        for (int ni = 0; ni < NPW; ++ni) { ssum[ni] = 0.f; ssq[ni] = 0.f; }
        // BatchNorm statistics of the raw accumulators (before bias / scale).  Full tiles take the branch-free loop.
        if (A.stats) {
            if (full) {
#pragma unroll
                for (int ni = 0; ni < NPW; ++ni)
#pragma unroll
                    for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
                        for (int r = 0; r < 16; ++r) { const float v = acc[mi][ni][r]; ssum[ni] += v; ssq[ni] = fmaf(v, v, ssq[ni]); }
            } else {
#pragma unroll
                for (int ni = 0; ni < NPW; ++ni)
#pragma unroll
                    for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int m = (wm * MPW + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                            const float v = ((y0 + m / TW) < A.H && (x0 + m % TW) < A.W) ? acc[mi][ni][r] : 0.f;
                            ssum[ni] += v;
                            ssq[ni] = fmaf(v, v, ssq[ni]);
                        }
            }
        }
        // accumulators -> 16-bit out tile in LDS.  A lane owns one output channel (column) of 16 pixel rows; two
        // neighbouring lanes swap one value per register pair through DPP (quad_perm [1,0,3,2]) so that each lane
        // ends up with the (even column, odd column) pair of ONE row and stores a packed dword: no LDS permutes, half
        // the stores.  bias, scale and shift fold into one fma; the ReLU is taken on the packed 16-bit patterns.
        auto write_tile = [&](auto f16c) {
            constexpr bool F16 = decltype(f16c)::value;
            const bool odd = (l31 & 1) != 0;
            const s16x2 lo = A.orelu ? s16x2{0, 0} : s16x2{(short)-32768, (short)-32768};
#pragma unroll
            for (int ni = 0; ni < NPW; ++ni) {
                const int col = (wn * NPW + ni) * 32 + l31;
                const int co = cout0 + col;
                const bool cok = co < A.Cout;
                const float osc = (A.oscale && cok) ? A.oscale[co] : 1.f;
                const float osh = fmaf((A.bias && cok) ? A.bias[co] : 0.f, osc, (A.oshift && cok) ? A.oshift[co] : 0.f);
                unsigned char *dst = s_out + (col & ~1) * 2 + (odd ? OSTR : 0);
#pragma unroll
                for (int mi = 0; mi < MPW; ++mi) {
#pragma unroll
                    for (int rp = 0; rp < 8; ++rp) {
                        const int r = 2 * rp;
                        const int m = (wm * MPW + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;     // row of register r
                        const float v0 = fmaf(acc[mi][ni][r], osc, osh), v1 = fmaf(acc[mi][ni][r + 1], osc, osh);
                        const float send = odd ? v0 : v1;
                        const float got = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, true));
                        const f32x2 pr = {odd ? got : v0, odd ? v1 : got};      // (even column, odd column) of row m (+1 on odd lanes)
                        s16x2 pk;
                        if (F16) pk = __builtin_bit_cast(s16x2, __builtin_convertvector(pr, h16x2));
                        else pk = __builtin_bit_cast(s16x2, __builtin_convertvector(pr, bf16x2));
                        pk = __builtin_elementwise_max(pk, lo);
                        *reinterpret_cast<unsigned *>(dst + m * OSTR) = __builtin_bit_cast(unsigned, pk);
                    }
                }
            }
        };
        if (A.out_f16 || A.eres) write_tile(std::true_type{});        // the fused residual epilogue stages r in fp16
        else write_tile(std::false_type{});
        if (A.stats) {
#pragma unroll
            for (int ni = 0; ni < NPW; ++ni) {
                ssum[ni] += __shfl_xor(ssum[ni], 32);
                ssq[ni] += __shfl_xor(ssq[ni], 32);
                if (half == 0) {
                    s_stats[wave][0][(wn * NPW + ni) * 32 + l31] = ssum[ni];
                    s_stats[wave][1][(wn * NPW + ni) * 32 + l31] = ssq[ni];
                }
            }
        }
        __syncthreads();
        if (A.stats && tid < 2 * BN) {
            const int which = tid / BN, col = tid % BN;
            const int wn_of = col / (NPW * 32);
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < WM; ++k) v += s_stats[k * WN + wn_of][which][col];
            const int co = cout0 + col;
            if (co < A.Cout) A.stats[((size_t)tile * 2 + which) * A.Cout + co] = v;
        }
        // coalesced store of the tile: 16-byte vectors, BN/8 per pixel
        {
            constexpr int VO = BN / 8;
            const int Ho = A.H * A.ostride, Wo = A.W * A.ostride;
            const int pa = par >> 1, pb = par & 1;
            ChanXf et;                                       // fused residual epilogue: the other branch's per-channel affine
            et.on = false;
            if (A.eres && A.eres_scale) {
                const int c8 = cout0 + (tid % VO) * 8;          // 256 % VO == 0: a thread always stores the same 8 channels
                et.on = true;
#pragma unroll
                for (int j = 0; j < 8; ++j) { et.sc[j] = c8 + j < A.Cout ? A.eres_scale[c8 + j] : 1.f; et.sh[j] = c8 + j < A.Cout ? A.eres_shift[c8 + j] : 0.f; }
            }
            // one 16-byte vector of the tile: optional fused residual epilogue, then the store
            auto store_vec = [&](int v, const uint4 *pre) {
                const int m = v / VO, q = v % VO;
                const int y = y0 + m / TW, x = x0 + m % TW;
                const int co = cout0 + q * 8;
                if (y < A.H && x < A.W && co < A.Cout) {
                    const int oy = y * A.ostride + pa, ox = x * A.ostride + pb;
                    uint4 val = *reinterpret_cast<const uint4 *>(s_out + m * OSTR + q * 16);
                    const size_t opix = ((size_t)n * Ho + oy) * Wo + ox;
                    if (A.eres) {
                        // out = bf16([relu]((eres * scale + shift) + r)), r = this convolution's fp16-rounded result: the same
                        // arithmetic as the staging transform of a (raw, residual) source pair (xform8)
                        V16 e, r;
                        e.u = pre ? *pre : *reinterpret_cast<const uint4 *>(A.eres + opix * A.Cout + co);
                        r.u = val;
                        if (A.eres_f16) val = xform8(e, &r, et, A.eres_relu != 0, true).u;
                        else {                                   // bf16 other branch (identity shortcut of an HRNet block)
                            V16 o;
#pragma unroll
                            for (int j = 0; j < 8; ++j) {
                                float t = bf2f(e.h[j]);
                                if (et.on) t = fmaf(t, et.sc[j], et.sh[j]);
                                t += ld16(r.h[j], true);
                                o.h[j] = f2bf(A.eres_relu ? fmaxf(t, 0.f) : t);
                            }
                            val = o.u;
                        }
                    }
                    unsigned short *dst = A.out + opix * A.out_cstride + A.out_coff + co;
                    *reinterpret_cast<uint4 *>(dst) = val;               // Cout % 8 == 0 (checked by the ABI entry)
                }
            };
            constexpr bool PRE = (BN == 64 && TH == 16 && CK == 16);      // the configuration the residual units run
            if constexpr (PRE) {
                if (A.eres) {
                    // the other branch's vectors are requested up front (clamped address): their latency overlaps instead of
                    // sitting in front of every store
                    constexpr int NV = TH * TW * VO / 256;
                    uint4 ev[NV];
#pragma unroll
                    for (int i = 0; i < NV; ++i) {
                        const int v = tid + i * 256, m = v / VO, q = v % VO;
                        int y = y0 + m / TW, x = x0 + m % TW, co = cout0 + q * 8;
                        y = y < A.H ? y : A.H - 1; x = x < A.W ? x : A.W - 1; co = co < A.Cout ? co : 0;
                        ev[i] = *reinterpret_cast<const uint4 *>(A.eres + (((size_t)n * A.H + y) * A.W + x) * A.Cout + co);
                    }
#pragma unroll
                    for (int i = 0; i < NV; ++i) store_vec(tid + i * 256, &ev[i]);
                } else {
                    for (int v = tid; v < TH * TW * VO; v += 256) store_vec(v, nullptr);
                }
            } else {
                for (int v = tid; v < TH * TW * VO; v += 256) store_vec(v, nullptr);
            }
        }
    }
}

template <int TH, int TW, int CK, int BN, int WM, int WN, int TAPS>
int launch_conv(const ConvArgs &A, hipStream_t st) {
    using LDS = ConvLds<TH, TW, CK, BN, TAPS>;
    int ctot = 0;
    for (int i = 0; i < A.nsrc; ++i) ctot += A.src[i].C;
    const int smem = LDS::bytes(ctot);
    const int total_tiles = cdiv(A.W, TW) * cdiv(A.H, TH) * A.N * A.npar;
    const int ctiles = cdiv(A.Cout, BN);
    dim3 grid(total_tiles, ctiles, 1);
    g_conv_last_form = conv_form(CDNET_CONV_FAMILY_FWD, BN, TAPS, 0, false, false, false, 0, 0, TH, CK);
    return launch_lds<conv_fwd_kernel<TH, TW, CK, BN, WM, WN, TAPS>>(grid, 256, LDS::bytes(XF_MAX), smem, st, "hipFuncSetAttribute(conv)", "conv_fwd_kernel", A);
}

template <int TAPS>
int dispatch_conv(const ConvArgs &A, hipStream_t st) {
    // configuration key: (tile, CK, BN); chosen by the host (cdnet_amd/engine.py) per layer
    const int key = A.tile * 10000 + A.CK * 100 + (A.BN == 128 ? 99 : A.BN);
    switch (key) {
        case 16 * 10000 + 16 * 100 + 32: return launch_conv<16, 16, 16, 32, 4, 1, TAPS>(A, st);
        case 16 * 10000 + 16 * 100 + 64: return launch_conv<16, 16, 16, 64, 4, 1, TAPS>(A, st);
        case 16 * 10000 + 32 * 100 + 32: return launch_conv<16, 16, 32, 32, 4, 1, TAPS>(A, st);
        case 16 * 10000 + 32 * 100 + 64: return launch_conv<16, 16, 32, 64, 4, 1, TAPS>(A, st);
        case 16 * 10000 + 32 * 100 + 99: return launch_conv<16, 16, 32, 128, 2, 2, TAPS>(A, st);
        case 16 * 10000 + 64 * 100 + 64: return launch_conv<16, 16, 64, 64, 4, 1, TAPS>(A, st);
        case 8 * 10000 + 32 * 100 + 64: return launch_conv<8, 8, 32, 64, 2, 2, TAPS>(A, st);
        case 8 * 10000 + 32 * 100 + 99: return launch_conv<8, 8, 32, 128, 2, 2, TAPS>(A, st);
        case 8 * 10000 + 64 * 100 + 64: return launch_conv<8, 8, 64, 64, 2, 2, TAPS>(A, st);
        default:
            set_error("cdnet_conv: unsupported configuration tile=%d CK=%d BN=%d", A.tile, A.CK, A.BN);
            return CDNET_E_ARG;
    }
}

// ------------------------------------------------------------------------------------------------------
// A source with its pending transform (BatchNorm scale/shift, residual, ReLU, 2x2 max-pool, pad offset) written out as a
// plain bf16 tensor - exactly the values stage_input would put into LDS.  Used where the on-the-fly transform costs more
// than a pass over HBM: max-pooled sources (4 loads + 4 transforms per staged element, repeated by every output-channel
// block and halo; the pooled staging path is not pipelined).
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void materialize_kernel(const ConvSrc s, int N, int H, int W, unsigned short *__restrict__ out) {
    const int VPP = s.C / 8;
    const size_t total = (size_t)N * H * W * VPP;
    const bool relu = s.relu != 0, f16 = s.f16 != 0;
    const int Hl = s.pool ? (s.Hs + (s.pool == 2)) / 2 : s.Hs, Wl = s.pool ? (s.Ws + (s.pool == 2)) / 2 : s.Ws;
    const size_t rs = s.row_stride ? (size_t)s.row_stride : (size_t)s.Ws * s.C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int slot = (int)(i % VPP);
        const size_t pix = i / VPP;
        const int x = (int)(pix % W), y = (int)((pix / W) % H), n = (int)(pix / ((size_t)W * H));
        ChanXf t;
        load_chan_xf(t, s, nullptr, 0, slot * 8);
        const bool plain = !t.on && !relu && s.res == nullptr && !f16;
        const size_t img = (size_t)n * s.Hs * rs;
        V16 val;
        val.u = make_uint4(0, 0, 0, 0);
        const int ys = y - s.off_y, xs = x - s.off_x;
        if (ys >= 0 && ys < Hl && xs >= 0 && xs < Wl) {
            if (!s.pool) {
                const size_t e = img + (size_t)ys * rs + (size_t)xs * s.C + slot * 8;
                V16 raw;
                raw.u = *reinterpret_cast<const uint4 *>(s.x + e);
                if (plain) val = raw;
                else if (s.res) { V16 r; r.u = *reinterpret_cast<const uint4 *>(s.res + e); val = xform8(raw, &r, t, relu, f16); }
                else val = xform8(raw, nullptr, t, relu, f16);
            } else {
                V16 raw[4];
                bool ok[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {                     // all four loads first (clamped address), then the math
                    int yy = 2 * ys + (q >> 1), xx = 2 * xs + (q & 1);
                    ok[q] = q == 0 || (yy < s.Hs && xx < s.Ws);   // ceil-mode partial window
                    yy = yy < s.Hs ? yy : s.Hs - 1;
                    xx = xx < s.Ws ? xx : s.Ws - 1;
                    raw[q].u = *reinterpret_cast<const uint4 *>(s.x + img + (size_t)yy * rs + (size_t)xx * s.C + slot * 8);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const V16 tv = plain ? raw[q] : xform8(raw[q], nullptr, t, relu, f16);
                    val = q == 0 ? tv : (ok[q] ? max8(val, tv, relu) : val);
                }
            }
        }
        *reinterpret_cast<uint4 *>(out + pix * s.C + slot * 8) = val.u;
    }
}

}  // namespace

// the launchers' record of the instantiation taken (conv_args.h; dry runs of cdnet_conv_ws_eligible and refused calls do not write it)
namespace cdnet {
thread_local int g_conv_last_form = 0;
}
extern "C" int cdnet_conv_forward_last_form(void) { return g_conv_last_form; }

extern "C" int cdnet_conv_forward(const cdnet_conv_args *args, void *stream) {
    CDNET_REQUIRE(args, "cdnet_conv_forward: null args");
    const ConvArgs &A = *reinterpret_cast<const ConvArgs *>(args);
    CDNET_REQUIRE(A.nsrc >= 1 && A.nsrc <= 2 && A.w && (A.out || A.dot_out), "cdnet_conv_forward: bad pointers / nsrc=%d", A.nsrc);
    CDNET_REQUIRE(!A.dot_out || (A.dot_w && !A.f32 && !A.pool_out), "cdnet_conv_forward: dot_out needs dot_w, the 16-bit path and no pool_out");
    CDNET_REQUIRE(A.N > 0 && A.H > 0 && A.W > 0 && A.Cout > 0 && A.Cout % 8 == 0, "cdnet_conv_forward: bad size (Cout must be a multiple of 8)");
    {
        int ctot_xf = 0;
        for (int i = 0; i < A.nsrc; ++i) ctot_xf += A.src[i].C;
        CDNET_REQUIRE(ctot_xf <= XF_MAX, "cdnet_conv_forward: %d source channels exceed the %d-entry scale/shift table", ctot_xf, XF_MAX);
    }
    CDNET_REQUIRE(A.ws == 0 || A.ws == 2, "cdnet_conv_forward: ws must be 0 or 2 (BatchNorm-backward statistics epilogue)");
    if (A.f32) {
        CDNET_REQUIRE(A.f32 == 1, "cdnet_conv_forward: f32 must be 0 or 1");
        for (int i = 0; i < A.nsrc; ++i)
            CDNET_REQUIRE(A.src[i].f16 == 2, "cdnet_conv_forward(f32): every source must be fp32 (f16 = 2)");
    } else {
        for (int i = 0; i < A.nsrc; ++i)
            CDNET_REQUIRE(A.src[i].f16 == 0 || A.src[i].f16 == 1, "cdnet_conv_forward: fp32 sources need args.f32 = 1");
    }
    if (A.eres && A.ws != 2) {
        CDNET_REQUIRE(A.ostride == 1 && A.npar == 1 && A.out_coff == 0 && A.out_cstride == A.Cout && !A.stats && !A.orelu &&
                      !A.out_f16 && ((A.eres_scale == nullptr) == (A.eres_shift == nullptr)),
                      "cdnet_conv_forward: fused residual epilogue needs a dense bf16 output, no statistics and no ReLU before the add");
    }
    int nchunk = 0;
    for (int i = 0; i < A.nsrc; ++i) {
        CDNET_REQUIRE(A.src[i].x && A.src[i].C % A.CK == 0, "cdnet_conv_forward: source %d channels %d not a multiple of CK=%d",
                      i, A.src[i].C, A.CK);
        CDNET_REQUIRE(!(A.src[i].pool && A.src[i].res), "cdnet_conv_forward: pool+residual source unsupported");
        nchunk += A.src[i].C / A.CK;
    }
    // (the second source of a two-source 3x3 launch of the 16-bit path may carry ONE padding chunk of zero weights beyond its channels - an even
    //  chunk count for conv_ws16_kernel's out-image form with pair requests; what a kernel reads for that chunk is the neighbouring pixel's
    //  channels, or zeros past the tensor's end: finite values times zero weights)
    const bool padded = A.nchunk == nchunk + 1 && A.taps == 9 && A.nsrc == 2 && !A.f32;
    CDNET_REQUIRE(nchunk == A.nchunk || padded, "cdnet_conv_forward: nchunk %d != %d", A.nchunk, nchunk);
    CDNET_REQUIRE((A.taps == 9 && A.npar == 1 && A.ostride == 1) || (A.taps == 1 && A.npar == 1 && A.ostride == 1) ||
                  (A.taps == 4 && A.npar == 4 && A.ostride == 2) || (A.taps == 1 && A.npar == 4 && A.ostride == 2),
                  "cdnet_conv_forward: taps=%d npar=%d ostride=%d", A.taps, A.npar, A.ostride);
    CDNET_REQUIRE(A.out_cstride % 8 == 0 && A.out_coff % 8 == 0, "cdnet_conv_forward: output channel slice must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    CDNET_REQUIRE(A.taps1 == 0 || A.taps1 == A.taps || (A.taps1 == 1 && A.taps == 9 && A.nsrc == 2), "cdnet_conv_forward: taps1 = %d (0, taps, or 1 beside a nine-tap first source)", A.taps1);
    if (A.f32) return conv_forward_f32(A, st);
    {
        const int rc = conv_forward_ws16(A, st);
        if (rc >= 0) return rc;
        CDNET_REQUIRE(A.taps1 == 0 || A.taps1 == A.taps, "cdnet_conv_forward: a one-tap second source runs on conv_ws16_kernel only (ask cdnet_conv_ws_eligible)");
        CDNET_REQUIRE(!A.pool_out, "cdnet_conv_forward: the fused max-pool output needs conv_ws16_kernel's out-image form (ask cdnet_conv_ws_eligible)");
        CDNET_REQUIRE(!A.dot_out, "cdnet_conv_forward: the fused 1x1 classifier (dot_out) needs conv_ws16_kernel's out-image form with resident weights (ask cdnet_conv_ws_eligible)");
        // (only conv_ws16_kernel / conv_ws_kernel read through bounded buffer descriptors: the one-tile kernels would index the scale / shift
        //  table and the tensor past the second source's channels)
        CDNET_REQUIRE(!padded, "cdnet_conv_forward: a padding chunk (nchunk = real + 1) runs on conv_ws16_kernel only (ask cdnet_conv_ws_eligible)");
    }
    static const int dbg = getenv("CDNET_CONV_DEBUG") ? atoi(getenv("CDNET_CONV_DEBUG")) : 0;
    if (!(A.debug & CONV_DBG_ONE_TILE)) {
        const int rc = conv_forward_ws(A, st);
        if (rc >= 0) return rc;
    }
    for (int i = 0; i < A.nsrc; ++i)
        CDNET_REQUIRE(A.src[i].relu >= 0 && A.src[i].relu <= 2, "cdnet_conv_forward: source %d: relu = %d (the BatchNorm-backward source of round 2, relu = 3, was removed)", i, A.src[i].relu);
    CDNET_REQUIRE(A.ws != 2, "cdnet_conv_forward: the BatchNorm-backward statistics epilogue (ws = 2) exists in fp32 mode on conv_ws32_kernel only "
                             "(ask cdnet_conv_ws_eligible first)");
    if (dbg) { ConvArgs B = A; B.debug = dbg; if (B.taps == 9) return dispatch_conv<9>(B, st); }
    if (A.debug & CONV_DBG_ONE_TILE) { ConvArgs B = A; B.debug = 0; if (B.taps == 9) return dispatch_conv<9>(B, st); if (B.taps == 4) return dispatch_conv<4>(B, st); return dispatch_conv<1>(B, st); }
    if (A.taps == 9) return dispatch_conv<9>(A, st);
    if (A.taps == 4) return dispatch_conv<4>(A, st);
    return dispatch_conv<1>(A, st);
}

/* non-zero when cdnet_conv_forward would run these arguments on a producer / consumer kernel: 2 = conv_ws16_kernel, 1 = conv_ws_kernel /
 * conv_ws32_kernel */
extern "C" int cdnet_conv_ws_eligible(const cdnet_conv_args *args) {
    if (!args) return 0;
    const ConvArgs &A = *reinterpret_cast<const ConvArgs *>(args);
    if (A.f32) return (!A.dot_out && conv_forward_f32_ws(A, nullptr, true) == CDNET_OK) ? 1 : 0;
    if (conv_forward_ws16(A, nullptr, true) == CDNET_OK) return 2;
    if ((A.taps1 != 0 && A.taps1 != A.taps) || A.pool_out || A.dot_out) return 0;
    if (A.debug & CONV_DBG_ONE_TILE) return 0;
    return conv_forward_ws(A, nullptr, true) == CDNET_OK ? 1 : 0;
}

extern "C" int cdnet_src_materialize(const cdnet_conv_src *src, int N, int H, int W, uint16_t *out, void *stream) {
    CDNET_REQUIRE(src && out && src->x && N > 0 && H > 0 && W > 0, "cdnet_src_materialize: bad args");
    const ConvSrc &s = *reinterpret_cast<const ConvSrc *>(src);
    CDNET_REQUIRE(s.C >= 8 && s.C % 8 == 0 && s.Hs > 0 && s.Ws > 0, "cdnet_src_materialize: C=%d must be a multiple of 8", s.C);
    CDNET_REQUIRE(!(s.pool && s.res), "cdnet_src_materialize: pooled sources carry no residual");
    CDNET_REQUIRE((s.scale == nullptr) == (s.shift == nullptr), "cdnet_src_materialize: scale and shift come together");
    if (s.f16 == 2) return materialize_f32(s, N, H, W, out, (hipStream_t)stream);
    const size_t total = (size_t)N * H * W * (s.C / 8);
    size_t g = (total + 255) / 256;
    g = g > 8192 ? 8192 : g;
    materialize_kernel<<<(int)g, 256, 0, (hipStream_t)stream>>>(s, N, H, W, out);
    return check_launch("cdnet_src_materialize");
}
