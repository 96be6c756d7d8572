// fp32-storage variant of the implicit-GEMM convolutions (the reference's precision): NHWC fp32 activations in HBM,
// every product a*b evaluated on the matrix cores as three bf16 MFMAs over split operands
//     a = a_hi + a_lo,  b = b_hi + b_lo  (hi = bf16(x), lo = bf16(x - hi): 16 significant bits each side)
//     a*b ~= a_lo*b_hi + a_hi*b_lo + a_hi*b_hi        (the dropped a_lo*b_lo term is 2^-16 of the product)
// accumulated in fp32 (v_mfma_f32_32x32x16_bf16).  gfx950 has no TF32/xf32 matrix path and its fp32 MFMA runs at 1/16 of
// the bf16 rate; three bf16 MFMAs cost 3/16 of that and keep ~fp32 products (relative error <= 2^-16 per product before
// fp32 accumulation - tighter than cuDNN's TF32 default for the reference on recent NVIDIA parts).
//
// Same cdnet_conv_args / cdnet_conv_src contract as conv.hip with args.f32 = 1: x / res / eres / out point to fp32
// tensors, `w` to the split pack (cdnet_pack_conv_weights, mode | 16: per chunk the hi image followed by the lo image).
// Differences from the 16-bit kernel: 16-channel chunks only; no pooled sources (max-pools are materialised:
// cdnet_src_materialize with f16 = 2); the tile leaves from the accumulators with 128-byte row segments (no LDS out tile).
//
// Replaces the same reference lines as conv.hip: models/dam/model_unet_rev1.py:86-170,244-287, models/unet.py:8-50,90-106.
#include <type_traits>
#include "common.h"
#include "conv_args.h"
#include "launch.h"
#include "split_bf16.h"
#include <stdlib.h>

using namespace cdnet;

namespace {

constexpr int CK = 16;
constexpr int PSTR = CK * 2 + 16;          // padded pixel stride of one LDS plane (bank-conflict-free b128 reads)
constexpr int XF_MAX = 2048;

template <int TH, int TW, int BN, int TAPS>
struct Lds32 {
    static constexpr int NPIX = (TH + 2) * (TW + 2);
    static constexpr int A_PLANE = NPIX * PSTR;
    static constexpr int B_PLANE = TAPS * CK * BN * 2;
    static constexpr int STAGE = 2 * A_PLANE + 2 * B_PLANE;
    static constexpr int STATS_BYTES = 4 * 2 * BN * 4;
    static constexpr int MAIN = ((STAGE > STATS_BYTES ? STAGE : STATS_BYTES) + 15) / 16 * 16;
    static int bytes(int ctot) { return MAIN + 2 * ((ctot + 7) / 8 * 8) * 4; }
};


// The finished tile leaves from the accumulators: lane (l31, half) of a 32 x 32 block owns output channel co and the pixels
// m0 + (r & 3) + 8 (r >> 2) + 4 half, r = 0..15.  Fast path for a full 16 x 16 tile, a full channel block and no residual input: one base
// pointer per block and 32-bit tile-relative offsets (the general path's 64-bit index arithmetic and bounds tests per element made the
// epilogue as long as the tile's MFMAs: 7.7 of 15 us per tile on the 64 -> 64 layer).
template <int MPW, int NPW, int TW>
__device__ __forceinline__ void store_tile_f32(const ConvArgs &A, const f32x16 (&acc)[MPW][NPW], int n, int y0, int x0, int mblock0, int nblock0,
                                               int half, int l31, int cout0, int pa_, int pb_) {
    const int Ho = A.H * A.ostride, Wo = A.W * A.ostride;
    float *out = reinterpret_cast<float *>(A.out);
    const float *eres = reinterpret_cast<const float *>(A.eres);
    const bool full = y0 + 16 <= A.H && x0 + TW <= A.W && cout0 + (nblock0 + NPW) * 32 <= A.Cout && A.ostride == 1 && TW == 16 &&
                      !(A.debug & 16);                       // (debug bit 16: tests compare the two epilogues bit for bit)
    if (full) {
        const int cs = A.out_cstride, ce = A.Cout;                    // (the residual input is a dense [N][H][W][Cout] tensor)
        float *tb = out + (((size_t)n * A.H + y0) * A.W + x0) * cs + A.out_coff;
        const float *te = eres ? eres + (((size_t)n * A.H + y0) * A.W + x0) * ce : nullptr;
#pragma unroll
        for (int ni = 0; ni < NPW; ++ni) {
            const int co = cout0 + (nblock0 + ni) * 32 + l31;
            const float osc = A.oscale ? A.oscale[co] : 1.f;
            const float osh = fmaf(A.bias ? A.bias[co] : 0.f, osc, A.oshift ? A.oshift[co] : 0.f);
            const float esc = (eres && A.eres_scale) ? A.eres_scale[co] : 1.f;
            const float esh = (eres && A.eres_shift) ? A.eres_shift[co] : 0.f;
            float *ob = tb + co;
#pragma unroll
            for (int mi = 0; mi < MPW; ++mi) {
                // block (mblock0 + mi): rows 2 (mblock0 + mi), +1 of the tile; this lane: pixel 4 half + (r & 3) + 8 (r >> 2) of the 32
                const int rowb = ((mblock0 + mi) * 2) * A.W + 4 * half;
                float ev[16];
                if (eres) {                        // the other branch of the residual unit, requested up front
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int p = (r & 3) + 8 * (r >> 2);
                        ev[r] = te[(rowb + (p / 16) * A.W + (p % 16)) * ce + co];
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = (r & 3) + 8 * (r >> 2);            // + 4 half: 0..31 -> (row p / 16, column p % 16); 4 half never carries
                    const int off = (rowb + (p / 16) * A.W + (p % 16)) * cs;
                    float v = fmaf(acc[mi][ni][r], osc, osh);
                    if (A.orelu) v = fmaxf(v, 0.f);
                    if (eres) {
                        v = fmaf(ev[r], esc, esh) + v;
                        if (A.eres_relu) v = fmaxf(v, 0.f);
                    }
                    ob[off] = v;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int ni = 0; ni < NPW; ++ni) {
        const int co = cout0 + (nblock0 + ni) * 32 + l31;
        const bool cok = co < A.Cout;
        const float osc = (A.oscale && cok) ? A.oscale[co] : 1.f;
        const float osh = fmaf((A.bias && cok) ? A.bias[co] : 0.f, osc, (A.oshift && cok) ? A.oshift[co] : 0.f);
        const float esc = (A.eres && A.eres_scale && cok) ? A.eres_scale[co] : 1.f;
        const float esh = (A.eres && A.eres_shift && cok) ? A.eres_shift[co] : 0.f;
#pragma unroll
        for (int mi = 0; mi < MPW; ++mi) {
            float ev[16];
            if (A.eres) {                          // the other branch of the residual unit, requested up front
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = (mblock0 + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    int y = y0 + m / TW, x = x0 + m % TW;
                    y = y < A.H ? y : A.H - 1; x = x < A.W ? x : A.W - 1;
                    ev[r] = eres[(((size_t)n * A.H + y) * A.W + x) * A.Cout + (cok ? co : 0)];
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (mblock0 + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int y = y0 + m / TW, x = x0 + m % TW;
                float v = fmaf(acc[mi][ni][r], osc, osh);
                if (A.orelu) v = fmaxf(v, 0.f);
                if (A.eres) {
                    v = fmaf(ev[r], esc, esh) + v;
                    if (A.eres_relu) v = fmaxf(v, 0.f);
                }
                if (cok && y < A.H && x < A.W) {
                    const size_t opix = ((size_t)n * Ho + (y * A.ostride + pa_)) * Wo + (x * A.ostride + pb_);
                    out[opix * A.out_cstride + A.out_coff + co] = v;
                }
            }
        }
    }
}

template <int TH, int TW, int BN, int WM, int WN, int TAPS>
__global__ __launch_bounds__(256, 2) void conv_f32_kernel(ConvArgs A) {
    using L = Lds32<TH, TW, BN, TAPS>;
    constexpr int HW_ = TW + 2, NPIX = L::NPIX;
    constexpr int MT = TH * TW / 32, NT = BN / 32;
    constexpr int MPW = MT / WM, NPW = NT / WN;
    constexpr int VPP = CK / 8;                                   // 8-channel vectors per pixel
    constexpr int NA = (NPIX * VPP + 255) / 256;                  // staged vectors per thread
    constexpr int NBV = 2 * L::B_PLANE / 16;                      // 16-byte vectors of one weight chunk (hi | lo)
    constexpr int NB = (NBV + 255) / 256;
    static_assert(MT % WM == 0 && NT % WN == 0 && WM * WN == 4, "wave tiling");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *lds_a = smem;                                  // [hi plane][lo plane]
    unsigned char *lds_b = smem + 2 * L::A_PLANE;                 // [hi image][lo image]
    float (*s_stats)[2][BN] = reinterpret_cast<float (*)[2][BN]>(smem);      // epilogue only
    float *s_xf = reinterpret_cast<float *>(smem + L::MAIN);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;
    const int c0n = A.src[0].C, ctot = c0n + (A.nsrc > 1 ? A.src[1].C : 0);
    const int xfs = (ctot + 7) / 8 * 8;
    for (int c = tid; c < ctot; c += 256) {
        const ConvSrc &S = c < c0n ? A.src[0] : A.src[1];
        const int cc = c < c0n ? c : c - c0n;
        s_xf[c] = S.scale ? S.scale[cc] : 1.f;
        s_xf[xfs + c] = S.shift ? S.shift[cc] : 0.f;
    }

    const int tiles_x = (A.W + TW - 1) / TW, tiles_y = (A.H + TH - 1) / TH;
    const int tiles_img = tiles_x * tiles_y;
    // XCD-aware order (see conv.hip): XCD k serves the k-th contiguous eighth of the (tile, cout block) sequence, the cout blocks of a
    // tile next to each other
    int tile, cout_tile;
    {
        const int NC = (int)gridDim.y, lin = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
        const int T = (int)gridDim.x * NC, q = T >> 3, rem = T & 7;
        const int xcd = lin & 7, idx = lin >> 3;
        const int seq = xcd < rem ? xcd * (q + 1) + idx : rem * (q + 1) + (xcd - rem) * q + idx;
        tile = seq / NC;
        cout_tile = seq - tile * NC;
    }
    const int z = tile / tiles_img, rt = tile - z * tiles_img;
    const int n = z / A.npar, par = z - n * A.npar;
    const int ty_ = rt / tiles_x;
    const int y0 = ty_ * TH, x0 = (rt - ty_ * tiles_x) * TW;

    // staging geometry of this thread's vectors, per source (element offset inside the image, -1 = zero fill)
    int eoff[2][NA];
    const int slot = tid % VPP;
#pragma unroll
    for (int si = 0; si < 2; ++si) {
        if (si >= A.nsrc) break;
        const ConvSrc &s = A.src[si];
        const int rs = s.row_stride ? s.row_stride : s.Ws * s.C;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int v = tid + i * 256;
            const int pix = v / VPP;
            const int hy = pix / HW_, hx = pix - hy * HW_;
            const int y = y0 - 1 + hy, x = x0 - 1 + hx;
            const int ys = y - s.off_y, xs = x - s.off_x;
            const bool ok = v < NPIX * VPP && (unsigned)y < (unsigned)A.H && (unsigned)x < (unsigned)A.W && (unsigned)ys < (unsigned)s.Hs &&
                            (unsigned)xs < (unsigned)s.Ws;
            eoff[si][i] = ok ? ys * rs + xs * s.C + slot * 8 : -1;
        }
    }
    auto chunk_src = [&](int c, int &si, int &cc0) {
        const int n0 = A.src[0].C / CK;
        if (c < n0) { si = 0; cc0 = c * CK; } else { si = 1; cc0 = (c - n0) * CK; }
    };
    const unsigned short *wbase = A.w + ((size_t)(par * gridDim.y + cout_tile) * A.nchunk) * (size_t)(L::B_PLANE);      // u16 elements: 2 planes x B_PLANE/2

    // register prefetch of one chunk: halo vectors (two float4 each) and the weight image
    f32x4 pa[NA][2];
    u32x4 pb[NB];
    auto issue = [&](int chunk) {
        int si, cc0;
        chunk_src(chunk, si, cc0);
        const ConvSrc &s = A.src[si];
        const size_t rs = s.row_stride ? (size_t)s.row_stride : (size_t)s.Ws * s.C;
        const float *base = reinterpret_cast<const float *>(s.x) + (size_t)n * s.Hs * rs + cc0;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = si ? eoff[1][i] : eoff[0][i];
            const f32x4 *p = reinterpret_cast<const f32x4 *>(base + (e >= 0 ? e : 0));
            pa[i][0] = p[0];
            pa[i][1] = p[1];
        }
        const u32x4 *wsrc = reinterpret_cast<const u32x4 *>(wbase + (size_t)chunk * L::B_PLANE);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int v = tid + i * 256;
            if (v < NBV) pb[i] = wsrc[v];
        }
    };
    auto commit = [&](int chunk) {
        int si, cc0;
        chunk_src(chunk, si, cc0);
        const ConvSrc &s = A.src[si];
        const bool on = s.scale != nullptr, relu = s.relu != 0;
        const float *xf = s_xf + (si ? c0n : 0) + cc0 + slot * 8;
        float sc[8], sh[8];
        if (on) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { sc[j] = xf[j]; sh[j] = xf[xfs + j]; }
        }
        f32x4 rr[NA][2];
        if (s.res) {
            const size_t rs = s.row_stride ? (size_t)s.row_stride : (size_t)s.Ws * s.C;
            const float *rbase = reinterpret_cast<const float *>(s.res) + (size_t)n * s.Hs * rs + cc0;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int e = si ? eoff[1][i] : eoff[0][i];
                const f32x4 *p = reinterpret_cast<const f32x4 *>(rbase + (e >= 0 ? e : 0));
                rr[i][0] = p[0];
                rr[i][1] = p[1];
            }
        }
        unsigned char *dst0 = lds_a + (tid / VPP) * PSTR + slot * 16;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if (tid + i * 256 >= NPIX * VPP) continue;
            const int e = si ? eoff[1][i] : eoff[0][i];
            u32x4 hi = {0u, 0u, 0u, 0u}, lo = {0u, 0u, 0u, 0u};
            if (e >= 0) {
                float v[8] = {pa[i][0][0], pa[i][0][1], pa[i][0][2], pa[i][0][3], pa[i][1][0], pa[i][1][1], pa[i][1][2], pa[i][1][3]};
                if (on) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = fmaf(v[j], sc[j], sh[j]);
                }
                if (s.res) {
                    const float r[8] = {rr[i][0][0], rr[i][0][1], rr[i][0][2], rr[i][0][3], rr[i][1][0], rr[i][1][1], rr[i][1][2], rr[i][1][3]};
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] += r[j];
                }
                if (relu) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
                }
                split8(v, hi, lo);
            }
            unsigned char *d = dst0 + i * (256 / VPP) * PSTR;
            *reinterpret_cast<u32x4 *>(d) = hi;
            *reinterpret_cast<u32x4 *>(d + L::A_PLANE) = lo;
        }
        u32x4 *bdst = reinterpret_cast<u32x4 *>(lds_b);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int v = tid + i * 256;
            if (v < NBV) bdst[v] = pb[i];
        }
    };

    int abase[MPW];
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
        const int m = (wm * MPW + mi) * 32 + l31;
        abase[mi] = ((m / TW) * HW_ + m % TW) * PSTR + half * 16;
    }
    const int bbase = half * BN * 16 + (wn * NPW * 32 + l31) * 16;
    int toff[TAPS];
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
    }
    f32x16 acc[MPW][NPW];
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
        for (int ni = 0; ni < NPW; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    issue(0);
    for (int chunk = 0; chunk < A.nchunk; ++chunk) {
        __syncthreads();                          // the previous chunk's fragment reads are done (first pass: the xf table is written)
        commit(chunk);
        __syncthreads();
        if (chunk + 1 < A.nchunk) issue(chunk + 1);
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            bf16x8 ah[MPW], al[MPW], bh[NPW], bl[NPW];
#pragma unroll
            for (int mi = 0; mi < MPW; ++mi) {
                ah[mi] = *reinterpret_cast<const bf16x8 *>(lds_a + abase[mi] + toff[t]);
                al[mi] = *reinterpret_cast<const bf16x8 *>(lds_a + L::A_PLANE + abase[mi] + toff[t]);
            }
#pragma unroll
            for (int ni = 0; ni < NPW; ++ni) {
                bh[ni] = *reinterpret_cast<const bf16x8 *>(lds_b + bbase + t * 2 * BN * 16 + ni * 512);
                bl[ni] = *reinterpret_cast<const bf16x8 *>(lds_b + L::B_PLANE + bbase + t * 2 * BN * 16 + ni * 512);
            }
#pragma unroll
            for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
                for (int ni = 0; ni < NPW; ++ni) {
                    acc[mi][ni] = mfma3(acc[mi][ni], ah[mi], al[mi], bh[ni], bl[ni]);
                }
        }
    }
    __syncthreads();

    // ---------------- epilogue ----------------
    const int cout0 = cout_tile * BN;
    if (A.stats) {
        float ssum[NPW], ssq[NPW];
        const bool full_tile = y0 + TH <= A.H && x0 + TW <= A.W && !(A.debug & 16);      // (no per-element bounds tests then; the sums are the same)
#pragma unroll
        for (int ni = 0; ni < NPW; ++ni) {
            ssum[ni] = 0.f; ssq[ni] = 0.f;
            if (full_tile) {
#pragma unroll
                for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = acc[mi][ni][r];
                        ssum[ni] += v;
                        ssq[ni] = fmaf(v, v, ssq[ni]);
                    }
            } else {
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
            ssum[ni] += __shfl_xor(ssum[ni], 32);
            ssq[ni] += __shfl_xor(ssq[ni], 32);
            if (half == 0) {
                s_stats[wave][0][(wn * NPW + ni) * 32 + l31] = ssum[ni];
                s_stats[wave][1][(wn * NPW + ni) * 32 + l31] = ssq[ni];
            }
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, col = tid % BN;
            const int wn_of = col / (NPW * 32);
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < WM; ++k) v += s_stats[k * WN + wn_of][which][col];
            const int co = cout0 + col;
            if (co < A.Cout) A.stats[((size_t)tile * 2 + which) * A.Cout + co] = v;
        }
    }
    // a lane owns one output channel; lanes 0..31 / 32..63 write two 128-byte row segments per instruction
    store_tile_f32<MPW, NPW, TW>(A, acc, n, y0, x0, wm * MPW, wn * NPW, half, l31, cout0, par >> 1, par & 1);
}

template <int TH, int TW, int BN, int WM, int WN, int TAPS>
int launch_conv32(const ConvArgs &A, hipStream_t st) {
    using L = Lds32<TH, TW, BN, TAPS>;
    int ctot = 0;
    for (int i = 0; i < A.nsrc; ++i) ctot += A.src[i].C;
    const int smem = L::bytes(ctot);
    dim3 grid(cdiv(A.W, TW) * cdiv(A.H, TH) * A.N * A.npar, cdiv(A.Cout, BN), 1);
    g_conv_last_form = conv_form(CDNET_CONV_FAMILY_F32, BN, TAPS, 0, false, false, false, 0, 0, TH);
    return launch_lds<conv_f32_kernel<TH, TW, BN, WM, WN, TAPS>>(grid, 256, L::bytes(XF_MAX), smem, st, "hipFuncSetAttribute(conv32)", "conv_f32_kernel", A);
}

template <int TAPS>
int dispatch_conv32(const ConvArgs &A, hipStream_t st) {
    if (A.tile == 16 && A.BN == 64) return launch_conv32<16, 16, 64, 4, 1, TAPS>(A, st);
    if (A.tile == 16 && A.BN == 32) return launch_conv32<16, 16, 32, 4, 1, TAPS>(A, st);
    if (A.tile == 8 && A.BN == 64) return launch_conv32<8, 8, 64, 2, 2, TAPS>(A, st);
    set_error("cdnet_conv_forward(f32): unsupported configuration tile=%d CK=%d BN=%d", A.tile, A.CK, A.BN);
    return CDNET_E_ARG;
}

// ----------------------------------------------------------------------------------------------------------------------------------
// 1x1 convolution over one dense source as the plain GEMM it is: [pixels x Cin] . [Cin x Cout], no halo, no tile geometry.  A wave
// works alone on blocks of 32 consecutive NHWC pixels (block index striding over the grid): lane (l31, half) loads the 8 fp32
// channels of k-half `half` of every chunk of pixel l31 straight from HBM (two 16-byte vectors per chunk - the A fragment's own
// channels), transforms and splits them in registers and issues the MFMAs against B fragments read from the workgroup's LDS copy of
// the split pack (written once, the only barrier).  The next block's loads are requested before this block's MFMAs, the other
// branch of a residual unit (eres) after them, into the registers the inputs have left.
// Same arithmetic as conv_f32_kernel per output element - chunks ascending, a_lo b_hi, a_hi b_lo, a_hi b_hi per chunk, commit()'s
// source transform, store_tile_f32's epilogue - so the outputs agree bit for bit (which pixel sits in which MFMA row enters no
// output element).  The tail block's missing pixels are outside its buffer descriptors' range: read as zero, not written.
// ----------------------------------------------------------------------------------------------------------------------------------
template <int BN, int NCH, bool XF, bool ERES>
__global__ __launch_bounds__(256, 4) void conv1x1_f32_stream_kernel(ConvArgs A) {
    constexpr int NPW = BN / 32;
    constexpr int B_PLANE = CK * BN * 2;                          // bytes of one weight image (hi or lo) of one chunk
    constexpr int CIN = NCH * CK;
    __shared__ __attribute__((aligned(16))) unsigned char smem[NCH * 2 * B_PLANE + 2 * CIN * 4];
    unsigned char *lds_b = smem;                                  // per chunk [hi image][lo image]
    float *s_xf = reinterpret_cast<float *>(smem + NCH * 2 * B_PLANE);       // [scale][shift] of the source

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int cout_tile = blockIdx.y, cout0 = cout_tile * BN;
    const ConvSrc &S = A.src[0];
    {
        const u32x4 *wsrc = reinterpret_cast<const u32x4 *>(A.w + (size_t)cout_tile * NCH * B_PLANE);       // u16 elements: 2 planes x B_PLANE / 2
        u32x4 *bdst = reinterpret_cast<u32x4 *>(lds_b);
        for (int v = tid; v < NCH * 2 * B_PLANE / 16; v += 256) bdst[v] = wsrc[v];
        for (int c = tid; c < CIN; c += 256) {
            s_xf[c] = S.scale ? S.scale[c] : 1.f;
            s_xf[CIN + c] = S.shift ? S.shift[c] : 0.f;
        }
    }
    __syncthreads();

    const size_t P = (size_t)A.N * A.H * A.W;
    const int nblk = (int)((P + 31) / 32), bstride = (int)gridDim.x * 4;
    int blk = (int)blockIdx.x * 4 + wave;
    if (blk >= nblk) return;
    const bool relu = S.relu != 0, orelu = A.orelu != 0, eres_relu = A.eres_relu != 0;
    const int cout = A.Cout;
    const int bbase = half * BN * 16 + l31 * 16;

    // per output channel, as store_tile_f32 forms them
    float osc[NPW], osh[NPW], esc[NPW], esh[NPW];
#pragma unroll
    for (int ni = 0; ni < NPW; ++ni) {
        const int co = cout0 + ni * 32 + l31, c = co < A.Cout ? co : 0;
        osc[ni] = A.oscale ? A.oscale[c] : 1.f;
        osh[ni] = fmaf(A.bias ? A.bias[c] : 0.f, osc[ni], A.oshift ? A.oshift[c] : 0.f);
        esc[ni] = (ERES && A.eres_scale) ? A.eres_scale[c] : 1.f;
        esh[ni] = (ERES && A.eres_shift) ? A.eres_shift[c] : 0.f;
    }

    // Every access goes through a buffer descriptor of its block (base = the block's first pixel, range = its pixels) with a 32-bit byte
    // offset of the lane: a lane without an output channel (co >= Cout) carries an offset outside every range, and what lies past the
    // tail block's last pixel reads as zero and is not written.  The row of the block is a scalar offset in full blocks (one address
    // register per lane and channel block); the range check does not see scalar offsets, so the tail block adds the row to the lane's.
    const char *xbase = reinterpret_cast<const char *>(S.x);
    char *obase = reinterpret_cast<char *>(A.out) + (size_t)A.out_coff * 4;
    const char *ebase = ERES ? reinterpret_cast<const char *>(A.eres) : xbase;
    const unsigned cs4 = (unsigned)A.out_cstride * 4, ce4 = (unsigned)cout * 4;
    const unsigned vo_in = l31 * (CIN * 4) + half * 32;
    unsigned vo_out[NPW], vo_eres[NPW];
#pragma unroll
    for (int ni = 0; ni < NPW; ++ni) {
        const unsigned co = cout0 + ni * 32 + l31;
        vo_out[ni] = co < (unsigned)cout ? 4 * half * cs4 + co * 4 : 0x7fff0000u;
        vo_eres[ni] = co < (unsigned)cout ? 4 * half * ce4 + co * 4 : 0x7fff0000u;
    }
    auto rsrc = [&](const char *base, size_t bytes) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base), 0, (int)bytes, 0x00020000);
    };

    auto request = [&](f32x4 (&v)[NCH][2], int b) {
        const size_t left = P - (size_t)b * 32;
        const __amdgpu_buffer_rsrc_t rx = rsrc(xbase + (size_t)b * (32 * CIN * 4), (left < 32 ? left : 32) * (CIN * 4));
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            v[c][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(vo_in + c * 64), 0, 0));
            v[c][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(vo_in + c * 64 + 16), 0, 0));
        }
    };
    auto block = [&](auto tail_c, const f32x4 (&cur)[NCH][2], f32x4 (&nxt)[NCH][2]) {
        constexpr bool TAIL = decltype(tail_c)::value;
        asm volatile("" ::: "memory");                           // (the B fragments are read from LDS block by block, not held in 16 NCH NPW registers)
        if (!TAIL) {
            request(nxt, blk + bstride < nblk ? blk + bstride : blk);    // (after the last block: the same again, no branch)
            __builtin_amdgcn_sched_barrier(0);                    // these requests stay in front of the MFMAs
        }
        f32x16 acc[NPW];
#pragma unroll
        for (int ni = 0; ni < NPW; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ni][r] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            float v[8] = {cur[c][0][0], cur[c][0][1], cur[c][0][2], cur[c][0][3], cur[c][1][0], cur[c][1][1], cur[c][1][2], cur[c][1][3]};
            if (XF) {                                              // (a ReLU comes with a scale / shift here: the dispatcher sees to it)
                const float *xf = s_xf + c * CK + half * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    v[j] = fmaf(v[j], xf[j], xf[CIN + j]);
                    v[j] = relu ? fmaxf(v[j], 0.f) : v[j];
                }
            }
            u32x4 hi, lo;
            split8(v, hi, lo);
            const bf16x8 ah = __builtin_bit_cast(bf16x8, hi), al = __builtin_bit_cast(bf16x8, lo);
#pragma unroll
            for (int ni = 0; ni < NPW; ++ni) {
                const bf16x8 bh = *reinterpret_cast<const bf16x8 *>(lds_b + c * 2 * B_PLANE + bbase + ni * 512);
                const bf16x8 bl = *reinterpret_cast<const bf16x8 *>(lds_b + c * 2 * B_PLANE + B_PLANE + bbase + ni * 512);
                acc[ni] = mfma3(acc[ni], ah, al, bh, bl);
            }
        }
        // a lane owns one output channel and the pixels (r & 3) + 8 (r >> 2) + 4 half of the block; lanes 0..31 / 32..63 write two 128-byte
        // pixel segments per instruction
        const size_t left = P - (size_t)blk * 32, rows = left < 32 ? left : 32;
        const __amdgpu_buffer_rsrc_t ro = rsrc(obase + (size_t)blk * 32 * cs4, rows * cs4);
        float ev[NPW][16];
        if (ERES) {                                                // the other branch of the residual unit
            const __amdgpu_buffer_rsrc_t re = rsrc(ebase + (size_t)blk * 32 * ce4, rows * ce4);
#pragma unroll
            for (int ni = 0; ni < NPW; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned pr = (r & 3) + 8 * (r >> 2);
                    ev[ni][r] = __builtin_bit_cast(float, TAIL ? __builtin_amdgcn_raw_buffer_load_b32(re, (int)(vo_eres[ni] + pr * ce4), 0, 0)
                                                               : __builtin_amdgcn_raw_buffer_load_b32(re, (int)vo_eres[ni], (int)(pr * ce4), 0));
                }
        }
#pragma unroll
        for (int ni = 0; ni < NPW; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned pr = (r & 3) + 8 * (r >> 2);
                float v = fmaf(acc[ni][r], osc[ni], osh[ni]);
                v = orelu ? fmaxf(v, 0.f) : v;
                if (ERES) {
                    v = fmaf(ev[ni][r], esc[ni], esh[ni]) + v;
                    v = eres_relu ? fmaxf(v, 0.f) : v;
                }
                if (TAIL) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ro, (int)(vo_out[ni] + pr * cs4), 0, 0);
                else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ro, (int)vo_out[ni], (int)(pr * cs4), 0);
            }
    };
    // two register sets take turns (a copy of one into the other would wait for the block's stores as well)
    f32x4 xa[NCH][2], xb[NCH][2];
    const int nfull = (int)(P / 32);
    if (blk < nfull) {
        request(xa, blk);
#pragma unroll
        for (int c = 0; c < NCH; ++c) asm volatile("" ::"v"(xa[c][0]), "v"(xa[c][1]));       // (arrived: the loop's own waits then never count this request, which would make them wait for a block's stores)
        for (;;) {
            block(std::false_type{}, xa, xb);
            blk += bstride;
            if (blk >= nfull) break;
            block(std::false_type{}, xb, xa);
            blk += bstride;
            if (blk >= nfull) break;
        }
    }
    if (blk < nblk) {                                             // (the tail block asks again for what the last block may have requested)
        request(xa, blk);
        block(std::true_type{}, xa, xb);
    }
}

template <int BN, int NCH>
int launch_conv1x1_stream(const ConvArgs &A, hipStream_t st) {
    int n_cu = 0;
    if (const int rc = cu_count(&n_cu)) return rc;
    // sixteen waves per CU are resident; every wave gets the same number of pixel blocks, give or take one
    const long long nblk = ((long long)A.N * A.H * A.W + 31) / 32;
    const int ctiles = cdiv(A.Cout, BN);
    const long long waves = (long long)n_cu * 16 / ctiles > 4 ? (long long)n_cu * 16 / ctiles : 4;
    const long long rounds = (nblk + waves - 1) / waves;
    const long long G = ((nblk + rounds - 1) / rounds + 3) / 4;
    dim3 grid((unsigned)G, ctiles, 1);
    return with_bool(A.src[0].scale != nullptr, [&](auto xf_c) {
        return with_bool(A.eres != nullptr, [&](auto er_c) {
            g_conv_last_form = conv_form(CDNET_CONV_FAMILY_STREAM, BN, 1, decltype(xf_c)::value ? 1 : 0, false, false, false, 0, 0, 16, 16, NCH, decltype(er_c)::value);
            conv1x1_f32_stream_kernel<BN, NCH, decltype(xf_c)::value, decltype(er_c)::value><<<grid, 256, 0, st>>>(A);
            return check_launch("conv1x1_f32_stream_kernel");
        });
    });
}

// -1 = not this kernel's launch (the caller goes on to conv_f32_kernel)
int try_conv1x1_stream(const ConvArgs &A, hipStream_t st) {
    if (A.debug & CONV_DBG_NO_STREAM_1X1) return -1;                                 // tests / A-B: conv_f32_kernel instead
    if (A.taps != 1 || A.taps1 != 0 || A.npar != 1 || A.ostride != 1 || A.ws || A.stats || A.pool_out || A.nsrc != 1) return -1;
    const ConvSrc &s = A.src[0];
    if (s.off_y || s.off_x || s.Hs != A.H || s.Ws != A.W || (s.row_stride && s.row_stride != s.Ws * s.C) || s.pool || s.res) return -1;
    if (s.relu && !s.scale) return -1;                           // (no instantiation for a ReLU without scale / shift)
    if (s.C != A.nchunk * CK || (long long)A.N * A.H * A.W > (1LL << 31) - 64 || (long long)A.out_cstride * 4 * 36 >= (1LL << 31)) return -1;
    auto go = [&](auto bn_c) -> int {
        constexpr int BN = decltype(bn_c)::value;
        if (A.nchunk == 1) return launch_conv1x1_stream<BN, 1>(A, st);
        if (A.nchunk == 2) return launch_conv1x1_stream<BN, 2>(A, st);
        if (A.nchunk == 4) return launch_conv1x1_stream<BN, 4>(A, st);
        return -1;
    };
    if (A.BN == 64) return go(std::integral_constant<int, 64>{});
    if (A.BN == 32) return go(std::integral_constant<int, 32>{});
    return -1;
}

// fp32 variant of materialize_kernel (conv.hip): the source with its pending transform (scale/shift, residual, ReLU, 2x2
// max-pool floor / ceil mode, pad offset) written out as a plain fp32 tensor
__global__ __launch_bounds__(256) void materialize_f32_kernel(const ConvSrc s, int N, int H, int W, float *__restrict__ out) {
    const int VPP = s.C / 4;
    const size_t total = (size_t)N * H * W * VPP;
    const bool relu = s.relu != 0, on = s.scale != nullptr;
    const int Hl = s.pool ? (s.Hs + (s.pool == 2)) / 2 : s.Hs, Wl = s.pool ? (s.Ws + (s.pool == 2)) / 2 : s.Ws;
    const size_t rs = s.row_stride ? (size_t)s.row_stride : (size_t)s.Ws * s.C;
    const float *sx = reinterpret_cast<const float *>(s.x), *sr = reinterpret_cast<const float *>(s.res);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % VPP) * 4;
        const size_t pix = i / VPP;
        const int x = (int)(pix % W), y = (int)((pix / W) % H), n = (int)(pix / ((size_t)W * H));
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) { sc = *reinterpret_cast<const float4 *>(s.scale + c); sh = *reinterpret_cast<const float4 *>(s.shift + c); }
        const size_t img = (size_t)n * s.Hs * rs;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        const int ys = y - s.off_y, xs = x - s.off_x;
        auto xf = [&](float4 v, const float4 *r) {
            v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y); v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
            if (r) { v.x += r->x; v.y += r->y; v.z += r->z; v.w += r->w; }
            if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            return v;
        };
        if (ys >= 0 && ys < Hl && xs >= 0 && xs < Wl) {
            if (!s.pool) {
                const size_t e = img + (size_t)ys * rs + (size_t)xs * s.C + c;
                const float4 raw = *reinterpret_cast<const float4 *>(sx + e);
                if (sr) { const float4 r = *reinterpret_cast<const float4 *>(sr + e); val = xf(raw, &r); }
                else val = xf(raw, nullptr);
            } else {
                float4 raw[4];
                bool ok[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    int yy = 2 * ys + (q >> 1), xx = 2 * xs + (q & 1);
                    ok[q] = q == 0 || (yy < s.Hs && xx < s.Ws);
                    yy = yy < s.Hs ? yy : s.Hs - 1;
                    xx = xx < s.Ws ? xx : s.Ws - 1;
                    raw[q] = *reinterpret_cast<const float4 *>(sx + img + (size_t)yy * rs + (size_t)xx * s.C + c);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 t = xf(raw[q], nullptr);
                    if (q == 0) val = t;
                    else if (ok[q]) { val.x = fmaxf(val.x, t.x); val.y = fmaxf(val.y, t.y); val.z = fmaxf(val.z, t.z); val.w = fmaxf(val.w, t.w); }
                }
            }
        }
        *reinterpret_cast<float4 *>(out + pix * s.C + c) = val;
    }
}

}  // namespace

namespace cdnet {

int conv_forward_f32(const ConvArgs &A, hipStream_t st) {
    CDNET_REQUIRE(A.CK == 16, "cdnet_conv_forward(f32): CK must be 16 (got %d)", A.CK);
    for (int i = 0; i < A.nsrc; ++i)
        CDNET_REQUIRE(!A.src[i].pool, "cdnet_conv_forward(f32): pooled sources must be materialised (cdnet_src_materialize)");
    CDNET_REQUIRE(!A.out_f16, "cdnet_conv_forward(f32): out_f16 must be 0");
    {
        const int rc = conv_forward_f32_ws(A, st);               // the producer / consumer kernel where it applies
        if (rc >= 0) return rc;
    }
    CDNET_REQUIRE(A.ws != 2, "cdnet_conv_forward(f32): the BatchNorm-backward statistics epilogue (ws = 2) needs the producer / consumer kernel "
                             "(ask cdnet_conv_ws_eligible first)");
    CDNET_REQUIRE(A.taps1 == 0 || A.taps1 == A.taps, "cdnet_conv_forward(f32): a one-tap second source runs on conv_ws32_kernel only (ask cdnet_conv_ws_eligible)");
    CDNET_REQUIRE(!A.pool_out, "cdnet_conv_forward(f32): the fused max-pool output rides in conv_ws32_kernel's epilogue only (ask cdnet_conv_ws_eligible)");
    if (A.taps == 9) return dispatch_conv32<9>(A, st);
    if (A.taps == 4) return dispatch_conv32<4>(A, st);
    {
        const int rc = try_conv1x1_stream(A, st);                // one dense source, a few chunks: the halo-free streaming kernel
        if (rc >= 0) return rc;
    }
    return dispatch_conv32<1>(A, st);
}

int materialize_f32(const ConvSrc &s, int N, int H, int W, void *out, hipStream_t st) {
    const size_t total = (size_t)N * H * W * (s.C / 4);
    size_t g = (total + 255) / 256;
    g = g > 8192 ? 8192 : g;
    materialize_f32_kernel<<<(int)g, 256, 0, st>>>(s, N, H, W, reinterpret_cast<float *>(out));
    return check_launch("cdnet_src_materialize(f32)");
}

}  // namespace cdnet
