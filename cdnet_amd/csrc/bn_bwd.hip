// BatchNorm + ReLU (+ residual) (+ consumers' max-pool / F.pad) backward: two streaming passes (HBM-bound) around a per-channel
// finalize.  The sums pass leaves one [2][C] row per workgroup, summed in a fixed order, so the result is bit-reproducible.
//
// Three access patterns, each in a 16-bit (8 channels per thread) and an fp32 (4 channels per thread) version; every kernel takes the pass
// as `template <bool APPLY>`:
//   window  : one 2x2 max-pool consumer + up to two same-size un-shifted ones        bn_bwd_window_kernel / bn_bwd_window32_kernel
//   flat    : every gradient source a same-size un-shifted tensor                     bn_bwd_flat_kernel / bn_bwd_flat32_kernel
//   generic : anything else (F.pad offsets, pool + residual, ...), per-pixel routing  bn_bwd_generic_kernel<F32>
// The two precisions stay separate kernels on purpose: channels per thread fix the pixel-to-thread map and so the order of every sum.
//
// Replaces loss.backward() (train_util_dam.py:307) for nn.BatchNorm2d / F.relu / the residual add / nn.MaxPool2d / F.pad.
#include "train_util.h"
#include "bn_sums.h"

using namespace cdnet;

namespace {

struct GradIn {
    const unsigned short *g;     // bf16 NHWC [N][Hg][Wg][C]: gradient w.r.t. this tensor as seen by one consumer
    int Hg, Wg;
    int oy, ox;                  // consumer read (y - oy, x - ox) of this tensor  => gradient sits at (y + oy, x + ox)
    int pooled;                  // consumer read maxpool2x2 of this tensor (1 floor / 2 ceil): route to the argmax
    int coff, cstride;           // channel slice of a wider gradient tensor
};

struct BnBwdArgs {
    const unsigned short *raw;   // stored forward output [N][H][W][C]
    const unsigned short *res;   // optional residual added before the ReLU
    int f16;                     // storage format of raw/res
    const float *scale, *shift;  // forward affine (NULL: identity)
    int relu;
    const float *mean, *invstd;  // saved batch statistics
    GradIn gin[3];
    int ngin;
    int N, H, W, C;
    float *partial;              // reduce: [nblocks][2][C]
    const float *k1, *k2, *k3;   // apply: draw = k1*(dz - k2 - xhat*k3)
    unsigned short *draw;        // bf16 [N][H][W][C]
    unsigned short *dz_out;      // optional bf16 copy of dz (gradient of the residual branch)
    int rev;                     // apply pass walks the tensor back to front (see cdnet_bn_backward)
    const float *hc_coef, *hc_w; // head-coefficient source (cdnet_bn_bwd_args.hc_*): rows f32 [px][16], weights f32 [hc_nk][64]
    int hc_slot, hc_nk;          // ... its position among the sources, 3 or 9 terms (0: none); first column HC_K0(hc_nk), checked by the host
};


// fp32 tensors (f16 == 2): the activated value in plain fp32 arithmetic; relu == 2: `res` is the stored post-ReLU output of the
// unit (fused residual epilogue) and the mask is read from it
__device__ __forceinline__ void act8_f32(const BnBwdArgs &A, size_t e, const float *sc, const float *sh, float *a, float *rawf) {
    float x[8], r[8];
    ldf8(A.raw, e, x);
    if (A.res) ldf8(A.res, e, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (rawf) rawf[j] = x[j];
        float v = A.scale ? fmaf(x[j], sc[j], sh[j]) : x[j];
        if (A.relu == 2) v = r[j];
        else {
            if (A.res) v += r[j];
            if (A.relu) v = fmaxf(v, 0.f);
        }
        a[j] = v;
    }
}

// activated value (rounded to bf16 like the forward staging does) of 8 channels at one pixel
template <bool F32 = false>
__device__ __forceinline__ void act8(const BnBwdArgs &A, size_t e, const float *sc, const float *sh, float *a, float *rawf) {
    if (F32) { act8_f32(A, e, sc, sh, a, rawf); return; }
    V16 r, rr;
    r.u = *reinterpret_cast<const uint4 *>(A.raw + e);
    rr.u = make_uint4(0, 0, 0, 0);
    if (A.res) rr.u = *reinterpret_cast<const uint4 *>(A.res + e);
    const bool f16 = A.f16 != 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float x = ld16(r.h[j], f16);
        if (rawf) rawf[j] = x;
        float v = A.scale ? fmaf(x, sc[j], sh[j]) : x;
        if (A.res) v += ld16(rr.h[j], f16);
        if (A.relu) v = fmaxf(v, 0.f);
        a[j] = bf2f(f2bf(v));
    }
}

// dz for 8 channels of pixel (n,y,x); also returns xhat
template <bool WANT_XHAT, bool F32 = false>
__device__ __forceinline__ void dz8(const BnBwdArgs &A, int n, int y, int x, int c0, const float *sc, const float *sh,
                                    const float *mu, const float *is, float *dz, float *xhat) {
    const size_t e = (((size_t)n * A.H + y) * A.W + x) * A.C + c0;
    float a[8], rawf[8];
    act8<F32>(A, e, sc, sh, a, rawf);
    float g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = 0.f;
    for (int k = 0; k < A.ngin; ++k) {
        const GradIn &gi = A.gin[k];
        if (!gi.pooled) {
            const int yy = y + gi.oy, xx = x + gi.ox;
            if (yy >= 0 && yy < gi.Hg && xx >= 0 && xx < gi.Wg) {
                const size_t ge = (((size_t)n * gi.Hg + yy) * gi.Wg + xx) * gi.cstride + gi.coff + c0;
                if (F32) {
                    float t[8];
                    ldf8(gi.g, ge, t);
#pragma unroll
                    for (int j = 0; j < 8; ++j) g[j] += t[j];
                } else {
                    V16 v;
                    v.u = *reinterpret_cast<const uint4 *>(gi.g + ge);
#pragma unroll
                    for (int j = 0; j < 8; ++j) g[j] += bf2f(v.h[j]);
                }
            }
        } else {
            const int py = y >> 1, px = x >> 1;
            if (py < gi.Hg && px < gi.Wg) {
                // is (y,x) the first maximum of its 2x2 window?  (nn.MaxPool2d backward)
                bool sel[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) sel[j] = true;
                const int q0 = (y & 1) * 2 + (x & 1);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q == q0) continue;
                    const int yy = (y & ~1) + (q >> 1), xx = (x & ~1) + (q & 1);
                    if (yy >= A.H || xx >= A.W) continue;
                    float b[8];
                    act8<F32>(A, (((size_t)n * A.H + yy) * A.W + xx) * A.C + c0, sc, sh, b, nullptr);
#pragma unroll
                    for (int j = 0; j < 8; ++j) sel[j] = sel[j] && (q < q0 ? a[j] > b[j] : a[j] >= b[j]);
                }
                const size_t ge = (((size_t)n * gi.Hg + py) * gi.Wg + px) * gi.cstride + gi.coff + c0;
                if (F32) {
                    float t[8];
                    ldf8(gi.g, ge, t);
#pragma unroll
                    for (int j = 0; j < 8; ++j) g[j] += sel[j] ? t[j] : 0.f;
                } else {
                    V16 v;
                    v.u = *reinterpret_cast<const uint4 *>(gi.g + ge);
#pragma unroll
                    for (int j = 0; j < 8; ++j) g[j] += sel[j] ? bf2f(v.h[j]) : 0.f;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        dz[j] = (A.relu && !(a[j] > 0.f)) ? 0.f : g[j];
        if (WANT_XHAT) xhat[j] = A.mean ? (rawf[j] - mu[j]) * is[j] : 0.f;
    }
}

// V per-channel constants of a thread from one of the [C] arrays; a NULL array gives the identity value
template <int V>
__device__ __forceinline__ void bn_load_row(const float *p, int c0, float *o, float dflt) {
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = p ? p[c0 + j] : dflt;
}

// all per-channel constants of a thread's V channels (V = 8: 16-bit and generic kernels, V = 4: fp32); k1..k3 in the apply pass only
template <int V>
__device__ __forceinline__ void bn_load_const(const BnBwdArgs &A, int c0, bool apply, float (&sc)[V], float (&sh)[V], float (&mu)[V], float (&is)[V],
                                              float (&k1)[V], float (&k2)[V], float (&k3)[V]) {
    bn_load_row<V>(A.scale, c0, sc, 1.f); bn_load_row<V>(A.shift, c0, sh, 0.f); bn_load_row<V>(A.mean, c0, mu, 0.f); bn_load_row<V>(A.invstd, c0, is, 1.f);
    if (apply) { bn_load_row<V>(A.k1, c0, k1, 1.f); bn_load_row<V>(A.k2, c0, k2, 0.f); bn_load_row<V>(A.k3, c0, k3, 0.f); }
}

// Block epilogue of the sums pass: row blockIdx.x of partial[nblocks][2][C].  Threads with the same slot (tid, tid + VPP, ...) hold
// the same channels: their s1 / s2 go through LDS and are summed in ascending thread order, the 2 * V values x VPP slots spread over
// the block.
template <int V>
__device__ __forceinline__ void bn_write_partial(float *partial, int C, int VPP, const float *s1, const float *s2) {
    __shared__ float s_red[256][2 * V + 1];
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < V; ++j) { s_red[tid][j] = s1[j]; s_red[tid][V + j] = s2[j]; }
    __syncthreads();
    for (int q = tid; q < 2 * V * VPP; q += 256) {
        const int sl = q % VPP, j = q / VPP;
        float t = 0.f;
        for (int k = sl; k < 256; k += VPP) t += s_red[k][j];
        float *op = partial + (size_t)blockIdx.x * 2 * C;
        op[(j / V) * C + sl * V + (j % V)] = t;
    }
}

// Both passes are pure streaming (HBM bound): every thread keeps BN_U independent pixels in flight per iteration.
constexpr int BN_U = 4;
constexpr int BN_MAX_BLOCKS = 2048;      // workspace rows
// blocks actually launched by the streaming passes: two 256-thread workgroups per CU keep 64-98 KB of loads in flight per CU, and the
// finalize pass (one workgroup per channel walking the partial rows with a 2 * C stride) has a quarter of the rows to sum - measured
// (bench.py, 16 tiles): 2048 blocks 1 641 tiles/s, 1024 1 645-1 655, 768 1 652-1 655, 512 1 654-1 663, 256 1 605-1 609
constexpr int BN_BLOCKS_CAP = 512;
static_assert(BN_BLOCKS_CAP <= BN_MAX_BLOCKS, "workspace rows");

// workgroups of a pass over `count` pixels (or pool windows): V channels per thread, `unroll` of them in flight per thread and trip.
// bn_bwd_finalize_kernel's result depends on the number of partial rows, so this is part of the arithmetic.
static int bn_grid(size_t count, int C, int V, int unroll) {
    const size_t per_block = (size_t)(256 / (C / V)) * unroll;
    const size_t nb = (count + per_block - 1) / per_block;
    return nb > (size_t)BN_BLOCKS_CAP ? BN_BLOCKS_CAP : (nb < 1 ? 1 : (int)nb);
}

template <bool F32 = false>
__device__ __forceinline__ void dz8_at(const BnBwdArgs &A, unsigned p, unsigned HW, int c0, const float *sc, const float *sh, const float *mu,
                                       const float *is, float *dz, float *xh) {
    const unsigned n = p / HW, r = p - n * HW;
    const unsigned y = r / (unsigned)A.W, x = r - y * (unsigned)A.W;
    dz8<true, F32>(A, (int)n, (int)y, (int)x, c0, sc, sh, mu, is, dz, xh);
}

// The storage format of the raw tensor (fp16 / bf16) and the ReLU mode (0 none, 1 mask from the recomputed activation, 2 mask from the
// stored output in `res`) are wave-uniform run-time fields: the pixel loop is instantiated per combination and chosen once at the top
// (tested per element they cost a scalar branch + an exec-mask save around every dz: ~25 instructions per element, the reduce pass ran at
// 3.9 TB/s beside the apply pass's 5.1).
template <typename Body>
__device__ __forceinline__ void bn_bwd_dispatch(bool f16, int relu, Body &&body) {
    using T_ = std::true_type;
    using F_ = std::false_type;
    if (f16) {
        if (relu == 0) body(T_{}, std::integral_constant<int, 0>{});
        else if (relu == 1) body(T_{}, std::integral_constant<int, 1>{});
        else body(T_{}, std::integral_constant<int, 2>{});
    } else {
        if (relu == 0) body(F_{}, std::integral_constant<int, 0>{});
        else if (relu == 1) body(F_{}, std::integral_constant<int, 1>{});
        else body(F_{}, std::integral_constant<int, 2>{});
    }
}

// Window kernels: the layer's consumers are one 2x2 max-pool plus NF same-size un-shifted tensors (the skip connection).
// One pooling window per thread: the four activations are read once, the pooled gradient goes to the first maximum
// (nn.MaxPool2d backward).  All loads are unconditional (clamped coordinates) and issued before any arithmetic.
template <int NF, bool APPLY>
__global__ __launch_bounds__(256) void bn_bwd_window_kernel(BnBwdArgs A, int kp) {
    const int VPP = A.C / 8;
    const int slot = (int)threadIdx.x % VPP, c0 = slot * 8;
    float sc[8], sh[8], mu[8], is[8], k1[8], k2[8], k3[8], s1[8], s2[8];
    bn_load_const(A, c0, APPLY, sc, sh, mu, is, k1, k2, k3);
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const unsigned H = A.H, W = A.W, Hp = (H + 1) / 2, Wp = (W + 1) / 2, nwin = (unsigned)A.N * Hp * Wp;
    const unsigned ppb = 256 / VPP;
    const GradIn gp = A.gin[kp];
    int kf[2] = {0, 0};
    {
        int m = 0;
        for (int k = 0; k < A.ngin && m < NF; ++k)
            if (k != kp) kf[m++] = k;
    }
    bn_bwd_dispatch(A.f16 != 0, A.relu != 0 ? 1 : 0, [&](auto f16_c, auto relu_c) {
    constexpr bool f16 = decltype(f16_c)::value, relu = decltype(relu_c)::value != 0;
    for (unsigned w0 = first_pixel(ppb, VPP); w0 < nwin; w0 += gridDim.x * ppb) {
        const unsigned w = (APPLY && A.rev) ? nwin - 1 - w0 : w0;
        const unsigned n = w / (Hp * Wp), r = w - n * Hp * Wp;
        const unsigned py = r / Wp, px = r - py * Wp;
        V16 raw[4], g[4][NF > 0 ? NF : 1], gv;
        unsigned pix[4];
        bool ok[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned yy = 2 * py + (q >> 1), xx = 2 * px + (q & 1);
            ok[q] = yy < H && xx < W;
            yy = yy < H ? yy : H - 1;
            xx = xx < W ? xx : W - 1;
            pix[q] = (n * H + yy) * W + xx;
            raw[q].u = *reinterpret_cast<const uint4 *>(A.raw + (size_t)pix[q] * A.C + c0);
#pragma unroll
            for (int m = 0; m < NF; ++m)
                g[q][m].u = *reinterpret_cast<const uint4 *>(A.gin[kf[m]].g + (size_t)pix[q] * A.gin[kf[m]].cstride + A.gin[kf[m]].coff + c0);
        }
        const bool pok = py < (unsigned)gp.Hg && px < (unsigned)gp.Wg;
        {
            const unsigned cy = pok ? py : 0, cx = pok ? px : 0;
            gv.u = *reinterpret_cast<const uint4 *>(gp.g + (((size_t)n * gp.Hg + cy) * gp.Wg + cx) * gp.cstride + gp.coff + c0);
        }
        V16 o[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float x[4], a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x[q] = ld16(raw[q].h[j], f16);
                float v = fmaf(x[q], sc[j], sh[j]);
                if (relu) v = fmaxf(v, 0.f);
                a[q] = bf2f(f2bf(v));
            }
            int bi = 0;
            float best = a[0];
#pragma unroll
            for (int q = 1; q < 4; ++q)
                if (ok[q] && a[q] > best) { best = a[q]; bi = q; }
            const float gpool = pok ? bf2f(gv.h[j]) : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float gs = (bi == q) ? gpool : 0.f;
#pragma unroll
                for (int m = 0; m < NF; ++m) gs += bf2f(g[q][m].h[j]);
                const float dz = (!ok[q] || (relu && !(a[q] > 0.f))) ? 0.f : gs;
                const float xh = (x[q] - mu[j]) * is[j];
                if (APPLY) o[q].h[j] = f2bf(k1[j] * (dz - k2[j] - xh * k3[j]));
                else { s1[j] += dz; s2[j] = fmaf(dz, xh, s2[j]); }
            }
        }
        if (APPLY) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (ok[q]) *reinterpret_cast<uint4 *>(A.draw + (size_t)pix[q] * A.C + c0) = o[q].u;
        }
    }
    });
    if (!APPLY) bn_write_partial<8>(A.partial, A.C, VPP, s1, s2);
}

// Flat kernels: every gradient source is a same-size un-shifted tensor, so dz needs only the pixel index.  Loads of BN_U
// pixels are issued back to back (clamped index, no branch), then each pixel is folded into the sums / written out.
template <int NG, bool RES, bool APPLY>
__global__ __launch_bounds__(256) void bn_bwd_flat_kernel(BnBwdArgs A) {
    const int VPP = A.C / 8;
    const int slot = (int)threadIdx.x % VPP, c0 = slot * 8;
    float sc[8], sh[8], mu[8], is[8], k1[8], k2[8], k3[8], s1[8], s2[8];
    bn_load_const(A, c0, APPLY, sc, sh, mu, is, k1, k2, k3);
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const unsigned npix = (unsigned)(A.N * A.H * A.W);
    const unsigned ppb = 256 / VPP, step = gridDim.x * ppb;
    const bool rev = APPLY && A.rev != 0;
    bn_bwd_dispatch(A.f16 != 0, A.relu, [&](auto f16_c, auto relu_c) {
        constexpr bool F16 = decltype(f16_c)::value;
        constexpr int RELU = decltype(relu_c)::value;
        for (unsigned p0 = first_pixel(ppb, VPP); p0 < npix; p0 += step * BN_U) {
            V16 raw[BN_U], res[BN_U], g[BN_U][NG];
#pragma unroll
            for (int u = 0; u < BN_U; ++u) {
                unsigned p = p0 + u * step;
                p = p < npix ? p : npix - 1;
                p = rev ? npix - 1 - p : p;
                raw[u].u = *reinterpret_cast<const uint4 *>(A.raw + (size_t)p * A.C + c0);
                if (RES) res[u].u = *reinterpret_cast<const uint4 *>(A.res + (size_t)p * A.C + c0);
#pragma unroll
                for (int k = 0; k < NG; ++k)
                    g[u][k].u = *reinterpret_cast<const uint4 *>(A.gin[k].g + (size_t)p * A.gin[k].cstride + A.gin[k].coff + c0);
            }
#pragma unroll
            for (int u = 0; u < BN_U; ++u) {
                const unsigned p = p0 + u * step;
                const bool valid = p < npix;
                V16 o, z;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = ld16(raw[u].h[j], F16);
                    float v = fmaf(x, sc[j], sh[j]);
                    if (RES) v = RELU == 2 ? bf2f(res[u].h[j]) : v + ld16(res[u].h[j], F16);     // RELU 2: res IS the stored output
                    float gs = bf2f(g[u][0].h[j]);
#pragma unroll
                    for (int k = 1; k < NG; ++k) gs += bf2f(g[u][k].h[j]);
                    // the forward rounds the activation to bf16 before the ReLU; rounding keeps the sign
                    // (a pixel past the end adds nothing to the sums; the apply pass does not write it)
                    const bool keep = (APPLY || valid) & (RELU == 0 || bf2f(f2bf(v)) > 0.f);
                    const float dz = keep ? gs : 0.f;
                    const float xh = (x - mu[j]) * is[j];
                    if (APPLY) {
                        o.h[j] = f2bf(k1[j] * (dz - k2[j] - xh * k3[j]));
                        z.h[j] = f2bf(dz);
                    } else {
                        s1[j] += dz;
                        s2[j] = fmaf(dz, xh, s2[j]);
                        if (RES) res[u].h[j] = f2bf(dz);                         // (the register is free: dz for the store below)
                    }
                }
                if (APPLY) {
                    if (valid) {
                        const unsigned pw = rev ? npix - 1 - p : p;
                        *reinterpret_cast<uint4 *>(A.draw + (size_t)pw * A.C + c0) = o.u;
                        if (RES) *reinterpret_cast<uint4 *>(A.dz_out + (size_t)pw * A.C + c0) = z.u;
                    }
                } else {
                    // a residual unit's bn2: dz is the 1x1 branch's gradient and is stored anyway - by this pass, so that the second pass reads
                    // one tensor instead of the NG gradient sources and the mask again (cdnet_bn_backward; it then sees dz rounded to bf16)
                    if (RES && A.dz_out && valid) *reinterpret_cast<uint4 *>(A.dz_out + (size_t)p * A.C + c0) = res[u].u;
                }
            }
        }
    });
    if (!APPLY) bn_write_partial<8>(A.partial, A.C, VPP, s1, s2);
}

// Head-coefficient source: the columns [K0, K0 + NK) of a pixel's row [dpt | du[9] | dm[3] | 0 0 0] as the aligned vectors that hold
// them (NK = 3: floats 10..12, NK = 9: floats 1..9); one 64-byte line per pixel, shared by the pixel's 16 threads
constexpr int HC_K0(int nk) { return nk == 3 ? 10 : 1; }
template <int NK> struct HcRow;
template <> struct HcRow<3> {
    f32x2 a; float b;
    __device__ __forceinline__ void load(const float *row) { a = *reinterpret_cast<const f32x2 *>(row + 10); b = row[12]; }
    template <int K> __device__ __forceinline__ float at() const { if constexpr (K < 2) return a[K]; else return b; }
};
template <> struct HcRow<9> {
    f32x4 a, b; f32x2 c;
    __device__ __forceinline__ void load(const float *row) {
        a = *reinterpret_cast<const f32x4 *>(row); b = *reinterpret_cast<const f32x4 *>(row + 4); c = *reinterpret_cast<const f32x2 *>(row + 8);
    }
    template <int K> __device__ __forceinline__ float at() const {
        if constexpr (K < 3) return a[K + 1]; else if constexpr (K < 7) return b[K - 3]; else return c[K - 7];
    }
};
template <> struct HcRow<0> {
    __device__ __forceinline__ void load(const float *) {}
};
// the source's value for channel weights w[0 .. NK): xf_axpy16's chain, fma(s, w, +0) first, then fma(s, w, sum)
template <int NK, int K = 0>
__device__ __forceinline__ float hc_value(const HcRow<NK> &row, const float (*w)[4], int j, float v = 0.f) {
    if constexpr (K < NK) return hc_value<NK, K + 1>(row, w, j, fmaf(row.template at<K>(), w[K][j], v));
    else return v;
}

// fp32 variants of the flat kernels: 4 channels per thread (one float4 per tensor and pixel), BN_U pixels in flight, plain
// fp32 arithmetic (no 16-bit rounding of the activation); relu == 2 reads the mask from the stored output in `res`.
// HS >= 0: source HS is a head-coefficient source of NK terms - no tensor is read for it; its value is the head kernels' xf_axpy16 chain
// (explicit fma from +0, in their order) over the pixel's coefficients and this thread's 4 channels of the NK weight rows, which stay in
// registers; it takes the tensor's place in the sum over the sources, so every result has the bits of the dense form.
template <int NG, bool RES, bool APPLY, int HS = -1, int NK = 0>
__global__ __launch_bounds__(256) void bn_bwd_flat32_kernel(BnBwdArgs A) {
    static_assert(HS < NG && (HS < 0) == (NK == 0) && (HS < 0 || (RES && !APPLY)), "head-coefficient source: sums pass of the residual form");
    const int VPP = A.C / 4;
    const int slot = (int)threadIdx.x % VPP, c0 = slot * 4;
    float sc[4], sh[4], mu[4], is[4], k1[4], k2[4], k3[4], s1[4], s2[4];
    // (row by row, not bn_load_const: behind that call the <1, false, *> instantiations - every plain fp32 layer - take 78 / 82 VGPRs
    // instead of 65 / 76 and lose a wave of occupancy each; the compiler orders the argument loads differently)
    bn_load_row<4>(A.scale, c0, sc, 1.f); bn_load_row<4>(A.shift, c0, sh, 0.f); bn_load_row<4>(A.mean, c0, mu, 0.f); bn_load_row<4>(A.invstd, c0, is, 1.f);
    if (APPLY) { bn_load_row<4>(A.k1, c0, k1, 1.f); bn_load_row<4>(A.k2, c0, k2, 0.f); bn_load_row<4>(A.k3, c0, k3, 0.f); }
#pragma unroll
    for (int j = 0; j < 4; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const unsigned npix = (unsigned)(A.N * A.H * A.W);
    const unsigned ppb = 256 / VPP, step = gridDim.x * ppb;
    const bool relu = A.relu != 0, outmask = A.relu == 2;
    const float *raw = reinterpret_cast<const float *>(A.raw), *resp = reinterpret_cast<const float *>(A.res);
    float *draw = reinterpret_cast<float *>(A.draw), *dzo = reinterpret_cast<float *>(A.dz_out);
    float hw[NK > 0 ? NK : 1][4];
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) hw[k][j] = A.hc_w[k * 64 + c0 + j];
    for (unsigned p0 = first_pixel(ppb, VPP); p0 < npix; p0 += step * BN_U) {
        f32x4 x[BN_U], r[BN_U], g[BN_U][NG];
        HcRow<NK> hc[BN_U];
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            unsigned p = p0 + u * step;
            p = p < npix ? p : npix - 1;
            if (APPLY && A.rev) p = npix - 1 - p;
            x[u] = *reinterpret_cast<const f32x4 *>(raw + (size_t)p * A.C + c0);
            if (RES) r[u] = *reinterpret_cast<const f32x4 *>(resp + (size_t)p * A.C + c0);
#pragma unroll
            for (int k = 0; k < NG; ++k)
                if (k != HS) g[u][k] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(A.gin[k].g) + (size_t)p * A.gin[k].cstride + A.gin[k].coff + c0);
            if (HS >= 0) hc[u].load(A.hc_coef + (size_t)p * 16);
        }
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const unsigned p = p0 + u * step;
            const bool valid = p < npix;
            f32x4 o, z;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = fmaf(x[u][j], sc[j], sh[j]);
                if (RES) v = outmask ? r[u][j] : v + r[u][j];
                const float hv = hc_value<NK>(hc[u], hw, j);
                float gs = HS == 0 ? hv : g[u][0][j];
#pragma unroll
                for (int k = 1; k < NG; ++k) gs += k == HS ? hv : g[u][k][j];
                const float dz = (!valid || (relu && !(v > 0.f))) ? 0.f : gs;
                const float xh = (x[u][j] - mu[j]) * is[j];
                if (APPLY) { o[j] = k1[j] * (dz - k2[j] - xh * k3[j]); z[j] = dz; }
                else { s1[j] += dz; s2[j] = fmaf(dz, xh, s2[j]); z[j] = dz; }
            }
            if (APPLY && valid) {
                const unsigned pw = A.rev ? npix - 1 - p : p;
                *reinterpret_cast<f32x4 *>(draw + (size_t)pw * A.C + c0) = o;
                if (RES) *reinterpret_cast<f32x4 *>(dzo + (size_t)pw * A.C + c0) = z;
            }
            // the sums pass of a residual unit's bn2 already leaves dz (the 1x1 branch's gradient): the second pass then reads one
            // tensor instead of the NG gradient sources and the mask again (cdnet_bn_backward)
            if (!APPLY && RES && dzo && valid) *reinterpret_cast<f32x4 *>(dzo + (size_t)p * A.C + c0) = z;
        }
    }
    if (!APPLY) bn_write_partial<4>(A.partial, A.C, VPP, s1, s2);
}

// fp32 variant of the window kernels (one 2x2 max-pool consumer + NF same-size un-shifted ones: the encoder's conv1_2 ... conv5_3):
// one pooling window x 4 channels per thread, the four raw vectors, their flat gradients and the pooled gradient requested back to back,
// plain fp32 arithmetic, the pooled gradient to the first maximum of relu(bn(raw)) (nn.MaxPool2d backward) - bit-identical to the
// generic per-pixel path (bn_bwd_generic_kernel<true, *>), which reads a window's raw vectors once per pixel.
template <int NF, bool APPLY>
__global__ __launch_bounds__(256) void bn_bwd_window32_kernel(BnBwdArgs A, int kp) {
    const int VPP = A.C / 4;
    const int slot = (int)threadIdx.x % VPP, c0 = slot * 4;
    float sc[4], sh[4], mu[4], is[4], k1[4], k2[4], k3[4], s1[4], s2[4];
    bn_load_const(A, c0, APPLY, sc, sh, mu, is, k1, k2, k3);
#pragma unroll
    for (int j = 0; j < 4; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const unsigned H = A.H, W = A.W, Hp = (H + 1) / 2, Wp = (W + 1) / 2, nwin = (unsigned)A.N * Hp * Wp;
    const unsigned ppb = 256 / VPP;
    const bool relu = A.relu != 0;
    const GradIn gp = A.gin[kp];
    const float *gpool_p = reinterpret_cast<const float *>(gp.g);
    const float *raw = reinterpret_cast<const float *>(A.raw);
    float *draw = reinterpret_cast<float *>(A.draw);
    const float *gf[NF > 0 ? NF : 1];
    int gcs[NF > 0 ? NF : 1], gco[NF > 0 ? NF : 1];
    {
        int m = 0;
        for (int k = 0; k < A.ngin && m < NF; ++k)
            if (k != kp) { gf[m] = reinterpret_cast<const float *>(A.gin[k].g); gcs[m] = A.gin[k].cstride; gco[m] = A.gin[k].coff; ++m; }
    }
    for (unsigned w0 = first_pixel(ppb, VPP); w0 < nwin; w0 += gridDim.x * ppb) {
        const unsigned w = (APPLY && A.rev) ? nwin - 1 - w0 : w0;
        const unsigned n = w / (Hp * Wp), r = w - n * Hp * Wp;
        const unsigned py = r / Wp, px = r - py * Wp;
        f32x4 x[4], g[4][NF > 0 ? NF : 1], gv;
        unsigned pix[4];
        bool ok[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned yy = 2 * py + (q >> 1), xx = 2 * px + (q & 1);
            ok[q] = yy < H && xx < W;
            yy = yy < H ? yy : H - 1;
            xx = xx < W ? xx : W - 1;
            pix[q] = (n * H + yy) * W + xx;
            x[q] = *reinterpret_cast<const f32x4 *>(raw + (size_t)pix[q] * A.C + c0);
#pragma unroll
            for (int m = 0; m < NF; ++m)
                g[q][m] = *reinterpret_cast<const f32x4 *>(gf[m] + (size_t)pix[q] * gcs[m] + gco[m] + c0);
        }
        const bool pok = py < (unsigned)gp.Hg && px < (unsigned)gp.Wg;
        {
            const unsigned cy = pok ? py : 0, cx = pok ? px : 0;
            gv = *reinterpret_cast<const f32x4 *>(gpool_p + (((size_t)n * gp.Hg + cy) * gp.Wg + cx) * gp.cstride + gp.coff + c0);
        }
        f32x4 o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float v = fmaf(x[q][j], sc[j], sh[j]);
                a[q] = relu ? fmaxf(v, 0.f) : v;
            }
            int bi = 0;
            float best = a[0];
#pragma unroll
            for (int q = 1; q < 4; ++q)
                if (ok[q] && a[q] > best) { best = a[q]; bi = q; }
            const float gpool = pok ? gv[j] : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // the generic path's order: 0 + the sources in argument order (kp = the pooled one's position)
                const float pt = (bi == q) ? gpool : 0.f;
                float gsum;
                if (NF == 0) gsum = 0.f + pt;
                else if (NF == 1) gsum = (0.f + (kp == 0 ? pt : g[q][0][j])) + (kp == 0 ? g[q][0][j] : pt);
                else gsum = ((0.f + (kp == 0 ? pt : g[q][0][j])) + (kp == 0 ? g[q][0][j] : (kp == 1 ? pt : g[q][NF - 1][j]))) +
                            (kp == 2 ? pt : g[q][NF - 1][j]);
                const float dz = (!ok[q] || (relu && !(a[q] > 0.f))) ? 0.f : gsum;
                const float xh = (x[q][j] - mu[j]) * is[j];
                if (APPLY) o[q][j] = k1[j] * (dz - k2[j] - xh * k3[j]);
                else { s1[j] += dz; s2[j] = fmaf(dz, xh, s2[j]); }
            }
        }
        if (APPLY) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (ok[q]) *reinterpret_cast<f32x4 *>(draw + (size_t)pix[q] * A.C + c0) = o[q];
        }
    }
    if (!APPLY) bn_write_partial<4>(A.partial, A.C, VPP, s1, s2);
}

// Generic kernels: per-pixel routing of every gradient source (dz8), 8 channels per thread in both precisions.
template <bool F32, bool APPLY>
__global__ __launch_bounds__(256) void bn_bwd_generic_kernel(BnBwdArgs A) {
    const int VPP = A.C / 8;
    const int slot = (int)threadIdx.x % VPP, c0 = slot * 8;
    float sc[8], sh[8], mu[8], is[8], k1[8], k2[8], k3[8], s1[8], s2[8];
    bn_load_const(A, c0, APPLY, sc, sh, mu, is, k1, k2, k3);
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    const unsigned HW = (unsigned)(A.H * A.W), npix = (unsigned)A.N * HW;
    const unsigned ppb = 256 / VPP;                                 // pixels per block per sub-iteration
    const unsigned step = gridDim.x * ppb;
    for (unsigned p0 = first_pixel(ppb, VPP); p0 < npix; p0 += step * BN_U) {
        float dz[BN_U][8], xh[BN_U][8];
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const unsigned p = p0 + u * step;
            if (p < npix) dz8_at<F32>(A, p, HW, c0, sc, sh, mu, is, dz[u], xh[u]);
            else if (!APPLY) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { dz[u][j] = 0.f; xh[u][j] = 0.f; }
            }
        }
#pragma unroll
        for (int u = 0; u < BN_U; ++u) {
            const unsigned p = p0 + u * step;
            if (!APPLY) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { s1[j] += dz[u][j]; s2[j] = fmaf(dz[u][j], xh[u][j], s2[j]); }
                continue;
            }
            if (p >= npix) continue;
            float o32[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o32[j] = k1[j] * (dz[u][j] - k2[j] - xh[u][j] * k3[j]);
            if (F32) {
                if (A.draw) stf8(A.draw, (size_t)p * A.C + c0, o32);
                if (A.dz_out) stf8(A.dz_out, (size_t)p * A.C + c0, dz[u]);
                continue;
            }
            V16 o, z;
#pragma unroll
            for (int j = 0; j < 8; ++j) { o.h[j] = f2bf(o32[j]); z.h[j] = f2bf(dz[u][j]); }
            if (A.draw) *reinterpret_cast<uint4 *>(A.draw + (size_t)p * A.C + c0) = o.u;
            if (A.dz_out) *reinterpret_cast<uint4 *>(A.dz_out + (size_t)p * A.C + c0) = z.u;
        }
    }
    if (!APPLY) bn_write_partial<8>(A.partial, A.C, VPP, s1, s2);
}

// sums [nb][2][C] -> dgamma, dbeta and the apply coefficients; one workgroup per channel, fixed LDS tree (deterministic)
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float *__restrict__ partial, int nb, int C, float M, const float *gamma,
                                                              const float *invstd, float *dgamma, float *dbeta, float *k1, float *k2,
                                                              float *k3) {
    const int c = blockIdx.x;
    double s1, s2;
    bn_sum_partials(partial, nb, C, c, s1, s2);
    if (threadIdx.x == 0) {
        if (dbeta) dbeta[c] = (float)s1;
        if (dgamma) dgamma[c] = (float)s2;
        k1[c] = gamma[c] * invstd[c];
        k2[c] = (float)(s1 / M);
        k3[c] = (float)(s2 / M);
    }
}

__global__ void bn_ktab_copy_kernel(const float *scale, const float *shift, const float *mean, const float *invstd, int C, float *ktab) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) { ktab[c] = scale[c]; ktab[C + c] = shift[c]; ktab[2 * C + c] = mean[c]; ktab[3 * C + c] = invstd[c]; }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------
// Host: launch plan and C ABI
// ------------------------------------------------------------------------------------------------------
static int fill_bn_args(const cdnet_bn_bwd_args *a, BnBwdArgs &A, const char *who, bool hc_ok = false) {
    CDNET_REQUIRE(a && a->raw, "%s: null pointer", who);
    CDNET_REQUIRE(a->C % 8 == 0 && a->C >= 8 && a->C <= 2048 , "%s: C=%d unsupported", who, a->C);
    CDNET_REQUIRE(a->ngin >= 1 && a->ngin <= 3, "%s: ngin=%d", who, a->ngin);
    A.raw = a->raw; A.res = a->res; A.f16 = a->f16; A.scale = a->scale; A.shift = a->shift; A.relu = a->relu;
    A.mean = a->mean; A.invstd = a->invstd;
    for (int k = 0; k < 3; ++k) {
        A.gin[k].g = a->gin[k].g; A.gin[k].Hg = a->gin[k].Hg; A.gin[k].Wg = a->gin[k].Wg;
        A.gin[k].oy = a->gin[k].oy; A.gin[k].ox = a->gin[k].ox; A.gin[k].pooled = a->gin[k].pooled;
        A.gin[k].coff = a->gin[k].coff; A.gin[k].cstride = a->gin[k].cstride ? a->gin[k].cstride : a->C;
        if (k < a->ngin) CDNET_REQUIRE(a->gin[k].g || (a->hc_nk && k == a->hc_slot), "%s: null gradient input %d", who, k);
        // (a floor-mode pool of a one-pixel-high or -wide tensor has no output: the window kernels' clamped load would read element 0 of it)
        if (k < a->ngin) CDNET_REQUIRE(a->gin[k].Hg >= 1 && a->gin[k].Wg >= 1, "%s: empty gradient input %d (%d x %d)", who, k, a->gin[k].Hg, a->gin[k].Wg);
    }
    A.ngin = a->ngin; A.N = a->N; A.H = a->H; A.W = a->W; A.C = a->C;
    A.partial = nullptr; A.k1 = A.k2 = A.k3 = nullptr; A.draw = nullptr; A.dz_out = nullptr;
    A.hc_coef = a->hc_coef; A.hc_w = a->hc_w; A.hc_slot = a->hc_slot; A.hc_nk = a->hc_nk;
    if (a->hc_nk) {
        // a head-coefficient source: cdnet_bn_backward alone takes one (and serves it on one plan, see there); the arguments are checked here
        CDNET_REQUIRE(hc_ok, "%s: no head-coefficient source here (cdnet_bn_backward, flat fp32 residual form only)", who);
        CDNET_REQUIRE((a->hc_nk == 3 || a->hc_nk == 9) && a->hc_k0 == HC_K0(a->hc_nk) && a->hc_coef && a->hc_w && a->C == 64 && a->hc_slot >= 0 &&
                      a->hc_slot < a->ngin && !a->gin[a->hc_slot].g,
                      "%s: head-coefficient source: hc_nk=%d hc_k0=%d hc_slot=%d C=%d (3 terms from column 10 or 9 from column 1, 64 channels, a slot "
                      "below ngin whose g is NULL)", who, a->hc_nk, a->hc_k0, a->hc_slot, a->C);
    }
    return CDNET_OK;
}

// Which kernels serve a layer and in how many workgroups; computed once, both passes launch from it.
enum BnPath { BN_WINDOW, BN_FLAT, BN_GENERIC };
struct BnPlan {
    BnPath path;
    bool f32;              // fp32 tensors (f16 == 2)
    int nb;                // workgroups of both passes = partial rows
    int kp, nflat;         // window: position of the pooled source, number of flat ones
    bool flat_sources;     // the flat pattern holds (whatever kernel serves it): what relu = 2 needs
};

static size_t bn_npix(const BnBwdArgs &A) { return (size_t)A.N * A.H * A.W; }

// the flat kernels' plan for the plain case of the split entries (bn_plain_case)
static BnPlan bn_plan_plain(const BnBwdArgs &A) {
    const bool f32 = A.f16 == 2;
    return BnPlan{BN_FLAT, f32, bn_grid(bn_npix(A), A.C, f32 ? 4 : 8, BN_U), 0, 0, true};
}

static BnPlan bn_plan(const BnBwdArgs &A, const void *draw, const void *dz_out) {
    bool simple = true;                               // every gradient source a same-size, un-shifted tensor?
    int npool = 0, kp = 0, nflat = 0;
    for (int k = 0; k < A.ngin; ++k) {
        const GradIn &g = A.gin[k];
        const bool same = !g.pooled && g.oy == 0 && g.ox == 0 && g.Hg == A.H && g.Wg == A.W;
        simple = simple && same;
        if (g.pooled) { ++npool; kp = k; }
        else if (same) ++nflat;
    }
    // window pattern: exactly one pooled consumer, every other one flat, a BatchNorm + ReLU layer without residual branch
    const bool window = npool == 1 && nflat == A.ngin - 1 && nflat <= 2 && A.mean && A.scale && !A.res && draw && !dz_out;
    const bool flat = !window && simple && A.mean && A.scale && draw && ((A.res != nullptr) == (dz_out != nullptr));
    // fp32 tensors: the 4-channel kernels hold C <= 1024; whatever they do not serve goes to the generic ones (pool / pad routing)
    const bool f32 = A.f16 == 2, fits32 = A.C <= 1024;
    BnPlan P{BN_GENERIC, f32, 0, kp, nflat, flat};
    if (window && (!f32 || (fits32 && A.shift && A.invstd))) P.path = BN_WINDOW;
    else if (flat && (!f32 || fits32)) P.path = BN_FLAT;
    const int V = f32 && P.path != BN_GENERIC ? 4 : 8;
    // (a window-pattern layer counts its workgroups in windows on the generic path too)
    P.nb = window ? bn_grid((size_t)A.N * ((A.H + 1) / 2) * ((A.W + 1) / 2), A.C, V, 1) : bn_grid(bn_npix(A), A.C, V, BN_U);
    return P;
}

// which instantiation the last launch of this thread took, per pass ([0] sums, [1] apply), and which pass came last
// (cdnet_bn_backward_last_plan / _last_sums_plan; host only, bit layout in cdnet_hip.h)
static thread_local int g_bn_last_plan[2] = {0, 0};
static thread_local int g_bn_last_pass = 0;

static int bn_plan_record(const BnPlan &P, const BnBwdArgs &A, bool apply, bool dz_source) {
    const int path = P.path == BN_WINDOW ? CDNET_BN_PATH_WINDOW : P.path == BN_FLAT ? CDNET_BN_PATH_FLAT : CDNET_BN_PATH_GENERIC;
    const int n = P.path == BN_WINDOW ? P.nflat : P.path == BN_FLAT ? A.ngin : 0;
    const int res = P.path == BN_FLAT && A.res ? 1 : 0;
    const int kp = P.path == BN_WINDOW ? P.kp : 0;
    return path | (P.f32 ? 1 : 0) << 2 | n << 3 | res << 5 | kp << 6 | (apply ? 1 : 0) << 8 | (dz_source ? 1 : 0) << 9 | P.nb << 10;
}

// one pass of the plan: the only place that turns run-time source counts into kernel instantiations
template <bool APPLY>
static void launch(const BnPlan &P, const BnBwdArgs &A, hipStream_t st, bool dz_source = false) {
    g_bn_last_plan[APPLY ? 1 : 0] = bn_plan_record(P, A, APPLY, dz_source);
    g_bn_last_pass = APPLY ? 1 : 0;
    auto window = [&](auto nf) {
        constexpr int NF = decltype(nf)::value;
        if (P.f32) bn_bwd_window32_kernel<NF, APPLY><<<P.nb, 256, 0, st>>>(A, P.kp);
        else bn_bwd_window_kernel<NF, APPLY><<<P.nb, 256, 0, st>>>(A, P.kp);
    };
    auto flat = [&](auto ng, auto res) {
        constexpr int NG = decltype(ng)::value;
        constexpr bool RES = decltype(res)::value;
        if constexpr (RES && !APPLY) {
            // head-coefficient source (cdnet_bn_backward has checked the plan): the instantiation of its slot and term count
            if (A.hc_nk) {
                auto hc = [&](auto hs) {
                    constexpr int HS = decltype(hs)::value;
                    if constexpr (HS < NG) {
                        if (A.hc_nk == 3) bn_bwd_flat32_kernel<NG, true, false, HS, 3><<<P.nb, 256, 0, st>>>(A);
                        else bn_bwd_flat32_kernel<NG, true, false, HS, 9><<<P.nb, 256, 0, st>>>(A);
                    }
                };
                if (A.hc_slot == 0) hc(std::integral_constant<int, 0>{});
                else if (A.hc_slot == 1) hc(std::integral_constant<int, 1>{});
                else hc(std::integral_constant<int, 2>{});
                return;
            }
        }
        if (P.f32) bn_bwd_flat32_kernel<NG, RES, APPLY><<<P.nb, 256, 0, st>>>(A);
        else bn_bwd_flat_kernel<NG, RES, APPLY><<<P.nb, 256, 0, st>>>(A);
    };
    using std::integral_constant;
    using std::true_type;
    using std::false_type;
    switch (P.path) {
        case BN_WINDOW:
            if (P.nflat == 0) window(integral_constant<int, 0>{});
            else if (P.nflat == 1) window(integral_constant<int, 1>{});
            else window(integral_constant<int, 2>{});
            break;
        case BN_FLAT:
            switch (A.ngin * 2 + (A.res ? 1 : 0)) {
                case 2: flat(integral_constant<int, 1>{}, false_type{}); break;
                case 3: flat(integral_constant<int, 1>{}, true_type{}); break;
                case 4: flat(integral_constant<int, 2>{}, false_type{}); break;
                case 5: flat(integral_constant<int, 2>{}, true_type{}); break;
                case 6: flat(integral_constant<int, 3>{}, false_type{}); break;
                default: flat(integral_constant<int, 3>{}, true_type{}); break;
            }
            break;
        case BN_GENERIC:
            if (P.f32) bn_bwd_generic_kernel<true, APPLY><<<P.nb, 256, 0, st>>>(A);
            else bn_bwd_generic_kernel<false, APPLY><<<P.nb, 256, 0, st>>>(A);
            break;
    }
}

// partial rows -> dgamma, dbeta and k1 | k2 | k3 at k[0 .. 3 C)
static void bn_finalize(const BnBwdArgs &A, const float *partial, int nb, const float *gamma, float *dgamma, float *dbeta, float *k,
                        hipStream_t st) {
    bn_bwd_finalize_kernel<<<A.C, 256, 0, st>>>(partial, nb, A.C, (float)bn_npix(A), gamma, A.invstd, dgamma, dbeta, k, k + A.C, k + 2 * A.C);
}

static void bn_set_coeffs(BnBwdArgs &A, const float *k) { A.k1 = k; A.k2 = k + A.C; A.k3 = k + 2 * A.C; }

// the apply pass's arguments when the sums pass stored dz: dz is the single plain source, no mask, no second dz store
static BnBwdArgs bn_dz_as_source(const BnBwdArgs &A, const unsigned short *dz) {
    BnBwdArgs B = A;
    B.ngin = 1;
    B.gin[0].g = dz; B.gin[0].Hg = A.H; B.gin[0].Wg = A.W; B.gin[0].oy = 0; B.gin[0].ox = 0; B.gin[0].pooled = 0;
    B.gin[0].coff = 0; B.gin[0].cstride = A.C;
    B.res = nullptr; B.relu = 0; B.dz_out = nullptr;
    return B;
}

extern "C" int cdnet_bn_backward(const cdnet_bn_bwd_args *a, const float *gamma, float *dgamma, float *dbeta, float *workspace,
                                 size_t workspace_floats, uint16_t *draw, uint16_t *dz_out, void *stream) {
    BnBwdArgs A;
    int rc = fill_bn_args(a, A, "cdnet_bn_backward", true);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = bn_npix(A);
    CDNET_REQUIRE(npix * (size_t)A.C < ((size_t)1 << 32) && npix < ((size_t)1 << 31), "cdnet_bn_backward: tensor too large for 32-bit pixel indexing");
    const BnPlan P = bn_plan(A, draw, dz_out);
    CDNET_REQUIRE(A.relu != 2 || (P.flat_sources && A.res), "cdnet_bn_backward: relu = 2 (mask from the stored output) needs same-size gradient sources and res");
    // A residual unit's bn2 stores dz anyway (the 1x1 branch's gradient).  The sums pass stores it, and the apply pass then reads that one
    // tensor instead of the gradient sources and the mask again (bit-identical, 9 instead of 12 tensor passes in fp32).
    static const bool dz_reuse = !(getenv("CDNET_BN_DZ_REUSE") && atoi(getenv("CDNET_BN_DZ_REUSE")) == 0);
    const bool reuse = dz_reuse && P.path == BN_FLAT && A.mean && A.res && dz_out;
    // a head-coefficient source: the sums pass of the flat fp32 residual form rebuilds it, the apply pass must read the stored dz
    CDNET_REQUIRE(!A.hc_nk || (reuse && P.f32), "cdnet_bn_backward: a head-coefficient source needs fp32 tensors, same-size sources, BatchNorm, res and dz_out "
                  "(the flat fp32 residual form, its second pass on the stored dz)");
    A.draw = draw;
    // The apply pass re-reads what the reduce pass just streamed (raw + gradients, up to 2 x 134 MB against 256 MB of
    // Infinity Cache): walking it back to front meets the most recently cached lines first instead of chasing the LRU tail.
    A.rev = 1;
    if (A.mean) {
        CDNET_REQUIRE(gamma && A.invstd && workspace, "cdnet_bn_backward: BatchNorm layer needs gamma/invstd/workspace");
        const size_t need = (size_t)P.nb * 2 * A.C + 3 * (size_t)A.C;
        if (workspace_floats < need) { set_error("cdnet_bn_backward: workspace %zu < %zu floats", workspace_floats, need); return CDNET_E_WORKSPACE; }
        A.partial = workspace;
        A.dz_out = dz_reuse ? dz_out : nullptr;       // (the sums pass stores dz only when the second pass is going to read it)
        float *k = workspace + (size_t)P.nb * 2 * A.C;
        launch<false>(P, A, st);
        bn_finalize(A, A.partial, P.nb, gamma, dgamma, dbeta, k, st);
        bn_set_coeffs(A, k);
    }
    A.dz_out = dz_out;
    launch<true>(P, reuse ? bn_dz_as_source(A, dz_out) : A, st, reuse);
    return check_launch("cdnet_bn_backward");
}

// The two passes of cdnet_bn_backward as separate calls, for the plain case (one same-size gradient source, BatchNorm + ReLU, no
// residual, 16-bit tensors): `stats` = reduce + finalize and the [7][C] table scale | shift | mean | invstd | k1 | k2 | k3 that both
// the apply pass and a fused consumer (cdnet_conv_src.relu = 3) read; `apply` = the second pass alone.  The trainer runs `stats`
// on the main chain, backward-data with the fused source right behind it, and `apply` + the weight gradient on the side stream.
// masked: the source may also be a gradient that already went through the ReLU (relu = 0: dz as a residual unit's sums pass stores it)
static bool bn_plain_case(const BnBwdArgs &A, bool masked = false) {
    const GradIn &g = A.gin[0];
    return A.ngin == 1 && !g.pooled && g.oy == 0 && g.ox == 0 && g.Hg == A.H && g.Wg == A.W && A.mean && A.scale && A.shift && A.invstd && !A.res &&
           (A.relu == 1 || (masked && A.relu == 0)) && (g.cstride == 0 || g.cstride == A.C) && g.coff == 0;
}

extern "C" int cdnet_bn_backward_stats(const cdnet_bn_bwd_args *a, const float *gamma, float *dgamma, float *dbeta, float *workspace,
                                       size_t workspace_floats, float *ktab, void *stream) {
    BnBwdArgs A;
    int rc = fill_bn_args(a, A, "cdnet_bn_backward_stats");
    if (rc) return rc;
    CDNET_REQUIRE(bn_plain_case(A) && A.f16 != 2 && gamma && workspace && ktab, "cdnet_bn_backward_stats: plain 16-bit case only (one same-size gradient, BatchNorm + ReLU, no residual)");
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = bn_npix(A);
    CDNET_REQUIRE(npix * (size_t)A.C < ((size_t)1 << 32) && npix < ((size_t)1 << 31), "cdnet_bn_backward_stats: tensor too large for 32-bit pixel indexing");
    const BnPlan P = bn_plan_plain(A);
    const size_t need = (size_t)P.nb * 2 * A.C;
    if (workspace_floats < need) { set_error("cdnet_bn_backward_stats: workspace %zu < %zu floats", workspace_floats, need); return CDNET_E_WORKSPACE; }
    A.partial = workspace;
    A.rev = 0;
    bn_ktab_copy_kernel<<<cdiv(A.C, 256), 256, 0, st>>>(A.scale, A.shift, A.mean, A.invstd, A.C, ktab);
    launch<false>(P, A, st);
    bn_finalize(A, A.partial, P.nb, gamma, dgamma, dbeta, ktab + 4 * A.C, st);
    return check_launch("cdnet_bn_backward_stats");
}

/* finalize pass alone over partial rows f32 [nb][2][C] that somebody else produced (the backward-data kernel with
 * cdnet_conv_args.ws = 2): dgamma, dbeta and rows 4..6 (k1 | k2 | k3) of ktab - all cdnet_bn_backward_apply reads; rows 0..3 are left
 * alone (their only reader, round 2's fused convolution source, is gone: nine copy launches per training step less) */
extern "C" int cdnet_bn_backward_finalize(const cdnet_bn_bwd_args *a, const float *gamma, float *dgamma, float *dbeta, const float *partial,
                                          int nb, float *ktab, void *stream) {
    BnBwdArgs A;
    int rc = fill_bn_args(a, A, "cdnet_bn_backward_finalize");
    if (rc) return rc;
    CDNET_REQUIRE(bn_plain_case(A) && gamma && partial && ktab && nb >= 1, "cdnet_bn_backward_finalize: plain case only");
    bn_finalize(A, partial, nb, gamma, dgamma, dbeta, ktab + 4 * A.C, (hipStream_t)stream);
    return check_launch("cdnet_bn_backward_finalize");
}

extern "C" int cdnet_bn_backward_apply(const cdnet_bn_bwd_args *a, const float *ktab, uint16_t *draw, void *stream) {
    BnBwdArgs A;
    int rc = fill_bn_args(a, A, "cdnet_bn_backward_apply");
    if (rc) return rc;
    CDNET_REQUIRE(bn_plain_case(A, true) && ktab && draw, "cdnet_bn_backward_apply: plain case only");
    // fp32 tensors (gradient, raw output, dRaw): the flat32 kernel
    CDNET_REQUIRE(A.f16 != 2 || A.C <= 1024, "cdnet_bn_backward_apply(f32): C=%d > 1024", A.C);
    A.rev = 1;
    A.draw = draw;
    bn_set_coeffs(A, ktab + 4 * A.C);
    launch<true>(bn_plan_plain(A), A, (hipStream_t)stream);
    return check_launch("cdnet_bn_backward_apply");
}

extern "C" int cdnet_bn_backward_last_plan(void) { return g_bn_last_plan[g_bn_last_pass]; }
extern "C" int cdnet_bn_backward_last_sums_plan(void) { return g_bn_last_plan[0]; }

extern "C" size_t cdnet_bn_backward_workspace_floats(int C) { return (size_t)BN_MAX_BLOCKS * 2 * C + 3 * (size_t)C; }
