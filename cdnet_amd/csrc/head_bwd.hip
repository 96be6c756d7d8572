// Backward of the 1x1 heads over the 64-channel features (HBM-bound streaming kernels): the DAM head (two kernels, or the one-pass
// form of the fp32 training step), the plain UNet's 64 -> K classifier and the bias gradient of its BatchNorm-less convolutions.
// Everything reduces through per-block partials that are summed in a fixed order, so a training step is bit-reproducible.
//
// Replaces, in the reference's train_util_dam.py: loss.backward() :307, the part that runs through model_dam.py's head
// (BatchNorm/ReLU/max-pool backward: bn_bwd.hip; the loss and its gradient: dam_loss.hip).
#include "train_util.h"
#include "head_feat.h"

using namespace cdnet;

namespace {

// ======================================================================================================
// DAM head backward
// ======================================================================================================
// fp32-stored feature (f16 == 2): 8 channels, plain fp32 arithmetic
__device__ __forceinline__ void feat8_f32(const HeadFeat &f, size_t pix, int c0, const float *s_sc, const float *s_sh, float *v) {
    float x[8], r[8];
    ldf8(f.raw, pix * 64 + c0, x);
    if (f.res) ldf8(f.res, pix * 64 + c0, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float t = x[j];
        if (f.scale) t = fmaf(t, s_sc[c0 + j], s_sh[c0 + j]);
        if (f.res) t += r[j];
        if (f.relu) t = fmaxf(t, 0.f);
        v[j] = t;
    }
}

// 8 channels [c0, c0+8) of the feature at one pixel
__device__ __forceinline__ void feat8(const HeadFeat &f, size_t pix, int c0, const float *s_sc, const float *s_sh, float *v) {
    if (f.f16 == 2) { feat8_f32(f, pix, c0, s_sc, s_sh, v); return; }
    V16 r, rr;
    r.u = *reinterpret_cast<const uint4 *>(f.raw + pix * 64 + c0);
    rr.u = make_uint4(0, 0, 0, 0);
    if (f.res) rr.u = *reinterpret_cast<const uint4 *>(f.res + pix * 64 + c0);
    if (f.f16 && f.scale && f.relu) {            // training-mode feature: packed math (xform.h)
        const u32x4 a = __builtin_bit_cast(u32x4, r.u), b = __builtin_bit_cast(u32x4, rr.u);
        if (f.res) xf_bnrelu_f16_to_f32<true>(a, b, s_sc + c0, s_sh + c0, v);
        else xf_bnrelu_f16_to_f32<false>(a, a, s_sc + c0, s_sh + c0, v);
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float x = f.f16 ? h2f(r.h[j]) : bf2f(r.h[j]);
        if (f.scale || f.res || f.relu) {
            if (f.scale) x = fmaf(x, s_sc[c0 + j], s_sh[c0 + j]);
            if (f.res) x += f.f16 ? h2f(rr.h[j]) : bf2f(rr.h[j]);
            if (f.relu) x = fmaxf(x, 0.f);
            x = bf2f(f2bf(x));
        }
        v[j] = x;
    }
}

// the same in two steps for 16-bit features: the raw vectors first (a kernel puts the loads of all its features in flight before it
// touches any of them - one memory round trip per pixel instead of one per feature), the lazily applied transform second.
// FM: 0 the feature is plain bf16 (a materialised tensor), 1 fp16 raw x scale + shift + residual -> ReLU (a lazily transformed
// training-mode residual-unit output), 2 anything (run-time flags)
struct FeatRaw8 {
    uint4 r, s;
};
template <int FM>
__device__ __forceinline__ void load_raw8(const HeadFeat &f, size_t pix, int c0, FeatRaw8 &R) {
    R.r = *reinterpret_cast<const uint4 *>(f.raw + pix * 64 + c0);
    R.s = make_uint4(0, 0, 0, 0);
    if (FM == 1 || (FM == 2 && f.res)) R.s = *reinterpret_cast<const uint4 *>(f.res + pix * 64 + c0);
}
template <int FM>
__device__ __forceinline__ void feat_from_raw8(const HeadFeat &f, const FeatRaw8 &R, int c0, const float *s_sc, const float *s_sh, float *v) {
    const u32x4 a = __builtin_bit_cast(u32x4, R.r), b = __builtin_bit_cast(u32x4, R.s);
    if (FM == 1) { xf_bnrelu_f16_to_f32<true>(a, b, s_sc + c0, s_sh + c0, v); return; }
    if (FM == 0) {
        V16 r0;
        r0.u = R.r;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = bf2f(r0.h[j]);
        return;
    }
    if (f.f16 && f.scale && f.relu) {
        if (f.res) xf_bnrelu_f16_to_f32<true>(a, b, s_sc + c0, s_sh + c0, v);
        else xf_bnrelu_f16_to_f32<false>(a, a, s_sc + c0, s_sh + c0, v);
        return;
    }
    V16 r, rr;
    r.u = R.r; rr.u = R.s;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float x = f.f16 ? h2f(r.h[j]) : bf2f(r.h[j]);
        if (f.scale || f.res || f.relu) {
            if (f.scale) x = fmaf(x, s_sc[c0 + j], s_sh[c0 + j]);
            if (f.res) x += f.f16 ? h2f(rr.h[j]) : bf2f(rr.h[j]);
            if (f.relu) x = fmaxf(x, 0.f);
            x = bf2f(f2bf(x));
        }
        v[j] = x;
    }
}

__device__ __forceinline__ void feat16(const HeadFeat &f, size_t pix, int q, const float *s_sc, const float *s_sh, float *v) {
    feat8(f, pix, q * 16, s_sc, s_sh, v);
    feat8(f, pix, q * 16 + 8, s_sc, s_sh, v + 8);
}
__device__ __forceinline__ void store16_bf16(unsigned short *dst, const float *v) {
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
        V16 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.h[j] = f2bf(v[h2 * 8 + j]);
        reinterpret_cast<uint4 *>(dst)[h2] = o.u;
    }
}

// 16 gradient values of one lane: element offset e of a bf16 (f32 = false) or fp32 tensor
__device__ __forceinline__ void store16_grad(unsigned short *base, size_t e, const float *v, bool f32) {
    if (f32) { stf8(base, e, v); stf8(base, e + 8, v + 8); }
    else store16_bf16(base + e, v);
}

// Kernel 1: four lanes per pixel (16 channels each).  Recomputes the head, writes the three feature gradients, the 13
// per-pixel coefficients {dpt, du[9], dm[3]} (f32 [px][16]) for the weight-gradient kernel, and per-block partial sums of
// the 23 scalar parameter gradients (biases and gate weights).
// FM: the storage of all three features (see FeatRaw8) - with a compile-time transform all three features' loads and the pixel's
// upstream gradients are in flight together; the run-time format tests of FM 2 make 6 000 instructions of branches whose joins
// drain the loads
template <int FM>
__global__ __launch_bounds__(256) void dam_head_bwd_kernel(HeadFeat f1, HeadFeat f2, HeadFeat f3, const HeadW *__restrict__ hw,
                                                           const float *__restrict__ dmask, const float *__restrict__ dpoint,
                                                           const float *__restrict__ ddir, int N, int plane,
                                                           unsigned short *__restrict__ df1, unsigned short *__restrict__ df2,
                                                           unsigned short *__restrict__ df3, float *__restrict__ coef,
                                                           float *__restrict__ partial) {
    __shared__ HeadW w;
    __shared__ float s_sc[3][64], s_sh[3][64];
    __shared__ float s_red[64][24];
    const int tid = threadIdx.x;
    {
        const float *src = reinterpret_cast<const float *>(hw);
        float *dst = reinterpret_cast<float *>(&w);
        for (int i = tid; i < HEADW_FLOATS; i += 256) dst[i] = src[i];
        if (tid < 64) {
            const HeadFeat *fs[3] = {&f1, &f2, &f3};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s_sc[k][tid] = fs[k]->scale ? fs[k]->scale[tid] : 1.f;
                s_sh[k][tid] = fs[k]->scale ? fs[k]->shift[tid] : 0.f;
            }
        }
    }
    __syncthreads();
    const size_t total = (size_t)N * plane;
    const int q = tid & 3;
    const bool f32 = f1.f16 == 2;                // fp32 features -> fp32 feature gradients
    // scalar gradients accumulated by the q == 0 lane of each pixel: dbm[3] | dbd[9] | dbp | da1 | da2[9]
    float sg[23];
#pragma unroll
    for (int j = 0; j < 23; ++j) sg[j] = 0.f;
    for (size_t base = (size_t)blockIdx.x * 64; base < total; base += (size_t)gridDim.x * 64) {
        const size_t i = base + (tid >> 2);
        const bool ok = i < total;
        const size_t ii = ok ? i : total - 1;
        const size_t n = ii / plane, p = ii - n * plane;
        // (the head weights stay in LDS: without this fence the compiler hoists a lane's 208 weight reads out of the loop)
        asm volatile("" ::: "memory");
        float v[16];
        FeatRaw8 R3[2], R2[2], R1[2];
        constexpr bool all16 = FM != 2;             // the generic instantiation keeps one feature at a time (registers)
        if (all16) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                load_raw8<FM>(f3, ii, q * 16 + h2 * 8, R3[h2]);
                load_raw8<FM>(f2, ii, q * 16 + h2 * 8, R2[h2]);
                load_raw8<FM>(f1, ii, q * 16 + h2 * 8, R1[h2]);
            }
        }
        // upstream gradients of this pixel: in flight with the features
        float go_m[3], go_d[9], go_p;
#pragma unroll
        for (int k = 0; k < 3; ++k) go_m[k] = ok ? dmask[(n * 3 + k) * plane + p] : 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) go_d[k] = ok ? ddir[(n * 9 + k) * plane + p] : 0.f;
        go_p = ok ? dpoint[n * plane + p] : 0.f;
        auto feat = [&](const HeadFeat &f, const FeatRaw8 (&R)[2], int k) {
            if (all16) {
                feat_from_raw8<FM>(f, R[0], q * 16, s_sc[k], s_sh[k], v);
                feat_from_raw8<FM>(f, R[1], q * 16 + 8, s_sc[k], s_sh[k], v + 8);
            } else {
                feat16(f, ii, q, s_sc[k], s_sh[k], v);
            }
        };
        feat(f3, R3, 2);
        const float pt = xf_quad_sum(xf_dot16(w.wp + q * 16, v)) + w.bp;
        const float sg1 = 1.f / (1.f + expf(-(w.a1 * pt)));
        const float g1 = 1.f + sg1;
        feat(f2, R2, 1);
        float u[9], d[9], q2 = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            u[k] = xf_quad_sum(xf_dot16(w.wd[k] + q * 16, v));
            d[k] = fmaf(g1, u[k], w.bd[k]);
            q2 = fmaf(w.a2[k], d[k], q2);
        }
        const float sg2 = 1.f / (1.f + expf(-q2));
        const float g2 = 1.f + sg2;
        feat(f1, R1, 0);
        float dm[3], dg2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float mk = xf_quad_sum(xf_dot16(w.wm[k] + q * 16, v));
            const float go = go_m[k];
            dg2 = fmaf(go, mk, dg2);
            dm[k] = go * g2;
            sg[k] += go;
        }
        // dF1 = sum_k dm_k * wm_k   (this lane's 16 channels)
        xf_axpy16(dm[0], w.wm[0] + q * 16, v, false);
        xf_axpy16(dm[1], w.wm[1] + q * 16, v, true);
        xf_axpy16(dm[2], w.wm[2] + q * 16, v, true);
        if (ok) store16_grad(df1, ii * 64 + q * 16, v, f32);
        const float dq2 = dg2 * sg2 * (1.f - sg2);
        float du[9], dg1 = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float dd = go_d[k] + dq2 * w.a2[k];
            sg[3 + k] += dd;
            sg[14 + k] = fmaf(dq2, d[k], sg[14 + k]);
            dg1 = fmaf(dd, u[k], dg1);
            du[k] = dd * g1;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) xf_axpy16(du[k], w.wd[k] + q * 16, v, k != 0);
        if (ok) store16_grad(df2, ii * 64 + q * 16, v, f32);
        const float dsg1 = dg1 * sg1 * (1.f - sg1);
        const float dpt = go_p + dsg1 * w.a1;
        sg[12] += dpt;
        sg[13] = fmaf(dsg1, pt, sg[13]);
        xf_axpy16(dpt, w.wp + q * 16, v, false);
        if (ok) {
            store16_grad(df3, ii * 64 + q * 16, v, f32);
            // coefficient row [dpt | du[9] | dm[3] | 0 0 0]: lane q writes floats 4q..4q+3
            float4 cf;
            if (q == 0) cf = make_float4(dpt, du[0], du[1], du[2]);
            else if (q == 1) cf = make_float4(du[3], du[4], du[5], du[6]);
            else if (q == 2) cf = make_float4(du[7], du[8], dm[0], dm[1]);
            else cf = make_float4(dm[2], 0.f, 0.f, 0.f);
            reinterpret_cast<float4 *>(coef + ii * 16)[q] = cf;
        }
    }
    // every lane of a pixel accumulated identical scalar sums: take the q == 0 lanes, fixed-order block reduction
    if (q == 0) {
#pragma unroll
        for (int j = 0; j < 23; ++j) s_red[tid >> 2][j] = sg[j];
    }
    __syncthreads();
    if (tid < 23) {
        float s = 0.f;
        for (int k = 0; k < 64; ++k) s += s_red[k][tid];
        int dst;                                     // HeadW tail: bp, bd[9], bm[3], a1, a2[9]
        if (tid < 3) dst = 832 + 10 + tid;
        else if (tid < 12) dst = 832 + 1 + (tid - 3);
        else if (tid == 12) dst = 832;
        else if (tid == 13) dst = 832 + 13;
        else dst = 832 + 14 + (tid - 14);
        partial[(size_t)blockIdx.x * HEADW_FLOATS + dst] = s;
    }
}

// Kernel 2: weight gradients  dW[row][c] = sum_px coef[px][row] * F_row(px, c),  rows = {dpt x F3, du[9] x F2, dm[3] x F1}.
// thread = (8 channels, pixel group); 104 accumulators; per-block partials in the HeadW layout.
template <int FM>
__global__ __launch_bounds__(256) void dam_head_wgrad_kernel(HeadFeat f1, HeadFeat f2, HeadFeat f3, const float *__restrict__ coef,
                                                             int N, int plane, float *__restrict__ partial) {
    __shared__ float s_sc[3][64], s_sh[3][64];
    __shared__ float s_w[4][13][64];
    const int tid = threadIdx.x;
    if (tid < 64) {
        const HeadFeat *fs[3] = {&f1, &f2, &f3};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s_sc[k][tid] = fs[k]->scale ? fs[k]->scale[tid] : 1.f;
            s_sh[k][tid] = fs[k]->scale ? fs[k]->shift[tid] : 0.f;
        }
    }
    __syncthreads();
    float gw[13][8];
#pragma unroll
    for (int j = 0; j < 13; ++j)
#pragma unroll
        for (int q = 0; q < 8; ++q) gw[j][q] = 0.f;
    const int c8 = (tid & 7) * 8, pg = tid >> 3;
    const size_t total = (size_t)N * plane;
    for (size_t ip = (size_t)blockIdx.x * 32 + pg; ip < total; ip += (size_t)gridDim.x * 32) {
        const float4 *cr = reinterpret_cast<const float4 *>(coef + ip * 16);
        const float4 c0 = cr[0], c1 = cr[1], c2 = cr[2], c3 = cr[3];
        const float cf[13] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x};
        float x[8];
        FeatRaw8 R3, R2, R1;
        constexpr bool all16 = FM != 2;
        if (all16) { load_raw8<FM>(f3, ip, c8, R3); load_raw8<FM>(f2, ip, c8, R2); load_raw8<FM>(f1, ip, c8, R1); }
        if (all16) feat_from_raw8<FM>(f3, R3, c8, s_sc[2], s_sh[2], x);
        else feat8(f3, ip, c8, s_sc[2], s_sh[2], x);
#pragma unroll
        for (int q = 0; q < 8; ++q) gw[0][q] = fmaf(cf[0], x[q], gw[0][q]);
        if (all16) feat_from_raw8<FM>(f2, R2, c8, s_sc[1], s_sh[1], x);
        else feat8(f2, ip, c8, s_sc[1], s_sh[1], x);
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
            for (int q = 0; q < 8; ++q) gw[1 + j][q] = fmaf(cf[1 + j], x[q], gw[1 + j][q]);
        if (all16) feat_from_raw8<FM>(f1, R1, c8, s_sc[0], s_sh[0], x);
        else feat8(f1, ip, c8, s_sc[0], s_sh[0], x);
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int q = 0; q < 8; ++q) gw[10 + j][q] = fmaf(cf[10 + j], x[q], gw[10 + j][q]);
    }
#pragma unroll
    for (int j = 0; j < 13; ++j)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float t = gw[j][q];
            t += __shfl_xor(t, 8); t += __shfl_xor(t, 16); t += __shfl_xor(t, 32);
            gw[j][q] = t;
        }
    if ((tid & 63) < 8) {
#pragma unroll
        for (int j = 0; j < 13; ++j)
#pragma unroll
            for (int q = 0; q < 8; ++q) s_w[tid >> 6][j][c8 + q] = gw[j][q];
    }
    __syncthreads();
    float *o = partial + (size_t)blockIdx.x * HEADW_FLOATS;
    for (int idx = tid; idx < 13 * 64; idx += 256) {
        const int row = idx / 64, cc = idx % 64;
        o[idx] = (s_w[0][row][cc] + s_w[1][row][cc]) + (s_w[2][row][cc] + s_w[3][row][cc]);
    }
}

// Kernels 1 and 2 in one pass over the features, for the fp32 training step: three plain stored fp32 features; f3 is the output of a
// residual unit with the fused epilogue that the head alone reads, so its gradient leaves as dz3 = (f3 > 0) ? dF3 : 0 (the sums pass of
// that unit's bn2 then reads one gradient tensor without the mask).  Every sum is taken in the order of the two-kernel path, so the
// results are bit-identical to it:
//   workgroup b (512 threads) owns the 32 pixel chains of dam_head_wgrad_kernel's workgroup b (pixels 32 b + j + 32768 it) and walks
//   four of its iterations per 128-pixel group.  Per pixel (four lanes) the arithmetic of dam_head_bwd_kernel in the same order; the 13
//   coefficients and the features go through LDS into dam_head_wgrad_kernel's mapping (thread = 8 channels x pixel chain; the 13 rows
//   split over the two halves of the workgroup: 56 accumulators per thread, the same fma chain per accumulator, the same reduction at
//   the end) - the coefficient tensor is never written, the features are read once.
//   The 23 scalar sums: dam_head_bwd_kernel's chain (workgroup b', slot s') is the pixels 64 b' + s' + 65536 it', i.e. here the quads of
//   iteration parity h & 1, alternately h < 2 and h >= 2: the quad with h < 2 keeps the chain and takes the other one's terms through LDS.
//   The per-chain sums go to sgbuf[1024][64][24]; head_scalar_reduce_kernel adds the 64 slots of a workgroup in that kernel's order.
// All of a pixel group's loads (three features, 13 gradient planes) are issued before the first use, indices clamped.
constexpr int HEAD_FUSED_BLOCKS = 1024;           // = the grid of the two-kernel path (the partition of the sums depends on it)
constexpr int HF_ROW = 68;                        // LDS floats per staged pixel (64 + 4: 16-byte aligned rows off the 64-float bank period)

// rows R0 .. R0 + 6 of the 13 x 64 block (row 13: a zero coefficient) for one pixel: row 0 x F3, rows 1..9 x F2, rows 10..12 x F1
template <int R0>
__device__ __forceinline__ void head_wgrad_rows(float (&gw)[7][8], const float *cfrow, const float *f3p, const float *f2p, const float *f1p) {
    const float4 *cr = reinterpret_cast<const float4 *>(cfrow);
    const float4 c0 = cr[0], c1 = cr[1], c2 = cr[2], c3 = cr[3];
    const float cf[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
    float x3[8], x2[8], x1[8];
    if (R0 == 0) ldf8(f3p, 0, x3);
    ldf8(f2p, 0, x2);
    if (R0 != 0) ldf8(f1p, 0, x1);
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        const int row = R0 + r;
        if (row >= 13) continue;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float x = row == 0 ? x3[k] : row < 10 ? x2[k] : x1[k];
            gw[r][k] = fmaf(cf[row], x, gw[r][k]);
        }
    }
}

// COEF: dF1 and dF2 are not stored (nor computed); the pixel's coefficient row [dpt | du[9] | dm[3] | 0 0 0] goes to coef f32 [px][16]
// (dam_head_bwd_kernel's layout) instead, 16 bytes per lane, and their one reader each - the sums pass of mask_feature.bn2 /
// direction_feature.bn2, bn_bwd_flat32_kernel's head-coefficient form - rebuilds its element with the xf_axpy16 chains below: the step
// stores 67 MB in place of 536 MB.  Everything else is the same code in the same order.
template <bool COEF>
__global__ __launch_bounds__(512)
void dam_head_bwd_fused_kernel(const float *__restrict__ f1, const float *__restrict__ f2, const float *__restrict__ f3,
                               const HeadW *__restrict__ hw, const float *__restrict__ dmask, const float *__restrict__ dpoint,
                               const float *__restrict__ ddir, int N, int plane, float *__restrict__ df1, float *__restrict__ df2,
                               float *__restrict__ coef, float *__restrict__ dz3, float *__restrict__ partial, float *__restrict__ sgbuf) {
    __shared__ HeadW w;
    __shared__ __attribute__((aligned(16))) float s_cf[128 * 16];
    __shared__ __attribute__((aligned(16))) float s_f[3][128 * HF_ROW];     // (>= 4 x 13 x 64: the waves' weight-gradient blocks at the end)
    __shared__ float s_sg[64 * 4][12];
    const int tid = threadIdx.x;
    {
        const float *src = reinterpret_cast<const float *>(hw);
        float *dst = reinterpret_cast<float *>(&w);
        for (int i = tid; i < HEADW_FLOATS; i += 512) dst[i] = src[i];
    }
    __syncthreads();
    const unsigned total = (unsigned)N * (unsigned)plane;          // (32-bit element indices: the entry checks total * 64 < 2^32)
    const int q = tid & 3, slot = tid >> 2;          // per-pixel phase: lane of the pixel's quad, pixel slot of the group (0..127)
    const int sh = slot >> 5, sj = slot & 31;        // ... = iteration of dam_head_wgrad_kernel within the group, and its chain
    const int c8 = (tid & 7) * 8, pg = (tid & 255) >> 3, rs = tid >> 8;     // weight-gradient phase: that kernel's mapping, half of the rows
    // the 23 scalar gradients dbm[3] | dbd[9] | dbp | da1 | da2[9] are the same on the four lanes of a pixel: lane q keeps those with
    // index 4 s + q (6 registers instead of 23); sum = fma(x, y, sum) with y = 1 for the plain sums (exact)
    float sgq[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) sgq[j] = 0.f;
    float gw[7][8];
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) gw[j][k] = 0.f;
    for (unsigned base = blockIdx.x * 32; base < total; base += 4 * 32768) {
        const unsigned i = base + sj + sh * 32768;
        const bool ok = i < total;
        const unsigned ii = ok ? i : total - 1;
        const unsigned n = ii / (unsigned)plane, p = ii - n * (unsigned)plane;
        // (the head weights stay in LDS: without this fence the compiler hoists a lane's 208 weight reads out of the loop)
        asm volatile("" ::: "memory");
        float F3[16], F2[16], F1[16], v[16];
        const unsigned e = ii * 64 + q * 16;
        ldf8(f3, e, F3); ldf8(f3, e + 8, F3 + 8);
        ldf8(f2, e, F2); ldf8(f2, e + 8, F2 + 8);
        ldf8(f1, e, F1); ldf8(f1, e + 8, F1 + 8);
        float go_m[3], go_d[9], go_p;
#pragma unroll
        for (int k = 0; k < 3; ++k) go_m[k] = dmask[(n * 3 + k) * plane + p];
#pragma unroll
        for (int k = 0; k < 9; ++k) go_d[k] = ddir[(n * 9 + k) * plane + p];
        go_p = dpoint[n * plane + p];
#pragma unroll
        for (int k = 0; k < 3; ++k) go_m[k] = ok ? go_m[k] : 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) go_d[k] = ok ? go_d[k] : 0.f;
        go_p = ok ? go_p : 0.f;
        // each feature goes to LDS for the weight-gradient phase as soon as its dot products are done (registers)
        auto stage = [&](const float *F, int k) {
            float *dst = s_f[k] + slot * HF_ROW + q * 16;
#pragma unroll
            for (int h = 0; h < 4; ++h) *reinterpret_cast<float4 *>(dst + 4 * h) = make_float4(F[4 * h], F[4 * h + 1], F[4 * h + 2], F[4 * h + 3]);
        };
        __syncthreads();                             // (the previous group's weight-gradient phase has read the slices)
        const float pt = xf_quad_sum(xf_dot16(w.wp + q * 16, F3)) + w.bp;
        unsigned pos3 = 0;                           // the unit's ReLU mask, read from the stored output
#pragma unroll
        for (int j = 0; j < 16; ++j) pos3 |= F3[j] > 0.f ? 1u << j : 0u;
        stage(F3, 0);
        __builtin_amdgcn_sched_barrier(0);           // (phases kept apart: interleaved, their LDS weight reads overflow the registers)
        const float sg1 = 1.f / (1.f + expf(-(w.a1 * pt)));
        const float g1 = 1.f + sg1;
        float u[9], d[9], q2 = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            u[k] = xf_quad_sum(xf_dot16(w.wd[k] + q * 16, F2));
            d[k] = fmaf(g1, u[k], w.bd[k]);
            q2 = fmaf(w.a2[k], d[k], q2);
        }
        stage(F2, 1);
        __builtin_amdgcn_sched_barrier(0);
        const float sg2 = 1.f / (1.f + expf(-q2));
        const float g2 = 1.f + sg2;
        float dm[3], dg2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float mk = xf_quad_sum(xf_dot16(w.wm[k] + q * 16, F1));
            const float go = go_m[k];
            dg2 = fmaf(go, mk, dg2);
            dm[k] = go * g2;
        }
        stage(F1, 2);
        __builtin_amdgcn_sched_barrier(0);
        if (!COEF) {
            xf_axpy16(dm[0], w.wm[0] + q * 16, v, false);
            xf_axpy16(dm[1], w.wm[1] + q * 16, v, true);
            xf_axpy16(dm[2], w.wm[2] + q * 16, v, true);
            if (ok) { stf8(df1, e, v); stf8(df1, e + 8, v + 8); }
        }
        __builtin_amdgcn_sched_barrier(0);
        const float dq2 = dg2 * sg2 * (1.f - sg2);
        float du[9], dd[9], dg1 = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            dd[k] = go_d[k] + dq2 * w.a2[k];
            dg1 = fmaf(dd[k], u[k], dg1);
            du[k] = dd[k] * g1;
        }
        if (!COEF) {
#pragma unroll
            for (int k = 0; k < 9; ++k) xf_axpy16(du[k], w.wd[k] + q * 16, v, k != 0);
            if (ok) { stf8(df2, e, v); stf8(df2, e + 8, v + 8); }
        }
        __builtin_amdgcn_sched_barrier(0);
        const float dsg1 = dg1 * sg1 * (1.f - sg1);
        const float dpt = go_p + dsg1 * w.a1;
        // this pixel's terms of the scalar sums (x, y) -> sum = fma(x, y, sum): the 4 s + q-th of [go_m[3] | dd[9] | dpt | dsg1 pt | dq2 d[9]]
        float sx[6], sy[6];
        {
            float tx[24], ty[24];
#pragma unroll
            for (int j = 0; j < 3; ++j) { tx[j] = go_m[j]; ty[j] = 1.f; }
#pragma unroll
            for (int j = 0; j < 9; ++j) { tx[3 + j] = dd[j]; ty[3 + j] = 1.f; tx[14 + j] = dq2; ty[14 + j] = d[j]; }
            tx[12] = dpt; ty[12] = 1.f; tx[13] = dsg1; ty[13] = pt; tx[23] = 0.f; ty[23] = 0.f;
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                sx[s] = q == 0 ? tx[4 * s] : q == 1 ? tx[4 * s + 1] : q == 2 ? tx[4 * s + 2] : tx[4 * s + 3];
                sy[s] = q == 0 ? ty[4 * s] : q == 1 ? ty[4 * s + 1] : q == 2 ? ty[4 * s + 2] : ty[4 * s + 3];
            }
        }
        if (sh < 2) {
#pragma unroll
            for (int s = 0; s < 6; ++s) sgq[s] = fmaf(sx[s], sy[s], sgq[s]);
        } else {
#pragma unroll
            for (int s = 0; s < 6; ++s) { s_sg[tid - 256][s] = sx[s]; s_sg[tid - 256][6 + s] = sy[s]; }
        }
        xf_axpy16(dpt, w.wp + q * 16, v, false);
        // v = dF3: through the unit's ReLU (mask from the stored output)
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = (pos3 >> j & 1) ? v[j] : 0.f;
        if (ok) { stf8(dz3, e, v); stf8(dz3, e + 8, v + 8); }
        __builtin_amdgcn_sched_barrier(0);
        // coefficient row [dpt | du[9] | dm[3] | 0 0 0] of the pixel: lane q writes floats 4q..4q+3
        {
            float4 cf;
            if (q == 0) cf = make_float4(dpt, du[0], du[1], du[2]);
            else if (q == 1) cf = make_float4(du[3], du[4], du[5], du[6]);
            else if (q == 2) cf = make_float4(du[7], du[8], dm[0], dm[1]);
            else cf = make_float4(dm[2], 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(s_cf + slot * 16 + q * 4) = cf;
            if (COEF && ok) *reinterpret_cast<float4 *>(coef + ii * 16 + q * 4) = cf;
        }
        __syncthreads();
        // the chain's next pixel (iteration h + 2 of this group) was computed by the quad 256 threads up
        if (sh < 2) {
#pragma unroll
            for (int s = 0; s < 6; ++s) sgq[s] = fmaf(s_sg[tid][s], s_sg[tid][6 + s], sgq[s]);
        }
        // weight gradients: dam_head_wgrad_kernel's four iterations of this group, one pixel of chain pg each, in its order
#pragma unroll 1
        for (int h = 0; h < 4; ++h) {
            if (base + pg + h * 32768 < total) {
                const int s = h * 32 + pg;
                if (rs == 0) head_wgrad_rows<0>(gw, s_cf + s * 16, s_f[0] + s * HF_ROW + c8, s_f[1] + s * HF_ROW + c8, s_f[2] + s * HF_ROW + c8);
                else head_wgrad_rows<7>(gw, s_cf + s * 16, s_f[0] + s * HF_ROW + c8, s_f[1] + s * HF_ROW + c8, s_f[2] + s * HF_ROW + c8);
            }
        }
    }
    // the chain of scalar sums this quad kept: dam_head_bwd_kernel's workgroup (b >> 1) + 512 (h & 1), slot 32 (b & 1) + j
    if (sh < 2) {
        float *o = sgbuf + ((size_t)((blockIdx.x >> 1) + 512 * sh) * 64 + 32 * (blockIdx.x & 1) + sj) * 24;
#pragma unroll
        for (int s = 0; s < 6; ++s) o[4 * s + q] = sgq[s];
    }
    // dam_head_wgrad_kernel's reduction: the 8 chains of a wave, then the four waves
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float t = gw[j][k];
            t += __shfl_xor(t, 8); t += __shfl_xor(t, 16); t += __shfl_xor(t, 32);
            gw[j][k] = t;
        }
    __syncthreads();
    float *s_w = s_f[0];                             // [4][13][64]
    if ((tid & 63) < 8) {
#pragma unroll
        for (int j = 0; j < 7; ++j)
            if (rs * 7 + j < 13) {
#pragma unroll
                for (int k = 0; k < 8; ++k) s_w[((((tid & 255) >> 6) * 13) + rs * 7 + j) * 64 + c8 + k] = gw[j][k];
            }
    }
    __syncthreads();
    float *o = partial + (size_t)blockIdx.x * HEADW_FLOATS;
    for (int idx = tid; idx < 13 * 64; idx += 512) o[idx] = (s_w[idx] + s_w[832 + idx]) + (s_w[2 * 832 + idx] + s_w[3 * 832 + idx]);
}

// dam_head_bwd_kernel's block reduction of the 23 scalar sums over the chains dam_head_bwd_fused_kernel left: workgroup = one workgroup
// of that kernel, the 64 slots added in its order
__global__ __launch_bounds__(64) void head_scalar_reduce_kernel(const float *__restrict__ sgbuf, float *__restrict__ partial) {
    const int tid = threadIdx.x;
    if (tid < 23) {
        const float *sg = sgbuf + (size_t)blockIdx.x * 64 * 24;
        float s = 0.f;
        for (int k = 0; k < 64; ++k) s += sg[k * 24 + tid];
        int dst;                                     // HeadW tail: bp, bd[9], bm[3], a1, a2[9]
        if (tid < 3) dst = 832 + 10 + tid;
        else if (tid < 12) dst = 832 + 1 + (tid - 3);
        else if (tid == 12) dst = 832;
        else if (tid == 13) dst = 832 + 13;
        else dst = 832 + 14 + (tid - 14);
        partial[(size_t)blockIdx.x * HEADW_FLOATS + dst] = s;
    }
}

// ======================================================================================================
// Backward of the plain UNet's 64 -> K classifier (models/unet.py:75,104).  Four lanes per pixel (16 channels each):
//   dF[c] = sum_k dlogit_k * w[k][c];  dW[k][c] = sum_px dlogit_k * F[c];  db[k] = sum_px dlogit_k.
// Per-block partial sums [K*64 | K], reduced in a fixed order by reduce_partials_kernel (deterministic).
// ======================================================================================================
constexpr int FC_KMAX = 4;            // plain UNet classifier (3 classes): 4 lanes per pixel x 16 channels
constexpr int FC_KWIDE = 12;          // the ablation heads' 9-class direction classifier: 8 lanes per pixel x 8 channels
constexpr int FC_KMOST = 20;          // model_unet_MandD16's 17-class direction classifier: same 8 x 8 split, 20 accumulator rows

// KM: classes the instantiation holds accumulators for; LPP lanes share a pixel (64 / LPP channels each)
template <int KM, int LPP>
__global__ __launch_bounds__(256) void final_conv_bwd_kernel(HeadFeat f, const float *__restrict__ w, const float *__restrict__ dl,
                                                             int K, int N, int plane, unsigned short *__restrict__ df,
                                                             float *__restrict__ partial) {
    constexpr int CH = 64 / LPP, PPB = 256 / LPP, ROW = KM * 64 + KM;
    static_assert(CH == 16 || CH == 8, "16 or 8 channels per lane");
    __shared__ float s_w[KM * 64], s_sc[64], s_sh[64];
    __shared__ float s_red[4][ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < K * 64; i += 256) s_w[i] = w[i];
    if (tid < 64) { s_sc[tid] = f.scale ? f.scale[tid] : 1.f; s_sh[tid] = f.scale ? f.shift[tid] : 0.f; }
    __syncthreads();
    const int q = tid % LPP;
    float gw[KM][CH], gb[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        gb[k] = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) gw[k][c] = 0.f;
    }
    const size_t total = (size_t)N * plane;
    for (size_t base = (size_t)blockIdx.x * PPB; base < total; base += (size_t)gridDim.x * PPB) {
        const size_t i = base + (tid / LPP);
        const bool ok = i < total;
        const size_t ii = ok ? i : total - 1;
        const size_t n = ii / plane, p = ii - n * plane;
        float v[CH], d[KM];
        if (CH == 16) feat16(f, ii, q, s_sc, s_sh, v);
        else feat8(f, ii, q * 8, s_sc, s_sh, v);
#pragma unroll
        for (int k = 0; k < KM; ++k) d[k] = (ok && k < K) ? dl[(n * K + k) * plane + p] : 0.f;
        float o[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < KM; ++k) {
                t = fmaf(d[k], s_w[(k < K ? k : 0) * 64 + q * CH + c], t);
                gw[k][c] = fmaf(d[k], v[c], gw[k][c]);
            }
            o[c] = t;
        }
#pragma unroll
        for (int k = 0; k < KM; ++k) gb[k] += d[k];
        if (ok) {
            if (CH == 16) store16_grad(df, ii * 64 + q * 16, o, f.f16 == 2);
            else if (f.f16 == 2) stf8(df, ii * 64 + q * 8, o);
            else {
                V16 ov;
#pragma unroll
                for (int j = 0; j < 8; ++j) ov.h[j] = f2bf(o[j]);
                *reinterpret_cast<uint4 *>(df + ii * 64 + q * 8) = ov.u;
            }
        }
    }
    // lanes with the same q own the same channels: butterfly over the pixel slots of the wave, then one row per wave
#pragma unroll
    for (int k = 0; k < KM; ++k) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            float t = gw[k][c];
#pragma unroll
            for (int m = LPP; m < 64; m <<= 1) t += __shfl_xor(t, m);
            if (lane < LPP) s_red[wave][k * 64 + lane * CH + c] = t;
        }
        float t = gb[k];
#pragma unroll
        for (int m = LPP; m < 64; m <<= 1) t += __shfl_xor(t, m);
        if (lane == 0) s_red[wave][KM * 64 + k] = t;
    }
    __syncthreads();
    for (int j = tid; j < ROW; j += 256)
        partial[(size_t)blockIdx.x * ROW + j] = (s_red[0][j] + s_red[1][j]) + (s_red[2][j] + s_red[3][j]);
}

__global__ void final_conv_scatter_kernel(const float *__restrict__ sums, int K, int KM, float *__restrict__ dw, float *__restrict__ db) {
    const int t = threadIdx.x + blockIdx.x * blockDim.x;
    if (t < K * 64) dw[t] = sums[t];
    if (t < K) db[t] = sums[KM * 64 + t];
}

// bias gradient of a BatchNorm-less convolution (the plain UNet's ConvTranspose2d, models/unet.py:30):
// db[c] = sum over pixels of the bf16 NHWC output gradient.  thread = (8 channels, pixel group); per-block partials.
template <bool F32>
__global__ __launch_bounds__(256) void bias_grad_kernel(const unsigned short *__restrict__ g, unsigned npix, int C,
                                                        float *__restrict__ partial) {
    __shared__ float s_red[256][9];
    const int VPP = C / 8, tid = threadIdx.x;
    const int slot = tid % VPP;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    const unsigned ppb = 256 / VPP;
    for (unsigned p = first_pixel(ppb, VPP); p < npix; p += gridDim.x * ppb) {
        if (F32) {
            float t[8];
            ldf8(g, (size_t)p * C + slot * 8, t);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += t[j];
        } else {
            V16 v;
            v.u = *reinterpret_cast<const uint4 *>(g + (size_t)p * C + slot * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += bf2f(v.h[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s_red[tid][j] = acc[j];
    __syncthreads();
    for (int q = tid; q < C; q += 256) {
        const int sl = q / 8, j = q % 8;
        float t = 0.f;
        for (int k = sl; k < 256; k += VPP) t += s_red[k][j];
        partial[(size_t)blockIdx.x * C + q] = t;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------
extern "C" int cdnet_dam_head_backward(const cdnet_head_feat *f1, const cdnet_head_feat *f2, const cdnet_head_feat *f3,
                                       const float *head_weights, const float *dmask, const float *dpoint, const float *ddir,
                                       int N, int H, int W, uint16_t *df1, uint16_t *df2, uint16_t *df3, float *workspace,
                                       size_t workspace_floats, float *dhead_weights, void *stream) {
    CDNET_REQUIRE(f1 && f2 && f3 && head_weights && dmask && dpoint && ddir && df1 && df2 && df3 && workspace && dhead_weights,
                  "cdnet_dam_head_backward: null pointer");
    const size_t total = (size_t)N * H * W;
    const int nb = 1024;                                    // both kernels write partial[nb][855] (disjoint column ranges)
    const size_t need = (size_t)nb * HEADW_FLOATS + total * 16;
    if (workspace_floats < need) { set_error("cdnet_dam_head_backward: workspace %zu < %zu floats", workspace_floats, need); return CDNET_E_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    float *partial = workspace, *coef = workspace + (size_t)nb * HEADW_FLOATS;
    const HeadFeat a = mk_hf(*f1), b = mk_hf(*f2), c = mk_hf(*f3);
    auto plain = [](const HeadFeat &f) { return f.f16 == 0 && !f.scale && !f.relu && !f.res; };
    auto train = [](const HeadFeat &f) { return f.f16 == 1 && f.scale && f.relu && f.res; };
    const HeadW *hw = reinterpret_cast<const HeadW *>(head_weights);
    if (plain(a) && plain(b) && plain(c)) {
        dam_head_bwd_kernel<0><<<nb, 256, 0, st>>>(a, b, c, hw, dmask, dpoint, ddir, N, H * W, df1, df2, df3, coef, partial);
        dam_head_wgrad_kernel<0><<<nb, 256, 0, st>>>(a, b, c, coef, N, H * W, partial);
    } else if (train(a) && train(b) && train(c)) {
        dam_head_bwd_kernel<1><<<nb, 256, 0, st>>>(a, b, c, hw, dmask, dpoint, ddir, N, H * W, df1, df2, df3, coef, partial);
        dam_head_wgrad_kernel<1><<<nb, 256, 0, st>>>(a, b, c, coef, N, H * W, partial);
    } else {
        dam_head_bwd_kernel<2><<<nb, 256, 0, st>>>(a, b, c, hw, dmask, dpoint, ddir, N, H * W, df1, df2, df3, coef, partial);
        dam_head_wgrad_kernel<2><<<nb, 256, 0, st>>>(a, b, c, coef, N, H * W, partial);
    }
    reduce_partials_kernel<<<cdiv(HEADW_FLOATS, 4), 256, 0, st>>>(workspace, nb, HEADW_FLOATS, dhead_weights);
    return check_launch("cdnet_dam_head_backward");
}

extern "C" size_t cdnet_dam_head_backward_workspace_floats(int N, int H, int W) {
    return (size_t)1024 * HEADW_FLOATS + (size_t)N * H * W * 16;
}

extern "C" int cdnet_dam_head_backward_fused_blocks(void) { return HEAD_FUSED_BLOCKS; }
/* private (scratch) memory per lane of dam_head_bwd_fused_kernel as built: it holds 256 VGPRs only just - a test keeps this at 0 */
template <bool COEF>
static int head_fused_scratch_bytes() {
    hipFuncAttributes at;
    if (hipFuncGetAttributes(&at, reinterpret_cast<const void *>(dam_head_bwd_fused_kernel<COEF>)) != hipSuccess) return -1;
    return (int)at.localSizeBytes;
}
extern "C" int cdnet_dam_head_backward_fused_scratch_bytes(void) { return head_fused_scratch_bytes<false>(); }
extern "C" int cdnet_dam_head_backward_coef_scratch_bytes(void) { return head_fused_scratch_bytes<true>(); }
extern "C" size_t cdnet_dam_head_backward_fused_workspace_floats(void) { return (size_t)HEAD_FUSED_BLOCKS * (HEADW_FLOATS + 64 * 24); }

// both forms of the one-pass head backward: coef == NULL stores df1 and df2, otherwise the coefficient rows
static int head_backward_fused(const char *who, const cdnet_head_feat *f1, const cdnet_head_feat *f2, const cdnet_head_feat *f3,
                               const float *head_weights, const float *dmask, const float *dpoint, const float *ddir, int N, int H, int W,
                               float *df1, float *df2, float *coef, float *dz3, float *workspace, size_t workspace_floats,
                               float *dhead_weights, void *stream);

extern "C" int cdnet_dam_head_backward_fused(const cdnet_head_feat *f1, const cdnet_head_feat *f2, const cdnet_head_feat *f3,
                                             const float *head_weights, const float *dmask, const float *dpoint, const float *ddir,
                                             int N, int H, int W, float *df1, float *df2, float *dz3, float *workspace,
                                             size_t workspace_floats, float *dhead_weights, void *stream) {
    CDNET_REQUIRE(f1 && f2 && f3 && head_weights && dmask && dpoint && ddir && df1 && df2 && dz3 && workspace && dhead_weights,
                  "cdnet_dam_head_backward_fused: null pointer");
    return head_backward_fused("cdnet_dam_head_backward_fused", f1, f2, f3, head_weights, dmask, dpoint, ddir, N, H, W, df1, df2, nullptr, dz3,
                               workspace, workspace_floats, dhead_weights, stream);
}

extern "C" int cdnet_dam_head_backward_coef(const cdnet_head_feat *f1, const cdnet_head_feat *f2, const cdnet_head_feat *f3,
                                            const float *head_weights, const float *dmask, const float *dpoint, const float *ddir,
                                            int N, int H, int W, float *coef, float *dz3, float *workspace, size_t workspace_floats,
                                            float *dhead_weights, void *stream) {
    CDNET_REQUIRE(f1 && f2 && f3 && head_weights && dmask && dpoint && ddir && coef && dz3 && workspace && dhead_weights,
                  "cdnet_dam_head_backward_coef: null pointer");
    return head_backward_fused("cdnet_dam_head_backward_coef", f1, f2, f3, head_weights, dmask, dpoint, ddir, N, H, W, nullptr, nullptr, coef, dz3,
                               workspace, workspace_floats, dhead_weights, stream);
}

static int head_backward_fused(const char *who, const cdnet_head_feat *f1, const cdnet_head_feat *f2, const cdnet_head_feat *f3,
                               const float *head_weights, const float *dmask, const float *dpoint, const float *ddir, int N, int H, int W,
                               float *df1, float *df2, float *coef, float *dz3, float *workspace, size_t workspace_floats,
                               float *dhead_weights, void *stream) {
    auto plain32 = [](const cdnet_head_feat &f) { return f.raw && f.f16 == 2 && !f.scale && !f.shift && !f.relu && !f.res; };
    CDNET_REQUIRE(plain32(*f1) && plain32(*f2) && plain32(*f3),
                  "%s: plain stored fp32 features only (f16 = 2, no scale / shift / relu / res)", who);
    CDNET_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: N=%d H=%d W=%d", who, N, H, W);
    CDNET_REQUIRE((size_t)N * H * W * 64 < ((size_t)1 << 32), "%s: tensor too large for 32-bit element indexing", who);
    static_assert(HEAD_FUSED_BLOCKS == 1024, "the chains of the two-kernel path: 1024 workgroups");
    const int nb = HEAD_FUSED_BLOCKS;
    const size_t need = (size_t)nb * (HEADW_FLOATS + 64 * 24);
    if (workspace_floats < need) { set_error("%s: workspace %zu < %zu floats", who, workspace_floats, need); return CDNET_E_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    float *partial = workspace, *sgbuf = workspace + (size_t)nb * HEADW_FLOATS;
    auto fp = [](const cdnet_head_feat &f) { return reinterpret_cast<const float *>(f.raw); };
    const HeadW *hw = reinterpret_cast<const HeadW *>(head_weights);
    if (coef) dam_head_bwd_fused_kernel<true><<<nb, 512, 0, st>>>(fp(*f1), fp(*f2), fp(*f3), hw, dmask, dpoint, ddir, N, H * W, df1, df2, coef, dz3, partial, sgbuf);
    else dam_head_bwd_fused_kernel<false><<<nb, 512, 0, st>>>(fp(*f1), fp(*f2), fp(*f3), hw, dmask, dpoint, ddir, N, H * W, df1, df2, coef, dz3, partial, sgbuf);
    head_scalar_reduce_kernel<<<nb, 64, 0, st>>>(sgbuf, partial);
    reduce_partials_kernel<<<cdiv(HEADW_FLOATS, 4), 256, 0, st>>>(workspace, nb, HEADW_FLOATS, dhead_weights);
    return check_launch(who);
}

extern "C" size_t cdnet_final_conv1x1_backward_workspace_floats(void) { return (size_t)1025 * (FC_KMOST * 64 + FC_KMOST); }

extern "C" int cdnet_final_conv1x1_backward(const cdnet_head_feat *f, const float *w, const float *dlogits, int K, int N, int H, int W,
                                            uint16_t *df, float *workspace, size_t workspace_floats, float *dw, float *db, void *stream) {
    CDNET_REQUIRE(f && f->raw && w && dlogits && df && workspace && dw && db, "cdnet_final_conv1x1_backward: null pointer");
    CDNET_REQUIRE(K >= 1 && K <= FC_KMOST && N > 0 && H > 0 && W > 0, "cdnet_final_conv1x1_backward: K=%d must be in [1,%d]", K, FC_KMOST);
    if (workspace_floats < cdnet_final_conv1x1_backward_workspace_floats()) { set_error("cdnet_final_conv1x1_backward: workspace too small"); return CDNET_E_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)N * H * W;
    const bool wide = K > FC_KMAX;
    const bool most = K > FC_KWIDE;
    const int KM = most ? FC_KMOST : wide ? FC_KWIDE : FC_KMAX;
    int nb = (int)((npix + (wide ? 31 : 63)) / (wide ? 32 : 64));
    if (nb > 1024) nb = 1024;
    const int ROW = KM * 64 + KM;
    float *sums = workspace + (size_t)1024 * ROW;
    if (most) final_conv_bwd_kernel<FC_KMOST, 8><<<nb, 256, 0, st>>>(mk_hf(*f), w, dlogits, K, N, H * W, df, workspace);
    else if (wide) final_conv_bwd_kernel<FC_KWIDE, 8><<<nb, 256, 0, st>>>(mk_hf(*f), w, dlogits, K, N, H * W, df, workspace);
    else final_conv_bwd_kernel<FC_KMAX, 4><<<nb, 256, 0, st>>>(mk_hf(*f), w, dlogits, K, N, H * W, df, workspace);
    reduce_partials_kernel<<<cdiv(ROW, 4), 256, 0, st>>>(workspace, nb, ROW, sums);
    final_conv_scatter_kernel<<<cdiv(K * 64, 256), 256, 0, st>>>(sums, K, KM, dw, db);
    return check_launch("cdnet_final_conv1x1_backward");
}

extern "C" size_t cdnet_bias_grad_workspace_floats(int C) { return (size_t)512 * C; }

static int bias_grad_impl(const uint16_t *grad_out, size_t npix, int C, float *workspace, size_t workspace_floats, float *db, void *stream, bool f32);
extern "C" int cdnet_bias_grad(const uint16_t *grad_out, size_t npix, int C, float *workspace, size_t workspace_floats, float *db,
                               void *stream) {
    return bias_grad_impl(grad_out, npix, C, workspace, workspace_floats, db, stream, false);
}
extern "C" int cdnet_bias_grad_f32(const float *grad_out, size_t npix, int C, float *workspace, size_t workspace_floats, float *db,
                                   void *stream) {
    return bias_grad_impl(reinterpret_cast<const uint16_t *>(grad_out), npix, C, workspace, workspace_floats, db, stream, true);
}
static int bias_grad_impl(const uint16_t *grad_out, size_t npix, int C, float *workspace, size_t workspace_floats, float *db, void *stream, bool f32) {
    CDNET_REQUIRE(grad_out && workspace && db, "cdnet_bias_grad: null pointer");
    CDNET_REQUIRE(C >= 8 && C % 8 == 0 && C <= 2048 && npix > 0 && npix < ((size_t)1 << 31), "cdnet_bias_grad: C=%d unsupported", C);
    if (workspace_floats < cdnet_bias_grad_workspace_floats(C)) { set_error("cdnet_bias_grad: workspace too small"); return CDNET_E_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const unsigned ppb = 256 / (C / 8);
    int nb = (int)((npix + ppb * 8 - 1) / (ppb * 8));
    if (nb > 512) nb = 512;
    if (nb < 1) nb = 1;
    if (f32) bias_grad_kernel<true><<<nb, 256, 0, st>>>(grad_out, (unsigned)npix, C, workspace);
    else bias_grad_kernel<false><<<nb, 256, 0, st>>>(grad_out, (unsigned)npix, C, workspace);
    reduce_partials_kernel<<<cdiv(C, 4), 256, 0, st>>>(workspace, nb, C, db);
    return check_launch("cdnet_bias_grad");
}
