// The backbone U-Net's 1x1 classifier (models/model_unet.py:166,194 final_conv 16 -> K) on the 16-channel feature the last
// decoder block leaves, forward and backward.  The feature is a cdnet_head_feat whose tensors are NHWC [N][H][W][16] and whose
// `res` is NULL: F = [relu](raw * scale + shift), bf16 / fp16 / fp32 storage.  Everything after the storage format is fp32:
// nothing is rounded to 16 bits between the feature and the logits (16 products per logit do not need the matrix cores).
#include "head_feat.h"
#include "launch.h"
#include "train_util.h"

using namespace cdnet;

namespace {

constexpr int C16 = 16;               // channels of the feature
constexpr int C16_KMAX = 20;          // most classes (the 64-channel backward's limit)
constexpr int C16_KFEW = 4;           // the instantiation of the 3-class configuration

// NC channels from c0 of pixel `pix`: storage format FMT (0 bf16, 1 fp16, 2 fp32) -> the activated fp32 feature
template <int FMT, int NC>
__device__ __forceinline__ void load_feat_c16(const HeadFeat &f, size_t pix, int c0, const float *s_sc, const float *s_sh, float *v) {
    static_assert(NC == 4 || NC == 16, "a quarter of the pixel or all of it");
    const size_t e = pix * C16 + c0;
    if constexpr (FMT == 2) {
        const float4 *p = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(f.raw) + e);
#pragma unroll
        for (int q = 0; q < NC / 4; ++q) {
            const float4 r = p[q];
            v[q * 4 + 0] = r.x; v[q * 4 + 1] = r.y; v[q * 4 + 2] = r.z; v[q * 4 + 3] = r.w;
        }
    } else if constexpr (NC == 16) {
        const uint4 *p = reinterpret_cast<const uint4 *>(f.raw + e);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            V16 r;
            r.u = p[q];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[q * 8 + j] = ld16(r.h[j], FMT == 1);
        }
    } else {
        const uint2 r = *reinterpret_cast<const uint2 *>(f.raw + e);
        const unsigned short *h = reinterpret_cast<const unsigned short *>(&r);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ld16(h[j], FMT == 1);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        float t = v[j];
        if (f.scale) t = fmaf(t, s_sc[c0 + j], s_sh[c0 + j]);
        if (f.relu) t = fmaxf(t, 0.f);
        v[j] = t;
    }
}

// logits f32 NCHW [N][K][plane]: one thread per pixel, weights / bias / affine staged in LDS once per workgroup
template <int FMT>
__global__ __launch_bounds__(256) void final_conv1x1_c16_kernel(HeadFeat f, const float *__restrict__ w, const float *__restrict__ b,
                                                                int K, size_t total, size_t plane, float *__restrict__ out) {
    __shared__ float s_w[C16_KMAX * C16], s_b[C16_KMAX], s_sc[C16], s_sh[C16];
    for (int i = threadIdx.x; i < K * C16; i += 256) s_w[i] = w[i];
    if (threadIdx.x < K) s_b[threadIdx.x] = b[threadIdx.x];
    if (threadIdx.x < C16) {
        s_sc[threadIdx.x] = f.scale ? f.scale[threadIdx.x] : 1.f;
        s_sh[threadIdx.x] = f.scale ? f.shift[threadIdx.x] : 0.f;
    }
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t n = i / plane, p = i - n * plane;
        float v[C16];
        load_feat_c16<FMT, C16>(f, i, 0, s_sc, s_sh, v);
        for (int k = 0; k < K; ++k) {
            float s = s_b[k];
#pragma unroll
            for (int c = 0; c < C16; ++c) s = fmaf(s_w[k * C16 + c], v[c], s);
            out[(n * K + k) * plane + p] = s;
        }
    }
}

// Backward.  Four lanes per pixel, four channels each (64 pixels per workgroup):
//   dF[c] = sum_k dlogit_k * w[k][c];  dW[k][c] = sum_px dlogit_k * F[c];  db[k] = sum_px dlogit_k.
// Per-workgroup partial rows [KM*16 | KM], summed in a fixed order by reduce_partials_kernel: no atomics, same bits every run.
constexpr int C16_LPP = 4, C16_CH = C16 / C16_LPP, C16_PPB = 256 / C16_LPP;
constexpr int C16_BLOCKS = 1024;      // most workgroups of the backward (rows of partial sums)

template <int FMT, int KM>
__global__ __launch_bounds__(256) void final_conv_c16_bwd_kernel(HeadFeat f, const float *__restrict__ w, const float *__restrict__ dl,
                                                                 int K, size_t total, size_t plane, void *__restrict__ df,
                                                                 float *__restrict__ partial) {
    constexpr int LPP = C16_LPP, CH = C16_CH, ROW = KM * C16 + KM;
    __shared__ float s_w[KM * C16], s_sc[C16], s_sh[C16];
    __shared__ float s_red[4][ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < KM * C16; i += 256) s_w[i] = i < K * C16 ? w[i] : 0.f;
    if (tid < C16) { s_sc[tid] = f.scale ? f.scale[tid] : 1.f; s_sh[tid] = f.scale ? f.shift[tid] : 0.f; }
    __syncthreads();
    const int q = tid % LPP;
    float gw[KM][CH], gb[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        gb[k] = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) gw[k][c] = 0.f;
    }
    for (size_t base = (size_t)blockIdx.x * C16_PPB; base < total; base += (size_t)gridDim.x * C16_PPB) {
        const size_t i = base + (tid / LPP);
        const bool ok = i < total;
        const size_t ii = ok ? i : total - 1;              // (lanes past the end read the last pixel and add zeros)
        const size_t n = ii / plane, p = ii - n * plane;
        float v[CH], d[KM], o[CH];
        load_feat_c16<FMT, CH>(f, ii, q * CH, s_sc, s_sh, v);
#pragma unroll
        for (int k = 0; k < KM; ++k) d[k] = (ok && k < K) ? dl[(n * K + k) * plane + p] : 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < KM; ++k) {
                t = fmaf(d[k], s_w[k * C16 + q * CH + c], t);
                gw[k][c] = fmaf(d[k], v[c], gw[k][c]);
            }
            o[c] = t;
        }
#pragma unroll
        for (int k = 0; k < KM; ++k) gb[k] += d[k];
        if (ok) {
            const size_t e = ii * C16 + q * CH;
            if constexpr (FMT == 2) {
                *reinterpret_cast<float4 *>(reinterpret_cast<float *>(df) + e) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
                uint2 pk;
                pk.x = (unsigned)f2bf(o[0]) | ((unsigned)f2bf(o[1]) << 16);
                pk.y = (unsigned)f2bf(o[2]) | ((unsigned)f2bf(o[3]) << 16);
                *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(df) + e) = pk;
            }
        }
    }
    // lanes with the same q own the same channels: butterfly over the 16 pixel slots of the wave, then one row per wave
#pragma unroll
    for (int k = 0; k < KM; ++k) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            float t = gw[k][c];
#pragma unroll
            for (int m = LPP; m < 64; m <<= 1) t += __shfl_xor(t, m);
            if (lane < LPP) s_red[wave][k * C16 + lane * CH + c] = t;
        }
        float t = gb[k];
#pragma unroll
        for (int m = LPP; m < 64; m <<= 1) t += __shfl_xor(t, m);
        if (lane == 0) s_red[wave][KM * C16 + k] = t;
    }
    __syncthreads();
    for (int j = tid; j < ROW; j += 256)
        partial[(size_t)blockIdx.x * ROW + j] = (s_red[0][j] + s_red[1][j]) + (s_red[2][j] + s_red[3][j]);
}

__global__ void final_conv_c16_scatter_kernel(const float *__restrict__ sums, int K, int KM, float *__restrict__ dw, float *__restrict__ db) {
    const int t = threadIdx.x + blockIdx.x * blockDim.x;
    if (t < K * C16) dw[t] = sums[t];
    if (t < K) db[t] = sums[KM * C16 + t];
}

// the checks both entries share; `what` names the entry in the message
int check_feat_c16(const cdnet_head_feat *f, int K, int N, int H, int W, const char *what) {
    CDNET_REQUIRE(f->res == nullptr, "%s: a 16-channel feature has no residual operand (res must be NULL)", what);
    CDNET_REQUIRE(f->f16 >= 0 && f->f16 <= 2, "%s: f16=%d must be 0 (bf16), 1 (fp16) or 2 (fp32)", what, f->f16);
    CDNET_REQUIRE((f->scale == nullptr) == (f->shift == nullptr), "%s: scale and shift come together", what);
    CDNET_REQUIRE(K >= 1 && K <= C16_KMAX, "%s: K=%d must be in [1,%d]", what, K, C16_KMAX);
    CDNET_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad size N=%d H=%d W=%d", what, N, H, W);
    CDNET_REQUIRE(reinterpret_cast<uintptr_t>(f->raw) % 16 == 0, "%s: the feature must be 16-byte aligned", what);
    return CDNET_OK;
}

template <int FMT>
void launch_c16_bwd(int KM, int nb, hipStream_t st, const HeadFeat &hf, const float *w, const float *dl, int K, size_t total, size_t plane,
                    void *df, float *partial) {
    if (KM == C16_KMAX) final_conv_c16_bwd_kernel<FMT, C16_KMAX><<<nb, 256, 0, st>>>(hf, w, dl, K, total, plane, df, partial);
    else final_conv_c16_bwd_kernel<FMT, C16_KFEW><<<nb, 256, 0, st>>>(hf, w, dl, K, total, plane, df, partial);
}

}  // namespace

extern "C" int cdnet_final_conv1x1_c16(const cdnet_head_feat *f, const float *w, const float *b, int K, int N, int H, int W,
                                       float *out, void *stream) {
    CDNET_REQUIRE(f && f->raw && w && b && out, "cdnet_final_conv1x1_c16: null pointer");
    if (int rc = check_feat_c16(f, K, N, H, W, "cdnet_final_conv1x1_c16")) return rc;
    const size_t plane = (size_t)H * W, total = (size_t)N * plane;
    const HeadFeat hf = mk_hf(*f);
    const int grid = lin_grid(total, 4096);
    hipStream_t st = (hipStream_t)stream;
    if (f->f16 == 2) final_conv1x1_c16_kernel<2><<<grid, 256, 0, st>>>(hf, w, b, K, total, plane, out);
    else if (f->f16 == 1) final_conv1x1_c16_kernel<1><<<grid, 256, 0, st>>>(hf, w, b, K, total, plane, out);
    else final_conv1x1_c16_kernel<0><<<grid, 256, 0, st>>>(hf, w, b, K, total, plane, out);
    return check_launch("cdnet_final_conv1x1_c16");
}

extern "C" size_t cdnet_final_conv1x1_c16_backward_workspace_floats(void) {
    return (size_t)(C16_BLOCKS + 1) * (C16_KMAX * C16 + C16_KMAX);
}

extern "C" int cdnet_final_conv1x1_c16_backward(const cdnet_head_feat *f, const float *w, const float *dlogits, int K, int N, int H, int W,
                                                void *df, float *workspace, size_t workspace_floats, float *dw, float *db, void *stream) {
    CDNET_REQUIRE(f && f->raw && w && dlogits && df && workspace && dw && db, "cdnet_final_conv1x1_c16_backward: null pointer");
    if (int rc = check_feat_c16(f, K, N, H, W, "cdnet_final_conv1x1_c16_backward")) return rc;
    CDNET_REQUIRE(reinterpret_cast<uintptr_t>(df) % 16 == 0, "cdnet_final_conv1x1_c16_backward: df must be 16-byte aligned");
    const size_t need = cdnet_final_conv1x1_c16_backward_workspace_floats();
    if (workspace_floats < need) {
        set_error("cdnet_final_conv1x1_c16_backward: workspace %zu < %zu floats", workspace_floats, need);
        return CDNET_E_WORKSPACE;
    }
    const size_t plane = (size_t)H * W, total = (size_t)N * plane;
    const size_t want = (total + C16_PPB - 1) / C16_PPB;
    const int nb = (int)(want > (size_t)C16_BLOCKS ? (size_t)C16_BLOCKS : want);
    const int KM = K > C16_KFEW ? C16_KMAX : C16_KFEW;
    const int ROW = KM * C16 + KM;
    float *sums = workspace + (size_t)C16_BLOCKS * ROW;
    const HeadFeat hf = mk_hf(*f);
    hipStream_t st = (hipStream_t)stream;
    if (f->f16 == 2) launch_c16_bwd<2>(KM, nb, st, hf, w, dlogits, K, total, plane, df, workspace);
    else if (f->f16 == 1) launch_c16_bwd<1>(KM, nb, st, hf, w, dlogits, K, total, plane, df, workspace);
    else launch_c16_bwd<0>(KM, nb, st, hf, w, dlogits, K, total, plane, df, workspace);
    reduce_partials_kernel<<<cdiv(ROW, 4), 256, 0, st>>>(workspace, nb, ROW, sums);
    final_conv_c16_scatter_kernel<<<cdiv(K * C16, 256), 256, 0, st>>>(sums, K, KM, dw, db);
    return check_launch("cdnet_final_conv1x1_c16_backward");
}
