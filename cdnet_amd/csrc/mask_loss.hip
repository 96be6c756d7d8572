// The plain UNet's loss (train_util.py:128-136, 183-190, 209-218): the mask terms of the DAM loss on their own, with a `terms` word
// that switches the weight map, the cross-entropy and the dice term (--weight-map, --alpha 2 / --dice 2, --dice 0), and the pixel
// metrics of the mask arg-max.  Three launches: per-chunk sums, one finalize block, the gradient.
//
// The reduction has the shape of dam_loss.hip's loss_reduce_kernel<9> / loss_finalize_kernel (256 threads, pixel i = chunk * 256 + tid,
// stride nchunk * 256, the 256 per-thread partials summed serially in lane order, the chunks in four chains: loss_util.h holds that
// text once for both) and the expressions of loss_grad_kernel's mask part, so with every term on the results equal
// cdnet_dam_loss_classes' mask terms bit for bit.  The private
// sums live in registers here (the DAM kernel keeps them in LDS because its direction sums are indexed by the target class): a sum
// that class `lab` does not touch adds +0.f, which leaves a non-negative float unchanged.
//
// Traffic per pixel: 12 B logits + 1 B label (+ 1 B weight) in each pass, 12 B gradient out: 38-40 B.
#include "loss_util.h"
#include "launch.h"

using namespace cdnet;

namespace {

// per-sample sums: 0..2 I_c = sum p_c [label==c]   3..5 P_c = sum p_c   6..8 T_c = sum [label==c]   9 ce   10 tp  11 fp  12 fn
constexpr int MS_SUMS = 13;
constexpr int MS_COEF = 6;          // dice alpha[3], beta[3] per sample (loss_finalize_kernel's cf[0..5])
constexpr int MS_TPB = 256;

struct MaskIn {
    const float *mask;              // f32 [B][3][P]
    const unsigned char *label;     // u8 [B][P]
    const unsigned char *weight;    // u8 [B][P] or NULL (WMAP clear)
    int B, P;
    unsigned terms;
};

__global__ __launch_bounds__(MS_TPB) void mask_loss_reduce_kernel(MaskIn L, float *__restrict__ partial, int *__restrict__ err) {
    __shared__ float acc[MS_SUMS][MS_TPB + 1];      // + 1: the 13 rows the serial sums walk start in 13 different banks
    const int tid = threadIdx.x, b = blockIdx.y;
    const bool wmap = (L.terms & CDNET_LOSS_WMAP) != 0;
    float s[MS_SUMS];
#pragma unroll
    for (int k = 0; k < MS_SUMS; ++k) s[k] = 0.f;
    int bad = 0;
    const size_t ob = (size_t)b * L.P;
    for (int i = blockIdx.x * MS_TPB + tid; i < L.P; i += gridDim.x * MS_TPB) {
        float l3[3], p3[3], lp3[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) l3[c] = L.mask[((size_t)b * 3 + c) * L.P + i];
        softmax3(l3, p3, lp3);
        int lab = L.label[ob + i];
        bad |= lab > 2;
        lab = lab > 2 ? 2 : lab;                   // (reported through *err: the finalize kernel poisons every value with NaN)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s[c] += c == lab ? p3[c] : 0.f;
            s[3 + c] += p3[c];
            s[6 + c] += c == lab ? 1.f : 0.f;
        }
        const float lpl = lab == 0 ? lp3[0] : lab == 1 ? lp3[1] : lp3[2];
        if (wmap) {
            const float w = (float)L.weight[ob + i] / 20.f;
            s[9] -= lpl * w;
        } else {
            s[9] -= lpl;
        }
        {   // np.argmax over the three classes (first maximum), "inside" = class 1 (train_util.py:211-212, utils.py:76-78)
            int am = 0;
            float best = l3[0];
#pragma unroll
            for (int c = 1; c < 3; ++c) if (l3[c] > best) { best = l3[c]; am = c; }
            const bool pi = am == 1, ti = lab == 1;
            s[10] += pi && ti ? 1.f : 0.f;
            s[11] += pi && !ti ? 1.f : 0.f;
            s[12] += !pi && ti ? 1.f : 0.f;
        }
    }
    if (bad) atomicOr(err, 1);
#pragma unroll
    for (int k = 0; k < MS_SUMS; ++k) acc[k][tid] = s[k];
    __syncthreads();
    row_sum<MS_TPB>(acc, tid, b, partial);
}

// single block: per-sample sums -> the eight reported values and the dice coefficients of the gradient pass
__global__ __launch_bounds__(256) void mask_loss_finalize_kernel(const float *__restrict__ partial, int nchunk, int B, int P, unsigned terms,
                                                                 float *__restrict__ coef, float *__restrict__ losses,
                                                                 const int *__restrict__ err) {
    constexpr int NS = MS_SUMS;
    __shared__ float s_sum[64 * NS];      // B <= 64
    __shared__ float s_term[3];
    const int tid = threadIdx.x;
    for (int idx = tid; idx < B * NS; idx += 256) {
        const int b = idx / NS, k = idx % NS;
        s_sum[idx] = chunk_sum<NS>(partial + (size_t)b * nchunk * NS + k, nchunk);
    }
    __syncthreads();
    const float fB = (float)B;
    for (int b = tid; b < B; b += 256) mask_dice_coef(s_sum + b * NS, fB, coef + (size_t)b * MS_COEF);
    if (tid < 3) s_term[tid] = dice_term<NS>(s_sum, B, fB, tid, 3 + tid, 6 + tid);      // 1 - mean_b 2 (I_c + 1) / (P_c + T_c + 1)
    __syncthreads();
    if (tid == 0) {
        const float n = (float)B * (float)P;
        float ce = 0.f;
        for (int b = 0; b < B; ++b) ce += s_sum[b * NS + 9];
        ce /= n;
        float dice = 0.f;
        for (int c = 0; c < 3; ++c) dice += s_term[c];
        const bool on_ce = (terms & CDNET_LOSS_CE) != 0, on_dice = (terms & CDNET_LOSS_DICE) != 0;
        losses[0] = on_ce && on_dice ? ce + dice : on_ce ? ce : on_dice ? dice : 0.f;
        losses[1] = ce; losses[2] = dice;
        pixel_metrics<NS>(s_sum, 10, B, P, losses + 3);
        poison_on_error(err, losses, 8);
    }
}

// gradient of `total` w.r.t. the logits: written, not accumulated (zeros when neither term is on)
__global__ __launch_bounds__(256) void mask_loss_grad_kernel(MaskIn L, const float *__restrict__ coef, float *__restrict__ dmask) {
    const int b = blockIdx.y;
    const float *cf = coef + (size_t)b * MS_COEF;
    const float inv_n = 1.f / ((float)L.B * (float)L.P);
    const size_t ob = (size_t)b * L.P;
    const bool wmap = (L.terms & CDNET_LOSS_WMAP) != 0, on_ce = (L.terms & CDNET_LOSS_CE) != 0, on_dice = (L.terms & CDNET_LOSS_DICE) != 0;
    if (!on_ce && !on_dice) {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < L.P; i += gridDim.x * 256)
#pragma unroll
            for (int c = 0; c < 3; ++c) dmask[((size_t)b * 3 + c) * L.P + i] = 0.f;
        return;
    }
    float cfr[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) cfr[k] = on_dice ? cf[k] : 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < L.P; i += gridDim.x * 256) {
        float l3[3], p3[3], lp3[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) l3[c] = L.mask[((size_t)b * 3 + c) * L.P + i];
        softmax3(l3, p3, lp3);
        const float w = wmap ? (float)L.weight[ob + i] / 20.f : 1.f;
        int lab = L.label[ob + i];
        lab = lab > 2 ? 2 : lab;
        // dice gradient w.r.t. the probabilities, through the softmax, plus the (weighted) CE
        float gp[3], dot = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { gp[c] = cfr[3 + c] + (c == lab ? cfr[c] : 0.f); dot = fmaf(p3[c], gp[c], dot); }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gd = p3[c] * (gp[c] - dot), gc = w * inv_n * (p3[c] - (c == lab ? 1.f : 0.f));
            dmask[((size_t)b * 3 + c) * L.P + i] = on_ce && on_dice ? gd + gc : on_dice ? gd : gc;
        }
    }
}

}  // namespace

extern "C" size_t cdnet_mask_loss_workspace_floats(int B, int P) {
    if (B < 1 || P < 1) return 0;
    return (size_t)B * loss_nchunk(P, MS_TPB) * MS_SUMS + (size_t)B * MS_COEF + 16;   // partial | coef | pad (error flag)
}

extern "C" int cdnet_mask_loss(const float *mask_logits, const uint8_t *label, const uint8_t *weight_u8, int B, int H, int W, unsigned terms,
                               float *workspace, size_t workspace_floats, float *losses, float *dmask, void *stream) {
    CDNET_REQUIRE(mask_logits && label && workspace && losses, "cdnet_mask_loss: null pointer");
    CDNET_REQUIRE(B >= 1 && B <= 64, "cdnet_mask_loss: batch %d not in [1,64]", B);
    CDNET_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL / 4, "cdnet_mask_loss: image %d x %d", H, W);
    CDNET_REQUIRE((terms & ~(CDNET_LOSS_WMAP | CDNET_LOSS_CE | CDNET_LOSS_DICE)) == 0, "cdnet_mask_loss: terms %u has unknown bits", terms);
    CDNET_REQUIRE(weight_u8 || !(terms & CDNET_LOSS_WMAP), "cdnet_mask_loss: CDNET_LOSS_WMAP needs the weight map");
    const int P = H * W;
    CDNET_REQUIRE(workspace_floats >= cdnet_mask_loss_workspace_floats(B, P), "cdnet_mask_loss: workspace too small");
    const int nchunk = loss_nchunk(P, MS_TPB);
    float *partial = workspace;
    float *coef = partial + (size_t)B * nchunk * MS_SUMS;
    int *err = reinterpret_cast<int *>(coef + (size_t)B * MS_COEF);
    MaskIn L;
    L.mask = mask_logits; L.label = label; L.weight = weight_u8; L.B = B; L.P = P; L.terms = terms;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) return check_launch("cdnet_mask_loss(memset)");
    mask_loss_reduce_kernel<<<dim3(nchunk, B), MS_TPB, 0, st>>>(L, partial, err);
    mask_loss_finalize_kernel<<<1, 256, 0, st>>>(partial, nchunk, B, P, terms, coef, losses, err);
    if (dmask) mask_loss_grad_kernel<<<dim3(lin_grid((size_t)P, 2048), B), 256, 0, st>>>(L, coef, dmask);
    return check_launch("cdnet_mask_loss");
}
