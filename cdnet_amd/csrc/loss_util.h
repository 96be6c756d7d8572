// What the two loss paths share (dam_loss.hip: the five-term DAM loss and validate()'s sums; mask_loss.hip: the plain UNet's mask
// terms): the softmaxes, the chunk rule and the pieces of the reduce / finalize kernels.  One text, so both paths compute the same
// bits (tests/test_gpu_mask_loss.py holds them bit-identical); the library is built with -ffp-contract=off, and the order of every
// floating-point operation here is part of that contract.
#pragma once
#include "common.h"

namespace cdnet {

// softmax and log-softmax of the three mask logits
__device__ __forceinline__ void softmax3(const float *l, float *p, float *logp) {
    const float m = fmaxf(l[0], fmaxf(l[1], l[2]));
    float e[3], s = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) { e[c] = expf(l[c] - m); s += e[c]; }
    const float ls = logf(s);
#pragma unroll
    for (int c = 0; c < 3; ++c) { p[c] = e[c] / s; logp[c] = l[c] - m - ls; }
}

template <int NC>
__device__ __forceinline__ void softmax_n(const float *l, float *p, float *logp) {
    float m = l[0];
#pragma unroll
    for (int c = 1; c < NC; ++c) m = fmaxf(m, l[c]);
    float e[NC], s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) { e[c] = expf(l[c] - m); s += e[c]; }
    const float ls = logf(s);
#pragma unroll
    for (int c = 0; c < NC; ++c) { p[c] = e[c] / s; logp[c] = l[c] - m - ls; }
}

// chunks (workgroups) per sample of the loss reductions: 8 pixels per thread, at most 64 chunks - beyond that the threads loop
static int loss_nchunk(int P, int tpb) {
    int nchunk = cdiv(P, tpb * 8);
    return nchunk > 64 ? 64 : nchunk;
}

// the end of a reduce kernel (after its barrier): thread tid < SUMS adds row tid of the LDS accumulator over the TPB threads in
// lane order and stores the chunk's sum.  W >= TPB is the row pitch (mask_loss.hip pads its rows by one float).
template <int TPB, int SUMS, int W>
__device__ __forceinline__ void row_sum(const float (&acc)[SUMS][W], int tid, int b, float *__restrict__ partial) {
    if (tid < SUMS) {
        float s = 0.f;
        for (int k = 0; k < TPB; ++k) s += acc[tid][k];
        partial[((size_t)b * gridDim.x + blockIdx.x) * SUMS + tid] = s;
    }
}

// sum k of sample b over its nchunk chunks, pp = partial + (b * nchunk) * NS + k: four independent chains of loads (a single
// dependent chain of nchunk L2 round trips dominated the finalize kernel), a scalar tail on the first chain
template <int NS>
__device__ __forceinline__ float chunk_sum(const float *pp, int nchunk) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int ch = 0;
    for (; ch + 3 < nchunk; ch += 4) {
        s0 += pp[(size_t)ch * NS]; s1 += pp[(size_t)(ch + 1) * NS];
        s2 += pp[(size_t)(ch + 2) * NS]; s3 += pp[(size_t)(ch + 3) * NS];
    }
    for (; ch < nchunk; ++ch) s0 += pp[(size_t)ch * NS];
    return (s0 + s1) + (s2 + s3);
}

// the mask dice coefficients of one sample for the gradient pass, from its sums S = {I[3], P[3], T[3], ...}:
// cf[c] = alpha_c = -2 / (B (U_c + 1)), cf[3 + c] = beta_c = 2 (I_c + 1) / (B (U_c + 1)^2), U_c = P_c + T_c
__device__ __forceinline__ void mask_dice_coef(const float *S, float fB, float *cf) {
    for (int c = 0; c < 3; ++c) {
        const float I = S[c], U = S[3 + c] + S[6 + c];
        cf[c] = -2.f / (fB * (U + 1.f));
        cf[3 + c] = 2.f * (I + 1.f) / (fB * (U + 1.f) * (U + 1.f));
    }
}

// one batch-mean dice term 1 - mean_b 2 (S[num] + 1) / (S[da] + S[db] + 1) over the rows S = s_sum + b * NS
template <int NS>
__device__ __forceinline__ float dice_term(const float *s_sum, int B, float fB, int num, int da, int db) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) { const float *S = s_sum + b * NS; acc += 2.f * (S[num] + 1.f) / (S[da] + S[db] + 1.f); }
    return 1.f - acc / fB;
}

// pixel-level metrics, mean over the samples (utils.py:67-110): accuracy, IoU, recall, precision, F1 -> out[0..4], from the
// per-sample tp, fp, fn at s_sum[b * NS + tp0 ...]
template <int NS>
__device__ __forceinline__ void pixel_metrics(const float *s_sum, int tp0, int B, int P, float *out) {
    double m[5] = {0, 0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
        const double tp = s_sum[b * NS + tp0], fp = s_sum[b * NS + tp0 + 1], fn = s_sum[b * NS + tp0 + 2];
        const double tn = (double)P - tp - fp - fn;
        const double precision = tp / (tp + fp + 1e-10), recall = tp / (tp + fn + 1e-10);
        m[0] += (tp + tn) / (tp + fp + tn + fn + 1e-10);
        m[1] += tp / (tp + fp + fn + 1e-10);
        m[2] += recall;
        m[3] += precision;
        m[4] += 2 * precision * recall / (precision + recall + 1e-10);
    }
    for (int k = 0; k < 5; ++k) out[k] = (float)(m[k] / B);
}

// label content out of range (*err raised by the scan or the reduce kernel): no silent garbage, every reported value is NaN
__device__ __forceinline__ void poison_on_error(const int *err, float *losses, int n) {
    if (*err) {
        for (int k = 0; k < n; ++k) losses[k] = __builtin_nanf("");
    }
}

}  // namespace cdnet
