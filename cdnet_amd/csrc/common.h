// Shared host-side helpers for the C ABI (error reporting, launch checks).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/cdnet_hip.h"

namespace cdnet {

void set_error(const char *fmt, ...);

inline int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return CDNET_E_LAUNCH;
    }
    return CDNET_OK;
}

#define CDNET_REQUIRE(cond, ...)                \
    do {                                        \
        if (!(cond)) {                          \
            cdnet::set_error(__VA_ARGS__);      \
            return CDNET_E_ARG;                 \
        }                                       \
    } while (0)

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

constexpr int WAVE = 64;

// Softmax of the K mask logits of one pixel with cdnet_probmaps' arithmetic (test_dam.py:984, test.py:634 F.softmax): fmaxf maximum,
// expf(a - max), sum from left to right, divide.  K == 1: 1 wherever the logit is finite (NaN otherwise) - what a one-channel softmax is.
// Shared by the mask-only kernels of postproc.hip and postproc_tile.hip so that their probabilities are bit-identical.
template <int K>
__device__ __forceinline__ void mask_softmax(const float *a, float *p) {
    float mx = a[0];
    if constexpr (K == 3) mx = fmaxf(a[0], fmaxf(a[1], a[2]));         // (probmaps_kernel's expression)
    else {
#pragma unroll
        for (int c = 1; c < K; ++c) mx = fmaxf(mx, a[c]);
    }
    float e[K];
#pragma unroll
    for (int c = 0; c < K; ++c) e[c] = expf(a[c] - mx);
    float s = e[0];
#pragma unroll
    for (int c = 1; c < K; ++c) s = s + e[c];
#pragma unroll
    for (int c = 0; c < K; ++c) p[c] = e[c] / s;
}

// Class of one pixel from its (mean) probabilities: K = 2 / 3 np.argmax (first maximum; the first NaN wins), K = 1 `prob >= 0.5`
// (test.py:270-275).  Foreground is class 1 in every case.
template <int K>
__device__ __forceinline__ int mask_class(const float *m) {
    if constexpr (K == 1) return m[0] >= 0.5f ? 1 : 0;
    int a = 0;
    float mx = m[0];
#pragma unroll
    for (int c = 1; c < K; ++c)
        if (m[c] > mx || (m[c] != m[c] && mx == mx)) { a = c; mx = m[c]; }
    return a;
}

// postproc.hip: 8-connected labelling with raster-order ids (shared with the CDM generator)
int label8_raster(const uint8_t *mask, int N, int H, int W, int *L, int *aux, int *chunk, int32_t *labels, int32_t *counts,
                  hipStream_t st);
// postproc_tile.hip: the same labelling of tiles (W % 64 == 0, at most 65 536 pixels) in one launch; false: shape not served, nothing queued
bool label8_tile(const uint8_t *mask, int N, int H, int W, int32_t *labels, int32_t *counts, hipStream_t st, int *rc);

}  // namespace cdnet
