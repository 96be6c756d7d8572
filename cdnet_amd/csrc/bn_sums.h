// The per-channel fp64 sum of BatchNorm's [T][2][C] tile partials (bn_finalize_train_kernel of model.hip, bn_bwd_finalize_kernel of
// bn_bwd.hip, bn_bwd_final_kernel of dilated_train.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace cdnet {

// s = sum_t part[t][0][c], q = sum_t part[t][1][c], in every thread of a 256-thread workgroup that calls it as a whole: thread i adds
// rows i, i + 256, ... in order, then a fixed 256-wide LDS tree - the same bits on every run.  One workgroup per channel keeps every CU
// busy; the 4-byte reads of different channels share cache lines in L2.
__device__ __forceinline__ void bn_sum_partials(const float *__restrict__ part, int T, int C, int c, double &s, double &q) {
    __shared__ double s_s[256], s_q[256];
    const int lane = threadIdx.x;
    s = 0.0; q = 0.0;
    for (int t = lane; t < T; t += 256) {
        s += (double)part[((size_t)t * 2) * C + c];
        q += (double)part[((size_t)t * 2 + 1) * C + c];
    }
    s_s[lane] = s; s_q[lane] = q;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (lane < o) { s_s[lane] += s_s[lane + o]; s_q[lane] += s_q[lane + o]; }
        __syncthreads();
    }
    s = s_s[0]; q = s_q[0];
}

}  // namespace cdnet
