// Device helpers shared by the backward streaming kernels (head_bwd.hip, bn_bwd.hip): fp32 8-channel loads / stores, the
// threads-per-pixel block layout and the fixed-order sum of per-block partial rows.  The 16-bit formats come from stage16.h.
#pragma once
#include "common.h"
#include "stage16.h"

namespace cdnet {

static __device__ __forceinline__ void ldf8(const void *base, size_t e, float *v) {
    const float4 *p = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(base) + e);
    const float4 a = p[0], b = p[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
static __device__ __forceinline__ void stf8(void *base, size_t e, const float *v) {
    float4 *p = reinterpret_cast<float4 *>(reinterpret_cast<float *>(base) + e);
    p[0] = make_float4(v[0], v[1], v[2], v[3]);
    p[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// first pixel (or pool window) of a thread in the "VPP threads per pixel, 256 / VPP pixels per block" layouts; when VPP does
// not divide 256 (HRNet's 48 / 80 / 144 channels) the left-over threads of the block sit the loop out
static __device__ __forceinline__ unsigned first_pixel(unsigned ppb, int VPP) {
    return (int)threadIdx.x < (int)ppb * VPP ? blockIdx.x * ppb + threadIdx.x / VPP : 0xffffffffu;
}

// out[k] = sum_b partial[b][k]: one wave per output, lanes stride over b, fixed butterfly -> deterministic
static __global__ __launch_bounds__(256) void reduce_partials_kernel(const float *__restrict__ partial, int nb, int K, float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    float s = 0.f;
    for (int b = lane; b < nb; b += 64) s += partial[(size_t)b * K + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[k] = s;
}

}  // namespace cdnet
