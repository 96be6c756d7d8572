// Connected components on the device: union-find over pixel indices, roots = smallest (raster-first) index of a component.
// One wave = 64 consecutive pixels of one row: the row runs come from a ballot, so only run heads talk to
// the forest.  Block (64,4); grid (ceil(W/64), ceil(H/4), N).  L: int32 per pixel, -1 = not in the mask.
// Shared by postproc.hip (cdnet_cc_chain, label8_raster, the watershed chain) and variance.hip (cdnet_variance_loss).  Everything
// sits in an unnamed namespace on purpose: every including file gets kernels of its own, as with the kernels it defines itself.
#pragma once
#include "common.h"

namespace cdnet {
namespace {

__device__ __forceinline__ int ld_relaxed(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int uf_find(const int *L, int a) {
    int p = ld_relaxed(L + a);
    while (p != a) { a = p; p = ld_relaxed(L + a); }
    return a;
}

__device__ __forceinline__ void uf_union(int *L, int a, int b) {
    bool done;
    do {
        a = uf_find(L, a);
        b = uf_find(L, b);
        if (a < b) { int old = atomicMin(L + b, a); done = (old == b); b = old; }
        else if (b < a) { int old = atomicMin(L + a, b); done = (old == a); a = old; }
        else done = true;
    } while (!done);
}

// index of the first lane of the run of set bits that contains `lane`
__device__ __forceinline__ int run_start(unsigned long long m, int lane) {
    unsigned long long zeros_below = ~m & ((1ull << lane) - 1ull);
    return zeros_below ? 64 - __clzll(zeros_below) : 0;
}
// number of set bits in the run starting at `lane` (lane is a run head)
__device__ __forceinline__ int run_length(unsigned long long m, int lane) {
    unsigned long long z = ~(m >> lane);          // first zero above
    return z ? __ffsll((long long)z) - 1 : 64 - lane;
}

// MODE 0: mask = (src != fgval)  [background of pred_inside, for fill-holes]; MODE 1: mask = (src != 0); MODE 2: mask = (src == fgval)
template <int MODE>
__device__ __forceinline__ bool in_mask(uint8_t v, int fgval) { return MODE == 0 ? (v != fgval) : MODE == 1 ? (v != 0) : (v == fgval); }

template <int MODE>
__global__ __launch_bounds__(256) void cc_init_kernel(const uint8_t *__restrict__ src, int fgval, int H, int W,
                                                      int *__restrict__ L) {
    const int n = blockIdx.z;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const size_t base = (size_t)n * H * W;
    const bool valid = x < W && y < H;
    const bool fg = valid && in_mask<MODE>(src[base + (size_t)y * W + x], fgval);
    const unsigned long long b = __ballot(fg);
    if (valid) L[base + (size_t)y * W + x] = fg ? (y * W + blockIdx.x * 64 + run_start(b, threadIdx.x)) : -1;
}

// CONN: 4 or 8.  Unions between a row run and the runs of the row above, plus the stitch to the left segment.
template <int MODE, int CONN>
__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t *__restrict__ src, int fgval, int H, int W,
                                                       int *L) {
    const int n = blockIdx.z;
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * 64, x = x0 + lane, y = blockIdx.y * 4 + threadIdx.y;
    if (y >= H) return;                                   // whole wave exits together (y is wave-uniform)
    const size_t base = (size_t)n * H * W;
    const uint8_t *m = src + base;
    int *Ln = L + base;
    const bool valid = x < W;
    const bool fg = valid && in_mask<MODE>(m[(size_t)y * W + x], fgval);
    const bool up = valid && y > 0 && in_mask<MODE>(m[(size_t)(y - 1) * W + x], fgval);
    // edge pixels outside this 64-segment
    bool left_edge = false, upleft_edge = false, upright_edge = false;
    if (lane == 0 && x0 > 0) {
        left_edge = in_mask<MODE>(m[(size_t)y * W + x0 - 1], fgval);
        if (y > 0) upleft_edge = in_mask<MODE>(m[(size_t)(y - 1) * W + x0 - 1], fgval);
    }
    if (lane == 63 && x0 + 64 < W && y > 0) upright_edge = in_mask<MODE>(m[(size_t)(y - 1) * W + x0 + 64], fgval);
    const unsigned long long bf = __ballot(fg), bu = __ballot(up);
    if (!fg) return;
    const bool left = lane > 0 ? ((bf >> (lane - 1)) & 1ull) : left_edge;
    const bool a = lane > 0 ? ((bu >> (lane - 1)) & 1ull) : upleft_edge;      // NW
    const bool b = (bu >> lane) & 1ull;                                        // N
    const bool c = lane < 63 ? ((bu >> (lane + 1)) & 1ull) : upright_edge;    // NE
    const int p = y * W + x;
    if (lane == 0 && left_edge) uf_union(Ln, p, p - 1);
    if (CONN == 4) {
        if (b && !(left && a)) uf_union(Ln, p, p - W);
    } else {
        if (b) { if (!left) uf_union(Ln, p, p - W); }
        else {
            if (a && !left) uf_union(Ln, p, p - W - 1);
            if (c) uf_union(Ln, p, p - W + 1);
        }
    }
}

// L[p] <- root(p).  FLAT_AREA: additionally aux[n][root] += run length (one atomic per row run); FLAT_COUNT: aux[n] += the number of
// roots (= components of image n; one integer atomic per wave that holds a root).
enum { FLAT_PLAIN = 0, FLAT_AREA = 1, FLAT_COUNT = 2 };
template <int EXTRA>
__global__ __launch_bounds__(256) void cc_flatten_kernel(int H, int W, int *L, int *aux) {
    const int n = blockIdx.z;
    const int lane = threadIdx.x;
    const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + threadIdx.y;
    const size_t base = (size_t)n * H * W;
    int *Ln = L + base;
    const bool valid = x < W && y < H;
    int r = -1;
    if (valid) {
        int l = Ln[(size_t)y * W + x];
        if (l >= 0) { r = uf_find(Ln, l); }
    }
    const unsigned long long bf = __ballot(r >= 0);
    if (EXTRA == FLAT_COUNT) {
        const unsigned long long roots = __ballot(r >= 0 && r == y * W + x);
        if (roots && lane == 0) atomicAdd(aux + n, __popcll(roots));
    }
    if (r >= 0) {
        Ln[(size_t)y * W + x] = r;
        if (EXTRA == FLAT_AREA) {
            bool head = lane == 0 || !((bf >> (lane - 1)) & 1ull);
            if (head) atomicAdd(aux + base + r, run_length(bf, lane));
        }
    }
}

inline dim3 grid_rows(int N, int H, int W) { return dim3(cdiv(W, 64), cdiv(H, 4), N); }

}  // namespace
}  // namespace cdnet
