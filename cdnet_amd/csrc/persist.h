// Device-side scaffolding of the wave-specialised persistent kernels (conv_ws_kernel, conv_ws16_kernel, conv_ws32_kernel,
// wgrad_ws32_kernel) - the counterpart of launch.h: a workgroup's run of tiles, the tile cursor, the halo validity masks, requests
// through buffer descriptors, the movers' hand-written barriers, the weight-chunk LDS-DMA.  Plain functions of values: what a kernel
// keeps in flight (register sets, ring slots, out image, planes) stays in the kernel.
// Every helper here leaves the device code of every instantiation as it was with the text in place (profiles/persist_header); the pieces
// that did not - the halo offsets of a tile, chunk -> source, the scale / shift table fill, the 16-bit commit transform, the consumers'
// tile advance - are still written out in each kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "conv_args.h"
#include "vec.h"

namespace cdnet {

// ---- run of tiles -------------------------------------------------------------------------------------------------------------------
// Workgroup b of G takes the contiguous run [t_lo, t_hi) of T tiles.  When G is a multiple of 8, XCD k (workgroups k, k + 8, ...) serves
// the k-th eighth of the tiles, split evenly among its G / 8 workgroups: neighbouring tiles - shared halos - meet in one L2.
__host__ __device__ __forceinline__ void tile_run(int T, int G, int b, int &t_lo, int &t_hi) {
    if ((G & 7) == 0) {
        const int xcd = b & 7, idx = b >> 3, nw = G >> 3;
        const long long x0 = (long long)T * xcd / 8, x1 = (long long)T * (xcd + 1) / 8;
        t_lo = (int)(x0 + (x1 - x0) * idx / nw);
        t_hi = (int)(x0 + (x1 - x0) * (idx + 1) / nw);
    } else {
        t_lo = (int)((long long)T * b / G);
        t_hi = (int)((long long)T * (b + 1) / G);
    }
}

// ---- tile cursor (16 x 16-pixel tiles, image-major, then rows, then columns) ----------------------------------------------------------
// tile index -> image, first row, first column
__host__ __device__ __forceinline__ void seek_tile(int t, int tiles_img, int tiles_x, int &n, int &y0, int &x0) {
    n = t / tiles_img;
    const int r = t - n * tiles_img, ty = r / tiles_x;
    y0 = ty * 16; x0 = (r - ty * tiles_x) * 16;
}
// ... and the tile after it, without a division
__host__ __device__ __forceinline__ void next_tile(int &n, int &y0, int &x0, int H, int W) {
    x0 += 16;
    if (x0 >= W) { x0 = 0; y0 += 16; if (y0 >= H) { y0 = 0; ++n; } }
}

// ---- requests through buffer descriptors -----------------------------------------------------------------------------------------------
// One descriptor per tensor (below 2 GB: in_mover_reach, launch.h).  A vector outside the image / the source window carries bit 31 in
// its byte offset and the range check returns zeros for it - no select, no 64-bit address arithmetic and, for plain sources, no mask
// per vector: every vector instruction of a mover wave costs the consumers' MFMA stream issue time.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void *p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
template <typename T>
__device__ __forceinline__ T buf_load128(__amdgpu_buffer_rsrc_t r, unsigned voff) {
    return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, 0));
}

// ---- halo geometry --------------------------------------------------------------------------------------------------------------------
// bits [lo, hi) clear, everything else set (lo, hi clamped to [0, 31]): the invalid rows / columns of a tile's halo as a scalar mask
__host__ __device__ __forceinline__ unsigned halo_bad_mask(int lo, int hi) {
    lo = lo < 0 ? 0 : (lo > 31 ? 31 : lo);
    hi = hi < lo ? lo : (hi > 31 ? 31 : hi);
    return ~(((1u << hi) - 1u) & ~((1u << lo) - 1u));
}
// (halo row r <-> y = y0 - 1 + r, halo column c <-> x = x0 - 1 + c; valid = inside the image and the source window: two masks per tile
// and source, rowbad | colbad; per vector (rowbad >> row) | (colbad >> column), whose bit 0 becomes bit 31 of the request's byte offset)

// ---- the movers' barriers by hand ---------------------------------------------------------------------------------------------------
// s_waitcnt's immediate on gfx9: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] << 14; a field at its maximum (7, 15, 63) waits
// for nothing.  vmcnt(N) waits until only the N youngest vector-memory operations of the wave are outstanding (they retire in order).
//
// Why not __syncthreads(): it carries a workgroup release fence, and with an LDS-DMA in the wave's history the compiler turns that fence
// into s_waitcnt vmcnt(0) - draining the halo requests in flight every interval.  What the consumers need from a mover wave is: its LDS
// writes done (lgkmcnt(0)), its weight DMA landed (everything older than the N youngest vector-memory operations - the halo requests
// and stores issued AFTER the DMA, which stay in flight), then the barrier.  The compiler fences keep the LDS writes in front of it.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {               // vmcnt(N) alone
    __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (15 << 8) | ((N >> 4) << 14));
}
template <int N>
__device__ __forceinline__ void barrier_keep_vm() {          // lgkmcnt(0), vmcnt(N), s_barrier
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt((N & 15) | (7 << 4) | (0 << 8) | ((N >> 4) << 14));
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ void barrier_lds_only() {         // lgkmcnt(0), s_barrier: no wait for vector memory at all
    barrier_keep_vm<63>();
}

// ---- weight chunks by LDS-DMA -------------------------------------------------------------------------------------------------------
// A packed weight chunk is its own LDS image.  The 16-bit kernels: BYTES of it -> wdst, one 1 KB wave-instruction per 64 vectors, the
// four mover waves (pw) take them in turn.
template <int BYTES>
__device__ __forceinline__ void dma_weight_chunk(const unsigned short *wsrc, unsigned char *wdst, int pw, int lane) {
    constexpr int NVEC = BYTES / 16;
    static_assert(NVEC % 64 == 0, "whole wave-instructions");
#pragma unroll
    for (int i = 0; i < (NVEC / 64 + 3) / 4; ++i) {
        const int v0 = (i * 4 + pw) * 64;
        if (v0 < NVEC)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(wsrc + (size_t)(v0 + lane) * 8),
                                             (__attribute__((address_space(3))) void *)(wdst + v0 * 16), 16, 0, 0);
    }
}
// One LDS-DMA piece (64 lanes x 16 bytes = 1 KB): global (uniform base + this lane's byte offset) -> LDS (uniform byte address + lane * 16).
// Inline assembly on purpose: the compiler does not count it, so (a) it puts no alias guard - s_waitcnt vmcnt(<everything up to the
// DMA>) - in front of this wave's later LDS accesses, which lets the weight DMA of an interval be issued FIRST and land while the halo
// chunk is transformed and written, and (b) the wave waits for it itself: barrier_keep_vm counts the vector-memory operations issued
// after it.  M0 (the DMA's LDS base) is saved and restored around the piece.
__device__ __forceinline__ void glds_piece(const void *gbase, unsigned lane_bytes, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_bytes), "s"(gbase), "s"(lds_dst) : "memory");
}

}  // namespace cdnet
