// FullNet training kernels next to the dilated convolution (include/cdnet_hip.h, "FullNet training"), gfx950, fp32 precision mode.
//
// Replaces what autograd derives for models/FullNet.py:14-52 in train(): the weight gradient of a dilated ConvLayer, the batch-statistics
// BatchNorm behind the LeakyReLU with the dense layers' dropout (forward into a channel slice, backward out of one) and the dropout mask.
// The backward-data kernel is the forward kernel on swapped roles and lives in dilated.hip.
//
// Weight gradient: dW[co][ci][tap] = sum_pixels g[pixel][co] * x[pixel + tap shift][ci] is a GEMM whose K runs over pixels while both
// operands are pixel-major in memory.  A workgroup owns one 32-wide tile of Cout, four 32-wide tiles of Cin (one per wave) and a slab of
// 32-pixel row strips.  Per strip it stages g [32 pixels][32 co] once and, per tap, every wave its own shifted x [32 pixels][32 ci] through
// LDS with 16-byte loads, and reads both K-major: lane (channel, half h) takes pixels 16 s + 8 h + [0, 8) of MFMA step s.  A staged pixel
// row is 36 floats: consecutive lanes read consecutive banks and the two halves' rows, 8 apart, lie 32 banks apart - no conflict.
// Both operands are activations: each is split into bf16 hi / lo after the LDS read, three MFMAs per product (split8, mfma3: split_bf16.h).
// A tap that no pixel of the strip reaches is skipped (no load, no MFMA).  Every slab stores its [taps][Cout tiles][Cin tiles] sums; a
// second launch adds the slabs in order - no atomics, the same bits on every run.
#include "common.h"
#include "bn_sums.h"
#include "launch.h"
#include "split_bf16.h"

using namespace cdnet;

namespace {

constexpr int STRIP = 32;            // pixels of a strip (two MFMA K steps of 16)
constexpr int ROW = 36;              // floats of a staged pixel row in LDS (32 channels + 4: see above)
constexpr int WG_WAVES = 4;          // Cin tiles of a workgroup
constexpr int WGRAD_WGS = 512;       // workgroups a launch aims at (two per CU)

// four channels c .. c + 3 of a pixel (channels >= cend selected to zero), or zero when !ok
__device__ __forceinline__ f32x4 load4(const float *p, bool ok, int c, int cend) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ok && c < cend) {
        v = *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c + j < cend ? v[j] : 0.f;
    }
    return v;
}

// the K-major fragment of MFMA step s: pixels 16 s + 8 h + [0, 8) of channel i
__device__ __forceinline__ void frag(const float *tile, int s, int h, int i, u32x4 &hi, u32x4 &lo) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tile[(16 * s + 8 * h + k) * ROW + i];
    split8(v, hi, lo);
}

struct WgradGeom { int nslab, strips_per_slab, nstrips, tiles_x, CoP, CiP; };

WgradGeom wgrad_geom(int N, int H, int W, int Cin, int Cout) {
    WgradGeom G;
    G.tiles_x = cdiv(W, STRIP);
    const long long nstrips = (long long)N * H * G.tiles_x;
    G.nstrips = (int)nstrips;
    const int tiles = cdiv(Cout, 32) * cdiv(cdiv(Cin, 32), WG_WAVES);
    long long nslab = WGRAD_WGS / tiles;
    if (nslab < 1) nslab = 1;
    if (nslab > nstrips) nslab = nstrips;
    G.strips_per_slab = (int)((nstrips + nslab - 1) / nslab);
    G.nslab = (int)((nstrips + G.strips_per_slab - 1) / G.strips_per_slab);
    G.CoP = cdiv(Cout, 32) * 32;
    G.CiP = cdiv(Cin, 32) * 32;
    return G;
}

// grid: x = slab, y = group of four Cin tiles, z = Cout tile
template <int TAPS>
__global__ __launch_bounds__(WG_WAVES * 64) void dilated_wgrad_kernel(const cdnet_dilated_wgrad_args A, const WgradGeom G) {
    __shared__ __attribute__((aligned(16))) float s_g[STRIP * ROW];
    __shared__ __attribute__((aligned(16))) float s_x[WG_WAVES][STRIP * ROW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    const int co0 = blockIdx.z * 32, ci0 = ((int)blockIdx.y * WG_WAVES + wave) * 32;
    const bool live = ci0 < A.Cin;                                    // (wave-uniform; a dead wave still takes every barrier)
    float *sx = s_x[wave];

    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int q0 = blockIdx.x * G.strips_per_slab;
    const int q1 = q0 + G.strips_per_slab < G.nstrips ? q0 + G.strips_per_slab : G.nstrips;
    for (int q = q0; q < q1; ++q) {
        const int x0 = (q % G.tiles_x) * STRIP, row = q / G.tiles_x, y = row % A.H, n = row / A.H;
        __syncthreads();                                              // the previous strip's fragments are read
        {
            const int pp = tid >> 3, c = co0 + (tid & 7) * 4;
            const bool ok = x0 + pp < A.W;
            const size_t off = (((size_t)n * A.H + y) * A.W + (size_t)(ok ? x0 + pp : 0)) * (size_t)A.g_cstride + (size_t)(c < A.Cout ? c : 0);
            *reinterpret_cast<f32x4 *>(&s_g[pp * ROW + (tid & 7) * 4]) = load4(A.g + off, ok, c, A.Cout);
        }
        __syncthreads();
        u32x4 ah[2], al[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) frag(s_g, s, h, i, ah[s], al[s]);
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
            const long long dy = TAPS == 9 ? (long long)(tap / 3 - 1) * A.dilation : 0;
            const long long dx = TAPS == 9 ? (long long)(tap % 3 - 1) * A.dilation : 0;
            const long long yy = y + dy;
            // pixels of the strip whose g and shifted x both lie inside the image (uniform over the workgroup)
            long long lo = -(x0 + dx), hi = (long long)A.W - 1 - x0 - dx;
            if (lo < 0) lo = 0;
            if (hi > A.W - 1 - x0) hi = A.W - 1 - x0;
            if (hi > STRIP - 1) hi = STRIP - 1;
            if (yy < 0 || yy >= A.H || lo > hi) continue;             // no pixel of the strip reaches this tap
            if (live) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int idx = lane + 64 * k, pp = idx >> 3, c = ci0 + (idx & 7) * 4;
                    const long long px = x0 + pp + dx;
                    const bool ok = pp >= lo && pp <= hi;
                    const size_t off = (((size_t)n * A.H + (size_t)yy) * A.W + (size_t)(ok ? px : 0)) * (size_t)A.x_cstride + (size_t)(c < A.Cin ? c : 0);
                    *reinterpret_cast<f32x4 *>(&sx[pp * ROW + (idx & 7) * 4]) = load4(A.x + off, ok, c, A.Cin);
                }
            }
            __syncthreads();                                          // (the wave's own tile: the barrier orders its lanes' writes and reads)
            if (live) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    u32x4 bh, bl;
                    frag(sx, s, h, i, bh, bl);
                    const bf16x8 a_hi = __builtin_bit_cast(bf16x8, ah[s]), a_lo = __builtin_bit_cast(bf16x8, al[s]);
                    const bf16x8 b_hi = __builtin_bit_cast(bf16x8, bh), b_lo = __builtin_bit_cast(bf16x8, bl);
                    acc[tap] = mfma3(acc[tap], a_hi, a_lo, b_hi, b_lo);
                }
            }
        }
    }
    if (!live) return;
    // lane (i, h) owns input channel ci0 + i and the output channels co0 + (r & 3) + 8 (r >> 2) + 4 h
    float *slab = static_cast<float *>(A.ws) + (size_t)blockIdx.x * TAPS * G.CoP * G.CiP;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            slab[((size_t)tap * G.CoP + co) * G.CiP + ci0 + i] = acc[tap][r];
        }
}

// dw[co][ci][tap] = the slabs' sums in slab order
__global__ __launch_bounds__(256) void dilated_wgrad_reduce_kernel(const float *ws, float *dw, int Cin, int Cout, int taps, const WgradGeom G) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)Cout * Cin * taps;
    if (e >= total) return;
    const int tap = (int)(e % taps), ci = (int)((e / taps) % Cin), co = (int)(e / taps / Cin);
    const size_t per = (size_t)taps * G.CoP * G.CiP;
    const float *p = ws + ((size_t)tap * G.CoP + co) * G.CiP + ci;
    float s = 0.f;
    for (int k = 0; k < G.nslab; ++k) s += p[(size_t)k * per];
    dw[e] = s;
}

// ------------------------------------------------------------------------------------------------------
// dropout: a counter-based hash of (key, layer, element index) - splitmix64's finaliser, twice
__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ unsigned long long layer_key(unsigned long long key, int layer) {
    return mix64(key + 0x9E3779B97F4A7C15ull * (unsigned long long)(unsigned)(layer + 1));
}

__host__ __device__ __forceinline__ unsigned drop_threshold(float p) { return (unsigned)(p * 16777216.0f); }

// true: element `idx` is kept
__device__ __forceinline__ bool keep(unsigned long long lkey, unsigned long long idx, unsigned thr) {
    return (unsigned)(mix64(lkey + 0x9E3779B97F4A7C15ull * (idx + 1)) >> 40) >= thr;
}

__global__ __launch_bounds__(256) void dropout_mask_kernel(unsigned long long lkey, size_t count, unsigned thr, uint8_t *mask) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        mask[i] = keep(lkey, i, thr) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------
// BatchNorm over a compact z [P][zs] with the result in / the gradient from a channel slice.
// Tile sums: a workgroup owns a tile of pixels and 32 channels; thread (channel, row r of 8) adds its pixels r, r + 8, ... in order, the
// eight rows are added in order.  [T][2][C] partials, reduced by a fixed fp64 tree (cdnet_bn_finalize_train / bn_bwd_final_kernel).
constexpr int BN_TILES = 1024;

struct BnGeom { int T; long long tile; };

BnGeom bn_geom(long long P) {
    BnGeom G;
    long long T = (P + 63) / 64;
    if (T > BN_TILES) T = BN_TILES;
    G.tile = (P + T - 1) / T;
    G.T = (int)((P + G.tile - 1) / G.tile);
    return G;
}

// BWD false: sums of z and z^2; true: sums of dyh and dyh * xhat
template <bool BWD>
__global__ __launch_bounds__(256) void bn_tile_sums_kernel(const float *__restrict__ z, int zs, const float *__restrict__ dy, int dys, int dyo,
                                                           const float *__restrict__ mean, const float *__restrict__ invstd, long long P, int C,
                                                           long long tile, unsigned long long lkey, unsigned thr, float keep_scale,
                                                           float *__restrict__ part) {
    __shared__ float s_a[8][32], s_b[8][32];
    const int cl = threadIdx.x & 31, r = threadIdx.x >> 5, c = blockIdx.y * 32 + cl;
    const long long p0 = (long long)blockIdx.x * tile, p1 = p0 + tile < P ? p0 + tile : P;
    float a = 0.f, b = 0.f;
    if (c < C) {
        const float mu = BWD ? mean[c] : 0.f, is = BWD ? invstd[c] : 0.f;
        for (long long p = p0 + r; p < p1; p += 8) {
            const float v = z[(size_t)p * zs + c];
            if constexpr (BWD) {
                float d = dy[(size_t)p * dys + dyo + c];
                if (thr) d = keep(lkey, (unsigned long long)p * C + c, thr) ? d * keep_scale : 0.f;
                a += d;
                b += d * ((v - mu) * is);
            } else {
                a += v;
                b += v * v;
            }
        }
    }
    s_a[r][cl] = a;
    s_b[r][cl] = b;
    __syncthreads();
    if (r == 0 && c < C) {
#pragma unroll
        for (int k = 1; k < 8; ++k) { a += s_a[k][cl]; b += s_b[k][cl]; }
        part[((size_t)blockIdx.x * 2) * C + c] = a;
        part[((size_t)blockIdx.x * 2 + 1) * C + c] = b;
    }
}

// one workgroup per channel: the fixed-order fp64 sums of bn_sums.h
__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const float *__restrict__ part, int T, int C, float *dgamma, float *dbeta) {
    const int c = blockIdx.x;
    double s, q;
    bn_sum_partials(part, T, C, c, s, q);
    if (threadIdx.x == 0) {
        dbeta[c] = (float)s;
        dgamma[c] = (float)q;
    }
}

// out[p][coff + c] = (z scale + shift) m / (1 - p_drop)
__global__ __launch_bounds__(256) void bn_fwd_apply_kernel(const float *__restrict__ z, int zs, const float *__restrict__ scale,
                                                           const float *__restrict__ shift, size_t total, int C, unsigned long long lkey,
                                                           unsigned thr, float keep_scale, float *__restrict__ out, int os, int oo) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const size_t p = e / C;
        float v = z[p * zs + c] * scale[c] + shift[c];
        if (thr) v = keep(lkey, e, thr) ? v * keep_scale : 0.f;
        out[p * os + oo + c] = v;
    }
}

// g[p][c] = gamma invstd (dyh - dbeta / P - xhat dgamma / P) * (z > 0 ? 1 : slope)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float *__restrict__ z, int zs, const float *__restrict__ dy, int dys, int dyo,
                                                           const float *__restrict__ mean, const float *__restrict__ invstd,
                                                           const float *__restrict__ gamma, const float *__restrict__ dgamma,
                                                           const float *__restrict__ dbeta, size_t total, int C, float inv_count, float slope,
                                                           unsigned long long lkey, unsigned thr, float keep_scale, float *__restrict__ g, int gs) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const size_t p = e / C;
        const float v = z[p * zs + c];
        float d = dy[p * dys + dyo + c];
        if (thr) d = keep(lkey, e, thr) ? d * keep_scale : 0.f;
        const float xhat = (v - mean[c]) * invstd[c];
        const float dz = gamma[c] * invstd[c] * (d - dbeta[c] * inv_count - xhat * (dgamma[c] * inv_count));
        g[p * gs + c] = v > 0.f ? dz : slope * dz;
    }
}

}  // namespace

extern "C" size_t cdnet_dilated_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int taps) {
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (taps != 1 && taps != 9)) return 0;
    if ((long long)N * H * cdiv(W, STRIP) >= (1ll << 31)) return 0;
    const WgradGeom G = wgrad_geom(N, H, W, Cin, Cout);
    return (size_t)G.nslab * taps * G.CoP * G.CiP * sizeof(float);
}

extern "C" int cdnet_dilated_conv_backward_weight(const cdnet_dilated_wgrad_args *args, void *stream) {
    CDNET_REQUIRE(args, "cdnet_dilated_conv_backward_weight: null args");
    const cdnet_dilated_wgrad_args &A = *args;
    CDNET_REQUIRE(A.x && A.g && A.dw && A.ws, "cdnet_dilated_conv_backward_weight: null x / g / dw / ws");
    CDNET_REQUIRE(A.taps == 1 || A.taps == 9, "cdnet_dilated_conv_backward_weight: taps %d (1 or 9)", A.taps);
    CDNET_REQUIRE(A.dilation >= 1, "cdnet_dilated_conv_backward_weight: dilation %d < 1", A.dilation);
    CDNET_REQUIRE(A.N >= 1 && A.H >= 1 && A.W >= 1 && A.Cin >= 1 && A.Cout >= 1,
                  "cdnet_dilated_conv_backward_weight: N %d H %d W %d Cin %d Cout %d must be positive", A.N, A.H, A.W, A.Cin, A.Cout);
    CDNET_REQUIRE(A.x_cstride >= A.Cin && A.x_cstride % 8 == 0,
                  "cdnet_dilated_conv_backward_weight: x_cstride %d must be a multiple of 8 and >= Cin %d", A.x_cstride, A.Cin);
    CDNET_REQUIRE(A.g_cstride >= A.Cout && A.g_cstride % 8 == 0,
                  "cdnet_dilated_conv_backward_weight: g_cstride %d must be a multiple of 8 and >= Cout %d", A.g_cstride, A.Cout);
    CDNET_REQUIRE((long long)A.N * A.H * cdiv(A.W, STRIP) < (1ll << 31), "cdnet_dilated_conv_backward_weight: image too large");
    const size_t need = cdnet_dilated_wgrad_workspace_bytes(A.N, A.H, A.W, A.Cin, A.Cout, A.taps);
    CDNET_REQUIRE(A.ws_bytes >= need, "cdnet_dilated_conv_backward_weight: workspace of %zu bytes, %zu needed", A.ws_bytes, need);
    const WgradGeom G = wgrad_geom(A.N, A.H, A.W, A.Cin, A.Cout);
    const dim3 grid((unsigned)G.nslab, (unsigned)cdiv(cdiv(A.Cin, 32), WG_WAVES), (unsigned)cdiv(A.Cout, 32));
    if (A.taps == 9) dilated_wgrad_kernel<9><<<grid, WG_WAVES * 64, 0, (hipStream_t)stream>>>(A, G);
    else dilated_wgrad_kernel<1><<<grid, WG_WAVES * 64, 0, (hipStream_t)stream>>>(A, G);
    const size_t total = (size_t)A.Cout * A.Cin * A.taps;
    dilated_wgrad_reduce_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(static_cast<const float *>(A.ws), A.dw, A.Cin,
                                                                                               A.Cout, A.taps, G);
    return check_launch("cdnet_dilated_conv_backward_weight");
}

extern "C" int cdnet_dropout_mask(unsigned long long key, int layer, size_t count, float p_drop, uint8_t *mask, void *stream) {
    CDNET_REQUIRE(mask, "cdnet_dropout_mask: null mask");
    CDNET_REQUIRE(count >= 1, "cdnet_dropout_mask: count must be positive");
    CDNET_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "cdnet_dropout_mask: p_drop %g outside [0, 1)", (double)p_drop);
    CDNET_REQUIRE(layer >= 0, "cdnet_dropout_mask: layer %d < 0", layer);
    dropout_mask_kernel<<<lin_grid(count, 8192), 256, 0, (hipStream_t)stream>>>(layer_key(key, layer), count, drop_threshold(p_drop), mask);
    return check_launch("cdnet_dropout_mask");
}

extern "C" size_t cdnet_slice_bn_workspace_floats(long long P, int C) {
    if (P < 1 || C < 1) return 0;
    return (size_t)bn_geom(P).T * 2 * C + 2 * (size_t)C;
}

extern "C" int cdnet_slice_bn_train_forward(const cdnet_slice_bn_fwd_args *args, void *stream) {
    CDNET_REQUIRE(args, "cdnet_slice_bn_train_forward: null args");
    const cdnet_slice_bn_fwd_args &A = *args;
    CDNET_REQUIRE(A.z && A.out && A.gamma && A.beta && A.mean && A.invstd && A.ws, "cdnet_slice_bn_train_forward: null pointer");
    CDNET_REQUIRE((A.running_mean == nullptr) == (A.running_var == nullptr), "cdnet_slice_bn_train_forward: one running statistic without the other");
    CDNET_REQUIRE(A.P >= 1 && A.C >= 1, "cdnet_slice_bn_train_forward: P %lld, C %d must be positive", A.P, A.C);
    CDNET_REQUIRE(A.z_cstride >= A.C, "cdnet_slice_bn_train_forward: z_cstride %d < C %d", A.z_cstride, A.C);
    CDNET_REQUIRE(A.out_coff >= 0 && (long long)A.out_coff + A.C <= A.out_cstride,
                  "cdnet_slice_bn_train_forward: out_coff %d + C %d exceeds out_cstride %d", A.out_coff, A.C, A.out_cstride);
    CDNET_REQUIRE((const void *)A.z != (const void *)A.out, "cdnet_slice_bn_train_forward: out must not be z");
    CDNET_REQUIRE(A.p_drop >= 0.f && A.p_drop < 1.f, "cdnet_slice_bn_train_forward: p_drop %g outside [0, 1)", (double)A.p_drop);
    CDNET_REQUIRE(A.layer >= 0, "cdnet_slice_bn_train_forward: layer %d < 0", A.layer);
    CDNET_REQUIRE(A.ws_floats >= cdnet_slice_bn_workspace_floats(A.P, A.C), "cdnet_slice_bn_train_forward: workspace of %zu floats, %zu needed",
                  A.ws_floats, cdnet_slice_bn_workspace_floats(A.P, A.C));
    const BnGeom G = bn_geom(A.P);
    hipStream_t st = (hipStream_t)stream;
    float *part = A.ws, *scale = A.ws + (size_t)G.T * 2 * A.C, *shift = scale + A.C;
    const unsigned long long lkey = layer_key(A.key, A.layer);
    const unsigned thr = drop_threshold(A.p_drop);
    const float ks = 1.f / (1.f - A.p_drop);
    bn_tile_sums_kernel<false><<<dim3((unsigned)G.T, (unsigned)cdiv(A.C, 32)), 256, 0, st>>>(A.z, A.z_cstride, nullptr, 0, 0, nullptr, nullptr, A.P,
                                                                                            A.C, G.tile, lkey, thr, ks, part);
    int rc = check_launch("cdnet_slice_bn_train_forward");
    if (rc) return rc;
    rc = cdnet_bn_finalize_train(part, G.T, A.C, (float)A.P, A.gamma, A.beta, nullptr, A.eps, A.momentum, A.running_mean, A.running_var, scale,
                                 shift, A.mean, A.invstd, stream);
    if (rc) return rc;
    const size_t total = (size_t)A.P * A.C;
    bn_fwd_apply_kernel<<<lin_grid(total, 8192), 256, 0, st>>>(A.z, A.z_cstride, scale, shift, total, A.C, lkey, thr, ks, A.out, A.out_cstride,
                                                          A.out_coff);
    return check_launch("cdnet_slice_bn_train_forward");
}

extern "C" int cdnet_slice_bn_train_backward(const cdnet_slice_bn_bwd_args *args, void *stream) {
    CDNET_REQUIRE(args, "cdnet_slice_bn_train_backward: null args");
    const cdnet_slice_bn_bwd_args &A = *args;
    CDNET_REQUIRE(A.dy && A.z && A.mean && A.invstd && A.gamma && A.dgamma && A.dbeta && A.g && A.ws, "cdnet_slice_bn_train_backward: null pointer");
    CDNET_REQUIRE(A.P >= 1 && A.C >= 1, "cdnet_slice_bn_train_backward: P %lld, C %d must be positive", A.P, A.C);
    CDNET_REQUIRE(A.z_cstride >= A.C, "cdnet_slice_bn_train_backward: z_cstride %d < C %d", A.z_cstride, A.C);
    CDNET_REQUIRE(A.g_cstride >= A.C, "cdnet_slice_bn_train_backward: g_cstride %d < C %d", A.g_cstride, A.C);
    CDNET_REQUIRE(A.dy_coff >= 0 && (long long)A.dy_coff + A.C <= A.dy_cstride,
                  "cdnet_slice_bn_train_backward: dy_coff %d + C %d exceeds dy_cstride %d", A.dy_coff, A.C, A.dy_cstride);
    CDNET_REQUIRE((const void *)A.g != (const void *)A.dy && (const void *)A.g != (const void *)A.z, "cdnet_slice_bn_train_backward: g must not be dy or z");
    CDNET_REQUIRE(A.p_drop >= 0.f && A.p_drop < 1.f, "cdnet_slice_bn_train_backward: p_drop %g outside [0, 1)", (double)A.p_drop);
    CDNET_REQUIRE(A.layer >= 0, "cdnet_slice_bn_train_backward: layer %d < 0", A.layer);
    CDNET_REQUIRE(A.ws_floats >= cdnet_slice_bn_workspace_floats(A.P, A.C), "cdnet_slice_bn_train_backward: workspace of %zu floats, %zu needed",
                  A.ws_floats, cdnet_slice_bn_workspace_floats(A.P, A.C));
    const BnGeom G = bn_geom(A.P);
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long lkey = layer_key(A.key, A.layer);
    const unsigned thr = drop_threshold(A.p_drop);
    const float ks = 1.f / (1.f - A.p_drop);
    bn_tile_sums_kernel<true><<<dim3((unsigned)G.T, (unsigned)cdiv(A.C, 32)), 256, 0, st>>>(A.z, A.z_cstride, A.dy, A.dy_cstride, A.dy_coff, A.mean,
                                                                                           A.invstd, A.P, A.C, G.tile, lkey, thr, ks, A.ws);
    bn_bwd_final_kernel<<<A.C, 256, 0, st>>>(A.ws, G.T, A.C, A.dgamma, A.dbeta);
    const size_t total = (size_t)A.P * A.C;
    bn_bwd_apply_kernel<<<lin_grid(total, 8192), 256, 0, st>>>(A.z, A.z_cstride, A.dy, A.dy_cstride, A.dy_coff, A.mean, A.invstd, A.gamma, A.dgamma,
                                                          A.dbeta, total, A.C, 1.f / (float)A.P, A.slope, lkey, thr, ks, A.g, A.g_cstride);
    return check_launch("cdnet_slice_bn_train_backward");
}
