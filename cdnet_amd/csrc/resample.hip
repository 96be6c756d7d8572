// FCN_pooling's two resampling steps (reference models/FullNet.py:169-172: nn.MaxPool2d(2, 2) behind trans1..trans4,
// nn.UpsamplingBilinear2d(scale_factor=4) behind trans5 and trans6), forward and backward, on NHWC tensors of which one side is a channel
// slice of a dense block's buffer.  Streaming kernels: one thread per (pixel of the smaller map's grid, group of V channels), V channels =
// 16 bytes where strides, offsets and base addresses allow it (4 fp32 / 8 bf16), else V = 1; the last, partial group of a vector launch is
// handled channel by channel.  No atomics, every output element is written by one thread in a fixed order of operations.
#include "common.h"
#include "launch.h"

using namespace cdnet;

namespace {

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
    T v[V];
};

__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(__bf16 v) { return (float)v; }

// ATen's max_pool2d rule (the one boundary.hip follows): the running maximum starts at the window's first element and is replaced by a
// later one that is greater or NaN, so `k` is the first maximum in raster order
template <typename T>
__device__ __forceinline__ void take(T v, int pos, T &m, int &k) {
    const float fv = to_f(v), fm = to_f(m);
    if (fv > fm || fv != fv) { m = v; k = pos; }
}

// item -> (pixel, first channel of the group); G groups per pixel
struct Item {
    unsigned pix;
    int c0;
};
__device__ __forceinline__ Item item_of(unsigned item, unsigned G, int V) {
    Item it;
    it.pix = item / G;
    it.c0 = (int)(item - it.pix * G) * V;
    return it;
}

template <typename T, int V, bool IDX>
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const T *__restrict__ x, int xs, T *__restrict__ y, int ys, int yoff,
                                                           uint8_t *__restrict__ idx, int is, int Ho, int Wo, int C, unsigned G, unsigned total) {
    const unsigned stride = gridDim.x * 256u;
    const size_t row = (size_t)2 * Wo * xs;                                  // one input row
    for (unsigned item = blockIdx.x * 256u + threadIdx.x; item < total; item += stride) {
        const Item it = item_of(item, G, V);
        const unsigned wo = it.pix % Wo, nh = it.pix / Wo;                   // nh = n * Ho + ho: input row 2 nh
        const T *a = x + ((size_t)nh * 2 * (2 * Wo) + 2 * wo) * xs + it.c0;
        T *o = y + (size_t)it.pix * ys + yoff + it.c0;
        uint8_t *ib = IDX ? idx + (size_t)it.pix * is + it.c0 : nullptr;
        if (it.c0 + V <= C) {
            const Pack<T, V> p0 = *reinterpret_cast<const Pack<T, V> *>(a), p1 = *reinterpret_cast<const Pack<T, V> *>(a + xs);
            const Pack<T, V> p2 = *reinterpret_cast<const Pack<T, V> *>(a + row), p3 = *reinterpret_cast<const Pack<T, V> *>(a + row + xs);
            Pack<T, V> m;
            Pack<uint8_t, V> kk;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                T mv = p0.v[j];
                int k = 0;
                take(p1.v[j], 1, mv, k);
                take(p2.v[j], 2, mv, k);
                take(p3.v[j], 3, mv, k);
                m.v[j] = mv;
                kk.v[j] = (uint8_t)k;
            }
            *reinterpret_cast<Pack<T, V> *>(o) = m;
            if (IDX) *reinterpret_cast<Pack<uint8_t, V> *>(ib) = kk;
        } else {
            for (int j = 0; it.c0 + j < C; ++j) {
                T mv = a[j];
                int k = 0;
                take(a[xs + j], 1, mv, k);
                take(a[row + j], 2, mv, k);
                take(a[row + xs + j], 3, mv, k);
                o[j] = mv;
                if (IDX) ib[j] = (uint8_t)k;
            }
        }
    }
}

template <int V>
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float *__restrict__ dy, int dys, int dyoff, const uint8_t *__restrict__ idx, int is,
                                                           float *__restrict__ dx, int dxs, int Ho, int Wo, int C, unsigned G, unsigned total) {
    const unsigned stride = gridDim.x * 256u;
    const size_t row = (size_t)2 * Wo * dxs;
    for (unsigned item = blockIdx.x * 256u + threadIdx.x; item < total; item += stride) {
        const Item it = item_of(item, G, V);
        const unsigned wo = it.pix % Wo, nh = it.pix / Wo;
        const float *g = dy + (size_t)it.pix * dys + dyoff + it.c0;
        const uint8_t *ib = idx + (size_t)it.pix * is + it.c0;
        float *o = dx + ((size_t)nh * 2 * (2 * Wo) + 2 * wo) * dxs + it.c0;
        if (it.c0 + V <= C) {
            const Pack<float, V> gv = *reinterpret_cast<const Pack<float, V> *>(g);
            const Pack<uint8_t, V> kk = *reinterpret_cast<const Pack<uint8_t, V> *>(ib);
            Pack<float, V> q[4];
#pragma unroll
            for (int j = 0; j < V; ++j)
#pragma unroll
                for (int pos = 0; pos < 4; ++pos) q[pos].v[j] = kk.v[j] == pos ? gv.v[j] : 0.f;
            *reinterpret_cast<Pack<float, V> *>(o) = q[0];
            *reinterpret_cast<Pack<float, V> *>(o + dxs) = q[1];
            *reinterpret_cast<Pack<float, V> *>(o + row) = q[2];
            *reinterpret_cast<Pack<float, V> *>(o + row + dxs) = q[3];
        } else {
            for (int j = 0; it.c0 + j < C; ++j) {
                const float gv = g[j];
                const int k = ib[j];
                o[j] = k == 0 ? gv : 0.f;
                o[dxs + j] = k == 1 ? gv : 0.f;
                o[row + j] = k == 2 ? gv : 0.f;
                o[row + dxs + j] = k == 3 ? gv : 0.f;
            }
        }
    }
}

// align_corners=True source coordinate of output index o on an axis of `src` -> `dst` = 4 src samples, in integers: q = o (src - 1),
// i0 = q / (dst - 1), lambda = float(q % (dst - 1)) / float(dst - 1) (a correctly rounded quotient), i1 = min(i0 + 1, src - 1)
struct Coord {
    int i0, i1;
    float l1, l0;                                                            // weights of i1 and of i0 (l0 = 1 - l1)
};
__device__ __forceinline__ Coord coord_of(int o, int src, int dst) {
    const int q = o * (src - 1), d = dst - 1;
    Coord c;
    c.i0 = q / d;
    c.i1 = c.i0 + 1 < src ? c.i0 + 1 : src - 1;
    c.l1 = (float)(q - c.i0 * d) / (float)d;
    c.l0 = 1.f - c.l1;
    return c;
}

__device__ __forceinline__ float lerp2(float x00, float x01, float x10, float x11, const Coord &ch, const Coord &cw) {
    const float top = x00 * cw.l0 + x01 * cw.l1, bot = x10 * cw.l0 + x11 * cw.l1;
    return top * ch.l0 + bot * ch.l1;
}

template <typename T, int V>
__global__ __launch_bounds__(256) void upsample4_fwd_kernel(const T *__restrict__ x, int xs, T *__restrict__ y, int ys, int yoff, int Hs, int Ws,
                                                            int C, unsigned G, unsigned total) {
    const unsigned stride = gridDim.x * 256u;
    const unsigned H = 4u * Hs, W = 4u * Ws;
    for (unsigned item = blockIdx.x * 256u + threadIdx.x; item < total; item += stride) {
        const Item it = item_of(item, G, V);
        const unsigned w = it.pix % W, nh = it.pix / W, h = nh % H, n = nh / H;
        const Coord ch = coord_of((int)h, Hs, (int)H), cw = coord_of((int)w, Ws, (int)W);
        const T *base = x + (size_t)n * Hs * Ws * xs + it.c0;
        const T *a00 = base + ((size_t)ch.i0 * Ws + cw.i0) * xs, *a01 = base + ((size_t)ch.i0 * Ws + cw.i1) * xs;
        const T *a10 = base + ((size_t)ch.i1 * Ws + cw.i0) * xs, *a11 = base + ((size_t)ch.i1 * Ws + cw.i1) * xs;
        T *o = y + (size_t)it.pix * ys + yoff + it.c0;
        if (it.c0 + V <= C) {
            const Pack<T, V> p00 = *reinterpret_cast<const Pack<T, V> *>(a00), p01 = *reinterpret_cast<const Pack<T, V> *>(a01);
            const Pack<T, V> p10 = *reinterpret_cast<const Pack<T, V> *>(a10), p11 = *reinterpret_cast<const Pack<T, V> *>(a11);
            Pack<T, V> r;
#pragma unroll
            for (int j = 0; j < V; ++j) r.v[j] = (T)lerp2(to_f(p00.v[j]), to_f(p01.v[j]), to_f(p10.v[j]), to_f(p11.v[j]), ch, cw);
            *reinterpret_cast<Pack<T, V> *>(o) = r;
        } else {
            for (int j = 0; it.c0 + j < C; ++j) o[j] = (T)lerp2(to_f(a00[j]), to_f(a01[j]), to_f(a10[j]), to_f(a11[j]), ch, cw);
        }
    }
}

// first and last output index whose source coordinate lies within one source step of `s` (a superset: an index at distance exactly one
// gets weight 0 from weight_of)
__device__ __forceinline__ void reach(int s, int src, int dst, int &lo, int &hi) {
    if (src == 1) { lo = 0; hi = dst - 1; return; }
    const int d = dst - 1, m = src - 1;
    lo = s > 0 ? ((s - 1) * d) / m : 0;
    hi = ((s + 1) * d + m - 1) / m;
    if (hi > d) hi = d;
}
// the forward's weight of source index s in output index o (0 when o does not read s)
__device__ __forceinline__ float weight_of(int o, int s, int src, int dst) {
    const Coord c = coord_of(o, src, dst);
    float wt = 0.f;
    if (c.i0 == s) wt = c.l0;
    if (c.i1 == s && c.i1 != c.i0) wt = c.l1;
    return wt;
}

template <int V>
__global__ __launch_bounds__(256) void upsample4_bwd_kernel(const float *__restrict__ dy, int dys, int dyoff, float *__restrict__ dx, int dxs,
                                                            int Hs, int Ws, int C, unsigned G, unsigned total) {
    const unsigned stride = gridDim.x * 256u;
    const int H = 4 * Hs, W = 4 * Ws;
    for (unsigned item = blockIdx.x * 256u + threadIdx.x; item < total; item += stride) {
        const Item it = item_of(item, G, V);
        const unsigned ws = it.pix % Ws, nh = it.pix / Ws, hs = nh % Hs, n = nh / Hs;
        int hlo, hhi, wlo, whi;
        reach((int)hs, Hs, H, hlo, hhi);
        reach((int)ws, Ws, W, wlo, whi);
        const float *base = dy + (size_t)n * H * W * dys + dyoff + it.c0;
        float *o = dx + (size_t)it.pix * dxs + it.c0;
        const bool vec = it.c0 + V <= C;
        const int nc = vec ? V : C - it.c0;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
        for (int h = hlo; h <= hhi; ++h) {                                   // ascending (h, w): the fixed summation order
            const float wy = weight_of(h, (int)hs, Hs, H);
            if (wy == 0.f) continue;
            for (int w = wlo; w <= whi; ++w) {
                const float wx = weight_of(w, (int)ws, Ws, W);
                if (wx == 0.f) continue;
                const float wt = wy * wx;
                const float *g = base + ((size_t)h * W + w) * dys;
                if (vec) {
                    const Pack<float, V> gv = *reinterpret_cast<const Pack<float, V> *>(g);
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] = acc[j] + wt * gv.v[j];
                } else {
                    for (int j = 0; j < nc; ++j) acc[j] = acc[j] + wt * g[j];
                }
            }
        }
        if (vec) {
            Pack<float, V> r;
#pragma unroll
            for (int j = 0; j < V; ++j) r.v[j] = acc[j];
            *reinterpret_cast<Pack<float, V> *>(o) = r;
        } else {
            for (int j = 0; j < nc; ++j) o[j] = acc[j];
        }
    }
}

inline bool aligned(const void *p, size_t a) { return ((size_t)p & (a - 1)) == 0; }

// a * b of non-negative counts, saturating at 2^62
inline long long mul_sat(long long a, long long b) { return b != 0 && a > (1ll << 62) / b ? 1ll << 62 : a * b; }

// items of a launch (pixels x channel groups), or 0 when they exceed the kernels' 32-bit item index
inline unsigned items_of(long long pixels, int C, int V, unsigned *G) {
    *G = (unsigned)((C + V - 1) / V);
    const long long t = mul_sat(pixels, *G);
    return t < (1ll << 31) ? (unsigned)t : 0u;
}

constexpr long long MAX_ELEMS = 1ll << 40;                                   // elements of the largest tensor (the offsets are 64-bit)

}  // namespace

#define RESAMPLE_SHAPE(name, N, H, W, C)                                                                                  \
    CDNET_REQUIRE((N) >= 1 && (H) >= 1 && (W) >= 1 && (C) >= 1, name ": N %d, H %d, W %d, C %d must be positive", N, H, W, C)

extern "C" int cdnet_maxpool2_forward(const void *x, int x_cstride, void *y, int y_cstride, int y_coff, uint8_t *idx, int idx_cstride, int N, int H,
                                      int W, int C, int f32, void *stream) {
    CDNET_REQUIRE(x && y, "cdnet_maxpool2_forward: null pointer");
    RESAMPLE_SHAPE("cdnet_maxpool2_forward", N, H, W, C);
    CDNET_REQUIRE(H % 2 == 0 && W % 2 == 0, "cdnet_maxpool2_forward: H %d and W %d must be even", H, W);
    CDNET_REQUIRE(x_cstride >= C, "cdnet_maxpool2_forward: x_cstride %d < C %d", x_cstride, C);
    CDNET_REQUIRE(y_coff >= 0 && (long long)y_coff + C <= y_cstride, "cdnet_maxpool2_forward: y_coff %d + C %d exceeds y_cstride %d", y_coff, C,
                  y_cstride);
    CDNET_REQUIRE(!idx || idx_cstride >= C, "cdnet_maxpool2_forward: idx_cstride %d < C %d", idx_cstride, C);
    CDNET_REQUIRE(x != y, "cdnet_maxpool2_forward: y must not be x");
    const long long pixels = mul_sat(mul_sat(N, H / 2), W / 2);
    const int es = f32 ? 4 : 2, VV = 16 / es;
    const bool vec = x_cstride % VV == 0 && y_cstride % VV == 0 && y_coff % VV == 0 && aligned(x, 16) && aligned(y, 16) &&
                     (!idx || (idx_cstride % VV == 0 && aligned(idx, VV)));
    unsigned G;
    const unsigned total = items_of(pixels, C, vec ? VV : 1, &G);
    CDNET_REQUIRE(total && mul_sat(4 * pixels, x_cstride > y_cstride ? x_cstride : y_cstride) < MAX_ELEMS, "cdnet_maxpool2_forward: tensor too large");
    hipStream_t st = (hipStream_t)stream;
    const int grid = lin_grid(total, 8192);
    auto go = [&](auto t, auto v, auto wi) {
        using T = decltype(t);
        maxpool2_fwd_kernel<T, decltype(v)::value, decltype(wi)::value><<<grid, 256, 0, st>>>((const T *)x, x_cstride, (T *)y, y_cstride, y_coff, idx,
                                                                                              idx_cstride, H / 2, W / 2, C, G, total);
    };
    auto by_idx = [&](auto t, auto v) { idx ? go(t, v, std::true_type{}) : go(t, v, std::false_type{}); };
    if (f32) vec ? by_idx(float{}, std::integral_constant<int, 4>{}) : by_idx(float{}, std::integral_constant<int, 1>{});
    else vec ? by_idx(__bf16{}, std::integral_constant<int, 8>{}) : by_idx(__bf16{}, std::integral_constant<int, 1>{});
    return check_launch("cdnet_maxpool2_forward");
}

extern "C" int cdnet_maxpool2_backward(const float *dy, int dy_cstride, int dy_coff, const uint8_t *idx, int idx_cstride, float *dx, int dx_cstride,
                                       int N, int H, int W, int C, void *stream) {
    CDNET_REQUIRE(dy && idx && dx, "cdnet_maxpool2_backward: null pointer");
    RESAMPLE_SHAPE("cdnet_maxpool2_backward", N, H, W, C);
    CDNET_REQUIRE(H % 2 == 0 && W % 2 == 0, "cdnet_maxpool2_backward: H %d and W %d must be even", H, W);
    CDNET_REQUIRE(dx_cstride >= C, "cdnet_maxpool2_backward: dx_cstride %d < C %d", dx_cstride, C);
    CDNET_REQUIRE(dy_coff >= 0 && (long long)dy_coff + C <= dy_cstride, "cdnet_maxpool2_backward: dy_coff %d + C %d exceeds dy_cstride %d", dy_coff,
                  C, dy_cstride);
    CDNET_REQUIRE(idx_cstride >= C, "cdnet_maxpool2_backward: idx_cstride %d < C %d", idx_cstride, C);
    CDNET_REQUIRE(dx != dy, "cdnet_maxpool2_backward: dx must not be dy");
    const long long pixels = mul_sat(mul_sat(N, H / 2), W / 2);
    const bool vec = dx_cstride % 4 == 0 && dy_cstride % 4 == 0 && dy_coff % 4 == 0 && idx_cstride % 4 == 0 && aligned(dx, 16) && aligned(dy, 16) &&
                     aligned(idx, 4);
    unsigned G;
    const unsigned total = items_of(pixels, C, vec ? 4 : 1, &G);
    CDNET_REQUIRE(total && mul_sat(4 * pixels, dx_cstride > dy_cstride ? dx_cstride : dy_cstride) < MAX_ELEMS,
                  "cdnet_maxpool2_backward: tensor too large");
    hipStream_t st = (hipStream_t)stream;
    const int grid = lin_grid(total, 8192);
    if (vec) maxpool2_bwd_kernel<4><<<grid, 256, 0, st>>>(dy, dy_cstride, dy_coff, idx, idx_cstride, dx, dx_cstride, H / 2, W / 2, C, G, total);
    else maxpool2_bwd_kernel<1><<<grid, 256, 0, st>>>(dy, dy_cstride, dy_coff, idx, idx_cstride, dx, dx_cstride, H / 2, W / 2, C, G, total);
    return check_launch("cdnet_maxpool2_backward");
}

extern "C" int cdnet_upsample4_bilinear_forward(const void *x, int x_cstride, void *y, int y_cstride, int y_coff, int N, int Hs, int Ws, int C, int f32,
                                                void *stream) {
    CDNET_REQUIRE(x && y, "cdnet_upsample4_bilinear_forward: null pointer");
    RESAMPLE_SHAPE("cdnet_upsample4_bilinear_forward", N, Hs, Ws, C);
    CDNET_REQUIRE(Hs <= 8192 && Ws <= 8192, "cdnet_upsample4_bilinear_forward: Hs %d, Ws %d beyond 8192", Hs, Ws);
    CDNET_REQUIRE(x_cstride >= C, "cdnet_upsample4_bilinear_forward: x_cstride %d < C %d", x_cstride, C);
    CDNET_REQUIRE(y_coff >= 0 && (long long)y_coff + C <= y_cstride, "cdnet_upsample4_bilinear_forward: y_coff %d + C %d exceeds y_cstride %d", y_coff,
                  C, y_cstride);
    CDNET_REQUIRE(x != y, "cdnet_upsample4_bilinear_forward: y must not be x");
    const long long pixels = mul_sat(mul_sat(N, 4ll * Hs), 4ll * Ws);
    const int es = f32 ? 4 : 2, VV = 16 / es;
    const bool vec = x_cstride % VV == 0 && y_cstride % VV == 0 && y_coff % VV == 0 && aligned(x, 16) && aligned(y, 16);
    unsigned G;
    const unsigned total = items_of(pixels, C, vec ? VV : 1, &G);
    CDNET_REQUIRE(total && mul_sat(pixels, x_cstride > y_cstride ? x_cstride : y_cstride) < MAX_ELEMS, "cdnet_upsample4_bilinear_forward: tensor too large");
    hipStream_t st = (hipStream_t)stream;
    const int grid = lin_grid(total, 8192);
    auto go = [&](auto t, auto v) {
        using T = decltype(t);
        upsample4_fwd_kernel<T, decltype(v)::value><<<grid, 256, 0, st>>>((const T *)x, x_cstride, (T *)y, y_cstride, y_coff, Hs, Ws, C, G, total);
    };
    if (f32) vec ? go(float{}, std::integral_constant<int, 4>{}) : go(float{}, std::integral_constant<int, 1>{});
    else vec ? go(__bf16{}, std::integral_constant<int, 8>{}) : go(__bf16{}, std::integral_constant<int, 1>{});
    return check_launch("cdnet_upsample4_bilinear_forward");
}

extern "C" int cdnet_upsample4_bilinear_backward(const float *dy, int dy_cstride, int dy_coff, float *dx, int dx_cstride, int N, int Hs, int Ws, int C,
                                                 void *stream) {
    CDNET_REQUIRE(dy && dx, "cdnet_upsample4_bilinear_backward: null pointer");
    RESAMPLE_SHAPE("cdnet_upsample4_bilinear_backward", N, Hs, Ws, C);
    CDNET_REQUIRE(Hs <= 8192 && Ws <= 8192, "cdnet_upsample4_bilinear_backward: Hs %d, Ws %d beyond 8192", Hs, Ws);
    CDNET_REQUIRE(dx_cstride >= C, "cdnet_upsample4_bilinear_backward: dx_cstride %d < C %d", dx_cstride, C);
    CDNET_REQUIRE(dy_coff >= 0 && (long long)dy_coff + C <= dy_cstride, "cdnet_upsample4_bilinear_backward: dy_coff %d + C %d exceeds dy_cstride %d",
                  dy_coff, C, dy_cstride);
    CDNET_REQUIRE(dx != dy, "cdnet_upsample4_bilinear_backward: dx must not be dy");
    const long long pixels = mul_sat(mul_sat(N, Hs), Ws);
    const bool vec = dx_cstride % 4 == 0 && dy_cstride % 4 == 0 && dy_coff % 4 == 0 && aligned(dx, 16) && aligned(dy, 16);
    unsigned G;
    const unsigned total = items_of(pixels, C, vec ? 4 : 1, &G);
    CDNET_REQUIRE(total && mul_sat(16 * pixels, dx_cstride > dy_cstride ? dx_cstride : dy_cstride) < MAX_ELEMS,
                  "cdnet_upsample4_bilinear_backward: tensor too large");
    hipStream_t st = (hipStream_t)stream;
    const int grid = lin_grid(total, 8192);
    if (vec) upsample4_bwd_kernel<4><<<grid, 256, 0, st>>>(dy, dy_cstride, dy_coff, dx, dx_cstride, Hs, Ws, C, G, total);
    else upsample4_bwd_kernel<1><<<grid, 256, 0, st>>>(dy, dy_cstride, dy_coff, dx, dx_cstride, Hs, Ws, C, G, total);
    return check_launch("cdnet_upsample4_bilinear_backward");
}
