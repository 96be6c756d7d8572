// Pillow's 8-bit bilinear resampler on the device: Image.resize((ow, oh), Image.BILINEAR) of mode L / RGB images, bit for bit
// (the 'scale' test transform, my_transforms_direction.py:38-65, and misc.imresize(pred2 * 255, (ori_h, ori_w), 'bilinear') of
// test.py:281-283 / test_dam.py:551-553).  gfx950 only.
//
// The coefficient tables are the caller's (cdnet_amd/resize.py, float64 in Pillow's operation order): per output index of an axis
// bounds = (first source index, number of taps) and ksize 22-bit fixed-point weights.  A pass is
//   clip8((2^21 + sum_x src[lo + x] * kk[x]) >> 22)        int32 sum, as ImagingResampleHorizontal_8bpc / Vertical_8bpc hold it.
// The horizontal pass runs first (only when ow != W) and is rounded to u8 before the vertical pass (only when oh != H) reads it.
//
// Two forms of the two-axis resize:
//   form 1 (LDS): one launch.  A workgroup owns a TH x TW tile of the output, runs the horizontal pass of the source rows its tile rows
//           read into LDS as u8 and the vertical pass from there; the intermediate image never reaches memory.
//   form 2 (two-pass): horizontal pass to a u8 intermediate in the workspace, then the vertical pass.  Taken when the source rows of a
//           tile exceed the LDS budget (the taps of a row grow with H / oh) and when one axis alone changes (then one launch, no workspace).
// Mask mode (C = 1): the input is {0, 1}, read as v * 255 by the first pass that runs; the last one writes (value > 127.5) as {0, 1}.
// Every load and store is a byte: no pointer or row needs more than byte alignment.  Table entries are clamped to the image before they
// index anything, so a wrong table gives a wrong picture, never an access outside the buffers.
#include <math.h>
#include "common.h"
#include "launch.h"

using namespace cdnet;

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Pillow's Resample.c
constexpr int TH = 16, TW = 64;                 // output tile of the LDS form
constexpr int LDS_BUDGET = 65536;               // bytes of dynamic LDS a workgroup may ask for without an opt-in

__device__ __forceinline__ uint8_t clip8(int ss) {
    const int v = ss >> PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

template <bool MASK_IN>
__device__ __forceinline__ int pixel(uint8_t v) {
    if constexpr (MASK_IN) return (int)(uint8_t)(v * 255);
    return (int)v;
}

template <bool MASK_OUT>
__device__ __forceinline__ uint8_t result(uint8_t v) {
    if constexpr (MASK_OUT) return v > 127 ? 1 : 0;         // (v > 127.5 of an integer)
    return v;
}

// (first source index, taps) of output index i, clamped to [0, in) and to the table's row
__device__ __forceinline__ void span(const int32_t *__restrict__ bounds, int i, int in, int ksize, int *lo, int *n) {
    int l = bounds[2 * i], c = bounds[2 * i + 1];
    l = l < 0 ? 0 : (l > in - 1 ? in - 1 : l);
    const int most = ksize < in - l ? ksize : in - l;
    *lo = l;
    *n = c < 0 ? 0 : (c > most ? most : c);
}

// horizontal pass: src [rows][W][C] -> out [rows][ow][C]; one thread per output byte, rows over blockIdx.y
template <int C, bool MASK_IN, bool MASK_OUT>
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t *__restrict__ src, size_t rows, int W, int ow,
                                                       const int32_t *__restrict__ hb, const int32_t *__restrict__ hk, int ks,
                                                       uint8_t *__restrict__ out) {
    const int xb = blockIdx.x * 256 + threadIdx.x;
    if (xb >= ow * C) return;
    const int xx = xb / C, c = xb - xx * C;
    int lo, n;
    span(hb, xx, W, ks, &lo, &n);
    const int32_t *k = hk + (size_t)xx * ks;
    for (size_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const uint8_t *p = src + r * ((size_t)W * C) + (size_t)lo * C + c;
        int ss = 1 << (PRECISION_BITS - 1);
        for (int x = 0; x < n; ++x) ss += pixel<MASK_IN>(p[x * C]) * k[x];
        out[r * ((size_t)ow * C) + xb] = result<MASK_OUT>(clip8(ss));
    }
}

// vertical pass: src [N][H][rowb] -> out [N][oh][rowb]; one thread per output byte, output rows over blockIdx.y, images over blockIdx.z
template <bool MASK_IN, bool MASK_OUT>
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t *__restrict__ src, int H, int rowb, int oh,
                                                       const int32_t *__restrict__ vb, const int32_t *__restrict__ vk, int ks,
                                                       uint8_t *__restrict__ out) {
    const int xb = blockIdx.x * 256 + threadIdx.x;
    if (xb >= rowb) return;
    const uint8_t *s = src + (size_t)blockIdx.z * H * rowb + xb;
    uint8_t *o = out + (size_t)blockIdx.z * oh * rowb + xb;
    for (int yy = blockIdx.y; yy < oh; yy += gridDim.y) {
        int lo, n;
        span(vb, yy, H, ks, &lo, &n);
        const int32_t *k = vk + (size_t)yy * ks;
        const uint8_t *p = s + (size_t)lo * rowb;
        int ss = 1 << (PRECISION_BITS - 1);
        for (int y = 0; y < n; ++y) ss += pixel<MASK_IN>(p[(size_t)y * rowb]) * k[y];
        o[(size_t)yy * rowb] = result<MASK_OUT>(clip8(ss));
    }
}

// LDS form: both passes of one TH x TW output tile; `cap` = rows of TW * C bytes the launch reserved
template <int C, bool MASK>
__global__ __launch_bounds__(256) void resize_lds_kernel(const uint8_t *__restrict__ src, int H, int W, int oh, int ow,
                                                         const int32_t *__restrict__ hb, const int32_t *__restrict__ hk, int hks,
                                                         const int32_t *__restrict__ vb, const int32_t *__restrict__ vk, int vks,
                                                         int cap, uint8_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tile[];
    constexpr int PITCH = TW * C;
    const int y0 = blockIdx.y * TH, x0 = blockIdx.x * TW;
    const int y1 = y0 + TH < oh ? y0 + TH : oh, x1 = x0 + TW < ow ? x0 + TW : ow;
    const int twb = (x1 - x0) * C;
    // the spans of the tile's rows are nested between the first row's start and the last row's end (both grow with the row)
    int r0, nf, rl, nl;
    span(vb, y0, H, vks, &r0, &nf);
    span(vb, y1 - 1, H, vks, &rl, &nl);
    int nrows = rl + nl - r0;
    nrows = nrows < 0 ? 0 : (nrows > cap ? cap : nrows);
    const uint8_t *img = src + (size_t)blockIdx.z * H * W * C;
    for (int i = threadIdx.x; i < nrows * PITCH; i += 256) {
        const int r = i / PITCH, xb = i - r * PITCH;
        if (xb >= twb) continue;
        const int px = xb / C, c = xb - px * C;
        int lo, n;
        span(hb, x0 + px, W, hks, &lo, &n);
        const int32_t *k = hk + (size_t)(x0 + px) * hks;
        const uint8_t *p = img + (size_t)(r0 + r) * W * C + (size_t)lo * C + c;
        int ss = 1 << (PRECISION_BITS - 1);
        for (int x = 0; x < n; ++x) ss += pixel<MASK>(p[x * C]) * k[x];
        tile[i] = clip8(ss);
    }
    __syncthreads();
    uint8_t *o = out + ((size_t)blockIdx.z * oh + y0) * ow * C + (size_t)x0 * C;
    for (int i = threadIdx.x; i < (y1 - y0) * PITCH; i += 256) {
        const int ty = i / PITCH, xb = i - ty * PITCH;
        if (xb >= twb) continue;
        int lo, n;
        span(vb, y0 + ty, H, vks, &lo, &n);
        lo -= r0;
        lo = lo < 0 ? 0 : lo;
        n = n < nrows - lo ? n : nrows - lo;
        const int32_t *k = vk + (size_t)(y0 + ty) * vks;
        const unsigned char *p = tile + lo * PITCH + xb;
        int ss = 1 << (PRECISION_BITS - 1);
        for (int y = 0; y < n; ++y) ss += (int)p[y * PITCH] * k[y];
        o[(size_t)ty * ow * C + xb] = result<MASK>(clip8(ss));
    }
}

// ksize of an axis as Pillow's precompute_coeffs sets it: support = max(in / out, 1) for the bilinear filter
int axis_ksize(int in, int out) {
    const double scale = (double)in / (double)out;
    const double support = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(support) * 2 + 1;
}

// Upper bound of the source rows one tile reads.  With c = (yy + 0.5) * scale and s = support, a row starts above c - s - 0.5 and ends
// at most at c + s + 0.5, so TH consecutive rows span fewer than (TH - 1) * scale + 2 s + 1 source rows; one more for the floating
// point, never more than the image has.
int tile_rows_cap(int H, int oh) {
    const double scale = (double)H / (double)oh;
    const double support = scale < 1.0 ? 1.0 : scale;
    const double bound = ceil((TH - 1) * scale + 2.0 * support + 1.0) + 1.0;
    return bound > (double)H ? H : (int)bound;
}

thread_local int g_resize_last_form = 0;

constexpr int MAX_EDGE = 1 << 20, MAX_IMAGES = 65535;

// the form a request resolves to: 0 = copy (no axis changes), 1, 2; -1 with the error set
int resolve_form(int H, int W, int C, int oh, int ow, int form) {
    const bool nh = ow != W, nv = oh != H;
    if (!nh && !nv) return 0;
    const long long lds = (long long)tile_rows_cap(H, oh) * TW * C;
    if (form == 1) {
        if (lds > LDS_BUDGET) {
            set_error("cdnet_resize_bilinear: form 1: the source rows of a %d-row tile need %lld bytes of LDS, the budget is %d (use form 0 or 2)", TH, lds, LDS_BUDGET);
            return -1;
        }
        if (!(nh && nv)) {
            set_error("cdnet_resize_bilinear: form 1: only one axis changes, there is nothing to fuse (use form 0 or 2)");
            return -1;
        }
        return 1;
    }
    if (form == 2) return 2;
    return nh && nv && lds <= LDS_BUDGET ? 1 : 2;
}

bool sizes_ok(int N, int H, int W, int C, int oh, int ow) {
    return N >= 1 && N <= MAX_IMAGES && H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && H <= MAX_EDGE && W <= MAX_EDGE && oh <= MAX_EDGE &&
           ow <= MAX_EDGE && (C == 1 || C == 3);
}

}  // namespace

extern "C" size_t cdnet_resize_workspace_bytes(int N, int H, int W, int C, int oh, int ow, int form) {
    if (!sizes_ok(N, H, W, C, oh, ow) || form < 0 || form > 2) return 0;
    if (ow == W || oh == H) return 0;
    if (form != 2 && (long long)tile_rows_cap(H, oh) * TW * C <= LDS_BUDGET) return 0;
    return (size_t)N * H * ow * C;
}

extern "C" int cdnet_resize_last_form(void) { return g_resize_last_form; }

extern "C" int cdnet_resize_bilinear(const uint8_t *src, int N, int H, int W, int C, int oh, int ow, const int32_t *hbounds,
                                     const int32_t *hkk, int hksize, const int32_t *vbounds, const int32_t *vkk, int vksize, int mask_mode,
                                     int form, void *workspace, size_t workspace_bytes, uint8_t *out, void *stream) {
    CDNET_REQUIRE(src && out, "cdnet_resize_bilinear: null pointer");
    CDNET_REQUIRE(N >= 1 && N <= MAX_IMAGES && H >= 1 && W >= 1 && oh >= 1 && ow >= 1,
                  "cdnet_resize_bilinear: bad size N=%d H=%d W=%d oh=%d ow=%d (every size >= 1, N <= %d)", N, H, W, oh, ow, MAX_IMAGES);
    CDNET_REQUIRE(H <= MAX_EDGE && W <= MAX_EDGE && oh <= MAX_EDGE && ow <= MAX_EDGE, "cdnet_resize_bilinear: an edge is longer than %d", MAX_EDGE);
    CDNET_REQUIRE(C == 1 || C == 3, "cdnet_resize_bilinear: C=%d not in {1, 3} (mode L or RGB)", C);
    CDNET_REQUIRE(mask_mode == 0 || (mask_mode == 1 && C == 1), "cdnet_resize_bilinear: mask_mode=%d (0, or 1 with C = 1)", mask_mode);
    CDNET_REQUIRE(form >= 0 && form <= 2, "cdnet_resize_bilinear: form=%d not in {0, 1, 2}", form);
    const bool nh = ow != W, nv = oh != H;
    if (nh) {
        CDNET_REQUIRE(hbounds && hkk, "cdnet_resize_bilinear: null pointer (horizontal tables)");
        CDNET_REQUIRE(hksize == axis_ksize(W, ow), "cdnet_resize_bilinear: hksize=%d, but %d -> %d columns have ksize %d", hksize, W, ow, axis_ksize(W, ow));
    }
    if (nv) {
        CDNET_REQUIRE(vbounds && vkk, "cdnet_resize_bilinear: null pointer (vertical tables)");
        CDNET_REQUIRE(vksize == axis_ksize(H, oh), "cdnet_resize_bilinear: vksize=%d, but %d -> %d rows have ksize %d", vksize, H, oh, axis_ksize(H, oh));
    }
    const size_t in_bytes = (size_t)N * H * W * C, out_bytes = (size_t)N * oh * ow * C;
    CDNET_REQUIRE(out + out_bytes <= src || src + in_bytes <= out, "cdnet_resize_bilinear: out overlaps src");
    const int f = resolve_form(H, W, C, oh, ow, form);
    if (f < 0) return CDNET_E_ARG;
    const size_t mid_bytes = (size_t)N * H * ow * C;
    if (f == 2 && nh && nv) {
        CDNET_REQUIRE(workspace, "cdnet_resize_bilinear: null pointer (workspace of the two-pass form)");
        if (workspace_bytes < mid_bytes) {
            set_error("cdnet_resize_bilinear: workspace %zu < %zu bytes", workspace_bytes, mid_bytes);
            return CDNET_E_WORKSPACE;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (f == 0) {                                            // Image.resize to the same size is a copy
        (void)hipMemcpyAsync(out, src, in_bytes, hipMemcpyDeviceToDevice, st);
        rc = check_launch("cdnet_resize_bilinear(copy)");
        if (rc == CDNET_OK) g_resize_last_form = 0;
        return rc;
    }
    const bool mask = mask_mode == 1;
    if (f == 1) {
        const int cap = tile_rows_cap(H, oh);
        const dim3 grid(cdiv(ow, TW), cdiv(oh, TH), N);
        const int smem = cap * TW * C;
        if (C == 3) resize_lds_kernel<3, false><<<grid, 256, smem, st>>>(src, H, W, oh, ow, hbounds, hkk, hksize, vbounds, vkk, vksize, cap, out);
        else if (mask) resize_lds_kernel<1, true><<<grid, 256, smem, st>>>(src, H, W, oh, ow, hbounds, hkk, hksize, vbounds, vkk, vksize, cap, out);
        else resize_lds_kernel<1, false><<<grid, 256, smem, st>>>(src, H, W, oh, ow, hbounds, hkk, hksize, vbounds, vkk, vksize, cap, out);
        rc = check_launch("cdnet_resize_bilinear(lds)");
        if (rc == CDNET_OK) g_resize_last_form = 1;
        return rc;
    }
    const uint8_t *vsrc = src;
    if (nh) {
        uint8_t *hout = nv ? (uint8_t *)workspace : out;
        const size_t rows = (size_t)N * H;
        const dim3 grid(cdiv(ow * C, 256), (unsigned)(rows < 65535 ? rows : 65535));
        const bool mo = mask && !nv;
        if (C == 3) resize_h_kernel<3, false, false><<<grid, 256, 0, st>>>(src, rows, W, ow, hbounds, hkk, hksize, hout);
        else if (mask && mo) resize_h_kernel<1, true, true><<<grid, 256, 0, st>>>(src, rows, W, ow, hbounds, hkk, hksize, hout);
        else if (mask) resize_h_kernel<1, true, false><<<grid, 256, 0, st>>>(src, rows, W, ow, hbounds, hkk, hksize, hout);
        else resize_h_kernel<1, false, false><<<grid, 256, 0, st>>>(src, rows, W, ow, hbounds, hkk, hksize, hout);
        vsrc = hout;
    }
    if (nv) {
        const int rowb = ow * C;
        const dim3 grid(cdiv(rowb, 256), oh < 65535 ? oh : 65535, N);
        const bool mi = mask && !nh;
        if (mask && mi) resize_v_kernel<true, true><<<grid, 256, 0, st>>>(vsrc, H, rowb, oh, vbounds, vkk, vksize, out);
        else if (mask) resize_v_kernel<false, true><<<grid, 256, 0, st>>>(vsrc, H, rowb, oh, vbounds, vkk, vksize, out);
        else resize_v_kernel<false, false><<<grid, 256, 0, st>>>(vsrc, H, rowb, oh, vbounds, vkk, vksize, out);
    }
    rc = check_launch("cdnet_resize_bilinear(two-pass)");
    if (rc == CDNET_OK) g_resize_last_form = 2;
    return rc;
}
