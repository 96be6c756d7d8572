// Device-side training augmentation: the reference's default recipe (my_transforms_direction.py:155-181 random_color,
// :224-259 flips, :262-352 random_elastic, :445-473 random_chooseAug, :496-540 random_crop) per sample on its whole source image,
// evaluated only where the crop needs it.  Four launches per batch:
//   aug_stats_kernel    partial sums of L(Brightness(Color(img))) over the whole source (the Contrast degenerate); clears `varied`
//   aug_field_v_kernel  vertical Gaussian pass of the two displacement-noise planes over the crop window (skipped when every alpha = 0)
//   aug_field_h_kernel  horizontal pass -> dx, dy over the crop window (+ the halo of the filters)
//   aug_tile_kernel     one workgroup per (sample, 32 x 32 output tile): warp the tile + halo into LDS, filter, write the planes
// The arithmetic follows Pillow 12 bit for bit (fp32 blends, fp32 3x3 / 5x5 kernels with a 0.5 rounding start, the u32 box blur); the
// geometry restates OpenCV 4's nearest rules (fixed-point warpAffine, AB_BITS = 10; remap rounds p + d half-to-even).  DESIGN.md section 8.
//
// cdnet_augment_batch_geo adds the three optional steps of the reference's chain (options.py:331-347): random_resize
// (my_transforms_direction.py:69-151) first, random_affine (:185-220) between colour and flips, random_rotation (:354-440) between elastic
// and the filters.  All three are nearest geometry, so `trace` walks a crop pixel back through them too: rotation inverse (OpenCV fixed
// point) -> field -> elastic affine -> un-flip -> Pillow's 16.16 affine -> colour chain at the pixel of the *virtual* resized image ->
// OpenCV's nearest resize map on each raw read.  The resized image is never stored.  The kernels are templated on GEO: the instantiation
// without the table is the code of the default recipe unchanged.
#include "common.h"
#include <math.h>

namespace {

constexpr int T = 32;                  // output tile edge
constexpr int HALO = 6;                // 3 box-blur passes x 2 px (BLUR needs 2, the median 1)
constexpr int WN = T + 2 * HALO;       // 44: LDS window edge
constexpr int NSTAT = 64;              // stats workgroups per sample (partial sums, no atomics)
constexpr int RMAX = 768;              // largest Gaussian radius (sigma <= 191.9): the vertical pass stages (64 + 2R) x 8 floats

__host__ __device__ inline int crop_field_edge(int size) { return size + 2 * HALO; }     // the field window without a rotation

__device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// counter-based U[-1, 1) in steps of 2^-23 (cdnet_amd/augment.py: field_noise is the same function in numpy)
__device__ inline float noise(uint32_t seed, int plane, int y, int x) {
    uint32_t h = fmix32(seed * 0x9E3779B1u + (uint32_t)plane * 0x7F4A7C15u);
    h = fmix32(h ^ ((uint32_t)y * 0xC2B2AE3Du));
    h = fmix32(h ^ ((uint32_t)x * 0x27D4EB2Fu));
    return (float)(h >> 8) * (1.0f / 8388608.0f) - 1.0f;
}

// scipy.ndimage 'reflect' (d c b a | a b c d | d c b a) for any distance
__device__ inline int reflect(int i, int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// PIL ImagingBlend on one u8 channel: fp32 in1 + a * (in2 - in1); truncated inside [0, 1], clipped outside
__device__ inline uint32_t blend(uint32_t deg, uint32_t v, float a) {
    const float t = (float)(int)deg + a * (float)((int)v - (int)deg);
    if (a >= 0.0f && a <= 1.0f) return (uint32_t)(uint8_t)t;
    if (t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
    return (uint32_t)(uint8_t)t;
}

__device__ inline uint32_t luma(uint32_t r, uint32_t g, uint32_t b) { return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16; }

__device__ inline uint32_t clip8(float v) {
    if (v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return (uint32_t)(uint8_t)v;
}

// Color then Brightness of one source pixel (u8 RGB; NC = 1, mode L: Pillow's Color degenerate of an L image is the image itself, so
// that blend returns the pixel for every factor and only Brightness is left)
template <int NC>
__device__ inline void color_bright(const uint8_t *p, const float *f, uint32_t *o) {
    if constexpr (NC == 1) {
        o[0] = blend(0, p[0], f[1]);
    } else {
        const uint32_t g = luma(p[0], p[1], p[2]);
        for (int c = 0; c < 3; ++c) o[c] = blend(0, blend(g, p[c], f[0]), f[1]);
    }
}

// what the Contrast degenerate averages: L of the brightness-adjusted pixel (mode L: the plane itself, no RGB -> L weights)
template <int NC>
__device__ inline uint32_t stat_value(const uint32_t *o) {
    if constexpr (NC == 1) return o[0];
    else return luma(o[0], o[1], o[2]);
}

// OpenCV 4 warpAffine, nearest: fixed point with AB_BITS = 10 and a half-step rounding delta (the host validates with the same function)
__host__ __device__ inline void warp_fixed(const double *M, int y, int x, int &Y, int &X) {
    const int X0 = (int)rint((M[1] * y + M[2]) * 1024.0) + 512, Y0 = (int)rint((M[4] * y + M[5]) * 1024.0) + 512;
    X = (X0 + (int)rint(M[0] * x * 1024.0)) >> 10;
    Y = (Y0 + (int)rint(M[3] * x * 1024.0)) >> 10;
}

// Pillow's FIX of ImagingTransformAffine's 16.16 path
__host__ __device__ inline int pil_fix(double v) { return (int)floor(v * 65536.0 + 0.5); }

constexpr uint32_t GEO_RESIZE = 1, GEO_AFFINE = 2, GEO_ROTATION = 4;

// The frame of sample b: the H x W image every step works in and the origin (fy0, fx0) of its displacement-field window.  Without the
// geo table that is the stored source and the crop + HALO at (y0 - HALO, x0 - HALO); with it the virtual resized image and the table's
// origin (a rotation's pre-image of the crop).  The field kernels and make_ctx both read it here.
struct FieldWin { int fy0, fx0, H, W; };
__device__ inline FieldWin field_win(const cdnet_aug_sample &s, const cdnet_aug_geo *geo, int b) {
    if (geo) return {geo[b].fy0, geo[b].fx0, geo[b].Hr, geo[b].Wr};
    return {s.y0 - HALO, s.x0 - HALO, s.H, s.W};
}

// one sample as the kernels see it.  s.H, s.W are the size every step works in: the stored source's, or with GEO the virtual resized
// image's (Hr x Wr); H0, W0 are the stored size and only the raw reads use them.
struct Ctx {
    cdnet_aug_sample s;
    int fy0, fx0, FE;                  // displacement-field window: origin and edge
    int H0, W0;
    uint32_t flags;
    double isy, isx;                   // OpenCV's 1 / (Hr / H), 1 / (Wr / W)
    int pa[6];                         // Pillow's fixed a0 a1 a2 a3 a4 a5 (a2, a5 with the half-pixel centre folded in)
    double rinv[6];
};

template <bool GEO>
__device__ inline Ctx make_ctx(const cdnet_aug_sample *samples, const cdnet_aug_geo *geo, int b, int FE) {
    Ctx c;
    c.s = samples[b];
    const FieldWin fw = field_win(c.s, GEO ? geo : nullptr, b);
    c.fy0 = fw.fy0;
    c.fx0 = fw.fx0;
    c.FE = FE;
    if constexpr (GEO) {
        const cdnet_aug_geo g = geo[b];
        c.H0 = c.s.H;
        c.W0 = c.s.W;
        c.s.H = fw.H;
        c.s.W = fw.W;
        c.flags = g.flags;
        c.isy = 1.0 / ((double)g.Hr / (double)c.H0);
        c.isx = 1.0 / ((double)g.Wr / (double)c.W0);
        const double *a = g.paff;
        c.pa[0] = pil_fix(a[0]); c.pa[1] = pil_fix(a[1]); c.pa[2] = pil_fix(a[2] + (a[0] * 0.5 + a[1] * 0.5));
        c.pa[3] = pil_fix(a[3]); c.pa[4] = pil_fix(a[4]); c.pa[5] = pil_fix(a[5] + (a[3] * 0.5 + a[4] * 0.5));
        for (int k = 0; k < 6; ++k) c.rinv[k] = g.rinv[k];
    }
    return c;
}

// OpenCV INTER_NEAREST resize: row / column of the stored image behind row / column v of the virtual one
template <bool GEO> __device__ inline int raw_y(const Ctx &c, int y) {
    if constexpr (GEO) {
        if (c.flags & GEO_RESIZE) { const int v = (int)floor(y * c.isy); return v < c.H0 - 1 ? v : c.H0 - 1; }
    }
    return y;
}
template <bool GEO> __device__ inline int raw_x(const Ctx &c, int x) {
    if constexpr (GEO) {
        if (c.flags & GEO_RESIZE) { const int v = (int)floor(x * c.isx); return v < c.W0 - 1 ? v : c.W0 - 1; }
    }
    return x;
}

// Color, Brightness, Contrast (degenerate `mean`) of stored pixel (y, x)
template <int NC>
__device__ inline void ccb(const cdnet_aug_sample &s, int y, int x, uint32_t mean, uint32_t *o) {
    uint32_t t[NC];
    color_bright<NC>(s.img + (size_t)y * s.img_stride + NC * x, s.color, t);
    for (int c = 0; c < NC; ++c) o[c] = blend(mean, t[c], s.color[2]);
}

// the whole random_color chain at pixel (y, x): Sharpness blends with SMOOTH ([1 1 1; 1 5 1; 1 1 1] / 13) of the Contrast image,
// whose outermost rows and columns are copied.  With GEO the pixel, its neighbours and the copied edge are the virtual image's: three
// row and three column maps serve the nine reads.
template <bool GEO, int NC>
__device__ inline void color_chain(const Ctx &cx, int y, int x, uint32_t mean, uint32_t *o) {
    const cdnet_aug_sample &s = cx.s;
    uint32_t mid[NC];
    ccb<NC>(s, raw_y<GEO>(cx, y), raw_x<GEO>(cx, x), mean, mid);
    uint32_t deg[NC];
    for (int c = 0; c < NC; ++c) deg[c] = mid[c];
    if (y >= 1 && y < s.H - 1 && x >= 1 && x < s.W - 1) {
        const int my[3] = {raw_y<GEO>(cx, y - 1), raw_y<GEO>(cx, y), raw_y<GEO>(cx, y + 1)};
        const int mx[3] = {raw_x<GEO>(cx, x - 1), raw_x<GEO>(cx, x), raw_x<GEO>(cx, x + 1)};
        uint32_t nb[3][3][NC];
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dy == 0 && dx == 0) {
                    for (int c = 0; c < NC; ++c) nb[1][1][c] = mid[c];
                } else {
                    ccb<NC>(s, my[dy + 1], mx[dx + 1], mean, nb[dy + 1][dx + 1]);
                }
            }
        const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
        for (int c = 0; c < NC; ++c) {
            float ss = 0.5f;
            for (int r = 2; r >= 0; --r) {          // Pillow sums the row below first
                const float kc = r == 1 ? k5 : k1;
                ss = ss + (((float)nb[r][0][c] * k1 + (float)nb[r][1][c] * kc) + (float)nb[r][2][c] * k1);
            }
            deg[c] = clip8(ss);
        }
    }
    for (int c = 0; c < NC; ++c) o[c] = blend(deg[c], mid[c], s.color[3]);
}

// pixel q of the last geometric step's output -> pixel of the unflipped, uncoloured (with GEO: virtual resized) image; false: outside
// at some step (every plane reads 0).  The host has validated that the field window holds the part of the image that the bounding box
// of the crop + HALO's corner pre-images covers, and with it every lookup below.
template <bool GEO>
__device__ inline bool trace(const Ctx &c, int qy, int qx, const float *fx, const float *fy, int &ty, int &tx) {
    const cdnet_aug_sample &s = c.s;
    if constexpr (GEO) {
        if (c.flags & GEO_ROTATION) {
            int Y, X;
            warp_fixed(c.rinv, qy, qx, Y, X);
            if ((unsigned)X >= (unsigned)s.W || (unsigned)Y >= (unsigned)s.H) return false;
            qy = Y;
            qx = X;
        }
    }
    int ry = qy, rx = qx;
    if (s.alpha != 0.0f) {
        const size_t o = (size_t)(qy - c.fy0) * c.FE + (qx - c.fx0);
        rx = (int)rintf((float)qx + fx[o]);
        ry = (int)rintf((float)qy + fy[o]);
        if ((unsigned)rx >= (unsigned)s.W || (unsigned)ry >= (unsigned)s.H) return false;
    }
    int X, Y;
    warp_fixed(s.minv, ry, rx, Y, X);
    if ((unsigned)X >= (unsigned)s.W || (unsigned)Y >= (unsigned)s.H) return false;
    tx = s.hflip ? s.W - 1 - X : X;
    ty = s.vflip ? s.H - 1 - Y : Y;
    if constexpr (GEO) {
        if (c.flags & GEO_AFFINE) {
            // Pillow affine_fixed: the sums wrap in 32 bits as its incremental adds do
            const int xin = (int)((uint32_t)c.pa[2] + (uint32_t)c.pa[1] * (uint32_t)ty + (uint32_t)c.pa[0] * (uint32_t)tx) >> 16;
            const int yin = (int)((uint32_t)c.pa[5] + (uint32_t)c.pa[4] * (uint32_t)ty + (uint32_t)c.pa[3] * (uint32_t)tx) >> 16;
            if ((unsigned)xin >= (unsigned)s.W || (unsigned)yin >= (unsigned)s.H) return false;
            tx = xin;
            ty = yin;
        }
    }
    return true;
}

// label at stored pixel (y, x)
__device__ inline int label_at(const cdnet_aug_sample &s, int y, int x) {
    return s.label_i32 ? ((const int32_t *)s.label)[(size_t)y * s.label_stride + x] : ((const uint8_t *)s.label)[(size_t)y * s.label_stride + x];
}

// with GEO the sum is over the virtual resized image (Contrast's mean is taken after random_resize): a workgroup walks whole rows, so
// the row map is computed once per row
template <bool GEO, int NC>
__global__ void __launch_bounds__(256) aug_stats_kernel(const cdnet_aug_sample *samples, const cdnet_aug_geo *geo, unsigned long long *partial,
                                                        int32_t *varied) {
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) varied[b] = 0;
    unsigned long long acc = 0;
    if constexpr (GEO) {
        const Ctx c = make_ctx<true>(samples, geo, b, 0);
        const cdnet_aug_sample &s = c.s;
        for (int y = blockIdx.x; y < s.H; y += gridDim.x) {
            const uint8_t *row = s.img + (size_t)raw_y<true>(c, y) * s.img_stride;
            for (int x = threadIdx.x; x < s.W; x += blockDim.x) {
                uint32_t o[NC];
                color_bright<NC>(row + NC * raw_x<true>(c, x), s.color, o);
                acc += stat_value<NC>(o);
            }
        }
    } else {
        const cdnet_aug_sample s = samples[b];
        const size_t n = (size_t)s.H * s.W;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
            const int y = (int)(i / s.W), x = (int)(i % s.W);
            uint32_t o[NC];
            color_bright<NC>(s.img + (size_t)y * s.img_stride + NC * x, s.color, o);
            acc += stat_value<NC>(o);
        }
    }
    __shared__ unsigned long long red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)b * NSTAT + blockIdx.x] = red[0];
}

__device__ inline int gauss_radius(float sigma) { return (int)(4.0f * sigma + 0.5f); }

// normalised scipy Gaussian weights (float64, truncate = 4) of sample s into w[0 .. 2R]
__device__ inline void gauss_weights(float sigma, int R, float *w, double *tmp) {
    const double s2 = (double)sigma * sigma;
    for (int k = threadIdx.x; k <= 2 * R; k += blockDim.x) tmp[k] = exp(-0.5 / s2 * (double)(k - R) * (k - R));
    __syncthreads();
    __shared__ double total;
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k <= 2 * R; ++k) t += tmp[k];
        total = t;
    }
    __syncthreads();
    for (int k = threadIdx.x; k <= 2 * R; k += blockDim.x) w[k] = (float)(tmp[k] / total);
    __syncthreads();
}

// tmp[b][p][r][e] = sum_k w_k noise(reflect(y + k), reflect(x)) for the window rows y = fy0 + r inside the image and the columns
// x = fx0 - R + e (e < FS + 2R) the horizontal pass reads.  A workgroup owns VC columns x VR rows: the noise of its rows +- R is
// hashed once into LDS (dynamic, (VR + 2 rmax) x VC floats; the float64 weights are staged there first), then every thread sums its taps
// from LDS.
constexpr int VC = 8, VR = 64;
__global__ void __launch_bounds__(256) aug_field_v_kernel(const cdnet_aug_sample *samples, const cdnet_aug_geo *geo, int FS, int rmax, float *tmp) {
    const int b = blockIdx.z, p = blockIdx.y;
    const cdnet_aug_sample s = samples[b];
    if (s.alpha == 0.0f) return;
    const FieldWin fw = field_win(s, geo, b);
    const int R = gauss_radius(s.sigma), TW = FS + 2 * rmax, E = FS + 2 * R;
    const int nby = (FS + VR - 1) / VR;
    const int e0 = (blockIdx.x / nby) * VC, r0 = (blockIdx.x % nby) * VR;
    if (e0 >= E) return;
    __shared__ float w[2 * RMAX + 1];
    extern __shared__ float nz[];                    // [VR + 2R][VC]
    gauss_weights(s.sigma, R, w, (double *)nz);
    const int rows = VR + 2 * R;
    for (int i = threadIdx.x; i < rows * VC; i += blockDim.x) {
        const int rr = i / VC, e = e0 + i % VC;
        const int y = fw.fy0 + r0 - R + rr;
        nz[i] = e < E ? noise(s.seed, p, reflect(y, fw.H), reflect(fw.fx0 - R + e, fw.W)) : 0.0f;
    }
    __syncthreads();
    const int c = threadIdx.x % VC, e = e0 + c;
    if (e >= E) return;
    for (int rr = threadIdx.x / VC; rr < VR; rr += blockDim.x / VC) {
        const int r = r0 + rr;
        if (r >= FS) break;
        const int y = fw.fy0 + r;
        float acc = 0.0f;
        if (y >= 0 && y < fw.H) {
            const float *col = nz + rr * VC + c;
            for (int k = 0; k <= 2 * R; ++k) acc += w[k] * col[k * VC];
        }
        tmp[(((size_t)b * 2 + p) * FS + r) * TW + e] = acc;
    }
}

// field[b][p][r][c] = alpha * sum_k w_k tmp[..][c + k + R]: p = 0 is dx (columns), 1 is dy (rows); 0 outside the image.  A workgroup owns
// 256 columns of one row; its tmp segment (256 + 2R floats) is staged in LDS.
__global__ void __launch_bounds__(256) aug_field_h_kernel(const cdnet_aug_sample *samples, const cdnet_aug_geo *geo, int FS, int rmax, const float *tmp,
                                                          float *field) {
    const int b = blockIdx.z, p = blockIdx.y;
    const cdnet_aug_sample s = samples[b];
    if (s.alpha == 0.0f) return;
    const FieldWin fw = field_win(s, geo, b);
    const int R = gauss_radius(s.sigma), TW = FS + 2 * rmax;
    const int nbx = (FS + 255) / 256;
    const int r = blockIdx.x / nbx, c0 = (blockIdx.x % nbx) * 256;
    __shared__ float w[2 * RMAX + 1];
    __shared__ double wd[2 * RMAX + 1];
    __shared__ float seg[256 + 2 * RMAX];
    gauss_weights(s.sigma, R, w, wd);
    const float *row = tmp + (((size_t)b * 2 + p) * FS + r) * TW;
    const int n = min(256, FS - c0) + 2 * R;
    for (int i = threadIdx.x; i < n; i += blockDim.x) seg[i] = row[c0 + i];
    __syncthreads();
    const int c = c0 + threadIdx.x;
    if (c >= FS) return;
    const int y = fw.fy0 + r, x = fw.fx0 + c;
    float acc = 0.0f;
    if (y >= 0 && y < fw.H && x >= 0 && x < fw.W) {
        for (int k = 0; k <= 2 * R; ++k) acc += w[k] * seg[threadIdx.x + k];
        acc *= s.alpha;
    }
    field[(((size_t)b * 2 + p) * FS + r) * FS + c] = acc;
}

// one Pillow box-blur pass (radius 1.375 -> ww, fw of ImagingHorizontalBoxBlur) at 5 u8 samples
struct Norm { int on; float mean[3], std[3]; };

constexpr uint32_t BOX_WW = 4473924u, BOX_FW = 1677722u;
__device__ inline uint8_t box5(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e) {
    return (uint8_t)((((b + c + d) * BOX_WW) + (a + e) * BOX_FW + (1u << 23)) >> 24);
}

template <bool GEO, int NC>
__global__ void __launch_bounds__(256) aug_tile_kernel(const cdnet_aug_sample *samples, const cdnet_aug_geo *geo, int size, int FS, int tiles_x,
                                                       const unsigned long long *partial, const float *field, Norm norm, float *image,
                                                       uint8_t *weight, void *label, int label_i32, int32_t *varied) {
    const int b = blockIdx.y;
    const Ctx ctx = make_ctx<GEO>(samples, geo, b, FS);
    const cdnet_aug_sample &s = ctx.s;                  // H, W: the image every step below works in (with GEO the virtual resized one)
    const int ty0 = (blockIdx.x / tiles_x) * T, tx0 = (blockIdx.x % tiles_x) * T;     // tile origin in the crop
    __shared__ uint8_t A[NC][WN][WN], Bf[NC][WN][WN];
    __shared__ uint32_t mean_s;
    __shared__ int ref_label;
    const float *fx = field + (size_t)b * 2 * FS * FS, *fy = fx + (size_t)FS * FS;
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (int k = 0; k < NSTAT; ++k) sum += partial[(size_t)b * NSTAT + k];
        mean_s = (uint32_t)(int)((double)sum / (double)((long long)s.H * s.W) + 0.5);        // ImageStat mean, int(+ 0.5)
        int ty, tx, l = 0;
        if (s.y0 < s.H && s.x0 < s.W && trace<GEO>(ctx, s.y0, s.x0, fx, fy, ty, tx)) l = label_at(s, raw_y<GEO>(ctx, ty), raw_x<GEO>(ctx, tx));
        ref_label = l;
    }
    __syncthreads();
    const uint32_t mean = mean_s;
    const size_t plane = (size_t)size * size;
    bool differs = false;
    // 1. warp the tile + halo: window (i, j) is the elastic-output pixel q = crop origin + tile origin - HALO + (i, j)
    for (int idx = threadIdx.x; idx < WN * WN; idx += blockDim.x) {
        const int i = idx / WN, j = idx % WN;
        const int cy = ty0 - HALO + i, cx = tx0 - HALO + j;              // crop coordinates
        if (cy >= size + HALO || cx >= size + HALO) continue;
        const int qy = s.y0 + cy, qx = s.x0 + cx;
        if (qy < 0 || qy >= s.H || qx < 0 || qx >= s.W) continue;        // never read: the filters clamp to the image
        int ty, tx;
        uint32_t v[NC] = {};
        const bool in = trace<GEO>(ctx, qy, qx, fx, fy, ty, tx);
        if (in) color_chain<GEO, NC>(ctx, ty, tx, mean, v);
        for (int c = 0; c < NC; ++c) A[c][i][j] = (uint8_t)v[c];
        if (i >= HALO && i < HALO + T && j >= HALO && j < HALO + T && cy < size && cx < size) {
            const size_t o = ((size_t)b * size + cy) * size + cx;
            const int my = in ? raw_y<GEO>(ctx, ty) : 0, mx = in ? raw_x<GEO>(ctx, tx) : 0;
            const int l = in ? label_at(s, my, mx) : 0;
            weight[o] = in ? s.weight[(size_t)my * s.weight_stride + mx] : 0;
            if (label_i32) ((int32_t *)label)[o] = l;
            else ((uint8_t *)label)[o] = (uint8_t)l;
            differs |= l != ref_label;
        }
    }
    // crop pixels outside the source (a source smaller than the crop): zero everywhere, weight 0
    for (int idx = threadIdx.x; idx < T * T; idx += blockDim.x) {
        const int cy = ty0 + idx / T, cx = tx0 + idx % T;
        if (cy >= size || cx >= size) continue;
        const int qy = s.y0 + cy, qx = s.x0 + cx;
        if (qy < s.H && qx < s.W) continue;
        const size_t o = ((size_t)b * size + cy) * size + cx;
        weight[o] = 0;
        if (label_i32) ((int32_t *)label)[o] = 0;
        else ((uint8_t *)label)[o] = 0;
        differs |= 0 != ref_label;
    }
    if (differs) varied[b] = 1;
    __syncthreads();
    // 2. GaussianBlur(2): three horizontal, then three vertical box passes, each rounded to u8; reads are clamped to the image
    uint8_t (*fin)[WN][WN] = A;
    const int wr0 = s.y0 + ty0 - HALO, wc0 = s.x0 + tx0 - HALO;          // image row / column of window (0, 0)
    if (s.filter == 2) {
        uint8_t (*src)[WN][WN] = A, (*dst)[WN][WN] = Bf;
        for (int pass = 1; pass <= 6; ++pass) {
            const bool horiz = pass <= 3;
            const int k = horiz ? pass : pass - 3;
            const int m0 = 2 * k, m1 = WN - 2 * k;                           // the window range shrinks by 2 per pass
            const int count = (horiz ? WN : (m1 - m0)) * (horiz ? (m1 - m0) : T);
            for (int idx = threadIdx.x; idx < count; idx += blockDim.x) {
                int i, j;
                if (horiz) { i = idx / (m1 - m0); j = m0 + idx % (m1 - m0); }
                else { j = HALO + idx % T; i = m0 + idx / T; }
                const int y = wr0 + i, x = wc0 + j;
                if (y < 0 || y >= s.H || x < 0 || x >= s.W) continue;
                if (i - HALO + ty0 >= size + HALO || j - HALO + tx0 >= size + HALO) continue;
                for (int c = 0; c < NC; ++c) {
                    uint32_t t[5];
                    for (int d = -2; d <= 2; ++d) {
                        if (horiz) t[d + 2] = src[c][i][clampi(x + d, 0, s.W - 1) - wc0];
                        else t[d + 2] = src[c][clampi(y + d, 0, s.H - 1) - wr0][j];
                    }
                    dst[c][i][j] = box5(t[0], t[1], t[2], t[3], t[4]);
                }
            }
            __syncthreads();
            uint8_t (*sw)[WN][WN] = src; src = dst; dst = sw;
        }
        fin = src;
    }
    // 3. the remaining filters at the tile's pixels, then the output planes
    for (int idx = threadIdx.x; idx < T * T; idx += blockDim.x) {
        const int i = HALO + idx / T, j = HALO + idx % T;
        const int cy = ty0 + idx / T, cx = tx0 + idx % T;
        if (cy >= size || cx >= size) continue;
        const int y = wr0 + i, x = wc0 + j;
        uint32_t v[NC] = {};
        if (y < s.H && x < s.W) {
            for (int c = 0; c < NC; ++c) v[c] = fin[c][i][j];
            if (s.filter == 1 && y >= 2 && y < s.H - 2 && x >= 2 && x < s.W - 2) {
                // BLUR: the 5 x 5 ring / 16, Pillow's order (row below first, left to right), 2-px image edge copied
                const float k = 1.0f / 16.0f;
                for (int c = 0; c < NC; ++c) {
                    float ss = 0.5f;
                    for (int dy = 2; dy >= -2; --dy) {
                        const bool ring = dy == 2 || dy == -2;
                        float t = (float)A[c][i + dy][j - 2] * k;
                        for (int dx = -1; dx <= 2; ++dx) t = t + (float)A[c][i + dy][j + dx] * ((ring || dx == 2) ? k : 0.0f);
                        ss = ss + t;
                    }
                    v[c] = clip8(ss);
                }
            } else if (s.filter == 3) {
                // MedianFilter(3) of the edge-replicated image
                for (int c = 0; c < NC; ++c) {
                    uint32_t m[9];
                    int n = 0;
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx)
                            m[n++] = A[c][clampi(y + dy, 0, s.H - 1) - wr0][clampi(x + dx, 0, s.W - 1) - wc0];
                    for (int a = 0; a <= 4; ++a)
                        for (int bb = a + 1; bb < 9; ++bb)
                            if (m[bb] < m[a]) { const uint32_t t = m[a]; m[a] = m[bb]; m[bb] = t; }
                    v[c] = m[4];
                }
            }
        }
        for (int c = 0; c < NC; ++c) {
            float f = (float)v[c] / 255.0f;
            if (norm.on) f = (f - norm.mean[c]) / norm.std[c];
            image[((size_t)b * NC + c) * plane + (size_t)cy * size + cx] = f;
        }
    }
}

constexpr int FIELD_EDGE_MAX = 16384;

// the stats launch and the tile launch of one batch for a plane count
template <int NC>
void launch_stats(const cdnet_aug_sample *samples, const cdnet_aug_geo *geo, int B, unsigned long long *partial, int32_t *varied, hipStream_t st) {
    if (geo) aug_stats_kernel<true, NC><<<dim3(NSTAT, B), 256, 0, st>>>(samples, geo, partial, varied);
    else aug_stats_kernel<false, NC><<<dim3(NSTAT, B), 256, 0, st>>>(samples, geo, partial, varied);
}

template <int NC>
void launch_tile(const cdnet_aug_sample *samples, const cdnet_aug_geo *geo, int B, int size, int FS, const unsigned long long *partial, const float *fld,
                 const Norm &norm, float *image, uint8_t *weight, void *label, int label_i32, int32_t *varied, hipStream_t st) {
    const int tiles = cdnet::cdiv(size, T);
    if (geo) aug_tile_kernel<true, NC><<<dim3(tiles * tiles, B), 256, 0, st>>>(samples, geo, size, FS, tiles, partial, fld, norm, image, weight, label, label_i32, varied);
    else aug_tile_kernel<false, NC><<<dim3(tiles * tiles, B), 256, 0, st>>>(samples, geo, size, FS, tiles, partial, fld, norm, image, weight, label, label_i32, varied);
}

// the entry behind the ABI calls: geo == nullptr is the default recipe (field window: crop + HALO at the crop origin); NC = 3 (RGB) or 1 (L)
int augment_batch(const char *who, const cdnet_aug_sample *samples, const cdnet_aug_sample *samples_host, const cdnet_aug_geo *geo,
                  const cdnet_aug_geo *geo_host, int FS, int B, int size, const float *norm_host, void *workspace, size_t workspace_bytes,
                  float *image, uint8_t *weight, void *label, int label_i32, int32_t *varied, float *field, void *stream, int NC) {
    if (NC != 1 && NC != 3) {
        cdnet::set_error("%s: channels is 1 (mode L) or 3 (RGB), got %d", who, NC);
        return CDNET_E_ARG;
    }
    CDNET_REQUIRE(samples && samples_host && image && weight && label && varied, "%s: null pointer", who);
    CDNET_REQUIRE((geo == nullptr) == (geo_host == nullptr), "%s: null pointer (geo table: device and host copy, or neither)", who);
    CDNET_REQUIRE(B >= 1 && B <= 4096 && size >= 1 && size <= 4096, "%s: B in 1..4096, size in 1..4096", who);
    CDNET_REQUIRE(label_i32 == 0 || label_i32 == 1, "%s: label_i32 is 0 or 1", who);
    CDNET_REQUIRE(FS >= 1 && FS <= FIELD_EDGE_MAX, "%s: field_edge in 1..%d", who, FIELD_EDGE_MAX);
    int rmax = 0;
    bool any_field = false;
    for (int b = 0; b < B; ++b) {
        const cdnet_aug_sample &s = samples_host[b];
        CDNET_REQUIRE(s.img && s.weight && s.label, "%s: null pointer in sample %d", who, b);
        CDNET_REQUIRE(s.H >= 1 && s.W >= 1 && s.img_stride >= NC * s.W && s.weight_stride >= s.W && s.label_stride >= s.W,
                      "%s: sample %d: bad size or row stride", who, b);
        CDNET_REQUIRE(s.label_i32 == label_i32, "%s: sample %d: label type differs from the batch's", who, b);
        CDNET_REQUIRE(s.filter >= 0 && s.filter <= 3, "%s: sample %d: filter code %d (0 none, 1 BLUR, 2 GaussianBlur, 3 MedianFilter)", who, b, s.filter);
        CDNET_REQUIRE((s.hflip == 0 || s.hflip == 1) && (s.vflip == 0 || s.vflip == 1), "%s: sample %d: flips are 0 or 1", who, b);
        int H = s.H, W = s.W, fy0 = s.y0 - HALO, fx0 = s.x0 - HALO;        // the image the steps work in, the field window's origin
        if (geo_host) {
            const cdnet_aug_geo &g = geo_host[b];
            CDNET_REQUIRE((g.flags & ~(GEO_RESIZE | GEO_AFFINE | GEO_ROTATION)) == 0, "%s: sample %d: unknown geo flags", who, b);
            CDNET_REQUIRE(g.Hr >= 1 && g.Wr >= 1 && g.Hr <= 32767 && g.Wr <= 32767, "%s: sample %d: resized size %d x %d outside 1..32767", who, b, g.Hr, g.Wr);
            CDNET_REQUIRE((g.flags & GEO_RESIZE) || (g.Hr == s.H && g.Wr == s.W), "%s: sample %d: resized size differs from the source's without the resize flag", who, b);
            for (int k = 0; k < 6; ++k)
                CDNET_REQUIRE(isfinite(g.paff[k]) && isfinite(g.rinv[k]) && fabs(g.paff[k]) < 1e6 && fabs(g.rinv[k]) < 1e6,
                              "%s: sample %d: geo matrix not finite", who, b);
            H = g.Hr, W = g.Wr, fy0 = g.fy0, fx0 = g.fx0;
            if (g.flags & GEO_AFFINE) {
                // Pillow takes its 16.16 path only while the four corners stay inside +-32768 (Geometry.c: check_fixed)
                const double *a = g.paff;
                for (int k = 0; k < 4; ++k) {
                    const double x = (k & 1) ? W : 0, y = (k & 2) ? H : 0;
                    CDNET_REQUIRE(fabs(x * a[0] + y * a[1] + a[2]) < 32768.0 && fabs(x * a[3] + y * a[4] + a[5]) < 32768.0,
                                  "%s: sample %d: affine leaves Pillow's 16.16 range", who, b);
                }
            }
        }
        CDNET_REQUIRE(s.y0 >= 0 && s.x0 >= 0 && s.y0 <= (H > size ? H - size : 0) && s.x0 <= (W > size ? W - size : 0),
                      "%s: sample %d: crop origin outside the source", who, b);
        CDNET_REQUIRE(isfinite(s.alpha), "%s: sample %d: alpha", who, b);
        for (int k = 0; k < 4; ++k) CDNET_REQUIRE(isfinite(s.color[k]), "%s: sample %d: colour factor", who, b);
        for (int k = 0; k < 6; ++k) CDNET_REQUIRE(isfinite(s.minv[k]) && fabs(s.minv[k]) < 1e6, "%s: sample %d: affine", who, b);
        if (s.alpha != 0.0f) {
            CDNET_REQUIRE(s.sigma > 0.0f && (int)(4.0f * s.sigma + 0.5f) <= RMAX, "%s: sample %d: sigma in (0, 191.8] (radius <= 768)", who, b);
            any_field = true;
            const int R = (int)(4.0f * s.sigma + 0.5f);
            rmax = R > rmax ? R : rmax;
            // the field is read at the rotation's pre-image of the crop + HALO, where that lies inside the image (`trace` stops before the
            // lookup elsewhere).  The fixed-point map is monotone in each coordinate, so the bounding box of the four corner pre-images
            // holds every pixel's: its part inside the image must lie in the window.
            long long ylo = 0, yhi = 0, xlo = 0, xhi = 0;
            for (int k = 0; k < 4; ++k) {
                int Y = s.y0 - HALO + ((k & 2) ? size + 2 * HALO - 1 : 0), X = s.x0 - HALO + ((k & 1) ? size + 2 * HALO - 1 : 0);
                if (geo_host && (geo_host[b].flags & GEO_ROTATION)) warp_fixed(geo_host[b].rinv, Y, X, Y, X);
                ylo = k == 0 || Y < ylo ? Y : ylo, yhi = k == 0 || Y > yhi ? Y : yhi;
                xlo = k == 0 || X < xlo ? X : xlo, xhi = k == 0 || X > xhi ? X : xhi;
            }
            ylo = ylo < 0 ? 0 : ylo, xlo = xlo < 0 ? 0 : xlo;
            yhi = yhi > H - 1 ? H - 1 : yhi, xhi = xhi > W - 1 ? W - 1 : xhi;
            if (ylo <= yhi && xlo <= xhi)
                CDNET_REQUIRE(ylo >= fy0 && yhi < (long long)fy0 + FS && xlo >= fx0 && xhi < (long long)fx0 + FS,
                              "%s: sample %d: field window (origin %d, %d, edge %d) misses rows %lld..%lld, columns %lld..%lld of the crop's pre-image",
                              who, b, fy0, fx0, FS, ylo, yhi, xlo, xhi);
        }
    }
    const size_t need = cdnet_augment_geo_workspace_bytes(B, size, rmax, FS);
    CDNET_REQUIRE(workspace || workspace_bytes == 0, "%s: null workspace", who);
    if (workspace_bytes < need) {
        cdnet::set_error("%s: workspace %zu bytes, need %zu", who, workspace_bytes, need);
        return CDNET_E_WORKSPACE;
    }
    char *ws = (char *)workspace;
    unsigned long long *partial = (unsigned long long *)ws;
    float *tmp = (float *)(ws + cdnet::align_up((size_t)B * NSTAT * 8, 256));
    float *fld = field ? field : (float *)((char *)tmp + cdnet::align_up((size_t)B * 2 * FS * (FS + 2 * rmax) * 4, 256));
    Norm norm = {norm_host != nullptr, {0, 0, 0}, {1, 1, 1}};
    for (int c = 0; norm_host && c < NC; ++c) {
        norm.mean[c] = norm_host[c];
        norm.std[c] = norm_host[NC + c];
    }
    hipStream_t st = (hipStream_t)stream;
    if (NC == 1) launch_stats<1>(samples, geo, B, partial, varied, st);
    else launch_stats<3>(samples, geo, B, partial, varied, st);
    if (any_field) {
        const int vblocks = cdnet::cdiv(FS, VR) * cdnet::cdiv(FS + 2 * rmax, VC);
        aug_field_v_kernel<<<dim3(vblocks, 2, B), 256, (size_t)(VR + 2 * rmax) * VC * 4, st>>>(samples, geo, FS, rmax, tmp);
        aug_field_h_kernel<<<dim3(FS * cdnet::cdiv(FS, 256), 2, B), 256, 0, st>>>(samples, geo, FS, rmax, tmp, fld);
    }
    if (NC == 1) launch_tile<1>(samples, geo, B, size, FS, partial, fld, norm, image, weight, label, label_i32, varied, st);
    else launch_tile<3>(samples, geo, B, size, FS, partial, fld, norm, image, weight, label, label_i32, varied, st);
    return cdnet::check_launch(who);
}

}  // namespace

extern "C" size_t cdnet_augment_geo_workspace_bytes(int B, int size, int max_radius, int field_edge) {
    if (B < 1 || size < 1 || max_radius < 0 || max_radius > RMAX || field_edge < 1 || field_edge > FIELD_EDGE_MAX) return 0;
    const size_t FS = field_edge;
    return cdnet::align_up((size_t)B * NSTAT * 8, 256) + cdnet::align_up((size_t)B * 2 * FS * (FS + 2 * max_radius) * 4, 256) + (size_t)B * 2 * FS * FS * 4;
}

extern "C" size_t cdnet_augment_workspace_bytes(int B, int size, int max_radius) {
    if (size < 1 || size > FIELD_EDGE_MAX - 2 * HALO) return 0;
    return cdnet_augment_geo_workspace_bytes(B, size, max_radius, crop_field_edge(size));
}

extern "C" int cdnet_augment_batch_c(const cdnet_aug_sample *samples, const cdnet_aug_sample *samples_host, int B, int size, const float *norm_host,
                                     void *workspace, size_t workspace_bytes, float *image, uint8_t *weight, void *label, int label_i32,
                                     int32_t *varied, float *field, void *stream, int channels) {
    return augment_batch("cdnet_augment_batch_c", samples, samples_host, nullptr, nullptr, crop_field_edge(size > 0 ? size : 1), B, size, norm_host,
                         workspace, workspace_bytes, image, weight, label, label_i32, varied, field, stream, channels);
}

extern "C" int cdnet_augment_batch_geo_c(const cdnet_aug_sample *samples, const cdnet_aug_sample *samples_host, const cdnet_aug_geo *geo,
                                         const cdnet_aug_geo *geo_host, int field_edge, int B, int size, const float *norm_host, void *workspace,
                                         size_t workspace_bytes, float *image, uint8_t *weight, void *label, int label_i32, int32_t *varied,
                                         float *field, void *stream, int channels) {
    if (channels != 1 && channels != 3) {
        cdnet::set_error("cdnet_augment_batch_geo_c: channels is 1 (mode L) or 3 (RGB), got %d", channels);
        return CDNET_E_ARG;
    }
    CDNET_REQUIRE(geo && geo_host, "cdnet_augment_batch_geo_c: null pointer (geo table)");
    return augment_batch("cdnet_augment_batch_geo_c", samples, samples_host, geo, geo_host, field_edge, B, size, norm_host, workspace,
                         workspace_bytes, image, weight, label, label_i32, varied, field, stream, channels);
}

// the RGB entries: the channels = 3 call
extern "C" int cdnet_augment_batch(const cdnet_aug_sample *samples, const cdnet_aug_sample *samples_host, int B, int size, const float *norm_host,
                                   void *workspace, size_t workspace_bytes, float *image, uint8_t *weight, void *label, int label_i32,
                                   int32_t *varied, float *field, void *stream) {
    return augment_batch("cdnet_augment_batch", samples, samples_host, nullptr, nullptr, crop_field_edge(size > 0 ? size : 1), B, size, norm_host,
                         workspace, workspace_bytes, image, weight, label, label_i32, varied, field, stream, 3);
}

extern "C" int cdnet_augment_batch_geo(const cdnet_aug_sample *samples, const cdnet_aug_sample *samples_host, const cdnet_aug_geo *geo,
                                       const cdnet_aug_geo *geo_host, int field_edge, int B, int size, const float *norm_host, void *workspace,
                                       size_t workspace_bytes, float *image, uint8_t *weight, void *label, int label_i32, int32_t *varied,
                                       float *field, void *stream) {
    CDNET_REQUIRE(geo && geo_host, "cdnet_augment_batch_geo: null pointer (geo table)");
    return augment_batch("cdnet_augment_batch_geo", samples, samples_host, geo, geo_host, field_edge, B, size, norm_host, workspace,
                         workspace_bytes, image, weight, label, label_i32, varied, field, stream, 3);
}
