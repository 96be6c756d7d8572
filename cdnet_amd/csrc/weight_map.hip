// U-Net border weight maps from instance labels: the `<stem>_weight.png` every training sample carries (train_util_dam.py:102,171,230,242
// read it as png / 20).  The reference has no generator for them.
//
//   w(p) = 1 + w0 * exp(-(d1 + d2)^2 / (2 sigma^2))     on background pixels, d1 <= d2 the Euclidean distances to the nearest and the
//                                                        second-nearest distinct instance
//   w(p) = 1                                             on the pixels of an instance, and where no second instance is in reach
//   stored u8 = floor(20 * w(p))
//
// The stored byte bounds the search exactly: 20 * w0 * exp(-s^2 / (2 sigma^2)) < 1 as soon as s = d1 + d2 > sigma * sqrt(2 ln(20 w0)), and
// d2 <= s, so no instance farther than R = ceil(sigma * sqrt(2 ln(20 w0))) changes a byte.  A pixel needs the labels inside a disc of radius R:
// one workgroup per WM_TILE x WM_TILE tile stages the tile plus R on each side into LDS (zeros outside the image) and every pixel keeps the two
// smallest squared integer distances to distinct ids while it visits the rows from dy = 0 outward, |dx| bounded by the circle of the current
// second-smallest distance; the scan ends once dy^2 >= that distance.  Integer arithmetic up to the last line, which is fp64.
#include <math.h>
#include "launch.h"

using namespace cdnet;

namespace {

constexpr int WM_TILE = 32, WM_THREADS = 256;
constexpr int WM_ROWS = WM_TILE * WM_TILE / WM_THREADS;        // pixels per thread: rows ty, ty + 8, ty + 16, ty + 24 of column tx
constexpr int WM_MAX_R = 64;                                   // (32 + 2 * 64)^2 * 4 B = 100 KB of the CU's 160 KB
constexpr int WM_MAX_LDS = (WM_TILE + 2 * WM_MAX_R) * (WM_TILE + 2 * WM_MAX_R) * 4;

// A wave is two tile rows of 32 adjacent columns: the 32 lanes of a ds_read_b32 lane group read 32 adjacent dwords, no bank conflicts.
__global__ __launch_bounds__(WM_THREADS) void weight_map_kernel(const int32_t *__restrict__ lab, int H, int W, int R, double w0, double sigma,
                                                                uint8_t *__restrict__ out) {
    extern __shared__ __align__(16) int32_t win[];
    __shared__ int s_first, s_multi;
    const int P = WM_TILE + 2 * R;                             // window side
    const int ty0 = blockIdx.y * WM_TILE, tx0 = blockIdx.x * WM_TILE;
    if (threadIdx.x == 0) s_first = s_multi = 0;
    __syncthreads();
    int first = 0;
    bool multi = false;
    for (int i = threadIdx.x; i < P * P; i += WM_THREADS) {
        const int wy = i / P, wx = i - wy * P;
        const int gy = ty0 - R + wy, gx = tx0 - R + wx;
        int v = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = lab[(size_t)gy * W + gx];
        v = v > 0 ? v : 0;
        win[i] = v;
        if (v) {
            if (!first) first = v;
            else if (v != first) multi = true;
        }
    }
    if (first) {
        const int old = atomicCAS(&s_first, 0, first);
        if (old != 0 && old != first) multi = true;
    }
    if (multi) s_multi = 1;
    __syncthreads();
    const bool two_ids = s_multi != 0;                         // false: no label, or one instance only, in the whole window - every byte is 20

    const int tx = threadIdx.x & (WM_TILE - 1), ty = threadIdx.x / WM_TILE;
    const int gx = tx0 + tx;
    if (gx >= W) return;
    const int R2 = R * R;
    for (int k = 0; k < WM_ROWS; ++k) {
        const int ly = ty + k * (WM_THREADS / WM_TILE), gy = ty0 + ly;
        if (gy >= H) break;
        uint8_t o = 20;
        const int32_t *c = win + (ly + R) * P + (tx + R);
        if (two_ids && c[0] == 0) {
            int b1 = R2 + 1, b2 = R2 + 1, id1 = 0, id2 = 0;   // the two smallest squared distances to distinct ids; R2 + 1: none in reach
            for (int dy = 0; dy <= R; ++dy) {
                const int dy2 = dy * dy;
                if (dy2 >= b2) break;                          // a candidate with r2 >= b2 changes nothing
                const int lim = b2 - 1 - dy2;                  // dx^2 <= lim
                int xm = (int)sqrtf((float)lim);
                if ((xm + 1) * (xm + 1) <= lim) ++xm;
                if (xm * xm > lim) --xm;
                for (int side = 0; side < (dy ? 2 : 1); ++side) {
                    const int32_t *row = side ? c - dy * P : c + dy * P;
                    for (int dx = -xm; dx <= xm; ++dx) {
                        const int id = row[dx];
                        if (id == 0) continue;
                        const int r2 = dx * dx + dy2;
                        if (id == id1) b1 = min(b1, r2);
                        else if (r2 < b1) { b2 = b1; id2 = id1; b1 = r2; id1 = id; }
                        else if (id == id2) b2 = min(b2, r2);
                        else if (r2 < b2) { b2 = r2; id2 = id; }
                    }
                }
            }
            if (b2 <= R2) {
                const double s = sqrt((double)b1) + sqrt((double)b2);
                o = (uint8_t)floor(20.0 * (1.0 + w0 * exp(-(s * s) / (2.0 * sigma * sigma))));
            }
        }
        out[(size_t)gy * W + gx] = o;
    }
}

// 0: refused
int radius_of(double w0, double sigma) {
    if (!(w0 > 0.0) || !(sigma > 0.0) || !(20.0 * (1.0 + w0) <= 255.0) || !isfinite(sigma)) return 0;
    if (20.0 * w0 <= 1.0) return 1;                            // the border term never reaches 1: any radius serves
    const double r = ceil(sigma * sqrt(2.0 * log(20.0 * w0)));
    return r < 1.0 ? 1 : (r > 1e6 ? 1000000 : (int)r);
}

}  // namespace

extern "C" int cdnet_weight_map_radius(double w0, double sigma) { return radius_of(w0, sigma); }

extern "C" int cdnet_weight_map(const int32_t *instances, int H, int W, double w0, double sigma, uint8_t *weight, void *stream) {
    CDNET_REQUIRE(instances && weight, "cdnet_weight_map: null pointer");
    CDNET_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL && cdiv(H, WM_TILE) <= 65535, "cdnet_weight_map: bad size %d x %d", H, W);
    CDNET_REQUIRE(w0 > 0.0 && sigma > 0.0 && isfinite(sigma), "cdnet_weight_map: w0 = %g and sigma = %g must be positive", w0, sigma);
    CDNET_REQUIRE(20.0 * (1.0 + w0) <= 255.0, "cdnet_weight_map: w0 = %g: the stored byte 20 * (1 + w0) would wrap past 255", w0);
    const int R = radius_of(w0, sigma);
    CDNET_REQUIRE(R >= 1 && R <= WM_MAX_R,
                  "cdnet_weight_map: search radius R = %d > %d (w0 = %g, sigma = %g): the LDS window of a %d x %d tile, (%d + 2 R)^2 * 4 B, "
                  "must fit the CU's 160 KB", R, WM_MAX_R, w0, sigma, WM_TILE, WM_TILE, WM_TILE);
    const int P = WM_TILE + 2 * R;
    return launch_lds<weight_map_kernel>(dim3(cdiv(W, WM_TILE), cdiv(H, WM_TILE)), dim3(WM_THREADS), WM_MAX_LDS, P * P * 4, (hipStream_t)stream,
                                         "cdnet_weight_map(LDS opt-in)", "cdnet_weight_map", instances, H, W, R, w0, sigma, weight);
}
