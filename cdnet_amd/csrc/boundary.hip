// Boundary and focal terms of the training loss (--boundary-loss 1|2|3) for gfx950 (wave64): value and gradient on the device.
//   kind 1  BoundaryLoss              <- loss.py:343-393 (theta0 = 3, theta = 5) fed the mask logits and the one-hot target (train_util_dam.py:195-199)
//   kind 2  FocalLoss2d               <- loss.py:37-78  (type 'sigmoid', gamma 2) fed the same two tensors (train_util_dam.py:200-203)
//   kind 3  RobustFocalLoss2d         <- loss.py:81-127: its clamp of (1 - pt)^2 to [0, 2] never binds for a probability; the same kernel as kind 2
//   their gradients                   <- autograd through F.max_pool2d (arg-max, first in raster order), softmax / sigmoid and clamp
// Launch plan, kind 1: bnd_sums (per-tile partials of the four sums per class) | bnd_grad (prologue: the sample's partials summed in a fixed
// order -> the per-class scalars; workgroup (0,0,0) also forms the loss and adds it to the total; then the tile's gradient).  With dmask NULL
// the second launch is that one workgroup.  kind 2 / 3: focal (value, gradient, per-workgroup partials) | focal_final (one workgroup).
// Reproducibility: every partial is a double written by one workgroup and summed in a fixed order; no atomics at all.
//
// kind 1 on a 32 x 32 tile.  With p the soft-max, t the one-hot target and every window clipped to the image:
//   pr_b = p - min3x3(p), pr_ext = max5x5(pr_b), gt_b = t - min3x3(t) (1 on a pixel of class c with a neighbour of another class: at most
//   ONE class per pixel has gt_b = 1, the pixel's own), gt_ext = max5x5(gt_b);
//   S1 = sum pr_b gt_ext, S2 = sum pr_b, S3 = sum pr_ext gt_b, S4 = sum gt_b;  P = S1 / (S2 + e), R = S3 / (S4 + e), BF1 = 2PR / (P + R + e).
// Backward as a gather: g[q] = dL/dpr_b[q] = a gt_ext[q] - b + r #{s in q's 5x5 : gt_b[s] and argmax5(s) == q},
//   dp[x] = g[x] - sum over q in x's 3x3 with argmin3(q) == x of g[q],  dz_k = p_k (dp_k - sum_j p_j dp_j).
// dz at a pixel reads p up to 6 pixels away (1 for the 3x3 scatter, 2 + 2 for the two 5x5 windows, 1 for pr_b) and labels up to 4 away.
// A label above 2 turns the sums that hold it into NaN (loss NaN, as cdnet_dam_loss); it matches no class and indexes nothing.
#include "common.h"

using namespace cdnet;

namespace {

constexpr int T = 32;                                 // tile side
constexpr int NT = 256;                               // threads per workgroup
constexpr int K = 3;
constexpr int NSUM = 4 * K;                           // S1..S4 per class
constexpr int RED = 16;                               // strides of the fixed-order sum over a sample's tiles
constexpr double EPS = 1e-7;
constexpr uint8_t NONE = 255;                         // label outside the image / no boundary here / no arg-min here
constexpr int FOCAL_PER = 1024;                       // elements per workgroup of the focal kernel

__device__ __forceinline__ bool inside(int y, int x, int H, int W) { return y >= 0 && y < H && x >= 0 && x < W; }

// labels of the tile with a halo of HL, NONE outside the image
template <int HL>
__device__ __forceinline__ void load_labels(const uint8_t *__restrict__ lab, int H, int W, int y0, int x0, uint8_t *s_lab) {
    constexpr int LW = T + 2 * HL;
    for (int i = threadIdx.x; i < LW * LW; i += NT) {
        const int y = y0 - HL + i / LW, x = x0 - HL + i % LW;
        s_lab[i] = inside(y, x, H, W) ? lab[(size_t)y * W + x] : NONE;
    }
}

// soft-max of the tile with a halo of HP, +inf outside the image (a minimum never takes it)
template <int HP>
__device__ __forceinline__ void load_softmax(const float *__restrict__ z, int H, int W, int y0, int x0, float *s_p) {
    constexpr int PW = T + 2 * HP;
    const size_t plane = (size_t)H * W;
    for (int i = threadIdx.x; i < PW * PW; i += NT) {
        const int y = y0 - HP + i / PW, x = x0 - HP + i % PW;
        float p[K] = {INFINITY, INFINITY, INFINITY};
        if (inside(y, x, H, W)) {
            float a[K];
#pragma unroll
            for (int c = 0; c < K; ++c) a[c] = z[c * plane + (size_t)y * W + x];
            mask_softmax<K>(a, p);
        }
#pragma unroll
        for (int c = 0; c < K; ++c) s_p[c * PW * PW + i] = p[c];
    }
}

// pr_b = p - min3x3(p) on the tile with a halo of HB (s_p has HB + 1), -inf outside the image (a maximum never takes it).  HA >= 0: also the
// position (0..8, row by row) of the FIRST minimum of the window for the pixels within HA of the tile, NONE outside the image.
template <int HB, int HA>
__device__ __forceinline__ void boundary_of_p(const float *s_p, int H, int W, int y0, int x0, float *s_prb, uint8_t *s_amin) {
    constexpr int BW = T + 2 * HB, PW = BW + 2, AW = T + 2 * HA;
    for (int i = threadIdx.x; i < BW * BW; i += NT) {
        const int by = i / BW, bx = i % BW;
        const bool in = inside(y0 - HB + by, x0 - HB + bx, H, W);
        const int ay = by - HB + HA, ax = bx - HB + HA;
        const bool keep = HA >= 0 && ay >= 0 && ay < AW && ax >= 0 && ax < AW;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const float *w = s_p + c * PW * PW + by * PW + bx;              // the window's first element
            float best = INFINITY;
            int idx = 0;
#pragma unroll
            for (int d = 0; d < 9; ++d) {
                const float v = w[(d / 3) * PW + d % 3];
                if (v < best) { best = v; idx = d; }
            }
            s_prb[c * BW * BW + i] = in ? w[PW + 1] - best : -INFINITY;
            if (keep) s_amin[c * AW * AW + ay * AW + ax] = in ? (uint8_t)idx : NONE;
        }
    }
}

// gt_b of the pixel at (ly, lx) of a label array of width LW (its 3x3 lies inside the array): the pixel's class when a neighbour inside the
// image has another one, NONE otherwise or when the label is no class
template <int LW>
__device__ __forceinline__ uint8_t boundary_of_t(const uint8_t *s_lab, int ly, int lx) {
    const uint8_t l = s_lab[ly * LW + lx];
    if (l >= K) return NONE;
    bool b = false;
#pragma unroll
    for (int d = 0; d < 9; ++d) {
        const uint8_t v = s_lab[(ly - 1 + d / 3) * LW + lx - 1 + d % 3];
        b |= v != NONE && v != l;
    }
    return b ? l : NONE;
}

// position (0..24, row by row) of the FIRST maximum of the 5x5 window of class c whose first element is w, and the maximum
template <int BW>
__device__ __forceinline__ int argmax5(const float *w, float *mx) {
    float best = -INFINITY;
    int idx = 0;
#pragma unroll
    for (int d = 0; d < 25; ++d) {
        const float v = w[(d / 5) * BW + d % 5];
        if (v > best) { best = v; idx = d; }
    }
    *mx = best;
    return idx;
}

// ---- pass 1: part[n][tile][c * 4 + k] = the tile's share of S_{k+1} of class c -------------------------------------------------
__global__ __launch_bounds__(NT) void bnd_sums_kernel(const float *__restrict__ logits, const uint8_t *__restrict__ label, int H, int W,
                                                      double *__restrict__ part) {
    constexpr int HP = 3, PW = T + 2 * HP, HB = 2, BW = T + 2 * HB, LW = T + 2 * 3;
    __shared__ float s_p[K * PW * PW];
    __shared__ float s_prb[K * BW * BW];
    __shared__ uint8_t s_lab[LW * LW];
    __shared__ uint8_t s_gtb[BW * BW];
    __shared__ double s_w[NT / WAVE][NSUM];
    const int n = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T, t = threadIdx.x;
    load_labels<3>(label + (size_t)n * H * W, H, W, y0, x0, s_lab);
    load_softmax<HP>(logits + (size_t)n * K * H * W, H, W, y0, x0, s_p);
    __syncthreads();
    boundary_of_p<HB, -1>(s_p, H, W, y0, x0, s_prb, nullptr);
    for (int i = t; i < BW * BW; i += NT) s_gtb[i] = boundary_of_t<LW>(s_lab, i / BW + 1, i % BW + 1);
    __syncthreads();
    double acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < T * T / NT; ++j) {
        const int ty = j * (NT / T) + t / T, tx = t % T;
        if (!inside(y0 + ty, x0 + tx, H, W)) continue;
        bad |= s_lab[(ty + 3) * LW + tx + 3] >= K;
        const uint8_t own = s_gtb[(ty + HB) * BW + tx + HB];
        bool ext[K] = {false, false, false};
#pragma unroll
        for (int d = 0; d < 25; ++d) {
            const uint8_t g = s_gtb[(ty + d / 5) * BW + tx + d % 5];
#pragma unroll
            for (int c = 0; c < K; ++c) ext[c] |= g == c;
        }
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const float b = s_prb[c * BW * BW + (ty + HB) * BW + tx + HB];
            if (ext[c]) acc[c * 4 + 0] += (double)b;
            acc[c * 4 + 1] += (double)b;
            if (own == c) {
                float mx;
                argmax5<BW>(s_prb + c * BW * BW + ty * BW + tx, &mx);
                acc[c * 4 + 2] += (double)mx;
                acc[c * 4 + 3] += 1.0;
            }
        }
    }
    bad = __syncthreads_or(bad);
#pragma unroll
    for (int k = 0; k < NSUM; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
        if ((t & 63) == 0) s_w[t >> 6][k] = acc[k];
    }
    __syncthreads();
    if (t < NSUM) {
        const double v = ((s_w[0][t] + s_w[1][t]) + s_w[2][t]) + s_w[3][t];
        const size_t tile = ((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part[tile * NSUM + t] = bad ? (double)NAN : v;
    }
}

// the NSUM sums of one sample from its tiles' partials, in a fixed order (RED strided chains, then the chains in order) -> s_sum[NSUM]
__device__ __forceinline__ void sample_sums(const double *__restrict__ part, int tiles, double *s_red, double *s_sum) {
    const int t = threadIdx.x;
    if (t < NSUM * RED) {
        const int k = t / RED;
        double a = 0.0;
        for (int i = t % RED; i < tiles; i += RED) a += part[(size_t)i * NSUM + k];
        s_red[t] = a;
    }
    __syncthreads();
    if (t < NSUM) {
        double a = 0.0;
        for (int j = 0; j < RED; ++j) a += s_red[t * RED + j];
        s_sum[t] = a;
    }
    __syncthreads();
}

// P, R, BF1 of one class and the scalars of g (a, b, r: see the head of the file); inv_bk = 1 / (B K)
__device__ __forceinline__ double f1_terms(const double *S, double inv_bk, double *coef) {
    const double P = S[0] / (S[1] + EPS), R = S[2] / (S[3] + EPS), D = P + R + EPS;
    const double gP = -inv_bk * 2.0 * R * (R + EPS) / (D * D), gR = -inv_bk * 2.0 * P * (P + EPS) / (D * D);
    coef[0] = gP / (S[1] + EPS);
    coef[1] = coef[0] * P;
    coef[2] = gR / (S[3] + EPS);
    return 2.0 * P * R / D;
}

// ---- pass 2: loss (workgroup (0,0,0)) and dmask += beta d loss / d logits on the tile ------------------------------------------
__global__ __launch_bounds__(NT) void bnd_grad_kernel(const float *__restrict__ logits, const uint8_t *__restrict__ label, int B, int H, int W,
                                                      const double *__restrict__ part, int tiles, float beta, float *__restrict__ loss_out,
                                                      float *__restrict__ total, float *__restrict__ dmask) {
    constexpr int HP = 6, PW = T + 2 * HP, HB = 5, BW = T + 2 * HB, HC = 3, CW = T + 2 * HC, HG = 1, GW = T + 2 * HG, HL = 4, LW = T + 2 * HL;
    __shared__ float s_p[K * PW * PW];
    __shared__ float s_prb[K * BW * BW];                  // pr_b, then g (K * GW * GW floats) in the same place
    __shared__ uint8_t s_amin[K * GW * GW];
    __shared__ uint8_t s_code[CW * CW];                   // where gt_b = 1: 32 * the pixel's class + its argmax5 position; NONE elsewhere
    __shared__ uint8_t s_lab[LW * LW];
    __shared__ double s_red[NSUM * RED];
    __shared__ double s_sum[NSUM];
    __shared__ double s_coef[K][3];
    static_assert(K * GW * GW <= K * BW * BW, "g lives in pr_b's array");
    const int n = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T, t = threadIdx.x;
    const double inv_bk = 1.0 / ((double)B * K);
    if (blockIdx.x == 0 && blockIdx.y == 0 && n == 0) {
        double sum = 0.0;                                 // (thread 0's) sum over (sample, class) of 1 - BF1, in that order
        for (int k = 0; k < B; ++k) {
            sample_sums(part + (size_t)k * tiles * NSUM, tiles, s_red, s_sum);
            if (t == 0) {
                double coef[3];
#pragma unroll
                for (int c = 0; c < K; ++c) sum += 1.0 - f1_terms(s_sum + c * 4, inv_bk, coef);
            }
            __syncthreads();
        }
        if (t == 0) {
            const float l = (float)(sum / ((double)B * K));
            *loss_out = l;
            if (total) *total = *total + beta * l;
        }
    }
    if (!dmask) return;
    sample_sums(part + (size_t)n * tiles * NSUM, tiles, s_red, s_sum);
    if (t < K) f1_terms(s_sum + t * 4, inv_bk, s_coef[t]);
    load_labels<HL>(label + (size_t)n * H * W, H, W, y0, x0, s_lab);
    load_softmax<HP>(logits + (size_t)n * K * H * W, H, W, y0, x0, s_p);
    __syncthreads();
    boundary_of_p<HB, HG>(s_p, H, W, y0, x0, s_prb, s_amin);
    __syncthreads();
    for (int i = t; i < CW * CW; i += NT) {
        const int cy = i / CW, cx = i % CW;
        const uint8_t c = boundary_of_t<LW>(s_lab, cy + HL - HC, cx + HL - HC);
        uint8_t code = NONE;
        if (c != NONE) {
            float mx;
            code = (uint8_t)(c * 32 + argmax5<BW>(s_prb + c * BW * BW + cy * BW + cx, &mx));       // (cy + HB - HC - 2 = cy)
        }
        s_code[i] = code;
    }
    __syncthreads();                                       // pr_b is consumed: g may overwrite it
    float *s_g = s_prb;
    for (int i = t; i < GW * GW; i += NT) {
        const int gy = i / GW, gx = i % GW;
        int cnt[K] = {0, 0, 0};
        bool ext[K] = {false, false, false};
        const bool in = inside(y0 - HG + gy, x0 - HG + gx, H, W);
        if (in) {
#pragma unroll
            for (int d = 0; d < 25; ++d) {
                // s = q + (d / 5 - 2, d % 5 - 2) chose q when its arg-max position is the mirrored one, 24 - d
                const uint8_t code = s_code[(gy + HC - HG - 2 + d / 5) * CW + gx + HC - HG - 2 + d % 5];
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const bool m = (code >> 5) == c;
                    ext[c] |= m;
                    cnt[c] += m && (code & 31) == 24 - d;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < K; ++c)
            s_g[c * GW * GW + i] = in ? (float)(s_coef[c][0] * (ext[c] ? 1.0 : 0.0) - s_coef[c][1] + s_coef[c][2] * (double)cnt[c]) : 0.0f;
    }
    __syncthreads();
    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int j = 0; j < T * T / NT; ++j) {
        const int ty = j * (NT / T) + t / T, tx = t % T;
        const int y = y0 + ty, x = x0 + tx;
        if (!inside(y, x, H, W)) continue;
        double dp[K], p[K], s = 0.0;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const float *g = s_g + c * GW * GW + ty * GW + tx;                   // the 3x3 around the pixel starts here
            const uint8_t *am = s_amin + c * GW * GW + ty * GW + tx;
            double a = (double)g[GW + 1];
#pragma unroll
            for (int d = 0; d < 9; ++d)
                if (am[(d / 3) * GW + d % 3] == 8 - d) a -= (double)g[(d / 3) * GW + d % 3];     // q's arg-min position of this pixel: mirrored
            dp[c] = a;
            p[c] = (double)s_p[c * PW * PW + (ty + HP) * PW + tx + HP];
            s += p[c] * a;
        }
#pragma unroll
        for (int c = 0; c < K; ++c) {
            float *q = dmask + ((size_t)n * K + c) * plane + (size_t)y * W + x;
            *q = *q + (float)((double)beta * (p[c] * (dp[c] - s)));
        }
    }
}

// ---- kinds 2 and 3: every logit element is one binary example ------------------------------------------------------------------
// pt, its clamp and (1 - pt)^2 in fp32 exactly as the reference's float32 run forms them (the saturated sigmoid makes the value depend on
// that: 1 - 1e-8 is 1 in fp32, and 1 - sigmoid is 0 from z = 17 on); the logarithm and the products in double.
__global__ __launch_bounds__(NT) void focal_kernel(const float *__restrict__ logits, const uint8_t *__restrict__ label, int plane, double scale,
                                                   float *__restrict__ dmask, double *__restrict__ part) {
    __shared__ double s_w[NT / WAVE];
    const int t = threadIdx.x, nc = blockIdx.y, n = nc / K, c = nc % K;
    double acc = 0.0;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < FOCAL_PER / NT; ++j) {
        const int i = blockIdx.x * FOCAL_PER + j * NT + t;
        if (i >= plane) continue;
        const uint8_t l = label[(size_t)n * plane + i];
        bad |= l >= K;
        const size_t e = (size_t)nc * plane + i;
        const float s = 1.0f / (1.0f + expf(-logits[e]));
        const float pt = l == c ? s : 1.0f - s;
        const bool in = pt >= 1e-8f;                       // the clamp's upper bound, 1 - 1e-8, is 1.0f: never exceeded
        const float ptc = in ? pt : 1e-8f, om = 1.0f - ptc, focus = om * om;
        const double lg = log((double)ptc);
        acc -= (double)focus * lg;
        if (dmask) {
            const double dpt = in ? 2.0 * (double)om * lg - (double)focus / (double)ptc : 0.0;
            const double ds = (double)s * (double)(1.0f - s);
            dmask[e] = dmask[e] + (float)(scale * (l == c ? dpt * ds : -dpt * ds));
        }
    }
    bad = __syncthreads_or(bad);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((t & 63) == 0) s_w[t >> 6] = acc;
    __syncthreads();
    if (t == 0) part[(size_t)nc * gridDim.x + blockIdx.x] = bad ? (double)NAN : ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// one workgroup: loss = (sum of the partials, NT strided chains, then the chains in order) / count
__global__ __launch_bounds__(NT) void focal_final_kernel(const double *__restrict__ part, int parts, double count, float beta,
                                                         float *__restrict__ loss_out, float *__restrict__ total) {
    __shared__ double s_red[NT];
    const int t = threadIdx.x;
    double a = 0.0;
    for (int i = t; i < parts; i += NT) a += part[i];
    s_red[t] = a;
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int j = 0; j < NT; ++j) sum += s_red[j];
        const float l = (float)(sum / count);
        *loss_out = l;
        if (total) *total = *total + beta * l;
    }
}

bool served(int kind, int B, int classes, int H, int W) {
    return kind >= 1 && kind <= 3 && classes == K && B > 0 && H > 0 && W > 0 && (size_t)H * W < (1u << 30) && (size_t)B * K <= 65535;
}

size_t ws_bytes(int kind, int B, int H, int W) {
    if (kind == 1) return (size_t)B * cdiv(H, T) * cdiv(W, T) * NSUM * sizeof(double);
    return (size_t)B * K * cdiv(H * W, FOCAL_PER) * sizeof(double);
}

}  // namespace

extern "C" size_t cdnet_boundary_loss_workspace_bytes(int kind, int B, int classes, int H, int W) {
    return served(kind, B, classes, H, W) ? ws_bytes(kind, B, H, W) : 0;
}

extern "C" int cdnet_boundary_loss_scratch_bytes(void) {
    hipFuncAttributes at;
    if (hipFuncGetAttributes(&at, reinterpret_cast<const void *>(bnd_grad_kernel)) != hipSuccess) return -1;
    return (int)at.localSizeBytes;
}

extern "C" int cdnet_boundary_loss(const float *mask_logits, const uint8_t *label, int kind, int B, int classes, int H, int W, float beta,
                                   void *workspace, size_t workspace_bytes, float *loss_out, float *total, float *dmask, void *stream) {
    CDNET_REQUIRE(mask_logits && label && workspace && loss_out, "cdnet_boundary_loss: null pointer");
    CDNET_REQUIRE(kind >= 1 && kind <= 3, "cdnet_boundary_loss: kind=%d not in {1,2,3}", kind);
    CDNET_REQUIRE(B > 0 && H > 0 && W > 0, "cdnet_boundary_loss: bad size B=%d H=%d W=%d", B, H, W);
    CDNET_REQUIRE(classes == K, "cdnet_boundary_loss: K=%d, the three-class mask only", classes);
    CDNET_REQUIRE(served(kind, B, classes, H, W), "cdnet_boundary_loss: B=%d H=%d W=%d too large for 32-bit pixel indices / the launch grid", B, H, W);
    CDNET_REQUIRE(((uintptr_t)workspace & 7) == 0, "cdnet_boundary_loss: workspace not 8-byte aligned");
    const size_t need = ws_bytes(kind, B, H, W);
    CDNET_REQUIRE(workspace_bytes >= need, "cdnet_boundary_loss: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)workspace;
    if (kind == 1) {
        const dim3 grid(cdiv(W, T), cdiv(H, T), B);
        const int tiles = (int)(grid.x * grid.y);
        bnd_sums_kernel<<<grid, NT, 0, st>>>(mask_logits, label, H, W, part);
        bnd_grad_kernel<<<dmask ? grid : dim3(1, 1, 1), NT, 0, st>>>(mask_logits, label, B, H, W, part, tiles, beta, loss_out, total, dmask);
    } else {
        const dim3 grid(cdiv(H * W, FOCAL_PER), B * K);
        const double count = (double)B * K * H * W;
        focal_kernel<<<grid, NT, 0, st>>>(mask_logits, label, H * W, (double)beta / count, dmask, part);
        focal_final_kernel<<<1, NT, 0, st>>>(part, (int)(grid.x * grid.y), count, beta, loss_out, total);
    }
    return check_launch("cdnet_boundary_loss");
}
