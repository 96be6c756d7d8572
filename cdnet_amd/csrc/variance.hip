// Instance variance loss of the training loop (--alpha 1) for gfx950 (wave64): value and gradient on the device.
//   labelling of the target   <- train_util_dam.py:176-178 (skimage.measure.label of target == 1, per sample, on the CPU)
//   LossVariance              <- loss.py:9-33 (a Python loop over the instances: unbiased variance of each channel's soft-max
//                                probabilities inside an instance, summed, / (instances + 1e-8), mean over the batch)
//   its gradient              <- autograd through loss.py:29 and F.softmax (train_util_dam.py:175)
// Launch plan (cdnet_variance_loss): memset of the accumulators | cc_init / cc_merge<8> / cc_flatten<FLAT_COUNT> of cc_forest.h over
// label == fg_value | var_sums | var_grad | var_final.
// Reproducibility: the per-instance sums of p are 64-bit FIXED POINT (p * 2^32 rounded) and the pixel counts integers, so their atomic adds are
// exact and order-free; the loss partials (one double per workgroup) are summed in a fixed order by one workgroup.  No float atomics.
// Cancellation: two passes - var_sums leaves sum(p) and n per instance, var_grad forms mu and sums (p - mu)^2 directly (never sum(p^2) - n mu^2);
// mu, the differences and the soft-max Jacobian are formed in double, p itself is the fp32 soft-max of mask_softmax.
// An instance's accumulator slot is the 2x2 cell of its root pixel: two pixels of one 2x2 cell are 8-connected, so a cell holds at most one
// root and ceil(H/2) * ceil(W/2) slots serve the worst case (a checkerboard of single pixels) without numbering the instances.
#include "cc_forest.h"

using namespace cdnet;

namespace {

constexpr int SLOT = 4;                               // u64 per slot: sum of p_c * 2^32 for c < K (K <= 3), pixel count in [3]
constexpr double FIX = 4294967296.0;                  // 2^32

__device__ __forceinline__ int slot_of(int root, int W, int Wh) { return ((root / W) >> 1) * Wh + ((root % W) >> 1); }

// sum(p_c) and n of every instance: one wave = 64 consecutive pixels of a row; the pixels of a row run share their root, so the wave forms
// the run sums from an inclusive scan (integers: exact) and the run head issues K + 1 integer atomics.
template <int K>
__global__ __launch_bounds__(256) void var_sums_kernel(const float *__restrict__ logits, const int *__restrict__ L, int H, int W,
                                                       unsigned long long *__restrict__ acc) {
    const int n = blockIdx.z, lane = threadIdx.x;
    const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + threadIdx.y;
    if (y >= H) return;                                   // whole wave exits together (y is wave-uniform)
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
    const int r = x < W ? L[(size_t)n * plane + pix] : -1;
    const unsigned long long bf = __ballot(r >= 0);
    if (!bf) return;
    unsigned long long v[K], inc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) v[c] = 0ull;
    if (r >= 0) {
        float a[K], p[K];
#pragma unroll
        for (int c = 0; c < K; ++c) a[c] = logits[((size_t)n * K + c) * plane + pix];
        mask_softmax<K>(a, p);
#pragma unroll
        for (int c = 0; c < K; ++c) v[c] = __double2ull_rn((double)p[c] * FIX);
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        inc[c] = v[c];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { unsigned long long t = __shfl_up(inc[c], o); if (lane >= o) inc[c] += t; }
    }
    const bool head = r >= 0 && (lane == 0 || !((bf >> (lane - 1)) & 1ull));
    const int len = run_length(bf, lane);                 // 0 off the mask
    const int end = (lane + len - 1) & 63;
    const int Wh = (W + 1) >> 1, Hh = (H + 1) >> 1;
    unsigned long long *slot = acc + ((size_t)n * Hh * Wh + (head ? slot_of(r, W, Wh) : 0)) * SLOT;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const unsigned long long e = __shfl(inc[c], end);  // every lane takes part in the shuffle
        if (head) atomicAdd(slot + c, e - (inc[c] - v[c]));
    }
    if (head) atomicAdd(slot + 3, (unsigned long long)len);
}

// per pixel of an instance with n > 1: d_c = p_c - mu_c; loss part sum_c d_c^2 / (n - 1); g_c = 2 d_c / ((n - 1) B (U + 1e-8));
// dmask_c += alpha p_c (g_c - sum_j p_j g_j).  part[workgroup] = the workgroup's loss part (unscaled), waves summed in wave order.
template <int K>
__global__ __launch_bounds__(256) void var_grad_kernel(const float *__restrict__ logits, const int *__restrict__ L, int B, int H, int W,
                                                       const unsigned long long *__restrict__ acc, const int *__restrict__ cnt, float alpha,
                                                       float *__restrict__ dmask, double *__restrict__ part) {
    __shared__ double s_w[4];
    const int n = blockIdx.z, lane = threadIdx.x;
    const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + threadIdx.y;
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
    const int r = (x < W && y < H) ? L[(size_t)n * plane + pix] : -1;
    double contrib = 0.0;
    if (r >= 0) {
        const int Wh = (W + 1) >> 1, Hh = (H + 1) >> 1;
        const unsigned long long *slot = acc + ((size_t)n * Hh * Wh + slot_of(r, W, Wh)) * SLOT;
        const long long cn = (long long)slot[3];
        if (cn > 1) {
            float a[K], p[K];
#pragma unroll
            for (int c = 0; c < K; ++c) a[c] = logits[((size_t)n * K + c) * plane + pix];
            mask_softmax<K>(a, p);
            const double inv = 1.0 / (double)(cn - 1);
            const double f = 2.0 * inv / ((double)B * ((double)cnt[n] + 1e-8));
            double g[K], s = 0.0;
#pragma unroll
            for (int c = 0; c < K; ++c) {
                const double mu = (double)slot[c] / FIX / (double)cn;
                const double d = (double)p[c] - mu;
                contrib += d * d;
                g[c] = d * f;
                s += (double)p[c] * g[c];
            }
            contrib *= inv;
            if (dmask) {
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    float *q = dmask + ((size_t)n * K + c) * plane + pix;
                    *q = *q + (float)((double)alpha * ((double)p[c] * (g[c] - s)));
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) contrib += __shfl_xor(contrib, o);
    if (lane == 0) s_w[threadIdx.y] = contrib;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0)
        part[((size_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// one workgroup: loss_var = sum_k (sum of sample k's partials) / (B (U_k + 1e-8)), every sum in a fixed order
__global__ __launch_bounds__(256) void var_final_kernel(const double *__restrict__ part, int per, int B, const int *__restrict__ cnt, float alpha,
                                                        float *__restrict__ loss_var, float *__restrict__ total, int32_t *__restrict__ counts) {
    __shared__ double s_w[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double loss = 0.0;
    for (int k = 0; k < B; ++k) {
        double a = 0.0;
        for (int i = t; i < per; i += 256) a += part[(size_t)k * per + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) s_w[w] = a;
        __syncthreads();
        if (t == 0) loss += (((s_w[0] + s_w[1]) + s_w[2]) + s_w[3]) / ((double)B * ((double)cnt[k] + 1e-8));
        __syncthreads();
    }
    if (t == 0) {
        const float lv = (float)loss;
        *loss_var = lv;
        if (total) *total = *total + alpha * lv;
    }
    if (counts)
        for (int k = t; k < B; k += 256) counts[k] = cnt[k];
}

// workspace: [accumulators u64 [B][slots][SLOT] | U_k i32 [B], padded to 16 bytes] (zeroed every call) | partials f64 | forest i32 [B][H][W]
size_t var_ws_layout(int B, int H, int W, size_t *o_cnt, size_t *o_part, size_t *o_L, size_t *zero_bytes) {
    const size_t slots = (size_t)((H + 1) / 2) * ((W + 1) / 2);
    size_t off = (size_t)B * slots * SLOT * sizeof(unsigned long long);
    *o_cnt = off;
    off += align_up((size_t)B * sizeof(int), 16);
    *zero_bytes = off;
    *o_part = off;
    off += align_up((size_t)B * cdiv(W, 64) * cdiv(H, 4) * sizeof(double), 16);
    *o_L = off;
    off += (size_t)B * H * W * sizeof(int);
    return off;
}

template <int K>
void var_launch(const float *logits, const int *L, int B, int H, int W, unsigned long long *acc, const int *cnt, float alpha, float *dmask,
                double *part, hipStream_t st) {
    const dim3 gr = grid_rows(B, H, W), br(64, 4);
    var_sums_kernel<K><<<gr, br, 0, st>>>(logits, L, H, W, acc);
    var_grad_kernel<K><<<gr, br, 0, st>>>(logits, L, B, H, W, acc, cnt, alpha, dmask, part);
}

}  // namespace

extern "C" size_t cdnet_variance_loss_workspace_bytes(int B, int K, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (K != 2 && K != 3) || (size_t)H * W >= (1u << 30)) return 0;
    size_t a, b, c, z;
    return var_ws_layout(B, H, W, &a, &b, &c, &z);
}

extern "C" int cdnet_variance_loss(const float *mask_logits, const uint8_t *label, int fg_value, int B, int K, int H, int W, float alpha,
                                   void *workspace, size_t workspace_bytes, float *loss_var, float *total, float *dmask,
                                   int32_t *root_out, int32_t *counts, void *stream) {
    CDNET_REQUIRE(mask_logits && label && workspace && loss_var, "cdnet_variance_loss: null pointer");
    CDNET_REQUIRE(B > 0 && H > 0 && W > 0, "cdnet_variance_loss: bad size B=%d H=%d W=%d", B, H, W);
    CDNET_REQUIRE(K == 2 || K == 3, "cdnet_variance_loss: K=%d not in {2,3}", K);
    CDNET_REQUIRE((size_t)H * W < (1u << 30), "cdnet_variance_loss: image too large for 32-bit pixel indices");
    CDNET_REQUIRE(((uintptr_t)workspace & 7) == 0, "cdnet_variance_loss: workspace not 8-byte aligned");
    size_t oCnt, oPart, oL, zero_bytes;
    const size_t need = var_ws_layout(B, H, W, &oCnt, &oPart, &oL, &zero_bytes);
    if (workspace_bytes < need) {
        set_error("cdnet_variance_loss: workspace %zu < %zu bytes", workspace_bytes, need);
        return CDNET_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    unsigned long long *acc = (unsigned long long *)ws;
    int *cnt = (int *)(ws + oCnt);
    double *part = (double *)(ws + oPart);
    int *L = root_out ? (int *)root_out : (int *)(ws + oL);          // the flattened forest IS the root map
    const dim3 gr = grid_rows(B, H, W), br(64, 4);
    if (hipMemsetAsync(ws, 0, zero_bytes, st) != hipSuccess) return check_launch("cdnet_variance_loss: memset");
    cc_init_kernel<2><<<gr, br, 0, st>>>(label, fg_value, H, W, L);
    cc_merge_kernel<2, 8><<<gr, br, 0, st>>>(label, fg_value, H, W, L);
    cc_flatten_kernel<FLAT_COUNT><<<gr, br, 0, st>>>(H, W, L, cnt);
    if (K == 2) var_launch<2>(mask_logits, L, B, H, W, acc, cnt, alpha, dmask, part, st);
    else var_launch<3>(mask_logits, L, B, H, W, acc, cnt, alpha, dmask, part, st);
    var_final_kernel<<<1, 256, 0, st>>>(part, (int)(gr.x * gr.y), B, cnt, alpha, loss_var, total, counts);
    return check_launch("cdnet_variance_loss");
}
