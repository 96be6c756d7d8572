// The optimisers on flat fp32 buffers (utils.py:907-939): the default Adam (adam_kernel: optimizer.step() of train_util_dam.py:308
// with utils.py:915-918), and the reference's other ones: RAdam, RAdam_4step, AdamW with warm-up
// (hhl_utils/radam.py:6-252), Ranger = RAdam + lookahead (hhl_utils/ranger.py:26-165) and torch.optim.SGD with momentum.
// Two streaming kernels for the latter: moment_kernel (the four moment rules) and sgd_kernel.  Every step-dependent coefficient is a host
// scalar (cdnet_amd/optim.py computes them in double like the reference's math.sqrt / ** and hands them over as float);
// the kernels branch on host scalars only.  16-byte loads and stores on the aligned body, scalar head and tail: a slice
// [a, b) of the flat buffers (bucket-wise stepping behind the all-reduce) starts at any 4-byte boundary.
// The operation order is the reference's (mul_ / addcmul_ / add_ / addcdiv_), no contraction (-ffp-contract=off).
#include "common.h"
#include "launch.h"
#include <math.h>

namespace {

using namespace cdnet;

struct MomentCoef {
    float b1, b2, omb1, omb2;      // beta, (float)(1 - beta) rounded from double as torch rounds its Python scalars
    float gscale, ndecay, nstep, vdiv, eps, alpha;
    int move, rect, sync;
};

__device__ __forceinline__ void moment_update(float &p, float g, float &m, float &v, float &s, const MomentCoef &c) {
    g = g * c.gscale;
    v = v * c.b2 + c.omb2 * (g * g);
    m = m * c.b1 + c.omb1 * g;
    if (c.move) {
        p = p + c.ndecay * p;                                      // decoupled decay: -weight_decay * lr_used
        if (c.rect) p = p + c.nstep * (m / (sqrtf(v) / c.vdiv + c.eps));
        else p = p + c.nstep * m;
    }
    if (c.sync) {                                                  // lookahead (ranger.py:160-163)
        s = s + c.alpha * (p - s);
        p = s;
    }
}

__global__ __launch_bounds__(256) void moment_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                     float *__restrict__ v, float *__restrict__ slow, size_t n, size_t head,
                                                     size_t nvec, MomentCoef c) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const bool touch_p = c.move || c.sync;                         // (a no-move step neither reads nor writes the parameters)
    float4 *p4 = (float4 *)(p + head), *m4 = (float4 *)(m + head), *v4 = (float4 *)(v + head);
    const float4 *g4 = (const float4 *)(g + head);
    float4 *s4 = c.sync ? (float4 *)(slow + head) : nullptr;
    for (size_t i = tid; i < nvec; i += stride) {
        const float4 gi = g4[i];
        float4 mi = m4[i], vi = v4[i];
        float4 pi = touch_p ? p4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 si = c.sync ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        moment_update(pi.x, gi.x, mi.x, vi.x, si.x, c);
        moment_update(pi.y, gi.y, mi.y, vi.y, si.y, c);
        moment_update(pi.z, gi.z, mi.z, vi.z, si.z, c);
        moment_update(pi.w, gi.w, mi.w, vi.w, si.w, c);
        m4[i] = mi; v4[i] = vi;
        if (touch_p) p4[i] = pi;
        if (c.sync) s4[i] = si;
    }
    // the unaligned head [0, head) and the tail [head + 4 nvec, n): at most 3 + 3 elements (all n of them when the buffers
    // do not share one alignment)
    const size_t body_end = head + 4 * nvec, nscalar = head + (n - body_end);
    for (size_t k = tid; k < nscalar; k += stride) {
        const size_t i = k < head ? k : body_end + (k - head);
        float pi = touch_p ? p[i] : 0.f, mi = m[i], vi = v[i], si = c.sync ? slow[i] : 0.f;
        moment_update(pi, g[i], mi, vi, si, c);
        m[i] = mi; v[i] = vi;
        if (touch_p) p[i] = pi;
        if (c.sync) slow[i] = si;
    }
}

struct SgdCoef {
    float gscale, wd, momentum, nlr;
    int first;
};

// torch.optim.SGD (dampening 0, no Nesterov): g += wd * p; buf = g on the first step, else momentum * buf + g; p -= lr * buf
__device__ __forceinline__ void sgd_update(float &p, float g, float &b, const SgdCoef &c) {
    g = g * c.gscale;
    g = g + c.wd * p;
    b = c.first ? g : b * c.momentum + g;
    p = p + c.nlr * b;
}

__global__ __launch_bounds__(256) void sgd_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ buf,
                                                  size_t n, size_t head, size_t nvec, SgdCoef c) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    float4 *p4 = (float4 *)(p + head), *b4 = (float4 *)(buf + head);
    const float4 *g4 = (const float4 *)(g + head);
    for (size_t i = tid; i < nvec; i += stride) {
        const float4 gi = g4[i];
        float4 pi = p4[i];
        float4 bi = c.first ? make_float4(0.f, 0.f, 0.f, 0.f) : b4[i];
        sgd_update(pi.x, gi.x, bi.x, c);
        sgd_update(pi.y, gi.y, bi.y, c);
        sgd_update(pi.z, gi.z, bi.z, c);
        sgd_update(pi.w, gi.w, bi.w, c);
        b4[i] = bi; p4[i] = pi;
    }
    const size_t body_end = head + 4 * nvec, nscalar = head + (n - body_end);
    for (size_t k = tid; k < nscalar; k += stride) {
        const size_t i = k < head ? k : body_end + (k - head);
        float pi = p[i], bi = c.first ? 0.f : buf[i];
        sgd_update(pi, g[i], bi, c);
        buf[i] = bi; p[i] = pi;
    }
}

// elements in front of the first 16-byte boundary when every buffer shares one alignment (slices of the flat buffers at
// one offset do); n otherwise: the scalar loop then covers everything
size_t scalar_head(size_t n, const void *const *ptrs, int count) {
    const uintptr_t a0 = (uintptr_t)ptrs[0] & 15;
    for (int k = 1; k < count; ++k)
        if (((uintptr_t)ptrs[k] & 15) != a0) return n;
    const size_t head = ((16 - a0) & 15) / 4;
    return head < n ? head : n;
}

bool aligned4(const void *const *ptrs, int count) {
    for (int k = 0; k < count; ++k)
        if ((uintptr_t)ptrs[k] & 3) return false;
    return true;
}

constexpr int STREAM_GRID_CAP = 2048;      // moment_kernel, sgd_kernel: 256 CUs x 8 workgroups, grid-stride beyond

// ======================================================================================================
// Adam (torch.optim.Adam semantics: L2 weight decay folded into the gradient, bias correction)
// ======================================================================================================
__global__ __launch_bounds__(256) void adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                   float *__restrict__ v, size_t n, float lr, float b1, float b2, float eps,
                                                   float wd, float bc1, float bc2_sqrt, float gscale) {
    const float step = lr / bc1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float gi = g[i] * gscale;
        const float pi = p[i];
        gi = fmaf(wd, pi, gi);
        float mi = m[i], vi = v[i];
        mi = mi + (gi - mi) * (1.f - b1);
        vi = vi * b2 + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = pi - step * (mi / denom);
    }
}

}  // namespace

extern "C" int cdnet_moment_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *slow, size_t n,
                                 double beta1, double beta2, float grad_scale, int move, int rect, float decay, float step_size,
                                 float v_div, float eps, int sync, float alpha, void *stream) {
    CDNET_REQUIRE(param && grad && exp_avg && exp_avg_sq, "cdnet_moment_step: null pointer");
    CDNET_REQUIRE(!sync || slow, "cdnet_moment_step: sync needs the slow buffer (null pointer)");
    CDNET_REQUIRE((move == 0 || move == 1) && (rect == 0 || rect == 1) && (sync == 0 || sync == 1),
                  "cdnet_moment_step: move / rect / sync must be 0 or 1");
    CDNET_REQUIRE(n <= ((size_t)1 << 40), "cdnet_moment_step: n=%zu out of range", n);
    CDNET_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "cdnet_moment_step: betas must lie in [0, 1)");
    CDNET_REQUIRE(v_div > 0.f && eps >= 0.f && alpha >= 0.f && alpha <= 1.f, "cdnet_moment_step: v_div=%g eps=%g alpha=%g", (double)v_div,
                  (double)eps, (double)alpha);
    const void *ptrs[5] = {param, grad, exp_avg, exp_avg_sq, slow};
    const int np = sync ? 5 : 4;
    CDNET_REQUIRE(aligned4(ptrs, np), "cdnet_moment_step: buffers must be 4-byte aligned");
    if (n == 0) return CDNET_OK;
    MomentCoef c;
    c.b1 = (float)beta1; c.b2 = (float)beta2; c.omb1 = (float)(1.0 - beta1); c.omb2 = (float)(1.0 - beta2);
    c.gscale = grad_scale; c.ndecay = -decay; c.nstep = -step_size; c.vdiv = v_div; c.eps = eps; c.alpha = alpha;
    c.move = move; c.rect = rect; c.sync = sync;
    const size_t head = scalar_head(n, ptrs, np), nvec = (n - head) / 4;
    moment_kernel<<<lin_grid(nvec, STREAM_GRID_CAP), 256, 0, (hipStream_t)stream>>>(param, grad, exp_avg, exp_avg_sq, sync ? slow : nullptr, n, head,
                                                                      nvec, c);
    return check_launch("cdnet_moment_step");
}

extern "C" int cdnet_sgd_step(float *param, const float *grad, float *momentum_buffer, size_t n, float lr, float momentum,
                              float weight_decay, int step, float grad_scale, void *stream) {
    CDNET_REQUIRE(param && grad && momentum_buffer, "cdnet_sgd_step: null pointer");
    CDNET_REQUIRE(step >= 1, "cdnet_sgd_step: step=%d is 1-based", step);
    CDNET_REQUIRE(n <= ((size_t)1 << 40), "cdnet_sgd_step: n=%zu out of range", n);
    CDNET_REQUIRE(momentum >= 0.f && weight_decay >= 0.f, "cdnet_sgd_step: momentum=%g weight_decay=%g", (double)momentum,
                  (double)weight_decay);
    const void *ptrs[3] = {param, grad, momentum_buffer};
    CDNET_REQUIRE(aligned4(ptrs, 3), "cdnet_sgd_step: buffers must be 4-byte aligned");
    if (n == 0) return CDNET_OK;
    SgdCoef c;
    c.gscale = grad_scale; c.wd = weight_decay; c.momentum = momentum; c.nlr = -lr; c.first = step == 1;
    const size_t head = scalar_head(n, ptrs, 3), nvec = (n - head) / 4;
    sgd_kernel<<<lin_grid(nvec, STREAM_GRID_CAP), 256, 0, (hipStream_t)stream>>>(param, grad, momentum_buffer, n, head, nvec, c);
    return check_launch("cdnet_sgd_step");
}

extern "C" int cdnet_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, float lr, float beta1,
                               float beta2, float eps, float weight_decay, int step, float grad_scale, void *stream) {
    CDNET_REQUIRE(param && grad && exp_avg && exp_avg_sq && step >= 1, "cdnet_adam_step: bad args");
    if (n == 0) return CDNET_OK;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    adam_kernel<<<lin_grid(n, 4096), 256, 0, (hipStream_t)stream>>>(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps,
                                                                    weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale);
    return check_launch("cdnet_adam_step");
}
