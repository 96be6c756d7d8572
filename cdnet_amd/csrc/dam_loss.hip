// The five-term CDNet loss with its gradient, and the per-sample sums of validate()'s loss mix (HBM-bound streaming kernels).
// Everything reduces through per-block partials that are summed in a fixed order, so a training step is bit-reproducible.
//
// Replaces, in the reference's train_util_dam.py:
//   loss terms :167-276 with loss.py:131-260 (dice / weighted cyclic dice), nn.NLLLoss(reduction='none') x weight map,
//   nn.MSELoss; the loss's own part of loss.backward() :307; the loss mix of validate() :499-580.
#include "loss_util.h"
#include "launch.h"
#include "stage16.h"

using namespace cdnet;

namespace {

// ======================================================================================================
// Loss (train_util_dam.py:167-276) - two passes over the logits
// ======================================================================================================
// per-sample sums (lsums<ND>() floats; ND = number of direction classes, 5 / 9 / 17 - options.py:45 "4 8 16" + background):
//   0..2  I_c   sum p_c [label==c]      3..5  P_c   sum p_c          6..8  T_c   sum [label==c]
//   PW+i  Pw_i  sum w q_i               TW+j  Tw_j sum w t_j
//   SS+j  S[j][j]  SN+j  S[next(j)][j]  SP+j  S[prev(j)][j]   (S[i][j] = sum w q_i t_j, j = target class)
//   SC+0 ce  +1 dce  +2 mse
//   SC+3 tp  +4 fp  +5 fn   of the pixel-level metric (argmax direction == 1 vs direction label == 1, train_util_dam.py:279-281)
// For ND = 9 this is the 60-float layout the first version fixed (PW 9, TW 18, SS 27, SN 36, SP 45, SC 54).
template <int ND> struct LossLay {
    static constexpr int PW = 9, TW = 9 + ND, SS = 9 + 2 * ND, SN = 9 + 3 * ND, SP = 9 + 4 * ND, SC = 9 + 5 * ND, SUMS = SC + 6;
    // coefficient block per sample: dice alpha[3], beta[3]; wdice: bsum[ND], a_self[ND], a_next[ND], a_prev[ND]
    //   a_self[j]  multiplies row i=j,        a_next[j] row i=next(j),  a_prev[j] row i=prev(j)  when the pixel's target is j
    static constexpr int COEF = 6 + 4 * ND;
    static constexpr int TPB = ND > 9 ? 128 : 256;      // reduce kernel: SUMS x TPB floats of LDS (<= 64 KB)
};
template <int ND> __device__ __forceinline__ int dnext(int i) { return i == ND - 1 ? 1 : i + 1; }      // cyclic over 1..ND-1 (loss.py:231-258)
template <int ND> __device__ __forceinline__ int dprev(int i) { return i == 1 ? ND - 1 : i - 1; }

struct LossIn {
    const float *mask, *point, *dirn;        // f32 NCHW logits [B][3][P], [B][1][P], [B][ND][P]
    const unsigned char *label, *dirlab;     // u8 [B][P]
    const unsigned short *point_t;           // f16 [B][P]
    const unsigned char *weight;             // u8 [B][P]  (png weight map; /20 on the fly)
    const int *single;                       // [B]: 1 if the sample's direction map is constant (train_util_dam.py:133,141)
    int B, P;
    int quirk0;                              // mask the direction one-hot with SAMPLE 0's foreground (:139)
    unsigned terms;                          // CDNET_LOSS_WMAP | CDNET_LOSS_CE | CDNET_LOSS_DICE (cdnet_dam_loss_terms)
};

// per sample: is the direction label constant (the one-hot of a single class, train_util_dam.py:131-137)?  The same scan
// validates the label content: a mask class > 2 or a direction class >= nd would index past the per-class accumulators, so
// it raises *err (the finalize kernel then poisons every loss with NaN - the reference's NLLLoss fails loudly on such targets)
// and the accumulation kernels clamp their indices.
// one workgroup of 1024 threads per sample, 16 label bytes per thread and load (the first version walked them a byte at a time with
// 256 threads: 64 us on the step's critical chain for 2 MB)
__global__ __launch_bounds__(1024) void loss_single_kernel(const unsigned char *dirlab, const unsigned char *label, int P, int nd, int *single, int *err) {
    __shared__ int s_min[16], s_max[16], s_lmax[16];
    const unsigned char *d = dirlab + (size_t)blockIdx.x * P;
    const unsigned char *l = label + (size_t)blockIdx.x * P;
    int mn = 255, mx = 0, lm = 0;
    const int tid = threadIdx.x;
    const bool vec = (P % 16 == 0) && ((reinterpret_cast<size_t>(d) | reinterpret_cast<size_t>(l)) % 16 == 0);
    if (vec) {
        const uint4 *d4 = reinterpret_cast<const uint4 *>(d), *l4 = reinterpret_cast<const uint4 *>(l);
        for (int i = tid; i < P / 16; i += 1024) {
            const uint4 dv = d4[i], lv = l4[i];
            const unsigned dw[4] = {dv.x, dv.y, dv.z, dv.w}, lw[4] = {lv.x, lv.y, lv.z, lv.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int b8 = 0; b8 < 4; ++b8) {
                    const int v = (dw[k] >> (8 * b8)) & 0xff, w = (lw[k] >> (8 * b8)) & 0xff;
                    mn = v < mn ? v : mn; mx = v > mx ? v : mx; lm = w > lm ? w : lm;
                }
        }
    } else {
        for (int i = tid; i < P; i += 1024) {
            int v = d[i]; mn = v < mn ? v : mn; mx = v > mx ? v : mx;
            v = l[i]; lm = v > lm ? v : lm;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int a = __shfl_xor(mn, m), b2 = __shfl_xor(mx, m), c = __shfl_xor(lm, m);
        mn = a < mn ? a : mn; mx = b2 > mx ? b2 : mx; lm = c > lm ? c : lm;
    }
    if ((tid & 63) == 0) { s_min[tid >> 6] = mn; s_max[tid >> 6] = mx; s_lmax[tid >> 6] = lm; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 16; ++i) {
            mn = s_min[i] < mn ? s_min[i] : mn; mx = s_max[i] > mx ? s_max[i] : mx; lm = s_lmax[i] > lm ? s_lmax[i] : lm;
        }
        single[blockIdx.x] = (mn == mx) ? 1 : 0;
        if (mx > nd - 1 || lm > 2) atomicOr(err, 1);
    }
}

// target class of the weighted dice for pixel i of sample b: -1 = all one-hot channels are zero
template <int ND>
__device__ __forceinline__ int dice_target(const LossIn &L, int b, int i) {
    if (L.single[b]) return 0;
    int t = L.dirlab[(size_t)b * L.P + i];
    t = t > ND - 1 ? ND - 1 : t;
    if (L.quirk0) return L.label[i] != 0 ? t : -1;               // sample 0's label
    return L.label[(size_t)b * L.P + i] != 0 ? t : -1;
}

// grid (chunks, B); private accumulators live in LDS ([k][tid]) because several are indexed by the target class
template <int ND>
__global__ __launch_bounds__(LossLay<ND>::TPB) void loss_reduce_kernel(LossIn L, float *__restrict__ partial) {
    using Y = LossLay<ND>;
    constexpr int TPB = Y::TPB;
    __shared__ float acc[Y::SUMS][TPB];
    const int tid = threadIdx.x, b = blockIdx.y;
#pragma unroll
    for (int k = 0; k < Y::SUMS; ++k) acc[k][tid] = 0.f;
    const size_t ob = (size_t)b * L.P;
    for (int i = blockIdx.x * TPB + tid; i < L.P; i += gridDim.x * TPB) {
        float l3[3], p3[3], lp3[3], l9[ND], p9[ND], lp9[ND];
#pragma unroll
        for (int c = 0; c < 3; ++c) l3[c] = L.mask[((size_t)b * 3 + c) * L.P + i];
#pragma unroll
        for (int c = 0; c < ND; ++c) l9[c] = L.dirn[((size_t)b * ND + c) * L.P + i];
        softmax3(l3, p3, lp3);
        softmax_n<ND>(l9, p9, lp9);
        const float w = (L.terms & CDNET_LOSS_WMAP) ? (float)L.weight[ob + i] / 20.f : 1.f;      // clear: both CE maps and the dice sums unweighted
        int lab = L.label[ob + i], dl = L.dirlab[ob + i];
        lab = lab > 2 ? 2 : lab; dl = dl > ND - 1 ? ND - 1 : dl;   // (out-of-range content is reported through *err, see loss_single_kernel)
        acc[lab][tid] += p3[lab];
        acc[6 + lab][tid] += 1.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[3 + c][tid] += p3[c];
#pragma unroll
        for (int c = 0; c < ND; ++c) acc[Y::PW + c][tid] = fmaf(w, p9[c], acc[Y::PW + c][tid]);
        const int t = dice_target<ND>(L, b, i);
        if (t >= 0) {
            acc[Y::TW + t][tid] += w;
            acc[Y::SS + t][tid] = fmaf(w, p9[t], acc[Y::SS + t][tid]);
            if (t >= 1) {
                acc[Y::SN + t][tid] = fmaf(w, p9[dnext<ND>(t)], acc[Y::SN + t][tid]);
                acc[Y::SP + t][tid] = fmaf(w, p9[dprev<ND>(t)], acc[Y::SP + t][tid]);
            }
        }
        acc[Y::SC][tid] -= lp3[lab] * w;
        acc[Y::SC + 1][tid] -= lp9[dl] * w;
        const float dpt = L.point[ob + i] - h2f(L.point_t[ob + i]);
        acc[Y::SC + 2][tid] = fmaf(dpt, dpt, acc[Y::SC + 2][tid]);
        {   // np.argmax over the direction classes (first maximum), "inside" = class 1 (utils.py:76-78)
            int am = 0;
            float best = l9[0];
#pragma unroll
            for (int c = 1; c < ND; ++c) if (l9[c] > best) { best = l9[c]; am = c; }
            const bool pi = am == 1, ti = dl == 1;
            if (pi && ti) acc[Y::SC + 3][tid] += 1.f;
            if (pi && !ti) acc[Y::SC + 4][tid] += 1.f;
            if (!pi && ti) acc[Y::SC + 5][tid] += 1.f;
        }
    }
    __syncthreads();
    row_sum<TPB>(acc, tid, b, partial);
}

// single block: per-sample sums -> loss terms (5 + total) and the pass-2 coefficients
template <int ND>
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float *__restrict__ partial, int nchunk, int B, int P,
                                                            float *__restrict__ sums, float *__restrict__ coef,
                                                            float *__restrict__ losses, const int *__restrict__ err, unsigned terms) {
    using Y = LossLay<ND>;
    constexpr int NS = Y::SUMS;
    // WMAP clear (train_util_dam.py:241-244): the direction dice is the plain MulticlassDiceLoss over the ND classes - a sum over the
    // classes of the (i, i) ratios, no / ND, no doubled class 0, no neighbour terms - of the sums the reduce kernel took with w = 1
    const bool plain = !(terms & CDNET_LOSS_WMAP);
    __shared__ float s_sum[64 * NS];      // B <= 64
    const int tid = threadIdx.x;
    for (int idx = tid; idx < B * NS; idx += 256) {
        const int b = idx / NS, k = idx % NS;
        const float s = chunk_sum<NS>(partial + (size_t)b * nchunk * NS + k, nchunk);
        s_sum[idx] = s;
        if (sums) sums[idx] = s;
    }
    __syncthreads();
    const float fB = (float)B;
    for (int b = tid; b < B; b += 256) {
        const float *S = s_sum + b * NS;
        float *cf = coef + (size_t)b * Y::COEF;
        mask_dice_coef(S, fB, cf);
        // row i, column j terms: alpha_ij = -2/(B (U_ij+1)), beta_ij = 2 (S_ij+1)/(B (U_ij+1)^2), U_ij = Pw_i + Tw_j
        float bsum[ND];
        for (int i = 0; i < ND; ++i) bsum[i] = 0.f;
        for (int j = 0; j < ND; ++j) {
            {   // (i=j, j)
                const float U = S[Y::PW + j] + S[Y::TW + j], Sij = S[Y::SS + j], m = j == 0 && !plain ? 2.f : 1.f;
                cf[6 + ND + j] = m * -2.f / (fB * (U + 1.f));
                bsum[j] += m * 2.f * (Sij + 1.f) / (fB * (U + 1.f) * (U + 1.f));
            }
            if (plain) { cf[6 + 2 * ND + j] = 0.f; cf[6 + 3 * ND + j] = 0.f; }
            else if (j >= 1) {
                const int in = dnext<ND>(j), ip = dprev<ND>(j);
                {   const float U = S[Y::PW + in] + S[Y::TW + j], Sij = S[Y::SN + j];
                    cf[6 + 2 * ND + j] = -2.f / (fB * (U + 1.f));
                    bsum[in] += 2.f * (Sij + 1.f) / (fB * (U + 1.f) * (U + 1.f)); }
                {   const float U = S[Y::PW + ip] + S[Y::TW + j], Sij = S[Y::SP + j];
                    cf[6 + 3 * ND + j] = -2.f / (fB * (U + 1.f));
                    bsum[ip] += 2.f * (Sij + 1.f) / (fB * (U + 1.f) * (U + 1.f)); }
            } else { cf[6 + 2 * ND] = 0.f; cf[6 + 3 * ND] = 0.f; }
        }
        for (int i = 0; i < ND; ++i) cf[6 + i] = bsum[i];
    }
    // the 3 ND + 1 batch-mean dice ratios, one thread each (they were ~450 serial divisions on thread 0):
    // [0,3) mask dice c; [3,3+ND) wdice(i,i); then wdice(i,prev(i)), i=1..ND-1; then wdice(i,next(i)), i=1..ND-1
    constexpr int T_PREV = 3 + ND, T_NEXT = T_PREV + ND - 1, NT = T_NEXT + ND - 1;
    __shared__ float s_term[NT];
    if (tid < NT) {
        int num, da, db;                      // mean_b 2 (S[num] + 1) / (S[da] + S[db] + 1)
        if (tid < 3) { num = tid; da = 3 + tid; db = 6 + tid; }
        else if (tid < T_PREV) { const int i = tid - 3; num = Y::SS + i; da = Y::PW + i; db = Y::TW + i; }
        else if (tid < T_NEXT) { const int i = tid - T_PREV + 1, j = dprev<ND>(i); num = Y::SN + j; da = Y::PW + i; db = Y::TW + j; }
        else { const int i = tid - T_NEXT + 1, j = dnext<ND>(i); num = Y::SP + j; da = Y::PW + i; db = Y::TW + j; }
        s_term[tid] = dice_term<NS>(s_sum, B, fB, num, da, db);
    }
    __syncthreads();
    if (tid == 0) {
        const float n = (float)B * (float)P;
        float ce = 0.f, dce = 0.f, mse = 0.f;
        for (int b = 0; b < B; ++b) { ce += s_sum[b * NS + Y::SC]; dce += s_sum[b * NS + Y::SC + 1]; mse += s_sum[b * NS + Y::SC + 2]; }
        ce /= n; dce /= n; mse /= n;
        float dice = 0.f;
        for (int c = 0; c < 3; ++c) dice += s_term[c];
        float wd = 0.f;
        for (int i = 0; i < ND; ++i) {
            if (i == 0) wd += 2.f * s_term[3];
            else wd += s_term[3 + i] - (1.f - s_term[T_PREV + i - 1]) - (1.f - s_term[T_NEXT + i - 1]);
        }
        wd /= (float)ND;
        if (plain) {
            wd = 0.f;
            for (int i = 0; i < ND; ++i) wd += s_term[3 + i];
        }
        losses[0] = (terms & CDNET_LOSS_CE) ? ce + dice + dce + wd + mse : dice + dce + wd + mse;
        losses[1] = dce; losses[2] = wd; losses[3] = mse; losses[4] = ce; losses[5] = dice;
        pixel_metrics<NS>(s_sum, Y::SC + 3, B, P, losses + 6);
        poison_on_error(err, losses, 11);
    }
}

// pass 2: gradients w.r.t. the logits (f32 NCHW, same layout as the logits)
template <int ND>
__global__ __launch_bounds__(256) void loss_grad_kernel(LossIn L, const float *__restrict__ coef, float *__restrict__ dmask,
                                                        float *__restrict__ dpoint, float *__restrict__ ddir) {
    const int b = blockIdx.y;
    const float *cf = coef + (size_t)b * LossLay<ND>::COEF;
    const float inv_n = 1.f / ((float)L.B * (float)L.P);
    const size_t ob = (size_t)b * L.P;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < L.P; i += gridDim.x * 256) {
        float l3[3], p3[3], lp3[3], l9[ND], p9[ND], lp9[ND];
#pragma unroll
        for (int c = 0; c < 3; ++c) l3[c] = L.mask[((size_t)b * 3 + c) * L.P + i];
#pragma unroll
        for (int c = 0; c < ND; ++c) l9[c] = L.dirn[((size_t)b * ND + c) * L.P + i];
        softmax3(l3, p3, lp3);
        softmax_n<ND>(l9, p9, lp9);
        const float w = (L.terms & CDNET_LOSS_WMAP) ? (float)L.weight[ob + i] / 20.f : 1.f;      // clear: both CE maps and the dice sums unweighted
        int lab = L.label[ob + i], dl = L.dirlab[ob + i];
        lab = lab > 2 ? 2 : lab; dl = dl > ND - 1 ? ND - 1 : dl;   // (out-of-range content is reported through *err, see loss_single_kernel)
        // mask: dice gradient w.r.t. probabilities, through the softmax, plus the weighted CE
        float gp[3], dot = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { gp[c] = cf[3 + c] + (c == lab ? cf[c] : 0.f); dot = fmaf(p3[c], gp[c], dot); }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            dmask[((size_t)b * 3 + c) * L.P + i] = (L.terms & CDNET_LOSS_CE) ? p3[c] * (gp[c] - dot) + w * inv_n * (p3[c] - (c == lab ? 1.f : 0.f))
                                                                              : p3[c] * (gp[c] - dot);
        // direction: weighted cyclic dice (average over the ND classes) + weighted CE
        const int t = dice_target<ND>(L, b, i);
        float gq[ND], dotq = 0.f;
#pragma unroll
        for (int c = 0; c < ND; ++c) gq[c] = cf[6 + c];
        if (t >= 0) {
#pragma unroll
            for (int c = 0; c < ND; ++c) {
                float a = 0.f;
                if (c == t) a = cf[6 + ND + t];
                else if (t >= 1 && c == dnext<ND>(t)) a = cf[6 + 2 * ND + t];
                else if (t >= 1 && c == dprev<ND>(t)) a = cf[6 + 3 * ND + t];
                gq[c] += a;
            }
        }
#pragma unroll
        for (int c = 0; c < ND; ++c) { if (L.terms & CDNET_LOSS_WMAP) gq[c] *= w * (1.f / (float)ND); dotq = fmaf(p9[c], gq[c], dotq); }
#pragma unroll
        for (int c = 0; c < ND; ++c)
            ddir[((size_t)b * ND + c) * L.P + i] = p9[c] * (gq[c] - dotq) + w * inv_n * (p9[c] - (c == dl ? 1.f : 0.f));
        if (dpoint) dpoint[ob + i] = 2.f * inv_n * (L.point[ob + i] - h2f(L.point_t[ob + i]));
    }
}

// ======================================================================================================
// validate() loss mix (train_util_dam.py:499-580) - per-sample sums, one pass over the logits.  The host combines them:
//   0..2 I_c = sum p_c [label==c]   3..5 P_c = sum p_c   6..8 T_c = sum [label==c]   9 sum -log p_label (UNweighted, :499-505)
//   10..18 Iq_i = sum q'_i t_i   19..27 Pq_i = sum q'_i   28..36 Tq_i = sum t_i   with q' = softmax(direction), q'_0 *= p_0 (:564-566)
//            and t = one-hot of the direction class RANK (lut) masked by SAMPLE 0's foreground (:463-470)
//   37 sum w * -log q_dir (:553-559)   38 sum (point - target / 255)^2 (:575-580)
//   39 tp  40 fp  41 fn  of (argmax mask == 1) vs (label == 1)  (utils.accuracy_pixel_level, :585-590)
// ======================================================================================================
// For ND direction classes (5 / 9 / 17) the three direction blocks are ND wide: IQ = 10, PQ = 10 + ND, TQ = 10 + 2 ND, then the five
// scalars at VS = 10 + 3 ND (42 floats for ND = 9, the layout above).
template <int ND> struct ValLay {
    static constexpr int IQ = 10, PQ = 10 + ND, TQ = 10 + 2 * ND, VS = 10 + 3 * ND, SUMS = VS + 5;
    static constexpr int TPB = ND > 9 ? 128 : 256;
};
static_assert(ValLay<9>::SUMS == CDNET_VAL_SUMS, "cdnet_dam_val_sums row layout");

struct ValIn {
    const float *mask, *point, *dirn;
    const unsigned char *label, *dirlab, *weight;
    const unsigned short *point_t;
    int lut[17];                             // direction class value -> channel (rank among the batch's unique values), -1 = absent
    int B, P;
};

template <int ND>
__global__ __launch_bounds__(ValLay<ND>::TPB) void val_sums_kernel(ValIn L, float *__restrict__ partial) {
    using Y = ValLay<ND>;
    constexpr int TPB = Y::TPB;
    __shared__ float acc[Y::SUMS][TPB];
    const int tid = threadIdx.x, b = blockIdx.y;
#pragma unroll
    for (int k = 0; k < Y::SUMS; ++k) acc[k][tid] = 0.f;
    const size_t ob = (size_t)b * L.P;
    for (int i = blockIdx.x * TPB + tid; i < L.P; i += gridDim.x * TPB) {
        float l3[3], p3[3], lp3[3], l9[ND], p9[ND], lp9[ND];
#pragma unroll
        for (int c = 0; c < 3; ++c) l3[c] = L.mask[((size_t)b * 3 + c) * L.P + i];
#pragma unroll
        for (int c = 0; c < ND; ++c) l9[c] = L.dirn[((size_t)b * ND + c) * L.P + i];
        softmax3(l3, p3, lp3);
        softmax_n<ND>(l9, p9, lp9);
        int lab = L.label[ob + i], dl = L.dirlab[ob + i];
        lab = lab > 2 ? 2 : lab; dl = dl > ND - 1 ? ND - 1 : dl;
        const float w = (float)L.weight[ob + i] / 20.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[3 + c][tid] += p3[c];
            if (c == lab) { acc[c][tid] += p3[c]; acc[6 + c][tid] += 1.f; }
        }
        acc[9][tid] -= lp3[lab];
        p9[0] *= p3[0];
        const bool fg0 = L.label[i] != 0;                     // sample 0's foreground (the reference indexes target[0])
        const int tch = (fg0 && L.lut[dl] >= 0) ? L.lut[dl] : -1;
#pragma unroll
        for (int c = 0; c < ND; ++c) {
            acc[Y::PQ + c][tid] += p9[c];
            if (c == tch) { acc[Y::IQ + c][tid] += p9[c]; acc[Y::TQ + c][tid] += 1.f; }
        }
        acc[Y::VS][tid] -= w * lp9[dl];
        const float dpt = L.point[ob + i] - h2f(L.point_t[ob + i]) / 255.f;
        acc[Y::VS + 1][tid] = fmaf(dpt, dpt, acc[Y::VS + 1][tid]);
        int am = 0;                                            // np.argmax: first maximum
        if (l3[1] > l3[am]) am = 1;
        if (l3[2] > l3[am]) am = 2;
        const bool pi = am == 1, ti = lab == 1;
        if (pi && ti) acc[Y::VS + 2][tid] += 1.f;
        if (pi && !ti) acc[Y::VS + 3][tid] += 1.f;
        if (!pi && ti) acc[Y::VS + 4][tid] += 1.f;
    }
    __syncthreads();
    row_sum<TPB>(acc, tid, b, partial);
}

// sums[b][k] = sum over chunks, fixed order
__global__ void val_sums_reduce_kernel(const float *__restrict__ partial, int nchunk, int B, int nsums, float *__restrict__ sums) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * nsums) return;
    const int b = idx / nsums, k = idx % nsums;
    double s = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) s += (double)partial[((size_t)b * nchunk + ch) * nsums + k];
    sums[idx] = (float)s;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------
// the workspace queries are reachable before any validation: a count other than 5 / 9 / 17 gets the 9-class answer
static int known_classes(int direction_classes) { return direction_classes == 5 || direction_classes == 17 ? direction_classes : 9; }

template <int ND>
static size_t dam_loss_ws(int B, int P) {
    using Y = LossLay<ND>;
    const int nchunk = loss_nchunk(P, Y::TPB);
    return (size_t)B * nchunk * Y::SUMS + (size_t)B * Y::COEF + (size_t)B * Y::SUMS + 16 + (size_t)B;   // partial | coef | sums | pad | single(int)
}

template <int ND>
static int dam_loss_impl(LossIn L, int B, int P, float *workspace, float *losses, float *dmask, float *dpoint, float *ddir, hipStream_t st) {
    using Y = LossLay<ND>;
    const int nchunk = loss_nchunk(P, Y::TPB);
    float *partial = workspace;
    float *coef = partial + (size_t)B * nchunk * Y::SUMS;
    float *sums = coef + (size_t)B * Y::COEF;
    int *err = reinterpret_cast<int *>(sums + (size_t)B * Y::SUMS);          // first word of the 16-float pad
    int *single = reinterpret_cast<int *>(sums + (size_t)B * Y::SUMS + 16);
    if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) return check_launch("cdnet_dam_loss(memset)");
    L.single = single;
    loss_single_kernel<<<B, 1024, 0, st>>>(L.dirlab, L.label, P, ND, single, err);
    loss_reduce_kernel<ND><<<dim3(nchunk, B), Y::TPB, 0, st>>>(L, partial);
    loss_finalize_kernel<ND><<<1, 256, 0, st>>>(partial, nchunk, B, P, sums, coef, losses, err, L.terms);
    if (dmask) loss_grad_kernel<ND><<<dim3(lin_grid((size_t)P, 256), B), 256, 0, st>>>(L, coef, dmask, dpoint, ddir);
    return check_launch("cdnet_dam_loss");
}

extern "C" size_t cdnet_dam_loss_classes_workspace_floats(int B, int P, int direction_classes) {
    size_t n = 0;
    with_int<5, 9, 17>(known_classes(direction_classes), [&](auto nd) { n = dam_loss_ws<decltype(nd)::value>(B, P); return CDNET_OK; });
    return n;
}
extern "C" size_t cdnet_dam_loss_workspace_floats(int B, int P) { return dam_loss_ws<9>(B, P); }

extern "C" int cdnet_dam_loss_terms(const float *mask, const float *point, const float *dirn, const uint8_t *label, const uint8_t *dirlab,
                                    const uint16_t *point_target_f16, const uint8_t *weight_u8, int B, int H, int W, int direction_classes,
                                    int quirk_sample0, float *workspace, size_t workspace_floats, float *losses, float *dmask,
                                    float *dpoint, float *ddir, void *stream, unsigned terms) {
    CDNET_REQUIRE(mask && point && dirn && label && dirlab && point_target_f16 && workspace && losses, "cdnet_dam_loss: null pointer");
    CDNET_REQUIRE((terms & ~(CDNET_LOSS_WMAP | CDNET_LOSS_CE | CDNET_LOSS_DICE)) == 0, "cdnet_dam_loss: terms %u has unknown bits", terms);
    CDNET_REQUIRE(terms & CDNET_LOSS_DICE, "cdnet_dam_loss: the DAM loss has no configuration without the dice terms (train_util_dam.py:297)");
    CDNET_REQUIRE(weight_u8 || !(terms & CDNET_LOSS_WMAP), "cdnet_dam_loss: CDNET_LOSS_WMAP needs the weight map");
    CDNET_REQUIRE(B >= 1 && B <= 64 && H > 0 && W > 0, "cdnet_dam_loss: batch %d not in [1,64]", B);
    CDNET_REQUIRE(direction_classes == 5 || direction_classes == 9 || direction_classes == 17,
                  "cdnet_dam_loss: direction_classes %d must be 5, 9 or 17 (options.py:45)", direction_classes);
    const int P = H * W;
    if (workspace_floats < cdnet_dam_loss_classes_workspace_floats(B, P, direction_classes)) { set_error("cdnet_dam_loss: workspace too small"); return CDNET_E_WORKSPACE; }
    CDNET_REQUIRE((dmask != nullptr) == (dpoint != nullptr) && (dmask != nullptr) == (ddir != nullptr),
                  "cdnet_dam_loss: all three gradient outputs or none");      // (dpoint or ddir alone used to be taken as none, silently)
    LossIn L;
    L.mask = mask; L.point = point; L.dirn = dirn; L.label = label; L.dirlab = dirlab; L.point_t = point_target_f16;
    L.weight = weight_u8; L.single = nullptr; L.B = B; L.P = P; L.quirk0 = quirk_sample0; L.terms = terms;
    hipStream_t st = (hipStream_t)stream;
    return with_int<5, 9, 17>(direction_classes, [&](auto nd) { return dam_loss_impl<decltype(nd)::value>(L, B, P, workspace, losses, dmask, dpoint, ddir, st); });
}

extern "C" int cdnet_dam_loss_classes(const float *mask, const float *point, const float *dirn, const uint8_t *label, const uint8_t *dirlab,
                                      const uint16_t *point_target_f16, const uint8_t *weight_u8, int B, int H, int W, int direction_classes,
                                      int quirk_sample0, float *workspace, size_t workspace_floats, float *losses, float *dmask,
                                      float *dpoint, float *ddir, void *stream) {
    CDNET_REQUIRE(weight_u8, "cdnet_dam_loss: null pointer");
    return cdnet_dam_loss_terms(mask, point, dirn, label, dirlab, point_target_f16, weight_u8, B, H, W, direction_classes, quirk_sample0,
                                workspace, workspace_floats, losses, dmask, dpoint, ddir, stream,
                                CDNET_LOSS_WMAP | CDNET_LOSS_CE | CDNET_LOSS_DICE);
}

extern "C" int cdnet_dam_loss(const float *mask, const float *point, const float *dirn, const uint8_t *label, const uint8_t *dirlab,
                              const uint16_t *point_target_f16, const uint8_t *weight_u8, int B, int H, int W, int quirk_sample0,
                              float *workspace, size_t workspace_floats, float *losses, float *dmask, float *dpoint, float *ddir,
                              void *stream) {
    return cdnet_dam_loss_classes(mask, point, dirn, label, dirlab, point_target_f16, weight_u8, B, H, W, 9, quirk_sample0, workspace,
                                  workspace_floats, losses, dmask, dpoint, ddir, stream);
}

template <int ND>
static int val_sums_impl(ValIn L, int B, int P, float *workspace, float *sums, hipStream_t st) {
    using Y = ValLay<ND>;
    const int nchunk = loss_nchunk(P, Y::TPB);
    val_sums_kernel<ND><<<dim3(nchunk, B), Y::TPB, 0, st>>>(L, workspace);
    val_sums_reduce_kernel<<<cdiv(B * Y::SUMS, 256), 256, 0, st>>>(workspace, nchunk, B, Y::SUMS, sums);
    return check_launch("cdnet_dam_val_sums");
}

extern "C" size_t cdnet_dam_val_sums_classes_workspace_floats(int B, int P, int direction_classes) {
    size_t n = 0;
    with_int<5, 9, 17>(known_classes(direction_classes), [&](auto nd) {
        using Y = ValLay<decltype(nd)::value>;
        n = (size_t)B * loss_nchunk(P, Y::TPB) * Y::SUMS;
        return CDNET_OK;
    });
    return n;
}
extern "C" size_t cdnet_dam_val_sums_workspace_floats(int B, int P) { return cdnet_dam_val_sums_classes_workspace_floats(B, P, 9); }

extern "C" int cdnet_dam_val_sums_classes(const float *mask, const float *point, const float *dirn, const uint8_t *label, const uint8_t *dirlab,
                                          const uint16_t *point_target_f16, const uint8_t *weight_u8, const int *dir_rank_host,
                                          int direction_classes, int B, int H, int W, float *workspace, size_t workspace_floats, float *sums,
                                          void *stream) {
    CDNET_REQUIRE(mask && point && dirn && label && dirlab && point_target_f16 && weight_u8 && dir_rank_host && workspace && sums,
                  "cdnet_dam_val_sums: null pointer");
    CDNET_REQUIRE(B >= 1 && B <= 64 && H > 0 && W > 0, "cdnet_dam_val_sums: batch %d not in [1,64]", B);
    CDNET_REQUIRE(direction_classes == 5 || direction_classes == 9 || direction_classes == 17,
                  "cdnet_dam_val_sums: direction_classes %d must be 5, 9 or 17 (options.py:45)", direction_classes);
    const int P = H * W;
    if (workspace_floats < cdnet_dam_val_sums_classes_workspace_floats(B, P, direction_classes)) { set_error("cdnet_dam_val_sums: workspace too small"); return CDNET_E_WORKSPACE; }
    ValIn L;
    L.mask = mask; L.point = point; L.dirn = dirn; L.label = label; L.dirlab = dirlab; L.weight = weight_u8; L.point_t = point_target_f16;
    for (int k = 0; k < 17; ++k) L.lut[k] = k < direction_classes ? dir_rank_host[k] : -1;
    L.B = B; L.P = P;
    hipStream_t st = (hipStream_t)stream;
    return with_int<5, 9, 17>(direction_classes, [&](auto nd) { return val_sums_impl<decltype(nd)::value>(L, B, P, workspace, sums, st); });
}

extern "C" int cdnet_dam_val_sums(const float *mask, const float *point, const float *dirn, const uint8_t *label, const uint8_t *dirlab,
                                  const uint16_t *point_target_f16, const uint8_t *weight_u8, const int *dir_rank_host, int B, int H, int W,
                                  float *workspace, size_t workspace_floats, float *sums, void *stream) {
    return cdnet_dam_val_sums_classes(mask, point, dirn, label, dirlab, point_target_f16, weight_u8, dir_rank_host, 9, B, H, W, workspace,
                                      workspace_floats, sums, stream);
}
