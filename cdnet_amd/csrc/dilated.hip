// Dilated dense-block convolution for FullNet inference (cdnet_dilated_conv_forward, include/cdnet_hip.h), gfx950.
//
// Replaces models/FullNet.py:14-36 (ConvLayer: Conv2d(dilation) -> LeakyReLU -> BatchNorm2d; BasicLayer / BottleneckLayer's
// torch.cat([x, out], 1)) and :90-138 (stem, transitions, final convolution) in eval mode.
//
// One staging form for every dilation: tap-shifted fragments straight from global memory, no halo tile.  A wave owns a strip of
// 32 pixels of MT consecutive rows; for each 32-channel step and each tap it reads the strip shifted by ((ky-1) d, (kx-1) d) directly
// in the MFMA A layout (lane = pixel, 16 consecutive channels per lane: 32 B bf16 / 64 B fp32 per lane and load pair), so the cost
// of a tap does not depend on d - a (16 + 2d)^2 halo tile would stage 58^2 pixels for 256 at d = 21.  The channel step is the OUTER
// loop: the nine shifted reads of a step then follow each other closely (measured 24 % faster at d = 1 than taps outside, DESIGN.md
// section 4.9); each pixel is still requested nine times, and the dense layers are bound by those requests, not by the matrix pipe:
// GEMM-N is one or two 32-wide MFMA columns (growth_rate = 24).  The B fragments come from the per-layer pack in load order (one
// 16-byte load per lane and K step, the same 1 KB for every wave).
// K order inside a 32-channel step: lane half h holds channels 16 h + [0, 16); MFMA s of the step takes the half's channels
// 8 s + [0, 8) - the pack uses the same order, which is all that a GEMM asks of K.
// Channels >= Cin of the last 8-channel unit and pixels outside the image are selected to zero before the MFMA (never multiplied).
// fp32 mode: fragments split into bf16 hi / lo, three MFMAs per product (split8 and mfma3 of split_bf16.h).
//
// Training: backward-data (cdnet_dilated_conv_backward_data) is this kernel on swapped roles - its input is the gradient g of the raw
// convolution output, GEMM-K runs over Cout x taps, GEMM-N over Cin, the pack is w'[ci][co][8 - tap] (cdnet_dilated_pack_weights_bwd) - with
// the template parameter ACC for the store that adds into a block's gradient buffer.  The other training kernels are in dilated_train.hip.
#include "common.h"
#include "launch.h"
#include "split_bf16.h"

using namespace cdnet;

namespace {

constexpr int TILE_W = 32;       // pixels of a strip (MFMA M)
constexpr int WAVES = 4;
constexpr int KPAIR = 32;        // channels of one load step (two MFMAs of 16)
constexpr int FRAG = 64 * 8;     // bf16 elements of one B fragment image

// the 8 channels at element offset `eoff` of `in` as MFMA operand words; rem = Cin - first channel (channels >= rem are zeroed),
// ok = false: the whole unit is zero and nothing is loaded
template <bool F32>
__device__ __forceinline__ void load_unit(const void *in, size_t eoff, bool ok, int rem, u32x4 &hi, u32x4 &lo) {
    hi = u32x4{0u, 0u, 0u, 0u};
    lo = u32x4{0u, 0u, 0u, 0u};
    if (!ok) return;
    if constexpr (F32) {
        const f32x4 *p = reinterpret_cast<const f32x4 *>(static_cast<const float *>(in) + eoff);
        const f32x4 a = p[0], b = p[1];
        float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        if (rem < 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j < rem ? v[j] : 0.f;
        }
        split8(v, hi, lo);
    } else {
        hi = *reinterpret_cast<const u32x4 *>(static_cast<const uint16_t *>(in) + eoff);
        if (rem < 8) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                hi[k] &= (2 * k < rem ? 0x0000ffffu : 0u) | (2 * k + 1 < rem ? 0xffff0000u : 0u);
        }
    }
}

__device__ __forceinline__ uint16_t to_bf16(float v) {
    return __builtin_bit_cast(uint16_t, static_cast<__bf16>(v));
}

// grid: x = 32-pixel strips x row groups of WAVES * MT rows, y = groups of NT 32-wide output tiles, z = image
// ACC: the NHWC store adds to what `out` holds (backward-data into a gradient buffer that other layers wrote, cdnet_dilated_conv_backward_data);
// the forward instantiations have ACC = false
template <int MT, int NT, bool F32, bool ACC = false>
__global__ __launch_bounds__(WAVES * 64) void dilated_conv_kernel(const cdnet_dilated_conv_args A) {
    constexpr int IMGS = F32 ? 2 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = lane & 31, h = lane >> 5;
    const int tiles_x = (A.W + TILE_W - 1) / TILE_W;
    const int x0 = (int)(blockIdx.x % tiles_x) * TILE_W, y0 = ((int)(blockIdx.x / tiles_x) * WAVES + wave) * MT;
    const int n = blockIdx.z, nt0 = blockIdx.y * NT;
    if (y0 >= A.H) return;                                        // (wave-uniform; the kernel has no barrier)
    const int NTT = (A.Cout + 31) / 32, KP = (A.Cin + KPAIR - 1) / KPAIR, KK = 2 * KP;
    const u32x4 *wfrag = static_cast<const u32x4 *>(A.w) + lane;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.f;

    // 32-channel steps outside, taps inside: the nine shifted reads of a channel step follow each other closely (at small d from the same
    // cache lines), instead of a whole strip of all channels between two reads of a pixel
    for (int ps = 0; ps < KP; ++ps) {
        for (int tap = 0; tap < A.taps; ++tap) {
            const long long dy = A.taps == 9 ? (long long)(tap / 3 - 1) * A.dilation : 0;
            const long long dx = A.taps == 9 ? (long long)(tap % 3 - 1) * A.dilation : 0;
            const long long xx = x0 + p + dx;
            bool ok[MT], any = false;
            size_t off[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const long long yy = y0 + m + dy;
                ok[m] = y0 + m < A.H && yy >= 0 && yy < A.H && xx >= 0 && xx < A.W;
                off[m] = ok[m] ? (((size_t)n * A.H + (size_t)yy) * A.W + (size_t)xx) * (size_t)A.in_cstride : 0;
                any |= ok[m];
            }
            if (__builtin_amdgcn_ballot_w64(any) == 0) continue;      // the tap lies outside the image for the whole strip
            const int c = ps * KPAIR + 16 * h;
            u32x4 ah[MT][2], al[MT][2];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int rem = A.Cin - (c + 8 * s);
                    load_unit<F32>(A.in, off[m] + (size_t)(c + 8 * s), ok[m] && rem > 0, rem, ah[m][s], al[m][s]);
                }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (ps * KPAIR + 8 * s >= A.Cin) break;           // both halves' units lie beyond Cin (uniform)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (nt0 + t >= NTT) break;                    // (uniform: the last group of an odd tile count)
                    const u32x4 *wb = wfrag + ((size_t)(tap * KK + 2 * ps + s) * NTT + (nt0 + t)) * (64 * IMGS);
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, wb[0]);
                    if constexpr (F32) {
                        const bf16x8 bl = __builtin_bit_cast(bf16x8, wb[64]);
#pragma unroll
                        for (int m = 0; m < MT; ++m) {
                            const bf16x8 a_hi = __builtin_bit_cast(bf16x8, ah[m][s]), a_lo = __builtin_bit_cast(bf16x8, al[m][s]);
                            acc[m][t] = mfma3(acc[m][t], a_hi, a_lo, bh, bl);
                        }
                    } else {
#pragma unroll
                        for (int m = 0; m < MT; ++m)
                            acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[m][s]), bh, acc[m][t], 0, 0, 0);
                    }
                }
            }
        }
    }

    // lane (p, h) of a 32 x 32 block owns output channel 32 tile + p and the strip's pixels (r & 3) + 8 (r >> 2) + 4 h, r = 0..15
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int co = (nt0 + t) * 32 + p;
        if (co >= A.Cout) continue;
        const float sc = A.scale ? A.scale[co] : 1.f, sh = A.shift ? A.shift[co] : 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int y = y0 + m;
            if (y >= A.H) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int x = x0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (x >= A.W) continue;
                float v = acc[m][t][r];
                if (A.leaky) v = v >= 0.f ? v : A.slope * v;
                v = v * sc + sh;
                if (A.out_nchw) {
                    static_cast<float *>(A.out)[(((size_t)n * A.Cout + co) * A.H + y) * A.W + x] = v;
                } else {
                    const size_t o = (((size_t)n * A.H + y) * A.W + x) * (size_t)A.out_cstride + A.out_coff + co;
                    if constexpr (F32) {
                        if constexpr (ACC) v += static_cast<float *>(A.out)[o];
                        static_cast<float *>(A.out)[o] = v;
                    } else {
                        if constexpr (ACC) v += __builtin_bit_cast(float, (unsigned)static_cast<uint16_t *>(A.out)[o] << 16);
                        static_cast<uint16_t *>(A.out)[o] = to_bf16(v);
                    }
                }
            }
        }
    }
}

// one thread per packed bf16x8 fragment row (lane of a (tap, K step, N tile) fragment).  BWD false: GEMM-N runs over Cout, GEMM-K over Cin;
// true, the backward-data pack: the same fragment order for w'[ci][co][taps - 1 - tap] - GEMM-N over Cin, GEMM-K over Cout, taps mirrored
template <bool BWD>
__global__ void dilated_pack_kernel(const float *w, uint16_t *packed, int Cin, int Cout, int taps, int f32, size_t rows) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const int NTT = ((BWD ? Cin : Cout) + 31) / 32, KK = 2 * (((BWD ? Cout : Cin) + KPAIR - 1) / KPAIR);
    const int lane = (int)(i % 64);
    const size_t f = i / 64;
    const int t = (int)(f % NTT), kk = (int)((f / NTT) % KK), tap = (int)(f / NTT / KK);
    const int n = t * 32 + (lane & 31), k0 = (kk >> 1) * KPAIR + 16 * (lane >> 5) + 8 * (kk & 1);
    uint16_t *dst = packed + f * (size_t)(FRAG * (f32 ? 2 : 1)) + (size_t)lane * 8;
    for (int j = 0; j < 8; ++j) {
        const int co = BWD ? k0 + j : n, ci = BWD ? n : k0 + j;
        const float v = (co < Cout && ci < Cin) ? w[((size_t)co * Cin + ci) * taps + (BWD ? taps - 1 - tap : tap)] : 0.f;
        const __bf16 hb = static_cast<__bf16>(v);
        dst[j] = __builtin_bit_cast(uint16_t, hb);
        if (f32) dst[FRAG + j] = to_bf16(v - static_cast<float>(hb));
    }
}

size_t pack_rows(int Cin, int Cout, int taps) {
    return (size_t)taps * (2 * ((Cin + KPAIR - 1) / KPAIR)) * ((Cout + 31) / 32) * 64;
}

// both pack entries: `who` is the entry's name, BWD its kernel; GEMM-N and GEMM-K swap for the backward-data pack
template <bool BWD>
int pack(const char *who, const float *w, void *packed, int Cin, int Cout, int taps, int f32, void *stream) {
    CDNET_REQUIRE(w && packed, "%s: null pointer", who);
    CDNET_REQUIRE(Cin >= 1 && Cout >= 1, "%s: Cin %d, Cout %d must be positive", who, Cin, Cout);
    CDNET_REQUIRE(taps == 1 || taps == 9, "%s: taps %d (1 or 9)", who, taps);
    const size_t rows = BWD ? pack_rows(Cout, Cin, taps) : pack_rows(Cin, Cout, taps);
    dilated_pack_kernel<BWD><<<(unsigned)((rows + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, static_cast<uint16_t *>(packed), Cin, Cout, taps,
                                                                                             f32 ? 1 : 0, rows);
    return check_launch(who);
}

// `who`: the entry's name; acc: the store adds (backward-data only)
template <int MT, int NT>
int launch(const cdnet_dilated_conv_args &A, bool acc, hipStream_t st, const char *who) {
    const int tiles_x = cdiv(A.W, TILE_W), tiles_y = cdiv(A.H, WAVES * MT);
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)cdiv(cdiv(A.Cout, 32), NT), (unsigned)A.N);
    return with_bool(A.f32 != 0, [&](auto f32_c) {
        return with_bool(acc, [&](auto acc_c) {
            dilated_conv_kernel<MT, NT, decltype(f32_c)::value, decltype(acc_c)::value><<<grid, WAVES * 64, 0, st>>>(A);
            return check_launch(who);
        });
    });
}

}  // namespace

extern "C" size_t cdnet_dilated_packed_weight_elems(int Cin, int Cout, int taps, int f32) {
    if (Cin < 1 || Cout < 1 || (taps != 1 && taps != 9)) return 0;
    return pack_rows(Cin, Cout, taps) * 8 * (f32 ? 2 : 1);
}

extern "C" int cdnet_dilated_pack_weights(const float *w, void *packed, int Cin, int Cout, int taps, int f32, void *stream) {
    return pack<false>("cdnet_dilated_pack_weights", w, packed, Cin, Cout, taps, f32, stream);
}

extern "C" int cdnet_dilated_conv_forward(const cdnet_dilated_conv_args *args, void *stream) {
    CDNET_REQUIRE(args, "cdnet_dilated_conv_forward: null args");
    const cdnet_dilated_conv_args &A = *args;
    CDNET_REQUIRE(A.in && A.w && A.out, "cdnet_dilated_conv_forward: null in / w / out");
    CDNET_REQUIRE(A.taps == 1 || A.taps == 9, "cdnet_dilated_conv_forward: taps %d (1 or 9)", A.taps);
    CDNET_REQUIRE(A.dilation >= 1, "cdnet_dilated_conv_forward: dilation %d < 1", A.dilation);
    CDNET_REQUIRE(A.N >= 1 && A.H >= 1 && A.W >= 1 && A.Cin >= 1 && A.Cout >= 1,
                  "cdnet_dilated_conv_forward: N %d H %d W %d Cin %d Cout %d must be positive", A.N, A.H, A.W, A.Cin, A.Cout);
    CDNET_REQUIRE(A.N <= 65535, "cdnet_dilated_conv_forward: N %d > 65535 images per launch", A.N);
    CDNET_REQUIRE(A.in_cstride >= A.Cin && A.in_cstride % 8 == 0,
                  "cdnet_dilated_conv_forward: in_cstride %d must be a multiple of 8 and >= Cin %d", A.in_cstride, A.Cin);
    if (A.out_nchw) {
        CDNET_REQUIRE(A.out_coff == 0, "cdnet_dilated_conv_forward: out_nchw needs out_coff 0");
        CDNET_REQUIRE(A.in != A.out, "cdnet_dilated_conv_forward: out_nchw cannot write in place");
    } else {
        CDNET_REQUIRE(A.out_coff >= 0 && A.out_cstride >= 1 && (long long)A.out_coff + A.Cout <= A.out_cstride,
                      "cdnet_dilated_conv_forward: out_coff %d + Cout %d exceeds out_cstride %d", A.out_coff, A.Cout, A.out_cstride);
        if (A.in == A.out) {
            CDNET_REQUIRE(A.in_cstride == A.out_cstride, "cdnet_dilated_conv_forward: in place with strides %d != %d", A.in_cstride, A.out_cstride);
            CDNET_REQUIRE(A.out_coff >= A.Cin, "cdnet_dilated_conv_forward: in place, output channels [%d, %d) overlap the input's [0, %d)",
                          A.out_coff, A.out_coff + A.Cout, A.Cin);
        }
    }
    CDNET_REQUIRE((long long)cdiv(A.W, TILE_W) * cdiv(A.H, WAVES) < (1ll << 31), "cdnet_dilated_conv_forward: image too large");
    if (A.Cout <= 32) return launch<4, 1>(A, false, (hipStream_t)stream, "cdnet_dilated_conv_forward");
    return launch<2, 2>(A, false, (hipStream_t)stream, "cdnet_dilated_conv_forward");
}

extern "C" int cdnet_dilated_pack_weights_bwd(const float *w, void *packed, int Cin, int Cout, int taps, int f32, void *stream) {
    return pack<true>("cdnet_dilated_pack_weights_bwd", w, packed, Cin, Cout, taps, f32, stream);
}

// dx = conv(g, w') is the forward kernel on swapped roles: its `in` is g (Cout channels), its output tile count runs over Cin
extern "C" int cdnet_dilated_conv_backward_data(const cdnet_dilated_bwd_data_args *args, void *stream) {
    CDNET_REQUIRE(args, "cdnet_dilated_conv_backward_data: null args");
    const cdnet_dilated_bwd_data_args &B = *args;
    CDNET_REQUIRE(B.g && B.w && B.dx, "cdnet_dilated_conv_backward_data: null g / w / dx");
    CDNET_REQUIRE(B.taps == 1 || B.taps == 9, "cdnet_dilated_conv_backward_data: taps %d (1 or 9)", B.taps);
    CDNET_REQUIRE(B.dilation >= 1, "cdnet_dilated_conv_backward_data: dilation %d < 1", B.dilation);
    CDNET_REQUIRE(B.N >= 1 && B.H >= 1 && B.W >= 1 && B.Cin >= 1 && B.Cout >= 1,
                  "cdnet_dilated_conv_backward_data: N %d H %d W %d Cin %d Cout %d must be positive", B.N, B.H, B.W, B.Cin, B.Cout);
    CDNET_REQUIRE(B.N <= 65535, "cdnet_dilated_conv_backward_data: N %d > 65535 images per launch", B.N);
    CDNET_REQUIRE(B.g_cstride >= B.Cout && B.g_cstride % 8 == 0,
                  "cdnet_dilated_conv_backward_data: g_cstride %d must be a multiple of 8 and >= Cout %d", B.g_cstride, B.Cout);
    CDNET_REQUIRE(B.dx_coff >= 0 && B.dx_cstride >= 1 && (long long)B.dx_coff + B.Cin <= B.dx_cstride,
                  "cdnet_dilated_conv_backward_data: dx_coff %d + Cin %d exceeds dx_cstride %d", B.dx_coff, B.Cin, B.dx_cstride);
    if (B.g == B.dx) {
        CDNET_REQUIRE(B.g_cstride == B.dx_cstride, "cdnet_dilated_conv_backward_data: in place with strides %d != %d", B.g_cstride, B.dx_cstride);
        CDNET_REQUIRE(B.dx_coff >= B.Cout, "cdnet_dilated_conv_backward_data: in place, target channels [%d, %d) overlap the source's [0, %d)",
                      B.dx_coff, B.dx_coff + B.Cin, B.Cout);
    }
    CDNET_REQUIRE((long long)cdiv(B.W, TILE_W) * cdiv(B.H, WAVES) < (1ll << 31), "cdnet_dilated_conv_backward_data: image too large");
    cdnet_dilated_conv_args A = {};
    A.in = B.g; A.w = B.w; A.scale = nullptr; A.shift = nullptr; A.out = B.dx;
    A.N = B.N; A.H = B.H; A.W = B.W;
    A.Cin = B.Cout; A.in_cstride = B.g_cstride;
    A.Cout = B.Cin; A.out_cstride = B.dx_cstride; A.out_coff = B.dx_coff;
    A.taps = B.taps; A.dilation = B.dilation; A.leaky = 0; A.slope = 0.f; A.f32 = B.f32 ? 1 : 0; A.out_nchw = 0;
    if (A.Cout <= 32) return launch<4, 1>(A, B.accumulate != 0, (hipStream_t)stream, "cdnet_dilated_conv_backward_data");
    return launch<2, 2>(A, B.accumulate != 0, (hipStream_t)stream, "cdnet_dilated_conv_backward_data");
}
