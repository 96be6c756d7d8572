// Kernel-side aliases of the public argument structs (include/cdnet_hip.h).
#pragma once
#include "../../include/cdnet_hip.h"

struct ConvSrc {
    const unsigned short *x;
    const unsigned short *res;
    const float *scale;
    const float *shift;
    int C, Hs, Ws, pool, relu, off_y, off_x;
    int f16, row_stride;
};

struct ConvArgs {
    ConvSrc src[2];
    int nsrc;
    const unsigned short *w;
    const float *bias;
    const float *oscale;
    const float *oshift;
    int orelu;
    unsigned short *out;
    int Cout, out_cstride, out_coff;
    float *stats;
    int N, H, W;
    int taps, npar, ostride, nchunk;
    int tile, CK, BN;
    int out_f16;
    int debug;
    int ws;
    int f32;
    const unsigned short *eres;
    const float *eres_scale, *eres_shift;
    int eres_f16, eres_relu;
    int taps1, pad_;
    unsigned short *pool_out;
    const float *dot_w, *dot_b;
    float *dot_out;
};

// Kernel-selection bits of cdnet_conv_args.debug, read by the host code (0 in production; the tests and tools pass the literals).
// The lower bits, and 512 / 1024 in conv_ws_kernel, are ablations read inside the kernels (tools/bench_conv*.py) and keep their literals.
//
//   bit(s)   read by                                      meaning
//   16       conv16ws.hip, launcher                       conv_ws16_kernel's quad-request form whatever the launch's size
//            (in kernels: conv_fwd_kernel - dispatch-order ablation; conv_f32_kernel / store_tile_f32 - the general epilogue
//             on full tiles too, for the tests that compare the two epilogues)
//   32       conv.hip, conv32ws.hip, conv16ws.hip         the one-tile kernels only (conv_fwd_kernel / conv_f32_kernel)
//   64       the three persistent launchers               the persistent kernel on small launches too
//   128      conv16ws.hip                                 conv_ws_kernel, the older 16-bit persistent kernel, instead of conv_ws16_kernel
//   256      conv32.hip, try_conv1x1_stream               conv_f32_kernel instead of conv1x1_f32_stream_kernel
//   >> 8     conv32ws.hip, conv16ws.hip                   at most (debug >> 8) workgroups per output-channel tile
//
// 256 is also the lowest bit of the workgroup cap: debug = 256 caps a persistent launch of conv_ws32_kernel / conv_ws16_kernel at one
// workgroup.  The two never meet - 256 is read for one-tap fp32 launches, the persistent kernels are nine-tap.  conv_ws_kernel reads
// 512 and 1024 as ablations of its own, so its launcher applies no cap.
enum : int {
    CONV_DBG_WS16_QUAD = 16,
    CONV_DBG_ONE_TILE = 32,
    CONV_DBG_PERSIST_SMALL = 64,
    CONV_DBG_OLD_WS16 = 128,
    CONV_DBG_NO_STREAM_1X1 = 256,
    CONV_DBG_GRID_SHIFT = 8,
};
// ... and of WgradArgs.debug (env CDNET_WGRAD_DEBUG; 1, 2, 4 are ablations inside the kernels), read by wgrad.hip's launchers:
//   8        the 8-wave kernels instead of the wave-specialised ones (wgrad_kernel for wgrad_ws_kernel, wgrad_f32_kernel for wgrad_ws32_kernel)
//   16       no small-channel forms: all four quadrants (QM = 0) in the fp32 kernels, the 32 x 128 form instead of wgrad_ws_kernel<1, 1>
enum : int {
    WGRAD_DBG_NO_WS = 8,
    WGRAD_DBG_ALL_QUADS = 16,
};

static_assert(sizeof(ConvSrc) == sizeof(cdnet_conv_src), "ConvSrc layout");
static_assert(sizeof(ConvArgs) == sizeof(cdnet_conv_args), "ConvArgs layout");

namespace cdnet {
// which instantiation the last launch of this thread took (cdnet_conv_forward_last_form; host only, bit layout in cdnet_hip.h): every
// launcher of conv.hip / conv_ws.hip / conv16ws.hip / conv32.hip / conv32ws.hip writes it just before its launch, the tests assert it
extern thread_local int g_conv_last_form;
constexpr int conv_form(int family, int bn, int taps, int xf = 0, bool stats = false, bool stream = false, bool mix = false, int ncs = 0,
                        int site = 0, int tile = 16, int ck = 16, int nch = 0, bool eres = false) {
    return family | ((bn == 128 ? 2 : (bn == 64 ? 1 : 0)) << 4) | (taps << 6) | (xf << 10) | ((stats ? 1 : 0) << 12) | ((stream ? 1 : 0) << 13) |
           ((mix ? 1 : 0) << 14) | (ncs << 15) | (site << 17) | ((tile == 8 ? 1 : 0) << 20) | ((ck == 64 ? 2 : (ck == 32 ? 1 : 0)) << 21) |
           (nch << 23) | ((eres ? 1 : 0) << 26);
}
// conv32.hip: the fp32-storage / split-bf16x3 variant
int conv_forward_f32(const ConvArgs &A, hipStream_t st);
// conv32ws.hip: its wave-specialised persistent form (3x3, full 16x16 tiles, >= 4 chunks); -1 = not eligible
int conv_forward_f32_ws(const ConvArgs &A, hipStream_t st, bool dry_run = false);
// conv16ws.hip: the 16-bit path's persistent kernel for launches without statistics (any chunk count, direct stores); -1 = not eligible
int conv_forward_ws16(const ConvArgs &A, hipStream_t st, bool dry_run = false);
// conv_ws.hip: the 16-bit path's persistent kernel for launches with statistics (3x3, 16-channel chunks in fours); -1 = not eligible
int conv_forward_ws(const ConvArgs &A, hipStream_t st, bool dry_run = false);
int materialize_f32(const ConvSrc &s, int N, int H, int W, void *out, hipStream_t st);
}
