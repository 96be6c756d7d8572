// Weight packer of the convolution kernels: fp32 master weights -> bf16 (or split hi | lo bf16) images in MFMA B-fragment order, one
// launch per tensor or every layer's packs in one batched launch.
#include <vector>
#include "common.h"
#include "stage16.h"

using namespace cdnet;

namespace {

// ------------------------------------------------------------------------------------------------------
// weight packing: fp32 master weights -> bf16 MFMA B-fragment order
//   packed[cout_tile][chunk][tap][kc][half][col BN][8]   value = w(cout = tile*BN+col, cin = chunk*CK+kc*16+half*8+j, tap)
// mode 0: Conv2d weight [Cout][Cin][KH][KW], forward       tap = kh*KW+kw
// mode 1: Conv2d weight, backward-data: roles of cin/cout swap, taps flip: "cout" := original cin,
//         "cin" := original cout, tap (kh,kw) := original (KH-1-kh, KW-1-kw)
// mode 2: ConvTranspose2d weight [Cin][Cout][4][4] forward, sub-pixel parity (a,b) in `parity`:
//         tap t=(ty,tx) in 2x2: rows {a==0: kh 1 (dy 0), kh 3 (dy -1); a==1: kh 0 (dy +1), kh 2 (dy 0)}
// mode 3: ConvTranspose2d weight [Cin][Cout][2][2] forward, parity (a,b): single tap (kh=a, kw=b)
// Channels beyond the real Cin/Cout (padding to CK / BN multiples) are zero.
// ------------------------------------------------------------------------------------------------------
struct PackDesc {            // one (layer, sub-pixel parity) packing job
    const float *w;
    unsigned short *out;
    int Cout, Cin, KH, KW, CK, BN, nchunk, ntile, TAPS, mode, parity;
    unsigned block0, nblocks; // its slice of the batched launch
    int split;                // 1: fp32-precision pack - per chunk the bf16(w) image followed by the bf16(w - bf16(w)) image
    const float *scale;       // optional per-output-channel multiplier applied in fp32 before the rounding (eval-mode BatchNorm fold; mode 0)
};

__device__ __forceinline__ void pack_range(const PackDesc &d, size_t first, size_t stride) {
    const float *__restrict__ w = d.w;
    unsigned short *__restrict__ out = d.out;
    const int Cout = d.Cout, Cin = d.Cin, KH = d.KH, KW = d.KW, CK = d.CK, BN = d.BN, nchunk = d.nchunk, TAPS = d.TAPS, mode = d.mode,
              parity = d.parity;
    // one thread = the 8 consecutive input channels of one (tile, chunk, tap, k-half, column): the index is decoded once per
    // 16-byte vector (decoding every element made this kernel 0.1 ms of integer divisions on the step's critical chain)
    const size_t total = (size_t)d.ntile * nchunk * TAPS * (CK / 16) * 2 * BN * (d.split ? 2 : 1);
    for (size_t i = first; i < total; i += stride) {
        // work order: the tap runs fastest - neighbouring lanes then read neighbouring floats of the [..][kh][kw] weight tensors (a wave's
        // load touches ~8 cache lines instead of 64; the scattered side is the 16-byte stores, an eighth as many) - the pack layout is
        // [tile][chunk][hi|lo][tap][k-chunk][k-half][column][8 channels]
        size_t r = i;
        int tap = r % TAPS; r /= TAPS;
        int col = r % BN; r /= BN;
        int half = r % 2; r /= 2;
        int kc = r % (CK / 16); r /= (CK / 16);
        int hl = 0;
        if (d.split) { hl = r % 2; r /= 2; }
        int chunk = r % nchunk; r /= nchunk;
        int tile = (int)r;
        int co = tile * BN + col;
        const size_t ovec = ((((((size_t)tile * nchunk + chunk) * (d.split ? 2 : 1) + hl) * TAPS + tap) * (CK / 16) + kc) * 2 + half) * BN + col;
        unsigned short o8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
        int ci = chunk * CK + kc * 16 + half * 8 + j;
        float v = 0.f;
        if (co < Cout && ci < Cin) {
            if (mode == 0) {
                v = w[(((size_t)co * Cin + ci) * KH + tap / KW) * KW + tap % KW];
            } else if (mode == 1) {
                int kh = KH - 1 - tap / KW, kw = KW - 1 - tap % KW;
                // here Cout/Cin are the ROLES in the backward GEMM: co indexes original cin, ci original cout
                v = w[(((size_t)ci * Cout + co) * KH + kh) * KW + kw];
            } else if (mode == 2) {
                int a = parity >> 1, b = parity & 1, ty = tap >> 1, tx = tap & 1;
                int kh = a == 0 ? (ty == 0 ? 1 : 3) : (ty == 0 ? 0 : 2);
                int kw = b == 0 ? (tx == 0 ? 1 : 3) : (tx == 0 ? 0 : 2);
                v = w[(((size_t)ci * Cout + co) * 4 + kh) * 4 + kw];
            } else if (mode == 3) {
                int a = parity >> 1, b = parity & 1;
                v = w[(((size_t)ci * Cout + co) * 2 + a) * 2 + b];
            } else if (mode == 7) {
                // backward-data of mode 6: GEMM co = (a, b, c) of the view (Cout = 4*Ct), ci = the conv's out channel,
                // taps flipped: dV[y'][x'][(a,b,c)] = sum_t dY[y' - dy_t][x' - dx_t][ci] * W[ci][c][ky][kx]
                const int Ct = Cout / 4;
                const int a = co / (2 * Ct), b = (co / Ct) & 1, c = co % Ct;
                const int tf = 8 - tap;
                const int kh = 2 * (tf / 3 - 1) + a + 1, kw = 2 * (tf % 3 - 1) + b + 1;
                if (kh >= 0 && kh < 3 && kw >= 0 && kw < 3) v = w[(((size_t)ci * Ct + c) * 3 + kh) * 3 + kw];
            } else {
                // modes 4/5: backward-data of a stride-2 transposed convolution as a convolution over the space-to-depth
                // view of the output gradient.  GEMM "cin" ci = a*(2*Ct) + b*Ct + c (row parity a = source, column parity
                // b, channel c of the transposed conv's Ct out_channels); GEMM "cout" co = its in_channel.
                const int Ct = Cin / 4;
                const int a = ci / (2 * Ct), b = (ci / Ct) & 1, c = ci % Ct;
                if (mode == 4) {
                    const int kh = 2 * (tap / 3) + a - 1, kw = 2 * (tap % 3) + b - 1;      // 3x3 taps (ky, kx)
                    if (kh >= 0 && kh < 4 && kw >= 0 && kw < 4) v = w[(((size_t)co * Ct + c) * 4 + kh) * 4 + kw];
                } else if (mode == 5) {
                    v = w[(((size_t)co * Ct + c) * 2 + a) * 2 + b];
                } else {
                    // mode 6: FORWARD 3x3 stride-2 pad-1 convolution [Cout][Ct][3][3] as a 3x3 convolution over the
                    // space-to-depth view of its input: in(2y+ky-1, 2x+kx-1) = view(y+dy, x+dx; parity a, b) with
                    // ky = 2*dy + a + 1 (tap row r = dy + 1), only dy in {-1, 0} contribute
                    const int kh = 2 * (tap / 3 - 1) + a + 1, kw = 2 * (tap % 3 - 1) + b + 1;
                    if (kh >= 0 && kh < 3 && kw >= 0 && kw < 3) v = w[(((size_t)co * Ct + c) * 3 + kh) * 3 + kw];
                }
            }
        }
        if (d.scale && co < Cout) v *= d.scale[co];
        const unsigned short hi = f2bf(v);
        o8[j] = hl ? f2bf(v - bf2f(hi)) : hi;
        }
        uint4 ov;
        ov.x = o8[0] | ((unsigned)o8[1] << 16); ov.y = o8[2] | ((unsigned)o8[3] << 16);
        ov.z = o8[4] | ((unsigned)o8[5] << 16); ov.w = o8[6] | ((unsigned)o8[7] << 16);
        reinterpret_cast<uint4 *>(out)[ovec] = ov;
    }
}

__global__ void pack_weights_kernel(PackDesc d) {
    pack_range(d, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// every layer's forward and backward-data packs in ONE launch (the training step re-packs ~80 small tensors after each
// Adam update; separate launches cost more than the work)
__global__ void pack_weights_batch_kernel(const PackDesc *__restrict__ table, int n) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {                          // last descriptor whose block0 <= blockIdx.x
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].block0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const PackDesc d = table[lo];
    pack_range(d, (size_t)(blockIdx.x - d.block0) * blockDim.x + threadIdx.x, (size_t)d.nblocks * blockDim.x);
}

}  // namespace

extern "C" size_t cdnet_conv_packed_weight_elems(int Cout, int Cin_padded_chunks, int taps, int CK, int BN, int npar) {
    return (size_t)npar * cdiv(Cout, BN) * Cin_padded_chunks * taps * CK * BN;
}

static int fill_pack_desc(PackDesc &d, const float *w, void *packed, int Cout, int Cin, int KH, int KW, int CK, int BN, int mode, int p,
                          const char *who) {
    const int split = (mode & 16) ? 1 : 0;            // CDNET_PACK_SPLIT: hi | lo images (fp32-precision convolutions)
    mode &= 15;
    CDNET_REQUIRE(w && packed, "%s: null pointer", who);
    CDNET_REQUIRE(CK % 16 == 0 && BN % 32 == 0 && Cin % CK == 0 && mode >= 0 && mode <= 7, "%s: Cin=%d CK=%d BN=%d mode=%d", who, Cin, CK, BN, mode);
    const int taps = mode == 2 ? 4 : (mode == 3 ? 1 : ((mode == 4 || mode == 6 || mode == 7) ? 9 : (mode == 5 ? 1 : KH * KW)));
    const int nchunk = Cin / CK, ntile = cdiv(Cout, BN);
    const size_t per = (size_t)ntile * nchunk * taps * CK * BN * (split ? 2 : 1);
    d.split = split;
    d.scale = nullptr;
    d.w = w; d.out = (unsigned short *)packed + (size_t)p * per;
    d.Cout = Cout; d.Cin = Cin; d.KH = KH; d.KW = KW; d.CK = CK; d.BN = BN; d.nchunk = nchunk; d.ntile = ntile; d.TAPS = taps; d.mode = mode;
    d.parity = p;
    d.block0 = 0;
    d.nblocks = (unsigned)((per + 2047) / 2048);          // 8 elements per thread
    if (d.nblocks > 4096) d.nblocks = 4096;
    return CDNET_OK;
}

extern "C" int cdnet_pack_conv_weights(const float *w, void *packed, int Cout, int Cin, int KH, int KW, int CK, int BN,
                                       int mode, void *stream) {
    const int npar = ((mode & 15) == 2 || (mode & 15) == 3) ? 4 : 1;
    for (int p = 0; p < npar; ++p) {
        PackDesc d;
        int rc = fill_pack_desc(d, w, packed, Cout, Cin, KH, KW, CK, BN, mode, p, "cdnet_pack_conv_weights");
        if (rc) return rc;
        pack_weights_kernel<<<d.nblocks, 256, 0, (hipStream_t)stream>>>(d);
    }
    return check_launch("cdnet_pack_conv_weights");
}

extern "C" int cdnet_pack_conv_weights_scaled(const float *w, const float *cout_scale, void *packed, int Cout, int Cin, int KH, int KW, int CK,
                                              int BN, int mode, void *stream) {
    CDNET_REQUIRE(cout_scale && (mode & 15) == 0, "cdnet_pack_conv_weights_scaled: forward Conv2d packs (mode 0) with a scale vector");
    PackDesc d;
    int rc = fill_pack_desc(d, w, packed, Cout, Cin, KH, KW, CK, BN, mode, 0, "cdnet_pack_conv_weights_scaled");
    if (rc) return rc;
    d.scale = cout_scale;
    pack_weights_kernel<<<d.nblocks, 256, 0, (hipStream_t)stream>>>(d);
    return check_launch("cdnet_pack_conv_weights_scaled");
}

extern "C" size_t cdnet_pack_batch_table_bytes(int n_jobs) { return (size_t)n_jobs * 4 * sizeof(PackDesc); }

extern "C" int cdnet_pack_conv_weights_batch(const cdnet_pack_job *jobs, int n_jobs, void *table, size_t table_bytes, int upload,
                                             void *stream) {
    CDNET_REQUIRE(jobs && n_jobs > 0 && table, "cdnet_pack_conv_weights_batch: null pointer / no jobs");
    CDNET_REQUIRE(table_bytes >= cdnet_pack_batch_table_bytes(n_jobs), "cdnet_pack_conv_weights_batch: table too small");
    static thread_local std::vector<PackDesc> host;
    host.clear();
    unsigned blocks = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const cdnet_pack_job &J = jobs[j];
        const int npar = ((J.mode & 15) == 2 || (J.mode & 15) == 3) ? 4 : 1;
        for (int p = 0; p < npar; ++p) {
            PackDesc d;
            int rc = fill_pack_desc(d, J.w, J.packed, J.Cout, J.Cin, J.KH, J.KW, J.CK, J.BN, J.mode, p, "cdnet_pack_conv_weights_batch");
            if (rc) return rc;
            d.block0 = blocks;
            blocks += d.nblocks;
            host.push_back(d);
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if (upload) {
        // (synchronous with respect to the host buffer: the table is rebuilt on every call)
        if (hipMemcpyAsync(table, host.data(), host.size() * sizeof(PackDesc), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return check_launch("cdnet_pack_conv_weights_batch(upload)");
    }
    pack_weights_batch_kernel<<<blocks, 256, 0, st>>>((const PackDesc *)table, (int)host.size());
    return check_launch("cdnet_pack_conv_weights_batch");
}
