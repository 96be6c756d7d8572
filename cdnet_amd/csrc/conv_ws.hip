// conv_ws_kernel: the wave-specialised, weight-stationary persistent 3x3 convolution of the 16-bit path for launches that carry
// training-mode BatchNorm statistics (every other persistent 16-bit launch takes conv_ws16_kernel, conv16ws.hip).  The movers' tile
// cursor, buffer descriptors, hand-written barriers and weight-chunk DMA are csrc/persist.h.
//
// Replaces the same reference lines as conv.hip: models/dam/model_unet_rev1.py:86-170, 244-287.
#include <type_traits>
#include "common.h"
#include "conv_args.h"
#include "launch.h"
#include "persist.h"
#include "xform.h"
#include "stage16.h"
#include <stdlib.h>

using namespace cdnet;

namespace {

// ------------------------------------------------------------------------------------------------------
// Wave-specialised, weight-stationary, persistent variant for the 3x3 layers with 64 input channels (four 16-channel chunks;
// the whole weight tile of a cout block - 74 KB for 64 couts - stays in LDS): the full-resolution layers of the encoder stem
// and of the three residual units, forward and backward-data.
//
//   * one 8-wave workgroup per CU, persistent over a contiguous run of tiles (XCD-contiguous, like conv_fwd_kernel);
//   * the weights of the workgroup's cout tile are loaded ONCE and stay in LDS;
//   * waves 4..7 (movers) only move data.  In: four 16-channel halo chunks in flight in registers (>= 2 us of HBM latency
//     covered; straight-line code so that the compiler counts the loads in flight instead of draining them), transform
//     (BatchNorm scale/shift, residual, ReLU), LDS ring of two slots.  Out: the finished tile's out image -> global memory,
//     spread over the first three chunk steps of the NEXT tile, so that no matrix wave ever waits for the write path;
//   * waves 0..3 (consumers) only read fragments, issue MFMAs, and at the end of a tile convert their 64 pixels x BN couts and
//     park them in LDS as [cout][pixel] blocks (8-byte writes straight from the accumulator registers; the movers read them
//     back with the transposing ds_read_b64_tr_b16, which yields pixel-major 16-byte vectors for NHWC stores);
//   * one barrier per 16-channel chunk step.
// Accumulation order, MFMA shapes and epilogue arithmetic are those of conv_fwd_kernel<16,16,16,BN,4,1,TAPS>: the results are
// bit-identical (tests/test_gpu_conv.py compares the two).
// Timeline of one workgroup (debug build -DCDNET_WS_STAMPS, tools/ws_stamps.py) before the write path moved to the movers: chunk
// step 0.80 us (36 MFMAs per wave: the matrix pipe at the clock the chip holds under this load), barrier 0.22 us, conversion +
// LDS writes 1.2 us and global stores 2.5 us per tile, both in the consumers' serial path: 8.0 us per tile, 128 us per launch.
// ------------------------------------------------------------------------------------------------------
#ifdef CDNET_WS_STAMPS
// debug build only (CDNET_HIPCC_FLAGS=-DCDNET_WS_STAMPS): wall-clock stamps (100 MHz) of one consumer and one mover wave of one
// workgroup, parked in LDS and dumped at the end of the kernel; read back with cdnet_debug_ws_stamps
__device__ unsigned long long g_ws_stamps[2 * 1024];      // consumer stamps from 0, mover stamps from 1024 (384 each)
extern "C" __attribute__((visibility("default"))) int cdnet_debug_ws_stamps(unsigned long long *dst) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_ws_stamps), sizeof(g_ws_stamps)) == hipSuccess ? 0 : 1;
}
#define WS_STAMP(id) do { if (stamp_on && sn < 380) { s_stamp[sn++] = (__builtin_amdgcn_s_memrealtime() << 8) | (unsigned long long)(id); } } while (0)
#define WS_STAMP_CYC(id) do { if (stamp_on && sn < 380) { s_stamp[sn++] = ((unsigned long long)__builtin_readcyclecounter() << 8) | (unsigned long long)(id); } } while (0)
#else
#define WS_STAMP(id) do { } while (0)
#define WS_STAMP_CYC(id) do { } while (0)
#endif

template <int BN, int TAPS>
struct WsLds {
    static constexpr int TH = 16, TW = 16, CK = 16;
    // halo image: 32 B per pixel, unpadded; the two 16-byte k-halves of a pixel sit at (half ^ (halo row & 1)) * 16.  An A-fragment
    // ds_read_b128 serves 16 lanes per LDS cycle - 8 pixels of one tile row and 8 of the next, same k-half - and with the row-parity
    // swizzle these land on 16 distinct 16-byte bank groups (tools/micro/lds_read_patterns.hip: 4 LDS cycles per read; the padded
    // 48-byte layout of conv_fwd_kernel takes 7-8)
    static constexpr int PSTR = CK * 2;
    static constexpr int NPIX = (TH + 2) * (TW + 2);
    static constexpr int A_BYTES = NPIX * PSTR;                   // one ring slot: the halo tile of a 16-channel chunk
    static constexpr int NSLOT = 4;                               // ring slots = the four chunks of a tile
    static constexpr int B_CHUNK = TAPS * CK * BN * 2;            // packed weights of one chunk
    static constexpr int IROW = 72;                               // a cout row of an out-image block: 32 pixels x 2 B + 8 (conflict-free 8-byte writes)
    static constexpr int IBLK = 32 * IROW;                        // one block: 32 couts x 32 pixels
    static constexpr int OUT_WAVE = 2 * (BN / 32) * IBLK;         // a consumer wave's 64 pixels x BN couts
    static constexpr int STATS_BYTES = 2 * 4 * 2 * BN * 4;        // double-buffered [wave][sum|sumsq][BN]
    __host__ __device__ static int bytes(int nchunk, int ctot, int xf_rows = 2) {      // (xf_rows: scale | shift)
        return nchunk * B_CHUNK + NSLOT * A_BYTES + 4 * OUT_WAVE + STATS_BYTES + xf_rows * ((ctot + 7) / 8 * 8) * 4;
    }
};

// XF: input transform of every source, decided by the launcher - 0 plain bf16, 1 fp16 raw x scale + shift -> ReLU (training-mode
// BatchNorm source, packed math), 2 anything (run-time flags).
// STATS: per-tile channel sums of the unrounded accumulators.
// STREAM: more than four chunks per tile (128+ input channels, two-source layers) - the weight tile no longer fits the LDS; its
// chunks then stream through a four-slot ring by LDS-DMA, two chunks ahead of the consumers, beside the halo ring.
// The launcher guarantees nchunk % 4 == 0 (== 4 without STREAM) and full tiles (H, W multiples of 16).
// (Round 2's mover-side BatchNorm-backward experiments - the second pass applied while staging, XF 3, and the channel sums beside the
// stores, cdnet_conv_args.ws = 2 - were correct and not faster: a vector instruction of a mover wave costs the matrix pipe issue time.
// They were removed in round 3; the fp32 kernel carries the sums in the consumers' gaps instead, conv32ws.hip.)
template <int BN, int TAPS, int XF, bool STATS, bool STREAM>
__global__ __launch_bounds__(512) void conv_ws_kernel(ConvArgs A) {
    using L = WsLds<BN, TAPS>;
    constexpr int TH = 16, TW = 16, CK = 16, PSTR = L::PSTR, HW_ = TW + 2, NPIX = L::NPIX;
    constexpr int NT = BN / 32, NPW = NT, MPW = 2;               // consumer wave wm: M tiles 2wm, 2wm+1 (64 pixels), all N tiles
    constexpr int VPP = CK / 8, NA = (NPIX * VPP + 255) / 256;
    constexpr int PF = 4;                                         // halo chunks in flight per mover thread
    constexpr int NWS = 4;                                        // weight slots in LDS (the whole tile without STREAM)
    const int NCH = STREAM ? A.nchunk : 4;                        // chunks per tile

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the halo ring first: its fragment addresses (slot, tap) then fit the 16-bit offset field of ds_read from one base register per M tile
    unsigned char *lds_a = smem;
    unsigned char *lds_w = smem + L::NSLOT * L::A_BYTES;
    unsigned char *lds_o = lds_w + NWS * L::B_CHUNK;
    float *s_stats = reinterpret_cast<float *>(lds_o + 4 * L::OUT_WAVE);          // [2][4][2][BN]
    float *s_xf = reinterpret_cast<float *>(lds_o + 4 * L::OUT_WAVE + L::STATS_BYTES);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0n = A.src[0].C, ctot = c0n + (A.nsrc > 1 ? A.src[1].C : 0);
    const int xfs = (ctot + 7) / 8 * 8;
    const int cout_tile = blockIdx.y;
    const int cout0 = cout_tile * BN;
#ifdef CDNET_WS_STAMPS
    unsigned long long *s_stamp = reinterpret_cast<unsigned long long *>(smem + L::bytes(NWS, ctot, 2)) + (wave >= 4 ? 384 : 0);
    const bool stamp_on = blockIdx.x == 17 && blockIdx.y == 0 && lane == 0 && (wave == 0 || wave == 4);
    int sn = 0;
#endif

    // this workgroup's contiguous run of tiles: persist.h's tile_run, written out (as a call it changed the code of four instantiations)
    const int tiles_x = A.W / TW, tiles_y = A.H / TH;
    const int tiles_img = tiles_x * tiles_y;
    const int T = A.N * tiles_img;
    int t_lo, t_hi;
    {
        const int G = (int)gridDim.x, b = (int)blockIdx.x;
        if ((G & 7) == 0) {
            const int xcd = b & 7, idx = b >> 3, nw = G >> 3;
            const long long x0 = (long long)T * xcd / 8, x1 = (long long)T * (xcd + 1) / 8;
            t_lo = (int)(x0 + (x1 - x0) * idx / nw);
            t_hi = (int)(x0 + (x1 - x0) * (idx + 1) / nw);
        } else {
            t_lo = (int)((long long)T * b / G);
            t_hi = (int)((long long)T * (b + 1) / G);
        }
    }
    const int ntl = t_hi - t_lo;
    const int S = ntl * NCH;                                      // chunk steps of this workgroup

    if (S == 0) return;
    // start-up: the movers put their first four halo chunks in flight and fill the scale/shift table while the consumers bring in the
    // resident weights; one barrier, then the movers stage chunks 0 and 1

    auto chunk_src = [&](int k, int &si, int &cc0) {
        const int n0 = A.src[0].C / CK;
        if (k < n0) { si = 0; cc0 = k * CK; } else { si = 1; cc0 = (k - n0) * CK; }
    };

    if (wave >= 4) {
        // ================================ movers ================================
        // Straight-line code only: every load is issued unconditionally (clamped address, clamped chunk index past the end of
        // the run) and out-of-range vectors are zeroed by a mask, so that the compiler can count the loads in flight
        // (s_waitcnt vmcnt(N)) instead of draining them at a join.
        const int ptid = tid - 256;
        // A request takes a chunk PAIR - 32 channels = 64 contiguous bytes of a pixel, a whole
        // sector of the memory side - instead of one chunk's 32 bytes (every sector was requested twice).  Lane -> pixel v / 4, 16-byte segment
        // v % 4 = chunk (v % 4) / 2 of the pair, k-half v % 2; register set R of a pair holds half of the pair's vectors (group R & 1), both sets
        // are written into the pair's two ring slots in the same interval.  The launcher guarantees pairs inside one source (n0 even).
        constexpr int VPQ = 2 * VPP, NG = 2;
        const int slot = ptid % VPQ;
        const int khalf = slot & 1, c2 = slot >> 1;
        u32x4 pa[PF][NA];
        unsigned eo[PF][NA];                     // byte offsets of the requests (read again for a residual operand); bit 31 = zero fill
        // per-thread constants: halo coordinates and LDS offsets of its vectors
        int hyx[NG][NA], doff[NG][NA];
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int v = ptid + (g * NA + i) * 256;
                const int pix = v / VPQ;
                const int hy = pix / HW_, hx = pix - hy * HW_;
                hyx[g][i] = v < NPIX * VPQ ? ((hy << 8) | hx) : 0x1f1f;      // (31 = a vector that never exists: bit 31 of the masks is always set)
                doff[g][i] = pix * PSTR + ((khalf ^ (hy & 1)) * 16);
            }
        // requests go through buffer descriptors, zero fill by bit 31 of the byte offset (persist.h)
        const unsigned src_bytes0 = (unsigned)(A.N * A.npar) * A.src[0].Hs * (A.src[0].row_stride ? A.src[0].row_stride : A.src[0].Ws * A.src[0].C) * 2u;
        const unsigned src_bytes1 = A.nsrc > 1 ? (unsigned)(A.N * A.npar) * A.src[1].Hs * (A.src[1].row_stride ? A.src[1].row_stride : A.src[1].Ws * A.src[1].C) * 2u : 0u;
        // (buf_load128 / halo_bad_mask of persist.h, as local lambdas: the functions changed the code of four instantiations)
        auto bload = [](__amdgpu_buffer_rsrc_t r, unsigned voff) -> u32x4 {
            return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, 0));
        };
        auto bad_mask = [](int lo, int hi) -> unsigned {
            lo = lo < 0 ? 0 : (lo > 31 ? 31 : lo);
            hi = hi < lo ? lo : (hi > 31 ? 31 : hi);
            return ~(((1u << hi) - 1u) & ~((1u << lo) - 1u));
        };
        const __amdgpu_buffer_rsrc_t rsx0 = buf_rsrc(A.src[0].x, src_bytes0);
        const __amdgpu_buffer_rsrc_t rsx1 = buf_rsrc(A.nsrc > 1 ? A.src[1].x : A.src[0].x, src_bytes1);
        const __amdgpu_buffer_rsrc_t rsr0 = buf_rsrc(A.src[0].res ? A.src[0].res : A.src[0].x, src_bytes0);
        const __amdgpu_buffer_rsrc_t rsr1 = buf_rsrc(A.nsrc > 1 && A.src[1].res ? A.src[1].res : A.src[0].x, src_bytes1);
        // cursors (no integer division per chunk): the issue cursor walks chunks 0, 1, 2, ... of the run and stops on the last
        // one; the commit cursor only needs the chunk-in-tile index
        int ik = 0, ic = 0, in_, iy0, ix0;
        seek_tile(t_lo, tiles_img, tiles_x, in_, iy0, ix0);
        int o_n = in_, o_y0 = iy0, o_x0 = ix0;   // out cursor: the tile the consumers are accumulating
        int s_n = 0, s_y0 = 0, s_x0 = 0;         // the finished tile whose out image the consumers park during interval A
        bool s_ok = false;
        int ck = 0;
        // staging geometry of the current tile and source (the chunks of one source share it): element offset of each vector
        // without the chunk's channel offset, validity mask
        unsigned ge[NG][NA];                     // byte offset of channel 0 of the tile's vectors in the current source, bit 31 = zero fill
        const int n0 = A.src[0].C / CK;
        auto issue = [&](auto rc) {
            constexpr int R = decltype(rc)::value;
            constexpr int G = R & 1;                              // which half of the pair's vectors this register set holds
            int si, cc0;
            chunk_src(ik & ~1, si, cc0);                          // (the pair's first chunk: both sets request from its base)
            const ConvSrc &s = A.src[si];
            if ((ik & ~1) == 0 || (ik & ~1) == n0) {
                const int rs = s.row_stride ? s.row_stride : s.Ws * s.C;
                // halo row r <-> y = iy0 - 1 + r, halo column c <-> x = ix0 - 1 + c; valid = inside the image and the source window
                const int ylo = s.off_y > 0 ? s.off_y : 0, yhi = A.H < s.off_y + s.Hs ? A.H : s.off_y + s.Hs;
                const int xlo = s.off_x > 0 ? s.off_x : 0, xhi = A.W < s.off_x + s.Ws ? A.W : s.off_x + s.Ws;
                const unsigned rowbad = bad_mask(ylo - (iy0 - 1), yhi - (iy0 - 1)), colbad = bad_mask(xlo - (ix0 - 1), xhi - (ix0 - 1));
                const unsigned img_b = (unsigned)((in_ * s.Hs + (iy0 - 1 - s.off_y)) * rs + (ix0 - 1 - s.off_x) * s.C) * 2u;
                const unsigned rs_b = (unsigned)rs * 2u, c_b = (unsigned)s.C * 2u;
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    const unsigned hy = (unsigned)hyx[G][i] >> 8, hx = (unsigned)hyx[G][i] & 0xffu;
                    const unsigned t = (rowbad >> hy) | (colbad >> hx);
                    ge[G][i] = ((img_b + hy * rs_b + hx * c_b + (unsigned)slot * 16u) & 0x7fffffffu) | (t << 31);
                }
            }
            const __amdgpu_buffer_rsrc_t rsx = si ? rsx1 : rsx0;
            const unsigned cc0_b = (unsigned)cc0 * 2u;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const unsigned voff = ge[G][i] + cc0_b;                // (a zero-fill vector keeps bit 31: beyond every tensor the launcher admits)
                eo[R][i] = voff;
                pa[R][i] = bload(rsx, voff);
            }
            // advance (saturating at the last chunk of the run)
            if (ic + 1 < S) {
                ++ic;
                if (++ik == NCH) { ik = 0; next_tile(in_, iy0, ix0, A.H, A.W); }
            }
        };
        // chunk c_ of the run (register set R = c_ % 4) -> ring slot c_ % 4
        auto commit = [&](auto rc, int c_) {
            constexpr int R = decltype(rc)::value;
            constexpr int G = R & 1;
            int si, cc0;
            chunk_src(ck & ~1, si, cc0);
            if (c_ + 1 < S) { if (++ck == NCH) ck = 0; }
            const ConvSrc &s = A.src[si];
            const float *xf = s_xf + (si ? c0n : 0) + cc0 + slot * 8;
            float sc[8], sh[8];
            if (XF != 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { sc[j] = xf[j]; sh[j] = xf[xfs + j]; }
            }
            unsigned char *dst0 = lds_a + ((R & 2) + c2) * L::A_BYTES;      // (this thread's vectors belong to chunk c2 of the pair, whichever set R is)
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                u32x4 val;
                if (XF == 0) val = pa[R][i];
                else if (XF == 1) val = xf_bnrelu_f16<false>(pa[R][i], pa[R][i], sc, sh);
                else {
                    ChanXf t;
                    t.on = s.scale != nullptr;
#pragma unroll
                    for (int j = 0; j < 8; ++j) { t.sc[j] = sc[j]; t.sh[j] = sh[j]; }
                    V16 raw, rr;
                    raw.u = __builtin_bit_cast(uint4, pa[R][i]);
                    const bool relu = s.relu != 0, f16 = s.f16 != 0;
                    if (s.res) {
                        rr.u = __builtin_bit_cast(uint4, bload(si ? rsr1 : rsr0, eo[R][i]));
                        val = __builtin_bit_cast(u32x4, xform8(raw, &rr, t, relu, f16).u);
                    } else if (!t.on && !relu && !f16) val = pa[R][i];
                    else val = __builtin_bit_cast(u32x4, xform8(raw, nullptr, t, relu, f16).u);
                }
                if (XF != 0) {                                   // (plain sources: the zero fill arrived as zeros)
                    const unsigned keep = (int)eo[R][i] < 0 ? 0u : 0xffffffffu;
                    val &= keep;
                }
#ifdef CDNET_WS_STAMPS
                if (A.debug & 1024) { if (val[0] == 0x12345678u) *reinterpret_cast<u32x4 *>(dst0 + doff[G][i]) = val; continue; }
#endif
                if (ptid + (G * NA + i) * 256 < NPIX * VPQ)
                    *reinterpret_cast<u32x4 *>(dst0 + doff[G][i]) = val;
            }
        };
        // ---- out path: mover wave w stores the region of consumer wave w.  Piece pc = (M tile mi, pixel half ch, cout pass kk): the four
        // ---- 16-lane groups take four cout octets, lane i of a group receives pixel i of tile row 4w + 2mi + ch (transposing read:
        // ---- lane 4q+p supplies the address of cout row q, pixels 4p..4p+3) -> one 16-byte NHWC store per lane
        constexpr int KO = BN / 32, NP = 4 * KO;
        typedef s16x4 __attribute__((address_space(3))) * lptr;
        const int pw = wave - 4;
        const int lg = lane >> 4, li = lane & 15;
        const unsigned char *s_img = lds_o + pw * L::OUT_WAVE + (li >> 2) * L::IROW + (li & 3) * 8;
        auto store_pieces = [&](bool now) {
            // all transposing reads first, into registers of their own, then the stores: with the pair of reads, the wait for them and
            // the store piece by piece through one register quad (what the compiler makes of a single loop) every piece paid the LDS
            // latency - 1.2 us per tile in the movers' second interval, where the consumers then waited 0.9 us (stamp build)
            s16x4 t1[NP], t2[NP];
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) {
                const int mi = pc / (2 * KO), ch = (pc / KO) % 2, kk = pc % KO;
                const int o = lg + 4 * kk;
                const int ni = o >> 2, r0 = 8 * (o & 3);
                const unsigned char *p = s_img + ((mi * NPW + ni) * 32 + r0) * L::IROW + ch * 32;
                t1[pc] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(p));
                t2[pc] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(p + 4 * L::IROW));
            }
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) {
                const int mi = pc / (2 * KO), ch = (pc / KO) % 2, kk = pc % KO;
                const int o = lg + 4 * kk;
                const int y = s_y0 + pw * 4 + mi * 2 + ch, x = s_x0 + li, co = cout0 + 8 * o;
                if (now && s_ok && co < A.Cout) {
                    const uint2 a = __builtin_bit_cast(uint2, t1[pc]), b2 = __builtin_bit_cast(uint2, t2[pc]);
                    *reinterpret_cast<uint4 *>(A.out + (((size_t)s_n * A.H + y) * A.W + x) * A.out_cstride + A.out_coff + co) = make_uint4(a.x, a.y, b2.x, b2.y);
                }
            }
        };
        // STREAM: weight chunk wk of the tile -> weight slot wk & 3 by LDS-DMA (persist.h); the cursor wraps at the end of a tile
        int wk = 0;
        auto dma_w = [&]() {
            dma_weight_chunk<L::B_CHUNK>(A.w + ((size_t)cout_tile * NCH + wk) * (L::B_CHUNK / 2), lds_w + (wk & 3) * L::B_CHUNK, pw, lane);
            if (++wk == NCH) wk = 0;
        };
        constexpr int NHL = 2 * NA;                               // halo requests of one interval (two chunks): issued after the weight DMA, they
                                                                  // stay in flight over the streaming loop's barrier (barrier_keep_vm, persist.h)
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>;
        issue(I0{});
        issue(I1{});
        issue(I2{});
        issue(I3{});
        for (int c = ptid; c < ctot; c += 256) {
            const ConvSrc &Sx = c < c0n ? A.src[0] : A.src[1];
            const int cc = c < c0n ? c : c - c0n;
            s_xf[c] = Sx.scale ? Sx.scale[cc] : 1.f;
            s_xf[xfs + c] = Sx.shift ? Sx.shift[cc] : 0.f;
        }
        __syncthreads();                                         // table + weights
        commit(I0{}, 0);
        commit(I1{}, 1);
        if (STREAM) { dma_w(); dma_w(); }
        issue(I0{});
        issue(I1{});
        if (STREAM) wait_vmcnt<NHL>();                              // weight chunks 0, 1 have landed (the two halo chunks requested after them stay in flight)
        __syncthreads();
        const int NIT = NCH / 4;                                 // loop iterations (four chunks = two barrier intervals) per tile
        int it = 0;
        // tile j (chunks q0 .. q0+3).  Interval A: the consumers work on chunks q0, q0+1 (slots 0, 1) and park the out image of tile
        // j-1; slots 2, 3 take chunks q0+2, q0+3.  Interval B: the consumers work on slots 2, 3; slots 0, 1 take the first two chunks
        // of tile j+1 and the out image of tile j-1 leaves for global memory.
        if (!STREAM) {
            for (int q0 = 0; q0 < S; q0 += 4) {
                WS_STAMP(1); commit(I2{}, q0 + 2); issue(I2{}); commit(I3{}, q0 + 3); issue(I3{}); WS_STAMP(3); __syncthreads();
                WS_STAMP(1); commit(I0{}, q0 + 4); issue(I0{}); commit(I1{}, q0 + 5); issue(I1{}); WS_STAMP(2); store_pieces(true); WS_STAMP(3); __syncthreads();
                s_n = o_n; s_y0 = o_y0; s_x0 = o_x0; s_ok = true;
                o_x0 += TW;
                if (o_x0 >= A.W) { o_x0 = 0; o_y0 += TH; if (o_y0 >= A.H) { o_y0 = 0; ++o_n; } }
            }
        } else {
            // per interval: the weight DMA of the two chunks after the ones being consumed first, (second interval of a tile: the
            // previous tile's out image), the halo commits and requests last - the explicit wait then leaves exactly the halo
            // requests of this interval in flight
            // (every LDS access of the interval - out-image reads, halo commits - comes BEFORE the DMA: the compiler cannot tell that
            //  the DMA's destination does not alias them and guards any later LDS access of this wave with s_waitcnt vmcnt(0),
            //  which would drain the halo requests in flight)
            for (int q0 = 0; q0 < S; q0 += 4) {
                commit(I2{}, q0 + 2); commit(I3{}, q0 + 3);
                dma_w(); dma_w();
                issue(I2{}); issue(I3{});
                barrier_keep_vm<NHL>();
                store_pieces(it == 0);
                commit(I0{}, q0 + 4); commit(I1{}, q0 + 5);
                dma_w(); dma_w();
                issue(I0{}); issue(I1{});
                barrier_keep_vm<NHL>();
                if (++it == NIT) {
                    it = 0;
                    s_n = o_n; s_y0 = o_y0; s_x0 = o_x0; s_ok = true;
                    o_x0 += TW;
                if (o_x0 >= A.W) { o_x0 = 0; o_y0 += TH; if (o_y0 >= A.H) { o_y0 = 0; ++o_n; } }
                }
            }
        }
        __syncthreads();                                         // the consumers have parked the last tile's out image
        store_pieces(true);
#ifdef CDNET_WS_STAMPS
        if (stamp_on) { for (int i = 0; i < sn; ++i) g_ws_stamps[1024 + i] = s_stamp[i]; g_ws_stamps[1024 + sn] = 0; }
#endif
        return;
    }

    // ================================ consumers ================================
    if (!STREAM) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(A.w + (size_t)cout_tile * 4 * (L::B_CHUNK / 2));
        u32x4 *dst = reinterpret_cast<u32x4 *>(lds_w);
        constexpr int nv = 4 * (L::B_CHUNK / 16), NW = (nv + 255) / 256;
        // all of a thread's vectors in flight at once (one memory round trip for the 74 KB; the accumulators are not live yet)
        u32x4 wv[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) wv[i] = src[tid + i * 256 < nv ? tid + i * 256 : 0];
#pragma unroll
        for (int i = 0; i < NW; ++i)
            if (tid + i * 256 < nv) dst[tid + i * 256] = wv[i];
    }
    __syncthreads();                                             // table + weights
    const int wm = wave;
    const int half = lane >> 5, l31 = lane & 31;
    int abase[MPW][2];                                           // [.][parity of the tap's row offset]: the k-half swizzle follows the halo row
#pragma unroll
    for (int mi = 0; mi < MPW; ++mi) {
        const int m = (wm * MPW + mi) * 32 + l31;
#pragma unroll
        for (int par = 0; par < 2; ++par) abase[mi][par] = ((m / TW) * HW_ + m % TW) * PSTR + ((half ^ ((m / TW + par) & 1)) * 16);
    }
    auto tpar = [](int t) { return (TAPS == 9 ? t / 3 : 1) & 1; };
    const int bbase = half * BN * 16 + l31 * 16;
    auto toff = [](int t) { return ((TAPS == 9 ? t / 3 : 1) * HW_ + (TAPS == 9 ? t % 3 : 1)) * PSTR; };      // folds to immediates
    // two accumulator sets: while one takes the current tile's MFMAs, the other (the finished tile) is converted and parked in the
    // shadow of those MFMAs
    f32x16 accA[MPW][NPW], accB[MPW][NPW];
    // this wave's out image: blocks [mi][ni] of 32 cout rows x 32 pixels; this lane owns cout row l31 of every block
    unsigned char *s_out = lds_o + wave * L::OUT_WAVE + l31 * L::IROW + half * 8;
    // epilogue constants of this lane (the same for every tile of the run)
    float e_osc[NPW], e_osh[NPW];
#pragma unroll
    for (int ni = 0; ni < NPW; ++ni) {
        const int co = cout0 + ni * 32 + l31;
        const bool cok = co < A.Cout;
        e_osc[ni] = (A.oscale && cok) ? A.oscale[co] : 1.f;
        e_osh[ni] = fmaf((A.bias && cok) ? A.bias[co] : 0.f, e_osc[ni], (A.oshift && cok) ? A.oshift[co] : 0.f);
    }
    const bool f16out = A.out_f16 != 0;
    const s16x2 lo_clamp = A.orelu ? s16x2{0, 0} : s16x2{(short)-32768, (short)-32768};

    // ---- epilogue units of a finished accumulator set (full tiles only).  Statistics: registers 4g..4g+3 of block (mi, ni) into the
    // ---- lane's running sums, blocks in the order (ni, mi) - the summation order of conv_fwd_kernel.  Image: bias/scale/shift,
    // ---- 16-bit conversion, ReLU; registers 4g..4g+3 are four consecutive pixels of this lane's cout: one 8-byte LDS write
    constexpr int NU = MPW * NPW * 4;
    float st_sum = 0.f, st_sq = 0.f;
    auto stat_unit = [&](const f32x16 (&P)[MPW][NPW], int u, int par) {
        const int ni = u / (MPW * 4), mi = (u / 4) % MPW, g = u % 4;
        if (mi == 0 && g == 0) { st_sum = 0.f; st_sq = 0.f; }
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float v = P[mi][ni][4 * g + j]; st_sum += v; st_sq = fmaf(v, v, st_sq); }
        if (mi == MPW - 1 && g == 3) {
            float *sp = s_stats + par * (4 * 2 * BN);
            const float a = st_sum + __shfl_xor(st_sum, 32), b2 = st_sq + __shfl_xor(st_sq, 32);
            if (half == 0) {
                sp[(wave * 2 + 0) * BN + ni * 32 + l31] = a;
                sp[(wave * 2 + 1) * BN + ni * 32 + l31] = b2;
            }
        }
    };
    auto img_unit = [&](const f32x16 (&P)[MPW][NPW], int u) {
        const int mi = u / (NPW * 4), ni = (u / 4) % NPW, g = u % 4;
        const float osc = e_osc[ni], osh = e_osh[ni];
        const f32x2 p0 = {fmaf(P[mi][ni][4 * g], osc, osh), fmaf(P[mi][ni][4 * g + 1], osc, osh)};
        const f32x2 p1 = {fmaf(P[mi][ni][4 * g + 2], osc, osh), fmaf(P[mi][ni][4 * g + 3], osc, osh)};
        const s16x2 h0 = __builtin_bit_cast(s16x2, __builtin_convertvector(p0, h16x2)), h1 = __builtin_bit_cast(s16x2, __builtin_convertvector(p1, h16x2));
        const s16x2 b0 = __builtin_bit_cast(s16x2, __builtin_convertvector(p0, bf16x2)), b1 = __builtin_bit_cast(s16x2, __builtin_convertvector(p1, bf16x2));
        const s16x2 k0 = __builtin_elementwise_max(f16out ? h0 : b0, lo_clamp), k1 = __builtin_elementwise_max(f16out ? h1 : b1, lo_clamp);
        *reinterpret_cast<uint2 *>(s_out + (mi * NPW + ni) * L::IBLK + g * 16) = make_uint2(__builtin_bit_cast(unsigned, k0), __builtin_bit_cast(unsigned, k1));
    };
    // slot sl (0 .. 2 * 36 - 1) of interval A -> unit: statistics on the even slots from 0, then the image on the odd slots
    constexpr int SLOTS = TAPS * MPW * NPW;                      // MFMAs of one chunk step
    constexpr int IMG0 = STATS ? 2 * NU + 1 : 0;
    static_assert(IMG0 + 2 * NU <= 2 * SLOTS, "the deferred epilogue fits the MFMA slots of interval A");

    int stats_tile = -1, stats_par = 0;                         // statistics parked in LDS by a finished epilogue
    auto flush_stats = [&]() {
        if (STATS && stats_tile >= 0 && tid < 2 * BN) {
            // per-tile channel sums: the four waves' partials in a fixed order (deterministic)
            const int which = tid / BN, col = tid % BN;
            const float *sp = s_stats + stats_par * (4 * 2 * BN);
            float v = 0.f;
#pragma unroll
            for (int w4 = 0; w4 < 4; ++w4) v += sp[(w4 * 2 + which) * BN + col];
            const int co = cout0 + col;
            if (co < A.Cout) A.stats[((size_t)stats_tile * 2 + which) * A.Cout + co] = v;
        }
        stats_tile = -1;
    };

    // one barrier interval on accumulator set C: two chunks = 2 * TAPS taps of MPW x NPW MFMAs; the fragments of a tap are requested
    // two taps ahead (three fragment sets): with four consumer waves reading, an LDS read issued only one tap (4 MFMAs = 128 cycles)
    // ahead is not back in time and every tap stalls.  FIRST: the tile's first chunk starts from zero.  EPI: the interval carries the
    // epilogue units of the finished set P after its MFMAs (program order = issue order: vector and LDS instructions ride in the MFMA shadow)
    auto interval = [&](auto first_c, auto epi_c, f32x16 (&C)[MPW][NPW], const f32x16 (&P)[MPW][NPW], int par, int c0) {
        constexpr bool FIRST = decltype(first_c)::value;
        constexpr bool EPI = decltype(epi_c)::value;
        constexpr int NTAP = 2 * TAPS;
        bf16x8 af[3][MPW], bfr[3][NPW];
        const unsigned char *la = lds_a + c0 * L::A_BYTES, *lw = lds_w + c0 * L::B_CHUNK;
        auto request = [&](int tau) {
            const int ch = tau / TAPS, t = tau % TAPS;
#pragma unroll
            for (int mi = 0; mi < MPW; ++mi) af[tau % 3][mi] = *reinterpret_cast<const bf16x8 *>(la + ch * L::A_BYTES + abase[mi][tpar(t)] + toff(t));
#pragma unroll
            for (int ni = 0; ni < NPW; ++ni) bfr[tau % 3][ni] = *reinterpret_cast<const bf16x8 *>(lw + ch * L::B_CHUNK + bbase + (t * 2) * BN * 16 + ni * 512);
        };
        request(0);
        request(1);
#pragma unroll
        for (int tau = 0; tau < NTAP; ++tau) {
            if (tau + 2 < NTAP) request(tau + 2);
#pragma unroll
            for (int mi = 0; mi < MPW; ++mi)
#pragma unroll
                for (int ni = 0; ni < NPW; ++ni) {
                    if (FIRST && tau == 0) {
                        const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                        C[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[tau % 3][mi], bfr[tau % 3][ni], z, 0, 0, 0);
                    } else {
                        C[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[tau % 3][mi], bfr[tau % 3][ni], C[mi][ni], 0, 0, 0);
                    }
                    // the gap behind this MFMA: in an epilogue interval, one unit of the finished tile
                    if (EPI) {
                        const int sl = (tau * MPW + mi) * NPW + ni;
                        if (STATS && sl < 2 * NU && (sl & 1) == 0) { __builtin_amdgcn_sched_barrier(0); stat_unit(P, sl / 2, par); __builtin_amdgcn_sched_barrier(0); }
                        if (sl >= IMG0 && sl < IMG0 + 2 * NU && ((sl - IMG0) & 1) == 0) { __builtin_amdgcn_sched_barrier(0); img_unit(P, (sl - IMG0) / 2); __builtin_amdgcn_sched_barrier(0); }
                    }
                }
        }
    };
    using F_ = std::false_type;
    using T_ = std::true_type;
    // tile j on set C; P = the finished tile j-1 (its epilogue rides in interval A)
    auto tile_step = [&](auto has_prev, f32x16 (&C)[MPW][NPW], const f32x16 (&P)[MPW][NPW], int j) {
        constexpr bool HP = decltype(has_prev)::value;
        const int par = (j + 1) & 1;
        WS_STAMP(10);
#ifdef CDNET_WS_STAMPS
        if (A.debug & 512) interval(T_{}, F_{}, C, P, par, 0); else
#endif
        interval(T_{}, has_prev, C, P, par, 0);
        if (HP && STATS) { stats_tile = t_lo + j - 1; stats_par = par; }
        WS_STAMP(11);
        __syncthreads();
        WS_STAMP(14);
        flush_stats();
        interval(F_{}, F_{}, C, P, par, 2);
        WS_STAMP(12);
        __syncthreads();
        WS_STAMP(13);
        if (STREAM) {
            // the rest of a long tile: intervals alternate between the two halves of the rings
            const int NI = NCH / 2;
            for (int i = 2; i < NI; ++i) {
                interval(F_{}, F_{}, C, P, par, (i & 1) * 2);
                __syncthreads();
            }
        }
    };
    // the last tile of the run: nothing left to hide behind
    auto serial_epilogue = [&](const f32x16 (&P)[MPW][NPW], int j) {
        const int par = j & 1;
        if (STATS) {
#pragma unroll
            for (int u = 0; u < NU; ++u) stat_unit(P, u, par);
            stats_tile = t_lo + j;
            stats_par = par;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) img_unit(P, u);
    };

    __syncthreads();                                             // chunks 0, 1 are staged
    tile_step(F_{}, accA, accB, 0);
    int j = 1;
    for (; j + 1 < ntl; j += 2) {
        tile_step(T_{}, accB, accA, j);
        tile_step(T_{}, accA, accB, j + 1);
    }
    if (j < ntl) {
        tile_step(T_{}, accB, accA, j);
        serial_epilogue(accB, j);
    } else {
        serial_epilogue(accA, ntl - 1);
    }
    __syncthreads();
    flush_stats();
#ifdef CDNET_WS_STAMPS
    if (stamp_on) { for (int i = 0; i < sn; ++i) g_ws_stamps[i] = s_stamp[i]; g_ws_stamps[sn] = 0; }
#endif
}

// eligibility + launch of the wave-specialised kernel; returns -1 when the layer must take conv_fwd_kernel
template <int BN, int TAPS>
int try_launch_conv_ws(const ConvArgs &A, hipStream_t st, bool dry_run = false) {
    using L = WsLds<BN, TAPS>;
    int ctot = 0;
    if (A.ws == 2) return -1;                                    // (BatchNorm-backward sums beside the stores: the fp32 kernel only, conv32ws.hip)
    if (A.eres) return -1;                                       // fused residual epilogues stay on conv_fwd_kernel
    if (A.nchunk < 4 || A.nchunk % 4 != 0) return -1;            // whole pairs of barrier intervals (two chunks each) per tile
    if ((A.src[0].C / 16) & 1) return -1;                        // (the movers request by chunk pairs: every pair inside one source)
    const bool stream = A.nchunk != 4;                           // 128+ input channels / two sources: the weight chunks stream through the LDS
    if (A.H % 16 != 0 || A.W % 16 != 0) return -1;               // full tiles only
    for (int i = 0; i < A.nsrc; ++i) {
        if (A.src[i].pool || A.src[i].relu == 3) return -1;
        ctot += A.src[i].C;
        if (!in_mover_reach(A.src[i], (long long)A.N * A.npar, 2)) return -1;
    }
#ifdef CDNET_WS_STAMPS
    const int smem = L::bytes(4, ctot, 2) + 2 * 384 * 8;
#else
    const int smem = L::bytes(4, ctot, 2);
#endif
    if (smem > 160 * 1024) return -1;
    const int T = (A.W / 16) * (A.H / 16) * A.N;
    int n_cu = 0;
    if (const int rc = cu_count(&n_cu)) return rc;
    const int ctiles = cdiv(A.Cout, BN);
    // a persistent workgroup pays ~3 us of start-up (weights + first chunks): worth it from a few tiles' worth of chunks per workgroup on
    const int Gmax = n_cu / ctiles > 0 ? n_cu / ctiles : 1;
    // (few tiles but long channel loops - the 16x16-pixel bottleneck layers - still take it: the workgroups that exist keep the memory
    //  pipeline full, which the one-tile-per-workgroup kernel does not)
    // (12, not 16: the decoder's first block - 768 -> 256 channels on 16 tiles of 16 x 16 pixels, 64 workgroups either way - 120 us on the one-tile kernel)
    if (!(A.debug & CONV_DBG_PERSIST_SMALL) && ((long long)T * A.nchunk < 12LL * Gmax || (T < Gmax && A.nchunk < 16))) return -1;
    bool all_plain = true, all_fast = true;
    for (int i = 0; i < A.nsrc; ++i) {
        const ConvSrc &s = A.src[i];
        all_plain = all_plain && !s.scale && !s.relu && !s.res && !s.f16;
        all_fast = all_fast && s.scale && s.relu && !s.res && s.f16 == 1;
    }
    // (no test cap: conv_ws_kernel reads debug bits 512 and 1024 as ablations of its own)
    dim3 grid(persistent_grid(n_cu, ctiles, T, 0, 0), ctiles, 1);
    const int xf = all_plain ? 0 : (all_fast ? 1 : 2);
    if (dry_run) return CDNET_OK;
    return with_bool(A.stats != nullptr, [&](auto st_c) {
        return with_int<0, 1, 2>(xf, [&](auto xf_c) {
            return with_bool(stream, [&](auto sm_c) {
                g_conv_last_form = conv_form(CDNET_CONV_FAMILY_WS, BN, TAPS, decltype(xf_c)::value, decltype(st_c)::value, decltype(sm_c)::value);
                return launch_lds<conv_ws_kernel<BN, TAPS, decltype(xf_c)::value, decltype(st_c)::value, decltype(sm_c)::value>>(
                    grid, 512, 160 * 1024, smem, st, "hipFuncSetAttribute(conv_ws)", "conv_ws_kernel", A);
            });
        });
    });
}

}  // namespace

namespace cdnet {
int conv_forward_ws(const ConvArgs &A, hipStream_t st, bool dry_run) {
    if (A.taps != 9 || A.npar != 1 || A.ostride != 1 || A.tile != 16 || A.CK != 16 || (A.BN != 64 && A.BN != 32)) return -1;
    return A.BN == 64 ? try_launch_conv_ws<64, 9>(A, st, dry_run) : try_launch_conv_ws<32, 9>(A, st, dry_run);
}
}  // namespace cdnet
