// Instance-segmentation metrics (stats_utils.py: get_fast_aji :7-106, get_fast_pq :182-276, get_dice_1 :323-335,
// remap_label :361-392): the O(pixels) part - per-label areas and the sparse table of pairwise intersections between
// ground-truth and predicted instances - in one pass over the two label images; the O(pairs) arithmetic stays on the host
// in float64 with the reference's exact formulas (cdnet_amd/stats_utils.py).  Replaces the reference's
// O(instances_true x pixels) mask loops.
//
// Object-level Hausdorff distances (utils.py:303, scipy's directed_hausdorff on both sides of every matched pair): a per-label list of
// pixel coordinates and one of boundary pixels per image (count, prefix sum, scatter), then one launch over (pair, direction, tile of A)
// that keeps, for every pixel of A outside B, the minimum squared distance to B's boundary and folds the maximum into d2[pair][dir].
// Integer min / max only, so the result depends neither on the order inside the lists nor on the order of the atomics.  A pixel of A
// outside B is never nearest to an interior pixel of B (all four neighbours of an interior pixel are in B, and the one towards the
// pixel along an axis where they differ is closer), so B's boundary list is enough.
#include "common.h"

using namespace cdnet;

namespace {

// open-addressing table per image: key = (true_id << 16) | pred_id (ids < 65536), 0 = empty (id pairs with a zero id
// are never inserted)
__global__ __launch_bounds__(256) void pair_hist_kernel(const int32_t *__restrict__ t, const int32_t *__restrict__ p, int plane, int cap,
                                                        unsigned hmask, int *__restrict__ area_t, int *__restrict__ area_p,
                                                        unsigned *__restrict__ hkeys, int *__restrict__ hcnt, int *__restrict__ err) {
    const int n = blockIdx.y;
    const size_t base = (size_t)n * plane;
    int *at = area_t + (size_t)n * cap, *ap = area_p + (size_t)n * cap;
    unsigned *hk = hkeys + (size_t)n * (hmask + 1);
    int *hc = hcnt + (size_t)n * (hmask + 1);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) {
        const int a = t[base + i], b = p[base + i];
        if (a < 0 || b < 0 || a >= cap || b >= cap) { *err = 1; continue; }
        if (a > 0) atomicAdd(at + a, 1);
        if (b > 0) atomicAdd(ap + b, 1);
        if (a > 0 && b > 0) {
            const unsigned key = ((unsigned)a << 16) | (unsigned)b;
            unsigned h = (key * 2654435761u) & hmask;
            for (unsigned probe = 0; probe <= hmask; ++probe) {
                const unsigned cur = atomicCAS(hk + h, 0u, key);
                if (cur == 0u || cur == key) { atomicAdd(hc + h, 1); break; }
                h = (h + 1) & hmask;
                if (probe == hmask) *err = 2;          // table full
            }
        }
    }
}

// remap_label: ids -> 1..K in increasing id order (stats_utils.py:361-392, by_size = False)
__global__ __launch_bounds__(256) void label_present_kernel(const int32_t *__restrict__ lab, int plane, int cap, int *__restrict__ present,
                                                            int *__restrict__ err) {
    const int n = blockIdx.y;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) {
        const int a = lab[(size_t)n * plane + i];
        if (a < 0 || a >= cap) { *err = 1; continue; }
        if (a > 0) present[(size_t)n * cap + a] = 1;
    }
}

__global__ __launch_bounds__(256) void label_rank_kernel(int cap, int *__restrict__ present) {
    // one block per image: in-place exclusive scan + 1 for present ids (serial over 256-wide strips; cap is small)
    __shared__ int s[256];
    __shared__ int carry;
    int *pr = present + (size_t)blockIdx.x * cap;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < cap; b0 += 256) {
        const int i = b0 + threadIdx.x;
        const int v = (i < cap && i > 0) ? pr[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int add = threadIdx.x >= o ? s[threadIdx.x - o] : 0;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < cap) pr[i] = v ? carry + s[threadIdx.x] : 0;
        __syncthreads();
        if (threadIdx.x == 255) carry += s[255];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void label_apply_kernel(const int32_t *__restrict__ lab, int plane, int cap, const int *__restrict__ rank,
                                                          int32_t *__restrict__ out) {
    const int n = blockIdx.y;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) {
        const int a = lab[(size_t)n * plane + i];
        out[(size_t)n * plane + i] = (a > 0 && a < cap) ? rank[(size_t)n * cap + a] : 0;
    }
}

// per-label areas alone (remap_label by_size = True)
__global__ __launch_bounds__(256) void label_area_kernel(const int32_t *__restrict__ lab, int plane, int cap, int *__restrict__ area,
                                                         int *__restrict__ err) {
    const int n = blockIdx.y;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) {
        const int a = lab[(size_t)n * plane + i];
        if (a < 0 || a >= cap) { *err = 1; continue; }
        if (a > 0) atomicAdd(area + (size_t)n * cap + a, 1);
    }
}

// ---- per-label coordinate lists -------------------------------------------------------------------------------------------------------
// tab[4][cap] of one image: pixels per id, boundary pixels per id, start of the id's segment in pix, start in bpix
enum { TAB_COUNT = 0, TAB_BCOUNT = 1, TAB_START = 2, TAB_BSTART = 3 };

// boundary pixel: on the image edge, or a 4-neighbour carries another id
__device__ __forceinline__ bool is_boundary(const int32_t *__restrict__ lab, int a, int y, int x, int H, int W) {
    if (y == 0 || x == 0 || y == H - 1 || x == W - 1) return true;
    const int32_t *c = lab + (size_t)y * W + x;
    return c[-W] != a || c[W] != a || c[-1] != a || c[1] != a;
}

__global__ __launch_bounds__(256) void csr_count_kernel(const int32_t *__restrict__ lab, int H, int W, int cap, int *__restrict__ tab,
                                                        int *__restrict__ err) {
    const int plane = H * W;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) {
        const int a = lab[i];
        if (a < 0 || a >= cap) { *err = 1; continue; }
        if (a == 0) continue;
        const int y = i / W, x = i - y * W;
        atomicAdd(tab + TAB_COUNT * cap + a, 1);
        if (is_boundary(lab, a, y, x, H, W)) atomicAdd(tab + TAB_BCOUNT * cap + a, 1);
    }
}

// one block: exclusive prefix sums of the two count rows into the two start rows and into the scatter cursors.  Each thread owns a
// contiguous run of ids (cap <= 65536: at most 256 each).
__global__ __launch_bounds__(256) void csr_scan_kernel(int cap, int *__restrict__ tab, int *__restrict__ cursor) {
    __shared__ int s[2][256];
    const int per = (cap + 255) / 256, i0 = threadIdx.x * per, i1 = min(cap, i0 + per);
    int sum[2] = {0, 0};
    for (int i = i0; i < i1; ++i) { sum[0] += tab[TAB_COUNT * cap + i]; sum[1] += tab[TAB_BCOUNT * cap + i]; }
    s[0][threadIdx.x] = sum[0];
    s[1][threadIdx.x] = sum[1];
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int a0 = threadIdx.x >= o ? s[0][threadIdx.x - o] : 0, a1 = threadIdx.x >= o ? s[1][threadIdx.x - o] : 0;
        __syncthreads();
        s[0][threadIdx.x] += a0;
        s[1][threadIdx.x] += a1;
        __syncthreads();
    }
    int run[2] = {s[0][threadIdx.x] - sum[0], s[1][threadIdx.x] - sum[1]};
    for (int i = i0; i < i1; ++i) {
        tab[TAB_START * cap + i] = cursor[i] = run[0];
        tab[TAB_BSTART * cap + i] = cursor[cap + i] = run[1];
        run[0] += tab[TAB_COUNT * cap + i];
        run[1] += tab[TAB_BCOUNT * cap + i];
    }
}

__global__ __launch_bounds__(256) void csr_scatter_kernel(const int32_t *__restrict__ lab, int H, int W, int cap, int *__restrict__ cursor,
                                                          int32_t *__restrict__ pix, int32_t *__restrict__ bpix) {
    const int plane = H * W;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += gridDim.x * blockDim.x) {
        const int a = lab[i];
        if (a <= 0 || a >= cap) continue;
        const int y = i / W, x = i - y * W, yx = (y << 16) | x;
        const int at = atomicAdd(cursor + a, 1);
        if (at < plane) pix[at] = yx;                       // (always, unless the image changed between the launches)
        if (is_boundary(lab, a, y, x, H, W)) {
            const int bt = atomicAdd(cursor + cap + a, 1);
            if (bt < plane) bpix[bt] = yx;
        }
    }
}

// ---- pairs ----------------------------------------------------------------------------------------------------------------------------
constexpr int HD_THREADS = 256, HD_REG = 4;
constexpr int HD_TILE = HD_THREADS * HD_REG;        // pixels of A per block, HD_REG in the registers of each thread
constexpr int HD_CHUNK = 1024;                      // boundary pixels of B per LDS pass

// one image's lists
struct HdSide {
    const int32_t *lab, *tab, *pix, *bpix;
};

// item = (2 * pair + direction, tile of A).  direction 0: A = the predicted object, B = the true one (h(P -> T)); 1: the reverse.
// d2[2 * pair + direction] = max over A's pixels outside B of the min over B's boundary of the squared distance; 0 when A lies in B.
__global__ __launch_bounds__(HD_THREADS) void hausdorff_pair_kernel(HdSide T, HdSide P, int W, int plane, int cap, const int32_t *__restrict__ pairs,
                                                                    int M, const int32_t *__restrict__ items, int *__restrict__ d2,
                                                                    int *__restrict__ err) {
    __shared__ int2 sb[HD_CHUNK];
    __shared__ int smax;
    const int slot = items[2 * blockIdx.x], tile = items[2 * blockIdx.x + 1];
    const int m = slot >> 1, dir = slot & 1;
    if (slot < 0 || m >= M || tile < 0) { if (threadIdx.x == 0) *err = 3; return; }
    const int idT = pairs[2 * m], idP = pairs[2 * m + 1];
    if (idT <= 0 || idP <= 0 || idT >= cap || idP >= cap) { if (threadIdx.x == 0) *err = 1; return; }
    const HdSide &A = dir == 0 ? P : T, &B = dir == 0 ? T : P;
    const int idA = dir == 0 ? idP : idT, idB = dir == 0 ? idT : idP;
    const int nA = A.tab[TAB_COUNT * cap + idA], a0 = A.tab[TAB_START * cap + idA];
    const int nB = B.tab[TAB_BCOUNT * cap + idB], b0 = B.tab[TAB_BSTART * cap + idB];
    if (nA <= 0 || nB <= 0 || a0 < 0 || b0 < 0 || (long long)a0 + nA > plane || (long long)b0 + nB > plane) {
        if (threadIdx.x == 0) *err = 3;                     // an id without pixels, or lists that are not this image's
        return;
    }
    if ((long long)tile * HD_TILE >= nA) return;
    if (threadIdx.x == 0) smax = 0;

    // this thread's pixels of A; the ones inside B (distance 0) and the ones past the end of the list stay idle
    int ay[HD_REG], ax[HD_REG], mn[HD_REG];
    bool live[HD_REG];
    int any = 0;
#pragma unroll
    for (int r = 0; r < HD_REG; ++r) {
        const int k = tile * HD_TILE + r * HD_THREADS + threadIdx.x;
        live[r] = false;
        ay[r] = ax[r] = 0;
        mn[r] = 0x7fffffff;
        if (k < nA) {
            const int yx = A.pix[a0 + k];
            ay[r] = yx >> 16;
            ax[r] = yx & 0xffff;
            const long long at = (long long)ay[r] * W + ax[r];
            live[r] = at < plane && B.lab[at] != idB;
        }
        any |= live[r];
    }
    if (!__syncthreads_or(any)) return;                     // the whole tile lies inside B

    for (int c0 = 0; c0 < nB; c0 += HD_CHUNK) {
        const int nc = min(HD_CHUNK, nB - c0);
        __syncthreads();
        for (int j = threadIdx.x; j < nc; j += HD_THREADS) {
            const int yx = B.bpix[b0 + c0 + j];
            sb[j] = make_int2(yx >> 16, yx & 0xffff);          // .x = row, .y = column
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < nc; ++j) {
            const int2 b = sb[j];                           // every lane reads the same address: a broadcast
#pragma unroll
            for (int r = 0; r < HD_REG; ++r) {
                const int dy = ay[r] - b.x, dx = ax[r] - b.y;     // |dy|, |dx| <= 32766: 24-bit products, the sum below 2^31
                mn[r] = min(mn[r], __mul24(dy, dy) + __mul24(dx, dx));
            }
        }
    }
    int mx = 0;
#pragma unroll
    for (int r = 0; r < HD_REG; ++r)
        if (live[r]) mx = max(mx, mn[r]);
    if (mx > 0) atomicMax(&smax, mx);
    __syncthreads();
    if (threadIdx.x == 0 && smax > 0) atomicMax(d2 + slot, smax);
}

inline int glin(int plane) { int g = cdiv(plane, 256); return g > 1024 ? 1024 : (g < 1 ? 1 : g); }

}  // namespace

extern "C" int cdnet_label_pair_histogram(const int32_t *true_lab, const int32_t *pred_lab, int N, int plane, int cap, int hash_slots,
                                          int32_t *area_true, int32_t *area_pred, uint32_t *hash_keys, int32_t *hash_counts,
                                          int32_t *err_flag, void *stream) {
    CDNET_REQUIRE(true_lab && pred_lab && area_true && area_pred && hash_keys && hash_counts && err_flag, "cdnet_label_pair_histogram: null pointer");
    CDNET_REQUIRE(N > 0 && plane > 0 && cap > 1 && cap <= 65536, "cdnet_label_pair_histogram: label capacity %d not in (1, 65536]", cap);
    CDNET_REQUIRE(hash_slots >= 2 && (hash_slots & (hash_slots - 1)) == 0, "cdnet_label_pair_histogram: hash_slots must be a power of two");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(area_true, 0, (size_t)N * cap * 4, st) != hipSuccess || hipMemsetAsync(area_pred, 0, (size_t)N * cap * 4, st) != hipSuccess ||
        hipMemsetAsync(hash_keys, 0, (size_t)N * hash_slots * 4, st) != hipSuccess ||
        hipMemsetAsync(hash_counts, 0, (size_t)N * hash_slots * 4, st) != hipSuccess || hipMemsetAsync(err_flag, 0, 4, st) != hipSuccess)
        return check_launch("cdnet_label_pair_histogram(memset)");
    pair_hist_kernel<<<dim3(glin(plane), N), 256, 0, st>>>(true_lab, pred_lab, plane, cap, (unsigned)hash_slots - 1, area_true, area_pred,
                                                           hash_keys, hash_counts, err_flag);
    return check_launch("cdnet_label_pair_histogram");
}

extern "C" int cdnet_remap_label(const int32_t *lab, int N, int plane, int cap, int32_t *scratch, int32_t *out, int32_t *err_flag,
                                 void *stream) {
    CDNET_REQUIRE(lab && scratch && out && err_flag, "cdnet_remap_label: null pointer");
    CDNET_REQUIRE(N > 0 && plane > 0 && cap > 1, "cdnet_remap_label: bad size");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(scratch, 0, (size_t)N * cap * 4, st) != hipSuccess || hipMemsetAsync(err_flag, 0, 4, st) != hipSuccess)
        return check_launch("cdnet_remap_label(memset)");
    label_present_kernel<<<dim3(glin(plane), N), 256, 0, st>>>(lab, plane, cap, scratch, err_flag);
    label_rank_kernel<<<N, 256, 0, st>>>(cap, scratch);
    label_apply_kernel<<<dim3(glin(plane), N), 256, 0, st>>>(lab, plane, cap, scratch, out);
    return check_launch("cdnet_remap_label");
}

extern "C" int cdnet_label_areas(const int32_t *lab, int N, int plane, int cap, int32_t *area, int32_t *err_flag, void *stream) {
    CDNET_REQUIRE(lab && area && err_flag, "cdnet_label_areas: null pointer");
    CDNET_REQUIRE(N > 0 && plane > 0 && cap > 1, "cdnet_label_areas: bad size");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(area, 0, (size_t)N * cap * 4, st) != hipSuccess || hipMemsetAsync(err_flag, 0, 4, st) != hipSuccess)
        return check_launch("cdnet_label_areas(memset)");
    label_area_kernel<<<dim3(glin(plane), N), 256, 0, st>>>(lab, plane, cap, area, err_flag);
    return check_launch("cdnet_label_areas");
}

extern "C" int cdnet_label_apply(const int32_t *lab, int N, int plane, int cap, const int32_t *lut, int32_t *out, void *stream) {
    CDNET_REQUIRE(lab && lut && out, "cdnet_label_apply: null pointer");
    CDNET_REQUIRE(N > 0 && plane > 0 && cap > 1, "cdnet_label_apply: bad size");
    label_apply_kernel<<<dim3(glin(plane), N), 256, 0, (hipStream_t)stream>>>(lab, plane, cap, lut, out);
    return check_launch("cdnet_label_apply");
}

extern "C" size_t cdnet_label_csr_workspace_bytes(int cap) { return cap > 1 && cap <= 65536 ? (size_t)2 * cap * 4 : 0; }

extern "C" int cdnet_label_csr(const int32_t *lab, int H, int W, int cap, void *workspace, size_t workspace_bytes, int32_t *tab, int32_t *pix,
                               int32_t *bpix, int32_t *err_flag, void *stream) {
    CDNET_REQUIRE(lab && workspace && tab && pix && bpix && err_flag, "cdnet_label_csr: null pointer");
    CDNET_REQUIRE(H > 0 && W > 0 && H <= 32767 && W <= 32767, "cdnet_label_csr: image %d x %d not within 32767 x 32767", H, W);
    CDNET_REQUIRE((long long)H * W <= 0x7fffffffLL, "cdnet_label_csr: more than 2^31 - 1 pixels");
    CDNET_REQUIRE(cap > 1 && cap <= 65536, "cdnet_label_csr: label capacity %d not in (1, 65536]", cap);
    CDNET_REQUIRE(workspace_bytes >= cdnet_label_csr_workspace_bytes(cap), "cdnet_label_csr: workspace of %zu bytes, %zu needed", workspace_bytes,
                  cdnet_label_csr_workspace_bytes(cap));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(tab, 0, (size_t)2 * cap * 4, st) != hipSuccess || hipMemsetAsync(err_flag, 0, 4, st) != hipSuccess)
        return check_launch("cdnet_label_csr(memset)");
    const int g = glin(H * W);
    csr_count_kernel<<<g, 256, 0, st>>>(lab, H, W, cap, tab, err_flag);
    csr_scan_kernel<<<1, 256, 0, st>>>(cap, tab, (int *)workspace);
    csr_scatter_kernel<<<g, 256, 0, st>>>(lab, H, W, cap, (int *)workspace, pix, bpix);
    return check_launch("cdnet_label_csr");
}

extern "C" int cdnet_hausdorff_tile_pixels(void) { return HD_TILE; }
extern "C" int cdnet_hausdorff_chunk_pixels(void) { return HD_CHUNK; }

extern "C" int cdnet_hausdorff_pairs(const int32_t *true_lab, const int32_t *true_tab, const int32_t *true_pix, const int32_t *true_bpix,
                                     const int32_t *pred_lab, const int32_t *pred_tab, const int32_t *pred_pix, const int32_t *pred_bpix, int H,
                                     int W, int cap, const int32_t *pairs, int M, const int32_t *items, int n_items, int32_t *d2,
                                     int32_t *err_flag, void *stream) {
    CDNET_REQUIRE(true_lab && true_tab && true_pix && true_bpix && pred_lab && pred_tab && pred_pix && pred_bpix && pairs && d2 && err_flag,
                  "cdnet_hausdorff_pairs: null pointer");
    CDNET_REQUIRE(H > 0 && W > 0 && H <= 32767 && W <= 32767, "cdnet_hausdorff_pairs: image %d x %d not within 32767 x 32767", H, W);
    CDNET_REQUIRE((long long)H * W <= 0x7fffffffLL, "cdnet_hausdorff_pairs: more than 2^31 - 1 pixels");
    CDNET_REQUIRE(cap > 1 && cap <= 65536, "cdnet_hausdorff_pairs: label capacity %d not in (1, 65536]", cap);
    CDNET_REQUIRE(M > 0 && M <= (1 << 29) && n_items >= 0 && (items || n_items == 0), "cdnet_hausdorff_pairs: bad pair or item count");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d2, 0, (size_t)M * 2 * 4, st) != hipSuccess || hipMemsetAsync(err_flag, 0, 4, st) != hipSuccess)
        return check_launch("cdnet_hausdorff_pairs(memset)");
    if (n_items == 0) return CDNET_OK;
    const HdSide T{true_lab, true_tab, true_pix, true_bpix}, P{pred_lab, pred_tab, pred_pix, pred_bpix};
    hausdorff_pair_kernel<<<n_items, HD_THREADS, 0, st>>>(T, P, W, H * W, cap, pairs, M, items, d2, err_flag);
    return check_launch("cdnet_hausdorff_pairs");
}
