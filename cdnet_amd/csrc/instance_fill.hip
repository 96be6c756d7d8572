// Per-instance re-dilation of a label map: the closing loop of postproc_other.process for 'micronet' (postproc_other.py:56-68, the 3 x 3
// cross) and 'dcan' (:81-97, k_disk).  Both structuring elements are diamonds S_r = {|dx| + |dy| <= r}, r = 1 and r = 3.  For every id k:
//
//   D_k = binary_dilation(lab == k, S_r)        outside the image counts as background (cv2.dilate's default border on a 0/1 image)
//   F_k = binary_fill_holes(D_k)                a pixel outside D_k is a hole when no 4-connected path outside D_k reaches the image's outside
//   canvas[F_k] = k, k ascending                = out(p) = max{k : p in F_k}, 0 where no F_k covers p
//
// All of F_k lies in the bounding box of k grown by r (clipped to the image): outside that window nothing belongs to D_k and every pixel is
// joined to the exterior, so every window-border pixel outside D_k is a flood seed and the flood never has to leave the window.
//
// Three steps.  (1) One pass over the pixels takes the bounding box of every id: only the first and the last pixel of a row run touch the
// box, with atomicMax on (W-1-x, H-1-y, x, y), behind a plain compare.  (2) A pass over the ids lists the present ones, windows that fit the
// LDS form from the front of the list, the others from its back.  (3) One wave per listed instance works on two bit planes of 64-bit row
// words, bit j of word w = window column 64 w + j:
//   `open`  = window bits outside D_k.  lab == k is gathered with wave ballots (64 adjacent pixels per load), D_k is the OR of the rows
//             y-r..y+r, each spread sideways by r - |dy| across the word boundaries.
//   `reach` = the flood: seeded with the window-border bits of `open`, then grown until a pass changes nothing.  A pass spreads along
//             every row (one lane per row; inside a word the carry of `open + reach` runs through a whole run of open bits at once, the
//             word's neighbours hand over one bit), then sweeps down and up (one lane per word column, spreading inside the word as it
//             goes, so a straight corridor takes one pass).
//   F_k     = window bits not in `reach`, painted with atomicMax into the zeroed output: the maximum does not depend on the order.
// Every pass that does not end the loop sets at least one bit of `reach`, so rows x columns + 1 passes cannot be exceeded; the loop counts
// them and leaves with err_flag 2 rather than trust that.
// Windows up to IF_ROWS x IF_COLS keep both planes in LDS (20 KB per wave: eight waves of different instances share a CU).  Larger ones run
// the same code on planes in the workspace, one wave per image taking its image's large instances in turn.
#include "launch.h"

using namespace cdnet;

namespace {

typedef unsigned long long u64;

constexpr int IF_ROWS = 256, IF_COLS = 256;                    // the LDS form's window capacity
constexpr int IF_STRIDE = (IF_COLS / 64) | 1;                  // odd row stride in words: rows of a 2- or 4-word window fall on different banks
constexpr int IF_PLANE = IF_ROWS * IF_STRIDE;                  // words per LDS plane
constexpr int IF_LDS = 2 * IF_PLANE * 8;
constexpr int IF_MAX_R = 3;
constexpr int IF_GRID = 2048;

__device__ __forceinline__ void raise_to(int *p, int v) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(p, v);
}

// box[N][cap][4] = max of (W-1-x, H-1-y, x, y) over the pixels of id k = 1..cap (slot k-1), -1 where the id is absent
__global__ __launch_bounds__(256) void if_box_kernel(const int32_t *__restrict__ lab, int H, int W, int cap, int *__restrict__ box,
                                                     int *__restrict__ err) {
    const int plane = H * W;
    const int32_t *L = lab + (size_t)blockIdx.y * plane;
    int *B = box + (size_t)blockIdx.y * cap * 4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < plane; i += gridDim.x * 256) {
        const int a = L[i];
        if (a == 0) continue;
        if (a < 0 || a > cap) { *err = 1; continue; }
        const int y = i / W, x = i - y * W;
        int *b = B + (size_t)(a - 1) * 4;
        if (x == 0 || L[i - 1] != a) { raise_to(b, W - 1 - x); raise_to(b + 1, H - 1 - y); raise_to(b + 3, y); }
        if (x == W - 1 || L[i + 1] != a) raise_to(b + 2, x);
    }
}

struct Window { int x0, y0, rows, cols; };

__device__ __forceinline__ Window window_of(const int *b, int H, int W, int r) {
    Window w;
    w.x0 = max(W - 1 - b[0] - r, 0);
    w.y0 = max(H - 1 - b[1] - r, 0);
    w.cols = min(b[2] + r, W - 1) - w.x0 + 1;
    w.rows = min(b[3] + r, H - 1) - w.y0 + 1;
    return w;
}

// list[0 .. cnt[0]) = entries n * cap + k - 1 whose window fits the LDS form; list[total - cnt[1] .. total) = the others
__global__ __launch_bounds__(256) void if_list_kernel(const int *__restrict__ box, int total, int H, int W, int r, int *__restrict__ list,
                                                      int *__restrict__ cnt) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int *b = box + (size_t)e * 4;
        if (b[2] < 0) continue;
        const Window w = window_of(b, H, W, r);
        if (w.rows <= IF_ROWS && w.cols <= IF_COLS) list[atomicAdd(cnt, 1)] = e;
        else list[total - 1 - atomicAdd(cnt + 1, 1)] = e;
    }
}

// r (a subset of m) spread through the runs of set bits of m: the carry of m + r clears a run from its lowest seed upward
__device__ __forceinline__ u64 spread(u64 r, u64 m) {
    const u64 up = ((m ^ (m + r)) & m) | r;
    const u64 mr = __brevll(m), rr = __brevll(r);
    return up | __brevll(((mr ^ (mr + rr)) & mr) | rr);
}

// One instance by one wave.  L, O: the image's labels and output; open_, reach: planes of at least rows * stride words.
__device__ __forceinline__ void instance_fill(const int32_t *__restrict__ L, int32_t *__restrict__ O, int W, int r, int k, Window win, u64 *open_,
                                              u64 *reach, int stride, int *__restrict__ err) {
    const int lane = threadIdx.x;
    const int rows = win.rows, cols = win.cols, ww = (cols + 63) >> 6, items = rows * ww;
    const u64 tail = (cols & 63) ? (1ull << (cols & 63)) - 1 : ~0ull;          // the valid bits of a row's last word
    // lab == k as a bit plane (in `reach` for now): one ballot per word, four loads in flight
    for (int it0 = 0; it0 < items; it0 += 4) {
        int v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int it = it0 + j, row = it / ww, w = it - row * ww, x = w * 64 + lane;
            v[j] = (it < items && x < cols) ? L[(size_t)(win.y0 + row) * W + win.x0 + x] : 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int it = it0 + j, row = it / ww, w = it - row * ww;
            const u64 bits = __ballot(v[j] == k);
            if (lane == 0 && it < items) reach[row * stride + w] = bits;
        }
    }
    __syncthreads();
    // open = not D_k
    for (int it = lane; it < items; it += WAVE) {
        const int row = it / ww, w = it - row * ww;
        u64 d = 0;
        for (int dy = -r; dy <= r; ++dy) {
            const int yy = row + dy, s = r - (dy < 0 ? -dy : dy);
            if (yy < 0 || yy >= rows) continue;
            const u64 *M = reach + yy * stride;
            const u64 m = M[w], lo = w > 0 ? M[w - 1] : 0, hi = w + 1 < ww ? M[w + 1] : 0;
            d |= m;
            for (int t = 1; t <= s; ++t) d |= (m << t) | (m >> t) | (lo >> (64 - t)) | (hi << (64 - t));
        }
        open_[row * stride + w] = ~d & (w == ww - 1 ? tail : ~0ull);
    }
    __syncthreads();
    // seeds: the window's border
    for (int it = lane; it < items; it += WAVE) {
        const int row = it / ww, w = it - row * ww;
        u64 edge = ~0ull;
        if (row > 0 && row < rows - 1) edge = (w == 0 ? 1ull : 0ull) | (w == ww - 1 ? 1ull << ((cols - 1) & 63) : 0ull);
        reach[row * stride + w] = open_[row * stride + w] & edge;
    }
    __syncthreads();
    const long long bound = (long long)rows * cols + 1;
    for (long long pass = 0;; ++pass) {
        if (pass >= bound) {                                    // cannot happen (see the head of the file): never spin
            if (lane == 0) *err = 2;
            return;
        }
        bool changed = false;
        for (int row = lane; row < rows; row += WAVE) {
            u64 *R = reach + row * stride;
            const u64 *M = open_ + row * stride;
            u64 carry = 0;
            for (int w = 0; w < ww; ++w) {
                const u64 m = M[w], v = R[w], nv = spread(v | (carry & m), m);
                if (nv != v) { R[w] = nv; changed = true; }
                carry = nv >> 63;
            }
            carry = 0;
            for (int w = ww - 1; w >= 0; --w) {
                const u64 m = M[w], v = R[w], nv = spread(v | (carry & m), m);
                if (nv != v) { R[w] = nv; changed = true; }
                carry = (nv & 1) << 63;
            }
        }
        __syncthreads();
        for (int w = lane; w < ww; w += WAVE) {
            u64 prev = reach[w];
            for (int row = 1; row < rows; ++row) {
                const u64 m = open_[row * stride + w], v = reach[row * stride + w];
                u64 nv = v | (prev & m);
                if (nv != v) { nv = spread(nv, m); reach[row * stride + w] = nv; changed = true; }
                prev = nv;
            }
            for (int row = rows - 2; row >= 0; --row) {
                const u64 m = open_[row * stride + w], v = reach[row * stride + w];
                u64 nv = v | (prev & m);
                if (nv != v) { nv = spread(nv, m); reach[row * stride + w] = nv; changed = true; }
                prev = nv;
            }
        }
        __syncthreads();
        if (__ballot(changed) == 0) break;
    }
    // F_k = the window without the flood
    for (int it = 0; it < items; ++it) {
        const int row = it / ww, w = it - row * ww;
        const u64 f = ~reach[row * stride + w] & (w == ww - 1 ? tail : ~0ull);
        if ((f >> lane) & 1) atomicMax(O + (size_t)(win.y0 + row) * W + win.x0 + w * 64 + lane, k);
    }
    __syncthreads();                                            // the planes are free for the next instance
}

__global__ __launch_bounds__(WAVE) void if_lds_kernel(const int32_t *__restrict__ lab, int H, int W, int r, int cap, const int *__restrict__ box,
                                                      const int *__restrict__ list, const int *__restrict__ cnt, int32_t *__restrict__ out,
                                                      int *__restrict__ err) {
    extern __shared__ __align__(16) u64 planes[];
    const int n_list = cnt[0];
    for (int i = blockIdx.x; i < n_list; i += gridDim.x) {
        const int e = list[i], n = e / cap, k = e - n * cap + 1;
        const Window win = window_of(box + (size_t)e * 4, H, W, r);
        if (win.rows > IF_ROWS || win.cols > IF_COLS) continue;                 // (the list kernel's own test: the planes' bounds)
        instance_fill(lab + (size_t)n * H * W, out + (size_t)n * H * W, W, r, k, win, planes, planes + IF_PLANE, ((win.cols + 63) >> 6) | 1, err);
    }
}

// the instances the LDS form does not hold: block n takes image n's, one after the other, on that image's two planes of H * stride words
__global__ __launch_bounds__(WAVE) void if_big_kernel(const int32_t *__restrict__ lab, int H, int W, int r, int cap, int total,
                                                      const int *__restrict__ box, const int *__restrict__ list, const int *__restrict__ cnt,
                                                      u64 *__restrict__ planes, int stride, int32_t *__restrict__ out, int *__restrict__ err) {
    const int n_big = cnt[1], n = blockIdx.x;
    u64 *open_ = planes + (size_t)n * 2 * H * stride, *reach = open_ + (size_t)H * stride;
    for (int i = 0; i < n_big; ++i) {
        const int e = list[total - 1 - i];
        if (e / cap != n) continue;
        const Window win = window_of(box + (size_t)e * 4, H, W, r);
        instance_fill(lab + (size_t)n * H * W, out + (size_t)n * H * W, W, r, e - n * cap + 1, win, open_, reach, stride, err);
    }
}

__global__ __launch_bounds__(256) void if_count_kernel(const int32_t *__restrict__ lab, int plane, int cap, int *__restrict__ seen,
                                                       int *__restrict__ counts, int *__restrict__ err) {
    const int32_t *L = lab + (size_t)blockIdx.y * plane;
    int *S = seen + (size_t)blockIdx.y * cap;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < plane; i += gridDim.x * 256) {
        const int a = L[i];
        if (a == 0) continue;
        if (a < 0 || a > cap) { *err = 1; continue; }
        if (__hip_atomic_load(S + a - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 && atomicExch(S + a - 1, 1) == 0)
            atomicAdd(counts + blockIdx.y, 1);
    }
}

// byte offsets of box, list, cnt and the large windows' planes; returns the total
size_t if_layout(int N, int H, int W, int cap, size_t *o) {
    const size_t total = (size_t)N * cap;
    size_t off = 0;
    o[0] = off; off = align_up(off + total * 16, 256);
    o[1] = off; off = align_up(off + total * 4, 256);
    o[2] = off; off = align_up(off + 16, 256);
    o[3] = off; off = align_up(off + (size_t)N * 2 * H * cdiv(W, 64) * 8, 256);
    return off;
}

bool if_size_ok(int N, int H, int W, int cap) {
    return N > 0 && H > 0 && W > 0 && cap > 0 && (long long)H * W <= 0x7fffffffLL && (long long)N * cap <= (1LL << 28);
}

}  // namespace

extern "C" int cdnet_instance_redilate_lds_rows(void) { return IF_ROWS; }
extern "C" int cdnet_instance_redilate_lds_cols(void) { return IF_COLS; }

extern "C" size_t cdnet_instance_redilate_workspace_bytes(int N, int H, int W, int cap) {
    if (!if_size_ok(N, H, W, cap)) return 0;
    size_t o[4];
    return if_layout(N, H, W, cap, o);
}

extern "C" int cdnet_instance_redilate(const int32_t *label, int N, int H, int W, int r, int cap, void *workspace, size_t workspace_bytes,
                                       int32_t *out, int32_t *err_flag, void *stream) {
    CDNET_REQUIRE(label && workspace && out && err_flag, "cdnet_instance_redilate: null pointer");
    CDNET_REQUIRE(if_size_ok(N, H, W, cap), "cdnet_instance_redilate: bad size N=%d H=%d W=%d cap=%d (N * cap <= 2^28)", N, H, W, cap);
    CDNET_REQUIRE(r >= 1 && r <= IF_MAX_R, "cdnet_instance_redilate: r %d not in [1,%d]", r, IF_MAX_R);
    CDNET_REQUIRE(((uintptr_t)workspace & 7) == 0, "cdnet_instance_redilate: workspace not 8-byte aligned");
    size_t o[4];
    const size_t need = if_layout(N, H, W, cap, o);
    if (workspace_bytes < need) { set_error("cdnet_instance_redilate: workspace %zu < %zu bytes", workspace_bytes, need); return CDNET_E_WORKSPACE; }
    const size_t n = (size_t)N * H * W;
    CDNET_REQUIRE(out + n <= label || label + n <= out, "cdnet_instance_redilate: out overlaps label");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    int *box = (int *)(ws + o[0]), *list = (int *)(ws + o[1]), *cnt = (int *)(ws + o[2]);
    u64 *planes = (u64 *)(ws + o[3]);
    const int total = N * cap;
    if (hipMemsetAsync(box, 0xff, (size_t)total * 16, st) != hipSuccess || hipMemsetAsync(cnt, 0, 16, st) != hipSuccess ||
        hipMemsetAsync(err_flag, 0, 4, st) != hipSuccess || hipMemsetAsync(out, 0, n * 4, st) != hipSuccess)
        return check_launch("cdnet_instance_redilate(memset)");
    if_box_kernel<<<dim3(lin_grid((size_t)H * W, 1024), N), 256, 0, st>>>(label, H, W, cap, box, err_flag);
    if_list_kernel<<<lin_grid(total, 1024), 256, 0, st>>>(box, total, H, W, r, list, cnt);
    const int grid = total < IF_GRID ? total : IF_GRID;
    const int rc = launch_lds<if_lds_kernel>(dim3(grid), dim3(WAVE), IF_LDS, IF_LDS, st, "cdnet_instance_redilate(LDS opt-in)",
                                             "cdnet_instance_redilate(lds)", label, H, W, r, cap, (const int *)box, (const int *)list,
                                             (const int *)cnt, out, err_flag);
    if (rc != CDNET_OK) return rc;
    if_big_kernel<<<N, WAVE, 0, st>>>(label, H, W, r, cap, total, box, list, cnt, planes, cdiv(W, 64), out, err_flag);
    return check_launch("cdnet_instance_redilate");
}

extern "C" int cdnet_label_count(const int32_t *lab, int N, int plane, int cap, int32_t *seen, int32_t *counts, int32_t *err_flag,
                                 void *stream) {
    CDNET_REQUIRE(lab && seen && counts && err_flag, "cdnet_label_count: null pointer");
    CDNET_REQUIRE(N > 0 && plane > 0 && cap > 0 && (long long)N * cap <= (1LL << 28), "cdnet_label_count: bad size");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(seen, 0, (size_t)N * cap * 4, st) != hipSuccess || hipMemsetAsync(counts, 0, (size_t)N * 4, st) != hipSuccess ||
        hipMemsetAsync(err_flag, 0, 4, st) != hipSuccess)
        return check_launch("cdnet_label_count(memset)");
    if_count_kernel<<<dim3(lin_grid((size_t)plane, 1024), N), 256, 0, st>>>(lab, plane, cap, seen, counts, err_flag);
    return check_launch("cdnet_label_count");
}
