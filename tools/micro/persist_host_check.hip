// Host check of csrc/persist.h's tile_run and tile cursor (no GPU, not loaded into Python):
//   hipcc --cuda-host-only -O1 -g -std=c++20 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         -I cdnet_amd/csrc tools/micro/persist_host_check.hip -o tools/micro/persist_host_check && tools/micro/persist_host_check
// tile_run, for every T in 0..300 and 2^20 + 3 and every G in 1..264: the runs of b = 0 .. G - 1 are disjoint, contiguous and cover
// [0, T); when G % 8 == 0 the workgroups b = k (mod 8) cover exactly [T k / 8, T (k + 1) / 8); the result equals the rule the kernels
// carried in place before the header (copied below).  Cursor, for N <= 3 and H, W in {16, 32, 48, 64}: next_tile from seek_tile(t)
// equals seek_tile(t + 1) for every t.
#include <stdio.h>
#include <stdlib.h>
#include "persist.h"

using namespace cdnet;

// the rule as conv_ws_kernel, conv_ws16_kernel and conv_ws32_kernel wrote it
static void tile_run_ref(int T, int G, int b, int &t_lo, int &t_hi) {
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

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL: " __VA_ARGS__); printf("\n"); return 1; } } while (0)

static int check_runs(int T, int G) {
    int *lo = (int *)malloc(sizeof(int) * G), *hi = (int *)malloc(sizeof(int) * G);
    for (int b = 0; b < G; ++b) {
        tile_run(T, G, b, lo[b], hi[b]);
        int rl, rh;
        tile_run_ref(T, G, b, rl, rh);
        CHECK(lo[b] == rl && hi[b] == rh, "T=%d G=%d b=%d: [%d, %d) against the reference [%d, %d)", T, G, b, lo[b], hi[b], rl, rh);
        CHECK(0 <= lo[b] && lo[b] <= hi[b] && hi[b] <= T, "T=%d G=%d b=%d: [%d, %d) outside [0, T)", T, G, b, lo[b], hi[b]);
    }
    // disjoint, contiguous, covering: in the order the runs lie in (XCD-major when G % 8 == 0, else by b) each starts where the last ended
    int at = 0;
    if ((G & 7) == 0) {
        for (int k = 0; k < 8; ++k) {
            const int e0 = (int)((long long)T * k / 8), e1 = (int)((long long)T * (k + 1) / 8);
            CHECK(at == e0, "T=%d G=%d: XCD %d starts at %d, not at %d", T, G, k, at, e0);
            for (int b = k; b < G; b += 8) {
                CHECK(lo[b] == at, "T=%d G=%d b=%d: run starts at %d, expected %d", T, G, b, lo[b], at);
                at = hi[b];
            }
            CHECK(at == e1, "T=%d G=%d: XCD %d ends at %d, not at %d", T, G, k, at, e1);
        }
    } else {
        for (int b = 0; b < G; ++b) {
            CHECK(lo[b] == at, "T=%d G=%d b=%d: run starts at %d, expected %d", T, G, b, lo[b], at);
            at = hi[b];
        }
    }
    CHECK(at == T, "T=%d G=%d: the runs end at %d", T, G, at);
    free(lo);
    free(hi);
    return 0;
}

int main() {
    long runs = 0, steps = 0;
    for (int G = 1; G <= 264; ++G) {
        for (int T = 0; T <= 300; ++T, ++runs)
            if (check_runs(T, G)) return 1;
        if (check_runs((1 << 20) + 3, G)) return 1;
        ++runs;
    }
    for (int N = 1; N <= 3; ++N)
        for (int H = 16; H <= 64; H += 16)
            for (int W = 16; W <= 64; W += 16) {
                const int tiles_x = W / 16, tiles_img = tiles_x * (H / 16), T = N * tiles_img;
                for (int t = 0; t < T; ++t, ++steps) {
                    int n, y0, x0, n1, y1, x1;
                    seek_tile(t, tiles_img, tiles_x, n, y0, x0);
                    CHECK(n >= 0 && n < N && y0 >= 0 && y0 < H && x0 >= 0 && x0 < W && y0 % 16 == 0 && x0 % 16 == 0,
                          "seek_tile(%d) N=%d H=%d W=%d: (%d, %d, %d)", t, N, H, W, n, y0, x0);
                    next_tile(n, y0, x0, H, W);
                    seek_tile(t + 1, tiles_img, tiles_x, n1, y1, x1);       // (t + 1 == T: image N, row 0, column 0 - where the cursor lands too)
                    CHECK(n == n1 && y0 == y1 && x0 == x1, "next_tile from tile %d N=%d H=%d W=%d: (%d, %d, %d), seek_tile(%d) = (%d, %d, %d)",
                          t, N, H, W, n, y0, x0, t + 1, n1, y1, x1);
                }
            }
    printf("ok: tile_run on %ld (T, G) pairs, cursor on %ld steps\n", runs, steps);
    return 0;
}
