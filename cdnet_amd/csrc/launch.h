// Host-side launch helpers: the CU count, the large-LDS opt-in, the persistent-grid rule and the movers' reach check of the
// convolution and weight-gradient launchers (conv.hip, conv32.hip, conv32ws.hip, conv16ws.hip, wgrad.hip); the linear-grid rule of the
// streaming kernels and the run-time -> template argument dispatch for every launcher.  Host code only.
// One device per process is assumed: the CU count and the opt-in flags are kept per process, not per device.
#pragma once
#include <type_traits>
#include "common.h"
#include "conv_args.h"

namespace cdnet {

// Compute units of the device (queried once; 256 when the runtime reports none).  A failed query is CDNET_E_LAUNCH whatever error state
// the runtime keeps.
inline int cu_count(int *n) {
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipGetDeviceProperties(&prop, dev);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("hipGetDeviceProperties: %s", hipGetErrorString(e));
            return CDNET_E_LAUNCH;
        }
        n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    *n = n_cu;
    return CDNET_OK;
}

// Launch of a kernel with more dynamic LDS than the default limit: opts Kern in to `optin_bytes` once per process, then launches with
// `smem` bytes.  The kernel is a template argument, so every kernel has a flag of its own (they all share one signature).
template <auto Kern, typename... Args>
int launch_lds(dim3 grid, dim3 block, int optin_bytes, int smem, hipStream_t st, const char *what_optin, const char *what, const Args &...args) {
    static bool optin_done = false;
    if (!optin_done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, optin_bytes) != hipSuccess)
            return check_launch(what_optin);
        optin_done = true;
    }
    Kern<<<grid, block, smem, st>>>(args...);
    return check_launch(what);
}

// Workgroups per output-channel tile of a persistent launch: the CUs shared among the `ctiles` channel tiles, at most one per spatial
// tile and at most `max_g` (0: no limit), a multiple of 8 from 8 up (as many on each of the 8 XCDs), at most `test_g` (0: no limit - the tests'
// debug >> CONV_DBG_GRID_SHIFT: few workgroups, long runs of tiles), at least 1.
inline int persistent_grid(int n_cu, int ctiles, int tiles, int max_g, int test_g) {
    int G = n_cu / ctiles;
    G = G > tiles ? tiles : G;
    if (max_g > 0 && G > max_g) G = max_g;
    if (G >= 8) G &= ~7;
    if (test_g > 0 && test_g < G) G = test_g;
    if (G < 1) G = 1;
    return G;
}

// The movers of the persistent kernels request a source by 31-bit byte offsets from its base (bit 31 marks a zero-fill vector): true
// when `images` images of `elem_bytes`-byte elements lie within that reach.
inline bool in_mover_reach(const ConvSrc &s, long long images, int elem_bytes) {
    const long long rs = s.row_stride ? s.row_stride : (long long)s.Ws * s.C;
    return images * s.Hs * rs * elem_bytes < (1LL << 31);
}

// Linear grid of 256-thread workgroups over `total` items, at most `cap` workgroups (the kernels stride beyond), at least 1.
inline int lin_grid(size_t total, int cap) {
    const size_t g = (total + 255) / 256;
    return (int)(g > (size_t)cap ? cap : (g < 1 ? 1 : g));
}

// f(std::integral_constant<int, V>{}) for the listed V that equals `value`: only the listed values are instantiated, any other is an error
template <int... Vs, typename F>
int with_int(int value, F &&f) {
    int rc = CDNET_E_ARG;
    const bool hit = (... || (value == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)));
    if (!hit) set_error("with_int: no instantiation for %d", value);
    return rc;
}

// f(std::true_type{}) or f(std::false_type{})
template <typename F>
int with_bool(bool flag, F &&f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace cdnet
