// The 1x1 heads' kernel arguments, shared by the forward (model.hip) and the backward (head_bwd.hip): a lazily transformed
// 64-channel feature and the DAM head's weight block.  Both layouts are ABI (cdnet_head_feat, CDNET_HEAD_WEIGHT_FLOATS).
// The feature loaders stay with their kernels: 16-channel quarters in the forward, 8-channel vectors in the backward.
#pragma once
#include "common.h"

namespace {      // (kernel argument types: internal to each translation unit, like the kernels that take them)

// Each feature F_k = relu(raw*scale + shift + res) is recomputed from its stored pieces
// (scale==NULL: the tensor already holds the activated feature).
struct HeadFeat {
    const unsigned short *raw;
    const unsigned short *res;
    const float *scale;
    const float *shift;
    int relu;
    int f16;
};

struct HeadW {            // 64-channel 1x1 heads, fp32
    float wp[64], wd[9][64], wm[3][64];
    float bp, bd[9], bm[3];
    float a1;             // directionAtt.Conv1x1 (1->1, no bias)
    float a2[9];          // maskAtt.Conv1x1 (9->1, no bias)
};
constexpr int HEADW_FLOATS = sizeof(HeadW) / 4;      // 855; the gradient block has the same layout
static_assert(HEADW_FLOATS == CDNET_HEAD_WEIGHT_FLOATS, "head weight block layout");

inline HeadFeat mk_hf(const cdnet_head_feat &f) {
    HeadFeat h;
    h.raw = f.raw; h.res = f.res; h.scale = f.scale; h.shift = f.shift; h.relu = f.relu; h.f16 = f.f16;
    return h;
}

}  // namespace
