/*
 * cdnet_hip.h - C ABI of libcdnet_hip.so: the MI355X (gfx950) implementation of CDNet's data-parallel hot path.
 *
 * The reference (honglianghe/CDNet) is pure Python: it has no FFI layer of its own.  Its "operator API" for
 * this path is a set of Python call signatures.  Each entry point below names the reference
 * call site(s) it replaces (paths relative to the reference repository root) - that is what a maintainer would
 * bind with ctypes (INTEGRATION.md shows the stubs; cdnet_amd/_lib.py is the binding the package itself uses).
 *
 * Conventions
 *   - every pointer argument is a DEVICE pointer unless its name ends in `_host`;
 *   - the caller owns all buffers (outputs and workspaces); nothing here allocates, frees or synchronises;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *   - return value: 0 = ok, otherwise a CDNET_E_* code; cdnet_last_error() gives a thread-local message;
 *   - images are dense row-major; batches are the leading dimension; activations are NHWC bf16 internally;
 *   - no global mutable state; re-entrant across streams.
 */
#ifndef CDNET_HIP_H
#define CDNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDNET_OK            0
#define CDNET_E_ARG         1   /* bad argument (null pointer, size, unsupported configuration) */
#define CDNET_E_WORKSPACE   2   /* workspace too small */
#define CDNET_E_LAUNCH      3   /* HIP launch error */

#define CDNET_ABI_VERSION   5   /* 2, 3 (round 4): cdnet_conv_args grew (taps1, pool_out; dot_w, dot_b, dot_out) - a caller built against an older
                                 version must not pass its struct.  4 (round 5): cdnet_spin added; cdnet_tta_boost_argmax accepts point_mean == NULL
                                 for one view in its own frame (no struct changed).  5 (round 6): cdnet_box_copy / cdnet_box_mfma (box calibration),
                                 cdnet_tile_postproc (the fused tile post-processing chain); no struct changed */

int         cdnet_abi_version(void);
/* sizeof() of an argument struct of this header by name ("cdnet_conv_args", ...), 0 for an unknown name: a binding that mirrors the structs
 * (ctypes, cgo, JNI) checks its own layout against the library's at load time. */
size_t      cdnet_abi_sizeof(const char *struct_name);
const char *cdnet_last_error(void);
/* static description: "gfx950;wave64;..." */
const char *cdnet_build_info(void);
/* One wavefront that spins for `microseconds` of the constant 100 MHz counter on `stream` and touches no memory (at most 1 s).  The host
 * side's stream probe times two of them on two streams (cdnet_amd/streams.py): streams that share a hardware queue run them one after the
 * other.  Replaces nothing of the reference (nn.DataParallel has no streams of its own, train.py:185); a diagnostic of the runtime. */
int         cdnet_spin(int microseconds, void *stream);
/* Box calibration (bench.py's `box` object: boxes of one pool differ by 10-25 % on memory-bound kernels and in the clock they hold under
 * matrix load; rates are reported beside what the box itself grants).  Diagnostics of the runtime; nothing of the reference.
 * cdnet_box_copy: dst[i] = src[i] over `bytes` (multiple of 16, both 16-byte aligned) with float4 accesses, 4096 workgroups grid-stride.
 * cdnet_box_mfma: `workgroups` x `waves_per_wg` waves each run `iters` iterations of four v_mfma_f32_32x32x16_bf16 whose operands are
 * re-read from LDS (64 KB of patterns copied from `seed`, u32 [16384] = bf16 pairs); 4 x 32768 flop per wave and iteration.  `stamps`
 * (NULL or u64 [2 * workgroups]): per workgroup the loop's duration in shader cycles (s_memtime) and in ticks of the constant 100 MHz counter
 * (s_memrealtime) - clock = cycles / ticks x 100 MHz. */
int         cdnet_box_copy(const void *src, void *dst, size_t bytes, void *stream);
int         cdnet_box_mfma(const uint32_t *seed, float *sink, unsigned long long *stamps, int workgroups, int waves_per_wg, int iters, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * The whole post-processing chain of a batch of independent tiles (one view each, in its own frame) in two launches (round 6).
 * Replaces, per tile, test_dam.py:982-1015 (get_probmaps epilogue), getDirectionDiffMap.py:44-108 (generate_dd_map), test_dam.py:529-539
 * (point-guided boost + arg-max) and test_dam.py:546-563 (fill holes, remove small objects, label, dilate) - the same steps as
 * cdnet_probmaps + cdnet_ddm_codes + cdnet_tta_boost_argmax (V = 1) + cdnet_cc_chain, with bit-identical results: launch 1 leaves the
 * direction-difference codes (its direction-class window lives in LDS, the halo recomputed from the logits), launch 2 runs everything else of
 * a tile inside ONE workgroup with the tile in LDS (16-bit union-find).
 *   mask_logits f32 [B,3,H,W], dir_logits f32 [B,C,H,W] (C = 5 / 9 / 17), point f32 [B,H,W]      (device, NCHW as Unet.forward returns them)
 *   lut_host: int8 [C*C] HOST memory as for cdnet_ddm_codes; nbr / extra_zero as there
 *   prob f32 [B,3,H,W] or NULL, dcm u8 [B,H,W] or NULL (stage outputs); minmax i32 [B,2] (min, max DDM code per tile: equal = the reference's
 *   assertion test_dam.py:535 would fail); pred u8 [B,H,W]; fill / small u8 [B,H,W] or NULL; label i32 [B,H,W] or NULL; final i32 [B,H,W];
 *   counts i32 [B] or NULL
 * Shapes: W a multiple of 64 and H * W <= 65536 (cdnet_tile_postproc_workspace_bytes returns 0 otherwise: use the per-step entries). */
size_t cdnet_tile_postproc_workspace_bytes(int B, int C, int H, int W);
int cdnet_tile_postproc(const float *mask_logits, const float *dir_logits, const float *point, int B, int C, int H, int W,
                        const int8_t *lut_host, int nbr, int extra_zero, int min_area, int radius, void *workspace, size_t workspace_bytes,
                        float *prob, uint8_t *dcm, int32_t *minmax, uint8_t *pred, uint8_t *fill, uint8_t *small, int32_t *label,
                        int32_t *final_, int32_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Direction-difference map.   Replaces data_prepare/getDirectionDiffMap.py:44-108 `generate_dd_map`
 * (+ `circshift` :14-42 and DTOffsetHelper.label_to_vector SegFix_offset_helper.py:246-261), which
 * test_dam.py:479-487 calls 8x per image.
 *
 * cdnet_ddm_codes: dcm u8 [N][H][W] (direction classes 0..classes-1) -> code u8 [N][H][W] in {0,1,2} and
 *   minmax i32 [N][2] = (min code, max code) per image.  `lut_host` int8 [classes*classes] holds
 *   round(cos(v_a, v_b)) for every class pair (host memory, copied into the launch); nbr = 8 (9/17 classes)
 *   or 4 (5 classes); extra_zero = 1 reproduces the reference's never-written cosine channels (17 classes).
 * cdnet_ddm_normalize: out f32 [N][H][W] = (code - min) / (max - min)  (NaN when a map is constant, as in
 *   the reference).
 * ---------------------------------------------------------------------------------------------------- */
int cdnet_ddm_codes(const uint8_t *dcm, int N, int H, int W, int classes, const int8_t *lut_host, int nbr,
                    int extra_zero, uint8_t *code, int32_t *minmax, void *stream);
int cdnet_ddm_normalize(const uint8_t *code, const int32_t *minmax, int N, int H, int W, float *out,
                        void *stream);

/* ------------------------------------------------------------------------------------------------------
 * get_probmaps epilogue.   Replaces test_dam.py:982-1015: softmax over the 3 mask logits, softmax over the
 * direction logits with channel 0 multiplied by P(background), argmax -> direction class map.
 * mask_logits f32 [N][3][H][W], dir_logits f32 [N][C][H][W] -> prob f32 [N][3][H][W], dcm u8 [N][H][W].
 * ---------------------------------------------------------------------------------------------------- */
int cdnet_probmaps(const float *mask_logits, const float *dir_logits, int N, int C, int H, int W,
                   float *prob, uint8_t *dcm, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * TTA mean + DDM fuse + point-guided boundary boost + argmax.   Replaces test_dam.py:445-450 (mean of the
 * un-flipped views), :479-491 (per-view DDM, mean), :529-539 (boost, argmax).
 *
 * Views are stored in their OWN frame; `view_xform[v]` (host, V ints, 0..7) tells how view v was made from the
 * image: bit0 = horizontal flip, bit1 = vertical flip, bit2 = rotated 90deg counter-clockwise first
 * (PIL rotate(90, expand=True), test_dam.py:372); the kernels read through the inverse map, which is what
 * np.flip / np.rot90(k=3) do in test_dam.py:356-441.  For rotated views the stored frame is [W][H].
 *   probs  f32 [I][V][3][h_v][w_v]   points f32 [I][V][h_v][w_v]
 *   codes  u8  [I][V][h_v][w_v]      minmax i32 [I][V][2]          (from cdnet_ddm_codes, N = I*V)
 * Outputs (image frame [H][W]): prob_mean f32 [I][3][H][W] (before the boost), point_mean f32 [I][H][W],
 *   ddm16 u8 [I][H][W] = 16 * mean_v DDM_v when every view has min=0,max in {1,2} (else the f64 path is used and
 *   ddm16 is 255), pred u8 [I][H][W] = argmax class.  Any of prob_mean / ddm16 may be NULL.  point_mean may be NULL only for ONE view in
 *   its own frame (V == 1, view_xform[0] == 0, prob_mean NULL, H*W a multiple of 4, points 16-byte aligned): the mean over views is the view
 *   itself, nothing is averaged or stored (the 256x256 tile pipeline).
 *   pmax_ws: f32 workspace [I] (global max of point_mean).
 * ---------------------------------------------------------------------------------------------------- */
int cdnet_tta_boost_argmax(const float *probs, const float *points, const uint8_t *codes, const int32_t *minmax,
                           int I, int V, const int *view_xform_host, int H, int W,
                           float *prob_mean, float *point_mean, uint8_t *ddm16, uint8_t *pred,
                           float *pmax_ws, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Watershed variant of the instance post-processing.   Replaces postproc_other.py:15-99 `process(pred, model_mode,
 * min_size, ws=True)` for the non-'dcan' modes, steps :36-48:
 *   scipy.ndimage.measurements.label (4-connected) -> gen_inst_dst_map (:16-27: per-instance distance_transform_edt
 *   scaled to 0..255 uint8) -> marker = label(binary_erosion(binary_fill_holes(dist > 125))) with labels smaller than
 *   min_size removed -> skimage.segmentation.watershed(-dist [uint8 wrap], marker, mask=pred) -> remove small labels.
 * pred u8 [N][H][W] already thresholded (0 / non-zero = `pred > 0.5`, :33-34).
 * Outputs: labels i32 [N][H][W] (required, marker ids are kept like the reference does); dist u8 and marker i32 stage
 * outputs (each may be NULL).  workspace: cdnet_watershed_workspace_bytes(N, H, W) bytes.
 * ---------------------------------------------------------------------------------------------------- */
size_t cdnet_watershed_workspace_bytes(int N, int H, int W);
int cdnet_watershed_process(const uint8_t *pred, int N, int H, int W, int min_size, void *workspace, size_t workspace_bytes,
                            uint8_t *dist, int32_t *marker, int32_t *labels, void *stream);
/* The ws = False branch of the same function (postproc_other.py:49-52; forced for model_mode 'unet' / 'micronet', :35):
 *   scipy.ndimage.binary_fill_holes -> measurements.label (4-connected, ids in raster order) -> remove_small_objects on the label
 *   image (labels with fewer than min_size pixels become 0; the other ids are kept).  pred u8 [N][H][W] non-zero = foreground;
 *   labels i32 [N][H][W]; workspace: cdnet_watershed_workspace_bytes(N, H, W) bytes. */
int cdnet_fill_label_process(const uint8_t *pred, int N, int H, int W, int min_size, void *workspace, size_t workspace_bytes,
                             int32_t *labels, void *stream);
/* The 'dcan' branch before its re-dilation (postproc_other.py:79-80): measurements.label (4-connected, ids in raster order) ->
 *   remove_small_objects, no hole filling.  Arguments and workspace as for cdnet_fill_label_process. */
int cdnet_label_process(const uint8_t *pred, int N, int H, int W, int min_size, void *workspace, size_t workspace_bytes,
                        int32_t *labels, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Per-instance re-dilation.   Replaces the closing loops of postproc_other.process: 'micronet' postproc_other.py:56-68 (cv2.dilate with
 * the 3 x 3 cross, r = 1) and 'dcan' :81-97 (k_disk, r = 3); both kernels are the diamond |dx| + |dy| <= r.  For every id k, ascending:
 *   inst = cv2.dilate(label == k, diamond(r)) (outside the image is background) -> binary_fill_holes(inst) -> canvas[inst] = k,
 * that is out(p) = the largest k whose dilated and filled instance covers p, 0 where none does.  Exact; the result does not depend on
 * the order the instances are worked in.
 *
 * cdnet_instance_redilate: label / out i32 [N][H][W] (out must not overlap label), r in 1..3, ids in 1..cap (0 = background), N * cap <= 2^28.
 *   workspace: cdnet_instance_redilate_workspace_bytes(N, H, W, cap) bytes (0 for sizes the entry refuses), 8-byte aligned.
 *   err_flag (1 int): 1 = an id outside 0..cap, 2 = the flood of an instance did not end within its pass bound (rows x columns of its
 *   window + 1, which it cannot exceed); out is unspecified then.  Instances whose window (bounding box grown by r, clipped) is at most
 *   cdnet_instance_redilate_lds_rows() x cdnet_instance_redilate_lds_cols() run in LDS, one wave each; larger ones on bit planes in the
 *   workspace, one after the other per image.
 * cdnet_label_count: counts[N] = the number of distinct ids in 1..cap of lab i32 [N][plane] (the instance count of a label map whose ids
 *   have gaps, kept on the device); seen i32 [N][cap] scratch; err_flag 1 = an id outside 0..cap.
 * ---------------------------------------------------------------------------------------------------- */
size_t cdnet_instance_redilate_workspace_bytes(int N, int H, int W, int cap);
int cdnet_instance_redilate(const int32_t *label, int N, int H, int W, int r, int cap, void *workspace, size_t workspace_bytes,
                            int32_t *out, int32_t *err_flag, void *stream);
int cdnet_instance_redilate_lds_rows(void);
int cdnet_instance_redilate_lds_cols(void);
int cdnet_label_count(const int32_t *lab, int N, int plane, int cap, int32_t *seen, int32_t *counts, int32_t *err_flag, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Connected-component chain.   Replaces test_dam.py:546-563:
 *   scipy.ndimage.binary_fill_holes -> skimage.morphology.remove_small_objects(min_area)
 *   -> skimage.measure.label (8-connectivity, ids in raster order) -> skimage.morphology.dilation(disk(radius)).
 * pred u8 [N][H][W]; a pixel is foreground when pred == fg_value (test_dam.py:538 `pred == 1`).
 * Outputs: final i32 [N][H][W] (required); fill u8, small u8, label i32 (stage outputs, each may be NULL);
 *   counts i32 [N] (number of instances, may be NULL).
 * workspace: cdnet_cc_workspace_bytes(N, H, W) bytes.
 * ---------------------------------------------------------------------------------------------------- */
size_t cdnet_cc_workspace_bytes(int N, int H, int W);
int cdnet_cc_chain(const uint8_t *pred, int fg_value, int N, int H, int W, int min_area, int radius,
                   void *workspace, size_t workspace_bytes,
                   uint8_t *fill, uint8_t *small, int32_t *label, int32_t *final_, int32_t *counts,
                   void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Mask-only inference (networks with one mask output: UNet, and output[0] of the model_unet_MandD* ablation heads).  Replaces test.py:216-275
 * (8-view TTA: per-view softmax of get_probmaps :634, np.flip / np.rot90(k=3) back to the image frame, the float32 mean
 * `(p + p_hf + ... + p_r90_hvf) / 8` :267-268, `np.argmax(prob, 0)` :274 or `prob[0] >= 0.5` :270-272) and, for tiles, :277-295 too.
 *
 * cdnet_mask_views_argmax: ONE launch for I images of V views each.
 *   logits f32 [I][V][K][h_v][w_v], K in {1,2,3}: view v in its own frame ([W][H] when rotated; view_xform_host as for
 *   cdnet_tta_boost_argmax) - the buffer utils.split_forward_views(..., out=) stitches.  prob_mean f32 [I][K][H][W] or NULL (the mean
 *   probabilities, test.py:376 saves plane 1); pred u8 [I][H][W]: K = 2 / 3 the arg-max with numpy's rules (first maximum, the first NaN wins),
 *   K = 1 `mean >= 0.5` - a one-channel softmax is 1 wherever the logit is finite, so such a model marks every finite pixel foreground, as the
 *   reference does.  Foreground is pred == 1 in every case.  Scalar stores: no alignment is assumed.
 * cdnet_tile_mask_postproc: B independent tiles, one view each, in TWO launches: softmax / class / foreground bit plane, then the
 *   connected-component chain of cdnet_tile_postproc's second launch (fill holes, remove small objects, 8-connected label, disk dilation:
 *   test.py:277-295 with postproc 0).  logits f32 [B][K][H][W] (NCHW, as UNet.forward returns them); prob f32 [B][K][H][W] or NULL; pred u8;
 *   fill / small u8 and label i32 or NULL (stage outputs); final i32 [B][H][W]; counts i32 [B].  Bit-identical to cdnet_mask_views_argmax
 *   (V = 1, view 0) followed by cdnet_cc_chain(pred, fg_value = 1).  Shapes: W a multiple of 64 and H * W <= 65536 -
 *   cdnet_tile_mask_postproc_workspace_bytes returns 0 for every other shape (and K); the bit plane's 8-byte words need an 8-byte aligned
 *   workspace, the other stores are scalar.
 * cdnet_dilate_labels: out = skimage.morphology.dilation(label, disk(radius)) (test.py:295 after postproc_other.process, :288-290), radius
 *   0..8, label / out i32 [N][H][W]; out must not overlap label.  Scalar stores: no alignment is assumed.
 * ---------------------------------------------------------------------------------------------------- */
int cdnet_mask_views_argmax(const float *logits, int I, int V, int K, const int *view_xform_host, int H, int W, float *prob_mean,
                            uint8_t *pred, void *stream);
size_t cdnet_tile_mask_postproc_workspace_bytes(int B, int K, int H, int W);
int cdnet_tile_mask_postproc(const float *logits, int B, int K, int H, int W, int min_area, int radius, void *workspace, size_t workspace_bytes,
                             float *prob, uint8_t *pred, uint8_t *fill, uint8_t *small, int32_t *label, int32_t *final_, int32_t *counts,
                             void *stream);
int cdnet_dilate_labels(const int32_t *label, int N, int H, int W, int radius, int32_t *out, void *stream);


/* ------------------------------------------------------------------------------------------------------
 * Convolution stack (MFMA implicit GEMM, NHWC bf16, fp32 accumulate).   Replaces the cuDNN/MIOpen calls behind
 * nn.Conv2d / nn.ConvTranspose2d / nn.BatchNorm2d / nn.ReLU / nn.MaxPool2d / F.pad / torch.cat in
 * models/dam/model_unet_rev1.py:86-170,244-287 and models/unet.py:8-50,90-106 (see DESIGN.md for the fusion map).
 *
 * A convolution reads up to two sources (virtual channel concat, torch.cat order).  Each source may carry the
 * PRODUCER's per-channel affine (BatchNorm as scale/shift), a residual tensor added before the ReLU, a ReLU, a 2x2
 * max-pool and an F.pad offset - all applied while the input tile is staged, never as separate passes.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct cdnet_conv_src {
    const uint16_t *x;      /* 16-bit NHWC [N][Hs][Ws][C] (bf16, or fp16 when f16 = 1) */
    const uint16_t *res;    /* optional bf16 tensor of the same shape added before the ReLU (ResidualUnit) */
    const float *scale;     /* optional per-channel affine of the producer (BN): v*scale[c]+shift[c] */
    const float *shift;
    int C;                  /* channels of this source (multiple of CK) */
    int Hs, Ws;             /* stored spatial size */
    int pool;               /* 1: logical input = maxpool2x2(transformed source), size Hs/2 x Ws/2 */
    int relu;
    int off_y, off_x;       /* F.pad: logical (y,x) reads source (y-off_y, x-off_x); outside -> 0 */
    int f16;                /* storage of x / res: 0 = bf16, 1 = fp16 (raw pre-BatchNorm outputs, residual branches),
                               2 = fp32 (the pointers then address float tensors; fp32-precision path, cdnet_conv_args.f32) */
    int row_stride;         /* elements between rows (0 = dense: Ws*C); images are Hs*row_stride apart.  Lets the
                               space-to-depth view of a 2x-upsampled gradient be read without a copy. */
} cdnet_conv_src;

typedef struct cdnet_conv_args {
    cdnet_conv_src src[2];
    int nsrc;
    const uint16_t *w;      /* packed bf16 weights (cdnet_pack_conv_weights) */
    const float *bias;      /* [Cout] or NULL: added in the epilogue (before oscale/oshift) */
    const float *oscale;    /* epilogue affine (eval-mode BN fold) or NULL */
    const float *oshift;
    int orelu;
    uint16_t *out;          /* bf16 NHWC [N][H*ostride][W*ostride][out_cstride], channels [out_coff, out_coff+Cout) */
    int Cout, out_cstride, out_coff;
    float *stats;           /* NULL or f32 [N*npar*tiles][2][Cout]: per-tile channel sum / sum of squares of the
                               fp32 accumulators (training-mode BatchNorm statistics, bias excluded) */
    int N, H, W;            /* logical input size (= output size / ostride) */
    int taps;               /* 9: 3x3 pad 1; 1: 1x1; 4: sub-pixel 2x2 of ConvTranspose2d(k4,s2,p1) */
    int npar;               /* 1, or 4 sub-pixel parities (ConvTranspose2d stride 2) */
    int ostride;            /* 1, or 2 for the transposed convolutions */
    int nchunk;             /* total Cin chunks over both sources (two-source 3x3 launches of the 16-bit path: one more is allowed - a padding chunk
                               behind the second source whose packed weights are zeros, making the count even for conv_ws16_kernel's out-image form.  Valid on conv_ws16_kernel ONLY
                               (bounded buffer descriptors): ask cdnet_conv_ws_eligible == 2 first, any other kernel returns CDNET_E_ARG) */
    int tile, CK, BN;       /* kernel configuration: spatial tile (16 or 8), Cin chunk, Cout tile */
    int out_f16;            /* 1: store the output as fp16 instead of bf16 */
    int debug;              /* 0 in production.  Kernel-selection switches for the tests (named, with the kernels that read them, in
                               cdnet_amd/csrc/conv_args.h): 32 = never take the wave-specialised persistent kernels (conv_ws16_kernel,
                               conv_ws_kernel; conv_ws32_kernel of the fp32 path), 64 = take them even for small launches; 128 (16-bit
                               path): conv_ws_kernel, the older persistent kernel, instead of conv_ws16_kernel; bits 8..: at most
                               (debug >> 8) persistent workgroups per output-channel tile (long runs of tiles on small test shapes;
                               conv_ws32_kernel, conv_ws16_kernel - so an odd cap also sets 256, which only a one-tap fp32 launch reads);
                               16 (16-bit path): conv_ws16_kernel's quad-request form whatever the launch's size (production: tensors
                               beyond the Infinity Cache); 256 (fp32 mode, taps = 1): conv_f32_kernel also where
                               conv1x1_f32_stream_kernel applies; other bits: ablations of tools/bench_conv.py */
    int ws;                 /* 0, or 2 (fp32 mode, conv_ws32_kernel only - ask cdnet_conv_ws_eligible): the launch also leaves the first
                               BatchNorm-backward pass of the layer its output feeds; eres / oscale / oshift / eres_scale / eres_shift /
                               stats then carry that layer's raw output, scale, shift, mean, invstd and the partial rows f32
                               [1024][2][Cout] (at most 4 x 256 workgroups write rows; see cdnet_bn_backward_finalize) */
    int f32;                /* 1: fp32 precision - x / res / eres / out are fp32 tensors (every source has f16 = 2), `w` is the split
                               pack (mode | CDNET_PACK_SPLIT), each product runs as three bf16 MFMAs over (hi, lo) operand pairs with
                               fp32 accumulation; CK = 16, no pooled sources (materialise them).  0: the 16-bit path. */
    /* Optional fused residual epilogue (ResidualUnit, model_unet_rev1.py:161-170: relu2(bn2(conv2(.)) + conv_1x1(x))): the
     * convolution result (bias added, rounded to fp16) is the residual r; eres = the other branch, a dense fp16 (eres_f16 = 1)
     * or bf16 tensor [N][H][W][Cout] with an optional per-channel affine (training: raw conv2 output x BatchNorm scale /
     * shift).  out = bf16( [relu]( (eres * eres_scale + eres_shift) + r ) ), bit-identical to cdnet_src_materialize over the
     * same pair.  The convolution's own epilogue affine (oscale / oshift: eval-mode BatchNorm fold) applies before the add, so
     * the identity-shortcut blocks of HRNet in eval mode (seg_hrnet_rev1.py:76-92, 113-133: relu(bn(conv(.)) + x), eres = x in
     * bf16) use it too.  NULL = off.  Needs ostride 1, out_coff 0, out_cstride = Cout, no stats, orelu = 0. */
    const uint16_t *eres;
    const float *eres_scale, *eres_shift;
    int eres_f16, eres_relu;
    /* taps of the chunks of the SECOND source: 0 = `taps` (the usual concatenation).  1 with taps = 9 (16-bit path, conv_ws16_kernel
     * only - ask cdnet_conv_ws_eligible): the second source contributes through a 1x1 convolution, its chunks carry the centre tap
     * alone.  `w` then holds, per output-channel tile, the nine-tap chunks of source 0 followed by the one-tap chunks of source 1
     * (two cdnet_pack_conv_weights packs laid end to end).  One launch computes relu(bn2(conv2(h)) + conv_1x1(x)) of a residual unit
     * in eval mode (model_unet_rev1.py:161-170) with the BatchNorm scale folded into conv2's weights and shift + bias in `oshift`. */
    int taps1;
    int pad_;
    /* Optional second output: nn.MaxPool2d(2, 2) of the (ReLU-activated, bf16) output, dense [N][H/2][W/2][Cout] - the 'M' layers of the
     * torchvision VGG16-BN encoder (model_unet_rev1.py:40-41) fused into the producing convolution's store path.  16-bit path:
     * conv_ws16_kernel's out-image form (cdnet_conv_ws_eligible answers 2 with the pointer set); fp32 mode (float tensors): conv_ws32_kernel
     * with plain sources, >= 4 chunks, BN = 64 (answer 1).  Otherwise leave it NULL and call cdnet_src_materialize.  Needs orelu = 1,
     * out_coff = 0, out_cstride = Cout. */
    uint16_t *pool_out;
    /* Optional 1x1 classifier over the (activated, bf16-rounded) output, fused into the store path: dot_out[n][y][x] = dot_b[0] +
     * sum_c dot_w[c] * out[n][y][x][c] as fp32 [N][H][W] - the DAM head's point logit (model_unet_rev1.py:252-253: point_conv over the
     * point feature, whose only other reader is nobody: with dot_out set `out` may be NULL and the 64-channel feature is then never
     * stored).  16-bit path, conv_ws16_kernel's out-image form only (cdnet_conv_ws_eligible answers 2 with the pointers set); needs
     * Cout <= BN (one output-channel tile), out_coff = 0; no pool_out beside it.  NULL = off. */
    const float *dot_w;     /* [Cout] */
    const float *dot_b;     /* [1], device memory */
    float *dot_out;
} cdnet_conv_args;

/* packed element count for a weight tensor; nchunk = Cin/CK over all sources */
size_t cdnet_conv_packed_weight_elems(int Cout, int nchunk, int taps, int CK, int BN, int npar);
/* fp32 master weights -> packed bf16.  mode 0: Conv2d [Cout][Cin][KH][KW] forward; mode 1: Conv2d backward-data
 * (Cout/Cin are the ROLES in the backward GEMM: Cout := original in_channels, Cin := original out_channels);
 * mode 2: ConvTranspose2d [Cin][Cout][4][4] k4 s2 p1 forward (4 parities); mode 3: ConvTranspose2d [Cin][Cout][2][2]
 * k2 s2 forward (4 parities); mode 7: backward-data of mode 6 (Cout := 4*C of the view, Cin := the conv's out_channels);
 * mode 4 / 5: backward-data of the k4 s2 p1 / k2 s2 transposed convolution, expressed as a
 * 3x3 / 1x1 convolution over the space-to-depth view of the output gradient (two sources = the two row parities, each
 * with 2*Cout_t channels ordered (column parity, channel)); Cout := transposed-conv in_channels, Cin := 4*out_channels.
 * mode 6: forward Conv2d [Cout][C][3][3] stride 2 pad 1 (HRNet transition / fuse layers, seg_hrnet_rev1.py:228-247,
 * 436-443) as a 3x3 convolution over the same space-to-depth view of its INPUT; Cin := 4*C. */
#define CDNET_PACK_SPLIT 16   /* OR into `mode`: fp32-precision pack = per Cin chunk the bf16(w) image followed by the
                                bf16(w - bf16(w)) image; twice cdnet_conv_packed_weight_elems elements */
int cdnet_pack_conv_weights(const float *w, void *packed, int Cout, int Cin, int KH, int KW, int CK, int BN, int mode,
                            void *stream);
/* mode 0 (optionally | CDNET_PACK_SPLIT) with every output channel's weights multiplied by cout_scale[cout] in fp32 before the rounding:
 * the eval-mode BatchNorm scale folded into the convolution (nn.BatchNorm2d in eval mode after nn.Conv2d, model_unet_rev1.py:40-41,
 * 112-114, 146-170), so that the epilogue is shift + ReLU only - what conv_ws16_kernel takes as the accumulators' initial value. */
int cdnet_pack_conv_weights_scaled(const float *w, const float *cout_scale, void *packed, int Cout, int Cin, int KH, int KW, int CK,
                                   int BN, int mode, void *stream);
/* The same packing for many tensors in one launch (the training step re-packs every layer's forward and backward-data
 * weights after each optimizer update - train_util_dam.py:308 optimizer.step()).  `table` is device scratch of
 * cdnet_pack_batch_table_bytes(n_jobs) bytes; upload = 1 copies the job table there (first call, or whenever the jobs
 * changed), upload = 0 re-runs the table uploaded before. */
typedef struct cdnet_pack_job {
    const float *w;
    void *packed;
    int Cout, Cin, KH, KW, CK, BN, mode, pad_;
} cdnet_pack_job;
size_t cdnet_pack_batch_table_bytes(int n_jobs);
int cdnet_pack_conv_weights_batch(const cdnet_pack_job *jobs, int n_jobs, void *table, size_t table_bytes, int upload,
                                  void *stream);
int cdnet_conv_forward(const cdnet_conv_args *args, void *stream);

/* The kernel instantiation the calling thread's last cdnet_conv_forward launched (host-side record, thread-local like
 * cdnet_last_error; 0 before the first launch; a refused call leaves it as it was).  For tests, which assert the dispatch form of
 * every case.  Bit layout (a field a family has no template argument for is 0):
 *   bits 0-3 family (CDNET_CONV_FAMILY_*), 4-5 BN (0 = 32, 1 = 64, 2 = 128), 6-9 TAPS, 10-11 XF (source transform form: 0 plain,
 *   1 fast, 2 generic; conv1x1_f32_stream_kernel: 1 = with scale / shift), bit 12 STATS, bit 13 STREAM (weights streamed through the
 *   LDS), bit 14 MIX (one-tap second source), bits 15-16 NCS (small-chunk-count form), bits 17-19 launch site (conv_ws16_kernel:
 *   0 direct stores, 1 out image with pair requests, 2 out image with quad requests, 3 streamed 16x16x32; conv_ws32_kernel: 0 plain,
 *   1 BatchNorm-backward sums, 2 mix, 3 pool), bit 20 tile (0 = 16 x 16, 1 = 8 x 8), bits 21-22 CK (0 = 16, 1 = 32, 2 = 64),
 *   bits 23-25 NCH (chunks of conv1x1_f32_stream_kernel), bit 26 ERES (its fused residual epilogue). */
#define CDNET_CONV_FAMILY_FWD    1   /* conv_fwd_kernel */
#define CDNET_CONV_FAMILY_WS     2   /* conv_ws_kernel */
#define CDNET_CONV_FAMILY_WS16   3   /* conv_ws16_kernel */
#define CDNET_CONV_FAMILY_F32    4   /* conv_f32_kernel */
#define CDNET_CONV_FAMILY_STREAM 5   /* conv1x1_f32_stream_kernel */
#define CDNET_CONV_FAMILY_WS32   6   /* conv_ws32_kernel */
int cdnet_conv_forward_last_form(void);

/* ------------------------------------------------------------------------------------------------------
 * Dilated dense-block convolution (dilated.hip): FullNet's ConvLayer (models/FullNet.py:14-36: Conv2d(dilation, bias=False) ->
 * LeakyReLU -> BatchNorm2d, then torch.cat([x, out], 1)) and its stem / transition / final convolutions (:90-138), eval mode.  NHWC:
 *
 *   out[n][y][x][out_coff + co] = post( sum_{ky,kx,ci<Cin} w[co][ci][ky][kx] * in[n][y + (ky-1) d][x + (kx-1) d][ci] )    zero outside the image
 *   post(v) = (leaky ? (v >= 0 ? v : slope v) : v) * scale[co] + shift[co]        (the LeakyReLU BEFORE the affine; scale NULL = 1, shift NULL = 0)
 *
 * taps = 9 (3x3, padding = dilation) or 1 (1x1, dilation ignored but >= 1); dilation >= 1 without an upper bound (it may exceed H and W:
 * a tap that no pixel of a wave's strip can reach costs no load and no MFMA).  Cin >= 1 is any count, in_cstride >= Cin the channel
 * stride of `in`, a multiple of 8 elements; the kernel loads up to round_up(Cin, 8) channels of a pixel and masks (selects, never
 * multiplies) those >= Cin, so NaN there is harmless.  Cout >= 1 is any count: exactly channels [out_coff, out_coff + Cout) of `out`
 * (channel stride out_cstride >= out_coff + Cout, no alignment asked of out_coff) are written, nothing else.
 * `in` and `out` may be the same tensor (then in_cstride == out_cstride) when [0, Cin) and [out_coff, out_coff + Cout) are disjoint: a
 * dense layer appends its growth_rate channels in place, the concatenation is never a copy.  Overlapping ranges are an argument error.
 * f32 = 0: in / out bf16, `w` the one-image pack, one bf16 MFMA per product, fp32 accumulation.
 * f32 = 1: in / out fp32, `w` the split pack, every product as a_lo b_hi + a_hi b_lo + a_hi b_hi like conv32.hip.
 * out_nchw = 1: `out` is fp32 [N][Cout][H][W] whatever f32 says (the logits cdnet_window_stitch and the soft-max read); out_coff = 0,
 * out_cstride is ignored and `out` must not be `in`.
 * Argument errors (CDNET_E_ARG: a null in / w / out, taps not 1 or 9, dilation < 1, a count < 1, a stride below its channel count or an
 * in_cstride that is no multiple of 8, overlapping in-place ranges) are found before any HIP call. */
typedef struct cdnet_dilated_conv_args {
    const void *in;          /* [N][H][W][in_cstride] bf16 / fp32 */
    const void *w;           /* cdnet_dilated_pack_weights */
    const float *scale;      /* [Cout] or NULL */
    const float *shift;      /* [Cout] or NULL */
    void *out;
    int N, H, W;
    int Cin, in_cstride;
    int Cout, out_cstride, out_coff;
    int taps, dilation;
    int leaky;
    float slope;
    int f32, out_nchw;
} cdnet_dilated_conv_args;
/* bf16 elements of the pack of one layer (f32 = 1: the hi and the lo image, twice as many) */
size_t cdnet_dilated_packed_weight_elems(int Cin, int Cout, int taps, int f32);
/* fp32 Conv2d weights [Cout][Cin][3][3] / [Cout][Cin][1][1] (device) -> the MFMA-fragment pack, once per layer: per (tap, 16-channel
 * K step, 32-wide output tile) the 64 lanes' 8 bf16 values in load order (f32 = 1: followed by the bf16(w - bf16(w)) image). */
int cdnet_dilated_pack_weights(const float *w, void *packed, int Cin, int Cout, int taps, int f32, void *stream);
int cdnet_dilated_conv_forward(const cdnet_dilated_conv_args *args, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * FullNet training (dilated.hip, dilated_train.hip): the backward of a ConvLayer (models/FullNet.py:14-21 in train(): Conv2d(dilation) ->
 * LeakyReLU(inplace) -> BatchNorm2d on batch statistics) and of the dense layers' dropout + torch.cat (:25-52), which autograd derives in
 * the reference (train_util.py:193-195 loss.backward()).  With g the gradient of the raw convolution output c:
 *
 *   dx[n][y][x][dx_coff + ci] (+)= sum_{ky,kx,co<Cout} w[co][ci][ky][kx] * g[n][y - (ky-1) d][x - (kx-1) d][co]          zero outside the image
 *   dW[co][ci][ky][kx]          = sum_{n,y,x}          g[n][y][x][co]    * x[n][y + (ky-1) d][x + (kx-1) d][ci]          zero outside the image
 *
 * Every entry finds its argument errors (CDNET_E_ARG: a null pointer, taps not 1 or 9, dilation < 1, a count < 1, a stride below its
 * channel count or no multiple of 8 where a 32-byte loader reads it, an accumulate target that overlaps the source, a short workspace)
 * before any HIP call. */

/* backward-data: the forward kernel with the roles swapped (GEMM-K = Cout x taps, GEMM-N = Cin) over the pack w'[ci][co][8 - tap] of
 * cdnet_dilated_pack_weights_bwd (cdnet_dilated_packed_weight_elems(Cout, Cin, taps, f32) elements).  accumulate = 0 stores channels
 * [dx_coff, dx_coff + Cin) of dx, accumulate = 1 adds to them (one read-modify-write per element by one lane: deterministic); no other
 * channel of dx is touched.  g and dx may be the same tensor only when [0, Cout) and [dx_coff, dx_coff + Cin) are disjoint and the strides
 * are equal.  g_cstride is a multiple of 8; any Cin, Cout, dilation >= 1; f32 as in cdnet_dilated_conv_args. */
typedef struct cdnet_dilated_bwd_data_args {
    const void *g;           /* [N][H][W][g_cstride], channels [0, Cout) */
    const void *w;           /* cdnet_dilated_pack_weights_bwd */
    void *dx;                /* [N][H][W][dx_cstride] */
    int N, H, W;
    int Cout, g_cstride;
    int Cin, dx_cstride, dx_coff;
    int taps, dilation;
    int accumulate;
    int f32;
} cdnet_dilated_bwd_data_args;
int cdnet_dilated_pack_weights_bwd(const float *w, void *packed, int Cin, int Cout, int taps, int f32, void *stream);
int cdnet_dilated_conv_backward_data(const cdnet_dilated_bwd_data_args *args, void *stream);

/* weight gradient, fp32 mode: dw fp32 [Cout][Cin][taps] in torch's layout (the parameter's view of the flat gradient buffer), stored.
 * x is read at its channel stride (the block buffer with Cin of its channels), g compact; both strides are multiples of 8 and channels
 * >= Cin / >= Cout are selected to zero, never multiplied.  The pixels are reduced on the matrix cores (both operands split into bf16
 * hi / lo on load, a_lo b_hi + a_hi b_lo + a_hi b_hi as in conv32.hip) into split-K slabs in `ws`, then summed in slab order by a second
 * launch: no floating-point atomics, two runs give the same bits.  ws_bytes >= cdnet_dilated_wgrad_workspace_bytes of the same shape. */
typedef struct cdnet_dilated_wgrad_args {
    const float *x;          /* [N][H][W][x_cstride], channels [0, Cin) */
    const float *g;          /* [N][H][W][g_cstride], channels [0, Cout) */
    float *dw;               /* [Cout][Cin][taps] */
    void *ws;
    size_t ws_bytes;
    int N, H, W;
    int Cin, x_cstride;
    int Cout, g_cstride;
    int taps, dilation;
} cdnet_dilated_wgrad_args;
size_t cdnet_dilated_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int taps);
int cdnet_dilated_conv_backward_weight(const cdnet_dilated_wgrad_args *args, void *stream);

/* BatchNorm2d in train() behind the LeakyReLU, plus F.dropout(training=True) of a dense layer's output (:33-35, :49-51), written into a
 * channel slice.  z fp32 [P][z_cstride] is the stored LeakyReLU output (P = N H W pixels, C real channels).
 *   forward:  per-tile sums [T][2][C] -> cdnet_bn_finalize_train (mean, invstd saved; running statistics with momentum and the unbiased
 *             variance) -> out[p][out_coff + c] = ((z - mean) invstd gamma + beta) m / (1 - p_drop)
 *   backward: dyh = dy m / (1 - p_drop); dbeta = sum dyh, dgamma = sum dyh xhat (per-tile sums, fixed tree with an fp64 top, stored);
 *             g[p][c] = gamma invstd (dyh - dbeta / P - xhat dgamma / P) * (z > 0 ? 1 : slope), compact at g_cstride
 * m is cdnet_dropout_mask's bit of element p * C + c of (key, layer), regenerated, never stored; p_drop = 0 skips the step exactly.
 * ws_floats >= cdnet_slice_bn_workspace_floats(P, C).  Channels outside the slice are not touched. */
typedef struct cdnet_slice_bn_fwd_args {
    const float *z;
    float *out;              /* [P][out_cstride] */
    const float *gamma, *beta;
    float *running_mean, *running_var;       /* [C], updated in place (both NULL: not tracked) */
    float *mean, *invstd;    /* [C] saved for backward */
    float *ws;
    size_t ws_floats;
    long long P;
    int C, z_cstride, out_cstride, out_coff;
    float eps, momentum, p_drop;
    int layer;
    unsigned long long key;
} cdnet_slice_bn_fwd_args;
typedef struct cdnet_slice_bn_bwd_args {
    const float *dy;         /* [P][dy_cstride], channels [dy_coff, dy_coff + C) */
    const float *z;
    const float *mean, *invstd, *gamma;
    float *dgamma, *dbeta;   /* [C] */
    float *g;                /* [P][g_cstride] */
    float *ws;
    size_t ws_floats;
    long long P;
    int C, z_cstride, dy_cstride, dy_coff, g_cstride;
    float slope, p_drop;
    int layer;
    unsigned long long key;
} cdnet_slice_bn_bwd_args;
size_t cdnet_slice_bn_workspace_floats(long long P, int C);
int cdnet_slice_bn_train_forward(const cdnet_slice_bn_fwd_args *args, void *stream);
int cdnet_slice_bn_train_backward(const cdnet_slice_bn_bwd_args *args, void *stream);
/* mask[i] = 1 where element i of (key, layer) is kept, i < count: a counter-based hash (two rounds of splitmix64's finaliser over key,
 * layer and i; the upper 24 bits against p_drop * 2^24), independent of the launch geometry.  0 <= p_drop < 1. */
int cdnet_dropout_mask(unsigned long long key, int layer, size_t count, float p_drop, uint8_t *mask, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * FCN_pooling's resampling steps (resample.hip): nn.MaxPool2d(kernel_size=2, stride=2) behind trans1..trans4 and
 * nn.UpsamplingBilinear2d(scale_factor=4) behind trans5 and trans6 (models/FullNet.py:169-172, applied by nn.Sequential in :191), and
 * their backward, which autograd derives in the reference (train_util.py:193-195 loss.backward()).  NHWC.  One side of every entry is
 * compact (a channel stride alone), the other a channel slice [coff, coff + C) of a dense block's buffer: a transition's resampled output
 * lands in the next block's base channels and is never copied.  C >= 1 is any count; channels outside the slice and the padding channels
 * of either stride are not written.  Accesses are 16 bytes wide where every stride and offset is a multiple of 16 bytes and the bases are
 * 16-byte aligned (the index bytes: 4 / 8 bytes wide), with a scalar tail; otherwise scalar.  No atomics: every output element comes
 * from one thread in a fixed order of operations.  f32 = 1: fp32 tensors, f32 = 0: bf16.
 * Argument errors (CDNET_E_ARG: a null pointer, a count < 1, odd H or W of the pool, a stride below coff + C, source and destination the
 * same tensor, sizes beyond the 31-bit item index or 2^40 elements) are found before any HIP call. */

/* y[n][h][w][y_coff + c] = max of x[n][2h + dy][2w + dx][c], dy, dx in {0, 1}: bit-equal to one of the four inputs (ATen's rule: a later
 * element replaces the running maximum when it is greater or NaN).  idx (NULL: inference, not written) u8 [N][H/2][W/2][idx_cstride]
 * gets 2 dy + dx of the window's first maximum in raster order.  H, W are the INPUT's sizes, both even. */
int cdnet_maxpool2_forward(const void *x, int x_cstride, void *y, int y_cstride, int y_coff, uint8_t *idx, int idx_cstride, int N, int H, int W,
                           int C, int f32, void *stream);
/* dx[n][h][w][c] = dy[n][h/2][w/2][dy_coff + c] where idx names (h & 1, w & 1), 0 elsewhere; fp32.  Every element of channels [0, C) of dx
 * is stored (no memset).  H, W are dx's sizes. */
int cdnet_maxpool2_backward(const float *dy, int dy_cstride, int dy_coff, const uint8_t *idx, int idx_cstride, float *dx, int dx_cstride, int N,
                            int H, int W, int C, void *stream);
/* [N][Hs][Ws][C] -> [N][4 Hs][4 Ws][C], bilinear with align_corners=True.  Source coordinates in integers: q = h (Hs - 1), h0 = q / (H - 1),
 * lambda = float(q % (H - 1)) / float(H - 1) with H = 4 Hs, h1 = min(h0 + 1, Hs - 1); columns alike; every weight is a correctly rounded
 * quotient at any size.  y = (x00 (1 - lw) + x01 lw) (1 - lh) + (x10 (1 - lw) + x11 lw) lh in fp32 (bf16: rounded once, on the store).
 * Hs = 1 or Ws = 1 copies along that axis.  Hs, Ws <= 8192. */
int cdnet_upsample4_bilinear_forward(const void *x, int x_cstride, void *y, int y_cstride, int y_coff, int N, int Hs, int Ws, int C, int f32,
                                     void *stream);
/* the transpose in gather form, fp32: dx[n][hs][ws][c] = sum over the outputs (h, w) that read (hs, ws), in ascending (h, w) order, of
 * (wy wx) dy[n][h][w][dy_coff + c] with the forward's weights wy, wx. */
int cdnet_upsample4_bilinear_backward(const float *dy, int dy_cstride, int dy_coff, float *dx, int dx_cstride, int N, int Hs, int Ws, int C,
                                      void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Model-path streaming kernels (not convolutions).
 * cdnet_input_pack: f32 NCHW [N][C<=16][H][W] (the ToTensor output, my_transforms_direction.py:945) -> bf16 NHWC
 *   [N][H][W][16] with zero-padded channels.
 * cdnet_bn_fold_eval: nn.BatchNorm2d in eval(): scale = g/sqrt(rv+eps), shift = b + (conv_bias - rm)*scale.
 * cdnet_bn_finalize_train: nn.BatchNorm2d in train(): reduces the per-tile statistics emitted by cdnet_conv_forward
 *   (stats f32 [T][2][C], `count` = N*H*W elements per channel) into scale/shift for the consumers, saves
 *   mean/invstd for backward and updates running_mean/var (momentum, unbiased variance); all reductions are
 *   deterministic (fixed tree, fp64).
 * ---------------------------------------------------------------------------------------------------- */
int cdnet_input_pack(const float *x, int N, int C, int H, int W, void *out_bf16_nhwc16, void *stream);
/* the same layout change for the fp32-precision path: out f32 NHWC [N][H][W][16] */
int cdnet_input_pack_f32(const float *x, int N, int C, int H, int W, float *out_f32_nhwc16, void *stream);
int cdnet_bn_fold_eval(const float *gamma, const float *beta, const float *running_mean, const float *running_var,
                       const float *conv_bias, float eps, int C, float *scale, float *shift, void *stream);
int cdnet_bn_finalize_train(const float *stats, int T, int C, float count, const float *gamma, const float *beta,
                            const float *conv_bias, float eps, float momentum, float *running_mean,
                            float *running_var, float *scale, float *shift, float *save_mean, float *save_invstd,
                            void *stream);

/* A 64-channel head feature F = [relu](raw*scale + shift + res), recomputed on the fly from its stored pieces. */
typedef struct cdnet_head_feat {
    const uint16_t *raw;    /* 16-bit NHWC [N][H][W][64] */
    const uint16_t *res;    /* optional residual, same shape and format */
    const float *scale;     /* optional per-channel affine */
    const float *shift;
    int relu;
    int f16;                /* 0: raw/res are bf16, 1: fp16, 2: fp32 (pointers address float tensors; nothing is rounded to 16 bits) */
} cdnet_head_feat;

/* Direction-aware-mask head: replaces models/dam/model_unet_rev1.py:258-263 (point_conv, directionAtt,
 * direction_conv, maskAtt, mask_conv; revAttention :8-17).  head_weights: device f32 block of
 * CDNET_HEAD_WEIGHT_FLOATS = { point_conv.w[64], direction_conv.w[9][64], mask_conv.w[3][64], point_conv.b,
 * direction_conv.b[9], mask_conv.b[3], directionAtt.w, maskAtt.w[9] }.
 * Outputs f32 NCHW: mask [N][3][H][W], point [N][1][H][W], direction [N][9][H][W] (the tuple Unet.forward returns).
 * f3->raw = NULL (f1 / f2 plain bf16): `point` is an INPUT - it already holds point_conv(point feature) + bias, left there by the
 * convolution that produced the point feature (cdnet_conv_args.dot_out) - and only mask / direction are written. */
#define CDNET_HEAD_WEIGHT_FLOATS 855
int cdnet_dam_head_forward(const cdnet_head_feat *f1, const cdnet_head_feat *f2, const cdnet_head_feat *f3,
                           const float *head_weights, int N, int H, int W, float *mask, float *point,
                           float *direction, void *stream);
/* plain UNet classifier (models/unet.py:75,104 final_conv 64->K): f32 NCHW logits from a 64-channel feature */
int cdnet_final_conv1x1(const cdnet_head_feat *f, const float *w, const float *b, int K, int N, int H, int W,
                        float *out, void *stream);
/* bias gradient of a convolution that is not followed by BatchNorm (plain UNet's ConvTranspose2d, models/unet.py:30):
 * db[c] = sum over the npix pixels of grad_out (bf16 NHWC [npix][C]).  workspace: cdnet_bias_grad_workspace_floats(C). */
size_t cdnet_bias_grad_workspace_floats(int C);
int cdnet_bias_grad(const uint16_t *grad_out, size_t npix, int C, float *workspace, size_t workspace_floats, float *db, void *stream);
int cdnet_bias_grad_f32(const float *grad_out, size_t npix, int C, float *workspace, size_t workspace_floats, float *db, void *stream);   /* fp32-precision path */
/* backward of that classifier (plain-UNet training, train_util.py:126-200 loss.backward()): dlogits f32 [N][K][H][W] ->
 * df bf16 NHWC [N][H][W][64] (gradient of the activated feature), dw f32 [K][64], db f32 [K].  K <= 20 (the 3-class mask and
 * 5- / 9- / 17-class direction classifiers of the ablation heads, models/dam/model_unet_MandD*.py).
 * workspace: cdnet_final_conv1x1_backward_workspace_floats() floats. */
size_t cdnet_final_conv1x1_backward_workspace_floats(void);
int cdnet_final_conv1x1_backward(const cdnet_head_feat *f, const float *w, const float *dlogits, int K, int N, int H, int W,
                                 uint16_t *df, float *workspace, size_t workspace_floats, float *dw, float *db, void *stream);
/* The backbone U-Net's classifier (models/model_unet.py:166,194 final_conv 16->K, 1 <= K <= 20) on the 16-channel feature of the last
 * decoder block: a cdnet_head_feat whose raw is NHWC [N][H][W][16] (f16 = 0 / 1 / 2: bf16 / fp16 / fp32), 16-byte aligned, with the
 * optional per-channel scale / shift (both or neither) and ReLU; res must be NULL (CDNET_E_ARG otherwise).  fp32 arithmetic behind the
 * storage format.  Forward: f32 NCHW logits out[N][K][H][W].  Backward: dlogits f32 [N][K][H][W] -> df [N][H][W][16], the gradient of
 * the activated feature (bf16 for f16 = 0 / 1, f32 for f16 = 2; 16-byte aligned), dw f32 [K][16], db f32 [K]; the sums go through
 * per-workgroup partial rows in `workspace` (cdnet_final_conv1x1_c16_backward_workspace_floats() floats) and a fixed-order reduce:
 * no atomics, two runs give the same bits. */
int cdnet_final_conv1x1_c16(const cdnet_head_feat *f, const float *w, const float *b, int K, int N, int H, int W,
                            float *out, void *stream);
size_t cdnet_final_conv1x1_c16_backward_workspace_floats(void);
int cdnet_final_conv1x1_c16_backward(const cdnet_head_feat *f, const float *w, const float *dlogits, int K, int N, int H, int W,
                                     void *df, float *workspace, size_t workspace_floats, float *dw, float *db, void *stream);

/* cdnet_src_materialize: a convolution source with its pending transform - BatchNorm scale / shift, residual add, ReLU,
 * nn.MaxPool2d(2, 2[, ceil_mode]) (model_unet_rev1.py:268-287 backbone 'M' layers, unet.py:19), F.pad offset - written out
 * as a plain bf16 NHWC tensor out[N][H][W][C]: bit-identical to what cdnet_conv_forward stages on the fly for the same
 * source (H, W = the logical size after the pool).  Consumers of a max-pooled training-mode activation read this copy. */
/* Non-zero when cdnet_conv_forward runs these arguments on a producer / consumer kernel: 2 = conv_ws16_kernel (16-bit path, launches
 * without statistics: the only one that takes cdnet_conv_args.taps1 = 1), 1 = conv_ws_kernel, or in fp32 mode conv_ws32_kernel - the
 * only one that takes cdnet_conv_args.ws = 2 (the BatchNorm-backward sums of the layer the output feeds, beside the stores).
 * Nothing is launched. */
int cdnet_conv_ws_eligible(const cdnet_conv_args *args);

int cdnet_src_materialize(const cdnet_conv_src *src, int N, int H, int W, uint16_t *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Backward-weight of a convolution (the dW half of loss.backward(), train_util_dam.py:307), one call per input
 * source of the layer.  `src` is the layer's forward source (its lazy transform is re-applied while staging),
 * grad_out the bf16 NHWC gradient w.r.t. the layer's raw output [N][H*ostride][W*ostride][Cout].
 * Work is split over `ksplit` slices of the 8x16-pixel tiles; partial fp32 slabs (cdnet_conv_wgrad_slab_floats)
 * are summed in a fixed order (bit-reproducible) and scattered into dw, the PyTorch-layout gradient:
 *   mode 0: Conv2d [Cout][Cin_real][KH][KW]; mode 2: ConvTranspose2d k4s2p1 [Cin_real][Cout][4][4];
 *   mode 3: ConvTranspose2d k2s2 [Cin_real][Cout][2][2].
 * src_coff: first channel of this source inside the weight's input-channel axis (torch.cat order); Csrc_real: real
 * channels of the source (3 for the zero-padded RGB stem).  ci_tiles in {1,2,4}: the workgroup owns
 * ci_tiles*32 input channels x (4/ci_tiles)*32 output channels.
 * ---------------------------------------------------------------------------------------------------- */
size_t cdnet_conv_wgrad_slab_floats(int C_src, int Cout, int taps, int npar, int ci_tiles, int ksplit);
int cdnet_conv_backward_weight(const cdnet_conv_src *src, int src_coff, int Csrc_real, int Cin_real,
                               const uint16_t *grad_out, int Cout, int N, int H, int W, int taps, int npar,
                               int ostride, int ci_tiles, int ksplit, float *slab, float *dw, int mode, void *stream);

/* The kernel instantiation the calling thread's last cdnet_conv_backward_weight launched (host-side record, thread-local like
 * cdnet_last_error; 0 before the first launch).  For tests, which assert the dispatch form of every case.  Bit layout:
 *   bits 0-3 family (CDNET_WGRAD_FAMILY_*), 4-7 CI_T, 8-11 CO_T (32-channel tiles of the workgroup's dW block), 12-15 TAPS,
 *   bit 16 RES (residual template form), bits 17-18 XF (0 plain, 1 fast, 2 generic; the fp32 kernel applies transforms at run time: 0),
 *   bits 19-21 QM (quadrant mode of the fp32 kernels; 0 for the 16-bit ones). */
#define CDNET_WGRAD_FAMILY_GEN  1   /* wgrad_kernel */
#define CDNET_WGRAD_FAMILY_WS   2   /* wgrad_ws_kernel */
#define CDNET_WGRAD_FAMILY_F32  3   /* wgrad_f32_kernel */
#define CDNET_WGRAD_FAMILY_WS32 4   /* wgrad_ws32_kernel */
int cdnet_conv_backward_weight_last_form(void);

/* Deferred split-K reduction: `mode | CDNET_WGRAD_DEFER_REDUCE` makes cdnet_conv_backward_weight stop after the slabs (which then
 * must stay untouched - one slab buffer per call); cdnet_wgrad_reduce_batch sums the slabs of any number of such calls and scatters
 * into their dw in ONE launch, bit-identical to the per-call reduction (same fixed order).  The table lives in device memory:
 * entries filled on the host by cdnet_wgrad_reduce_desc_fill (block0 = sum of the `blocks` of the entries before it), copied by
 * the caller; total_blocks = block0 + blocks of the last entry.  (The reference has no counterpart: autograd accumulates dW inside
 * cuDNN's backward-filter call, train_util_dam.py:307.) */
#define CDNET_WGRAD_DEFER_REDUCE 0x100
typedef struct cdnet_wgrad_reduce_desc {
    const float *slab;
    float *dw;
    int ksplit, npar, ci_blocks, co_blocks, taps, CI, CO, Csrc_real, Cin_real, src_coff, Cout, mode;
    int block0, blocks;
} cdnet_wgrad_reduce_desc;
int cdnet_wgrad_reduce_desc_fill(int C_src, int src_coff, int Csrc_real, int Cin_real, int Cout, int taps, int npar, int ci_tiles,
                                 int ksplit, const float *slab, float *dw, int mode, int block0, cdnet_wgrad_reduce_desc *out);
int cdnet_wgrad_reduce_batch(const cdnet_wgrad_reduce_desc *table_dev, int n, int total_blocks, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Training-only streaming kernels.  Together with cdnet_conv_forward (backward-data packs) and
 * cdnet_conv_backward_weight they replace loss.backward() / optimizer.step() of train_util_dam.py:303-308.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct cdnet_grad_in {     /* gradient w.r.t. a tensor as delivered by ONE of its consumers */
    const uint16_t *g;             /* bf16 NHWC [N][Hg][Wg][C] */
    int Hg, Wg;
    int oy, ox;                    /* the consumer read the tensor through F.pad offsets (oy, ox) */
    int pooled;                    /* the consumer read maxpool2x2 of the tensor: route to the first maximum */
    int coff, cstride;             /* channel slice [coff, coff+C) of a tensor with cstride channels (concat consumers) */
    int pad_;
} cdnet_grad_in;

typedef struct cdnet_bn_bwd_args {
    const uint16_t *raw;           /* the layer's stored forward output [N][H][W][C] (fp16 when f16 = 1, else bf16) */
    const uint16_t *res;           /* residual that was added before the ReLU (same format) or NULL; with relu = 2: the stored
                                      post-ReLU OUTPUT of the unit (bf16) - the ReLU mask is read from it instead of being recomputed */
    const float *scale, *shift;    /* forward per-channel affine (BatchNorm as applied), NULL = identity */
    const float *mean, *invstd;    /* saved batch statistics; NULL = no BatchNorm (gradient passes through) */
    cdnet_grad_in gin[3];
    int ngin;
    int f16, relu;                 /* relu: 0 none, 1 relu(affine [+ res]), 2 mask = res > 0 (fused residual epilogue of cdnet_conv_forward) */
    int N, H, W, C;
    /* Head-coefficient source (hc_nk = 0: none).  Gradient source number hc_slot is then not a stored tensor (gin[hc_slot].g = NULL, its
     * Hg x Wg = H x W, nothing else set) but the DAM head's feature gradient rebuilt per element from the per-pixel coefficient rows of
     * cdnet_dam_head_backward_coef, hc_coef f32 [N * H * W][16], and hc_nk rows of 64 weights inside the head weight block, hc_w f32
     * [hc_nk][64]:   v = fma(coef[p][hc_k0], w[0][c], +0);  v = fma(coef[p][hc_k0 + k], w[k][c], v), k = 1 .. hc_nk - 1
     * - the operations, in the order, of the head kernels' own dF, so the value has the bits of the tensor it replaces, and it is added
     * at position hc_slot of the sum over the sources.  hc_nk is 3 (mask head: hc_k0 = 10) or 9 (direction head: hc_k0 = 1), C = 64.
     * Served by cdnet_bn_backward alone, for fp32 tensors with same-size sources, res and dz_out (the flat fp32 residual form); every
     * other entry or plan refuses the arguments (CDNET_E_ARG) before any launch. */
    const float *hc_coef, *hc_w;
    int hc_slot, hc_k0, hc_nk, hc_pad_;
} cdnet_bn_bwd_args;

/* BatchNorm(train) + residual + ReLU backward with the consumers' max-pool / pad routing and the summation of up to
 * three consumer gradients fused in:  dz = (sum_k g_k) * [activation > 0];  dgamma = sum dz*xhat;  dbeta = sum dz;
 * draw = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)) (bf16); dz_out (optional, bf16) = dz for the residual
 * branch.  workspace: cdnet_bn_backward_workspace_floats(C) floats. */
size_t cdnet_bn_backward_workspace_floats(int C);
/* The two passes of cdnet_bn_backward as separate calls for the plain case (one same-size gradient source, BatchNorm + ReLU, no
 * residual branch).  cdnet_bn_backward_stats (16-bit tensors) = reduce + finalize; it also writes ktab f32 [7][C] =
 * scale | shift | mean | invstd | k1 | k2 | k3, the table cdnet_bn_backward_apply reads (the second pass alone: draw = k1 * (dz - k2 -
 * xhat * k3); 16-bit and fp32 tensors; relu = 0 as well: the one source is a gradient that already passed the ReLU, the dz a
 * residual unit's sums pass or cdnet_dam_head_backward_fused stored).  The trainer uses finalize + apply behind a backward-data launch that carried the sums
 * (cdnet_conv_args.ws = 2, fp32 mode). */
int cdnet_bn_backward_stats(const cdnet_bn_bwd_args *args, const float *gamma, float *dgamma, float *dbeta, float *workspace,
                            size_t workspace_floats, float *ktab, void *stream);
int cdnet_bn_backward_apply(const cdnet_bn_bwd_args *args, const float *ktab, uint16_t *draw, void *stream);
/* The finalize pass alone, over partial rows f32 [nb][2][C] produced by the backward-data launch that computed this layer's output
 * gradient: cdnet_conv_args.ws = 2 with eres = the layer's raw fp16 forward output [N][H][W][Cout], oscale / oshift / eres_scale /
 * eres_shift = its BatchNorm scale / shift / batch mean / invstd (f32 [Cout]), stats = the partial rows (4 per workgroup of the
 * producer / consumer kernel, at most 1024: zero-fill the buffer once and pass nb = 1024).  The first BatchNorm-backward pass then costs no pass of
 * its own over the two tensors.  Writes dgamma, dbeta and rows 4..6 (k1 | k2 | k3) of ktab - what cdnet_bn_backward_apply reads; rows 0..3 are not touched
 * (fp32 mode: eres = the raw fp32 output, conv_ws32_kernel). */
int cdnet_bn_backward_finalize(const cdnet_bn_bwd_args *args, const float *gamma, float *dgamma, float *dbeta, const float *partial,
                               int nb, float *ktab, void *stream);
int cdnet_bn_backward(const cdnet_bn_bwd_args *args, const float *gamma, float *dgamma, float *dbeta, float *workspace,
                      size_t workspace_floats, uint16_t *draw, uint16_t *dz_out, void *stream);

/* The launch plan of the calling thread's last BatchNorm-backward kernel launch (any of the four entries; host-side record,
 * thread-local like cdnet_last_error; 0 before the first launch; a refused call leaves it alone).  For tests, which assert the kernel
 * instantiation and the workgroup count of every case.  cdnet_bn_backward_last_sums_plan: the same record of the last SUMS pass (the
 * fused entry launches sums, finalize, apply: its apply pass is what cdnet_bn_backward_last_plan then returns).  Bit layout:
 *   bits 0-1  path (CDNET_BN_PATH_*)
 *   bit  2    f32: the fp32 kernels (4 channels per thread on the window / flat paths)
 *   bits 3-4  NF (window: same-size sources beside the pooled one, 0-2) or NG (flat: gradient sources, 1-3); 0 on the generic path
 *   bit  5    RES (flat: the residual template form); 0 elsewhere
 *   bits 6-7  kp (window: position of the pooled source among the sources); 0 elsewhere
 *   bit  8    pass: 0 sums, 1 apply
 *   bit  9    the apply pass ran on the dz the sums pass stored (one plain source, no mask) instead of the caller's sources
 *   bits 10-21 nb: workgroups of the launch = partial rows of the sums pass (1 .. 2048) */
#define CDNET_BN_PATH_WINDOW  1   /* bn_bwd_window_kernel / bn_bwd_window32_kernel */
#define CDNET_BN_PATH_FLAT    2   /* bn_bwd_flat_kernel / bn_bwd_flat32_kernel */
#define CDNET_BN_PATH_GENERIC 3   /* bn_bwd_generic_kernel */
int cdnet_bn_backward_last_plan(void);
int cdnet_bn_backward_last_sums_plan(void);

/* DAM head backward (model_unet_rev1.py:258-263): gradients of the three logit maps (f32 NCHW) -> gradients of the
 * three 64-channel features (bf16 NHWC) and of the head weights (f32, CDNET_HEAD_WEIGHT_FLOATS layout). */
size_t cdnet_dam_head_backward_workspace_floats(int N, int H, int W);
int cdnet_dam_head_backward(const cdnet_head_feat *f1, const cdnet_head_feat *f2, const cdnet_head_feat *f3,
                            const float *head_weights, const float *dmask, const float *dpoint, const float *ddir,
                            int N, int H, int W, uint16_t *df1, uint16_t *df2, uint16_t *df3, float *workspace,
                            size_t workspace_floats, float *dhead_weights, void *stream);
/* The same in ONE pass over the features for the fp32 training step (model_unet_rev1.py:150-170 - the residual unit whose output is the
 * third feature -, :258-263; loss.backward(), train_util_dam.py:303-308): the feature gradients and the head's weight gradients from one
 * kernel that reads each feature once and writes no per-pixel coefficient tensor.  Serves one case and refuses every other
 * (CDNET_E_ARG): f1, f2, f3 are plain stored fp32 NHWC tensors with 64 channels (f16 = 2, no scale / shift / relu / res), f3 the output
 * of a residual unit with the fused epilogue that the head alone reads.
 *   df1, df2 f32 [N][H][W][64]: the feature gradients
 *   dz3 f32 [N][H][W][64] = (f3 > 0) ? dF3 : 0: the gradient behind the unit's ReLU (dF3 itself is not stored); the unit's bn2 takes it
 *       as a relu = 0 source without residual (cdnet_bn_backward: its sums pass then reads two tensors and writes none)
 *   dhead_weights as above.  workspace: cdnet_dam_head_backward_fused_workspace_floats().
 * Every sum is taken in the order of cdnet_dam_head_backward (cdnet_dam_head_backward_fused_blocks() = its 1024 workgroups): df1, df2,
 * dz3 = [f3 > 0] df3 and dhead_weights are bit-identical to its results. */
int cdnet_dam_head_backward_fused_blocks(void);
int cdnet_dam_head_backward_fused_scratch_bytes(void);   /* scratch bytes per lane of the kernel as built (-1: query failed); expected 0 */
size_t cdnet_dam_head_backward_fused_workspace_floats(void);
int cdnet_dam_head_backward_fused(const cdnet_head_feat *f1, const cdnet_head_feat *f2, const cdnet_head_feat *f3,
                                  const float *head_weights, const float *dmask, const float *dpoint, const float *ddir, int N, int H,
                                  int W, float *df1, float *df2, float *dz3, float *workspace, size_t workspace_floats,
                                  float *dhead_weights, void *stream);
/* The same launch without df1 and df2: they are rank 3 and rank 9 per pixel, dF1[p][c] = sum_k dm_k[p] wm[k][c] and dF2[p][c] = sum_k
 * du_k[p] wd[k][c], so what leaves is the pixel's coefficient row coef f32 [N * H * W][16] = [dpt | du[0..8] | dm[0..2] | 0 0 0] - the
 * layout and the bits of the rows cdnet_dam_head_backward keeps in its workspace -, 64 bytes a pixel in place of 512.  The one reader of
 * each gradient, the sums pass of its residual unit's bn2, rebuilds the element (cdnet_bn_bwd_args.hc_*).  dz3, dhead_weights,
 * workspace, the refusals and the order of every sum are cdnet_dam_head_backward_fused's. */
int cdnet_dam_head_backward_coef_scratch_bytes(void);    /* as cdnet_dam_head_backward_fused_scratch_bytes, of this form's kernel */
int cdnet_dam_head_backward_coef(const cdnet_head_feat *f1, const cdnet_head_feat *f2, const cdnet_head_feat *f3,
                                 const float *head_weights, const float *dmask, const float *dpoint, const float *ddir, int N, int H,
                                 int W, float *coef, float *dz3, float *workspace, size_t workspace_floats, float *dhead_weights,
                                 void *stream);

/* The five-term CDNet loss (train_util_dam.py:167-276; loss.py:131-260) and its gradient w.r.t. the logits.
 * label u8 {0,1,2}, dirlab u8 0..8, point target f16, weight map u8 (divided by 20 on the fly, :102).
 * quirk_sample0 = 1 reproduces train_util_dam.py:139 (direction one-hot masked by sample 0's foreground).
 * losses[11] = {total, direction CE, direction weighted dice, MSE, CE, dice, then the pixel-level metrics of
 * train_util_dam.py:279-293 (argmax direction class == 1 vs direction label == 1, utils.py:67-110), averaged over the batch:
 * accuracy, IoU, recall, precision, F1}.  dmask/dpoint/ddir may all be NULL (values only); some but not all of them: CDNET_E_ARG.
 * Label content is validated on the device: a mask class > 2 or a direction class > 8 makes every entry of `losses` NaN
 * (indices are clamped, nothing is read or written out of bounds) - the reference's nn.NLLLoss raises on such targets.
 */
size_t cdnet_dam_loss_workspace_floats(int B, int P);
int cdnet_dam_loss(const float *mask, const float *point, const float *direction, const uint8_t *label,
                   const uint8_t *dirlab, const uint16_t *point_target_f16, const uint8_t *weight_u8, int B, int H, int W,
                   int quirk_sample0, float *workspace, size_t workspace_floats, float *losses, float *dmask,
                   float *dpoint, float *ddir, void *stream);
/* the same loss for direction maps of direction_classes = 5, 9 or 17 classes (options.py:45 "4 8 16" + background; the 4- and
 * 16-direction ablation models models/dam/model_unet_MandD4.py / model_unet_MandD16.py): direction / ddir f32 [B][classes][H][W],
 * dirlab u8 0..classes-1; loss.py:216-260 runs its cyclic neighbour terms over 1..classes-1 and averages over `classes`.
 * cdnet_dam_loss is this entry with 9 classes. */
size_t cdnet_dam_loss_classes_workspace_floats(int B, int P, int direction_classes);
int cdnet_dam_loss_classes(const float *mask, const float *point, const float *direction, const uint8_t *label,
                           const uint8_t *dirlab, const uint16_t *point_target_f16, const uint8_t *weight_u8, int B, int H, int W,
                           int direction_classes, int quirk_sample0, float *workspace, size_t workspace_floats, float *losses,
                           float *dmask, float *dpoint, float *ddir, void *stream);

/* The switches of the mask and DAM losses (options.py --weight-map, --dice, --alpha 2): one word of term bits. */
#define CDNET_LOSS_WMAP 1u   /* CE map x weight / 20 (train_util.py:134-135) */
#define CDNET_LOSS_CE   2u   /* mask CE in total and gradient */
#define CDNET_LOSS_DICE 4u   /* MulticlassDiceLoss of softmax(mask) in total and gradient */

/* cdnet_dam_loss_classes with the term word; cdnet_dam_loss_classes is this entry with every term set, with unchanged results.
 *   WMAP clear (--weight-map 0, train_util_dam.py:170-172, 229-246): both CE maps are unweighted and weight_u8 may be NULL; the direction dice
 *     becomes the plain MulticlassDiceLoss over the direction classes (:241-244: a sum over the classes, no / classes, no doubled class 0, no
 *     neighbour terms) against the same one-hot target (sample-0 quirk and constant-map rule kept); slot 2 of `losses` reports it.
 *   CE clear (--alpha 2, :182-189): the mask CE leaves the total and dmask and stays in slot 4.
 *   DICE clear: CDNET_E_ARG - the reference has no working DAM configuration without it (--dice 0|2 dies at :297 on an unbound
 *     loss_direction_dice). */
int cdnet_dam_loss_terms(const float *mask, const float *point, const float *direction, const uint8_t *label,
                         const uint8_t *dirlab, const uint16_t *point_target_f16, const uint8_t *weight_u8, int B, int H, int W,
                         int direction_classes, int quirk_sample0, float *workspace, size_t workspace_floats, float *losses,
                         float *dmask, float *dpoint, float *ddir, void *stream, unsigned terms);

/* The plain UNet's loss and pixel metrics (mask_loss.hip).  Replaces train_util.py:128-136 (log-softmax + NLL, x weight map / 20 with
 * add_weightMap), :183-190 (MulticlassDiceLoss of the softmax, loss.py:131-176; dice = 2: the dice term alone), :209-218 with utils.py:67-110
 * (accuracy_pixel_level of the arg-max), and the gradient autograd takes; validate's unweighted CE (:387-389) is the same entry with WMAP clear.
 * mask_logits f32 [B][3][H][W]; label u8 [B][H][W] in {0,1,2}; weight_u8 u8 [B][H][W], NULL allowed when WMAP is clear; 1 <= B <= 64.
 * losses f32 [8] = {total, ce, dice, accuracy, IoU, recall, precision, F1}: ce = mean of -log p_label (x w / 20 with WMAP), dice = sum_c
 * (1 - mean_b 2 (I_c + 1) / (P_c + T_c + 1)); both are always reported, total holds the terms that are on (both: the fp32 sum ce + dice).  The
 * metrics score arg-max (first maximum) == 1 against label == 1 from per-sample tp / fp / fn counts, finished in double.
 * dmask NULL or f32 [B][3][H][W]: written (not accumulated) with d total / d logits - zeros when neither term is on; cdnet_variance_loss and
 * cdnet_boundary_loss add to it afterwards.  A label above 2 makes all eight values NaN and nothing is read or written out of bounds.
 * With WMAP | CE | DICE the values and the gradient equal cdnet_dam_loss_classes' mask terms bit for bit.  No atomics except the error flag,
 * no host synchronisation, fixed-order sums; argument errors (CDNET_E_ARG, a short workspace included) are found before any HIP call.
 * workspace: cdnet_mask_loss_workspace_floats(B, H * W) floats. */
size_t cdnet_mask_loss_workspace_floats(int B, int P);
int cdnet_mask_loss(const float *mask_logits, const uint8_t *label, const uint8_t *weight_u8, int B, int H, int W, unsigned terms,
                    float *workspace, size_t workspace_floats, float *losses, float *dmask, void *stream);

/* The instance variance term of the training loss (--alpha 1; --alpha 2, :182-189: alpha = 2 here and CDNET_LOSS_CE clear in the loss entry).
 * Replaces train_util_dam.py:174-180: F.softmax of the mask logits, the per-sample
 * skimage.measure.label(target == 1) on the CPU (8-connectivity) and LossVariance (loss.py:9-33), with the gradient autograd takes through both:
 *   loss_var = (1/B) sum_k [ sum over the instances with n > 1 pixels and the K channels of  sum_i (p_ci - mu_c)^2 / (n - 1) ] / (U_k + 1e-8),
 *   U_k = number of instances of sample k (single pixels included); a sample without foreground contributes 0.
 * mask_logits f32 [B][K][H][W], K in {2, 3}; label u8 [B][H][W], an instance pixel is label == fg_value (1).
 * loss_var f32 [1] is written; total (NULL or f32 [1]): *total += alpha * loss_var; dmask (NULL or f32 [B][K][H][W]): += alpha * d loss_var /
 * d logits; root_out (NULL or i32 [B][H][W]): the raster-first pixel index (y * W + x) of the pixel's instance, -1 off the mask; counts (NULL
 * or i32 [B]): U_k.  Bit-identical from call to call (fixed-point integer accumulation, fixed-order sums).  No host synchronisation: graph-capturable.
 * workspace: cdnet_variance_loss_workspace_bytes(B, K, H, W) bytes, 8-byte aligned (0 for shapes / K the entry does not serve). */
size_t cdnet_variance_loss_workspace_bytes(int B, int K, int H, int W);
int cdnet_variance_loss(const float *mask_logits, const uint8_t *label, int fg_value, int B, int K, int H, int W, float alpha,
                        void *workspace, size_t workspace_bytes, float *loss_var, float *total, float *dmask, int32_t *root_out,
                        int32_t *counts, void *stream);

/* The boundary / focal term of the training loss (--boundary-loss 1|2|3).  Replaces train_util_dam.py:195-208 and train_util.py:170-178, which
 * add BoundaryLoss (loss.py:331-393, kind 1), FocalLoss2d (loss.py:37-78, kind 2) or RobustFocalLoss2d (loss.py:81-127, kind 3) of the mask
 * logits and the one-hot target to the loss, with the gradient autograd takes.
 *   kind 1: p = softmax(z), t = [label == c], every pooling window clipped to the image (F.max_pool2d pads with -inf):
 *     gt_b = t - min3x3(t), gt_ext = max5x5(gt_b), pr_b = p - min3x3(p) (the reference's maxpool(1 - p) - (1 - p)), pr_ext = max5x5(pr_b);
 *     per (sample, class)  P = sum(pr_b gt_ext) / (sum(pr_b) + 1e-7),  R = sum(pr_ext gt_b) / (sum(gt_b) + 1e-7),  BF1 = 2PR / (P + R + 1e-7);
 *     loss = mean over (sample, class) of 1 - BF1.  A pool's gradient goes to the window's FIRST maximum in raster order (ATen's rule).
 *   kind 2: every logit element is one binary example: pt = t ? sigmoid(z) : 1 - sigmoid(z) clamped to [1e-8, 1 - 1e-8] (1 in fp32; gradient 0
 *     outside), loss = mean of -(1 - pt)^2 log(pt) over the B K H W elements.  pt is formed in fp32 as the reference forms it.
 *   kind 3: the robust form clamps (1 - pt)^2 to [0, 2], which never binds for a probability: the same kernel as kind 2, bitwise equal results.
 * The one-hot target is [label == c] for the classes 0, 1, 2.  The reference builds it from np.unique over the batch (train_util_dam.py:85-100),
 * which shifts the channels when a batch lacks a class; that accident is NOT reproduced.
 * mask_logits f32 [B][3][H][W] (K != 3: CDNET_E_ARG), any H, W >= 1; label u8 [B][H][W] in {0,1,2} - a larger value makes loss_out NaN (as
 * cdnet_dam_loss) and nothing is read or written out of bounds.  loss_out f32 [1] is always written; total (NULL or f32 [1]): *total += beta *
 * loss; dmask (NULL or f32 [B][3][H][W]): += beta * d loss / d logits.  No host synchronisation, no atomics: per-workgroup partials summed in
 * a fixed order, bit-identical from call to call, graph-capturable.  Two launches.
 * workspace: cdnet_boundary_loss_workspace_bytes(kind, B, K, H, W) bytes, 8-byte aligned (0 for what the entry does not serve); a NULL or short
 * workspace is an argument error (CDNET_E_ARG), found like the other argument errors before any HIP call. */
size_t cdnet_boundary_loss_workspace_bytes(int kind, int B, int K, int H, int W);
int cdnet_boundary_loss(const float *mask_logits, const uint8_t *label, int kind, int B, int K, int H, int W, float beta,
                        void *workspace, size_t workspace_bytes, float *loss_out, float *total, float *dmask, void *stream);
int cdnet_boundary_loss_scratch_bytes(void);   /* scratch bytes per lane of kind 1's gradient kernel as built (-1: query failed); expected 0 */

/* validate() loss mix of train_util_dam.py:367-636 (default options): per-sample sums of ONE pass over the logits, combined on the
 * host by cdnet_amd.train_util_dam.validate.  sums f32 [B][CDNET_VAL_SUMS]:
 *   0..2 sum p_c [label==c], 3..5 sum p_c, 6..8 sum [label==c], 9 sum -log p_label (unweighted mask CE, :499-505);
 *   10..18 / 19..27 / 28..36 the same three sums for the direction probabilities with channel 0 multiplied by P(background)
 *   (:564-566) against the one-hot direction target - channel = dir_rank_host[class value] (the rank among the batch's unique
 *   values, :462-468; -1 = absent), zeroed off SAMPLE 0's foreground (:469); 37 sum w * -log q_dir (:553-559);
 *   38 sum (point - target / 255)^2 (:575-580); 39..41 tp, fp, fn of (argmax mask == 1) vs (label == 1) (:585-590).
 * workspace: cdnet_dam_val_sums_workspace_floats(B, H * W) floats. */
#define CDNET_VAL_SUMS 42
size_t cdnet_dam_val_sums_workspace_floats(int B, int P);
int cdnet_dam_val_sums(const float *mask, const float *point, const float *dirn, const uint8_t *label, const uint8_t *dirlab,
                       const uint16_t *point_target_f16, const uint8_t *weight_u8, const int *dir_rank_host, int B, int H, int W,
                       float *workspace, size_t workspace_floats, float *sums, void *stream);
/* the same for direction_classes = ND in {5, 9, 17} (model_unet_MandD4 / MandD16): dir_rank_host holds ND entries and
 * sums f32 [B][15 + 3 ND]: 0..9 as above, the three direction blocks at 10, 10 + ND, 10 + 2 ND (ND wide each), the five scalars
 * {weighted direction CE, MSE, tp, fp, fn} at 10 + 3 ND.  cdnet_dam_val_sums is this entry with ND = 9. */
size_t cdnet_dam_val_sums_classes_workspace_floats(int B, int P, int direction_classes);
int cdnet_dam_val_sums_classes(const float *mask, const float *point, const float *dirn, const uint8_t *label, const uint8_t *dirlab,
                               const uint16_t *point_target_f16, const uint8_t *weight_u8, const int *dir_rank_host,
                               int direction_classes, int B, int H, int W, float *workspace, size_t workspace_floats, float *sums,
                               void *stream);

/* torch.optim.Adam step (utils.py:915-918: betas (0.9, 0.99), L2 weight decay added to the gradient) on flat fp32
 * buffers; `step` is 1-based; grad_scale multiplies the gradient first (1/world_size after an all-reduce). */
int cdnet_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int step, float grad_scale, void *stream);

/* The reference's other optimisers (utils.py:907-939) on flat fp32 buffers.  The step-dependent coefficients are host
 * scalars: the caller computes them in double, as the reference does with math.sqrt and **, and passes them as float
 * (cdnet_amd/optim.py: moment_scalars).  Any 4-byte aligned slice of the flat buffers is served (16-byte accesses on the
 * aligned body when the buffers share one alignment).
 *
 * cdnet_moment_step - one update of the four moment rules, per element:
 *     g = grad * grad_scale;  v = v * beta2 + (1 - beta2) * g * g;  m = m * beta1 + (1 - beta1) * g       (always)
 *     move: p = p + (-decay) * p;  p = rect ? p - step_size * m / (sqrt(v) / v_div + eps) : p - step_size * m
 *     sync: slow = slow + alpha * (p - slow);  p = slow
 *   RAdam (hhl_utils/radam.py:6-81): rect = N_sma >= 5, decay = weight_decay * lr, v_div = 1, eps 1e-8.
 *   RAdam_4step(update_all=False, additional_four=False) (radam.py:84-180, utils.py:923-928): move = 0 for steps 1-4 (the moments
 *     advance, the parameters stay), then always rectified with v_div = sqrt(1 - beta2^t) and no (1 - beta2^t) in step_size.
 *   AdamW(warmup=4000) (radam.py:183-252, utils.py:929-932): rect = 1, step_size and decay from the warm-up rate lr_t, v_div = 1.
 *   Ranger (hhl_utils/ranger.py:26-165, utils.py:933-935): RAdam with rect = N_sma > 5, eps 1e-5, and the lookahead sync every
 *     k = 6 steps with alpha = 0.5; `slow` holds the parameters as they were when the first step started (ranger.py:113-114).
 *   `slow` may be NULL unless sync is set.  beta1 / beta2 are doubles so that (1 - beta) rounds to float as torch rounds it.
 * cdnet_sgd_step - torch.optim.SGD(lr, momentum, weight_decay), dampening 0, no Nesterov (utils.py:910-914): g = grad * grad_scale +
 *   weight_decay * p; buf = g at step 1, else momentum * buf + g; p = p - lr * buf.  `step` is 1-based. */
int cdnet_moment_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *slow, size_t n, double beta1,
                      double beta2, float grad_scale, int move, int rect, float decay, float step_size, float v_div, float eps,
                      int sync, float alpha, void *stream);
int cdnet_sgd_step(float *param, const float *grad, float *momentum_buffer, size_t n, float lr, float momentum, float weight_decay,
                   int step, float grad_scale, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Sliding-window inference.  Replaces utils.split_forward_dam (utils.py:658-726) and the construction of the eight
 * test-time-augmentation views (test_dam.py:313-385) without ever materialising a flipped / rotated / padded image.
 * cdnet_window_pack: img f32 [C<=16][H][W] -> ny*nx windows bf16 NHWC [ny*nx][tile_h][tile_w][16] of view `view_xform`
 *   (bit0 hflip, bit1 vflip, bit2 rot90 ccw first); window (ky,kx) starts at (ky*stride, kx*stride) of the view, pixels
 *   beyond the view are the zero padding of utils.py:665-676.
 * cdnet_window_stitch: window outputs f32 [ny*nx][K][tile_h][tile_w] -> out f32 [K][Hv][Wv], keeping for every pixel
 *   the last window whose interior (overlap/2 trimmed, except at the image border) contains it (utils.py:683-712).
 *   With more than one window along an axis the tile must hold that interior: tile >= stride + overlap/2 (CDNET_E_ARG
 *   otherwise; every geometry of utils.window_grid has tile = stride + overlap there).
 * ---------------------------------------------------------------------------------------------------- */
int cdnet_window_pack(const float *img, int C, int H, int W, int view_xform, int tile_h, int tile_w, int stride, int ny,
                      int nx, void *out_bf16_nhwc16, void *stream);
/* fp32-precision path: the same windows as f32 NHWC [ny*nx][tile_h][tile_w][16] */
int cdnet_window_pack_f32(const float *img, int C, int H, int W, int view_xform, int tile_h, int tile_w, int stride, int ny,
                          int nx, float *out_f32_nhwc16, void *stream);
int cdnet_window_stitch(const float *tiles, int K, int tile_h, int tile_w, int stride, int overlap, int ny, int nx, int Hv,
                        int Wv, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Training augmentation of the reference's default recipe, per sample on its whole source image, evaluated only where the crop needs it.
 * Replaces my_transforms_direction.py:155-181 (RandomColor: Color, Brightness, Contrast, Sharpness blends), :224-259 (random horizontal /
 * vertical flip), :262-352 (RandomElasticDeform, do_albu = 1: albumentations ElasticTransform(alpha, sigma, alpha_affine, nearest, zero
 * border) = random affine + Gaussian-smoothed displacement field), :445-473 (RandomChooseAug: BLUR / GaussianBlur / MedianFilter / none)
 * and :496-540 (RandomCrop; a source smaller than the crop is zero-padded with weight 0 instead of resized).
 *   cdnet_aug_sample: one source (device pointers, row strides: img in bytes, weight in bytes, label in elements) and its drawn parameters:
 *     minv = the inverse of the affine M (row-major 2 x 3, destination -> source pixel, in the flipped frame), color = the four factors,
 *     filter 0 none / 1 BLUR / 2 GaussianBlur(2) / 3 MedianFilter(3), (y0, x0) the crop origin, alpha = 0: no displacement field,
 *     seed: the field's counter-based noise.  label_i32 = 1: the label is an i32 instance-id plane, else u8 (channel 0 of the label image).
 *   samples: the table in device memory; samples_host: the same table in host memory (validation and launch geometry).
 *   norm_host: NULL or f32 [6] = mean[3], std[3] (the `normalize` transform).
 * Outputs: image f32 [B][3][size][size] (/ 255, normalised), weight u8 [B][size][size], label u8 or i32 [B][size][size] (label_i32),
 *   varied i32 [B] (0: the label crop holds one value - the DataFolder re-draw rule, data_folder.py:103-105), field NULL or
 *   f32 [B][2][size + 12][size + 12] (dx, dy over the crop + 6 px, origin (y0 - 6, x0 - 6); else kept in the workspace).
 * cdnet_augment_workspace_bytes: max_radius = the largest int(4 sigma + 0.5) of a sample with alpha != 0 (0 = none, at most 768); 0 for
 *   bad sizes.
 * Four launches (stats, two field passes when some alpha != 0, one tile pass).  The colour chain and the filters equal Pillow's bit for bit;
 * the geometry restates OpenCV 4's nearest warpAffine / remap (cv2 parity unpinned).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct cdnet_aug_sample {
    double minv[6];
    const uint8_t *img;
    const uint8_t *weight;
    const void *label;
    int32_t H, W, img_stride, weight_stride, label_stride, label_i32;
    float color[4];
    int32_t hflip, vflip, filter, y0, x0;
    float alpha, sigma;
    uint32_t seed;
} cdnet_aug_sample;
size_t cdnet_augment_workspace_bytes(int B, int size, int max_radius);
int cdnet_augment_batch(const cdnet_aug_sample *samples, const cdnet_aug_sample *samples_host, int B, int size, const float *norm_host,
                        void *workspace, size_t workspace_bytes, float *image, uint8_t *weight, void *label, int label_i32, int32_t *varied,
                        float *field, void *stream);

/* The three optional steps of the reference's chain (options.py:331-347 fixes the order random_resize -> random_color -> random_affine ->
 * flips -> random_elastic -> random_rotation -> random_chooseAug -> random_crop), all nearest-neighbour geometry on image, weight and label
 * together, traced back per output pixel like the rest:
 *   random_resize (my_transforms_direction.py:69-151, albu.Resize nearest): the source is seen as a virtual Hr x Wr image, row y reading
 *     stored row min(floor(y * (1 / (Hr / H))), H - 1) (OpenCV's INTER_NEAREST rule, cv2 parity unpinned); every later step - the Contrast
 *     mean, Sharpness's neighbours, the elastic affine, the field, the crop origin - works in Hr x Wr.  Nothing is materialised.
 *   random_affine (:185-220, PIL Image.transform(AFFINE), NEAREST): paff = Pillow's a b c d e f (output -> input pixel), applied in Pillow's
 *     16.16 fixed point, bit for bit; outside reads 0.  (For b = d = 0 Pillow itself takes a scaling path that accumulates in double;
 *     the two agree for the identity, which is all random_affine can draw with b = d = 0, and are not pinned for other pure scales.)
 *   random_rotation (:354-440, albu.Rotate nearest, zero border): rinv = the inverse (invertAffineTransform's formula) of
 *     getRotationMatrix2D((Wr / 2, Hr / 2), angle, 1), applied in OpenCV's fixed point like minv (cv2 / albumentations parity unpinned).
 *   cdnet_aug_geo: one row per sample beside cdnet_aug_sample: flags = 1 resize | 2 affine | 4 rotation (a step whose bit is clear is
 *     skipped; without bit 1, Hr x Wr must equal H x W); (fy0, fx0) = the origin of the sample's displacement-field window.
 *   field_edge: the window's edge, one per batch.  The field is needed where the rotation's pre-image of the crop + 6 px falls: with no
 *     rotation that is size + 12 at (y0 - 6, x0 - 6) - then the call computes what cdnet_augment_batch does; else the caller takes the
 *     bounding box of the four corner pre-images (+ 2 px, clipped to the image).  The fixed-point map is monotone in each coordinate,
 *     so that box holds every pixel's pre-image: the entry checks before any launch that, for a sample with alpha != 0, the part of
 *     the box inside the image lies in the window (every field lookup then does), and that 1 <= Hr, Wr <= 32767, the matrices are
 *     finite, the affine stays in Pillow's 16.16 range and the crop origin lies inside Hr x Wr (CDNET_E_ARG otherwise).
 *   field (optional output): f32 [B][2][field_edge][field_edge], origin (fy0, fx0) per sample, 0 outside the image.
 * cdnet_augment_geo_workspace_bytes: as cdnet_augment_workspace_bytes for a window of field_edge; 0 for bad sizes. */
typedef struct cdnet_aug_geo {
    double paff[6];
    double rinv[6];
    int32_t Hr, Wr, fy0, fx0;
    uint32_t flags;
    int32_t reserved;
} cdnet_aug_geo;
size_t cdnet_augment_geo_workspace_bytes(int B, int size, int max_radius, int field_edge);
int cdnet_augment_batch_geo(const cdnet_aug_sample *samples, const cdnet_aug_sample *samples_host, const cdnet_aug_geo *geo,
                            const cdnet_aug_geo *geo_host, int field_edge, int B, int size, const float *norm_host, void *workspace,
                            size_t workspace_bytes, float *image, uint8_t *weight, void *label, int label_i32, int32_t *varied, float *field,
                            void *stream);

/* The same two calls for a plane count: channels = 3 (RGB) is what cdnet_augment_batch / cdnet_augment_batch_geo compute, byte for byte;
 * channels = 1 is Pillow's mode L (grey-scale datasets); anything else is CDNET_E_ARG before any HIP call.
 *   img u8 [H][W][channels] (img_stride in bytes, >= channels * W), image f32 [B][channels][size][size], norm_host NULL or
 *   f32 [2 * channels] = mean[channels], std[channels].  The structs, the workspace entries, the geometry, the flips, the label / weight planes,
 *   the re-draw flag and the field are those of the RGB calls.
 * Mode L as Pillow computes it: ImageEnhance.Color is the identity for every factor (its degenerate image is the image itself; color[0]
 *   is ignored), Brightness blends with 0, Contrast's degenerate value is int(mean + 0.5) of the brightness-adjusted plane itself (no
 *   RGB -> L weights; u64 sum, divided in double), Sharpness blends with SMOOTH of the one plane (same summation order, 0.5 start, copied
 *   edge rows and columns), BLUR / GaussianBlur(2) / MedianFilter(3) work on the one plane. */
int cdnet_augment_batch_c(const cdnet_aug_sample *samples, const cdnet_aug_sample *samples_host, int B, int size, const float *norm_host,
                          void *workspace, size_t workspace_bytes, float *image, uint8_t *weight, void *label, int label_i32, int32_t *varied,
                          float *field, void *stream, int channels);
int cdnet_augment_batch_geo_c(const cdnet_aug_sample *samples, const cdnet_aug_sample *samples_host, const cdnet_aug_geo *geo,
                              const cdnet_aug_geo *geo_host, int field_edge, int B, int size, const float *norm_host, void *workspace,
                              size_t workspace_bytes, float *image, uint8_t *weight, void *label, int label_i32, int32_t *varied, float *field,
                              void *stream, int channels);

/* ------------------------------------------------------------------------------------------------------
 * Training-target generation.  Replaces my_transforms_direction.py:687-885 `LabelEncoding.__call__` (3-class-PNG input,
 * do_direction = 1) with get_centerpoint2 (:650-685), Sobel.kernel (SegFix_offset_helper.py:97-132) and
 * DTOffsetHelper.align_angle / angle_to_vector / vector_to_label (:311-341, 423-450, 486-506).
 *   label_ch0 u8 [N][H][W] (channel 0 of the label PNG; > 127 = inside)
 *   -> label3 u8 {0,127,255}, point f16 [N][H][W] (Gaussian sigma 2 of 255-impulses at the nucleus centres),
 *      direction u8 0..8 (centripetal class + 1, background 0); optional inst i32 (grown instance ids), counts i32 [N].
 * rays_host: 16 doubles {sin(2 pi k/8), cos(2 pi k/8)} k = 0..7 and gauss_host: 9 doubles (normalised half kernel,
 * centre first) are evaluated by the HOST math library so that they equal the reference's math.sin/cos and scipy weights.
 * max_instances: upper bound of nuclei per image (ids above it are dropped - check counts).
 * ---------------------------------------------------------------------------------------------------- */
size_t cdnet_label_encoding_workspace_bytes(int N, int H, int W, int max_instances);
int cdnet_label_encoding(const uint8_t *label_ch0, int N, int H, int W, int max_instances, const double *rays_host,
                         const double *gauss_host, void *workspace, size_t workspace_bytes, uint8_t *label3,
                         uint16_t *point_f16, uint8_t *direction, int32_t *inst_out, int32_t *counts_out, void *stream);
/* The instance-label input branch of the same transform (my_transforms_direction.py:752-760, `label_level_len > 2`; the
 * reference's default training data <label_dir>/train_ins): label_inst i32 [N][H][W] holds instance ids.  inside = id > 0 (dropped
 * when an image has fewer than 5 foreground pixels, :755), boundary = pixels whose 4-neighbourhood holds different ids (:759:
 * dilation(label) & ~erosion(label, disk(1)) on the integer ids), instances = dilation(postproc_other.process((new_label == 1) * 255,
 * 'modelName', min_size=5), disk(1)) - the watershed variant (cdnet_watershed_process) - then the same centre / direction / point
 * stage.  N <= 64.  Outputs as cdnet_label_encoding; counts = max_instances (watershed ids are not contiguous). */
size_t cdnet_label_encoding_instances_workspace_bytes(int N, int H, int W, int max_instances);
int cdnet_label_encoding_instances(const int32_t *label_inst, int N, int H, int W, int max_instances, const double *rays_host,
                                   const double *gauss_host, void *workspace, size_t workspace_bytes, uint8_t *label3,
                                   uint16_t *point_f16, uint8_t *direction, int32_t *inst, int32_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * HRNet fuse / residual sums.  Replaces the y = y + x[j] / y = y + F.interpolate(..., mode='bilinear') / relu(y) chains of
 * seg_hrnet_rev1.py:256-283, the residual adds of BasicBlock / Bottleneck (:76-92, :113-133) and the F.upsample + torch.cat
 * of the four branches (:528-533).  out[N][H][W] = [relu](sum of 1..4 terms), every term a bf16 NHWC tensor with C
 * channels (optionally with a per-channel affine), either [H][W] or a lower resolution that is up-sampled bilinearly
 * (align_corners = False).  The output may be a
 * channel slice [out_coff, out_coff + C) of pixels out_cstride wide (0 = C).  The 16-bit entry refuses N * H * W * C / 8 >= 2^31.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct cdnet_fuse_term {
    const uint16_t *x;      /* bf16 (or fp16 when f16 = 1) NHWC [N][Hs][Ws][C] */
    int Hs, Ws;
    const float *scale;     /* optional per-channel affine applied to the term (training mode: raw conv output x BatchNorm */
    const float *shift;     /* scale / shift), both NULL or both set */
    int f16, pad_;
} cdnet_fuse_term;
int cdnet_fuse_sum(const cdnet_fuse_term *terms, int nterm, int N, int H, int W, int C, int relu, uint16_t *out, int out_cstride,
                   int out_coff, void *stream);

/* backward pieces of the HRNet training step (loss.backward() through seg_hrnet_rev1.py:256-283, 436-443):
 * cdnet_upsample_bilinear_backward: transpose of the bilinear up-sampling done inside cdnet_fuse_sum: dout bf16 NHWC
 *   [N][H][W] (channel slice coff / cstride allowed) -> din bf16 [N][Hs][Ws][C], for any Hs <= H, Ws <= W (the ratio need not be an
 *   integer; (2 Hs + 1) H must fit 32 bits);
 * cdnet_s2d_to_nhwc: gradient computed in the space-to-depth view [N][H2][W2][(a, b, c)] -> [N][2*H2][2*W2][C]
 *   (input gradient of a stride-2 convolution; weight pack mode 7 = backward-data of mode 6). */
int cdnet_upsample_bilinear_backward(const uint16_t *dout, int N, int H, int W, int C, int dout_cstride, int dout_coff, int Hs, int Ws,
                                     uint16_t *din, void *stream);
int cdnet_s2d_to_nhwc(const uint16_t *in, int N, int H2, int W2, int C, uint16_t *out, void *stream);
/* the three entries above for fp32 tensors (fp32 precision mode: every term has f16 = 2; same arithmetic, nothing is rounded to 16 bits) */
int cdnet_fuse_sum_f32(const cdnet_fuse_term *terms, int nterm, int N, int H, int W, int C, int relu, float *out, int out_cstride,
                       int out_coff, void *stream);
int cdnet_upsample_bilinear_backward_f32(const float *dout, int N, int H, int W, int C, int dout_cstride, int dout_coff, int Hs, int Ws,
                                         float *din, void *stream);
int cdnet_s2d_to_nhwc_f32(const float *in, int N, int H2, int W2, int C, float *out, void *stream);

/* cdnet_grad_sum: backward of the sums above (autograd's AddBackward + ReluBackward over seg_hrnet_rev1.py:76-92, 256-283 and the
 * torch.cat of :533): out[npix][C] = [mask > 0] * sum of 1..6 gradient contributions, each a bf16 tensor [npix][cstride] read at
 * channel slice [coff, coff + C) (cstride 0 = C).  mask = the stored (post-ReLU) forward output, or NULL for a sum without ReLU. */
typedef struct cdnet_grad_term {
    const uint16_t *g;
    int cstride, coff;
} cdnet_grad_term;
int cdnet_grad_sum(const cdnet_grad_term *terms, int nterm, const uint16_t *mask, long long npix, int C, uint16_t *out, void *stream);
/* the same over fp32 tensors (fp32 precision mode: `g` of every term, mask and out point at float data; strides in elements) */
int cdnet_grad_sum_f32(const cdnet_grad_term *terms, int nterm, const float *mask, long long npix, int C, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Instance metrics (stats_utils.py): one pass over a ground-truth and a predicted label image [N][plane] i32 gives the
 * per-label areas (area_*[N][cap], ids must be < cap <= 65536) and a sparse table of pairwise intersections (open
 * addressing, hash_slots a power of two >= 2 x expected pairs: hash_keys[N][slots] = (true_id << 16) | pred_id, 0 = empty;
 * hash_counts = pixels).  get_fast_aji :7-106, get_fast_pq :182-276 and get_dice_1 :323-335 are finished on the host from
 * these (cdnet_amd/stats_utils.py).  err_flag (1 int): 1 = id out of range, 2 = table full.
 * cdnet_remap_label = remap_label :361-392 (by_size = False); scratch i32 [N][cap].
 * ---------------------------------------------------------------------------------------------------- */
int cdnet_label_pair_histogram(const int32_t *true_lab, const int32_t *pred_lab, int N, int plane, int cap, int hash_slots,
                               int32_t *area_true, int32_t *area_pred, uint32_t *hash_keys, int32_t *hash_counts, int32_t *err_flag,
                               void *stream);
int cdnet_remap_label(const int32_t *lab, int N, int plane, int cap, int32_t *scratch, int32_t *out, int32_t *err_flag, void *stream);
/* remap_label by_size = True in two halves: cdnet_label_areas counts the pixels of every id (area[N][cap]; err_flag 1 = id outside
 * [0, cap)), the host orders the ids, cdnet_label_apply writes out = lut[N][cap][lab] (ids outside (0, cap) -> 0). */
int cdnet_label_areas(const int32_t *lab, int N, int plane, int cap, int32_t *area, int32_t *err_flag, void *stream);
int cdnet_label_apply(const int32_t *lab, int N, int plane, int cap, const int32_t *lut, int32_t *out, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Object-level Hausdorff distances (utils.py:303: scipy's directed_hausdorff both ways between the pixel sets of a true and a predicted
 * object), exact: integer squared distances, minima and maxima only.
 *
 * cdnet_label_csr, once per label image [H][W] i32 (H, W <= 32767, ids < cap <= 65536): tab[4][cap] = pixels per id, boundary pixels per
 * id, start of the id's segment in pix, start of its segment in bpix; pix[H * W] = the coordinates (y << 16 | x) of all labelled pixels
 * grouped by id, bpix[H * W] = the same for boundary pixels only (on the image edge, or a 4-neighbour carries another id).  The order
 * inside a segment is arbitrary.  workspace: cdnet_label_csr_workspace_bytes(cap).  err_flag 1 = id outside [0, cap).  Four launches.
 *
 * cdnet_hausdorff_pairs, one launch for all pairs: pairs[M][2] = (true id, pred id); items[n_items][2] = (2 * pair + direction, tile),
 * one per cdnet_hausdorff_tile_pixels() pixels of the direction's source object A (direction 0: A = the predicted object, 1: the true
 * one), written by the caller from tab's counts - so the caller also decides which pairs run here.  d2[M][2] = (h(P -> T)^2,
 * h(T -> P)^2), h(A -> B) = max over a in A of min over b in B of |a - b|; pairs without items keep 0.  Objects may be of any size: a
 * block holds one tile of A in registers and streams B's boundary through LDS cdnet_hausdorff_chunk_pixels() at a time.  The work is
 * about |A \ B| x |boundary of B| distance evaluations per item set, which the caller should bound.  err_flag: 1 = pair id outside
 * (0, cap), 3 = an item out of range or an id without pixels.
 * ---------------------------------------------------------------------------------------------------- */
size_t cdnet_label_csr_workspace_bytes(int cap);
int cdnet_label_csr(const int32_t *lab, int H, int W, int cap, void *workspace, size_t workspace_bytes, int32_t *tab, int32_t *pix,
                    int32_t *bpix, int32_t *err_flag, void *stream);
int cdnet_hausdorff_tile_pixels(void);
int cdnet_hausdorff_chunk_pixels(void);
int cdnet_hausdorff_pairs(const int32_t *true_lab, const int32_t *true_tab, const int32_t *true_pix, const int32_t *true_bpix,
                          const int32_t *pred_lab, const int32_t *pred_tab, const int32_t *pred_pix, const int32_t *pred_bpix, int H, int W,
                          int cap, const int32_t *pairs, int M, const int32_t *items, int n_items, int32_t *d2, int32_t *err_flag,
                          void *stream);

/* ------------------------------------------------------------------------------------------------------
 * Border weight maps from instance labels: the `<stem>_weight.png` of every training sample, which the losses read as png / 20
 * (train_util_dam.py:102,171,230,242).  The reference has no generator for them; the map is U-Net's,
 *   w = 1 + w0 * exp(-(d1 + d2)^2 / (2 sigma^2)) on background pixels, 1 on the pixels of an instance,  weight u8 = floor(20 * w),
 * d1 <= d2 the Euclidean distances (pixel centres) to the nearest and the second-nearest distinct instance; a pixel without two
 * instances in reach gets 20.
 *
 * cdnet_weight_map_radius: R = ceil(sigma * sqrt(2 ln(20 w0))), the distance beyond which no instance changes a stored byte (17 for the
 *   defaults w0 = 10, sigma = 5); 0 when w0 <= 0, sigma <= 0 or 20 * (1 + w0) > 255.
 * cdnet_weight_map: instances i32 [H][W] (ids <= 0 are background, positive ids arbitrary) -> weight u8 [H][W], any H, W >= 1, one launch.
 *   Refused before any HIP call: a null pointer, w0 <= 0, sigma <= 0, 20 * (1 + w0) > 255 (the byte would wrap) and R > 64 (the LDS
 *   window of a 32 x 32 tile, (32 + 2 R)^2 * 4 B, must fit the CU's 160 KB).
 * ---------------------------------------------------------------------------------------------------- */
int cdnet_weight_map_radius(double w0, double sigma);
int cdnet_weight_map(const int32_t *instances, int H, int W, double w0, double sigma, uint8_t *weight, void *stream);

/* ------------------------------------------------------------------------------------------------------
 * The 'scale' test transform on the device (resize.hip): Pillow's 8-bit bilinear resampler, bit for bit.  Replaces
 *   my_transforms_direction.py:38-65 (Scale: img.resize((ow, oh), Image.BILINEAR) before the network, through test_dam.py:297 /
 *   test.py:213) and test_dam.py:551-553 / test.py:281-283 (misc.imresize(pred2 * 255, (ori_h, ori_w), 'bilinear') > 127.5: the mask back).
 *
 * cdnet_resize_bilinear: src u8 [N][H][W][C] -> out u8 [N][oh][ow][C]; C = 1 (mode L) or 3 (mode RGB, interleaved as np.asarray gives
 *   it); any H, W, oh, ow >= 1 (at most 2^20), N <= 65535.  Pointers and rows need byte alignment only.
 *   Tables (device memory, made by cdnet_amd/resize.py resize_tables in float64 in Pillow's operation order; the device computes no
 *   coefficient): per axis bounds i32 [out][2] = (first source index, taps) and kk i32 [out][ksize], 22-bit fixed point, with
 *   ksize = 2 * ceil(max(in / out, 1)) + 1.  An axis whose size does not change takes no tables (NULL, ksize ignored) and runs no pass.
 *   A pass is clip8((2^21 + sum src * kk) >> 22) in int32; the horizontal pass runs first and is rounded to u8 before the vertical one.
 *   mask_mode 1 (C = 1): src is {0, 1} and read as v * 255, out is (resized > 127.5) as {0, 1} - test_dam.py:552-553 in one call.
 *   form: 0 = choose, 1 = LDS form (one launch: a workgroup runs the horizontal pass of the source rows of its 16 x 64 output tile into
 *   LDS and the vertical pass from there; CDNET_E_ARG when those rows exceed 64 KB of LDS or when one axis alone changes), 2 = two-pass
 *   form (the horizontal result goes through `workspace`; one launch and no workspace when one axis alone changes).  Equal sizes: a copy.
 *   workspace: cdnet_resize_workspace_bytes(..., form) bytes (0: may be NULL).
 * cdnet_resize_last_form: what the calling thread's last successful cdnet_resize_bilinear ran: 0 copy, 1 LDS form, 2 two-pass form.
 * cdnet_label8_dilate: skimage.measure.label (8-connected, ids in raster order) of mask u8 [N][H][W] (non-zero = foreground), then
 *   dilation(disk(radius)) - test_dam.py:561-563 / test.py:292-295: the last two stages of cdnet_cc_chain WITHOUT hole filling and
 *   small-object removal, which the reference does not repeat after the resize.  label i32 (may be NULL), final i32, counts i32 [N]
 *   (the number of components); workspace: cdnet_cc_workspace_bytes(N, H, W).
 * cdnet_fill_remove_small: binary_fill_holes then remove_small_objects(min_area) of (pred == fg_value), pred u8 [N][H][W] -> small u8 {0, 1}
 *   (test_dam.py:546-548, test.py:277-279): the first two stages of cdnet_cc_chain alone, its `small` output bit for bit, without the
 *   chain's numbering, relabel and dilation - the mask the 'scale' transform resizes back.  workspace: cdnet_cc_workspace_bytes(N, H, W).
 * Every entry checks its arguments and returns before any HIP call.
 * ---------------------------------------------------------------------------------------------------- */
size_t cdnet_resize_workspace_bytes(int N, int H, int W, int C, int oh, int ow, int form);
int cdnet_resize_bilinear(const uint8_t *src, int N, int H, int W, int C, int oh, int ow, const int32_t *hbounds, const int32_t *hkk,
                          int hksize, const int32_t *vbounds, const int32_t *vkk, int vksize, int mask_mode, int form, void *workspace,
                          size_t workspace_bytes, uint8_t *out, void *stream);
int cdnet_resize_last_form(void);
int cdnet_fill_remove_small(const uint8_t *pred, int fg_value, int N, int H, int W, int min_area, void *workspace, size_t workspace_bytes,
                            uint8_t *small, void *stream);
int cdnet_label8_dilate(const uint8_t *mask, int N, int H, int W, int radius, void *workspace, size_t workspace_bytes, int32_t *label,
                        int32_t *final_, int32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CDNET_HIP_H */
