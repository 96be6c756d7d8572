"""ctypes binding of libcdnet_hip.so (the C ABI of include/cdnet_hip.h).

There is NO fallback: if the library is missing or a symbol is absent the import of the compute path fails
loudly.  PyTorch is used by the callers only for device memory and streams; nothing torch-typed crosses the ABI.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CDNET_LIB_PATH') or os.path.join(_HERE, 'libcdnet_hip.so')      # (the override: A/B builds of tools/build_variant.sh)

_vp, _i, _sz, _f, _u = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_uint


# ctypes mirrors of the argument structs of include/cdnet_hip.h: every one is defined here, once (MIRRORS below names them for tests/test_abi.py)
class ConvSrc(C.Structure):                  # cdnet_conv_src
    _fields_ = [('x', C.c_void_p), ('res', C.c_void_p), ('scale', C.c_void_p), ('shift', C.c_void_p),
                ('C', C.c_int), ('Hs', C.c_int), ('Ws', C.c_int), ('pool', C.c_int), ('relu', C.c_int),
                ('off_y', C.c_int), ('off_x', C.c_int), ('f16', C.c_int), ('row_stride', C.c_int)]


class ConvArgs(C.Structure):                 # cdnet_conv_args
    _fields_ = [('src', ConvSrc * 2), ('nsrc', C.c_int), ('w', C.c_void_p), ('bias', C.c_void_p),
                ('oscale', C.c_void_p), ('oshift', C.c_void_p), ('orelu', C.c_int), ('out', C.c_void_p),
                ('Cout', C.c_int), ('out_cstride', C.c_int), ('out_coff', C.c_int), ('stats', C.c_void_p),
                ('N', C.c_int), ('H', C.c_int), ('W', C.c_int), ('taps', C.c_int), ('npar', C.c_int),
                ('ostride', C.c_int), ('nchunk', C.c_int), ('tile', C.c_int), ('CK', C.c_int), ('BN', C.c_int),
                ('out_f16', C.c_int), ('debug', C.c_int), ('ws', C.c_int), ('f32', C.c_int),
                ('eres', C.c_void_p), ('eres_scale', C.c_void_p), ('eres_shift', C.c_void_p), ('eres_f16', C.c_int), ('eres_relu', C.c_int),
                ('taps1', C.c_int), ('pad_', C.c_int), ('pool_out', C.c_void_p),
                ('dot_w', C.c_void_p), ('dot_b', C.c_void_p), ('dot_out', C.c_void_p)]


class PackJob(C.Structure):                  # cdnet_pack_job
    _fields_ = [('w', C.c_void_p), ('packed', C.c_void_p), ('Cout', C.c_int), ('Cin', C.c_int), ('KH', C.c_int), ('KW', C.c_int),
                ('CK', C.c_int), ('BN', C.c_int), ('mode', C.c_int), ('pad_', C.c_int)]


class HeadFeat(C.Structure):                 # cdnet_head_feat
    _fields_ = [('raw', C.c_void_p), ('res', C.c_void_p), ('scale', C.c_void_p), ('shift', C.c_void_p),
                ('relu', C.c_int), ('f16', C.c_int)]


class FuseTerm(C.Structure):                 # cdnet_fuse_term
    _fields_ = [('x', C.c_void_p), ('Hs', C.c_int), ('Ws', C.c_int), ('scale', C.c_void_p), ('shift', C.c_void_p),
                ('f16', C.c_int), ('pad_', C.c_int)]


class GradTerm(C.Structure):                 # cdnet_grad_term
    _fields_ = [('g', C.c_void_p), ('cstride', C.c_int), ('coff', C.c_int)]


class GradIn(C.Structure):                   # cdnet_grad_in
    _fields_ = [('g', C.c_void_p), ('Hg', C.c_int), ('Wg', C.c_int), ('oy', C.c_int), ('ox', C.c_int),
                ('pooled', C.c_int), ('coff', C.c_int), ('cstride', C.c_int), ('pad_', C.c_int)]


class BnBwdArgs(C.Structure):                # cdnet_bn_bwd_args
    _fields_ = [('raw', C.c_void_p), ('res', C.c_void_p), ('scale', C.c_void_p), ('shift', C.c_void_p),
                ('mean', C.c_void_p), ('invstd', C.c_void_p), ('gin', GradIn * 3), ('ngin', C.c_int),
                ('f16', C.c_int), ('relu', C.c_int), ('N', C.c_int), ('H', C.c_int), ('W', C.c_int), ('C', C.c_int),
                ('hc_coef', C.c_void_p), ('hc_w', C.c_void_p), ('hc_slot', C.c_int), ('hc_k0', C.c_int), ('hc_nk', C.c_int),
                ('hc_pad_', C.c_int)]


class AugSample(C.Structure):                # cdnet_aug_sample
    _fields_ = [('minv', C.c_double * 6), ('img', C.c_void_p), ('weight', C.c_void_p), ('label', C.c_void_p)] + \
        [(n, C.c_int32) for n in ('H', 'W', 'img_stride', 'weight_stride', 'label_stride', 'label_i32')] + \
        [('color', C.c_float * 4)] + [(n, C.c_int32) for n in ('hflip', 'vflip', 'filter', 'y0', 'x0')] + \
        [('alpha', C.c_float), ('sigma', C.c_float), ('seed', C.c_uint32)]


class AugGeo(C.Structure):                   # cdnet_aug_geo
    _fields_ = [('paff', C.c_double * 6), ('rinv', C.c_double * 6)] + [(n, C.c_int32) for n in ('Hr', 'Wr', 'fy0', 'fx0')] + \
        [('flags', C.c_uint32), ('reserved', C.c_int32)]


class WgradReduceDesc(C.Structure):          # cdnet_wgrad_reduce_desc (include/cdnet_hip.h)
    _fields_ = [('slab', C.c_void_p), ('dw', C.c_void_p)] + [(n, C.c_int) for n in (
        'ksplit', 'npar', 'ci_blocks', 'co_blocks', 'taps', 'CI', 'CO', 'Csrc_real', 'Cin_real', 'src_coff', 'Cout', 'mode', 'block0', 'blocks')]

class DilatedConvArgs(C.Structure):          # cdnet_dilated_conv_args
    _fields_ = [(n, C.c_void_p) for n in ('in_', 'w', 'scale', 'shift', 'out')] + [(n, C.c_int) for n in (
        'N', 'H', 'W', 'Cin', 'in_cstride', 'Cout', 'out_cstride', 'out_coff', 'taps', 'dilation', 'leaky')] + [
        ('slope', C.c_float), ('f32', C.c_int), ('out_nchw', C.c_int)]

class DilatedBwdDataArgs(C.Structure):       # cdnet_dilated_bwd_data_args
    _fields_ = [(n, C.c_void_p) for n in ('g', 'w', 'dx')] + [(n, C.c_int) for n in (
        'N', 'H', 'W', 'Cout', 'g_cstride', 'Cin', 'dx_cstride', 'dx_coff', 'taps', 'dilation', 'accumulate', 'f32')]

class DilatedWgradArgs(C.Structure):         # cdnet_dilated_wgrad_args
    _fields_ = [(n, C.c_void_p) for n in ('x', 'g', 'dw', 'ws')] + [('ws_bytes', C.c_size_t)] + [(n, C.c_int) for n in (
        'N', 'H', 'W', 'Cin', 'x_cstride', 'Cout', 'g_cstride', 'taps', 'dilation')]

class SliceBnFwdArgs(C.Structure):           # cdnet_slice_bn_fwd_args
    _fields_ = [(n, C.c_void_p) for n in ('z', 'out', 'gamma', 'beta', 'running_mean', 'running_var', 'mean', 'invstd', 'ws')] + [
        ('ws_floats', C.c_size_t), ('P', C.c_longlong)] + [(n, C.c_int) for n in ('C', 'z_cstride', 'out_cstride', 'out_coff')] + [
        (n, C.c_float) for n in ('eps', 'momentum', 'p_drop')] + [('layer', C.c_int), ('key', C.c_ulonglong)]

class SliceBnBwdArgs(C.Structure):           # cdnet_slice_bn_bwd_args
    _fields_ = [(n, C.c_void_p) for n in ('dy', 'z', 'mean', 'invstd', 'gamma', 'dgamma', 'dbeta', 'g', 'ws')] + [
        ('ws_floats', C.c_size_t), ('P', C.c_longlong)] + [(n, C.c_int) for n in ('C', 'z_cstride', 'dy_cstride', 'dy_coff', 'g_cstride')] + [
        (n, C.c_float) for n in ('slope', 'p_drop')] + [('layer', C.c_int), ('key', C.c_ulonglong)]


# struct name of include/cdnet_hip.h -> its mirror; must list every name cdnet_abi_sizeof knows (tests/test_abi.py checks)
MIRRORS = {
    'cdnet_conv_src': ConvSrc, 'cdnet_conv_args': ConvArgs, 'cdnet_pack_job': PackJob, 'cdnet_head_feat': HeadFeat,
    'cdnet_wgrad_reduce_desc': WgradReduceDesc, 'cdnet_grad_in': GradIn, 'cdnet_bn_bwd_args': BnBwdArgs, 'cdnet_fuse_term': FuseTerm,
    'cdnet_grad_term': GradTerm, 'cdnet_aug_sample': AugSample, 'cdnet_aug_geo': AugGeo, 'cdnet_dilated_conv_args': DilatedConvArgs,
    'cdnet_dilated_bwd_data_args': DilatedBwdDataArgs, 'cdnet_dilated_wgrad_args': DilatedWgradArgs,
    'cdnet_slice_bn_fwd_args': SliceBnFwdArgs, 'cdnet_slice_bn_bwd_args': SliceBnBwdArgs,
}

# name -> (restype, argtypes); must list every symbol include/cdnet_hip.h declares (tests/test_abi.py checks)
SIGNATURES = {
    'cdnet_abi_version': (_i, []),
    'cdnet_abi_sizeof': (_sz, [C.c_char_p]),
    'cdnet_last_error': (C.c_char_p, []),
    'cdnet_build_info': (C.c_char_p, []),
    'cdnet_spin': (_i, [_i, _vp]),
    'cdnet_box_copy': (_i, [_vp, _vp, _sz, _vp]),
    'cdnet_box_mfma': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    'cdnet_ddm_codes': (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp]),
    'cdnet_ddm_normalize': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    'cdnet_probmaps': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    'cdnet_tta_boost_argmax': (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'cdnet_fuse_sum': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    'cdnet_upsample_bilinear_backward': (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'cdnet_s2d_to_nhwc': (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    'cdnet_fuse_sum_f32': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    'cdnet_upsample_bilinear_backward_f32': (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    'cdnet_s2d_to_nhwc_f32': (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    'cdnet_bn_backward_stats': (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    'cdnet_bn_backward_apply': (_i, [_vp, _vp, _vp, _vp]),
    'cdnet_bn_backward_finalize': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    'cdnet_conv_ws_eligible': (_i, [_vp]),
    'cdnet_grad_sum': (_i, [_vp, _i, _vp, C.c_longlong, _i, _vp, _vp]),
    'cdnet_grad_sum_f32': (_i, [_vp, _i, _vp, C.c_longlong, _i, _vp, _vp]),
    'cdnet_label_pair_histogram': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'cdnet_remap_label': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    'cdnet_label_areas': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    'cdnet_label_apply': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    'cdnet_label_csr_workspace_bytes': (_sz, [_i]),
    'cdnet_label_csr': (_i, [_vp, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    'cdnet_hausdorff_tile_pixels': (_i, []),
    'cdnet_hausdorff_chunk_pixels': (_i, []),
    'cdnet_hausdorff_pairs': (_i, [_vp] * 8 + [_i, _i, _i, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    'cdnet_watershed_workspace_bytes': (_sz, [_i, _i, _i]),
    'cdnet_watershed_process': (_i, [_vp, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp]),
    'cdnet_fill_label_process': (_i, [_vp, _i, _i, _i, _i, _vp, _sz, _vp, _vp]),
    'cdnet_label_process': (_i, [_vp, _i, _i, _i, _i, _vp, _sz, _vp, _vp]),
    'cdnet_instance_redilate_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'cdnet_instance_redilate': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp]),
    'cdnet_instance_redilate_lds_rows': (_i, []),
    'cdnet_instance_redilate_lds_cols': (_i, []),
    'cdnet_label_count': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    'cdnet_tile_postproc_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'cdnet_tile_postproc': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, _sz] + [_vp] * 10),
    'cdnet_cc_workspace_bytes': (_sz, [_i, _i, _i]),
    'cdnet_cc_chain': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    'cdnet_mask_views_argmax': (_i, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp]),
    'cdnet_tile_mask_postproc_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'cdnet_tile_mask_postproc': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _sz] + [_vp] * 8),
    'cdnet_dilate_labels': (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    'cdnet_conv_packed_weight_elems': (_sz, [_i] * 6),
    'cdnet_pack_conv_weights': (_i, [_vp, _vp] + [_i] * 7 + [_vp]),
    'cdnet_pack_conv_weights_scaled': (_i, [_vp, _vp, _vp] + [_i] * 7 + [_vp]),
    'cdnet_pack_batch_table_bytes': (_sz, [_i]),
    'cdnet_pack_conv_weights_batch': (_i, [_vp, _i, _vp, _sz, _i, _vp]),
    'cdnet_conv_forward': (_i, [_vp, _vp]),
    'cdnet_dilated_packed_weight_elems': (_sz, [_i, _i, _i, _i]),
    'cdnet_dilated_pack_weights': (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    'cdnet_dilated_conv_forward': (_i, [_vp, _vp]),
    'cdnet_dilated_pack_weights_bwd': (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    'cdnet_dilated_conv_backward_data': (_i, [_vp, _vp]),
    'cdnet_dilated_wgrad_workspace_bytes': (_sz, [_i] * 6),
    'cdnet_dilated_conv_backward_weight': (_i, [_vp, _vp]),
    'cdnet_slice_bn_workspace_floats': (_sz, [C.c_longlong, _i]),
    'cdnet_slice_bn_train_forward': (_i, [_vp, _vp]),
    'cdnet_slice_bn_train_backward': (_i, [_vp, _vp]),
    'cdnet_dropout_mask': (_i, [C.c_ulonglong, _i, _sz, _f, _vp, _vp]),
    'cdnet_maxpool2_forward': (_i, [_vp, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'cdnet_maxpool2_backward': (_i, [_vp, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    'cdnet_upsample4_bilinear_forward': (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'cdnet_upsample4_bilinear_backward': (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    'cdnet_src_materialize': (_i, [_vp, _i, _i, _i, _vp, _vp]),
    'cdnet_input_pack': (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    'cdnet_input_pack_f32': (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    'cdnet_bn_fold_eval': (_i, [_vp, _vp, _vp, _vp, _vp, _f, _i, _vp, _vp, _vp]),
    'cdnet_bn_finalize_train': (_i, [_vp, _i, _i, _f, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'cdnet_dam_head_forward': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    'cdnet_final_conv1x1': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    'cdnet_bias_grad_workspace_floats': (_sz, [_i]),
    'cdnet_bias_grad': (_i, [_vp, _sz, _i, _vp, _sz, _vp, _vp]),
    'cdnet_bias_grad_f32': (_i, [_vp, _sz, _i, _vp, _sz, _vp, _vp]),
    'cdnet_final_conv1x1_backward_workspace_floats': (_sz, []),
    'cdnet_final_conv1x1_backward': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp]),
    'cdnet_final_conv1x1_c16': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    'cdnet_final_conv1x1_c16_backward_workspace_floats': (_sz, []),
    'cdnet_final_conv1x1_c16_backward': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp]),
    'cdnet_conv_wgrad_slab_floats': (_sz, [_i] * 6),
    'cdnet_conv_backward_weight': (_i, [_vp, _i, _i, _i, _vp] + [_i] * 9 + [_vp, _vp, _i, _vp]),
    'cdnet_conv_backward_weight_last_form': (_i, []),
    'cdnet_conv_forward_last_form': (_i, []),
    'cdnet_wgrad_reduce_desc_fill': (_i, [_i] * 9 + [_vp, _vp, _i, _i, _vp]),
    'cdnet_wgrad_reduce_batch': (_i, [_vp, _i, _i, _vp]),
    'cdnet_bn_backward_workspace_floats': (_sz, [_i]),
    'cdnet_bn_backward': (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    'cdnet_bn_backward_last_plan': (_i, []),
    'cdnet_bn_backward_last_sums_plan': (_i, []),
    'cdnet_dam_head_backward_workspace_floats': (_sz, [_i, _i, _i]),
    'cdnet_dam_head_backward': (_i, [_vp] * 7 + [_i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    'cdnet_dam_head_backward_fused_blocks': (_i, []),
    'cdnet_dam_head_backward_fused_scratch_bytes': (_i, []),
    'cdnet_dam_head_backward_fused_workspace_floats': (_sz, []),
    'cdnet_dam_head_backward_fused': (_i, [_vp] * 7 + [_i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    'cdnet_dam_head_backward_coef_scratch_bytes': (_i, []),
    'cdnet_dam_head_backward_coef': (_i, [_vp] * 7 + [_i, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp]),
    'cdnet_dam_loss_workspace_floats': (_sz, [_i, _i]),
    'cdnet_dam_loss': (_i, [_vp] * 7 + [_i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    'cdnet_dam_loss_classes_workspace_floats': (_sz, [_i, _i, _i]),
    'cdnet_dam_loss_classes': (_i, [_vp] * 7 + [_i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    'cdnet_dam_loss_terms': (_i, [_vp] * 7 + [_i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _u]),
    'cdnet_mask_loss_workspace_floats': (_sz, [_i, _i]),
    'cdnet_mask_loss': (_i, [_vp, _vp, _vp, _i, _i, _i, _u, _vp, _sz, _vp, _vp, _vp]),
    'cdnet_variance_loss_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'cdnet_variance_loss': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    'cdnet_boundary_loss_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'cdnet_boundary_loss': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _sz, _vp, _vp, _vp, _vp]),
    'cdnet_boundary_loss_scratch_bytes': (_i, []),
    'cdnet_dam_val_sums_workspace_floats': (_sz, [_i, _i]),
    'cdnet_dam_val_sums': (_i, [_vp] * 8 + [_i, _i, _i, _vp, _sz, _vp, _vp]),
    'cdnet_dam_val_sums_classes_workspace_floats': (_sz, [_i, _i, _i]),
    'cdnet_dam_val_sums_classes': (_i, [_vp] * 8 + [_i, _i, _i, _i, _vp, _sz, _vp, _vp]),
    'cdnet_adam_step': (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _i, _f, _vp]),
    'cdnet_moment_step': (_i, [_vp, _vp, _vp, _vp, _vp, _sz, C.c_double, C.c_double, _f, _i, _i, _f, _f, _f, _f, _i, _f, _vp]),
    'cdnet_sgd_step': (_i, [_vp, _vp, _vp, _sz, _f, _f, _f, _i, _f, _vp]),
    'cdnet_window_pack': (_i, [_vp] + [_i] * 9 + [_vp, _vp]),
    'cdnet_window_pack_f32': (_i, [_vp] + [_i] * 9 + [_vp, _vp]),
    'cdnet_window_stitch': (_i, [_vp] + [_i] * 9 + [_vp, _vp]),
    'cdnet_label_encoding_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'cdnet_label_encoding_instances_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'cdnet_label_encoding_instances': (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    'cdnet_augment_workspace_bytes': (_sz, [_i, _i, _i]),
    'cdnet_augment_batch': (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    'cdnet_augment_geo_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'cdnet_augment_batch_geo': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    'cdnet_augment_batch_c': (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i]),
    'cdnet_augment_batch_geo_c': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i]),
    'cdnet_label_encoding': (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    'cdnet_weight_map_radius': (_i, [C.c_double, C.c_double]),
    'cdnet_weight_map': (_i, [_vp, _i, _i, C.c_double, C.c_double, _vp, _vp]),
    'cdnet_resize_workspace_bytes': (_sz, [_i] * 7),
    'cdnet_resize_bilinear': (_i, [_vp] + [_i] * 6 + [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    'cdnet_resize_last_form': (_i, []),
    'cdnet_fill_remove_small': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _vp]),
    'cdnet_label8_dilate': (_i, [_vp, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _vp, _vp]),
}

_lib = None


class CdnetHipError(RuntimeError):
    pass


def load():
    """Load the library once; raise if it is not built (python -m cdnet_amd.csrc.build)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7, the same
    # as /opt/rocm's).  Importing torch FIRST makes the dynamic loader satisfy our NEEDED libamdhip64.so.7 with
    # the copy torch already mapped, so torch's streams / allocations and our launches share one runtime.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise CdnetHipError('libcdnet_hip.so is not built: run `python -m cdnet_amd.csrc.build` '
                            '(or __graft_entry__.build()). There is no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.cdnet_abi_version() != 5:
        raise CdnetHipError('ABI version mismatch (libcdnet_hip.so is version %d, this binding 5): rebuild with python -m cdnet_amd.csrc.build' % lib.cdnet_abi_version())
    _lib = lib
    return lib


def check(status, what=''):
    if status != 0:
        msg = load().cdnet_last_error().decode(errors='replace')
        raise CdnetHipError('%s failed (code %d): %s' % (what, status, msg))


def call(name, *args):
    check(getattr(load(), name)(*args), name)


def entry(name, f32):
    """the fp32 twin `<name>_f32` of an entry point that exists once per activation type, or `name` itself (the 16-bit one)"""
    return name + '_f32' if f32 else name


_RAW_STREAM = None


def stream_ptr():
    """The current PyTorch HIP stream as a void* for the ABI (the raw-handle query: torch.cuda.current_stream() builds a Stream object
    through several Python layers, ~4 us - on every one of the ~250 launches of a training step)."""
    global _RAW_STREAM
    if _RAW_STREAM is None:
        import torch
        get, dev = getattr(torch._C, '_cuda_getCurrentRawStream', None), getattr(torch._C, '_cuda_getDevice', None)
        if get is not None and dev is not None:
            _RAW_STREAM = lambda: get(dev())
        else:
            _RAW_STREAM = lambda: torch.cuda.current_stream().cuda_stream
    return C.c_void_p(_RAW_STREAM())


def ptr(t):
    """Device pointer of a contiguous torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), 'ABI needs contiguous device tensors'
    return C.c_void_p(t.data_ptr())
