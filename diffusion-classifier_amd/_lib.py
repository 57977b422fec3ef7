"""ctypes binding of libdcamd.so (C-ABI declared in include/dcamd.h).

The product path has NO fallback: if the HIP library is missing or does not load, every
entry point raises.  Nothing here imports `oracle/`.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DCAMD_LIB") or os.path.join(_HERE, "libdcamd.so")   # DCAMD_LIB: diagnostic builds only

ABI_VERSION = 5      # include/dcamd.h DC_ABI_VERSION
DC_F32, DC_BF16, DC_F16 = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_GELU_TANH = 0, 1, 2, 3
OP_QSAMPLE, OP_SINUSOID, OP_IGEMM, OP_GROUPNORM, OP_LAYERNORM, OP_ATTENTION, OP_EPS_MSE, OP_TBLOCK_FRONT = 1, 2, 3, 4, 5, 6, 7, 8
OP_CROSS_ATTENTION = 9
OP_CROSS_ATTENTION_LEN = 10
OP_ATTENTION_BIAS, OP_RMSNORM, OP_EMBED_ROWS, OP_RELU = 11, 12, 13, 14
ATTENTION_BIAS_MAX_L = 512      # include/dcamd.h DC_ATTENTION_BIAS_MAX_L
OP_ATTENTION_CAUSAL, OP_LAYERNORM_ROWS, OP_EMBED_ROWS_POS, OP_ACT_PASS = 15, 16, 17, 18
ATTENTION_CAUSAL_MAX_L = 512    # include/dcamd.h DC_ATTENTION_CAUSAL_MAX_L
PASS_QUICK_GELU, PASS_GELU_ERF = 1, 2       # dc_pass_kind
OP_ERR_MAP = 19
EVIDENCE_FRAC_BITS, EVIDENCE_VMAX = 30, 16384.0      # include/dcamd.h DC_EVIDENCE_FRAC_BITS / DC_EVIDENCE_VMAX
OP_ATTENTION_WIDE, OP_IM2COL_S2 = 20, 21
ATTENTION_WIDE_DIMS = (256, 512)     # head widths of dc_attention_wide
OP_CONV3_PN_TAIL = 22
OP_LATENT_IM2COL = 23

i32, i64, u64, f32, vp = C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_void_p


class QsampleParams(C.Structure):
    _fields_ = [("x", vp), ("eps", vp), ("alpha", vp), ("sigma", vp), ("img_of_bj", vp),
                ("out", vp), ("out_dtype", i32),
                ("n_bj", i32), ("C", i32), ("H", i32), ("W", i32), ("ld", i32), ("im2col", i32), ("patch", i32)]


class SinusoidParams(C.Structure):
    _fields_ = [("lam", vp), ("out", vp), ("n", i32), ("dim", i32), ("flip_sin_to_cos", i32), ("freq_shift", f32)]


class IgemmParams(C.Structure):
    _fields_ = [("dtype", i32), ("taps", i32), ("stride", i32), ("upsample", i32),
                ("n_img", i32), ("Hin", i32), ("Win", i32), ("Hout", i32), ("Wout", i32),
                ("src0", vp), ("map0", vp), ("C0", i32), ("ld0", i32),
                ("src1", vp), ("map1", vp), ("C1", i32), ("ld1", i32),
                ("W", vp), ("Cout", i32), ("tile_n", i32),
                ("bias", vp),
                ("rowvec", vp), ("rowvec_map", vp), ("rowvec_ld", i32), ("act", i32),
                ("gate", vp), ("gate_map", vp), ("gate_ld", i32), ("pad2_", i32),
                ("residual", vp), ("res_map", vp), ("res_dtype", i32), ("res_ld", i32),
                ("out", vp), ("out_dtype", i32), ("out_ld", i32),
                ("gn_scale", vp), ("gn_shift", vp), ("gn_silu", i32), ("pad3_", i32),
                ("src2", vp), ("map2", vp), ("W2", vp), ("C2", i32), ("ld2", i32),
                ("ln_eps", f32), ("up4", i32), ("qstats", vp),
                ("pn_out", vp), ("pn_gamma", vp), ("pn_beta", vp), ("pn_cnt", vp),
                ("pn_ld", i32), ("pn_groups", i32), ("pn_silu", i32), ("pn_eps", f32)]


class PnTailParams(C.Structure):
    _fields_ = [("Wt", vp), ("bias", vp), ("pred", vp), ("ring", vp), ("gamma", vp), ("beta", vp), ("cnt", vp),
                ("Co", i32), ("pred_ld", i32), ("groups", i32), ("silu", i32), ("eps", f32), ("pad_", i32)]


class Conv3PnTailOp(C.Structure):
    _fields_ = [("conv", C.POINTER(IgemmParams)), ("tail", C.POINTER(PnTailParams))]


class GroupnormParams(C.Structure):
    _fields_ = [("x", vp), ("map0", vp), ("x1", vp), ("map1", vp),
                ("y", vp), ("dtype", i32), ("out_dtype", i32),
                ("n", i32), ("HW", i32), ("C", i32), ("C1", i32), ("groups", i32), ("silu", i32),
                ("splits", i32), ("eps", f32),
                ("gamma", vp), ("beta", vp), ("ws", vp), ("out_scale", vp), ("out_shift", vp),
                ("qstats", vp), ("qparts", i32), ("pad_", i32)]


class LayernormParams(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("dtype", i32), ("out_dtype", i32),
                ("rows", i32), ("C", i32), ("rows_per_sample", i32), ("mod_ld", i32), ("eps", f32),
                ("gamma", vp), ("beta", vp), ("scale", vp), ("shift", vp), ("mod_map", vp)]


class AttentionParams(C.Structure):
    _fields_ = [("q", vp), ("k", vp), ("v", vp), ("out", vp),
                ("dtype", i32), ("n", i32), ("L", i32), ("heads", i32), ("d", i32),
                ("ld_qkv", i32), ("ld_out", i32), ("scale", f32)]


class AttentionWideParams(C.Structure):
    _fields_ = AttentionParams._fields_


class Im2colS2Params(C.Structure):
    _fields_ = [("x", vp), ("out", vp), ("dtype", i32), ("n", i32), ("H", i32), ("W", i32), ("C", i32), ("ld", i32)]


class LatentIm2colParams(C.Structure):
    _fields_ = [("z", vp), ("Q", vp), ("bias", vp), ("out", vp),
                ("out_dtype", i32), ("n", i32), ("Z", i32), ("H", i32), ("W", i32), ("Kpad", i32), ("inv_scale", f32), ("shift", f32)]


class CrossAttentionParams(C.Structure):
    _fields_ = [("q", vp), ("k", vp), ("v", vp), ("out", vp), ("q_map", vp), ("kv_map", vp),
                ("dtype", i32), ("n", i32), ("Lq", i32), ("S", i32), ("heads", i32), ("d", i32),
                ("ld_q", i32), ("ld_kv", i32), ("ld_out", i32), ("scale", f32)]


class CrossAttentionLenParams(C.Structure):
    _fields_ = [("q", vp), ("k", vp), ("v", vp), ("out", vp), ("q_map", vp), ("kv_map", vp), ("kv_len", vp),
                ("dtype", i32), ("n", i32), ("Lq", i32), ("S", i32), ("heads", i32), ("d", i32),
                ("ld_q", i32), ("ld_kv", i32), ("ld_out", i32), ("scale", f32)]


class AttentionBiasParams(C.Structure):
    _fields_ = [("q", vp), ("k", vp), ("v", vp), ("out", vp), ("bias", vp), ("kv_len", vp),
                ("dtype", i32), ("n", i32), ("L", i32), ("heads", i32), ("d", i32), ("ld_qkv", i32), ("ld_out", i32), ("scale", f32)]


class RmsnormParams(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("weight", vp), ("row_len", vp),
                ("dtype", i32), ("out_dtype", i32), ("rows", i32), ("C", i32), ("rows_per_sample", i32), ("eps", f32)]


class EmbedRowsParams(C.Structure):
    _fields_ = [("table", vp), ("ids", vp), ("out", vp), ("out_dtype", i32), ("rows", i32), ("C", i32), ("vocab", i32)]


class ReluParams(C.Structure):
    _fields_ = [("x", vp), ("n", i64), ("dtype", i32), ("pad_", i32)]


class AttentionCausalParams(C.Structure):
    _fields_ = [("q", vp), ("k", vp), ("v", vp), ("out", vp), ("row_len", vp),
                ("dtype", i32), ("n", i32), ("L", i32), ("heads", i32), ("d", i32), ("ld_qkv", i32), ("ld_out", i32), ("scale", f32)]


class LayernormRowsParams(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("gamma", vp), ("beta", vp), ("row_len", vp),
                ("dtype", i32), ("out_dtype", i32), ("rows", i32), ("C", i32), ("rows_per_sample", i32), ("eps", f32)]


class EmbedRowsPosParams(C.Structure):
    _fields_ = [("table", vp), ("pos", vp), ("ids", vp), ("out", vp),
                ("out_dtype", i32), ("rows", i32), ("C", i32), ("vocab", i32), ("L", i32), ("pad_", i32)]


class ActPassParams(C.Structure):
    _fields_ = [("x", vp), ("n", i64), ("dtype", i32), ("kind", i32)]


class TblockFrontParams(C.Structure):
    _fields_ = [("x", vp), ("Wp", vp), ("bp", vp), ("ln_g", vp), ("ln_b", vp), ("Wqkv", vp), ("Wo", vp), ("bo", vp),
                ("rowvec", vp), ("rowvec_map", vp), ("out", vp),
                ("dtype", i32), ("n", i32), ("L", i32), ("C", i32), ("heads", i32), ("ldx", i32), ("ld_out", i32), ("rowvec_ld", i32),
                ("ln_eps", f32), ("scale", f32)]


class EpsMseParams(C.Structure):
    _fields_ = [("pred", vp), ("eps", vp), ("x", vp), ("alpha", vp), ("sigma", vp),
                ("bj_of_unit", vp), ("img_of_bj", vp), ("out_index", vp),
                ("out", vp), ("n_units", i32), ("C", i32), ("H", i32), ("W", i32), ("ld", i32), ("v_param", i32), ("patch", i32)]


class ErrMapParams(C.Structure):
    _fields_ = [("pred", vp), ("eps", vp), ("x", vp), ("alpha", vp), ("sigma", vp),
                ("bj_of_unit", vp), ("img_of_bj", vp), ("out_index", vp),
                ("acc", vp), ("bad", vp),
                ("n_units", i32), ("C", i32), ("H", i32), ("W", i32), ("ld", i32), ("v_param", i32), ("patch", i32),
                ("T", i32), ("cells", i32), ("pad_", i32)]


class EvidenceMapsParams(C.Structure):
    _fields_ = [("acc", vp), ("bad", vp), ("stage_ends", vp), ("n_eval", vp), ("winner", vp),
                ("mean_map", vp), ("delta_map", vp), ("invalid", vp),
                ("n_stages", i32), ("BS", i32), ("C", i32), ("HW", i32)]


class DdpmStepParams(C.Structure):
    _fields_ = [("z", vp), ("pred", vp), ("noise", vp), ("out", vp),
                ("n", i32), ("C", i32), ("H", i32), ("W", i32), ("ld", i32), ("patch", i32), ("v_param", i32),
                ("w", f32), ("alpha_t", f32), ("sigma_t", f32), ("alpha_s", f32), ("c", f32), ("sd", f32), ("one_plus_w", f32)]


class DdpmStepSharedParams(C.Structure):
    _fields_ = [("z", vp), ("pred", vp), ("noise", vp), ("out", vp),
                ("n", i32), ("C", i32), ("H", i32), ("W", i32), ("ld", i32), ("patch", i32), ("v_param", i32), ("noise_div", i32),
                ("w", f32), ("alpha_t", f32), ("sigma_t", f32), ("alpha_s", f32), ("c", f32), ("sd", f32), ("one_plus_w", f32), ("pad_", i32)]


class SolverStepParams(C.Structure):
    _fields_ = [("z", vp), ("pred", vp), ("xprev", vp), ("xhat", vp), ("out", vp),
                ("n", i32), ("C", i32), ("H", i32), ("W", i32), ("ld", i32), ("patch", i32), ("v_param", i32), ("clamp", i32), ("final_pass", i32),
                ("w", f32), ("one_plus_w", f32), ("alpha_t", f32), ("sigma_t", f32), ("k1", f32), ("k2", f32), ("k3", f32)]


class DdpmNoiseMapParams(C.Structure):
    _fields_ = [("z", vp), ("pred", vp), ("x_next", vp), ("out", vp),
                ("n", i32), ("C", i32), ("H", i32), ("W", i32), ("ld", i32), ("patch", i32), ("v_param", i32),
                ("w", f32), ("one_plus_w", f32), ("alpha_t", f32), ("sigma_t", f32), ("alpha_s", f32), ("c", f32), ("sd", f32)]


class AbsDiffMapParams(C.Structure):
    _fields_ = [("a", vp), ("r", vp), ("r_of_a", vp), ("out", vp),
                ("n", i32), ("m", i32), ("C", i32), ("H", i32), ("W", i32), ("pad_", i32)]


class ClassPosteriorParams(C.Structure):
    _fields_ = [("errors", vp), ("probs", vp), ("entropy", vp), ("margin", vp), ("margin_z", vp),
                ("winner", vp), ("runner", vp), ("invalid", vp), ("means", vp), ("delta", vp), ("n_eval", vp),
                ("BS", i32), ("C", i32), ("T", i32), ("t_end", i32), ("temperature", f32), ("pad_", i32)]


class Op(C.Structure):
    _fields_ = [("kind", i32), ("pad_", i32), ("params", vp)]


# every symbol include/dcamd.h declares (tests check that the library exports all of them)
EXPORTS = ["dc_abi_version", "dc_last_error", "dc_arch", "dc_qsample", "dc_philox_normal", "dc_sinusoid",
           "dc_igemm", "dc_igemm_cout_pad", "dc_igemm_variant", "dc_igemm_instance", "dc_igemm_gn_fusable", "dc_igemm_side_ok", "dc_igemm_ln_ok", "dc_igemm_qstats_parts", "dc_igemm_up4_ok", "dc_igemm_pn_ok", "dc_pn_timeouts", "dc_conv3_pn_tail", "dc_conv3_pn_tail_ok", "dc_conv3_pn_tail_variant", "dc_conv3_pn_tail_ring_floats", "dc_groupnorm", "dc_groupnorm_variant", "dc_groupnorm_ws_floats", "dc_groupnorm_splits",
           "dc_layernorm", "dc_layernorm_variant", "dc_attention", "dc_attention_variant", "dc_attention_wide", "dc_attention_wide_variant", "dc_im2col_s2", "dc_latent_im2col", "dc_cross_attention", "dc_cross_attention_variant", "dc_cross_attention_len", "dc_cross_attention_len_variant", "dc_attention_bias", "dc_attention_bias_variant", "dc_rmsnorm", "dc_embed_rows", "dc_relu", "dc_attention_causal", "dc_attention_causal_variant", "dc_layernorm_rows", "dc_embed_rows_pos", "dc_act_pass", "dc_tblock_front", "dc_tblock_front_ok", "dc_eps_mse", "dc_err_map", "dc_evidence_maps", "dc_ddpm_step", "dc_ddpm_step_shared", "dc_solver_step", "dc_ddpm_noise_map", "dc_abs_diff_map", "dc_haar_dwt2", "dc_haar_idwt2", "dc_stage_topk", "dc_reduce_argmin", "dc_stage_maps", "dc_stage_maps_rows", "dc_stage_stop", "dc_class_posterior", "dc_run_plan", "dc_run_plan_timed",
           "dc_packed_bytes", "dc_pack_weights_matrix", "dc_pack_weights_conv3x3", "dc_pack_weights_up4", "dc_pack_weights_geglu",
           "dc_fold_layernorm_bias", "dc_workspace_bytes_groupnorm", "dc_workspace_bytes_igemm", "dc_workspace_bytes_attention",
           "dc_workspace_bytes_layernorm"]

_lib = None


class DcamdError(RuntimeError):
    pass


def lib():
    """Load libdcamd.so once.  Raises (never falls back) when the extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DcamdError(
            f"HIP extension {LIB_PATH} is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C diffusion-classifier_amd/csrc`). There is no CPU fallback for the scoring path.")
    L = C.CDLL(LIB_PATH)
    L.dc_abi_version.restype = i32
    L.dc_last_error.restype = C.c_char_p
    L.dc_arch.restype = C.c_char_p
    for name, argt in [("dc_qsample", [C.POINTER(QsampleParams), vp]),
                       ("dc_sinusoid", [C.POINTER(SinusoidParams), vp]),
                       ("dc_igemm", [C.POINTER(IgemmParams), vp]),
                       ("dc_groupnorm", [C.POINTER(GroupnormParams), vp]),
                       ("dc_layernorm", [C.POINTER(LayernormParams), vp]),
                       ("dc_attention", [C.POINTER(AttentionParams), vp]),
                       ("dc_attention_wide", [C.POINTER(AttentionWideParams), vp]),
                       ("dc_im2col_s2", [C.POINTER(Im2colS2Params), vp]),
                       ("dc_latent_im2col", [C.POINTER(LatentIm2colParams), vp]),
                       ("dc_cross_attention", [C.POINTER(CrossAttentionParams), vp]),
                       ("dc_cross_attention_len", [C.POINTER(CrossAttentionLenParams), vp]),
                       ("dc_attention_bias", [C.POINTER(AttentionBiasParams), vp]),
                       ("dc_rmsnorm", [C.POINTER(RmsnormParams), vp]),
                       ("dc_embed_rows", [C.POINTER(EmbedRowsParams), vp]),
                       ("dc_relu", [C.POINTER(ReluParams), vp]),
                       ("dc_attention_causal", [C.POINTER(AttentionCausalParams), vp]),
                       ("dc_layernorm_rows", [C.POINTER(LayernormRowsParams), vp]),
                       ("dc_embed_rows_pos", [C.POINTER(EmbedRowsPosParams), vp]),
                       ("dc_act_pass", [C.POINTER(ActPassParams), vp]),
                       ("dc_tblock_front", [C.POINTER(TblockFrontParams), vp]),
                       ("dc_eps_mse", [C.POINTER(EpsMseParams), vp]),
                       ("dc_err_map", [C.POINTER(ErrMapParams), vp]),
                       ("dc_evidence_maps", [C.POINTER(EvidenceMapsParams), vp]),
                       ("dc_class_posterior", [C.POINTER(ClassPosteriorParams), vp]),
                       ("dc_ddpm_step", [C.POINTER(DdpmStepParams), vp]),
                       ("dc_ddpm_step_shared", [C.POINTER(DdpmStepSharedParams), vp]),
                       ("dc_solver_step", [C.POINTER(SolverStepParams), vp]),
                       ("dc_ddpm_noise_map", [C.POINTER(DdpmNoiseMapParams), vp]),
                       ("dc_abs_diff_map", [C.POINTER(AbsDiffMapParams), vp]),
                       ("dc_run_plan", [C.POINTER(Op), i32, vp]),
                       ("dc_run_plan_timed", [C.POINTER(Op), i32, vp, vp]),
                       ("dc_philox_normal", [vp, i64, i64, vp, u64, vp]),
                       ("dc_haar_dwt2", [vp, vp, i32, i32, i32, i32, f32, vp]),
                       ("dc_haar_idwt2", [vp, vp, i32, i32, i32, i32, f32, vp]),
                       ("dc_pack_weights_matrix", [vp, i32, i32, i32, vp, vp, vp, i32, i32, vp]),
                       ("dc_pack_weights_conv3x3", [vp, i32, i32, i32, i32, i32, vp, i32, i32, vp]),
                       ("dc_pack_weights_up4", [vp, i32, i32, vp, i32, i32, vp]),
                       ("dc_pack_weights_geglu", [vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp]),
                       ("dc_fold_layernorm_bias", [vp, vp, vp, i32, i32, vp, vp]),
                       ("dc_stage_topk", [vp, i32, i32, i32, i32, i32, vp, vp, vp]),
                       ("dc_reduce_argmin", [vp, i32, i32, i32, i32, vp, vp, vp]),
                       ("dc_stage_maps", [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
                       ("dc_stage_maps_rows", [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
                       ("dc_stage_stop", [vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp])]:
        fn = getattr(L, name)
        fn.argtypes = argt
        fn.restype = i32
    L.dc_igemm_ln_ok.argtypes = [C.POINTER(IgemmParams)]
    L.dc_igemm_ln_ok.restype = C.c_int32
    L.dc_igemm_qstats_parts.argtypes = [C.POINTER(IgemmParams)]
    L.dc_igemm_qstats_parts.restype = C.c_int32
    L.dc_igemm_up4_ok.argtypes = [C.POINTER(IgemmParams)]
    L.dc_igemm_up4_ok.restype = C.c_int32
    L.dc_igemm_pn_ok.argtypes = [C.POINTER(IgemmParams)]
    L.dc_igemm_pn_ok.restype = C.c_int32
    L.dc_tblock_front_ok.argtypes = [C.POINTER(TblockFrontParams)]
    L.dc_tblock_front_ok.restype = C.c_int32
    L.dc_pn_timeouts.argtypes = []
    L.dc_pn_timeouts.restype = C.c_int32
    L.dc_conv3_pn_tail.argtypes = [C.POINTER(IgemmParams), C.POINTER(PnTailParams), vp]
    L.dc_conv3_pn_tail.restype = i32
    L.dc_conv3_pn_tail_ok.argtypes = [C.POINTER(IgemmParams), C.POINTER(PnTailParams)]
    L.dc_conv3_pn_tail_ok.restype = i32
    L.dc_conv3_pn_tail_variant.argtypes = [C.POINTER(IgemmParams), C.POINTER(PnTailParams)]
    L.dc_conv3_pn_tail_variant.restype = C.c_char_p
    L.dc_conv3_pn_tail_ring_floats.argtypes = [C.POINTER(IgemmParams), C.POINTER(PnTailParams)]
    L.dc_conv3_pn_tail_ring_floats.restype = i64
    L.dc_igemm_side_ok.argtypes = [C.POINTER(IgemmParams)]
    L.dc_igemm_side_ok.restype = C.c_int32
    L.dc_igemm_variant.argtypes = [C.POINTER(IgemmParams)]
    L.dc_igemm_variant.restype = C.c_char_p
    L.dc_igemm_instance.argtypes = [C.POINTER(IgemmParams), C.POINTER(C.c_int32)]
    L.dc_igemm_instance.restype = C.c_char_p
    L.dc_attention_variant.argtypes = [C.POINTER(AttentionParams)]
    L.dc_attention_variant.restype = C.c_char_p
    L.dc_attention_wide_variant.argtypes = [C.POINTER(AttentionWideParams)]
    L.dc_attention_wide_variant.restype = C.c_char_p
    L.dc_cross_attention_variant.argtypes = [C.POINTER(CrossAttentionParams)]
    L.dc_cross_attention_variant.restype = C.c_char_p
    L.dc_cross_attention_len_variant.argtypes = [C.POINTER(CrossAttentionLenParams)]
    L.dc_cross_attention_len_variant.restype = C.c_char_p
    L.dc_attention_bias_variant.argtypes = [C.POINTER(AttentionBiasParams)]
    L.dc_attention_bias_variant.restype = C.c_char_p
    L.dc_attention_causal_variant.argtypes = [C.POINTER(AttentionCausalParams)]
    L.dc_attention_causal_variant.restype = C.c_char_p
    L.dc_groupnorm_variant.argtypes = [C.POINTER(GroupnormParams)]
    L.dc_groupnorm_variant.restype = C.c_char_p
    L.dc_layernorm_variant.argtypes = [C.POINTER(LayernormParams)]
    L.dc_layernorm_variant.restype = C.c_char_p
    L.dc_igemm_gn_fusable.argtypes = [C.POINTER(IgemmParams)]
    L.dc_igemm_gn_fusable.restype = i32
    L.dc_igemm_cout_pad.argtypes = [i32, i32]
    L.dc_igemm_cout_pad.restype = i32
    L.dc_packed_bytes.argtypes = [i32, i32, i32, i32]
    L.dc_packed_bytes.restype = i64
    for name, pt in (("dc_workspace_bytes_groupnorm", GroupnormParams), ("dc_workspace_bytes_igemm", IgemmParams),
                     ("dc_workspace_bytes_attention", AttentionParams), ("dc_workspace_bytes_layernorm", LayernormParams)):
        getattr(L, name).argtypes = [C.POINTER(pt)]
        getattr(L, name).restype = i64
    L.dc_groupnorm_ws_floats.argtypes = [i32, i32, i32]
    L.dc_groupnorm_ws_floats.restype = i64
    L.dc_groupnorm_splits.argtypes = [i32, i32, i32]
    L.dc_groupnorm_splits.restype = i32
    if L.dc_abi_version() != ABI_VERSION:
        raise DcamdError(f"libdcamd ABI {L.dc_abi_version()} != {ABI_VERSION} (stale libdcamd.so? rebuild with `make -C diffusion-classifier_amd/csrc`)")
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        raise DcamdError(f"{what} failed (status {rc}): {lib().dc_last_error().decode()}")


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise DcamdError("the diffusion-classifier scoring path needs an MI355X (HIP device); no CPU fallback exists")
    return lib()
