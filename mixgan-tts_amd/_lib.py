"""ctypes binding of libmixgan_hip.so (C ABI: include/mixgan_hip.h)."""
import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

class MixganHipError(RuntimeError):
    pass


# ---- constants of include/mixgan_hip.h under their header names.  tests/test_host_cpu.py holds every MG_* name of this
# module to the header's value, and _signatures() to its prototypes.
MG_OK, MG_ERR_ARG, MG_ERR_SHAPE, MG_ERR_WORKSPACE = 0, -1, -2, -3
MG_ACT_NONE, MG_ACT_RELU, MG_ACT_LRELU02, MG_ACT_TANH, MG_ACT_LRELU = range(5)
MG_PACK_PLAIN, MG_PACK_GATE, MG_PACK_DGRAD, MG_PACK_TPOSE, MG_PACK_PLAIN16, MG_PACK_GATE16 = range(6)
MG_DEN_BACKWARD, MG_DEN_SPLIT, MG_DEN_P16, MG_DEN_JOBS_RESIDENT = 1, 2, 4, 8      # mg_denoiser_pack flags
MG_FWD_SAVE, MG_FWD_SPLIT, MG_FWD_P16 = 1, 2, 4                                   # mg_denoiser_fwd modes
MG_PLAN_PER_LAYER, MG_PLAN_SINGLE = 0, 1                                          # mg_fwd_plan.path
MG_PLAN_PERSIST, MG_PLAN_PERSIST16, MG_PLAN_TEAM16 = 0, 1, 2                      # mg_fwd_plan.family
MG_STATUS_TICKET, MG_STATUS_ERROR, MG_STATUS_LAUNCHES, MG_STATUS_DONE, MG_STATUS_WORDS = range(5)   # mg_denoiser_*_status
MG_CONV_EPI_PLAIN, MG_CONV_EPI_REFLECT, MG_CONV_EPI_PHASES_SLICE, MG_CONV_EPI_NEEDS_WM2 = range(4)   # mg_conv1d_fwd_plan
MG_CONV_EPI_PERIOD = 5                                                            # (4 names no list: MG_ERR_ARG)
# the denoiser's weight / gradient pointer table: head slots, then MG_DEN_LAYER_PTRS slots per residual layer
MG_DEN_HEAD_PTRS, MG_DEN_LAYER_PTRS = 8, 9
(MG_DEN_IN_W, MG_DEN_IN_B, MG_DEN_MLP0_W, MG_DEN_MLP2_W, MG_DEN_SKIP_W, MG_DEN_SKIP_B, MG_DEN_OUT_W,
 MG_DEN_OUT_B) = range(MG_DEN_HEAD_PTRS)
(MG_DEN_L_CONV_W, MG_DEN_L_CONV_B, MG_DEN_L_DIFF_W, MG_DEN_L_COND_W, MG_DEN_L_COND_B, MG_DEN_L_OUT_W, MG_DEN_L_OUT_B,
 MG_DEN_L_SPK_W, MG_DEN_L_RESERVED) = range(MG_DEN_LAYER_PTRS)
MG_LOSS_MAX_TERMS, MG_LOSS_GROUPS = 16, 4
MG_RESAMPLE_MAX_UP, MG_RESAMPLE_MAX_TAPS, MG_RESAMPLE_TILE, MG_RESAMPLE_MAX_SPAN = 1024, 1024, 1024, 16384
MG_PITCH_N, MG_PITCH_W, MG_PITCH_K, MG_PITCH_PARAMS = 1024, 512, 4, 7
(MG_PITCH_P_SR, MG_PITCH_P_TAU_MAX, MG_PITCH_P_THETA, MG_PITCH_P_BETA, MG_PITCH_P_LAMBDA, MG_PITCH_P_SWITCH,
 MG_PITCH_P_GATE) = range(MG_PITCH_PARAMS)
MG_ALIGN_MAX_D, MG_ALIGN_MAX_G, MG_ALIGN_MAX_S, MG_ALIGN_MAX_T = 128, 1024, 2048, 4096
MG_CEPSTRA_MAX_M, MG_DTW_MAX_T, MG_DTW_MAX_D = 128, 4096, 64
MG_GCONV_FWD, MG_GCONV_DGRAD = 0, 1                                               # mg_gconv_pack modes
MG_LOSSMODE_MSE, MG_LOSSMODE_L1, MG_LOSSMODE_HINGE, MG_LOSSMODE_MEAN = range(4)    # MgLossTerm.mode
MG_ATTN_PLAIN128, MG_ATTN_KSPLIT64, MG_ATTN_KSPLIT128, MG_ATTN_WIDE256 = range(4)  # mg_attention_form


class LossTerm(ctypes.Structure):
    _fields_ = [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("da", ctypes.c_void_p), ("n", ctypes.c_size_t),
                ("c", ctypes.c_float), ("weight", ctypes.c_float), ("mode", ctypes.c_int32), ("group", ctypes.c_int32)]


class DenoiserDims(ctypes.Structure):
    _fields_ = [("n_layers", ctypes.c_int32), ("channels", ctypes.c_int32), ("cond_channels", ctypes.c_int32),
                ("mel_bins", ctypes.c_int32), ("multi_speaker", ctypes.c_int32)]


class SamplingLoop(ctypes.Structure):
    """mg_sampling_loop (include/mixgan_hip.h): what the steps of one sampling loop share."""
    _fields_ = [("cproj", ctypes.c_void_p), ("cproj_out", ctypes.c_void_p), ("step_vectors", ctypes.c_void_p),
                ("step_index", ctypes.c_int32), ("step_count", ctypes.c_int32)]


class FwdPlan(ctypes.Structure):
    """mg_fwd_plan (include/mixgan_hip.h): which kernel the denoiser forward runs."""
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "family", "nt", "waves", "solo", "team", "cproj_mode", "grid",
                                              "block")]


class ConvPlan(ctypes.Structure):
    """mg_conv_plan (include/mixgan_hip.h): which instantiation of the convolution kernel a launch runs."""
    _fields_ = [(n, ctypes.c_int32) for n in ("kw", "stride", "ck", "dilmax", "mw", "wm", "nnb", "ksplit", "grid")]


def library_path():
    # MG_HIP_LIB: another build of the same library (tools: A/B timing of two builds inside one gpurun call)
    return os.environ.get("MG_HIP_LIB") or os.path.join(_HERE, "libmixgan_hip.so")


def build(force=False):
    """Compile the HIP sources in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(library_path()):
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"] + (["-B"] if force else []))
    return library_path()


def lib():
    """Load the HIP library; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise MixganHipError(
                "libmixgan_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C mixgan-tts_amd/csrc`. There is no CPU fallback." % path)
        L = ctypes.CDLL(path)
        _declare(L)
        _LIB = L
    return _LIB


def _signatures():
    """name -> (restype, argtypes) for every export of include/mixgan_hip.h."""
    vp, i, f, sz, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_long
    dp = ctypes.POINTER(DenoiserDims)
    return {
        "mg_version": (i, []),
        "mg_error_string": (ctypes.c_char_p, [i]),
        "mg_conv_packed_floats": (sz, [i, i, i, i]),
        "mg_conv_pack": (i, [vp, vp, i, i, i, i, vp]),
        "mg_conv1d_fwd": (i, [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, f, i, vp]),
        "mg_conv1d_fwd_ex": (i, [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, f, i, f, f, i, vp]),
        "mg_conv1d_fwd_split": (i, [vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, f, i, f, f, i, vp, sz, vp]),
        "mg_conv1d_fwd_plan": (i, [i, i, i, i, i, i, i, sz, i, ctypes.POINTER(ConvPlan)]),
        "mg_upsample_zero_act": (i, [vp, vp, i, i, i, i, f, vp]),
        "mg_diffuse_trace_bwd": (i, [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]),
        "mg_bgemm": (i, [vp, vp, vp, i, i, i, i, i] + [lg] * 11 + [f, i, vp]),
        "mg_bgemm_tile": (i, [i, i, i, i]),
        "mg_softmax_rows_fwd": (i, [vp, vp, i, i, i, f, vp]),
        "mg_softmax_rows_bwd": (i, [vp, vp, i, i, i, f, vp]),
        "mg_layernorm_cm_train_fwd": (i, [vp, vp, f, vp, vp, vp, vp, vp, vp, i, i, i, f, vp]),
        "mg_layernorm_cm_bwd": (i, [vp, vp, vp, vp, vp, f, vp, vp, vp, vp, i, i, i, f, vp]),
        "mg_bn_stats": (i, [vp, vp, vp, i, i, i, vp]),
        "mg_bn_act_fwd": (i, [vp, vp, vp, vp, vp, vp, f, i, vp, vp, i, i, i, vp]),
        "mg_bn_act_bwd_reduce": (i, [vp, vp, f, vp, vp, vp, vp, i, vp, vp, i, i, i, vp]),
        "mg_bn_act_bwd_apply": (i, [vp, vp, f, vp, vp, vp, vp, vp, vp, vp, f, i, vp, i, i, i, vp]),
        "mg_conv_transpose_packed_floats": (sz, [i, i, i]),
        "mg_conv_transpose_pack": (i, [vp, vp, i, i, i, vp]),
        "mg_conv_transpose1d_fwd": (i, [vp, vp, vp, vp, i, i, i, i, i, f, f, vp]),
        "mg_diffuse_fwd": (i, [vp] * 9 + [i, i, i, i, vp]),
        "mg_posterior_sample_fwd": (i, [vp] * 10 + [i, i, i, i, i, vp]),
        "mg_transpose_bml": (i, [vp] * 5 + [i, i, i, i, i, vp]),
        "mg_posterior_sample_bwd": (i, [vp] * 7 + [i, i, i, i, i, vp]),
        "mg_spec_affine": (i, [vp, vp, vp, vp, i, sz, i, vp]),
        "mg_conv_pack_at": (i, [vp, vp, i, i, i, i, i, i, vp]),
        "mg_conv1d_wgrad_scratch_floats": (sz, [i, i, i]),
        "mg_conv1d_wgrad": (i, [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, f, i, vp]),
        "mg_conv1d_wgrad_strided": (i, [vp, lg, vp, lg, vp, vp, vp, i, i, i, i, i, i, i, i, f, i, vp]),
        "mg_rowsum": (i, [vp, lg, i, i, i, vp, vp, f, i, vp]),
        "mg_conv1d_wgrad_grouped_scratch_floats": (sz, [i, i, i, i]),
        "mg_conv1d_wgrad_grouped": (i, [vp, lg, lg, vp, lg, lg, vp, lg, vp, i, i, i, i, i, i, i, i, i, f, i, vp]),
        "mg_conv1d_wgrad_grouped_bias": (i, [vp, lg, lg, vp, lg, lg, vp, lg, vp, lg, vp, i, i, i, i, i, i, i, i, i, f, i, vp]),
        "mg_denoiser_packed_floats": (sz, [dp, i]),
        "mg_denoiser_pack": (i, [dp, vp, vp, vp, i, vp]),
        "mg_denoiser_pack_plan": (i, [dp, vp, vp, vp, i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
        "mg_denoiser_bwd_workspace_floats": (sz, [dp, i, i]),
        "mg_denoiser_bwd": (i, [dp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, i, i, vp]),
        "mg_denoiser_bwd_staged": (i, [dp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, i, i, vp, vp]),
        "mg_denoiser_workspace_floats": (sz, [dp, i, i, i]),
        "mg_denoiser_fwd": (i, [dp, vp, vp, vp, vp, vp, vp, vp, sz, i, i, i, vp]),
        "mg_denoiser_fwd_pair": (i, [dp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, sz, i, i, vp]),
        "mg_denoiser_fwd_plan": (i, [dp, i, i, i, i, i, ctypes.POINTER(FwdPlan)]),
        "mg_transpose_bml_strided": (i, [vp] * 5 + [i, i, i, i, i, lg, vp]),
        "mg_transpose_max_m": (i, []),
        "mg_act_bwd": (i, [vp, vp, vp, i, sz, vp]),
        "mg_upsample_zero": (i, [vp, vp, i, i, i, i, vp]),
        "mg_step_mlp_fwd": (i, [vp] * 8 + [i, i, i, i, vp]),
        "mg_step_mlp_bwd": (i, [vp] * 8 + [i, i, i, i, vp]),
        "mg_linear_small_fwd": (i, [vp, vp, vp, i, i, i, vp]),
        "mg_linear_small_bwd": (i, [vp, vp, vp, vp, vp, i, i, i, vp]),
        "mg_loss_sum": (i, [vp, vp, f, i, sz, vp, vp]),
        "mg_multi_loss_scratch_floats": (sz, []),
        "mg_multi_loss_fwd": (i, [vp, i, vp, vp, vp]),
        "mg_multi_loss_bwd": (i, [vp, i, vp, vp]),
        "mg_multi_loss_fwd_den": (i, [vp, i, vp, vp, vp, vp]),
        "mg_multi_loss_bwd_den": (i, [vp, i, vp, vp, vp]),
        "mg_grad_norm_scratch_floats": (sz, []),
        "mg_grad_norm": (i, [vp, sz, f, vp, vp, vp]),
        "mg_adam_flat": (i, [vp, vp, vp, vp, sz, f, f, f, f, f, lg, vp, vp]),
        "mg_adam_flat_dev": (i, [vp, vp, vp, vp, sz, f, f, f, f, f, lg, vp, vp, vp]),
        "mg_loss_grad": (i, [vp, vp, f, i, vp, f, sz, vp, vp]),
        "mg_mel_l1_fwd": (i, [vp, vp, vp, i, i, vp, vp]),
        "mg_mel_l1_bwd": (i, [vp, vp, vp, i, i, vp, vp, vp, vp]),
        "mg_mel_count_rows": (i, [vp, vp, i, i, vp, vp]),
        "mg_attention_fwd": (i, [vp, vp, vp, i, i, i, i, f, vp]),
        "mg_attention_fwd_f16": (i, [vp, vp, vp, i, i, i, i, f, vp]),
        "mg_attention_form": (i, [i, i, i, i]),
        "mg_layernorm_cm_fwd": (i, [vp, vp, vp, vp, vp, vp, i, i, i, f, vp]),
        "mg_length_regulate_fwd": (i, [vp, vp, vp, vp, i, i, i, i, vp]),
        "mg_length_regulate_bwd": (i, [vp, vp, vp, i, i, i, i, vp]),
        "mg_word_pool_fwd": (i, [vp, vp, vp, vp, i, i, i, i, i, i, vp]),
        "mg_word_pool_bwd": (i, [vp, vp, vp, vp, i, i, i, i, i, i, vp]),
        "mg_mapping_mask": (i, [vp, vp, vp, vp, i, i, i, i, vp]),
        "mg_rel_coef": (i, [vp, vp, vp, vp, i, i, i, vp]),
        "mg_rel_attention_fwd": (i, [vp, vp, vp, vp, vp, i, i, i, i, i, vp]),
        "mg_w2p_attention_fwd": (i, [vp] * 10 + [i, i, i, i, i, vp]),
        "mg_le_attention_rows": (i, [i]),
        "mg_embed_cm": (i, [vp, vp, vp, vp, i, i, i, i, vp]),
        "mg_variance_head": (i, [vp, vp, vp, vp, f, vp, vp, i, vp, vp, vp, i, i, i, vp]),
        "mg_duration_head": (i, [vp, vp, vp, vp, f, vp, vp, i, i, i, i, vp]),
        "mg_posenc_add": (i, [vp, i, vp, vp, vp, i, i, i, vp]),
        "mg_rel_attention_train_fwd": (i, [vp, vp, vp, vp, vp, f, vp, vp, i, i, i, i, i, vp]),
        "mg_rel_attention_bwd_ws_floats": (sz, [i, i, i, i]),
        "mg_rel_attention_bwd": (i, [vp, vp, vp, vp, f] + [vp] * 7 + [sz, i, i, i, i, i, vp]),
        "mg_w2p_attention_bwd_ws_floats": (sz, [i, i, i, i]),
        "mg_w2p_attention_bwd": (i, [vp] * 16 + [sz, i, i, i, i, i, vp]),
        "mg_embed_cm_bwd": (i, [vp, vp, vp, vp, i, i, i, i, i, vp]),
        "mg_variance_head_bwd": (i, [vp, vp, vp, f, vp, vp, vp, vp, i, i, i, vp]),
        "mg_duration_head_bwd": (i, [vp] * 6 + [i, i, i, i, vp]),
        "mg_posenc_add_bwd": (i, [vp, vp, vp, i, i, i, vp]),
        "mg_dropout_apply": (i, [vp, vp, f, vp, sz, vp]),
        "mg_resblock_fwd": (i, [vp] * 16 + [i, i, i, i, vp]),
        "mg_gate_bwd": (i, [vp, vp, vp, vp, i, i, i, vp]),
        "mg_mish_fwd": (i, [vp, vp, sz, vp]),
        "mg_mish_bwd": (i, [vp, vp, vp, sz, vp]),
        "mg_step_embed": (i, [vp, vp, vp, i, i, vp]),
        "mg_denoiser_psample": (i, [dp] + [vp] * 8 + [i, vp, ctypes.c_ulonglong, ctypes.c_ulonglong, i, vp, vp, vp, vp, sz,
                                    i, i, i, vp]),
        "mg_denoiser_step_vectors_floats": (sz, [dp, i, i]),
        "mg_denoiser_step_vectors": (i, [dp, vp, vp, vp, vp, sz, i, i, vp]),
        "mg_denoiser_cond_project": (i, [dp, vp, vp, vp, i, i, vp]),
        "mg_persist_error": (ctypes.c_uint, [i]),
        "mg_denoiser_persist_status": (i, [dp, vp, i, i, vp, vp]),
        "mg_denoiser_bwd_status": (i, [dp, vp, i, i, vp, vp]),
        "mg_profile_begin": (i, [i]),
        "mg_profile_begin_sampled": (i, [i, i]),
        "mg_profile_end": (i, [vp, i]),
        "mg_conv_transpose1d_fwd_slice": (i, [vp, vp, vp, vp, lg, i, i, i, i, i, f, f, vp]),
        "mg_conv1d_reflect_fwd": (i, [vp, lg, vp, vp, vp, lg, i, i, i, i, i, i, f, i, f, f, vp]),
        "mg_conv1x1_fwd_strided": (i, [vp, lg, vp, vp, vp, lg, i, i, i, i, vp]),
        "mg_melgan_stack_fwd": (i, [vp, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                    ctypes.POINTER(vp), i, i, i, vp]),
        "mg_melgan_stack_tile": (i, [i]),
        "mg_stft_fwd": (i, [vp, lg, vp, i, i, i, vp, vp, vp, vp, lg, lg, lg, i, vp]),
        "mg_stft_mel": (i, [vp, lg, vp, i, i, i, vp, vp, vp, vp, i, vp, vp, i, vp]),
        "mg_istft": (i, [vp, vp, lg, lg, lg, i, i, i, vp, vp, vp, vp, i, vp]),
        "mg_ds_fbank": (i, [vp, lg, vp, vp, vp, i, i, i, i, vp, vp, vp, i, vp, vp]),
        "mg_ds_conv2d": (i, [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, vp]),
        "mg_ds_head": (i, [vp, vp, vp, vp, i, i, i, i, vp]),
        "mg_betabinom_prior": (i, [vp, vp, ctypes.POINTER(ctypes.c_double), vp, i, i, i, i, vp]),
        "mg_phoneme_average": (i, [vp, vp, vp, vp, vp, i, i, i, i, vp]),
        "mg_resample_poly": (i, [vp, lg, vp, i, i, vp, i, i, i, i, vp, lg, i, vp]),
        "mg_peak_normalize_i16": (i, [vp, lg, vp, i, i, f, vp, lg, vp]),
        "mg_yin_candidates": (i, [vp, lg, vp, i, i, i, i, i, vp, vp, vp, vp, i, vp]),
        "mg_pitch_track_workspace_bytes": (sz, [i, i]),
        "mg_pitch_track": (i, [vp, vp, vp, vp, i, i, ctypes.POINTER(ctypes.c_double), vp, vp, sz, vp]),
        "mg_align_emissions": (i, [vp, vp, i, i, i, vp, vp, vp, i, vp, vp]),
        "mg_align_viterbi_workspace_bytes": (sz, [i, i, i]),
        "mg_align_viterbi": (i, [vp, vp, vp, vp, vp, i, i, i, i, vp, vp, vp, vp, sz, vp]),
        "mg_align_stats": (i, [vp, vp, vp, i, i, vp, vp, vp]),
        "mg_mel_cepstra": (i, [vp, vp, i, i, i, i, vp, vp]),
        "mg_dtw_workspace_bytes": (sz, [i, i, i]),
        "mg_dtw": (i, [vp, vp, vp, vp, i, i, i, i, vp, vp, vp, vp, sz, vp]),
        "mg_conv1d_wgrad_ex": (i, [vp, lg, vp, lg, vp, vp, i, i, i, i, i, i, i, i, f, f, i, vp]),
        "mg_lrelu_bwd": (i, [vp, vp, vp, vp, f, sz, vp]),
        "mg_conv1d_reflect_wgrad": (i, [vp, lg, vp, lg, vp, vp, i, i, i, i, i, i, f, f, i, vp]),
        "mg_conv1d_reflect_dgrad_workspace_floats": (sz, [i, i, i, i, i]),
        "mg_conv1d_reflect_dgrad": (i, [vp, vp, vp, lg, vp, lg, vp, vp, sz, i, i, i, i, i, i, f, f, vp]),
        "mg_reflect_fold_bwd": (i, [vp, lg, vp, lg, vp, lg, vp, i, i, i, i, f, vp]),
        "mg_conv_transpose1d_dgrad_workspace_floats": (sz, [i, i, i, i, i]),
        "mg_conv_transpose1d_dgrad": (i, [vp, vp, vp, vp, vp, sz, i, i, i, i, i, f, f, vp]),
        "mg_conv_transpose1d_wgrad_scratch_floats": (sz, [i, i, i]),
        "mg_conv_transpose1d_wgrad": (i, [vp, vp, vp, vp, i, i, i, i, i, f, f, i, vp]),
        "mg_stft_mel_bwd_workspace_bytes": (sz, [i, i]),
        "mg_stft_mel_bwd": (i, [vp, lg, vp, i, i, i, vp, vp, vp, vp, i, vp, i, vp, lg, vp, sz, vp]),
        "mg_gconv_packed_floats": (sz, [i, i, i, i, i, i]),
        "mg_gconv_pack": (i, [vp, vp, i, i, i, i, i, i, vp]),
        "mg_gconv1d_fwd": (i, [vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, f, vp]),
        "mg_gconv1d_dgrad": (i, [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, f, vp]),
        "mg_gconv1d_wgrad_scratch_floats": (sz, [i, i, i, i, i, i, i]),
        "mg_gconv1d_wgrad": (i, [vp, vp, vp, vp, sz, i, i, i, i, i, i, i, i, i, vp]),
        "mg_conv1d_c1_fwd": (i, [vp, vp, vp, vp, i, i, i, i, i, i, f, vp]),
        "mg_conv1d_c1_dgrad": (i, [vp, vp, vp, i, i, i, i, i, vp]),
        "mg_conv1d_c1_wgrad_scratch_floats": (sz, [i, i, i, i]),
        "mg_conv1d_c1_wgrad": (i, [vp, vp, vp, vp, vp, sz, i, i, i, i, i, vp]),
        "mg_avgpool4s2_fwd": (i, [vp, vp, i, i, vp]),
        "mg_avgpool4s2_bwd": (i, [vp, vp, i, i, vp]),
        "mg_avgpool4s2p1_fwd": (i, [vp, vp, i, i, vp]),
        "mg_avgpool4s2p1_bwd": (i, [vp, vp, i, i, vp]),
        "mg_reflect_pad1d_fwd": (i, [vp, vp, i, i, i, vp]),
        "mg_reflect_pad1d_bwd": (i, [vp, vp, i, i, i, vp]),
        "mg_period_geometry": (i, [i, i, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
        "mg_period_fold_fwd": (i, [vp, vp, i, i, i, vp]),
        "mg_period_fold_bwd": (i, [vp, vp, i, i, i, vp]),
        "mg_period_conv_fwd": (i, [vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, i, f, vp, sz, vp]),
        "mg_period_dgrad3_packed_floats": (sz, [i, i]),
        "mg_period_dgrad3_pack": (i, [vp, vp, i, i, vp]),
        "mg_period_conv_dgrad": (i, [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, f, vp, sz, vp]),
    }


EXPORTS = tuple(_signatures())


def _declare(L):
    for name, (res, args) in _signatures().items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args


def check(rc):
    if rc != 0:
        raise MixganHipError("libmixgan_hip: %s (code %d)" % (lib().mg_error_string(rc).decode(), rc))


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def fptr(t, allow_none=False):
    """Device pointer of a contiguous fp32 CUDA tensor (the ABI takes plain pointers)."""
    if t is None:
        if allow_none:
            return ctypes.c_void_p(0)
        raise MixganHipError("missing tensor")
    if not t.is_cuda:
        raise MixganHipError("tensor is not on the GPU: the HIP path has no CPU fallback")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise MixganHipError("expected a contiguous fp32 tensor, got %s contiguous=%s" % (t.dtype, t.is_contiguous()))
    return ctypes.c_void_p(t.data_ptr())


def iptr(t, dtype, allow_none=False):
    if t is None:
        if allow_none:
            return ctypes.c_void_p(0)
        raise MixganHipError("missing tensor")
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise MixganHipError("expected a contiguous %s CUDA tensor" % dtype)
    return ctypes.c_void_p(t.data_ptr())
