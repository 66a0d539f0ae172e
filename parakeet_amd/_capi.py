"""ctypes binding of include/pk_synth.h (libpk_synth.so).

There is no fallback: if the shared library is missing or a call fails, an
exception is raised.  Status codes map back to the exception classes the
reference raises at the same places.
"""
import ctypes as C
import os

# PyTorch-ROCm bundles its own libamdhip64; two HIP runtimes in one process cannot both own
# the device.  Importing torch first makes libpk_synth.so bind to the runtime torch loaded.
import torch  # noqa: F401  (load order matters)

_HERE = os.path.dirname(os.path.abspath(__file__))
# PK_PROFILE_LIB=1 (read HERE, in Python -- the product library itself reads no environment variable): load the profile
# build (parakeet_amd.build.build(profile=True)), the one that carries the measurement / ablation switches tools/ uses.
PROFILE_LIB = os.environ.get("PK_PROFILE_LIB", "0") not in ("", "0")
LIB_PATH = os.path.join(_HERE, "libpk_synth_prof.so" if PROFILE_LIB else "libpk_synth.so")

PK_OK = 0
PK_EUNSUPPORTED = -3       # include/pk_synth.h pk_status: configuration not implemented
PK_HOST_IO = 1
PK_PWG_C_HAS_CONTEXT = 2
PK_APPLY_NORMALIZER = 4
PK_TTS_KEEP_ATT = 8
PK_PWG_MATH_F32, PK_PWG_MATH_BF16X3, PK_PWG_MATH_F16X3 = 0, 1, 2
PK_MEL_LOSS_ROWS = 16      # csrc/pk_mel_loss.h: map rows per tile of pk_mel_loss_run
# csrc/pk_seq_loss.h: entries per tile of pk_pair_loss_run / pk_bce_logits_run, rows x columns of pk_guided_attn_run's tile,
# the longest fp32 accumulation chain of the three (0: float64 throughout)
PK_SEQ_LOSS_PAIR_TILE, PK_SEQ_LOSS_GUIDE_ROWS, PK_SEQ_LOSS_GUIDE_COLS, PK_SEQ_LOSS_F32_CHAIN = 4096, 16, 64, 0
# csrc/pk_trim.h: windows per scan step of the VAD mask kernel; the pad modes of pk_trim_run
PK_TRIM_SCAN_CHUNK = 256
PK_TRIM_PAD = {None: 0, "reflect": 1, "constant": 2}
# csrc/pk_stats.h: the envelope of pk_stats_*; pk_stats_update's flag
PK_STATS_MAX_DIM, PK_STATS_MAX_ROWS, PK_STATS_MOMENTS_ONLY = 1024, 2 ** 31 - 1, 1
# pk_mel_set_transform / pk_istft_set_transform
PK_TRANSFORM = {"dense": 0, "fft": 1}
_EXC = {
    -1: ValueError,
    -2: AssertionError,
    -3: NotImplementedError,
    -4: RuntimeError,
    -5: MemoryError,
    -6: RuntimeError,
}


class PwgCfg(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("kernel_size", C.c_int32),
        ("layers", C.c_int32), ("stacks", C.c_int32), ("residual_channels", C.c_int32),
        ("gate_channels", C.c_int32), ("skip_channels", C.c_int32), ("aux_channels", C.c_int32),
        ("aux_context_window", C.c_int32), ("n_upsample", C.c_int32),
        ("upsample_scales", C.c_int32 * 8), ("use_causal_conv", C.c_int32),
    ]


class Fs2Cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "idim", "odim", "adim", "aheads", "elayers", "eunits", "dlayers", "dunits",
        "positionwise_conv_kernel_size", "positionwise_layer_type",
        "duration_predictor_layers", "duration_predictor_chans", "duration_predictor_kernel_size",
        "pitch_predictor_layers", "pitch_predictor_chans", "pitch_predictor_kernel_size",
        "energy_predictor_layers", "energy_predictor_chans", "energy_predictor_kernel_size",
        "pitch_embed_kernel_size", "energy_embed_kernel_size",
        "postnet_layers", "postnet_chans", "postnet_filts",
        "use_batch_norm", "use_scaled_pos_enc", "encoder_normalize_before", "decoder_normalize_before",
        "reduction_factor", "num_speakers", "spk_embed_dim", "spk_embed_integration_type", "num_tones", "tone_embed_dim",
        "tone_embed_integration_type", "encoder_concat_after", "decoder_concat_after")]


class WfCfg(C.Structure):
    _fields_ = [("n_upsample", C.c_int32), ("upsample_factors", C.c_int32 * 4), ("n_flows", C.c_int32),
                ("n_layers", C.c_int32), ("n_group", C.c_int32), ("channels", C.c_int32), ("n_mels", C.c_int32),
                ("kernel_h", C.c_int32), ("kernel_w", C.c_int32)]


class SsCfg(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("tone_size", C.c_int32), ("encoder_hidden_size", C.c_int32),
                ("encoder_kernel_size", C.c_int32), ("n_encoder_dilations", C.c_int32),
                ("encoder_dilations", C.c_int32 * 32), ("duration_predictor_hidden_size", C.c_int32),
                ("decoder_hidden_size", C.c_int32), ("decoder_output_size", C.c_int32),
                ("decoder_kernel_size", C.c_int32), ("n_decoder_dilations", C.c_int32),
                ("decoder_dilations", C.c_int32 * 32), ("same_padding_resets_dilation", C.c_int32)]


class TtsCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "idim", "odim", "embed_dim", "eprenet_conv_layers", "eprenet_conv_chans", "eprenet_conv_filts",
        "dprenet_layers", "dprenet_units", "adim", "aheads", "elayers", "eunits", "dlayers", "dunits",
        "postnet_layers", "postnet_chans", "postnet_filts", "positionwise_layer_type",
        "positionwise_conv_kernel_size", "use_scaled_pos_enc", "use_batch_norm", "encoder_normalize_before",
        "decoder_normalize_before", "encoder_concat_after", "decoder_concat_after", "reduction_factor",
        "spk_embed_dim", "use_gst", "spk_embed_integration_type", "gst_tokens", "gst_heads", "gst_conv_layers",
        "gst_conv_kernel_size", "gst_conv_stride", "gst_gru_layers", "gst_gru_units")] + [("gst_conv_chans", C.c_int32 * 8)]


class TacoCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "vocab_size", "n_tones", "d_mels", "reduction_factor", "d_encoder", "encoder_conv_layers",
        "encoder_kernel_size", "d_prenet", "d_attention_rnn", "d_decoder_rnn", "d_attention", "attention_filters",
        "attention_kernel_size", "d_postnet", "postnet_kernel_size", "postnet_conv_layers", "d_global_condition",
        "use_stop_token")] + [("p_prenet_dropout", C.c_float)]


class SpkCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "num_layers", "hidden_size", "output_size")]


class IstftCfg(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("hop_length", C.c_int32), ("center", C.c_int32)]


class ResampleCfg(C.Structure):
    _fields_ = [("up", C.c_int32), ("down", C.c_int32), ("taps", C.c_int32)]


class PitchCfg(C.Structure):
    _fields_ = [("sr", C.c_int32), ("hop", C.c_int32), ("tau_min", C.c_int32), ("tau_max", C.c_int32), ("win", C.c_int32),
                ("threshold", C.c_float)]


class PitchTrackCfg(C.Structure):
    _fields_ = [("K", C.c_int32), ("theta_c", C.c_float), ("lambda_", C.c_double), ("unvoiced_cost", C.c_double),
                ("switch_cost", C.c_double)]


class StoiResult(C.Structure):
    """pk_stoi_result"""
    _fields_ = [("d", C.c_double), ("segments", C.c_int32), ("kept", C.c_int32), ("frames", C.c_int32), ("reserved", C.c_int32)]


class MelCfg(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("hop_length", C.c_int32), ("center", C.c_int32), ("power", C.c_int32),
                ("n_mels", C.c_int32), ("log_base", C.c_int32), ("log_floor", C.c_float)]


class StftdRes(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("hop_length", C.c_int32), ("center", C.c_int32)]


class StftdCfg(C.Structure):
    _fields_ = [("n_res", C.c_int32), ("power_floor", C.c_float), ("log_floor", C.c_float)]


class PwgdCfg(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("in_channels", "out_channels", "kernel_size", "layers", "conv_channels",
                                          "dilation_factor")] + [("negative_slope", C.c_float), ("bias", C.c_int32)])


class HfgCfg(C.Structure):
    """pk_hfg_cfg"""
    _fields_ = ([(n, C.c_int32) for n in ("in_channels", "out_channels", "channels", "kernel_size", "n_upsample")] +
                [("upsample_scales", C.c_int32 * 6), ("upsample_kernel_sizes", C.c_int32 * 6), ("n_blocks", C.c_int32),
                 ("resblock_kernel_sizes", C.c_int32 * 4), ("n_dilations", C.c_int32 * 4),
                 ("resblock_dilations", (C.c_int32 * 4) * 4), ("use_additional_convs", C.c_int32), ("bias", C.c_int32),
                 ("negative_slope", C.c_float)])


class MganCfg(C.Structure):
    """pk_mgan_cfg"""
    _fields_ = ([(n, C.c_int32) for n in ("in_channels", "out_channels", "channels", "kernel_size", "n_upsample")] +
                [("upsample_scales", C.c_int32 * 6), ("stacks", C.c_int32), ("stack_kernel_size", C.c_int32), ("bias", C.c_int32),
                 ("use_final_nonlinear_activation", C.c_int32), ("negative_slope", C.c_float)])


class PqmfCfg(C.Structure):
    """pk_pqmf_cfg"""
    _fields_ = [("subbands", C.c_int32), ("taps", C.c_int32), ("cutoff_ratio", C.c_float), ("beta", C.c_float)]


class OpGemmCfg(C.Structure):
    """pk_op_gemm_cfg"""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "A2", "res", "a_amax", "a2_amax", "rowvalid", "out_rowmap", "C", "C2",
                                           "W", "bias", "cscale", "cshift", "W2", "bias2")] +
                [("tap_off", C.c_int64 * 12), ("tap_w", C.c_int32 * 12)] +
                [(n, C.c_int32) for n in ("M", "N", "Cin", "taps", "pad", "ntaps", "wtaps", "Cin2", "w2_slab0", "lda", "lda2",
                                          "ldr", "ldc", "ldc2", "math", "tile", "act", "epi", "res_pos", "nsplit", "acc2",
                                          "kernel")])


class OpRowgemmCfg(C.Structure):
    """pk_op_rowgemm_cfg"""
    _fields_ = ([(n, C.c_void_p) for n in ("x", "res", "y", "lstm_c", "lstm_h1", "lstm_h2", "drop_seeds", "stop_minlen",
                                           "stop_maxlen", "stop_probs", "stop_len", "stop_ndone", "W", "bias", "ln_g", "ln_b",
                                           "stop_w")] +
                [("drop_base", C.c_uint64)] +
                [(n, C.c_int32) for n in ("M", "K", "N", "ldx", "ldr", "ldy", "act")] + [("ln_eps", C.c_float)] +
                [(n, C.c_int32) for n in ("lstm_H", "lstm_ld1", "lstm_ld2", "dropout", "drop_J", "drop_j")] +
                [("drop_thr", C.c_uint32), ("drop_scale", C.c_float), ("stop_bias", C.c_float), ("stop_thr", C.c_float)] +
                [(n, C.c_int32) for n in ("stop_kind", "stop_max_steps", "stop_step")])


_lib = None


def _declare(lib):
    vp, i32, i64, f32p, i32p, i64p, cstr = (C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_char_p)
    sig = {
        "pk_last_error": (cstr, []),
        "pk_version": (cstr, []),
        "pk_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "pk_ctx_set_stream": (C.c_int, [vp, vp]),
        "pk_sync": (C.c_int, [vp]),
        "pk_ctx_destroy": (None, [vp]),
        "pk_prof_enable": (C.c_int, [vp, C.c_int]),
        "pk_prof_reset": (C.c_int, [vp]),
        "pk_prof_read": (C.c_int, [vp, cstr, C.POINTER(i64), C.POINTER(C.c_double)]),
        "pk_prof_dump": (C.c_int, [vp, C.c_char_p, i64]),
        "pk_pwg_create": (C.c_int, [vp, C.POINTER(PwgCfg), C.POINTER(vp)]),
        "pk_pwg_set_param": (C.c_int, [vp, cstr, f32p, i64p, i32]),
        "pk_pwg_set_normalizer": (C.c_int, [vp, f32p, f32p, i32]),
        "pk_randn": (C.c_int, [vp, f32p, i64, C.c_uint64, C.c_uint64, i32]),
        "pk_pwg_set_seed": (C.c_int, [vp, C.c_uint64]),
        "pk_wf_set_seed": (C.c_int, [vp, C.c_uint64]),
        "pk_pwg_set_math": (C.c_int, [vp, i32]),
        "pk_pwg_set_chunk_samples": (C.c_int, [vp, i64]),
        "pk_pwg_set_option": (C.c_int, [vp, cstr, i64]),
        "pk_pwg_scale_overshoot": (C.c_int, [vp, f32p, i32, i32p]),
        "pk_pwg_finalize": (C.c_int, [vp]),
        "pk_pwg_infer": (C.c_int, [vp, f32p, i32p, i32, f32p, f32p, i32]),
        "pk_pwg_debug_read": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_pwg_destroy": (None, [vp]),
        "pk_fs2_create": (C.c_int, [vp, C.POINTER(Fs2Cfg), C.POINTER(vp)]),
        "pk_fs2_set_param": (C.c_int, [vp, cstr, f32p, i64p, i32]),
        "pk_fs2_set_normalizer": (C.c_int, [vp, f32p, f32p, i32]),
        "pk_fs2_set_math": (C.c_int, [vp, i32]),
        "pk_fs2_set_option": (C.c_int, [vp, cstr, i64]),
        "pk_fs2_set_speakers": (C.c_int, [vp, i64p, f32p, i32]),
        "pk_fs2_set_tones": (C.c_int, [vp, i64p, i64]),
        "pk_fs2_set_targets": (C.c_int, [vp, i64p, f32p, f32p, i64]),
        "pk_fs2_read_predictions": (C.c_int, [vp, f32p, f32p, f32p, i64]),
        "pk_fs2_read_before": (C.c_int, [vp, f32p, i32]),
        "pk_fs2_finalize": (C.c_int, [vp]),
        "pk_fs2_encode": (C.c_int, [vp, i64p, i32p, i32, C.c_float, i32p]),
        "pk_fs2_decode": (C.c_int, [vp, f32p, i32]),
        "pk_fs2_set_debug": (C.c_int, [vp, i32]),
        "pk_fs2_debug_read": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_fs2_destroy": (None, [vp]),
        "pk_wf_create": (C.c_int, [vp, C.POINTER(WfCfg), C.POINTER(vp)]),
        "pk_wf_set_param": (C.c_int, [vp, cstr, f32p, i64p, i32]),
        "pk_wf_set_math": (C.c_int, [vp, i32]),
        "pk_wf_set_option": (C.c_int, [vp, cstr, i64]),
        "pk_wf_finalize": (C.c_int, [vp]),
        "pk_wf_cond_length": (C.c_int, [vp, i32, i32p, i32p]),
        "pk_wf_infer": (C.c_int, [vp, f32p, i32p, i32, f32p, f32p, i32]),
        "pk_wf_forward_length": (C.c_int, [vp, i32, i32, i32p]),
        "pk_wf_forward": (C.c_int, [vp, f32p, i32p, f32p, i32p, i32, f32p, C.c_void_p, i32]),
        "pk_wf_debug_read": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_wf_destroy": (None, [vp]),
        "pk_ss_create": (C.c_int, [vp, C.POINTER(SsCfg), C.POINTER(vp)]),
        "pk_ss_set_param": (C.c_int, [vp, cstr, f32p, i64p, i32]),
        "pk_ss_set_normalizer": (C.c_int, [vp, f32p, f32p, i32]),
        "pk_ss_set_math": (C.c_int, [vp, i32]),
        "pk_ss_finalize": (C.c_int, [vp]),
        "pk_ss_encode": (C.c_int, [vp, i64p, i64p, i32p, i32, i32p]),
        "pk_ss_encode_given": (C.c_int, [vp, i64p, i64p, i32p, i64p, i32p, i32, i32p]),
        "pk_ss_pred_durations": (C.c_int, [vp, f32p, i32]),
        "pk_ss_set_valid_tokens": (C.c_int, [vp, i32p, i32]),
        "pk_ss_duration_loss": (C.c_int, [vp, C.c_void_p, i32]),
        "pk_ss_decode": (C.c_int, [vp, f32p, i32]),
        "pk_ss_debug_read": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_ss_destroy": (None, [vp]),
        "pk_tts_create": (C.c_int, [vp, C.POINTER(TtsCfg), C.POINTER(vp)]),
        "pk_tts_set_param": (C.c_int, [vp, cstr, f32p, i64p, i32]),
        "pk_tts_set_normalizer": (C.c_int, [vp, f32p, f32p, i32]),
        "pk_tts_set_math": (C.c_int, [vp, i32]),
        "pk_tts_set_option": (C.c_int, [vp, cstr, i64]),
        "pk_tts_set_dropout": (C.c_int, [vp, i32]),
        "pk_tts_set_speakers": (C.c_int, [vp, f32p, i32]),
        "pk_tts_set_style_reference": (C.c_int, [vp, f32p, i32p, i32]),
        "pk_tts_finalize": (C.c_int, [vp]),
        "pk_tts_infer": (C.c_int, [vp, i64p, i32p, i32, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_uint64), i32,
                                   i32p]),
        "pk_tts_teacher": (C.c_int, [vp, i64p, i32p, i32, f32p, i32p, C.POINTER(C.c_uint64), i32, i32p]),
        "pk_tts_read": (C.c_int, [vp, f32p, f32p, f32p, i32]),
        "pk_tts_read_teacher": (C.c_int, [vp, f32p, f32p, i32]),
        "pk_tts_debug_read": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_tts_destroy": (None, [vp]),
        "pk_taco_create": (C.c_int, [vp, C.POINTER(TacoCfg), C.POINTER(vp)]),
        "pk_taco_set_param": (C.c_int, [vp, cstr, f32p, i64p, i32]),
        "pk_taco_set_math": (C.c_int, [vp, i32]),
        "pk_taco_set_dropout": (C.c_int, [vp, i32]),
        "pk_taco_finalize": (C.c_int, [vp]),
        "pk_taco_set_global_condition": (C.c_int, [vp, f32p, i32]),
        "pk_taco_infer": (C.c_int, [vp, i64p, i64p, i32p, i32, i32, C.POINTER(C.c_uint64), i32, i32p]),
        "pk_taco_teacher": (C.c_int, [vp, i64p, i64p, i32p, i32, f32p, i32p, C.POINTER(C.c_uint64), i32, i32p]),
        "pk_taco_read": (C.c_int, [vp, f32p, f32p, f32p, f32p, i32]),
        "pk_taco_debug_read": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_taco_destroy": (None, [vp]),
        "pk_spk_create": (C.c_int, [vp, C.POINTER(SpkCfg), C.POINTER(vp)]),
        "pk_spk_set_param": (C.c_int, [vp, cstr, f32p, i64p, i32]),
        "pk_spk_set_math": (C.c_int, [vp, i32]),
        "pk_spk_finalize": (C.c_int, [vp]),
        "pk_spk_embed": (C.c_int, [vp, f32p, i32, i32, f32p, f32p, i32p, i32, f32p]),
        "pk_spk_ge2e": (C.c_int, [vp, f32p, i32, i32, i32, f32p, f32p, f32p, C.c_void_p, C.c_void_p]),
        "pk_spk_cosine": (C.c_int, [vp, f32p, f32p, i32, i32, f32p]),
        "pk_spk_destroy": (None, [vp]),
        "pk_mel_create": (C.c_int, [vp, C.POINTER(MelCfg), f32p, f32p, C.POINTER(vp)]),
        "pk_mel_num_frames": (C.c_int, [vp, i32, i32p]),
        "pk_mel_run": (C.c_int, [vp, f32p, i32p, i32, f32p, i32, i32]),
        "pk_mel_set_transform": (C.c_int, [vp, i32]),
        "pk_mel_destroy": (None, [vp]),
        "pk_rfft_supported": (C.c_int, [i32]),
        "pk_rfft_tile_rows": (C.c_int, [i32, i32p]),
        "pk_op_rfft": (C.c_int, [vp, f32p, i64, i32, f32p]),
        "pk_op_irfft": (C.c_int, [vp, f32p, i64, i32, f32p]),
        "pk_istft_create": (C.c_int, [vp, C.POINTER(IstftCfg), f32p, C.POINTER(vp)]),
        "pk_istft_num_samples": (C.c_int, [vp, i32, i32p]),
        "pk_istft_run": (C.c_int, [vp, f32p, i32p, i32, f32p, i32]),
        "pk_gl_run": (C.c_int, [vp, vp, f32p, i32p, i32, i32, C.c_float, C.POINTER(C.c_uint64), f32p, f32p, i32]),
        "pk_gl_debug_read": (C.c_int, [vp, i32, f32p, i64]),
        "pk_istft_set_transform": (C.c_int, [vp, i32]),
        "pk_istft_destroy": (None, [vp]),
        "pk_resample_create": (C.c_int, [vp, C.POINTER(ResampleCfg), f32p, C.POINTER(vp)]),
        "pk_resample_out_len": (C.c_int, [vp, i64, i64p]),
        "pk_resample_tile_samples": (C.c_int, [vp, i32p]),
        "pk_resample_run": (C.c_int, [vp, f32p, i32p, i32, f32p, i32]),
        "pk_resample_destroy": (None, [vp]),
        "pk_pitch_create": (C.c_int, [vp, C.POINTER(PitchCfg), C.POINTER(vp)]),
        "pk_pitch_frames": (C.c_int, [vp, i64, i32p]),
        "pk_pitch_tile_frames": (C.c_int, [vp, i32p]),
        "pk_pitch_run": (C.c_int, [vp, f32p, i32p, i32, f32p, C.c_void_p, f32p, i32]),
        "pk_pitch_track_run": (C.c_int, [vp, f32p, i32p, i32, C.POINTER(PitchTrackCfg), f32p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, i32]),
        "pk_pitch_track_from_cmnd": (C.c_int, [vp, f32p, i32p, i32, C.POINTER(PitchTrackCfg), f32p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, i32]),
        "pk_pitch_set_option": (C.c_int, [vp, cstr, i64]),
        "pk_pitch_destroy": (None, [vp]),
        "pk_op_continuous_f0": (C.c_int, [vp, f32p, i32p, i32, i32, f32p]),
        "pk_trim_create": (C.c_int, [vp, C.POINTER(vp)]),
        "pk_trim_destroy": (None, [vp]),
        "pk_trim_num_frames": (C.c_int, [i64, i32, i32, i32, i64p]),
        "pk_trim_tile_frames": (C.c_int, [i32, i32, i32p]),
        "pk_trim_run": (C.c_int, [vp, f32p, i32p, i32, i32, i32, i32, C.c_double, i32, f32p, C.c_void_p, C.c_void_p]),
        "pk_vad_mask": (C.c_int, [vp, f32p, i32p, i32, i32, i32, i32, C.c_void_p, C.c_double, C.c_double, f32p, C.c_void_p,
                                  C.c_void_p, i32p]),
        "pk_vad_gather": (C.c_int, [vp, f32p, i32p, i32, i32, C.c_void_p, i32p, f32p]),
        "pk_peak_normalize": (C.c_int, [vp, f32p, i32p, i32, f32p]),
        "pk_stftd_create": (C.c_int, [vp, C.POINTER(StftdCfg), C.POINTER(StftdRes), f32p, C.POINTER(vp)]),
        "pk_stftd_num_frames": (C.c_int, [vp, i32, i32, i32p]),
        "pk_stftd_run": (C.c_int, [vp, f32p, f32p, i32p, i32, C.c_void_p, i32]),
        "pk_stftd_magnitude": (C.c_int, [vp, i32, f32p, i32p, i32, f32p, i32]),
        "pk_stftd_destroy": (None, [vp]),
        "pk_pwgd_create": (C.c_int, [vp, C.POINTER(PwgdCfg), C.POINTER(vp)]),
        "pk_pwgd_set_param": (C.c_int, [vp, cstr, f32p, i64p, i32]),
        "pk_pwgd_finalize": (C.c_int, [vp]),
        "pk_pwgd_set_math": (C.c_int, [vp, i32]),
        "pk_pwgd_tile_samples": (C.c_int, [vp, i32p, i32p]),
        "pk_pwgd_run": (C.c_int, [vp, f32p, i32p, i32, f32p, C.c_void_p, i32]),
        "pk_pwgd_set_debug": (C.c_int, [vp, i32]),
        "pk_pwgd_debug_read": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_pwgd_destroy": (None, [vp]),
        "pk_hfg_create": (C.c_int, [vp, C.POINTER(HfgCfg), C.POINTER(vp)]),
        "pk_hfg_set_param": (C.c_int, [vp, cstr, f32p, i64p, i32]),
        "pk_hfg_finalize": (C.c_int, [vp]),
        "pk_hfg_set_math": (C.c_int, [vp, i32]),
        "pk_hfg_set_normalizer": (C.c_int, [vp, f32p, f32p, i32]),
        "pk_hfg_infer": (C.c_int, [vp, f32p, i32p, i32, f32p, i32]),
        "pk_hfg_debug_read": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_hfg_debug_conv": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_hfg_destroy": (None, [vp]),
        "pk_pqmf_create": (C.c_int, [vp, C.POINTER(PqmfCfg), C.POINTER(vp)]),
        "pk_pqmf_filters": (C.c_int, [vp, f32p, f32p, i64]),
        "pk_pqmf_analysis": (C.c_int, [vp, f32p, i32p, i32, f32p, i32]),
        "pk_pqmf_synthesis": (C.c_int, [vp, f32p, i32p, i32, f32p, i32]),
        "pk_pqmf_destroy": (None, [vp]),
        "pk_mgan_create": (C.c_int, [vp, C.POINTER(MganCfg), C.POINTER(vp)]),
        "pk_mgan_set_param": (C.c_int, [vp, cstr, f32p, i64p, i32]),
        "pk_mgan_finalize": (C.c_int, [vp]),
        "pk_mgan_set_math": (C.c_int, [vp, i32]),
        "pk_mgan_set_normalizer": (C.c_int, [vp, f32p, f32p, i32]),
        "pk_mgan_min_frames": (i32, [vp]),
        "pk_mgan_set_pqmf": (C.c_int, [vp, vp]),
        "pk_mgan_infer": (C.c_int, [vp, f32p, i32p, i32, f32p, i32]),
        "pk_mgan_debug_read": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_mgan_debug_conv": (C.c_int, [vp, i32, i32, f32p, i64]),
        "pk_mgan_destroy": (None, [vp]),
        "pk_mel_loss_run": (C.c_int, [vp, f32p, f32p, i32p, i32p, i32, i32, i32, C.c_void_p, f32p, i32]),
        "pk_pair_loss_run": (C.c_int, [vp, f32p, f32p, i64p, i64p, i64, i64, i32p, i32, i32, C.c_void_p, i32]),
        "pk_bce_logits_run": (C.c_int, [vp, f32p, f32p, i64p, i64p, i32p, i32, C.c_float, C.c_void_p, i32]),
        "pk_guided_attn_run": (C.c_int, [vp, f32p, i64p, i64, i64, i32p, i32p, i32p, i32, C.c_double, C.c_void_p, i32]),
        "pk_mas_run": (C.c_int, [vp, f32p, i64p, i64, i32p, i32p, i32, i32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, f32p]),
        "pk_mas_lds_words": (C.c_int, [i32p]),
        "pk_focus_rate_run": (C.c_int, [vp, f32p, i64p, i64, i64, i32p, i32p, i32p, i32, C.c_void_p]),
        "pk_dtw_run": (C.c_int, [vp, i32, f32p, f32p, i64p, i64p, i64, i64, i32, i32, i32, i32p, i32p, i32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
        "pk_dtw_cost": (C.c_int, [vp, f32p, f32p, i64p, i64p, i64, i64, i32, i32, i32, i32p, i32p, i32, f32p]),
        "pk_dtw_lds_words": (C.c_int, [i32p]),
        "pk_dtw_cost_cap": (C.c_int, [i64, i64p]),
        "pk_dtw_path_stats": (C.c_int, [vp, C.c_void_p, C.c_void_p, C.c_void_p, f32p, f32p, i64p, i64p, i64, i64, i32, i32, i32,
                                        i32p, i32p, i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "pk_edit_run": (C.c_int, [vp, C.c_void_p, C.c_void_p, i64p, i64p, i32p, i32p, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
        "pk_edit_lds_words": (C.c_int, [i32p]),
        "pk_stoi_run": (C.c_int, [vp, f32p, f32p, i64p, i32, i32, C.c_void_p]),
        "pk_stoi_mask": (C.c_int, [vp, f32p, i64p, i32, f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "pk_stoi_bands": (C.c_int, [vp, f32p, i64p, i32, f32p]),
        "pk_stoi_segments": (C.c_int, [vp, f32p, f32p, i32p, i32, i32, C.c_void_p, C.c_void_p]),
        "pk_stoi_num_frames": (C.c_int, [i64, i64p]),
        "pk_stoi_band_edges": (C.c_int, [i32p, i32p]),
        "pk_iir_create": (C.c_int, [vp, C.POINTER(C.c_double), i32, C.POINTER(vp)]),
        "pk_iir_destroy": (None, [vp]),
        "pk_iir_transition": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "pk_iir_run": (C.c_int, [vp, f32p, i32p, i32, f32p]),
        "pk_loudness_run": (C.c_int, [vp, f32p, i32p, i32, i32, C.c_void_p, C.c_void_p, f32p, C.c_void_p]),
        "pk_gain_run": (C.c_int, [vp, f32p, i32p, i32, C.POINTER(C.c_float), f32p]),
        "pk_pvoc_num_frames": (C.c_int, [i64, C.c_double, i64p]),
        "pk_pvoc_run": (C.c_int, [vp, f32p, i32p, i32, i32, C.POINTER(C.c_double), f32p]),
        "pk_stats_create": (C.c_int, [vp, i32, C.POINTER(vp)]),
        "pk_stats_destroy": (None, [vp]),
        "pk_stats_reset": (C.c_int, [vp, f32p]),
        "pk_stats_tile_rows": (C.c_int, [i32, i32p]),
        "pk_stats_update": (C.c_int, [vp, f32p, i64p, i32, C.c_void_p, i32]),
        "pk_stats_get": (C.c_int, [vp, i64p, i32p, f32p, C.c_void_p, C.c_void_p]),
        "pk_stats_set": (C.c_int, [vp, i64, f32p, C.c_void_p, C.c_void_p]),
        "pk_op_average_by_duration":(C.c_int, [vp, f32p, i64, i32, i64p, i32, f32p]),
        "pk_op_expand": (C.c_int, [vp, f32p, i64p, i32, i32, i32, i32, f32p]),
        "pk_op_sinusoid_position_encoding": (C.c_int, [vp, i32, i32, C.c_float, i32, f32p]),
        "pk_op_scaled_dot_product_attention": (C.c_int, [vp, f32p, f32p, f32p, f32p, i32, i32, i32, i32, i32, i32,
                                                         f32p, f32p]),
        "pk_op_matmul": (C.c_int, [vp, f32p, i32, i32, i32, f32p, f32p, f32p]),
        "pk_op_conv1d_cell_step": (C.c_int, [vp, f32p, f32p, f32p, f32p, i32, i32, i32, i32, i32, f32p]),
        "pk_op_conv1d_batchnorm_nlc": (C.c_int, [vp, f32p, i32, i32, i32, i32, i32, i32, f32p, f32p, f32p, f32p,
                                                 f32p, f32p, C.c_float, f32p]),
        "pk_op_gemm": (C.c_int, [vp, C.POINTER(OpGemmCfg)]),
        "pk_op_rowgemm": (C.c_int, [vp, C.POINTER(OpRowgemmCfg)]),
        "pk_op_row_amax": (C.c_int, [vp, f32p, i64, i32, i64, i64, f32p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    return sig


def lib():
    """Load libpk_synth.so (built by parakeet_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP engine is not built "
                "(run `python -m parakeet_amd.build`); there is no CPU fallback")
        # The library must have been built from the sources next to it.  PK_ALLOW_STALE_LIB skips the check; so does an
        # install that ships the library without csrc/ or include/ (nothing to compare with).
        if not os.environ.get("PK_ALLOW_STALE_LIB"):
            from . import build as _build
            try:
                want = _build.source_hash()
            except FileNotFoundError:
                want = None
            have = _build.library_hash(LIB_PATH) if want is not None else None
            if have != want:
                raise RuntimeError(
                    f"{LIB_PATH} was built from other sources (library {str(have)[:12]}, tree {want[:12]}): "
                    "run `python -m parakeet_amd.build` (or __graft_entry__.build()); a stale engine is never used")
        _lib = C.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


def check(status):
    if status != PK_OK:
        msg = lib().pk_last_error().decode("utf-8", "replace")
        raise _EXC.get(status, RuntimeError)(f"pk_synth[{status}]: {msg}")


def fptr(arr):
    """Pointer of a C-contiguous float32 numpy array."""
    return arr.ctypes.data_as(C.c_void_p)
