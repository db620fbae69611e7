"""ctypes binding of librvcx.so (C ABI declared in include/rvcx.h).

Loading is strict: a missing library is an ImportError-grade failure (``RvcxError``) -- there
is no CPU fallback anywhere in the product path.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import types
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RVCX_LIBRARY") or os.path.join(_HERE, "librvcx.so")   # RVCX_LIBRARY: A/B runs of two builds


class RvcxError(RuntimeError):
    pass


class Tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("dtype", C.c_int32),
                ("ndim", C.c_int32), ("shape", C.c_int64 * 4)]


class SynthCfg(C.Structure):
    _fields_ = [("inter_channels", C.c_int32), ("hidden_channels", C.c_int32),
                ("filter_channels", C.c_int32), ("n_heads", C.c_int32), ("n_layers", C.c_int32),
                ("kernel_size", C.c_int32), ("n_resblocks", C.c_int32),
                ("res_kernels", C.c_int32 * 4), ("res_dilations", (C.c_int32 * 3) * 4),
                ("n_ups", C.c_int32), ("up_rates", C.c_int32 * 6), ("up_kernels", C.c_int32 * 6),
                ("up_initial_channel", C.c_int32), ("spk_embed_dim", C.c_int32),
                ("gin_channels", C.c_int32), ("sr", C.c_int32), ("input_dim", C.c_int32)]


class RmvpeCfg(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("en_de_layers", C.c_int32), ("inter_layers", C.c_int32),
                ("en_out_channels", C.c_int32)]


class FcpeCfg(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("n_chans", C.c_int32), ("input_channel", C.c_int32),
                ("out_dims", C.c_int32), ("heads", C.c_int32), ("dim_head", C.c_int32),
                ("nb_features", C.c_int32), ("dw_kernel", C.c_int32), ("mel_fmin", C.c_float),
                ("mel_fmax", C.c_float)]


class HubertCfg(C.Structure):
    _fields_ = [("conv_dim", C.c_int32), ("n_conv", C.c_int32), ("conv_kernels", C.c_int32 * 8),
                ("conv_strides", C.c_int32 * 8), ("embed_dim", C.c_int32), ("ffn_dim", C.c_int32),
                ("heads", C.c_int32), ("layers", C.c_int32), ("pos_kernel", C.c_int32),
                ("pos_groups", C.c_int32)]


class Params(C.Structure):
    _fields_ = [("pitch", C.c_float), ("f0_min", C.c_float), ("f0_max", C.c_float),
                ("index_rate", C.c_float), ("protect", C.c_float), ("volume_envelope", C.c_float),
                ("sid", C.c_int32), ("x_pad", C.c_int32), ("x_query", C.c_int32),
                ("x_center", C.c_int32), ("x_max", C.c_int32), ("seed", C.c_uint64),
                ("f0_method", C.c_int32), ("resample_sr", C.c_int32), ("hop_length", C.c_int32), ("reserved", C.c_int32)]


class UttExtra(C.Structure):
    _fields_ = [("inp_f0", C.POINTER(C.c_float)), ("inp_f0_rows", C.c_int32), ("reserved", C.c_int32),
                ("crepe_dither", C.POINTER(C.c_float)), ("crepe_dither_n", C.c_int64)]


F0_RMVPE, F0_FCPE, F0_CREPE = 0, 1, 2        # rvcx_params.f0_method


FX_FIELDS = ("reverb_rm_size", "reverb_wet", "reverb_dry", "reverb_damping", "reverb_width", "low_shelf_gain",
             "high_shelf_gain", "compressor_ratio", "compressor_threshold", "noise_gate_threshold", "noise_gate_ratio",
             "noise_gate_attack", "noise_gate_release", "chorus_rate_hz", "chorus_depth", "chorus_centre_delay_ms",
             "chorus_feedback", "chorus_mix")


class FxParams(C.Structure):
    """rvcx_fx_params: the eighteen values of add_effects (audio_processing.py:54-75) in its order, then rate and channels"""
    _fields_ = [(k, C.c_float) for k in FX_FIELDS] + [("sample_rate", C.c_int32), ("channels", C.c_int32)]

    @classmethod
    def make(cls, values, sample_rate, channels=2):
        """values: the eighteen add_effects values in order, or a dict of them"""
        p = cls()
        if isinstance(values, dict):
            values = [values[k] for k in FX_FIELDS]
        if len(values) != len(FX_FIELDS):
            raise RvcxError(f"FxParams: {len(FX_FIELDS)} effect values expected, got {len(values)}")
        for k, v in zip(FX_FIELDS, values):
            setattr(p, k, float(v))
        p.sample_rate, p.channels = int(sample_rate), int(channels)
        return p


# the processing tab's defaults (tabs/processing/processing.py): chorus off, shelves flat
FX_UI_DEFAULTS = dict(reverb_rm_size=0.1, reverb_wet=0.1, reverb_dry=0.8, reverb_damping=0.9, reverb_width=1.0,
                      low_shelf_gain=0, high_shelf_gain=0, compressor_ratio=4, compressor_threshold=-12,
                      noise_gate_threshold=-40, noise_gate_ratio=8, noise_gate_attack=10, noise_gate_release=100,
                      chorus_rate_hz=0, chorus_depth=0, chorus_centre_delay_ms=0, chorus_feedback=0, chorus_mix=0)


class StreamIO(C.Structure):
    """rvcx_stream_io: the rates at the two edges of a live-stream session (0: none on that side)"""
    _fields_ = [("in_rate", C.c_int32), ("in_channels", C.c_int32), ("out_rate", C.c_int32), ("reserved", C.c_int32)]


def stream_resample_delay(sr_in: int, sr_out: int) -> int:
    """rvcx_stream_resample_delay (host only): the delay of a session's resampler in output samples, 0 for equal rates,
    ceil(96 * max(1, sr_out / sr_in)) otherwise; -1 for rates a session refuses"""
    return int(lib().rvcx_stream_resample_delay(int(sr_in), int(sr_out)))


class StreamCfg(C.Structure):
    """rvcx_stream_cfg: the geometry of a live-stream session in 10 ms frames"""
    _fields_ = [("n_streams", C.c_int32), ("block_frames", C.c_int32), ("context_frames", C.c_int32),
                ("crossfade_frames", C.c_int32), ("search_frames", C.c_int32)]


def head_from_rate(T: int, rate) -> int:
    """head = int(z_p.shape[2] * (1.0 - rate.item())) of Synthesizer.infer (synthesizers.py:177) for a float32 `rate` tensor:
    .item() widens the float32 value to a Python float, the rest is float64.  T = 40: rate 0.3 -> 27 (not 28), 0.25 -> 30."""
    return int(int(T) * (1.0 - float(np.float32(rate))))


def sola_reference(y, b, Lb, Lx, Ls, offset=None):
    """rvcx_op_sola restated in float64 numpy (the yardstick of its tests; no GPU): (out, new carry, offset, scores, mags)
    with scores[d] = nom[d] / den[d] and mags[d] = sum |y[d+i] b[i]| / den[d] (what the rounding-error bound of a float32
    evaluation scales with).  offset: apply this one instead of the first index of the maximum."""
    y, b = np.asarray(y, np.float64), np.asarray(b, np.float64)
    Lb, Lx, Ls = int(Lb), int(Lx), int(Ls)
    assert y.shape == (Lb + Lx + Ls,) and b.shape == (Lx,)
    win = np.lib.stride_tricks.sliding_window_view(y[:Ls + Lx], Lx)          # (Ls + 1, Lx)
    den = np.sqrt((win * win).sum(1) + 1e-8)
    scores = (win @ b) / den
    mags = (np.abs(win) @ np.abs(b)) / den
    d = int(np.argmax(scores)) if offset is None else int(offset)            # argmax: the first index of the maximum
    out = y[d:d + Lb].copy()
    k = min(Lx, Lb)
    fin = np.sin(0.5 * np.pi * np.arange(Lx) / max(Lx - 1, 1)) ** 2
    out[:k] = y[d:d + k] * fin[:k] + b[:k] * (1.0 - fin[:k])
    return out, y[d + Lb:d + Lb + Lx].copy(), d, scores, mags


_lib = None

# every symbol include/rvcx.h declares (tests/test_abi.py checks the .so exports all of them)
SYMBOLS = [
    "rvcx_create", "rvcx_destroy", "rvcx_last_error", "rvcx_version", "rvcx_load_hubert",
    "rvcx_load_rmvpe", "rvcx_index_exhaustive", "rvcx_load_crepe", "rvcx_crepe_frames", "rvcx_crepe_predict", "rvcx_op_crepe_decode", "rvcx_get_f0_crepe_x", "rvcx_load_fcpe", "rvcx_fcpe_f0", "rvcx_fcpe_frames", "rvcx_get_f0_fcpe_x", "rvcx_op_fcpe_post", "rvcx_load_synth", "rvcx_unload_synth", "rvcx_load_index", "rvcx_load_index_ivf",
    "rvcx_weights_regions", "rvcx_weights_adopt", "rvcx_weights_clone", "rvcx_rmvpe_f0", "rvcx_rmvpe_frames", "rvcx_rmvpe_mel", "rvcx_synth_infer_taps", "rvcx_hubert_features",
    "rvcx_hubert_frames", "rvcx_synth_infer", "rvcx_synth_infer_window", "rvcx_synth_dec_rf", "rvcx_synth_upp", "rvcx_index_blend",
    "rvcx_out_len", "rvcx_convert_batch", "rvcx_convert_batch_f64", "rvcx_micro_batch", "rvcx_bucket_length", "rvcx_last_micro_batches", "rvcx_last_cuts", "rvcx_noise_len",
    "rvcx_get_f0", "rvcx_get_f0_x", "rvcx_vc", "rvcx_vc_frames", "rvcx_last_timing",
    "rvcx_flop_counter", "rvcx_fp32_reruns", "rvcx_mem_info", "rvcx_conv_profile", "rvcx_conv_profile_csv", "rvcx_stream", "rvcx_op_conv1d", "rvcx_op_resblock_pair", "rvcx_bench_resblock_pair", "rvcx_bench_conv1d", "rvcx_conv_override", "rvcx_op_convtranspose1d",
    "rvcx_op_conv2d3x3", "rvcx_op_convblock2d", "rvcx_op_convtranspose2d", "rvcx_op_attention", "rvcx_op_layernorm_c",
    "rvcx_op_bigru", "rvcx_op_highpass", "rvcx_highpass_exact", "rvcx_convert_batch_ex", "rvcx_get_f0_x_ex", "rvcx_fp32_layers", "rvcx_fp32_pinned",
    "rvcx_gru_fallbacks", "rvcx_gru_publish_probe", "rvcx_debug_inject", "rvcx_f0_file_track", "rvcx_op_gemm_tm", "rvcx_op_layernorm_tm",
    "rvcx_resample_len", "rvcx_resample_f64", "rvcx_resample_f64_kind", "rvcx_bench_gemm", "rvcx_device_info",
    "rvcx_convert_submit", "rvcx_convert_wait", "rvcx_convert_poll", "rvcx_convert_inflight", "rvcx_ticket_lead_ms",
    "rvcx_synth_infer_head", "rvcx_op_sola", "rvcx_stream_open", "rvcx_stream_step", "rvcx_stream_reset", "rvcx_stream_close",
    "rvcx_stream_out_len", "rvcx_stream_noise_len", "rvcx_stream_frames",
    "rvcx_stream_open_io", "rvcx_stream_in_len", "rvcx_stream_delays", "rvcx_stream_resample_delay", "rvcx_stream_last_taps",
    "rvcx_stream_set", "rvcx_op_stream_resample",
    "rvcx_stream_open_fx", "rvcx_stream_out_channels", "rvcx_stream_set_fx", "rvcx_stream_last_fx_ms", "rvcx_op_stream_fx",
    "rvcx_fx_reverb_host",
    "rvcx_fx_chain", "rvcx_op_fx_highpass", "rvcx_op_fx_compressor", "rvcx_op_fx_gate", "rvcx_op_fx_reverb", "rvcx_op_fx_shelf",
    "rvcx_op_fx_chorus", "rvcx_op_fx_mix", "rvcx_fx_chunk", "rvcx_fx_last_passes", "rvcx_fx_cte", "rvcx_fx_delay",
    "rvcx_fx_coeffs", "rvcx_fx_highpass_host", "rvcx_fx_biquad_host", "rvcx_fx_follower_host", "rvcx_fx_compressor_host",
    "rvcx_fx_gate_host", "rvcx_fx_comb_host", "rvcx_fx_allpass_host", "rvcx_fx_chorus_host", "rvcx_fx_mix_host",
    "rvcx_fx_momentary_len", "rvcx_fx_loudness", "rvcx_op_fx_truepeak", "rvcx_op_fx_limit", "rvcx_fx_master",
    "rvcx_fx_kweight_coeffs", "rvcx_fx_truepeak_taps", "rvcx_fx_loudness_host", "rvcx_fx_truepeak_host", "rvcx_fx_limit_host",
    "rvcx_fx_master_host",
    "rvcx_fx_stretch_len", "rvcx_fx_stretch_frames", "rvcx_fx_pitch_ratio", "rvcx_fx_stretch_chunk", "rvcx_fx_stretch",
    "rvcx_fx_pitch_shift", "rvcx_op_fx_stretch_taps", "rvcx_fx_stretch_host", "rvcx_fx_pitch_shift_host",
    "rvcx_fx_stretch_own_host", "rvcx_fx_stretch_override",
    "rvcx_fx_denoise_frames", "rvcx_fx_denoise_tiles", "rvcx_fx_denoise", "rvcx_op_fx_denoise_taps", "rvcx_fx_denoise_host",
    "rvcx_fx_denoise_smooth_host",
    "rvcx_stream_denoise_delay", "rvcx_stream_denoise_frames", "rvcx_stream_open_dn", "rvcx_stream_set_denoise",
    "rvcx_stream_last_dn_ms", "rvcx_op_stream_denoise", "rvcx_fx_denoise_live_host",
    "rvcx_fx_formant_frames", "rvcx_fx_formant", "rvcx_fx_pitch_shift_formant", "rvcx_op_fx_formant_taps",
    "rvcx_fx_formant_host", "rvcx_fx_pitch_shift_formant_host", "rvcx_fx_formant_envelope_host",
    "rvcx_stream_formant_delay", "rvcx_stream_formant_frames", "rvcx_stream_open_fm", "rvcx_stream_set_formant",
    "rvcx_stream_last_fm_ms", "rvcx_op_stream_formant", "rvcx_op_stream_formant_history", "rvcx_fx_formant_live_host",
    "rvcx_op_groupnorm_gelu", "rvcx_op_hubert_conv0", "rvcx_op_sine_source", "rvcx_op_randn", "rvcx_op_reflect_pad",
    "rvcx_op_mel_post", "rvcx_op_decode_f0", "rvcx_op_avgpool2", "rvcx_op_gru_input", "rvcx_op_upsample_protect",
    "rvcx_kmeans", "rvcx_ivf_assign", "rvcx_kmeans_exhaustive", "rvcx_index_features",
    "rvcx_op_resblock3", "rvcx_flac_encode_bound", "rvcx_flac_encode_s16", "rvcx_flac_info", "rvcx_flac_decode_s32", "rvcx_flac_last_error",
]


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RvcxError(f"{LIB_PATH} not built (run `make` / __graft_entry__.build()); "
                            "rvcx has no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _lib.rvcx_last_error.restype = C.c_char_p
        _lib.rvcx_version.restype = C.c_char_p
        _lib.rvcx_flop_counter.restype = C.c_double
        _lib.rvcx_stream.restype = C.c_void_p
        _lib.rvcx_conv_profile_csv.restype = C.c_char_p
        _lib.rvcx_out_len.restype = C.c_int64
        _lib.rvcx_fp32_reruns.restype = C.c_int64
        _lib.rvcx_fp32_layers.restype = C.c_int64
        _lib.rvcx_gru_fallbacks.restype = C.c_int64
        _lib.rvcx_bucket_length.restype = C.c_int64
        _lib.rvcx_last_cuts.restype = C.c_int64
        _lib.rvcx_last_cuts.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        _lib.rvcx_resample_len.restype = C.c_int64
        _lib.rvcx_noise_len.restype = C.c_int64
        _lib.rvcx_crepe_frames.restype = C.c_int64
        _lib.rvcx_index_exhaustive.restype = C.c_int64
        _lib.rvcx_kmeans_exhaustive.restype = C.c_int64
        _lib.rvcx_kmeans.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.rvcx_ivf_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _lib.rvcx_flac_encode_bound.restype = C.c_int64
        _lib.rvcx_flac_encode_s16.restype = C.c_int64
        _lib.rvcx_flac_decode_s32.restype = C.c_int64
        _lib.rvcx_flac_last_error.restype = C.c_char_p
        _lib.rvcx_flac_encode_bound.argtypes = [C.c_int64, C.c_int]
        _lib.rvcx_flac_encode_s16.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64]
        _lib.rvcx_flac_info.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        _lib.rvcx_flac_decode_s32.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        _lib.rvcx_convert_submit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(C.c_int64)]
        _lib.rvcx_convert_wait.argtypes = [C.c_void_p, C.c_int64]
        _lib.rvcx_convert_poll.argtypes = [C.c_void_p, C.c_int64]
        _lib.rvcx_convert_inflight.argtypes = [C.c_void_p]
        _lib.rvcx_ticket_lead_ms.argtypes = [C.c_void_p, C.c_int64]
        _lib.rvcx_ticket_lead_ms.restype = C.c_float
        _lib.rvcx_stream_out_len.restype = C.c_int64
        _lib.rvcx_stream_noise_len.restype = C.c_int64
        _lib.rvcx_stream_out_len.argtypes = [C.c_void_p, C.c_int]
        _lib.rvcx_stream_noise_len.argtypes = [C.c_void_p, C.c_int]
        _lib.rvcx_stream_frames.argtypes = [C.c_void_p, C.c_int]
        _lib.rvcx_stream_in_len.restype = C.c_int64
        _lib.rvcx_stream_in_len.argtypes = [C.c_void_p, C.c_int]
        _lib.rvcx_stream_resample_delay.argtypes = [C.c_int, C.c_int]
        _lib.rvcx_stream_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float]
        _lib.rvcx_op_stream_resample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p]
        fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
        _lib.rvcx_op_groupnorm_gelu.argtypes = [vp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, ip, fp, fp, fp]
        _lib.rvcx_op_hubert_conv0.argtypes = [vp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, ip,
                                              C.c_int, fp, fp, C.POINTER(C.c_uint16)]
        _lib.rvcx_op_sine_source.argtypes = [vp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, ip, fp]
        _lib.rvcx_op_randn.argtypes = [vp, C.c_int64, C.c_uint64, C.c_uint64, fp]
        _lib.rvcx_op_reflect_pad.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, ip, fp]
        _lib.rvcx_op_mel_post.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp, ip, ip, fp]
        _lib.rvcx_op_decode_f0.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, fp]
        _lib.rvcx_op_avgpool2.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, fp]
        _lib.rvcx_op_gru_input.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp]
        _lib.rvcx_op_upsample_protect.argtypes = [vp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int,
                                                  C.c_int, fp]
        f, d, i, i64 = C.c_float, C.c_double, C.c_int, C.c_int64
        _lib.rvcx_fx_chain.argtypes = [vp, i, vp, vp, C.POINTER(FxParams), vp]
        _lib.rvcx_op_fx_highpass.argtypes = [vp, vp, i64, i, i, f, vp]
        _lib.rvcx_op_fx_compressor.argtypes = [vp, vp, i64, i, i, f, f, f, f, vp, vp]
        _lib.rvcx_op_fx_gate.argtypes = [vp, vp, i64, i, i, f, f, f, f, vp, vp]
        _lib.rvcx_op_fx_reverb.argtypes = [vp, vp, i64, i, i, f, f, f, f, f, vp]
        _lib.rvcx_op_fx_shelf.argtypes = [vp, vp, i64, i, i, i, f, f, f, vp]
        _lib.rvcx_op_fx_chorus.argtypes = [vp, vp, i64, i, i, f, f, f, f, f, vp]
        _lib.rvcx_op_fx_mix.argtypes = [vp, vp, i64, vp, i64, f, f, vp]
        _lib.rvcx_fx_last_passes.argtypes = [vp, vp]
        _lib.rvcx_fx_cte.argtypes, _lib.rvcx_fx_cte.restype = [d, i], f
        _lib.rvcx_fx_delay.argtypes = [i, i]
        _lib.rvcx_fx_coeffs.argtypes = [i, i, d, d, d, vp]
        _lib.rvcx_fx_highpass_host.argtypes = [vp, i64, i, f, vp]
        _lib.rvcx_fx_biquad_host.argtypes = [vp, i64, vp, vp]
        _lib.rvcx_fx_follower_host.argtypes = [vp, i64, i, i, f, f, vp]
        _lib.rvcx_fx_compressor_host.argtypes = [vp, i64, i, f, f, f, f, vp, vp]
        _lib.rvcx_fx_gate_host.argtypes = [vp, i64, i, f, f, f, f, vp, vp]
        _lib.rvcx_fx_comb_host.argtypes = [vp, i64, i, f, f, vp]
        _lib.rvcx_fx_allpass_host.argtypes = [vp, i64, i, vp]
        _lib.rvcx_fx_chorus_host.argtypes = [vp, i64, i, f, f, f, f, f, vp]
        _lib.rvcx_fx_mix_host.argtypes = [vp, i64, vp, i64, f, f, vp]
        _lib.rvcx_fx_reverb_host.argtypes = [vp, i64, i, f, f, f, f, f, vp]
        _lib.rvcx_stream_open_fx.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp]
        _lib.rvcx_stream_out_channels.argtypes = [vp, i]
        _lib.rvcx_stream_set_fx.argtypes = [vp, i, vp]
        _lib.rvcx_stream_last_fx_ms.argtypes = [vp, i, vp]
        _lib.rvcx_op_stream_fx.argtypes = [vp, vp, i, i64, i, i, i, vp, C.c_uint32, vp]
        _lib.rvcx_fx_momentary_len.argtypes, _lib.rvcx_fx_momentary_len.restype = [i64, i], i64
        _lib.rvcx_fx_loudness.argtypes = [vp, i, vp, vp, i, i, vp, vp, vp]
        _lib.rvcx_op_fx_truepeak.argtypes = [vp, vp, i64, i, vp, vp]
        _lib.rvcx_op_fx_limit.argtypes = [vp, vp, i64, i, i, f, f, f, vp, vp]
        _lib.rvcx_fx_master.argtypes = [vp, i, vp, vp, vp, vp, i, d, d, d, vp, vp]
        _lib.rvcx_fx_kweight_coeffs.argtypes = [i, vp]
        _lib.rvcx_fx_truepeak_taps.argtypes = [vp]
        _lib.rvcx_fx_loudness_host.argtypes = [vp, i64, i, i, vp, vp]
        _lib.rvcx_fx_truepeak_host.argtypes = [vp, i64, i, vp, vp]
        _lib.rvcx_fx_limit_host.argtypes = [vp, i64, i, i, f, f, f, vp, vp]
        _lib.rvcx_fx_master_host.argtypes = [vp, i64, vp, i64, i, d, d, d, vp, vp]
        _lib.rvcx_fx_stretch_len.argtypes, _lib.rvcx_fx_stretch_len.restype = [i64, i64, i64], i64
        _lib.rvcx_fx_stretch_frames.argtypes = [i64, i, i64, i64, vp, vp, vp]
        _lib.rvcx_fx_pitch_ratio.argtypes, _lib.rvcx_fx_pitch_ratio.restype = [i, d], i64
        _lib.rvcx_fx_stretch.argtypes = [vp, i, vp, vp, i, i, i64, i64, vp]
        _lib.rvcx_fx_pitch_shift.argtypes = [vp, i, vp, vp, i, i, d, vp]
        _lib.rvcx_op_fx_stretch_taps.argtypes = [vp, vp, i64, i, i64, i64, vp, vp, vp, vp, vp]
        _lib.rvcx_fx_stretch_host.argtypes = [vp, i64, i, i, i64, i64, vp, vp, vp, vp, vp]
        _lib.rvcx_fx_pitch_shift_host.argtypes = [vp, i64, i, i, d, vp, vp, vp, vp, vp]
        _lib.rvcx_fx_stretch_own_host.argtypes = [vp, i, vp]
        _lib.rvcx_fx_stretch_override.argtypes = [i, i]
        _lib.rvcx_fx_denoise_frames.argtypes = [i64, i, vp, vp, vp, vp]
        _lib.rvcx_fx_denoise_tiles.argtypes = [vp, vp, vp]
        _lib.rvcx_fx_denoise.argtypes = [vp, i, vp, vp, vp, vp, vp, vp]
        _lib.rvcx_op_fx_denoise_taps.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib.rvcx_fx_denoise_host.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib.rvcx_fx_denoise_smooth_host.argtypes = [vp, i64, i, i, i, vp]
        _lib.rvcx_stream_denoise_delay.argtypes = [i]
        _lib.rvcx_stream_denoise_frames.argtypes = [i64, i, f, f, vp, vp, vp, vp]
        _lib.rvcx_stream_open_dn.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib.rvcx_stream_set_denoise.argtypes = [vp, i, i, vp]
        _lib.rvcx_stream_last_dn_ms.argtypes = [vp, i, vp]
        _lib.rvcx_op_stream_denoise.argtypes = [vp, vp, i, i64, i, i, vp, vp, i64, vp, vp, vp, vp]
        _lib.rvcx_fx_denoise_live_host.argtypes = [vp, i64, i, vp, i64, vp, vp, vp, vp, vp, vp]
        _lib.rvcx_fx_formant_frames.argtypes = [i64, i, f, vp, vp, vp]
        _lib.rvcx_fx_formant.argtypes = [vp, i, vp, vp, vp, vp, vp]
        _lib.rvcx_fx_pitch_shift_formant.argtypes = [vp, i, vp, vp, i, i, d, vp, vp]
        _lib.rvcx_op_fx_formant_taps.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib.rvcx_fx_formant_host.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib.rvcx_fx_pitch_shift_formant_host.argtypes = [vp, i64, i, i, d, vp, vp]
        _lib.rvcx_fx_formant_envelope_host.argtypes = [vp, i, i, i, vp]
        _lib.rvcx_stream_formant_delay.argtypes = [i]
        _lib.rvcx_stream_formant_frames.argtypes = [i64, i, f, vp, vp, vp]
        _lib.rvcx_stream_open_fm.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib.rvcx_stream_set_formant.argtypes = [vp, i, i, vp]
        _lib.rvcx_stream_last_fm_ms.argtypes = [vp, i, vp]
        _lib.rvcx_op_stream_formant.argtypes = [vp, vp, i, i64, i, i, vp, vp, vp, vp, vp]
        _lib.rvcx_op_stream_formant_history.argtypes = [vp, vp, i, i64, i, i, i, vp, vp, vp, vp, vp, vp]
        _lib.rvcx_fx_formant_live_host.argtypes = [vp, i64, i, vp, vp, vp, vp, vp, vp]
    return _lib


# ---- post-production on the host (rvcx.h "post-production": no GPU, no context; one channel, float32, sequential) ----------
def _fx_host(name, rc):
    if rc != 0:
        raise RvcxError(f"{name}: " + (lib().rvcx_last_error(None) or b"").decode())


def fx_chunk() -> int:
    """samples per chunk of the scan and follower kernels"""
    return int(lib().rvcx_fx_chunk())


def fx_cte(ms: float, sr: int) -> np.float32:
    return np.float32(lib().rvcx_fx_cte(float(ms), int(sr)))


def fx_delay(sr: int, D: int) -> int:
    return int(lib().rvcx_fx_delay(int(sr), int(D)))


def fx_coeffs(kind: int, sr: int, fc: float, Q: float = 2.0 ** -0.5, gain_db: float = 0.0) -> np.ndarray:
    """float32 {b0, b1, b2, a1, a2}: kind 0 the first-order high-pass, 1 the low shelf, 2 the high shelf"""
    c = np.zeros(5, np.float32)
    _fx_host("fx_coeffs", lib().rvcx_fx_coeffs(int(kind), int(sr), float(fc), float(Q), float(gain_db), c.ctypes.data))
    return c


def _fx_out(x, y):
    return np.empty_like(x) if y is None else y


def fx_highpass_host(x, sr, fc=50.0, out=None):
    x = f32(x)
    y = _fx_out(x, out)
    _fx_host("fx_highpass_host", lib().rvcx_fx_highpass_host(x.ctypes.data, x.shape[0], int(sr), float(fc), y.ctypes.data))
    return y


def fx_biquad_host(x, coef5):
    x, c = f32(x), f32(coef5)
    y = np.empty_like(x)
    _fx_host("fx_biquad_host", lib().rvcx_fx_biquad_host(x.ctypes.data, x.shape[0], c.ctypes.data, y.ctypes.data))
    return y


def fx_follower_host(x, c_attack, c_release, square=False, sqrt_out=False, out=None):
    x = f32(x)
    y = _fx_out(x, out)
    _fx_host("fx_follower_host", lib().rvcx_fx_follower_host(x.ctypes.data, x.shape[0], int(square), int(sqrt_out),
                                                             float(c_attack), float(c_release), y.ctypes.data))
    return y


def fx_compressor_host(x, sr, ratio, threshold_db, attack_ms=1.0, release_ms=100.0, out=None):
    """(y, envelope) of stage 2 on one channel"""
    x = f32(x)
    y, e = _fx_out(x, out), np.zeros_like(x)
    _fx_host("fx_compressor_host", lib().rvcx_fx_compressor_host(x.ctypes.data, x.shape[0], int(sr), float(ratio),
                                                                 float(threshold_db), float(attack_ms), float(release_ms),
                                                                 y.ctypes.data, e.ctypes.data))
    return y, e


def fx_gate_host(x, sr, threshold_db, ratio, attack_ms, release_ms, out=None):
    """(y, envelope) of stage 3 on one channel"""
    x = f32(x)
    y, e = _fx_out(x, out), np.zeros_like(x)
    _fx_host("fx_gate_host", lib().rvcx_fx_gate_host(x.ctypes.data, x.shape[0], int(sr), float(threshold_db), float(ratio),
                                                     float(attack_ms), float(release_ms), y.ctypes.data, e.ctypes.data))
    return y, e


def fx_comb_host(x, D, fb, d):
    x = f32(x)
    y = np.empty_like(x)
    _fx_host("fx_comb_host", lib().rvcx_fx_comb_host(x.ctypes.data, x.shape[0], int(D), float(fb), float(d), y.ctypes.data))
    return y


def fx_allpass_host(x, D):
    x = f32(x)
    y = np.empty_like(x)
    _fx_host("fx_allpass_host", lib().rvcx_fx_allpass_host(x.ctypes.data, x.shape[0], int(D), y.ctypes.data))
    return y


def fx_chorus_host(x, sr, rate_hz, depth, centre_delay_ms, feedback, mix, out=None):
    x = f32(x)
    y = _fx_out(x, out)
    _fx_host("fx_chorus_host", lib().rvcx_fx_chorus_host(x.ctypes.data, x.shape[0], int(sr), float(rate_hz), float(depth),
                                                         float(centre_delay_ms), float(feedback), float(mix), y.ctypes.data))
    return y


def fx_reverb_host(x, sr, room_size, damping, wet, dry, width):
    """rvcx_fx_reverb_host: stage 4 on one stereo item (n, 2), sequentially in float32 -- what a live session's reverb
    equals bit for bit"""
    x = f32(x)
    if x.ndim != 2 or x.shape[1] != 2:
        raise RvcxError("fx_reverb_host: a stereo item of shape (frames, 2) expected")
    y = np.empty_like(x)
    _fx_host("fx_reverb_host", lib().rvcx_fx_reverb_host(x.ctypes.data, x.shape[0], int(sr), float(room_size), float(damping),
                                                         float(wet), float(dry), float(width), y.ctypes.data))
    return y


def fx_values(effects, base=None) -> dict:
    """the eighteen add_effects values as a dict: `effects` (a dict of some of them, or an FxParams) laid over `base`
    (FX_UI_DEFAULTS when None).  An unknown name is refused."""
    if isinstance(effects, FxParams):
        return {k: float(getattr(effects, k)) for k in FX_FIELDS}
    out = dict(FX_UI_DEFAULTS if base is None else base)
    unknown = sorted(set(effects) - set(FX_FIELDS))
    if unknown:
        raise RvcxError(f"effects: unknown name(s) {unknown}; the names are those of add_effects: {list(FX_FIELDS)}")
    out.update({k: float(v) for k, v in effects.items()})
    return out


def _stereo_i16(a, what):
    a = np.ascontiguousarray(a)
    if a.dtype != np.int16 or a.ndim != 2 or a.shape[1] != 2:
        raise RvcxError(f"{what}: int16 array of shape (frames, 2) expected")
    return a


def fx_mix_host(vocal, inst, vocal_gain_db=0.0, inst_gain_db=0.0, out=None):
    v, m = _stereo_i16(vocal, "fx_mix_host"), _stereo_i16(inst, "fx_mix_host")
    y = _fx_out(v, out)
    _fx_host("fx_mix_host", lib().rvcx_fx_mix_host(v.ctypes.data, v.shape[0], m.ctypes.data, m.shape[0], float(vocal_gain_db),
                                                   float(inst_gain_db), y.ctypes.data))
    return y


# ---- loudness, true peak, limiter, master on the host (rvcx.h stages 9 - 12) --------------------------------------------------
MASTER_REPORT = ("vocal_lufs", "instrumental_lufs", "mix_lufs", "lufs", "true_peak_in_db", "true_peak_db", "min_gain")


def _fx_sig(x, what):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim not in (1, 2) or (x.ndim == 2 and x.shape[1] not in (1, 2)):
        raise RvcxError(f"{what}: float array of shape (frames,) or (frames, 1 or 2) expected")
    return x, (1 if x.ndim == 1 else x.shape[1])


def _stereo_f32(a, what):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 2:
        raise RvcxError(f"{what}: float array of shape (frames, 2) expected")
    return a


def fx_momentary_len(n: int, sr: int) -> int:
    """blocks of 400 ms at 75 % overlap in n frames"""
    return int(lib().rvcx_fx_momentary_len(int(n), int(sr)))


def fx_kweight_coeffs(sr: int) -> np.ndarray:
    """float64 {shelf b0, b1, b2, a1, a2, high-pass b0, b1, b2, a1, a2} of the K-weighting filter"""
    c = np.zeros(10, np.float64)
    _fx_host("fx_kweight_coeffs", lib().rvcx_fx_kweight_coeffs(int(sr), c.ctypes.data))
    return c


def fx_truepeak_taps() -> np.ndarray:
    """float32 (3, 24): phases 1 - 3 of the 4x interpolator; tap j of a phase multiplies x[n + 12 - j]"""
    t = np.zeros((3, 24), np.float32)
    _fx_host("fx_truepeak_taps", lib().rvcx_fx_truepeak_taps(t.ctypes.data))
    return t


def fx_loudness_host(x, sr, momentary=False):
    """stage 9 sequentially -> LUFS (float, -inf without a block), or (LUFS, float32 momentary values)"""
    x, ch = _fx_sig(x, "fx_loudness_host")
    L = C.c_double()
    m = np.zeros(max(fx_momentary_len(x.shape[0], sr), 1), np.float32) if momentary else None
    _fx_host("fx_loudness_host", lib().rvcx_fx_loudness_host(x.ctypes.data, x.shape[0], ch, int(sr), C.byref(L),
                                                             None if m is None else m.ctypes.data))
    return (L.value, m[:fx_momentary_len(x.shape[0], sr)]) if momentary else L.value


def fx_truepeak_host(x, want_p=False):
    """stage 10 sequentially -> dBTP, or (dBTP, p[n])"""
    x, ch = _fx_sig(x, "fx_truepeak_host")
    tp = C.c_double()
    p = np.zeros(max(x.shape[0], 1), np.float32) if want_p else None
    _fx_host("fx_truepeak_host", lib().rvcx_fx_truepeak_host(x.ctypes.data, x.shape[0], ch, None if p is None else p.ctypes.data,
                                                             C.byref(tp)))
    return (tp.value, p[:x.shape[0]]) if want_p else tp.value


def fx_limit_host(x, sr, ceiling_db=-1.0, lookahead_ms=2.0, release_ms=100.0, out=None):
    """stage 11 sequentially -> (y, s[n])"""
    x, ch = _fx_sig(x, "fx_limit_host")
    y, g = _fx_out(x, out), np.ones(max(x.shape[0], 1), np.float32)
    _fx_host("fx_limit_host", lib().rvcx_fx_limit_host(x.ctypes.data, x.shape[0], ch, int(sr), float(ceiling_db),
                                                       float(lookahead_ms), float(release_ms), y.ctypes.data, g.ctypes.data))
    return y, g[:x.shape[0]]


def fx_master_host(vocal, inst, sr, target_lufs=-16.0, vocal_offset_lu=0.0, ceiling_dbtp=-1.0, out=None):
    """stage 12 sequentially -> ((n_v, 2) int16, report dict)"""
    v, m = _stereo_f32(vocal, "fx_master_host"), _stereo_f32(inst, "fx_master_host")
    y = np.zeros((v.shape[0], 2), np.int16) if out is None else out
    rep = np.zeros(7, np.float64)
    _fx_host("fx_master_host", lib().rvcx_fx_master_host(v.ctypes.data, v.shape[0], m.ctypes.data, m.shape[0], int(sr),
                                                         float(target_lufs), float(vocal_offset_lu), float(ceiling_dbtp),
                                                         y.ctypes.data, rep.ctypes.data))
    return y, dict(zip(MASTER_REPORT, (float(r) for r in rep)))


# ---- time stretch and pitch shift on the host (rvcx.h stages 13 and 14) ---------------------------------------------------------
def fx_stretch_chunk() -> int:
    """output frames per chunk of the stage-13 scan"""
    return int(lib().rvcx_fx_stretch_chunk())


def fx_stretch_len(n: int, P: int, Q: int) -> int:
    """samples stage 13 returns for n: floor((n P + floor(Q / 2)) / Q); -1 for a refused ratio"""
    return int(lib().rvcx_fx_stretch_len(int(n), int(P), int(Q)))


def fx_stretch_frames(n: int, sr: int, P: int, Q: int):
    """(T analysis frames, J output frames, N) of stage 13"""
    T, J, N = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    _fx_host("fx_stretch_frames", lib().rvcx_fx_stretch_frames(int(n), int(sr), int(P), int(Q), C.byref(T), C.byref(J), C.byref(N)))
    return int(T.value), int(J.value), int(N.value)


def fx_pitch_ratio(sr: int, semitones: float) -> int:
    """P of stage 14 (Q = sr): floor(sr 2^(s / 12) + 0.5); -1 when refused"""
    return int(lib().rvcx_fx_pitch_ratio(int(sr), float(semitones)))


def fx_stretch_override(chunk_frames: int = 0, segment_frames: int = 0):
    """test hook (RVCX_DEBUG=1): chunk and segment length of stage 13 in output frames; 0 = the default"""
    if lib().rvcx_fx_stretch_override(int(chunk_frames), int(segment_frames)) != 0:
        raise RvcxError("fx_stretch_override: " + (lib().rvcx_last_error(None) or b"").decode())


def _stretch_taps(n, sr, P, Q, want):
    """arrays for the optional outputs D, own, TH, R of one channel"""
    if not want:
        return {}
    T, J, N = fx_stretch_frames(n, sr, P, Q)
    nb = N // 2 + 1
    return dict(D=np.zeros((T + 2, nb, 2), np.float32), own=np.zeros((T + 2, nb), np.int32), TH=np.zeros((T + 2, nb), np.uint32),
                R=np.zeros((J, nb), np.uint32))


def _tap_ptrs(t):
    return [t[k].ctypes.data if k in t else None for k in ("D", "own", "TH", "R")]


def fx_stretch_host(x, sr, P, Q, taps=False):
    """stage 13 on the host (FFT and synthesis in double) -> y, or (y, dict of D, own, TH, R) for a one-channel signal"""
    x, ch = _fx_sig(x, "fx_stretch_host")
    n = x.shape[0]
    ns = max(fx_stretch_len(n, P, Q), 0)
    y = np.zeros((ns,) + x.shape[1:], np.float32)
    t = _stretch_taps(n, sr, P, Q, taps)
    _fx_host("fx_stretch_host", lib().rvcx_fx_stretch_host(x.ctypes.data, n, ch, int(sr), int(P), int(Q), y.ctypes.data,
                                                           *_tap_ptrs(t)))
    return (y, t) if taps else y


def fx_pitch_shift_host(x, sr, semitones, taps=False):
    """stage 14 on the host -> y of x's shape, or (y, taps of its stage 13) for a one-channel signal"""
    x, ch = _fx_sig(x, "fx_pitch_shift_host")
    n = x.shape[0]
    y = np.zeros_like(x)
    P = fx_pitch_ratio(sr, semitones)
    t = _stretch_taps(n, sr, P, sr, taps) if P > 0 and P != sr else {}
    _fx_host("fx_pitch_shift_host", lib().rvcx_fx_pitch_shift_host(x.ctypes.data, n, ch, int(sr), float(semitones), y.ctypes.data,
                                                                   *_tap_ptrs(t)))
    return (y, t) if taps else y


def fx_stretch_own_host(D):
    """own of one frame (13.2) from its float32 spectrum: D (nb, 2) float pairs or a complex array of nb bins"""
    D = np.asarray(D)
    if np.iscomplexobj(D):
        D = np.stack([D.real, D.imag], axis=-1)
    D = np.ascontiguousarray(D, dtype=np.float32)
    own = np.zeros(D.shape[0], np.int32)
    _fx_host("fx_stretch_own_host", lib().rvcx_fx_stretch_own_host(D.ctypes.data, D.shape[0], own.ctypes.data))
    return own


# ---- noise reduction on the host (rvcx.h stage 15) -------------------------------------------------------------------------------
class FxDenoiseParams(C.Structure):
    """rvcx_fx_denoise_params; make() fills the defaults of include/rvcx.h stage 15"""
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("mode", C.c_int32), ("strength", C.c_float),
                ("n_std", C.c_float), ("knee_db", C.c_float), ("thresh_mult", C.c_float), ("slope", C.c_float),
                ("time_constant_s", C.c_float), ("freq_smooth_hz", C.c_float), ("time_smooth_ms", C.c_float)]
    DEFAULTS = dict(mode=1, strength=0.7, n_std=3.0, knee_db=1.0, thresh_mult=1.0, slope=5.0, time_constant_s=2.0,
                    freq_smooth_hz=500.0, time_smooth_ms=50.0)
    MODES = {"profile": 0, "adaptive": 1}

    @classmethod
    def make(cls, sr, channels=1, **values):
        unknown = set(values) - set(cls.DEFAULTS)
        if unknown:
            raise RvcxError(f"FxDenoiseParams: unknown value(s) {sorted(unknown)}")
        v = dict(cls.DEFAULTS, **values)
        v["mode"] = cls.MODES.get(v["mode"], v["mode"])
        return cls(int(sr), int(channels), int(v["mode"]), *[float(v[k]) for k in list(cls.DEFAULTS)[1:]])

    def with_shape(self, sr, channels):
        return type(self)(int(sr), int(channels), *[getattr(self, k) for k in self.DEFAULTS])


def fx_denoise_frames(n: int, sr: int):
    """(T frames, N, nf, nt) of stage 15 for n frames at sr; nf and nt are those of the default smoothing widths"""
    T, N, nf, nt = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _fx_host("fx_denoise_frames", lib().rvcx_fx_denoise_frames(int(n), int(sr), C.byref(T), C.byref(N), C.byref(nf), C.byref(nt)))
    return int(T.value), int(N.value), int(nf.value), int(nt.value)


def fx_denoise_tiles():
    """(frames per smoothing tile, bins per smoothing tile, profile frames per partial sum of the statistics)"""
    a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    lib().rvcx_fx_denoise_tiles(C.byref(a), C.byref(b), C.byref(c))
    return int(a.value), int(b.value), int(c.value)


def _denoise_taps(n, params, want):
    """arrays for the optional outputs of one channel: D, S, m and mu, sd (mode 0) or b (mode 1)"""
    if not want:
        return {}
    T, N, _, _ = fx_denoise_frames(n, params.sample_rate)
    nb = N // 2 + 1
    t = dict(D=np.zeros((T, nb, 2), np.float32), S=np.zeros((T, nb), np.float32), m=np.zeros((T, nb), np.float32))
    if params.mode == 0:
        t.update(mu=np.zeros(nb, np.float64), sd=np.zeros(nb, np.float64))
    elif params.mode == 1:
        t.update(b=np.zeros((T, nb), np.float64))
    return t


def _denoise_tap_ptrs(t):
    return [t[k].ctypes.data if k in t else None for k in ("D", "S", "mu", "sd", "b", "m")]


def _denoise_clip(noise, ch, what):
    """a noise clip as float32 of the item's channel count, or None"""
    if noise is None:
        return None
    z, zc = _fx_sig(noise, what)
    if zc != ch:
        raise RvcxError(f"{what}: the noise clip has {zc} channel(s), the item {ch}")
    if z.shape[0] < 1:
        raise RvcxError(f"{what}: a noise clip needs at least one frame")
    return z


def fx_denoise_host(x, sr, params=None, noise=None, taps=False):
    """stage 15 on the host (transforms and synthesis in double) -> y, or (y, dict of taps) for a one-channel signal"""
    x, ch = _fx_sig(x, "fx_denoise_host")
    p = (params or FxDenoiseParams.make(sr, ch)).with_shape(sr, ch)
    z = _denoise_clip(noise, ch, "fx_denoise_host")
    y = np.zeros_like(x)
    t = _denoise_taps(x.shape[0], p, taps)
    _fx_host("fx_denoise_host", lib().rvcx_fx_denoise_host(x.ctypes.data, x.shape[0], None if z is None else z.ctypes.data,
                                                           0 if z is None else z.shape[0], C.byref(p), y.ctypes.data,
                                                           *_denoise_tap_ptrs(t)))
    return (y, t) if taps else y


def fx_denoise_smooth_host(A2, nf, nt):
    """the smoothing of stage 15 alone on a (T, nb) float32 array"""
    A2 = np.ascontiguousarray(A2, dtype=np.float32)
    if A2.ndim != 2:
        raise RvcxError("fx_denoise_smooth_host: an array of shape (T, nb) expected")
    S = np.zeros_like(A2)
    _fx_host("fx_denoise_smooth_host", lib().rvcx_fx_denoise_smooth_host(A2.ctypes.data, A2.shape[0], A2.shape[1], int(nf), int(nt),
                                                                         S.ctypes.data))
    return S


# ---- formant shift and formant-preserving pitch shift on the host (rvcx.h stages 17 and 18) ------------------------------------
class FxFormantParams(C.Structure):
    """rvcx_fx_formant_params; make() fills the defaults of include/rvcx.h stage 17 (semitones= sets ratio = 2^(s / 12))"""
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("ratio", C.c_float), ("amount", C.c_float),
                ("quefrency_ms", C.c_float), ("iterations", C.c_int32), ("max_gain_db", C.c_float), ("keep_energy", C.c_int32)]
    DEFAULTS = dict(ratio=1.0, amount=1.0, quefrency_ms=1.5, iterations=8, max_gain_db=24.0, keep_energy=1)
    INTS = ("iterations", "keep_energy")

    @classmethod
    def make(cls, sr, channels=1, **values):
        if "semitones" in values:
            if "ratio" in values:
                raise RvcxError("FxFormantParams: ratio or semitones, not both")
            values["ratio"] = formant_ratio(values.pop("semitones"))
        unknown = set(values) - set(cls.DEFAULTS)
        if unknown:
            raise RvcxError(f"FxFormantParams: unknown value(s) {sorted(unknown)}")
        v = dict(cls.DEFAULTS, **values)
        for k in cls.INTS:
            if int(v[k]) != v[k]:
                raise RvcxError(f"FxFormantParams: {k} must be an integer")
        return cls(int(sr), int(channels), *[(int if k in cls.INTS else float)(v[k]) for k in cls.DEFAULTS])

    def with_shape(self, sr, channels):
        return type(self)(int(sr), int(channels), *[getattr(self, k) for k in self.DEFAULTS])


def formant_ratio(semitones) -> float:
    """ratio of stage 17 for a move of the formants by `semitones`: 2^(s / 12), |s| <= 12"""
    s = float(semitones)
    if not np.isfinite(s) or abs(s) > 12.0:
        raise RvcxError("formant_ratio: semitones must lie in -12 .. 12")
    return float(np.float32(2.0 ** (s / 12.0)))


def formant_shift_params(sr, channels, semitones, quefrency_ms=1.5, amount=1.0):
    """the FxFormantParams of a formant shift by `semitones` as the mirror modules build them, or None at 0 semitones; every
    refusal (semitones, amount, the rate, a quefrency outside 1 <= nc <= N / 8) as ValueError, before anything is read or
    written"""
    if not (np.isfinite(semitones) and abs(semitones) <= 12.0):
        raise ValueError(f"formant shift of {semitones!r} semitones: a finite value within -12 .. 12 is expected")
    if not (np.isfinite(amount) and 0.0 <= amount <= 1.0):
        raise ValueError(f"formant shift amount {amount!r}: a value within 0 .. 1 is expected")
    if not (np.isfinite(quefrency_ms) and quefrency_ms > 0.0):
        raise ValueError(f"formant quefrency of {quefrency_ms!r} ms: a positive value is expected")
    try:
        fx_formant_frames(1, sr, quefrency_ms)                      # the rate, and nc against N / 8
    except RvcxError as e:
        raise ValueError(str(e)) from None
    if not semitones:
        return None
    return FxFormantParams.make(sr, channels, semitones=float(semitones), quefrency_ms=float(quefrency_ms), amount=float(amount))


def fx_formant_frames(n: int, sr: int, quefrency_ms=1.5):
    """(T frames, N, nc) of stage 17 for n frames at sr"""
    T, N, nc = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    _fx_host("fx_formant_frames", lib().rvcx_fx_formant_frames(int(n), int(sr), float(quefrency_ms), C.byref(T), C.byref(N),
                                                               C.byref(nc)))
    return int(T.value), int(N.value), int(nc.value)


def _formant_taps(n, params, want):
    """arrays for the optional outputs of one channel: D, E, Es, g and s"""
    if not want:
        return {}
    T, N, _ = fx_formant_frames(n, params.sample_rate, params.quefrency_ms)
    nb = N // 2 + 1
    return dict(D=np.zeros((T, nb, 2), np.float32), E=np.zeros((T, nb), np.float32), Es=np.zeros((T, nb), np.float32),
                g=np.zeros((T, nb), np.float32), s=np.zeros(T, np.float32))


def _formant_tap_ptrs(t):
    return [t[k].ctypes.data if k in t else None for k in ("D", "E", "Es", "g", "s")]


def _formant_source(source, x, what):
    """a source as float32 of the item's shape, or None"""
    if source is None:
        return None
    z, _ = _fx_sig(source, what)
    if z.shape != x.shape:
        raise RvcxError(f"{what}: the source has shape {z.shape}, the item {x.shape} (same length and channel count required)")
    return z


def fx_formant_host(x, sr, params=None, source=None, taps=False):
    """stage 17 on the host (transforms and synthesis in double) -> y, or (y, dict of taps) for a one-channel signal"""
    x, ch = _fx_sig(x, "fx_formant_host")
    p = (params or FxFormantParams.make(sr, ch)).with_shape(sr, ch)
    z = _formant_source(source, x, "fx_formant_host")
    y = np.zeros_like(x)
    t = _formant_taps(x.shape[0], p, taps)
    _fx_host("fx_formant_host", lib().rvcx_fx_formant_host(x.ctypes.data, x.shape[0], None if z is None else z.ctypes.data,
                                                           C.byref(p), y.ctypes.data, *_formant_tap_ptrs(t)))
    return (y, t) if taps else y


def fx_pitch_shift_formant_host(x, sr, semitones, params=None):
    """stage 18 on the host -> y of x's shape"""
    x, ch = _fx_sig(x, "fx_pitch_shift_formant_host")
    p = (params or FxFormantParams.make(sr, ch)).with_shape(sr, ch)
    y = np.zeros_like(x)
    _fx_host("fx_pitch_shift_formant_host", lib().rvcx_fx_pitch_shift_formant_host(x.ctypes.data, x.shape[0], ch, int(sr),
                                                                                   float(semitones), C.byref(p), y.ctypes.data))
    return y


def fx_formant_envelope_host(L, N, nc, iterations=8):
    """the true envelope of one frame from its nb = N / 2 + 1 values L (float32)"""
    L = np.ascontiguousarray(L, dtype=np.float32)
    if L.shape != (int(N) // 2 + 1,):
        raise RvcxError("fx_formant_envelope_host: N / 2 + 1 values expected")
    E = np.zeros_like(L)
    _fx_host("fx_formant_envelope_host", lib().rvcx_fx_formant_envelope_host(L.ctypes.data, int(N), int(nc), int(iterations),
                                                                             E.ctypes.data))
    return E


# ---- live noise reduction on the host (rvcx.h stage 16) ---------------------------------------------------------------------------
class LiveDenoiseParams(C.Structure):
    """rvcx_live_denoise_params; make() fills the defaults of include/rvcx.h stage 16"""
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("mode", C.c_int32), ("strength", C.c_float),
                ("n_std", C.c_float), ("knee_db", C.c_float), ("thresh_mult", C.c_float), ("slope", C.c_float),
                ("time_constant_s", C.c_float), ("fall_time_s", C.c_float), ("freq_smooth_hz", C.c_float),
                ("time_smooth_ms", C.c_float)]
    DEFAULTS = dict(mode=1, strength=0.9, n_std=3.0, knee_db=1.0, thresh_mult=1.0, slope=5.0, time_constant_s=2.0,
                    fall_time_s=0.2, freq_smooth_hz=500.0, time_smooth_ms=50.0)
    MODES = {"profile": 0, "adaptive": 1}

    @classmethod
    def make(cls, sr=0, **values):
        unknown = set(values) - set(cls.DEFAULTS)
        if unknown:
            raise RvcxError(f"LiveDenoiseParams: unknown value(s) {sorted(unknown)}")
        v = dict(cls.DEFAULTS, **values)
        v["mode"] = cls.MODES.get(v["mode"], v["mode"])
        return cls(int(sr), 1, int(v["mode"]), *[float(v[k]) for k in list(cls.DEFAULTS)[1:]])

    def values(self):
        return {k: getattr(self, k) for k in self.DEFAULTS}


class StreamDenoiseSide(C.Structure):
    """rvcx_stream_dn_side: params NULL, the side is absent"""
    _fields_ = [("params", C.c_void_p), ("noise", C.c_void_p), ("n_noise", C.c_int64)]


class StreamDenoise(C.Structure):
    """rvcx_stream_dn (`in` is `inp` here)"""
    _fields_ = [("inp", StreamDenoiseSide), ("out", StreamDenoiseSide)]


def _live_denoise(params, sr=0):
    """(LiveDenoiseParams, noise clip or None) from a LiveDenoiseParams or a dict of values with an optional noise= array"""
    if isinstance(params, LiveDenoiseParams):
        return LiveDenoiseParams(int(sr), 1, *[getattr(params, k) for k in LiveDenoiseParams.DEFAULTS]), None
    v = dict(params or {})
    noise = v.pop("noise", None)
    if noise is not None:
        noise = f32(noise)
        if noise.ndim != 1:
            raise RvcxError("live denoise: the noise clip must be one channel of shape (samples,)")
    return LiveDenoiseParams.make(sr, **v), noise


def _stream_denoise(sides):
    """rvcx_stream_dn from the two sides, each None or what _live_denoise returned (which the caller keeps alive)"""
    dn = StreamDenoise()
    for name, sd in zip(("inp", "out"), sides):
        if sd is not None:
            p, z = sd
            setattr(dn, name, StreamDenoiseSide(C.cast(C.pointer(p), C.c_void_p), None if z is None else z.ctypes.data,
                                                0 if z is None else z.shape[0]))
    return dn


def stream_denoise_delay(sr: int) -> int:
    """N of stage 16 at this rate: the samples a side delays its signal by (RvcxError for a refused rate)"""
    N = int(lib().rvcx_stream_denoise_delay(int(sr)))
    if N < 0:
        raise RvcxError("stream_denoise_delay: the sample rate must be a multiple of 100 Hz within 3200 .. 192000")
    return N


def stream_denoise_frames(n: int, sr: int, freq_smooth_hz=500.0, time_smooth_ms=50.0):
    """(T frames complete in n samples, N, nf, nt) of stage 16"""
    T, N, nf, nt = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _fx_host("stream_denoise_frames", lib().rvcx_stream_denoise_frames(int(n), int(sr), float(freq_smooth_hz), float(time_smooth_ms),
                                                                       C.byref(T), C.byref(N), C.byref(nf), C.byref(nt)))
    return int(T.value), int(N.value), int(nf.value), int(nt.value)


def _live_taps(S, n, sr, mode, want, host):
    if not want:
        return {}
    T, N, _, _ = stream_denoise_frames(n, sr)
    shape = (T, N // 2 + 1) if S is None else (S, T, N // 2 + 1)
    t = dict(S=np.zeros(shape, np.float32), m=np.zeros(shape, np.float32))
    if host:
        t.update(D=np.zeros(shape + (2,), np.float32))
    if mode == 1:
        t.update(f=np.zeros(shape, np.float64))
    return t


def fx_denoise_live_host(x, sr, params=None, noise=None, taps=False):
    """stage 16 on the host (transforms and synthesis in double) on the whole signal -> y delayed by N, or (y, dict of the
    taps D (T, nb, 2), S, m (T, nb) and f (T, nb), mode 1)"""
    x = f32(x)
    if x.ndim != 1:
        raise RvcxError("fx_denoise_live_host: one channel of shape (samples,) expected")
    p, z = _live_denoise(params, sr)
    z = z if noise is None else f32(noise)
    y = np.zeros_like(x)
    rate_ok = lib().rvcx_stream_denoise_delay(int(sr)) > 0          # (a refused rate: the library says so below)
    t = _live_taps(None, x.shape[0], sr, p.mode, taps, True) if rate_ok else {}
    _fx_host("fx_denoise_live_host", lib().rvcx_fx_denoise_live_host(
        x.ctypes.data, x.shape[0], int(sr), None if z is None else z.ctypes.data, 0 if z is None else z.shape[0], C.byref(p),
        y.ctypes.data, *[t[k].ctypes.data if k in t else None for k in ("D", "S", "f", "m")]))
    return (y, t) if taps else y


# ---- live formant shift on the host (rvcx.h stage 19) ------------------------------------------------------------------------------
class LiveFormantParams(C.Structure):
    """rvcx_live_formant_params; make() fills the defaults of include/rvcx.h stage 19 (semitones= sets ratio through
    formant_ratio, the float32 rule of stage 17's layer)"""
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("ratio", C.c_float), ("amount", C.c_float),
                ("quefrency_ms", C.c_float), ("iterations", C.c_int32), ("max_gain_db", C.c_float), ("keep_energy", C.c_int32)]
    DEFAULTS = dict(ratio=1.0, amount=1.0, quefrency_ms=1.5, iterations=8, max_gain_db=24.0, keep_energy=1)
    INTS = ("iterations", "keep_energy")

    @classmethod
    def make(cls, sr=0, **values):
        if "semitones" in values:
            if "ratio" in values:
                raise RvcxError("LiveFormantParams: ratio or semitones, not both")
            values["ratio"] = formant_ratio(values.pop("semitones"))
        unknown = set(values) - set(cls.DEFAULTS)
        if unknown:
            raise RvcxError(f"LiveFormantParams: unknown value(s) {sorted(unknown)}")
        v = dict(cls.DEFAULTS, **values)
        for k in cls.INTS:
            if int(v[k]) != v[k]:
                raise RvcxError(f"LiveFormantParams: {k} must be an integer")
        return cls(int(sr), 1, *[(int if k in cls.INTS else float)(v[k]) for k in cls.DEFAULTS])

    def values(self):
        return {k: getattr(self, k) for k in self.DEFAULTS}


class StreamFormantSide(C.Structure):
    """rvcx_stream_fm_side: params NULL, the side is absent"""
    _fields_ = [("params", C.c_void_p)]


class StreamFormant(C.Structure):
    """rvcx_stream_fm (`in` is `inp` here)"""
    _fields_ = [("inp", StreamFormantSide), ("out", StreamFormantSide)]


def _live_formant(params, sr=0):
    """LiveFormantParams from a LiveFormantParams or a dict of values (semitones= in place of ratio=)"""
    if isinstance(params, LiveFormantParams):
        return LiveFormantParams(int(sr), 1, *[getattr(params, k) for k in LiveFormantParams.DEFAULTS])
    return LiveFormantParams.make(sr, **dict(params or {}))


def stream_formant_delay(sr: int) -> int:
    """N of stage 19 at this rate: the samples a side delays its signal by (RvcxError for a refused rate)"""
    N = int(lib().rvcx_stream_formant_delay(int(sr)))
    if N < 0:
        raise RvcxError("stream_formant_delay: the sample rate must be a multiple of 100 Hz within 3200 .. 192000")
    return N


def stream_formant_frames(n: int, sr: int, quefrency_ms=1.5):
    """(T frames complete in n samples, N, nc) of stage 19"""
    T, N, nc = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    _fx_host("stream_formant_frames", lib().rvcx_stream_formant_frames(int(n), int(sr), float(quefrency_ms), C.byref(T),
                                                                       C.byref(N), C.byref(nc)))
    return int(T.value), int(N.value), int(nc.value)


def _live_formant_taps(S, n, sr, want, host):
    if not want:
        return {}
    N = stream_formant_delay(sr)
    T = stream_denoise_frames(n, sr)[0]
    shape = (T, N // 2 + 1) if S is None else (S, T, N // 2 + 1)
    t = dict(E=np.zeros(shape, np.float32), g=np.zeros(shape, np.float32), s=np.zeros(shape[:-1], np.float32))
    if host:
        t.update(D=np.zeros(shape + (2,), np.float32))
    return t


def fx_formant_live_host(x, sr, params=None, taps=False):
    """stage 19 on the host (transforms and synthesis in double) on the whole signal -> y delayed by N, or (y, dict of the
    taps D (T, nb, 2), E, g (T, nb) and s (T))"""
    x = f32(x)
    if x.ndim != 1:
        raise RvcxError("fx_formant_live_host: one channel of shape (samples,) expected")
    p = _live_formant(params, sr)
    y = np.zeros_like(x)
    rate_ok = lib().rvcx_stream_formant_delay(int(sr)) > 0          # (a refused rate: the library says so below)
    t = _live_formant_taps(None, x.shape[0], sr, taps, True) if rate_ok else {}
    _fx_host("fx_formant_live_host", lib().rvcx_fx_formant_live_host(
        x.ctypes.data, x.shape[0], int(sr), C.byref(p), y.ctypes.data,
        *[t[k].ctypes.data if k in t else None for k in ("D", "E", "g", "s")]))
    return (y, t) if taps else y


_device_info_cache = {}


def device_info(device: int = 0):
    """(name, total bytes) of GPU `device`, or (None, None) when no HIP device is visible (asked once per device: Config()
    is built per request by the reference's callers)"""
    if device in _device_info_cache:
        return _device_info_cache[device]
    _device_info_cache[device] = _device_info(device)
    return _device_info_cache[device]


def _device_info(device: int = 0):
    name = C.create_string_buffer(256)
    total = C.c_int64(0)
    if lib().rvcx_device_info(int(device), name, 256, C.byref(total)) != 0:
        return None, None
    return name.value.decode(), int(total.value)


def flac_encode(pcm, sample_rate: int) -> bytes:
    """int16 PCM, (frames,) or (frames, channels) -> the bytes of a FLAC stream (host code, csrc/flac.hip)"""
    a = np.ascontiguousarray(pcm)
    if a.dtype != np.int16 or a.ndim not in (1, 2):
        raise RvcxError("flac_encode: int16 array of shape (frames,) or (frames, channels) expected")
    frames, ch = a.shape[0], (1 if a.ndim == 1 else a.shape[1])
    cap = lib().rvcx_flac_encode_bound(frames, ch)
    out = np.empty(max(int(cap), 64), np.uint8)
    n = lib().rvcx_flac_encode_s16(a.ctypes.data, frames, ch, int(sample_rate), out.ctypes.data, out.shape[0])
    if n < 0:
        raise RvcxError((lib().rvcx_flac_last_error() or b"").decode())
    return out[:n].tobytes()


def flac_decode(data: bytes):
    """bytes of a FLAC stream -> (int32 array (frames,) or (frames, channels), sample rate, bits per sample)"""
    buf = np.frombuffer(data, np.uint8)
    frames, ch, sr, bits = C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    if lib().rvcx_flac_info(buf.ctypes.data, buf.shape[0], C.byref(frames), C.byref(ch), C.byref(sr), C.byref(bits)) != 0:
        raise RvcxError((lib().rvcx_flac_last_error() or b"").decode())
    # rvcx_flac_info counts the frames itself when STREAMINFO leaves the total at 0 (streamed encodes) and refuses totals
    # that are implausible for the byte count, so this allocation is exact and bounded by the stream's size
    total = max(1, int(frames.value))
    out = np.empty((total, ch.value), np.int32)
    n = lib().rvcx_flac_decode_s32(buf.ctypes.data, buf.shape[0], out.ctypes.data, out.size)
    if n < 0:
        raise RvcxError((lib().rvcx_flac_last_error() or b"").decode())
    out = out[:n]
    return (out[:, 0].copy() if ch.value == 1 else out.copy()), int(sr.value), int(bits.value)


def f0_file_track(inp_f0) -> np.ndarray:
    """host-side piece of VC.get_f0's f0-file branch as the library computes it (no GPU needed)"""
    tab = np.ascontiguousarray(inp_f0, dtype=np.float32).reshape(-1, 2)
    out = np.empty(65536, np.float64)
    n = lib().rvcx_f0_file_track(tab.ctypes.data_as(C.POINTER(C.c_float)), tab.shape[0],
                                 out.ctypes.data_as(C.POINTER(C.c_double)), out.shape[0])
    if n < 0:
        raise RvcxError("f0_file_track: " + (lib().rvcx_last_error(None) or b"").decode())
    return out[:n].copy()


def highpass_exact(x) -> np.ndarray:
    """scipy.signal.filtfilt(bh, ah, x) of pipeline.py:329 on the host, bit for bit (the cut search's filter; no GPU)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    if lib().rvcx_highpass_exact(x.ctypes.data_as(C.POINTER(C.c_double)), y.ctypes.data_as(C.POINTER(C.c_double)),
                                 C.c_int64(x.shape[0])) != 0:
        raise RvcxError("highpass_exact: " + (lib().rvcx_last_error(None) or b"").decode())
    return y


def _p(a: Optional[np.ndarray], ctype=C.c_float):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(ctype))


def f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def i32(a) -> Optional[np.ndarray]:
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def make_table(state: dict):
    """dict name -> numpy/torch tensor  ->  (ctypes Tensor array, keep-alive list)."""
    keep, items = [], []
    for name, t in state.items():
        if hasattr(t, "detach"):
            t = t.detach().cpu().numpy()
        a = np.asarray(t)
        if a.dtype == np.float32:
            dt = 0
        elif a.dtype == np.float16:
            dt = 1
        elif a.dtype == np.int64:
            dt = 2
        else:
            a = a.astype(np.float32)
            dt = 0
        a = np.ascontiguousarray(a)
        if a.ndim > 4:
            raise RvcxError(f"tensor {name} has {a.ndim} dims")
        keep.append(a)
        nm = name.encode()
        keep.append(nm)
        shp = (C.c_int64 * 4)(*(list(a.shape) + [1] * (4 - a.ndim)))
        items.append(Tensor(nm, a.ctypes.data, dt, a.ndim, shp))
    arr = (Tensor * len(items))(*items)
    return arr, keep


class Ticket:
    """A conversion in flight (Context.convert_submit).  The object keeps every numpy array the library borrowed alive
    until the ticket has been waited for; dropped unwaited, its finaliser waits."""

    def __init__(self, ctx, tid, keep, outs, f32s, out_n):
        self._ctx, self.id, self._keep = ctx, int(tid), keep
        self._outs, self._f32s, self._out_n = outs, f32s, out_n
        self._waited = False
        self._lead = None

    def done(self) -> bool:
        """True when wait() will not block on the device"""
        if self._waited:
            return True
        rc = lib().rvcx_convert_poll(self._ctx._h, self.id)
        self._ctx._ck(0 if rc >= 0 else rc, "convert_poll")
        return rc == 1

    def wait(self):
        """what Context.convert_batch returns for the same arguments"""
        if self._waited:
            raise RvcxError("Ticket.wait: the ticket has already been waited for")
        self._waited = True
        try:
            self._ctx._ck(lib().rvcx_convert_wait(self._ctx._h, self.id), "convert_wait")
            self._lead = float(lib().rvcx_ticket_lead_ms(self._ctx._h, self.id))
            if self._outs is None:        # convert_submit_raw: the caller's own buffers hold the samples
                return [int(v) for v in self._out_n]
            pcm = [o[:self._out_n[i]].copy() for i, o in enumerate(self._outs)]
            if self._f32s is not None:
                return pcm, [o[:self._out_n[i]].copy() for i, o in enumerate(self._f32s)]
            return pcm
        finally:
            self._keep = None      # the borrowed buffers are the caller's again

    @property
    def lead_ms(self) -> float:
        """device ms between this ticket's first front-end work and the completion of the ticket submitted before it
        (positive: they overlapped); valid after wait()"""
        if self._lead is None:
            raise RvcxError("Ticket.lead_ms is valid after wait()")
        return self._lead

    def __del__(self):
        try:
            if not self._waited and getattr(self._ctx, "_h", None):
                self._waited = True
                lib().rvcx_convert_wait(self._ctx._h, self.id)
        except Exception:
            pass


class StreamSession:
    """S lock-step live streams (Context.stream_open).  step() takes one block per stream -- 16 kHz mono, or in_rate x
    in_channels when the session was opened with them -- and returns the converted blocks at the voice model's rate, or at
    out_rate; the rolling context, the resamplers' FIFOs, the SOLA carry and the noise counters live on the device."""

    def __init__(self, ctx, sid, cfg, io, upp):
        self._ctx, self.id, self.cfg, self.io = ctx, sid, cfg, io
        self.n_streams = int(cfg.n_streams)
        self.in_channels = int(io.in_channels)
        self.block_in = int(lib().rvcx_stream_in_len(ctx._h, sid))        # frames per block at the input rate
        self.block_out = int(lib().rvcx_stream_out_len(ctx._h, sid))      # frames per block as step() returns them
        self.out_channels = int(lib().rvcx_stream_out_channels(ctx._h, sid))   # 2 when the effects board is on
        self.effects = None                                               # the eighteen values in force (a dict), or None
        self.denoise = [None, None]                                       # per side (in, out): the values in force, or None
        self.formant = [None, None]                                       # the same for the live formant shift
        self.noise_len = int(lib().rvcx_stream_noise_len(ctx._h, sid))
        self.frames = int(lib().rvcx_stream_frames(ctx._h, sid))          # T of the TextEncoder
        din, dout = C.c_int32(0), C.c_int32(0)
        ctx._ck(lib().rvcx_stream_delays(ctx._h, sid, C.byref(din), C.byref(dout)), "stream_delays")
        self.in_delay, self.out_delay = int(din.value), int(dout.value)   # samples at 16 kHz / at the output rate
        # model-rate lengths: upp comes from the library, not from block_out (the output may be resampled)
        Fb = int(cfg.block_frames)
        self.upp = int(upp)
        self.block_native = Fb * self.upp
        self.out_rate = 100 * self.block_out // Fb
        self.out_resampled = self.out_rate != 100 * self.upp
        self.tail_len = (Fb + int(cfg.crossfade_frames) + int(cfg.search_frames)) * self.upp
        self.skip_head = self.frames - self.tail_len // self.upp
        # the two resamplers' delays, plus the 10 ms of the p_len clamp (rvcx.h: the newest ring frame is not synthesized)
        self.latency_ms = 1e3 * self.in_delay / 16000.0 + 1e3 * self.out_delay / float(self.out_rate) + 10.0

    def step(self, blocks, noise=None, taps=False):
        """blocks (S, block_in) float32 -- (S, block_in, in_channels) for in_channels > 1 -- -> (S, block_out) float32,
        (S, block_out, 2) from a session with effects.
        noise (S, noise_len): parity noise of this step (z_noise then src_noise per stream).  taps=True: (out, pre_sola
        (S, tail_len), offsets (S,)), the latter two at the model's rate."""
        if self.id is None:
            raise RvcxError("StreamSession.step: the session is closed")
        S = self.n_streams
        x = f32(blocks)
        want = (S, self.block_in) if self.in_channels == 1 else (S, self.block_in, self.in_channels)
        if x.shape != want:
            raise RvcxError(f"StreamSession.step: blocks must be {want}, got {x.shape}")
        nz = None
        if noise is not None:
            nz = f32(noise)
            if nz.shape != (S, self.noise_len):
                raise RvcxError(f"StreamSession.step: noise must be ({S}, {self.noise_len})")
        out = np.empty((S, self.block_out) if self.out_channels == 1 else (S, self.block_out, 2), np.float32)
        pre = np.empty((S, self.tail_len), np.float32) if taps else None
        offs = np.empty(S, np.int32) if taps else None
        self._ctx._ck(lib().rvcx_stream_step(self._ctx._h, self.id, self._table(x), self._table(nz), self._table(out),
                                             self._table(pre), _p(offs, C.c_int32)), "stream_step")
        return (out, pre, offs) if taps else out

    def _table(self, a):
        return None if a is None else (C.c_void_p * self.n_streams)(*[a[i].ctypes.data for i in range(self.n_streams)])

    def last_taps(self):
        """(in16k (S, Fb * 160), native (S, Fb * upp)) of the last successful step: the blocks that entered the rings and the
        SOLA output in front of the output resampler (None when the output is not resampled: step() returned it)"""
        S = self.n_streams
        in16k = np.empty((S, int(self.cfg.block_frames) * 160), np.float32)
        native = np.empty((S, self.block_native), np.float32) if self.out_resampled else None
        self._ctx._ck(lib().rvcx_stream_last_taps(self._ctx._h, self.id, self._table(in16k), self._table(native)),
                      "stream_last_taps")
        return in16k, native

    def set(self, pitches=None, sids=None, index_rate=None, protect=None):
        """live controls, applied from the next step on (None keeps the current value); ring, FIFOs, carry and noise
        counters are untouched.  A refused value (speaker id out of range, index of the wrong width) changes nothing."""
        S = self.n_streams
        pit = None if pitches is None else f32(np.atleast_1d(pitches))
        sid = None if sids is None else i32(np.atleast_1d(sids))
        if (pit is not None and pit.shape != (S,)) or (sid is not None and sid.shape != (S,)):
            raise RvcxError("StreamSession.set: one pitch and one speaker id per stream")
        nan = float("nan")
        self._ctx._ck(lib().rvcx_stream_set(self._ctx._h, self.id, None if pit is None else pit.ctypes.data,
                                            None if sid is None else sid.ctypes.data,
                                            nan if index_rate is None else float(index_rate),
                                            nan if protect is None else float(protect)), "stream_set")

    def set_effects(self, **changes):
        """rvcx_stream_set_fx: new values for some of the eighteen add_effects names, applied from the next step on; the others
        keep their current value.  All state is kept (a reverb tail rings on), except that of a stage the new values turn
        into an identity.  A refused value changes nothing; a session opened without effects refuses the call."""
        if self.effects is None:
            raise RvcxError("StreamSession.set_effects: the session was opened without effects (its channel count is fixed "
                            "at open)")
        values = fx_values(changes, self.effects)
        p = FxParams.make(values, 0, 0)
        self._ctx._ck(lib().rvcx_stream_set_fx(self._ctx._h, self.id, C.byref(p)), "stream_set_fx")
        self.effects = values

    def last_fx_ms(self):
        """per-stage device ms of the board in the last step (rvcx_stream_last_fx_ms)"""
        ms = (C.c_float * 8)()
        self._ctx._ck(lib().rvcx_stream_last_fx_ms(self._ctx._h, self.id, ms), "stream_last_fx_ms")
        names = ["highpass", "compressor", "gate", "reverb", "low_shelf", "high_shelf", "chorus", "total"]
        return dict(zip(names, [float(v) for v in ms]))

    SIDES = {"in": 0, "input": 0, 0: 0, "out": 1, "output": 1, 1: 1}

    def set_denoise(self, side, **changes):
        """rvcx_stream_set_denoise: new values for some of the ten LiveDenoiseParams names on side "in" or "out", applied from
        the next step on; the others keep their current value.  All state is kept (the floor stays learned).  A refused value
        changes nothing; a side that was absent at open refuses the call."""
        if side not in self.SIDES:
            raise RvcxError("StreamSession.set_denoise: side must be 'in' or 'out'")
        k = self.SIDES[side]
        if self.denoise[k] is None:
            raise RvcxError("StreamSession.set_denoise: the session was opened without noise reduction on this side (its "
                            "delay is fixed at open)")
        p = LiveDenoiseParams.make(0, **dict(self.denoise[k], **changes))
        self._ctx._ck(lib().rvcx_stream_set_denoise(self._ctx._h, self.id, k, C.byref(p)), "stream_set_denoise")
        self.denoise[k] = p.values()

    def last_dn_ms(self):
        """device ms of the input and the output noise gate in the last step (rvcx_stream_last_dn_ms; 0 for an absent side)"""
        ms = (C.c_float * 2)()
        self._ctx._ck(lib().rvcx_stream_last_dn_ms(self._ctx._h, self.id, ms), "stream_last_dn_ms")
        return float(ms[0]), float(ms[1])

    def set_formant(self, side, **changes):
        """rvcx_stream_set_formant: new values for some of the six LiveFormantParams names (semitones= in place of ratio=) on
        side "in" or "out", applied from the next step on; the others keep their current value.  All state is kept.  A refused
        value changes nothing; a side that was absent at open refuses the call."""
        if side not in self.SIDES:
            raise RvcxError("StreamSession.set_formant: side must be 'in' or 'out'")
        k = self.SIDES[side]
        if self.formant[k] is None:
            raise RvcxError("StreamSession.set_formant: the session was opened without a formant shift on this side (its "
                            "delay is fixed at open)")
        base = dict(self.formant[k])
        if "semitones" in changes:
            base.pop("ratio")
        p = LiveFormantParams.make(0, **dict(base, **changes))
        self._ctx._ck(lib().rvcx_stream_set_formant(self._ctx._h, self.id, k, C.byref(p)), "stream_set_formant")
        self.formant[k] = p.values()

    def last_fm_ms(self):
        """device ms of the input and the output formant shift in the last step (rvcx_stream_last_fm_ms; 0 for an absent side)"""
        ms = (C.c_float * 2)()
        self._ctx._ck(lib().rvcx_stream_last_fm_ms(self._ctx._h, self.id, ms), "stream_last_fm_ms")
        return float(ms[0]), float(ms[1])

    def reset(self):
        """zero ring, carry, the board's state and the step counter: the session then replays a fresh one"""
        self._ctx._ck(lib().rvcx_stream_reset(self._ctx._h, self.id), "stream_reset")

    def close(self):
        if self.id is not None and getattr(self._ctx, "_h", None):
            sid, self.id = self.id, None
            self._ctx._ck(lib().rvcx_stream_close(self._ctx._h, sid), "stream_close")
        self.id = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Context:
    """One rvcx context (= one GPU)."""

    regions_on_device = True       # weights_regions() returns device pointers (dist.broadcast_weights checks this)

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        rc = lib().rvcx_create(int(device), C.byref(self._h))
        if rc != 0:
            raise RvcxError("rvcx_create: " + (lib().rvcx_last_error(None) or b"").decode())
        self.device = device
        # Every C entry point takes the context's own mutex (csrc/api_internal.h), so threads that share this object queue
        # instead of racing.  Multi-call sequences that must not interleave -- "make this index resident, then convert
        # with it" in the mirror's VC.pipeline -- hold this lock around the whole sequence.
        self.lock = threading.RLock()

    def close(self):
        if getattr(self, "_h", None):
            lib().rvcx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise RvcxError(f"{what}: " + (lib().rvcx_last_error(self._h) or b"").decode())

    # ---- kernel-level ops -------------------------------------------------------------
    def conv1d(self, x, w, bias=None, res=None, stride=1, dil=1, pad_left=0, Tout=None, groups=1,
               pre_lrelu=None, act=0, act_slope=0.0, lens_in=None, lens_out=None):
        x, w = f32(x), f32(w)
        B, Cin, Tin = x.shape
        Cout, _, K = w.shape
        if Tout is None:
            Tout = (Tin + 2 * pad_left - dil * (K - 1) - 1) // stride + 1
        y = np.empty((B, Cout, Tout), np.float32)
        bias = None if bias is None else f32(bias)
        res = None if res is None else f32(res)
        li, lo = i32(lens_in), i32(lens_out)
        self._ck(lib().rvcx_op_conv1d(self._h, _p(x), _p(w), _p(bias), _p(res), _p(y), B, Cin, Tin, Cout, K,
                                      stride, dil, pad_left, Tout, groups,
                                      0 if pre_lrelu is None else 1,
                                      C.c_float(0.0 if pre_lrelu is None else pre_lrelu), act,
                                      C.c_float(act_slope), _p(li, C.c_int32), _p(lo, C.c_int32)), "op_conv1d")
        return y

    def resblock_pair(self, x, w1, b1, w2, b2, dil=1, slope=0.1, fused=True, lens=None):
        x, w1, w2 = f32(x), f32(w1), f32(w2)
        B, Cc, T = x.shape
        K = w1.shape[2]
        y = np.empty_like(x)
        b1 = None if b1 is None else f32(b1)
        b2 = None if b2 is None else f32(b2)
        li = i32(lens)
        self._ck(lib().rvcx_op_resblock_pair(self._h, _p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(y), B, Cc, T, K, dil,
                                             C.c_float(slope), 1 if fused else 0, _p(li, C.c_int32)),
                 "op_resblock_pair")
        return y

    def resblock3(self, x, w1, b1, w2, b2, dils=(1, 3, 5), slope=0.1, lens=None):
        """a whole k = 3 ResBlock1 (three steps) in one kernel; w1 / w2 (3, C, C, 3), b1 / b2 (3, C) or None"""
        x, w1, w2 = f32(x), f32(w1), f32(w2)
        B, Cc, T = x.shape
        y = np.empty_like(x)
        b1 = None if b1 is None else f32(b1)
        b2 = None if b2 is None else f32(b2)
        d = i32(list(dils))
        li = i32(lens)
        self._ck(lib().rvcx_op_resblock3(self._h, _p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(y), B, Cc, T, _p(d, C.c_int32),
                                         C.c_float(slope), _p(li, C.c_int32)), "op_resblock3")
        return y

    def bench_resblock_pair(self, B, Cc, T, K, dil=1, fused=True, iters=10):
        ms = C.c_float(0)
        self._ck(lib().rvcx_bench_resblock_pair(self._h, B, Cc, T, K, dil, 1 if fused else 0, iters, C.byref(ms)),
                 "bench_resblock_pair")
        return ms.value, 4.0 * B * Cc * Cc * K * T / (ms.value * 1e-3) / 1e12

    @staticmethod
    def conv_override(tile=-1, variant=-1, splitk=-1):
        """tuning hook; the library refuses it (and debug_inject / bench_*) unless the process started with RVCX_DEBUG=1"""
        if lib().rvcx_conv_override(tile, variant, splitk) != 0:
            raise RvcxError("conv_override: " + (lib().rvcx_last_error(None) or b"").decode())

    def bench_conv1d(self, B, Cin, Tin, Cout, K, stride=1, dil=1, groups=1, iters=10):
        ms = C.c_float(0)
        self._ck(lib().rvcx_bench_conv1d(self._h, B, Cin, Tin, Cout, K, stride, dil, groups, iters, C.byref(ms)),
                 "bench_conv1d")
        pad = (K * dil - dil) // 2
        Tout = (Tin + 2 * pad - dil * (K - 1) - 1) // stride + 1
        flops = 2.0 * B * Cout * Tout * K * (Cin // groups)
        return ms.value, flops / (ms.value * 1e-3) / 1e12

    def convtranspose1d(self, x, w, bias=None, stride=1, pad=0, pre_lrelu=None):
        x, w = f32(x), f32(w)
        B, Cin, Tin = x.shape
        _, Cout, K = w.shape
        Tout = (Tin - 1) * stride - 2 * pad + K
        y = np.empty((B, Cout, Tout), np.float32)
        bias = None if bias is None else f32(bias)
        self._ck(lib().rvcx_op_convtranspose1d(self._h, _p(x), _p(w), _p(bias), _p(y), B, Cin, Tin, Cout, K,
                                               stride, pad, 0 if pre_lrelu is None else 1,
                                               C.c_float(0.0 if pre_lrelu is None else pre_lrelu)),
                 "op_convtranspose1d")
        return y

    def conv2d3x3(self, x, w, bias=None, res=None, act=0):
        x, w = f32(x), f32(w)
        B, Cin, H, W = x.shape
        Cout = w.shape[0]
        y = np.empty((B, Cout, H, W), np.float32)
        bias = None if bias is None else f32(bias)
        res = None if res is None else f32(res)
        self._ck(lib().rvcx_op_conv2d3x3(self._h, _p(x), _p(w), _p(bias), _p(res), _p(y), B, Cin, H, W, Cout,
                                         act), "op_conv2d3x3")
        return y

    def convblock2d(self, x, w1, b1, w2, b2, wsc=None, bsc=None, rows=None):
        """one ConvBlockRes (RMVPE.py:140-175, BN folded by the caller) through the F0 model's own block path"""
        x, w1, w2 = f32(x), f32(w1), f32(w2)
        B, Cin, H, W = x.shape
        Cout = w1.shape[0]
        y = np.empty((B, Cout, H, W), np.float32)
        b1 = None if b1 is None else f32(b1)
        b2 = None if b2 is None else f32(b2)
        wsc = None if wsc is None else f32(wsc)
        bsc = None if bsc is None else f32(bsc)
        ri = i32(rows)
        self._ck(lib().rvcx_op_convblock2d(self._h, _p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(wsc), _p(bsc), _p(y), B, Cin,
                                           Cout, H, W, _p(ri, C.c_int32)), "op_convblock2d")
        return y

    def convtranspose2d(self, x, w, bias=None, act=0):
        x, w = f32(x), f32(w)
        B, Cin, H, W = x.shape
        Cout = w.shape[1]
        y = np.empty((B, Cout, 2 * H, 2 * W), np.float32)
        bias = None if bias is None else f32(bias)
        self._ck(lib().rvcx_op_convtranspose2d(self._h, _p(x), _p(w), _p(bias), _p(y), B, Cin, H, W, Cout, act),
                 "op_convtranspose2d")
        return y

    def attention(self, q, k, v, heads, scale, emb_rel_k=None, emb_rel_v=None, window=10, lens=None):
        q, k, v = f32(q), f32(k), f32(v)
        B, HD, T = q.shape
        D = HD // heads
        out = np.empty_like(q)
        ek = None if emb_rel_k is None else f32(emb_rel_k)
        ev = None if emb_rel_v is None else f32(emb_rel_v)
        li = i32(lens)
        self._ck(lib().rvcx_op_attention(self._h, _p(q), _p(k), _p(v), _p(out), B, heads, D, T, C.c_float(scale),
                                         _p(ek), _p(ev), window, _p(li, C.c_int32)), "op_attention")
        return out

    def gemm_tm(self, x_cf, w, bias=None, res_tm=None, act=0, exact_fp32=False):
        """the time-major Linear kernel: x_cf (B, Cin, T) -> (y_tm (B*T, Cout), y_cf (B, Cout, T), y_split decoded)"""
        x_cf, w = f32(x_cf), f32(w)
        B, Cin, T = x_cf.shape
        Cout = w.shape[0]
        bias = None if bias is None else f32(bias)
        res = None if res_tm is None else f32(res_tm)
        y = np.empty((B * T, Cout), np.float32)
        ycf = np.empty((B, Cout, T), np.float32)
        ysp = np.empty((B * T, Cout), np.float32) if Cout % 16 == 0 else None
        self._ck(lib().rvcx_op_gemm_tm(self._h, _p(x_cf), _p(w), _p(bias), _p(res), B, T, Cin, Cout, int(act),
                                       1 if exact_fp32 else 0, _p(y), _p(ycf), _p(ysp)), "op_gemm_tm")
        return y, ycf, ysp

    def bench_gemm(self, rows, cin, cout, iters=20):
        ms = C.c_float(0)
        self._ck(lib().rvcx_bench_gemm(self._h, C.c_int64(rows), cin, cout, iters, C.byref(ms)), "bench_gemm")
        return ms.value, 2.0 * rows * cin * cout / (ms.value * 1e-3) / 1e12

    def layernorm_tm(self, x, gamma, beta, eps=1e-5):
        x = f32(x)
        rows, Cc = x.shape
        y = np.empty_like(x)
        ysp = np.empty_like(x) if Cc % 16 == 0 else None
        self._ck(lib().rvcx_op_layernorm_tm(self._h, _p(x), _p(f32(gamma)), _p(f32(beta)), _p(y), _p(ysp),
                                            C.c_int64(rows), Cc, C.c_float(eps)), "op_layernorm_tm")
        return y, ysp

    def layernorm_c(self, x, gamma, beta, eps=1e-5):
        x = f32(x)
        B, Cc, T = x.shape
        y = np.empty_like(x)
        self._ck(lib().rvcx_op_layernorm_c(self._h, _p(x), _p(f32(gamma)), _p(f32(beta)), _p(y), B, Cc, T,
                                           C.c_float(eps)), "op_layernorm_c")
        return y

    def groupnorm_gelu(self, x, gamma, beta, eps=1e-5, lens=None, split=True):
        """GroupNorm(C, C) + GELU of x (B, C, T): (y, stats (B, C, 2) = {mean, rstd}, y_split decoded); the last two are None
        unless split (C a multiple of 16)"""
        x = f32(x)
        B, Cc, T = x.shape
        y = np.empty_like(x)
        split = bool(split) and Cc % 16 == 0
        st = np.empty((B, Cc, 2), np.float32) if split else None
        ys = np.empty_like(x) if split else None
        li = i32(lens)
        self._ck(lib().rvcx_op_groupnorm_gelu(self._h, _p(x), _p(f32(gamma)), _p(f32(beta)), B, Cc, T, eps,
                                              _p(li, C.c_int32), _p(y), _p(st), _p(ys)), "op_groupnorm_gelu")
        return y, st, ys

    def hubert_conv0(self, wav, w, gamma, beta, stride=5, eps=1e-5, lens=None, fused=True):
        """HuBERT's first layer, wav (B, n) and w (C, 1, K) -> (stats (B, C, 2), y_split decoded (B, C, T0), the split image's
        raw halves (uint16)); fused: the form without the fp32 map, else conv + statistics + split store"""
        wav, w = f32(wav), f32(w)
        B, n = wav.shape
        Cc, _, K = w.shape
        T0 = (n - K) // stride + 1
        st = np.empty((B, Cc, 2), np.float32)
        ys = np.empty((B, Cc, T0), np.float32)
        raw = np.empty(B * Cc * T0 * 2, np.uint16)
        li = i32(lens)
        self._ck(lib().rvcx_op_hubert_conv0(self._h, _p(wav), _p(w), _p(f32(gamma)), _p(f32(beta)), B, Cc, n, K, int(stride),
                                            eps, _p(li, C.c_int32), 1 if fused else 0, _p(st), _p(ys), _p(raw, C.c_uint16)),
                 "op_hubert_conv0")
        return st, ys, raw

    def sine_source(self, f0, noise, lin_wb, upp, sr, lens=None):
        """NSF harmonic source: f0 (B, T), noise (B, T * upp), lin_wb (w, b) -> har (B, T * upp)"""
        f0, noise, wb = f32(f0), f32(noise), f32(lin_wb)
        B, T = f0.shape
        assert noise.shape == (B, T * upp) and wb.shape == (2,)
        har = np.empty_like(noise)
        li = i32(lens)
        self._ck(lib().rvcx_op_sine_source(self._h, _p(f0), _p(noise), _p(wb), B, T, int(upp), float(sr), _p(li, C.c_int32),
                                           _p(har)), "op_sine_source")
        return har

    def randn(self, n, seed, offset=0):
        """n values of the Philox noise stream `seed` from counter `offset` on (four values per counter step)"""
        out = np.empty(int(n), np.float32)
        self._ck(lib().rvcx_op_randn(self._h, int(n), int(seed), int(offset), _p(out)), "op_randn")
        return out

    def reflect_pad(self, x, p, ns=None):
        x = f32(x)
        B, n = x.shape
        y = np.empty((B, n + 2 * int(p)), np.float32)
        li = i32(ns)
        self._ck(lib().rvcx_op_reflect_pad(self._h, _p(x), B, n, int(p), _p(li, C.c_int32), _p(y)), "op_reflect_pad")
        return y

    def mel_post(self, mel, Tp, bn, fs=None, tps=None):
        """mel (B, nmel, F) -> row-padded log-mel (B, Tp, nmel + 2); bn = (scale, shift)"""
        mel, bn = f32(mel), f32(bn)
        B, nmel, F = mel.shape
        out = np.empty((B, int(Tp), nmel + 2), np.float32)
        fi, ti = i32(fs), i32(tps)
        self._ck(lib().rvcx_op_mel_post(self._h, _p(mel), B, nmel, F, int(Tp), _p(bn), _p(fi, C.c_int32), _p(ti, C.c_int32),
                                        _p(out)), "op_mel_post")
        return out

    def decode_f0(self, sal, thred=0.03, f0_min=50.0, f0_max=1100.0):
        """salience (B, T, ld >= 360; the first 360 columns count) -> f0 (B, T)"""
        sal = f32(sal)
        B, T, ld = sal.shape
        f0 = np.empty((B, T), np.float32)
        self._ck(lib().rvcx_op_decode_f0(self._h, _p(sal), B, T, ld, thred, f0_min, f0_max, _p(f0)), "op_decode_f0")
        return f0

    def avgpool2(self, x, H, Wp, y_ps=None):
        """x (planes, x_ps >= H * Wp): row-padded planes -> (planes, y_ps) holding (H // 2, (Wp - 2) // 2 + 2) planes"""
        x = f32(x)
        planes, x_ps = x.shape
        dense = (H // 2) * ((Wp - 2) // 2 + 2)
        y_ps = dense if y_ps is None else int(y_ps)
        y = np.empty((planes, y_ps), np.float32)
        self._ck(lib().rvcx_op_avgpool2(self._h, _p(x), planes, int(H), int(Wp), x_ps, y_ps, _p(y)), "op_avgpool2")
        return y

    def gru_input(self, x):
        """row-padded (B, C, T, Wp) -> (B, C * (Wp - 2), T)"""
        x = f32(x)
        B, Cc, T, Wp = x.shape
        y = np.empty((B, Cc * (Wp - 2), T), np.float32)
        self._ck(lib().rvcx_op_gru_input(self._h, _p(x), B, Cc, T, Wp, _p(y)), "op_gru_input")
        return y

    def upsample_protect(self, feats, feats0, pitchf, Th, p_len, protect=0.33, use_protect=True, ld_out=None):
        """feats / feats0 (C, ld_in >= Th), pitchf (p_len) -> out (C, ld_out >= p_len)"""
        feats = f32(feats)
        Cc, ld_in = feats.shape
        feats0 = None if feats0 is None else f32(feats0)
        pitchf = None if pitchf is None else f32(pitchf)
        ld_out = int(p_len) if ld_out is None else int(ld_out)
        out = np.empty((Cc, ld_out), np.float32)
        self._ck(lib().rvcx_op_upsample_protect(self._h, _p(feats), _p(feats0), _p(pitchf), Cc, int(Th), int(p_len), protect,
                                                1 if use_protect else 0, ld_in, ld_out, _p(out)), "op_upsample_protect")
        return out

    # ---- models -----------------------------------------------------------------------
    def load_synth(self, cfg_struct, state: dict) -> int:
        tbl, keep = make_table(state)
        mid = C.c_int(-1)
        self._ck(lib().rvcx_load_synth(self._h, C.byref(cfg_struct), tbl, len(tbl), C.byref(mid)), "load_synth")
        return mid.value

    def unload_synth(self, model_id: int):
        self._ck(lib().rvcx_unload_synth(self._h, int(model_id)), "unload_synth")

    def synth_upp(self, model_id: int) -> int:
        return int(lib().rvcx_synth_upp(self._h, model_id))

    def synth_dec_rf(self, model_id) -> int:
        """frames of z an output sample of the NSF decoder can depend on, each side (+ 2)"""
        return int(lib().rvcx_synth_dec_rf(self._h, int(model_id)))

    def synth_infer(self, model_id, phone, pitch, pitchf, lens=None, sid=None, z_noise=None, src_noise=None,
                    seed=0, taps=False, dec_skip=0, skip_head=None):
        """skip_head (frames; Synthesizer.infer's `rate`, see head_from_rate): the flow, the source and the decoder run on
        frames [skip_head:] only -- returns (out (B, (T - skip_head) * upp), zflow (B, inter, T - skip_head) or None without
        z_noise); src_noise is (B, (T - skip_head) * upp)"""
        phone, pitchf = f32(phone), f32(pitchf)
        pitch = i32(pitch)
        B, T, _ = phone.shape
        upp = self.synth_upp(model_id)
        out = np.empty((B, T * upp), np.float32)
        lens = i32(np.full(B, T) if lens is None else lens)
        sid = i32(np.zeros(B) if sid is None else sid)
        zn = None if z_noise is None else f32(z_noise)
        sn = None if src_noise is None else f32(src_noise)
        if skip_head is not None:
            if taps or dec_skip:
                raise RvcxError("synth_infer: dec_skip / taps and skip_head exclude each other")
            head = int(skip_head)
            Tk = max(T - head, 0)
            if sn is not None and sn.size != B * Tk * upp:
                raise RvcxError("synth_infer(skip_head=): src_noise must hold (T - skip_head) * upp samples per item")
            out = np.empty((B, Tk * upp), np.float32)
            zflow = None if zn is None else np.empty((B, zn.shape[1], Tk), np.float32)
            self._ck(lib().rvcx_synth_infer_head(self._h, model_id, B, T, _p(lens, C.c_int32), _p(phone),
                                                 _p(pitch, C.c_int32), _p(pitchf), _p(sid, C.c_int32), _p(zn), _p(sn),
                                                 C.c_uint64(seed), head, _p(out), _p(zflow)), "synth_infer_head")
            return out, zflow
        if taps:
            inter = (zn.shape[1] if zn is not None else None)
            if inter is None:
                raise RvcxError("synth_infer(taps=True) needs z_noise (its shape gives inter_channels)")
            stats = np.empty((B, 2 * inter, T), np.float32)
            zflow = np.empty((B, inter, T), np.float32)
            self._ck(lib().rvcx_synth_infer_taps(self._h, model_id, B, T, _p(lens, C.c_int32), _p(phone),
                                                 _p(pitch, C.c_int32), _p(pitchf), _p(sid, C.c_int32), _p(zn), _p(sn),
                                                 C.c_uint64(seed), _p(out), _p(stats), _p(zflow)), "synth_infer_taps")
            return out, stats, zflow
        if dec_skip:
            self._ck(lib().rvcx_synth_infer_window(self._h, model_id, B, T, _p(lens, C.c_int32), _p(phone),
                                                   _p(pitch, C.c_int32), _p(pitchf), _p(sid, C.c_int32), _p(zn), _p(sn),
                                                   C.c_uint64(seed), int(dec_skip), _p(out)), "synth_infer_window")
            return out
        self._ck(lib().rvcx_synth_infer(self._h, model_id, B, T, _p(lens, C.c_int32), _p(phone),
                                        _p(pitch, C.c_int32), _p(pitchf), _p(sid, C.c_int32), _p(zn), _p(sn),
                                        C.c_uint64(seed), _p(out)), "synth_infer")
        return out

    def sola(self, y, b, Lb, Lx, Ls, scores=False):
        """rvcx_op_sola: (out (Lb,), new carry (Lx,), offset[, scores (Ls + 1,)])"""
        y, b = f32(y), f32(b)
        Lb, Lx, Ls = int(Lb), int(Lx), int(Ls)
        if y.shape != (Lb + Lx + Ls,) or b.shape != (Lx,):
            raise RvcxError("sola: y must hold Lb + Lx + Ls samples and b Lx")
        out, nb = np.empty(Lb, np.float32), np.empty(Lx, np.float32)
        off = C.c_int32(-1)
        sc = np.empty(Ls + 1, np.float32) if scores else None
        self._ck(lib().rvcx_op_sola(self._h, _p(y), _p(b), Lb, Lx, Ls, _p(out), _p(nb), C.byref(off), _p(sc)), "op_sola")
        return (out, nb, int(off.value), sc) if scores else (out, nb, int(off.value))

    def stream_resample(self, x, sr_in: int, sr_out: int, block_frames: int) -> np.ndarray:
        """rvcx_op_stream_resample: a session's resampler without a session.  x (S, frames) or (S, frames, channels) float32,
        cut into blocks of block_frames * sr_in / 100 frames -> (S, frames * sr_out / sr_in) float32, delayed by
        stream_resample_delay(sr_in, sr_out) samples."""
        x = f32(x)
        if x.ndim not in (2, 3):
            raise RvcxError("stream_resample: x must be (S, frames) or (S, frames, channels)")
        S, frames, ch = x.shape[0], x.shape[1], (1 if x.ndim == 2 else x.shape[2])
        n_out = frames * int(sr_out) // max(int(sr_in), 1) if int(sr_in) > 0 and int(sr_out) > 0 else 0
        y = np.empty((S, max(n_out, 0)), np.float32)
        self._ck(lib().rvcx_op_stream_resample(self._h, x.ctypes.data, S, C.c_int64(frames), ch, int(sr_in), int(sr_out),
                                               int(block_frames), y.ctypes.data), "op_stream_resample")
        return y

    def stream_open(self, model_id, params: "Params", sids, pitches, block_frames, context_frames, crossfade_frames,
                    search_frames, in_rate=0, in_channels=1, out_rate=0, effects=None, denoise_in=None,
                    denoise_out=None, formant_in=None, formant_out=None) -> "StreamSession":
        """rvcx_stream_open_io: len(sids) lock-step live streams on voice model `model_id` (frames of 10 ms).  in_rate /
        in_channels: what step() takes (0 or 16000 with one channel: 16 kHz mono); out_rate: what it returns (0 or the
        model's rate: the model's rate).  effects: a dict of add_effects names laid over FX_UI_DEFAULTS, or an FxParams --
        the board runs inside every step on what would have left and step() returns stereo (rvcx_stream_open_fx).
        denoise_in / denoise_out: a dict of LiveDenoiseParams values (with noise= a clip for mode 0), or a LiveDenoiseParams --
        live noise reduction on the 16 kHz block in front of the ring / on what leaves, in front of the board; each side
        delays its signal by stream_denoise_delay(rate) samples (rvcx_stream_open_dn).
        formant_in / formant_out: a dict of LiveFormantParams values (semitones= in place of ratio=), or a LiveFormantParams --
        the live formant shift behind the noise gate of that side; each side delays its signal by stream_formant_delay(rate)
        samples (rvcx_stream_open_fm).  With the defaults this is rvcx_stream_open."""
        values = None if effects is None else fx_values(effects)
        sid, pit = i32(np.atleast_1d(sids)), f32(np.atleast_1d(pitches))
        if sid.ndim != 1 or sid.shape != pit.shape or sid.shape[0] < 1:
            raise RvcxError("stream_open: one speaker id and one pitch per stream")
        cfg = StreamCfg(int(sid.shape[0]), int(block_frames), int(context_frames), int(crossfade_frames), int(search_frames))
        io = StreamIO(int(in_rate), int(in_channels), int(out_rate), 0)
        h = C.c_int(0)
        if any(v is not None for v in (denoise_in, denoise_out, formant_in, formant_out)):
            # stage 16 on the 16 kHz block in front of the ring and / or on what leaves, in front of the board; stage 19 behind
            # it on either side.  Without a formant side the session is opened as it was before stage 19 existed
            dsides = [None if v is None else _live_denoise(v) for v in (denoise_in, denoise_out)]
            fsides = [None if v is None else _live_formant(v) for v in (formant_in, formant_out)]
            dn, fm = _stream_denoise(dsides), StreamFormant()
            for name, fs in zip(("inp", "out"), fsides):
                if fs is not None:
                    setattr(fm, name, StreamFormantSide(C.cast(C.pointer(fs), C.c_void_p)))
            fx = None if values is None else FxParams.make(values, 0, 0)
            front = (self._h, int(model_id), C.byref(cfg), C.byref(io), None if fx is None else C.byref(fx))
            back = (C.byref(params), sid.ctypes.data, pit.ctypes.data, C.byref(h))
            if fsides == [None, None]:
                self._ck(lib().rvcx_stream_open_dn(*front, C.byref(dn), *back), "stream_open")
            else:
                self._ck(lib().rvcx_stream_open_fm(*front, None if dsides == [None, None] else C.byref(dn), C.byref(fm), *back),
                         "stream_open")
            se = StreamSession(self, int(h.value), cfg, io, self.synth_upp(model_id))
            se.effects = values
            se.denoise = [None if sd is None else sd[0].values() for sd in dsides]
            se.formant = [None if fs is None else fs.values() for fs in fsides]
            return se
        if values is None:
            self._ck(lib().rvcx_stream_open_io(self._h, int(model_id), C.byref(cfg), C.byref(io), C.byref(params),
                                               _p(sid, C.c_int32), _p(pit), C.byref(h)), "stream_open")
        else:
            fx = FxParams.make(values, 0, 0)
            self._ck(lib().rvcx_stream_open_fx(self._h, int(model_id), C.byref(cfg), C.byref(io), C.byref(fx), C.byref(params),
                                               sid.ctypes.data, pit.ctypes.data, C.byref(h)), "stream_open")
        se = StreamSession(self, int(h.value), cfg, io, self.synth_upp(model_id))
        se.effects = values
        return se

    def stream_fx(self, x, sr: int, block_frames: int, params, stages=None) -> np.ndarray:
        """rvcx_op_stream_fx: a session's effects board without a session.  x (S, frames) or (S, frames, 2) float32, cut into
        blocks of block_frames * sr / 100 frames and sent through the state and kernels a session runs per step ->
        (S, frames, 2).  params: a dict of add_effects names laid over FX_UI_DEFAULTS, or an FxParams.  stages: the stage
        numbers 1 .. 7 to run (None: all); the others are skipped like identities."""
        x = f32(x)
        if x.ndim not in (2, 3):
            raise RvcxError("stream_fx: x must be (S, frames) or (S, frames, channels)")
        S, frames, ch = x.shape[0], x.shape[1], (1 if x.ndim == 2 else x.shape[2])
        fx = FxParams.make(fx_values(params), 0, 0)
        mask = 0x7F if stages is None else sum(1 << (int(k) - 1) for k in set(stages))
        y = np.empty((S, frames, 2), np.float32)
        self._ck(lib().rvcx_op_stream_fx(self._h, x.ctypes.data, S, C.c_int64(frames), ch, int(sr), int(block_frames),
                                         C.byref(fx), mask, y.ctypes.data), "op_stream_fx")
        return y

    def stream_denoise(self, x, sr: int, block_frames: int, params=None, noise=None, taps=False):
        """rvcx_op_stream_denoise: a session's noise gate without a session.  x (S, frames) float32 at rate sr, cut into blocks
        of block_frames * sr / 100 samples and sent through the state and kernel a session runs per step -> (S, frames),
        delayed by stream_denoise_delay(sr).  params: a dict of LiveDenoiseParams values or a LiveDenoiseParams; noise: the
        clip of mode 0 (a numpy array, or an int device pointer with its length as a pair).  taps=True: (y, dict of S, m
        (S, T, nb) and f (mode 1))."""
        x = f32(x)
        if x.ndim != 2:
            raise RvcxError("stream_denoise: x must be (S, frames)")
        S, frames = x.shape
        p, z = _live_denoise(params, sr)
        zp, zn = None, 0
        if isinstance(noise, tuple):
            zp, zn = int(noise[0]), int(noise[1])
        else:
            z = z if noise is None else f32(noise)
            if z is not None:
                if z.ndim != 1:
                    raise RvcxError("stream_denoise: the noise clip must be one channel of shape (samples,)")
                zp, zn = z.ctypes.data, z.shape[0]
        y = np.full((S, frames), np.nan, np.float32)
        rate_ok = lib().rvcx_stream_denoise_delay(int(sr)) > 0      # (a refused rate: the library says so below)
        t = _live_taps(S, frames, sr, p.mode, taps, False) if rate_ok else {}
        self._ck(lib().rvcx_op_stream_denoise(self._h, x.ctypes.data, S, C.c_int64(frames), int(sr), int(block_frames), C.byref(p),
                                              zp, C.c_int64(zn), y.ctypes.data,
                                              *[t[k].ctypes.data if k in t else None for k in ("S", "f", "m")]),
                 "op_stream_denoise")
        return (y, t) if taps else y

    def stream_formant(self, x, sr: int, block_frames: int, params=None, taps=False, history=None):
        """rvcx_op_stream_formant: a session's formant shift without a session.  x (S, frames) float32 at rate sr, cut into blocks
        of block_frames * sr / 100 samples and sent through the state and kernels a session runs per step -> (S, frames),
        delayed by stream_formant_delay(sr).  params: a dict of LiveFormantParams values or a LiveFormantParams.  history: further
        (block, params) pairs in ascending block order -- what set_formant in front of step `block` leaves in a session.
        taps=True: (y, dict of E, g (S, T, nb) and s (S, T))."""
        x = f32(x)
        if x.ndim != 2:
            raise RvcxError("stream_formant: x must be (S, frames)")
        S, frames = x.shape
        plist = [_live_formant(params, sr)] + [_live_formant(q, sr) for _, q in (history or [])]
        arr = (LiveFormantParams * len(plist))(*plist)
        at = np.asarray([0] + [int(k) for k, _ in (history or [])], np.int64)
        y = np.full((S, frames), np.nan, np.float32)
        rate_ok = lib().rvcx_stream_formant_delay(int(sr)) > 0      # (a refused rate: the library says so below)
        t = _live_formant_taps(S, frames, sr, taps, False) if rate_ok else {}
        self._ck(lib().rvcx_op_stream_formant_history(self._h, x.ctypes.data, S, C.c_int64(frames), int(sr), int(block_frames),
                                                      len(plist), arr, at.ctypes.data, y.ctypes.data,
                                                      *[t[k].ctypes.data if k in t else None for k in ("E", "g", "s")]),
                 "op_stream_formant")
        return (y, t) if taps else y

    def load_rmvpe(self, cfg_struct, state: dict):
        tbl, keep = make_table(state)
        self._ck(lib().rvcx_load_rmvpe(self._h, C.byref(cfg_struct), tbl, len(tbl)), "load_rmvpe")
        self.rmvpe_loaded = True

    def load_fcpe(self, cfg_struct, state: dict):
        tbl, keep = make_table(state)
        self._ck(lib().rvcx_load_fcpe(self._h, C.byref(cfg_struct), tbl, len(tbl)), "load_fcpe")
        self.fcpe_loaded = True

    def load_crepe(self, state: dict):
        """torchcrepe's model.Crepe state dict (capacity read off the shapes)."""
        tbl, keep = make_table(state)
        self._ck(lib().rvcx_load_crepe(self._h, tbl, len(tbl)), "load_crepe")
        self.crepe_loaded = True

    @staticmethod
    def crepe_frames(n: int, hop: int) -> int:
        return int(lib().rvcx_crepe_frames(C.c_int64(int(n)), int(hop)))

    def crepe_predict(self, x, hop, fmin, fmax, dither=None, seed=0, return_parts=False):
        """get_f0_crepe up to the resize: x / quantile -> torchcrepe.predict(..., batch_size=2*hop, pad=True): pitch (F,)
        [, sigmoid outputs (F, 360), Viterbi bins (F,)]."""
        x = f32(x)
        F = self.crepe_frames(x.shape[0], hop)
        pitch = np.empty(F, np.float32)
        probs = np.empty((360, F), np.float32) if return_parts else None
        bins = np.empty(F, np.int32) if return_parts else None
        d = None if dither is None else f32(dither)
        if d is not None and d.shape[0] < F:
            raise RvcxError("crepe dither shorter than the frame count")
        self._ck(lib().rvcx_crepe_predict(self._h, _p(x), C.c_int64(x.shape[0]), int(hop), C.c_float(fmin), C.c_float(fmax),
                                          _p(d), C.c_uint64(seed), _p(pitch), _p(probs), _p(bins, C.c_int32)), "crepe_predict")
        if return_parts:
            return pitch, np.ascontiguousarray(probs.T), bins
        return pitch

    def crepe_decode(self, probs, batch, fmin, fmax, dither):
        """core.postprocess + Viterbi + bins_to_frequency on sigmoid outputs (F, 360): (pitch (F,), bins (F,))."""
        pr = np.ascontiguousarray(f32(probs).T)
        F = pr.shape[1]
        d = f32(dither)
        pitch, bins = np.empty(F, np.float32), np.empty(F, np.int32)
        self._ck(lib().rvcx_op_crepe_decode(self._h, _p(pr), C.c_int64(F), int(batch), C.c_float(fmin), C.c_float(fmax),
                                            _p(d), _p(pitch), _p(bins, C.c_int32)), "crepe_decode")
        return pitch, bins

    def get_f0_crepe_x(self, x, p_len, params: "Params", inp_f0=None, dither=None):
        """VC.get_f0(..., "mangio-crepe", hop_length=params.hop_length) on the padded signal: (coarse, f0) of p_len frames."""
        x = f32(x)
        coarse, f0 = np.empty(int(p_len), np.int32), np.empty(int(p_len), np.float32)
        tab = None if inp_f0 is None else np.ascontiguousarray(inp_f0, dtype=np.float32).reshape(-1, 2)
        d = None if dither is None else f32(dither)
        self._ck(lib().rvcx_get_f0_crepe_x(self._h, _p(x), C.c_int64(x.shape[0]), C.c_int64(int(p_len)), C.byref(params),
                                           _p(tab), 0 if tab is None else tab.shape[0], _p(d),
                                           C.c_int64(0 if d is None else d.shape[0]), _p(coarse, C.c_int32), _p(f0)),
                 "get_f0_crepe_x")
        return coarse, f0

    def fcpe_f0(self, audio, threshold=0.05, return_salience=False, return_mel=False):
        """FCPEInfer.__call__: audio (n,) or (B,n) at 16 kHz -> Hz (B, n//160 + 1) [, salience (B,F,360)] [, mel (B,128,F)]."""
        audio = f32(audio)
        if audio.ndim == 1:
            audio = audio[None]
        B, n = audio.shape
        F = 1 + n // 160
        f0 = np.empty((B, F), np.float32)
        sal = np.empty((B, F, 360), np.float32) if return_salience else None
        mel = np.empty((B, 128, F), np.float32) if return_mel else None
        self._ck(lib().rvcx_fcpe_f0(self._h, B, _p(audio), C.c_int64(n), C.c_float(threshold), _p(f0), _p(sal),
                                    _p(mel)), "fcpe_f0")
        out = (f0,) + ((sal,) if return_salience else ()) + ((mel,) if return_mel else ())
        return out if len(out) > 1 else f0

    def get_f0_fcpe_x(self, x, p_len, params: "Params"):
        """VC.get_f0(..., f0_method="fcpe") on the already padded + filtered signal: (coarse, f0) of p_len frames."""
        x = f32(x)
        coarse = np.empty(int(p_len), np.int32)
        f0 = np.empty(int(p_len), np.float32)
        self._ck(lib().rvcx_get_f0_fcpe_x(self._h, _p(x), C.c_int64(x.shape[0]), C.c_int64(int(p_len)),
                                          C.byref(params), _p(coarse, C.c_int32), _p(f0)), "get_f0_fcpe_x")
        return coarse, f0

    def fcpe_post(self, raw, p_len, pitch=0.0, f0_min=50, f0_max=1100):
        raw = f32(raw)
        coarse = np.empty(int(p_len), np.int32)
        f0 = np.empty(int(p_len), np.float32)
        self._ck(lib().rvcx_op_fcpe_post(self._h, _p(raw), int(raw.shape[0]), int(p_len), C.c_double(pitch),
                                         C.c_double(f0_min), C.c_double(f0_max), _p(coarse, C.c_int32), _p(f0)),
                 "fcpe_post")
        return coarse, f0

    def load_hubert(self, cfg_struct, state: dict):
        tbl, keep = make_table(state)
        self._ck(lib().rvcx_load_hubert(self._h, C.byref(cfg_struct), tbl, len(tbl)), "load_hubert")

    def rmvpe_f0(self, audio, thred=0.03, f0_min=50, f0_max=1100, return_hidden=False):
        audio = f32(audio)
        if audio.ndim == 1:
            audio = audio[None]
        B, n = audio.shape
        F = 1 + n // 160
        f0 = np.empty((B, F), np.float32)
        hid = np.empty((B, F, 360), np.float32) if return_hidden else None
        self._ck(lib().rvcx_rmvpe_f0(self._h, B, _p(audio), C.c_int64(n), C.c_float(thred), C.c_float(f0_min),
                                     C.c_float(f0_max), _p(f0), _p(hid)), "rmvpe_f0")
        return (f0, hid) if return_hidden else f0

    def rmvpe_mel(self, audio):
        audio = f32(audio)
        if audio.ndim == 1:
            audio = audio[None]
        B, n = audio.shape
        mel = np.empty((B, 128, 1 + n // 160), np.float32)
        self._ck(lib().rvcx_rmvpe_mel(self._h, B, _p(audio), C.c_int64(n), _p(mel)), "rmvpe_mel")
        return mel

    def hubert_frames(self, n: int) -> int:
        return int(lib().rvcx_hubert_frames(self._h, C.c_int64(n)))

    def hubert_features(self, wav, embed_dim, output_layer=12):
        wav = f32(wav)
        if wav.ndim == 1:
            wav = wav[None]
        B, n = wav.shape
        T = self.hubert_frames(n)
        out = np.empty((B, T, embed_dim), np.float32)
        self._ck(lib().rvcx_hubert_features(self._h, B, _p(wav), C.c_int64(n), output_layer, _p(out)),
                 "hubert_features")
        return out

    def bigru(self, x, sd, prefix="fc.0.gru"):
        x = f32(x)
        B, T, I = x.shape
        g = lambda n: f32(sd[f"{prefix}.{n}"])
        H = g("weight_hh_l0").shape[1]
        y = np.empty((B, T, 2 * H), np.float32)
        a = [g("weight_ih_l0"), g("weight_hh_l0"), g("bias_ih_l0"), g("bias_hh_l0"), g("weight_ih_l0_reverse"),
             g("weight_hh_l0_reverse"), g("bias_ih_l0_reverse"), g("bias_hh_l0_reverse")]
        self._ck(lib().rvcx_op_bigru(self._h, _p(x), *[_p(t) for t in a], _p(y), B, T, I, H), "op_bigru")
        return y

    def load_index(self, big_npy):
        if big_npy is None:
            self._ck(lib().rvcx_load_index(self._h, None, C.c_int64(0), 0), "load_index")
            return
        b = f32(big_npy)
        self._ck(lib().rvcx_load_index(self._h, _p(b), C.c_int64(b.shape[0]), int(b.shape[1])), "load_index")

    def load_index_ivf(self, big_npy, centroids, assign, nprobe=1):
        """faiss "IVF{nlist},Flat": stored vectors + coarse centroids + list id per vector; nprobe = 1 search."""
        b, c = f32(big_npy), f32(centroids)
        a = i32(assign)
        self._ck(lib().rvcx_load_index_ivf(self._h, _p(b), C.c_int64(b.shape[0]), int(b.shape[1]), _p(c), int(c.shape[0]),
                                           _p(a, C.c_int32), int(nprobe)), "load_index_ivf")

    def index_blend(self, feats, index_rate):
        f = f32(feats).copy()
        T = f.shape[0]
        ids = np.empty((T, 8), np.int64)
        dist = np.empty((T, 8), np.float32)
        self._ck(lib().rvcx_index_blend(self._h, _p(f), T, C.c_float(index_rate), _p(ids, C.c_int64), _p(dist)),
                 "index_blend")
        return f, ids, dist

    # ---- index building (rvcx.h "index building"; index_build.py is the product-side caller) ----
    def kmeans(self, x, init, iters=1):
        """`iters` Lloyd iterations from the centroids `init` -> dict(centroids (k, dim), assign (n) of the LAST assignment
        step, counts (k) = its histogram, objective (iters) float64, splits (iters) empty clusters treated per iteration)."""
        x, init = f32(x), f32(init)
        if x.ndim != 2 or init.ndim != 2 or x.shape[1] != init.shape[1]:
            raise ValueError("kmeans: x (n, dim) and init (k, dim) must be matrices of one width")
        (n, dim), k, iters = x.shape, init.shape[0], int(iters)
        cent = np.empty((k, dim), np.float32)
        assign, counts = np.empty(n, np.int32), np.empty(k, np.int32)
        obj, splits = np.zeros(max(iters, 1), np.float64), np.zeros(max(iters, 1), np.int32)
        self._ck(lib().rvcx_kmeans(self._h, x.ctypes.data, n, dim, init.ctypes.data, k, iters, cent.ctypes.data,
                                   assign.ctypes.data, counts.ctypes.data, obj.ctypes.data, splits.ctypes.data), "kmeans")
        return dict(centroids=cent, assign=assign, counts=counts, objective=obj, splits=splits)

    def ivf_assign(self, x, centroids):
        """list id (int32) of every row: the coarse quantiser of the IVF search, the first minimum on ties"""
        x, c = f32(x), f32(centroids)
        if x.ndim != 2 or c.ndim != 2 or x.shape[1] != c.shape[1]:
            raise ValueError("ivf_assign: x (n, dim) and centroids (nlist, dim) must be matrices of one width")
        a = np.empty(x.shape[0], np.int32)
        self._ck(lib().rvcx_ivf_assign(self._h, x.ctypes.data, x.shape[0], x.shape[1], c.ctypes.data, c.shape[0],
                                       a.ctypes.data), "ivf_assign")
        return a

    def index_features(self, wav, out_dim):
        """the rows an index is built from, (B, T, out_dim): HuBERT layer 12 (out_dim = embed_dim, RVC v2) or final_proj of
        layer 9 (out_dim = its width, RVC v1) -- what VC.vc hands the retrieval blend"""
        wav = f32(wav)
        if wav.ndim == 1:
            wav = wav[None]
        B, n = wav.shape
        out = np.empty((B, self.hubert_frames(n), int(out_dim)), np.float32)
        self._ck(lib().rvcx_index_features(self._h, B, _p(wav), C.c_int64(n), int(out_dim), _p(out)), "index_features")
        return out

    def kmeans_exhaustive(self) -> int:
        """rows of the last kmeans() call (over all its iterations) that took the exact scan over every centroid"""
        return int(lib().rvcx_kmeans_exhaustive(self._h))

    def highpass(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        self._ck(lib().rvcx_op_highpass(self._h, _p(x, C.c_double), _p(y, C.c_double), C.c_int64(x.shape[0])),
                 "op_highpass")
        return y

    def get_f0(self, wav, params: "Params"):
        wav = f32(wav)
        n = wav.shape[0]
        cap = (n + 2 * 16000 * params.x_pad) // 160 + 8
        coarse = np.empty(cap, np.int32)
        f0 = np.empty(cap, np.float32)
        pl = C.c_int64(0)
        self._ck(lib().rvcx_get_f0(self._h, _p(wav), C.c_int64(n), C.byref(params), _p(coarse, C.c_int32), _p(f0),
                                   C.byref(pl)), "get_f0")
        return coarse[:pl.value].copy(), f0[:pl.value].copy()

    def out_capacity(self, model_id, n, params) -> int:
        return int(lib().rvcx_out_len(self._h, model_id, C.c_int64(n), C.byref(params)))

    def noise_capacity(self, model_id, n, params) -> int:
        return int(lib().rvcx_noise_len(self._h, model_id, C.c_int64(n), C.byref(params)))

    def _convert_tables(self, what, model_id, wavs, params, noises, want_f32, inp_f0, crepe_dither):
        """The argument tables of rvcx_convert_batch* / rvcx_convert_submit for a list of numpy clips.  float64 clips (what
        the reference's load_audio returns) cross the ABI as float64; anything else as float32.  `keep` holds every array
        the tables point into."""
        B = len(wavs)
        t = types.SimpleNamespace(B=B)
        t.is64 = B > 0 and all(np.asarray(w).dtype == np.float64 for w in wavs)
        wavs = [np.ascontiguousarray(w, dtype=np.float64 if t.is64 else np.float32) for w in wavs]
        t.ns = (C.c_int64 * B)(*[w.shape[0] for w in wavs])
        wt = C.c_double if t.is64 else C.c_float
        t.wp = (C.POINTER(wt) * B)(*[_p(w, wt) for w in wavs])
        caps = [self.out_capacity(model_id, w.shape[0], params) for w in wavs]
        if any(c < 0 for c in caps):
            raise RvcxError(f"{what}: no voice model with id {model_id} is resident in this context")
        t.outs = [np.empty(c, np.int16) for c in caps]
        t.op = (C.POINTER(C.c_int16) * B)(*[_p(o, C.c_int16) for o in t.outs])
        t.f32s, t.fp = None, None
        if want_f32:
            t.f32s = [np.empty(c, np.float32) for c in caps]
            t.fp = (C.POINTER(C.c_float) * B)(*[_p(o) for o in t.f32s])
        nz, t.npp = None, None
        if noises is not None:
            nz = []
            for w, nv in zip(wavs, noises):
                if nv is None:
                    nz.append(None)
                    continue
                cap = self.noise_capacity(model_id, w.shape[0], params)
                buf = np.zeros(cap, np.float32)
                nv = f32(nv).ravel()
                if nv.shape[0] > cap:
                    raise RvcxError("noise longer than rvcx_noise_len")
                buf[:nv.shape[0]] = nv
                nz.append(buf)
            t.npp = (C.POINTER(C.c_float) * B)(*[_p(b) for b in nz])
        t.out_n = (C.c_int64 * B)()
        t.ex, tabs, dith = None, None, None
        if inp_f0 is not None or crepe_dither is not None:
            # f0 files: (rows, 2) float32 tables of (time [s], f0 [Hz]) per utterance; crepe dither: one float per frame
            tabs = [None if (inp_f0 is None or x is None) else np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 2)
                    for x in (inp_f0 if inp_f0 is not None else [None] * B)]
            dith = [None if (crepe_dither is None or d is None) else f32(d).ravel()
                    for d in (crepe_dither if crepe_dither is not None else [None] * B)]
            t.ex = (UttExtra * B)(*[UttExtra(_p(x), 0 if x is None else x.shape[0], 0, _p(d), 0 if d is None else d.shape[0])
                                    for x, d in zip(tabs, dith)])
        t.wv = (C.c_void_p * B)(*[w.ctypes.data for w in wavs])
        t.keep = (wavs, nz, tabs, dith, t.outs, t.f32s, t.out_n, t.ns, t.wp, t.wv, t.op, t.fp, t.npp, t.ex)
        return t

    def convert_batch(self, model_id, wavs, params: "Params", noises=None, want_f32=False, inp_f0=None, crepe_dither=None):
        """VC.pipeline for a list of 16 kHz mono clips -> list of int16 arrays (and the pre-quantisation
        float waveforms when want_f32).  float64 clips (what the reference's load_audio returns) cross the
        ABI as float64; anything else as float32.  Clips of one length class are converted as ragged micro-batches."""
        t = self._convert_tables("convert_batch", model_id, wavs, params, noises, want_f32, inp_f0, crepe_dither)
        if t.ex is not None:
            self._ck(lib().rvcx_convert_batch_ex(self._h, model_id, t.B, t.wv, 1 if t.is64 else 0, t.ns, C.byref(params),
                                                 t.npp, t.ex, t.op, t.fp, t.out_n), "convert_batch_ex")
        else:
            fn = lib().rvcx_convert_batch_f64 if t.is64 else lib().rvcx_convert_batch
            self._ck(fn(self._h, model_id, t.B, t.wp, t.ns, C.byref(params), t.npp, t.op, t.fp, t.out_n), "convert_batch")
        pcm = [o[:t.out_n[i]].copy() for i, o in enumerate(t.outs)]
        if want_f32:
            return pcm, [o[:t.out_n[i]].copy() for i, o in enumerate(t.f32s)]
        return pcm

    def convert_submit(self, model_id, wavs, params: "Params", noises=None, want_f32=False, inp_f0=None,
                       crepe_dither=None) -> "Ticket":
        """convert_batch without the wait: enqueues the conversion and returns a Ticket; Ticket.wait() returns what
        convert_batch returns.  Two tickets may be in flight per context (a third submit completes the oldest first)."""
        t = self._convert_tables("convert_submit", model_id, wavs, params, noises, want_f32, inp_f0, crepe_dither)
        tid = C.c_int64(0)
        cast = lambda a: None if a is None else C.cast(a, C.c_void_p)  # noqa: E731
        self._ck(lib().rvcx_convert_submit(self._h, model_id, t.B, cast(t.wv), 1 if t.is64 else 0, cast(t.ns), C.byref(params),
                                           cast(t.npp), cast(t.ex), cast(t.op), cast(t.fp), cast(t.out_n), C.byref(tid)),
                 "convert_submit")
        return Ticket(self, tid.value, t.keep, t.outs, t.f32s, t.out_n)

    def convert_submit_raw(self, model_id, wav_ptrs, ns, params, out_ptrs, f32_ptrs=None, noise_ptrs=None) -> "Ticket":
        """convert_submit with raw (host or device) addresses of float32 clips, as convert_batch_raw takes them; the
        caller keeps the buffers valid until Ticket.wait(), which returns the produced sample counts."""
        B = len(wav_ptrs)
        wp = (C.c_void_p * B)(*wav_ptrs)
        op = (C.c_void_p * B)(*out_ptrs)
        fp = None if f32_ptrs is None else (C.c_void_p * B)(*f32_ptrs)
        npp = None if noise_ptrs is None else (C.c_void_p * B)(*noise_ptrs)
        nn = (C.c_int64 * B)(*ns)
        out_n = (C.c_int64 * B)()
        tid = C.c_int64(0)
        self._ck(lib().rvcx_convert_submit(self._h, model_id, B, wp, 0, nn, C.byref(params), npp, None, op, fp, out_n,
                                           C.byref(tid)), "convert_submit")
        return Ticket(self, tid.value, (out_n,), None, None, out_n)

    def convert_inflight(self) -> int:
        """tickets submitted and not yet completed on the device"""
        return int(lib().rvcx_convert_inflight(self._h))

    def convert_batch_raw(self, model_id, wav_ptrs, ns, params, out_ptrs, f32_ptrs=None, noise_ptrs=None):
        """Same as convert_batch but with raw (host or device) addresses of float32 clips: nothing is staged
        through numpy.  Returns the list of produced sample counts."""
        B = len(wav_ptrs)
        wp = (C.c_void_p * B)(*wav_ptrs)
        op = (C.c_void_p * B)(*out_ptrs)
        fp = None if f32_ptrs is None else (C.c_void_p * B)(*f32_ptrs)
        npp = None if noise_ptrs is None else (C.c_void_p * B)(*noise_ptrs)
        nn = (C.c_int64 * B)(*ns)
        out_n = (C.c_int64 * B)()
        self._ck(lib().rvcx_convert_batch(self._h, model_id, B, wp, nn, C.byref(params), npp, op, fp, out_n),
                 "convert_batch")
        return [int(v) for v in out_n]

    def micro_batch(self, model_id, n, params) -> int:
        return int(lib().rvcx_micro_batch(self._h, model_id, C.c_int64(n), C.byref(params)))

    def bucket_length(self, model_id, n, params) -> int:
        """the length whose launch geometry an n-sample utterance runs with: equal values share micro-batches"""
        return int(lib().rvcx_bucket_length(self._h, model_id, C.c_int64(n), C.byref(params)))

    def last_micro_batches(self):
        """member counts of the micro-batches the last convert_batch call formed"""
        cap = 4096
        buf = (C.c_int32 * cap)()
        k = int(lib().rvcx_last_micro_batches(self._h, buf, cap))
        return [int(buf[i]) for i in range(min(k, cap))]

    def last_cuts(self):
        """the cut points (the reference's opt_ts) the last convert_batch call cut each clip at, in call order"""
        k = int(lib().rvcx_last_cuts(self._h, None, 0))
        buf = np.zeros(max(k, 1), np.int64)
        lib().rvcx_last_cuts(self._h, buf.ctypes.data, k)
        out, i = [], 0
        while i < k:
            c = int(buf[i])
            out.append([int(v) for v in buf[i + 1:i + 1 + c]])
            i += 1 + c
        return out

    def get_f0_x(self, x, params: "Params"):
        """VC.get_f0 on the already padded + filtered signal: (coarse, f0) of 1 + n/160 frames."""
        x = f32(x)
        F = 1 + x.shape[0] // 160
        coarse = np.empty(F, np.int32)
        f0 = np.empty(F, np.float32)
        self._ck(lib().rvcx_get_f0_x(self._h, _p(x), C.c_int64(x.shape[0]), C.byref(params), _p(coarse, C.c_int32),
                                     _p(f0)), "get_f0_x")
        return coarse, f0

    def get_f0_x_ex(self, x, p_len, params: "Params", inp_f0=None):
        """VC.get_f0 in full (F0 model by params.f0_method, pitch shift, optional f0-file table, coarse) on the padded
        signal: (coarse, f0) of 1 + n/160 frames (rmvpe+) or p_len frames (fcpe)."""
        x = f32(x)
        cap = max(int(p_len), 1 + x.shape[0] // 160)
        coarse = np.empty(cap, np.int32)
        f0 = np.empty(cap, np.float32)
        tab = None if inp_f0 is None else np.ascontiguousarray(inp_f0, dtype=np.float32).reshape(-1, 2)
        got = C.c_int64(0)
        self._ck(lib().rvcx_get_f0_x_ex(self._h, _p(x), C.c_int64(x.shape[0]), C.c_int64(int(p_len)), C.byref(params),
                                        _p(tab), 0 if tab is None else tab.shape[0], _p(coarse, C.c_int32), _p(f0),
                                        C.byref(got)), "get_f0_x_ex")
        return coarse[:got.value].copy(), f0[:got.value].copy()

    def resample(self, audio, sr_in: int, sr_out: int, kind: int = -1) -> np.ndarray:
        """librosa.resample(librosa.to_mono(audio.T), sr_in -> sr_out): audio (frames,) or (frames, channels) -> float64 mono.
        kind -1: the default filter (kaiser_hq: a Kaiser design to soxr_hq's published targets), 1: resampy's kaiser_best"""
        a = np.ascontiguousarray(audio, dtype=np.float64)
        frames, ch = a.shape[0], (1 if a.ndim == 1 else a.shape[1])
        n_out = int(lib().rvcx_resample_len(C.c_int64(frames), int(sr_in), int(sr_out)))
        y = np.empty(max(n_out, 0), np.float64)
        self._ck(lib().rvcx_resample_f64_kind(self._h, _p(a, C.c_double), C.c_int64(frames), ch, int(sr_in), int(sr_out),
                                              int(kind), _p(y, C.c_double)), "resample_f64")
        return y

    # ---- post-production (rvcx.h "post-production"): signals are float32 (frames,) or (frames, channels) -------------------
    @staticmethod
    def _fx_in(x):
        x = f32(x)
        if x.ndim not in (1, 2) or x.shape[0] < 1:
            raise RvcxError("fx: array of shape (frames,) or (frames, channels) with at least one frame expected")
        return x, (1 if x.ndim == 1 else x.shape[1])

    def _fx_items(self, items, what):
        """the input tables of a batched call: (arrays, channels, B, pointer table, frame counts)"""
        xs = [self._fx_in(x) for x in items]
        if not xs or any(ch != xs[0][1] for _, ch in xs):
            raise RvcxError(f"{what}: a non-empty list of items with one channel count expected")
        B = len(xs)
        xp = (C.c_void_p * B)(*[x.ctypes.data for x, _ in xs])
        n = (C.c_int64 * B)(*[x.shape[0] for x, _ in xs])
        return [x for x, _ in xs], xs[0][1], B, xp, n

    @staticmethod
    def _fx_table(arrays):
        """a pointer table over a list of arrays; None (or an array without a frame) gives a null entry"""
        return (C.c_void_p * len(arrays))(*[None if a is None or a.shape[0] == 0 else a.ctypes.data for a in arrays])

    def _named_timing(self, names):
        """rvcx_last_timing's nine slots under a stage's names for them (names starting with "_" are left out)"""
        ms = (C.c_float * 9)()
        lib().rvcx_last_timing(self._h, ms)
        return {k: float(v) for k, v in zip(names, ms) if not k.startswith("_")}

    def fx_chain(self, items, params: "FxParams"):
        """rvcx_fx_chain: the whole board on a list of (frames, 2) float32 arrays in one call -> list of arrays"""
        xs, ch, B, xp, n = self._fx_items(items, "fx_chain")
        if ch != params.channels:
            raise RvcxError("fx_chain: every item needs params.channels channels")
        ys = [np.empty_like(x) for x in xs]
        self._ck(lib().rvcx_fx_chain(self._h, B, xp, n, C.byref(params), self._fx_table(ys)), "fx_chain")
        return ys

    def fx_last_passes(self):
        """({compressor, gate x^2 follower, gate peak follower} relaxation passes, groups) of the last post-production call"""
        p = (C.c_int32 * 3)()
        g = lib().rvcx_fx_last_passes(self._h, p)
        return [int(v) for v in p], int(g)

    def fx_last_timing(self):
        """per-stage device ms of the last fx_chain call (rvcx_last_timing's nine slots under their post-production names)"""
        return self._named_timing(["highpass", "compressor", "gate", "reverb", "low_shelf", "high_shelf", "chorus", "copies",
                                   "total"])

    # ---- loudness, true peak, limiter, master (rvcx.h stages 9 - 12) --------------------------------------------------------
    def fx_loudness(self, items, sr, momentary=False):
        """rvcx_fx_loudness on a list of signals of one rate and channel count in one call -> list of (LUFS, dBTP), with
        momentary=True of (LUFS, dBTP, float32 momentary values)"""
        xs, ch, B, xp, n = self._fx_items(items, "fx_loudness")
        L, tp = np.zeros(B, np.float64), np.zeros(B, np.float64)
        ms = [np.zeros(max(fx_momentary_len(x.shape[0], sr), 1), np.float32) for x in xs] if momentary else None
        mp = self._fx_table(ms) if momentary else None
        self._ck(lib().rvcx_fx_loudness(self._h, B, xp, n, ch, int(sr), L.ctypes.data, tp.ctypes.data, mp), "fx_loudness")
        if momentary:
            return [(float(L[b]), float(tp[b]), ms[b][:fx_momentary_len(xs[b].shape[0], sr)]) for b in range(B)]
        return [(float(L[b]), float(tp[b])) for b in range(B)]

    def fx_loudness_timing(self):
        """per-stage device ms of the last fx_loudness call"""
        return self._named_timing(["copies_in", "chunk_states", "carry", "kweight_energy", "gates", "true_peak", "copies_out", "unused",
                                   "total"])

    def fx_master_timing(self):
        """per-stage device ms of the last fx_master call"""
        return self._named_timing(["stem_loudness", "mix", "mix_loudness", "scale_true_peak", "limiter_gain", "gain_int16",
                                   "result_meters", "copies", "total"])

    def fx_true_peak(self, x, want_p=False):
        """rvcx_op_fx_truepeak -> dBTP, or (dBTP, p[n])"""
        x, ch = self._fx_in(x)
        tp = C.c_double()
        p = np.zeros(x.shape[0], np.float32) if want_p else None
        self._ck(lib().rvcx_op_fx_truepeak(self._h, x.ctypes.data, x.shape[0], ch, None if p is None else p.ctypes.data,
                                           C.byref(tp)), "op_fx_truepeak")
        return (tp.value, p) if want_p else tp.value

    def fx_limit(self, x, sr, ceiling_db=-1.0, lookahead_ms=2.0, release_ms=100.0, want_gain=False):
        """rvcx_op_fx_limit -> y, or (y, s[n])"""
        x, ch = self._fx_in(x)
        y, g = np.empty_like(x), (np.zeros(x.shape[0], np.float32) if want_gain else None)
        self._ck(lib().rvcx_op_fx_limit(self._h, x.ctypes.data, x.shape[0], ch, int(sr), float(ceiling_db), float(lookahead_ms),
                                        float(release_ms), y.ctypes.data, None if g is None else g.ctypes.data), "op_fx_limit")
        return (y, g) if want_gain else y

    def fx_master(self, vocals, insts, sr, target_lufs=-16.0, vocal_offset_lu=0.0, ceiling_dbtp=-1.0):
        """rvcx_fx_master: lists of (n_v, 2) and (n_i, 2) float32 stems of one rate -> (list of (n_v, 2) int16, list of
        report dicts)"""
        vs = [_stereo_f32(v, "fx_master") for v in vocals]
        ms = [_stereo_f32(m, "fx_master") for m in insts]
        if not vs or len(vs) != len(ms) or any(v.shape[0] < 1 for v in vs):
            raise RvcxError("fx_master: as many instrumentals as vocals, at least one, every vocal with a frame")
        B = len(vs)
        ys = [np.zeros((v.shape[0], 2), np.int16) for v in vs]
        nv = (C.c_int64 * B)(*[v.shape[0] for v in vs])
        ni = (C.c_int64 * B)(*[m.shape[0] for m in ms])
        rep = np.zeros((B, 7), np.float64)
        self._ck(lib().rvcx_fx_master(self._h, B, self._fx_table(vs), nv, self._fx_table(ms), ni, int(sr), float(target_lufs),
                                      float(vocal_offset_lu), float(ceiling_dbtp), self._fx_table(ys), rep.ctypes.data), "fx_master")
        return ys, [dict(zip(MASTER_REPORT, (float(r) for r in row))) for row in rep]

    # ---- time stretch and pitch shift (rvcx.h stages 13 and 14) -------------------------------------------------------------
    def fx_stretch(self, items, sr, P, Q):
        """rvcx_fx_stretch: a list of float32 signals of one rate and channel count, stretched by P / Q in one call"""
        xs, ch, B, xp, n = self._fx_items(items, "fx_stretch")
        ys = [np.zeros((max(fx_stretch_len(x.shape[0], P, Q), 1),) + x.shape[1:], np.float32) for x in xs]
        self._ck(lib().rvcx_fx_stretch(self._h, B, xp, n, ch, int(sr), int(P), int(Q), self._fx_table(ys)), "fx_stretch")
        return [y[:fx_stretch_len(x.shape[0], P, Q)] for x, y in zip(xs, ys)]

    def fx_pitch_shift(self, items, sr, semitones, preserve_formants=False, formant_params=None):
        """rvcx_fx_pitch_shift: every item shifted by `semitones` at its own length.  preserve_formants: stage 18
        (rvcx_fx_pitch_shift_formant), the envelope of each item put back onto its shifted copy; formant_params: the
        FxFormantParams of that transfer (its ratio is not read)"""
        xs, ch, B, xp, n = self._fx_items(items, "fx_pitch_shift")
        ys = [np.zeros_like(x) for x in xs]
        yp = self._fx_table(ys)
        if preserve_formants:
            p = (formant_params or FxFormantParams.make(sr, ch)).with_shape(sr, ch)
            self._ck(lib().rvcx_fx_pitch_shift_formant(self._h, B, xp, n, ch, int(sr), float(semitones), C.byref(p), yp),
                     "fx_pitch_shift_formant")
            return ys
        if formant_params is not None:
            raise RvcxError("fx_pitch_shift: formant_params without preserve_formants")
        self._ck(lib().rvcx_fx_pitch_shift(self._h, B, xp, n, ch, int(sr), float(semitones), yp), "fx_pitch_shift")
        return ys

    def fx_stretch_taps(self, x, sr, P, Q):
        """rvcx_op_fx_stretch_taps on one channel -> (y, dict of D (T + 2, nb, 2), own, TH (T + 2, nb) and R (J, nb))"""
        x, ch = self._fx_in(x)
        if ch != 1 or x.ndim != 1:
            raise RvcxError("fx_stretch_taps: one channel of shape (frames,) expected")
        n = x.shape[0]
        if fx_stretch_len(n, P, Q) < 0:
            raise RvcxError("fx_stretch_taps: 1 <= Q <= 2^20 and Q / 2 <= P <= 2 Q are required")
        y = np.zeros(max(fx_stretch_len(n, P, Q), 1), np.float32)
        t = _stretch_taps(n, sr, P, Q, True)
        self._ck(lib().rvcx_op_fx_stretch_taps(self._h, x.ctypes.data, n, int(sr), int(P), int(Q), y.ctypes.data, *_tap_ptrs(t)),
                 "op_fx_stretch_taps")
        return y[:fx_stretch_len(n, P, Q)], t

    def fx_stretch_timing(self):
        """per-kernel device ms of the last fx_stretch / fx_pitch_shift call"""
        return self._named_timing(["copies_in", "transforms", "owners", "scan", "inverse_transforms", "overlap_add", "resampler",
                                   "copies_out", "total"])

    # ---- noise reduction (rvcx.h stage 15) -------------------------------------------------------------------------------------
    def fx_denoise(self, items, sr, params=None, noise=None):
        """rvcx_fx_denoise: a list of float32 signals of one rate and channel count in one call -> list of arrays.  noise:
        one array for all items, or a list with one entry (an array or None) per item"""
        xs, ch, B, xp, n = self._fx_items(items, "fx_denoise")
        p = (params or FxDenoiseParams.make(sr, ch)).with_shape(sr, ch)
        if noise is None or isinstance(noise, np.ndarray):
            clips = [_denoise_clip(noise, ch, "fx_denoise")] * B
        else:
            clips = [_denoise_clip(z, ch, "fx_denoise") for z in noise]
            if len(clips) != B:
                raise RvcxError("fx_denoise: one noise entry per item expected")
        ys = [np.zeros_like(x) for x in xs]
        zn = (C.c_int64 * B)(*[0 if z is None else z.shape[0] for z in clips])
        self._ck(lib().rvcx_fx_denoise(self._h, B, xp, n, self._fx_table(clips), zn, C.byref(p), self._fx_table(ys)), "fx_denoise")
        return ys

    def fx_denoise_taps(self, x, sr, params=None, noise=None):
        """rvcx_op_fx_denoise_taps on one channel -> (y, dict of D (T, nb, 2), S, m (T, nb) and mu, sd (nb) or b (T, nb))"""
        x, ch = self._fx_in(x)
        if ch != 1 or x.ndim != 1:
            raise RvcxError("fx_denoise_taps: one channel of shape (frames,) expected")
        p = (params or FxDenoiseParams.make(sr, 1)).with_shape(sr, 1)
        z = _denoise_clip(noise, 1, "fx_denoise_taps")
        y = np.zeros_like(x)
        t = _denoise_taps(x.shape[0], p, True)
        self._ck(lib().rvcx_op_fx_denoise_taps(self._h, x.ctypes.data, x.shape[0], None if z is None else z.ctypes.data,
                                               0 if z is None else z.shape[0], C.byref(p), y.ctypes.data, *_denoise_tap_ptrs(t)),
                 "op_fx_denoise_taps")
        return y, t

    def fx_denoise_timing(self):
        """per-kernel device ms of the last fx_denoise call"""
        return self._named_timing(["copies_in", "analysis", "smoothing", "stats_or_floor", "mask", "synthesis", "overlap_add",
                                   "copies_out", "total"])

    # ---- formant shift (rvcx.h stages 17 and 18; stage 18 is fx_pitch_shift(preserve_formants=True)) --------------------------
    def fx_formant(self, items, sr, params=None, source=None):
        """rvcx_fx_formant: a list of float32 signals of one rate and channel count in one call -> list of arrays.  source:
        a list with one entry (an array of its item's shape, or None) per item"""
        xs, ch, B, xp, n = self._fx_items(items, "fx_formant")
        p = (params or FxFormantParams.make(sr, ch)).with_shape(sr, ch)
        if source is None:
            srcs = [None] * B
        else:
            if isinstance(source, np.ndarray) or len(source) != B:
                raise RvcxError("fx_formant: one source entry per item expected")
            srcs = [_formant_source(z, x, "fx_formant") for z, x in zip(source, xs)]
        ys = [np.zeros_like(x) for x in xs]
        self._ck(lib().rvcx_fx_formant(self._h, B, xp, n, self._fx_table(srcs), C.byref(p), self._fx_table(ys)), "fx_formant")
        return ys

    def fx_formant_taps(self, x, sr, params=None, source=None):
        """rvcx_op_fx_formant_taps on one channel -> (y, dict of D (T, nb, 2), E, Es, g (T, nb) and s (T))"""
        x, ch = self._fx_in(x)
        if ch != 1 or x.ndim != 1:
            raise RvcxError("fx_formant_taps: one channel of shape (frames,) expected")
        p = (params or FxFormantParams.make(sr, 1)).with_shape(sr, 1)
        z = _formant_source(source, x, "fx_formant_taps")
        y = np.zeros_like(x)
        t = _formant_taps(x.shape[0], p, True)
        self._ck(lib().rvcx_op_fx_formant_taps(self._h, x.ctypes.data, x.shape[0], None if z is None else z.ctypes.data,
                                               C.byref(p), y.ctypes.data, *_formant_tap_ptrs(t)), "op_fx_formant_taps")
        return y, t

    def fx_formant_timing(self):
        """device ms of the last fx_formant / fx_pitch_shift(preserve_formants=True) call"""
        return self._named_timing(["copies_in", "frames", "overlap_add", "copies_out", "_4", "_5", "_6", "pitch_shift", "total"])

    def fx_highpass(self, x, sr, fc=50.0):
        x, ch = self._fx_in(x)
        y = np.empty_like(x)
        self._ck(lib().rvcx_op_fx_highpass(self._h, x.ctypes.data, x.shape[0], ch, int(sr), float(fc), y.ctypes.data), "op_fx_highpass")
        return y

    def fx_compressor(self, x, sr, ratio, threshold_db, attack_ms=1.0, release_ms=100.0, want_env=False):
        x, ch = self._fx_in(x)
        y, e = np.empty_like(x), (np.zeros_like(x) if want_env else None)
        self._ck(lib().rvcx_op_fx_compressor(self._h, x.ctypes.data, x.shape[0], ch, int(sr), float(ratio), float(threshold_db),
                                             float(attack_ms), float(release_ms), y.ctypes.data,
                                             None if e is None else e.ctypes.data), "op_fx_compressor")
        return (y, e) if want_env else y

    def fx_gate(self, x, sr, threshold_db, ratio, attack_ms, release_ms, want_env=False):
        x, ch = self._fx_in(x)
        y, e = np.empty_like(x), (np.zeros_like(x) if want_env else None)
        self._ck(lib().rvcx_op_fx_gate(self._h, x.ctypes.data, x.shape[0], ch, int(sr), float(threshold_db), float(ratio),
                                       float(attack_ms), float(release_ms), y.ctypes.data,
                                       None if e is None else e.ctypes.data), "op_fx_gate")
        return (y, e) if want_env else y

    def fx_reverb(self, x, sr, room_size, damping, wet, dry, width):
        x, ch = self._fx_in(x)
        y = np.empty_like(x)
        self._ck(lib().rvcx_op_fx_reverb(self._h, x.ctypes.data, x.shape[0], ch, int(sr), float(room_size), float(damping),
                                         float(wet), float(dry), float(width), y.ctypes.data), "op_fx_reverb")
        return y

    def fx_shelf(self, x, sr, gain_db, high=False, fc=440.0, Q=2.0 ** -0.5):
        x, ch = self._fx_in(x)
        y = np.empty_like(x)
        self._ck(lib().rvcx_op_fx_shelf(self._h, x.ctypes.data, x.shape[0], ch, int(sr), int(bool(high)), float(gain_db),
                                        float(fc), float(Q), y.ctypes.data), "op_fx_shelf")
        return y

    def fx_chorus(self, x, sr, rate_hz, depth, centre_delay_ms, feedback, mix):
        x, ch = self._fx_in(x)
        y = np.empty_like(x)
        self._ck(lib().rvcx_op_fx_chorus(self._h, x.ctypes.data, x.shape[0], ch, int(sr), float(rate_hz), float(depth),
                                         float(centre_delay_ms), float(feedback), float(mix), y.ctypes.data), "op_fx_chorus")
        return y

    def fx_mix(self, vocal, inst, vocal_gain_db=0.0, inst_gain_db=0.0):
        """rvcx_op_fx_mix: (n_v, 2) and (n_i, 2) int16 -> (n_v, 2) int16"""
        v, m = _stereo_i16(vocal, "fx_mix"), _stereo_i16(inst, "fx_mix")
        y = np.empty_like(v)
        self._ck(lib().rvcx_op_fx_mix(self._h, v.ctypes.data, v.shape[0], m.ctypes.data, m.shape[0], float(vocal_gain_db),
                                      float(inst_gain_db), y.ctypes.data), "op_fx_mix")
        return y

    def vc_frames(self, n: int) -> int:
        return int(lib().rvcx_vc_frames(self._h, C.c_int64(n)))

    def vc(self, model_id, audio0, pitch, pitchf, sid=0, index_rate=0.0, protect=0.5, z_noise=None, src_noise=None,
           seed=0):
        """VC.vc: one chunk of audio_pad -> the un-trimmed float32 waveform."""
        a = f32(audio0)
        pitch, pitchf = i32(np.asarray(pitch).ravel()), f32(np.asarray(pitchf).ravel())
        T = self.vc_frames(a.shape[0])
        if T <= 0:
            raise RvcxError("vc: chunk too short")
        out = np.empty(T * self.synth_upp(model_id), np.float32)
        zn = None if z_noise is None else f32(z_noise)
        sn = None if src_noise is None else f32(src_noise)
        got = C.c_int64(0)
        self._ck(lib().rvcx_vc(self._h, model_id, _p(a), C.c_int64(a.shape[0]), _p(pitch, C.c_int32), _p(pitchf),
                               int(min(pitch.shape[0], pitchf.shape[0])), int(sid), C.c_float(index_rate),
                               C.c_float(protect), _p(zn), _p(sn), C.c_uint64(seed), _p(out), C.byref(got)), "vc")
        return out[:got.value]

    def weights_regions(self):
        """[(device pointer, used bytes)] of every weight chunk + the shape-only layout hash."""
        h = C.c_uint64(0)
        n = lib().rvcx_weights_regions(self._h, 0, None, None, C.byref(h))
        if n < 0:
            self._ck(-1, "weights_regions")
        ptrs, sizes = (C.c_void_p * max(n, 1))(), (C.c_int64 * max(n, 1))()
        n2 = lib().rvcx_weights_regions(self._h, n, ptrs, sizes, C.byref(h))
        if n2 != n:
            raise RvcxError("weights_regions: chunk count changed between calls")
        return [(int(ptrs[i] or 0), int(sizes[i])) for i in range(n)], int(h.value)

    def weights_clone(self, src: "Context"):
        """copy the folded weights of ``src`` (same GPU, same model configurations) into this context"""
        self._ck(lib().rvcx_weights_clone(self._h, src._h), "weights_clone")

    def weights_adopt(self):
        self._ck(lib().rvcx_weights_adopt(self._h), "weights_adopt")

    def conv_profile_begin(self):
        z = (C.c_int64 * 72)()
        self._ck(lib().rvcx_conv_profile(self._h, 1, z, None, None, None, None, None, 0), "conv_profile")

    def conv_profile_end(self):
        N = 72
        la, fl, ms = (C.c_int64 * N)(), (C.c_double * N)(), (C.c_double * N)()
        bm, bn, kd = (C.c_int32 * N)(), (C.c_int32 * N)(), (C.c_int32 * N)()
        self._ck(lib().rvcx_conv_profile(self._h, 0, la, fl, ms, bm, bn, kd, N), "conv_profile")

        def name(i):
            if kd[i] < 0:
                return f"conv_mfma_kernel<{bm[i]},{bn[i]}> (generic, strided/grouped)"
            if kd[i] == 600001:
                return "gemm_f32<64,64> (time-major Linear, exact fp32)"
            if kd[i] == 600002:
                return f"gemm_bd<{bm[i]},{bn[i]}> (time-major Linear, activations straight from global memory)"
            if kd[i] >= 600000:
                return f"gemm_h3<{bm[i]},{bn[i]}> (time-major Linear)"
            if kd[i] == 500003:
                return "resblock3 (whole k=3 ResBlock: three fused steps, persistent)"
            if kd[i] >= 500000:
                return f"resblock_pair<C={kd[i] - 500000},N1={bn[i]}> (c1 -> c2 -> +x fused)"
            if kd[i] >= 400000:
                c = kd[i] - 400000
                return f"conv_h3<{bm[i]},{bn[i]},{'linear' if c == 1 else 'stride2' if c == 2 else 'halo%d' % c}>"
            if kd[i] == 300001:
                return "conv_cout1 (vector FMA, Cout=1)"
            if kd[i] == 300003:
                return "conv_ws<64,320> (weight-stationary tile: a stage = one 16-channel chunk x all taps; K segments + finish)"
            if kd[i] == 300004:
                return "conv3_thin (3x3, C=16/32: streaming MFMA, B operand from global, DPP-shifted taps)"
            if kd[i] == 300002:
                return "convt_thin (ConvTranspose1d k4 s2, streaming MFMA + fused noise conv)"
            if kd[i] >= 300000:
                return "conv_cin1 (vector FMA, Cin=1)"
            if kd[i] >= 200000:
                return f"conv_fast_sb<{bm[i]},{bn[i]},stride2>"
            if kd[i] >= 100000:
                return f"conv_fast_sb<{bm[i]},{bn[i]},linear>"
            return f"conv_fast_sb<{bm[i]},{bn[i]},halo{kd[i] // 10}>"
        self._tile_names = [name(i) for i in range(N)]
        return [dict(tile=name(i), launches=int(la[i]), flops=float(fl[i]), ms=float(ms[i]))
                for i in range(N) if la[i] > 0]

    def conv_profile_csv(self) -> str:
        """per-launch table of the last profile; the tile column carries the kernel's name (conv_profile_end first)"""
        txt = (lib().rvcx_conv_profile_csv(self._h) or b"").decode()
        names = getattr(self, "_tile_names", None)
        if not names:
            return txt
        out = []
        for i, line in enumerate(txt.splitlines()):
            head, _, rest = line.partition(",")
            if i > 0 and head.isdigit() and int(head) < len(names):
                head = '"' + names[int(head)].split(" (")[0] + '"'
            out.append(head + "," + rest)
        return "\n".join(out) + "\n"

    def last_timing(self):
        ms = (C.c_float * 9)()
        lib().rvcx_last_timing(self._h, ms)
        names = ["highpass", "rmvpe", "hubert", "index", "enc_p", "flow", "decoder", "post", "total"]
        return dict(zip(names, [float(v) for v in ms]))

    def mem_info(self):
        f, t = C.c_int64(0), C.c_int64(0)
        self._ck(lib().rvcx_mem_info(self._h, C.byref(f), C.byref(t)), "mem_info")
        return f.value, t.value

    def fp32_reruns(self) -> int:
        """calls repeated on the exact-fp32 kernels after an fp16-split overflow"""
        return int(lib().rvcx_fp32_reruns(self._h))

    def fp32_pinned(self) -> str:
        """text, one line per layer the range guard pinned to the exact-fp32 kernels at run time (rvcx_fp32_pinned)"""
        buf = C.create_string_buffer(1 << 16)
        if lib().rvcx_fp32_pinned(self._h, buf, len(buf)) < 0:
            raise RvcxError("fp32_pinned")
        return buf.value.decode()

    def fp32_layers(self) -> int:
        """layers pinned to the exact-fp32 kernels after an activation left fp16 range (sticky per model)"""
        return int(lib().rvcx_fp32_layers(self._h))

    def index_exhaustive(self) -> int:
        """queries searched exhaustively (pre-filter not certifiable) since the last call; clears the counter"""
        return int(lib().rvcx_index_exhaustive(self._h))

    def gru_fallbacks(self) -> int:
        return int(lib().rvcx_gru_fallbacks(self._h))

    def gru_publish_probe(self) -> int:
        """1: the cluster BiGRU's plain-store publish was verified on this device, 0: it failed and the write-through
        publish is used, -1: undecided"""
        return int(lib().rvcx_gru_publish_probe(self._h))

    def debug_inject(self, what: int):
        self._ck(lib().rvcx_debug_inject(self._h, int(what)), "debug_inject")

    def flop_counter(self, reset=False) -> float:
        return float(lib().rvcx_flop_counter(self._h, 1 if reset else 0))
