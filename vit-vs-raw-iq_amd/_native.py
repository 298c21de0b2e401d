"""ctypes binding of the C ABI declared in include/iqvit.h (libiqvit.so, gfx950).

There is no fallback: if the library is missing or a call fails the product path raises.
PyTorch is used above this layer only for device memory, streams and torch.distributed.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IQ_LIBIQVIT") or os.path.join(_HERE, "libiqvit.so")      # (override: A/B runs of two builds on one box)

BWD_PARAM_GRADS = 1     # iq_model_backward_input flag (IQ_BWD_PARAM_GRADS)

STATUS = {0: "ok", 1: "invalid argument", 2: "unsupported shape/configuration", 3: "HIP launch error"}


class IqError(RuntimeError):
    pass


class Dropout(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("step", C.c_uint32), ("site", C.c_uint32), ("p", C.c_float),
                ("step_dev", C.c_void_p)]


class Impair(C.Structure):
    _fields_ = [("phase_lo", C.c_float), ("phase_hi", C.c_float), ("cfo_lo", C.c_float), ("cfo_hi", C.c_float),
                ("rot90", C.c_int), ("conj", C.c_int), ("shift_max", C.c_int), ("gain_db_lo", C.c_float),
                ("gain_db_hi", C.c_float), ("snr_db_lo", C.c_float), ("snr_db_hi", C.c_float), ("seed", C.c_uint64),
                ("step", C.c_uint32), ("frame_base", C.c_uint64)]


class SynthClass(C.Structure):
    _fields_ = [("kind", C.c_int), ("offset", C.c_int), ("count", C.c_int)]


class Synth(C.Structure):
    _fields_ = [("points", C.c_void_p), ("classes", C.POINTER(SynthClass)), ("n_classes", C.c_int),
                ("snrs_db", C.POINTER(C.c_float)), ("n_snrs", C.c_int), ("balanced", C.c_int), ("seed", C.c_uint64),
                ("stream", C.c_uint32), ("frame_base", C.c_uint64)]


class Waveform(C.Structure):
    _fields_ = [("points", C.c_void_p), ("classes", C.POINTER(SynthClass)), ("n_classes", C.c_int),
                ("snrs_db", C.POINTER(C.c_float)), ("n_snrs", C.c_int), ("balanced", C.c_int), ("seed", C.c_uint64),
                ("stream", C.c_uint32), ("frame_base", C.c_uint64), ("sps", C.c_int), ("span", C.c_int), ("n_phase", C.c_int),
                ("timing", C.c_int), ("pulse", C.c_void_p), ("fpulse", C.c_void_p), ("n_taps", C.c_int), ("los", C.c_float),
                ("tap_sigma", C.c_float * 8)]


class Fading(C.Structure):
    _fields_ = [("mode", C.c_int), ("len_in", C.c_int), ("n_taps", C.c_int), ("n_sin", C.c_int), ("K", C.c_int),
                ("n_frac", C.c_int), ("normalise", C.c_int), ("timing", C.c_int), ("interp", C.c_void_p), ("snr_db", C.c_void_p),
                ("paths", C.c_void_p), ("amps", C.c_void_p), ("clock", C.c_void_p), ("delay", C.c_int32 * 8),
                ("los", C.c_float * 8), ("tap_sigma", C.c_float * 8), ("fd_lo", C.c_float), ("fd_hi", C.c_float),
                ("d_lo", C.c_int32), ("d_hi", C.c_int32), ("start", C.c_int32), ("stream", C.c_uint32), ("seed", C.c_uint64),
                ("frame_base", C.c_uint64)]


class Receiver(C.Structure):
    _fields_ = [("sps", C.c_int), ("span", C.c_int), ("n_frac", C.c_int), ("mode", C.c_int), ("normalise", C.c_int),
                ("table", C.c_void_p), ("u", C.c_void_p)]


class Spectrogram(C.Structure):
    _fields_ = [("n_fft", C.c_int), ("hop", C.c_int), ("pad", C.c_int), ("width", C.c_int), ("mode", C.c_int),
                ("inv_norm", C.c_float), ("floor", C.c_float), ("scale", C.c_float), ("shift", C.c_float)]


class Constellation(C.Structure):
    _fields_ = [("height", C.c_int), ("width", C.c_int), ("radius", C.c_int), ("n_frac", C.c_int), ("mode", C.c_int),
                ("x_scale", C.c_float), ("x_off", C.c_float), ("y_scale", C.c_float), ("y_off", C.c_float),
                ("inv_norm", C.c_float), ("floor", C.c_float), ("scale", C.c_float), ("shift", C.c_float)]


class Carrier(C.Structure):
    _fields_ = [("order", C.c_int), ("n1", C.c_int), ("n2", C.c_int), ("k_max", C.c_int), ("refine", C.c_int),
                ("planar", C.c_int), ("mode", C.c_int), ("t1", C.c_void_p), ("t2", C.c_void_p), ("tw", C.c_void_p),
                ("fth", C.c_void_p)]


class Equaliser(C.Structure):
    _fields_ = [("taps", C.c_int), ("iters", C.c_int), ("planar", C.c_int), ("mode", C.c_int), ("mu", C.c_float),
                ("modulus", C.c_float), ("w", C.c_void_p), ("w0", C.c_void_p)]


class EqualiserTrack(C.Structure):
    _fields_ = [("taps", C.c_int), ("iters", C.c_int), ("planar", C.c_int), ("mode", C.c_int), ("seg", C.c_int), ("hop", C.c_int),
                ("mu", C.c_float), ("modulus", C.c_float), ("w", C.c_void_p), ("w0", C.c_void_p), ("taper", C.c_void_p)]


class Likelihood(C.Structure):
    _fields_ = [("points", C.c_void_p), ("classes", C.POINTER(SynthClass)), ("n_classes", C.c_int), ("rot", C.c_void_p),
                ("n_rot", C.c_int), ("planar", C.c_int), ("mode", C.c_int), ("gain", C.c_void_p)]


class LikelihoodEm(C.Structure):
    _fields_ = [("points", C.c_void_p), ("classes", C.POINTER(SynthClass)), ("n_classes", C.c_int), ("starts", C.c_void_p),
                ("n_starts", C.c_int), ("iters", C.c_int), ("planar", C.c_int), ("mode", C.c_int), ("f0", C.c_float),
                ("floor", C.c_float), ("h0", C.c_void_p), ("v0", C.c_void_p)]


class Cumulants(C.Structure):
    _fields_ = [("planar", C.c_int), ("sigma2", C.c_void_p), ("mu", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("n_classes", C.c_int)]


class Cyclic(C.Structure):
    _fields_ = [("n_fft", C.c_int), ("hop", C.c_int), ("pad", C.c_int), ("columns", C.c_int), ("kind", C.c_int),
                ("mode", C.c_int), ("inv_norm", C.c_float), ("floor", C.c_float), ("scale", C.c_float), ("shift", C.c_float)]


class Epilogue(C.Structure):
    _fields_ = [("bias", C.c_void_p), ("relu", C.c_int), ("pe", C.c_void_p), ("tok", C.c_int), ("seq", C.c_int),
                ("cls_off", C.c_int), ("drop", Dropout), ("gate", C.c_void_p), ("ldg", C.c_int),
                ("gate_scale", C.c_float), ("residual", C.c_void_p), ("ldr", C.c_int)]


class WgradProblem(C.Structure):
    _fields_ = [("dY", C.c_void_p), ("ldy", C.c_int), ("X", C.c_void_p), ("ldx", C.c_int), ("dW", C.c_void_p),
                ("dbias", C.c_void_p), ("N", C.c_int), ("K", C.c_int)]


class ReduceSeg(C.Structure):
    _fields_ = [("partials", C.c_void_p), ("rows", C.c_int), ("row_stride", C.c_int64), ("out", C.c_void_p),
                ("n", C.c_int64)]


class ReduceJobSeg(C.Structure):
    _fields_ = [("partials", C.c_void_p), ("out", C.c_void_p), ("n", C.c_int64), ("stride", C.c_int64), ("rows", C.c_int),
                ("blk0", C.c_int), ("tall", C.c_int)]


class ReduceJob(C.Structure):      # filled by iq_gemm_bf16_wgrad_grouped_deferred, opaque to callers
    _fields_ = [("seg", ReduceJobSeg * 12), ("nseg", C.c_int), ("nblk", C.c_int), ("accumulate", C.c_int)]


class ModelCfg(C.Structure):
    _fields_ = [("kind", C.c_int), ("in_channels", C.c_int), ("img_h", C.c_int), ("img_w", C.c_int),
                ("patch", C.c_int), ("seq_length", C.c_int), ("conv_k", C.c_int), ("use_cls", C.c_int),
                ("num_classes", C.c_int), ("d_model", C.c_int), ("n_head", C.c_int), ("n_layers", C.c_int),
                ("ffn_hidden", C.c_int), ("drop_prob", C.c_float)]


_P, _I, _Z, _F = C.c_void_p, C.c_int, C.c_size_t, C.c_float
_U64, _U32 = C.c_uint64, C.c_uint32

# name -> (restype, argtypes); must list every symbol include/iqvit.h declares
SIGNATURES = {
    "iq_ln_supported": (_I, [_I]),
    "iq_ln_fwd": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _F, _P]),
    "iq_ln_bwd_ws_bytes": (_Z, [_I]),
    "iq_ln_bwd_partial_rows": (_I, [_I, _I]),
    "iq_ln_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, C.POINTER(Dropout), _P, _P, _P, _I, _I, _I, _P]),
    "iq_gemm_bf16_nt": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, C.POINTER(Epilogue), _P]),
    "iq_gemm_ln_supported": (_I, [_I, _I]),
    "iq_gemm_bf16_ln": (_I, [_P, _I, _P, _I, _P, _P, _I, C.POINTER(Dropout), _P, _P, _F, _P, _P, _P, _P, _I, _I, _I, _P]),
    "iq_gemm_lnbwd_supported": (_I, [_I, _I]),
    "iq_gemm_lnbwd_partial_rows": (_I, [_I]),
    "iq_gemm_bf16_lnbwd": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P, _P, C.POINTER(Dropout), _P, _P, _P, _I, _I, _I, _P]),
    "iq_ffn_chain_supported": (_I, [_I, _I, _I]),
    "iq_ffn_chain_bwd_partial_rows": (_I, [_I]),
    "iq_ffn_chain_bwd": (_I, [_P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _P, C.POINTER(Dropout), _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "iq_qkv_dgrad_ffn_chain_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, C.POINTER(Dropout), _P, _P, _P,
                                        _P, _P, _F, _P, _P, _P, _P, _P, _P, _P, C.POINTER(Dropout), _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "iq_ffn_chain_gate_bytes": (_Z, [_I, _I]),
    "iq_ffn_chain_fwd": (_I, [_P, _P, _P, C.POINTER(Dropout), _P, _P, _P, C.POINTER(Dropout), _P, _P, _F, _P, _P, _P, _P, _P, _I, _I,
                              _I, _I, _P]),
    "iq_attn_out_ffn_chain_fwd": (_I, [_P, _P, _P, C.POINTER(Dropout), _P, _P, _P, _P, _P, _P, _P,
                                       _P, _P, C.POINTER(Dropout), _P, _P, _P, C.POINTER(Dropout), _P, _P, _F, _P, _P, _P, _P, _P,
                                       _P, _P, _P, _I, _I, _I, _I, _P]),
    "iq_wgrad_ws_bytes": (_Z, [_I, _I, _I]),
    "iq_gemm_bf16_wgrad": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _P, _Z, _I, _P]),
    "iq_wgrad_grouped_ws_bytes": (_Z, [_P, _I, _I, _I]),
    "iq_gemm_bf16_wgrad_grouped": (_I, [_P, _I, _I, _P, _Z, _I, _I, _P, _I, _P]),
    "iq_gemm_bf16_wgrad_grouped_deferred": (_I, [_P, _I, _I, _P, _Z, _I, _I, _P, _I, C.POINTER(ReduceJob), _P]),
    "iq_reduce_job_run": (_I, [C.POINTER(ReduceJob), _P]),
    "iq_gemm_bf16_lnbwd_ride": (_I, [_P, _I, _P, _I, _P, _I, _P, _P, _P, _P, C.POINTER(Dropout), _P, _P, _P, _I, _I, _I,
                                     C.POINTER(ReduceJob), _P]),
    "iq_gemm_lnbwd_ride_workgroups": (_I, [_I, _I, _I, _I]),
    "iq_attn_supported": (_I, [_I, _I]),
    "iq_attn_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "iq_attn_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "iq_attn_fwd_masked": (_I, [_P, _P, _P, _P, C.c_long, _I, _I, _I, _I, _P]),
    "iq_attn_bwd_masked": (_I, [_P, _P, _P, _P, _P, _P, C.c_long, _I, _I, _I, _I, _P]),
    "iq_attn_probs": (_I, [_P, _P, _P, C.c_long, _I, _I, _I, _I, _I, _I, _P]),
    "iq_attn_grad_probs": (_I, [_P, _P, _P, _P, C.c_long, _I, _I, _I, _I, _I, _I, _I, _P]),
    "iq_attn_relevance_step": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "iq_frames_preprocess": (_I, [_P, _P, _I, _I, _I, C.POINTER(C.c_float), _P]),
    "iq_frames_impair": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(Impair), _P]),
    "iq_frames_synth": (_I, [_P, _P, _P, _P, _P, _I, _I, C.POINTER(Synth), _P]),
    "iq_frames_waveform": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, C.POINTER(Waveform), _P]),
    "iq_frames_fade": (_I, [_P, _P, _P, _P, _P, _I, _I, C.POINTER(Fading), _P]),
    "iq_frames_receive": (_I, [_P, _P, _P, _P, _I, _I, C.POINTER(Receiver), _P]),
    "iq_frames_receive_bwd": (_I, [_P, _P, _P, _P, _I, _I, C.POINTER(Receiver), _P]),
    "iq_frames_spectrogram": (_I, [_P, _P, _P, _I, _I, C.POINTER(Spectrogram), _P]),
    "iq_frames_spectrogram_bwd": (_I, [_P, _P, _P, _P, _I, _I, C.POINTER(Spectrogram), _P]),
    "iq_frames_cyclic": (_I, [_P, _P, _P, _P, _I, _I, C.POINTER(Cyclic), _P]),
    "iq_frames_cyclic_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, C.POINTER(Cyclic), _P]),
    "iq_frames_constellation": (_I, [_P, _P, _P, _I, _I, C.POINTER(Constellation), _P]),
    "iq_frames_constellation_bwd": (_I, [_P, _P, _P, _P, _I, _I, C.POINTER(Constellation), _P]),
    "iq_frames_carrier": (_I, [_P, _P, _P, _P, _P, _I, _I, C.POINTER(Carrier), _P]),
    "iq_frames_carrier_bwd": (_I, [_P, _P, _I, _I, C.POINTER(Carrier), _P]),
    "iq_frames_equalise": (_I, [_P, _P, _P, _P, _I, _I, C.POINTER(Equaliser), _P]),
    "iq_frames_equalise_bwd": (_I, [_P, _P, _I, _I, C.POINTER(Equaliser), _P]),
    "iq_frames_equalise_track": (_I, [_P, _P, _P, _P, _I, _I, C.POINTER(EqualiserTrack), _P]),
    "iq_frames_equalise_track_bwd": (_I, [_P, _P, _I, _I, C.POINTER(EqualiserTrack), _P]),
    "iq_frames_likelihood": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, C.POINTER(Likelihood), _P]),
    "iq_frames_likelihood_em": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, C.POINTER(LikelihoodEm), _P]),
    "iq_frames_likelihood_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, C.POINTER(Likelihood), _P]),
    "iq_frames_likelihood_em_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, C.POINTER(LikelihoodEm), _P]),
    "iq_frames_cumulants": (_I, [_P, _P, _P, _P, _P, _I, _I, C.POINTER(Cumulants), _P]),
    "iq_frames_cumulants_bwd": (_I, [_P, _P, _P, _P, _I, _I, C.POINTER(Cumulants), _P]),
    "iq_patchify": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "iq_cls_rows": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(Dropout), _P]),
    "iq_embed_bwd_gather": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, C.POINTER(Dropout), _I, _P]),
    "iq_embed_dgrad": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "iq_linf_step": (_I, [_P, _P, _P, _F, _F, _F, _F, _Z, _P]),
    "iq_head_fwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "iq_ce_fwd_bwd": (_I, [_P, _P, _I, _I, _F, _F, _P, _P, _P, _P]),
    "iq_head_bwd": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "iq_gradnorm_ws_bytes": (_Z, [_Z]),
    "iq_gradnorm_sq": (_I, [_P, _Z, _F, _P, _P, _P]),
    "iq_adamw_step": (_I, [_P, _P, _P, _P, _P, _Z, _F, _F, _F, _F, _F, _I, _P, _F, _F, _P, _P]),
    "iq_counter_add": (_I, [_P, _U32, _P, _F, _P]),
    "iq_cast_bf16": (_I, [_P, _P, _Z, _P]),
    "iq_transpose_cast_bf16": (_I, [_P, _P, _I, _I, _P]),
    "iq_model_create": (_I, [C.POINTER(ModelCfg), C.POINTER(_P)]),
    "iq_model_destroy": (None, [_P]),
    "iq_model_last_error": (C.c_char_p, [_P]),
    "iq_model_tokens": (_I, [_P]),
    "iq_model_param_floats": (_Z, [_P]),
    "iq_model_param_entries": (_I, [_P]),
    "iq_model_param_entry": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(_Z), C.POINTER(_I), C.POINTER(_I)]),
    "iq_model_shadow_bytes": (_Z, [_P]),
    "iq_model_workspace_bytes": (_Z, [_P, _I, _I]),
    "iq_model_bind": (_I, [_P, _P, _P, _P, _P]),
    "iq_model_bind_step_counter": (_I, [_P, _P]),
    "iq_model_refresh_shadow": (_I, [_P, _P]),
    "iq_model_refresh_transposed": (_I, [_P, _P]),
    "iq_model_forward": (_I, [_P, _P, _I, _P, _Z, _I, _U64, _U32, _P, _P, _P]),
    "iq_model_backward": (_I, [_P, _P, _P, _I, _P, _Z, _I, _I, _I, _P]),
    "iq_model_grad_range": (_I, [_P, _I, _I, C.POINTER(_Z), C.POINTER(_Z)]),
    "iq_model_backward_input": (_I, [_P, _P, _P, _I, _P, _Z, _P, _I, _P]),
    "iq_model_attention": (_I, [_P, _P, _Z, _I, _I, _I, _I, _P, C.c_long, _P]),
    "iq_model_attention_rollout": (_I, [_P, _P, _Z, _I, _F, _P, _P]),
    "iq_model_attention_relevance": (_I, [_P, _P, _I, _P, _Z, _P, C.POINTER(_P), _I, _I, _I, C.c_long, _P]),
    "iq_prof_enable": (_I, [_I]),
    "iq_prof_collect": (_I, [C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "iq_prof_kernels": (_Z, [C.c_char_p, _Z, _I]),
}

_lib = None


def lib():
    """Load libiqvit.so (once).  Raises if it has not been built -- never falls back."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IqError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C vit-vs-raw-iq_amd/csrc`). "
                "There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)      # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what, model=None):
    if rc != 0:
        detail = ""
        if model is not None:
            msg = lib().iq_model_last_error(model)
            if msg:
                detail = ": " + msg.decode()
        raise IqError(f"{what} failed: {STATUS.get(rc, rc)}{detail}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_handle():
    import torch
    return torch.cuda.current_stream().cuda_stream
