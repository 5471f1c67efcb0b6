"""ctypes binding of libwcb.so (C ABI: include/wcb.h).

The library is the ONLY compute path: if it is missing or fails to load, every product entry point
raises — there is no CPU fallback (the numpy oracle lives under /oracle and is test-only).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwcb.so")
CSRC = os.path.join(_HERE, "csrc")

WCB_BF16, WCB_F16, WCB_F32 = 0, 1, 2
DTYPES = {"bf16": WCB_BF16, "f16": WCB_F16, "fp16": WCB_F16, "f32": WCB_F32, "fp32": WCB_F32}


class WcbModelDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "d_model", "n_layers", "n_heads", "ffn", "vocab", "n_mel", "n_audio_ctx", "n_text_ctx",
        "eos_token_id", "pad_token_id", "decoder_start_token_id", "dtype")]


class WcbGenCfg(C.Structure):
    _fields_ = [("max_new_tokens", C.c_int), ("min_new_tokens", C.c_int), ("num_beams", C.c_int),
                ("bias_boost", C.c_float), ("use_graph", C.c_int), ("async_out", C.c_int)]


class WcbSampleCfg(C.Structure):
    _fields_ = [("temperature", C.c_float), ("seeds", C.POINTER(C.c_uint64))]


class WcbTokenRules(C.Structure):
    _fields_ = [("suppress", C.POINTER(C.c_int32)), ("n_suppress", C.c_int),
                ("begin_suppress", C.POINTER(C.c_int32)), ("n_begin_suppress", C.c_int),
                ("timestamps", C.c_int), ("timestamp_begin", C.c_int), ("no_timestamps_token_id", C.c_int),
                ("max_initial_timestamp_index", C.c_int)]


def token_rules(suppress=(), begin_suppress=(), timestamps=False, timestamp_begin=0, no_timestamps=0,
                max_initial_timestamp_index=-1):
    """A WcbTokenRules and the arrays it points into (keep both alive for the call)."""
    import numpy as np
    sup = np.ascontiguousarray(np.asarray(list(suppress), dtype=np.int32))
    beg = np.ascontiguousarray(np.asarray(list(begin_suppress), dtype=np.int32))
    p32 = C.POINTER(C.c_int32)
    r = WcbTokenRules(sup.ctypes.data_as(p32) if len(sup) else None, len(sup),
                      beg.ctypes.data_as(p32) if len(beg) else None, len(beg), int(bool(timestamps)),
                      int(timestamp_begin), int(no_timestamps), int(max_initial_timestamp_index))
    return r, (sup, beg)


class WcbRepeatRules(C.Structure):
    _fields_ = [("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int)]


class WcbAlignCfg(C.Structure):
    _fields_ = [("heads", C.POINTER(C.c_int32)), ("n_heads", C.c_int), ("median_width", C.c_int),
                ("num_frames", C.POINTER(C.c_int32))]


def align_cfg(heads=None, median_width=7, num_frames=None):
    """A WcbAlignCfg and the arrays it points into (keep both alive for the call)."""
    import numpy as np
    p32 = C.POINTER(C.c_int32)
    hd = np.ascontiguousarray(np.asarray(heads, dtype=np.int32).reshape(-1, 2)) if heads is not None else None
    nf = np.ascontiguousarray(np.asarray(num_frames, dtype=np.int32)) if num_frames is not None else None
    cfg = WcbAlignCfg(hd.ctypes.data_as(p32) if hd is not None and len(hd) else None, len(hd) if hd is not None else 0,
                      int(median_width), nf.ctypes.data_as(p32) if nf is not None else None)
    return cfg, (hd, nf)


class WcbWindows(C.Structure):
    _fields_ = [("mel", C.c_void_p), ("clips", C.c_int), ("T", C.c_int), ("T_ld", C.c_int),
                ("clip_idx", C.POINTER(C.c_int32)), ("seek", C.POINTER(C.c_int32)), ("seek_num_frames", C.POINTER(C.c_int32))]


def windows(mel_ptr, clips, T, T_ld, clip_idx, seek, seek_num_frames):
    """A WcbWindows and the int arrays it points into (keep both alive for the call)."""
    import numpy as np
    p32 = C.POINTER(C.c_int32)
    arrs = tuple(np.ascontiguousarray(np.asarray(a, dtype=np.int32)) for a in (clip_idx, seek, seek_num_frames))
    w = WcbWindows(mel_ptr, int(clips), int(T), int(T_ld), *(a.ctypes.data_as(p32) for a in arrs))
    return w, arrs


class WcbLangCfg(C.Structure):
    _fields_ = [("lang_begin", C.c_int), ("n_lang", C.c_int), ("candidates", C.POINTER(C.c_uint32)),
                ("column_from_end", C.c_int), ("out_ids", C.c_void_p), ("out_probs", C.c_void_p)]


def lang_cfg(lang_begin, n_lang, candidates, column_from_end, out_ids_ptr, out_probs_ptr):
    """A WcbLangCfg and the candidate bitmap it points into (uint32 words or None; keep both alive for the call)."""
    cand = candidates.ctypes.data_as(C.POINTER(C.c_uint32)) if candidates is not None else None
    return WcbLangCfg(int(lang_begin), int(n_lang), cand, int(column_from_end), out_ids_ptr, out_probs_ptr), candidates


PROJ_QKV, PROJ_LN_PLAIN, PROJ_LN_GELU, PROJ_RESID, PROJ_KQ, PROJ_XQK = range(6)
PATH_DEC, PATH_LEAN, PATH_LEAN_FOLD, PATH_LEAN_FOLD_FM, PATH_LN_RING, PATH_RING_FOLD, PATH_WIDE = range(7)
# GemmTaken of csrc/kernels.h (the low byte of wcb_dec_proj.taken; ring tiles: + 256 · tile)
TAKEN_LEAN, TAKEN_XQK, TAKEN_DEC_MF, TAKEN_SKINNY, TAKEN_RING_DEC, TAKEN_WIDE, TAKEN_TILE = range(1, 8)


class WcbDecProj(C.Structure):
    """wcb_dec_proj (include/wcb.h), field for field."""
    _fields_ = [("kind", C.c_int), ("path", C.c_int), ("dtype", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("Wk", C.c_void_p),
                ("x", C.c_void_p), ("a16", C.c_void_p), ("a_fm", C.c_void_p), ("out", C.c_void_p), ("out_fm", C.c_int),
                ("out16", C.c_void_p), ("out16_fm", C.c_void_p), ("st_in", C.c_void_p), ("st_out", C.c_void_p),
                ("rst_in", C.c_void_p), ("rst_out", C.c_void_p), ("kv", C.c_void_p), ("pos", C.c_void_p),
                ("kv_B", C.c_int), ("kv_T", C.c_int), ("kv_rps", C.c_int), ("n_split", C.c_int), ("ring_kt", C.c_int),
                ("xqk_nch", C.c_int), ("u_out", C.c_void_p), ("c_out", C.c_void_p), ("wg_out", C.c_void_p),
                ("taken", C.POINTER(C.c_int32))]


class WcbTensorView(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("dtype", C.c_int), ("ndim", C.c_int),
                ("shape", C.c_int64 * 4), ("stride", C.c_int64 * 4)]


# name -> (restype, argtypes)
_P = C.c_void_p
SIGNATURES = {
    "wcb_create": (C.c_int, [C.POINTER(WcbModelDesc), C.c_int, C.POINTER(_P)]),
    "wcb_destroy": (None, [_P]),
    "wcb_last_error": (C.c_char_p, [_P]),
    "wcb_set_weight": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int]),
    "wcb_load_weights": (C.c_int, [_P, C.POINTER(WcbTensorView), C.c_int, _P]),
    "wcb_finalize_weights": (C.c_int, [_P]),
    "wcb_log_mel": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int64, _P, _P]),
    "wcb_encode": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "wcb_generate": (C.c_int, [_P, _P, C.c_int, C.POINTER(WcbGenCfg), _P, _P, C.c_int, _P,
                               C.POINTER(C.c_int32), _P]),
    "wcb_synchronize": (C.c_int, [_P]),
    "wcb_decode_begin": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_float, C.c_int, C.POINTER(_P), _P]),
    "wcb_decode_step": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "wcb_decode_end": (C.c_int, [_P, _P]),
    "wcb_decode_begin_beams": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_float, C.c_int,
                                         C.POINTER(_P), _P]),
    "wcb_decode_parents": (C.c_int, [_P, _P, _P, _P]),
    "wcb_decode_info": (C.c_int, [_P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "wcb_decode_result": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_int32), _P]),
    "wcb_forward": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P, _P]),
    "wcb_forward_enc": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P]),
    "wcb_forward_cached": (C.c_int, [_P, _P, _P, C.c_int, _P, _P]),
    "wcb_bias_create": (C.c_int, [_P, _P, _P, C.c_int, _P, C.POINTER(_P)]),
    "wcb_bias_destroy": (None, [_P]),
    "wcb_bias_num_states": (C.c_int, [_P]),
    "wcb_bias_batch_create": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.POINTER(_P)]),
    "wcb_bias_batch_destroy": (None, [_P]),
    "wcb_bias_batch_num_states": (C.c_int, [_P, C.c_int]),
    "wcb_generate_biased": (C.c_int, [_P, _P, C.c_int, C.POINTER(WcbGenCfg), _P, _P, C.c_int, _P,
                                      C.POINTER(C.c_int32), _P]),
    "wcb_decode_bias_batch": (C.c_int, [_P, _P, _P]),
    "wcb_generate_scored": (C.c_int, [_P, _P, C.c_int, C.POINTER(WcbGenCfg), _P, _P, _P, C.c_int, _P, _P, _P,
                                      C.POINTER(C.c_int32), _P]),
    "wcb_decode_enable_logprobs": (C.c_int, [_P, _P]),
    "wcb_decode_logprobs": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_int32), _P]),
    "wcb_op_lm_head_lse": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_long, _P, _P, _P]),
    "wcb_generate_sampled": (C.c_int, [_P, _P, C.c_int, C.POINTER(WcbGenCfg), C.POINTER(WcbSampleCfg), _P, _P, _P, C.c_int,
                                       _P, _P, C.POINTER(C.c_int32), _P]),
    "wcb_decode_enable_sampling": (C.c_int, [_P, _P, C.c_float, C.POINTER(C.c_uint64)]),
    "wcb_op_lm_head_sample": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                        C.POINTER(C.c_uint64), C.c_int, _P, C.c_long, _P, _P, _P]),
    "wcb_generate_prompted": (C.c_int, [_P, _P, C.c_int, C.POINTER(WcbGenCfg), C.POINTER(WcbSampleCfg), _P, _P, _P, C.c_int,
                                        _P, _P, _P, C.POINTER(C.c_int32), _P]),
    "wcb_decode_begin_prompted": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, C.c_float, C.c_int, C.POINTER(_P), _P]),
    "wcb_detect_language": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "wcb_generate_lang": (C.c_int, [_P, _P, C.c_int, C.POINTER(WcbGenCfg), C.POINTER(WcbSampleCfg), _P, _P, _P, C.c_int,
                                    _P, C.POINTER(WcbLangCfg), _P, _P, C.POINTER(C.c_int32), _P]),
    "wcb_decode_begin_lang": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, _P, C.POINTER(WcbLangCfg), C.c_float, C.c_int,
                                        C.POINTER(_P), _P]),
    "wcb_op_lang_head": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, C.c_long, _P]),
    "wcb_op_attention_decode_window": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P,
                                                 C.c_int, _P]),
    "wcb_log_mel_long": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int64, _P, C.c_int, _P]),
    "wcb_encode_windows": (C.c_int, [_P, C.POINTER(WcbWindows), C.c_int, _P, _P]),
    "wcb_generate_windows": (C.c_int, [_P, C.POINTER(WcbWindows), C.c_int, C.POINTER(WcbGenCfg), _P, _P, _P, C.c_int, _P,
                                       _P, _P, _P, C.POINTER(C.c_int32), _P]),
    "wcb_decode_enable_no_speech": (C.c_int, [_P, _P]),
    "wcb_decode_no_speech": (C.c_int, [_P, _P, _P, _P]),
    "wcb_op_window_cut": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "wcb_sample_noise": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "wcb_set_token_rules": (C.c_int, [_P, C.POINTER(WcbTokenRules)]),
    "wcb_token_rules_apply_host": (C.c_int, [C.POINTER(WcbTokenRules), C.c_int, C.c_int, _P, C.c_int, _P]),
    "wcb_op_lm_head_rules": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WcbTokenRules),
                                       C.c_int, _P, C.c_int, _P, _P, C.c_long, _P, _P]),
    "wcb_set_repeat_rules": (C.c_int, [_P, C.POINTER(WcbRepeatRules)]),
    "wcb_repeat_rules_apply_host": (C.c_int, [C.POINTER(WcbRepeatRules), C.c_int, _P, C.c_int, _P]),
    "wcb_op_lm_head_repeat": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WcbRepeatRules),
                                        C.c_int, _P, C.c_int, _P, _P, C.c_long, _P, _P]),
    "wcb_align": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, _P, C.c_int, C.POINTER(WcbAlignCfg), _P, _P, _P]),
    "wcb_op_align_capture": (C.c_int, [C.c_int, _P, C.c_long, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P]),
    "wcb_op_align_matrix": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P]),
    "wcb_op_dtw": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P, _P]),
    "wcb_dtw_host": (C.c_int, [_P, C.c_int, C.c_int, C.c_long, _P, C.c_int, _P, _P, _P]),
    "wcb_debug_counter": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "wcb_debug_copy": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, C.c_int]),
    "wcb_profile_enable": (C.c_int, [_P, C.c_int]),
    "wcb_profile_read": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P]),
    "wcb_profile_kernel": (C.c_int, [_P, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64)]),
    "wcb_op_gemm": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P,
                              C.c_int, _P]),
    "wcb_op_gemm_kernel": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P,
                                     C.c_int, C.c_int, _P]),
    "wcb_op_gemm_ln": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P,
                                 C.c_int, _P]),
    "wcb_op_embed": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P,
                               C.c_int, _P]),
    "wcb_op_dec_proj": (C.c_int, [C.POINTER(WcbDecProj), _P]),
    "wcb_op_weighted_ce": (C.c_int, [_P, C.c_long, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int,
                                     C.c_float, _P, _P, _P, _P]),
    "wcb_wer_counts": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int,
                                 C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "wcb_bias_counts": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int,
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "wcb_op_layernorm": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "wcb_op_attention_decode": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          _P]),
    "wcb_op_attention": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, _P]),
    "wcb_op_cross_attention_enc": (C.c_int, [C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_int, _P]),
    "wcb_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
}


class WcbError(RuntimeError):
    pass


class WcbArgError(WcbError, ValueError):
    """WCB_ERR_ARG: the reference raises ValueError for these (e.g. whisper_medical.py:87-90)."""


class WcbStateError(WcbError):
    """WCB_ERR_STATE: a call out of order (e.g. no encoder state held for wcb_align(enc = NULL))."""


_lib = None


def build(force: bool = False, jobs: int = 8) -> str:
    """Compile libwcb.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-C", CSRC, f"-j{jobs}"], check=True)
    return LIB_PATH


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WcbError(f"libwcb.so not found at {LIB_PATH}; build it with "
                       f"`make -C {CSRC}` (no CPU fallback exists)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, handle=None, what: str = ""):
    if rc < 0:
        lib = load()
        msg = lib.wcb_last_error(handle)
        cls = WcbArgError if rc == -1 else WcbStateError if rc == -2 else WcbError
        raise cls(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
    return rc
