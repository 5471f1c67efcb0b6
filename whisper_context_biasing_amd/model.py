"""Drop-in inference surface of the reference model class, backed by libwcb.so.

`WhisperCB` mirrors the parts of `WhisperForConditionalGenerationWeightCE`
(`models/whisper_medical.py:12-172`) that the reference's evaluation path touches
(`scripts/evaluation.py:164-206` → `[tf] trainer_seq2seq.py:329`):

* `generate(input_features, labels=None, bias_spans=None, max_length=...)` → LongTensor [B, ≤max_length]
  without the start token, right-padded with pad_token_id (same return convention as HF);
  `return_dict_in_generate=True` returns `.sequences` that include the start token.
* `forward(input_features, decoder_input_ids, labels=None, bias_spans=None)` → output with
  `.logits` f32 [B, T, V], `.encoder_last_hidden_state`, and the reference's weighted-CE `.loss`
  (`models/whisper_medical.py:113-156`, computed host-side on the returned logits: a training-loss
  path, not the inference hot path).
* `generation_config`, `config.use_cache`, `config.suppress_tokens`, `freeze_encoder()` and `.to()` are
  accepted exactly as the reference mutates them (`scripts/evaluation.py:173-183`).

All arithmetic runs in hand-written HIP kernels through the C ABI; torch only holds device
memory and streams. There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import longform as _longform
from . import prompts as _prompts
from . import request as _request
from .config import (FRAME_SECONDS, HOP, N_SAMPLES, WhisperDims, dims_from_hf_config, get_dims, language_ids, parse_segments,
                     start_of_prev_token_id, timestamp_ids, words_from_token_times)
from .request import DecodeRequest, _mix64, clip_seeds, compression_ratio  # noqa: F401  (importable from here, as ever)

_TORCH_DT = {_lib.WCB_BF16: torch.bfloat16, _lib.WCB_F16: torch.float16, _lib.WCB_F32: torch.float32}


def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


@dataclass
class GenerateOutput:
    sequences: torch.Tensor
    # generate(output_logprobs=True). Greedy: token_logprobs [B, n] f32, the model's own log-prob of every
    # generated token (raw logits: no boost, no EOS mask; 0 where a finished row emits pad), aligned with
    # sequences[:, len(prefix):], and avg_logprob [B], its mean over each row's tokens up to and including its
    # EOS (Whisper's avg_logprob). Beam search: sequences_scores [B] f32 (HF's).
    token_logprobs: Optional[torch.Tensor] = None
    avg_logprob: Optional[torch.Tensor] = None
    sequences_scores: Optional[torch.Tensor] = None
    # generate(temperature=(t0, t1, ...)): the temperature each clip's result was decoded at, [B] f32
    temperatures: Optional[torch.Tensor] = None
    # generate(return_timestamps=True): per clip a list of (start_s, end_s, token_ids) parsed on the host from the
    # generated ids (config.parse_segments); end_s None for a trailing segment without a closing timestamp
    segments: Optional[list] = None
    # generate(return_token_timestamps=True): token_timestamps [B, P + n] f32 seconds, aligned with `sequences` (0 over
    # the prefix, as HF), from the DTW over the cross-attention of a teacher-forced pass (wcb_align); `words`, when
    # the model has a word_start mask: per clip a list of (start_s, end_s, token_ids) (config.words_from_token_times)
    token_timestamps: Optional[torch.Tensor] = None
    words: Optional[list] = None
    # generate(prompt_ids=[[...], ...]) (per-clip prompts): prompt_lengths [B] int64, P_b = len(prompt b) + 1; sequences
    # is then [B, Pmax + n], clip b's prompt left-padded with pad_token_id to Pmax = max P_b (prompts.unpack_prompts)
    prompt_lengths: Optional[torch.Tensor] = None
    # a long-form window decode (transcribe_long): no_speech_prob [B] f32, softmax(raw logits at the start token)[<|nospeech|>]
    no_speech_prob: Optional[torch.Tensor] = None
    # generate(language=...): languages [B] int64, every clip's language token id (given, or with "auto" detected on the
    # device); with per-clip languages or "auto" the forced tail [language, task(, <|notimestamps|>)] follows the start
    # token in `sequences` and prompt_lengths [B] = len(prompt b) + 1 + len(tail) (prompts.split_row). language_probs
    # [B, n_lang] f32 with "auto": the softmax over the (candidate) language tokens
    languages: Optional[torch.Tensor] = None
    language_probs: Optional[torch.Tensor] = None


@dataclass
class LongFormOutput:
    """transcribe_long()'s result. sequences [B, W] int64: every clip's segments' tokens (timestamps included), right-padded
    with pad_token_id, as HF returns them; segments: per clip a list of (start_s, end_s, token_ids) in absolute seconds;
    seeks: per clip the window starts in mel frames; no_speech_probs / avg_logprobs: per clip one float per window;
    window_ids: per clip every window's generated ids (EOS and pads stripped; a skipped window's too)."""
    sequences: torch.Tensor
    segments: list
    seeks: list
    no_speech_probs: list
    avg_logprobs: list
    window_ids: list
    # transcribe_long(language=...): every clip's language token id [B] int64 (with "auto": detected from its first window)
    languages: Optional[torch.Tensor] = None
    language_probs: Optional[torch.Tensor] = None


class _WindowBatch:
    """The clips of one long-form decode as the library takes them (wcb_windows): long features [clips, n_mel, T_ld] f32 on
    the device with T valid frames per row, and per decode row its clip, window start and frame count. Sliced by rows like
    the mel tensor of a short-form call."""

    def __init__(self, feats: torch.Tensor, T: int, clip_idx, seek, frames):
        self.feats, self.T = feats, int(T)
        self.clip_idx, self.seek, self.frames = (np.ascontiguousarray(np.asarray(a, dtype=np.int32)) for a in (clip_idx, seek, frames))

    @property
    def shape(self):
        return (len(self.clip_idx),)

    def __getitem__(self, rows):
        return _WindowBatch(self.feats, self.T, self.clip_idx[rows], self.seek[rows], self.frames[rows])

    def abi(self):
        f = self.feats
        return _lib.windows(f.data_ptr(), f.shape[0], self.T, f.shape[2], self.clip_idx, self.seek, self.frames)


class _PackedPrompts:
    """Per-clip prompts in the library's left-padded layout (prompts.pack_prompts): rows int32 [B, Pmax], lengths [B]."""

    def __init__(self, rows: np.ndarray, lengths: np.ndarray):
        self.rows, self.lengths = np.ascontiguousarray(rows), np.ascontiguousarray(lengths)

    def __len__(self) -> int:   # the prompt width Pmax: what a flat prefix's length is to the length cap
        return int(self.rows.shape[1])


@dataclass
class Seq2SeqLMOutput:
    loss: Optional[torch.Tensor]
    logits: torch.Tensor
    encoder_last_hidden_state: torch.Tensor
    past_key_values: Optional["DecoderCache"] = None

    def to_tuple(self):
        return tuple(v for v in (self.loss, self.logits, self.past_key_values, self.encoder_last_hidden_state)
                     if v is not None)

    def __getitem__(self, i):
        return self.to_tuple()[i]


class BiasList:
    """Device Aho-Corasick automaton of a bias list (list of token-id sequences)."""

    def __init__(self, model: "WhisperCB", phrases: Sequence[Sequence[int]]):
        lib = _lib.load()
        phrases = [list(map(int, p)) for p in phrases if len(p) > 0]
        toks = np.asarray([t for p in phrases for t in p] or [0], dtype=np.int32)
        offs = np.zeros(len(phrases) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(p) for p in phrases]) if phrases else []
        ws = model.word_start
        h = C.c_void_p()
        _lib.check(lib.wcb_bias_create(model._h, toks.ctypes.data, offs.ctypes.data, len(phrases),
                                       ws.ctypes.data if ws is not None else None, C.byref(h)),
                   model._h, "wcb_bias_create")
        self._h = h
        self._lib = lib   # held so the destructor still works during interpreter shutdown
        self.n_phrases = len(phrases)
        self.n_states = lib.wcb_bias_num_states(h)

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self, "_lib", None) is not None:
            self._lib.wcb_bias_destroy(self._h)
            self._h = None


class BiasBatch:
    """Per-utterance bias lists of one batch (wcb_bias_batch): clip b's own list of token-id sequences,
    compiled on the host into one forest of automata. Host data: a decode call copies it, so it can be
    dropped as soon as the call returns (also with block=False). Not cached: it is per call."""

    def __init__(self, model: "WhisperCB", lists: Sequence[Sequence[Sequence[int]]]):
        lib = _lib.load()
        lists = [[list(map(int, p)) for p in L if len(p) > 0] for L in lists]
        phrases = [p for L in lists for p in L]
        toks = np.asarray([t for p in phrases for t in p] or [0], dtype=np.int32)
        poff = np.zeros(len(phrases) + 1, dtype=np.int32)
        poff[1:] = np.cumsum([len(p) for p in phrases]) if phrases else []
        coff = np.zeros(len(lists) + 1, dtype=np.int32)
        coff[1:] = np.cumsum([len(L) for L in lists]) if lists else []
        ws = model.word_start
        h = C.c_void_p()
        _lib.check(lib.wcb_bias_batch_create(model._h, len(lists), toks.ctypes.data, poff.ctypes.data, coff.ctypes.data,
                                             ws.ctypes.data if ws is not None else None, C.byref(h)),
                   model._h, "wcb_bias_batch_create")
        self._h = h
        self._lib = lib
        self.B = len(lists)
        self.n_states = lib.wcb_bias_batch_num_states(h, -1)

    def close(self):
        if getattr(self, "_h", None) and getattr(self, "_lib", None) is not None:
            self._lib.wcb_bias_batch_destroy(self._h)
            self._h = None

    __del__ = close


class StepDecoder:
    """One step-wise decode (WhisperCB.decode_begin). Greedy: step() -> (next ids [B] int32, scores [B] f32:
    the chosen token's logit + bias boost). Beam search (num_beams = nb > 1): step() -> (the token each
    running beam appended [B·nb] int32, the running log-prob sums [B·nb] f32), parents() -> [B·nb] int32,
    the beam (0..nb-1 of the same clip) each running beam extends. result() -> generate()'s output for the
    steps taken (beams: the best finished sequence of every clip so far). All on the model's device;
    close() ends the decode."""

    def __init__(self, model, st, B, bias, num_beams=1):
        self.model, self._st, self.B, self._bias, self.num_beams = model, st, B, bias, num_beams
        self.languages = self.language_probs = None   # decode_begin(language=...)

    def step(self):
        m = self.model
        R = self.B * self.num_beams
        ids = torch.empty(R, dtype=torch.int32, device=m.device)
        sc = torch.empty(R, dtype=torch.float32, device=m.device)
        _lib.check(m._lib.wcb_decode_step(m._h, self._st, self._bias._h if self._bias else None, _ptr(ids), _ptr(sc),
                                          _stream(m.device)), m._h, "wcb_decode_step")
        return ids, sc

    def parents(self):
        m = self.model
        par = torch.empty(self.B * self.num_beams, dtype=torch.int32, device=m.device)
        _lib.check(m._lib.wcb_decode_parents(m._h, self._st, _ptr(par), _stream(m.device)), m._h, "wcb_decode_parents")
        return par

    def info(self):
        """(max_new, steps, done): the state's column capacity, the steps taken, and whether every utterance
        has finished (beams: the search is frozen — further steps give identity parents and pad ids)."""
        m = self.model
        mx, st, dn = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(m._lib.wcb_decode_info(m._h, self._st, C.byref(mx), C.byref(st), C.byref(dn)), m._h,
                   "wcb_decode_info")
        return mx.value, st.value, bool(dn.value)

    @property
    def done(self) -> bool:
        return self.info()[2]

    def result(self, max_new: Optional[int] = None):
        """[B, n] int64 ids as generate() returns them (Whisper-trimmed), n = the generated columns. The
        output width is the library's (wcb_decode_info); `max_new` is accepted for compatibility and, when
        given, must be at least the number of generated columns."""
        m = self.model
        width = self.info()[0]
        out = torch.empty(self.B, width, dtype=torch.int32, device=m.device)
        n = C.c_int32(0)
        _lib.check(m._lib.wcb_decode_result(m._h, self._st, _ptr(out), width, C.byref(n), _stream(m.device)), m._h,
                   "wcb_decode_result")
        if max_new is not None and max_new < n.value:
            raise ValueError(f"result(max_new={max_new}): {n.value} columns were generated")
        return m._whisper_trim(out[:, :n.value].to(torch.int64))

    def logprobs(self):
        """[B, steps] f32: the model's own log-prob of the token each step chose (decode_begin(logprobs=True);
        greedy), 0 where a finished row emitted pad."""
        m = self.model
        width = self.info()[0]
        out = torch.empty(self.B, width, dtype=torch.float32, device=m.device)
        n = C.c_int32(0)
        _lib.check(m._lib.wcb_decode_logprobs(m._h, self._st, _ptr(out), width, C.byref(n), _stream(m.device)), m._h,
                   "wcb_decode_logprobs")
        return out[:, :n.value]

    def no_speech_prob(self):
        """[B] f32: softmax(raw logits of the first step)[<|nospeech|>] (decode_begin(logprobs=True, no_speech=True)),
        once a step was taken."""
        m = self.model
        out = torch.empty(self.B, dtype=torch.float32, device=m.device)
        _lib.check(m._lib.wcb_decode_no_speech(m._h, self._st, _ptr(out), _stream(m.device)), m._h, "wcb_decode_no_speech")
        return out

    def close(self):
        if self._st:
            _lib.check(self.model._lib.wcb_decode_end(self.model._h, self._st), self.model._h, "wcb_decode_end")
            self._st = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecoderCache:
    """`past_key_values` of `WhisperCB.forward(..., use_cache=True)` (models/whisper_medical.py:54-55, 89-110):
    the decoder's self-attention KV cache and the encoder state, held on the device by a prefix-free step-wise
    state (wcb_decode_begin); each forward(past_key_values=cache) appends its decoder_input_ids' positions
    (wcb_forward_cached). One open cache (or StepDecoder) per model: a new use_cache=True forward closes the
    previous cache, and close() frees it."""

    def __init__(self, model: "WhisperCB", enc: torch.Tensor):
        self.model, self.encoder_last_hidden_state, self.B = model, enc, enc.shape[0]
        st = C.c_void_p()
        _lib.check(model._lib.wcb_decode_begin(model._h, _ptr(enc), self.B, 1, None, 1, 0.0, 0, C.byref(st),
                                               _stream(model.device)), model._h, "wcb_decode_begin")
        self._st = st
        self._seen = 0

    def get_seq_length(self) -> int:   # the HF Cache accessor
        return self._seen

    def extend(self, ids: torch.Tensor) -> torch.Tensor:
        m = self.model
        if not self._st:
            raise _lib.WcbError("past_key_values was closed (one open cache per model)")
        if ids.shape[0] != self.B:
            raise ValueError(f"decoder_input_ids has {ids.shape[0]} rows, the cache {self.B}")
        T = ids.shape[1]
        logits = torch.empty(self.B, T, m.dims.vocab, dtype=torch.float32, device=m.device)
        _lib.check(m._lib.wcb_forward_cached(m._h, self._st, _ptr(ids), T, _ptr(logits), _stream(m.device)),
                   m._h, "wcb_forward_cached")
        self._seen += T
        return logits

    def close(self):
        if self._st:
            _lib.check(self.model._lib.wcb_decode_end(self.model._h, self._st), self.model._h, "wcb_decode_end")
            self._st = None
            if self.model._cache is self:
                self.model._cache = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WhisperCB:
    main_input_name = "input_features"

    def __init__(self, dims: WhisperDims, dtype: str = "bf16", device: int = 0, bias_weight: float = 10.0,
                 options: Optional[Dict[str, int]] = None):
        if not torch.cuda.is_available():
            raise _lib.WcbError("WhisperCB needs a ROCm GPU (no CPU fallback by design)")
        lib = _lib.load()
        self.dims = dims
        self.dtype_code = _lib.DTYPES[dtype]
        self.device = torch.device("cuda", device)
        self.bias_weight = bias_weight
        desc = _lib.WcbModelDesc(dims.d_model, dims.n_layers, dims.n_heads, dims.ffn, dims.vocab,
                                 dims.n_mel, dims.n_audio_ctx, dims.n_text_ctx, dims.eos_token_id,
                                 dims.pad_token_id, dims.decoder_start_token_id, self.dtype_code)
        h = C.c_void_p()
        _lib.check(lib.wcb_create(C.byref(desc), device, C.byref(h)), None, "wcb_create")
        self._h = h
        self._lib = lib
        self.config = SimpleNamespace(use_cache=True, suppress_tokens=[], forced_decoder_ids=None,
                                      decoder_start_token_id=dims.decoder_start_token_id,
                                      pad_token_id=dims.pad_token_id, eos_token_id=dims.eos_token_id,
                                      vocab_size=dims.vocab, d_model=dims.d_model,
                                      max_target_positions=dims.n_text_ctx, num_mel_bins=dims.n_mel)
        self.generation_config = SimpleNamespace(max_length=448, pad_token_id=dims.pad_token_id,
                                                 eos_token_id=dims.eos_token_id,
                                                 decoder_start_token_id=dims.decoder_start_token_id,
                                                 use_cache=True, num_beams=1, forced_decoder_ids=None)
        # device automatons of recently used bias lists (LRU: per-batch bias_spans lists would otherwise
        # accumulate one V-sized automaton per distinct batch)
        self._bias_cache: "OrderedDict[tuple, BiasList]" = OrderedDict()
        self.bias_cache_size = 8
        # automatons evicted from the LRU: destroying one waits for this handle's queued work
        # (wcb_bias_destroy drops the decode graphs that captured it), so they are kept until the next
        # synchronize() — where the streams are idle and the wait is free — instead of stalling an
        # asynchronous (block=False) generate call. Past kRetiredMax they are released anyway (one stall).
        self._bias_retired: List[BiasList] = []
        self._word_start: Optional[np.ndarray] = None
        self._rules_key = None   # the token rules installed on the handle (wcb_set_token_rules), None: none
        self._repeat_key = None  # the repeat rules (p, n) installed on the handle (wcb_set_repeat_rules), None: none
        self._loaded = False
        self._cache: Optional["DecoderCache"] = None   # the open forward(use_cache=True) state, if any
        # options last: a rejected option raises with every attribute __del__ reads already set
        for k, v in (options or {}).items():   # wcb_set_option: alternative formulations (tests)
            _lib.check(lib.wcb_set_option(h, k.encode(), int(v)), h, f"wcb_set_option({k})")

    # ------------------------------------------------------------------ construction / weights
    @classmethod
    def from_state_dict(cls, dims_or_config, state_dict, dtype: str = "bf16", device: int = 0,
                        bias_weight: float = 10.0, options: Optional[Dict[str, int]] = None) -> "WhisperCB":
        dims = dims_or_config if isinstance(dims_or_config, WhisperDims) else (
            get_dims(dims_or_config) if isinstance(dims_or_config, str) else dims_from_hf_config(dims_or_config))
        m = cls(dims, dtype=dtype, device=device, bias_weight=bias_weight, options=options)
        m.load_state_dict(state_dict)
        return m

    @classmethod
    def from_seed(cls, size: str, seed: int = 0, recipe: str = "diverse", dtype: str = "bf16",
                  device: int = 0) -> "WhisperCB":
        from .weights import make_weights
        dims = get_dims(size)
        return cls.from_state_dict(dims, make_weights(dims, seed=seed, recipe=recipe), dtype, device)

    _VIEW_DTYPES = {torch.float32: _lib.WCB_F32, torch.bfloat16: _lib.WCB_BF16, torch.float16: _lib.WCB_F16}

    def load_state_dict(self, state_dict):
        """Device tensors (this GPU; f32 / bf16 / f16, any strides) are handed over as borrowed views
        (wcb_load_weights: gathered on the device, no host round trip); host arrays go through
        wcb_set_weight. Then wcb_finalize_weights builds the device layouts."""
        views, keep = [], []
        for name, t in state_dict.items():
            if (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device.index
                    and t.dtype in self._VIEW_DTYPES and 1 <= t.dim() <= 4):
                nm = name.encode()
                keep.append(nm)
                v = _lib.WcbTensorView(nm, t.data_ptr(), self._VIEW_DTYPES[t.dtype], t.dim(),
                                       (C.c_int64 * 4)(*t.shape), (C.c_int64 * 4)(*t.stride()))
                views.append((v, t))
                continue
            if isinstance(t, torch.Tensor):
                a = t.detach().to("cpu", torch.float32).contiguous().numpy()
            else:
                a = np.ascontiguousarray(t, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            _lib.check(self._lib.wcb_set_weight(self._h, name.encode(), a.ctypes.data, shape, a.ndim),
                       self._h, f"wcb_set_weight({name})")
        if views:
            arr = (_lib.WcbTensorView * len(views))(*[v for v, _ in views])
            _lib.check(self._lib.wcb_load_weights(self._h, arr, len(views), _stream(self.device)), self._h,
                       "wcb_load_weights")
        _lib.check(self._lib.wcb_finalize_weights(self._h), self._h, "wcb_finalize_weights")
        self._loaded = True
        return self

    def __del__(self):
        if getattr(self, "_h", None):
            getattr(self, "_bias_cache", {}).clear()
            self._lib.wcb_destroy(self._h)
            self._h = None

    def set_option(self, name: str, value: int) -> None:
        """wcb_set_option on this handle (alternative formulations; include/wcb.h lists them)."""
        _lib.check(self._lib.wcb_set_option(self._h, name.encode(), int(value)), self._h, f"wcb_set_option({name})")

    # reference-compatible no-ops (scripts/evaluation.py:181-183)
    def freeze_encoder(self):
        return self

    def to(self, device=None, *a, **k):
        return self

    def eval(self):
        return self

    # --------------------------------------------------------------------------- front end
    @property
    def torch_dtype(self):
        return _TORCH_DT[self.dtype_code]

    def log_mel(self, pcm) -> torch.Tensor:
        """WhisperFeatureExtractor equivalent: f32 PCM [B, N] (or [N]) → f32 mel [B, n_mel, 3000]."""
        x = torch.as_tensor(pcm, dtype=torch.float32)
        if x.dim() == 1:
            x = x[None]
        x = x.to(self.device).contiguous()
        B, N = x.shape
        out = torch.empty(B, self.dims.n_mel, 3000, dtype=torch.float32, device=self.device)
        _lib.check(self._lib.wcb_log_mel(self._h, _ptr(x), B, min(N, N_SAMPLES), N, _ptr(out),
                                         _stream(self.device)), self._h, "wcb_log_mel")
        return out

    def _features(self, input_features) -> torch.Tensor:
        x = torch.as_tensor(input_features)
        if x.dim() == 2:
            x = x[None]
        if x.shape[-1] != 3000:
            # same check as [tf] modeling_whisper.py:612-616
            raise ValueError(f"Whisper expects the mel input features to be of length 3000, but found {x.shape[-1]}")
        if x.shape[-2] != self.dims.n_mel:
            raise ValueError(f"expected {self.dims.n_mel} mel bins, got {x.shape[-2]}")
        return x.to(self.device, torch.float32).contiguous()

    def encode(self, input_features) -> torch.Tensor:
        x = self._features(input_features)
        B = x.shape[0]
        enc = torch.empty(B, self.dims.n_audio_ctx, self.dims.d_model, dtype=self.torch_dtype, device=self.device)
        _lib.check(self._lib.wcb_encode(self._h, _ptr(x), B, _ptr(enc), _stream(self.device)), self._h, "wcb_encode")
        return enc

    def log_mel_long(self, pcm, num_samples=None):
        """WhisperFeatureExtractor(truncation=False, padding="longest", return_attention_mask=True) equivalent: f32 PCM
        [B, N] (or [N], or a list of clips of different lengths) -> (mel f32 [B, n_mel, N // 160] on the device, max_frames
        [B] int64 = the attention mask's sum). `num_samples` [B]: the valid samples of every row (default: the clips' own
        lengths, N for an array); the samples past them read as zero. The max - 8 clamp is taken over the whole clip."""
        if isinstance(pcm, (list, tuple)) and len(pcm) and np.ndim(pcm[0]) == 1:
            if num_samples is None:
                num_samples = [len(c) for c in pcm]
            x = torch.zeros(len(pcm), max(len(c) for c in pcm), dtype=torch.float32)
            for b, c in enumerate(pcm):
                x[b, :len(c)] = torch.as_tensor(c, dtype=torch.float32)
        else:
            x = torch.as_tensor(pcm, dtype=torch.float32)
            if x.dim() == 1:
                x = x[None]
        x = x.to(self.device).contiguous()
        B, N = x.shape
        nv = np.full(B, N, dtype=np.int32) if num_samples is None else np.ascontiguousarray(np.asarray(num_samples, dtype=np.int32).reshape(-1))
        if nv.shape[0] != B:
            raise ValueError(f"num_samples has {nv.shape[0]} entries, the batch {B} clips")
        T = N // HOP
        out = torch.empty(B, self.dims.n_mel, T, dtype=torch.float32, device=self.device)
        _lib.check(self._lib.wcb_log_mel_long(self._h, _ptr(x), B, nv.ctypes.data, N, N, _ptr(out), T, _stream(self.device)),
                   self._h, "wcb_log_mel_long")
        return out, np.minimum((nv.astype(np.int64) + HOP - 1) // HOP, T)   # every 160th sample's flag, as HF rescales the mask

    def encode_windows(self, features, clip_idx, seek, seek_num_frames, num_frames: Optional[int] = None) -> torch.Tensor:
        """The encoder on windows cut from long features [clips, n_mel, T_ld] f32 (`num_frames` = T valid frames per
        row, default T_ld): row r = frames [seek[r], seek[r] + seek_num_frames[r]) of clip clip_idx[r], zero-padded to
        3000 (wcb_encode_windows: the cut writes the conv input directly) -> [rows, 1500, d]."""
        f = self._long_features(features)
        wb = _WindowBatch(f, f.shape[2] if num_frames is None else num_frames, clip_idx, seek, seek_num_frames)
        rows = wb.shape[0]
        enc = torch.empty(rows, self.dims.n_audio_ctx, self.dims.d_model, dtype=self.torch_dtype, device=self.device)
        w, keep = wb.abi()
        _lib.check(self._lib.wcb_encode_windows(self._h, C.byref(w), rows, _ptr(enc), _stream(self.device)), self._h,
                   "wcb_encode_windows")
        del keep
        return enc

    def _long_features(self, features) -> torch.Tensor:
        x = torch.as_tensor(features)
        if x.dim() == 2:
            x = x[None]
        if x.dim() != 3 or x.shape[1] != self.dims.n_mel or x.shape[2] < 1:
            raise ValueError(f"expected features [B, {self.dims.n_mel}, T], got {tuple(x.shape)}")
        return x.to(self.device, torch.float32).contiguous()

    # ------------------------------------------------------------------------------ biasing
    @property
    def word_start(self) -> Optional[np.ndarray]:
        """[vocab] uint8 mask of the tokens a bias match may start at (None = every token)."""
        return self._word_start

    def set_word_start(self, mask) -> None:
        """Word-start gate of the bias boost: for a BPE vocabulary, True on the tokens that begin a word
        (a leading space), e.g. `[t.startswith("\u0120") for t in tokenizer.convert_ids_to_tokens(range(V))]`.
        None disables the gate. Cached automata are rebuilt."""
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask, dtype=bool).astype(np.uint8))
            if mask.shape != (self.dims.vocab,):
                raise ValueError(f"word_start must have shape ({self.dims.vocab},), got {mask.shape}")
        self._word_start = mask
        self._bias_cache.clear()

    def bias_list(self, phrases: Sequence[Sequence[int]]) -> BiasList:
        key = tuple(tuple(int(t) for t in p) for p in phrases)
        b = self._bias_cache.get(key)
        if b is None:
            b = BiasList(self, phrases)
            self._bias_cache[key] = b
            while len(self._bias_cache) > self.bias_cache_size:
                self._bias_retired.append(self._bias_cache.popitem(last=False)[1])
            if len(self._bias_retired) > self.kRetiredMax:
                self.synchronize()
        else:
            self._bias_cache.move_to_end(key)
        return b

    # ---------------------------------------------------------------------------- generation
    def _install_rules(self, key) -> None:
        """Make `key` the handle's token rules (handle state, like a generation config; a no-op when it already is);
        a key that carries repeat rules (request.split_rules) installs or removes those the same way."""
        key, repeat = _request.split_rules(key)
        if repeat != self._repeat_key:
            r = None if repeat is None else C.byref(_lib.WcbRepeatRules(*repeat))
            _lib.check(self._lib.wcb_set_repeat_rules(self._h, r), self._h, "wcb_set_repeat_rules")
            self._repeat_key = repeat
        if key == self._rules_key:
            return
        if key is None:
            _lib.check(self._lib.wcb_set_token_rules(self._h, None), self._h, "wcb_set_token_rules")
        else:
            sup, beg, ts, mi = key
            ts0, nots = timestamp_ids(self.dims)
            r, keep = _lib.token_rules(sup, beg, ts, ts0, nots, mi)
            _lib.check(self._lib.wcb_set_token_rules(self._h, C.byref(r)), self._h, "wcb_set_token_rules")
            del keep
        self._rules_key = key

    def _segments(self, ids) -> list:
        ts0 = timestamp_ids(self.dims)[0]
        return [parse_segments(row, ts0, self.dims.eos_token_id) for row in np.asarray(ids)]

    def generate(self, input_features=None, labels=None, bias_spans=None, max_length: Optional[int] = None,
                 num_beams: Optional[int] = None, bias_list=None, bias_boost: float = 0.0,
                 min_new_tokens: int = 0, prompt_ids=None, return_dict_in_generate: bool = False,
                 generation_config=None, use_graph: bool = True, block: bool = True, bias_lists=None,
                 per_utterance_bias: bool = False, output_logprobs: bool = False, temperature=0.0, seed=0,
                 do_sample: Optional[bool] = None, logprob_threshold: Optional[float] = -1.0,
                 compression_ratio_threshold: Optional[float] = 2.4, return_timestamps: bool = False,
                 suppress_tokens=None, begin_suppress_tokens=None, max_initial_timestamp: Optional[float] = None,
                 return_token_timestamps: bool = False, alignment_heads=None, num_frames=None,
                 median_filter_width: int = 7, language=None, task: Optional[str] = None, language_candidates=None,
                 repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None, **kwargs):
        """Greedy (num_beams = 1, the reference's eval setting) or HF beam
        search (num_beams = 2..8, [tf] generation/utils.py:3208) on the device.

        Returns Whisper's post-processed ids ([tf] generation_whisper.py:1063-1086, 213-225): per row
        the trailing pads and the final EOS dropped, right-padded with pad to the longest row.

        `labels` / `bias_spans` are accepted and ignored for token selection exactly like the
        reference (`[tf] trainer_seq2seq.py:310-329`), unless `bias_boost > 0` and no explicit
        `bias_list` is given — then the batch's spans form the boosted bias list: their union over the
        batch by default, or with `per_utterance_bias=True` row b's spans for clip b alone (a clip's
        transcript then does not depend on its batch; a clip without spans is not boosted).

        `bias_lists=[phrases of clip 0, ...]` (length B) boosts every clip with its own list
        (wcb_generate_biased); a shared `bias_list` given with it is appended to every clip's list.

        `block=False` (serving pipelines): the caller's stream is not made to wait for the decode, so
        the next call's front end + encoder overlap this decode; the returned ids (and the inputs)
        must be kept alive and are valid only after `synchronize()`. Only meaningful with
        `min_new_tokens >= max_length` (no early-exit polling). Beam search returns all `max_length`
        columns then (pad past each clip's best sequence: its length is not read back).

        `output_logprobs=True` (implies `return_dict_in_generate`) also returns, computed on the device in
        the same decode (wcb_generate_scored): greedy, `token_logprobs` [B, n] — the model's own log-prob of
        every generated token from the raw logits (the boost and the EOS mask pick the token but never enter
        it), 0 where a finished row emits pad — and `avg_logprob` [B]; beam search, `sequences_scores` [B].
        With `block=False` the result is a GenerateOutput of device views valid after `synchronize()`:
        `sequences` the int32 generated columns, `token_logprobs` / `sequences_scores`; `avg_logprob` is a
        host computation and stays None.

        `temperature > 0` (or `do_sample=True`, temperature then defaulting to 1.0) samples every token from
        softmax(score / temperature) on the device (wcb_generate_sampled; greedy only: `num_beams` must be 1),
        score = logit + bias boost; token log-probs keep their meaning (raw logits). `seed` = an int, expanded
        per clip by `clip_seeds(seed, 0, B)`, or a sequence of B 64-bit per-clip seeds; the same seeds give the
        same tokens whatever the batch split. `temperature=0` (the default) is the call as it always was.

        `temperature=(0.0, 0.2, ...)` (a sequence) runs Whisper's temperature fallback (HF
        `generate_with_fallback`, greedy and sampling only): attempt i decodes the still-failing clips at
        temperature[i] with log-probs; a clip fails when its avg_logprob < `logprob_threshold` or its
        `compression_ratio` > `compression_ratio_threshold` (None disables either); a clip that passes keeps
        that result, one that fails at the last temperature keeps the last. An int seed gives attempt i
        `clip_seeds(seed, 0, B, attempt=i)`, explicit per-clip seeds s_b give s_b + i·0x9E3779B97F4A7C15 (mod
        2^64). Returns a GenerateOutput with `temperatures` [B]. Failing clips are re-encoded from their mel.

        Token rules, applied on the device at every greedy step (wcb_set_token_rules; all off by default, and
        `config.suppress_tokens` is not read): `suppress_tokens=[...]` are never generated,
        `begin_suppress_tokens=[...]` not as the first token. `return_timestamps=True` decodes with Whisper's
        timestamp grammar (HF WhisperTimeStampLogitsProcessor: drive it from a prompt without <|notimestamps|>)
        and returns a GenerateOutput whose `segments` holds per clip a list of (start_s, end_s, token_ids);
        `max_initial_timestamp=1.0` (seconds) bounds the first timestamp. Greedy only: with `num_beams > 1`, and
        for timestamps also with `temperature > 0` or a temperature sequence, the call raises ValueError.

        `return_token_timestamps=True` (HF's; implies `return_dict_in_generate`, needs `block=True`) adds
        `token_timestamps` [B, P + n] f32 seconds — when each token was spoken — from a teacher-forced post-pass over
        the ids the decode produced (wcb_align: cross-attention of `alignment_heads`, a list of (layer, head), default
        every head of the upper half of the layers; normalised, median-filtered over `median_filter_width` frames, DTW
        on the device). It works with every decode mode above and changes none of them. `num_frames` = mel frames of
        every clip ([B] ints, default 3000) crops the alignment to each clip's audio. With a `word_start` mask set the
        result also holds `words`.

        `prompt_ids` = one flat prompt for every clip, or a sequence of B prompts, one per clip, of any lengths (an
        empty one: no prompt; wcb_generate_prompted, greedy family only). Clip b then decodes exactly as it decodes
        alone with `prompt_ids=prompt_ids[b]`. With `return_dict_in_generate` (or anything implying it) `sequences` is
        [B, Pmax + n]: clip b's prompt and the start token left-padded with `pad_token_id` to Pmax = the longest
        prompt + 1, so every clip's start token is column Pmax - 1 and the generated tokens follow in the same columns
        (HF's layout for batched decoder prompts); `prompt_lengths` [B] = len(prompt b) + 1
        (`prompts.unpack_prompts(sequences, prompt_lengths)` gives the prompts back). `token_logprobs`, `segments` and
        `temperatures` stay aligned with the generated columns. The length cap is the widest prompt's: at most
        `n_text_ctx - Pmax` new tokens. It works with bias lists, log-probs, sampling and the temperature fallback (a
        failing clip is re-decoded with its own prompt), token rules, `use_graph` both ways, `block=False` and above 64
        clips. Raises ValueError with `num_beams > 1` (beam scores count the prompt), with
        `return_token_timestamps=True` (the alignment pass takes one shared prefix), and when the number of prompts
        is not the number of clips.

        `language` / `task` (multilingual models; HF's arguments): the decoder prompt goes on after the
        start token with the forced tail [language, task] — `task` "transcribe" (the default) or "translate" — and
        <|notimestamps|> unless `return_timestamps=True`; clip b's prompt is prompt_b + [start] + tail_b. `language` = a
        code ("fr"), an English name ("french") or a token string ("<|fr|>"), case-insensitively; a sequence of B of
        them; or "auto": every clip's language is detected on the device between the encoder and the prefill (one decoder
        pass over [start], the language head, no logits leave the chip), from `language_candidates` when given. One
        language for the whole batch is a flat prefix (it works with `num_beams > 1` and `return_token_timestamps`);
        differing languages or "auto" go through the per-clip prompt path (greedy family only), and every clip decodes as
        it decodes alone with its language. A GenerateOutput then holds `languages` [B] (token ids) and with "auto"
        `language_probs` [B, n_lang]; "auto" implies `return_dict_in_generate`. With all three left at None the call is
        exactly the call without them. ValueError: any of them on an English-only model, `task` without `language`,
        `language_candidates` without "auto", an unknown language (or one this vocabulary has no token for), a list
        whose length is not B, differing languages or "auto" with `num_beams > 1` or `return_token_timestamps`.

        `repetition_penalty` / `no_repeat_ngram_size` (HF's; None = the generation config's value when it has one, else
        1.0 / 0 = off): applied on the device at every greedy step to the raw logits, before the boost and
        every other rule (wcb_set_repeat_rules). The history they look at is the clip's own prompt, the start token, the
        forced language / task tail (a detected language included) and the tokens generated so far — not the padding of
        a ragged batch, so a clip decodes as it decodes alone. Token log-probs stay raw. They work with bias lists,
        `prompt_ids`, `language=`, `output_logprobs`, the deny lists, `min_new_tokens`, `block=False`, `use_graph` both
        ways and above 64 clips; two calls that differ only in the two values replay the same graphs. ValueError with
        `num_beams > 1`, `temperature > 0` or a temperature sequence, and `return_timestamps=True` (hence
        `transcribe_long`). With both off the call is exactly the call without them.
        """
        if not self._loaded:
            raise _lib.WcbError("weights not loaded")
        x = torch.as_tensor(input_features)
        req = _request.resolve(   # every ValueError of the arguments, before any device work
            self.dims, generation_config or self.generation_config, int(x.shape[0]) if x.dim() > 2 else 1,
            bias_spans=None if bias_spans is None else (lambda: torch.as_tensor(bias_spans).cpu().numpy()),
            max_length=max_length, num_beams=num_beams, bias_list=bias_list, bias_boost=bias_boost, bias_lists=bias_lists,
            per_utterance_bias=per_utterance_bias, min_new_tokens=min_new_tokens, prompt_ids=prompt_ids, use_graph=use_graph,
            block=block, return_dict_in_generate=return_dict_in_generate, output_logprobs=output_logprobs, seed=seed,
            temperature=temperature, do_sample=do_sample, logprob_threshold=logprob_threshold,
            compression_ratio_threshold=compression_ratio_threshold, return_timestamps=return_timestamps,
            suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens,
            max_initial_timestamp=max_initial_timestamp, return_token_timestamps=return_token_timestamps,
            alignment_heads=alignment_heads, num_frames=num_frames, median_filter_width=median_filter_width,
            language=language, task=task, language_candidates=language_candidates,
            repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)
        x = self._features(x)
        res = self._generate_with_fallback(x, req) if req.temperatures is not None else self._decode(x, req)
        if req.align is not None:   # right after the decode: one library call leaves its encoder state to the alignment
            res = self._attach_token_timestamps(res, x, req.prompt_width, req.align)
        return res

    def _decode(self, x, req: DecodeRequest):
        """generate()'s result for the clips x of `req`: one library call, or — the library takes at most 64 clips
        (512 decoder rows) per call — one per chunk in order, each blocking, on its own slice of the request, joined."""
        per_call = self.max_clips_per_call(req.num_beams)
        if req.B <= per_call:
            return self._decode_call(x, req)
        parts = []
        for i in range(0, req.B, per_call):
            sub = replace(req.take(range(i, min(i + per_call, req.B))), block=True)
            parts.append((slice(i, i + sub.B), slice(None), self._decode_call(x[i:i + per_call], sub), sub.prompt_width))
        return self._join(req, parts)

    def _prefix(self, req: DecodeRequest):
        """The decoder prompt of one library call: flat prompt + start token, or per-clip prompts packed at these clips' width."""
        start = self.dims.decoder_start_token_id
        if req.language is not None:   # the forced tail after the start token; a language still to detect holds <|en|>
            if req.packed:
                return _PackedPrompts(*_prompts.pack_rows(req.clip_rows(language_ids(self.dims)[0]), start, self.dims.pad_token_id))
            return list(req.prompt or []) + [start, int(req.language.ids[0])] + list(req.language.rest)
        if req.per_clip_prompts:
            return _PackedPrompts(*_prompts.pack_prompts(req.prompt, start, self.dims.pad_token_id))
        return list(req.prompt or []) + [start]

    def _automaton(self, shared, bias_boost: float) -> Optional[BiasList]:
        """A shared bias source's automaton: a prebuilt BiasList (this model's) as it is, phrases through the LRU, or None."""
        if shared is None or not bias_boost > 0:
            return None
        if _request.is_prebuilt(shared):
            return shared
        return self.bias_list(shared) if shared else None

    def _decode_call(self, x, req: DecodeRequest):
        """One library decode of the clips x (at most max_clips_per_call) as `req` asks, and generate()'s result for it.
        With a boost: the shared automaton `bl`, the per-clip lists (a BiasBatch that lives for this call) or neither;
        seeds sample; `scored` asks for token log-probs (greedy) or sequence scores (beams)."""
        prefix = self._prefix(req)
        cfg = _lib.WcbGenCfg(req.max_new(self.dims.n_text_ctx), req.min_new_tokens, req.num_beams, req.bias_boost,
                             int(req.use_graph), int(not req.block))
        smp = _lib.WcbSampleCfg(req.temperature, req.seeds.ctypes.data_as(C.POINTER(C.c_uint64))) if req.seeds is not None else None
        bl = self._automaton(req.bias_shared, req.bias_boost)
        bias_lists, scored = req.bias_lists if req.bias_boost > 0 else None, req.scored
        self._install_rules(req.rules)
        B, max_new, beams = x.shape[0], cfg.max_new_tokens, cfg.num_beams > 1
        out = torch.empty(B, max_new, dtype=torch.int32, device=self.device)
        lp = torch.zeros(B, max_new, dtype=torch.float32, device=self.device) if scored and not beams else None
        ss = torch.zeros(B, dtype=torch.float32, device=self.device) if scored and beams else None
        steps = C.c_int32(0)
        packed = isinstance(prefix, _PackedPrompts)
        pre = None if packed else np.asarray(prefix, dtype=np.int32)
        bb = BiasBatch(self, bias_lists) if bias_lists is not None else None   # per call: not in the automaton LRU
        windows = isinstance(x, _WindowBatch)   # long-form: rows cut from long features, the no-speech probability beside the log-probs
        win, keep_win = x.abi() if windows else (None, None)
        nsp = torch.zeros(B, dtype=torch.float32, device=self.device) if windows and lp is not None else None
        plan = req.language
        lang_ids = lang_probs = lcfg = keep_lang = None
        if plan is not None and plan.auto:   # the language slot: detected on the device, patched into the prompt rows
            lang_begin, n_lang = language_ids(self.dims)
            lang_ids = torch.empty(B, dtype=torch.int32, device=self.device)
            lang_probs = torch.empty(B, n_lang, dtype=torch.float32, device=self.device)
            lcfg, keep_lang = _lib.lang_cfg(lang_begin, n_lang, _request.candidate_bitmap(self.dims, plan.candidates),
                                            len(plan.rest), _ptr(lang_ids), _ptr(lang_probs))
        head = (self._h, C.byref(win) if windows else _ptr(x), B, C.byref(cfg))
        bias = (bl._h if (bl and not bb) else None, bb._h if bb else None)
        mid = None if packed else (pre.ctypes.data if len(prefix) > 1 else None, len(prefix), _ptr(out))
        scores = (_ptr(lp) if lp is not None else None, _ptr(ss) if ss is not None else None)
        tail = (C.byref(steps), _stream(self.device))
        if windows:   # (transcribe_long: always per-clip prompts, never sampled; its languages are always given)
            name = "wcb_generate_windows"
            args = head + bias + (prefix.rows.ctypes.data, prefix.rows.shape[1], prefix.lengths.ctypes.data, _ptr(out)) + scores[:1] + (
                _ptr(nsp) if nsp is not None else None,) + tail
        elif packed:   # per-clip prompts: the greedy family in one entry point (with a language slot: its _lang form)
            name = "wcb_generate_prompted" if lcfg is None else "wcb_generate_lang"
            args = head + (C.byref(smp) if smp is not None else None,) + bias + (
                prefix.rows.ctypes.data, prefix.rows.shape[1], prefix.lengths.ctypes.data) + (
                () if lcfg is None else (C.byref(lcfg),)) + (_ptr(out),) + scores[:1] + tail
        elif smp is not None:
            name, args = "wcb_generate_sampled", head + (C.byref(smp),) + bias + mid + scores[:1] + tail
        elif scored:
            name, args = "wcb_generate_scored", head + bias + mid + scores + tail
        elif bb:
            name, args = "wcb_generate_biased", head + bias[1:] + mid + tail
        else:
            name, args = "wcb_generate", head + bias[:1] + mid + tail
        try:
            _lib.check(getattr(self._lib, name)(*args), self._h, name)
        finally:
            if bb:
                bb.close()   # the call copied it, as it copied the seeds (also with block=False)
        del keep_win, keep_lang
        if lang_ids is not None and req.block:   # the detected ids into the host copy of the prompt rows (`sequences`)
            prefix.rows[:, prefix.rows.shape[1] - 1 - len(plan.rest)] = lang_ids.cpu().numpy()
        res = self._generate_result(out, steps.value, prefix, req.block, req.as_dict, lp, ss, req.timestamps)
        if nsp is not None:
            res.no_speech_prob = nsp
        if plan is not None and (isinstance(res, GenerateOutput) or plan.auto):
            if not isinstance(res, GenerateOutput):   # block=False: device views, valid after synchronize()
                res = GenerateOutput(sequences=res)
            if plan.auto:   # (block=False: the int32 ids the decode stream writes, like the other device views)
                res.languages = lang_ids.to(torch.int64) if req.block else lang_ids
            else:
                res.languages = torch.from_numpy(plan.ids).to(self.device)
            res.language_probs = lang_probs
        return res

    def _prompt_columns(self, prefix, B: int):
        """(the prompt columns of `sequences`, int64 [B, P]; prompt_lengths [B], None for a shared prefix)."""
        if isinstance(prefix, _PackedPrompts):
            return (torch.from_numpy(prefix.rows.astype(np.int64)).to(self.device),
                    torch.from_numpy(prefix.lengths.astype(np.int64)).to(self.device))
        return torch.tensor(prefix, dtype=torch.int64, device=self.device)[None].expand(B, -1), None

    def _generate_result(self, out, n, prefix, block, as_dict, lp=None, ss=None, timestamps=False):
        """generate()'s return value from a decode's ids [B, max_new] (n columns generated) and its scores, if any."""
        if not block:   # device views (int32 ids), valid after synchronize()
            if lp is None and ss is None:
                return out[:, :n]
            return GenerateOutput(sequences=out[:, :n], token_logprobs=lp[:, :n] if lp is not None else None,
                                  sequences_scores=ss)
        ids = out[:, :n].to(torch.int64)
        if not as_dict:
            return self._whisper_trim(ids)
        B = ids.shape[0]
        sot, plen = self._prompt_columns(prefix, B)
        res = GenerateOutput(sequences=torch.cat([sot, ids], dim=1), sequences_scores=ss, prompt_lengths=plen,
                             segments=self._segments(ids.cpu().numpy()) if timestamps else None)
        if lp is not None:
            res.token_logprobs = lp[:, :n]
            # Whisper's avg_logprob on the host: each row's tokens up to and including its EOS (a finished row's
            # pads, which may equal EOS, come after it), every token of a row that never finished
            ids_h, lp_h = ids.cpu().numpy(), res.token_logprobs.cpu().numpy()
            avg = np.zeros(B, dtype=np.float32)
            for b in range(B):
                hit = np.flatnonzero(ids_h[b] == self.dims.eos_token_id)
                cnt = int(hit[0]) + 1 if len(hit) else n
                avg[b] = lp_h[b, :cnt].astype(np.float64).mean() if cnt else 0.0
            res.avg_logprob = torch.from_numpy(avg).to(self.device)
        return res

    def _join(self, req: DecodeRequest, parts):
        """One result for the clips of `req` from decodes of some of them (the chunks of a split, the attempts of a
        fallback). parts: (dst, src, result, P) — rows `src` of `result`, a decode at prompt width P, are clips `dst`
        of the batch (each a slice or an index tensor). Ids are padded with pad and log-probs with 0 to the widest
        part that gives a row; the prompt columns are packed again at this batch's width."""
        results, pad = [r for _, _, r, _ in parts], self.dims.pad_token_id

        def scatter(vals, fill=0.0, dtype=torch.float32):   # [k] or [k, w] of every part -> [B] or [B, widest w]
            if any(v is None for v in vals):
                return None
            flat = vals[0].dim() == 1
            vals = [v[src].reshape(-1, 1) if flat else v[src] for (_, src, _, _), v in zip(parts, vals)]
            out = torch.full((req.B, max((v.shape[1] for v in vals if len(v)), default=0)), fill, dtype=dtype, device=self.device)
            for (dst, _, _, _), v in zip(parts, vals):
                if len(v):
                    out[dst, :v.shape[1]] = v
            return out[:, 0] if flat else out

        if not req.as_dict:   # every part trimmed on its own: Whisper's padding of the joined output
            return scatter(results, pad, torch.int64)
        sot, plen = self._prompt_columns(self._prefix(req), req.B)
        ids = scatter([r.sequences[:, P:] for _, _, r, P in parts], pad, torch.int64)
        languages = scatter([r.languages for r in results], 0, torch.int64) if req.language is not None else None
        if languages is not None and req.language.auto:   # the detected ids into the prompt columns packed again
            sot = sot.clone()
            sot[:, sot.shape[1] - 1 - len(req.language.rest)] = languages
        return GenerateOutput(
            languages=languages, language_probs=scatter([r.language_probs for r in results]) if languages is not None else None,
            sequences=torch.cat([sot, ids], dim=1), prompt_lengths=plen, token_logprobs=scatter([r.token_logprobs for r in results]),
            avg_logprob=scatter([r.avg_logprob for r in results]), sequences_scores=scatter([r.sequences_scores for r in results]),
            no_speech_prob=scatter([r.no_speech_prob for r in results]),
            # token rules never meet the fallback (resolve() refuses it): the parts are whole chunks, in order
            segments=[s for r in results for s in r.segments] if req.timestamps else None)

    def _generate_with_fallback(self, x, req: DecodeRequest) -> GenerateOutput:
        """generate(temperature=(t0, t1, ...)): HF's generate_with_fallback rule. Attempt i decodes the still-failing
        clips (their mel re-encoded: the rare path pays the encoder again) through _decode, so a failing subset above
        64 clips splits as any batch does; a clip keeps the first attempt it passes, or the last one."""
        kept, used, todo, probs = [], np.zeros(req.B, dtype=np.float32), np.arange(req.B), None
        lpt, crt = req.logprob_threshold, req.compression_ratio_threshold
        for i, T in enumerate(req.temperatures):
            whole = len(todo) == req.B   # then the caller's tensor itself: no gather
            sub = req.attempt(i) if whole else req.attempt(i).take(todo)
            res = self._decode(x if whole else x[torch.as_tensor(todo, device=x.device)], sub)
            ids_h, avg_h = res.sequences[:, sub.prompt_width:].cpu().numpy(), res.avg_logprob.cpu().numpy()
            fail = np.asarray([i + 1 < len(req.temperatures) and (   # the last attempt's result stands
                (lpt is not None and avg_h[j] < lpt) or
                (crt is not None and compression_ratio(ids_h[j], self.dims.vocab, self.dims.eos_token_id) > crt))
                for j in range(sub.B)], dtype=bool)
            used[todo[~fail]] = T
            kept.append((torch.as_tensor(todo[~fail], device=self.device),
                         torch.as_tensor(np.flatnonzero(~fail), device=self.device), res, sub.prompt_width))
            todo = todo[fail]
            if not len(todo):
                break
            if req.language is not None and req.language.auto:   # detected on the first attempt: given from now on
                probs = res.language_probs
                req = req.with_languages(res.languages.cpu().numpy())
        out = replace(self._join(req, kept), temperatures=torch.from_numpy(used).to(self.device))
        if probs is not None:
            out.language_probs = probs
        return out

    def detect_language(self, input_features=None, encoder_outputs=None, language_candidates=None, return_probs: bool = False):
        """HF `detect_language` on the device: every clip's language token id, [B] int64, from `input_features`
        [B, n_mel, 3000] (encoded here) or `encoder_outputs` [B, 1500, d] — exactly one of them. One decoder pass over
        [start], the language head over the language tokens only and the argmax, all on the chip (wcb_detect_language);
        `language_candidates` (codes, names or token strings) restricts the choice. `return_probs=True` also returns
        [B, n_lang] f32: the softmax over the (candidate) language tokens only, 0 for a language that is no candidate."""
        if not self._loaded:
            raise _lib.WcbError("weights not loaded")
        if input_features is None and encoder_outputs is None:
            raise ValueError("You have to specify either `input_features` or `encoder_outputs`")
        if input_features is not None and encoder_outputs is not None:
            raise ValueError("Make sure to specify only one of `input_features` or `encoder_outputs` - not both!")
        plan = _request.resolve_language(self.dims, 1, "auto", None, language_candidates)
        x = self._features(input_features) if input_features is not None else self._encoder_state(encoder_outputs)
        ids, probs = [], []
        for i in range(0, x.shape[0], 64):   # 64 clips per library call
            enc = self.encode(x[i:i + 64]) if input_features is not None else x[i:i + 64]
            a, b = self._detect(enc, plan.candidates)
            ids.append(a)
            probs.append(b)
        ids = torch.cat(ids).to(torch.int64)
        return (ids, torch.cat(probs)) if return_probs else ids

    def _detect(self, enc: torch.Tensor, candidates):
        """wcb_detect_language on at most 64 encoder outputs -> (ids int32 [B], probs f32 [B, n_lang]), on the device."""
        lang_begin, n_lang = language_ids(self.dims)
        B = enc.shape[0]
        ids = torch.empty(B, dtype=torch.int32, device=self.device)
        probs = torch.empty(B, n_lang, dtype=torch.float32, device=self.device)
        bits = _request.candidate_bitmap(self.dims, candidates)
        _lib.check(self._lib.wcb_detect_language(self._h, _ptr(enc), B, lang_begin, n_lang, bits.ctypes.data if bits is not None else None,
                                                 _ptr(ids), _ptr(probs), _stream(self.device)), self._h, "wcb_detect_language")
        return ids, probs

    def transcribe_long(self, input_features=None, attention_mask=None, *, pcm=None, num_samples=None, max_new_tokens: int = 224,
                        condition_on_prev_tokens: bool = False, prompt_ids=None, prompt_condition_type: str = "first-segment",
                        bias_lists=None, bias_list=None, bias_boost: float = 0.0, suppress_tokens=None,
                        begin_suppress_tokens=None, max_initial_timestamp: Optional[float] = None,
                        logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = None,
                        use_graph: bool = True, temperature=0.0, num_beams: int = 1,
                        return_token_timestamps: bool = False, language=None, task: Optional[str] = None,
                        language_candidates=None) -> LongFormOutput:
        """Long-form transcription: audio of any length, HF `WhisperGenerationMixin.generate`'s long-form branch on this
        library's greedy path. Input: `input_features` [B, n_mel, T] (the extractor's long mode, T > 3000
        allowed) with `attention_mask` [B, T] (its sum = the clip's frames; None: T), or `pcm` ([B, N], or a list of clips)
        with `num_samples`, from which the whole-recording log-mel is computed on the device (log_mel_long).

        Every clip keeps a `seek` in mel frames. While a clip's seek is short of its frames it is active: its next window
        (at most 3000 frames from seek, zero-padded) is cut on the device straight into the encoder's input, and the
        active clips are decoded in one greedy batch with the timestamp grammar (`return_timestamps=True`), the caller's
        `suppress_tokens` / `begin_suppress_tokens` / `max_initial_timestamp`, token log-probs and every clip's own bias
        list at `bias_boost`; at most `max_new_tokens` tokens per window (capped by n_text_ctx minus the widest prompt).
        The ids decide the segments and how far seek advances (longform.retrieve_segments). The batch shrinks as clips
        finish and never reorders; a clip's result does not depend on the clips it is batched with.

        `condition_on_prev_tokens=True`: a window's decoder prompt is <|startofprev|> + the last n_text_ctx // 2 - 1 tokens
        of the clip's earlier segments (per-clip prompts of different lengths in one batch). `prompt_ids` (one flat prompt)
        follows HF's `prompt_condition_type`: "first-segment" or "all-segments" (the latter needs conditioning).
        `no_speech_threshold` (None: off): a window whose avg_logprob < `logprob_threshold` and whose no-speech probability
        exceeds it is skipped: no segments, seek moves past it.

        `language` / `task` / `language_candidates` as generate() takes them: every window's prompt continues after the
        start token with [language, task] (long-form always decodes with timestamps, so without <|notimestamps|>). With
        "auto" every clip's language is detected from its first window (HF), on the device, and every later window of the
        clip reuses it; `languages` (and `language_probs`) of the result hold it. Not together with `no_speech_threshold`
        (HF reads the no-speech probability at the start token, which then lies inside the prefill): ValueError.

        Refused with ValueError before any device work: a temperature sequence or `temperature > 0` (the timestamp
        grammar needs the unperturbed text maximum: no sampling, no temperature fallback inside the loop); `num_beams > 1`;
        `return_token_timestamps` together with `condition_on_prev_tokens` (the alignment pass takes one shared prefix;
        without conditioning it is not implemented either and raises NotImplementedError)."""
        if not self._loaded:
            raise _lib.WcbError("weights not loaded")
        _longform.check_args(temperature=temperature, num_beams=num_beams, return_token_timestamps=return_token_timestamps,
                             condition_on_prev_tokens=condition_on_prev_tokens, prompt_ids=prompt_ids,
                             prompt_condition_type=prompt_condition_type)
        if return_token_timestamps:
            raise NotImplementedError("transcribe_long(return_token_timestamps=True) is not implemented")
        if (input_features is None) == (pcm is None):
            raise ValueError("transcribe_long takes input_features or pcm")
        if language is not None or task is not None or language_candidates is not None:   # before any device work
            if no_speech_threshold is not None:
                raise ValueError("language with no_speech_threshold is not supported (the no-speech probability is read at the "
                                 "start token, which a language prompt puts inside the prefill)")
            src = pcm if pcm is not None else input_features
            n_clips = len(src) if isinstance(src, (list, tuple)) else 1 if np.ndim(src) == (1 if pcm is not None else 2) else int(np.shape(src)[0])
            _request.resolve_language(self.dims, n_clips, language, task, language_candidates, timestamps=True)
        if pcm is not None:
            feats, max_frames = self.log_mel_long(pcm, num_samples)
        else:
            feats = self._long_features(input_features)
            if attention_mask is not None and tuple(torch.as_tensor(attention_mask).shape) != (feats.shape[0], feats.shape[2]):
                raise ValueError(f"attention_mask must be [{feats.shape[0]}, {feats.shape[2]}] like the features")
            max_frames = (np.full(feats.shape[0], feats.shape[2], dtype=np.int64) if attention_mask is None
                          else torch.as_tensor(attention_mask).sum(-1).cpu().numpy().astype(np.int64))
        B, T = feats.shape[0], feats.shape[2]
        req = _request.resolve(   # every ValueError of the decode arguments, once
            self.dims, self.generation_config, B, max_length=max_new_tokens, num_beams=1, bias_list=bias_list, bias_boost=bias_boost,
            bias_lists=bias_lists, prompt_ids=[[] for _ in range(B)], use_graph=use_graph, output_logprobs=True,
            return_timestamps=True, suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens,
            max_initial_timestamp=max_initial_timestamp, language=language, task=task, language_candidates=language_candidates)
        lang_probs = None
        if req.language is not None and req.language.auto:   # every clip's language from its first window, then given
            first = [b for b in range(B) if max_frames[b] > 0]
            found = np.full(B, language_ids(self.dims)[0], dtype=np.int64)
            lang_probs = torch.zeros(B, language_ids(self.dims)[1], dtype=torch.float32, device=self.device)
            if first:
                frames = [_longform.seek_num_frames(0, int(max_frames[b])) for b in first]
                enc = self.encode_windows(feats, first, np.zeros(len(first), dtype=np.int64), frames, T)
                ids, probs = self._detect(enc, req.language.candidates)
                found[first] = ids.cpu().numpy()
                lang_probs[torch.as_tensor(first, device=self.device)] = probs
            req = req.with_languages(found)
        st = _longform.LongFormState(
            max_frames, eos=self.dims.eos_token_id, pad=self.dims.pad_token_id, timestamp_begin=timestamp_ids(self.dims)[0],
            prev_sot=start_of_prev_token_id(self.dims), n_text_ctx=self.dims.n_text_ctx,
            condition_on_prev_tokens=condition_on_prev_tokens, prompt_ids=prompt_ids, prompt_condition_type=prompt_condition_type,
            logprob_threshold=logprob_threshold, no_speech_threshold=no_speech_threshold)
        while True:
            active = st.active()
            if not active:
                break
            seek, frames = st.windows(active)
            sub = replace(req.take(active), prompt=st.prompts(active))
            res = self._decode(_WindowBatch(feats, T, active, seek, frames), sub)
            st.update(active, res.sequences[:, sub.prompt_width:].cpu().numpy(), res.avg_logprob.cpu().numpy(),
                      res.no_speech_prob.cpu().numpy())
        return LongFormOutput(sequences=torch.from_numpy(st.sequences()).to(self.device), segments=st.segments, seeks=st.seeks,
                              no_speech_probs=st.no_speech_probs, avg_logprobs=st.avg_logprobs, window_ids=st.window_ids,
                              languages=None if req.language is None else torch.from_numpy(req.language.ids).to(self.device),
                              language_probs=lang_probs)

    def decode_begin(self, encoder_outputs, prompt_ids=None, bias_list=None, bias_boost: float = 0.0,
                     min_new_tokens: int = 0, num_beams: int = 1, max_length: Optional[int] = None,
                     bias_lists=None, logprobs: bool = False, temperature: float = 0.0, seed=0,
                     return_timestamps: bool = False, suppress_tokens=None, begin_suppress_tokens=None,
                     max_initial_timestamp: Optional[float] = None, no_speech: bool = False, language=None,
                     task: Optional[str] = None, language_candidates=None, repetition_penalty: Optional[float] = None,
                     no_repeat_ngram_size: Optional[int] = None) -> "StepDecoder":
        """Step-wise decoding from an encoder output [B, 1500, d] (this model's dtype, on its device): the
        streaming form of generate() (wcb_decode_begin / wcb_decode_begin_beams). Greedy (num_beams = 1) or
        beam search (num_beams 2..8; `max_length` = generate()'s, the beams' length cap: None = the
        max_target_positions cap). `prompt_ids` = one prompt for every clip, a [B, P] array of per-clip
        prompts, or a list of B prompts of different lengths (empty: none; wcb_decode_begin_prompted, greedy only:
        ValueError with num_beams > 1 or when its length is not B) — decoder_start_token_id is appended as
        generate() does, every clip decodes as it does alone with its prompt, and step() / result() / logprobs()
        return the generated tokens as for any decode. `bias_lists` = per-clip phrase lists as
        generate() takes them (wcb_decode_bias_batch; a shared `bias_list` of phrases is appended to each).
        `logprobs=True` (greedy): StepDecoder.logprobs() gives the token log-probs of the steps taken.
        `temperature > 0` (greedy): every step samples as generate(temperature=..., seed=...) does
        (wcb_decode_enable_sampling; `seed` an int through clip_seeds, or B per-clip seeds); step()'s scores are
        then the winners' perturbed values. `return_timestamps` / `suppress_tokens` / `begin_suppress_tokens` /
        `max_initial_timestamp`: generate()'s token rules for every step of this decode (greedy only; timestamps
        not with sampling: ValueError). `no_speech=True` (needs `logprobs=True`: ValueError): StepDecoder.no_speech_prob()
        gives every clip's no-speech probability after the first step. `language` / `task` / `language_candidates`:
        generate()'s (the forced tail after the start token; "auto" detects on the device before the prefill —
        wcb_decode_begin_lang); the StepDecoder then has `languages` [B] int64 and, with "auto", `language_probs`.
        `repetition_penalty` / `no_repeat_ngram_size`: generate()'s repeat rules for every step of this decode (greedy
        only, not with sampling or timestamps: ValueError)."""
        T, nb = _request.sampling_temperature(temperature), int(num_beams)
        repeat = _request.repeat_key(repetition_penalty, no_repeat_ngram_size, self.generation_config)
        if repeat is not None and (nb != 1 or T > 0.0 or return_timestamps):
            raise ValueError("repetition_penalty / no_repeat_ngram_size are greedy only: not with num_beams > 1, sampling "
                             "or return_timestamps")
        if no_speech and not logprobs:
            raise ValueError("no_speech needs logprobs=True (it reuses the log-probs' logsumexp)")
        rules = _request.rules_key(self.dims, return_timestamps, suppress_tokens, begin_suppress_tokens, max_initial_timestamp)
        if rules is not None and nb != 1:
            raise ValueError("suppress_tokens / begin_suppress_tokens / return_timestamps are greedy only: num_beams must be 1")
        if return_timestamps and T > 0.0:
            raise ValueError("return_timestamps with sampling is not supported")
        if T > 0.0 and nb != 1:
            raise ValueError("sampling (temperature > 0) is greedy only: num_beams must be 1")
        enc = self._encoder_state(encoder_outputs)   # [B, 1500, d] checked: the library copies B·1500·d
        B = enc.shape[0]
        if B > 64:
            raise ValueError("decode_begin takes at most 64 clips")
        seeds = _request.seed_array(seed, B) if T > 0.0 else None
        start = self.dims.decoder_start_token_id
        packed = None
        plan = _request.resolve_language(self.dims, B, language, task, language_candidates, timestamps=bool(return_timestamps),
                                         num_beams=nb)
        if plan is not None:   # every clip's full decoder prompt: prompt_b + [start] + tail_b
            if prompt_ids is None:
                plists = [[] for _ in range(B)]
            elif _prompts.is_nested(prompt_ids):
                plists = _prompts.as_lists(prompt_ids)
            else:
                plists = [[int(t) for t in prompt_ids]] * B
            if len(plists) != B:
                raise ValueError(f"prompt_ids holds {len(plists)} prompts, the batch {B} clips")
            tails = [[language_ids(self.dims)[0] if plan.ids is None else int(plan.ids[b])] + list(plan.rest) for b in range(B)]
            if plan.per_clip or len({len(p) for p in plists}) > 1:
                if nb != 1:
                    raise ValueError("per-clip prompts of different lengths are greedy only: num_beams must be 1")
                packed = _PackedPrompts(*_prompts.pack_rows(list(zip(plists, tails)), start, self.dims.pad_token_id))
                prompt_ids = None
            else:   # one language, prompts of one length: the dense [B, P] rows, whose last token is the first step's input
                pre_rows = np.asarray([p + [start] + t for p, t in zip(plists, tails)], dtype=np.int32)
        elif _prompts.is_nested(prompt_ids) and not isinstance(prompt_ids, np.ndarray):
            plists = _prompts.as_lists(prompt_ids)
            if len(plists) != B:
                raise ValueError(f"prompt_ids holds {len(plists)} prompts, the batch {B} clips")
            if len({len(p) for p in plists}) > 1:   # ragged: the left-padded form (equal lengths: the [B, P] path)
                if nb != 1:
                    raise ValueError("per-clip prompts of different lengths are greedy only: num_beams must be 1")
                packed = _PackedPrompts(*_prompts.pack_prompts(plists, start, self.dims.pad_token_id))
            prompt_ids = plists
        if plan is not None and packed is None:
            pre = np.ascontiguousarray(pre_rows)
        elif prompt_ids is None or packed is not None:
            pre = None
        else:
            p = np.asarray(prompt_ids, dtype=np.int32)
            if p.ndim == 1:
                p = np.broadcast_to(p, (B, p.shape[-1]))
            elif p.ndim != 2 or p.shape[0] != B:
                raise ValueError(f"prompt_ids must be one prompt or a [{B}, P] array, got shape {p.shape}")
            pre = np.ascontiguousarray(np.concatenate([p, np.full((B, 1), start, np.int32)], axis=1))
        shared, bias_lists = _request.bias_source(B, bias_list, bias_lists, bias_boost)
        bl = self._automaton(shared, bias_boost)
        st = C.c_void_p()
        self._install_rules(rules if repeat is None else (rules or _request.NO_TOKEN_RULES) + (repeat,))
        flat = (pre.ctypes.data, pre.shape[1]) if pre is not None else (None, 1)
        lang_ids = lang_probs = keep_lang = None
        if packed is not None and plan is not None and plan.auto:
            lang_begin, n_lang = language_ids(self.dims)
            lang_ids = torch.empty(B, dtype=torch.int32, device=self.device)
            lang_probs = torch.empty(B, n_lang, dtype=torch.float32, device=self.device)
            lcfg, keep_lang = _lib.lang_cfg(lang_begin, n_lang, _request.candidate_bitmap(self.dims, plan.candidates),
                                            len(plan.rest), _ptr(lang_ids), _ptr(lang_probs))
            name, args = "wcb_decode_begin_lang", (1, packed.rows.ctypes.data, packed.rows.shape[1], packed.lengths.ctypes.data,
                                                   C.byref(lcfg))
        elif packed is not None:
            name, args = "wcb_decode_begin_prompted", (packed.rows.ctypes.data, packed.rows.shape[1], packed.lengths.ctypes.data)
        elif nb > 1 and max_length is not None:
            name, args = "wcb_decode_begin_beams", (nb,) + flat + (int(max_length),)
        else:
            name, args = "wcb_decode_begin", (nb,) + flat
        _lib.check(getattr(self._lib, name)(self._h, _ptr(enc), B, *args, float(bias_boost), int(min_new_tokens), C.byref(st),
                                            _stream(self.device)), self._h, name)
        del keep_lang
        dec = StepDecoder(self, st, B, bl, nb)
        if plan is not None:
            dec.languages = lang_ids.to(torch.int64) if plan.auto else torch.from_numpy(plan.ids).to(self.device)
            dec.language_probs = lang_probs
        if logprobs:   # greedy only (wcb.h): every step records the log-prob of its token
            _lib.check(self._lib.wcb_decode_enable_logprobs(self._h, st), self._h, "wcb_decode_enable_logprobs")
        if no_speech:
            _lib.check(self._lib.wcb_decode_enable_no_speech(self._h, st), self._h, "wcb_decode_enable_no_speech")
        if seeds is not None:
            _lib.check(self._lib.wcb_decode_enable_sampling(self._h, st, T, seeds.ctypes.data_as(C.POINTER(C.c_uint64))),
                       self._h, "wcb_decode_enable_sampling")
        if bias_lists is not None and bias_boost > 0:
            bb = BiasBatch(self, bias_lists)
            try:
                _lib.check(self._lib.wcb_decode_bias_batch(self._h, st, bb._h), self._h, "wcb_decode_bias_batch")
            finally:
                bb.close()
        return dec

    @staticmethod
    def max_clips_per_call(num_beams: int = 1) -> int:
        """Clips one wcb_generate call takes (64, and at most 512 decoder rows = clips x beams)."""
        return max(1, min(64, 512 // max(1, int(num_beams))))

    def _whisper_trim(self, ids: torch.Tensor) -> torch.Tensor:
        """Whisper's short-form post-processing ([tf] generation_whisper.py:1063-1086, then
        _pad_to_max_length :213-225): per row drop the pads (all but one when pad == eos) and the
        final EOS, then right-pad every row with pad to the longest one."""
        eos, pad = self.dims.eos_token_id, self.dims.pad_token_id
        rows = ids.cpu().numpy()
        lens = []
        for r in rows:
            n = len(r)
            if n and r[-1] == pad:
                n -= int((r == pad).sum()) - (1 if pad == eos else 0)
            if n and r[n - 1] == eos:
                n -= 1
            lens.append(n)
        W = max(lens, default=0)
        out = ids[:, :W].clone()
        for i, n in enumerate(lens):
            if n < W:
                out[i, n:] = pad
        return out

    # ------------------------------------------------------------------------- token timestamps
    def _align_args(self, B: int, alignment_heads, num_frames, median_filter_width) -> dict:
        """The checked alignment arguments (ValueError for what wcb_align refuses)."""
        return _request.align_args(self.dims, B, alignment_heads, num_frames, median_filter_width)

    def _align_call(self, enc, ids: torch.Tensor, prefix, akw, nf, matrix: bool = False):
        """wcb_align on one batch of at most 64 clips: ids int32 [B, n] (device) -> frames int32 [B, n] (and the cost
        matrices [B, n - 1, n_audio_ctx] f32 when `matrix`)."""
        B, n = ids.shape
        frames = torch.empty(B, n, dtype=torch.int32, device=self.device)
        mat = torch.zeros(B, max(n - 1, 1), self.dims.n_audio_ctx, dtype=torch.float32, device=self.device) if matrix else None
        cfg, keep = _lib.align_cfg(akw["heads"], akw["width"], nf)
        pre = np.asarray(prefix, dtype=np.int32)
        _lib.check(self._lib.wcb_align(self._h, _ptr(enc) if enc is not None else None, B, _ptr(ids), ids.stride(0), n,
                                       pre.ctypes.data if len(prefix) > 1 else None, len(prefix), C.byref(cfg),
                                       _ptr(frames), _ptr(mat) if mat is not None else None, _stream(self.device)),
                   self._h, "wcb_align")
        del keep
        return (frames, mat) if matrix else frames

    def _attach_token_timestamps(self, res: GenerateOutput, x: torch.Tensor, P: int, akw) -> GenerateOutput:
        """token_timestamps (and words) of a finished generate(): through the encoder state the decode left in its
        context when the library still holds it for exactly this batch (one library call decoded it: the library's own
        check, WCB_ERR_STATE otherwise), else re-encoded in batches of at most 64 clips."""
        seq = res.sequences
        B = seq.shape[0]
        prefix = [int(t) for t in seq[0, :P].tolist()]
        ids = seq[:, P:].to(torch.int32).contiguous()
        nf = akw["num_frames"]
        frames = None
        if ids.shape[1] == 0:
            frames = torch.zeros(B, 0, dtype=torch.int32, device=self.device)
        elif B <= 64:
            try:
                frames = self._align_call(None, ids, prefix, akw, nf)
            except _lib.WcbStateError:
                frames = None
        if frames is None:
            parts = []
            for i in range(0, B, 64):
                enc = self.encode(x[i:i + 64])
                parts.append(self._align_call(enc, ids[i:i + 64].contiguous(), prefix, akw, nf[i:i + 64] if nf is not None else None))
            frames = torch.cat(parts)
        ts = torch.zeros(B, seq.shape[1], dtype=torch.float32, device=self.device)
        ts[:, P:] = frames.to(torch.float32) * FRAME_SECONDS
        res.token_timestamps = ts
        if self._word_start is not None:
            ids_h, t_h = ids.cpu().numpy(), ts[:, P:].cpu().numpy()
            res.words = [words_from_token_times(ids_h[b], t_h[b], self._word_start, self.dims.eos_token_id,
                                                (float(nf[b]) if nf is not None else 2.0 * self.dims.n_audio_ctx) * 0.01)
                         for b in range(B)]
        return res

    def align(self, encoder_outputs, sequences, prefix_len: int = 1, alignment_heads=None, num_frames=None,
              median_filter_width: int = 7, return_matrix: bool = False):
        """Forced alignment of given token sequences: `sequences` [B, P + n] (the first `prefix_len` = P columns the
        shared prompt ending in decoder_start, as generate()'s `.sequences`) against `encoder_outputs` [B, 1500, d]
        -> token_timestamps [B, P + n] f32 seconds (0 over the prefix), exactly what
        generate(return_token_timestamps=True) returns for those sequences. `return_matrix` also returns the DTW's
        cost matrices [B, n - 1, 1500] f32 (rows below each clip's length and columns below its frames are
        meaningful)."""
        if not self._loaded:
            raise _lib.WcbError("weights not loaded")
        seq = torch.as_tensor(sequences).to(self.device)
        if seq.dim() != 2:
            raise ValueError("sequences must be [B, P + n]")
        B, P = seq.shape[0], int(prefix_len)
        if not 1 <= P < seq.shape[1]:
            raise ValueError(f"prefix_len must lie in [1, {seq.shape[1] - 1}]")
        if P + (seq.shape[1] - P) - 1 > self.dims.n_text_ctx:
            raise ValueError("sequences longer than max_target_positions")
        if B > 64:
            raise ValueError("align takes at most 64 clips per call")
        if bool(((seq < 0) | (seq >= self.dims.vocab)).any()):
            raise ValueError(f"token ids outside [0, {self.dims.vocab})")
        if bool((seq[:, :P] != seq[:1, :P]).any()):
            raise ValueError("the prefix columns must be the same for every clip")
        akw = self._align_args(B, alignment_heads, num_frames, median_filter_width)
        enc = self._encoder_state(encoder_outputs)
        if enc.shape[0] != B:
            raise ValueError(f"encoder_outputs has {enc.shape[0]} clips, sequences {B}")
        prefix = [int(t) for t in seq[0, :P].tolist()]
        ids = seq[:, P:].to(torch.int32).contiguous()
        out = self._align_call(enc, ids, prefix, akw, akw["num_frames"], matrix=return_matrix)
        frames, mat = out if return_matrix else (out, None)
        ts = torch.zeros(B, seq.shape[1], dtype=torch.float32, device=self.device)
        ts[:, P:] = frames.to(torch.float32) * FRAME_SECONDS
        return (ts, mat) if return_matrix else ts

    kRetiredMax = 32

    def debug_counter(self, name: str) -> int:
        """wcb_debug_counter: e.g. "graph_captures", the decode graphs instantiated so far."""
        v = C.c_int64(0)
        _lib.check(self._lib.wcb_debug_counter(self._h, name.encode(), C.byref(v)), self._h, f"wcb_debug_counter({name})")
        return v.value

    def synchronize(self):
        """Wait for every queued front-end / encoder / decode operation of this model (and release the
        bias automatons evicted since the last call, now that no queued work reads them)."""
        _lib.check(self._lib.wcb_synchronize(self._h), self._h, "wcb_synchronize")
        self._bias_retired.clear()

    # ------------------------------------------------------------------------------- forward
    # forward() arguments of the reference signature (models/whisper_medical.py:45-65) that change nothing here:
    # Whisper's encoder ignores attention_mask, and return_dict / output flags left at their defaults
    _FORWARD_NOOP = {"attention_mask": None, "output_attentions": (None, False), "output_hidden_states": (None, False),
                     "cache_position": None, "decoder_attention_mask": None}

    def _encoder_state(self, encoder_outputs) -> torch.Tensor:
        """encoder_outputs as HF accepts it: a BaseModelOutput, a tuple whose [0] is the last hidden state
        ([tf] modeling_whisper.py WhisperModel.forward), or that tensor; [B, 1500, d], cast to the model dtype."""
        e = getattr(encoder_outputs, "last_hidden_state", None)
        if e is None:
            e = encoder_outputs[0] if isinstance(encoder_outputs, (tuple, list)) else encoder_outputs
        e = torch.as_tensor(e)
        if e.dim() == 2:
            e = e[None]
        if tuple(e.shape[1:]) != (self.dims.n_audio_ctx, self.dims.d_model):
            raise ValueError(f"encoder_outputs must be [B, {self.dims.n_audio_ctx}, {self.dims.d_model}], "
                             f"got {tuple(e.shape)}")
        return e.to(self.device, self.torch_dtype).contiguous()

    def forward(self, input_features=None, decoder_input_ids=None, labels=None, bias_spans=None,
                encoder_outputs=None, past_key_values=None, use_cache=None, return_dict: bool = True,
                **kwargs) -> Seq2SeqLMOutput:
        """Teacher-forced decoder logits (models/whisper_medical.py:45-172): from `input_features` (encoded
        here), from a given `encoder_outputs` (not re-encoded: bit-identical logits), or continuing a
        `past_key_values` cache. `use_cache=True` returns the cache as `.past_key_values` (a DecoderCache:
        one open per model); the default keeps none. The reference's weighted-CE `.loss` with `labels`."""
        for k, v in kwargs.items():
            ok = self._FORWARD_NOOP.get(k, "missing")
            if ok == "missing" or (v is not None and not (isinstance(ok, tuple) and v in ok)):
                raise NotImplementedError(f"forward(): argument {k}={v!r} is not supported by this path")
        if labels is not None:
            labels = torch.as_tensor(labels)
            if labels.shape[1] > self.dims.n_text_ctx:
                raise ValueError(f"Labels' sequence length {labels.shape[1]} cannot exceed the maximum allowed "
                                 f"length of {self.dims.n_text_ctx} tokens.")
            if decoder_input_ids is None:
                # shift_tokens_right ([tf] modeling_whisper.py:67-80)
                dec = torch.full_like(labels, self.dims.pad_token_id)
                dec[:, 1:] = labels[:, :-1].clone()
                dec[:, 0] = self.dims.decoder_start_token_id
                dec[dec == -100] = self.dims.pad_token_id
                decoder_input_ids = dec
        if decoder_input_ids is None:
            raise ValueError("forward() needs decoder_input_ids (or labels)")
        ids = torch.as_tensor(decoder_input_ids).to(self.device, torch.int32).contiguous()

        def out(logits, enc, cache=None):
            loss = None
            if labels is not None:
                from .loss import weighted_ce
                loss = weighted_ce(logits, labels.to(self.device), bias_spans, self.bias_weight)
            return Seq2SeqLMOutput(loss=loss, logits=logits, encoder_last_hidden_state=enc, past_key_values=cache)

        if past_key_values is not None:   # continue a cache: logits of the new positions only
            if not isinstance(past_key_values, DecoderCache) or past_key_values.model is not self:
                raise TypeError("past_key_values must be the DecoderCache this model returned (use_cache=True)")
            return out(past_key_values.extend(ids), past_key_values.encoder_last_hidden_state, past_key_values)
        if input_features is None and encoder_outputs is None:
            raise ValueError("You have to specify either input_features or encoder_outputs")
        if use_cache:
            enc = self._encoder_state(encoder_outputs) if encoder_outputs is not None else self.encode(input_features)
            if enc.shape[0] > 64:
                raise ValueError("use_cache=True takes at most 64 clips per cache")
            if self._cache is not None:
                self._cache.close()
            self._cache = DecoderCache(self, enc)
            return out(self._cache.extend(ids), enc, self._cache)
        if encoder_outputs is not None:
            enc = self._encoder_state(encoder_outputs)
            B, T = ids.shape
            if enc.shape[0] != B:
                raise ValueError(f"encoder_outputs has {enc.shape[0]} clips, decoder_input_ids {B} rows")
            logits = torch.empty(B, T, self.dims.vocab, dtype=torch.float32, device=self.device)
            for i in range(0, B, 64):   # 64 clips per library call
                n = min(64, B - i)
                _lib.check(self._lib.wcb_forward_enc(self._h, _ptr(enc[i:i + n]), n, _ptr(ids[i:i + n]), T,
                                                     _ptr(logits[i:i + n]), _stream(self.device)),
                           self._h, "wcb_forward_enc")
            return out(logits, enc)
        x = self._features(input_features)
        if x.shape[0] > 64:   # 64 clips per library call: split, concatenate
            outs = [self.forward(x[i:i + 64], decoder_input_ids=ids[i:i + 64]) for i in range(0, x.shape[0], 64)]
            return out(torch.cat([o.logits for o in outs]), torch.cat([o.encoder_last_hidden_state for o in outs]))
        B, T = ids.shape
        logits = torch.empty(B, T, self.dims.vocab, dtype=torch.float32, device=self.device)
        enc = torch.empty(B, self.dims.n_audio_ctx, self.dims.d_model, dtype=self.torch_dtype, device=self.device)
        _lib.check(self._lib.wcb_forward(self._h, _ptr(x), B, _ptr(ids), T, _ptr(logits), _ptr(enc),
                                         _stream(self.device)), self._h, "wcb_forward")
        return out(logits, enc)

    __call__ = forward

    # ---------------------------------------------------------------------------- profiling
    def profile_enable(self, on: bool = True, events: bool = True, stamps: bool = True):
        """HIP-event timing of front-end/encoder launches (`events`) and device-stamped timing of the
        decode cross-attention graph nodes (`stamps`); counters reset."""
        mode = (int(events) | (int(stamps) << 1)) if on else 0
        _lib.check(self._lib.wcb_profile_enable(self._h, mode), self._h, "wcb_profile_enable")

    def profile_read(self) -> Dict[str, dict]:
        n = 64
        names = (C.c_char * 32 * n)()
        launches = (C.c_int64 * n)()
        ms = (C.c_double * n)()
        flops = (C.c_double * n)()
        byts = (C.c_double * n)()
        cnt = _lib.check(self._lib.wcb_profile_read(self._h, n, names, launches, ms, flops, byts), self._h,
                         "wcb_profile_read")
        out = {}
        for i in range(min(cnt, n)):
            nm = bytes(names[i]).split(b"\0", 1)[0].decode()
            kname = C.create_string_buffer(512)
            grid = C.c_int64(0)
            _lib.check(self._lib.wcb_profile_kernel(self._h, i, kname, 512, C.byref(grid)), self._h,
                       "wcb_profile_kernel")
            out[nm] = dict(launches=launches[i], ms=ms[i], flops=flops[i], bytes=byts[i],
                           kernel=kname.value.decode(errors="replace"), grid=grid.value)
        return out
