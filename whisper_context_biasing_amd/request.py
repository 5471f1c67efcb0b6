"""What one generate() / decode_begin() call asks for, checked and normalised once, before any device work.
`resolve()` turns generate()'s arguments into a `DecodeRequest` or raises the ValueError; `DecodeRequest.take()` is
the request of a subset of its clips (a chunk of the split at 64 clips, the clips a temperature fallback decodes
again), the one place where per-clip fields are sliced. `rules_key`, `sampling_temperature`, `seed_array`, `bias_source`
and `align_args` serve decode_begin() too. Pure: stdlib, numpy and the package's pure modules; no library, no torch."""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, replace
from typing import Any, List, Optional, Tuple

import numpy as np

from . import prompts as _prompts
from .config import TIME_PRECISION, TASKS, is_multilingual, language_ids, language_token_id, task_ids, timestamp_ids

_M64 = (1 << 64) - 1


def _mix64(z: int) -> int:
    """splitmix64's finaliser: a bijection of the 64-bit integers."""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def clip_seeds(seed: int, first_clip: int, n: int, attempt: int = 0) -> np.ndarray:
    """The per-clip 64-bit sampling seeds an int `seed` stands for: clip c (its index in the WHOLE batch) of
    fallback attempt a draws with  mix64(mix64(seed) + (a << 32 | c))  (mix64 = splitmix64's finaliser, sums
    mod 2^64). Returns the seeds of clips first_clip .. first_clip + n - 1 as uint64 [n]. A pure function:
    mix64 is a bijection, so distinct (clip < 2^32, attempt < 2^32) give distinct seeds, a batch split anywhere
    gives the values of the unsplit batch, and every attempt draws fresh noise."""
    if not (0 <= int(first_clip) and int(first_clip) + int(n) <= 1 << 32 and 0 <= int(attempt) < 1 << 32):
        raise ValueError("clip_seeds: clip indices and attempt must fit 32 bits")
    base = _mix64(int(seed))
    return np.asarray([_mix64(base + ((int(attempt) << 32) | c)) for c in range(int(first_clip), int(first_clip) + int(n))],
                      dtype=np.uint64)


def seed_array(seed, B: int, attempt: int = 0) -> np.ndarray:
    """The seed rule: the uint64 [B] seeds of the whole batch for fallback attempt `attempt`. An int seed is expanded by
    clip_seeds(seed, 0, B, attempt); a sequence of B per-clip seeds s_b gives s_b + attempt·0x9E3779B97F4A7C15 (mod 2^64)."""
    if isinstance(seed, (int, np.integer)):
        return clip_seeds(int(seed), 0, B, attempt)
    seeds = np.ascontiguousarray(np.asarray([(int(v) + attempt * 0x9E3779B97F4A7C15) & _M64 for v in seed], dtype=np.uint64))
    if seeds.shape[0] != B:
        raise ValueError(f"seed has {seeds.shape[0]} entries, the batch {B} clips")
    return seeds


def compression_ratio(ids, vocab: int, eos: Optional[int] = None) -> float:
    """HF's `_retrieve_compression_ratio` ([tf] generation_whisper.py) of one clip's tokens: those before the
    first `eos` (all of them when eos is None or absent), each written as int(log2(vocab) / 8) + 1 little-endian
    bytes; len(bytes) / len(zlib.compress(bytes)). No tokens: 0.0."""
    toks = [int(t) for t in np.asarray(ids).reshape(-1)]
    if eos is not None and int(eos) in toks:
        toks = toks[:toks.index(int(eos))]
    if not toks:
        return 0.0
    length = int(math.log2(vocab) / 8) + 1
    data = b"".join(t.to_bytes(length, "little") for t in toks)
    return len(data) / len(zlib.compress(data))


def sampling_temperature(temperature, do_sample: Optional[bool] = None) -> float:
    """The temperature a call decodes at, 0 meaning argmax: do_sample=True makes a temperature of 0 mean 1,
    do_sample=False forces 0."""
    T = float(temperature)
    if do_sample and T == 0.0:
        T = 1.0
    if do_sample is False:
        T = 0.0
    if not (T >= 0.0 and math.isfinite(T)):
        raise ValueError(f"temperature must be finite and >= 0, got {temperature!r}")
    return T


def rules_key(dims, return_timestamps=False, suppress_tokens=None, begin_suppress_tokens=None, max_initial_timestamp=None):
    """The token rules the four generate() / decode_begin() arguments ask for, as a hashable key (None: none)."""
    sup = tuple(sorted({int(t) for t in (suppress_tokens or ())}))
    beg = tuple(sorted({int(t) for t in (begin_suppress_tokens or ())}))
    ts = bool(return_timestamps)
    for t in sup + beg:
        if not 0 <= t < dims.vocab:
            raise ValueError(f"suppress id {t} outside [0, {dims.vocab})")
    mi = -1
    if max_initial_timestamp is not None:
        if not ts:
            raise ValueError("max_initial_timestamp needs return_timestamps=True")
        if not (float(max_initial_timestamp) >= 0.0 and math.isfinite(float(max_initial_timestamp))):
            raise ValueError(f"max_initial_timestamp must be finite and >= 0, got {max_initial_timestamp!r}")
        mi = int(round(float(max_initial_timestamp) / TIME_PRECISION))
    if not (ts or sup or beg):
        return None
    if ts:
        ts0 = timestamp_ids(dims)[0]
        if ts0 <= dims.eos_token_id:
            raise ValueError("this vocabulary has no timestamp tokens past EOS")
        bad = [t for t in sup + beg if t >= ts0]
        if bad:
            raise ValueError(f"suppress ids {bad} are timestamp tokens (>= {ts0}): the grammar decides those")
    return (sup, beg, ts, mi)


NO_TOKEN_RULES = ((), (), False, -1)   # rules_key()'s form of "no deny list, no grammar" when only repeat rules ride along


def repeat_key(repetition_penalty=None, no_repeat_ngram_size=None, generation_config=None):
    """The repeat rules `repetition_penalty` / `no_repeat_ngram_size` ask for (HF's arguments; None: the
    generation config's when it has one, else 1.0 / 0) as (p, n), or None when both are off (p == 1.0 and n == 0)."""
    p, n = repetition_penalty, no_repeat_ngram_size
    if p is None:
        p = getattr(generation_config, "repetition_penalty", None)
    if n is None:
        n = getattr(generation_config, "no_repeat_ngram_size", None)
    p, n = 1.0 if p is None else p, 0 if n is None else n
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not (math.isfinite(float(p)) and float(p) > 0):
        raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {p!r}")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 0:
        raise ValueError(f"`no_repeat_ngram_size` has to be a non-negative integer, but is {n!r}")
    p, n = float(np.float32(p)), int(n)   # the library takes an f32
    return None if p == 1.0 and n == 0 else (p, n)


def split_rules(rules):
    """A request's `rules` value -> (the token rules as rules_key() gives them, or None; the repeat rules (p, n), or None)."""
    if rules is None or len(rules) == 4:
        return rules, None
    token = tuple(rules[:4])
    return (None if token == NO_TOKEN_RULES else token), rules[4]


def align_args(dims, B: int, alignment_heads, num_frames, median_filter_width) -> dict:
    """The checked alignment arguments (ValueError for what wcb_align refuses)."""
    W = int(median_filter_width)
    if W < 1 or W % 2 == 0:
        raise ValueError(f"median_filter_width must be odd and positive, got {median_filter_width!r}")
    if W > 15:
        raise ValueError("median_filter_width above 15 is not supported")
    heads = None
    if alignment_heads is not None:
        heads = [(int(l), int(h)) for l, h in alignment_heads]
        if not heads:
            raise ValueError("alignment_heads is empty")
        for l, h in heads:
            if not (0 <= l < dims.n_layers and 0 <= h < dims.n_heads):
                raise ValueError(f"alignment head ({l}, {h}) outside {dims.n_layers} layers x {dims.n_heads} heads")
        for l in {l for l, _ in heads}:
            if sum(1 for x, _ in heads if x == l) > 32:
                raise ValueError("more than 32 alignment heads in one layer")
    nf = None
    if num_frames is not None:
        nf = np.asarray(num_frames, dtype=np.int64).reshape(-1)
        if nf.shape[0] == 1 and B > 1:
            nf = np.repeat(nf, B)
        if nf.shape[0] != B:
            raise ValueError(f"num_frames has {nf.shape[0]} entries, the batch {B} clips")
        if (nf < 2 * W).any() or (nf > 2 * dims.n_audio_ctx).any():
            raise ValueError(f"num_frames must lie in [{2 * W}, {2 * dims.n_audio_ctx}]")
    return dict(heads=heads, num_frames=nf, width=W)


@dataclass(frozen=True)
class LanguagePlan:
    """What `language=` / `task=` / `language_candidates=` ask of a decode of B clips (resolve_language)."""
    ids: Optional[np.ndarray]            # int64 [B] language token ids; None with "auto" (the device fills them in)
    auto: bool                           # detect every clip's language on the device
    candidates: Optional[Tuple[int, ...]]   # token ids detection may choose from (None: every language)
    rest: Tuple[int, ...]                # the forced tokens after the language: the task, then <|notimestamps|> or not
    per_clip: bool                       # differing languages or "auto": the per-clip prompt path


def resolve_language(dims, B: int, language=None, task=None, language_candidates=None, *, timestamps: bool = False,
                     num_beams: int = 1, token_timestamps: bool = False) -> Optional[LanguagePlan]:
    """The language layer of a call (HF _retrieve_init_tokens: the decoder prompt continues [language, task] after the
    start token, task defaulting to transcribe, then <|notimestamps|> unless the call decodes with timestamps), or None
    when none of the three arguments is given. ValueError for what the call cannot mean."""
    if language is None and task is None and language_candidates is None:
        return None
    if not is_multilingual(dims):
        raise ValueError("language / task / language_candidates need a multilingual model: this vocabulary "
                         f"(eos {dims.eos_token_id}) has no language tokens")
    if language is None:
        raise ValueError("task needs language" if task is not None else 'language_candidates needs language="auto"')
    if task is not None and task not in TASKS:
        raise ValueError(f"The `{task}` task is not supported. The task should be one of {list(TASKS)}")
    auto = isinstance(language, str) and language.lower() == "auto"
    if language_candidates is not None and not auto:
        raise ValueError('language_candidates needs language="auto"')
    ids = cands = None
    if auto:
        if language_candidates is not None:
            cands = tuple(sorted({language_token_id(dims, l) for l in language_candidates}))
            if not cands:
                raise ValueError("language_candidates is empty")
    elif isinstance(language, (list, tuple, np.ndarray)):
        if len(language) != B:
            raise ValueError("When passing a list of languages, the length of the list must match the batch size. "
                             f"Expected length of {B}, but got {len(language)} languages.")
        ids = np.asarray([language_token_id(dims, l) for l in language], dtype=np.int64)
    else:
        ids = np.full(B, language_token_id(dims, language), dtype=np.int64)
    per_clip = auto or bool((ids != ids[0]).any())
    if per_clip and num_beams != 1:
        raise ValueError('differing languages or language="auto" are greedy only: num_beams must be 1 (the ragged path)')
    if per_clip and token_timestamps:
        raise ValueError('return_token_timestamps with differing languages or language="auto" is not supported '
                         "(the alignment pass takes one shared prefix)")
    rest = (task_ids(dims)[task or "transcribe"],) + (() if timestamps else (timestamp_ids(dims)[1],))
    return LanguagePlan(ids=ids, auto=auto, candidates=cands, rest=rest, per_clip=per_clip)


def candidate_bitmap(dims, candidates) -> Optional[np.ndarray]:
    """The candidate languages (token ids; None: every language) as the library's bitmap: uint32 words, bit i of word
    i // 32 = language lang_begin + i."""
    if candidates is None:
        return None
    lang_begin, n_lang = language_ids(dims)
    bits = np.zeros((n_lang + 31) // 32, dtype=np.uint32)
    for t in candidates:
        i = int(t) - lang_begin
        bits[i >> 5] |= np.uint32(1 << (i & 31))
    return bits


def span_lists(bias_spans, union: bool = False, pad: int = 50256):
    """The collator's padded per-sample spans ([B, N, L] ints; the pad is the literal 50256 whatever the model —
    data_utils/data_collator.py:107-125) with the padding stripped: row b's distinct spans, in first-seen order, are
    clip b's list; an all-zeros span (the [B, 1, 1] "no spans" form) is none. `union`: one list for the batch
    instead, the distinct spans of all rows in first-seen order."""
    out = []
    for sample in np.asarray(bias_spans):
        spans = [tuple(int(t) for t in span if int(t) != pad) for span in sample]
        out.append([list(s) for s in dict.fromkeys(spans) if s and any(s)])
    return [list(s) for s in dict.fromkeys(tuple(s) for L in out for s in L)] if union else out


def is_prebuilt(bias_list) -> bool:
    """A shared bias list given as a prebuilt automaton (model.BiasList, opaque here), not as phrases."""
    return bias_list is not None and not hasattr(bias_list, "__iter__")


def bias_source(B: int, bias_list, bias_lists, bias_boost: float, bias_spans=None, per_utterance: bool = False):
    """Which bias source applies to a batch of B clips -> (shared, lists), at most one not None: `bias_lists` (checked
    against B, also when bias_boost is 0; a shared `bias_list` of phrases is appended to every clip's); else the shared
    `bias_list` (phrases or a prebuilt automaton, passed through); else, with bias_boost > 0, the batch's `bias_spans` (the
    array, or a callable that returns it, called only here): per clip with `per_utterance`, else their union over the batch."""
    if bias_lists is None and bias_list is None and bias_boost > 0 and bias_spans is not None:
        found = span_lists(bias_spans() if callable(bias_spans) else bias_spans, union=not per_utterance)
        bias_list, bias_lists = (None, found) if per_utterance else (found, None)
    if bias_lists is None:
        return bias_list, None
    lists = [[list(map(int, p)) for p in L] for L in bias_lists]
    if len(lists) != B:
        raise ValueError(f"bias_lists has {len(lists)} lists, the batch {B} clips")
    if is_prebuilt(bias_list):
        raise ValueError("bias_lists takes a shared bias_list as phrases, not as a prebuilt BiasList")
    shared = [list(map(int, p)) for p in (() if bias_list is None else bias_list)]
    return None, [L + shared for L in lists]


@dataclass(frozen=True)
class DecodeRequest:
    """Everything a decode of B clips needs. Per clip: seeds, attempt_seeds, prompt (with per_clip_prompts),
    bias_lists and align["num_frames"]; the rest is shared by any subset of the clips."""
    B: int
    num_beams: int
    max_length: int
    min_new_tokens: int
    bias_boost: float
    use_graph: bool
    block: bool
    temperature: float = 0.0                      # 0: argmax
    seeds: Optional[np.ndarray] = None            # uint64 [B] exactly when temperature > 0
    temperatures: Optional[Tuple[float, ...]] = None   # the temperature fallback's (None: one decode), and ...
    attempt_seeds: Optional[np.ndarray] = None    # ... uint64 [attempts, B]: attempt i samples with attempt_seeds[i]
    logprob_threshold: Optional[float] = None
    compression_ratio_threshold: Optional[float] = None
    prompt: Optional[list] = None                 # one flat prompt, or with per_clip_prompts B prompts
    per_clip_prompts: bool = False
    bias_shared: Any = None                       # phrases, or a prebuilt automaton
    bias_lists: Optional[List[List[List[int]]]] = None
    rules: Optional[tuple] = None                 # rules_key(), + ((p, n),) with repeat rules on (split_rules)
    scored: bool = False
    as_dict: bool = False
    timestamps: bool = False
    align: Optional[dict] = None                  # align_args() when token timestamps are asked for
    language: Optional[LanguagePlan] = None       # resolve_language() when language= is given (ids: per clip)

    @property
    def tail_width(self) -> int:
        """Forced tokens after the start token: the language, the task and <|notimestamps|> (0 without language=)."""
        return 0 if self.language is None else 1 + len(self.language.rest)

    @property
    def packed(self) -> bool:
        """The call goes through the per-clip prompt path: per-clip prompts, differing languages or "auto"."""
        return self.per_clip_prompts or (self.language is not None and self.language.per_clip)

    def clip_rows(self, placeholder: int) -> List[List[int]]:
        """Every clip's decoder prompt for the per-clip path: prompt_b + [start] + tail_b, without the start token's id
        (the caller's: rows[b] = (prompt_b, tail_b)); `placeholder` stands where the device writes a detected language."""
        prompts = self.prompt if self.per_clip_prompts else [list(self.prompt or ())] * self.B
        if self.language is None:
            return [(list(p), []) for p in prompts]
        L = self.language
        return [(list(p), [placeholder if L.ids is None else int(L.ids[b])] + list(L.rest)) for b, p in enumerate(prompts)]

    @property
    def prompt_width(self) -> int:
        """Columns of the decoder prompt: the (widest) prompt, the start token and the forced tail."""
        if self.per_clip_prompts:
            return 1 + max(len(p) for p in self.prompt) + self.tail_width
        return 1 + len(self.prompt or ()) + self.tail_width

    def max_new(self, n_text_ctx: int) -> int:
        """HF: max_length + prompt tokens, capped at max_target_positions ([tf] generation_whisper.py:1932-1940)."""
        n = min(self.max_length, n_text_ctx - self.prompt_width)
        if n < 1:
            raise ValueError("prompt leaves no room for new tokens")
        return n

    def take(self, indices) -> "DecodeRequest":
        """The request of clips `indices` of this batch, each keeping what it has in the whole batch."""
        idx = np.asarray(indices, dtype=np.int64)
        cut = lambda a, axis=0: None if a is None else np.ascontiguousarray(np.take(a, idx, axis))   # noqa: E731
        rows = lambda L: None if L is None else [L[b] for b in idx]   # noqa: E731
        return replace(self, B=len(idx), seeds=cut(self.seeds), attempt_seeds=cut(self.attempt_seeds, 1),
                       prompt=rows(self.prompt) if self.per_clip_prompts else self.prompt, bias_lists=rows(self.bias_lists),
                       align=self.align and dict(self.align, num_frames=cut(self.align["num_frames"])),
                       language=self.language and replace(self.language, ids=cut(self.language.ids)))

    def with_languages(self, ids) -> "DecodeRequest":
        """This request with every clip's language given (ids [B]: what an "auto" decode detected): still the per-clip path."""
        return replace(self, language=replace(self.language, ids=np.asarray(ids, dtype=np.int64).reshape(-1), auto=False,
                                              candidates=None))

    def attempt(self, i: int) -> "DecodeRequest":
        """Attempt i of the temperature fallback: one scored decode of these clips at temperatures[i]."""
        T = self.temperatures[i]
        return replace(self, temperature=T, seeds=self.attempt_seeds[i] if T > 0.0 else None, temperatures=None,
                       attempt_seeds=None, scored=True, as_dict=True)


def resolve(dims, generation_config, B: int, *, bias_spans=None, max_length=None, num_beams=None, bias_list=None,
            bias_boost=0.0, min_new_tokens=0, prompt_ids=None, return_dict_in_generate=False, use_graph=True, block=True,
            bias_lists=None, per_utterance_bias=False, output_logprobs=False, temperature=0.0, seed=0, do_sample=None,
            logprob_threshold=-1.0, compression_ratio_threshold=2.4, return_timestamps=False, suppress_tokens=None,
            begin_suppress_tokens=None, max_initial_timestamp=None, return_token_timestamps=False, alignment_heads=None,
            num_frames=None, median_filter_width=7, language=None, task=None, language_candidates=None,
            repetition_penalty=None, no_repeat_ngram_size=None) -> DecodeRequest:
    """generate()'s arguments for a batch of B clips -> the DecodeRequest, or the ValueError of what the call cannot mean.
    `generation_config` is the effective one (it defaults max_length and num_beams); `bias_spans` as bias_source() takes it."""
    nb = int(num_beams if num_beams is not None else getattr(generation_config, "num_beams", 1) or 1)
    if max_length is None:
        max_length = getattr(generation_config, "max_length", 448)
    fallback, per_clip = isinstance(temperature, (list, tuple, np.ndarray)), _prompts.is_nested(prompt_ids)
    prompt = _prompts.as_lists(prompt_ids) if per_clip else None if prompt_ids is None else [int(t) for t in prompt_ids]
    temps = tuple(sampling_temperature(t) for t in temperature) if fallback else None   # do_sample plays no part then
    T = 0.0 if fallback else sampling_temperature(temperature, do_sample)
    rules = rules_key(dims, return_timestamps, suppress_tokens, begin_suppress_tokens, max_initial_timestamp)
    repeat = repeat_key(repetition_penalty, no_repeat_ngram_size, generation_config)
    lang = resolve_language(dims, B, language, task, language_candidates, timestamps=bool(return_timestamps), num_beams=nb,
                            token_timestamps=bool(return_token_timestamps))
    for refused, why in (   # what the library, or the host side of the decode, cannot do
            (per_clip and return_token_timestamps,
             "return_token_timestamps with per-clip prompts is not supported (the alignment pass takes one shared prefix)"),
            (per_clip and nb != 1, "per-clip prompts are greedy only: num_beams must be 1 (beam scores count the prompt)"),
            (per_clip and len(prompt or ()) != B, f"prompt_ids holds {len(prompt or ())} prompts, the batch {B} clips"),
            (return_token_timestamps and not block,
             "return_token_timestamps reads the ids of the finished decode: block=False is not supported"),
            (repeat is not None and nb != 1, "repetition_penalty / no_repeat_ngram_size are greedy only: num_beams must be 1"),
            (repeat is not None and (fallback or T > 0.0),
             "repetition_penalty / no_repeat_ngram_size with sampling or a temperature fallback are not supported"),
            (repeat is not None and bool(return_timestamps),
             "repetition_penalty / no_repeat_ngram_size with return_timestamps are not supported (hence not in transcribe_long)"),
            (rules is not None and nb != 1,
             "suppress_tokens / begin_suppress_tokens / return_timestamps are greedy only: num_beams must be 1"),
            (return_timestamps and (fallback or T > 0.0),
             "return_timestamps with sampling or a temperature fallback is not supported"),
            (return_timestamps and not block, "return_timestamps parses the ids on the host: block=False is not supported"),
            (fallback and not block, "temperature fallback reads every attempt's scores: block=False is not supported"),
            (fallback and not temps, "temperature: an empty sequence"),
            (fallback and nb != 1, "temperature fallback is greedy and sampling only: num_beams must be 1"),
            (T > 0.0 and nb != 1, "sampling (temperature > 0) is greedy only: num_beams must be 1"),
            (not 1 <= nb <= 8, "num_beams must be in [1, 8]")):
        if refused:
            raise ValueError(why)
    shared, lists = bias_source(B, bias_list, bias_lists, bias_boost, bias_spans, per_utterance_bias)
    if repeat is not None:   # carried inside `rules`: the token rules' 4-tuple (or its empty form), then (p, n)
        rules = (rules or NO_TOKEN_RULES) + (repeat,)
    req = DecodeRequest(
        B=B, num_beams=nb, max_length=int(max_length), min_new_tokens=int(min_new_tokens), bias_boost=float(bias_boost),
        use_graph=bool(use_graph), block=bool(block), temperature=T,
        seeds=seed_array(seed, B) if T > 0.0 else None,   # with T = 0 a seed of any form is ignored
        temperatures=temps, attempt_seeds=np.stack([seed_array(seed, B, i) for i in range(len(temps))]) if fallback else None,
        logprob_threshold=logprob_threshold, compression_ratio_threshold=compression_ratio_threshold,
        prompt=prompt, per_clip_prompts=per_clip, bias_shared=shared, bias_lists=lists, rules=rules,
        scored=bool(output_logprobs), timestamps=bool(return_timestamps),
        align=align_args(dims, B, alignment_heads, num_frames, median_filter_width) if return_token_timestamps else None,
        as_dict=bool(return_dict_in_generate or output_logprobs or return_timestamps or return_token_timestamps or fallback
                     or (lang is not None and lang.auto)),   # (a detected language is part of the result)
        language=lang)
    req.max_new(dims.n_text_ctx)
    return req
