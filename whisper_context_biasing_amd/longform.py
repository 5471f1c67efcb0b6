"""Long-form transcription on the host: the seek loop of HF `WhisperGenerationMixin.generate` for audio past 30 s,
restricted to the greedy, temperature-0 path. Pure Python and numpy, like request.py and prompts.py:
no library, no torch.

One clip has `max_frames` mel frames (0.01 s each) and a `seek` that starts at 0. While seek < max_frames the clip is
active: its next window is the frames [seek, seek + seek_num_frames), seek_num_frames = min(max_frames - seek, 3000),
zero-padded to 3000; the window is decoded with the timestamp grammar and the ids decide how far seek advances
(`retrieve_segments`, HF `_retrieve_segment`). With `condition_on_prev_tokens` the decoder prompt of a window carries
the clip's earlier text (`window_prompt`, HF `_prepare_decoder_input_ids`). `LongFormState` holds the loop state of a
batch; every rule is per clip, so a clip's result never depends on the clips it is batched with."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .config import N_FRAMES, TIME_PRECISION

INPUT_STRIDE = 2                 # mel frames per encoder position (conv2's stride): one timestamp step = 2 frames
FRAME_PRECISION = 0.01           # seconds per mel frame (HF time_precision_features)


def seek_num_frames(seek: int, max_frames: int) -> int:
    return min(int(max_frames) - int(seek), N_FRAMES)


def strip_window(ids: Sequence[int], eos: int, pad: int) -> List[int]:
    """The generated ids of one window as HF's fallback loop hands them to `_retrieve_segment`: the trailing pads
    dropped (all but one when pad == eos: that one is the row's EOS), then the final EOS."""
    seq = [int(t) for t in ids]
    if seq and seq[-1] == pad:
        n = sum(1 for t in seq if t == pad) - (1 if pad == eos else 0)
        if n:
            seq = seq[:-n]
    if seq and seq[-1] == eos:
        seq = seq[:-1]
    return seq


def retrieve_segments(seq: Sequence[int], seek: int, num_frames: int, timestamp_begin: int) -> Tuple[list, int]:
    """HF `_retrieve_segment` on the stripped ids `seq` of a window that starts at mel frame `seek` and holds `num_frames`
    frames -> (segments, segment_offset). A segment is (start_s, end_s, token_ids) in absolute seconds (float64, HF's
    own arithmetic: seek * 0.02 / 2 + timestamp index * 0.02), its tokens including the timestamps that delimit it.
    Segments split at consecutive timestamp pairs. segment_offset, the frames seek advances by: the last closed pair's
    timestamp * 2, or `num_frames` when the ids end in a single timestamp or hold no pair. Without a pair the whole
    sequence is one segment that ends at its last timestamp if it has one other than <|0.00|>, else at the window's end."""
    seq = [int(t) for t in seq]
    ts0 = int(timestamp_begin)
    is_ts = [t >= ts0 for t in seq]
    offset = float(seek) * TIME_PRECISION / INPUT_STRIDE
    single_ending = is_ts[-2:] == [False, True]
    slices = [i + 1 for i in range(len(seq) - 1) if is_ts[i] and is_ts[i + 1]]
    if slices:
        if single_ending:
            slices.append(len(seq))
        else:
            slices[-1] += 1   # the last segment keeps both closing timestamps: it did not end in a single one
        segments, last = [], 0
        for i, cur in enumerate(slices):
            toks = seq[last:cur]
            end_i = -1 if (i != len(slices) - 1 or single_ending) else -2
            segments.append((offset + float(toks[0] - ts0) * TIME_PRECISION, offset + float(toks[end_i] - ts0) * TIME_PRECISION,
                             toks))
            last = cur
        if single_ending:
            return segments, int(num_frames)
        return segments, (seq[last - 2] - ts0) * INPUT_STRIDE
    last_pos = float(int(int(num_frames) * FRAME_PRECISION / TIME_PRECISION))
    stamps = [t for t in seq if t >= ts0]
    if stamps and stamps[-1] != ts0:
        last_pos = float(stamps[-1] - ts0)
    return [(offset, offset + last_pos * TIME_PRECISION, seq)], int(num_frames)


def previous_tokens(segment_tokens: Sequence[Sequence[int]], timestamp_begin: int, cut_off_length: int) -> List[int]:
    """The clip's earlier text as HF `_pad_to_max_length(skip_ending_double_timestamps=True, cut_off_length=...)`
    joins it: every segment's tokens, a segment that ends in two timestamps without its last token, the last
    `cut_off_length` tokens of the concatenation."""
    out: List[int] = []
    for toks in segment_tokens:
        toks = [int(t) for t in toks]
        out += toks[:-1] if (len(toks) > 2 and toks[-2] >= timestamp_begin) else toks
    return out[-int(cut_off_length):]


def window_prompt(segment_tokens: Sequence[Sequence[int]], *, condition_on_prev_tokens: bool, prev_sot: int, timestamp_begin: int,
                  n_text_ctx: int, prompt_ids: Optional[Sequence[int]] = None,
                  prompt_condition_type: str = "first-segment") -> List[int]:
    """The decoder prompt of a clip's next window WITHOUT the start token (the library appends it), HF
    `_prepare_decoder_input_ids`: with conditioning on and at least one earlier segment, <|startofprev|> (or, with
    prompt_condition_type "all-segments", the user's prompt_ids) + the last n_text_ctx // 2 - 1 previous tokens; else
    the user's prompt_ids if any; else nothing. `segment_tokens`: the token lists of the clip's segments so far (with
    "first-segment" the state puts the user's prompt there as a pseudo-segment, as HF `_prepare_segments` does)."""
    if condition_on_prev_tokens and len(segment_tokens) > 0:
        head = [int(t) for t in prompt_ids] if (prompt_ids is not None and prompt_condition_type == "all-segments") else [int(prev_sot)]
        return head + previous_tokens(segment_tokens, timestamp_begin, n_text_ctx // 2 - 1)
    if prompt_ids is not None:
        return [int(t) for t in prompt_ids]
    return []


def should_skip(avg_logprob: float, no_speech_prob: float, logprob_threshold: Optional[float],
                no_speech_threshold: Optional[float]) -> bool:
    """HF `_need_fallback`'s skip rule: the window holds no speech."""
    if no_speech_threshold is None or logprob_threshold is None:
        return False
    return bool(avg_logprob < logprob_threshold and no_speech_prob > no_speech_threshold)


def check_args(*, temperature=0.0, num_beams=1, return_token_timestamps=False, condition_on_prev_tokens=False, prompt_ids=None,
               prompt_condition_type="first-segment") -> None:
    """The ValueErrors of transcribe_long's arguments, before any device work."""
    if isinstance(temperature, (list, tuple, np.ndarray)) or float(temperature) > 0.0:
        raise ValueError("long-form decoding is temperature 0 only: the timestamp grammar needs the unperturbed text "
                         "maximum, so neither sampling nor the temperature fallback runs inside the seek loop")
    if int(num_beams) != 1:
        raise ValueError("long-form decoding is greedy only: num_beams must be 1")
    if return_token_timestamps and condition_on_prev_tokens:
        raise ValueError("return_token_timestamps with condition_on_prev_tokens is not supported (the alignment pass "
                         "takes one shared prefix)")
    if prompt_condition_type not in ("first-segment", "all-segments"):
        raise ValueError("prompt_condition_type must be 'first-segment' or 'all-segments'")
    if prompt_condition_type == "all-segments" and prompt_ids is not None and not condition_on_prev_tokens:
        raise ValueError("prompt_condition_type='all-segments' needs condition_on_prev_tokens=True")


class LongFormState:
    """The seek loop's state for a batch of clips: seek, max_frames, and per clip the segments, the window starts and the
    per-window figures. Drive it as: while active(): windows(a), prompts(a), decode, update(a, ...)."""

    def __init__(self, max_frames: Sequence[int], *, eos: int, pad: int, timestamp_begin: int, prev_sot: int, n_text_ctx: int,
                 condition_on_prev_tokens: bool = False, prompt_ids: Optional[Sequence[int]] = None,
                 prompt_condition_type: str = "first-segment", logprob_threshold: Optional[float] = -1.0,
                 no_speech_threshold: Optional[float] = None):
        self.max_frames = [int(v) for v in max_frames]
        if any(v < 1 for v in self.max_frames):
            raise ValueError("every clip needs at least one mel frame")
        B = len(self.max_frames)
        self.eos, self.pad, self.ts0, self.prev_sot, self.n_text_ctx = int(eos), int(pad), int(timestamp_begin), int(prev_sot), int(n_text_ctx)
        self.condition = bool(condition_on_prev_tokens)
        self.prompt_ids = None if prompt_ids is None else [int(t) for t in prompt_ids]
        self.prompt_type = prompt_condition_type
        self.logprob_threshold, self.no_speech_threshold = logprob_threshold, no_speech_threshold
        self.seek = [0] * B
        self.segments: List[list] = [[] for _ in range(B)]      # (start_s, end_s, token_ids)
        self.seeks: List[List[int]] = [[] for _ in range(B)]
        self.avg_logprobs: List[List[float]] = [[] for _ in range(B)]
        self.no_speech_probs: List[List[float]] = [[] for _ in range(B)]
        self.skipped: List[List[bool]] = [[] for _ in range(B)]
        self.window_ids: List[List[List[int]]] = [[] for _ in range(B)]   # every window's stripped ids, skipped ones too
        # HF _prepare_segments: a "first-segment" prompt counts as the clip's first segment, minus its <|startofprev|>
        self._head = None
        if self.prompt_ids is not None and self.prompt_type == "first-segment":
            self._head = self.prompt_ids[1:] if (self.prompt_ids and self.prompt_ids[0] == self.prev_sot) else self.prompt_ids

    def active(self) -> List[int]:
        return [b for b in range(len(self.seek)) if self.seek[b] < self.max_frames[b]]

    def windows(self, active: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
        """(seek, seek_num_frames) int32 [len(active)] of the active clips' next windows."""
        s = np.asarray([self.seek[b] for b in active], dtype=np.int32)
        n = np.asarray([seek_num_frames(self.seek[b], self.max_frames[b]) for b in active], dtype=np.int32)
        return s, n

    def _segment_tokens(self, b: int) -> list:
        head = [self._head] if self._head is not None else []
        return head + [toks for _, _, toks in self.segments[b]]

    def prompts(self, active: Sequence[int]) -> List[List[int]]:
        """The decoder prompts (without the start token) of the active clips' next windows."""
        return [window_prompt(self._segment_tokens(b), condition_on_prev_tokens=self.condition, prev_sot=self.prev_sot,
                              timestamp_begin=self.ts0, n_text_ctx=self.n_text_ctx, prompt_ids=self.prompt_ids,
                              prompt_condition_type=self.prompt_type) for b in active]

    def update(self, active: Sequence[int], ids, avg_logprob=None, no_speech_prob=None) -> None:
        """Fold one decode of the active clips' windows into the state: ids [len(active), n] the generated columns."""
        for i, b in enumerate(active):
            n = seek_num_frames(self.seek[b], self.max_frames[b])
            lp = float(avg_logprob[i]) if avg_logprob is not None else float("nan")
            ns = float(no_speech_prob[i]) if no_speech_prob is not None else float("nan")
            self.seeks[b].append(self.seek[b])
            self.avg_logprobs[b].append(lp)
            self.no_speech_probs[b].append(ns)
            skip = no_speech_prob is not None and avg_logprob is not None and should_skip(
                lp, ns, self.logprob_threshold, self.no_speech_threshold)
            self.skipped[b].append(bool(skip))
            seq = strip_window(ids[i], self.eos, self.pad)
            self.window_ids[b].append(seq)
            if skip:
                self.seek[b] += n
                continue
            segs, off = retrieve_segments(seq, self.seek[b], n, self.ts0)
            self.segments[b] += segs
            self.seek[b] += int(off)

    def sequences(self) -> np.ndarray:
        """[B, W] int64: every clip's segments' tokens in order, right-padded with pad, as HF returns them."""
        rows = [[t for _, _, toks in segs for t in toks] for segs in self.segments]
        W = max((len(r) for r in rows), default=0)
        out = np.full((len(rows), W), self.pad, dtype=np.int64)
        for b, r in enumerate(rows):
            out[b, :len(r)] = r
        return out
