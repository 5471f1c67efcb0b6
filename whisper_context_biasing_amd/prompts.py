"""Per-clip prompts of different lengths: the left-padded layout generate() and decode_begin() hand to the
library (wcb_generate_prompted / wcb_decode_begin_prompted) and return in `sequences`. Pure numpy.

Clip b's decoder prompt is its prompt tokens followed by the decoder start token, P_b = len(prompt b) + 1 tokens; a
batch is Pmax = max P_b wide and clip b sits right-aligned in row b, columns Pmax - P_b .. Pmax - 1, so the start
token of every clip is column Pmax - 1 and the generated tokens follow in the same columns for all clips (HF's
layout for batched decoder prompts). The columns before a clip's prompt hold the pad token."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

_SEQ = (list, tuple, np.ndarray)


def is_nested(prompt_ids) -> bool:
    """True for a sequence of per-clip prompts (each a sequence of ids, empty = no prompt); False for None and for
    one flat prompt."""
    if prompt_ids is None or not isinstance(prompt_ids, _SEQ):
        return False
    if isinstance(prompt_ids, np.ndarray):
        return prompt_ids.ndim == 2
    return len(prompt_ids) > 0 and all(isinstance(p, _SEQ) for p in prompt_ids)


def as_lists(prompt_ids) -> List[List[int]]:
    out = []
    for b, p in enumerate(prompt_ids):
        if isinstance(p, np.ndarray) and p.ndim != 1:
            raise ValueError(f"prompt_ids[{b}] must be a flat sequence of token ids")
        out.append([int(t) for t in p])
    return out


def pack_prompts(prompts: Sequence[Sequence[int]], start_token: int, pad_token: int) -> Tuple[np.ndarray, np.ndarray]:
    """prompts (B sequences of ids) -> (rows int32 [B, Pmax] left-padded with pad_token, each prompt followed by
    start_token; lengths int32 [B] = len(prompt b) + 1)."""
    if len(prompts) == 0:
        raise ValueError("prompt_ids: no clips")
    lens = np.asarray([len(p) + 1 for p in prompts], dtype=np.int32)
    P = int(lens.max())
    rows = np.full((len(prompts), P), int(pad_token), dtype=np.int32)
    for b, p in enumerate(prompts):
        rows[b, P - int(lens[b]):P - 1] = np.asarray(p, dtype=np.int32)
        rows[b, P - 1] = int(start_token)
    return rows, lens


def pack_rows(rows: Sequence[Tuple[Sequence[int], Sequence[int]]], start_token: int, pad_token: int) -> Tuple[np.ndarray, np.ndarray]:
    """pack_prompts for prompts that go on after the start token (generate(language=...)): rows = B pairs
    (prompt b, tail b), clip b's decoder prompt being prompt_b + [start_token] + tail_b -> (rows int32 [B, Pmax]
    left-padded with pad_token, lengths int32 [B] = len(prompt b) + 1 + len(tail b)). The tails of one batch have one
    length, so they occupy the same last columns in every row. With empty tails it is pack_prompts."""
    if len(rows) == 0:
        raise ValueError("prompt_ids: no clips")
    if len({len(t) for _, t in rows}) != 1:
        raise ValueError("pack_rows: the tails of one batch must have one length")
    full = [[int(t) for t in p] + [int(start_token)] + [int(t) for t in tail] for p, tail in rows]
    lens = np.asarray([len(r) for r in full], dtype=np.int32)
    P = int(lens.max())
    out = np.full((len(full), P), int(pad_token), dtype=np.int32)
    for b, r in enumerate(full):
        out[b, P - len(r):] = np.asarray(r, dtype=np.int32)
    return out, lens


def split_row(row, length: int, tail_len: int, width: int = None) -> Tuple[List[int], int, List[int]]:
    """One row of the packed layout (or of generate()'s `sequences`: pass width = Pmax, the prompt columns) with
    prompt_lengths[b] = `length` and a tail of `tail_len` tokens -> (prompt ids, the start token, tail ids)."""
    row = [int(t) for t in np.asarray(row).reshape(-1)]
    P = len(row) if width is None else int(width)
    if not (0 <= tail_len and tail_len + 1 <= length <= P <= len(row)):
        raise ValueError("split_row: tail_len + 1 <= length <= width <= len(row) expected")
    s = P - 1 - tail_len
    return row[P - length:s], row[s], row[s + 1:P]


def unpack_prompts(rows, lengths) -> List[List[int]]:
    """The inverse of pack_prompts on the first Pmax = max(lengths) columns of `rows` (generate()'s `sequences` or the
    packed rows): per clip its prompt ids, without the start token."""
    rows = np.asarray(rows)
    lengths = np.asarray(lengths).astype(np.int64)
    P = int(lengths.max())
    if rows.ndim != 2 or rows.shape[0] != lengths.shape[0] or rows.shape[1] < P or int(lengths.min()) < 1:
        raise ValueError("unpack_prompts: rows [B, >= max(lengths)] and lengths [B] >= 1 expected")
    return [[int(t) for t in rows[b, P - int(lengths[b]):P - 1]] for b in range(rows.shape[0])]

