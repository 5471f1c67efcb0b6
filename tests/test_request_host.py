"""Host: argument resolution of generate() / decode_begin() (whisper_context_biasing_amd/request.py) — the refusals,
the seed and temperature rules, what take() gives a subset of the clips, and the stripping of the collator's spans.
Pure Python: no library, no GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

from whisper_context_biasing_amd import get_dims
from whisper_context_biasing_amd.config import timestamp_ids
from whisper_context_biasing_amd.model import clip_seeds as model_clip_seeds
from whisper_context_biasing_amd.request import bias_source, clip_seeds, resolve, seed_array, span_lists

DIMS = get_dims("micro")
CONFIG = SimpleNamespace(max_length=448, num_beams=1)
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
PROMPTS = [[400, 500, 600], [], [7]]


def req(B=3, config=CONFIG, **kw):
    return resolve(DIMS, config, B, **kw)


class Prebuilt:   # stands for model.BiasList: opaque to the request
    pass


TS0 = timestamp_ids(DIMS)[0]
REFUSALS = [
    # tests/test_gpu_token_rules.py::test_refused_combinations
    (dict(return_timestamps=True, num_beams=2), "greedy only: num_beams must be 1"),
    (dict(suppress_tokens=[5], num_beams=2), "greedy only: num_beams must be 1"),
    (dict(return_timestamps=True, temperature=0.5), "return_timestamps with sampling or a temperature fallback"),
    (dict(return_timestamps=True, temperature=(0.0, 0.5)), "return_timestamps with sampling or a temperature fallback"),
    (dict(return_timestamps=True, do_sample=True), "return_timestamps with sampling or a temperature fallback"),
    (dict(max_initial_timestamp=1.0), "max_initial_timestamp needs return_timestamps=True"),
    (dict(suppress_tokens=[DIMS.vocab]), r"suppress id \d+ outside"),
    (dict(return_timestamps=True, suppress_tokens=[TS0 + 1]), "are timestamp tokens"),
    (dict(return_timestamps=True, max_initial_timestamp=-1.0), "max_initial_timestamp must be finite"),
    (dict(return_timestamps=True, block=False), "return_timestamps parses the ids on the host"),
    # tests/test_gpu_prompts.py::test_refusals
    (dict(prompt_ids=PROMPTS, num_beams=2), "per-clip prompts are greedy only"),
    (dict(prompt_ids=PROMPTS, return_token_timestamps=True), "return_token_timestamps with per-clip prompts"),
    (dict(prompt_ids=PROMPTS[:2]), "prompt_ids holds 2 prompts, the batch 3 clips"),
    (dict(prompt_ids=[[1], np.zeros((2, 2), dtype=np.int64), []]), "must be a flat sequence"),
    (dict(prompt_ids=list(range(DIMS.n_text_ctx - 1))), "prompt leaves no room for new tokens"),
    # tests/test_gpu_sampling.py::test_sampling_errors
    (dict(num_beams=2, temperature=0.5), "sampling .* is greedy only"),
    (dict(temperature=0.5, seed=[1, 2]), "seed has 2 entries, the batch 3 clips"),
    (dict(temperature=-0.5), "temperature must be finite and >= 0"),
    (dict(temperature=float("nan")), "temperature must be finite and >= 0"),
    (dict(num_beams=2, temperature=(0.0, 0.5)), "temperature fallback is greedy and sampling only"),
    (dict(temperature=(0.0, 0.5), seed=[1, 2]), "seed has 2 entries, the batch 3 clips"),
    (dict(temperature=(0.0, -0.5)), "temperature must be finite and >= 0"),
    (dict(temperature=()), "temperature: an empty sequence"),
    (dict(temperature=(0.0, 0.5), block=False), "temperature fallback reads every attempt's scores"),
    (dict(num_beams=9), r"num_beams must be in \[1, 8\]"),
    # tests/test_gpu_bias_per_utterance.py: the lists against the batch, with and without a boost
    (dict(bias_lists=[[[1]], []], bias_boost=2.0), "bias_lists has 2 lists, the batch 3 clips"),
    (dict(bias_lists=[[[1]], []]), "bias_lists has 2 lists, the batch 3 clips"),
    (dict(bias_lists=[[[1]], [], []], bias_list=Prebuilt()), "not as a prebuilt BiasList"),
    (dict(bias_spans=np.zeros((2, 1, 1), dtype=np.int64), per_utterance_bias=True, bias_boost=2.0), "bias_lists has 2 lists"),
    # token timestamps
    (dict(return_token_timestamps=True, block=False), "return_token_timestamps reads the ids"),
    (dict(return_token_timestamps=True, median_filter_width=4), "median_filter_width must be odd"),
    (dict(return_token_timestamps=True, median_filter_width=17), "above 15"),
    (dict(return_token_timestamps=True, alignment_heads=[]), "alignment_heads is empty"),
    (dict(return_token_timestamps=True, alignment_heads=[(DIMS.n_layers, 0)]), "alignment head"),
    (dict(return_token_timestamps=True, num_frames=[3000, 3000]), "num_frames has 2 entries"),
    (dict(return_token_timestamps=True, num_frames=[3000, 3000, 5]), "num_frames must lie in"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[f"{i}-{'-'.join(kw)}" for i, (kw, _) in enumerate(REFUSALS)])
def test_refusals(kw, message):
    with pytest.raises(ValueError, match=message):
        req(**kw)


def test_defaults_and_generation_config():
    r = req()
    assert (r.B, r.num_beams, r.max_length, r.min_new_tokens, r.bias_boost) == (3, 1, 448, 0, 0.0)
    assert r.use_graph and r.block and not (r.scored or r.as_dict or r.timestamps)
    assert r.temperature == 0.0 and r.seeds is None and r.temperatures is None and r.rules is None and r.align is None
    assert r.prompt is None and r.prompt_width == 1 and r.max_new(DIMS.n_text_ctx) == DIMS.n_text_ctx - 1
    r = req(config=SimpleNamespace(max_length=20, num_beams=4))
    assert (r.num_beams, r.max_length) == (4, 20)
    r = req(config=SimpleNamespace(max_length=20, num_beams=4), num_beams=2, max_length=7)
    assert (r.num_beams, r.max_length, r.max_new(DIMS.n_text_ctx)) == (2, 7, 7)
    assert req(config=SimpleNamespace(num_beams=None)).num_beams == 1
    # what implies a GenerateOutput
    for kw in (dict(return_dict_in_generate=True), dict(output_logprobs=True), dict(return_timestamps=True),
               dict(return_token_timestamps=True), dict(temperature=(0.0, 0.5))):
        assert req(**kw).as_dict, kw
    r = req(return_timestamps=True, suppress_tokens=[9, 5, 5], begin_suppress_tokens=[7], max_initial_timestamp=1.0)
    assert r.rules == ((5, 9), (7,), True, 50) and r.timestamps
    r = req(return_token_timestamps=True, num_frames=[2000], alignment_heads=[(1, 0)])
    assert r.align["heads"] == [(1, 0)] and r.align["width"] == 7 and r.align["num_frames"].tolist() == [2000] * 3


def test_temperature_rules():
    assert req(do_sample=True, temperature=0).temperature == 1.0
    assert req(do_sample=True, temperature=0.3).temperature == 0.3
    r = req(do_sample=False, temperature=0.7, seed=[1, 2])   # T = 0: a seed sequence of any length is ignored
    assert r.temperature == 0.0 and r.seeds is None
    assert req(temperature=0.0, seed=[1]).seeds is None
    r = req(temperature=0.7, seed=3)
    assert r.temperature == 0.7 and r.temperatures is None and np.array_equal(r.seeds, clip_seeds(3, 0, 3))
    r = req(temperature=(0.0, 0.2, 1.0), logprob_threshold=-0.5, compression_ratio_threshold=None, do_sample=True)
    assert r.temperatures == (0.0, 0.2, 1.0) and (r.logprob_threshold, r.compression_ratio_threshold) == (-0.5, None)
    assert r.seeds is None and r.attempt_seeds.shape == (3, 3) and r.block
    a0, a2 = r.attempt(0), r.attempt(2)   # an attempt: one scored decode; do_sample plays no part
    assert a0.temperature == 0.0 and a0.seeds is None and a0.temperatures is None and a0.scored and a0.as_dict
    assert a2.temperature == 1.0 and np.array_equal(a2.seeds, clip_seeds(0, 0, 3, attempt=2))
    assert req(temperature=np.asarray([0.0, 0.5])).temperatures == (0.0, 0.5)


def test_take_slices_the_whole_batch_seeds_for_a_split():
    assert model_clip_seeds is clip_seeds   # importable from the model, as ever
    r = req(B=66, temperature=0.9, seed=31)
    tail = r.take(range(64, 66))
    assert tail.B == 2 and tail.seeds.dtype == np.uint64 and tail.seeds.flags["C_CONTIGUOUS"]
    assert np.array_equal(tail.seeds, clip_seeds(31, 0, 66)[64:])
    assert np.array_equal(r.take(range(0, 64)).seeds, clip_seeds(31, 0, 64))
    explicit = list(range(100, 166))
    assert r.take([65, 2]).temperature == 0.9
    assert req(B=66, temperature=0.9, seed=explicit).take(range(64, 66)).seeds.tolist() == [164, 165]


def test_take_slices_the_whole_batch_seeds_for_a_fallback_attempt():
    todo = [1, 4, 5]
    r = req(B=6, temperature=(0.0, 0.5, 1.0), seed=42)
    for i in (1, 2):
        want = clip_seeds(42, 0, 6, attempt=i)[todo]
        assert np.array_equal(r.attempt(i).take(todo).seeds, want)
        assert np.array_equal(r.take(todo).attempt(i).seeds, want)
        assert np.array_equal(seed_array(42, 6, attempt=i)[todo], want)
    explicit = [5, 1 << 63, M64, M64 - 3, 0, M64 + 7]   # near 2^64: the sum wraps; above it: masked first
    r = req(B=6, temperature=(0.0, 0.5, 1.0), seed=explicit)
    for i in (0, 1, 2):
        want = [((explicit[b] & M64) + i * GOLDEN) % (1 << 64) for b in todo]
        got = r.attempt(i).take(todo)
        assert got.seeds is None if i == 0 else got.seeds.tolist() == want
        assert seed_array(explicit, 6, attempt=i)[todo].tolist() == want
    assert (M64 + 2 * GOLDEN) % (1 << 64) < M64 and r.attempt(2).seeds[2] == (M64 + 2 * GOLDEN) % (1 << 64)


def test_take_slices_per_clip_fields_and_shares_the_rest():
    lists = [[[1, 2]], [], [[3], [4, 5]]]
    r = req(prompt_ids=PROMPTS, bias_lists=lists, bias_list=[[9]], bias_boost=2.0, suppress_tokens=[5], max_length=12)
    assert r.per_clip_prompts and r.prompt == PROMPTS and r.prompt_width == 4 and r.bias_shared is None
    assert r.bias_lists == [[[1, 2], [9]], [[9]], [[3], [4, 5], [9]]]   # the shared phrases appended to every clip's
    sub = r.take([2, 1])
    assert sub.B == 2 and sub.prompt == [[7], []] and sub.prompt_width == 2   # packed at its own widest prompt
    assert sub.max_new(DIMS.n_text_ctx) == 12 and sub.bias_lists == [[[3], [4, 5], [9]], [[9]]]
    assert (sub.rules, sub.max_length, sub.bias_boost, sub.num_beams) == (r.rules, 12, 2.0, 1)
    wide = req(prompt_ids=[list(range(440)), [], [1]]).take([1, 2])   # the length cap follows the subset's width
    assert wide.max_new(DIMS.n_text_ctx) == DIMS.n_text_ctx - 2
    # a shared prompt and a shared list are left alone
    pre = Prebuilt()
    r = req(prompt_ids=[400, 500], bias_list=pre, bias_boost=2.0)
    sub = r.take([0, 2])
    assert not sub.per_clip_prompts and sub.prompt == [400, 500] and sub.prompt_width == 3 and sub.bias_shared is pre
    r = req(prompt_ids=np.asarray([400, 500]), bias_list=[[1, 2], [3]], bias_boost=2.0)
    assert r.take([1]).prompt == [400, 500] and r.take([1]).bias_shared == [[1, 2], [3]] and r.take([1]).bias_lists is None
    r = req(return_token_timestamps=True, num_frames=[1000, 2000, 3000])
    assert r.take([2, 0]).align["num_frames"].tolist() == [3000, 1000] and r.take([1]).align["width"] == 7


SPANS = np.asarray([[[11, 12, 50256], [0, 0, 0], [11, 12, 50256], [13, 50256, 50256]],
                    [[0, 0, 0], [50256, 50256, 50256], [0, 50256, 50256], [0, 0, 0]],
                    [[13, 50256, 50256], [14, 0, 15], [11, 12, 50256], [13, 50256, 50256]]])


def test_span_stripping():
    assert span_lists(SPANS) == [[[11, 12], [13]], [], [[13], [14, 0, 15], [11, 12]]]
    assert span_lists(SPANS, union=True) == [[11, 12], [13], [14, 0, 15]]
    assert span_lists(np.zeros((2, 1, 1), dtype=np.int64)) == [[], []]   # the collator's "no spans" form
    assert span_lists(np.zeros((2, 1, 1), dtype=np.int64), union=True) == []
    assert span_lists(SPANS.tolist()) == span_lists(SPANS)


def test_bias_source():
    calls = []

    def spans():
        calls.append(1)
        return SPANS

    assert bias_source(3, None, None, 0.0, spans) == (None, None) and not calls   # no boost: the spans are not read
    assert bias_source(3, [[1]], None, 2.0, spans) == ([[1]], None) and not calls   # an explicit list wins
    assert bias_source(3, None, None, 2.0, spans) == ([[11, 12], [13], [14, 0, 15]], None) and len(calls) == 1
    assert bias_source(3, None, None, 2.0, SPANS, per_utterance=True) == (None, span_lists(SPANS))
    assert bias_source(3, [[1]], None, 2.0, SPANS, per_utterance=True) == ([[1]], None)
    assert bias_source(3, None, [[], [], [[2]]], 2.0, spans, per_utterance=True) == (None, [[], [], [[2]]]) and len(calls) == 1
    # the union is taken over the whole batch, before any subset
    r = req(bias_spans=SPANS, bias_boost=2.0)
    assert r.take([1]).bias_shared == [[11, 12], [13], [14, 0, 15]] and r.bias_lists is None
    r = req(bias_spans=SPANS, bias_boost=2.0, per_utterance_bias=True)
    assert r.take([2, 1]).bias_lists == [[[13], [14, 0, 15], [11, 12]], []] and r.bias_shared is None
    r = req(bias_lists=[[[1]], [], []])   # no boost: checked, carried, and for the decode to leave unused
    assert r.bias_boost == 0.0 and r.bias_lists == [[[1]], [], []]
