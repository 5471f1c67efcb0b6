"""Host: the language layer of generate() / decode_begin() / transcribe_long() — the tables against
transformers', the ids of both multilingual vocabularies, the forced tail against HF's `_retrieve_init_tokens`, every
refusal with its message, the invariant that a request resolved without the new arguments is today's request, the
packed layout with tails and the long-form window prompt with a tail. Pure Python: no library, no GPU."""
import os
from dataclasses import fields
from types import SimpleNamespace

import numpy as np
import pytest

from whisper_context_biasing_amd import config as CFG
from whisper_context_biasing_amd import get_dims
from whisper_context_biasing_amd import prompts as P
from whisper_context_biasing_amd.longform import window_prompt
from whisper_context_biasing_amd.request import DecodeRequest, candidate_bitmap, resolve, resolve_language

SMALL, LARGE, EN, MICRO = get_dims("small"), get_dims("large-v3"), get_dims("tiny.en"), get_dims("micro")
CONFIG = SimpleNamespace(max_length=448, num_beams=1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def req(B=3, dims=SMALL, **kw):
    return resolve(dims, CONFIG, B, **kw)


# ------------------------------------------------------------------------------------------------ tables
def test_tables_match_transformers():
    tw = pytest.importorskip("transformers.models.whisper.tokenization_whisper")
    assert list(CFG.LANGUAGES.items()) == list(tw.LANGUAGES.items())   # the order is the token order
    assert CFG.TO_LANGUAGE_CODE == tw.TO_LANGUAGE_CODE
    assert len(CFG.LANGUAGE_CODES) == 100 and CFG.LANGUAGE_CODES[-1] == "yue"


def test_ids_of_both_vocabularies():
    assert CFG.language_ids(SMALL) == (50259, 99) and CFG.language_ids(LARGE) == (50259, 100)
    assert CFG.task_ids(SMALL) == {"translate": 50357, "transcribe": 50358}
    assert CFG.task_ids(LARGE) == {"translate": 50358, "transcribe": 50359}
    assert CFG.is_multilingual(SMALL) and CFG.is_multilingual(MICRO) and not CFG.is_multilingual(EN)
    assert CFG.language_token_id(SMALL, "en") == 50259 and CFG.language_token_id(SMALL, "su") == 50357
    assert CFG.language_token_id(LARGE, "yue") == 50358
    for spelling in ("fr", "FR", "french", "French", "<|fr|>", "<|FR|>", 50265, np.int64(50265)):
        assert CFG.language_token_id(SMALL, spelling) == 50265, spelling
    assert CFG.language_token_id(SMALL, "castilian") == CFG.language_token_id(SMALL, "es")
    assert CFG.language_code(SMALL, 50265) == "fr"
    # derived from dims, nothing hard-coded: another start token moves the range
    moved = get_dims("small", decoder_start_token_id=50300)
    assert CFG.language_ids(moved)[0] == 50301


def hf_init_tokens(dims, language, task, timestamps):
    """HF's own `_retrieve_init_tokens` on a bare object: no model, no weights"""
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    lang_begin, n_lang = CFG.language_ids(dims)
    gc = SimpleNamespace(decoder_start_token_id=dims.decoder_start_token_id, task=task, language=language,
                         lang_to_id={f"<|{CFG.LANGUAGE_CODES[i]}|>": lang_begin + i for i in range(n_lang)},
                         task_to_id=CFG.task_ids(dims), no_timestamps_token_id=CFG.timestamp_ids(dims)[1],
                         return_timestamps=timestamps, forced_decoder_ids=None)
    me = SimpleNamespace(device="cpu")
    B = len(language) if isinstance(language, list) else 2
    out = gw.WhisperGenerationMixin._retrieve_init_tokens(me, None, B, gc, SimpleNamespace(forced_decoder_ids=None), 3000, {})
    return out.numpy()


@pytest.mark.parametrize("dims", [SMALL, LARGE], ids=["51865", "51866"])
@pytest.mark.parametrize("timestamps", [False, True])
@pytest.mark.parametrize("language,task", [("fr", None), ("French", "translate"), ("<|de|>", "transcribe"),
                                           (["fr", "ja"], None), (["en", "zh"], "translate")])
def test_forced_tail_equals_hf(dims, language, task, timestamps):
    hf = hf_init_tokens(dims, language, task, timestamps)
    B = hf.shape[0]
    r = req(B, dims, language=language, task=task, return_timestamps=timestamps)
    rows = r.clip_rows(-1)
    mine = np.asarray([[dims.decoder_start_token_id] + tail for _, tail in rows])
    assert np.array_equal(mine, hf), (mine, hf)
    assert r.tail_width == hf.shape[1] - 1 and r.prompt_width == hf.shape[1]
    assert r.language.per_clip == (isinstance(language, list))


# ---------------------------------------------------------------------------------------------- refusals
REFUSALS = [
    (EN, dict(language="en"), "need a multilingual model"),
    (EN, dict(task="transcribe"), "need a multilingual model"),
    (EN, dict(language_candidates=["en"]), "need a multilingual model"),
    (SMALL, dict(task="translate"), "task needs language"),
    (SMALL, dict(language="fr", language_candidates=["fr", "de"]), 'language_candidates needs language="auto"'),
    (SMALL, dict(language_candidates=["fr", "de"]), 'language_candidates needs language="auto"'),
    (SMALL, dict(language="klingon"), "Unsupported language: klingon"),
    (SMALL, dict(language="yue"), r"<\|yue\|> is not supported by this model"),
    (SMALL, dict(language="auto", language_candidates=["xx"]), "Unsupported language: xx"),
    (SMALL, dict(language=["fr", "de"]), "Expected length of 3, but got 2 languages"),
    (SMALL, dict(language="fr", task="summarise"), "task is not supported"),
    (SMALL, dict(language=["fr", "de", "fr"], num_beams=2), "greedy only: num_beams must be 1"),
    (SMALL, dict(language="auto", num_beams=2), "greedy only: num_beams must be 1"),
    (SMALL, dict(language=["fr", "de", "fr"], return_token_timestamps=True), "the alignment pass takes one shared prefix"),
    (SMALL, dict(language="auto", return_token_timestamps=True), "the alignment pass takes one shared prefix"),
    (SMALL, dict(language=50258), "outside the language tokens"),
]


@pytest.mark.parametrize("dims,kw,msg", REFUSALS, ids=[f"{d.name}-{i}" for i, (d, _, _) in enumerate(REFUSALS)])
def test_refusals(dims, kw, msg):
    with pytest.raises(ValueError, match=msg):
        req(3, dims, **kw)


def test_uniform_language_works_with_beams_and_token_timestamps():
    r = req(3, language=["fr", "French", "<|fr|>"], num_beams=3)
    assert not r.language.per_clip and not r.packed and r.prompt_width == 4
    r = req(3, language="fr", return_token_timestamps=True, prompt_ids=[7, 8])
    assert not r.packed and r.prompt_width == 6
    assert req(3, language="fr", prompt_ids=[[1], [], [2, 3]]).packed   # per-clip prompts: the per-clip route


def test_transcribe_long_refuses_language_with_no_speech_threshold():
    """model.transcribe_long's own refusal, raised before any device work: the check reads only its arguments"""
    import inspect

    from whisper_context_biasing_amd.model import WhisperCB
    src = inspect.getsource(WhisperCB.transcribe_long)
    assert src.index("language with no_speech_threshold is not supported") < src.index("log_mel_long(pcm")
    me = SimpleNamespace(_loaded=True, dims=SMALL)
    with pytest.raises(ValueError, match="language with no_speech_threshold is not supported"):
        WhisperCB.transcribe_long(me, input_features=np.zeros((1, 80, 3000), np.float32), language="fr", no_speech_threshold=0.6)
    with pytest.raises(ValueError, match="need a multilingual model"):
        WhisperCB.transcribe_long(SimpleNamespace(_loaded=True, dims=EN), input_features=np.zeros((1, 80, 3000), np.float32),
                                  language="en")


# -------------------------------------------------------------------------------------------- the invariant
TODAY = dict(B=3, num_beams=1, max_length=448, min_new_tokens=0, bias_boost=0.0, use_graph=True, block=True, temperature=0.0,
             seeds=None, temperatures=None, attempt_seeds=None, logprob_threshold=-1.0, compression_ratio_threshold=2.4,
             prompt=None, per_clip_prompts=False, bias_shared=None, bias_lists=None, rules=None, scored=False, as_dict=False,
             timestamps=False, align=None)


def test_request_without_the_arguments_is_todays_request():
    r = req(3)
    got = {f.name: getattr(r, f.name) for f in fields(DecodeRequest)}
    assert got.pop("language") is None          # the one new field, and it is off
    assert got == TODAY                         # every field the request had before, with the value it had
    assert r.prompt_width == 1 and r.tail_width == 0 and not r.packed
    for kw in (dict(prompt_ids=[5, 6]), dict(prompt_ids=[[5], [], [6, 7]]), dict(return_timestamps=True)):
        a = req(3, **kw)
        assert a.language is None and a.tail_width == 0 and a.packed == a.per_clip_prompts
        assert a.prompt_width == 1 + max((len(p) for p in a.prompt), default=0) if a.per_clip_prompts else 1 + len(a.prompt or ())
    # pack_rows with empty tails is pack_prompts, bit for bit: the per-clip route packs what it packed
    prompts = [[400, 500, 600], [], [7]]
    a, b = P.pack_rows([(p, []) for p in prompts], 50258, 50257), P.pack_prompts(prompts, 50258, 50257)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype


def test_take_and_with_languages():
    r = req(4, language=["fr", "de", "ja", "fr"], task="translate", prompt_ids=[[1], [], [2, 3], [4]])
    s = r.take([2, 0])
    assert s.language.ids.tolist() == [50266, 50265] and s.prompt == [[2, 3], [1]] and s.language.rest == r.language.rest
    a = req(2, language="auto", language_candidates=["fr", "German"])
    assert a.language.auto and a.language.ids is None and a.language.candidates == (50261, 50265) and a.as_dict
    assert [t for _, t in a.clip_rows(50259)] == [[50259, 50358, 50363]] * 2
    g = a.with_languages([50265, 50261])
    assert not g.language.auto and g.language.per_clip and g.language.candidates is None and g.packed
    bits = candidate_bitmap(SMALL, a.language.candidates)
    assert bits.dtype == np.uint32 and bits.tolist() == [(1 << 2) | (1 << 6), 0, 0, 0]
    assert candidate_bitmap(SMALL, None) is None
    assert resolve_language(SMALL, 2) is None


# ------------------------------------------------------------------------------------------------ layout
def test_pack_and_split_with_tails():
    start, pad = 50258, 50257
    prompts = [[400, 500, 600], [], [7]]
    tails = [[50265, 50358, 50363], [50261, 50358, 50363], [50266, 50358, 50363]]
    rows, lens = P.pack_rows(list(zip(prompts, tails)), start, pad)
    assert rows.shape == (3, 7) and lens.tolist() == [7, 4, 5]
    assert rows[1].tolist() == [pad, pad, pad, start, 50261, 50358, 50363]
    assert (rows[:, -4] == start).all() and (rows[:, -3:] == np.asarray(tails)).all()   # the tail: the same last columns
    for b in range(3):
        assert P.split_row(rows[b], int(lens[b]), 3) == (prompts[b], start, tails[b])
    seq = np.concatenate([rows, np.full((3, 5), 11)], axis=1)     # generate()'s `sequences`: generated columns follow
    assert P.split_row(seq[0], 7, 3, width=7) == (prompts[0], start, tails[0])
    with pytest.raises(ValueError, match="one length"):
        P.pack_rows([([], [1]), ([], [1, 2])], start, pad)
    with pytest.raises(ValueError, match="split_row"):
        P.split_row(rows[1], 2, 3)
    # unpack_prompts is left alone: with a tail it still reads lengths as "prompt + start"
    assert P.unpack_prompts(*P.pack_prompts(prompts, start, pad)) == prompts


def test_longform_window_prompt_with_a_tail():
    """Every window's decoder prompt is window_prompt(...) + [start] + tail; the request's width counts the tail, so the
    window's token budget shrinks by it."""
    dims = MICRO
    ts0 = CFG.timestamp_ids(dims)[0]
    prev = window_prompt([[11, 12, ts0 + 5], [13]], condition_on_prev_tokens=True, prev_sot=CFG.start_of_prev_token_id(dims),
                         timestamp_begin=ts0, n_text_ctx=dims.n_text_ctx, prompt_ids=None, prompt_condition_type="first-segment")
    r = resolve(dims, CONFIG, 2, max_length=224, prompt_ids=[[], []], return_timestamps=True, output_logprobs=True,
                language=["fr", "de"], task="translate")
    from dataclasses import replace
    sub = replace(r, prompt=[list(prev), []])
    assert sub.language.rest == (CFG.task_ids(dims)["translate"],)        # long-form decodes with timestamps: no <|notimestamps|>
    rows, lens = P.pack_rows(sub.clip_rows(0), dims.decoder_start_token_id, dims.pad_token_id)
    assert lens.tolist() == [len(prev) + 3, 3] and sub.prompt_width == len(prev) + 3
    assert rows[0].tolist() == list(prev) + [dims.decoder_start_token_id, 50265, 50357]
    assert rows[1, -3:].tolist() == [dims.decoder_start_token_id, 50261, 50357]
    assert sub.max_new(dims.n_text_ctx) == min(224, dims.n_text_ctx - sub.prompt_width)


# ----------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("size,B,detected", [("micro", 6, [83, 83, 37, 83, 83, 83]), ("small", 3, [92, 50, 92])])
def test_fixture_guard(size, B, detected):
    """On the fixture alone: every row's top-2 margin of the language logits is at least 0.05, both cases hold two distinct
    languages, and no row is ever skipped by the tests that read it."""
    g = np.load(os.path.join(GOLDEN, f"lang_{size}_margin_s1.npz"))
    dims = get_dims(size)
    lang_begin, n_lang = CFG.language_ids(dims)
    L = g["lang_logits"]
    assert L.shape == (B, n_lang) and L.dtype == np.float32
    srt = np.sort(L, axis=-1)
    assert ((srt[:, -1] - srt[:, -2]) >= 0.05).all(), srt[:, -1] - srt[:, -2]
    assert (g["detect_ids"] - lang_begin).tolist() == detected == L.argmax(-1).tolist()
    assert len(set(detected)) == 2
    assert g["mixed_sequences"][:, 0].tolist() == [dims.decoder_start_token_id] * B
    assert np.array_equal(g["mixed_sequences"][:, 1], g["mixed_languages"]) and len(set(g["mixed_languages"].tolist())) > 1
    assert (g["mixed_sequences"][:, 2] == CFG.task_ids(dims)["transcribe"]).all()
    assert (g["mixed_sequences"][:, 3] == CFG.timestamp_ids(dims)[1]).all()
