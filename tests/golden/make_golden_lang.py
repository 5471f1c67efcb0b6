"""Generate the language fixtures by running the REFERENCE stack itself (survey container only), as make_golden.py and
make_golden_longform.py do: the reference's model class with the seeded weights, HF's `detect_language` and HF's
`generate(language=..., task=...)`. Data only is stored (inputs are regenerated from seeds):

  lang_<size>_margin_s1.npz
    detect_ids        [B]          HF detect_language token ids
    lang_logits       [B, n_lang]  the f32 logits of the language tokens after [start] (what detect_language reduces)
    mixed_languages   [B]          the language token id given to every clip of the mixed-language batch
    mixed_sequences   [B, 4 + n]   HF generate(language=[...per clip...], task="transcribe") greedy, prompt included
    mixed_step_margin [B, n]       the top-2 margin of every step of that decode (processed scores)
    translate_ids     [B, n]       HF generate(language="fr", task="translate", return_timestamps=True): the generated
                                   ids alone (HF strips the prompt there)
    top2_margin       [B]          lang_logits' top-2 margin per clip (the tests guard it on the fixture alone)

Cases: micro f32-weights 6 clips; small (bf16-rounded weights) 3 clips; recipe margin, seed 1; synth_batch clips.

Run:  python tests/golden/make_golden_lang.py [micro] [small]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden import ref_model  # noqa: E402
from whisper_context_biasing_amd.config import (LANGUAGE_CODES, get_dims, is_multilingual, language_ids, task_ids,  # noqa: E402
                                                timestamp_ids)
from whisper_context_biasing_amd.synth import synth_batch  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402

CASES = {"micro": dict(B=6, n_new=12, mixed=["fr", "de", "en", "ja", "fr", "es"]),
         "small": dict(B=3, n_new=8, mixed=["fr", "de", "ja"])}
RECIPE, SEED = "margin", 1


def generation_config(dims, n_new):
    from transformers import GenerationConfig
    lang_begin, n_lang = language_ids(dims)
    gc = GenerationConfig(max_new_tokens=n_new, pad_token_id=dims.pad_token_id, eos_token_id=dims.eos_token_id,
                          decoder_start_token_id=dims.decoder_start_token_id, use_cache=True)
    gc.lang_to_id = {f"<|{LANGUAGE_CODES[i]}|>": lang_begin + i for i in range(n_lang)}
    gc.task_to_id = task_ids(dims)
    gc.is_multilingual = is_multilingual(dims)
    gc.no_timestamps_token_id = timestamp_ids(dims)[1]
    return gc


def fixture(size):
    from transformers import WhisperFeatureExtractor
    c = CASES[size]
    dims = get_dims(size)
    sd = make_weights(dims, seed=SEED, recipe=RECIPE)
    fe = WhisperFeatureExtractor(feature_size=dims.n_mel)
    mel = np.stack([fe(p, sampling_rate=16000).input_features[0] for p in synth_batch(c["B"])]).astype(np.float32)
    m = ref_model(dims, sd)
    m.config.suppress_tokens = None
    m.config.begin_suppress_tokens = None
    m.config.forced_decoder_ids = None
    lang_begin, n_lang = language_ids(dims)
    x = torch.from_numpy(mel)
    out = {"mel_sum": mel.sum(dtype=np.float64)}
    with torch.no_grad():
        gc = generation_config(dims, c["n_new"])
        m.generation_config = gc
        out["detect_ids"] = m.detect_language(input_features=x, generation_config=gc).numpy().astype(np.int64)
        start = torch.full((c["B"], 1), dims.decoder_start_token_id, dtype=torch.long)
        logits = m(input_features=x, decoder_input_ids=start, use_cache=False).logits[:, -1].float().numpy()
        out["lang_logits"] = logits[:, lang_begin:lang_begin + n_lang].astype(np.float32)
        assert np.array_equal(out["detect_ids"], lang_begin + out["lang_logits"].argmax(-1))
        srt = np.sort(out["lang_logits"], axis=-1)
        out["top2_margin"] = (srt[:, -1] - srt[:, -2]).astype(np.float32)
        out["mixed_languages"] = np.asarray([gc.lang_to_id[f"<|{l}|>"] for l in c["mixed"]], dtype=np.int64)
        g = m.generate(input_features=x, generation_config=generation_config(dims, c["n_new"]), language=list(c["mixed"]),
                       task="transcribe", return_dict_in_generate=True, output_scores=True)
        out["mixed_sequences"] = g.sequences.numpy().astype(np.int64)
        sc = np.sort(torch.stack(g.scores, 1).float().numpy(), axis=-1)
        out["mixed_step_margin"] = (sc[..., -1] - sc[..., -2]).astype(np.float32)
        t = m.generate(input_features=x, generation_config=generation_config(dims, c["n_new"]), language="fr", task="translate",
                       return_timestamps=True, return_dict_in_generate=True)
        out["translate_ids"] = (t["sequences"] if isinstance(t, dict) else t.sequences).numpy().astype(np.int64)
    out["meta"] = np.array([str(dict(size=size, recipe=RECIPE, seed=SEED, B=c["B"], n_new=c["n_new"], mixed=c["mixed"]))])
    print(size, "detect", (out["detect_ids"] - lang_begin).tolist(), "margins", np.round(out["top2_margin"], 3).tolist())
    print(size, "mixed", out["mixed_sequences"].tolist(), "min step margin", float(out["mixed_step_margin"].min()))
    print(size, "translate", out["translate_ids"].tolist())
    assert float(out["top2_margin"].min()) >= 0.05, "change the seed: a language row is near a tie"
    np.savez_compressed(os.path.join(HERE, f"lang_{size}_{RECIPE}_s{SEED}.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for size in (sys.argv[1:] or list(CASES)):
        fixture(size)
