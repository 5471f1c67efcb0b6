"""Model dimensions and special token ids for the Whisper sizes on the hot path.

The reference never defines dimensions itself: it loads them from the hub config of the
checkpoint it evaluates (`scripts/evaluation.py:164`, `models/whisper_medical.py:16-22`).
These tables restate the public OpenAI Whisper configs that `BASELINE.json` names
(tiny.en for C1, small for C2/C4, medium for C3, large-v3 for C5).
Special ids follow SURVEY.md §9.10: `.en` vocab uses eot 50256 / sot 50257, multilingual
uses eot 50257 / sot 50258 — never hard-code them elsewhere.
"""
from __future__ import annotations

from dataclasses import dataclass, asdict, replace
from numbers import Integral

N_AUDIO_CTX = 1500          # encoder positions ([tf] modeling_whisper.py:612-616)
N_SAMPLES = 480000          # 30 s at 16 kHz ([tf] feature_extraction_whisper.py:91)
N_FRAMES = 3000             # mel frames = N_SAMPLES // HOP
N_FFT = 400
HOP = 160
SAMPLE_RATE = 16000
N_TEXT_CTX = 448            # decoder positions (max_target_positions)


@dataclass(frozen=True)
class WhisperDims:
    name: str
    d_model: int
    n_layers: int           # encoder layers == decoder layers for every released size
    n_heads: int
    ffn: int
    vocab: int
    n_mel: int
    eos_token_id: int
    pad_token_id: int
    decoder_start_token_id: int
    n_audio_ctx: int = N_AUDIO_CTX
    n_text_ctx: int = N_TEXT_CTX

    @property
    def head_dim(self) -> int:
        return self.d_model // self.n_heads

    def to_dict(self):
        return asdict(self)

    def hf_config_kwargs(self):
        """Keyword arguments for `transformers.WhisperConfig` describing the same model."""
        return dict(
            vocab_size=self.vocab, num_mel_bins=self.n_mel, d_model=self.d_model,
            encoder_layers=self.n_layers, decoder_layers=self.n_layers,
            encoder_attention_heads=self.n_heads, decoder_attention_heads=self.n_heads,
            encoder_ffn_dim=self.ffn, decoder_ffn_dim=self.ffn,
            max_source_positions=self.n_audio_ctx, max_target_positions=self.n_text_ctx,
            pad_token_id=self.pad_token_id, eos_token_id=self.eos_token_id,
            bos_token_id=self.eos_token_id, decoder_start_token_id=self.decoder_start_token_id,
            activation_function="gelu", scale_embedding=False, use_cache=True,
        )


_EN = dict(eos_token_id=50256, pad_token_id=50256, decoder_start_token_id=50257)
_ML = dict(eos_token_id=50257, pad_token_id=50257, decoder_start_token_id=50258)

MODELS = {
    # micro: the golden-fixture config of SURVEY.md §8(c) recipe (i)
    "micro": WhisperDims("micro", 64, 2, 1, 256, 51865, 80, **_ML),   # head_dim 64 like every release
    "tiny.en": WhisperDims("tiny.en", 384, 4, 6, 1536, 51864, 80, **_EN),
    "tiny": WhisperDims("tiny", 384, 4, 6, 1536, 51865, 80, **_ML),
    "base.en": WhisperDims("base.en", 512, 6, 8, 2048, 51864, 80, **_EN),
    "small": WhisperDims("small", 768, 12, 12, 3072, 51865, 80, **_ML),
    "medium": WhisperDims("medium", 1024, 24, 16, 4096, 51865, 80, **_ML),
    "large-v3": WhisperDims("large-v3", 1280, 32, 20, 5120, 51866, 128, **_ML),
}


def get_dims(name: str, **overrides) -> WhisperDims:
    if name not in MODELS:
        raise KeyError(f"unknown Whisper size {name!r}; known: {sorted(MODELS)}")
    d = MODELS[name]
    return replace(d, **overrides) if overrides else d


def dims_from_hf_config(cfg) -> WhisperDims:
    """Build dims from a `transformers.WhisperConfig`-like object (attribute access)."""
    if cfg.encoder_layers != cfg.decoder_layers:
        raise ValueError("encoder_layers != decoder_layers is not a released Whisper shape")
    return WhisperDims(
        name=getattr(cfg, "name_or_path", "") or "custom", d_model=cfg.d_model,
        n_layers=cfg.encoder_layers, n_heads=cfg.encoder_attention_heads,
        ffn=cfg.encoder_ffn_dim, vocab=cfg.vocab_size, n_mel=cfg.num_mel_bins,
        eos_token_id=cfg.eos_token_id, pad_token_id=cfg.pad_token_id,
        decoder_start_token_id=cfg.decoder_start_token_id,
        n_audio_ctx=cfg.max_source_positions, n_text_ctx=cfg.max_target_positions)


N_TIMESTAMPS = 1501         # <|0.00|> .. <|30.00|> in 0.02 s steps, the last ids of every Whisper vocabulary
TIME_PRECISION = 0.02       # seconds per timestamp step


def timestamp_ids(dims):
    """(timestamp_begin, no_timestamps) of a vocabulary: the 1501 timestamp tokens are its last ids and
    <|notimestamps|> sits right before them (51864: 50363 / 50362, 51865: 50364 / 50363, 51866: 50365 / 50364)."""
    vocab = dims.vocab if hasattr(dims, "vocab") else int(dims)
    timestamp_begin = vocab - N_TIMESTAMPS
    return timestamp_begin, timestamp_begin - 1


def no_speech_token_id(dims) -> int:
    """<|nospeech|> (<|nocaptions|> in the older vocabularies): the id right before <|notimestamps|>, as HF's
    WhisperNoSpeechDetection takes it (51864: 50361, 51865: 50362, 51866: 50363)."""
    return timestamp_ids(dims)[1] - 1


def start_of_prev_token_id(dims) -> int:
    """<|startofprev|>: two ids before <|notimestamps|> (51864: 50360, 51865: 50361, 51866: 50362)."""
    return timestamp_ids(dims)[1] - 2


# Whisper's languages in the order of its tokenizer: <|en|> is decoder_start_token_id + 1, <|zh|> the next id, and so
# on. The last one, yue, exists only in the 51866 vocabulary (large-v3).
LANGUAGES = dict((
    ("en", "english"), ("zh", "chinese"), ("de", "german"), ("es", "spanish"), ("ru", "russian"), ("ko", "korean"),
    ("fr", "french"), ("ja", "japanese"), ("pt", "portuguese"), ("tr", "turkish"), ("pl", "polish"),
    ("ca", "catalan"), ("nl", "dutch"), ("ar", "arabic"), ("sv", "swedish"), ("it", "italian"), ("id", "indonesian"),
    ("hi", "hindi"), ("fi", "finnish"), ("vi", "vietnamese"), ("he", "hebrew"), ("uk", "ukrainian"), ("el", "greek"),
    ("ms", "malay"), ("cs", "czech"), ("ro", "romanian"), ("da", "danish"), ("hu", "hungarian"), ("ta", "tamil"),
    ("no", "norwegian"), ("th", "thai"), ("ur", "urdu"), ("hr", "croatian"), ("bg", "bulgarian"),
    ("lt", "lithuanian"), ("la", "latin"), ("mi", "maori"), ("ml", "malayalam"), ("cy", "welsh"), ("sk", "slovak"),
    ("te", "telugu"), ("fa", "persian"), ("lv", "latvian"), ("bn", "bengali"), ("sr", "serbian"),
    ("az", "azerbaijani"), ("sl", "slovenian"), ("kn", "kannada"), ("et", "estonian"), ("mk", "macedonian"),
    ("br", "breton"), ("eu", "basque"), ("is", "icelandic"), ("hy", "armenian"), ("ne", "nepali"),
    ("mn", "mongolian"), ("bs", "bosnian"), ("kk", "kazakh"), ("sq", "albanian"), ("sw", "swahili"),
    ("gl", "galician"), ("mr", "marathi"), ("pa", "punjabi"), ("si", "sinhala"), ("km", "khmer"), ("sn", "shona"),
    ("yo", "yoruba"), ("so", "somali"), ("af", "afrikaans"), ("oc", "occitan"), ("ka", "georgian"),
    ("be", "belarusian"), ("tg", "tajik"), ("sd", "sindhi"), ("gu", "gujarati"), ("am", "amharic"),
    ("yi", "yiddish"), ("lo", "lao"), ("uz", "uzbek"), ("fo", "faroese"), ("ht", "haitian creole"), ("ps", "pashto"),
    ("tk", "turkmen"), ("nn", "nynorsk"), ("mt", "maltese"), ("sa", "sanskrit"), ("lb", "luxembourgish"),
    ("my", "myanmar"), ("bo", "tibetan"), ("tl", "tagalog"), ("mg", "malagasy"), ("as", "assamese"), ("tt", "tatar"),
    ("haw", "hawaiian"), ("ln", "lingala"), ("ha", "hausa"), ("ba", "bashkir"), ("jw", "javanese"),
    ("su", "sundanese"), ("yue", "cantonese"),
))
LANGUAGE_CODES = tuple(LANGUAGES)
# English name -> code: the names above and the aliases transformers accepts
TO_LANGUAGE_CODE = {**{name: code for code, name in LANGUAGES.items()},
                    "burmese": "my", "valencian": "ca", "flemish": "nl", "haitian": "ht", "letzeburgesch": "lb",
                    "pushto": "ps", "panjabi": "pa", "moldavian": "ro", "moldovan": "ro", "sinhalese": "si",
                    "castilian": "es", "mandarin": "zh"}
TASKS = ("translate", "transcribe")


def is_multilingual(dims) -> bool:
    """A multilingual vocabulary: EOS is 50257 (the English-only ones end at 50256 and have no language tokens)."""
    return dims.eos_token_id == 50257


def language_ids(dims):
    """(lang_begin, n_lang): the language tokens are the n_lang ids from decoder_start_token_id + 1 on, up to the two task
    tokens (99 for vocab 51865, 100 for 51866)."""
    lang_begin = dims.decoder_start_token_id + 1
    return lang_begin, timestamp_ids(dims)[0] - 6 - lang_begin


def task_ids(dims) -> dict:
    """<|translate|> and <|transcribe|>: the ids 7 and 6 before the first timestamp token."""
    ts0 = timestamp_ids(dims)[0]
    return {"translate": ts0 - 7, "transcribe": ts0 - 6}


def language_token_id(dims, language) -> int:
    """The token id of one language given as a code ("fr"), an English name ("french"), a token string ("<|fr|>") —
    case-insensitively, as transformers takes them — or as the token id itself. ValueError for a language Whisper does
    not know and for one this vocabulary has no token for (yue with 99 languages)."""
    lang_begin, n_lang = language_ids(dims)
    if isinstance(language, Integral):
        t = int(language)
        if not lang_begin <= t < lang_begin + n_lang:
            raise ValueError(f"language id {t} outside the language tokens [{lang_begin}, {lang_begin + n_lang})")
        return t
    if not isinstance(language, str):
        raise ValueError(f"language must be a code, a name, a token string or a token id, got {language!r}")
    name = language.lower()
    code = name[2:-2] if name.startswith("<|") and name.endswith("|>") else TO_LANGUAGE_CODE.get(name, name)
    if code not in LANGUAGES:
        raise ValueError(f"Unsupported language: {language}. Language should be one of: {list(LANGUAGES)} or {list(TO_LANGUAGE_CODE)}.")
    i = LANGUAGE_CODES.index(code)
    if i >= n_lang:
        raise ValueError(f"<|{code}|> is not supported by this model: its vocabulary has {n_lang} language tokens")
    return lang_begin + i


def language_code(dims, token_id: int) -> str:
    """The language code of a language token id."""
    lang_begin, n_lang = language_ids(dims)
    if not lang_begin <= int(token_id) < lang_begin + n_lang:
        raise ValueError(f"{token_id} is no language token")
    return LANGUAGE_CODES[int(token_id) - lang_begin]


def parse_segments(ids, timestamp_begin, eos=None):
    """Segments of one row of generated ids decoded with timestamps: a list of (start_s, end_s, token_ids). The
    text between one timestamp token and the next is a segment, time = (token - timestamp_begin) * 0.02 s; of a
    doubled timestamp the second one starts the next segment; a trailing segment without a closing timestamp has
    end_s None. The row ends at its first `eos`."""
    segs, start, toks = [], None, []
    for t in (int(v) for v in ids):
        if eos is not None and t == eos:
            break
        if t >= timestamp_begin:
            sec = round((t - timestamp_begin) * TIME_PRECISION, 2)
            if toks:
                segs.append((start, sec, toks))
                toks = []
            start = sec
        else:
            toks.append(t)
    if toks:
        segs.append((start, None, toks))
    return segs


FRAME_SECONDS = 0.02        # one encoder position (two mel frames of 0.01 s)


def words_from_token_times(ids, times, word_start, eos, audio_end=30.0):
    """Words of one row of generated ids with a time per token (generate(return_token_timestamps=True)): a list of
    (start_s, end_s, token_ids). A word starts at a text token whose `word_start` flag is set, or at the row's first
    text token; ids >= `eos` (EOS, pads, special and timestamp tokens) are skipped; a word ends where the next one
    starts, the last one at `audio_end` (the clip's num_frames * 0.01 s)."""
    words = []
    for t, sec in zip((int(v) for v in ids), times):
        if t >= eos:
            continue
        if not words or word_start[t]:
            words.append([float(sec), None, [t]])
        else:
            words[-1][2].append(t)
    for i, w in enumerate(words):
        w[1] = words[i + 1][0] if i + 1 < len(words) else float(audio_end)
    return [(w[0], w[1], w[2]) for w in words]
