"""GPU: language prompts and per-clip language detection on the chip.

1. wcb_op_lang_head on exact operands (identity A, W = k/8): ids == numpy's argmax over the language range (and over the
   candidates), probs == numpy's float64 softmax to f32 rounding, planted larger logits just outside the range on each
   side, a tie inside it (lowest index), a bitmap that excludes the unrestricted winner; only the tiles' columns written.
2. detect_language against HF's (tests/golden/lang_*.npz, written by tests/golden/make_golden_lang.py): micro f32 and
   small bf16; language_candidates against the golden logits.
3. generate(language=..., task=...) against HF's greedy ids: a mixed-language batch and translate with timestamps.
4. Self-consistency: "auto" == explicit detected languages, bit for bit; clip b of a mixed batch == clip b alone; with
   ragged prompts, per-clip bias lists and timestamps; step-wise; above 64 clips; no new graph captures; long form;
   a uniform language under beam search against oracle/beam_np.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import token_rules_np as R  # noqa: E402
from oracle import whisper_np as W  # noqa: E402
from oracle.beam_np import generate_beam  # noqa: E402
from whisper_context_biasing_amd import _lib  # noqa: E402
from whisper_context_biasing_amd import prompts as P  # noqa: E402
from whisper_context_biasing_amd.config import (LANGUAGE_CODES, get_dims, language_ids, start_of_prev_token_id, task_ids,  # noqa: E402
                                                timestamp_ids)
from whisper_context_biasing_amd.model import WhisperCB  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch, synth_bias_list  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402

DT = {"bf16": (torch.bfloat16, _lib.WCB_BF16), "f16": (torch.float16, _lib.WCB_F16), "f32": (torch.float32, _lib.WCB_F32)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOGPROB_ATOL, LOGPROB_RTOL = 1e-3, 1e-4   # the project's token log-prob tolerance (tests/test_gpu_logprobs.py)
RECIPE, SEED = "margin", 1
_C, _M = {}, {}


def case(size):
    """The fixture, the mel of its clips and the dims, once per size."""
    if size not in _C:
        g = np.load(os.path.join(GOLDEN, f"lang_{size}_{RECIPE}_s{SEED}.npz"))
        dims = get_dims(size)
        B = g["detect_ids"].shape[0]
        mel = W.log_mel(synth_batch(B), dims.n_mel)
        assert abs(mel.sum(dtype=np.float64) - float(g["mel_sum"])) < 2e-5 * mel.size   # the clips the fixture was made from
        srt = np.sort(g["lang_logits"], axis=-1)
        assert ((srt[:, -1] - srt[:, -2]) >= 0.05).all()      # the fixture guard: no row near a tie, none skipped
        _C[size] = dict(g=g, dims=dims, B=B, x=torch.from_numpy(mel), sd=make_weights(dims, seed=SEED, recipe=RECIPE))
    return _C[size]


def model(size, dtype):
    if (size, dtype) not in _M:
        c = case(size)
        _M[size, dtype] = WhisperCB.from_state_dict(c["dims"], c["sd"], dtype=dtype)
    return _M[size, dtype]


def log_softmax64(L):
    L = np.asarray(L, dtype=np.float64)
    mx = L.max(-1, keepdims=True)
    return L - mx - np.log(np.exp(L - mx).sum(-1, keepdims=True))


# ------------------------------------------------------------------------------------------------- 1. the op
V_OP, LANG_BEGIN_OP = 2200, 699       # 699 = 11 mod 16 and 27 mod 32: a tile and a bitmap word straddle the range at both ends
# probs against float64: the planted logits are multiples of 1/8, so v - max is exact; what is left is expf (2 ulp), at
# most 8 merges of (max, sum) partials on any path (one lane-strided push, then 6 butterfly steps, each an expf and an
# fma: 3 ulp) and the division: under 32 ulp of f32, taken as 64
PROB_RTOL = 64 * 2.0 ** -24


def planted_logits(M, n_lang, seed):
    """[M][V] multiples of 1/8 (exact in bf16, f16 and f32): random in [-3, 3] everywhere, per row a larger value right
    before and right after the range, and in the rows m % 3 == 1 a tie of the two largest values inside it"""
    g = np.random.default_rng(seed)
    L = g.integers(-24, 25, size=(M, V_OP)).astype(np.float32) / 8
    lo, hi = LANG_BEGIN_OP, LANG_BEGIN_OP + n_lang
    L[:, lo - 1] = 30.0
    L[:, hi] = 30.0
    L[:, lo - 16:lo - 1] += 8.0       # the rest of the first tile, all above the range's values
    for m in range(M):
        w = int(g.integers(lo, hi))
        L[m, w] = 5.0 + (m % 4) / 8
        if m % 3 == 1:
            t = int(g.integers(lo, hi))
            L[m, t] = L[m, w]          # a tie (or the same column): the lowest index must win
    return L


def lang_head_op(dt, L, K, n_lang, cand=None, probs=True):
    lib = _lib.load()
    M = L.shape[0]
    A = torch.zeros(M, K)
    A[torch.arange(M), torch.arange(M) % K] = 1.0          # row m = e_(m % K): logits[m] = L[m % K] exactly
    Wt = torch.zeros(V_OP, K)
    Wt[:, :min(M, K)] = torch.from_numpy(L[:min(M, K)].T.copy())
    A, Wt = A.to(DT[dt][0]).cuda(), Wt.to(DT[dt][0]).cuda()
    logits = torch.full((M, V_OP + 8), float("nan"), dtype=torch.float32, device="cuda")
    ids = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    pr = torch.full((M, n_lang), float("nan"), dtype=torch.float32, device="cuda") if probs else None
    bits = None
    if cand is not None:
        bits = np.zeros(4, dtype=np.uint32)
        for i in cand:
            bits[i >> 5] |= np.uint32(1 << (i & 31))
    rc = lib.wcb_op_lang_head(DT[dt][1], A.data_ptr(), Wt.data_ptr(), M, V_OP, K, LANG_BEGIN_OP, n_lang,
                              bits.ctypes.data if bits is not None else None, ids.data_ptr(), pr.data_ptr() if probs else None,
                              logits.data_ptr(), V_OP + 8, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.wcb_last_error(None)
    torch.cuda.synchronize()
    return logits.cpu().numpy(), ids.cpu().numpy(), pr.cpu().numpy() if probs else None


@pytest.mark.parametrize("n_lang", [99, 100])
@pytest.mark.parametrize("dt,K", [(dt, K) for dt in ("bf16", "f16", "f32") for K in (64, 32, 1280)])
def test_lang_head_op(dt, K, n_lang):
    lo, hi = LANG_BEGIN_OP, LANG_BEGIN_OP + n_lang
    c0, c1 = lo // 16 * 16, (hi + 15) // 16 * 16
    for M in (1, 3, 17, 64):
        L = planted_logits(M, n_lang, seed=1000 * M + K + n_lang)
        want = L[np.arange(M) % K]                             # the logits of every row
        logits, ids, probs = lang_head_op(dt, L, K, n_lang)
        assert np.array_equal(logits[:, c0:c1], want[:, c0:c1]), (dt, K, M, "logits of the covered tiles are exact")
        out = np.ones(logits.shape[1], bool)
        out[c0:c1] = False
        assert np.isnan(logits[:, out]).all(), "only the tiles that cover the range are written"
        rng = want[:, lo:hi].astype(np.float64)
        assert ((ids >= lo) & (ids < hi)).all(), "a column outside the range was chosen"
        assert np.array_equal(ids, lo + rng.argmax(-1)), (dt, K, M, ids, lo + rng.argmax(-1))   # numpy: lowest index on ties
        ref = np.exp(log_softmax64(rng))
        assert np.isfinite(probs).all() and np.allclose(probs, ref, rtol=PROB_RTOL, atol=0), np.abs(probs / ref - 1).max()
        # candidates: every third language, a bit in each of the four words, without the unrestricted winner of any row
        winners = set((ids - lo).tolist())
        cand = [i for i in range(n_lang) if (i % 3 == 0 or i in (31, 32, 63, 64, 95, 96, n_lang - 1)) and i not in winners]
        logits2, ids2, probs2 = lang_head_op(dt, L, K, n_lang, cand)
        masked = np.full_like(rng, -np.inf)
        masked[:, cand] = rng[:, cand]
        assert np.array_equal(ids2, lo + masked.argmax(-1)) and not (set((ids2 - lo).tolist()) & winners)
        ref2 = np.exp(log_softmax64(masked))
        assert np.allclose(probs2, ref2, rtol=PROB_RTOL, atol=0)
        assert (probs2[:, [i for i in range(n_lang) if i not in cand]] == 0).all()
        assert np.array_equal(logits2[:, c0:c1], logits[:, c0:c1])
        _, ids3, _ = lang_head_op(dt, L, K, n_lang, probs=False)   # out_probs = NULL
        assert np.array_equal(ids3, ids)


# ----------------------------------------------------------------------------------------- 2. detect_language
def forward_lang_logits(m, c):
    """the existing path: wcb_forward_enc's logits for [start], the language columns"""
    lang_begin, n_lang = language_ids(c["dims"])
    enc = m.encode(c["x"])
    start = torch.full((c["B"], 1), c["dims"].decoder_start_token_id, dtype=torch.int32)
    lg = m.forward(encoder_outputs=enc, decoder_input_ids=start).logits[:, 0, lang_begin:lang_begin + n_lang]
    return enc, lg.cpu().numpy()


def test_detect_language_micro_f32():
    c, m = case("micro"), model("micro", "f32")
    g = c["g"]
    ids, probs = m.detect_language(c["x"], return_probs=True)
    assert ids.dtype == torch.int64 and ids.cpu().numpy().tolist() == g["detect_ids"].tolist()
    want = log_softmax64(g["lang_logits"])
    got = np.log(probs.cpu().numpy().astype(np.float64))
    err = np.abs(got - want)
    print(f"detect_language micro f32: max |log p - golden| {err.max():.3e}")
    assert (err <= LOGPROB_ATOL + LOGPROB_RTOL * np.abs(want)).all(), err.max()
    enc, _ = forward_lang_logits(m, c)
    ids2, probs2 = m.detect_language(encoder_outputs=enc, return_probs=True)     # the same bits from the encoder output
    assert torch.equal(ids2, ids) and torch.equal(probs2, probs)
    assert torch.equal(m.detect_language(encoder_outputs=(enc,)), ids)
    for kw in (dict(), dict(input_features=c["x"], encoder_outputs=enc)):
        with pytest.raises(ValueError, match="input_features"):
            m.detect_language(**kw)
    one = m.detect_language(c["x"][2:3], return_probs=True)                     # a clip's result does not depend on its batch
    assert torch.equal(one[0], ids[2:3]) and torch.equal(one[1], probs[2:3])


def test_detect_language_small_bf16():
    """ids equal HF's; log-probs within 2 E of the golden log-softmax, E = the largest error of the EXISTING path's
    language-column logits (wcb_forward_enc for [start]) against the golden logits: a log-softmax at most doubles a bound
    on the logits. Measured on one MI355X: E = 0.1909, the detection's largest error 0.2068."""
    c, m = case("small"), model("small", "bf16")
    g = c["g"]
    _, lg = forward_lang_logits(m, c)
    E = float(np.abs(lg.astype(np.float64) - g["lang_logits"]).max())
    ids, probs = m.detect_language(c["x"], return_probs=True)
    want = log_softmax64(g["lang_logits"])
    err = np.abs(np.log(probs.cpu().numpy().astype(np.float64)) - want)
    print(f"detect_language small bf16: E (forward_enc logits vs golden) {E:.4e}, max |log p - golden| {err.max():.4e}, bound {2 * E:.4e}")
    assert ids.cpu().numpy().tolist() == g["detect_ids"].tolist()
    assert err.max() <= 2 * E, (err.max(), E)


@pytest.mark.parametrize("size,dtype", [("micro", "f32"), ("small", "bf16")])
def test_language_candidates(size, dtype):
    c, m = case(size), model(size, dtype)
    lang_begin, n_lang = language_ids(c["dims"])
    L = c["g"]["lang_logits"].astype(np.float64)
    top = set(L.argmax(-1).tolist())
    cand = [i for i in range(n_lang) if i % 7 == 3 and i not in top] + [0, 31, 32, 64, n_lang - 1]
    cand = sorted(set(cand) - top)                               # the unrestricted winners are no candidates
    masked = np.full_like(L, -np.inf)
    masked[:, cand] = L[:, cand]
    srt = np.sort(masked, axis=-1)
    assert ((srt[:, -1] - srt[:, -2]) >= 0.02).all(), "the candidates' own margin (fixture alone)"
    names = [LANGUAGE_CODES[i] if i % 2 else f"<|{LANGUAGE_CODES[i].upper()}|>" for i in cand]
    ids, probs = m.detect_language(c["x"], language_candidates=names, return_probs=True)
    assert (ids.cpu().numpy() - lang_begin).tolist() == masked.argmax(-1).tolist()
    p = probs.cpu().numpy()
    assert (p[:, [i for i in range(n_lang) if i not in cand]] == 0).all() and abs(p.sum(-1) - 1).max() < 1e-5
    out = m.generate(c["x"], language="auto", language_candidates=names, max_length=4)
    assert torch.equal(out.languages, ids) and torch.equal(out.language_probs, probs)


# ------------------------------------------------------------------------------------- 3. generate against HF
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("size,dtype", [("micro", "f32"), ("small", "bf16")])
def test_generate_matches_hf(size, dtype, use_graph):
    c, m = case(size), model(size, dtype)
    g, dims = c["g"], c["dims"]
    n = g["mixed_sequences"].shape[1] - 4
    langs = [LANGUAGE_CODES[int(t) - language_ids(dims)[0]] for t in g["mixed_languages"]]
    out = m.generate(c["x"], language=langs, task="transcribe", max_length=n, return_dict_in_generate=True, use_graph=use_graph)
    assert np.array_equal(out.sequences.cpu().numpy(), g["mixed_sequences"]), (out.sequences.cpu().numpy(), g["mixed_sequences"])
    assert out.prompt_lengths.tolist() == [4] * c["B"] and out.languages.tolist() == g["mixed_languages"].tolist()
    assert out.language_probs is None
    nt = g["translate_ids"].shape[1]
    tr = m.generate(c["x"], language="French", task="translate", return_timestamps=True, max_length=nt, use_graph=use_graph)
    assert tr.sequences[:, :3].tolist() == [[dims.decoder_start_token_id, 50265, task_ids(dims)["translate"]]] * c["B"]
    assert np.array_equal(tr.sequences[:, 3:].cpu().numpy(), g["translate_ids"]), (tr.sequences[:, 3:].cpu().numpy(), g["translate_ids"])
    assert tr.prompt_lengths is None and tr.languages.tolist() == [50265] * c["B"]   # one language: the flat prefix


# --------------------------------------------------------------------------------------- 4. self-consistency
N_NEW = 12
RAGGED = [[start_of_prev_token_id(get_dims("micro")), 400, 500], [], [7], [], [1, 2, 3, 4, 5, 6, 7, 8, 9], [11]]


def same(a, b):
    assert torch.equal(a.sequences, b.sequences)
    assert (a.token_logprobs is None) == (b.token_logprobs is None)
    if a.token_logprobs is not None:
        assert torch.equal(a.token_logprobs, b.token_logprobs) and torch.equal(a.avg_logprob, b.avg_logprob)
    assert a.segments == b.segments
    assert torch.equal(a.prompt_lengths, b.prompt_lengths) and torch.equal(a.languages, b.languages)


VARIANTS = {
    "plain": dict(),
    "ragged_prompts": dict(prompt_ids=RAGGED),
    "bias_lists": dict(bias_lists=[synth_bias_list(8, seed=b, eot=50257) for b in range(6)], bias_boost=2.0),
    "timestamps": dict(return_timestamps=True),
    "all": dict(prompt_ids=RAGGED, bias_lists=[synth_bias_list(8, seed=b, eot=50257) for b in range(6)], bias_boost=2.0,
                return_timestamps=True),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_auto_equals_explicit_and_clip_alone(name):
    c, m = case("micro"), model("micro", "f32")
    dims, kw = c["dims"], dict(VARIANTS[name], max_length=N_NEW, output_logprobs=True)
    auto = m.generate(c["x"], language="auto", **kw)
    assert auto.languages.tolist() == c["g"]["detect_ids"].tolist() and auto.language_probs.shape == (6, 99)
    given = m.generate(c["x"], language=auto.languages.tolist(), **kw)
    same(auto, given)
    assert given.language_probs is None
    tail = 2 if kw.get("return_timestamps") else 3
    plens = [len(p) + 1 + tail for p in kw.get("prompt_ids", [[]] * 6)]
    assert auto.prompt_lengths.tolist() == plens
    Pmax, seq = max(plens), auto.sequences.cpu().numpy()
    ts0 = timestamp_ids(dims)[0]
    for b in range(6):
        prompt, start, tl = P.split_row(seq[b], plens[b], tail, width=Pmax)
        assert prompt == list(kw.get("prompt_ids", [[]] * 6)[b]) and start == dims.decoder_start_token_id
        assert tl == [int(auto.languages[b]), task_ids(dims)["transcribe"]] + ([] if tail == 2 else [ts0 - 1])
        if kw.get("return_timestamps"):
            assert R.grammar_ok(seq[b, Pmax:], ts0, dims.eos_token_id, dims.pad_token_id)
    # a mixed-language batch: clip b decodes as it decodes alone with its own language (and prompt, and list)
    mixed = [int(t) for t in c["g"]["mixed_languages"]]
    batch = m.generate(c["x"], language=mixed, **kw)
    assert len(set(mixed)) > 1 and batch.languages.tolist() == mixed
    for b in (0, 2, 4):
        solo_kw = dict(kw)
        if "prompt_ids" in kw:
            solo_kw["prompt_ids"] = [kw["prompt_ids"][b]]
        if "bias_lists" in kw:
            solo_kw["bias_lists"] = [kw["bias_lists"][b]]
        solo = m.generate(c["x"][b:b + 1], language=[mixed[b]], **solo_kw)
        n = solo.sequences.shape[1] - plens[b]
        assert torch.equal(solo.sequences[0, -n:], batch.sequences[b, Pmax:Pmax + n]), (name, b)
        # (the ids are equal; the log-probs to the project's tolerance: the prefill of a 1-row and of a 6-row call run in
        # passes of different shapes, §5f's own bound — bit-identity is what "auto" against the given ids has, above)
        lp_s, lp_b = solo.token_logprobs[0, :n].cpu().numpy().astype(np.float64), batch.token_logprobs[b, :n].cpu().numpy()
        assert (np.abs(lp_s - lp_b) <= LOGPROB_ATOL + LOGPROB_RTOL * np.abs(lp_s)).all(), (name, b, np.abs(lp_s - lp_b).max())
        assert (batch.sequences[b, Pmax + n:] == dims.pad_token_id).all()


def test_stepwise_auto_equals_generate():
    c, m = case("micro"), model("micro", "f32")
    kw = dict(prompt_ids=RAGGED, return_timestamps=True)
    ref = m.generate(c["x"], language="auto", max_length=N_NEW, min_new_tokens=N_NEW, output_logprobs=True, **kw)
    dec = m.decode_begin(m.encode(c["x"]), language="auto", min_new_tokens=N_NEW, logprobs=True, **kw)
    try:
        cols = [dec.step()[0].clone() for _ in range(N_NEW)]
        assert torch.equal(dec.languages, ref.languages) and torch.equal(dec.language_probs, ref.language_probs)
        Pmax = int(ref.prompt_lengths.max())
        assert torch.equal(torch.stack(cols, 1).to(torch.int64), ref.sequences[:, Pmax:])
        assert torch.equal(dec.logprobs(), ref.token_logprobs)
    finally:
        dec.close()
    # a uniform language and prompts of one length: the dense step-wise path
    dec = m.decode_begin(m.encode(c["x"]), language="de", task="translate", min_new_tokens=4)
    try:
        cols = torch.stack([dec.step()[0].clone() for _ in range(4)], 1).to(torch.int64)
    finally:
        dec.close()
    flat = m.generate(c["x"], language="de", task="translate", max_length=4, min_new_tokens=4, return_dict_in_generate=True)
    assert torch.equal(cols, flat.sequences[:, 4:]) and dec.languages.tolist() == [50261] * 6


def test_above_64_clips_and_no_new_graphs():
    c, m = case("micro"), model("micro", "f32")
    x70 = m.log_mel(torch.from_numpy(synth_batch(70)).cuda())   # (the device front end: 70 clips)
    kw = dict(language="auto", max_length=6, min_new_tokens=6, output_logprobs=True)
    whole = m.generate(x70, **kw)
    a, b = m.generate(x70[:64], **kw), m.generate(x70[64:], **kw)
    assert torch.equal(whole.sequences, torch.cat([a.sequences, b.sequences]))
    assert torch.equal(whole.token_logprobs, torch.cat([a.token_logprobs, b.token_logprobs]))
    assert torch.equal(whole.languages, torch.cat([a.languages, b.languages]))
    assert torch.equal(whole.language_probs, torch.cat([a.language_probs, b.language_probs]))
    assert len(set(whole.languages.tolist())) > 1
    # other audio, other languages, other candidates: the same graphs
    kw = dict(max_length=6, min_new_tokens=6)
    m.generate(x70[:6], language="auto", **kw)
    m.generate(x70[:6], language=["fr", "de", "fr", "ja", "en", "es"], **kw)
    before = m.debug_counter("graph_captures")
    m.generate(x70[6:12], language="auto", **kw)
    m.generate(x70[12:18], language="auto", language_candidates=["fr", "de", "sv"], **kw)
    m.generate(x70[18:24], language=["zh", "zh", "ko", "it", "it", "pt"], **kw)
    assert m.debug_counter("graph_captures") == before


def test_auto_without_blocking():
    """block=False: device views valid after synchronize() — the generated columns and the int32 detected ids"""
    c, m = case("micro"), model("micro", "f32")
    kw = dict(language="auto", max_length=N_NEW, min_new_tokens=N_NEW)
    ref = m.generate(c["x"], **kw)
    out = m.generate(c["x"], block=False, **kw)
    m.synchronize()
    assert torch.equal(out.sequences.to(torch.int64), ref.sequences[:, 4:])
    assert torch.equal(out.languages.to(torch.int64), ref.languages) and torch.equal(out.language_probs, ref.language_probs)


def test_fallback_detects_once():
    c, m = case("micro"), model("micro", "f32")
    kw = dict(max_length=N_NEW, temperature=(0.0, 0.4), seed=3, logprob_threshold=0.0)   # every clip fails attempt 0
    auto = m.generate(c["x"], language="auto", **kw)
    given = m.generate(c["x"], language=c["g"]["detect_ids"].tolist(), **kw)
    assert auto.languages.tolist() == c["g"]["detect_ids"].tolist() and auto.language_probs.shape == (6, 99)
    assert torch.equal(auto.sequences, given.sequences) and torch.equal(auto.temperatures, given.temperatures)
    assert (auto.temperatures > 0).all()


def test_abi_refusals_on_a_handle():
    c, m = case("micro"), model("micro", "f32")
    lib, dims = m._lib, c["dims"]
    lang_begin, n_lang = language_ids(dims)
    enc = m.encode(c["x"][:2])
    ids = torch.empty(2, dtype=torch.int32, device="cuda")
    for lb, nl, cand in ((dims.eos_token_id, n_lang, None), (dims.vocab - 50, n_lang, None), (lang_begin, 0, None),
                         (lang_begin, n_lang, np.zeros(4, dtype=np.uint32))):
        rc = lib.wcb_detect_language(m._h, enc.data_ptr(), 2, lb, nl, cand.ctypes.data if cand is not None else None,
                                     ids.data_ptr(), None, None)
        assert rc == -1, (lb, nl)
    rows, lens = P.pack_rows([([], [lang_begin, 50358, 50363])] * 2, dims.decoder_start_token_id, dims.pad_token_id)
    lcfg, keep = _lib.lang_cfg(lang_begin, n_lang, None, 2, ids.data_ptr(), None)
    import ctypes as C
    st = C.c_void_p()
    rc = lib.wcb_decode_begin_lang(m._h, enc.data_ptr(), 2, 3, rows.ctypes.data, 4, lens.ctypes.data, C.byref(lcfg), 0.0, 0,
                                   C.byref(st), None)
    assert rc == -4                                                    # num_beams > 1 with a language slot
    lcfg.column_from_end = 3                                           # the slot on the start token
    rc = lib.wcb_decode_begin_lang(m._h, enc.data_ptr(), 2, 1, rows.ctypes.data, 4, lens.ctypes.data, C.byref(lcfg), 0.0, 0,
                                   C.byref(st), None)
    assert rc == -1 and not st.value


# ------------------------------------------------------------------------------------------------ long form
@pytest.mark.parametrize("cond", [False, True], ids=["plain", "condition_on_prev"])
def test_long_form_auto(cond):
    import longform_np as LN
    c, m = case("micro"), model("micro", "f32")
    dims = c["dims"]
    e = LN.e2e_case("margin", 0)
    feats = torch.from_numpy(e["feats"])
    mask = (torch.arange(feats.shape[2])[None] < torch.as_tensor(e["max_frames"])[:, None]).to(torch.int64)
    kw = dict(attention_mask=mask, max_new_tokens=24, condition_on_prev_tokens=cond)
    seen = []
    inner = m._prefix
    m._prefix = lambda req: seen.append(inner(req)) or seen[-1]
    try:
        auto = m.transcribe_long(feats, language="auto", task="translate", **kw)
    finally:
        del m._prefix
    first = m.detect_language(torch.from_numpy(np.stack([LN.cut_window(e["feats"][b], 0, min(int(e["max_frames"][b]), 3000))[0]
                                                         for b in range(3)])))
    assert torch.equal(auto.languages, first) and auto.language_probs.shape == (3, 99)
    given = m.transcribe_long(feats, language=first.tolist(), task="translate", **kw)
    assert torch.equal(auto.sequences, given.sequences) and auto.segments == given.segments and auto.seeks == given.seeks
    assert auto.window_ids == given.window_ids and max(len(s) for s in auto.seeks) > 1
    tr = task_ids(dims)["translate"]
    assert seen
    for packed in seen:            # every window's prompt: ... [start, language of the row's clip, <|translate|>]
        assert (packed.rows[:, -3] == dims.decoder_start_token_id).all() and (packed.rows[:, -1] == tr).all()
        assert set(packed.rows[:, -2].tolist()) <= set(first.tolist())
    if cond:
        assert max(int(p.lengths.max()) for p in seen) > 3   # a later window carries previous tokens before the start token
    with pytest.raises(ValueError, match="no_speech_threshold"):
        m.transcribe_long(feats, language="auto", no_speech_threshold=0.6, **kw)


# -------------------------------------------------------------------------------------------------- beams
def test_uniform_language_beam_search_matches_oracle():
    c, m = case("micro"), model("micro", "f32")
    dims = c["dims"]
    om = W.OracleModel.from_dims(dims, c["sd"])
    x = c["x"][:3]
    prefix = [dims.decoder_start_token_id, 50265, task_ids(dims)["transcribe"], timestamp_ids(dims)[1]]
    ref = generate_beam(om, mel=x.numpy(), num_beams=3, max_length=10, prefix=prefix)
    ids = m.generate(x, language=["fr", "FRENCH", "<|fr|>"], num_beams=3, max_length=10).cpu().numpy()
    assert ids.shape == ref.shape and np.array_equal(ids, ref), (ids, ref)
    out = m.generate(x, language="fr", num_beams=3, max_length=10, return_dict_in_generate=True)
    assert out.sequences[:, :4].tolist() == [prefix] * 3 and out.languages.tolist() == [50265] * 3
