"""GPU: repetition penalty and no-repeat n-grams on the chip in the greedy decoder.

1. wcb_op_lm_head_repeat — the LM head with the per-row seen bitmap plus the history pass of the finalize on caller
   operands: planted rows with exact logits (tests/repeat_np.py planted_case: ids equal the restatement, no row
   excluded) in f32 / bf16 / f16, and random operands against the float64 restatement, where only rows whose
   top-two score gap lies inside the logit error may be skipped (at most 10 %).
2. End to end: f32 micro against repeat_steps on the oracle (graph and eager, three rule pairs, log-probs raw, ids
   differ from the unruled decode); bf16 tiny.en with no_repeat_ngram_size=2 through the margin gate of
   test_gpu_configs.py (tau = 0.05) with no token skipped.
3. Composition with bias lists, ragged prompts, deny lists, the step-wise API, block=False and the split above 64
   clips; graph reuse across (p, n); the refused combinations (Python and the ABI's codes, wcb_generate_windows and
   transcribe_long among them); language="auto": the detected token is part of the history."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import repeat_np as RP  # noqa: E402
from oracle import whisper_np as W  # noqa: E402
from whisper_context_biasing_amd import _lib  # noqa: E402
from whisper_context_biasing_amd.config import get_dims  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch, synth_bias_list  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402

DT = {"bf16": (torch.bfloat16, _lib.WCB_BF16), "f16": (torch.float16, _lib.WCB_F16), "f32": (torch.float32, _lib.WCB_F32)}
TAU = 0.05   # tests/test_gpu_configs.py's margin gate (bf16 logits against the f32 reference)


# ------------------------------------------------------------------------------------------------ 1. the kernels
def lm_head_repeat(dt, A, Wt, p, n, hists, walkers=256, eos=RP.OP["eos"]):
    lib = _lib.load()
    M, K = A.shape
    V = Wt.shape[0]
    logits = torch.empty(M, V, device="cuda", dtype=torch.float32)
    nxt = torch.full((M,), -7, device="cuda", dtype=torch.int32)
    ld = max(len(h) for h in hists)
    hist = np.zeros((M, ld), dtype=np.int32)
    for m, h in enumerate(hists):
        hist[m, :len(h)] = h
    lens = np.asarray([len(h) for h in hists], dtype=np.int32)
    r = _lib.WcbRepeatRules(p, n)
    rc = lib.wcb_op_lm_head_repeat(DT[dt][1], A.data_ptr(), Wt.data_ptr(), M, V, K, walkers, C.byref(r), eos,
                                   hist.ctypes.data, ld, lens.ctypes.data, logits.data_ptr(), V, nxt.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    if rc < 0:
        return rc, None, None
    torch.cuda.synchronize()
    return rc, logits.cpu().numpy(), nxt.cpu().numpy()


def exact_operands(dt, L, K):
    """A = identity rows [M][K], W[v][m] = L[m][v]: logits[m][v] = L[m][v] exactly (every value k/8, |k| < 256)"""
    M, V = L.shape
    A = torch.zeros(M, K)
    A[torch.arange(M), torch.arange(M)] = 1.0
    Wt = torch.zeros(V, K)
    Wt[:, :M] = torch.from_numpy(L.T.copy())
    return A.to(DT[dt][0]).cuda(), Wt.to(DT[dt][0]).cuda()


@pytest.mark.parametrize("K", [64, 32])          # 64: the column walk; 32: the skinny 64-column epilogue
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_planted_rows(dt, K):
    c = RP.OP
    for p, n in RP.PLANTED_CALLS:
        L, hists, expect = RP.planted_case(p, n)
        A, Wt = exact_operands(dt, L, K)
        for walkers in (128, 256):
            rc, logits, nxt = lm_head_repeat(dt, A, Wt, p, n, hists, walkers)
            assert rc == 0
            assert np.array_equal(logits, L), (dt, p, n, "logits are exact")
            want = [RP.choose(logits[m], hists[m], p, n, c["eos"])[0] for m in range(c["M"])]
            assert np.array_equal(want, expect)
            assert np.array_equal(nxt, want), (dt, K, p, n, walkers, nxt.tolist(), want)
    # three rows at a time: one 16-row block with most of it empty
    L, hists, expect = RP.planted_case(2.0, 3)
    A, Wt = exact_operands(dt, L[4:7], K)
    rc, _, nxt = lm_head_repeat(dt, A, Wt, 2.0, 3, hists[4:7])
    assert rc == 0 and np.array_equal(nxt, expect[4:7])


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_random_rows(dt):
    """ids against the float64 restatement on float64 logits. A row may be skipped only when its top-two score gap
    is within twice the score error: the logit bound tests/test_gpu_kernels.py holds a decode-row GEMM with f32
    output to (1e-4·|ref| + 2e-4, at the row's largest |logit|) times max(p, 1/p)."""
    c = RP.OP
    rows = skipped = 0
    for call in range(RP.RANDOM_CASE["calls"]):
        A, Wt, hists, (p, n) = RP.random_case(call, DT[dt][0])
        ref, ids, ok = RP.random_expectation(A, Wt, hists, p, n)
        rc, logits, nxt = lm_head_repeat(dt, A.cuda(), Wt.cuda(), p, n, hists)
        assert rc == 0
        assert (np.abs(logits - ref) <= RP.logit_tol(ref)).all()
        for m in range(c["M"]):
            rows += 1
            if not ok[m]:
                skipped += 1
                continue
            assert nxt[m] == ids[m], (dt, call, m, p, n, hists[m], int(nxt[m]), int(ids[m]))
    print(f"random rows {dt}: {rows} rows, {skipped} inside the logit error")
    assert skipped <= 0.10 * rows


def test_op_argument_errors():
    A, Wt = exact_operands("f32", np.zeros((2, 32), np.float32), 64)
    assert lm_head_repeat("f32", A, Wt, 0.0, 0, [[1], [2]])[0] == -1
    assert lm_head_repeat("f32", A, Wt, 1.2, -1, [[1], [2]])[0] == -1
    assert lm_head_repeat("f32", A, Wt, 1.2, 2, [[1], [32]])[0] == -1    # an id outside the vocabulary
    assert lm_head_repeat("f32", A, Wt, 1.2, 2, [[1], []])[0] == -1     # an empty history is not a decoder row


# ------------------------------------------------------------------------------------- 2. end to end
B5, N = 5, 16
PAIRS = [(1.3, 0), (1.0, 2), (1.3, 3)]
_CASE = {}


def case():
    if not _CASE:
        dims = get_dims("micro")
        sd = make_weights(dims, seed=0, recipe="diverse")
        om = W.OracleModel.from_dims(dims, sd)
        mel = W.log_mel(synth_batch(B5), dims.n_mel)
        enc = om.encode(mel)
        m = WhisperCB.from_state_dict(dims, sd, dtype="f32")
        x = torch.from_numpy(mel)
        plain = m.generate(x, max_length=N, min_new_tokens=N).cpu().numpy()
        assert np.array_equal(plain, om.generate(mel, enc=enc, max_length=N, min_new_tokens=N, trim=False))
        _CASE.update(dims=dims, om=om, mel=mel, enc=enc, m=m, x=x, plain=plain, ref={})
    return _CASE


def oracle_rows(c, p, n, B=B5, n_tok=N, lists=None, lam=0.0, prompts=None, suppress=()):
    """repeat_steps free-running on every clip: (ids [B, n_tok], steps per clip); computed once per argument set"""
    key = (p, n, B, n_tok, repr(lists), lam, repr(prompts), tuple(suppress))
    if key not in c["ref"]:
        steps = [RP.repeat_steps(c["om"], c["enc"][b:b + 1], p, n, lists[b] if lists else None, lam, n_tok=n_tok,
                                 min_new=n_tok, prompt=prompts[b] if prompts else (), suppress=suppress) for b in range(B)]
        c["ref"][key] = (np.asarray([[s[0] for s in st] for st in steps]), steps)
    return c["ref"][key]


def logsumexp(row):
    row = np.asarray(row, dtype=np.float64)
    return float(row.max() + np.log(np.exp(row - row.max()).sum()))


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("p,n", PAIRS)
def test_generate_f32_equals_the_oracle(p, n, use_graph):
    c = case()
    ref, steps = oracle_rows(c, p, n)
    out = c["m"].generate(c["x"], max_length=N, min_new_tokens=N, repetition_penalty=p, no_repeat_ngram_size=n,
                          output_logprobs=True, use_graph=use_graph)
    ids = out.sequences[:, 1:].cpu().numpy()
    assert np.array_equal(ids, ref), (p, n, ids, ref)
    assert not np.array_equal(ids, c["plain"]), "the rules change the decode"
    lp = out.token_logprobs.cpu().numpy()
    want = np.asarray([[float(row[tok]) - logsumexp(row) for tok, _, _, row in st] for st in steps])
    np.testing.assert_allclose(lp, want, atol=1e-3, rtol=1e-4)   # test_gpu_logprobs.py's f32 tolerance: raw log-probs
    if n:
        for b in range(B5):   # no n-gram repeats in prompt + generated
            h = [c["dims"].decoder_start_token_id] + ids[b].tolist()
            grams = [tuple(h[i:i + n]) for i in range(len(h) - n + 1)]
            assert len(grams) == len(set(grams)), (b, h)


def test_generate_bf16_ngram_matches_the_oracle_through_the_margin_gate():
    """tiny.en / margin / seed 1, 3 clips, 24 tokens, no_repeat_ngram_size=2: every token checked (the oracle's
    smallest top-two margin per clip stays above tau). The penalty is not pinned end to end in bf16: on this model
    p >= 2 leaves oracle margins below tau; its 16-bit check is test_planted_rows / test_random_rows."""
    dims = get_dims("tiny.en")
    sd = make_weights(dims, seed=1, recipe="margin")
    om = W.OracleModel.from_dims(dims, sd)
    mel = W.log_mel(synth_batch(3), dims.n_mel)
    enc = om.encode(mel)
    steps = [RP.repeat_steps(om, enc[b:b + 1], 1.0, 2, n_tok=24, min_new=24) for b in range(3)]
    ref = np.asarray([[s[0] for s in st] for st in steps])
    margin = np.asarray([[s[2] for s in st] for st in steps])
    print("smallest oracle margins:", margin.min(axis=1))
    assert (margin >= TAU).all(), margin.min(axis=1)   # no token is skipped
    m = WhisperCB.from_state_dict(dims, sd, dtype="bf16")
    x = torch.from_numpy(mel)
    ids = m.generate(x, max_length=24, min_new_tokens=24, no_repeat_ngram_size=2).cpu().numpy()
    assert np.array_equal(ids, ref), (ids, ref)
    assert not np.array_equal(ids, m.generate(x, max_length=24, min_new_tokens=24).cpu().numpy())


# ------------------------------------------------------------------------------------- 3. composition
B3 = 3
P, NG = 1.3, 3


def bias_lists(c):
    eot, plain = c["dims"].eos_token_id, c["plain"]
    shared = synth_bias_list(200, eot=eot) + [list(map(int, plain[0, 2:5])), list(map(int, plain[1, 1:3])) + [7, 8]]
    lists = [synth_bias_list(200, eot=eot, seed=7) + [list(map(int, plain[0, 2:5]))],
             synth_bias_list(200, eot=eot, seed=8) + [list(map(int, plain[1, 1:3])) + [7, 8]], []]
    return shared, lists


@pytest.mark.parametrize("bias", ["shared", "per_clip"])
def test_with_bias_lists(bias):
    c = case()
    shared, lists = bias_lists(c)
    kw = dict(bias_list=shared) if bias == "shared" else dict(bias_lists=lists)
    per = [shared] * B3 if bias == "shared" else lists
    ref, _ = oracle_rows(c, P, NG, B=B3, lists=per, lam=2.0)
    for use_graph in (True, False):
        ids = c["m"].generate(c["x"][:B3], max_length=N, min_new_tokens=N, repetition_penalty=P, no_repeat_ngram_size=NG,
                              bias_boost=2.0, use_graph=use_graph, **kw).cpu().numpy()
        assert np.array_equal(ids, ref), (bias, use_graph, ids, ref)
    unboosted, _ = oracle_rows(c, P, NG)
    assert not np.array_equal(ref, unboosted[:B3])


def test_ragged_prompts_equal_the_solo_decodes():
    """a clip decodes as it decodes alone: its own prompt tokens are part of the history, the dead left-padding
    slots of the batch are not"""
    c, m = case(), case()["m"]
    plain = c["plain"]
    # clip 0: no prompt; clip 1: a prompt holding the tokens it would generate first; clip 2: a long prompt
    prompts = [[], [int(t) for t in plain[1, :4]], [int(t) for t in np.random.RandomState(2).randint(300, 20000, 70)] + [int(plain[2, 0])]]
    kw = dict(max_length=N, min_new_tokens=N, repetition_penalty=P, no_repeat_ngram_size=2)
    got = m.generate(c["x"][:B3], prompt_ids=prompts, **kw).cpu().numpy()
    ref, _ = oracle_rows(c, P, 2, B=B3, prompts=prompts)
    for b in range(B3):
        solo = m.generate(c["x"][b:b + 1], prompt_ids=prompts[b], **kw).cpu().numpy()[0]
        assert np.array_equal(got[b], solo), b
    assert np.array_equal(got, ref), (got, ref)
    noprompt, _ = oracle_rows(c, P, 2)
    free = m.generate(c["x"][:B3], prompt_ids=prompts, max_length=N, min_new_tokens=N).cpu().numpy()
    assert not np.array_equal(got[1], free[1])   # the prompt's tokens are penalised / complete banned n-grams
    assert np.array_equal(got[0], noprompt[0])   # the clip without a prompt: its padding is not history


def test_with_suppress_tokens_and_stepwise_and_async():
    c, m = case(), case()["m"]
    x = c["x"][:B3]
    ruled, _ = oracle_rows(c, P, NG)
    deny = sorted({int(t) for t in ruled[:B3, :2].ravel()})
    ref, _ = oracle_rows(c, P, NG, B=B3, suppress=deny)
    kw = dict(repetition_penalty=P, no_repeat_ngram_size=NG, suppress_tokens=deny)
    ids = m.generate(x, max_length=N, min_new_tokens=N, **kw).cpu().numpy()
    assert np.array_equal(ids, ref) and not set(deny) & set(ids.ravel().tolist())
    # step-wise: the same decode, one token per call, bit for bit
    dec = m.decode_begin(m.encode(x), min_new_tokens=N, logprobs=True, **kw)
    step_ids = torch.stack([dec.step()[0] for _ in range(N)], 1).cpu().numpy()
    assert _lib.load().wcb_set_repeat_rules(m._h, None) == -2   # fixed while a step-wise decode is open
    lp = dec.logprobs().cpu().numpy()
    dec.close()
    assert np.array_equal(step_ids, ids)
    out = m.generate(x, max_length=N, min_new_tokens=N, output_logprobs=True, **kw)
    assert np.array_equal(out.token_logprobs.cpu().numpy(), lp)
    # block=False: valid after synchronize()
    xd = x.to(m.device)
    outs = [m.generate(xd, max_length=N, min_new_tokens=N, block=False, **kw) for _ in range(3)]
    m.synchronize()
    for o in outs:
        assert np.array_equal(o.cpu().numpy(), ids)


def test_split_above_64_clips():
    c, m = case(), case()["m"]
    ref, _ = oracle_rows(c, P, NG)
    x = c["x"].to(m.device).repeat(14, 1, 1)[:66]
    ids = m.generate(x, max_length=N, min_new_tokens=N, repetition_penalty=P, no_repeat_ngram_size=NG).cpu().numpy()
    assert ids.shape == (66, N)
    for i in range(66):
        assert np.array_equal(ids[i], ref[i % B5]), i


# ------------------------------------------------------------------------------------- 4. graphs; refusals
def test_values_share_one_graph_and_rules_off_is_the_old_decode():
    c, m = case(), case()["m"]
    kw = dict(max_length=N, min_new_tokens=N)
    want = {pn: oracle_rows(c, *pn)[0] for pn in PAIRS}
    for _ in range(2):   # both kinds captured in both decode contexts (calls alternate between the two)
        m.generate(c["x"], repetition_penalty=1.3, **kw)
        m.generate(c["x"], **kw)
    n0 = m.debug_counter("graph_captures")
    for p, n in PAIRS + PAIRS[::-1] + PAIRS:
        got = m.generate(c["x"], repetition_penalty=p, no_repeat_ngram_size=n, **kw).cpu().numpy()
        assert np.array_equal(got, want[p, n]), (p, n)
        assert np.array_equal(m.generate(c["x"], **kw).cpu().numpy(), c["plain"])   # off after on: today's ids
    assert m.debug_counter("graph_captures") == n0


def test_refused_combinations():
    c, m = case(), case()["m"]
    x = c["x"][:B3]
    for rep in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2)):
        for kw in (dict(num_beams=2), dict(temperature=0.5), dict(temperature=(0.0, 0.5)), dict(do_sample=True),
                   dict(return_timestamps=True)):
            with pytest.raises(ValueError):
                m.generate(x, max_length=4, **rep, **kw)
        with pytest.raises(ValueError):
            m.decode_begin(m.encode(x), num_beams=2, **rep)
        with pytest.raises(ValueError):
            m.decode_begin(m.encode(x), temperature=0.7, **rep)
    with pytest.raises(ValueError):
        m.generate(x, max_length=4, repetition_penalty=0.0)
    # transcribe_long decodes with the timestamp grammar: refused through the generation config as well
    m.generation_config.repetition_penalty = 1.3
    try:
        with pytest.raises(ValueError):
            m.transcribe_long(torch.zeros(1, c["dims"].n_mel, 6000))
    finally:
        del m.generation_config.repetition_penalty
    # the ABI's own codes; the handle state goes in and out through the model, as generate() installs it
    from whisper_context_biasing_amd import request as RQ
    from whisper_context_biasing_amd.model import _WindowBatch
    from whisper_context_biasing_amd.prompts import pack_prompts
    lib = _lib.load()
    for p, n in ((0.0, 0), (float("nan"), 0), (1.2, -1)):
        assert lib.wcb_set_repeat_rules(m._h, C.byref(_lib.WcbRepeatRules(p, n))) == -1
    m._install_rules(RQ.NO_TOKEN_RULES + ((1.2, 2),))
    out = torch.empty(B3, 4, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    steps = C.c_int32(0)
    beams = _lib.WcbGenCfg(4, 0, 2, 0.0, 1, 0)
    cfg = _lib.WcbGenCfg(4, 0, 1, 0.0, 1, 0)

    def greedy(g):
        return lib.wcb_generate(m._h, xg.data_ptr(), B3, C.byref(g), None, None, 1, out.data_ptr(), C.byref(steps), None)
    assert greedy(beams) == -4
    seeds = np.arange(B3, dtype=np.uint64)
    smp = _lib.WcbSampleCfg(1.0, seeds.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert lib.wcb_generate_sampled(m._h, xg.data_ptr(), B3, C.byref(cfg), C.byref(smp), None, None, None, 1,
                                    out.data_ptr(), None, C.byref(steps), None) == -4
    rows_p, lens_p = pack_prompts([[]] * B3, c["dims"].decoder_start_token_id, c["dims"].pad_token_id)
    w, keep = _WindowBatch(xg, 3000, list(range(B3)), [0] * B3, [3000] * B3).abi()
    lp = torch.zeros(B3, 4, dtype=torch.float32, device="cuda")
    assert lib.wcb_generate_windows(m._h, C.byref(w), B3, C.byref(cfg), None, None, rows_p.ctypes.data, 1, lens_p.ctypes.data,
                                    out.data_ptr(), lp.data_ptr(), None, C.byref(steps), None) == -4
    del keep
    assert greedy(cfg) == 0
    m._install_rules(RQ.rules_key(c["dims"], True) + ((1.2, 2),))   # the timestamp grammar beside the repeat rules
    assert greedy(cfg) == -4
    m._install_rules(None)
    assert greedy(cfg) == 0
    assert np.array_equal(m.generate(c["x"], max_length=N, min_new_tokens=N).cpu().numpy(), c["plain"])


def test_detected_language_is_part_of_the_history():
    """language="auto": the token the device patches into the prompt rows is in hist — the bitmap is built after the
    patch. Every clip's own language token is boosted far above everything else, so the unruled decode emits it first;
    with no_repeat_ngram_size=1 (every seen token banned) it is never emitted. The candidates exclude <|en|>, the
    placeholder the prompt rows hold before the patch."""
    c, m = case(), case()["m"]
    x = c["x"][:B3]
    kw = dict(language="auto", language_candidates=["fr", "de", "es"], max_length=8, min_new_tokens=8)
    langs = m.generate(x, **kw).languages.cpu().numpy().tolist()
    lists = [[[int(t)]] for t in langs]
    for use_graph in (True, False):
        free = m.generate(x, bias_lists=lists, bias_boost=50.0, use_graph=use_graph, **kw)
        n = free.sequences.shape[1] - 8
        assert free.sequences[:, n].cpu().numpy().tolist() == langs, "the boosted language token wins the unruled first step"
        out = m.generate(x, bias_lists=lists, bias_boost=50.0, no_repeat_ngram_size=1, use_graph=use_graph, **kw)
        assert out.languages.cpu().numpy().tolist() == langs
        gen = out.sequences[:, n:].cpu().numpy()
        for b in range(B3):
            assert langs[b] not in gen[b], (b, langs[b], gen[b])
            assert len(set(gen[b].tolist())) == 8   # n = 1: no token twice
