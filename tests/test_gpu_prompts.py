"""GPU: per-clip prompts of different lengths in one greedy batch (wcb_generate_prompted, wcb_decode_begin_prompted,
wcb_op_attention_decode_window; generate(prompt_ids=[[...], ...]), decode_begin(prompt_ids=<ragged list>)).

The oracle is one sentence: clip b of a ragged batch decodes exactly as clip b decoded alone with its own prompt.
tests/test_prompts_host.py shows on the CPU that the numpy restatement of the left-padded layout meets it, that the
tolerances below tell an implementation without the key window or without the shifted positions from a right one
(the log-probs of rows 0-3 then move by 0.036 .. 0.099, the f32 tolerance is 1e-3), and that the bf16 gate's
condition (every oracle margin >= TAU) holds on the reference alone.

Inputs (tests/prompts_np.py): synth_batch(5), prompt tokens [0, 1, 6, 63, 70] -> P = 1, 2, 7, 64, 71 (around the 8-key
lane group and the 64-key chunk of the one-token kernels), 12 new tokens, EOS masked."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import prompts_np as PN  # noqa: E402
from oracle import whisper_np as W  # noqa: E402
from test_gpu_configs import TAU, gated_equal  # noqa: E402
from whisper_context_biasing_amd import _lib  # noqa: E402
from whisper_context_biasing_amd import prompts as P  # noqa: E402
from whisper_context_biasing_amd.config import get_dims  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB, clip_seeds  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch, synth_bias_list  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402

DT = {"bf16": (torch.bfloat16, _lib.WCB_BF16), "f16": (torch.float16, _lib.WCB_F16), "f32": (torch.float32, _lib.WCB_F32)}
N = PN.N_NEW
B = 5
MICRO, TINY = ("micro", "diverse", 0), ("tiny.en", "margin", 1)

# The bf16 log-prob tolerance of test_bf16_matches_solo_oracle: 2 x the largest |log-prob - oracle| the dense solo
# decodes of the same five clips show in bf16 on the commit before this feature (generate(x[b:b+1], prompt_ids=
# prompts[b]) one clip at a time, tiny.en / margin / seed 1, one MI355X). The factor 2 allows for the different
# prefill chunking of a 5-row batch.
BF16_SOLO_ERR_PARENT = 0.04586   # clip 0 (no prompt); the others 0.00698, 0.00002, 0.00032, 0.00249
BF16_LOGPROB_TOL = 2 * BF16_SOLO_ERR_PARENT

_C, _M = {}, {}


def _s():
    return torch.cuda.current_stream().cuda_stream


def case(key):
    """Oracle model, mel, encoder output and the five solo decodes (ids, log-probs, margins), once per model."""
    if key not in _C:
        size, recipe, seed = key
        dims = get_dims(size)
        sd = make_weights(dims, seed=seed, recipe=recipe)
        om = W.OracleModel.from_dims(dims, sd)
        mel = W.log_mel(synth_batch(B), dims.n_mel)
        enc = om.encode(mel)
        prompts = PN.fixed_prompts()
        ids, lps, mg = PN.solo_decodes(om, enc, prompts, margins=True)
        _C[key] = dict(dims=dims, sd=sd, om=om, enc=enc, x=torch.from_numpy(mel), prompts=prompts, ids=ids, lps=lps, mg=mg,
                       rows=P.pack_prompts(prompts, dims.decoder_start_token_id, dims.pad_token_id))
    return _C[key]


def model(key, dtype):
    if (key, dtype) not in _M:
        c = case(key)
        _M[key, dtype] = WhisperCB.from_state_dict(c["dims"], c["sd"], dtype=dtype)
    return _M[key, dtype]


KW = dict(max_length=N, min_new_tokens=N)


# ------------------------------------------------------------------------------------------- 3. the windowed op
def window_op(dt, q, k, v, start, Sq, variant):
    """start None: the dense kernels on the same launch"""
    lib = _lib.load()
    Bq, H, Sk = k.shape[0], k.shape[1], k.shape[2]
    o = torch.full_like(q, float("nan"))
    _lib.check(lib.wcb_op_attention_decode_window(DT[dt][1], q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), Bq, H,
                                                  Sq, Sk, start.data_ptr() if start is not None else None, variant, _s()),
               None, "attention_decode_window")
    torch.cuda.synchronize()
    return o


def window_ref(q, k, v, start, Sq):
    """fp64: the query at slot s = Sk - Sq + i of row b over keys [min(start_b, s), s]."""
    Bq, H, Sk = k.shape[0], k.shape[1], k.shape[2]
    s = q.double().view(Bq, Sq, H, 64).transpose(1, 2) @ k.double().transpose(-1, -2)        # [B, H, Sq, Sk]
    slot = (Sk - Sq + torch.arange(Sq, device=q.device))[None, :, None]
    key = torch.arange(Sk, device=q.device)[None, None, :]
    ok = (key <= slot) & (key >= torch.minimum(start.long()[:, None, None], slot))
    s = s.masked_fill(~ok[:, None], float("-inf"))
    return (torch.softmax(s, -1) @ v.double()).transpose(1, 2).reshape(Bq, Sq, H * 64)


@pytest.mark.parametrize("Sk,Sq", [(Sk, Sq) for Sk in (1, 9, 64, 65, 130) for Sq in (1, 5) if Sq <= Sk])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_windowed_attention_op(dt, Sk, Sq):
    """Every kernel the decode step (6, 7) and the prefill (0-5, also with split-KV chunks: + 100 per chunk) can
    launch, against fp64 at test_decode_attention_variants' tolerance; keys below a row's window hold NaN without
    changing a bit of the output; all starts 0 is the dense kernel bit for bit (key_start = NULL at any Sq, and
    wcb_op_attention_decode at Sq = 1); 7 is 6 bit for bit."""
    lib = _lib.load()
    Bq, H = 6, 2
    g = torch.Generator(device="cpu").manual_seed(1000 * Sq + Sk)
    q = (torch.randn(Bq, Sq, H * 64, generator=g) * 0.3).to(DT[dt][0]).cuda()
    k = torch.randn(Bq, H, Sk, 64, generator=g).to(DT[dt][0]).cuda()
    v = torch.randn(Bq, H, Sk, 64, generator=g).to(DT[dt][0]).cuda()
    start = torch.tensor([0, Sk - 1, min(7, Sk - 1), min(63, Sk - 1), min(64, Sk - 1), Sk // 2], dtype=torch.int32).cuda()
    zero = torch.zeros_like(start)
    ref = window_ref(q, k, v, start, Sq)
    kn, vn = k.clone(), v.clone()
    for b in range(Bq):   # below the lowest window of the row's queries: never read into a result
        dead = min(int(start[b]), Sk - Sq)
        kn[b, :, :dead] = float("nan")
        vn[b, :, :dead] = float("nan")
    tol = 1e-5 if dt == "f32" else 1e-2
    variants = [0, 1, 2, 3, 4, 5, 201, 300, 403] + ([6, 7] if Sq == 1 else [])
    outs = {}
    for var in variants:
        o = window_op(dt, q, k, v, start, Sq, var)
        err = (o.double() - ref).abs().max().item()
        print(f"window op {dt} Sk={Sk} Sq={Sq} variant {var}: err {err:.3e}")
        assert torch.isfinite(o.float()).all() and err < tol, (dt, Sk, Sq, var, err)
        assert torch.equal(window_op(dt, q, kn, vn, start, Sq, var), o), (dt, Sk, Sq, var, "NaN below the window")
        outs[var] = o
        # all starts 0: the dense instantiation of the same launch (the causal prefill, Sq = 5, included), bit for bit
        o0 = window_op(dt, q, k, v, zero, Sq, var)
        assert torch.equal(o0, window_op(dt, q, k, v, None, Sq, var)), (dt, Sk, Sq, var, "starts 0 vs the dense kernel")
        if Sq == 1:   # ... which is wcb_op_attention_decode's
            od = torch.empty_like(o0)
            _lib.check(lib.wcb_op_attention_decode(DT[dt][1], q.data_ptr(), k.data_ptr(), v.data_ptr(), od.data_ptr(), Bq, H,
                                                   Sk, max(var // 100, 1), var % 100, _s()), None, "attention_decode")
            torch.cuda.synchronize()
            assert torch.equal(o0, od), (dt, Sk, var, "starts 0 vs the dense op")
    if Sq == 1:
        assert torch.equal(outs[7], outs[6])


# ----------------------------------------------------------------------------------- 4. end to end, f32, micro
@pytest.mark.parametrize("use_graph", [True, False])
def test_f32_matches_solo_oracle(use_graph):
    c, m = case(MICRO), model(MICRO, "f32")
    out = m.generate(c["x"], prompt_ids=c["prompts"], output_logprobs=True, use_graph=use_graph, **KW)
    rows, lens = c["rows"]
    seq = out.sequences.cpu().numpy()
    assert seq.shape == (B, 71 + N) and np.array_equal(seq[:, :71], rows)
    assert (seq[:, 70] == c["dims"].decoder_start_token_id).all() and (seq[0, :70] == c["dims"].pad_token_id).all()
    assert out.prompt_lengths.cpu().tolist() == lens.tolist() == [1, 2, 7, 64, 71]
    assert P.unpack_prompts(seq, out.prompt_lengths.cpu().numpy()) == c["prompts"]
    assert np.array_equal(seq[:, 71:], c["ids"]), (seq[:, 71:], c["ids"])
    lp = out.token_logprobs.cpu().numpy()
    print(f"f32 ragged vs solo oracle (graph {use_graph}): max |dlogprob| {np.abs(lp - c['lps']).max():.3e}")
    assert lp.shape == (B, N) and lp.dtype == np.float32
    np.testing.assert_allclose(lp, c["lps"], atol=1e-3, rtol=1e-4)   # test_gpu_logprobs.py's, same quantity and oracle


# ----------------------------------------------------------------------------------- 5. end to end, bf16, tiny.en
def test_bf16_matches_solo_oracle():
    """The lean 16-bit kernels. Measured on one MI355X: see BF16_SOLO_ERR_PARENT (the parent commit's dense solo
    decodes) and DESIGN.md §5f for this commit's ragged batch."""
    c, m = case(TINY), model(TINY, "bf16")
    out = m.generate(c["x"], prompt_ids=c["prompts"], output_logprobs=True, **KW)
    ids = out.sequences[:, 71:].cpu().numpy()
    assert gated_equal(ids, c["ids"], c["mg"], tau=TAU, name="tiny.en-bf16-margin-ragged-prompts") == B * N
    err = np.abs(out.token_logprobs.cpu().numpy() - c["lps"]).max()
    print(f"bf16 ragged vs solo oracle: max |dlogprob| {err:.4f} (tolerance {BF16_LOGPROB_TOL:.4f})")
    assert err <= BF16_LOGPROB_TOL, (err, BF16_LOGPROB_TOL)


# ------------------------------------------------------------------------------------------------ 6. step-wise
@pytest.mark.parametrize("temperature", [0.0, 0.7])
def test_stepwise_equals_generate(temperature):
    c, m = case(MICRO), model(MICRO, "f32")
    skw = dict(temperature=temperature, seed=11) if temperature else {}
    out = m.generate(c["x"], prompt_ids=c["prompts"], output_logprobs=True, **KW, **skw)
    dec = m.decode_begin(m.encode(c["x"]), prompt_ids=c["prompts"], min_new_tokens=N, logprobs=True, **skw)
    try:
        toks = torch.stack([dec.step()[0] for _ in range(N)], dim=1)
        lp = dec.logprobs()
        res = dec.result()
    finally:
        dec.close()
    assert torch.equal(toks.to(torch.int64), out.sequences[:, 71:])
    assert torch.equal(res, out.sequences[:, 71:])
    assert torch.equal(lp, out.token_logprobs)   # bitwise
    if not temperature:
        assert np.array_equal(toks.cpu().numpy(), c["ids"])


# ---------------------------------------------------------------------------------------------- 7. composition
def test_per_clip_bias_lists_with_ragged_prompts():
    c, m = case(MICRO), model(MICRO, "f32")
    eot = c["dims"].eos_token_id
    # each clip's list pulls its second token elsewhere: the first token it would emit, then a token of its own
    lists = [synth_bias_list(40, eot=eot, seed=20 + b) + [[int(c["ids"][b, 0]), 1000 + b]] for b in range(B)]
    ids, lps = PN.solo_decodes(c["om"], c["enc"], c["prompts"], bias=lists, bias_boost=2.0)
    assert not np.array_equal(ids, c["ids"])
    out = m.generate(c["x"], prompt_ids=c["prompts"], bias_lists=lists, bias_boost=2.0, output_logprobs=True, **KW)
    assert np.array_equal(out.sequences[:, 71:].cpu().numpy(), ids)
    np.testing.assert_allclose(out.token_logprobs.cpu().numpy(), lps, atol=1e-3, rtol=1e-4)
    shared = m.generate(c["x"], prompt_ids=c["prompts"], bias_list=lists[2], bias_boost=2.0, **KW).cpu().numpy()
    assert np.array_equal(shared[2], ids[2])   # the shared automaton: clip 2 sees the list it saw alone


@pytest.mark.parametrize("rules", ["suppress", "timestamps"])
def test_token_rules_in_a_ragged_batch_equal_the_dense_solo_decodes(rules):
    c, m = case(MICRO), model(MICRO, "f32")
    if rules == "suppress":
        kw = dict(suppress_tokens=sorted({int(t) for t in c["ids"][:, :3].ravel()}), begin_suppress_tokens=[int(c["ids"][4, 3])])
    else:
        kw = dict(return_timestamps=True, max_initial_timestamp=1.0)
    out = m.generate(c["x"], prompt_ids=c["prompts"], return_dict_in_generate=True, **KW, **kw)
    got = out.sequences[:, 71:].cpu().numpy()
    assert rules != "suppress" or not np.array_equal(got, c["ids"])
    for b in range(B):
        solo = m.generate(c["x"][b:b + 1], prompt_ids=c["prompts"][b], return_dict_in_generate=True, **KW, **kw)
        assert np.array_equal(solo.sequences[0, len(c["prompts"][b]) + 1:].cpu().numpy(), got[b]), b
        if rules == "timestamps":
            assert solo.segments[0] == out.segments[b]


def test_temperature_fallback_redecodes_with_the_clips_own_prompt():
    c, m = case(MICRO), model(MICRO, "f32")
    avg = c["lps"].mean(axis=1)
    thr = float(np.sort(avg)[2] - 1e-3)          # the two clips with the lowest greedy avg_logprob fail (f32: 1e-3 clear)
    fail = [b for b in range(B) if avg[b] < thr]
    assert len(fail) == 2 and np.abs(avg - thr).min() > 5e-4
    out = m.generate(c["x"], prompt_ids=c["prompts"], temperature=(0.0, 0.7), seed=3, logprob_threshold=thr,
                     compression_ratio_threshold=None, **KW)
    seq, temps = out.sequences.cpu().numpy(), out.temperatures.cpu().numpy()
    assert seq.shape == (B, 71 + N) and np.array_equal(seq[:, :71], c["rows"][0])
    assert out.prompt_lengths.cpu().tolist() == [1, 2, 7, 64, 71]
    for b in range(B):
        if b not in fail:
            assert temps[b] == 0.0 and np.array_equal(seq[b, 71:], c["ids"][b])
            continue
        assert np.isclose(temps[b], 0.7)
        solo = m.generate(c["x"][b:b + 1], prompt_ids=c["prompts"][b], temperature=0.7, output_logprobs=True,
                          seed=[int(clip_seeds(3, 0, B, attempt=1)[b])], **KW)
        assert np.array_equal(solo.sequences[0, len(c["prompts"][b]) + 1:].cpu().numpy(), seq[b, 71:]), b


def test_async_and_split_batches():
    """block=False keeps the caller's arrays out of the decode (they are garbage when it runs); more than 64 clips
    split into sub-batches with prompt widths of their own, joined at the batch's."""
    c, m = case(MICRO), model(MICRO, "f32")
    xd = c["x"].to(m.device)
    outs = []
    for i in range(3):
        prompts = [list(p) for p in c["prompts"]]
        outs.append(m.generate(xd, prompt_ids=prompts, block=False, **KW))
        for p in prompts:
            p[:] = [1] * len(p)
    m.synchronize()
    for o in outs:
        assert np.array_equal(o.cpu().numpy(), c["ids"])
    # 66 clips: the long prompts in the first sub-batch only, so the second is 7 wide and re-padded to 71
    reps = 14
    x = xd.repeat(reps, 1, 1)[:66]
    order = [3, 4, 0, 1, 2]
    prompts = [c["prompts"][order[i % B]] if i < 64 else c["prompts"][i % 3] for i in range(66)]
    clip = [i % B for i in range(66)]
    want = {}
    for i in range(66):   # the few (clip, prompt) pairs off the diagonal: the dense solo path
        pi = c["prompts"].index(prompts[i])
        if (clip[i], pi) not in want:
            want[clip[i], pi] = (c["ids"][pi] if clip[i] == pi else m.generate(
                xd[clip[i]:clip[i] + 1], prompt_ids=prompts[i], **KW).cpu().numpy()[0])
    out = m.generate(x, prompt_ids=prompts, return_dict_in_generate=True, **KW)
    seq = out.sequences.cpu().numpy()
    assert seq.shape == (66, 71 + N) and out.prompt_lengths.cpu().tolist() == [len(p) + 1 for p in prompts]
    assert P.unpack_prompts(seq, out.prompt_lengths.cpu().numpy()) == prompts
    for i in range(66):
        assert np.array_equal(seq[i, 71:], want[clip[i], c["prompts"].index(prompts[i])]), i


# ---------------------------------------------------------------------------------------------- 8. graph reuse
def test_length_vectors_share_one_graph():
    c, m = case(MICRO), model(MICRO, "f32")
    rev = c["prompts"][::-1]                                  # lengths 71, 64, 7, 2, 1: same B and Pmax
    ids_rev, _ = PN.solo_decodes(c["om"], c["enc"], rev)
    for _ in range(2):                                        # both decode contexts hold the ragged graph
        a = m.generate(c["x"], prompt_ids=c["prompts"], **KW).cpu().numpy()
    n0 = m.debug_counter("graph_captures")
    for _ in range(2):
        r = m.generate(c["x"], prompt_ids=rev, **KW).cpu().numpy()
        assert np.array_equal(r, ids_rev)
    assert m.debug_counter("graph_captures") == n0
    assert np.array_equal(a, c["ids"])
    assert np.array_equal(m.generate(c["x"], prompt_ids=c["prompts"], **KW).cpu().numpy(), c["ids"])
    assert m.debug_counter("graph_captures") == n0


# --------------------------------------------------------------------------------- 9. equal-length fallthrough
def test_equal_lengths_are_the_dense_path():
    c, m = case(MICRO), model(MICRO, "f32")
    p = c["prompts"][2]
    same = [[t + b for t in p] for b in range(B)]             # one length, different tokens per clip
    enc = m.encode(c["x"])
    runs = []
    for form in (same, np.asarray(same, dtype=np.int32)):     # the nested list, and today's [B, P] array
        dec = m.decode_begin(enc, prompt_ids=form, min_new_tokens=N, logprobs=True)
        try:
            toks = torch.stack([dec.step()[0] for _ in range(N)], dim=1)
            runs.append((toks, dec.logprobs()))
        finally:
            dec.close()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    g = m.generate(c["x"], prompt_ids=same, output_logprobs=True, **KW)
    assert g.sequences.shape == (B, 7 + N) and g.prompt_lengths.cpu().tolist() == [7] * B
    assert torch.equal(g.sequences[:, 7:], runs[1][0].to(torch.int64)) and torch.equal(g.token_logprobs, runs[1][1])
    one = m.generate(c["x"], prompt_ids=[p] * B, output_logprobs=True, **KW)      # nested, the same prompt for all
    flat = m.generate(c["x"], prompt_ids=p, output_logprobs=True, **KW)           # the shared row of wcb_generate
    assert torch.equal(one.sequences, flat.sequences) and torch.equal(one.token_logprobs, flat.token_logprobs)


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals():
    c, m = case(MICRO), model(MICRO, "f32")
    with pytest.raises(ValueError):
        m.generate(c["x"], prompt_ids=c["prompts"], num_beams=2, **KW)
    with pytest.raises(ValueError):
        m.generate(c["x"], prompt_ids=c["prompts"], return_token_timestamps=True, **KW)
    with pytest.raises(ValueError):
        m.generate(c["x"], prompt_ids=c["prompts"][:3], **KW)
    with pytest.raises(ValueError):
        m.decode_begin(m.encode(c["x"]), prompt_ids=c["prompts"], num_beams=2)
    lib = _lib.load()
    xd = c["x"].to(m.device).contiguous()
    rows, lens = c["rows"]
    out = torch.empty(B, N, dtype=torch.int32, device=m.device)
    steps = C.c_int32(0)

    def call(num_beams, lens_, max_new=N):
        cfg = _lib.WcbGenCfg(max_new, max_new, num_beams, 0.0, 1, 0)
        ln = np.ascontiguousarray(lens_, dtype=np.int32)
        return lib.wcb_generate_prompted(m._h, xd.data_ptr(), B, C.byref(cfg), None, None, None, rows.ctypes.data, 71,
                                         ln.ctypes.data, out.data_ptr(), None, C.byref(steps), _s())

    assert call(2, lens) == -4                                 # WCB_ERR_UNSUPPORTED
    assert call(1, [0, 2, 7, 64, 71]) == -1                    # WCB_ERR_ARG
    assert call(1, [1, 2, 7, 64, 72]) == -1
    assert call(1, lens, max_new=c["dims"].n_text_ctx - 71 + 2) == -1   # the length rule of prefix_len
    assert call(1, lens) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), c["ids"])
