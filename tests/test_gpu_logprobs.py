"""GPU: token log-probabilities and sequence scores (wcb_generate_scored, wcb_decode_enable_logprobs /
wcb_decode_logprobs, wcb_op_lm_head_lse; generate(output_logprobs=True), decode_begin(logprobs=True)).

logprob[b][t] = logit[b][t][tok] − logsumexp(logit[b][t][:]) over the step's RAW f32 logits: the bias boost and
the EOS mask pick the token and never enter it; a finished row's pad columns hold exactly 0. Beam search returns
the best hypothesis's score (HF sequences_scores). Scoring never changes an id.

The lse bound. The LM head keeps per (row, workgroup) online-softmax partials and the selection kernel merges
them; against the float64 logsumexp of the very logits the op returned the error is a few f32 roundings of a
number of lse's magnitude, so it is held in units of the f32 spacing at lse. Measured on an MI355X over every
case of test_lm_head_lse_op (M 3 / 17, K 64 / 384, V 649 / 51865, 128 / 256 / 1024 walkers, three dtypes, flat /
rising / falling logits: 216 op calls, plus 54 at the skinny kernel's K = 32): see LSE_ERR_ULPS_MEASURED; the bound is
4x that, 9.12 spacings. For flat logits at V = 51865 (lse = ln V = 10.86, spacing 9.5e-7) the bound must stay
below 1e-5, half the shift one vocabulary column causes there — it is 8.7e-6, asserted in the test itself.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import whisper_np as W  # noqa: E402
from oracle.beam_np import generate_beam  # noqa: E402
from whisper_context_biasing_amd import _lib  # noqa: E402
from whisper_context_biasing_amd.config import get_dims  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch, synth_bias_list  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402

DT = {"bf16": (torch.bfloat16, _lib.WCB_BF16), "f16": (torch.float16, _lib.WCB_F16), "f32": (torch.float32, _lib.WCB_F32)}

# max |lse − lse64| / spacing(lse64) measured over the cases of test_lm_head_lse_op; the tests hold 4x that.
# Measured (all three dtypes alike): flat logits 2.28 spacings at V = 649 (1.1e-6 at lse = 6.5) and 1.73 at
# V = 51865 (1.65e-6 at lse = 10.86), the same for 128 / 256 / 1024 walkers — one logf and one add of the f32
# result, not the merge order; rising / falling logits 0.62 spacings (4.7e-6 at |lse| = 90 .. 99).
LSE_ERR_ULPS_MEASURED = 2.28
LSE_BOUND_ULPS = 4 * LSE_ERR_ULPS_MEASURED


def lse_bound(lse64):
    """The bound on |lse − lse64| at that value: LSE_BOUND_ULPS spacings of f32 there."""
    return LSE_BOUND_ULPS * np.spacing(np.abs(np.asarray(lse64, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def logsumexp64(rows):
    rows = np.asarray(rows, dtype=np.float64)
    mx = rows.max(axis=-1, keepdims=True)
    return (mx + np.log(np.exp(rows - mx).sum(axis=-1, keepdims=True)))[..., 0]


def logprob_tol(logit, lse64):
    """|(logit − lse) computed in f32 − the float64 value|: the lse bound plus the rounding of the subtraction."""
    big = np.maximum(np.abs(logit), np.abs(lse64)).astype(np.float32)
    return lse_bound(lse64) + np.spacing(big).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. the kernel
def lm_head_lse(dt, A, Wt, walkers):
    lib = _lib.load()
    M, K = A.shape
    V = Wt.shape[0]
    logits = torch.empty(M, V, device="cuda", dtype=torch.float32)
    lse = torch.empty(M, device="cuda", dtype=torch.float32)
    am = torch.empty(M, device="cuda", dtype=torch.int32)
    _lib.check(lib.wcb_op_lm_head_lse(DT[dt][1], A.data_ptr(), Wt.data_ptr(), M, V, K, walkers, logits.data_ptr(), V,
                                      lse.data_ptr(), am.data_ptr(), torch.cuda.current_stream().cuda_stream),
               None, "wcb_op_lm_head_lse")
    torch.cuda.synchronize()
    return logits.cpu().numpy(), lse.cpu().numpy(), am.cpu().numpy()


def lm_head_inputs(dt, kind, M, K, V):
    """A [M][K], W [V][K] in dtype. flat: logits within ~1e-3 of each other (every column counts equally);
    rising / falling: logit ≈ a ramp over the column index from −90 to +90 (or back) times 0.9 .. 1.1 per row, so
    the running maximum moves at every tile and Σ exp(logit) overflows f32 without the max subtracted."""
    g = torch.Generator(device="cpu").manual_seed(1000 * M + K + V % 97)
    if kind == "flat":
        A = torch.randn(M, K, generator=g)
        Wt = torch.randn(V, K, generator=g) * (1e-3 / K)
    else:
        u = torch.full((K,), 1.0 / K ** 0.5)
        ramp = torch.linspace(-90.0, 90.0, V)
        if kind == "falling":
            ramp = ramp.flip(0)
        A = torch.linspace(0.9, 1.1, M)[:, None] * u[None] + torch.randn(M, K, generator=g) * (0.01 / K ** 0.5)
        Wt = ramp[:, None] * u[None] + torch.randn(V, K, generator=g) * (0.05 / K ** 0.5)
    return A.to(DT[dt][0]).cuda(), Wt.to(DT[dt][0]).cuda()


def lm_head_case(dt, kind, M, K, V, walkers):
    """One op call checked for logits and argmax; returns (|lse − lse64|, lse64) per row."""
    A, Wt = lm_head_inputs(dt, kind, M, K, V)
    logits, lse, am = lm_head_lse(dt, A, Wt, walkers)
    a64, w64 = A.double().cpu().numpy(), Wt.double().cpu().numpy()
    ref = a64 @ w64.T
    scale = np.abs(a64) @ np.abs(w64).T + 1.0
    err = (np.abs(logits - ref) / scale).max()   # test_gpu_kernels.test_gemm_matches_fp64's bound
    assert err < 1e-5, (dt, kind, M, K, V, walkers, err)
    assert np.array_equal(am, logits.argmax(axis=1)), (dt, kind, M, K, V, walkers)
    lse64 = logsumexp64(logits)
    return np.abs(lse.astype(np.float64) - lse64), lse64


LM_HEAD_SHAPES = [(K, V) for K in (64, 384) for V in (649, 51865)] + [(32, 649)]   # K = 32: the skinny kernel


@pytest.mark.parametrize("K,V", LM_HEAD_SHAPES)
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_lm_head_lse_op(dt, K, V):
    for kind in ("flat", "rising", "falling"):
        for M in (3, 17):
            for walkers in (128, 256, 1024):
                err, lse64 = lm_head_case(dt, kind, M, K, V, walkers)
                print(f"lse {dt} {kind} M={M} K={K} V={V} walkers={walkers}: err {err.max():.3e} "
                      f"ulps {(err / np.spacing(np.abs(lse64).astype(np.float32))).max():.2f}")
                bound = lse_bound(lse64)
                if kind == "flat" and V == 51865:
                    assert bound.max() < 1e-5, bound.max()   # half of one column's shift, 1 / V = 1.9e-5
                assert (err <= bound).all(), (dt, kind, M, K, V, walkers, err.max(), bound.min())


# ------------------------------------------------------------------------------------- shared end-to-end fixtures
B = 3
_CASE, _MODELS, _WEIGHTS, _MEL = {}, {}, {}, {}


def weights(size):
    if size not in _WEIGHTS:
        _WEIGHTS[size] = make_weights(get_dims(size), seed=0, recipe="diverse")
    return _WEIGHTS[size]


def model(dtype="f32", size="micro", **options):
    key = (dtype, size, tuple(sorted(options.items())))
    if key not in _MODELS:
        _MODELS[key] = WhisperCB.from_state_dict(get_dims(size), weights(size), dtype=dtype, options=options or None)
    return _MODELS[key]


def mel_batch(n):
    """[n, 80, 3000] f32 on the device (the library's own front end; every size here has 80 mel bins)"""
    if n not in _MEL:
        _MEL[n] = model("f32").log_mel(torch.from_numpy(synth_batch(n)))
    return _MEL[n]


def case():
    if not _CASE:
        dims = get_dims("micro")
        om = W.OracleModel.from_dims(dims, weights("micro"))
        mel = W.log_mel(synth_batch(B), dims.n_mel)
        enc = om.encode(mel)
        plain = om.generate(mel, enc=enc, max_length=16, min_new_tokens=16)
        eot = dims.eos_token_id
        shared = synth_bias_list(200, eot=eot) + [list(map(int, plain[0, 2:5])), list(map(int, plain[1, 1:3])) + [7, 8]]
        lists = [synth_bias_list(200, eot=eot, seed=7) + [list(map(int, plain[0, 2:5]))],
                 synth_bias_list(200, eot=eot, seed=8) + [list(map(int, plain[1, 1:3])) + [7, 8]],
                 []]
        _CASE.update(dims=dims, om=om, mel=mel, enc=enc, plain=plain, shared=shared, lists=lists, x=torch.from_numpy(mel),
                     ref={})
    return _CASE


def oracle_logprobs(lists, lam, n, min_new, prefix=None):
    """(ids [B, w], logprobs [B, w] float64): the oracle's greedy decode of every clip alone with its own list
    (one list for all = the shared automaton's result), float64 log-softmax of its raw logits at the ids it chose,
    0 at the pads of a finished row. Computed once per configuration."""
    c = case()
    key = (tuple(tuple(map(tuple, L)) for L in lists), lam, n, min_new, tuple(prefix or ()))
    if key not in c["ref"]:
        rows = []
        for b in range(B):
            ids, logits = c["om"].generate(c["mel"][b:b + 1], enc=c["enc"][b:b + 1], max_length=n, min_new_tokens=min_new,
                                           bias=lists[b], bias_boost=lam, return_logits=True, trim=False, prefix=prefix)
            lp = np.take_along_axis(logits[0].astype(np.float64), ids[0][:, None], axis=1)[:, 0] - logsumexp64(logits[0])
            assert np.abs(logits).max() < 4.0   # (micro: the magnitude the walkers comparison relies on)
            rows.append((ids[0], lp))
        w = max(len(i) for i, _ in rows)
        pad = c["dims"].pad_token_id
        ids = np.full((B, w), pad, dtype=np.int64)
        lps = np.zeros((B, w), dtype=np.float64)
        for b, (i, lp) in enumerate(rows):
            ids[b, :len(i)], lps[b, :len(i)] = i, lp
            eos = np.flatnonzero(i == c["dims"].eos_token_id)
            if len(eos):
                lps[b, eos[0] + 1:] = 0.0
        c["ref"][key] = (ids, lps)
    return c["ref"][key]


# --------------------------------------------------------------------------------- 2. greedy against the oracle
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("bias", ["none", "shared", "per_clip"])
def test_greedy_logprobs_match_oracle_f32(bias, use_graph):
    c = case()
    m = model("f32")
    kw = dict(max_length=16, min_new_tokens=16, use_graph=use_graph, output_logprobs=True)
    if bias == "none":
        out, lists, lam = m.generate(c["x"], bias_list=c["shared"], bias_boost=0.0, **kw), [[]] * B, 0.0
    elif bias == "shared":
        out, lists, lam = m.generate(c["x"], bias_list=c["shared"], bias_boost=2.0, **kw), [c["shared"]] * B, 2.0
    else:
        out, lists, lam = m.generate(c["x"], bias_lists=c["lists"], bias_boost=2.0, **kw), c["lists"], 2.0
    ids, lps = oracle_logprobs(lists, lam, 16, 16)
    got = out.sequences[:, 1:].cpu().numpy()
    assert np.array_equal(got, ids), (got, ids)
    lp = out.token_logprobs.cpu().numpy()
    assert lp.shape == ids.shape and lp.dtype == np.float32
    # twice the 5e-4 logit tolerance held against the reference goldens: the chosen logit's error + the largest one's
    np.testing.assert_allclose(lp, lps, atol=1e-3, rtol=1e-4)
    np.testing.assert_allclose(out.avg_logprob.cpu().numpy(), lp.astype(np.float64).mean(axis=1), rtol=1e-6, atol=1e-7)
    assert out.sequences_scores is None
    if bias != "none":   # the boost moved tokens, and a moved token shows as a lower model log-prob
        plain_ids, plain_lps = oracle_logprobs([[]] * B, 0.0, 16, 16)
        assert not np.array_equal(ids, plain_ids)


def test_async_calls_and_prompts_carry_their_logprobs():
    """block=False with more calls in flight than decode contexts: every call's log-probs are its own (the
    buffer is per decode context and copied out with the ids); a prompt shifts nothing: the log-probs stay
    aligned with the generated columns."""
    c = case()
    m = model("f32")
    xd = c["x"].to(m.device)
    kw = dict(max_length=16, min_new_tokens=16, bias_lists=c["lists"], bias_boost=2.0, output_logprobs=True)
    ref = m.generate(xd, **kw)
    plain = m.generate(xd, max_length=16, min_new_tokens=16, output_logprobs=True)
    outs = [m.generate(xd, block=False, **(kw if i % 2 == 0 else dict(kw, bias_boost=0.0))) for i in range(4)]
    m.synchronize()
    for i, o in enumerate(outs):
        want = ref if i % 2 == 0 else plain
        assert torch.equal(o.sequences.to(torch.int64), want.sequences[:, 1:]), i
        assert torch.equal(o.token_logprobs, want.token_logprobs), i
    prompt = [400, 500, 600]
    out = m.generate(xd, prompt_ids=prompt, **kw)
    ids, lps = oracle_logprobs(c["lists"], 2.0, 16, 16, prefix=prompt + [c["dims"].decoder_start_token_id])
    assert np.array_equal(out.sequences[:, :4].cpu().numpy(), np.tile(prompt + [c["dims"].decoder_start_token_id], (B, 1)))
    assert np.array_equal(out.sequences[:, 4:].cpu().numpy(), ids)
    np.testing.assert_allclose(out.token_logprobs.cpu().numpy(), lps, atol=1e-3, rtol=1e-4)


# ------------------------------------------------------------------------------------------------ 3. early finish
def test_early_finish_pads_hold_zero():
    c = case()
    dims, plain = c["dims"], c["plain"]
    eos = dims.eos_token_id
    lists = [[[int(plain[0, 2]), eos]], [], [[int(plain[2, 5]), eos]]]
    m = model("f32")
    out = m.generate(c["x"], bias_lists=lists, bias_boost=8.0, max_length=16, output_logprobs=True)
    ids, lps = oracle_logprobs(lists, 8.0, 16, 0)
    assert [list(ids[b]).index(eos) + 1 if eos in ids[b] else None for b in range(B)] == [2, None, 2], ids
    got = out.sequences[:, 1:].cpu().numpy()
    assert np.array_equal(got, ids), (got, ids)
    lp = out.token_logprobs.cpu().numpy()
    np.testing.assert_allclose(lp, lps, atol=1e-3, rtol=1e-4)
    for b in (0, 2):
        assert lp[b, 1] < 0 and lps[b, 1] < 0          # the EOS the row emitted carries its real log-prob
        assert (lp[b, 2:] == 0.0).all()                # exactly 0 at every pad column
    avg = out.avg_logprob.cpu().numpy()
    for b in (0, 2):
        np.testing.assert_allclose(avg[b], lp[b, :2].astype(np.float64).mean(), rtol=1e-6)
    np.testing.assert_allclose(avg[1], lp[1].astype(np.float64).mean(), rtol=1e-6)


# --------------------------------------------------------------------------------------- 4. bit-identity, graphs
@pytest.mark.parametrize("size", ["micro", "tiny"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_scoring_changes_no_id_and_replays_its_graph(dtype, size):
    c = case()
    m = model(dtype, size)
    others = [model(dtype, size, lm_walkers=w) for w in (128, 1024)]
    for nclip in (3, 17):
        x = mel_batch(nclip)
        for lam in (0.0, 2.0):
            kw = dict(max_length=16, min_new_tokens=16, bias_list=c["shared"], bias_boost=lam)
            before = m.generate(x, return_dict_in_generate=True, **kw).sequences
            for _ in range(2):   # one capture per decode context
                scored = m.generate(x, output_logprobs=True, **kw)
            assert torch.equal(scored.sequences, before), (dtype, size, nclip, lam)
            captures = m.debug_counter("graph_captures")
            for _ in range(2):
                again = m.generate(x, output_logprobs=True, **kw)
            assert m.debug_counter("graph_captures") == captures
            assert torch.equal(again.sequences, before) and torch.equal(again.token_logprobs, scored.token_logprobs)
            after = m.generate(x, return_dict_in_generate=True, **kw).sequences
            assert torch.equal(after, before)
            lp = scored.token_logprobs.cpu().numpy().astype(np.float64)
            assert np.isfinite(lp).all() and (lp <= 0).all()
            for o in others:   # another partial count: the same ids, the log-probs within twice the bound
                so = o.generate(x, output_logprobs=True, **kw)
                assert torch.equal(so.sequences, before), (dtype, size, nclip, lam)
                lpo = so.token_logprobs.cpu().numpy().astype(np.float64)
                # (the logits do not depend on the walkers, so the difference is the two lse errors and the two
                # subtractions' roundings; |lse| <= |log-prob| + |logit| and these random-weight models' logits stay
                # below 4 — the step-wise test reads and asserts it — so the spacing is taken at |log-prob| + 4)
                mag = np.abs(lp) + 4.0
                tol = 2 * (lse_bound(mag) + np.spacing(mag.astype(np.float32)).astype(np.float64))
                assert (np.abs(lpo - lp) <= tol).all(), (dtype, size, nclip, lam, np.abs(lpo - lp).max())


# ------------------------------------------------------------------------------- 5. 16-bit: the step's own logits
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_stepwise_logprobs_match_the_steps_logits(dtype):
    m = model(dtype, "tiny")
    lib = _lib.load()
    x = mel_batch(B)
    V = m.dims.vocab
    ld = (V + 127) // 128 * 128
    dec = m.decode_begin(m.encode(x), min_new_tokens=6, logprobs=True)
    try:
        want, tol = [], []
        buf = torch.empty(B, ld, dtype=torch.float32, device=m.device)
        for t in range(6):
            ids, _ = dec.step()
            _lib.check(lib.wcb_debug_copy(m._h, b"step_logits", buf.data_ptr(), buf.numel() * 4, -1), m._h, "wcb_debug_copy")
            logits = buf[:, :V].cpu().numpy()
            print(f"step {t} {dtype}: max |logit| {np.abs(logits).max():.2f}")
            assert np.abs(logits).max() < 4.0   # (the magnitude the walkers comparison above relies on)
            tok = ids.cpu().numpy().astype(np.int64)
            masked = logits.copy()
            masked[:, m.dims.eos_token_id] = -np.inf   # (min_new_tokens: EOS cannot be chosen — it still counts in lse)
            assert np.array_equal(tok, masked.argmax(axis=1))
            lse64 = logsumexp64(logits)
            chosen = logits[np.arange(B), tok]
            want.append(chosen.astype(np.float64) - lse64)
            tol.append(logprob_tol(chosen, lse64))
        lp = dec.logprobs().cpu().numpy()
        assert lp.shape == (B, 6)
        err = np.abs(lp.astype(np.float64) - np.stack(want, axis=1))
        assert (err <= np.stack(tol, axis=1)).all(), (err.max(), np.stack(tol, axis=1).min())
        small = torch.empty(B, 5, dtype=torch.float32, device=m.device)
        n = C.c_int32(0)
        rc = lib.wcb_decode_logprobs(m._h, dec._st, small.data_ptr(), 5, C.byref(n), torch.cuda.current_stream().cuda_stream)
        assert rc == -1   # WCB_ERR_ARG: 6 steps do not fit 5 columns
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------------ 6. beams
@pytest.mark.parametrize("per_clip", [False, True])
def test_beam_sequences_scores_match_oracle_f32(per_clip):
    c = case()
    m = model("f32")
    kw = dict(max_length=10, min_new_tokens=10, num_beams=3)
    if per_clip:
        out = m.generate(c["x"], bias_lists=c["lists"], bias_boost=2.0, output_logprobs=True, **kw)
        refs = [generate_beam(c["om"], enc=c["enc"][b:b + 1], bias=c["lists"][b], bias_boost=2.0, return_scores=True, **kw)
                for b in range(B)]
    else:
        out = m.generate(c["x"], output_logprobs=True, **kw)
        refs = [generate_beam(c["om"], enc=c["enc"][b:b + 1], return_scores=True, **kw) for b in range(B)]
    got = out.sequences[:, 1:].cpu().numpy()
    for b, (ids, sc) in enumerate(refs):
        w = ids.shape[1]
        assert np.array_equal(got[b, :w], ids[0]) and (got[b, w:] == c["dims"].pad_token_id).all(), (b, got, ids)
    ref_sc = np.asarray([float(sc[0]) for _, sc in refs])
    assert out.token_logprobs is None and out.avg_logprob is None
    np.testing.assert_allclose(out.sequences_scores.cpu().numpy(), ref_sc, atol=1e-3, rtol=0)


def test_wrong_score_pointer_for_the_mode_is_unsupported():
    c = case()
    m = model("f32")
    lib = _lib.load()
    x = c["x"].to(m.device).contiguous()
    ids = torch.empty(B, 10, dtype=torch.int32, device=m.device)
    buf = torch.zeros(B, 10, dtype=torch.float32, device=m.device)
    steps = C.c_int32(0)
    stream = torch.cuda.current_stream().cuda_stream
    for beams, lp, ss in ((3, buf, None), (1, None, buf)):
        cfg = _lib.WcbGenCfg(10, 10, beams, 0.0, 1, 0)
        rc = lib.wcb_generate_scored(m._h, x.data_ptr(), B, C.byref(cfg), None, None, None, 1, ids.data_ptr(),
                                     lp.data_ptr() if lp is not None else None, ss.data_ptr() if ss is not None else None,
                                     C.byref(steps), stream)
        assert rc == -4, (beams, rc)   # WCB_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------- 7. split path
def test_more_than_64_clips_split_and_join():
    m = model("f32")
    x = mel_batch(70)
    kw = dict(max_length=6, output_logprobs=True)
    whole = m.generate(x, **kw)
    a, b = m.generate(x[:64], **kw), m.generate(x[64:], **kw)
    assert whole.token_logprobs.shape[0] == 70 and whole.avg_logprob.shape == (70,)
    w = whole.token_logprobs.shape[1]
    assert w == max(a.token_logprobs.shape[1], b.token_logprobs.shape[1])
    parts = torch.cat([torch.nn.functional.pad(t.token_logprobs, (0, w - t.token_logprobs.shape[1])) for t in (a, b)])
    assert torch.equal(whole.token_logprobs, parts)
    assert torch.equal(whole.avg_logprob, torch.cat([a.avg_logprob, b.avg_logprob]))
    assert torch.equal(whole.sequences[:64, :a.sequences.shape[1]], a.sequences)
