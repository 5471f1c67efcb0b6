"""GPU: token rules of the greedy decoder (deny lists + Whisper's timestamp grammar on the chip).

1. wcb_op_lm_head_rules — the LM head with the deny bitmap plus the finalize's rule reduction on caller operands:
   exact logits (identity A, W = k/8), one planted case per branch of the rule per row, next_ids == the argmax of
   the numpy rule (tests/token_rules_np.py) applied in float64 to the logits the op returned, no row excluded; a
   random-W parametrisation where only rows whose rule-5 margin lies inside the f32 logsumexp bound may be skipped.
2. End to end on the micro model (f32, B = 3, 24 new tokens): graph and eager, generate and step-wise, no boost /
   a shared list / per-clip lists, with and without token log-probs — grammar properties on every output and
   parity with the oracle teacher-forced along the device's ids.
3. Rules off: ids as before, graphs not re-captured when alternating; the refused combinations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import token_rules_np as R  # noqa: E402
from oracle import whisper_np as W  # noqa: E402
from whisper_context_biasing_amd import _lib  # noqa: E402
from whisper_context_biasing_amd.config import get_dims, timestamp_ids  # noqa: E402
from whisper_context_biasing_amd.model import WhisperCB  # noqa: E402
from whisper_context_biasing_amd.synth import synth_batch, synth_bias_list  # noqa: E402
from whisper_context_biasing_amd.weights import make_weights  # noqa: E402

DT = {"bf16": (torch.bfloat16, _lib.WCB_BF16), "f16": (torch.float16, _lib.WCB_F16), "f32": (torch.float32, _lib.WCB_F32)}
RULE5_MARGIN = 1e-3


# ------------------------------------------------------------------------------------------------ 1. the kernels
def lm_head_rules(dt, A, Wt, walkers, r, gens):
    lib = _lib.load()
    M, K = A.shape
    V = Wt.shape[0]
    logits = torch.empty(M, V, device="cuda", dtype=torch.float32)
    nxt = torch.full((M,), -7, device="cuda", dtype=torch.int32)
    ld = max(1, max(len(g) for g in gens))
    gen = np.zeros((M, ld), dtype=np.int32)
    for m, g in enumerate(gens):
        gen[m, :len(g)] = g
    lens = np.asarray([len(g) for g in gens], dtype=np.int32)
    rules, keep = r.abi()
    rc = lib.wcb_op_lm_head_rules(DT[dt][1], A.data_ptr(), Wt.data_ptr(), M, V, K, walkers, C.byref(rules), r.eos,
                                  gen.ctypes.data, ld, lens.ctypes.data, logits.data_ptr(), V, nxt.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    del keep
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


def check_planted(dt, K, M, V, ts0, eos, walkers, max_init, offset):
    L, gens = R.planted_case(M, V, ts0, eos, offset)
    r = R.op_rules(V, ts0, eos, True, max_init)
    A, Wt = exact_operands(dt, L, K)
    rc, logits, nxt = lm_head_rules(dt, A, Wt, walkers, r, gens)
    assert rc == 0
    assert np.array_equal(logits, L), (dt, K, M, V, walkers, "logits are exact")
    for m in range(M):
        tok, lse_ts, max_text = R.choose(r, logits[m], gens[m])
        if np.isfinite(lse_ts) and np.isfinite(max_text):   # both outcomes of rule 5 are planted with a clear margin
            assert abs(lse_ts - max_text) >= RULE5_MARGIN, (m, lse_ts, max_text)
        assert nxt[m] == tok, (dt, K, M, V, walkers, max_init, "row", m, "kind", (m + offset) % R.N_KINDS, int(nxt[m]), tok)


@pytest.mark.parametrize("K", [64, 32])          # 64: the column walk; 32: the skinny 64-column epilogue
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_planted_branches(dt, K):
    V, ts0, eos = 2200, 699, 600    # aligned to neither 16 nor 32: a tile and a bitmap word straddle the classes
    for walkers in (128, 256):
        for max_init in (None, 50):
            check_planted(dt, K, 17, V, ts0, eos, walkers, max_init, 0)
    for offset in (0, 3, 6, 9):     # three rows at a time: every branch in a single 16-row block too
        check_planted(dt, K, 3, V, ts0, eos, 256, 50, offset)


def test_planted_branches_whisper_vocabulary():
    check_planted("bf16", 64, 17, 51865, 50364, 50257, 256, 50, 0)


@pytest.mark.parametrize("dt,K", [("bf16", 64), ("f32", 32)])
def test_deny_lists_without_timestamps(dt, K):
    V, ts0, eos = 2200, 699, 600
    r = R.op_rules(V, ts0, eos, False)
    L, _ = R.planted_case(17, V, ts0, eos, 0)
    L[:, ts0:] = np.tile(L[:, :ts0], (1, 3))[:, :V - ts0]   # timestamps are ordinary tokens here
    L[0, 5], L[1, eos], L[2, 3] = 30.0, 30.0, 30.0
    A, Wt = exact_operands(dt, L, K)
    for gens in ([[]] * 17, [[1, 2]] * 17):
        rc, logits, nxt = lm_head_rules(dt, A, Wt, 128, r, gens)
        assert rc == 0 and np.array_equal(logits, L)
        want = [R.choose(r, logits[m], gens[m])[0] for m in range(17)]
        assert np.array_equal(nxt, want), (nxt, want)
    assert want[0] == 5 and want[1] == eos and want[2] != 3    # begin_suppress lifts after the first token; suppress never
    # rows at t == 0 and t > 0 in one launch with begin_suppress ids: refused
    assert lm_head_rules(dt, A, Wt, 128, r, [[]] + [[1]] * 16)[0] == -1
    # every token denied: EOS
    allr = R.Rules(V, eos, list(range(V)), [], False, ts0, ts0 - 1)
    rc, _, nxt = lm_head_rules(dt, A, Wt, 128, allr, [[1]] * 17)
    assert rc == 0 and (nxt == eos).all()


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_random_logits(dt):
    c = R.RANDOM_CASE
    r = R.op_rules(c["V"], c["ts0"], c["eos"], True, 50)
    rows = skipped = 0
    for call in range(c["calls"]):
        A, Wt, gens = R.random_case(call, DT[dt][0])
        rc, logits, nxt = lm_head_rules(dt, A.cuda(), Wt.cuda(), 256, r, gens)
        assert rc == 0
        ref = A.double().numpy() @ Wt.double().numpy().T
        assert np.abs(logits - ref).max() < 1e-4 * (np.abs(ref).max() + 1.0)
        for m in range(c["M"]):
            tok, lse_ts, max_text = R.choose(r, logits[m], gens[m])
            rows += 1
            if np.isfinite(lse_ts) and np.isfinite(max_text) and abs(lse_ts - max_text) <= R.lse_bound(lse_ts):
                skipped += 1
                continue
            assert nxt[m] == tok, (dt, call, m, gens[m], int(nxt[m]), tok, lse_ts, max_text)
    print(f"random logits {dt}: {rows} rows, {skipped} inside the logsumexp bound")
    assert skipped <= 0.01 * rows


# ------------------------------------------------------------------------------------- 2. end to end, micro f32
B, N = 3, 24
_CASE = {}


def case():
    if not _CASE:
        dims = get_dims("micro")
        sd = make_weights(dims, seed=0, recipe="diverse")
        om = W.OracleModel.from_dims(dims, sd)
        mel = W.log_mel(synth_batch(B), dims.n_mel)
        enc = om.encode(mel)
        plain = om.generate(mel, enc=enc, max_length=8, min_new_tokens=8)
        eot = dims.eos_token_id
        shared = synth_bias_list(200, eot=eot) + [list(map(int, plain[0, 2:5])), list(map(int, plain[1, 1:3])) + [7, 8]]
        lists = [synth_bias_list(200, eot=eot, seed=7) + [list(map(int, plain[0, 2:5]))],
                 synth_bias_list(200, eot=eot, seed=8) + [list(map(int, plain[1, 1:3])) + [7, 8]], []]
        ts0, no_ts = timestamp_ids(dims)
        suppress = sorted({int(v) for v in plain[:, :3].ravel()} | {dims.decoder_start_token_id})   # tokens greedy picks
        begin = [220, eot]
        m = WhisperCB.from_state_dict(dims, sd, dtype="f32")
        _CASE.update(dims=dims, om=om, mel=mel, enc=enc, shared=shared, lists=lists, x=torch.from_numpy(mel), m=m,
                     ts0=ts0, suppress=suppress, begin=begin,
                     rules=R.Rules(dims.vocab, eot, suppress, begin, True, ts0, no_ts, 50))
    return _CASE


def bias_kw(c, bias):
    if bias == "none":
        return {}, [[]] * B, 0.0
    if bias == "shared":
        return dict(bias_list=c["shared"], bias_boost=2.0), [c["shared"]] * B, 2.0
    return dict(bias_lists=c["lists"], bias_boost=2.0), c["lists"], 2.0


RULE_KW = dict(return_timestamps=True, max_initial_timestamp=1.0)


def check_rows(c, ids, lists, lam, logprobs=None):
    """grammar properties of every row; parity with the oracle teacher-forced along the row"""
    dims, r = c["dims"], c["rules"]
    steps = skipped = 0
    for b in range(B):
        R.grammar_ok(ids[b], c["ts0"], dims.eos_token_id, dims.pad_token_id, 50, c["suppress"], c["begin"])
        st = R.ruled_steps(c["om"], c["enc"][b:b + 1], r, lists[b], lam, ids=ids[b], n=len(ids[b]))
        for t, (tok, got, best, margin, row) in enumerate(st):
            steps += 1
            if logprobs is not None:   # the raw log-softmax of the chosen token: the rules never enter it
                want = float(row[tok]) - R.logsumexp(row)
                np.testing.assert_allclose(logprobs[b, t], want, atol=1e-3, rtol=1e-4)
            if margin < RULE5_MARGIN:
                skipped += 1
                continue
            assert np.isfinite(got) and got >= best - 1e-3, (b, t, tok, got, best, margin)
        if logprobs is not None:
            assert (logprobs[b, len(st):] == 0).all()
    assert skipped <= 0.05 * steps, (skipped, steps)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("bias", ["none", "shared", "per_clip"])
def test_generate_with_timestamps(bias, use_graph):
    c = case()
    kw, lists, lam = bias_kw(c, bias)
    kw.update(RULE_KW, suppress_tokens=c["suppress"], begin_suppress_tokens=c["begin"], max_length=N, use_graph=use_graph)
    out = c["m"].generate(c["x"], **kw)
    ids = out.sequences[:, 1:].cpu().numpy()
    assert ids.shape[1] <= N
    check_rows(c, ids, lists, lam)
    assert len(out.segments) == B
    for b in range(B):
        for (s0, s1, toks) in out.segments[b]:
            assert toks and all(t < c["ts0"] for t in toks) and (s1 is None or s0 <= s1)
    scored = c["m"].generate(c["x"], output_logprobs=True, **kw)
    assert np.array_equal(scored.sequences[:, 1:].cpu().numpy(), ids)
    check_rows(c, ids, lists, lam, scored.token_logprobs.cpu().numpy())


@pytest.mark.parametrize("bias", ["none", "shared", "per_clip"])
def test_stepwise_with_timestamps(bias):
    c = case()
    m = c["m"]
    kw, lists, lam = bias_kw(c, bias)
    ref = m.generate(c["x"], max_length=N, suppress_tokens=c["suppress"], begin_suppress_tokens=c["begin"], **RULE_KW,
                     **kw).sequences[:, 1:].cpu().numpy()
    enc = m.encode(c["x"])
    for logprobs in (False, True):
        dec = m.decode_begin(enc, logprobs=logprobs, suppress_tokens=c["suppress"], begin_suppress_tokens=c["begin"],
                             **RULE_KW, **kw)
        ids = torch.stack([dec.step()[0] for _ in range(ref.shape[1])], 1).cpu().numpy()
        lp = dec.logprobs().cpu().numpy() if logprobs else None
        assert _lib.load().wcb_set_token_rules(m._h, None) == -2   # fixed while a step-wise decode is open
        dec.close()
        assert np.array_equal(ids, ref), (ids, ref)
        check_rows(c, ids, lists, lam, lp)


# --------------------------------------------------------------------------------- 3. rules off; refused calls
def test_rules_off_is_the_old_decode_and_graphs_are_kept():
    c = case()
    m = c["m"]
    kw = dict(max_length=12, min_new_tokens=12, bias_list=c["shared"], bias_boost=2.0)
    before = m.generate(c["x"], **kw).cpu().numpy()
    ref = c["om"].generate(c["mel"], enc=c["enc"], max_length=12, min_new_tokens=12, bias=c["shared"], bias_boost=2.0)
    assert np.array_equal(before, ref)
    deny = [int(before[0, 0])]
    ruled = m.generate(c["x"], suppress_tokens=deny, **kw).cpu().numpy()
    assert deny[0] not in ruled and not np.array_equal(ruled, before)
    for on in (True, False):   # both kinds captured in both decode contexts (calls alternate between the two)
        m.generate(c["x"], suppress_tokens=deny if on else None, **kw)
    n0 = m.debug_counter("graph_captures")
    for on in (False, True, True, False, True, False, False, True):   # each kind replays its own graphs
        got = m.generate(c["x"], suppress_tokens=deny if on else None, **kw).cpu().numpy()
        assert np.array_equal(got, ruled if on else before)
    assert m.debug_counter("graph_captures") == n0
    # deny lists work with sampling: the denied token is never drawn
    smp = m.generate(c["x"], suppress_tokens=deny, temperature=1.0, seed=3, **kw).cpu().numpy()
    assert deny[0] not in smp
    assert np.array_equal(m.generate(c["x"], **kw).cpu().numpy(), before)


def test_refused_combinations():
    c = case()
    m, x = c["m"], c["x"]
    for kw in (dict(return_timestamps=True, num_beams=2), dict(suppress_tokens=[5], num_beams=2),
               dict(return_timestamps=True, temperature=0.5), dict(return_timestamps=True, temperature=(0.0, 0.5)),
               dict(return_timestamps=True, do_sample=True), dict(max_initial_timestamp=1.0),
               dict(suppress_tokens=[c["dims"].vocab]), dict(return_timestamps=True, suppress_tokens=[c["ts0"] + 1])):
        with pytest.raises(ValueError):
            m.generate(x, max_length=4, **kw)
    with pytest.raises(ValueError):
        m.decode_begin(m.encode(x), return_timestamps=True, num_beams=2)
    with pytest.raises(ValueError):
        m.decode_begin(m.encode(x), return_timestamps=True, temperature=0.7)
    # the ABI's own codes
    lib = _lib.load()
    r, keep = c["rules"].abi()
    assert lib.wcb_set_token_rules(m._h, C.byref(r)) == 0
    m._rules_key = "set by the test"
    out = torch.empty(B, 4, dtype=torch.int32, device="cuda")
    xg = x.cuda()
    steps = C.c_int32(0)
    cfg = _lib.WcbGenCfg(4, 0, 2, 0.0, 1, 0)
    assert lib.wcb_generate(m._h, xg.data_ptr(), B, C.byref(cfg), None, None, 1, out.data_ptr(), C.byref(steps), None) == -4
    cfg = _lib.WcbGenCfg(4, 0, 1, 0.0, 1, 0)
    seeds = np.arange(B, dtype=np.uint64)
    smp = _lib.WcbSampleCfg(1.0, seeds.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert lib.wcb_generate_sampled(m._h, xg.data_ptr(), B, C.byref(cfg), C.byref(smp), None, None, None, 1,
                                    out.data_ptr(), None, C.byref(steps), None) == -4
    bad, keep2 = _lib.token_rules([c["dims"].vocab], [], False)
    assert lib.wcb_set_token_rules(m._h, C.byref(bad)) == -1
    bad, keep2 = _lib.token_rules([], [], True, c["dims"].eos_token_id, 5, -1)
    assert lib.wcb_set_token_rules(m._h, C.byref(bad)) == -1
    assert lib.wcb_set_token_rules(m._h, None) == 0
    m._rules_key = None
    assert m.generate(x, max_length=4).shape[0] == B
